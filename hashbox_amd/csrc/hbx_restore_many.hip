// hbx_restore_many.hip — K11: put the verified blocks of MANY files together in
// one packed image, or compare them with the files' local copies (the read
// side's last step for a tree of small files).
//
// Reference: restoreDir walks a directory's entries and restores each one
// (hashback/restore.go:137-162), restoreFileData appends each verified block
// (restore.go:45-66); diffDir / diffEntry / diffFileData do the same walk and
// compare instead (restore.go:249-277, 279-414).
//
// K10 (hbx_restore.hip) serves one file per launch: a 256-thread workgroup per
// piece of up to 64 KiB and one 64-bit word for the whole launch.  A window of
// a tree holds thousands of blocks of a few hundred bytes, of many files.  So
// here a piece belongs to one WAVE (four pieces per 256-thread workgroup, no
// LDS, nothing shared between the waves), is at most kPieceMany bytes, and
// carries its file's index:
//   hbx_k11_gather  copies the piece to image + dst, with K10's scheme: 16-byte
//                   stores aligned to the DESTINATION, the bytes before the
//                   first and after the last aligned granule one per lane, the
//                   source read at whatever alignment that leaves it.  Nothing
//                   outside [dst, dst + len) is written and nothing outside
//                   [src, src + len) is read.  The image may be pinned host
//                   memory: the kernel ends with a system-scope fence.
//   hbx_k11_diff    compares the piece with local + dst and writes nothing but
//                   first[file]: the smallest offset INSIDE THE FILE at which a
//                   byte differs (atomicMin; the host presets every word to
//                   UINT64_MAX).  A wave reduces its lanes by __shfl_xor and
//                   lane 0 issues the atomic only if the wave saw a difference.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "hbx_restore.hip"

namespace hbxm {

// Bytes per piece (per wave): 16 granules per lane.  -DHBX_PIECE_MANY builds a
// variant for tools/bench_restore_many.py's sweep (DESIGN §8 has what was measured).
#ifndef HBX_PIECE_MANY
#define HBX_PIECE_MANY 16384
#endif
constexpr uint32_t kPieceMany = HBX_PIECE_MANY;
static_assert(kPieceMany >= 1024 && kPieceMany % 16 == 0, "a piece is whole granules");
constexpr uint32_t kThreads = 256;
constexpr uint32_t kWaves = kThreads / 64;  // pieces per workgroup

struct Piece {
  uint64_t src;   // device address of the piece's first byte
  uint64_t dst;   // its byte offset in the window's packed image (gather) / packed local image (diff)
  uint64_t foff;  // its byte offset inside its file
  uint32_t len;   // 1..kPieceMany
  uint32_t file;  // index of its file in the window's `first` words (diff)
};
static_assert(sizeof(Piece) == 32, "piece layout shared with the host");

}  // namespace hbxm

extern "C" __global__ __launch_bounds__(256) void hbx_k11_gather(const hbxm::Piece* __restrict__ pieces,
                                                                 uint32_t n, uint8_t* __restrict__ image) {
  using namespace hbxm;
  const uint32_t i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i < n) {  // uniform per wave
    const Piece p = pieces[i];
    const uint8_t* src = reinterpret_cast<const uint8_t*>(p.src);
    uint8_t* dst = image + p.dst;
    const uint32_t len = p.len;
    const uint32_t head = min(len, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    const uint32_t nvec = (len - head) >> 4;
    const uint32_t tail0 = head + (nvec << 4);  // first byte after the last whole granule
    const uint32_t t = threadIdx.x & 63u;
    if (t < head) dst[t] = src[t];
    for (uint32_t v = t; v < nvec; v += 64u)
      *reinterpret_cast<uint4*>(dst + head + 16u * v) = hbxr::load16_any(src + head + 16u * v);
    if (t < len - tail0) dst[tail0 + t] = src[tail0 + t];
  }
  __threadfence_system();
}

extern "C" __global__ __launch_bounds__(256) void hbx_k11_diff(const hbxm::Piece* __restrict__ pieces, uint32_t n,
                                                               const uint8_t* __restrict__ local,
                                                               unsigned long long* __restrict__ first) {
  using namespace hbxm;
  const uint32_t i = blockIdx.x * kWaves + (threadIdx.x >> 6);
  if (i >= n) return;  // uniform per wave
  const Piece p = pieces[i];
  const uint8_t* src = reinterpret_cast<const uint8_t*>(p.src);
  const uint8_t* loc = local + p.dst;
  const uint32_t len = p.len;
  const uint32_t head = min(len, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(loc) & 15u)) & 15u);
  const uint32_t nvec = (len - head) >> 4;
  const uint32_t tail0 = head + (nvec << 4);
  const uint32_t t = threadIdx.x & 63u;
  uint32_t best = 0xFFFFFFFFu;  // offset in the piece of this lane's first differing byte
  if (t < head && src[t] != loc[t]) best = t;
  for (uint32_t v = t; v < nvec; v += 64u) {  // ascending per lane: the first hit is the lane's smallest
    const uint32_t at = head + 16u * v;
    const uint4 a = hbxr::load16_any(src + at);
    const uint4 b = *reinterpret_cast<const uint4*>(loc + at);
    if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) {
      best = min(best, at + hbxr::first_diff16(a, b));
      break;
    }
  }
  if (t < len - tail0 && src[tail0 + t] != loc[tail0 + t]) best = min(best, tail0 + t);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, m, 64));
  if (t == 0 && best != 0xFFFFFFFFu) atomicMin(&first[p.file], (unsigned long long)(p.foff + best));
}
