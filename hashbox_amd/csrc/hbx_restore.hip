// hbx_restore.hip — K10: put a file's verified blocks together, or compare
// them with a local copy (the read side's last step).
//
// Reference: restoreFileData appends each verified block to the file
// (hashback/restore.go:45-66); diffFileData compares each verified block with
// the local file at the running offset and reports the first differing
// 16-byte line (restore.go:249-277).
//
// After K8 the inflated blocks lie in aligned slots, one per block; raw blocks
// (BlockDataTypeRaw) lie where the input was staged, at any byte address.
// Block i's len[i] bytes belong at byte off[i] of the file image, off being
// the exclusive prefix sum of the lengths.  The host cuts every block into
// PIECES of at most kPiece bytes (one 8 MiB block is 128 workgroups' job, not
// one's) and both kernels take one piece per workgroup:
//   hbx_k10_gather  copies the piece to image + dst.  The stores are 16-byte
//                   vectors aligned to the DESTINATION; the bytes before the
//                   first and after the last aligned granule go one per lane.
//                   The source is read at whatever alignment that leaves it
//                   (the hardware splits an unaligned vector load).  Nothing
//                   outside [dst, dst + len) is written and nothing outside
//                   [src, src + len) is read.  The image may be pinned host
//                   memory: the kernel ends with a system-scope fence, as
//                   hbx_result_push does.
//   hbx_k10_diff    compares the piece with local + dst and writes nothing but
//                   one 64-bit word: the smallest file offset at which a byte
//                   differs (atomicMin; the host presets UINT64_MAX).  A wave
//                   reduces its lanes first, a workgroup its waves, and only a
//                   workgroup that saw a difference issues the atomic.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace hbxr {

constexpr uint32_t kPiece = 65536;  // bytes per piece (per workgroup)
constexpr uint32_t kThreads = 256;
constexpr uint64_t kNoDiff = ~0ull;

struct Piece {
  uint64_t src;  // device address of the piece's first byte
  uint64_t dst;  // its byte offset in the image (gather) / in the local copy and the file (diff)
  uint32_t len;  // 1..kPiece
  uint32_t pad;
};
static_assert(sizeof(Piece) == 24, "piece layout shared with the host");

// 16 bytes at any byte address.
__device__ __forceinline__ uint4 load16_any(const uint8_t* p) {
  uint4 v;
  __builtin_memcpy(&v, p, 16);
  return v;
}

// Index of the first byte in which two 16-byte granules differ (they do).
__device__ __forceinline__ uint32_t first_diff16(uint4 a, uint4 b) {
  const uint32_t x0 = a.x ^ b.x, x1 = a.y ^ b.y, x2 = a.z ^ b.z, x3 = a.w ^ b.w;
  if (x0) return (uint32_t)__builtin_ctz(x0) >> 3;
  if (x1) return 4u + ((uint32_t)__builtin_ctz(x1) >> 3);
  if (x2) return 8u + ((uint32_t)__builtin_ctz(x2) >> 3);
  return 12u + ((uint32_t)__builtin_ctz(x3) >> 3);
}

}  // namespace hbxr

extern "C" __global__ __launch_bounds__(256) void hbx_k10_gather(const hbxr::Piece* __restrict__ pieces,
                                                                 uint32_t n, uint8_t* __restrict__ image) {
  using namespace hbxr;
  const uint32_t i = blockIdx.x;
  if (i < n) {
    const Piece p = pieces[i];
    const uint8_t* src = reinterpret_cast<const uint8_t*>(p.src);
    uint8_t* dst = image + p.dst;
    const uint32_t len = p.len;
    const uint32_t head = min(len, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(dst) & 15u)) & 15u);
    const uint32_t nvec = (len - head) >> 4;
    const uint32_t tail0 = head + (nvec << 4);  // first byte after the last whole granule
    const uint32_t t = threadIdx.x;
    if (t < head) dst[t] = src[t];
    for (uint32_t v = t; v < nvec; v += kThreads)
      *reinterpret_cast<uint4*>(dst + head + 16u * v) = load16_any(src + head + 16u * v);
    if (t < len - tail0) dst[tail0 + t] = src[tail0 + t];
  }
  __threadfence_system();
}

extern "C" __global__ __launch_bounds__(256) void hbx_k10_diff(const hbxr::Piece* __restrict__ pieces, uint32_t n,
                                                               const uint8_t* __restrict__ local,
                                                               unsigned long long* __restrict__ first) {
  using namespace hbxr;
  __shared__ unsigned long long wmin[kThreads / 64];
  const uint32_t i = blockIdx.x;
  if (i >= n) return;  // uniform per workgroup
  const Piece p = pieces[i];
  const uint8_t* src = reinterpret_cast<const uint8_t*>(p.src);
  const uint8_t* loc = local + p.dst;
  const uint32_t len = p.len;
  const uint32_t head = min(len, (16u - (uint32_t)(reinterpret_cast<uintptr_t>(loc) & 15u)) & 15u);
  const uint32_t nvec = (len - head) >> 4;
  const uint32_t tail0 = head + (nvec << 4);
  const uint32_t t = threadIdx.x;
  uint32_t best = 0xFFFFFFFFu;  // offset in the piece of this lane's first differing byte
  if (t < head && src[t] != loc[t]) best = t;
  for (uint32_t v = t; v < nvec; v += kThreads) {  // ascending per lane: the first hit is the lane's smallest
    const uint32_t at = head + 16u * v;
    const uint4 a = load16_any(src + at);
    const uint4 b = *reinterpret_cast<const uint4*>(loc + at);
    if (a.x != b.x || a.y != b.y || a.z != b.z || a.w != b.w) {
      best = min(best, at + first_diff16(a, b));
      break;
    }
  }
  if (t < len - tail0 && src[tail0 + t] != loc[tail0 + t]) best = min(best, tail0 + t);
  // the wave's smallest, then the workgroup's
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, m, 64));
  if ((t & 63u) == 0u) wmin[t >> 6] = best == 0xFFFFFFFFu ? kNoDiff : p.dst + best;
  __syncthreads();
  if (t == 0) {
    unsigned long long m = wmin[0];
#pragma unroll
    for (uint32_t w = 1; w < kThreads / 64; w++) m = wmin[w] < m ? wmin[w] : m;
    if (m != kNoDiff) atomicMin(first, m);
  }
}
