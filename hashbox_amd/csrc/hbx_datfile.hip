// hbx_datfile.hip — K14: find and frame the entries of a storage data file
// whose image lies in device memory (the server's verify and recover walks).
//
// Reference: a data file (*.dat, pkg/storagedb/data.go, storagedb.go:40-53) is
// a 16-byte header followed by entries ("hblk" + HashboxBlock.Serialize,
// data.go:33-37, block.go:56-94) and free-space markers ("Cgap" + BE64 skip,
// data.go:142-164).  RecoverData (integrity.go:74-143) walks it one entry at a
// time and, after damage, resynchronises on the next "hblk" anywhere in the
// bytes (forwardToDataMarker).  So every "hblk" in the file may become the
// walk's next block offset: K14 finds them all and frames each one, the
// existing kernels (K8 / K8s, K6) inflate and verify every framed entry in
// place, and the walk itself (hbx_datfile.h, host) is left with list lookups.
//
//   hbx_k14_scan   every byte position p in [16, size - 4] is compared with
//                  both 4-byte patterns.  A lane takes 16 positions per
//                  iteration: one 16-byte load at a 16-byte boundary plus the
//                  dword behind it (positions 13..15 need 3 of its bytes; the
//                  image has readable bytes behind `size`, but no byte at or
//                  past `size` decides anything: a position counts only if
//                  p + 4 <= size).  256-thread workgroups in a grid-stride
//                  loop whose trip count is the same for every lane of a
//                  wave, so each byte is read from HBM once and every lane
//                  reaches the ballots.  Hits go to two lists of 8-byte
//                  positions (markers, gaps): a wave whose ballot shows a hit
//                  sums its lanes' hit counts by shuffles and lane 0 issues
//                  ONE agent-scope add per list; each lane then stores its
//                  positions behind the wave's base.  The add counts past the
//                  list's capacity (the stores do not go there), so the host
//                  learns the needed capacity.  The order in a list depends
//                  on which wave's add came first: the host sorts them.
//   hbx_k14_parse  one thread per position: the structural rules of an entry
//                  (hbx_datfile.h restates them for the host), or the skip of
//                  a gap marker, into one 64-byte hbx_dat_record (four uint4
//                  stores).  n_links and data_len are untrusted 32-bit
//                  values: all arithmetic on them is 64-bit and every byte is
//                  read only after its offset was compared with `size`.
//
// No spin, no LDS, no inline assembly; every loop is bounded by the input
// (the scan by size / 16 granules, the hit stores by 16 positions per lane);
// plain loads only, of an image nothing writes during the launch; the lists'
// counters are touched with agent-scope atomics only.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/hbxgpu.h"

namespace hbxf {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kMarkerLE = 0x6B6C6268u;  // "hblk" as a little-endian dword
constexpr uint32_t kGapLE = 0x70616743u;     // "Cgap"

struct ScanArgs {
  const uint8_t* image;  // 16-byte aligned, >= HBX_DAT_IMAGE_SLACK readable bytes behind size
  uint64_t size;
  uint64_t* markers;     // cap positions each
  uint64_t* gaps;
  unsigned long long* counts;  // [0] markers, [1] gaps: every hit, also those past cap
  uint64_t cap;
};

struct ParseArgs {
  const uint8_t* image;
  uint64_t size;
  const uint64_t* pos;  // n positions; the first n_entries are entry positions, the rest gap markers
  uint4* rec;           // n hbx_dat_record, four uint4 each
  uint64_t n, n_entries;
  uint64_t in_bound;    // hbx_restore_in_bound(max_block)
};

// The dword at byte j (0..3) of the pair (lo, hi).
__device__ __forceinline__ uint32_t window(uint32_t lo, uint32_t hi, uint32_t j) {
  return (uint32_t)((((uint64_t)hi << 32) | lo) >> (8u * j));
}

// A wave's exclusive prefix sum of n (every lane calls it); *total = the wave's sum.
__device__ __forceinline__ uint32_t wave_excl(uint32_t n, uint32_t lane, uint32_t* total) {
  uint32_t incl = n;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const uint32_t up = (uint32_t)__shfl_up((int)incl, d, 64);
    if (lane >= (uint32_t)d) incl += up;
  }
  *total = (uint32_t)__shfl((int)incl, 63, 64);
  return incl - n;
}

// Append the positions g16 + bit for the bits of `mask` to a list; wave-uniform call.
__device__ __forceinline__ void append(uint32_t mask, uint64_t g16, uint32_t lane, uint64_t* list,
                                       unsigned long long* count, uint64_t cap) {
  uint32_t total = 0;
  const uint32_t before = wave_excl((uint32_t)__popc(mask), lane, &total);
  unsigned long long base = 0;
  if (lane == 0) base = __hip_atomic_fetch_add(count, (unsigned long long)total, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  base = (unsigned long long)__shfl((long long)base, 0, 64);
  uint64_t at = base + before;
  for (uint32_t m = mask; m; m &= m - 1u, at++)  // at most 16 bits
    if (at < cap) list[at] = g16 + (uint32_t)__builtin_ctz(m);
}

__device__ __forceinline__ uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}

}  // namespace hbxf

static_assert(sizeof(hbx_dat_record) == 64, "hbx_dat_record is four uint4");

extern "C" __global__ __launch_bounds__(256) void hbx_k14_scan(hbxf::ScanArgs a) {
  using namespace hbxf;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t granules = (a.size + 15u) >> 4;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  // (base is the wave's first granule: the loop condition is wave-uniform)
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u); base < granules; base += stride) {
    const uint64_t g = base + lane;
    uint32_t mm = 0, gm = 0;  // bit j: a marker / gap pattern starts at position 16 g + j
    if (g < granules) {
      const uint4 v = *reinterpret_cast<const uint4*>(a.image + 16u * g);
      const uint32_t next = *reinterpret_cast<const uint32_t*>(a.image + 16u * g + 16u);
      const uint32_t w[5] = {v.x, v.y, v.z, v.w, next};
#pragma unroll
      for (uint32_t j = 0; j < 16u; j++) {
        const uint32_t x = window(w[j >> 2], w[(j >> 2) + 1u], j & 3u);
        mm |= (x == kMarkerLE ? 1u : 0u) << j;
        gm |= (x == kGapLE ? 1u : 0u) << j;
      }
      // positions before the header's end or whose four bytes do not all lie inside the file
      // (the header is granule 0; position p0 + j counts while p0 + j + 4 <= size)
      const uint64_t p0 = 16u * g;
      uint32_t keep = 0u;
      if (p0 >= HBX_DAT_HEADER && a.size >= p0 + 4u)
        keep = (1u << (uint32_t)(a.size - p0 - 3u < 16u ? a.size - p0 - 3u : 16u)) - 1u;
      mm &= keep;
      gm &= keep;
    }
    if (__ballot(mm != 0u)) append(mm, 16u * g, lane, a.markers, a.counts, a.cap);
    if (__ballot(gm != 0u)) append(gm, 16u * g, lane, a.gaps, a.counts + 1, a.cap);
  }
}

extern "C" __global__ __launch_bounds__(256) void hbx_k14_parse(hbxf::ParseArgs a) {
  using namespace hbxf;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= a.n) return;
  const uint64_t off = a.pos[i], size = a.size;
  const uint8_t* p = a.image + off;
  const uint64_t avail = off < size ? size - off : 0;  // bytes of the file from off on
  uint32_t flags = 0, status = HBX_DAT_ST_INVALID, n_links = 0, data_len = 0, type = 0;
  uint64_t esize = 0, data_off = 0, links_off = 0;
  uint4 id = make_uint4(0u, 0u, 0u, 0u);
  if (i >= a.n_entries) {  // a gap marker: "Cgap" | BE64 skip
    flags = HBX_DAT_F_GAP;
    if (avail >= 12u && be32(p) == HBX_DAT_GAP) {
      flags |= HBX_DAT_F_MARKER;
      esize = ((uint64_t)be32(p + 4) << 32) | be32(p + 8);  // the skip, two's complement
      status = 0u;
    }
  } else {
    if (avail >= 4u && be32(p) == HBX_DAT_MARKER) flags |= HBX_DAT_F_MARKER;
    if ((flags & HBX_DAT_F_MARKER) && avail >= 24u) {
      const uint32_t nl = be32(p + 20);
      const uint64_t head = 24ull + 16ull * nl + 5ull;  // up to and including data_len
      if (avail >= head) {
        const uint32_t t = p[head - 5u];
        const uint32_t dl = be32(p + (head - 4u));
        if (avail - head >= dl && (t == HBX_BLOCK_RAW || t == HBX_BLOCK_ZLIB) && dl <= a.in_bound) {
          status = 0u;
          n_links = nl;
          data_len = dl;
          type = t;
          esize = head + dl;
          links_off = off + 24u;
          data_off = off + head;
          __builtin_memcpy(&id, p + 4, 16);
        }
      }
    }
  }
  uint4* r = a.rec + 4u * i;
  r[0] = make_uint4((uint32_t)off, (uint32_t)(off >> 32), (uint32_t)esize, (uint32_t)(esize >> 32));
  r[1] = make_uint4((uint32_t)data_off, (uint32_t)(data_off >> 32), (uint32_t)links_off, (uint32_t)(links_off >> 32));
  r[2] = make_uint4(data_len, n_links, status, type | (flags << 8));
  r[3] = id;
}

namespace hbxf {

// K14's default grid: every granule once, at most 2,048 workgroups (8 per CU).
inline uint32_t scan_grid(uint64_t size, uint32_t knob) {
  const uint64_t wgs = (((size + 15u) >> 4) + kThreads - 1) / kThreads;
  const uint64_t most = knob ? knob : 2048u;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(wgs, most));
}

}  // namespace hbxf
