// hbx_compact.hip — K16: compact a storage data file whose image lies in device
// memory: the kept entries that cannot stay where they are packed back to back
// into one stream, and the meta and index records the move implies.
//
// Reference: CompactFile (pkg/storagedb/gc.go:208-318) reads a data file one
// entry at a time on one goroutine, appends every kept entry behind the
// high-water mark to the store's free file (Serialize, gc.go:274) and collects
// a relocation per entry; writeBlockFile (data.go:85-102) shows the
// StorageMetaEntry (meta.go:21-39) and StorageIXEntry (index.go:24-38) a block
// at a location needs.  include/hbxgpu.h states the semantics; hbx_compact.h
// is the same plan on the host.
//
//   hbx_k16_break  one thread per entry of the uploaded table: the first
//                  index at which the kept prefix ends (a dropped entry, or
//                  one that does not start where the entry before ends; entry
//                  0: at 16).  By induction that is the first i with off[i] !=
//                  16 + the sizes before it.  A wave that saw a failure issues
//                  ONE agent-scope min of its lowest failing index.  Not
//                  launched without HBX_CMP_F_KEEP_PREFIX (the break is 0).
//   hbx_k16_plan   one thread per entry: the class, and the three values the
//                  scans run over: the moved size, the meta size, and the
//                  pair (1 if kept) << 32 | (1 if moved).
//   hbx_k15_scan_sums / _scan_top / _scan_add   K15's three-launch exclusive
//                  64-bit scan, once per value (n < 2^31: the pair cannot carry).
//   hbx_k16_place  one thread per entry: new_off and meta_off from the scans
//                  (in place: a thread reads and writes its own words), the
//                  movers compacted into msrc[k] (offset in the image) and
//                  mstart[k] (offset in the stream), the first entry past the
//                  16 GiB limit by the same one-min-per-wave, and the totals
//                  by the last entry's thread (mstart[n_moved] = moved_bytes).
//   hbx_k16_pack   THE HOT PATH, tiled by destination.  A 256-thread workgroup
//                  owns T bytes of the moved stream (64 KiB: sixteen 16-byte
//                  granules per lane, consecutive lanes consecutive granules).
//                  It finds the movers of the tile's first and last byte by a
//                  binary search over mstart in which every lane reads the same
//                  words; a lane narrows that range to its granule's first
//                  byte, starting from the mover of its granule before.  A
//                  granule inside one entry is one 16-byte load at any source
//                  alignment and one aligned 16-byte store.  A granule across
//                  a boundary takes the LAST 16 bytes of the entry it starts
//                  in and the FIRST 16 of the next (an entry has at least 29
//                  bytes, so both loads lie inside their entries and a granule
//                  touches two entries at most) and joins them by two shifts.
//                  Only the stream's last partial granule goes out byte by
//                  byte.  Every byte of [0, moved_bytes) is written once,
//                  nothing outside it, and nothing outside a mover's
//                  [off, off + size) is read.
//   hbx_k16_meta   one kept entry per thread: the 34 header bytes of its meta
//                  record and its 24-byte index record built in registers and
//                  stored where they lie; the links copied by K15's degree
//                  classes: a lane alone up to kLaneMax links, the row's wave
//                  up to kWaveMax (64 links per step), the workgroup beyond
//                  (256 per step).
//
// Visibility, as K14 / K15: plain loads only of bytes nothing writes in that
// launch; the two minima and nothing else are touched with agent-scope
// atomics; the kernel boundary publishes.  No spin, no grid-wide barrier, no
// inline assembly; every loop is bounded by the table, the tile or a list.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/hbxgpu.h"
#include "hbx_graph.hip"
#include "hbx_restore.hip"

namespace hbxk {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTile = 65536;  // bytes of the moved stream per workgroup
constexpr uint64_t kNever = ~0ull;
enum { kTotMoved, kTotMeta, kTotCounts, kTotBreak, kTotPast, kTotWords };

static_assert(sizeof(hbx_dat_entry) == 64, "the uploaded table");
static_assert(HBX_DAT_ENTRY_MIN >= 16, "a 16-byte granule touches at most two entries");
static_assert(sizeof(hbx_dat_compact_args) == 32 && sizeof(hbx_dat_compact_summary) == 88, "C-ABI");

struct PlanArgs {
  const hbx_dat_entry* ent;
  const uint8_t* keep;
  uint8_t* klass;
  unsigned long long* msz;   // plan: the moved size; after the scan: its exclusive sum; after place: new_off
  unsigned long long* tsz;   // the same for the meta size / meta_off
  unsigned long long* cnt;   // kept << 32 | moved, then the exclusive sums: the ranks
  unsigned long long* msrc;  // place: n + 1 words
  unsigned long long* mstart;
  unsigned long long* tot;   // kTotWords
  hbx_dat_compact_args a;
  uint32_t n;
};

struct PackArgs {
  const uint8_t* image;
  const unsigned long long* msrc;
  const unsigned long long* mstart;  // n_moved + 1 words, the last one moved_bytes
  uint8_t* out;                      // 16-byte aligned
  uint64_t moved_bytes;
  uint32_t n_moved, tile;
};

struct MetaArgs {
  const uint8_t* image;
  const hbx_dat_entry* ent;
  const uint8_t* klass;
  const unsigned long long* new_off;
  const unsigned long long* meta_off;
  const unsigned long long* cnt;
  uint8_t* meta;  // nullptr: not wanted
  uint8_t* ix;    // nullptr: not wanted
  hbx_dat_compact_args a;
  uint32_t n;
};

// The wave's lowest index among the lanes with `hit` goes into *word by one agent-scope min.
__device__ __forceinline__ void wave_min(bool hit, uint64_t i, unsigned long long* word) {
  const unsigned long long w = __ballot(hit);
  if (!w) return;
  const int first = __builtin_ctzll(w);  // indices ascend with the lane
  if ((int)(threadIdx.x & 63u) == first)
    (void)__hip_atomic_fetch_min(word, (unsigned long long)i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The largest k in [lo, hi] with mstart[k] <= at (mstart[lo] <= at).
__device__ __forceinline__ uint32_t mover_of(const unsigned long long* mstart, uint32_t lo, uint32_t hi, uint64_t at) {
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1u) / 2u;
    if (mstart[mid] <= at)
      lo = mid;
    else
      hi = mid - 1u;
  }
  return lo;
}

// sixByteLocation.Set (storagedb.go:90-101) into p[0..6).
__device__ __forceinline__ void put_location(uint8_t* p, uint32_t file, uint64_t off) {
  const uint64_t l = ((uint64_t)file << 34) | (off & HBX_DAT_OFFSET_LIMIT);
#pragma unroll
  for (int b = 0; b < 6; b++) p[b] = (uint8_t)(l >> (40 - 8 * b));
}

__device__ __forceinline__ void put_be32(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 24);
  p[1] = (uint8_t)(v >> 16);
  p[2] = (uint8_t)(v >> 8);
  p[3] = (uint8_t)v;
}

// Link k of a list at src to dst, both at any alignment.
__device__ __forceinline__ void copy_link(const uint8_t* src, uint8_t* dst, uint64_t k) {
  const uint4 v = hbxr::load16_any(src + 16u * k);
  __builtin_memcpy(dst + 16u * k, &v, 16);
}

}  // namespace hbxk

extern "C" __global__ __launch_bounds__(256) void hbx_k16_break(hbxk::PlanArgs p) {
  using namespace hbxk;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool fails = false;
  if (i < p.n) {
    const uint64_t want = i ? p.ent[i - 1].off + p.ent[i - 1].size : (uint64_t)HBX_DAT_HEADER;
    fails = p.keep[i] == 0 || p.ent[i].off != want;
  }
  wave_min(fails, i, p.tot + kTotBreak);
}

extern "C" __global__ __launch_bounds__(256) void hbx_k16_plan(hbxk::PlanArgs p) {
  using namespace hbxk;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= p.n) return;
  const unsigned long long brk = p.tot[kTotBreak];  // (the launch before wrote it)
  const bool kept = p.keep[i] != 0;
  const uint32_t k = !kept ? HBX_CMP_DROP : i < brk ? HBX_CMP_STAY : HBX_CMP_MOVE;
  p.klass[i] = (uint8_t)k;
  p.msz[i] = k == HBX_CMP_MOVE ? p.ent[i].size : 0ull;
  p.tsz[i] = kept ? HBX_META_HEAD + 16ull * p.ent[i].n_links : 0ull;
  p.cnt[i] = ((unsigned long long)(kept ? 1u : 0u) << 32) | (k == HBX_CMP_MOVE ? 1u : 0u);
}

extern "C" __global__ __launch_bounds__(256) void hbx_k16_place(hbxk::PlanArgs p) {
  using namespace hbxk;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool past = false;
  if (i < p.n) {
    const uint32_t k = p.klass[i];
    const unsigned long long before = p.msz[i], mbefore = p.tsz[i], ranks = p.cnt[i];
    const uint64_t size = p.ent[i].size, off = p.ent[i].off;
    unsigned long long no = kNever, mo = kNever;
    if (k != HBX_CMP_DROP) {
      no = k == HBX_CMP_STAY ? off : p.a.dst_base + before;
      mo = p.a.meta_base + mbefore;
      past = no > HBX_DAT_OFFSET_LIMIT || mo > HBX_DAT_OFFSET_LIMIT;
    }
    if (k == HBX_CMP_MOVE) {
      const uint32_t at = (uint32_t)ranks;  // movers before this one
      p.msrc[at] = off;
      p.mstart[at] = before;
    }
    if (i == p.n - 1u) {  // the totals: the exclusive sums plus the last entry's own values
      const unsigned long long moved = before + (k == HBX_CMP_MOVE ? size : 0ull);
      const unsigned long long all =
          ranks + (((unsigned long long)(k != HBX_CMP_DROP ? 1u : 0u) << 32) | (k == HBX_CMP_MOVE ? 1u : 0u));
      p.tot[kTotMoved] = moved;
      p.tot[kTotMeta] = mbefore + (k != HBX_CMP_DROP ? HBX_META_HEAD + 16ull * p.ent[i].n_links : 0ull);
      p.tot[kTotCounts] = all;
      p.msrc[(uint32_t)all] = 0ull;
      p.mstart[(uint32_t)all] = moved;  // the end of the last mover
    }
    p.msz[i] = no;
    p.tsz[i] = mo;
  }
  wave_min(past, i, p.tot + kTotPast);
}

extern "C" __global__ __launch_bounds__(256) void hbx_k16_pack(hbxk::PackArgs p) {
  using namespace hbxk;
  const uint64_t t0 = (uint64_t)blockIdx.x * p.tile;
  if (t0 >= p.moved_bytes || p.n_moved == 0) return;  // (uniform)
  const uint64_t t1 = std::min<uint64_t>(t0 + p.tile, p.moved_bytes);
  // the tile's movers: every lane reads the same words
  const uint32_t first = mover_of(p.mstart, 0u, p.n_moved - 1u, t0);
  const uint32_t last = mover_of(p.mstart, first, p.n_moved - 1u, t1 - 1u);
  uint32_t k = first;
  for (uint32_t g = threadIdx.x; g < p.tile / 16u; g += kThreads) {
    const uint64_t s = t0 + 16ull * g;  // the granule's first byte in the stream
    if (s >= t1) break;
    k = mover_of(p.mstart, k, last, s);
    const uint64_t e0 = p.mstart[k], e1 = p.mstart[k + 1u];  // (k + 1 <= n_moved: the list has that word)
    const uint8_t* src = p.image + p.msrc[k];
    if (s + 16u <= e1) {  // inside one entry
      *reinterpret_cast<uint4*>(p.out + s) = hbxr::load16_any(src + (s - e0));
    } else if (s + 16u <= p.moved_bytes) {  // across a boundary: e1 < moved_bytes, so mover k + 1 exists
      const uint32_t c1 = (uint32_t)(e1 - s);  // 1..15 bytes from this entry, 16 - c1 from the next
      const uint4 a = hbxr::load16_any(src + (e1 - e0) - 16u);     // this entry's last 16 bytes
      const uint4 b = hbxr::load16_any(p.image + p.msrc[k + 1u]);  // the next entry's first 16
      unsigned __int128 lo, hi;
      __builtin_memcpy(&lo, &a, 16);
      __builtin_memcpy(&hi, &b, 16);
      const unsigned __int128 v = (lo >> (8u * (16u - c1))) | (hi << (8u * c1));
      uint4 o;
      __builtin_memcpy(&o, &v, 16);
      *reinterpret_cast<uint4*>(p.out + s) = o;
    } else {  // the stream's last, partial granule
      const uint8_t* nxt = k + 1u < p.n_moved ? p.image + p.msrc[k + 1u] : src;
      for (uint64_t q = s; q < p.moved_bytes; q++) p.out[q] = q < e1 ? src[q - e0] : nxt[q - e1];
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void hbx_k16_meta(hbxk::MetaArgs p) {
  using namespace hbxk;
  __shared__ uint32_t s_big[kThreads];
  __shared__ uint32_t s_nbig;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < p.n; base += stride) {
    const uint64_t i = base + threadIdx.x;
    const uint32_t k = i < p.n ? p.klass[i] : HBX_CMP_DROP;
    const bool has = k != HBX_CMP_DROP;
    uint32_t nl = 0;
    const uint8_t* lsrc = nullptr;
    uint8_t* ldst = nullptr;
    if (has) {
      const hbx_dat_entry& e = p.ent[i];
      nl = e.n_links;
      const uint64_t no = p.new_off[i], mo = p.meta_off[i];
      uint4 id;
      __builtin_memcpy(&id, e.id, 16);
      if (p.meta) {
        uint8_t h[HBX_META_HEAD];
        put_be32(h, HBX_DAT_MARKER);
        __builtin_memcpy(h + 4, &id, 16);
        put_location(h + 20, k == HBX_CMP_STAY ? p.a.file_no : p.a.dst_file_no, no);
        put_be32(h + 26, (uint32_t)e.size);
        put_be32(h + 30, nl);
        uint8_t* rec = p.meta + (mo - p.a.meta_base);
        __builtin_memcpy(rec, h, HBX_META_HEAD);
        lsrc = p.image + e.off + 24u;
        ldst = rec + HBX_META_HEAD;
      }
      if (p.ix) {
        uint8_t x[HBX_IX_ENTRY];
        const uint32_t flags = HBX_IX_F_EXISTS | (nl == 0 ? HBX_IX_F_NOLINKS : 0u);
        x[0] = (uint8_t)(flags >> 8);
        x[1] = (uint8_t)flags;
        __builtin_memcpy(x + 2, &id, 16);
        put_location(x + 18, p.a.meta_file_no, mo);
        __builtin_memcpy(p.ix + HBX_IX_ENTRY * (p.cnt[i] >> 32), x, HBX_IX_ENTRY);  // its rank among the kept
      }
    }
    if (!p.meta) continue;  // (uniform)
    // the links, by degree as hbxg::walk
    if (threadIdx.x == 0) s_nbig = 0;
    __syncthreads();
    if (nl > hbxg::kWaveMax) s_big[atomicAdd(&s_nbig, 1u)] = (uint32_t)i;  // (LDS; at most one per thread)
    if (nl <= hbxg::kLaneMax)
      for (uint32_t j = 0; j < nl; j++) copy_link(lsrc, ldst, j);
    for (unsigned long long rows = __ballot(nl > hbxg::kLaneMax && nl <= hbxg::kWaveMax); rows; rows &= rows - 1ull) {
      const int from = __builtin_ctzll(rows);
      const uint8_t* s = reinterpret_cast<const uint8_t*>(__shfl((long long)reinterpret_cast<uintptr_t>(lsrc), from, 64));
      uint8_t* d = reinterpret_cast<uint8_t*>(__shfl((long long)reinterpret_cast<uintptr_t>(ldst), from, 64));
      const uint32_t cnt = (uint32_t)__shfl((int)nl, from, 64);
      for (uint32_t j = lane; j < cnt; j += 64u) copy_link(s, d, j);
    }
    __syncthreads();
    const uint32_t nbig = s_nbig;
    for (uint32_t b = 0; b < nbig; b++) {
      const uint32_t r = s_big[b];
      const uint8_t* s = p.image + p.ent[r].off + 24u;
      uint8_t* d = p.meta + (p.meta_off[r] - p.a.meta_base) + HBX_META_HEAD;
      const uint32_t cnt = p.ent[r].n_links;
      for (uint32_t j = threadIdx.x; j < cnt; j += kThreads) copy_link(s, d, j);
    }
    __syncthreads();
  }
}

namespace hbxk {

inline uint32_t tile_of(int knob) { return knob == 256 || knob == 4096 || knob == 65536 ? (uint32_t)knob : kTile; }

}  // namespace hbxk
