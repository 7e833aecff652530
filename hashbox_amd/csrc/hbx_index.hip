// hbx_index.hip — K17: the store's open-addressed index files (*.idx) as
// images in device memory, and the reference's operations on them.
//
// Reference: pkg/storagedb/index.go (findIXOffset :54-107), gc.go:24-206
// (MarkIndexes, SweepIndexes, CompactIndexes), integrity.go:354-410
// (CheckIndexes): one goroutine, a seek and a read per probe.
// include/hbxgpu.h "Index files" states the format and THE RULE; hbx_index.h
// is every operation on the host.
//
// The images.  Every file of an hbx_index has its own allocation of the same
// capacity, 16 + 24 * columns bytes; a COLUMN is a slot number, shared by all
// files.  Behind a file's size the image holds zero bytes, always (the open,
// a compaction and a grown capacity see to it).  A zero slot reads as
// "Exists clear", and the rule treats such a slot exactly as it treats an
// offset at or past the file's end (it stops; the place is the remembered free
// one, else this one).  So inside the sweep the rule runs over the capacity
// (probe<true>) and a file's size is no state that two lanes share; outside it
// the rule runs over the sizes (probe<false>).
//
//   hbx_k17_probe    one lane per ID walks the rule.  A slot is 8-byte aligned
//                    (16 + 24 s), never 16: three 64-bit loads, the flags from
//                    the first, the ID compared as two 64-bit words put
//                    together by shifts, the location from the last.  A
//                    dependent gather, bound by latency: 256-thread workgroups
//                    of few registers, so many IDs are in flight per CU.
//   hbx_k17_mark / hbx_k17_update   the scatters behind a probe: one lane per
//                    hit sets Marked (one byte; idempotent), or replaces the
//                    location and the NoLinks bit (distinct IDs, distinct slots).
//   hbx_k17_count    one lane per slot, a workgroup per 256 slots of one file:
//                    the class of each slot, the counts per file (ballots; a
//                    workgroup strides over the tiles and adds its counts once
//                    per file), the live entries per tile.
//   hbx_k15_scan_*   K15's three-launch exclusive scan over the tile counts.
//   hbx_k17_pack     the same tiling: a live slot's rank is its tile's scan
//                    plus the ballot prefix; the live table in (file, offset)
//                    order, and `state` by the rule when it is wanted.
//   hbx_k17_spans    one lane per MARKED live entry: the interval of columns
//                    its sweep step can read or write, as +1 at its first
//                    column and -1 at its last in a difference array.
//                      file 0, home <= s < home + 682:  [home, s]
//                      otherwise:  [min(home, s), max(s, home + 681)]
//                    (the probes start at home in every file and make 682 at
//                    most; with stop_on_free they end at the first slot that
//                    is not live, at the ID, or, in file 0, at s itself).  An
//                    entry without a mark touches its own slot only.
//   hbx_k15_scan_*   the exclusive scan of the differences: link[c] = how many
//                    intervals hold both c - 1 and c.  A RANGE is a maximal
//                    run of columns joined by links: entries of two ranges
//                    share no column, so the ranges are independent, and
//                    inside one the reference's order is file-major, then by
//                    offset.
//   hbx_k17_sweep    one lane per column; the lane of a range's first column
//                    runs the reference's loop over it.  Its entries' ranks
//                    in the live table: one binary search per file, then by
//                    counting (a slot the lane reaches is as the sweep found
//                    it: a move only writes earlier in the order).  A move
//                    past a file's end raises that file's new size by an
//                    agent-scope max.
//   hbx_k17_tally / hbx_k15_scan_* / hbx_k17_kill_put   the actions counted
//                    (the sweep itself adds to no shared counter), and the
//                    deleted entries compacted in live order.
//   hbx_k17_compact  one lane per slot: an Invalid slot becomes three zero
//                    words; the last live slot per file by a max.
//
// Visibility: plain loads and stores; the counters, minima and maxima are
// agent-scope atomics; a kernel boundary publishes.  In the sweep a lane reads
// only what it or an earlier kernel wrote (its range's columns).  No spin, no
// grid barrier, no inline assembly; every loop is bounded by the probe limit,
// the file count, a range or a table.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hbxgpu.h"
#include "hbx_graph.hip"

namespace hbxx {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kTile = 256;  // slots of one file per workgroup of count / pack / compact
static_assert(HBX_IX_SWEEP_TILE == kThreads, "the sweep's columns per workgroup");
static_assert(sizeof(hbx_ix_hit) == 32 && sizeof(hbx_ix_live) == 48 && sizeof(hbx_ix_killed) == 32, "C-ABI");

struct File {
  uint8_t* img;
  uint64_t size;   // the file's size
  uint64_t slots;  // (size - 16) / 24
  uint64_t tile0;  // its first tile among all files' tiles
  uint64_t live0;  // the live entries in the files before it (the sweep sets it)
};
struct Tab {
  File f[HBX_IX_FILES_MAX];
  uint64_t lim;  // 16 + 24 * columns: every image's capacity
  uint32_t n;
};

// per file (unsigned long long each); behind the files' rows: the call's counters
enum { kStLive, kStInvalid, kStEmpty, kStMarked, kStNoLinks, kStMisplaced, kStFirstMisplaced, kStLastLive, kStMaxHome, kStWords };
enum { kCtObsolete, kCtCutOff, kCtMissing, kCtCleared, kCtAct, kCtFirstAbort = kCtAct + 6, kCtSize, kCtWords = kCtSize + HBX_IX_FILES_MAX };
constexpr uint32_t kStatWords = kStWords * HBX_IX_FILES_MAX + kCtWords;

struct Slot {
  uint64_t w0, w1, w2;
};
__device__ __forceinline__ Slot load_slot(const uint8_t* p) {
  const uint64_t* q = reinterpret_cast<const uint64_t*>(p);
  return Slot{q[0], q[1], q[2]};
}
__device__ __forceinline__ uint32_t flags_of(uint64_t w0) { return (uint32_t)__builtin_bswap16((uint16_t)w0); }
__device__ __forceinline__ bool live(uint32_t flags) { return (flags & HBX_IX_F_EXISTS) && !(flags & HBX_IX_F_INVALID); }
__device__ __forceinline__ uint64_t id_a(const Slot& s) { return (s.w0 >> 16) | (s.w1 << 48); }  // bytes 2..9
__device__ __forceinline__ uint64_t id_b(const Slot& s) { return (s.w1 >> 16) | (s.w2 << 48); }  // bytes 10..17
__device__ __forceinline__ uint64_t home_of(uint64_t idb) {  // id[13] << 16 | id[14] << 8 | id[15]
  return (((idb >> 40) & 0xFFull) << 16) | (((idb >> 48) & 0xFFull) << 8) | (idb >> 56);
}
__device__ __forceinline__ uint64_t location_of(uint64_t w2) { return __builtin_bswap64(w2) & 0xFFFFFFFFFFFFull; }
__device__ __forceinline__ uint64_t slot_off(uint64_t s) { return HBX_IX_HEADER + (uint64_t)HBX_IX_ENTRY * s; }

struct Place {
  bool found;
  uint32_t file;
  uint64_t off;
  uint64_t w0, w2;  // found: the slot's first and last word
};

// THE RULE (include/hbxgpu.h).  kPadded: over the capacity, whose tail is zero.
template <bool kPadded>
__device__ __forceinline__ Place probe(const Tab* t, uint64_t qa, uint64_t qb, bool stop_on_free) {
  const uint32_t n = t->n;
  const uint64_t base = slot_off(home_of(qb));
  uint32_t f = 0, free_f = 0;
  uint64_t o = base, free_o = base;
  bool have_free = false, stop = false;
  while (!stop && f < n) {
    const uint64_t size = kPadded ? t->lim : t->f[f].size;
    if (o > size) break;
    const uint8_t* img = t->f[f].img;
    for (uint32_t i = 0; i < HBX_IX_PROBE_LIMIT; i++) {
      if (o >= size) {
        stop = true;
        break;
      }
      const Slot s = load_slot(img + o);
      const uint32_t flags = flags_of(s.w0);
      if (live(flags)) {
        if (id_a(s) == qa && id_b(s) == qb) return Place{true, f, o, s.w0, s.w2};
      } else {
        if (!have_free) {
          free_f = f;
          free_o = o;
          have_free = true;
        }
        if (stop_on_free || !(flags & HBX_IX_F_EXISTS)) {
          stop = true;
          break;
        }
      }
      o += HBX_IX_ENTRY;
    }
    if (stop) break;
    f++;
    o = base;
  }
  if (have_free) return Place{false, free_f, free_o, 0, 0};
  return Place{false, f, o, 0, 0};
}

__device__ __forceinline__ void add(unsigned long long* w, unsigned long long v) {
  (void)__hip_atomic_fetch_add(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void amin(unsigned long long* w, unsigned long long v) {
  (void)__hip_atomic_fetch_min(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void amax(unsigned long long* w, unsigned long long v) {
  (void)__hip_atomic_fetch_max(w, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// The file of tile `tile` (uniform over the workgroup).
__device__ __forceinline__ uint32_t file_of_tile(const Tab* t, uint64_t tile) {
  uint32_t f = 0;
  while (f + 1 < t->n && tile >= t->f[f + 1].tile0) f++;
  return f;
}

struct ScanArgs {
  const Tab* tab;
  unsigned long long* stat;    // kStatWords
  unsigned long long* tcount;  // per tile: count writes the live entries, the scan their exclusive sums
  hbx_ix_live* live;
  uint64_t live_cap;
  uint64_t tiles;
  uint32_t want_state;
};

struct SweepArgs {
  const Tab* tab;
  const hbx_ix_live* live;
  const unsigned long long* link;   // columns + 1 words
  unsigned long long* stat;
  uint8_t* action;
  unsigned long long* moved_to;
  uint64_t n_live, columns;
};

}  // namespace hbxx

extern "C" __global__ __launch_bounds__(256) void hbx_k17_probe(const hbxx::Tab* tab, const uint64_t* ids, uint64_t n,
                                                                 uint32_t stop_on_free, hbx_ix_hit* hits) {
  using namespace hbxx;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const Place p = probe<false>(tab, ids[2 * i], ids[2 * i + 1], stop_on_free != 0);
  hbx_ix_hit h;
  h.found = p.found ? 1u : 0u;
  h.flags = p.found ? flags_of(p.w0) : 0u;
  h.file = p.file;
  const uint64_t l = p.found ? location_of(p.w2) : 0ull;
  h.meta_file = (uint32_t)(l >> 34);
  h.offset = p.off;
  h.meta_off = l & HBX_DAT_OFFSET_LIMIT;
  hits[i] = h;
}

extern "C" __global__ __launch_bounds__(256) void hbx_k17_mark(const hbxx::Tab* tab, const hbx_ix_hit* hits, uint64_t n,
                                                                uint8_t* found, unsigned long long* stat) {
  using namespace hbxx;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  bool miss = false;
  if (i < n) {
    const hbx_ix_hit h = hits[i];
    miss = h.found == 0;
    if (!miss) {
      uint8_t* p = tab->f[h.file].img + h.offset + 1;  // the low byte of the BE16 flags
      *p = (uint8_t)(*p | HBX_IX_F_MARKED);
    }
    found[i] = miss ? 0 : 1;
  }
  const unsigned long long m = __ballot(miss);
  if (m && (threadIdx.x & 63u) == 0) add(stat + HBX_IX_FILES_MAX * kStWords + kCtMissing, (unsigned long long)__popcll(m));
}

extern "C" __global__ __launch_bounds__(256) void hbx_k17_update(const hbxx::Tab* tab, const hbx_ix_hit* hits, uint64_t n,
                                                                  const uint8_t* recs, uint8_t* status) {
  using namespace hbxx;
  const uint64_t i = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const hbx_ix_hit h = hits[i];
  if (h.found) {
    uint8_t* p = tab->f[h.file].img + h.offset;
    const uint8_t* r = recs + (uint64_t)HBX_IX_ENTRY * i;
    p[1] = (uint8_t)((p[1] & ~HBX_IX_F_NOLINKS) | (r[1] & HBX_IX_F_NOLINKS));
#pragma unroll
    for (int b = 18; b < 24; b++) p[b] = r[b];
  }
  status[i] = h.found ? 0 : 1;
}

// The workgroup's counters of file f (LDS) into the call's, and cleared for the next file.
__device__ __forceinline__ void hbx_k17_flush(unsigned long long* s_c, unsigned long long* stat, uint32_t f) {
  using namespace hbxx;
  __syncthreads();
  if (threadIdx.x < kStWords) {
    unsigned long long* st = stat + (uint64_t)f * kStWords;
    const unsigned long long v = s_c[threadIdx.x];
    if (threadIdx.x == kStFirstMisplaced) {
      if (v != ~0ull) amin(st + threadIdx.x, v);
    } else if (threadIdx.x == kStLastLive || threadIdx.x == kStMaxHome) {
      if (v) amax(st + threadIdx.x, v);
    } else if (v) {
      add(st + threadIdx.x, v);
    }
    s_c[threadIdx.x] = threadIdx.x == kStFirstMisplaced ? ~0ull : 0ull;
  }
  __syncthreads();
}

// A workgroup takes the tiles blockIdx.x, + gridDim.x, ...: its counts stay in
// LDS and reach the call's counters once per file it met, not once per tile
// (tens of thousands of workgroups adding to the same few words run at the
// atomics' rate, not at the memory's).
extern "C" __global__ __launch_bounds__(256) void hbx_k17_count(hbxx::ScanArgs a) {
  using namespace hbxx;
  __shared__ unsigned long long s_c[kStWords];
  __shared__ uint32_t s_w[kThreads / 64];
  const Tab* t = a.tab;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  if (threadIdx.x < kStWords) s_c[threadIdx.x] = threadIdx.x == kStFirstMisplaced ? ~0ull : 0ull;
  __syncthreads();
  uint32_t cur = file_of_tile(t, blockIdx.x);
  for (uint64_t tile = blockIdx.x; tile < a.tiles; tile += gridDim.x) {
    const uint32_t f = file_of_tile(t, tile);
    if (f != cur) {  // (uniform)
      hbx_k17_flush(s_c, a.stat, cur);
      cur = f;
    }
    const uint64_t s = (tile - t->f[f].tile0) * kTile + threadIdx.x;
    bool is_live = false, inv = false, empty = false, marked = false, nolinks = false, misplaced = false;
    unsigned long long mh = 0;  // home + 1 of a live slot
    if (s < t->f[f].slots) {
      const Slot x = load_slot(t->f[f].img + slot_off(s));
      const uint32_t flags = flags_of(x.w0);
      inv = (flags & HBX_IX_F_INVALID) != 0;
      empty = !inv && !(flags & HBX_IX_F_EXISTS);
      is_live = !inv && !empty;
      if (is_live) {
        marked = (flags & HBX_IX_F_MARKED) != 0;
        nolinks = (flags & HBX_IX_F_NOLINKS) != 0;
        mh = home_of(id_b(x)) + 1;
        misplaced = s + 1 < mh;
      }
    }
    const unsigned long long b0 = __ballot(is_live), b1 = __ballot(inv), b2 = __ballot(empty), b3 = __ballot(marked),
                             b4 = __ballot(nolinks), b5 = __ballot(misplaced);
    // the extremes from one lane per wave: the slots ascend with the lane; the homes need every live lane
#pragma unroll
    for (int d = 32; d; d >>= 1) {
      const unsigned long long o = (unsigned long long)__shfl_xor((long long)mh, d, 64);
      mh = o > mh ? o : mh;
    }
    if (lane == 0) {
      s_w[wave] = (uint32_t)__popcll(b0);
      if (b0) {
        (void)atomicAdd(&s_c[kStLive], (unsigned long long)__popcll(b0));
        (void)atomicMax(&s_c[kStLastLive], (unsigned long long)(s + 64 - __builtin_clzll(b0)));
        (void)atomicMax(&s_c[kStMaxHome], mh);
      }
      if (b1) (void)atomicAdd(&s_c[kStInvalid], (unsigned long long)__popcll(b1));
      if (b2) (void)atomicAdd(&s_c[kStEmpty], (unsigned long long)__popcll(b2));
      if (b3) (void)atomicAdd(&s_c[kStMarked], (unsigned long long)__popcll(b3));
      if (b4) (void)atomicAdd(&s_c[kStNoLinks], (unsigned long long)__popcll(b4));
      if (b5) {
        (void)atomicAdd(&s_c[kStMisplaced], (unsigned long long)__popcll(b5));
        (void)atomicMin(&s_c[kStFirstMisplaced], (unsigned long long)slot_off(s + __builtin_ctzll(b5)));
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) a.tcount[tile] = (unsigned long long)s_w[0] + s_w[1] + s_w[2] + s_w[3];
    __syncthreads();
  }
  hbx_k17_flush(s_c, a.stat, cur);
}

extern "C" __global__ __launch_bounds__(256) void hbx_k17_pack(hbxx::ScanArgs a) {
  using namespace hbxx;
  __shared__ uint32_t s_w[kThreads / 64];
  const Tab* t = a.tab;
  const uint32_t f = file_of_tile(t, blockIdx.x);
  const uint64_t s = ((uint64_t)blockIdx.x - t->f[f].tile0) * kTile + threadIdx.x;
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  Slot x{0, 0, 0};
  bool is_live = false;
  if (s < t->f[f].slots) {
    x = load_slot(t->f[f].img + slot_off(s));
    is_live = live(flags_of(x.w0));
  }
  const unsigned long long b = __ballot(is_live);
  if (lane == 0) s_w[wave] = (uint32_t)__popcll(b);
  __syncthreads();
  if (!is_live) return;
  uint64_t j = a.tcount[blockIdx.x] + (uint64_t)__popcll(b & ((1ull << lane) - 1ull));
  for (uint32_t w = 0; w < wave; w++) j += s_w[w];
  const uint64_t o = slot_off(s);
  uint32_t state = 0;
  if (a.want_state) {
    const Place p = probe<false>(t, id_a(x), id_b(x), false);
    state = !p.found ? 2u : (p.file == f && p.off == o) ? 0u : 1u;
    if (state) add(a.stat + HBX_IX_FILES_MAX * kStWords + (state == 1 ? kCtObsolete : kCtCutOff), 1ull);
  }
  if (j >= a.live_cap) return;
  const uint64_t l = location_of(x.w2);
  hbx_ix_live e;
  const uint64_t ia = id_a(x), ib = id_b(x);
  __builtin_memcpy(e.id, &ia, 8);
  __builtin_memcpy(e.id + 8, &ib, 8);
  e.flags = flags_of(x.w0);
  e.ix_file = f;
  e.ix_offset = o;
  e.meta_file = (uint32_t)(l >> 34);
  e.state = state;
  e.meta_off = l & HBX_DAT_OFFSET_LIMIT;
  a.live[j] = e;
}

// diff[c] += 1 at an interval's first column, -= 1 at its last (columns + 1 words, zeroed before).
extern "C" __global__ __launch_bounds__(256) void hbx_k17_spans(const hbx_ix_live* live, uint64_t n_live, uint64_t columns,
                                                                 unsigned long long* diff) {
  using namespace hbxx;
  const uint64_t j = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (j >= n_live) return;
  const hbx_ix_live& e = live[j];
  if (!(e.flags & HBX_IX_F_MARKED)) return;  // deleted: its own slot only
  uint64_t ib;
  __builtin_memcpy(&ib, e.id + 8, 8);
  const uint64_t home = home_of(ib), s = (e.ix_offset - HBX_IX_HEADER) / HBX_IX_ENTRY;
  uint64_t lo, hi;
  if (e.ix_file == 0 && home <= s && s < home + HBX_IX_PROBE_LIMIT) {
    lo = home;
    hi = s;
  } else {
    lo = home < s ? home : s;
    hi = home + HBX_IX_PROBE_LIMIT - 1u;
    if (hi < s) hi = s;
  }
  if (hi > columns - 1u) hi = columns - 1u;  // (the capacity holds every home + 681: nothing is cut)
  if (lo >= hi) return;
  add(diff + lo, 1ull);
  add(diff + hi, ~0ull);  // -1
}

extern "C" __global__ __launch_bounds__(256) void hbx_k17_sweep(hbxx::SweepArgs a) {
  using namespace hbxx;
  const uint64_t c = (uint64_t)blockIdx.x * kThreads + threadIdx.x;
  if (c >= a.columns) return;
  if (c > 0 && a.link[c] != 0) return;  // joined to the column before: another lane's range
  uint64_t last = c;
  while (last + 1 < a.columns && a.link[last + 1] != 0) last++;
  const Tab* t = a.tab;
  unsigned long long* ct = a.stat + HBX_IX_FILES_MAX * kStWords;
  for (uint32_t f = 0; f < t->n; f++) {
    const uint64_t slots = t->f[f].slots;
    if (c >= slots) continue;
    const uint64_t end = last < slots - 1 ? last : slots - 1;
    uint8_t* img = t->f[f].img;
    uint64_t j = ~0ull;
    for (uint64_t s = c; s <= end; s++) {
      const uint64_t o = slot_off(s);
      uint8_t* p = img + o;
      const Slot x = load_slot(p);
      uint32_t flags = flags_of(x.w0);
      if (!live(flags)) continue;
      if (j == ~0ull) {  // the rank of the lane's first live entry in this file
        uint64_t lo = t->f[f].live0, hi = f + 1 < t->n ? t->f[f + 1].live0 : a.n_live;
        while (lo < hi) {
          const uint64_t mid = lo + (hi - lo) / 2;
          if (a.live[mid].ix_offset < o)
            lo = mid + 1;
          else
            hi = mid;
        }
        j = lo;
      } else {
        j++;
      }
      if (j >= a.n_live) return;  // (cannot be: the table names every live slot)
      uint32_t act;
      unsigned long long to_f = ~0ull, to_o = ~0ull;
      if (!(flags & HBX_IX_F_MARKED)) {
        flags |= HBX_IX_F_INVALID;
        act = HBX_IX_ACT_DELETED;
      } else {
        flags &= ~HBX_IX_F_MARKED;
        const Place q = probe<true>(t, id_a(x), id_b(x), true);
        if (q.file == f && q.off == o) {
          act = HBX_IX_ACT_STAY;
        } else if (q.found) {
          flags |= HBX_IX_F_INVALID;
          act = HBX_IX_ACT_OBSOLETE;
        } else if (q.file < f || (q.file == f && q.off < o)) {
          if (q.off + HBX_IX_ENTRY <= t->lim) {  // (always: the capacity holds home + 681)
            uint64_t* d = reinterpret_cast<uint64_t*>(t->f[q.file].img + q.off);
            d[0] = (x.w0 & ~0xFFFFull) | (uint64_t)__builtin_bswap16((uint16_t)flags);
            d[1] = x.w1;
            d[2] = x.w2;
            if (q.off + HBX_IX_ENTRY > t->f[q.file].size) amax(ct + kCtSize + q.file, q.off + HBX_IX_ENTRY);
          }
          to_f = q.file;
          to_o = q.off;
          flags |= HBX_IX_F_INVALID;
          act = HBX_IX_ACT_MOVED;
        } else {
          act = HBX_IX_ACT_ABORT;
        }
      }
      if (act != HBX_IX_ACT_ABORT) *reinterpret_cast<uint16_t*>(p) = __builtin_bswap16((uint16_t)flags);
      a.action[j] = (uint8_t)act;
      a.moved_to[2 * j] = to_f;
      a.moved_to[2 * j + 1] = to_o;
    }
  }
}

// The actions counted (one set of atomics per workgroup, which strides over the
// table), the first abort, and flag[j] = 1 where entry j was deleted.
extern "C" __global__ __launch_bounds__(256) void hbx_k17_tally(const uint8_t* action, uint64_t n_live,
                                                                 unsigned long long* flag, unsigned long long* stat) {
  using namespace hbxx;
  __shared__ unsigned long long s_n[6];
  if (threadIdx.x < 6) s_n[threadIdx.x] = 0;
  __syncthreads();
  unsigned long long* ct = stat + HBX_IX_FILES_MAX * kStWords;
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long cnt[6] = {0, 0, 0, 0, 0, 0};  // (lane 0 of each wave counts for it)
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < n_live; base += stride) {
    const uint64_t j = base + threadIdx.x;
    const uint32_t act = j < n_live ? action[j] : 0u;
    if (j < n_live) flag[j] = act == HBX_IX_ACT_DELETED ? 1ull : 0ull;
#pragma unroll
    for (uint32_t k = HBX_IX_ACT_DELETED; k <= HBX_IX_ACT_ABORT; k++) cnt[k] += (unsigned long long)__popcll(__ballot(act == k));
    const unsigned long long ab = __ballot(act == HBX_IX_ACT_ABORT);
    if (ab && (int)lane == __builtin_ctzll(ab)) amin(ct + kCtFirstAbort, j);
  }
  if (lane == 0)
    for (uint32_t k = HBX_IX_ACT_DELETED; k <= HBX_IX_ACT_ABORT; k++)
      if (cnt[k]) (void)atomicAdd(&s_n[k], cnt[k]);
  __syncthreads();
  if (threadIdx.x >= HBX_IX_ACT_DELETED && threadIdx.x <= HBX_IX_ACT_ABORT && s_n[threadIdx.x])
    add(ct + kCtAct + threadIdx.x, s_n[threadIdx.x]);
}

extern "C" __global__ __launch_bounds__(256) void hbx_k17_kill_put(const uint8_t* action, const hbx_ix_live* live,
                                                                    uint64_t n_live, const unsigned long long* rank,
                                                                    hbx_ix_killed* killed) {
  const uint64_t j = (uint64_t)blockIdx.x * hbxx::kThreads + threadIdx.x;
  if (j >= n_live || action[j] != HBX_IX_ACT_DELETED) return;
  hbx_ix_killed k;
  __builtin_memcpy(k.id, live[j].id, 16);
  k.meta_file = live[j].meta_file;
  k.reserved = 0;
  k.meta_off = live[j].meta_off;
  killed[rank[j]] = k;
}

// Tiles blockIdx.x, + gridDim.x, ... as hbx_k17_count: a wave's lane 0 keeps its
// counts and adds them once at the end, a file's last live slot when the file changes.
extern "C" __global__ __launch_bounds__(256) void hbx_k17_compact(const hbxx::Tab* t, uint64_t tiles,
                                                                   unsigned long long* stat) {
  using namespace hbxx;
  const uint32_t lane = threadIdx.x & 63u;
  unsigned long long cleared = 0, last = 0;
  uint32_t cur = file_of_tile(t, blockIdx.x);
  for (uint64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {
    const uint32_t f = file_of_tile(t, tile);
    if (f != cur) {  // (uniform)
      if (lane == 0 && last) amax(stat + (uint64_t)cur * kStWords + kStLastLive, last);
      last = 0;
      cur = f;
    }
    const uint64_t s = (tile - t->f[f].tile0) * kTile + threadIdx.x;
    bool inv = false, kept = false;
    if (s < t->f[f].slots) {
      uint64_t* p = reinterpret_cast<uint64_t*>(t->f[f].img + slot_off(s));
      const uint32_t flags = flags_of(p[0]);
      inv = (flags & HBX_IX_F_INVALID) != 0;
      kept = !inv && (flags & HBX_IX_F_EXISTS);
      if (inv) {
        p[0] = 0;
        p[1] = 0;
        p[2] = 0;
      }
    }
    const unsigned long long b = __ballot(inv), k = __ballot(kept);
    cleared += (unsigned long long)__popcll(b);
    if (k) {  // (lane 0 holds the wave's first slot: the slots ascend with the lane)
      const unsigned long long end = s + 64 - __builtin_clzll(k);
      last = end > last ? end : last;
    }
  }
  if (lane == 0) {
    if (last) amax(stat + (uint64_t)cur * kStWords + kStLastLive, last);
    if (cleared) add(stat + HBX_IX_FILES_MAX * kStWords + kCtCleared, cleared);
  }
}
