// hbx_graph.hip — K15: the block graph of a store on the device: every link
// resolved to the row of the block it names, the GC mark from the roots, and
// the block-tree check up from the damaged blocks.
//
// Reference: MarkIndexes (pkg/storagedb/gc.go:24-69) follows links breadth-
// first from every dataset state's block ID and marks what it reaches;
// checkBlockFromIXEntry (integrity.go:298-329) recurses into every link of a
// block and calls the block valid only if its own check passed, every link
// exists and every linked block is valid.  Both run on one goroutine with one
// index probe and one meta read per block.  Here the table is in device memory
// (include/hbxgpu.h states the semantics) and both are level-synchronous
// sweeps over it:
//
//   table          K13's (hbx_k13_build over the rows' IDs as they are): a
//                  slot ends as the LOWEST row carrying its ID, the ID's node.
//   hbx_k15_resolve  grid-stride over a list of 16-byte keys (the links, the
//                  roots, the rows' own IDs), one uint4 load and one probe
//                  each as hbx_k13_lookup probes (nothing writes the table in
//                  this launch: plain loads), one uint32 row or NONE stored.
//                  Misses (for the rows' own IDs: aliases, row != own index)
//                  are counted per wave by ballot + popcount, one add per wave.
//   rows by degree walk(): wherever a row's list is walked, a lane walks it
//                  alone only up to kLaneMax links; a longer list is walked by
//                  the row's whole wave, 64 consecutive words per step; one
//                  above kWaveMax by the row's whole workgroup, 256 words per
//                  step (the rows go through a list in LDS).  Every visit is a
//                  wave-converged call, so a visit may ballot.
//   hbx_k15_seed   every representative row: faulty (bad[i] or a missing link)
//                  = claimed at fault depth 0 and appended to the frontier.
//   hbx_k15_indeg / hbx_k15_scan_* / hbx_k15_fill   the transposed graph in
//                  CSR form, only when a faulty row exists: in-degree per
//                  target by agent-scope add, an exclusive scan in three plain
//                  launches (per-workgroup sums, a scan of the sums, add), and
//                  a fill whose add on the target's cursor turns the target's
//                  start into its end: afterwards row t's reverse list is
//                  [t ? rend[t - 1] : 0, rend[t]).  The order inside a list is
//                  arrival order; no output depends on it.
//   hbx_k15_roots  claims the resolved roots at mark depth 0.
//   hbx_k15_expand ONE BFS LEVEL, either direction: every link of every
//                  frontier row claims its target with an agent-scope
//                  CAS(depth + t, NONE, level + 1); winners are appended to
//                  the next frontier with K14's wave-aggregated append (one
//                  add per wave, lanes store behind that base).  A row is
//                  claimed once, so a frontier never holds more than n rows.
//                  The host reads the next frontier's length back and stops
//                  at 0.  The depth a row gets is its BFS level whichever
//                  lane wins; the frontier's order is arrival order and
//                  nothing that leaves the device depends on it.
//   hbx_k15_finish copies the depths of representatives to their aliases and
//                  counts marked, invalid and marked-and-invalid
//                  representatives, one add per wave and counter.
//
// Visibility, as K9 / K13: a word another workgroup may write in the same
// launch (a depth, a counter, a cursor) is touched with agent-scope atomics
// only; every plain load reads bytes nothing writes in that launch; every
// plain store goes to a word no other lane reads or writes in that launch.
// The kernel boundary publishes: a BFS level is a launch.  No grid-wide
// barrier, no spin, no waiting for another lane, no inline assembly; every
// loop is bounded by its table or its list.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "../../include/hbxgpu.h"
#include "hbx_dedup.hip"
#include "hbx_locate.hip"

namespace hbxg {

constexpr uint32_t kThreads = 256;
constexpr uint32_t kNone = HBX_GRAPH_NONE;
constexpr uint32_t kLaneMax = HBX_GRAPH_LANE_MAX;  // a lane walks a list of at most this many links alone
constexpr uint32_t kWaveMax = HBX_GRAPH_WAVE_MAX;  // a wave one of at most this many; a workgroup the rest
constexpr uint32_t kScanChunk = kThreads * 8;      // elements per workgroup of the exclusive scan
static_assert(kLaneMax <= 64 && kLaneMax < kWaveMax, "degree thresholds");

// counters of one call (unsigned long long each)
enum { kCntMissLinks, kCntMissRoots, kCntAlias, kCntMarked, kCntInvalid, kCntMarkedFaulty, kCntFrontier, kCntWords };

// Forward: row i's list is adj[base[i] .. base[i] + cnt[i]).  Transposed
// (rend != nullptr): adj[(i ? rend[i - 1] : 0) .. rend[i]).
struct Graph {
  const uint64_t* base;
  const uint32_t* cnt;
  const uint64_t* rend;
  const uint32_t* adj;
};

struct ResolveArgs {
  const uint4* ids;       // the table's keys: n rows
  const uint32_t* table;  // mask + 1 words, row + 1
  const uint4* keys;      // n_keys IDs to look up
  uint32_t* out;          // n_keys rows
  unsigned long long* count;
  uint64_t n_keys;
  uint32_t n, mask;
  uint32_t self;          // keys are the rows' own IDs: count out[e] != e, and a key without a slot is its own row
};

struct RowArgs {
  Graph g;
  const uint32_t* rep;
  const uint8_t* bad;           // seed: may be nullptr
  uint32_t* depth;              // seed: fault depths
  uint32_t* frontier;           // seed: the faulty rows
  unsigned long long* n_out;    // seed: their count
  unsigned long long* cursor;   // indeg: counts; fill: cursors (starts before, ends after)
  uint32_t* rsrc;               // fill: cap source rows
  uint64_t cap;                 // seed: frontier capacity; fill: capacity of rsrc
  uint32_t n;
};

struct RootArgs {
  const uint32_t* root_row;
  uint64_t n_roots;
  uint32_t* depth;
  uint32_t* frontier;
  unsigned long long* n_out;
  uint64_t cap;
};

struct ExpandArgs {
  Graph g;
  const uint32_t* frontier_in;
  uint64_t n_in;
  uint32_t* depth;
  uint32_t level;
  uint32_t* frontier_out;
  unsigned long long* n_out;
  uint64_t cap;
};

struct FinishArgs {
  const uint32_t* rep;
  uint32_t* mark;   // nullptr: the mark did not run
  uint32_t* fault;  // nullptr: the tree check did not run
  unsigned long long* counts;
  uint32_t n;
};

__device__ __forceinline__ void row_span(const Graph& g, uint32_t row, uint64_t* start, uint64_t* deg) {
  if (g.rend) {
    *start = row ? g.rend[row - 1] : 0;
    *deg = g.rend[row] - *start;
  } else {
    *start = g.base[row];
    *deg = g.cnt[row];
  }
}

// Claim depth[t] = value where it is NONE, for the lanes that want to, and
// append the winners' rows to a frontier: one add per wave, the winners store
// behind that base in lane order.  Wave-converged call.
__device__ __forceinline__ void claim(bool want, uint32_t t, uint32_t* depth, uint32_t value, uint32_t* frontier,
                                      unsigned long long* n_out, uint64_t cap, uint32_t lane) {
  bool won = false;
  if (want) {
    uint32_t seen = kNone;
    won = __hip_atomic_compare_exchange_strong(depth + t, &seen, value, __ATOMIC_RELAXED, __ATOMIC_RELAXED,
                                               __HIP_MEMORY_SCOPE_AGENT);
  }
  const unsigned long long w = __ballot(won);
  if (!w) return;
  unsigned long long base = 0;
  if (lane == 0)
    base = __hip_atomic_fetch_add(n_out, (unsigned long long)__popcll(w), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  base = (unsigned long long)__shfl((long long)base, 0, 64);
  if (won) {
    const uint64_t at = base + (uint64_t)__popcll(w & ((1ull << lane) - 1ull));
    if (at < cap) frontier[at] = t;
  }
}

// The lists of a workgroup's 256 rows (one per thread; has = this thread
// brings one), split by degree.  visit(valid, row, target) is called by all 64
// lanes of a wave together.  Workgroup-converged call; s_big holds kThreads
// words, s_nbig one.
template <class Visit>
__device__ __forceinline__ void walk(const Graph& g, bool has, uint32_t row, uint32_t* s_big, uint32_t* s_nbig,
                                     Visit&& visit) {
  const uint32_t lane = threadIdx.x & 63u;
  uint64_t start = 0, deg = 0;
  if (has) row_span(g, row, &start, &deg);
  if (threadIdx.x == 0) *s_nbig = 0;
  __syncthreads();
  if (deg > kWaveMax) s_big[atomicAdd(s_nbig, 1u)] = row;  // (LDS; at most one per thread)
  // a lane alone: at most kLaneMax links
  const uint32_t own = deg <= kLaneMax ? (uint32_t)deg : 0u;
  for (uint32_t k = 0; k < kLaneMax; k++) {
    const bool v = k < own;
    if (!__ballot(v)) break;
    const uint32_t t = v ? g.adj[start + k] : kNone;
    visit(v, row, t);
  }
  // the row's wave: 64 consecutive words per step
  for (unsigned long long rows = __ballot(deg > kLaneMax && deg <= kWaveMax); rows; rows &= rows - 1ull) {
    const int from = __builtin_ctzll(rows);
    const uint64_t s = (uint64_t)__shfl((long long)start, from, 64);
    const uint32_t d = (uint32_t)__shfl((int)(uint32_t)deg, from, 64);  // <= kWaveMax
    const uint32_t r = (uint32_t)__shfl((int)row, from, 64);
    for (uint32_t k = 0; k < d; k += 64u) {
      const bool v = k + lane < d;
      const uint32_t t = v ? g.adj[s + k + lane] : kNone;
      visit(v, r, t);
    }
  }
  __syncthreads();
  // the row's workgroup: 256 consecutive words per step
  const uint32_t nbig = *s_nbig;
  for (uint32_t b = 0; b < nbig; b++) {
    const uint32_t r = s_big[b];
    uint64_t s = 0, d = 0;
    row_span(g, r, &s, &d);
    for (uint64_t k = 0; k < d; k += kThreads) {
      const bool v = k + threadIdx.x < d;
      const uint32_t t = v ? g.adj[s + k + threadIdx.x] : kNone;
      visit(v, r, t);
    }
  }
  __syncthreads();
}

// A wave's exclusive prefix sum of v (every lane calls it); *total = the wave's sum.
__device__ __forceinline__ unsigned long long wave_excl64(unsigned long long v, uint32_t lane,
                                                          unsigned long long* total) {
  unsigned long long incl = v;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const unsigned long long up = (unsigned long long)__shfl_up((long long)incl, d, 64);
    if (lane >= (uint32_t)d) incl += up;
  }
  *total = (unsigned long long)__shfl((long long)incl, 63, 64);
  return incl - v;
}

// A workgroup's exclusive prefix sum of v (every thread calls it); s_w holds 4 words.
__device__ __forceinline__ unsigned long long block_excl64(unsigned long long v, unsigned long long* s_w,
                                                           unsigned long long* total) {
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long wt = 0;
  const unsigned long long ex = wave_excl64(v, lane, &wt);
  if (lane == 0) s_w[wave] = wt;
  __syncthreads();
  unsigned long long before = 0, all = 0;
#pragma unroll
  for (uint32_t w = 0; w < kThreads / 64; w++) {
    if (w < wave) before += s_w[w];
    all += s_w[w];
  }
  __syncthreads();
  *total = all;
  return before + ex;
}

enum RowMode { kSeed, kIndeg, kFill };

template <int Mode>
__device__ __forceinline__ void rows(const RowArgs& a, uint32_t* s_big, uint32_t* s_nbig) {
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < a.n; base += stride) {
    const uint64_t i = base + threadIdx.x;
    const bool has = i < a.n && a.rep[i] == (uint32_t)i;  // an alias row brings nothing
    const uint32_t row = (uint32_t)i;
    if (Mode == kSeed) claim(has && a.bad && a.bad[i], row, a.depth, 0u, a.frontier, a.n_out, a.cap, lane);
    walk(a.g, has, row, s_big, s_nbig, [&](bool v, uint32_t src, uint32_t t) {
      if (Mode == kSeed) {
        claim(v && t == kNone, src, a.depth, 0u, a.frontier, a.n_out, a.cap, lane);
      } else if (v && t != kNone) {
        const unsigned long long at =
            __hip_atomic_fetch_add(a.cursor + t, 1ull, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (Mode == kFill && at < a.cap) a.rsrc[at] = src;
      }
    });
  }
}

}  // namespace hbxg

extern "C" __global__ __launch_bounds__(256) void hbx_k15_resolve(hbxg::ResolveArgs a) {
  using namespace hbxg;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  unsigned long long counted = 0;
  // (base is the wave's first key: the loop condition is wave-uniform)
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u); base < a.n_keys; base += stride) {
    const uint64_t e = base + lane;
    uint32_t row = kNone;
    if (e < a.n_keys) {
      if (a.n) {
        const uint4 id = a.keys[e];
        uint32_t h = hbxd::home_slot(id, a.mask);
        for (uint64_t step = 0; step <= a.mask; step++, h = (h + 1) & a.mask) {
          const uint32_t v = a.table[h];
          if (!v) break;
          if (v <= a.n && hbxd::id_eq(a.ids[v - 1], id)) {
            row = v - 1;
            break;
          }
        }
      }
      if (a.self && row == kNone) row = (uint32_t)e;
      a.out[e] = row;
    }
    const bool c = e < a.n_keys && (a.self ? row != (uint32_t)e : row == kNone);
    counted += (unsigned long long)__popcll(__ballot(c));
  }
  if (lane == 0 && counted)
    __hip_atomic_fetch_add(a.count, counted, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

extern "C" __global__ __launch_bounds__(256) void hbx_k15_seed(hbxg::RowArgs a) {
  __shared__ uint32_t s_big[hbxg::kThreads];
  __shared__ uint32_t s_nbig;
  hbxg::rows<hbxg::kSeed>(a, s_big, &s_nbig);
}

extern "C" __global__ __launch_bounds__(256) void hbx_k15_indeg(hbxg::RowArgs a) {
  __shared__ uint32_t s_big[hbxg::kThreads];
  __shared__ uint32_t s_nbig;
  hbxg::rows<hbxg::kIndeg>(a, s_big, &s_nbig);
}

extern "C" __global__ __launch_bounds__(256) void hbx_k15_fill(hbxg::RowArgs a) {
  __shared__ uint32_t s_big[hbxg::kThreads];
  __shared__ uint32_t s_nbig;
  hbxg::rows<hbxg::kFill>(a, s_big, &s_nbig);
}

// sums[b] = the sum of x[b kScanChunk .. (b + 1) kScanChunk); grid = the chunks
extern "C" __global__ __launch_bounds__(256) void hbx_k15_scan_sums(const unsigned long long* x, uint64_t n,
                                                                    unsigned long long* sums) {
  using namespace hbxg;
  __shared__ unsigned long long s_w[kThreads / 64];
  const uint64_t first = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * 8u;
  unsigned long long v = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8u; j++)
    if (first + j < n) v += x[first + j];
  unsigned long long total = 0;
  (void)block_excl64(v, s_w, &total);
  if (threadIdx.x == 0) sums[blockIdx.x] = total;
}

// sums[0 .. nb) to its exclusive prefix sums, in place; one workgroup
extern "C" __global__ __launch_bounds__(256) void hbx_k15_scan_top(unsigned long long* sums, uint64_t nb) {
  using namespace hbxg;
  __shared__ unsigned long long s_w[kThreads / 64];
  unsigned long long carry = 0;
  for (uint64_t c = 0; c < nb; c += kThreads) {
    const uint64_t k = c + threadIdx.x;
    const unsigned long long v = k < nb ? sums[k] : 0ull;
    unsigned long long total = 0;
    const unsigned long long ex = block_excl64(v, s_w, &total);
    if (k < nb) sums[k] = carry + ex;
    carry += total;
  }
}

// x to its exclusive prefix sums, in place: a chunk's own scan plus sums[chunk]
extern "C" __global__ __launch_bounds__(256) void hbx_k15_scan_add(unsigned long long* x, uint64_t n,
                                                                   const unsigned long long* sums) {
  using namespace hbxg;
  __shared__ unsigned long long s_w[kThreads / 64];
  const uint64_t first = (uint64_t)blockIdx.x * kScanChunk + (uint64_t)threadIdx.x * 8u;
  unsigned long long e[8], v = 0;
#pragma unroll
  for (uint32_t j = 0; j < 8u; j++) {
    e[j] = first + j < n ? x[first + j] : 0ull;
    v += e[j];
  }
  unsigned long long total = 0;
  unsigned long long at = sums[blockIdx.x] + block_excl64(v, s_w, &total);
#pragma unroll
  for (uint32_t j = 0; j < 8u; j++) {
    if (first + j < n) x[first + j] = at;
    at += e[j];
  }
}

extern "C" __global__ __launch_bounds__(256) void hbx_k15_roots(hbxg::RootArgs a) {
  using namespace hbxg;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u); base < a.n_roots; base += stride) {
    const uint64_t q = base + lane;
    const uint32_t t = q < a.n_roots ? a.root_row[q] : kNone;
    claim(t != kNone, t, a.depth, 0u, a.frontier, a.n_out, a.cap, lane);
  }
}

extern "C" __global__ __launch_bounds__(256) void hbx_k15_expand(hbxg::ExpandArgs a) {
  using namespace hbxg;
  __shared__ uint32_t s_big[kThreads];
  __shared__ uint32_t s_nbig;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads; base < a.n_in; base += stride) {
    const uint64_t k = base + threadIdx.x;
    const bool has = k < a.n_in;
    const uint32_t row = has ? a.frontier_in[k] : 0u;
    walk(a.g, has, row, s_big, &s_nbig, [&](bool v, uint32_t, uint32_t t) {
      claim(v && t != kNone, t, a.depth, a.level + 1u, a.frontier_out, a.n_out, a.cap, lane);
    });
  }
}

extern "C" __global__ __launch_bounds__(256) void hbx_k15_finish(hbxg::FinishArgs a) {
  using namespace hbxg;
  const uint32_t lane = threadIdx.x & 63u;
  const uint64_t stride = (uint64_t)gridDim.x * kThreads;
  unsigned long long marked = 0, invalid = 0, both = 0;
  for (uint64_t base = (uint64_t)blockIdx.x * kThreads + (threadIdx.x & ~63u); base < a.n; base += stride) {
    const uint64_t i = base + lane;
    bool is_rep = false;
    uint32_t md = kNone, fd = kNone;
    if (i < a.n) {
      // (a representative's depths are read, an alias's written: never the same word)
      const uint32_t r = a.rep[i];
      is_rep = r == (uint32_t)i;
      if (a.mark) {
        md = a.mark[r];
        if (!is_rep) a.mark[i] = md;
      }
      if (a.fault) {
        fd = a.fault[r];
        if (!is_rep) a.fault[i] = fd;
      }
    }
    marked += (unsigned long long)__popcll(__ballot(is_rep && md != kNone));
    invalid += (unsigned long long)__popcll(__ballot(is_rep && fd != kNone));
    both += (unsigned long long)__popcll(__ballot(is_rep && md != kNone && fd != kNone));
  }
  if (lane == 0) {
    if (marked) __hip_atomic_fetch_add(a.counts + kCntMarked, marked, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (invalid) __hip_atomic_fetch_add(a.counts + kCntInvalid, invalid, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (both) __hip_atomic_fetch_add(a.counts + kCntMarkedFaulty, both, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

namespace hbxg {

// The grid of a K15 launch over `items`: every item once, at most 2,048
// workgroups (8 per CU) as K14's, or the knob's count (tests).
inline uint32_t grid(uint64_t items, uint32_t knob) {
  const uint64_t wgs = (items + kThreads - 1) / kThreads;
  const uint64_t most = knob ? knob : 2048u;
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(wgs, most));
}

}  // namespace hbxg
