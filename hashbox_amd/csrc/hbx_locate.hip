// hbx_locate.hip — K13: for every block ID a restore needs, find where a pool
// of local files already holds a chunk with that ID, so that chunk's bytes
// come off the local disk instead of the wire.
//
// Reference: restoreFileData (hashback/restore.go:45-66) fetches every block of
// every file it writes.  A block ID binds the block's length and bytes
// (pkg/core/block.go:96-111), and content-defined chunking leaves the IDs of
// the chunks around a local change as they were: a chunk of ANY local file
// that carries a wanted ID is that block.  (The caller still hands the bytes to
// VerifyBlock: the pool was hashed a moment ago, not now.)
//
// For a pool P[0..np) and wanted IDs W[0..nw): src[j] = the lowest k with
// P[k] == W[j] in all 16 bytes, or none.  The lowest index makes the answer
// the same on every run.  The join is K9's scratch table with a payload
// (hbx_dedup.hip): a memset of table_slots(np) uint32 words (pool index + 1,
// 0 = empty; home slot and probing as K9 documents them), then two launches:
//   build   one thread per pool ID: CAS empty -> k + 1 from the home slot on;
//           on an occupied slot (or a lost CAS) compare P[v - 1] with the ID:
//           equal = atomicMin(slot, k + 1) and stop, different = next slot.  A
//           slot never changes its key, only its representative, which ends
//           as the key's lowest index.
//   lookup  one thread per wanted ID; nothing writes the table in this launch,
//           so it probes with plain loads until an empty slot (a miss) or a
//           slot whose P[v - 1] equals the ID.  A hit is resolved to its file
//           by binary search over pool_first (the last f with pool_first[f] <=
//           k, which steps over files without chunks) and written as one
//           32-byte hbx_block_loc with two uint4 stores.  Hits are counted with
//           one add per wave.
// Visibility, as K9: a slot word another workgroup may write in the same
// launch is touched with agent-scope atomics only; every plain load reads
// bytes nothing writes in that launch; the kernel boundary publishes the
// table.  Every probe loop is bounded by the table's size; no spin, no waiting
// for another lane.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hbxgpu.h"
#include "hbx_dedup.hip"

namespace hbxl {

constexpr uint32_t kThreads = 256;

// pool_first: files + 1 running counts from 0 (pool_first[files] == np);
// cut_ends runs parallel to pool and is relative to each file.
struct Args {
  const uint4* pool;
  const uint64_t* cut_ends;
  const uint64_t* pool_first;
  const uint4* want;
  uint32_t* table;  // mask + 1 words
  uint4* out;       // hbx_block_loc[nw], two uint4 each
  unsigned long long* found;
  uint32_t np, nw, files, mask;
};

}  // namespace hbxl

static_assert(sizeof(hbx_block_loc) == 32, "hbx_block_loc is two uint4");

extern "C" __global__ __launch_bounds__(256) void hbx_k13_build(hbxl::Args a) {
  using namespace hbxd;
  const uint32_t k = blockIdx.x * hbxl::kThreads + threadIdx.x;
  if (k >= a.np) return;
  const uint4 id = a.pool[k];
  uint32_t h = home_slot(id, a.mask);
  for (uint64_t step = 0; step <= a.mask; step++, h = (h + 1) & a.mask) {
    const uint32_t v = slot_cas(a.table + h, k + 1);
    if (!v) break;
    if (v <= a.np && id_eq(a.pool[v - 1], id)) {
      __hip_atomic_fetch_min(a.table + h, k + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
  }
}

extern "C" __global__ __launch_bounds__(256) void hbx_k13_lookup(hbxl::Args a) {
  using namespace hbxd;
  const uint32_t j = blockIdx.x * hbxl::kThreads + threadIdx.x;
  uint32_t hit = 0;  // pool index + 1
  if (j < a.nw && a.np) {
    const uint4 id = a.want[j];
    uint32_t h = home_slot(id, a.mask);
    for (uint64_t step = 0; step <= a.mask; step++, h = (h + 1) & a.mask) {
      const uint32_t v = a.table[h];
      if (!v) break;
      if (v <= a.np && id_eq(a.pool[v - 1], id)) {
        hit = v;
        break;
      }
    }
  }
  if (j < a.nw) {
    uint4 r0 = make_uint4(0xFFFFFFFFu, 0u, 0u, 0u), r1 = make_uint4(0u, 0u, 0u, 0u);
    if (hit) {
      const uint64_t k = hit - 1;
      uint32_t lo = 0, hi = a.files;  // pool_first[lo] <= k (pool_first[0] = 0), pool_first[hi] > k
      while (hi - lo > 1) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (a.pool_first[mid] <= k) lo = mid; else hi = mid;
      }
      const uint64_t c = k - a.pool_first[lo];
      const uint64_t end = a.cut_ends[k];
      const uint64_t off = c ? a.cut_ends[k - 1] : 0;
      const uint64_t len = end - off;
      r0 = make_uint4(lo, (uint32_t)c, (uint32_t)off, (uint32_t)(off >> 32));
      r1 = make_uint4((uint32_t)len, (uint32_t)(len >> 32), 0u, 0u);
    }
    a.out[2 * (uint64_t)j] = r0;
    a.out[2 * (uint64_t)j + 1] = r1;
  }
  // one add per wave: every lane of the wave reaches the ballot
  const unsigned long long m = __ballot(hit != 0);
  if (m && (threadIdx.x & 63u) == 0)
    __hip_atomic_fetch_add(a.found, (unsigned long long)__popcll(m), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

namespace hbxl {

// Enqueue K13 on `s`: the table cleared, built from the pool, then looked up.
// a.table must hold table_slots(a.np) words, a.mask = that - 1; *a.found is
// cleared here.
inline hipError_t locate(hipStream_t s, const Args& a) {
  if (!a.nw) return hipSuccess;
  hipError_t e = hipMemsetAsync(a.found, 0, sizeof(unsigned long long), s);
  if (e != hipSuccess) return e;
  if (a.np) {
    e = hipMemsetAsync(a.table, 0, ((uint64_t)a.mask + 1) * sizeof(uint32_t), s);
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(hbx_k13_build, dim3((a.np + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
  }
  hipLaunchKernelGGL(hbx_k13_lookup, dim3((a.nw + kThreads - 1) / kThreads), dim3(kThreads), 0, s, a);
  return hipGetLastError();
}

}  // namespace hbxl
