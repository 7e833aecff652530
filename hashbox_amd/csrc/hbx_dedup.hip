// hbx_dedup.hip — K9: a device-resident set of block IDs, consulted in submit
// order so that only blocks never seen before are compressed and sent.
//
// Reference: the client compresses a block only once it is known to be new:
// StoreBlock drops an ID already in its queue map (pkg/core/client.go:571-576),
// the server answers allo with ACKN for a block it holds (server/server.go:
// 160-168), and a send worker calls CompressData only for blocks the server
// asked for with READ (client.go:211-214, 249-258).
//
// Layout of a set of capacity C (hbx_idset, include/hbxgpu.h):
//   keys   uint4[C]   the IDs in insertion order, append-only
//   slots  uint32[S]  key index + 1, or 0 for empty; S = hbx_idset_slots(C):
//                     the smallest power of two >= 2 C, at least 64
//   ctl    {uint32 count, uint32 pad, uint64 dropped}
// HOME SLOT of an ID = LE64(id[0..8]) & (S - 1), linear probing that wraps
// around (an MD5 needs no further mixing).  Tests build collisions from this
// rule.  A slot holds an index because a 32-bit word can be claimed with one
// atomic and a 128-bit key cannot; a reader compares against keys[index],
// which a kernel boundary published.
//
// One MARK over n IDs in order 0..n-1 (hbxd::mark) is a memset of a scratch
// slot table (uint32, a power of two >= 2 n, input index + 1) and three
// launches:
//   probe    looks every ID up in the set (read-only in this launch: plain
//            loads).  Found = seen.  Otherwise the ID goes into the scratch
//            table: CAS empty -> i + 1; on an occupied slot (or a lost CAS)
//            compare ids[j] with ids[i]: equal = atomicMin(slot, i + 1),
//            different = next slot.  A slot never changes its key, only its
//            representative, which ends as the key's lowest index.
//   resolve  every ID not found looks its key's scratch slot up (nothing
//            writes that table in this launch): fresh[i] = (owner == i).
//   insert   every fresh ID takes position p = atomicAdd(count, 1); p < C:
//            keys[p] = id and the first empty slot from its home is claimed
//            with CAS empty -> p + 1, moving on WITHOUT comparing after a
//            lost CAS (the keys one launch inserts are distinct from each
//            other and from the set); p >= C: the ID is counted in `dropped`,
//            count is put back, and nothing is inserted.
// Visibility (no hand-off inside a launch, no spin, no waiting for another
// lane): a slot word that another workgroup may write in the same launch is
// touched with agent-scope atomics only; every plain load reads bytes no
// workgroup writes in that launch; kernel boundaries publish keys and the
// finished tables.  Every probe loop is bounded by its table's size.
//
// THE INVARIANT: an ID is reported seen (fresh = 0) only if an equal 16-byte
// ID was inserted before it, by an earlier mark or at a lower index of this
// one.  A wrong "seen" loses data (the block is never sent); a wrong "fresh"
// costs only work.  So a full set degrades to fresh: a dropped ID is never
// found, and is fresh again the next time.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace hbxd {

constexpr uint32_t kThreads = 256;
constexpr uint8_t kSeen = 0, kFresh = 1, kPending = 2;  // fresh[]: kPending only between probe and resolve
constexpr uint64_t kMaxCapacity = 1ull << 31;           // key index + 1 fits a slot word
constexpr uint64_t kMaxMark = 1ull << 30;               // IDs per mark: 2 n scratch slots, index + 1 in 32 bits

// Slots of a table holding up to n keys: the smallest power of two >= 2 n, at
// least 64 (0 for n beyond kMaxCapacity).
inline uint64_t table_slots(uint64_t n) {
  if (n > kMaxCapacity) return 0;
  uint64_t s = 64;
  while (s < 2 * n) s <<= 1;
  return s;
}

struct Set {
  uint4* keys;
  uint32_t* slots;
  uint32_t* ctl;  // [0] count, [2..3] dropped (uint64)
  uint32_t capacity;
  uint32_t mask;  // S - 1
};

// The IDs of a mark.  files == 0: a plain list, every index is an ID.
// Otherwise the result slots of a pipeline batch: slot k belongs to the file f
// with cut_base[f] <= k < cut_base[f + 1] and holds an ID where
// k - cut_base[f] < counts[f].
struct Ids {
  const uint4* ids;
  const uint64_t* cut_base;
  const uint32_t* counts;
  uint32_t n, files;
};

__device__ __forceinline__ bool id_eq(uint4 a, uint4 b) {
  return ((a.x ^ b.x) | (a.y ^ b.y) | (a.z ^ b.z) | (a.w ^ b.w)) == 0u;
}
__device__ __forceinline__ uint32_t home_slot(uint4 id, uint32_t mask) {
  return (uint32_t)((((uint64_t)id.y << 32) | id.x) & (uint64_t)mask);
}
__device__ __forceinline__ bool holds_id(const Ids& in, uint32_t k) {
  if (!in.files) return true;
  uint32_t lo = 0, hi = in.files;  // cut_base[lo] <= k (cut_base[0] = 0, strictly increasing)
  while (hi - lo > 1) {
    const uint32_t mid = lo + (hi - lo) / 2;
    if (in.cut_base[mid] <= k) lo = mid; else hi = mid;
  }
  return k - in.cut_base[lo] < in.counts[lo];
}
__device__ __forceinline__ uint32_t slot_cas(uint32_t* p, uint32_t want) {  // the word found (0 = claimed)
  uint32_t seen = 0;
  __hip_atomic_compare_exchange_strong(p, &seen, want, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  return seen;
}
// Index + 1 of `id` in the set, 0 if it is not there.  The set is not written
// in the calling launch.
__device__ __forceinline__ uint32_t set_find(const Set& s, uint4 id) {
  uint32_t h = home_slot(id, s.mask);
  for (uint64_t step = 0; step <= s.mask; step++, h = (h + 1) & s.mask) {
    const uint32_t v = s.slots[h];
    if (!v) return 0;
    if (v <= s.capacity && id_eq(s.keys[v - 1], id)) return v;
  }
  return 0;
}

}  // namespace hbxd

extern "C" __global__ __launch_bounds__(hbxd::kThreads) void hbx_k9_probe(hbxd::Set set, hbxd::Ids in,
                                                                          uint32_t* scratch, uint32_t qmask,
                                                                          uint8_t* fresh) {
  using namespace hbxd;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= in.n) return;
  if (!holds_id(in, i) || set_find(set, in.ids[i])) {
    fresh[i] = kSeen;
    return;
  }
  const uint4 id = in.ids[i];
  uint32_t h = home_slot(id, qmask);
  for (uint64_t step = 0; step <= qmask; step++, h = (h + 1) & qmask) {
    const uint32_t v = slot_cas(scratch + h, i + 1);
    if (!v) break;
    if (v <= in.n && id_eq(in.ids[v - 1], id)) {
      __hip_atomic_fetch_min(scratch + h, i + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break;
    }
  }
  fresh[i] = kPending;
}

extern "C" __global__ __launch_bounds__(hbxd::kThreads) void hbx_k9_resolve(hbxd::Ids in, const uint32_t* scratch,
                                                                            uint32_t qmask, uint8_t* fresh) {
  using namespace hbxd;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= in.n || fresh[i] != kPending) return;
  const uint4 id = in.ids[i];
  uint32_t owner = i;  // (a key without a slot cannot happen with 2 n slots; it would be fresh, the safe side)
  uint32_t h = home_slot(id, qmask);
  for (uint64_t step = 0; step <= qmask; step++, h = (h + 1) & qmask) {
    const uint32_t v = scratch[h];
    if (!v) break;
    if (v <= in.n && id_eq(in.ids[v - 1], id)) {
      owner = v - 1;
      break;
    }
  }
  fresh[i] = owner == i ? kFresh : kSeen;
}

extern "C" __global__ __launch_bounds__(hbxd::kThreads) void hbx_k9_insert(hbxd::Set set, hbxd::Ids in,
                                                                           const uint8_t* fresh) {
  using namespace hbxd;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= in.n || fresh[i] != kFresh) return;
  const uint32_t p = __hip_atomic_fetch_add(set.ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (p >= set.capacity) {  // full: count stays at the capacity (it never drops below it again)
    __hip_atomic_fetch_sub(set.ctl, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(set.ctl + 2), 1ull, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
    return;
  }
  const uint4 id = in.ids[i];
  set.keys[p] = id;
  uint32_t h = home_slot(id, set.mask);
  for (uint64_t step = 0; step <= set.mask; step++, h = (h + 1) & set.mask)
    if (!slot_cas(set.slots + h, p + 1)) break;
}

// The slots of keys[0 .. m) into a cleared slot table (hbx_idset_truncate).
extern "C" __global__ __launch_bounds__(hbxd::kThreads) void hbx_k9_rebuild(hbxd::Set set, uint32_t m) {
  using namespace hbxd;
  const uint32_t p = blockIdx.x * kThreads + threadIdx.x;
  if (p >= m) return;
  uint32_t h = home_slot(set.keys[p], set.mask);
  for (uint64_t step = 0; step <= set.mask; step++, h = (h + 1) & set.mask)
    if (!slot_cas(set.slots + h, p + 1)) break;
}

extern "C" __global__ __launch_bounds__(hbxd::kThreads) void hbx_k9_contains(hbxd::Set set, const uint4* ids,
                                                                             uint32_t n, uint8_t* found) {
  using namespace hbxd;
  const uint32_t i = blockIdx.x * kThreads + threadIdx.x;
  if (i < n) found[i] = set_find(set, ids[i]) ? 1 : 0;
}

namespace hbxd {

// Enqueue one mark on `s`: fresh[i] = 1 for the first occurrence of an ID the
// set does not hold, which is then inserted; 0 elsewhere (and for a slot that
// holds no ID).  `scratch` must hold table_slots(in.n) words.
inline hipError_t mark(hipStream_t s, const Set& set, const Ids& in, uint32_t* scratch, uint8_t* fresh) {
  if (!in.n) return hipSuccess;
  const uint64_t q = table_slots(in.n);
  const dim3 grid((in.n + kThreads - 1) / kThreads), block(kThreads);
  hipError_t e = hipMemsetAsync(scratch, 0, q * sizeof(uint32_t), s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(hbx_k9_probe, grid, block, 0, s, set, in, scratch, (uint32_t)(q - 1), fresh);
  hipLaunchKernelGGL(hbx_k9_resolve, grid, block, 0, s, in, static_cast<const uint32_t*>(scratch), (uint32_t)(q - 1),
                     fresh);
  hipLaunchKernelGGL(hbx_k9_insert, grid, block, 0, s, set, in, static_cast<const uint8_t*>(fresh));
  return hipGetLastError();
}

}  // namespace hbxd
