// hbx_match.hip — K12: compare each file's local block-ID list with the chain
// the store holds for it, so a diff or a restore over an existing tree skips
// the files whose blocks need not come off the wire.
//
// Reference: diffEntry / diffFileData (hashback/restore.go:249-277, 317-367)
// fetch, verify and compare every data block of every file.  A file's stored
// chain is its list of block IDs, and a block ID binds the block's length and
// bytes (pkg/core/block.go:96-111): if cutting and hashing the local file gives
// the same ID list, the file equals the stored one.  The converse does not
// hold (a chain cut by another chunker names the same bytes with other IDs), so
// a mismatch only sends the file to the byte comparison.
//
// One wave per file (grid = files x 64 threads, as K4).  In step i lane l loads
// the local and the expected ID of chunk i + l (one uint4 each) and compares
// them; the wave ballots and stops at the first step that holds a mismatch, or
// at min(n_local, n_expect).  Lane 0 writes the file's 32-byte record.  No LDS,
// no atomics, plain loads; both loops are bounded by the two counts.  Nothing
// is read past counts[f] result slots (clamped to the slots the batch has) or
// past expect_first[f + 1].
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/hbxgpu.h"
#include "hbx_dedup.hip"

namespace hbxm {

// `local` is the view K9 takes of a batch's result slots: file f's IDs are
// local.ids[cut_base[f] ..], counts[f] of them (K3 and K2 left them there);
// local.n is the number of slots.  counts == nullptr (the direct call): a
// packed list, cut_base holds files + 1 running counts.  cut_ends (may be
// nullptr) runs parallel to the IDs.  expect_first holds files + 1 running
// counts into expect_ids; both may lie in pinned host memory.
struct Args {
  hbxd::Ids local;
  const uint64_t* cut_ends;
  const uint64_t* expect_first;
  const uint4* expect_ids;
  uint4* out;  // hbx_chain_match[files], two uint4 each
};

}  // namespace hbxm

static_assert(sizeof(hbx_chain_match) == 32, "hbx_chain_match is two uint4");

extern "C" __global__ __launch_bounds__(64) void hbx_k12_chain_match(hbxm::Args a) {
  const uint32_t f = blockIdx.x, lane = threadIdx.x;
  if (f >= a.local.files) return;
  const uint64_t base = a.local.cut_base[f];
  uint64_t nl64 = a.local.counts ? (uint64_t)a.local.counts[f] : a.local.cut_base[f + 1] - base;
  const uint64_t room = base < a.local.n ? (uint64_t)a.local.n - base : 0;
  if (nl64 > room) nl64 = room;
  const uint32_t n_local = (uint32_t)nl64;
  const uint64_t e0 = a.expect_first[f];
  const uint32_t n_expect = (uint32_t)(a.expect_first[f + 1] - e0);
  const uint32_t lim = n_local < n_expect ? n_local : n_expect;
  const uint4* lp = a.local.ids + base;
  const uint4* ep = a.expect_ids + e0;
  uint32_t n_match = lim;
  for (uint32_t i = 0; i < lim; i += 64) {  // (i and lim are wave-uniform)
    const uint32_t k = i + lane;
    bool differs = false;
    if (k < lim) differs = !hbxd::id_eq(lp[k], ep[k]);
    const unsigned long long m = __ballot(differs);
    if (m) {
      n_match = i + (uint32_t)__ffsll(m) - 1u;
      break;
    }
  }
  if (lane != 0) return;
  const uint64_t mb = (a.cut_ends && n_match) ? a.cut_ends[base + n_match - 1] : 0;
  const uint32_t same = (n_match == n_local && n_match == n_expect) ? 1u : 0u;
  a.out[2 * (uint64_t)f] = make_uint4(n_match, n_local, n_expect, same);
  a.out[2 * (uint64_t)f + 1] = make_uint4((uint32_t)mb, (uint32_t)(mb >> 32), 0u, 0u);
}

namespace hbxm {

// Enqueue K12 over `files` files on `s`.
inline hipError_t match(hipStream_t s, const Args& a) {
  if (!a.local.files) return hipSuccess;
  hipLaunchKernelGGL(hbx_k12_chain_match, dim3(a.local.files), dim3(64), 0, s, a);
  return hipGetLastError();
}

}  // namespace hbxm
