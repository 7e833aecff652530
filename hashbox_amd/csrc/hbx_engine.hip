// hbx_engine.hip — host engine + C-ABI (include/hbxgpu.h) for libhbxgpu.so.
//
// One context = one GPU + one HIP stream + a grown-on-demand workspace.  A
// batch of files runs as five launches on the stream:
//   K1  window-digest scan  grid = tiles (16 MiB of one file each), 1024 thr
//   K2  cut chain           grid = files, 1 wave each (sequential store.go loop)
//   K2c plan                1 workgroup: chunks bucketed by length, longest first
//   K3  block MD5           one 512-thread workgroup per CU, lane per chunk
//   K4  content id          grid = files/64, lane per file
// then one D2H of counts/cuts/ids/content ids into pinned memory.
// Reference seams: hashback/store.go:111-199 (storeFile), pkg/core/client.go:
// 556-560 + block.go:96-111 (StoreData -> HashData).
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hsa/hsa.h>
#include <hsa/hsa_ext_amd.h>

#include <fcntl.h>
#include <sys/stat.h>
#include <unistd.h>

#include <cerrno>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <functional>
#include <future>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/hbxgpu.h"
#include "hbx_kernels.hip"
#include "hbx_deflate.hip"
#include "hbx_inflate.hip"
#include "hbx_inflate_split.hip"
#include "hbx_dedup.hip"
#include "hbx_match.hip"
#include "hbx_locate.hip"
#include "hbx_restore.hip"
#include "hbx_restore_many.hip"
#include "hbx_datfile.hip"
#include "hbx_graph.hip"
#include "hbx_compact.hip"
#include "hbx_index.hip"
#include "hbx_formats.h"
#include "hbx_wire.h"
#include "hbx_datfile.h"
#include "hbx_compact.h"
#include "hbx_index.h"

namespace {

struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap && p) return hipSuccess;
    if (p) {
      hipError_t e = hipFree(p);
      if (e != hipSuccess) return e;
      p = nullptr;
      cap = 0;
    }
    size_t want = std::max<size_t>(n, 256);
    want = (want + 4095) & ~size_t(4095);
    hipError_t e = hipMalloc(&p, want);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

struct PinBuf {
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t n) {
    if (n <= cap && p) return hipSuccess;
    if (p) {
      (void)hipHostFree(p);
      p = nullptr;
      cap = 0;
    }
    size_t want = std::max<size_t>(n, 4096);
    want = (want + 4095) & ~size_t(4095);
    hipError_t e = hipHostMalloc(&p, want, hipHostMallocDefault);
    if (e == hipSuccess) cap = want;
    return e;
  }
  void release() {
    if (p) (void)hipHostFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const {
    return static_cast<T*>(p);
  }
};

// Per-kernel cumulative timing: one event pair per launch, harvested once the
// end event has completed (hbx_stage_totals).  `owned`: the pair came from
// the context's pool (returned there once harvested); a pair of a batch's own
// events (lean marks) stays with the batch.
struct TimedLaunch {
  hipEvent_t a, b;
  int stage;
  bool owned = true;
};

// Layout of a batch's results, the same on the device (d_res) and in the
// pinned host block (h_res), so one copy moves them all.
struct ResLayout {
  size_t counts = 0, cuts = 0, ids = 0, cid = 0, ctype = 0, total = 0;
  size_t fresh = 0;  // K9 flags, one byte per result slot: only for a batch submitted with an ID set
  size_t match = 0;  // K12 records, 32 bytes per file: only for a batch submitted with expected chains
};
inline size_t al256(size_t x) { return (x + 255) & ~size_t(255); }
ResLayout res_layout(uint64_t n_files, uint64_t total_cap, bool dedup = false, bool match = false) {
  ResLayout r;
  r.cuts = al256(n_files * 4);
  r.ids = r.cuts + al256(total_cap * 8);
  r.cid = r.ids + al256(total_cap * 16);
  r.ctype = r.cid + al256(n_files * 16);
  r.total = r.ctype + al256(n_files * 4);
  if (dedup) {  // behind everything else: the layout and the copy of a batch without a set do not change
    r.fresh = r.total;
    r.total += al256(total_cap);
  }
  if (match) {  // likewise behind everything else; without a set it follows the content ids and types, so a
                // verdict-only batch pushes [cid, total): its per-file sections in one contiguous range
    r.match = r.total;
    r.total += al256(n_files * sizeof(hbx_chain_match));
  }
  return r;
}

}  // namespace

// One file streamed in segments (hbx_seg_open).  The carry word lives in
// device memory (a slot of hbx_ctx::seg_words): K2 of segment j stores the
// chain's resume point there and K2 of segment j+1 loads it, so no segment
// waits for the host.  The host side keeps what the final content id needs.
struct hbx_seg {
  uint64_t file_len = 0;
  uint64_t* d_carry = nullptr;
  uint64_t end = 0;           // file offset where the latest submitted segment ends
  bool any = false;           // a segment has been submitted
  bool final_sent = false;    // the final segment has been submitted
  uint32_t inflight = 0;      // submitted segments not yet collected
  std::vector<uint8_t> ids;   // the file's chunk ids collected so far (the chain block's links)
  bool keep_cuts = false;     // hbx_store_file_seg: collect the cut ends here too
  std::vector<uint64_t> cuts;
  uint64_t last_cut = 0;      // the latest collected cut end: where the next segment's first chunk starts
};

// A set of block IDs in device memory (hbx_idset_create; layout and kernels:
// hbx_dedup.hip).  Every kernel that touches it runs on the context's result
// stream, so marks, lookups and rebuilds are ordered by that stream alone.
struct hbx_idset {
  uint64_t capacity = 0, slots = 0;
  DevBuf d_keys, d_slots, d_ctl;
  DevBuf d_in, d_flag, d_scratch;  // the direct calls' staging: IDs, flags, scratch slot table
  uint32_t inflight = 0;           // pending batches submitted with it
  hbxd::Set view() const {
    return hbxd::Set{d_keys.as<uint4>(), d_slots.as<uint32_t>(), d_ctl.as<uint32_t>(), (uint32_t)capacity,
                     (uint32_t)(slots - 1)};
  }
  void release() {
    for (DevBuf* d : {&d_keys, &d_slots, &d_ctl, &d_in, &d_flag, &d_scratch}) d->release();
  }
};

// A store's index files in device memory (hbx_index_open; layout and kernels:
// hbx_index.hip).  Every image has the capacity 16 + 24 * columns and is zero
// behind its size.  Every kernel that touches it runs on the result stream.
struct hbx_index {
  uint32_t n = 0;
  uint64_t columns = 0, tiles = 0;
  uint64_t size[HBX_IX_FILES_MAX] = {};
  hbxx::Tab tab;  // what d_tab holds
  DevBuf img[HBX_IX_FILES_MAX], save[HBX_IX_FILES_MAX];
  // the table, the counters, the tiles' scan, the live table; a call's IDs / records, hits and flags;
  // the sweep's links, actions, targets, the deleted entries' ranks and records
  DevBuf d_tab, d_stat, d_tiles, d_live, d_in, d_hits, d_out, d_link, d_act, d_moved, d_kflag, d_killed;
  void release() {
    for (DevBuf& d : img) d.release();
    for (DevBuf& d : save) d.release();
    for (DevBuf* d : {&d_tab, &d_stat, &d_tiles, &d_live, &d_in, &d_hits, &d_out, &d_link, &d_act, &d_moved, &d_kflag,
                      &d_killed})
      d->release();
  }
};

namespace {

// One submitted batch.  Its device buffers live until its results are
// collected: K3 writes BlockIDs into d_ids across several launches when the
// MD5 stage is time-sliced.
struct Batch {
  uint64_t n = 0, caps = 0;
  std::vector<uint64_t> cut_base;
  DevBuf d_meta, d_res;  // d_res: cut counts | cut ends | ids | content ids | types (rl)
  ResLayout rl;
  uint8_t* res(size_t off) const { return static_cast<uint8_t*>(d_res.p) + off; }
  uint64_t* cuts_d() const { return reinterpret_cast<uint64_t*>(res(rl.cuts)); }
  uint32_t* count_d() const { return reinterpret_cast<uint32_t*>(res(rl.counts)); }
  uint32_t* ids_d() const { return reinterpret_cast<uint32_t*>(res(rl.ids)); }
  DevBuf d_run, d_fresh, d_fcnt;  // the batch's MD5 chains (K2r), their order entries, count
  PinBuf h_meta, h_res;
  uint64_t* cut_ends = nullptr;
  uint8_t* ids = nullptr;
  hbx_file_summary* sums = nullptr;
  std::vector<uint64_t> out_base, capv;
  uint32_t need = 1, done = 0;  // K3 launches its chains need / have had
  bool joined = false;          // its chains are in the carried order lists (a plan took them)
  bool ev3 = false;             // ev[3] recorded (synchronous batches only)
  bool k2_ev5 = false;          // lean marks: K2's end is ev[5] and ev[2] is not recorded
  uint64_t final_launch = 0;    // index of the K3 launch after which it was finalized
  bool finalized = false;
  // a VerifyBlock batch (hbx_verify_submit_device) instead of files
  bool verify = false;
  uint8_t* v_ids = nullptr;
  const uint8_t* v_expect = nullptr;
  uint8_t* v_ok = nullptr;
  uint64_t* v_nbad = nullptr;
  // a batch of file segments (hbx_seg_submit_device): entry f is the next
  // segment of segs[f], file bytes [seg_off[f], seg_off[f] + len); K2 is the
  // segment form, K4 is skipped, and the collect adds seg_off to the cuts
  std::vector<hbx_seg*> segs;
  std::vector<uint64_t> seg_off;
  std::vector<uint8_t> seg_final;
  // submitted with an ID set (hbx_submit_device_dd, hbx_seg_submit_device_dd): K9 marks its result slots
  // when it is finalized, dd_seq-th of the context's marks; the flags go to
  // fresh_out[out_base[f] + q] at the collect
  hbx_idset* set = nullptr;
  uint8_t* fresh_out = nullptr;
  uint64_t dd_seq = 0;
  // submitted with expected chains (hbx_submit_device_match, hbx_store_paths_match): K12 compares each
  // file's result slots with its expected chain when the batch is finalized.  h_exp is the copy made at
  // submit (n + 1 running counts | the IDs), fetched into d_exp for K12; the records go to match_out[f] at the
  // collect.  verdict_only: the caller gave no chunk arrays, and only [rl.cid, rl.total) is pushed
  PinBuf h_exp;
  DevBuf d_exp;
  size_t exp_ids_at = 0, exp_bytes = 0;  // (exp_bytes: a multiple of 16)
  hbx_chain_match* match_out = nullptr;
  bool verdict_only = false;
  // K1 start | K1 end | K2r end | plan+K3 end (first) | results ready | K2 end (lean marks)
  hipEvent_t ev[6] = {};
  void release() {
    for (DevBuf* d : {&d_meta, &d_res, &d_run, &d_fresh, &d_fcnt, &d_exp}) d->release();
    h_meta.release();
    h_res.release();
    h_exp.release();
    for (auto& e : ev)
      if (e) (void)hipEventDestroy(e);
  }
};

}  // namespace

constexpr uint32_t kK3TimeRing = 4096;  // hbx_ctx::h_k3t slots (2 x u64 each)
constexpr int kDoneRing = 16;         // hbx_ctx::order_free: completion events of the latest K3 launches

struct hbx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;   // scan stream: input copies, K1, K2 (and hbx_block_id)
  hipStream_t cstream = nullptr;  // cut stream: K2 (after its batch's K1 on the scan stream)
  hipStream_t hstream = nullptr;  // hash stream: chain plan, K3
  hipStream_t rstream = nullptr;  // result stream: K4 + result D2H of batches whose chains are done
  hipEvent_t producer = nullptr;  // hbx_after_stream: the caller's stream, waited for on the scan stream
  std::mutex mu;
  std::string err;
  // K1 tile length in 64 KiB iterations; 0 = per batch (k1_tile_iters):
  // about two tiles per CU (four up to 4 GiB), 16..256.  At 8 GiB batches
  // that is 256 (fewer halo primes and, beside K3, fewer, longer K1
  // workgroups: 2,139-2,146 vs 2,088-2,108 GiB/s for 64); a 1 GiB batch gets
  // 16 so that its K1 spreads evenly over the CUs K3 leaves
  uint32_t tile_iters = 0;
  uint32_t join_lag = 1;      // hbx_set_join_lag
  // where and when K2c plans run follows from the join lag (plan_mode_of)
  bool preplanned = false;    // the plan of launch `launches` is enqueued (mode 2)
  std::vector<Batch*> pre_nb; // the batches whose chains that plan adds
  // K3 period (hbx_set_k3_period): one K3 launch every `k3_period` submits,
  // with `k3_period` x the slice per chain, joining every batch old enough:
  // the launch's fixed start-up and tail are paid once per period (small
  // per-GPU batches, the N = 8 share of configs[2]).  k3_tick counts submits.
  uint32_t k3_period = 1;
  uint64_t k3_tick = 0;
  uint32_t k4_window = 1024;  // K4's LDS window of ids (HBX_K4_WINDOW, 1..1024: tests)
  int k2_own = -1;            // ensure_cut_stream: -1 = by join lag (HBX_K2_STREAM for A/B)
  uint32_t md5_wgs = 256;     // K3 grid: one 256-thread workgroup per CU (set from the device)
  // K3P: a producer wave per MD5 wave (HBX_K3_PROD=0 for the self-staging K3,
  // A/B): 1,435 vs 1,586 cycles per block inside the bench schedule, +1.7 %
  // (200 steps) and +2.9 % at 8 files per GPU (profiles/r05f)
  uint32_t k3_prod = 1;
  // K3P producer register sets in flight: 3 (a stage more of memory latency
  // hidden) 2,297-2,318 vs 2,286-2,308 GiB/s in three alternating pairs at 64
  // files, equal at 8 (profiles/r05af); HBX_K3_PSETS=2 for A/B
  uint32_t k3_psets = 3;
  uint32_t k3_spin = 0;
  // full-slice chains ordered by data address in plan_addr granules of
  // 2^plan_addr_shift bytes (plan_bin; HBX_PLAN_ADDR=0..512, 0 = by count
  // only as before round 6; HBX_PLAN_ADDR_SHIFT=20..40)
  uint32_t plan_addr = 512, plan_addr_shift = 29;
  // K1 launched with its batch's ev[0]/ev[1] as hipExtLaunchKernel start/stop
  // events instead of marker packets around it (HBX_K1_EXT=0: markers)
  uint32_t k1_ext = 1;
  uint32_t k1_dma4 = 1;  // K1's four LDS-DMA pieces in one statement (HBX_K1_DMA4=0: one per piece)
  // K1's first two DMA iterations issued before the halo's loads (HBX_K1_EARLY=0:
  // after the prime); one memory round trip per tile fewer in principle,
  // neutral in measurement (64 files 2,328/2,329 vs 2,337/2,351, 8 files
  // 2,075/2,082 vs 2,041/2,062 GiB/s, profiles/r06u)
  uint32_t k1_early = 1;
  // at join lag 2, preplan on the cut stream (mode 3; HBX_PLAN_CUT=0: mode 1,
  // the plan on the hash stream): +2.7 % with K3P (profiles/r05e)
  // 2 (default): at lag 3 and 4 too, off the scan loop (8 files per GPU, K3
  // period 4: 2,075-2,079 vs 2,031-2,049 GiB/s, profiles/r05l); 1: lag 2 only
  uint32_t plan_cut = 2;
  // the batch meta reaches the device by hbx_meta_fetch, a kernel on the scan
  // stream, instead of an SDMA copy (HBX_META_KERNEL=0 for A/B)
  uint32_t meta_kernel = 1;
  // round 6: the meta copy inside the K1 gate kernel (hbx_k1_gate_meta), one
  // scan-stream kernel fewer per step (HBX_GATE_META=0: separate kernels)
  uint32_t gate_meta = 1;
  // a finished batch's results reach the host by hbx_result_push, a kernel
  // on the result stream, instead of an SDMA copy (HBX_D2H_KERNEL=0 for A/B):
  // the copy call held the host ~7 ms once per ~16 submits after a drain
  // (profiles/r05az: 8-file 20-step window 1,395 -> 1,994-2,033 GiB/s)
  uint32_t d2h_kernel = 64;  // workgroups (0 = SDMA copy)
  // K1's LDS image transposed per 1 KiB: its per-lane reads become
  // conflict-free (SQ_LDS_BANK_CONFLICT 1.0e8 -> 0 per launch), K1 beside K3
  // 3.26 -> 3.19 ms per 8 GiB (profiles/r05ab); HBX_K1_SWZ=0 for the old image
  uint32_t k1_swz = 1;
  // K3Q: items per group (parts of each slice, handed out through a queue;
  // 0 = off, K3P's static groups; HBX_K3_ITEMS for A/B)
  uint32_t k3_items = 0;
  PinBuf h_err;  // K3Q: set by a wave that gave up waiting for an item (never expected)
  uint32_t md5_slice = 16384; // K3 time slice: full MD5 blocks per chain per launch (0 = unlimited)
  // K1 gate (hbx_k1_gate): a batch's K1 waits until every workgroup of the K3
  // launch of the same submit has been dispatched.  k3_started counts K3
  // workgroups on the device; k3_dispatched is the host's running total.
  uint32_t k1_gate = 1;
  // Lean marks (HBX_LEAN_MARKS=0 for A/B): every event record or zero-fill
  // between two kernels of one stream costs ~5 us of dispatch, and the scan
  // stream's gate -> K1 -> K2 -> K2r -> plan is one of the step's two
  // equal-length loops.  With them K1 and K2 are timed by the
  // batch's own ev[0] | ev[1] | ev[5], K2 zeroes K2r's counter, the plan's
  // timing end event is what K3 waits on, and the plan bins are zeroed
  // after each plan (off the loop) instead of before it.
  uint32_t lean_marks = 1;  // 0 off (the old schedule, A/B), 1 on
  hipStream_t plan_zeroed_on = nullptr;  // stream whose last op leaves d_plan zeroed (lean)
  TimedLaunch plan_timer[3];             // lean: the plan's timing pair, queued once K3 waits on it
  bool plan_timer_set[3] = {false, false, false};
  hipEvent_t plan_wait[3] = {nullptr, nullptr, nullptr};  // what K3 of launch j%3 waits on
  // lean: hbx_input_after_oldest's wait (for K3 launch input_wait_L), enqueued
  // on the scan stream only just before the next thing that could touch the
  // old input (flush_input_wait), i.e. after the plan instead of before it
  bool input_wait_pending = false;
  uint64_t input_wait_L = 0;
  // the launch the latest hbx_input_after_oldest ordered input behind
  // (hbx_input_fence hands it to a caller's stream); unset once known complete
  bool input_fence_set = false;
  uint64_t input_fence_L = 0;
  DevBuf d_gate;
  uint32_t k3_dispatched = 0;
  // K3 launch times measured on the device (no timing events on the hash
  // stream, which carries only K3 and its completion event): K3's first
  // workgroup and its last wave stamp s_memrealtime into slot (launch %
  // kK3TimeRing) of this pinned ring; tickets from d_gate[0] (workgroups
  // started) and d_gate[1] (waves ended).  Harvested once a launch is known
  // complete (k3_done_upto: launches [0, k3_done_upto) are).
  PinBuf h_k3t;
  PinBuf h_probe;  // hbx_set_k3_probe: per-wave times of the latest K3 launch (hbx_k3_wave_times)
  uint32_t k3_waves = 0;
  std::deque<uint64_t> k3_open;
  uint64_t k3_done_upto = 0;
  float stage_ms[5] = {0, 0, 0, 0, 0};

  // host-side plan scratch
  std::vector<uint64_t> h_slice_base;
  std::vector<uint4> h_tiles;

  // K1 -> K2 slice summaries, two slots used by alternate batches: K1 of
  // batch i+1 (scan stream) overlaps K2 of batch i (cut stream)
  DevBuf d_ssum[2];
  int ssum_slot = 0;
  hipEvent_t ssum_free[2] = {nullptr, nullptr};  // recorded after the K2 that last read the slot
  bool ssum_used[2] = {false, false};
  // hbx_k1_summaries: the slot the latest synchronous batch's K1 wrote (-1: none, or overwritten since) and
  // its slices; the per-file bases are still h_slice_base
  int k1_sum_slot = -1;
  uint64_t k1_sum_slices = 0;
  // K3 launch orders (triple-buffered by launch index % 3): plan j (scan
  // stream) writes order[j%3] from order[(j-1)%3]; K3 j (hash stream) reads it
  DevBuf d_order[3], d_octl[3], d_q[3];  // (+ K3Q's item queue per slot)
  hipEvent_t plan_done[3] = {nullptr, nullptr, nullptr};   // plan j%3 written
  // completion of K3 launch L: order_free[L % kDoneRing] (recorded again by
  // launch L + kDoneRing).  The plan of launch j waits for launch j - 3, the
  // last reader of its order slot; hbx_input_after_oldest for the launch that
  // finished the oldest batch, which with a K3 period or a long lead is
  // several launches back (with 3 events it fell back to the newest launch,
  // serializing the next K1 behind the running K3: 8 files per GPU at K3
  // period 8 and lead 11, 1,579 vs 2,079 GiB/s, profiles/r05n)
  hipEvent_t order_free[kDoneRing] = {};
  uint64_t launches = 0;    // K3 launches planned so far
  uint32_t last_budget = 0; // budget of the last planned launch
  DevBuf d_stage;           // host-input arena
  DevBuf d_msg;             // hbx_block_id message
  DevBuf d_plan;            // chain planner: global bin counts + cursors
  DevBuf d_vdesc, d_vlinks, d_vout, d_vexp, d_zeros;  // hbx_verify_blocks*
  DevBuf d_zblk, d_zinfo, d_zoff, d_zlen, d_zout, d_zimg;  // hbx_deflate_blocks*
  DevBuf d_idesc, d_ires;                                  // hbx_inflate_blocks_device
  DevBuf d_sreg, d_sstart, d_sres, d_sscratch, d_smeta;    // its split path (K8s)
  // hbx_restore_*: staged input (two windows), inflate slots, the gathered
  // image / the local copy (diff), the piece table, the diff word; the pinned
  // staging and output of two windows; the stream the next window is filled on
  DevBuf d_rin[2], d_rslots, d_rimg, d_rpiece, d_rword;
  DevBuf d_rretry;  // hbx_restore_files_*: max_block slots of the streams that outgrew their size hint
  // the latest hbx_restore_files_* call: staged windows, K11 passes, streams inflated again
  uint64_t many_windows = 0, many_passes = 0, many_retries = 0;
  PinBuf h_rin[2], h_rout[2];
  hipStream_t fstream = nullptr;
  // host ms of the latest hbx_restore_* call per phase, each ending on a
  // synchronization: input staging, inflate, VerifyBlock beside K10, copy-out
  double restore_ms[4] = {0, 0, 0, 0};
  uint64_t k8_split_streams = 0, k8_split_fallbacks = 0;   // (hbx_knobs: how often the split path resolved)
  // SDMA engines warmed at context creation (warm_sdma_engines): H2D and D2H
  // engine masks, and the milliseconds this context spent on it (0 once the
  // process has done it for the device)
  uint32_t sdma_h2d = 0, sdma_d2h = 0;
  double sdma_warm_ms = 0.0;
  // hbx_host_call_max: the longest host time of one H2D copy call and of one
  // batch submit since the last reset (hbx_memcpy_h2d_async, the disk path's
  // copies, submit_batch), ms
  double max_copy_ms = 0.0, max_submit_ms = 0.0;
  uint32_t sdma_warm = 1;
  PinBuf h_read[2];         // hbx_store_paths: pinned landing slots for file reads
  PinBuf h_zstage;          // hbx_store_paths_z: compressed streams of one batch (synchronous form)
  // hbx_store_paths_z: compression stages in flight, each on its own stream
  static constexpr int kZStages = 2;  // three measured slower (16.1 vs 21.8 GiB/s, profiles/r02i_zpipe)
  struct ZStage {
    DevBuf blk, info, off, len, img, out;
    PinBuf desc, lens, stage;
    hipEvent_t done = nullptr;
    hipStream_t stream = nullptr;  // one per stage: one job's K7 overlaps another's copy-back
  } zs[kZStages];
  hipEvent_t h2d_done[2] = {nullptr, nullptr};  // slot's H2D copy has completed
  std::vector<DevBuf> d_ring;  // hbx_store_paths: device arenas of the batches in flight
  double io_s[3] = {0, 0, 0};  // hbx_store_paths: reading files | waiting for an arena | waiting for a copy

  // hbx_seg_*: open segmented files, their carry words (8 bytes each, handed
  // out from 4 KiB device blocks and reused: closing a file frees no device
  // memory, which would wait for the device), the final chain block's
  // message and the stream its block id is computed on (created by the first
  // hbx_seg_open; beside, never inside, the pipeline's four streams)
  // hbx_idset_*: the context's ID sets; the scratch slot table of the pipeline's
  // marks (one at a time: they all run on the result stream); marks are
  // numbered at submit (dd_submitted) and must be enqueued in that order
  // (dd_marked, finalize_batch)
  std::vector<hbx_idset*> idsets;
  std::vector<hbx_index*> indexes;  // hbx_index_open: the context's index handles
  DevBuf d_dscratch;
  uint64_t dd_submitted = 0, dd_marked = 0;
  uint64_t match_push_bytes = 0;  // hbx_knobs: bytes of the result pushes of match batches
  DevBuf d_mt[5], d_mtout;        // hbx_match_chains: the two ID lists, their firsts, the cut ends; the records
  // hbx_locate_ids: the pool's IDs, cut ends and firsts, the wanted IDs, the slot table, the records + hit count
  DevBuf d_lc[6];
  // hbx_datfile_*: K14's two position lists + counts, the sorted positions, the records; the image and the
  // two pinned staging buffers of the path variants; K14's workgroup count (0 = by size; HBX_K14_WGS: tests);
  // the latest call's windows and streams inflated again
  DevBuf d_df[3], d_dfimg;
  PinBuf h_dfstage[2];
  uint32_t k14_wgs = 0;
  uint64_t dat_windows = 0, dat_retries = 0;
  // hbx_block_graph (bg_layout names the buffers); K15's workgroup cap (0 = by size; HBX_K15_WGS: tests)
  DevBuf d_bg[16];
  uint32_t k15_wgs = 0;
  // hbx_datfile_compact_* (the kCp* enum names the buffers); K16's tile in bytes (HBX_K16_TILE: tests)
  DevBuf d_cp[12];
  uint32_t k16_tile = hbxk::kTile;
  std::vector<hbx_seg*> segs_open;
  std::vector<DevBuf> seg_words;
  std::vector<uint64_t*> seg_words_free;
  hipStream_t sstream = nullptr;
  DevBuf d_segmsg;

  std::deque<Batch*> pending;  // submitted, not yet collected (FIFO)
  std::vector<Batch*> pool;
  // A HIP error after a batch's device work was enqueued leaves chains of it
  // in the carried order lists: the context refuses further pipelined work
  // (HBX_ERR_STATE) and the batch's buffers are parked here, never reused,
  // until hbx_ctx_destroy.
  bool broken = false;
  std::vector<Batch*> parked;
  // Batches whose chains are cut (K2r enqueued) but not yet in a plan, oldest
  // first: a batch joins the K3 launch issued `join_lag` submits after its
  // own (or a wait's drain), so K3 launch j never waits for batch j's own
  // scan and the scan side runs join_lag steps ahead of the hash stream.
  std::deque<Batch*> unjoined;
  std::vector<TimedLaunch> open_t;
  std::vector<hipEvent_t> ev_pool;
  double tot_ms[5] = {0, 0, 0, 0, 0};
  uint64_t tot_n[5] = {0, 0, 0, 0, 0};

  int fail(int code, const std::string& m) {
    err = m;
    return code;
  }
  int hip(hipError_t e, const char* what) {
    if (e == hipSuccess) return HBX_OK;
    err = std::string(what) + ": " + hipGetErrorString(e);
    return HBX_ERR_HIP;
  }
  hipEvent_t event() {
    if (!ev_pool.empty()) {
      hipEvent_t e = ev_pool.back();
      ev_pool.pop_back();
      return e;
    }
    hipEvent_t e = nullptr;
    return hipEventCreate(&e) == hipSuccess ? e : nullptr;
  }
};

#define HBX_TRY(ctx, expr)                                \
  do {                                                    \
    int _rc = (ctx)->hip((expr), #expr);                  \
    if (_rc != HBX_OK) return _rc;                        \
  } while (0)

namespace {

inline uint64_t max_chunks(uint64_t len) { return len / HBX_MIN_BLOCK_SIZE + 1; }

// Grow a buffer the streams may still be using: drain both streams first.  A
// drain stalls the pipeline, so growth is geometric (and hbx_reserve sizes
// everything up front for a known workload).
int ensure_shared(hbx_ctx* c, DevBuf& b, size_t n) {
  if (n <= b.cap && b.p) return HBX_OK;
  HBX_TRY(c, hipStreamSynchronize(c->stream));
  HBX_TRY(c, hipStreamSynchronize(c->cstream));
  HBX_TRY(c, hipStreamSynchronize(c->hstream));
  HBX_TRY(c, hipStreamSynchronize(c->rstream));
  HBX_TRY(c, b.ensure(b.p ? std::max(n, b.cap + b.cap / 2) : n));
  return HBX_OK;
}

// Bracket one launch with an event pair for hbx_stage_totals.
struct StageTimer {
  hbx_ctx* c;
  hipStream_t s;
  TimedLaunch t;
  // on = false: a no-op (the caller times the launch with events it records anyway)
  StageTimer(hbx_ctx* ctx, hipStream_t st, int stage, bool on = true) : c(ctx), s(st) {
    t.stage = stage;
    t.a = on ? c->event() : nullptr;
    t.b = on ? c->event() : nullptr;
    if (t.a) (void)hipEventRecord(t.a, s);
  }
  ~StageTimer() {
    if (!t.a && !t.b) return;
    if (t.a && t.b && hipEventRecord(t.b, s) == hipSuccess) {
      c->open_t.push_back(t);
    } else {
      if (t.a) c->ev_pool.push_back(t.a);
      if (t.b) c->ev_pool.push_back(t.b);
    }
  }
};

// Timed launches of one stage run on one stream, so they complete in order:
// once one is still running, the later ones of its stage are not queried (a
// host far ahead of the device keeps many open, and each query costs µs).
void harvest_timings(hbx_ctx* c) {
  size_t keep = 0;
  bool open[5] = {false, false, false, false, false};
  for (size_t i = 0; i < c->open_t.size(); i++) {
    TimedLaunch& t = c->open_t[i];
    float ms = 0.f;
    bool done = false;
    if (!open[t.stage]) {
      done = hipEventQuery(t.b) == hipSuccess && hipEventElapsedTime(&ms, t.a, t.b) == hipSuccess;
      open[t.stage] = !done;
    }
    if (done) {
      c->tot_ms[t.stage] += ms;
      c->tot_n[t.stage] += 1;
      if (t.owned) {
        c->ev_pool.push_back(t.a);
        c->ev_pool.push_back(t.b);
      }
    } else {
      c->open_t[keep++] = t;
    }
  }
  c->open_t.resize(keep);
}


// Add the device-measured K3 launches known complete to the totals.
void harvest_k3(hbx_ctx* c) {
  while (!c->k3_open.empty() && c->k3_open.front() < c->k3_done_upto) {
    const volatile uint64_t* t = c->h_k3t.as<uint64_t>() + 2 * (c->k3_open.front() % kK3TimeRing);
    const uint64_t a = t[0], e = t[1];
    if (a && e >= a) {
      c->tot_ms[3] += (double)(e - a) * 1e-5;  // s_memrealtime: 100 MHz
      c->tot_n[3] += 1;
    }
    c->k3_open.pop_front();
  }
}

Batch* acquire_batch(hbx_ctx* c) {
  Batch* b;
  if (!c->pool.empty()) {
    b = c->pool.back();
    c->pool.pop_back();
  } else {
    b = new Batch();
    for (auto& e : b->ev) {
      if (hipEventCreate(&e) != hipSuccess) {
        b->release();
        delete b;
        return nullptr;
      }
    }
  }
  b->n = b->caps = 0;
  b->need = 1;
  b->done = 0;
  b->rl = ResLayout{};  // a verify batch keeps its ids at offset 0 of d_res
  b->joined = false;
  b->ev3 = false;
  b->k2_ev5 = false;
  b->final_launch = 0;
  b->finalized = false;
  b->cut_ends = nullptr;
  b->ids = nullptr;
  b->sums = nullptr;
  b->verify = false;
  b->v_ids = nullptr;
  b->v_expect = nullptr;
  b->v_ok = nullptr;
  b->v_nbad = nullptr;
  b->segs.clear();
  b->seg_off.clear();
  b->seg_final.clear();
  b->set = nullptr;
  b->fresh_out = nullptr;
  b->dd_seq = 0;
  b->match_out = nullptr;
  b->verdict_only = false;
  return b;
}

static double ms_since(std::chrono::steady_clock::time_point t) {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

// HBX_TRACE_SLOW_SUBMIT=<ms>: a submit slower than that prints where its host
// time went (diagnostics for one-off host stalls; off by default).
struct SlowSubmit {
  double limit_ms = -1.0;
  double fin[3] = {0, 0, 0};  // finalize: K4 (+ its timing events), D2H copy, completion record
  std::chrono::steady_clock::time_point t[12];
  SlowSubmit() {
    if (const char* v = std::getenv("HBX_TRACE_SLOW_SUBMIT")) limit_ms = std::atof(v);
  }
  void mark(int i) {
    if (limit_ms >= 0) t[i] = std::chrono::steady_clock::now();
  }
  void report(uint64_t launches) {
    if (limit_ms < 0) return;
    auto ms = [&](int a, int b) { return std::chrono::duration<double, std::milli>(t[b] - t[a]).count(); };
    if (ms(0, 5) < limit_ms) return;
    std::fprintf(stderr, "hbx slow submit (launch %llu): %.3f ms = setup %.3f, buffers %.3f, md5_step %.3f, preplan %.3f, scan %.3f"
                 " | md5_launch: entry %.3f, k3 launch %.3f, record %.3f, finalize %.3f\n",
                 (unsigned long long)launches, ms(0, 5), ms(0, 1), ms(1, 2), ms(2, 3), ms(3, 4), ms(4, 5),
                 ms(2, 6), ms(6, 7), ms(7, 8), ms(8, 9));
    std::fprintf(stderr, "  finalize: k4 %.3f, d2h %.3f, record %.3f\n", fin[0], fin[1], fin[2]);
  }
  void clear() {
    if (limit_ms < 0) return;
    for (int i = 6; i < 10; i++) t[i] = t[0];
    fin[0] = fin[1] = fin[2] = 0;
  }
  // one host call outside submit (e.g. the H2D copy call), reported alone
  void call(const char* what, std::chrono::steady_clock::time_point a, uint64_t launches) {
    if (limit_ms < 0) return;
    const double d = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - a).count();
    if (d >= limit_ms)
      std::fprintf(stderr, "hbx slow call (launch %llu): %s %.3f ms\n", (unsigned long long)launches, what, d);
  }
  void lap(int k, std::chrono::steady_clock::time_point& a) {
    if (limit_ms < 0) return;
    const auto b = std::chrono::steady_clock::now();
    fin[k] += std::chrono::duration<double, std::milli>(b - a).count();
    a = b;
  }
};
// Per thread (advisor r05): a context's calls are serialised by its own lock
// only, so contexts submitting from different threads must not share it; two
// contexts on one thread never overlap.
static thread_local SlowSubmit g_slow;

// K4 + D2H of one batch whose chains are all hashed, on the result stream
// (after the finalizing K3's completion event), so the hash stream goes straight on with the next plan
// and K3 launch.
int finalize_batch(hbx_ctx* c, Batch* b) {
  hipStream_t s = c->rstream;
  b->finalized = true;
  if (b->verify) {
    if (b->n) HBX_TRY(c, hipMemcpyAsync(b->h_res.p, b->d_res.p, b->n * 16, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipEventRecord(b->ev[4], s));
    return HBX_OK;
  }
  auto lap = std::chrono::steady_clock::now();
  if (b->n) {
    const uint64_t n = b->n;
    const uint64_t* d_cb = b->d_meta.as<uint64_t>() + 3 * n;
    // (a segment's content id is the whole file's: the collect of the final
    // segment computes it, collect_segments)
    if (b->segs.empty()) {
      StageTimer t(c, s, 4);
      hipLaunchKernelGGL(hbx_k4_content_id, dim3((uint32_t)n), dim3(64), 0, s,
                         (uint32_t)n, d_cb, b->count_d(), b->ids_d(), reinterpret_cast<uint32_t*>(b->res(b->rl.cid)),
                         reinterpret_cast<int32_t*>(b->res(b->rl.ctype)), c->k4_window);
    }
    HBX_TRY(c, hipGetLastError());
    if (b->set) {
      // K9: one mark over the batch's result slots.  "First in submit order"
      // holds because every mark is enqueued here, on the one result stream,
      // in the order of the submits (md5_launch holds a batch back until the
      // older batches with a set are marked)
      if (b->dd_seq != c->dd_marked) return c->fail(HBX_ERR_STATE, "ID set marks out of submit order (internal)");
      c->dd_marked++;
      const hbxd::Ids in{reinterpret_cast<const uint4*>(b->res(b->rl.ids)), d_cb, b->count_d(), (uint32_t)b->caps,
                         (uint32_t)n};
      HBX_TRY(c, hbxd::mark(s, b->set->view(), in, c->d_dscratch.as<uint32_t>(), b->res(b->rl.fresh)));
    }
    // what the push brings back: everything, or a verdict-only batch's per-file sections
    size_t push_at = 0;
    if (b->match_out) {
      // K12: every chain of the batch is hashed here, whatever the slice, join lag and K3 period.  The
      // expected chains come over PCIe from the batch's pinned copy by hbx_meta_fetch (system-scope reads:
      // the staging is reused by later batches), a kernel and not an SDMA copy between two kernels of this
      // stream
      const uint32_t e16 = (uint32_t)(b->exp_bytes / 16);
      hipLaunchKernelGGL(hbx_meta_fetch, dim3(std::min<uint32_t>(64, (e16 + 255) / 256)), dim3(256), 0, s,
                         static_cast<const uint4*>(b->h_exp.p), b->d_exp.as<uint4>(), e16);
      HBX_TRY(c, hipGetLastError());
      const uint8_t* he = b->d_exp.as<uint8_t>();
      const hbxm::Args ma{hbxd::Ids{reinterpret_cast<const uint4*>(b->res(b->rl.ids)), d_cb, b->count_d(),
                                    (uint32_t)b->caps, (uint32_t)n},
                          b->cuts_d(), reinterpret_cast<const uint64_t*>(he),
                          reinterpret_cast<const uint4*>(he + b->exp_ids_at),
                          reinterpret_cast<uint4*>(b->res(b->rl.match))};
      HBX_TRY(c, hbxm::match(s, ma));
      if (b->verdict_only) push_at = b->rl.cid;
      c->match_push_bytes += b->rl.total - push_at;
    }
    g_slow.lap(0, lap);
    // one copy for every result (5 copies before: each a dispatch on this stream)
    if (c->d2h_kernel && b->rl.total % 16 == 0) {
      const uint64_t n16 = (b->rl.total - push_at) / 16;
      hipLaunchKernelGGL(hbx_result_push, dim3((uint32_t)std::min<uint64_t>(c->d2h_kernel, (n16 + 255) / 256)),
                         dim3(256), 0, s, reinterpret_cast<const uint4*>(b->res(push_at)),
                         reinterpret_cast<uint4*>(b->h_res.as<uint8_t>() + push_at), n16);
      HBX_TRY(c, hipGetLastError());
    } else {
      HBX_TRY(c, hipMemcpyAsync(b->h_res.as<uint8_t>() + push_at, b->res(push_at), b->rl.total - push_at,
                                hipMemcpyDeviceToHost, s));
    }
    g_slow.lap(1, lap);
  }
  HBX_TRY(c, hipEventRecord(b->ev[4], s));
  g_slow.lap(2, lap);
  return HBX_OK;
}

// One MD5 launch: plan (carried chains + the new batch's chunks, if any) and
// K3 with `budget` blocks per chain.  Afterwards every pending batch has had
// one more launch; those whose chains are now guaranteed complete are
// finalized.  A budget of kBudgetAll completes every chain in flight.
// Plan launch j = c->launches on the scan stream: order[j%3] from
// order[(j-1)%3] (advanced by the budget of launch j-1) plus the fresh chains
// of batch nb (if any).  Needs no result of any K3 launch.
int ensure_plan_buffers(hbx_ctx* c, uint64_t extra);

// Where and when plans run (the plan of launch j+1 adds batch j+1-lag).
// * lag 1, mode 0: submit j+1 enqueues it on the scan stream, after batch j's
//   K1 (and K2), whose chains it adds.
// * lag 2, mode 1: the batch was cut a step earlier, so the plan can go on the
//   hash stream between K3 j and K3 j+1, off the scan stream (which then
//   carries only the K1 gate and K1).  Costs ~0.06 ms of dispatch gaps per
//   step on the hash stream.
// * lag >= 3, mode 2 (preplan): submit j enqueues it on the scan stream right
//   after launching K3 j and BEFORE batch j's K1; the batch it adds (j-2 or
//   older) was cut during the previous step, so the plan never waits for a K2
//   and the hash stream carries nothing but K3 launches.  At lag 2 the same
//   schedule would make K1 j wait for K2 of batch j-1 (measured 1,575 GiB/s at
//   8 files per GPU, vs 1,890 for mode 1).
// * lag 2, mode 3 (preplan on the cut stream, c->plan_cut): the same preplan
//   as mode 2, but on the cut stream, right behind batch j-1's K2 and K2r
//   (whose chains it adds) and before batch j's K2: neither the scan stream
//   nor the hash stream waits for it, and the hash stream carries nothing but
//   K3 launches.
// The blocks per chain of one K3 launch for a per-submit slice `budget`.
uint32_t launch_budget(const hbx_ctx* c, uint32_t budget) {
  if (budget == kBudgetAll || c->k3_period <= 1) return budget;
  return (uint32_t)std::min<uint64_t>((uint64_t)budget * c->k3_period, kBudgetAll - 1);
}

int plan_mode_of(const hbx_ctx* c) {
  if ((c->join_lag == 2 ? c->plan_cut : c->plan_cut > 1 && c->join_lag > 2) && c->cstream != c->stream) return 3;
  return c->join_lag >= 3 ? 2 : c->join_lag == 2 ? 1 : 0;
}
hipStream_t plan_stream(const hbx_ctx* c) {
  const int m = plan_mode_of(c);
  return m == 1 ? c->hstream : m == 3 ? c->cstream : c->stream;
}

// K2 + K2r get a stream of their own once the join lag allows it (or
// HBX_K2_STREAM=1): K1 of the next batch then no longer queues behind this
// batch's K2 (at 8 files per GPU, 1,578 -> 1,825 GiB/s).  At lag 1 the plan
// needs K2r right away, and a fourth stream of ours shares one of the
// GPU_MAX_HW_QUEUES = 4 hardware queues (measured +0.2 ms hash-stream gap),
// so K2 stays on the scan stream.  Created once; never dropped.
int ensure_cut_stream(hbx_ctx* c) {
  const bool want = c->k2_own < 0 ? c->join_lag >= 2 : c->k2_own > 0;
  if (!want || c->cstream != c->stream || c->hstream == c->stream) return HBX_OK;
  hipStream_t s = nullptr;
  HBX_TRY(c, hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  c->cstream = s;
  return HBX_OK;
}

// Enqueue a deferred hbx_input_after_oldest wait on the scan stream (nothing
// once the host has seen that launch complete).  Called before anything that
// may read or write a caller's input on the scan stream, and before any K3
// launch could record the launch's completion slot again.
int flush_input_wait(hbx_ctx* c) {
  if (!c->input_wait_pending) return HBX_OK;
  c->input_wait_pending = false;
  hipEvent_t e = c->order_free[c->input_wait_L % kDoneRing];
  if (hipEventQuery(e) == hipSuccess) return HBX_OK;
  HBX_TRY(c, hipStreamWaitEvent(c->stream, e, 0));
  return HBX_OK;
}

int plan_launch(hbx_ctx* c, const std::vector<Batch*>& nbs, uint32_t budget) {
  hipStream_t s = plan_stream(c);
  const int slot = (int)(c->launches % 3), ps = (int)((c->launches + 2) % 3);
  int rc = ensure_plan_buffers(c, 0);  // nb (if any) is already in pending
  if (rc) return rc;
  // the K3 launch that read this slot three launches ago must be done (lean:
  // no wait enqueued once the host has seen it complete, the usual case)
  if (c->launches >= 3 && c->hstream != s) {
    hipEvent_t e = c->order_free[(c->launches - 3) % kDoneRing];
    if (!(c->lean_marks && hipEventQuery(e) == hipSuccess)) HBX_TRY(c, hipStreamWaitEvent(s, e, 0));
  }
  // carried chains exist only while an older batch is unfinalized (a batch
  // is finalized once every chain of it is hashed); without one the previous
  // list is not read at all (hbx_reserve may have reallocated it)
  bool has_prev = false;
  for (Batch* b : c->pending)
    if (b->joined && !b->finalized && std::find(nbs.begin(), nbs.end(), b) == nbs.end()) has_prev = true;
  has_prev = has_prev && c->launches > 0;
  FreshSet fs{};
  for (Batch* nb : nbs) {
    if (!nb->n) continue;
    fs.f[fs.k] = nb->d_fresh.as<OrderEntry>();
    fs.n[fs.k] = nb->d_fcnt.as<uint32_t>();
    fs.k++;
    // the joining batch's chains come from K2r (cut stream) or K6p (scan stream)
    if (!(s == c->stream && c->cstream == s)) HBX_TRY(c, hipStreamWaitEvent(s, nb->ev[2], 0));
  }
  // the plan stream changed (hbx_set_join_lag): the trailing bin fill queued on
  // the old one must not land inside this plan
  if (c->plan_zeroed_on && c->plan_zeroed_on != s) {
    HBX_TRY(c, hipStreamSynchronize(c->plan_zeroed_on));
    c->plan_zeroed_on = nullptr;
  }
  if (c->lean_marks) {
    TimedLaunch t;
    t.stage = 2;
    t.a = c->event();
    t.b = c->event();
    if (t.a && t.b) {
      HBX_TRY(c, hipEventRecord(t.a, s));
      if (c->plan_zeroed_on != s) HBX_TRY(c, hipMemsetAsync(c->d_plan.p, 0, 2 * kPlanBins * sizeof(uint32_t), s));
      for (uint32_t phase = 0; phase < 2; phase++)
        hipLaunchKernelGGL(hbx_k2c_plan, dim3(kPlanGroups), dim3(kPlanThreads), 0, s,
                           has_prev ? c->d_order[ps].as<OrderEntry>() : nullptr,
                           has_prev ? c->d_octl[ps].as<uint32_t>() : nullptr, c->last_budget,
                           fs, budget, c->d_order[slot].as<OrderEntry>(), c->d_octl[slot].as<uint32_t>(),
                           c->d_plan.as<uint32_t>(), phase | (c->plan_addr << 8) | (c->plan_addr_shift << 24));
      HBX_TRY(c, hipGetLastError());
      HBX_TRY(c, hipEventRecord(t.b, s));
      // K3 waits on the timing end itself; the pair is queued for harvest
      // only once that wait is enqueued (md5_launch), so the pool cannot hand
      // t.b out again before
      if (c->plan_timer_set[slot]) c->open_t.push_back(c->plan_timer[slot]);  // (not reached: K3 took it)
      c->plan_timer[slot] = t;
      c->plan_timer_set[slot] = true;
      c->plan_wait[slot] = t.b;
      // the bins for the next plan, while K3 is being dispatched
      c->plan_zeroed_on = nullptr;
      HBX_TRY(c, hipMemsetAsync(c->d_plan.p, 0, 2 * kPlanBins * sizeof(uint32_t), s));
      c->plan_zeroed_on = s;
      return flush_input_wait(c);
    }
    if (t.a) c->ev_pool.push_back(t.a);
    if (t.b) c->ev_pool.push_back(t.b);
  }
  c->plan_zeroed_on = nullptr;
  {
    StageTimer t(c, s, 2);
    HBX_TRY(c, hipMemsetAsync(c->d_plan.p, 0, 2 * kPlanBins * sizeof(uint32_t), s));
    for (uint32_t phase = 0; phase < 2; phase++)
      hipLaunchKernelGGL(hbx_k2c_plan, dim3(kPlanGroups), dim3(kPlanThreads), 0, s,
                         has_prev ? c->d_order[ps].as<OrderEntry>() : nullptr,
                         has_prev ? c->d_octl[ps].as<uint32_t>() : nullptr, c->last_budget,
                         fs, budget, c->d_order[slot].as<OrderEntry>(), c->d_octl[slot].as<uint32_t>(),
                         c->d_plan.as<uint32_t>(), phase | (c->plan_addr << 8) | (c->plan_addr_shift << 24));
  }
  HBX_TRY(c, hipGetLastError());
  HBX_TRY(c, hipEventRecord(c->plan_done[slot], s));
  c->plan_wait[slot] = c->plan_done[slot];
  return flush_input_wait(c);
}

// One MD5 launch (planned by plan_launch just before): K3 with `budget`
// blocks per chain.  Afterwards every pending batch has had one more launch;
// those whose chains are now guaranteed complete are finalized.  A budget of
// kBudgetAll completes every chain in flight.
int md5_launch(hbx_ctx* c, const std::vector<Batch*>& nbs, uint32_t budget) {
  if (int frc = flush_input_wait(c)) return frc;  // (a preplanned launch comes without a plan_launch)
  hipStream_t s = c->hstream;
  const int slot = (int)(c->launches % 3);
  if (s != plan_stream(c)) HBX_TRY(c, hipStreamWaitEvent(s, c->plan_wait[slot], 0));
  if (c->plan_timer_set[slot]) {  // lean marks: the wait is enqueued, the pair may be harvested
    c->open_t.push_back(c->plan_timer[slot]);
    c->plan_timer_set[slot] = false;
  }
  // the device-timing slot of this launch (its previous user, kK3TimeRing
  // launches back, must have been harvested)
  const uint64_t L = c->launches;
  if (!c->k3_open.empty() && c->k3_open.front() + kK3TimeRing <= L) {
    HBX_TRY(c, hipStreamSynchronize(s));
    c->k3_done_upto = L;
    harvest_k3(c);
  }
  uint64_t* tslot = nullptr;
  if (c->h_k3t.p) {
    tslot = c->h_k3t.as<uint64_t>() + 2 * (L % kK3TimeRing);
    tslot[0] = tslot[1] = 0;
    c->k3_open.push_back(L);
  }
  const uint32_t waves = c->md5_wgs * (kK3Threads / 64);
  g_slow.mark(6);
  const uint32_t parts = c->k3_items && budget != kBudgetAll && budget >= 64u * c->k3_items ? c->k3_items : 0u;
  if (parts && !c->h_err.p) {
    HBX_TRY(c, c->h_err.ensure(64));
    std::memset(c->h_err.p, 0, 64);
  }
  if (parts)
    hipLaunchKernelGGL(hbx_k3q_block_md5, dim3(c->md5_wgs), dim3(kK3PThreads), 0, s,
                       c->d_order[slot].as<OrderEntry>(), static_cast<const uint32_t*>(c->d_octl[slot].as<uint32_t>()),
                       budget, c->d_gate.as<uint32_t>(), c->k3_dispatched, c->k3_waves + waves - 1u, tslot,
                       c->h_probe.p ? c->h_probe.as<uint64_t>() : nullptr, c->d_octl[slot].as<uint32_t>() + 1,
                       c->d_q[slot].as<uint64_t>(), (uint32_t)(L + 1), parts, c->h_err.as<uint32_t>());
  else if (c->k3_prod)
    hipLaunchKernelGGL(hbx_k3p_block_md5, dim3(c->md5_wgs), dim3(kK3PThreads), 0, s,
                       c->d_order[slot].as<OrderEntry>(), static_cast<const uint32_t*>(c->d_octl[slot].as<uint32_t>()),
                       budget, c->d_gate.as<uint32_t>(), c->k3_dispatched, c->k3_waves + waves - 1u, tslot,
                       c->h_probe.p ? c->h_probe.as<uint64_t>() : nullptr, c->k3_psets | (c->k3_spin ? 0x100u : 0u));
  else
    hipLaunchKernelGGL(hbx_k3_block_md5, dim3(c->md5_wgs), dim3(kK3Threads), 0, s,
                       c->d_order[slot].as<OrderEntry>(), static_cast<const uint32_t*>(c->d_octl[slot].as<uint32_t>()),
                       budget, c->d_gate.as<uint32_t>(), c->k3_dispatched, c->k3_waves + waves - 1u, tslot,
                       c->h_probe.p ? c->h_probe.as<uint64_t>() : nullptr);
  g_slow.mark(7);
  HBX_TRY(c, hipGetLastError());
  c->k3_dispatched += c->md5_wgs;
  c->k3_waves += waves;
  c->last_budget = budget;  // what the next plan advances this list by
  // the launch's one completion event: the plan three launches on waits for
  // it, and so does the result stream for the batches it completes
  HBX_TRY(c, hipEventRecord(c->order_free[L % kDoneRing], s));
  g_slow.mark(8);
  c->launches++;
  if (budget == kBudgetAll)  // per-batch stage times of a synchronous batch (hbx_stage_times)
    for (Batch* nb : nbs) {
      HBX_TRY(c, hipEventRecord(nb->ev[3], s));
      nb->ev3 = true;
    }
  bool forked = false;
  bool dd_older = false;  // an older batch with an ID set is not finalized yet: its mark goes first
  for (Batch* b : c->pending) {
    if (b->finalized) continue;
    if (!b->joined) {
      dd_older = dd_older || b->set;
      continue;
    }
    b->done++;
    const bool hashed = budget == kBudgetAll || b->done >= b->need;
    if (b->set && (dd_older || !hashed)) {  // (held back: finalized by the launch that finalizes the older ones)
      dd_older = true;
      continue;
    }
    if (hashed) {
      if (!forked && c->rstream != s) {  // the result stream picks up after this K3
        HBX_TRY(c, hipStreamWaitEvent(c->rstream, c->order_free[L % kDoneRing], 0));
        forked = true;
      }
      b->final_launch = L;
      int rc = finalize_batch(c, b);
      if (rc) return rc;
    }
  }
  g_slow.mark(9);
  return HBX_OK;
}

// One pipeline step on the hash side: launch j = plan (the carried chains +
// the chains of every unjoined batch at least join_lag submits old) then K3
// with `budget` blocks per chain.  Issued by every submit BEFORE the new
// batch's own scan is enqueued (with a K3 period P, by every P-th submit
// only, with P x the slice), and by wait_oldest (`drain`, with kBudgetAll:
// the oldest unjoined batch joins whatever its age).  Nothing is launched
// when no chain is in flight.
// The unjoined batches (oldest first) that join a launch whose FIFO holds
// `size` of them, `older` submits from now: those join_lag or more old then.
uint32_t joiners(const hbx_ctx* c, uint64_t older, bool drain) {
  const uint64_t size = c->unjoined.size();
  uint64_t k = size + older >= c->join_lag ? size + older + 1 - c->join_lag : 0;
  if (drain) k = std::max<uint64_t>(k, 1);
  return (uint32_t)std::min<uint64_t>(std::min<uint64_t>(k, size), kMaxFresh);
}

int md5_step(hbx_ctx* c, uint32_t budget, bool drain = false) {
  if (!drain && c->k3_period > 1 && c->k3_tick++ % c->k3_period != 0) return HBX_OK;  // not this submit
  budget = launch_budget(c, budget);
  if (c->preplanned) {  // planned one launch ahead (mode 2): any budget may run it
    std::vector<Batch*> nbs;
    nbs.swap(c->pre_nb);
    c->preplanned = false;
    for (Batch* nb : nbs) nb->joined = true;
    return md5_launch(c, nbs, budget);
  }
  std::vector<Batch*> nbs(c->unjoined.begin(), c->unjoined.begin() + joiners(c, 0, drain));
  bool live = !nbs.empty();
  for (Batch* b : c->pending)
    if (b->joined && !b->finalized) live = true;
  if (!live) return HBX_OK;
  int rc = plan_launch(c, nbs, budget);
  if (rc) return rc;
  for (Batch* nb : nbs) {
    nb->joined = true;
    c->unjoined.pop_front();
  }
  return md5_launch(c, nbs, budget);
}

// Modes 2 and 3: enqueue the plan of the NEXT launch now, before the
// submitting batch's own K1.  It adds the unjoined batches that are join_lag
// submits old at the next submit (the submitting batch is not in the FIFO
// yet, hence `older` 1).  With a K3 period, only when the next submit
// launches.  Nothing is planned when no chain would be in flight; the next
// submit then plans inline.
int preplan(hbx_ctx* c, uint32_t budget) {
  const int mode = plan_mode_of(c);
  if ((mode != 2 && mode != 3) || c->preplanned || c->hstream == c->stream) return HBX_OK;
  if (c->k3_period > 1 && c->k3_tick % c->k3_period != 0) return HBX_OK;
  budget = launch_budget(c, budget);
  std::vector<Batch*> nbs(c->unjoined.begin(), c->unjoined.begin() + joiners(c, 1, false));
  bool live = !nbs.empty();
  for (Batch* b : c->pending)
    if (b->joined && !b->finalized) live = true;
  if (!live) return HBX_OK;
  int rc = ensure_plan_buffers(c, 0);  // its slot's last reader (K3 three launches back) is waited for
  if (!rc) rc = plan_launch(c, nbs, budget);
  if (rc) return rc;
  for (size_t i = 0; i < nbs.size(); i++) c->unjoined.pop_front();
  c->pre_nb = std::move(nbs);
  c->preplanned = true;
  return HBX_OK;
}

// The order-list and planner buffers the next launch's plan writes, with
// `extra` chains joining the unfinalized batches' chains.  Only the slot the
// plan writes may grow: growing reallocates without copying, and the slot of
// the previous launch holds the carried chains the plan reads.
int ensure_plan_buffers(hbx_ctx* c, uint64_t extra) {
  if (c->preplanned) return HBX_OK;  // that slot holds the next launch's list already
  uint64_t bound = 64 + extra;  // entries <= chains of the unfinalized batches
  for (Batch* b : c->pending)
    if (!b->finalized) bound += b->caps;
  const int slot = (int)(c->launches % 3);
  int rc = ensure_shared(c, c->d_order[slot], bound * sizeof(OrderEntry));
  if (!rc) rc = ensure_shared(c, c->d_octl[slot], 256);
  if (!rc) rc = ensure_shared(c, c->d_q[slot], (bound / 64 + 2) * 8 * 8);  // groups x up to 8 parts
  if (!rc) rc = ensure_shared(c, c->d_plan, 2 * kPlanBins * sizeof(uint32_t));
  return rc;
}

// A submit failed.  Before any device work of `b` was enqueued (`enqueued`
// false) the batch simply returns to the pool.  After it, the batch leaves
// the FIFO (so no later wait collects it into caller memory that may be
// freed), the streams drain, its buffers are parked (its chains may still be
// in the carried order lists) and the context refuses further pipelined work.
int submit_abort(hbx_ctx* c, Batch* b, int rc, bool enqueued) {
  const std::string keep = c->err;
  for (auto it = c->unjoined.begin(); it != c->unjoined.end(); ++it)
    if (*it == b) {
      c->unjoined.erase(it);
      break;
    }
  for (auto it = c->pending.begin(); it != c->pending.end(); ++it)
    if (*it == b) {
      c->pending.erase(it);
      break;
    }
  if (!enqueued) {
    c->pool.push_back(b);
    return rc;
  }
  for (hipStream_t s : {c->stream, c->cstream, c->hstream, c->rstream})
    if (s) (void)hipStreamSynchronize(s);
  c->parked.push_back(b);
  c->broken = true;
  c->err = keep + " (context is unusable for pipelined work; destroy it)";
  return rc;
}

int submit_batch_launch(hbx_ctx* c, Batch* b, const void* d_arena, uint64_t n, const uint64_t* offs,
                        const uint64_t* lens, uint32_t budget, uint64_t slices, size_t meta_bytes, int slot);

// K1 tiles of one file of `iters` 64 KiB iterations: `tile` each.
// (Queuing each file's last eighth as 1 MiB tiles after the long ones, to
// round off K1's last pass over the CUs K3 leaves free, measured slower: K1
// 3.18 -> 3.33 ms beside K3 at 33 resident batches, from the extra halos and
// workgroups.)
void k1_tiles(hbx_ctx* c, uint32_t f, uint32_t iters, uint32_t tile) {
  for (uint32_t i = 0; i < iters; i += tile) c->h_tiles.push_back(make_uint4(f, i, std::min(tile, iters - i), 0u));
}

constexpr uint32_t kTileItersMin = 16, kTileItersMax = 256;

// K1 tile length for a batch of `total` iterations (c->tile_iters, or about
// two or four tiles per CU when that is 0)
uint32_t k1_tile_iters(const hbx_ctx* c, uint64_t total) {
  if (c->tile_iters) return c->tile_iters;
  // about two tiles per CU for large batches, four up to 4 GiB (65,536
  // iterations), 8/3 up to 2 GiB: the strong-scaling shares of configs[2]
  // (tools/gpu_tile_sweep.sh, profiles/r02n_tiles: 1 GiB 1,825 -> 1,948 GiB/s
  // with 16 instead of 32 iterations, 2 GiB 2,068 -> 2,147 with 32 instead of
  // 64; 4 GiB equal; 8 GiB 2,231 at 256 vs 2,205 at 128).  With the K3 period
  // (round 5) 1 GiB does best at 24 (2,141-2,150 vs 2,096-2,132 GiB/s at 16,
  // three alternating rounds, profiles/r05s) and 2 GiB at 48 (2,275 vs 2,254)
  const uint64_t num = total <= 32768ull ? 3ull : 1ull;
  const uint64_t den = total <= 32768ull ? 8ull : total <= 65536ull ? 4ull : 2ull;
  const uint64_t t = (total * num + den * c->md5_wgs - 1) / (den * c->md5_wgs);
  return (uint32_t)std::min<uint64_t>(kTileItersMax, std::max<uint64_t>(kTileItersMin, t));
}

inline uint64_t scan_iters(uint64_t N) {  // K1 iterations of a file (0: no split candidates)
  return N > 2ull * HBX_MIN_BLOCK_SIZE ? (N + HBX_MIN_BLOCK_SIZE - 1) / HBX_MIN_BLOCK_SIZE : 0;
}

// Plan + enqueue one device batch (K1, K2, first MD5 launch).  Results are
// collected by wait_oldest in submission order.  Every validation and
// allocation happens before the batch joins the FIFO; a failure after that
// removes it again (submit_abort), so a failed submit leaves no pending batch.
// The expected chains of a match batch (hbx_submit_device_match, hbx_store_paths_match): file f's chain is
// ids[16 first[f] .. 16 first[f + 1]) (validated by the caller: non-decreasing, each chain below 2^32
// IDs); out[f] receives its record at the collect.  verdict_only: no chunk arrays, out_base and caps NULL.
struct MatchIn {
  const uint64_t* first = nullptr;
  const uint8_t* ids = nullptr;
  hbx_chain_match* out = nullptr;
  bool verdict_only = false;
};
int submit_batch_timed(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                       const uint64_t* lens, uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base,
                       const uint64_t* caps, hbx_file_summary* sums, uint32_t budget, hbx_seg* const* segs,
                       const uint64_t* seg_offs, hbx_idset* set, uint8_t* fresh, const MatchIn* mi);
}  // namespace
// hbx_reserve with the context's lock already held (defined beside it, inside
// the C-ABI block; not exported)
extern "C" __attribute__((visibility("hidden"))) int reserve_locked(hbx_ctx* c, uint32_t batches, uint64_t files,
                                                                    uint64_t bytes, bool dedup = false,
                                                                    bool match = false, uint64_t match_ids = 0);
namespace {
int submit_batch(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                 const uint64_t* lens, uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base,
                 const uint64_t* caps, hbx_file_summary* sums, uint32_t budget, hbx_seg* const* segs = nullptr,
                 const uint64_t* seg_offs = nullptr, hbx_idset* set = nullptr, uint8_t* fresh = nullptr,
                 const MatchIn* mi = nullptr) {
  const auto t0 = std::chrono::steady_clock::now();
  const int rc = submit_batch_timed(c, d_arena, n, offs, lens, cut_ends, ids, out_base, caps, sums, budget, segs,
                                    seg_offs, set, fresh, mi);
  c->max_submit_ms = std::max(c->max_submit_ms, ms_since(t0));
  return rc;
}
int submit_batch_timed(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                       const uint64_t* lens, uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base,
                       const uint64_t* caps, hbx_file_summary* sums, uint32_t budget, hbx_seg* const* segs,
                       const uint64_t* seg_offs, hbx_idset* set, uint8_t* fresh, const MatchIn* mi) {
  g_slow.mark(0);
  g_slow.clear();
  c->k1_sum_slot = -1;  // h_slice_base and a summary slot are about to be rewritten
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  if (n > 0xFFFFFFFFull) return c->fail(HBX_ERR_ARG, "too many files");
  for (uint64_t f = 0; f < n; f++)
    if (offs[f] % HBX_ARENA_ALIGN) return c->fail(HBX_ERR_ARG, "file offset not 16-byte aligned");
  Batch* b = acquire_batch(c);
  if (!b) return c->fail(HBX_ERR_HIP, "cannot create batch events");
  b->n = n;
  b->cut_ends = cut_ends;
  b->ids = ids;
  b->sums = sums;
  if (out_base) {
    b->out_base.assign(out_base, out_base + n);
    b->capv.assign(caps, caps + n);
  } else {  // verdict-only: nothing is scattered; the result slots are sized by hbx_max_chunks(len)
    b->out_base.assign(n, 0);
    b->capv.resize(n);
    for (uint64_t f = 0; f < n; f++) b->capv[f] = max_chunks(lens[f]);
  }
  b->cut_base.resize(n);
  if (segs) {  // (validated by the caller: seg_submit)
    b->segs.assign(segs, segs + n);
    b->seg_off.assign(seg_offs, seg_offs + n);
    b->seg_final.resize(n);
    for (uint64_t f = 0; f < n; f++) b->seg_final[f] = seg_offs[f] + lens[f] == segs[f]->file_len;
  }
  c->h_slice_base.resize(n);
  c->h_tiles.clear();
  uint64_t slices = 0, tcaps = 0, longest = 0, total_iters = 0;
  for (uint64_t f = 0; f < n; f++) {
    const uint64_t iters = scan_iters(lens[f]);
    if (iters > 0xFFFFFFFFull) {
      c->pool.push_back(b);
      return c->fail(HBX_ERR_ARG, "file too large");
    }
    total_iters += iters;
  }
  const uint32_t tile = k1_tile_iters(c, total_iters);
  for (uint64_t f = 0; f < n; f++) {
    const uint64_t N = lens[f];
    longest = std::max(longest, N);
    c->h_slice_base[f] = slices;
    b->cut_base[f] = tcaps;
    tcaps += max_chunks(N);
    if (const uint64_t iters = scan_iters(N)) {  // only files with split candidates scan
      slices += (N + kSlice - 1) / kSlice;
      k1_tiles(c, (uint32_t)f, (uint32_t)iters, tile);
    }
  }
  b->caps = tcaps;
  if (set && tcaps > hbxd::kMaxMark) {
    c->pool.push_back(b);
    return c->fail(HBX_ERR_ARG, "too many chunks in one batch for an ID set");
  }
  // launches this batch's chains need: a chunk is <= min(longest file, MAX)
  // bytes, i.e. <= nfull full message blocks, and each launch advances it by
  // slice_cnt(remaining, budget) blocks (the part short of a slice first, then
  // full slices): ceil(blocks / budget) launches either way
  const uint64_t nfull = (std::min<uint64_t>(longest, HBX_MAX_BLOCK_SIZE) + 8) >> 6;
  const uint64_t lb = launch_budget(c, budget);  // a K3 period multiplies the slice
  b->need = budget == kBudgetAll ? 1u : (uint32_t)std::max<uint64_t>(1, (nfull + lb - 1) / lb);
  const uint64_t nt = c->h_tiles.size();
  // meta block: off | len | slice_base | cut_base | tiles, and for segments
  // | carry address | seg_off | final | first start (written by K2)
  const size_t meta_bytes = n * 8 * 4 + nt * sizeof(uint4) + (segs ? n * 8 * 4 : 0);
  const int slot = c->ssum_slot;
  g_slow.mark(1);
  if (n) {  // every allocation first: the batch is not in the FIFO yet
    int rc = HBX_OK;
    b->rl = res_layout(n, tcaps, set != nullptr, mi != nullptr);
    if (mi) {  // firsts (rebased to 0) | IDs, copied now: the caller's arrays are free on return
      const uint64_t e0 = mi->first[0], ne = mi->first[n] - e0;
      b->exp_ids_at = al256((n + 1) * 8);
      b->exp_bytes = b->exp_ids_at + 16 * ne;
      for (hipError_t e : {b->h_exp.ensure(b->exp_bytes), b->d_exp.ensure(b->exp_bytes)})
        if (e != hipSuccess && !rc) rc = c->hip(e, "batch buffers (expected chains)");
      if (!rc) {
        uint64_t* hf = b->h_exp.as<uint64_t>();
        for (uint64_t f = 0; f <= n; f++) hf[f] = mi->first[f] - e0;
        std::memset(hf + n + 1, 0, b->exp_ids_at - (n + 1) * 8);
        if (ne) std::memcpy(b->h_exp.as<uint8_t>() + b->exp_ids_at, mi->ids + 16 * e0, 16 * ne);
        b->match_out = mi->out;
        b->verdict_only = mi->verdict_only;
      }
    }
    for (hipError_t e : {b->h_meta.ensure(meta_bytes), b->d_meta.ensure(meta_bytes), b->d_res.ensure(b->rl.total),
                         b->d_run.ensure(tcaps * sizeof(Chain)),
                         b->d_fresh.ensure(tcaps * sizeof(OrderEntry)), b->d_fcnt.ensure(256),
                         b->h_res.ensure(b->rl.total)})
      if (e != hipSuccess && !rc) rc = c->hip(e, "batch buffers");
    if (!rc) rc = ensure_shared(c, c->d_ssum[slot], (slices + 1) * sizeof(uint2));  // +1: dummy slot
    if (!rc) rc = ensure_plan_buffers(c, tcaps);
    if (!rc && set) rc = ensure_shared(c, c->d_dscratch, hbxd::table_slots(tcaps) * sizeof(uint32_t));
    if (rc) return submit_abort(c, b, rc, false);
    if (set) {  // (a batch without files has no chunk to mark)
      b->set = set;
      b->fresh_out = fresh;
      b->dd_seq = c->dd_submitted++;
      set->inflight++;
    }
  }
  c->pending.push_back(b);
  g_slow.mark(2);
  const int rc = submit_batch_launch(c, b, d_arena, n, offs, lens, budget, slices, meta_bytes, slot);
  g_slow.mark(5);
  g_slow.report(c->launches);
  return rc ? submit_abort(c, b, rc, true) : HBX_OK;
}

int submit_batch_launch(hbx_ctx* c, Batch* b, const void* d_arena, uint64_t n, const uint64_t* offs,
                        const uint64_t* lens, uint32_t budget, uint64_t slices, size_t meta_bytes, int slot) {
  hipStream_t s = c->stream;
  // launch j hashes the chains in flight plus the previous batch's; it is
  // enqueued (plan on the scan stream) before this batch's K1, so it never
  // waits for this batch's scan
  const uint64_t launches0 = c->launches;
  int rc = md5_step(c, budget);
  g_slow.mark(3);
  if (!rc) rc = preplan(c, budget);
  g_slow.mark(4);
  if (rc) return rc;
  const bool gate = c->k1_gate && c->launches != launches0 && c->hstream != s;
  if (n == 0) {
    for (int i = 0; i < 4; i++) HBX_TRY(c, hipEventRecord(b->ev[i], s));
    b->finalized = true;
    HBX_TRY(c, hipEventRecord(b->ev[4], s));
    return HBX_OK;
  }
  const uint64_t nt = c->h_tiles.size();
  uint64_t* hm = b->h_meta.as<uint64_t>();
  std::memcpy(hm, offs, n * 8);
  std::memcpy(hm + n, lens, n * 8);
  std::memcpy(hm + 2 * n, c->h_slice_base.data(), n * 8);
  std::memcpy(hm + 3 * n, b->cut_base.data(), n * 8);
  if (nt) std::memcpy(hm + 4 * n, c->h_tiles.data(), nt * sizeof(uint4));
  const bool seg = !b->segs.empty();
  const size_t seg_at = 4 * n + 2 * nt;  // in u64 units
  if (seg)
    for (uint64_t f = 0; f < n; f++) {
      hm[seg_at + f] = reinterpret_cast<uint64_t>(b->segs[f]->d_carry);
      hm[seg_at + n + f] = b->seg_off[f];
      hm[seg_at + 2 * n + f] = b->seg_final[f];
      hm[seg_at + 3 * n + f] = 0;
    }
  c->ssum_slot ^= 1;
  DevBuf& ssum = c->d_ssum[slot];

  if (int frc = flush_input_wait(c)) return frc;  // (no launch this submit: nothing flushed it yet)
  const bool gate_meta = c->meta_kernel && c->gate_meta && c->k1_gate;
  if (gate_meta) {  // one kernel: the meta copy, then (if a K3 launch was issued) the gate
    if (c->ssum_used[slot] && c->cstream != s) HBX_TRY(c, hipStreamWaitEvent(s, c->ssum_free[slot], 0));
    const uint32_t n16 = (uint32_t)(meta_bytes / 16);
    hipLaunchKernelGGL(hbx_k1_gate_meta, dim3(std::min<uint32_t>(16, (n16 + 255) / 256)), dim3(256), 0, s,
                       static_cast<const uint32_t*>(c->d_gate.as<uint32_t>()), c->k3_dispatched, 1000000u,
                       gate ? 1u : 0u, static_cast<const uint4*>(b->h_meta.p), b->d_meta.as<uint4>(), n16);
    HBX_TRY(c, hipGetLastError());
  } else if (c->meta_kernel) {  // meta_bytes is a multiple of 16
    const uint32_t n16 = (uint32_t)(meta_bytes / 16);
    hipLaunchKernelGGL(hbx_meta_fetch, dim3(std::min<uint32_t>(64, (n16 + 255) / 256)), dim3(256), 0, s,
                       static_cast<const uint4*>(b->h_meta.p), b->d_meta.as<uint4>(), n16);
    HBX_TRY(c, hipGetLastError());
  } else {
    HBX_TRY(c, hipMemcpyAsync(b->d_meta.p, hm, meta_bytes, hipMemcpyHostToDevice, s));
  }
  const uint64_t* d_off = b->d_meta.as<uint64_t>();
  const uint64_t* d_len = d_off + n;
  const uint64_t* d_sb = d_off + 2 * n;
  const uint64_t* d_cb = d_off + 3 * n;
  const uint4* d_tiles = reinterpret_cast<const uint4*>(d_off + 4 * n);
  const uint8_t* arena = static_cast<const uint8_t*>(d_arena);

  // the K2 that last read this summary slot (two batches back) must be done
  if (!gate_meta && c->ssum_used[slot] && c->cstream != s) HBX_TRY(c, hipStreamWaitEvent(s, c->ssum_free[slot], 0));
  if (gate && !gate_meta) {  // K1 after the K3 launch above has all its workgroups on CUs (<= 10 ms)
    hipLaunchKernelGGL(hbx_k1_gate, dim3(1), dim3(64), 0, s, static_cast<const uint32_t*>(c->d_gate.as<uint32_t>()),
                       c->k3_dispatched, 1000000u);
    HBX_TRY(c, hipGetLastError());
  }
  // lean marks with K2 on this stream: ev[0] | K1 | ev[1] | K2 | ev[5] | K2r
  // (| ev[2] unless the plan follows on this stream), one record between
  // kernels, the batch's events doubling as K1's
  // and K2's timers (the batch outlives their harvest: it is reused only
  // after its collect, long after both completed)
  hipStream_t s2 = c->cstream;
  const bool lean = c->lean_marks && s2 == s;
  if (nt && c->k1_ext) {
    // round 6: ev[0] / ev[1] bound to K1's own dispatch (hipExtLaunchKernel's
    // start and stop events), not recorded as marker packets around it: at
    // join lag >= 2 K1 had four (ev[0], its timer's pair, ev[1]) between the
    // scan loop's kernels.  They double as K1's timer and K2's dependency.
    hipExtLaunchKernelGGL(hbx_k1_digest_scan_dma, dim3((uint32_t)nt), dim3(kK1Threads), 0, s, b->ev[0], b->ev[1], 0,
                          arena, d_off, d_len, d_sb, d_tiles, ssum.as<uint2>(), slices,
                          c->k1_swz | (c->k1_dma4 ? 0u : 2u) | (c->k1_early ? 0u : 4u));
    HBX_TRY(c, hipGetLastError());
    c->open_t.push_back(TimedLaunch{b->ev[0], b->ev[1], 0, false});
  } else {
    HBX_TRY(c, hipEventRecord(b->ev[0], s));
    if (nt) {
      StageTimer t(c, s, 0, !lean);
      hipLaunchKernelGGL(hbx_k1_digest_scan_dma, dim3((uint32_t)nt), dim3(kK1Threads), 0, s, arena, d_off, d_len,
                         d_sb, d_tiles, ssum.as<uint2>(), slices, c->k1_swz | (c->k1_dma4 ? 0u : 2u) | (c->k1_early ? 0u : 4u));
    }
    HBX_TRY(c, hipGetLastError());
    HBX_TRY(c, hipEventRecord(b->ev[1], s));
    if (lean && nt) c->open_t.push_back(TimedLaunch{b->ev[0], b->ev[1], 0, false});
  }
  // K2 on the cut stream: the scan stream goes straight on with the next
  // batch's K1 (into the other summary slot)
  if (s2 != s) HBX_TRY(c, hipStreamWaitEvent(s2, b->ev[1], 0));
  // Segments: the carry of a file goes from this K2 to the K2 of its next
  // segment through device memory, so the two must run in submit order.
  // They do: every K2 of a context is launched here, on the cut stream, and
  // that stream changes only while no batch is pending (ensure_cut_stream).
  uint64_t* d_first = seg ? b->d_meta.as<uint64_t>() + seg_at + 3 * n : nullptr;
  {
    StageTimer t(c, s2, 1, !lean);
    if (seg)
      hipLaunchKernelGGL(hbx_k2s_cut_chain_seg, dim3((uint32_t)n), dim3(64), 0, s2, arena, d_off, d_len,
                         d_sb, ssum.as<uint2>(), d_cb, b->cuts_d(), b->count_d(),
                         lean ? b->d_fcnt.as<uint32_t>() : nullptr, d_off + seg_at, d_off + seg_at + n,
                         d_off + seg_at + 2 * n, d_first);
    else
      hipLaunchKernelGGL(hbx_k2_cut_chain, dim3((uint32_t)n), dim3(64), 0, s2, arena, d_off, d_len,
                         d_sb, ssum.as<uint2>(), d_cb, b->cuts_d(), b->count_d(),
                         lean ? b->d_fcnt.as<uint32_t>() : nullptr);
  }
  HBX_TRY(c, hipGetLastError());
  if (lean) {  // the summary slot's next writer (K1, this stream) follows in order: no ssum_free
    HBX_TRY(c, hipEventRecord(b->ev[5], s2));
    c->open_t.push_back(TimedLaunch{b->ev[1], b->ev[5], 1, false});
  } else {
    HBX_TRY(c, hipEventRecord(c->ssum_free[slot], s2));
  }
  c->ssum_used[slot] = true;
  // K2r: the batch's chains and their order entries (lean: K2 zeroed the count)
  if (!lean) HBX_TRY(c, hipMemsetAsync(b->d_fcnt.p, 0, 4, s2));
  hipLaunchKernelGGL(hbx_k2r_new_chains, dim3((uint32_t)((n * kPlanLanesPerFile + 255) / 256)), dim3(256), 0, s2,
                     (uint32_t)n, arena, d_off, d_cb, b->cuts_d(), b->count_d(), b->ids_d(), b->d_run.as<Chain>(), b->d_fresh.as<OrderEntry>(),
                     b->d_fcnt.as<uint32_t>(), static_cast<const uint64_t*>(d_first));
  HBX_TRY(c, hipGetLastError());
  // the plan this batch joins waits for ev[2] (plan_launch), so with a join
  // lag of 2 the scan stream never waits for this K2.  Lean marks with the
  // plan on this same stream: no one waits, and ev[5] already marks K2's end
  if (lean && plan_stream(c) == s2) {
    b->k2_ev5 = true;
  } else {
    HBX_TRY(c, hipEventRecord(b->ev[2], s2));
  }
  c->unjoined.push_back(b);
  return HBX_OK;
}

int submit_verify_launch(hbx_ctx* c, Batch* b, const uint8_t* arena, uint64_t n, const uint64_t* offs,
                         const uint64_t* lens, const uint8_t* links, const uint64_t* link_base,
                         const uint32_t* n_links, uint64_t nlinks_total, size_t meta_bytes, uint32_t budget);

// Plan + enqueue a VerifyBlock batch: K6p hashes each block's prefix blocks
// and turns the rest into K3 chains, which then share the time-sliced MD5
// pipeline (and the FIFO of hbx_wait) with the chunking batches.
int submit_verify(hbx_ctx* c, const uint8_t* arena, uint64_t n, const uint64_t* offs, const uint64_t* lens,
                  const uint8_t* links, const uint64_t* link_base, const uint32_t* n_links, uint8_t* ids,
                  const uint8_t* expect, uint8_t* ok, uint64_t* n_bad, uint32_t budget) {
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  if (n > 0xFFFFFFFFull) return c->fail(HBX_ERR_ARG, "too many blocks");
  uint64_t nlinks_total = 0, longest = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t nl = n_links ? n_links[i] : 0u;
    if (nl && (!links || !link_base)) return c->fail(HBX_ERR_ARG, "links missing");
    if (lens[i] + 8ull + 16ull * nl + 128ull > 0xFFFFFFFFull) return c->fail(HBX_ERR_ARG, "block too large");
    if (nl) nlinks_total = std::max(nlinks_total, link_base[i] + nl);
    longest = std::max<uint64_t>(longest, (lens[i] + 8ull + 16ull * nl) >> 6);
  }
  Batch* b = acquire_batch(c);
  if (!b) return c->fail(HBX_ERR_HIP, "cannot create batch events");
  b->verify = true;
  b->n = n;
  b->caps = n;
  b->v_ids = ids;
  b->v_expect = expect;
  b->v_ok = ok;
  b->v_nbad = n_bad;
  const uint64_t lb = launch_budget(c, budget);
  b->need = budget == kBudgetAll ? 1u : (uint32_t)std::max<uint64_t>(1, (longest + lb - 1) / lb);
  // meta block: descriptors | links
  const size_t meta_bytes = n * sizeof(VerifyDesc) + 16 * nlinks_total;
  if (n) {  // every allocation first: the batch is not in the FIFO yet
    int rc = HBX_OK;
    for (hipError_t e : {b->h_meta.ensure(meta_bytes), b->d_meta.ensure(meta_bytes), b->d_res.ensure(n * 16),
                         b->d_run.ensure(n * sizeof(Chain)), b->d_fresh.ensure(n * sizeof(OrderEntry)),
                         b->d_fcnt.ensure(256), b->h_res.ensure(n * 16)})
      if (e != hipSuccess && !rc) rc = c->hip(e, "verify batch buffers");
    if (!rc) rc = ensure_plan_buffers(c, n);
    if (rc) return submit_abort(c, b, rc, false);
  }
  c->pending.push_back(b);
  const int rc = submit_verify_launch(c, b, arena, n, offs, lens, links, link_base, n_links, nlinks_total,
                                      meta_bytes, budget);
  return rc ? submit_abort(c, b, rc, true) : HBX_OK;
}

int submit_verify_launch(hbx_ctx* c, Batch* b, const uint8_t* arena, uint64_t n, const uint64_t* offs,
                         const uint64_t* lens, const uint8_t* links, const uint64_t* link_base,
                         const uint32_t* n_links, uint64_t nlinks_total, size_t meta_bytes, uint32_t budget) {
  hipStream_t s = c->stream;
  int rc = md5_step(c, budget);  // launch j first, as in submit_batch_launch
  if (!rc) rc = preplan(c, budget);
  if (!rc) rc = flush_input_wait(c);
  if (rc) return rc;
  if (n == 0) {
    for (int i = 0; i < 4; i++) HBX_TRY(c, hipEventRecord(b->ev[i], s));
    b->finalized = true;
    HBX_TRY(c, hipEventRecord(b->ev[4], s));
    return HBX_OK;
  }
  VerifyDesc* hd = b->h_meta.as<VerifyDesc>();
  uint8_t* dl = b->d_meta.as<uint8_t>() + n * sizeof(VerifyDesc);
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t nl = n_links ? n_links[i] : 0u;
    hd[i].src = reinterpret_cast<uint64_t>(arena + offs[i]);
    hd[i].links = reinterpret_cast<uint64_t>(dl + (nl ? 16 * link_base[i] : 0));
    hd[i].len = (uint32_t)lens[i];
    hd[i].n_links = nl;
    hd[i].pad = 0;
  }
  if (nlinks_total) std::memcpy(b->h_meta.as<uint8_t>() + n * sizeof(VerifyDesc), links, 16 * nlinks_total);
  HBX_TRY(c, hipEventRecord(b->ev[0], s));
  HBX_TRY(c, hipMemcpyAsync(b->d_meta.p, b->h_meta.p, meta_bytes, hipMemcpyHostToDevice, s));
  HBX_TRY(c, hipMemsetAsync(b->d_fcnt.p, 0, 4, s));
  HBX_TRY(c, hipEventRecord(b->ev[1], s));
  hipLaunchKernelGGL(hbx_k6p_verify_chains, dim3((uint32_t)((n + 255) / 256)), dim3(256), 0, s,
                     b->d_meta.as<VerifyDesc>(), (uint32_t)n, b->ids_d(), b->d_run.as<Chain>(),
                     b->d_fresh.as<OrderEntry>(), b->d_fcnt.as<uint32_t>());
  HBX_TRY(c, hipGetLastError());
  HBX_TRY(c, hipEventRecord(b->ev[2], s));
  c->unjoined.push_back(b);
  return HBX_OK;
}

// MD5(BE32(n_links) || links || BE32(len) || data) on stream `s`, the message
// staged in `buf` (HashboxBlock.HashData, block.go:96-111): hbx_block_id, and
// the FileChainBlock id of a segmented file.  Waits for `s` only.  A message
// of a block or more goes through hbx_k5r_md5_run, a shorter one through K5.
int block_id_on(hbx_ctx* c, hipStream_t s, DevBuf& buf, const uint8_t* links, uint32_t n_links,
                const uint8_t* data, uint64_t len, uint8_t out[16]) {
  const uint64_t n = 8 + 16ull * n_links + len;
  std::vector<uint8_t> msg(n);
  auto be32 = [](uint8_t* b, uint32_t v) {
    b[0] = (uint8_t)(v >> 24);
    b[1] = (uint8_t)(v >> 16);
    b[2] = (uint8_t)(v >> 8);
    b[3] = (uint8_t)v;
  };
  be32(msg.data(), n_links);
  if (n_links) std::memcpy(msg.data() + 4, links, 16ull * n_links);
  be32(msg.data() + 4 + 16ull * n_links, (uint32_t)len);
  if (len) std::memcpy(msg.data() + 8 + 16ull * n_links, data, len);
  HBX_TRY(c, buf.ensure(n + 16 + 128));  // (+128: hbx_k5r_md5_run reads up to 63 bytes past the message)
  uint8_t* dm = buf.as<uint8_t>();
  HBX_TRY(c, hipMemcpyAsync(dm + 16, msg.data(), n, hipMemcpyHostToDevice, s));
  if (n >= 64)
    hipLaunchKernelGGL(hbx_k5r_md5_run, dim3(1), dim3(64), 0, s, dm + 16, (uint32_t)n,
                       reinterpret_cast<uint32_t*>(dm));
  else
    hipLaunchKernelGGL(hbx_k5_md5_raw, dim3(1), dim3(64), 0, s, dm + 16, (uint32_t)n,
                       reinterpret_cast<uint32_t*>(dm));
  HBX_TRY(c, hipGetLastError());
  HBX_TRY(c, hipMemcpyAsync(out, dm, 16, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  return HBX_OK;
}

// entry.ContentType / ContentBlockID of a segmented file whose final segment
// has been collected (store.go:187-196), from the chunk ids gathered in its
// handle: one chunk = that chunk's id, more = the id of the FileChainBlock
// with the ids as links, hashed on the device (K5) on the segment stream,
// beside the batches still in flight.
int seg_file_summary(hbx_ctx* c, hbx_seg* h, hbx_file_summary* sum) {
  const uint64_t k = h->ids.size() / 16;
  std::memset(sum->content_id, 0, 16);
  sum->content_type = 0;
  if (k == 0) return HBX_OK;
  if (k == 1) {
    std::memcpy(sum->content_id, h->ids.data(), 16);
    sum->content_type = HBX_CONTENT_FILE_DATA;
    return HBX_OK;
  }
  // the block's data is 8 + 32k bytes behind BE32(len); the whole message
  // (16 + 48k bytes) must also fit the MD5 kernel's 32-bit length
  const uint64_t body = 8 + 32 * k;
  if (body > 0xFFFFFFFFull || 16 + 48 * k + 16 + 128 > 0xFFFFFFFFull)
    return c->fail(HBX_ERR_CAPACITY, "file has too many chunks for one FileChainBlock (" + std::to_string(k) + ")");
  std::vector<uint8_t> blk(body);
  uint64_t wrote = 0;
  if (hbx_chain_block_serialize(h->ids.data(), nullptr, (uint32_t)k, blk.data(), body, &wrote) != HBX_OK || wrote != body)
    return c->fail(HBX_ERR_STATE, "chain block serialization (internal)");
  int rc = block_id_on(c, c->sstream, c->d_segmsg, h->ids.data(), (uint32_t)k, blk.data(), body, sum->content_id);
  if (rc) return rc;
  sum->content_type = HBX_CONTENT_FILE_CHAIN;
  return HBX_OK;
}

// A collected batch of segments: cut ends become absolute file offsets, the
// chunk ids join their file's handle, and a final segment's summary carries
// the whole file's content type and id.
int collect_segments(hbx_ctx* c, Batch* b) {
  const ResLayout& rl = b->rl;
  const uint8_t* hr = b->h_res.as<uint8_t>();
  const uint32_t* counts = reinterpret_cast<const uint32_t*>(hr + rl.counts);
  const uint64_t* cuts = reinterpret_cast<const uint64_t*>(hr + rl.cuts);
  const uint8_t* hid = hr + rl.ids;
  int rc = HBX_OK;
  for (uint64_t f = 0; f < b->n; f++) {
    hbx_seg* h = b->segs[f];
    const uint64_t k = counts[f], ib = b->cut_base[f], so = b->seg_off[f];
    h->inflight--;
    h->ids.insert(h->ids.end(), hid + 16 * ib, hid + 16 * (ib + k));
    if (k) h->last_cut = so + cuts[ib + k - 1];
    if (h->keep_cuts)
      for (uint64_t i = 0; i < k; i++) h->cuts.push_back(so + cuts[ib + i]);
    hbx_file_summary sum{};
    sum.n_chunks = (uint32_t)k;
    if (b->seg_final[f]) {
      const int r2 = seg_file_summary(c, h, &sum);
      if (r2 && !rc) rc = r2;
    }
    if (b->sums) b->sums[f] = sum;
    if (k > b->capv[f]) {  // (not reached: the submit checked caps against hbx_max_chunks)
      rc = c->fail(HBX_ERR_CAPACITY, "output capacity too small for segment " + std::to_string(f));
      continue;
    }
    if (b->cut_ends)
      for (uint64_t i = 0; i < k; i++) b->cut_ends[b->out_base[f] + i] = so + cuts[ib + i];
    if (b->ids) std::memcpy(b->ids + 16 * b->out_base[f], hid + 16 * ib, k * 16);
    // (the set's inflight count is the batch's, not the segment's: collect_batch drops it once)
    if (b->set && b->fresh_out) std::memcpy(b->fresh_out + b->out_base[f], hr + rl.fresh + ib, k);
  }
  return rc;
}

// Scatter a collected batch's pinned results into the caller's arrays.
int collect_batch(hbx_ctx* c, Batch* b) {
  const uint64_t n = b->n;
  if (b->verify) {  // VerifyBlock: ids, and the comparison with the expected ids
    const uint8_t* hid = b->h_res.as<uint8_t>();
    if (b->v_ids && n) std::memcpy(b->v_ids, hid, n * 16);
    uint64_t bad = 0;
    if (b->v_expect) {
      for (uint64_t i = 0; i < n; i++) {
        const uint8_t good = std::memcmp(hid + 16 * i, b->v_expect + 16 * i, 16) == 0;
        if (b->v_ok) b->v_ok[i] = good;
        bad += good ? 0 : 1;
      }
    }
    if (b->v_nbad) *b->v_nbad = bad;
    return HBX_OK;
  }
  const ResLayout& rl = b->rl;
  const uint8_t* hr = b->h_res.as<uint8_t>();
  const uint32_t* counts = reinterpret_cast<const uint32_t*>(hr + rl.counts);
  const uint64_t* cuts = reinterpret_cast<const uint64_t*>(hr + rl.cuts);
  const uint8_t* hid = hr + rl.ids;
  const uint8_t* cid = hr + rl.cid;
  const int32_t* ctype = reinterpret_cast<const int32_t*>(hr + rl.ctype);
  int rc = b->segs.empty() ? HBX_OK : collect_segments(c, b);
  // (a verdict-only batch pushed [rl.cid, rl.total) only: the chunk count comes from the file's record)
  const hbx_chain_match* mt = b->match_out ? reinterpret_cast<const hbx_chain_match*>(hr + rl.match) : nullptr;
  for (uint64_t f = 0; f < n && b->segs.empty(); f++) {
    const uint64_t k = b->verdict_only ? mt[f].n_local : counts[f];
    const uint64_t ib = b->cut_base[f];
    if (mt) b->match_out[f] = mt[f];
    if (b->sums) {
      std::memcpy(b->sums[f].content_id, cid + 16 * f, 16);
      b->sums[f].content_type = ctype[f];
      b->sums[f].n_chunks = (uint32_t)k;
    }
    if (k > b->capv[f]) {
      rc = c->fail(HBX_ERR_CAPACITY, "output capacity too small for file " + std::to_string(f));
      continue;
    }
    if (b->cut_ends) std::memcpy(b->cut_ends + b->out_base[f], cuts + ib, k * 8);
    if (b->ids) std::memcpy(b->ids + 16 * b->out_base[f], hid + 16 * ib, k * 16);
    if (b->set && b->fresh_out) std::memcpy(b->fresh_out + b->out_base[f], hr + rl.fresh + ib, k);
  }
  if (b->set) b->set->inflight--;
  float ms = 0.f;
  // stage boundaries: K1 start | K1 end | K2 end | plan+K3 end | results
  // ready (K2's end is ev[5] where lean marks left ev[2] unrecorded)
  const hipEvent_t bd[5] = {b->ev[0], b->ev[1], b->k2_ev5 ? b->ev[5] : b->ev[2], b->ev[3], b->ev[4]};
  for (int i = 0; i < 4; i++) {
    c->stage_ms[i] = 0.f;
    // a pipelined batch has no ev[3]: [2] then spans K2 end -> results ready
    const int e = (i == 2 && !b->ev3) ? 4 : i + 1;
    if ((i != 3 || b->ev3) && hipEventElapsedTime(&ms, bd[i], bd[e]) == hipSuccess) c->stage_ms[i] = ms;
  }
  if (hipEventElapsedTime(&ms, b->ev[0], b->ev[4]) == hipSuccess) c->stage_ms[4] = ms;
  return rc;
}

// Complete the oldest pending batch (draining the MD5 chains first if its
// chains are not yet guaranteed hashed) and collect it.
int wait_oldest(hbx_ctx* c) {
  if (c->pending.empty()) return HBX_OK;
  Batch* b = c->pending.front();
  if (c->broken) {  // drop it uncollected: its results are never written to the caller
    c->pending.pop_front();
    c->parked.push_back(b);
    return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  }
  // drain: every chain in flight; a pre-planned launch runs first (with an
  // unlimited budget), then b joins if it had not yet (b is the oldest)
  for (int k = 0; !b->finalized; k++) {
    const uint64_t l0 = c->launches;
    int rc = md5_step(c, kBudgetAll, true);
    if (rc) return rc;
    if (c->launches == l0 || k > 2) return c->fail(HBX_ERR_STATE, "drain launched nothing (internal)");
  }
  HBX_TRY(c, hipEventSynchronize(b->ev[4]));
  if (c->h_err.p && *static_cast<volatile uint32_t*>(c->h_err.p)) {  // a K3Q wave gave up: results wrong
    c->pending.pop_front();
    c->parked.push_back(b);
    c->broken = true;
    return c->fail(HBX_ERR_STATE, "K3 item queue: a wave timed out waiting for an item (internal); destroy the context");
  }
  c->pending.pop_front();
  // ev[4] follows the K3 launch that finalized b (the result stream waited for it)
  if (b->joined) c->k3_done_upto = std::max<uint64_t>(c->k3_done_upto, b->final_launch + 1);
  int rc = collect_batch(c, b);
  c->pool.push_back(b);
  harvest_timings(c);
  harvest_k3(c);
  return rc;
}

int run_device_sync(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                    const uint64_t* lens, uint64_t* cut_ends, uint8_t* ids,
                    const uint64_t* out_base, const uint64_t* caps, hbx_file_summary* sums) {
  const int slot = c->ssum_slot;  // the summary slot this batch's K1 writes
  int rc = submit_batch(c, d_arena, n, offs, lens, cut_ends, ids, out_base, caps, sums, kBudgetAll);
  if (rc) return rc;
  rc = wait_oldest(c);
  if (rc == HBX_OK || rc == HBX_ERR_CAPACITY) {  // the scan ran whole either way: hbx_k1_summaries may read it
    uint64_t slices = 0;
    for (uint64_t f = 0; f < n; f++)
      if (scan_iters(lens[f])) slices += (lens[f] + kSlice - 1) / kSlice;
    c->k1_sum_slot = slot;
    c->k1_sum_slices = slices;
  }
  return rc;
}

}  // namespace

// ======================================================================
extern "C" {

int hbx_version(void) { return 1; }

int hbx_device_count(int* n) {
  if (!n) return HBX_ERR_ARG;
  int c = 0;
  if (hipGetDeviceCount(&c) != hipSuccess) c = 0;
  *n = c;
  return c > 0 ? HBX_OK : HBX_ERR_NODEV;
}

uint64_t hbx_max_chunks(uint64_t len) { return max_chunks(len); }

// A/B and diagnostic switches (HBX_*) are read only when HBX_AB=1 is set as
// well: a caller's stray environment must not change the product path.  The
// effective values are reported by hbx_knobs().
static const char* ab_env(const char* name) {
  const char* ab = std::getenv("HBX_AB");
  return (ab && std::atoi(ab) != 0) ? std::getenv(name) : nullptr;
}

// HBX_SCAN_CUS / HBX_HASH_CUS / HBX_RES_CUS = "first:count[:stride]" restrict a
// stream's dispatches to those CU indices (hipExtStreamCreateWithCUMask);
// "off" or unset = an ordinary stream.  The scan stream defaults to a full
// mask: a CU-masked stream gets a hardware queue of its own, and K1/K2 on it
// beside K3 run 2.6 % faster end to end (2,100 vs 2,046 GiB/s, 3 A/B pairs,
// tools/gpu_ab_cumask3.sh).  Masking the hash or result stream, even with
// all CUs, serializes K1 and K3 (1,510-1,540 GiB/s): leave them unmasked.
static hipError_t make_stream(hipStream_t* s, const char* env, int ncu, const char* dflt = nullptr) {
  const char* v = ab_env(env);
  if (!v) v = dflt;
  int first = 0, count = 0, stride = 1;
  if (!v || std::sscanf(v, "%d:%d:%d", &first, &count, &stride) < 2 || count <= 0 || ncu <= 0) {
    // A/B only: "prio:hi" / "prio:lo" = an unmasked stream at the device's
    // greatest / least priority
    int lo = 0, hi = 0;
    if (v && std::strncmp(v, "prio:", 5) == 0 && hipDeviceGetStreamPriorityRange(&lo, &hi) == hipSuccess)
      return hipStreamCreateWithPriority(s, hipStreamNonBlocking, std::strcmp(v + 5, "hi") == 0 ? hi : lo);
    return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
  }
  std::vector<uint32_t> mask((size_t)(ncu + 31) / 32, 0u);
  for (int i = 0, cu = first; i < count && cu < ncu; i++, cu += std::max(1, stride))
    mask[(size_t)cu / 32] |= 1u << (cu % 32);
  // the mask is a scheduling choice, not a requirement: a runtime that
  // refuses it gets an ordinary stream
  if (hipExtStreamCreateWithCUMask(s, (uint32_t)mask.size(), mask.data()) == hipSuccess) return hipSuccess;
  (void)hipGetLastError();
  return hipStreamCreateWithFlags(s, hipStreamNonBlocking);
}

// SDMA engine warm-up (verdict r05 item 2: the ~7 ms host stall in the copy
// call).  The HSA runtime creates an SDMA engine's queue the first time a
// copy is put on that engine, and hipMemcpyAsync puts a copy on the first
// engine that is free at the call: with one 8 GiB H2D copy still running the
// next goes to the next engine, so the first copies of a pipeline each met a
// fresh engine and the call held the host 7.2-7.6 ms while the runtime
// built its queue (AMD_LOG_LEVEL=4 of the e2e leg: only the first 8 GiB copy on
// engines 0x2, 0x4, 0x8 and 0x10 was slow, every later one on the same engine
// took 17-34 us; HSA_ENABLE_SDMA=0 removed the stall with blit kernels,
// ROC_SIGNAL_POOL_SIZE and HSA_ENABLE_SDMA_GANG did not move it;
// profiles/r06c).  So every engine the runtime reports for H2D and D2H gets
// one 64-byte copy here, once per device per process, before any pipeline
// runs.  HBX_SDMA_WARM=0 (A/B) leaves the engines cold.
static hsa_status_t first_cpu_agent(hsa_agent_t a, void* data) {
  hsa_device_type_t t;
  if (hsa_agent_get_info(a, HSA_AGENT_INFO_DEVICE, &t) == HSA_STATUS_SUCCESS && t == HSA_DEVICE_TYPE_CPU) {
    *static_cast<hsa_agent_t*>(data) = a;
    return HSA_STATUS_INFO_BREAK;
  }
  return HSA_STATUS_SUCCESS;
}
static void warm_sdma_engines(hbx_ctx* c) {
  static std::mutex mu;
  static uint64_t done = 0;  // devices warmed in this process (bit per device)
  std::lock_guard<std::mutex> g(mu);
  if (c->device >= 64 || (done >> c->device) & 1u) return;
  const auto t0 = std::chrono::steady_clock::now();
  void* d = nullptr;
  void* h = nullptr;
  if (hipMalloc(&d, 4096) != hipSuccess || hipHostMalloc(&h, 4096, hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    if (d) (void)hipFree(d);
    return;  // no warm-up: correct, only the first copies per engine are slow
  }
  std::memset(h, 0, 4096);
  hsa_amd_pointer_info_t pi;
  std::memset(&pi, 0, sizeof(pi));
  pi.size = sizeof(pi);
  hsa_agent_t cpu{0};
  hsa_signal_t sig{0};
  if (hsa_amd_pointer_info(d, &pi, nullptr, nullptr, nullptr) == HSA_STATUS_SUCCESS && pi.agentOwner.handle &&
      hsa_iterate_agents(first_cpu_agent, &cpu) != HSA_STATUS_ERROR && cpu.handle &&
      hsa_signal_create(1, 0, nullptr, &sig) == HSA_STATUS_SUCCESS) {
    const hsa_agent_t gpu = pi.agentOwner;
    for (int dir = 0; dir < 2; dir++) {
      const hsa_agent_t dst = dir ? cpu : gpu, src = dir ? gpu : cpu;
      uint32_t mask = 0;
      if (hsa_amd_memory_copy_engine_status(dst, src, &mask) != HSA_STATUS_SUCCESS) continue;
      (dir ? c->sdma_d2h : c->sdma_h2d) = mask;
      for (uint32_t bit = 1; bit && bit <= mask; bit <<= 1) {
        if (!(mask & bit)) continue;
        hsa_signal_store_screlease(sig, 1);
        if (hsa_amd_memory_async_copy_on_engine(dir ? h : d, dst, dir ? d : h, src, 64, 0, nullptr, sig,
                                                (hsa_amd_sdma_engine_id_t)bit, true) != HSA_STATUS_SUCCESS)
          continue;
        (void)hsa_signal_wait_scacquire(sig, HSA_SIGNAL_CONDITION_LT, 1, UINT64_MAX, HSA_WAIT_STATE_BLOCKED);
      }
    }
    hsa_signal_destroy(sig);
  }
  (void)hipHostFree(h);
  (void)hipFree(d);
  done |= 1ull << c->device;
  c->sdma_warm_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

int hbx_ctx_create(int device, hbx_ctx** out) {
  if (!out) return HBX_ERR_ARG;
  *out = nullptr;
  int nd = 0;
  if (hipGetDeviceCount(&nd) != hipSuccess || nd <= 0) return HBX_ERR_NODEV;
  if (device < 0 || device >= nd) return HBX_ERR_ARG;
  hbx_ctx* c = new hbx_ctx();
  c->device = device;
  hipDeviceProp_t prop;
  int ncu = 0;
  if (hipGetDeviceProperties(&prop, device) == hipSuccess && prop.multiProcessorCount > 0)
    c->md5_wgs = (uint32_t)(ncu = prop.multiProcessorCount);
  if (const char* v = ab_env("HBX_TILE_ITERS")) c->tile_iters = (uint32_t)std::min(1024, std::max(0, std::atoi(v)));
  if (const char* v = ab_env("HBX_K3_PERIOD")) c->k3_period = (uint32_t)std::min(kMaxFresh, std::max(1, std::atoi(v)));
  if (const char* v = ab_env("HBX_JOIN_LAG")) c->join_lag = (uint32_t)std::min(4, std::max(1, std::atoi(v)));
  if (const char* v = ab_env("HBX_K4_WINDOW")) c->k4_window = (uint32_t)std::min(1024, std::max(1, std::atoi(v)));
  if (const char* v = ab_env("HBX_MD5_SLICE")) c->md5_slice = (uint32_t)std::max(0, std::atoi(v));
  if (const char* v = ab_env("HBX_K1_GATE")) c->k1_gate = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_LEAN_MARKS")) c->lean_marks = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_D2H_KERNEL")) c->d2h_kernel = (uint32_t)std::min(std::max(std::atoi(v), 0), 1024);
  if (const char* v = ab_env("HBX_K3_PROD")) c->k3_prod = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_PLAN_CUT")) c->plan_cut = (uint32_t)std::min(2, std::max(0, std::atoi(v)));
  if (const char* v = ab_env("HBX_META_KERNEL")) c->meta_kernel = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_GATE_META")) c->gate_meta = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_SDMA_WARM")) c->sdma_warm = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_K3_PSETS")) c->k3_psets = std::atoi(v) == 3 ? 3u : 2u;
  if (const char* v = ab_env("HBX_K3_SPIN")) c->k3_spin = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_PLAN_ADDR")) c->plan_addr = (uint32_t)std::min(512, std::max(0, std::atoi(v)));
  if (const char* v = ab_env("HBX_PLAN_ADDR_SHIFT")) c->plan_addr_shift = (uint32_t)std::min(40, std::max(20, std::atoi(v)));
  if (const char* v = ab_env("HBX_K1_EXT")) c->k1_ext = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_K1_DMA4")) c->k1_dma4 = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_K1_EARLY")) c->k1_early = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_K1_SWZ")) c->k1_swz = std::atoi(v) ? 1u : 0u;
  if (const char* v = ab_env("HBX_K3_ITEMS")) c->k3_items = (uint32_t)std::min(8, std::max(0, std::atoi(v)));
  // (tests: a K3 grid of a few workgroups, so every wave takes many groups)
  if (const char* v = ab_env("HBX_K3_WGS")) c->md5_wgs = (uint32_t)std::min<int>(std::max(1, ncu), std::max(1, std::atoi(v)));
  // (tests: a K14 grid of one or two workgroups, so a small image spans several grid-stride rounds)
  if (const char* v = ab_env("HBX_K14_WGS")) c->k14_wgs = (uint32_t)std::min(65536, std::max(0, std::atoi(v)));
  // (tests: a K15 grid of one or two workgroups, so a small table spans several grid-stride rounds)
  if (const char* v = ab_env("HBX_K15_WGS")) c->k15_wgs = (uint32_t)std::min(65536, std::max(0, std::atoi(v)));
  // (tests: K16 tiles of 256 and 4,096 bytes, so a small stream spans many tiles)
  if (const char* v = ab_env("HBX_K16_TILE")) c->k16_tile = hbxk::tile_of(std::atoi(v));
  if (hipSetDevice(device) != hipSuccess || make_stream(&c->stream, "HBX_SCAN_CUS", ncu, "0:4096") != hipSuccess) {
    delete c;
    return HBX_ERR_HIP;
  }
  if (const char* v = ab_env("HBX_K2_STREAM")) c->k2_own = std::atoi(v) ? 1 : 0;
  c->cstream = c->stream;
  if (make_stream(&c->hstream, "HBX_HASH_CUS", ncu) != hipSuccess ||
             make_stream(&c->rstream, "HBX_RES_CUS", ncu) != hipSuccess || ensure_cut_stream(c) != HBX_OK) {
    hbx_ctx_destroy(c);
    return HBX_ERR_HIP;
  }
  if (c->h_k3t.ensure(kK3TimeRing * 16) == hipSuccess) std::memset(c->h_k3t.p, 0, kK3TimeRing * 16);
  if (c->d_gate.ensure(256) != hipSuccess || hipMemset(c->d_gate.p, 0, 256) != hipSuccess ||
      hipEventCreateWithFlags(&c->ssum_free[0], hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&c->ssum_free[1], hipEventDisableTiming) != hipSuccess) {
    hbx_ctx_destroy(c);
    return HBX_ERR_HIP;
  }
  for (int t = 0; t < kDoneRing; t++) {
    if ((t >= 3 || hipEventCreateWithFlags(&c->plan_done[t], hipEventDisableTiming) == hipSuccess) &&
        hipEventCreateWithFlags(&c->order_free[t], hipEventDisableTiming) == hipSuccess)
      continue;
    hbx_ctx_destroy(c);
    return HBX_ERR_HIP;
  }
  if (c->sdma_warm) warm_sdma_engines(c);
  *out = c;
  return HBX_OK;
}

void hbx_ctx_destroy(hbx_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  for (hipStream_t s : {c->stream, c->cstream, c->hstream, c->rstream})
    if (s) (void)hipStreamSynchronize(s);
  for (hipEvent_t e : {c->producer, c->ssum_free[0], c->ssum_free[1], c->plan_done[0], c->plan_done[1],
                       c->plan_done[2]})
    if (e) (void)hipEventDestroy(e);
  for (hipEvent_t e : c->order_free)
    if (e) (void)hipEventDestroy(e);
  for (DevBuf* b : {&c->d_ssum[0], &c->d_ssum[1], &c->d_order[0], &c->d_order[1], &c->d_order[2],
                    &c->d_octl[0], &c->d_octl[1], &c->d_octl[2], &c->d_q[0], &c->d_q[1], &c->d_q[2], &c->d_gate,
                    &c->d_stage, &c->d_msg, &c->d_plan, &c->d_vdesc, &c->d_vlinks,
                    &c->d_vout, &c->d_vexp, &c->d_zeros, &c->d_zblk, &c->d_zinfo, &c->d_zoff,
                    &c->d_zlen, &c->d_zout, &c->d_zimg, &c->d_idesc, &c->d_ires, &c->d_sreg, &c->d_sstart,
                    &c->d_sres, &c->d_sscratch, &c->d_smeta, &c->d_rin[0], &c->d_rin[1], &c->d_rslots, &c->d_rimg,
                    &c->d_rpiece, &c->d_rword, &c->d_rretry})
    b->release();
  for (PinBuf* h : {&c->h_rin[0], &c->h_rin[1], &c->h_rout[0], &c->h_rout[1]}) h->release();
  if (c->fstream) {
    (void)hipStreamSynchronize(c->fstream);
    (void)hipStreamDestroy(c->fstream);
  }
  for (PinBuf& h : c->h_read) h.release();
  c->h_zstage.release();
  for (auto& z : c->zs)
    if (z.stream) (void)hipStreamSynchronize(z.stream);
  for (auto& z : c->zs) {
    for (DevBuf* b : {&z.blk, &z.info, &z.off, &z.len, &z.img, &z.out}) b->release();
    z.desc.release();
    z.lens.release();
    z.stage.release();
    if (z.done) (void)hipEventDestroy(z.done);
    if (z.stream) (void)hipStreamDestroy(z.stream);
  }
  if (c->sstream) {
    (void)hipStreamSynchronize(c->sstream);
    (void)hipStreamDestroy(c->sstream);
  }
  for (hbx_idset* t : c->idsets) {
    t->release();
    delete t;
  }
  for (hbx_index* x : c->indexes) {
    x->release();
    delete x;
  }
  c->d_dscratch.release();
  for (DevBuf& d : c->d_mt) d.release();
  c->d_mtout.release();
  for (DevBuf& d : c->d_lc) d.release();
  for (DevBuf& d : c->d_df) d.release();
  for (DevBuf& d : c->d_bg) d.release();
  for (DevBuf& d : c->d_cp) d.release();
  c->d_dfimg.release();
  for (PinBuf& h : c->h_dfstage) h.release();
  for (hbx_seg* h : c->segs_open) delete h;
  for (DevBuf& d : c->seg_words) d.release();
  c->d_segmsg.release();
  c->h_k3t.release();
  c->h_probe.release();
  c->h_err.release();
  for (DevBuf& d : c->d_ring) d.release();
  for (hipEvent_t e : c->h2d_done)
    if (e) (void)hipEventDestroy(e);
  for (Batch* b : c->pending) c->pool.push_back(b);
  for (Batch* b : c->parked) c->pool.push_back(b);
  for (Batch* b : c->pool) {
    b->release();
    delete b;
  }
  for (int i = 0; i < 3; i++)
    if (c->plan_timer_set[i]) c->open_t.push_back(c->plan_timer[i]);
  for (TimedLaunch& t : c->open_t) {
    if (!t.owned) continue;  // a batch's own events (released with the batch)
    (void)hipEventDestroy(t.a);
    (void)hipEventDestroy(t.b);
  }
  for (hipEvent_t e : c->ev_pool) (void)hipEventDestroy(e);
  for (hipStream_t s : {c->cstream, c->hstream, c->rstream})
    if (s && s != c->stream) (void)hipStreamDestroy(s);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

// Failures of calls made without a context (hbx_plan_pipeline with ctx NULL)
// are described per thread.
static thread_local std::string g_noctx_err;
// A context's text is written under its lock by whichever thread fails a call
// there, so it is read under that lock too, into a copy of the calling
// thread's: another thread failing a call meanwhile can neither tear the text
// nor free it under the reader (tests/test_gpu_threads.py has four threads
// failing calls on one context).  The copy lives until this thread asks again.
const char* hbx_last_error(const hbx_ctx* c) {
  if (!c) return g_noctx_err.empty() ? "null context" : g_noctx_err.c_str();
  static thread_local std::string mine;
  std::lock_guard<std::mutex> g(const_cast<hbx_ctx*>(c)->mu);
  mine = c->err;
  return mine.c_str();
}

int hbx_set_tile_iters(hbx_ctx* c, uint32_t iters) {
  if (!c || iters > 1024) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  c->tile_iters = iters;
  return HBX_OK;
}

int hbx_set_join_lag(hbx_ctx* c, uint32_t lag) {
  if (!c || lag < 1 || lag > 4) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  // pending batches were counted against the lag of their submit
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  c->join_lag = lag;
  return ensure_cut_stream(c);
}

int hbx_set_k3_period(hbx_ctx* c, uint32_t period) {
  if (!c || period < 1 || period > (uint32_t)kMaxFresh) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  // pending batches were counted against the launch budget of their submit
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  c->k3_period = period;
  c->k3_tick = 0;
  return HBX_OK;
}

// The pipeline's operating point (DESIGN.md §3 "Throughput model", §7):
// throughput ~ bytes resident / a batch's lifetime, so R = as many arenas as
// hbm_frac of the free memory holds; a batch holds its arena for its `need`
// launches (period P apart) plus the join lag and lead, so the slice is the
// longest chain's blocks over the launches that fit in R - lead - (P - 1)
// submits.  bench.py takes every plan from here (tests/test_plan.py checks
// it against the round-5 Python planner at N = 1..8).
int hbx_plan_pipeline(hbx_ctx* c, const hbx_plan_request* q, hbx_pipeline_plan* p) {
  if (!q || !p) return HBX_ERR_ARG;
  auto bad = [&](const std::string& m) {
    if (c) return c->fail(HBX_ERR_ARG, m);
    g_noctx_err = m;
    return HBX_ERR_ARG;
  };
  if (q->n_files == 0) return bad("hbx_plan_pipeline: no files");
  if (q->join_lag > 4) return bad("hbx_plan_pipeline: join lag must be 1..4");
  if (q->k3_period > kMaxFresh) return bad("hbx_plan_pipeline: K3 period must be 1..8");
  uint64_t free_b = q->free_bytes;
  if (free_b == 0) {
    if (!c) return bad("hbx_plan_pipeline: free_bytes 0 needs a context");
    std::lock_guard<std::mutex> g(c->mu);
    size_t fr = 0, tot = 0;
    HBX_TRY(c, hipSetDevice(c->device));
    HBX_TRY(c, hipMemGetInfo(&fr, &tot));
    free_b = fr;
  }
  const int64_t lag = q->join_lag > 0 ? q->join_lag : 2;
  const bool host_in = (q->flags & HBX_PLAN_HOST_INPUT) != 0;
  int64_t per = 1;
  if (q->k3_period > 0) {
    per = q->k3_period;
  } else if (q->n_files < 32 && !host_in) {
    // small per-GPU batches: the launch's start-up and tail once per 4 steps
    // (profiles/r05j, r05o: 8 files 2,013 -> 2,056-2,083 GiB/s; 32 files P1
    // 2,277-2,294 vs P2 2,260-2,272)
    per = (q->steps == 0 || q->steps % 4 == 0) ? 4 : (q->steps % 2 == 0) ? 2 : 1;
  }
  // lead (steps an arena stays resident beyond its batch's launches): the join
  // lag at 64 or more files per GPU (round 6: the next batch's K1 follows the
  // launch that finishes the old one through hbx_input_after_oldest; R = 33 at
  // 64 files then holds 31 launches instead of 30: 2,380-2,391 vs 2,303-2,350
  // GiB/s in three alternating pairs, profiles/r06p), lag + 1 below (32 files:
  // 2,229/2,232 vs 2,279/2,273, profiles/r06zf, where the extra chains take
  // CUs from a K1 that already sets the step; 8 files: 2,045 vs 2,082) and for
  // host input
  const int64_t ld = q->lead >= 0 ? q->lead : lag + ((q->n_files >= 64 && !host_in) ? 0 : 1);
  const uint64_t nfull = (std::min<uint64_t>(q->longest_file, HBX_MAX_BLOCK_SIZE) + 8u) >> 6;
  const double frac = q->hbm_frac > 0.0 ? q->hbm_frac : 0.95;
  const uint64_t share = (uint64_t)((double)free_b * frac / (double)std::max<uint32_t>(1u, q->ranks_per_device));
  const uint64_t stride = q->arena_bytes + HBX_PLAN_ARENA_SLACK;
  int64_t r_fit = std::max<int64_t>(ld + 1, (int64_t)(share / stride));
  if (host_in) r_fit = std::min<int64_t>(r_fit, ld + 2);  // PCIe-bound: a shallow pipeline suffices
  auto cdiv = [](uint64_t a, uint64_t b) { return (a + b - 1) / b; };
  auto slice_for = [&](int64_t R) {  // launches of P x B blocks, P submits apart, within R - lead - (P - 1)
    const int64_t launches = std::max<int64_t>(1, (R - ld - per + 1) / per);
    return cdiv(nfull, (uint64_t)(launches * per));
  };
  int64_t R;
  uint64_t B;
  if (q->md5_slice < 0) {
    R = q->arenas > 0 ? q->arenas : r_fit;
    B = slice_for(R);
  } else {
    B = (uint64_t)q->md5_slice;
    R = q->arenas > 0 ? q->arenas
                      : std::min<int64_t>((B == 0 ? 1 : (int64_t)cdiv(nfull, B * per)) * per + ld + per - 1, r_fit);
  }
  const int64_t need = B == 0 ? 1 : (int64_t)cdiv(nfull, B * per);  // K3 launches per batch
  if (need * per + lag + per - 1 > R)
    return bad("hbx_plan_pipeline: pipeline depth " + std::to_string(R) + " < launches per batch " +
               std::to_string(need) + " x period " + std::to_string(per) + " + join lag " + std::to_string(lag) +
               " + " + std::to_string(per - 1) + ": more arenas or a larger slice");
  if (B > 0xFFFFFFFFull || R > 0xFFFFFFFFll) return bad("hbx_plan_pipeline: plan out of range");
  p->resident = (uint32_t)R;
  p->md5_slice = (uint32_t)B;
  p->join_lag = (uint32_t)lag;
  p->lead = (uint32_t)ld;
  p->k3_period = (uint32_t)per;
  p->launches_per_batch = (uint32_t)need;
  p->hbm_bytes = (uint64_t)R * stride;
  return HBX_OK;
}

int hbx_apply_plan(hbx_ctx* c, const hbx_pipeline_plan* p, uint64_t files, uint64_t bytes) {
  if (!c || !p || p->resident == 0) return HBX_ERR_ARG;
  int rc = hbx_set_md5_slice(c, p->md5_slice);
  if (!rc) rc = hbx_set_join_lag(c, p->join_lag);
  if (!rc) rc = hbx_set_k3_period(c, p->k3_period);
  if (!rc) rc = hbx_reserve(c, p->resident + 2u, files, bytes);
  return rc;
}

int hbx_knobs(hbx_ctx* c, char* out, uint64_t cap) {
  if (!c || !out || cap == 0) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  const char* ab = std::getenv("HBX_AB");
  const int n = std::snprintf(
      out, (size_t)cap,
      "{\"ab_env\": %d, \"md5_slice\": %u, \"join_lag\": %u, \"tile_iters\": %u, \"k1_gate\": %u, "
      "\"md5_wgs\": %u, \"plan_mode\": %d, \"k2_own\": %d, \"k4_window\": %u, \"k3_probe\": %d, "
      "\"lean_marks\": %u, \"k3_prod\": %u, \"k3_items\": %u, \"k3_period\": %u, \"meta_kernel\": %u, "
      "\"plan_cut\": %u, \"k1_swz\": %u, \"k3_psets\": %u, \"d2h_kernel\": %u, \"k8_split_streams\": %llu, "
      "\"k8_split_fallbacks\": %llu, \"gate_meta\": %u, \"sdma_warm\": %u, \"sdma_h2d_mask\": %u, "
      "\"sdma_d2h_mask\": %u, \"sdma_warm_ms\": %.3f, \"k3_spin\": %u, \"plan_addr\": %u, \"plan_addr_shift\": %u, \"k1_ext\": %u, \"k1_dma4\": %u, \"k1_early\": %u, "
      "\"restore_ms\": [%.3f, %.3f, %.3f, %.3f], \"restore_many\": [%llu, %llu, %llu], "
      "\"match_push_bytes\": %llu, \"k14_wgs\": %u, \"datfile\": [%llu, %llu], \"k15_wgs\": %u, "
      "\"k15_lane_max\": %u, \"k15_wave_max\": %u, \"k16_tile\": %u}",
      (ab && std::atoi(ab) != 0) ? 1 : 0, c->md5_slice, c->join_lag, c->tile_iters, c->k1_gate, c->md5_wgs,
      plan_mode_of(c), c->k2_own, c->k4_window, c->h_probe.p ? 1 : 0, c->lean_marks, c->k3_prod, c->k3_items,
      c->k3_period, c->meta_kernel, c->plan_cut, c->k1_swz, c->k3_psets, c->d2h_kernel,
      (unsigned long long)c->k8_split_streams, (unsigned long long)c->k8_split_fallbacks, c->gate_meta,
      c->sdma_warm, c->sdma_h2d, c->sdma_d2h, c->sdma_warm_ms, c->k3_spin, c->plan_addr, c->plan_addr_shift, c->k1_ext, c->k1_dma4, c->k1_early,
      c->restore_ms[0], c->restore_ms[1], c->restore_ms[2], c->restore_ms[3],
      (unsigned long long)c->many_windows, (unsigned long long)c->many_passes, (unsigned long long)c->many_retries,
      (unsigned long long)c->match_push_bytes, c->k14_wgs, (unsigned long long)c->dat_windows,
      (unsigned long long)c->dat_retries, c->k15_wgs, hbxg::kLaneMax, hbxg::kWaveMax, c->k16_tile);
  return (n > 0 && (uint64_t)n < cap) ? HBX_OK : HBX_ERR_ARG;
}

int hbx_set_k3_probe(hbx_ctx* c, int on) {
  if (!c) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  // the launch in flight may still write the records
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  HBX_TRY(c, hipStreamSynchronize(c->hstream));
  if (!on) {
    c->h_probe.release();
    return HBX_OK;
  }
  const size_t n = (size_t)c->md5_wgs * (kK3Threads / 64) * 64;
  HBX_TRY(c, c->h_probe.ensure(n));
  std::memset(c->h_probe.p, 0, n);
  return HBX_OK;
}

int hbx_k3_wave_times(hbx_ctx* c, uint64_t* out, uint32_t max_waves, uint32_t* n_waves) {
  if (!c || !n_waves) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  *n_waves = 0;
  if (!c->h_probe.p) return c->fail(HBX_ERR_STATE, "K3 probe not enabled (hbx_set_k3_probe)");
  HBX_TRY(c, hipSetDevice(c->device));
  HBX_TRY(c, hipStreamSynchronize(c->hstream));
  const uint32_t n = c->md5_wgs * (kK3Threads / 64);
  if (out) std::memcpy(out, c->h_probe.p, (size_t)std::min(n, max_waves) * 64);
  *n_waves = n;
  return HBX_OK;
}

int hbx_k1_summaries(hbx_ctx* c, uint64_t* first, uint64_t* count, uint64_t max_files, uint64_t* n_files,
                     uint32_t* pairs, uint64_t max_slices, uint64_t* n_slices) {
  if (!c || !n_files || !n_slices) return HBX_ERR_ARG;
  if ((max_files && (!first || !count)) || (max_slices && !pairs)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  *n_files = 0;
  *n_slices = 0;
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (c->k1_sum_slot < 0)
    return c->fail(HBX_ERR_STATE, "no synchronous device batch since the context was created, reserved or last submitted to");
  const uint64_t n = c->h_slice_base.size(), slices = c->k1_sum_slices;
  *n_files = n;
  *n_slices = slices;
  if (max_files < n || max_slices < slices) return c->fail(HBX_ERR_CAPACITY, "hbx_k1_summaries: output arrays too small");
  for (uint64_t f = 0; f < n; f++) {
    first[f] = c->h_slice_base[f];
    count[f] = (f + 1 < n ? c->h_slice_base[f + 1] : slices) - c->h_slice_base[f];
  }
  if (!slices) return HBX_OK;
  HBX_TRY(c, hipSetDevice(c->device));
  // the batch was collected, so its K1 and K2 are complete; the dummy slot behind the last slice is left out
  HBX_TRY(c, hipMemcpy(pairs, c->d_ssum[c->k1_sum_slot].p, slices * sizeof(uint2), hipMemcpyDeviceToHost));
  return HBX_OK;
}

int hbx_stage_times(hbx_ctx* c, float ms[5]) {
  if (!c || !ms) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  for (int i = 0; i < 5; i++) ms[i] = c->stage_ms[i];
  return HBX_OK;
}

int hbx_set_md5_slice(hbx_ctx* c, uint32_t blocks) {
  if (!c) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  // a pending batch's launch count was fixed at submit from the slice of
  // that moment: changing it now would finalize batches whose chains are
  // not all hashed
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  c->md5_slice = blocks;
  return HBX_OK;
}

int hbx_reserve(hbx_ctx* c, uint32_t batches, uint64_t files, uint64_t bytes) {
  if (!c || files > 0xFFFFFFFFull) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return reserve_locked(c, batches, files, bytes);
}

int reserve_locked(hbx_ctx* c, uint32_t batches, uint64_t files, uint64_t bytes, bool dedup, bool match,
                   uint64_t match_ids) {
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  c->k1_sum_slot = -1;  // the summary slots may be reallocated
  const uint64_t caps = bytes / HBX_MIN_BLOCK_SIZE + files;  // >= sum of max_chunks over the files
  const uint64_t tiles = bytes / ((uint64_t)(c->tile_iters ? c->tile_iters : kTileItersMin) * HBX_MIN_BLOCK_SIZE) + files;
  const uint64_t slices = bytes / kSlice + files;
  const size_t meta_bytes = files * 8 * 8 + tiles * sizeof(uint4);  // (8: a batch of segments)
  int rc = HBX_OK;
  for (int t = 0; t < 2 && !rc; t++) rc = ensure_shared(c, c->d_ssum[t], (slices + 1) * sizeof(uint2));
  if (!rc) rc = ensure_shared(c, c->d_plan, 2 * kPlanBins * sizeof(uint32_t));
  for (int t = 0; t < 3 && !rc; t++) {
    rc = ensure_shared(c, c->d_order[t], ((uint64_t)batches * caps + 64) * sizeof(OrderEntry));
    if (!rc) rc = ensure_shared(c, c->d_octl[t], 256);
    if (!rc) rc = ensure_shared(c, c->d_q[t], (((uint64_t)batches * caps + 64) / 64 + 2) * 8 * 8);
  }
  if (!rc && dedup) rc = ensure_shared(c, c->d_dscratch, hbxd::table_slots(caps) * sizeof(uint32_t));
  if (rc) return rc;
  std::vector<Batch*> ready;
  while (ready.size() < batches) {
    Batch* b = acquire_batch(c);  // pooled first, then new
    if (!b) break;
    ready.push_back(b);
    const size_t rbytes = res_layout(files, caps, dedup, match).total;
    if (match) {  // the staging of the batch's expected chains: the steady state allocates nothing
      const size_t ebytes = al256((files + 1) * 8) + 16 * match_ids;
      for (auto r : {b->h_exp.ensure(ebytes), b->d_exp.ensure(ebytes)})
        if (r != hipSuccess && !rc) rc = c->hip(r, "hbx_reserve");
    }
    for (auto r : {b->h_meta.ensure(meta_bytes), b->d_meta.ensure(meta_bytes), b->d_res.ensure(rbytes),
                   b->d_run.ensure(caps * sizeof(Chain)), b->d_fresh.ensure(caps * sizeof(OrderEntry)),
                   b->d_fcnt.ensure(256), b->h_res.ensure(rbytes)})
      if (r != hipSuccess && !rc) rc = c->hip(r, "hbx_reserve");
    if (rc) break;
  }
  for (Batch* b : ready) c->pool.push_back(b);
  if (!rc && ready.size() < batches) rc = c->fail(HBX_ERR_HIP, "cannot create batch events");
  return rc;
}

int hbx_stage_totals(hbx_ctx* c, double ms[5], uint64_t launches[5], int reset) {
  if (!c) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  harvest_timings(c);
  if (c->hstream && hipStreamQuery(c->hstream) == hipSuccess) c->k3_done_upto = c->launches;
  harvest_k3(c);
  for (int i = 0; i < 5; i++) {
    if (ms) ms[i] = c->tot_ms[i];
    if (launches) launches[i] = c->tot_n[i];
    if (reset) {
      c->tot_ms[i] = 0.0;
      c->tot_n[i] = 0;
    }
  }
  return HBX_OK;
}

int hbx_chunk_hash_device(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                          const uint64_t* lens, uint64_t* cut_ends, uint8_t* ids,
                          const uint64_t* out_base, const uint64_t* caps,
                          hbx_file_summary* sums) {
  if (!c) return HBX_ERR_ARG;
  if (n && (!d_arena || !offs || !lens || !out_base || !caps)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  return run_device_sync(c, d_arena, n, offs, lens, cut_ends, ids, out_base, caps, sums);
}

int hbx_submit_device(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                      const uint64_t* lens, uint64_t* cut_ends, uint8_t* ids,
                      const uint64_t* out_base, const uint64_t* caps, hbx_file_summary* sums) {
  return hbx_submit_device_dd(c, d_arena, n, offs, lens, cut_ends, ids, out_base, caps, sums, nullptr, nullptr);
}

int hbx_submit_device_dd(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs, const uint64_t* lens,
                         uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base, const uint64_t* caps,
                         hbx_file_summary* sums, hbx_idset* set, uint8_t* fresh) {
  if (!c) return HBX_ERR_ARG;
  if (n && (!d_arena || !offs || !lens || !out_base || !caps)) return HBX_ERR_ARG;
  if (set && !fresh) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (set && std::find(c->idsets.begin(), c->idsets.end(), set) == c->idsets.end())
    return c->fail(HBX_ERR_ARG, "not an ID set of this context");
  HBX_TRY(c, hipSetDevice(c->device));
  return submit_batch(c, d_arena, n, offs, lens, cut_ends, ids, out_base, caps, sums,
                      c->md5_slice ? c->md5_slice : kBudgetAll, nullptr, nullptr, set, set ? fresh : nullptr);
}

namespace {
// The checks the match calls share, before the context is touched: *vo = verdict-only mode.
int match_args(uint64_t n, uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base, const uint64_t* caps,
               const uint64_t* first, const uint8_t* eids, const hbx_chain_match* out, bool* vo) {
  if (!out) return HBX_ERR_ARG;
  *vo = !out_base && !caps;
  if (*vo ? (cut_ends || ids) : (n && (!out_base || !caps))) return HBX_ERR_ARG;
  for (uint64_t f = 0; f < n; f++)
    if (first[f + 1] < first[f] || first[f + 1] - first[f] > 0xFFFFFFFFull) return HBX_ERR_ARG;
  if (first[n] > first[0] && !eids) return HBX_ERR_ARG;
  return HBX_OK;
}
}  // namespace

int hbx_submit_device_match(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs, const uint64_t* lens,
                            uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base, const uint64_t* caps,
                            hbx_file_summary* sums, const uint64_t* expect_first, const uint8_t* expect_ids,
                            hbx_chain_match* match) {
  if (!c) return HBX_ERR_ARG;
  if (!expect_first) return hbx_submit_device(c, d_arena, n, offs, lens, cut_ends, ids, out_base, caps, sums);
  if (n && (!d_arena || !offs || !lens)) return HBX_ERR_ARG;
  bool vo = false;
  if (int rc = match_args(n, cut_ends, ids, out_base, caps, expect_first, expect_ids, match, &vo)) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  HBX_TRY(c, hipSetDevice(c->device));
  const MatchIn mi{expect_first, expect_ids, match, vo};
  return submit_batch(c, d_arena, n, offs, lens, cut_ends, ids, out_base, caps, sums,
                      c->md5_slice ? c->md5_slice : kBudgetAll, nullptr, nullptr, nullptr, nullptr, &mi);
}

int hbx_match_chains(hbx_ctx* c, uint64_t n, const uint64_t* local_first, const uint8_t* local_ids,
                     const uint64_t* local_cut_ends, const uint64_t* expect_first, const uint8_t* expect_ids,
                     hbx_chain_match* match) {
  if (!c) return HBX_ERR_ARG;
  if (n == 0) return HBX_OK;
  if (!local_first || !expect_first || !match || n > 0x7FFFFFFFull) return HBX_ERR_ARG;
  for (uint64_t f = 0; f < n; f++)
    if (local_first[f + 1] < local_first[f] || expect_first[f + 1] < expect_first[f] ||
        expect_first[f + 1] - expect_first[f] > 0xFFFFFFFFull)
      return HBX_ERR_ARG;
  const uint64_t l0 = local_first[0], nl = local_first[n] - l0, e0 = expect_first[0], ne = expect_first[n] - e0;
  if (nl > 0xFFFFFFFFull || (nl && !local_ids) || (ne && !expect_ids)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  HBX_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->rstream;
  // K12 alone, as hbx_idset_insert runs K9 alone: the lists staged in device memory, firsts rebased to 0
  std::vector<uint64_t> fl(n + 1), fe(n + 1);
  for (uint64_t f = 0; f <= n; f++) {
    fl[f] = local_first[f] - l0;
    fe[f] = expect_first[f] - e0;
  }
  const bool cuts = local_cut_ends && nl;
  HBX_TRY(c, c->d_mt[0].ensure((n + 1) * 8));
  HBX_TRY(c, c->d_mt[1].ensure((n + 1) * 8));
  HBX_TRY(c, c->d_mt[2].ensure(nl * 16));
  HBX_TRY(c, c->d_mt[3].ensure(ne * 16));
  if (cuts) HBX_TRY(c, c->d_mt[4].ensure(nl * 8));
  HBX_TRY(c, c->d_mtout.ensure(n * sizeof(hbx_chain_match)));
  HBX_TRY(c, hipMemcpyAsync(c->d_mt[0].p, fl.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  HBX_TRY(c, hipMemcpyAsync(c->d_mt[1].p, fe.data(), (n + 1) * 8, hipMemcpyHostToDevice, s));
  if (nl) HBX_TRY(c, hipMemcpyAsync(c->d_mt[2].p, local_ids + 16 * l0, nl * 16, hipMemcpyHostToDevice, s));
  if (ne) HBX_TRY(c, hipMemcpyAsync(c->d_mt[3].p, expect_ids + 16 * e0, ne * 16, hipMemcpyHostToDevice, s));
  if (cuts) HBX_TRY(c, hipMemcpyAsync(c->d_mt[4].p, local_cut_ends + l0, nl * 8, hipMemcpyHostToDevice, s));
  const hbxm::Args ma{hbxd::Ids{c->d_mt[2].as<uint4>(), c->d_mt[0].as<uint64_t>(), nullptr, (uint32_t)nl, (uint32_t)n},
                      cuts ? c->d_mt[4].as<uint64_t>() : nullptr, c->d_mt[1].as<uint64_t>(), c->d_mt[3].as<uint4>(),
                      c->d_mtout.as<uint4>()};
  HBX_TRY(c, hbxm::match(s, ma));
  HBX_TRY(c, hipMemcpyAsync(match, c->d_mtout.p, n * sizeof(hbx_chain_match), hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  return HBX_OK;
}

int hbx_locate_ids(hbx_ctx* c, uint64_t nf, const uint64_t* pool_first, const uint8_t* pool_ids,
                   const uint64_t* pool_cut_ends, uint64_t nw, const uint8_t* want_ids, hbx_block_loc* loc,
                   uint64_t* n_found) {
  if (!c) return HBX_ERR_ARG;
  if (nf > 0x7FFFFFFFull || nw > 0xFFFFFFFFull || (nf && !pool_first) || (nw && (!want_ids || !loc)))
    return HBX_ERR_ARG;
  for (uint64_t f = 0; f < nf; f++)
    if (pool_first[f + 1] < pool_first[f]) return HBX_ERR_ARG;
  const uint64_t p0 = nf ? pool_first[0] : 0, np = nf ? pool_first[nf] - p0 : 0;
  if (np > hbxd::kMaxMark || (np && (!pool_ids || !pool_cut_ends))) return HBX_ERR_ARG;
  if (nw == 0) {
    if (n_found) *n_found = 0;
    return HBX_OK;
  }
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  HBX_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->rstream;
  // K13 alone, as hbx_match_chains runs K12 alone: the lists staged in device memory, firsts rebased to 0
  std::vector<uint64_t> first(nf + 1, 0);
  for (uint64_t f = 0; f <= nf && nf; f++) first[f] = pool_first[f] - p0;
  const uint64_t slots = hbxd::table_slots(np);
  HBX_TRY(c, c->d_lc[0].ensure(np * 16));
  HBX_TRY(c, c->d_lc[1].ensure(np * 8));
  HBX_TRY(c, c->d_lc[2].ensure((nf + 1) * 8));
  HBX_TRY(c, c->d_lc[3].ensure(nw * 16));
  HBX_TRY(c, c->d_lc[4].ensure(slots * sizeof(uint32_t)));
  HBX_TRY(c, c->d_lc[5].ensure(nw * sizeof(hbx_block_loc) + 8));
  if (np) {
    HBX_TRY(c, hipMemcpyAsync(c->d_lc[0].p, pool_ids + 16 * p0, np * 16, hipMemcpyHostToDevice, s));
    HBX_TRY(c, hipMemcpyAsync(c->d_lc[1].p, pool_cut_ends + p0, np * 8, hipMemcpyHostToDevice, s));
  }
  HBX_TRY(c, hipMemcpyAsync(c->d_lc[2].p, first.data(), (nf + 1) * 8, hipMemcpyHostToDevice, s));
  HBX_TRY(c, hipMemcpyAsync(c->d_lc[3].p, want_ids, nw * 16, hipMemcpyHostToDevice, s));
  unsigned long long* d_found =
      reinterpret_cast<unsigned long long*>(c->d_lc[5].as<uint8_t>() + nw * sizeof(hbx_block_loc));
  const hbxl::Args la{c->d_lc[0].as<uint4>(), c->d_lc[1].as<uint64_t>(), c->d_lc[2].as<uint64_t>(),
                      c->d_lc[3].as<uint4>(), c->d_lc[4].as<uint32_t>(), c->d_lc[5].as<uint4>(), d_found,
                      (uint32_t)np, (uint32_t)nw, (uint32_t)nf, (uint32_t)(slots - 1)};
  HBX_TRY(c, hbxl::locate(s, la));
  unsigned long long found = 0;
  HBX_TRY(c, hipMemcpyAsync(loc, c->d_lc[5].p, nw * sizeof(hbx_block_loc), hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipMemcpyAsync(&found, d_found, sizeof(found), hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  if (n_found) *n_found = found;
  return HBX_OK;
}

// ---- K15: the block graph (DESIGN.md §5 "K15", hbx_graph.hip) --------------
namespace {
// hbx_ctx::d_bg
enum {
  kBgIds, kBgNLinks, kBgBase, kBgBad, kBgLinks, kBgRoots, kBgTable, kBgRep, kBgLinkRow, kBgRootRow, kBgMark,
  kBgFault, kBgFrontier, kBgCounts, kBgRend, kBgRsrc, kBgBufs
};
static_assert(kBgBufs == 16, "hbx_ctx::d_bg");

// One sweep from the frontier in front[0] (n_front rows at depth 0), a launch
// per level; *levels = the levels that held a row.
int bg_sweep(hbx_ctx* c, hipStream_t s, const hbxg::Graph& g, uint32_t* depth, uint32_t* front[2], uint64_t n_front,
             unsigned long long* d_cnt, uint64_t n, uint64_t* levels) {
  uint32_t level = 0;
  *levels = 0;
  while (n_front && level <= n) {  // (a level claims at least one row: at most n levels)
    *levels = (uint64_t)level + 1;
    HBX_TRY(c, hipMemsetAsync(d_cnt, 0, sizeof(unsigned long long), s));
    const hbxg::ExpandArgs ea{g, front[level & 1], n_front, depth, level, front[(level + 1) & 1], d_cnt, n};
    hipLaunchKernelGGL(hbx_k15_expand, dim3(hbxg::grid(n_front, c->k15_wgs)), dim3(hbxg::kThreads), 0, s, ea);
    HBX_TRY(c, hipGetLastError());
    unsigned long long next = 0;
    HBX_TRY(c, hipMemcpyAsync(&next, d_cnt, sizeof(next), hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
    n_front = std::min<uint64_t>(next, n);
    level++;
  }
  return HBX_OK;
}
}  // namespace

static_assert(sizeof(hbx_graph_summary) == 96, "hbx_graph_summary is twelve uint64");

int hbx_block_graph(hbx_ctx* c, uint64_t n, const uint8_t* ids, const uint32_t* n_links, const uint64_t* link_base,
                    uint64_t m, const uint8_t* links, const uint8_t* bad, uint64_t n_roots, const uint8_t* root_ids,
                    uint32_t* rep, uint32_t* link_row, uint32_t* root_row, uint32_t* mark_depth,
                    uint32_t* fault_depth, hbx_graph_summary* sum) {
  if (!c || !sum) return HBX_ERR_ARG;
  if (n > 0x7FFFFFFFull || (n && (!ids || !n_links || !link_base)) || (m && !links) || (n_roots && !root_ids))
    return HBX_ERR_ARG;
  uint64_t sum_links = 0;  // bounds the transposed graph
  for (uint64_t i = 0; i < n; i++) {
    if (link_base[i] > m || n_links[i] > m - link_base[i]) return HBX_ERR_ARG;
    sum_links += n_links[i];
  }
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  std::memset(sum, 0, sizeof(*sum));
  sum->n_rows = n;
  sum->n_links = m;
  sum->n_roots = n_roots;
  if (n == 0) {  // nothing to look anything up in
    if (link_row) std::fill(link_row, link_row + m, hbxg::kNone);
    if (root_row) std::fill(root_row, root_row + n_roots, hbxg::kNone);
    sum->n_missing_links = m;
    sum->n_roots_missing = n_roots;
    return HBX_OK;
  }
  HBX_TRY(c, hipSetDevice(c->device));
  hipStream_t s = c->rstream;
  const bool run_mark = mark_depth || n_roots, run_tree = fault_depth != nullptr;
  const uint64_t slots = hbxd::table_slots(n), chunks = (n + hbxg::kScanChunk - 1) / hbxg::kScanChunk;
  size_t need[kBgBufs] = {};
  need[kBgIds] = n * 16;
  need[kBgNLinks] = n * 4;
  need[kBgBase] = n * 8;
  need[kBgBad] = bad ? n : 0;
  need[kBgLinks] = m * 16;
  need[kBgRoots] = n_roots * 16;
  need[kBgTable] = slots * sizeof(uint32_t);
  need[kBgRep] = n * 4;
  need[kBgLinkRow] = m * 4;
  need[kBgRootRow] = n_roots * 4;
  need[kBgMark] = run_mark ? n * 4 : 0;
  need[kBgFault] = run_tree ? n * 4 : 0;
  need[kBgFrontier] = 2 * n * 4;
  need[kBgCounts] = hbxg::kCntWords * sizeof(unsigned long long);
  // (the transposed graph is sized when a faulty row turns up)
  auto fits = [&](std::initializer_list<int> which) -> int {
    uint64_t grow = 0;
    for (int b : which)
      if (need[b] > c->d_bg[b].cap) grow += need[b] + 4096 - c->d_bg[b].cap;
    size_t fr = 0, tot = 0;
    HBX_TRY(c, hipMemGetInfo(&fr, &tot));
    if (grow > fr)
      return c->fail(HBX_ERR_CAPACITY, "hbx_block_graph: the table needs " + std::to_string(grow) +
                                           " more bytes of device memory, " + std::to_string(fr) + " are free");
    for (int b : which) HBX_TRY(c, c->d_bg[b].ensure(need[b]));
    return HBX_OK;
  };
  if (int rc = fits({kBgIds, kBgNLinks, kBgBase, kBgBad, kBgLinks, kBgRoots, kBgTable, kBgRep, kBgLinkRow, kBgRootRow,
                     kBgMark, kBgFault, kBgFrontier, kBgCounts}))
    return rc;
  const uint4* d_ids = c->d_bg[kBgIds].as<uint4>();
  const uint32_t* d_nl = c->d_bg[kBgNLinks].as<uint32_t>();
  const uint64_t* d_base = c->d_bg[kBgBase].as<uint64_t>();
  const uint8_t* d_bad = bad ? c->d_bg[kBgBad].as<uint8_t>() : nullptr;
  uint32_t* d_table = c->d_bg[kBgTable].as<uint32_t>();
  uint32_t* d_rep = c->d_bg[kBgRep].as<uint32_t>();
  uint32_t* d_lrow = c->d_bg[kBgLinkRow].as<uint32_t>();
  uint32_t* d_rrow = c->d_bg[kBgRootRow].as<uint32_t>();
  uint32_t* d_mark = run_mark ? c->d_bg[kBgMark].as<uint32_t>() : nullptr;
  uint32_t* d_fault = run_tree ? c->d_bg[kBgFault].as<uint32_t>() : nullptr;
  uint32_t* front[2] = {c->d_bg[kBgFrontier].as<uint32_t>(), c->d_bg[kBgFrontier].as<uint32_t>() + n};
  unsigned long long* d_cnt = c->d_bg[kBgCounts].as<unsigned long long>();
  const uint32_t wgs = c->k15_wgs, mask = (uint32_t)(slots - 1);
  const dim3 block(hbxg::kThreads);
  // the frontier's length after the launch that filled it
  auto frontier_len = [&](uint64_t* len) -> int {
    unsigned long long v = 0;
    HBX_TRY(c, hipMemcpyAsync(&v, d_cnt + hbxg::kCntFrontier, sizeof(v), hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
    *len = std::min<uint64_t>(v, n);
    return HBX_OK;
  };
  const int rc = [&]() -> int {
    HBX_TRY(c, hipMemcpyAsync(c->d_bg[kBgIds].p, ids, n * 16, hipMemcpyHostToDevice, s));
    HBX_TRY(c, hipMemcpyAsync(c->d_bg[kBgNLinks].p, n_links, n * 4, hipMemcpyHostToDevice, s));
    HBX_TRY(c, hipMemcpyAsync(c->d_bg[kBgBase].p, link_base, n * 8, hipMemcpyHostToDevice, s));
    if (bad) HBX_TRY(c, hipMemcpyAsync(c->d_bg[kBgBad].p, bad, n, hipMemcpyHostToDevice, s));
    if (m) HBX_TRY(c, hipMemcpyAsync(c->d_bg[kBgLinks].p, links, m * 16, hipMemcpyHostToDevice, s));
    if (n_roots) HBX_TRY(c, hipMemcpyAsync(c->d_bg[kBgRoots].p, root_ids, n_roots * 16, hipMemcpyHostToDevice, s));
    HBX_TRY(c, hipMemsetAsync(d_cnt, 0, hbxg::kCntWords * sizeof(unsigned long long), s));
    // 1. the table: K13's build over the rows' IDs as they are
    HBX_TRY(c, hipMemsetAsync(d_table, 0, slots * sizeof(uint32_t), s));
    const hbxl::Args la{d_ids, nullptr, nullptr, nullptr, d_table, nullptr, nullptr, (uint32_t)n, 0u, 0u, mask};
    hipLaunchKernelGGL(hbx_k13_build, dim3((uint32_t)((n + hbxl::kThreads - 1) / hbxl::kThreads)),
                       dim3(hbxl::kThreads), 0, s, la);
    HBX_TRY(c, hipGetLastError());
    // 2. resolve: the rows' own IDs (rep), the links, the roots
    const hbxg::ResolveArgs rs[3] = {
        {d_ids, d_table, d_ids, d_rep, d_cnt + hbxg::kCntAlias, n, (uint32_t)n, mask, 1u},
        {d_ids, d_table, c->d_bg[kBgLinks].as<uint4>(), d_lrow, d_cnt + hbxg::kCntMissLinks, m, (uint32_t)n, mask, 0u},
        {d_ids, d_table, c->d_bg[kBgRoots].as<uint4>(), d_rrow, d_cnt + hbxg::kCntMissRoots, n_roots, (uint32_t)n,
         mask, 0u}};
    for (const hbxg::ResolveArgs& ra : rs)
      if (ra.n_keys) hipLaunchKernelGGL(hbx_k15_resolve, dim3(hbxg::grid(ra.n_keys, wgs)), block, 0, s, ra);
    HBX_TRY(c, hipGetLastError());
    const hbxg::Graph fwd{d_base, d_nl, nullptr, d_lrow};
    // 3. mark: the roots at depth 0, then a launch per level
    if (run_mark) {
      HBX_TRY(c, hipMemsetAsync(d_mark, 0xFF, n * 4, s));
      uint64_t n_front = 0;
      if (n_roots) {
        const hbxg::RootArgs ra{d_rrow, n_roots, d_mark, front[0], d_cnt + hbxg::kCntFrontier, n};
        hipLaunchKernelGGL(hbx_k15_roots, dim3(hbxg::grid(n_roots, wgs)), block, 0, s, ra);
        HBX_TRY(c, hipGetLastError());
        if (int e = frontier_len(&n_front)) return e;
      }
      if (int e = bg_sweep(c, s, fwd, d_mark, front, n_front, d_cnt + hbxg::kCntFrontier, n, &sum->mark_levels)) return e;
    }
    // 4. tree check: the faulty rows at depth 0; only with one of them the transposed graph and its sweep
    if (run_tree) {
      HBX_TRY(c, hipMemsetAsync(d_fault, 0xFF, n * 4, s));
      HBX_TRY(c, hipMemsetAsync(d_cnt + hbxg::kCntFrontier, 0, sizeof(unsigned long long), s));
      hbxg::RowArgs wa{fwd, d_rep, d_bad, d_fault, front[0], d_cnt + hbxg::kCntFrontier, nullptr, nullptr, n, (uint32_t)n};
      hipLaunchKernelGGL(hbx_k15_seed, dim3(hbxg::grid(n, wgs)), block, 0, s, wa);
      HBX_TRY(c, hipGetLastError());
      if (int e = frontier_len(&sum->n_faulty)) return e;
      if (sum->n_faulty) {
        need[kBgRend] = (n + chunks) * 8;
        need[kBgRsrc] = sum_links * 4;
        if (int e = fits({kBgRend, kBgRsrc})) return e;
        unsigned long long* d_rend = c->d_bg[kBgRend].as<unsigned long long>();
        unsigned long long* d_sums = d_rend + n;
        HBX_TRY(c, hipMemsetAsync(d_rend, 0, n * 8, s));
        wa.cursor = d_rend;
        wa.rsrc = c->d_bg[kBgRsrc].as<uint32_t>();
        wa.cap = sum_links;
        hipLaunchKernelGGL(hbx_k15_indeg, dim3(hbxg::grid(n, wgs)), block, 0, s, wa);
        hipLaunchKernelGGL(hbx_k15_scan_sums, dim3((uint32_t)chunks), block, 0, s, d_rend, n, d_sums);
        hipLaunchKernelGGL(hbx_k15_scan_top, dim3(1), block, 0, s, d_sums, chunks);
        hipLaunchKernelGGL(hbx_k15_scan_add, dim3((uint32_t)chunks), block, 0, s, d_rend, n, d_sums);
        hipLaunchKernelGGL(hbx_k15_fill, dim3(hbxg::grid(n, wgs)), block, 0, s, wa);
        HBX_TRY(c, hipGetLastError());
        const hbxg::Graph back{nullptr, nullptr, reinterpret_cast<const uint64_t*>(d_rend), wa.rsrc};
        if (int e = bg_sweep(c, s, back, d_fault, front, sum->n_faulty, d_cnt + hbxg::kCntFrontier, n,
                             &sum->fault_levels))
          return e;
      }
    }
    // 5. finish: the aliases' depths, the counts
    if (run_mark || run_tree) {
      const hbxg::FinishArgs fa{d_rep, d_mark, d_fault, d_cnt, (uint32_t)n};
      hipLaunchKernelGGL(hbx_k15_finish, dim3(hbxg::grid(n, wgs)), block, 0, s, fa);
      HBX_TRY(c, hipGetLastError());
    }
    unsigned long long cnt[hbxg::kCntWords] = {};
    if (rep) HBX_TRY(c, hipMemcpyAsync(rep, d_rep, n * 4, hipMemcpyDeviceToHost, s));
    if (link_row && m) HBX_TRY(c, hipMemcpyAsync(link_row, d_lrow, m * 4, hipMemcpyDeviceToHost, s));
    if (root_row && n_roots) HBX_TRY(c, hipMemcpyAsync(root_row, d_rrow, n_roots * 4, hipMemcpyDeviceToHost, s));
    if (mark_depth) HBX_TRY(c, hipMemcpyAsync(mark_depth, d_mark, n * 4, hipMemcpyDeviceToHost, s));
    if (fault_depth) HBX_TRY(c, hipMemcpyAsync(fault_depth, d_fault, n * 4, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipMemcpyAsync(cnt, d_cnt, sizeof(cnt), hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
    sum->n_alias = cnt[hbxg::kCntAlias];
    sum->n_missing_links = cnt[hbxg::kCntMissLinks];
    sum->n_roots_missing = cnt[hbxg::kCntMissRoots];
    sum->n_marked = cnt[hbxg::kCntMarked];
    sum->n_invalid = cnt[hbxg::kCntInvalid];
    sum->n_marked_faulty = cnt[hbxg::kCntMarkedFaulty];
    return HBX_OK;
  }();
  if (rc != HBX_OK) {  // leave the stream idle and the error state clean: the context stays usable
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
  }
  return rc;
}

int hbx_wait(hbx_ctx* c) {
  if (!c) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HBX_TRY(c, hipSetDevice(c->device));
  return wait_oldest(c);
}

int hbx_pending(hbx_ctx* c) {
  if (!c) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return (int)c->pending.size();
}

// ---- K9: the set of block IDs (DESIGN.md §5 "K9", hbx_dedup.hip) ----------
namespace {
constexpr uint64_t kIdsetCallChunk = 1ull << 22;  // IDs per mark of a direct call: 64 MiB of staging at most

// count and dropped as the device holds them (waits for the result stream).
int idset_count(hbx_ctx* c, hbx_idset* t, uint64_t* count, uint64_t* dropped) {
  uint32_t ctl[4] = {0, 0, 0, 0};
  HBX_TRY(c, hipMemcpyAsync(ctl, t->d_ctl.p, sizeof(ctl), hipMemcpyDeviceToHost, c->rstream));
  HBX_TRY(c, hipStreamSynchronize(c->rstream));
  if (count) *count = std::min<uint64_t>(ctl[0], t->capacity);
  if (dropped) *dropped = (uint64_t)ctl[2] | ((uint64_t)ctl[3] << 32);
  return HBX_OK;
}

// Keep the first m keys: count = m, the slot table cleared and rebuilt from them.
int idset_truncate(hbx_ctx* c, hbx_idset* t, uint64_t m) {
  uint64_t count = 0;
  if (int rc = idset_count(c, t, &count, nullptr)) return rc;
  if (m > count) return c->fail(HBX_ERR_ARG, "hbx_idset_truncate: the set holds fewer IDs");
  if (m == count) return HBX_OK;
  hipStream_t s = c->rstream;
  const uint32_t m32 = (uint32_t)m;
  HBX_TRY(c, hipMemcpyAsync(t->d_ctl.p, &m32, 4, hipMemcpyHostToDevice, s));
  HBX_TRY(c, hipMemsetAsync(t->d_slots.p, 0, t->slots * sizeof(uint32_t), s));
  if (m32) {
    hipLaunchKernelGGL(hbx_k9_rebuild, dim3((m32 + hbxd::kThreads - 1) / hbxd::kThreads), dim3(hbxd::kThreads), 0, s,
                       t->view(), m32);
    HBX_TRY(c, hipGetLastError());
  }
  HBX_TRY(c, hipStreamSynchronize(s));  // (m32 is read by the copy above)
  return HBX_OK;
}

// The checks every direct call shares; the context's lock is held.
int idset_direct(hbx_ctx* c, hbx_idset* t) {
  if (std::find(c->idsets.begin(), c->idsets.end(), t) == c->idsets.end())
    return c->fail(HBX_ERR_ARG, "not an ID set of this context");
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  return c->hip(hipSetDevice(c->device), "hipSetDevice");
}
}  // namespace

uint64_t hbx_idset_slots(uint64_t capacity) { return hbxd::table_slots(capacity); }

int hbx_idset_create(hbx_ctx* c, uint64_t capacity, hbx_idset** out) {
  if (!c || !out) return HBX_ERR_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> g(c->mu);
  const uint64_t S = hbxd::table_slots(capacity);
  if (capacity == 0 || S == 0) return c->fail(HBX_ERR_ARG, "hbx_idset_create: capacity must be 1..2^31");
  HBX_TRY(c, hipSetDevice(c->device));
  hbx_idset* t = new hbx_idset();
  t->capacity = capacity;
  t->slots = S;
  int rc = HBX_OK;
  for (hipError_t e : {t->d_keys.ensure(capacity * 16), t->d_slots.ensure(S * sizeof(uint32_t)), t->d_ctl.ensure(256)})
    if (e != hipSuccess && !rc) rc = c->hip(e, "hbx_idset_create");
  if (!rc) rc = c->hip(hipMemsetAsync(t->d_slots.p, 0, S * sizeof(uint32_t), c->rstream), "hbx_idset_create");
  if (!rc) rc = c->hip(hipMemsetAsync(t->d_ctl.p, 0, 256, c->rstream), "hbx_idset_create");
  if (!rc) rc = c->hip(hipStreamSynchronize(c->rstream), "hbx_idset_create");
  if (rc) {
    (void)hipGetLastError();
    t->release();
    delete t;
    return rc;
  }
  c->idsets.push_back(t);
  *out = t;
  return HBX_OK;
}

int hbx_idset_destroy(hbx_ctx* c, hbx_idset* t) {
  if (!c || !t) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = std::find(c->idsets.begin(), c->idsets.end(), t);
  if (it == c->idsets.end()) return c->fail(HBX_ERR_ARG, "not an ID set of this context");
  // (a broken context never collects: its batches are parked until destroy)
  if (t->inflight && !c->broken) return c->fail(HBX_ERR_STATE, "pending batches still use the ID set");
  HBX_TRY(c, hipSetDevice(c->device));
  HBX_TRY(c, hipStreamSynchronize(c->rstream));
  c->idsets.erase(it);
  t->release();
  delete t;
  return HBX_OK;
}

int hbx_idset_insert(hbx_ctx* c, hbx_idset* t, uint64_t n, const uint8_t* ids, uint8_t* fresh) {
  if (!c || !t || (n && !ids)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = idset_direct(c, t)) return rc;
  hipStream_t s = c->rstream;
  // one mark per chunk of the list, in order: a later chunk finds what an
  // earlier one inserted
  for (uint64_t at = 0; at < n; at += kIdsetCallChunk) {
    const uint64_t k = std::min(kIdsetCallChunk, n - at);
    HBX_TRY(c, t->d_in.ensure(k * 16));
    HBX_TRY(c, t->d_flag.ensure(k));
    HBX_TRY(c, t->d_scratch.ensure(hbxd::table_slots(k) * sizeof(uint32_t)));
    HBX_TRY(c, hipMemcpyAsync(t->d_in.p, ids + 16 * at, k * 16, hipMemcpyHostToDevice, s));
    const hbxd::Ids in{t->d_in.as<uint4>(), nullptr, nullptr, (uint32_t)k, 0u};
    HBX_TRY(c, hbxd::mark(s, t->view(), in, t->d_scratch.as<uint32_t>(), t->d_flag.as<uint8_t>()));
    if (fresh) HBX_TRY(c, hipMemcpyAsync(fresh + at, t->d_flag.p, k, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
  }
  return HBX_OK;
}

int hbx_idset_contains(hbx_ctx* c, hbx_idset* t, uint64_t n, const uint8_t* ids, uint8_t* found) {
  if (!c || !t || (n && (!ids || !found))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = idset_direct(c, t)) return rc;
  hipStream_t s = c->rstream;
  for (uint64_t at = 0; at < n; at += kIdsetCallChunk) {
    const uint64_t k = std::min(kIdsetCallChunk, n - at);
    HBX_TRY(c, t->d_in.ensure(k * 16));
    HBX_TRY(c, t->d_flag.ensure(k));
    HBX_TRY(c, hipMemcpyAsync(t->d_in.p, ids + 16 * at, k * 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(hbx_k9_contains, dim3((uint32_t)((k + hbxd::kThreads - 1) / hbxd::kThreads)),
                       dim3(hbxd::kThreads), 0, s, t->view(), static_cast<const uint4*>(t->d_in.as<uint4>()),
                       (uint32_t)k, t->d_flag.as<uint8_t>());
    HBX_TRY(c, hipGetLastError());
    HBX_TRY(c, hipMemcpyAsync(found + at, t->d_flag.p, k, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
  }
  return HBX_OK;
}

int hbx_idset_stats(hbx_ctx* c, hbx_idset* t, uint64_t* count, uint64_t* capacity, uint64_t* slots,
                    uint64_t* dropped) {
  if (!c || !t) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = idset_direct(c, t)) return rc;
  if (capacity) *capacity = t->capacity;
  if (slots) *slots = t->slots;
  return idset_count(c, t, count, dropped);
}

int hbx_idset_export(hbx_ctx* c, hbx_idset* t, uint8_t* ids, uint64_t cap, uint64_t* n) {
  if (!c || !t || !n) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = idset_direct(c, t)) return rc;
  uint64_t count = 0;
  if (int rc = idset_count(c, t, &count, nullptr)) return rc;
  *n = count;
  if (count > cap) return c->fail(HBX_ERR_CAPACITY, "hbx_idset_export: the set holds " + std::to_string(count) + " IDs");
  if (count && !ids) return c->fail(HBX_ERR_ARG, "hbx_idset_export: null output");
  if (count) {
    HBX_TRY(c, hipMemcpyAsync(ids, t->d_keys.p, count * 16, hipMemcpyDeviceToHost, c->rstream));
    HBX_TRY(c, hipStreamSynchronize(c->rstream));
  }
  return HBX_OK;
}

int hbx_idset_truncate(hbx_ctx* c, hbx_idset* t, uint64_t count) {
  if (!c || !t) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = idset_direct(c, t)) return rc;
  return idset_truncate(c, t, count);
}

// ---- files larger than a batch: segments (DESIGN.md "Segmented files") ----
int hbx_seg_next(uint64_t file_len, uint64_t seg_bytes, uint64_t prev_end, uint64_t* off, uint64_t* len) {
  if (!off || !len) return HBX_ERR_ARG;
  if (seg_bytes < HBX_SEG_MIN_BYTES || seg_bytes % HBX_ARENA_ALIGN) return HBX_ERR_ARG;
  if (prev_end > 0 && (prev_end >= file_len || prev_end < HBX_SEG_OVERLAP)) return HBX_ERR_ARG;  // nothing is left
  const uint64_t o = prev_end ? prev_end - HBX_SEG_OVERLAP : 0;
  *off = o;
  *len = std::min(seg_bytes, file_len - o);
  return HBX_OK;
}

int hbx_seg_open(hbx_ctx* c, uint64_t file_len, hbx_seg** out) {
  if (!c || !out) return HBX_ERR_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  HBX_TRY(c, hipSetDevice(c->device));
  if (!c->sstream) HBX_TRY(c, hipStreamCreateWithFlags(&c->sstream, hipStreamNonBlocking));
  if (c->seg_words_free.empty()) {  // 512 more carry words
    c->seg_words.emplace_back();
    DevBuf& blk = c->seg_words.back();
    if (int rc = c->hip(blk.ensure(4096), "carry words")) {
      c->seg_words.pop_back();
      return rc;
    }
    for (int i = 511; i >= 0; i--) c->seg_words_free.push_back(blk.as<uint64_t>() + i);
  }
  hbx_seg* h = new hbx_seg();
  h->file_len = file_len;
  h->d_carry = c->seg_words_free.back();  // (never read before a K2 of this file has written it)
  c->seg_words_free.pop_back();
  c->segs_open.push_back(h);
  *out = h;
  return HBX_OK;
}

int hbx_seg_close(hbx_ctx* c, hbx_seg* h) {
  if (!c || !h) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = std::find(c->segs_open.begin(), c->segs_open.end(), h);
  if (it == c->segs_open.end()) return c->fail(HBX_ERR_ARG, "not an open segmented file of this context");
  // (a broken context never collects: its batches are parked until destroy)
  if (h->inflight && !c->broken) return c->fail(HBX_ERR_STATE, "a segment of the file is still pending");
  c->segs_open.erase(it);
  // with nothing pending every K2 that touched the word has completed
  if (!h->inflight) c->seg_words_free.push_back(h->d_carry);
  delete h;
  return HBX_OK;
}

namespace {
// Validate one batch of segments against their handles and enqueue it; the
// handles advance only once the batch is in the FIFO.
int seg_submit(hbx_ctx* c, uint64_t n, hbx_seg* const* segs, const void* d_arena, const uint64_t* arena_offs,
               const uint64_t* seg_lens, uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base,
               const uint64_t* caps, hbx_file_summary* sums, uint32_t budget, hbx_idset* set = nullptr,
               uint8_t* fresh = nullptr) {
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  std::vector<uint64_t> seg_offs(n);
  for (uint64_t f = 0; f < n; f++) {
    hbx_seg* h = segs[f];
    if (!h || std::find(c->segs_open.begin(), c->segs_open.end(), h) == c->segs_open.end())
      return c->fail(HBX_ERR_ARG, "segment " + std::to_string(f) + ": not an open segmented file of this context");
    for (uint64_t g = 0; g < f; g++)
      if (segs[g] == h) return c->fail(HBX_ERR_ARG, "two segments of one file in a batch");
    if (h->final_sent) return c->fail(HBX_ERR_STATE, "segment " + std::to_string(f) + ": the file's final segment was already submitted");
    const uint64_t off = h->any ? h->end - HBX_SEG_OVERLAP : 0, L = seg_lens[f];
    seg_offs[f] = off;
    if (L > h->file_len - off) return c->fail(HBX_ERR_ARG, "segment " + std::to_string(f) + ": longer than the rest of the file");
    const bool final = off + L == h->file_len;
    if (!final && (L < HBX_SEG_MIN_BYTES || L % HBX_ARENA_ALIGN))
      return c->fail(HBX_ERR_ARG, "segment " + std::to_string(f) +
                                      ": a non-final segment is at least HBX_SEG_MIN_BYTES and a multiple of HBX_ARENA_ALIGN");
    if (caps[f] < max_chunks(L))
      return c->fail(HBX_ERR_CAPACITY, "segment " + std::to_string(f) + ": caps below hbx_max_chunks(seg_len)");
  }
  int rc = submit_batch(c, d_arena, n, arena_offs, seg_lens, cut_ends, ids, out_base, caps, sums, budget, segs,
                        seg_offs.data(), set, set ? fresh : nullptr);
  if (rc) return rc;
  for (uint64_t f = 0; f < n; f++) {
    hbx_seg* h = segs[f];
    h->any = true;
    h->end = seg_offs[f] + seg_lens[f];
    h->final_sent = h->end == h->file_len;
    h->inflight++;
  }
  return HBX_OK;
}
}  // namespace

int hbx_seg_submit_device(hbx_ctx* c, uint64_t n, hbx_seg* const* segs, const void* d_arena,
                          const uint64_t* arena_offs, const uint64_t* seg_lens, uint64_t* cut_ends, uint8_t* ids,
                          const uint64_t* out_base, const uint64_t* caps, hbx_file_summary* sums) {
  return hbx_seg_submit_device_dd(c, n, segs, d_arena, arena_offs, seg_lens, cut_ends, ids, out_base, caps, sums,
                                  nullptr, nullptr);
}

int hbx_seg_submit_device_dd(hbx_ctx* c, uint64_t n, hbx_seg* const* segs, const void* d_arena,
                             const uint64_t* arena_offs, const uint64_t* seg_lens, uint64_t* cut_ends, uint8_t* ids,
                             const uint64_t* out_base, const uint64_t* caps, hbx_file_summary* sums, hbx_idset* set,
                             uint8_t* fresh) {
  if (!c) return HBX_ERR_ARG;
  if (!n || !segs || !d_arena || !arena_offs || !seg_lens || !out_base || !caps) return HBX_ERR_ARG;
  if (set && !fresh) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (set && std::find(c->idsets.begin(), c->idsets.end(), set) == c->idsets.end())
    return c->fail(HBX_ERR_ARG, "not an ID set of this context");
  HBX_TRY(c, hipSetDevice(c->device));
  return seg_submit(c, n, segs, d_arena, arena_offs, seg_lens, cut_ends, ids, out_base, caps, sums,
                    c->md5_slice ? c->md5_slice : kBudgetAll, set, fresh);
}

int hbx_chunk_hash_batch(hbx_ctx* c, uint64_t n, const uint8_t* const* datas,
                         const uint64_t* lens, uint64_t* cut_ends, uint8_t* ids,
                         const uint64_t* out_base, const uint64_t* caps,
                         hbx_file_summary* sums) {
  if (!c) return HBX_ERR_ARG;
  if (n && (!datas || !lens || !out_base || !caps)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  std::vector<uint64_t> offs(n);
  uint64_t total = 0;
  for (uint64_t f = 0; f < n; f++) {
    offs[f] = total;
    total += (lens[f] + 255) & ~uint64_t(255);
  }
  HBX_TRY(c, c->d_stage.ensure(total + 65536));
  uint8_t* arena = c->d_stage.as<uint8_t>();
  for (uint64_t f = 0; f < n; f++) {
    if (lens[f] && !datas[f]) return c->fail(HBX_ERR_ARG, "null file data");
    if (lens[f])
      HBX_TRY(c, hipMemcpyAsync(arena + offs[f], datas[f], lens[f], hipMemcpyHostToDevice,
                                c->stream));
  }
  return run_device_sync(c, arena, n, offs.data(), lens, cut_ends, ids, out_base, caps, sums);
}

int hbx_chunk_hash(hbx_ctx* c, const uint8_t* data, uint64_t len, uint64_t* cut_ends,
                   uint8_t* ids, uint64_t cap, uint64_t* n_chunks) {
  if (!c || (len && !data)) return HBX_ERR_ARG;
  const uint64_t base = 0;
  hbx_file_summary s{};
  int rc = hbx_chunk_hash_batch(c, 1, &data, &len, cut_ends, ids, &base, &cap, &s);
  // the count is meaningful on success and on HBX_ERR_CAPACITY (the caller
  // retries with that many slots); otherwise it is left untouched
  if (n_chunks && (rc == HBX_OK || rc == HBX_ERR_CAPACITY)) *n_chunks = s.n_chunks;
  return rc;
}

int hbx_block_id(hbx_ctx* c, const uint8_t* links, uint32_t n_links, const uint8_t* data,
                 uint64_t len, uint8_t out[16]) {
  if (!c || !out || (n_links && !links) || (len && !data)) return HBX_ERR_ARG;
  if (len > 0xFFFFFFFFull) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HBX_TRY(c, hipSetDevice(c->device));
  const uint64_t n = 8 + 16ull * n_links + len;
  if (n + 16 + 128 > 0xFFFFFFFFull) return HBX_ERR_ARG;
  return block_id_on(c, c->stream, c->d_msg, links, n_links, data, len, out);
}

// MD5(data) on the device (K5 over the raw message): core.Hash (core.go:46-48),
// the primitive under Hmac/DeepHmac (core.go:51-80), whose KAT rows
// (core_test.go:23-30) tests/test_gpu_parity.py runs through this call.
int hbx_md5(hbx_ctx* c, const uint8_t* data, uint64_t len, uint8_t out[16]) {
  if (!c || !out || (len && !data) || len > 0xFFFFFFFEull - 16ull) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HBX_TRY(c, hipSetDevice(c->device));
  HBX_TRY(c, c->d_msg.ensure(len + 16));
  uint8_t* dm = c->d_msg.as<uint8_t>();
  if (len) HBX_TRY(c, hipMemcpyAsync(dm + 16, data, len, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(hbx_k5_md5_raw, dim3(1), dim3(64), 0, c->stream, dm + 16, (uint32_t)len,
                     reinterpret_cast<uint32_t*>(dm));
  HBX_TRY(c, hipGetLastError());
  HBX_TRY(c, hipMemcpyAsync(out, dm, 16, hipMemcpyDeviceToHost, c->stream));
  HBX_TRY(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

namespace {
// K6 over n blocks whose data is already on the device (block i at
// arena + offs[i]); lanes are ordered longest first so each wave's 64 chains
// are about equally long.  The restore path passes arena = NULL with absolute
// device addresses in offs (its blocks lie in two buffers): the sum is only
// ever turned into an integer address, so that is part of this contract.
// link_addr (the data file path, whose links lie in the device image beside
// the data): block i's links are at that device address and `links` /
// `link_base` are not used.
int verify_device(hbx_ctx* c, const uint8_t* arena, uint64_t n, const uint64_t* offs,
                  const uint64_t* lens, const uint8_t* links, const uint64_t* link_base,
                  const uint32_t* n_links, uint8_t* ids, const uint8_t* expect, uint8_t* ok,
                  uint64_t* n_bad, const uint64_t* link_addr = nullptr) {
  if (n_bad) *n_bad = 0;
  if (n == 0) return HBX_OK;
  if (n > 0xFFFFFFFFull) return c->fail(HBX_ERR_ARG, "too many blocks");
  uint64_t nlinks_total = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint32_t nl = n_links ? n_links[i] : 0u;
    if (nl && !link_addr && (!links || !link_base)) return c->fail(HBX_ERR_ARG, "links missing");
    if (lens[i] + 8ull + 16ull * nl + 128ull > 0xFFFFFFFFull) return c->fail(HBX_ERR_ARG, "block too large");
    if (nl && !link_addr) nlinks_total = std::max(nlinks_total, link_base[i] + nl);
  }
  std::vector<uint32_t> perm(n);
  for (uint64_t i = 0; i < n; i++) perm[i] = (uint32_t)i;
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return lens[a] > lens[b]; });
  HBX_TRY(c, c->d_vdesc.ensure(n * sizeof(VerifyDesc)));
  HBX_TRY(c, c->d_vlinks.ensure(std::max<uint64_t>(16 * nlinks_total, 16)));
  HBX_TRY(c, c->d_vout.ensure(n * 17));
  HBX_TRY(c, c->d_zeros.ensure(256));
  if (expect) HBX_TRY(c, c->d_vexp.ensure(n * 16));
  const uint8_t* dl = c->d_vlinks.as<uint8_t>();
  std::vector<VerifyDesc> desc(n);
  std::vector<uint8_t> exp_p(expect ? n * 16 : 0);
  for (uint64_t k = 0; k < n; k++) {
    const uint32_t i = perm[k];
    const uint32_t nl = n_links ? n_links[i] : 0u;
    desc[k].src = reinterpret_cast<uint64_t>(arena) + offs[i];
    desc[k].links = link_addr ? link_addr[i] : reinterpret_cast<uint64_t>(dl + (nl ? 16 * link_base[i] : 0));
    desc[k].len = (uint32_t)lens[i];
    desc[k].n_links = nl;
    desc[k].pad = 0;
    if (expect) std::memcpy(&exp_p[16 * k], expect + 16ull * i, 16);
  }
  hipStream_t s = c->stream;
  HBX_TRY(c, hipMemsetAsync(c->d_zeros.p, 0, 256, s));
  HBX_TRY(c, hipMemcpyAsync(c->d_vdesc.p, desc.data(), n * sizeof(VerifyDesc), hipMemcpyHostToDevice, s));
  if (nlinks_total) HBX_TRY(c, hipMemcpyAsync(c->d_vlinks.p, links, 16 * nlinks_total, hipMemcpyHostToDevice, s));
  if (expect) HBX_TRY(c, hipMemcpyAsync(c->d_vexp.p, exp_p.data(), n * 16, hipMemcpyHostToDevice, s));
  uint8_t* dout = c->d_vout.as<uint8_t>();
  hipLaunchKernelGGL(hbx_k6_hash_blocks, dim3((uint32_t)((n + 63) / 64)), dim3(64), 0, s,
                     c->d_vdesc.as<VerifyDesc>(), (uint32_t)n, c->d_zeros.as<uint8_t>(),
                     reinterpret_cast<uint32_t*>(dout), expect ? c->d_vexp.as<uint32_t>() : nullptr,
                     dout + 16 * n);
  HBX_TRY(c, hipGetLastError());
  std::vector<uint8_t> out(n * 17);
  HBX_TRY(c, hipMemcpyAsync(out.data(), dout, n * 17, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  uint64_t bad = 0;
  for (uint64_t k = 0; k < n; k++) {
    const uint32_t i = perm[k];
    if (ids) std::memcpy(ids + 16ull * i, &out[16 * k], 16);
    if (expect) {
      const uint8_t good = out[16 * n + k];
      if (ok) ok[i] = good;
      bad += good ? 0 : 1;
    }
  }
  if (n_bad) *n_bad = bad;
  return HBX_OK;
}
}  // namespace

int hbx_verify_blocks_device(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                             const uint64_t* lens, const uint8_t* links, const uint64_t* link_base,
                             const uint32_t* n_links, uint8_t* ids, const uint8_t* expect, uint8_t* ok,
                             uint64_t* n_bad) {
  if (!c || (n && (!d_arena || !offs || !lens))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  return verify_device(c, static_cast<const uint8_t*>(d_arena), n, offs, lens, links, link_base, n_links,
                       ids, expect, ok, n_bad);
}

int hbx_verify_blocks(hbx_ctx* c, uint64_t n, const uint8_t* const* datas, const uint64_t* lens,
                      const uint8_t* links, const uint64_t* link_base, const uint32_t* n_links,
                      uint8_t* ids, const uint8_t* expect, uint8_t* ok, uint64_t* n_bad) {
  if (!c || (n && (!datas || !lens))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  std::vector<uint64_t> offs(n);
  uint64_t total = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (lens[i] && !datas[i]) return c->fail(HBX_ERR_ARG, "null block data");
    offs[i] = total;
    total += (lens[i] + 255) & ~uint64_t(255);
  }
  HBX_TRY(c, c->d_stage.ensure(total + 65536));
  uint8_t* arena = c->d_stage.as<uint8_t>();
  for (uint64_t i = 0; i < n; i++)
    if (lens[i]) HBX_TRY(c, hipMemcpyAsync(arena + offs[i], datas[i], lens[i], hipMemcpyHostToDevice, c->stream));
  return verify_device(c, arena, n, offs.data(), lens, links, link_base, n_links, ids, expect, ok, n_bad);
}

int hbx_arena_alloc(hbx_ctx* c, uint64_t bytes, void** d_ptr) {
  if (!c || !d_ptr) return HBX_ERR_ARG;
  HBX_TRY(c, hipSetDevice(c->device));
  HBX_TRY(c, hipMalloc(d_ptr, bytes + 65536));
  return HBX_OK;
}

int hbx_arena_free(hbx_ctx* c, void* d_ptr) {
  if (!c) return HBX_ERR_ARG;
  if (!d_ptr) return HBX_OK;
  HBX_TRY(c, hipSetDevice(c->device));
  HBX_TRY(c, hipFree(d_ptr));
  return HBX_OK;
}

int hbx_memcpy_h2d(hbx_ctx* c, void* d, const void* h, uint64_t n) {
  if (!c || (n && (!d || !h))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HBX_TRY(c, hipSetDevice(c->device));
  if (int frc = flush_input_wait(c)) return frc;
  HBX_TRY(c, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->stream));
  HBX_TRY(c, hipStreamSynchronize(c->stream));
  return HBX_OK;
}

// ---- files on disk -> pinned -> HBM -> results (BASELINE configs[4]) ----
namespace {

// Read whole files into dst + offs[i] with `threads` threads (files are
// independent).  Returns 0 or HBX_ERR_IO with the offending path in err.
// With `status` (per file of this list), the failures the reference treats
// per file are recorded there instead of failing the call, and the file is
// skipped (hbx_store_paths_status): an open() failure (os.Open returns it,
// storeDir logs and continues: store.go:101-103, 221-224) and a read failing
// with EBADF (minorPathError, hashback_unix.go:57-63).  Any other read error
// or a short file is a panic in storeFile (CopyNOrPanic, utils.go:95-99):
// the call fails either way.
int read_files(uint64_t n, const char* const* paths, const uint64_t* lens, const uint64_t* offs,
               uint8_t* dst, uint32_t threads, std::string& err, int32_t* status = nullptr) {
  std::atomic<uint64_t> next{0};
  std::atomic<int> failed{0};
  std::mutex emu;
  auto worker = [&]() {
    for (;;) {
      const uint64_t i = next.fetch_add(1);
      if (i >= n || failed.load()) return;
      if (status) status[i] = 0;
      const int fd = ::open(paths[i], O_RDONLY | O_CLOEXEC);
      int e = fd < 0 ? errno : 0;
      if (fd < 0 && status) {
        status[i] = e ? e : EIO;
        continue;
      }
      uint64_t got = 0;
      while (fd >= 0 && got < lens[i]) {
        const ssize_t r = ::pread(fd, dst + offs[i] + got, lens[i] - got, (off_t)got);
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          e = r < 0 ? errno : 0;  // 0: end of file before lens[i] bytes
          break;
        }
        got += (uint64_t)r;
      }
      if (fd >= 0) ::close(fd);
      if (fd >= 0 && got == lens[i]) continue;
      if (status && e == EBADF) {
        status[i] = EBADF;
        continue;
      }
      failed.store(1);
      std::lock_guard<std::mutex> g(emu);
      err = std::string("cannot read ") + std::to_string(lens[i]) + " bytes of " + paths[i] + ": " +
            (fd < 0 ? std::string("open: ") + std::strerror(e)
                    : e ? std::string(std::strerror(e)) : "end of file after " + std::to_string(got) + " bytes");
      return;
    }
  };
  const uint32_t nt = std::max<uint32_t>(1, std::min<uint64_t>(threads, n));
  std::vector<std::thread> pool;
  for (uint32_t t = 1; t < nt; t++) pool.emplace_back(worker);
  worker();
  for (auto& t : pool) t.join();
  return failed.load() ? HBX_ERR_IO : HBX_OK;
}

}  // namespace

namespace {
int deflate_device(hbx_ctx* c, uint64_t n, const uint64_t* src, const uint64_t* lens, const uint64_t* dst,
                   uint64_t* out_lens);

// Output of hbx_store_paths_z (null members: no compression).
struct ZOut {
  uint8_t* zout = nullptr;
  const uint64_t* zbase = nullptr;
  uint64_t* zoff = nullptr;
  uint64_t* zlen = nullptr;
  hbx_batch_ready_fn ready = nullptr;  // called once a batch's results are all written
  void* user = nullptr;
  // hbx_store_paths_dd: the K9 flags (parallel to cut_ends); a chunk that is
  // not fresh is not compressed, not copied back and not placed (zlen 0)
  const uint8_t* fresh = nullptr;
};
constexpr uint64_t kNoStream = ~0ull;  // ZPend::dst of a chunk without a stream
// A collected batch whose device arena still holds its files.
struct ZJob {
  uint64_t first = 0, count = 0;
  const uint8_t* arena = nullptr;
  std::vector<uint64_t> offs;
};

// CompressData of every chunk of a collected batch (client.go:249-258),
// asynchronous: K7 reads the batch's arena on the engine's compression
// streams (one per stage) and the streams come back in one D2H copy into a pinned stage, while
// the caller's loop goes on reading and copying later batches.  Two stages
// rotate; a stage is unpacked (streams placed per file at zout[zbase[f] ..],
// the batch's callback) before it is reused, and every job is unpacked in
// FIFO order before hbx_store_paths_z returns.
struct ZPend {
  ZJob job;
  int stage = 0;
  std::vector<uint64_t> dst;  // stream offset of each chunk in the stage
  std::shared_future<int> fin;  // its unpack (z_finish), on a worker thread
  double t_sync = 0.0;          // HBX_ZDIAG: time that unpack waited for the GPU
  std::string err;              // the worker's error text: it never writes c->err,
                                // which the main loop owns; zdrain_one copies it
};

int z_launch(hbx_ctx* c, int stage, std::vector<hbxz::ZBlock>& zb, uint64_t d, uint64_t nseg);

int z_start(hbx_ctx* c, ZPend& zp, const uint64_t* cut_ends, const uint64_t* out_base,
            const hbx_file_summary* sums, const uint8_t* fresh) {
  std::vector<hbxz::ZBlock> zb;
  uint64_t d = 0, nseg = 0;
  for (uint64_t i = 0; i < zp.job.count; i++) {
    const uint64_t f = zp.job.first + i;
    uint64_t start = 0;
    for (uint32_t q = 0; q < sums[f].n_chunks; q++) {
      const uint64_t e = cut_ends[out_base[f] + q];
      const uint64_t len = e - start, ns = (len + hbxz::kSeg - 1) / hbxz::kSeg;
      if (fresh && !fresh[out_base[f] + q]) {  // seen before: the caller sends nothing for it
        zp.dst.push_back(kNoStream);
        start = e;
        continue;
      }
      zb.push_back(hbxz::ZBlock{reinterpret_cast<uint64_t>(zp.job.arena + zp.job.offs[i] + start), d, len,
                                (uint32_t)nseg, (uint32_t)ns});
      zp.dst.push_back(d);
      d += (hbx_deflate_bound(len) + 15) & ~uint64_t(15);
      nseg += ns;
      start = e;
    }
  }
  return z_launch(c, zp.stage, zb, d, nseg);
}

// Enqueue K7 over `zb` (dst: offsets into the stage, d bytes in all, nseg
// 32 KiB pieces) on the stage's stream, the copy-back of the lengths and the
// streams into its pinned buffers, and its completion event.
int z_launch(hbx_ctx* c, int stage, std::vector<hbxz::ZBlock>& zb, uint64_t d, uint64_t nseg) {
  auto& Z = c->zs[stage];
  const uint64_t n = zb.size();
  if (n == 0) return HBX_OK;
  if (nseg > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "too much data in one batch");
  if (!Z.stream) HBX_TRY(c, hipStreamCreateWithFlags(&Z.stream, hipStreamNonBlocking));
  if (!Z.done) HBX_TRY(c, hipEventCreateWithFlags(&Z.done, hipEventDisableTiming));
  HBX_TRY(c, Z.out.ensure(d + 64));
  HBX_TRY(c, Z.stage.ensure(d + 64));
  HBX_TRY(c, Z.desc.ensure(n * sizeof(hbxz::ZBlock)));
  HBX_TRY(c, Z.lens.ensure(n * 8));
  HBX_TRY(c, Z.blk.ensure(n * sizeof(hbxz::ZBlock)));
  HBX_TRY(c, Z.info.ensure(std::max<uint64_t>(nseg, 1) * sizeof(hbxz::SegInfo)));
  HBX_TRY(c, Z.off.ensure(std::max<uint64_t>(nseg, 1) * 8));
  HBX_TRY(c, Z.len.ensure(n * 8));
  HBX_TRY(c, Z.img.ensure(std::max<uint64_t>(nseg, 1) * hbxz::kSlot));
  const uint64_t base = reinterpret_cast<uint64_t>(Z.out.p);
  for (auto& x : zb) x.dst += base;  // stage offsets -> device addresses
  std::memcpy(Z.desc.p, zb.data(), n * sizeof(hbxz::ZBlock));
  hipStream_t s = Z.stream;
  HBX_TRY(c, hipMemcpyAsync(Z.blk.p, Z.desc.p, n * sizeof(hbxz::ZBlock), hipMemcpyHostToDevice, s));
  const hbxz::ZBlock* dz = Z.blk.as<hbxz::ZBlock>();
  hipLaunchKernelGGL(hbx_k7_deflate_entropy, dim3((uint32_t)nseg), dim3(hbxz::kEThreads), 0, s, dz, (uint32_t)n,
                     (uint32_t)nseg, Z.info.as<hbxz::SegInfo>());
  hipLaunchKernelGGL(hbx_k7_deflate_size, dim3((uint32_t)nseg), dim3(hbxz::kThreads), 0, s, dz, (uint32_t)n,
                     (uint32_t)nseg, Z.info.as<hbxz::SegInfo>(), Z.img.as<uint32_t>());
  hipLaunchKernelGGL(hbx_k7_deflate_code, dim3((uint32_t)nseg), dim3(hbxz::kThreads), 0, s, dz, (uint32_t)n,
                     (uint32_t)nseg, Z.info.as<hbxz::SegInfo>(), Z.img.as<uint32_t>());
  HBX_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(hbx_k7_deflate_plan, dim3((uint32_t)n), dim3(64), 0, s, dz, (uint32_t)n,
                     Z.info.as<hbxz::SegInfo>(), Z.off.as<uint64_t>(), Z.len.as<uint64_t>());
  HBX_TRY(c, hipGetLastError());
  hipLaunchKernelGGL(hbx_k7_deflate_write, dim3((uint32_t)nseg), dim3(hbxz::kWThreads), 0, s, (uint32_t)nseg,
                     Z.info.as<hbxz::SegInfo>(), Z.img.as<uint32_t>(), Z.off.as<uint64_t>(), dz, (uint32_t)n);
  HBX_TRY(c, hipGetLastError());
  HBX_TRY(c, hipMemcpyAsync(Z.lens.p, Z.len.p, n * 8, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipMemcpyAsync(Z.stage.p, Z.out.p, d, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipEventRecord(Z.done, s));
  return HBX_OK;
}

// Wait for a started job, place its streams and call the batch back.
// Runs on a worker thread: reports errors only through zp.err (never c->err,
// c->hip or c->fail, which the caller's thread uses meanwhile).
int z_finish(const hbx_ctx* c, ZPend& zp, const uint64_t* out_base, const hbx_file_summary* sums, const ZOut& z,
             uint32_t threads, double& t_sync) {
  const auto& Z = c->zs[zp.stage];
  const uint64_t nc = zp.dst.size();
  if (nc) {
    const auto t0 = std::chrono::steady_clock::now();
    // (a batch without a fresh chunk started no job: nothing to wait for)
    const bool started = std::count(zp.dst.begin(), zp.dst.end(), kNoStream) != (int64_t)nc;
    const hipError_t e = started ? hipEventSynchronize(Z.done) : hipSuccess;
    if (e != hipSuccess) {
      zp.err = std::string("hipEventSynchronize(compression stage): ") + hipGetErrorString(e);
      return HBX_ERR_HIP;
    }
    t_sync += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    const uint8_t* h = Z.stage.as<uint8_t>();
    const uint64_t* ol = Z.lens.as<uint64_t>();
    // placement (serial, cheap), then the copies out of the pinned stage on
    // `threads` threads (one thread copies a few GB/s)
    // (ol and the stage hold the compressed chunks only, in order: zi)
    std::vector<uint64_t> to(nc), zl(nc);
    uint64_t k = 0, zi = 0;
    for (uint64_t i = 0; i < zp.job.count; i++) {
      const uint64_t f = zp.job.first + i;
      uint64_t run = z.zbase[f];
      for (uint32_t q = 0; q < sums[f].n_chunks; q++, k++) {
        zl[k] = zp.dst[k] == kNoStream ? 0 : ol[zi++];
        to[k] = run;
        z.zoff[out_base[f] + q] = run;
        z.zlen[out_base[f] + q] = zl[k];
        run += zl[k];
      }
    }
    const uint32_t nt = std::max<uint32_t>(1u, std::min<uint32_t>(threads, 64u));
    std::vector<std::thread> pool;
    for (uint32_t t = 0; t < nt; t++)
      pool.emplace_back([&, t] {
        for (uint64_t i = t; i < nc; i += nt)
          if (zl[i]) std::memcpy(z.zout + to[i], h + zp.dst[i], zl[i]);
      });
    for (auto& th : pool) th.join();
  }
  if (z.ready) z.ready(z.user, zp.job.first, zp.job.count);
  return HBX_OK;
}

int store_paths_impl(hbx_ctx* c, uint64_t n, const char* const* paths, const uint64_t* lens,
                     uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base, const uint64_t* caps,
                     hbx_file_summary* sums, uint32_t io_threads, uint64_t batch_bytes, const ZOut& z,
                     int32_t* status = nullptr, hbx_idset* set = nullptr, uint8_t* fresh = nullptr,
                     const MatchIn* mi = nullptr);
}  // namespace

int hbx_store_paths(hbx_ctx* c, uint64_t n, const char* const* paths, const uint64_t* lens,
                    uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base,
                    const uint64_t* caps, hbx_file_summary* sums, uint32_t io_threads,
                    uint64_t batch_bytes) {
  if (!c) return HBX_ERR_ARG;
  if (n && (!paths || !lens || !out_base || !caps)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return store_paths_impl(c, n, paths, lens, cut_ends, ids, out_base, caps, sums, io_threads, batch_bytes,
                          ZOut{});
}

int hbx_store_paths_status(hbx_ctx* c, uint64_t n, const char* const* paths, const uint64_t* lens,
                           uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base, const uint64_t* caps,
                           hbx_file_summary* sums, int32_t* status, uint32_t io_threads, uint64_t batch_bytes,
                           uint8_t* zout, const uint64_t* zbase, uint64_t* zoff, uint64_t* zlen,
                           hbx_batch_ready_fn ready, void* user) {
  if (c && n && !status) return HBX_ERR_ARG;
  return hbx_store_paths_dd(c, n, paths, lens, cut_ends, ids, out_base, caps, sums, status, io_threads, batch_bytes,
                            zout, zbase, zoff, zlen, ready, user, nullptr, nullptr);
}

int hbx_store_paths_dd(hbx_ctx* c, uint64_t n, const char* const* paths, const uint64_t* lens, uint64_t* cut_ends,
                       uint8_t* ids, const uint64_t* out_base, const uint64_t* caps, hbx_file_summary* sums,
                       int32_t* status, uint32_t io_threads, uint64_t batch_bytes, uint8_t* zout,
                       const uint64_t* zbase, uint64_t* zoff, uint64_t* zlen, hbx_batch_ready_fn ready, void* user,
                       hbx_idset* set, uint8_t* fresh) {
  if (!c) return HBX_ERR_ARG;
  if (set && !fresh) return HBX_ERR_ARG;
  const bool z = zout || zbase || zoff || zlen;
  if (n && (!paths || !lens || !out_base || !caps)) return HBX_ERR_ARG;
  if (n && z && (!sums || !zout || !zbase || !zoff || !zlen)) return HBX_ERR_ARG;
  if (!z && ready) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (set && std::find(c->idsets.begin(), c->idsets.end(), set) == c->idsets.end())
    return c->fail(HBX_ERR_ARG, "not an ID set of this context");
  for (uint64_t i = 0; status && i < n; i++) status[i] = 0;
  return store_paths_impl(c, n, paths, lens, cut_ends, ids, out_base, caps, sums, io_threads, batch_bytes,
                          z ? ZOut{zout, zbase, zoff, zlen, ready, user, set ? fresh : nullptr} : ZOut{}, status,
                          set, set ? fresh : nullptr);
}

int hbx_store_paths_match(hbx_ctx* c, uint64_t n, const char* const* paths, const uint64_t* lens, uint64_t* cut_ends,
                          uint8_t* ids, const uint64_t* out_base, const uint64_t* caps, hbx_file_summary* sums,
                          int32_t* status, uint32_t io_threads, uint64_t batch_bytes, const uint64_t* expect_first,
                          const uint8_t* expect_ids, hbx_chain_match* match) {
  if (!c) return HBX_ERR_ARG;
  if (!expect_first)
    return hbx_store_paths_dd(c, n, paths, lens, cut_ends, ids, out_base, caps, sums, status, io_threads, batch_bytes,
                              nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr);
  if (n && (!paths || !lens)) return HBX_ERR_ARG;
  bool vo = false;
  if (int rc = match_args(n, cut_ends, ids, out_base, caps, expect_first, expect_ids, match, &vo)) return rc;
  std::lock_guard<std::mutex> g(c->mu);
  for (uint64_t i = 0; status && i < n; i++) status[i] = 0;
  const MatchIn mi{expect_first, expect_ids, match, vo};
  return store_paths_impl(c, n, paths, lens, cut_ends, ids, out_base, caps, sums, io_threads, batch_bytes, ZOut{},
                          status, nullptr, nullptr, &mi);
}

uint64_t hbx_deflate_file_bound(uint64_t len) {
  return len + 16ull * hbx_max_chunks(len) + 5ull * (len / hbxz::kSeg);
}

int hbx_store_paths_z(hbx_ctx* c, uint64_t n, const char* const* paths, const uint64_t* lens,
                      uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base, const uint64_t* caps,
                      hbx_file_summary* sums, uint32_t io_threads, uint64_t batch_bytes, uint8_t* zout,
                      const uint64_t* zbase, uint64_t* zoff, uint64_t* zlen) {
  if (!c) return HBX_ERR_ARG;
  if (n && (!paths || !lens || !out_base || !caps || !sums || !zout || !zbase || !zoff || !zlen))
    return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return store_paths_impl(c, n, paths, lens, cut_ends, ids, out_base, caps, sums, io_threads, batch_bytes,
                          ZOut{zout, zbase, zoff, zlen, nullptr, nullptr});
}

int hbx_store_paths_zcb(hbx_ctx* c, uint64_t n, const char* const* paths, const uint64_t* lens,
                        uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base, const uint64_t* caps,
                        hbx_file_summary* sums, uint32_t io_threads, uint64_t batch_bytes, uint8_t* zout,
                        const uint64_t* zbase, uint64_t* zoff, uint64_t* zlen, hbx_batch_ready_fn ready,
                        void* user) {
  if (!c) return HBX_ERR_ARG;
  if (n && (!paths || !lens || !out_base || !caps || !sums || !zout || !zbase || !zoff || !zlen))
    return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  return store_paths_impl(c, n, paths, lens, cut_ends, ids, out_base, caps, sums, io_threads, batch_bytes,
                          ZOut{zout, zbase, zoff, zlen, ready, user});
}

namespace {
// Device arenas of the disk paths' ring (2..64) for a per-submit slice
// `budget`: a batch's chains join the launch join_lag submits later (up to
// P - 1 more with a K3 period P) and need ceil(nfull / (P x budget)) launches
// P submits apart, so this many arenas keep the collect from forcing a drain.
size_t ring_depth(const hbx_ctx* c, uint32_t budget) {
  const uint64_t nfull_max = (HBX_MAX_BLOCK_SIZE + 8ull) >> 6;
  const uint64_t lb = launch_budget(c, budget), per = std::max<uint32_t>(1, c->k3_period);
  return budget == kBudgetAll ? 2 : (size_t)std::min<uint64_t>(64, (nfull_max + lb - 1) / lb * per + c->join_lag + per);
}

int store_paths_impl(hbx_ctx* c, uint64_t n, const char* const* paths, const uint64_t* lens,
                     uint64_t* cut_ends, uint8_t* ids, const uint64_t* out_base, const uint64_t* caps,
                     hbx_file_summary* sums, uint32_t io_threads, uint64_t batch_bytes, const ZOut& z,
                     int32_t* status, hbx_idset* set, uint8_t* fresh, const MatchIn* mi) {
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  // with an ID set the batch size is the caller's down to 1 MiB (the flags do
  // not depend on how the files fall into batches, and tests check that with
  // small files); without one it is at least 64 MiB, as ever
  // (likewise with expected chains: the records do not depend on the batches either)
  const uint64_t batch_min = set || mi ? 1ull << 20 : 64ull << 20;
  if (batch_bytes < batch_min) batch_bytes = batch_min;
  uint64_t set_count0 = 0;  // a failed call puts the set back to this
  if (set)
    if (int r0 = idset_count(c, set, &set_count0, nullptr)) return r0;
  for (hipEvent_t& e : c->h2d_done)
    if (!e) HBX_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  // Pipeline: files of batch k are read (io_threads) into pinned slot k % 2
  // while earlier batches copy and hash; the H2D copy runs on the scan
  // stream into device arena k % depth, and the batch joins the time-sliced
  // MD5 chains.  A pinned slot is free once its copy has completed, a device
  // arena once its batch has been collected.
  const uint32_t budget = c->md5_slice ? c->md5_slice : kBudgetAll;
  const size_t depth = ring_depth(c, budget);
  if (c->d_ring.size() < depth) c->d_ring.resize(depth);
  // size every staging buffer once, for the largest batch this call forms
  // (growing one later would re-pin host memory or drain the streams)
  uint64_t biggest = 0, zbytes = 0, zchunks = 0, zsegs = 0, most_files = 0, most_expect = 0;
  for (uint64_t i = 0; i < n;) {
    uint64_t tot = 0, cnt = 0;
    const uint64_t i0 = i;
    while (i < n && (cnt == 0 || tot + lens[i] <= batch_bytes) && cnt < 65536) {
      tot += (lens[i] + 255) & ~uint64_t(255);
      i++;
      cnt++;
    }
    biggest = std::max(biggest, tot);
    most_files = std::max(most_files, cnt);
    if (mi) most_expect = std::max(most_expect, mi->first[i] - mi->first[i0]);
    // compression stage bounds of this batch: chunks <= a file's
    // max_chunks, a chunk's stream <= hbx_deflate_bound rounded to 16 B
    const uint64_t nch = tot / HBX_MIN_BLOCK_SIZE + cnt;
    zchunks = std::max(zchunks, nch);
    zsegs = std::max(zsegs, tot / hbxz::kSeg + nch);
    zbytes = std::max<uint64_t>(zbytes, tot + 5ull * (tot / hbxz::kSeg) + 31ull * nch + 64);
  }
  for (PinBuf& h : c->h_read) HBX_TRY(c, h.ensure(biggest + 65536));
  if (z.zout)  // every compression stage sized once (growing one would re-pin or drain the device)
    for (auto& Z : c->zs) {
      HBX_TRY(c, Z.out.ensure(zbytes));
      HBX_TRY(c, Z.stage.ensure(zbytes));
      HBX_TRY(c, Z.desc.ensure(zchunks * sizeof(hbxz::ZBlock)));
      HBX_TRY(c, Z.lens.ensure(zchunks * 8));
      HBX_TRY(c, Z.blk.ensure(zchunks * sizeof(hbxz::ZBlock)));
      HBX_TRY(c, Z.info.ensure(std::max<uint64_t>(zsegs, 1) * sizeof(hbxz::SegInfo)));
      HBX_TRY(c, Z.off.ensure(std::max<uint64_t>(zsegs, 1) * 8));
      HBX_TRY(c, Z.len.ensure(zchunks * 8));
      HBX_TRY(c, Z.img.ensure(std::max<uint64_t>(zsegs, 1) * hbxz::kSlot));
    }
  for (size_t i = 0; i < depth; i++) {
    int r0 = ensure_shared(c, c->d_ring[i], biggest + 65536);
    if (r0) return r0;
  }
  // every batch slot of the pipeline sized for the largest batch up front: a
  // pooled batch that met a larger batch later reallocated its pinned meta and
  // result buffers inside that submit (19-28 ms per submit of config 5,
  // HBX_TRACE_SLOW_SUBMIT "buffers", profiles/r06e)
  if (int r0 = reserve_locked(c, (uint32_t)depth + 2u, most_files, biggest, set != nullptr, mi != nullptr, most_expect))
    return r0;
  auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
  bool slot_used[2] = {false, false};
  std::vector<uint64_t> offs, skip_lens;
  uint64_t f = 0, k = 0;
  int rc = HBX_OK;
  // with compression, each collected batch is compressed from its arena on
  // the compression stream (z_start); the next batch copied into that arena
  // waits for it on the GPU, and the host unpacks a stage (z_finish, FIFO)
  // before reusing it and at the end
  std::deque<ZJob> jobs;
  std::deque<ZPend> zq;
  uint64_t zjobs = 0;
  double zt[4] = {0, 0, 0, 0};  // HBX_ZDIAG: wait_oldest | z_start | z_finish | its event waits
  int arena_zstage = -1;  // the stage that reads the arena just freed by collect()
  auto zdrain_one = [&]() -> int {
    const double t0 = now();
    const int r = zq.front().fin.get();
    if (r && !zq.front().err.empty()) c->err = zq.front().err;  // the worker's text, on this thread
    zt[2] += now() - t0;
    zt[3] += zq.front().t_sync;
    zq.pop_front();
    return r;
  };
  // every compression stream idle: K7 of a failed job may still read an arena
  // that the next call rewrites
  auto zsync_all = [&]() {
    for (auto& Z : c->zs)
      if (Z.stream) (void)hipStreamSynchronize(Z.stream);
  };
  auto collect = [&]() -> int {
    const double t0 = now();
    int r = wait_oldest(c);
    zt[0] += now() - t0;
    arena_zstage = -1;
    if (z.zout && !jobs.empty()) {
      if (!r && zq.size() >= (size_t)hbx_ctx::kZStages) r = zdrain_one();  // the stage this job takes
      if (!r) {
        ZPend zp;
        zp.job = std::move(jobs.front());
        zp.stage = (int)(zjobs++ % (uint64_t)hbx_ctx::kZStages);
        const double t1 = now();
        r = z_start(c, zp, cut_ends, out_base, sums, z.fresh);
        zt[1] += now() - t1;
        arena_zstage = zp.stage;
        // the unpack runs on a worker thread while this loop reads and copies
        // the next batches; each waits for its predecessor (FIFO callbacks)
        std::shared_future<int> prev = zq.empty() ? std::shared_future<int>() : zq.back().fin;
        zq.push_back(std::move(zp));
        if (!r) {
          ZPend* zpp = &zq.back();  // a deque keeps element addresses on push_back / pop_front
          const uint32_t ut = std::max<uint32_t>(1u, io_threads / 2u);
          zpp->fin = std::async(std::launch::async, [c, zpp, prev, out_base, sums, &z, ut]() -> int {
                       if (prev.valid()) {
                         const int r0 = prev.get();
                         if (r0) return r0;
                       }
                       (void)hipSetDevice(c->device);
                       return z_finish(c, *zpp, out_base, sums, z, ut, zpp->t_sync);
                     }).share();
        } else {
          std::promise<int> pr;
          pr.set_value(r);
          zq.back().fin = pr.get_future().share();
        }
      }
      jobs.pop_front();
    }
    return r;
  };
  while (f < n && rc == HBX_OK) {
    const uint64_t first = f;
    offs.clear();
    uint64_t tot = 0;
    while (f < n && (offs.empty() || tot + lens[f] <= batch_bytes) && offs.size() < 65536) {
      offs.push_back(tot);
      tot += (lens[f] + 255) & ~uint64_t(255);
      f++;
    }
    const int p = (int)(k & 1);
    DevBuf& arena = c->d_ring[k % depth];
    double t0 = now();
    if (c->pending.size() >= depth && (rc = collect())) break;  // frees arena k % depth
    double t1 = now();
    if (slot_used[p] && (rc = c->hip(hipEventSynchronize(c->h2d_done[p]), "h2d wait"))) break;
    double t2 = now();
    rc = read_files(f - first, paths + first, lens + first, offs.data(), c->h_read[p].as<uint8_t>(),
                    io_threads, c->err, status ? status + first : nullptr);
    c->io_s[0] += now() - t2;
    c->io_s[1] += t1 - t0;
    c->io_s[2] += t2 - t1;
    if (rc) break;
    // the arena's previous batch may still be read by its compression job
    if (arena_zstage >= 0 && c->zs[arena_zstage].done &&
        (rc = c->hip(hipStreamWaitEvent(c->stream, c->zs[arena_zstage].done, 0), "hipStreamWaitEvent")))
      break;
    arena_zstage = -1;
    const auto tc = std::chrono::steady_clock::now();
    if ((rc = c->hip(hipMemcpyAsync(arena.p, c->h_read[p].p, tot, hipMemcpyHostToDevice, c->stream),
                     "hipMemcpyAsync")))
      break;
    c->max_copy_ms = std::max(c->max_copy_ms, ms_since(tc));
    g_slow.call("store_paths h2d: hipMemcpyAsync", tc, c->launches);
    if ((rc = c->hip(hipEventRecord(c->h2d_done[p], c->stream), "hipEventRecord"))) break;
    slot_used[p] = true;
    // a skipped file (status != 0) goes in as an empty file: no chunks
    const uint64_t* blens = lens + first;
    if (status) {
      skip_lens.assign(lens + first, lens + f);
      for (uint64_t i = first; i < f; i++)
        if (status[i]) skip_lens[i - first] = 0;
      blens = skip_lens.data();
    }
    MatchIn bm;  // this batch's share of the expected chains
    if (mi) bm = MatchIn{mi->first + first, mi->ids, mi->out + first, mi->verdict_only};
    rc = submit_batch(c, arena.p, f - first, offs.data(), blens, cut_ends, ids,
                      out_base ? out_base + first : nullptr, caps ? caps + first : nullptr,
                      sums ? sums + first : nullptr, budget, nullptr, nullptr, set, fresh, mi ? &bm : nullptr);
    if (z.zout && rc == HBX_OK) jobs.push_back(ZJob{first, f - first, static_cast<const uint8_t*>(arena.p), offs});
    k++;
  }
  // collect everything in flight (also after a failure: the caller's arrays
  // must not be written once this call has returned); counted as waiting
  // for collection
  const double td = now();
  while (!c->pending.empty()) {
    const std::string keep = c->err;
    const int r2 = rc == HBX_OK ? collect() : wait_oldest(c);
    if (rc == HBX_OK) rc = r2;
    else c->err = keep;
  }
  // every compression job unpacked (also after a failure: the stages must be
  // idle before the arena ring is reused)
  while (!zq.empty()) {
    if (rc == HBX_OK) {
      rc = zdrain_one();
    } else {
      zq.front().fin.wait();  // its worker must be done before the stages and arenas go
      zq.pop_front();
    }
  }
  if (rc != HBX_OK && z.zout) zsync_all();
  // the caller saw none of a failed call's chunks: the set forgets them
  if (rc != HBX_OK && set && !c->broken) {
    const std::string keep = c->err;
    (void)idset_truncate(c, set, set_count0);
    c->err = keep;
  }
  c->io_s[1] += now() - td;
  if (z.zout && ab_env("HBX_ZDIAG"))
    std::fprintf(stderr, "zdiag: wait_oldest %.3f s, z_start %.3f s, z_finish %.3f s (event waits %.3f s), jobs %llu\n",
                 zt[0], zt[1], zt[2], zt[3], (unsigned long long)zjobs);
  return rc;
}
}  // namespace

namespace {
// Read file bytes [off, off + len) of `fd` into dst with `threads` ranged
// preads (pieces of whole MiB).  0, or HBX_ERR_IO with the reason in err.
int read_range(int fd, const char* path, uint64_t off, uint64_t len, uint8_t* dst, uint32_t threads,
               std::string& err) {
  const uint64_t piece = std::max<uint64_t>(1ull << 20, ((len + threads - 1) / std::max(1u, threads) + 0xFFFFFull) & ~0xFFFFFull);
  const uint64_t np = (len + piece - 1) / piece;
  std::atomic<uint64_t> next{0};
  std::atomic<int> failed{0};
  std::mutex emu;
  auto worker = [&]() {
    for (;;) {
      const uint64_t i = next.fetch_add(1);
      if (i >= np || failed.load()) return;
      const uint64_t a = i * piece, want = std::min(piece, len - a);
      uint64_t got = 0;
      int e = 0;
      while (got < want) {
        const ssize_t r = ::pread(fd, dst + a + got, want - got, (off_t)(off + a + got));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {
          e = r < 0 ? errno : 0;  // 0: end of file before the stated size
          break;
        }
        got += (uint64_t)r;
      }
      if (got == want) continue;
      failed.store(1);
      std::lock_guard<std::mutex> g(emu);
      err = std::string("cannot read ") + std::to_string(want) + " bytes at " + std::to_string(off + a) + " of " + path +
            ": " + (e ? std::string(std::strerror(e)) : "end of file after " + std::to_string(got) + " bytes");
      return;
    }
  };
  const uint32_t nt = (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(threads, np));
  std::vector<std::thread> pool;
  for (uint32_t t = 1; t < nt; t++) pool.emplace_back(worker);
  worker();
  for (auto& t : pool) t.join();
  return failed.load() ? HBX_ERR_IO : HBX_OK;
}
}  // namespace

int hbx_store_file_seg(hbx_ctx* c, const char* path, uint64_t file_len, uint64_t seg_bytes, uint32_t io_threads,
                       uint64_t* cut_ends, uint8_t* ids, uint64_t cap, hbx_file_summary* summary) {
  if (!c || !path || !summary || (cap && (!cut_ends || !ids))) return HBX_ERR_ARG;
  if (seg_bytes < HBX_SEG_MIN_BYTES || seg_bytes % HBX_ARENA_ALIGN) return HBX_ERR_ARG;
  hbx_seg* h = nullptr;
  {
    std::lock_guard<std::mutex> g(c->mu);
    if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  }
  int rc = hbx_seg_open(c, file_len, &h);
  if (rc) return rc;
  {
    std::lock_guard<std::mutex> g(c->mu);
    h->keep_cuts = true;
    rc = [&]() -> int {
      if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
      HBX_TRY(c, hipSetDevice(c->device));
      for (hipEvent_t& e : c->h2d_done)
        if (!e) HBX_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      // Every buffer is sized by the segment, never by the file: two pinned
      // slots and `depth` device arenas of min(seg_bytes, file_len) + 64 KiB
      const uint32_t budget = c->md5_slice ? c->md5_slice : kBudgetAll;
      const size_t depth = ring_depth(c, budget);
      const uint64_t slot_bytes = std::min(seg_bytes, file_len) + 65536;
      if (c->d_ring.size() < depth) c->d_ring.resize(depth);
      for (PinBuf& p : c->h_read) HBX_TRY(c, p.ensure(slot_bytes));
      for (size_t i = 0; i < depth; i++)
        if (int r0 = ensure_shared(c, c->d_ring[i], slot_bytes)) return r0;
      if (int r0 = reserve_locked(c, (uint32_t)depth + 2u, 1, slot_bytes)) return r0;
      const int fd = file_len ? ::open(path, O_RDONLY | O_CLOEXEC) : -1;
      if (file_len && fd < 0)
        return c->fail(HBX_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
      auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
      bool slot_used[2] = {false, false};
      const uint64_t zero = 0;
      uint64_t prev_end = 0, k = 0;
      int r = HBX_OK;
      // Segment k is read into pinned slot k % 2 while earlier segments copy
      // and hash; reading never waits for a cut: the chain's resume point goes
      // from segment to segment on the device (hbx_k2s_cut_chain_seg).
      for (bool more = true; more && r == HBX_OK; k++) {
        uint64_t off = 0, len = 0;
        if ((r = hbx_seg_next(file_len, seg_bytes, prev_end, &off, &len))) {
          r = c->fail(r, "segment layout (internal)");
          break;
        }
        prev_end = off + len;
        more = prev_end < file_len;
        const int p = (int)(k & 1);
        DevBuf& arena = c->d_ring[k % depth];
        const double t0 = now();
        if (c->pending.size() >= depth && (r = wait_oldest(c))) break;  // frees arena k % depth
        const double t1 = now();
        if (slot_used[p] && (r = c->hip(hipEventSynchronize(c->h2d_done[p]), "h2d wait"))) break;
        const double t2 = now();
        if (len) r = read_range(fd, path, off, len, c->h_read[p].as<uint8_t>(), std::max(1u, io_threads), c->err);
        c->io_s[0] += now() - t2;
        c->io_s[1] += t1 - t0;
        c->io_s[2] += t2 - t1;
        if (r) break;
        if (len) {
          const auto tc = std::chrono::steady_clock::now();
          if ((r = c->hip(hipMemcpyAsync(arena.p, c->h_read[p].p, len, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync")))
            break;
          c->max_copy_ms = std::max(c->max_copy_ms, ms_since(tc));
          if ((r = c->hip(hipEventRecord(c->h2d_done[p], c->stream), "hipEventRecord"))) break;
          slot_used[p] = true;
        }
        const uint64_t scap = max_chunks(len);
        r = seg_submit(c, 1, &h, arena.p, &zero, &len, nullptr, nullptr, &zero, &scap, summary, budget);
      }
      if (fd >= 0) ::close(fd);
      // collect everything in flight, also after a failure
      const double td = now();
      while (!c->pending.empty()) {
        const std::string keep = c->err;
        const int r2 = wait_oldest(c);
        if (r == HBX_OK) r = r2;
        else c->err = keep;
      }
      c->io_s[1] += now() - td;
      return r;
    }();
    if (rc == HBX_OK) {
      // (`summary` was written by every segment's collect; the final one's,
      // collected last, carries the file's content type and id)
      const uint64_t kk = h->cuts.size();
      summary->n_chunks = (uint32_t)kk;
      if (kk > cap) {
        rc = c->fail(HBX_ERR_CAPACITY, "output capacity too small for the file (" + std::to_string(kk) + " chunks)");
      } else if (kk) {
        std::memcpy(cut_ends, h->cuts.data(), kk * 8);
        std::memcpy(ids, h->ids.data(), kk * 16);
      }
    }
  }
  const std::string keep = c->err;
  (void)hbx_seg_close(c, h);
  if (rc) c->err = keep;
  return rc;
}

namespace {
// One segment of hbx_store_file_stream, from its submit to the end of its sink
// call: the arrays its batch is collected into, then what the sink is shown.
struct StreamSeg {
  uint64_t off = 0, len = 0;       // file bytes [off, off + len)
  const uint8_t* arena = nullptr;  // the ring arena that holds them
  size_t ring = 0;                 // its slot in the ring
  bool final = false;
  uint64_t first_chunk = 0, k = 0;  // index of its first chunk in the file; chunks it completed
  uint64_t prev_cut = 0;            // where its first chunk starts: the file's previous last cut end
  std::vector<uint64_t> cuts, zoff, zlen;
  std::vector<uint8_t> ids, fresh;
  hbx_file_summary sum{};
  int stage = -1;             // its compression stage (-1: none)
  bool zstarted = false;      // K7 of it is on the stage's stream
  std::vector<uint64_t> dst;  // stage offset of each chunk's stream (kNoStream: not compressed)
  std::shared_future<int> fin;  // its worker: waits for the stage, then runs the sink
  std::string err;              // the worker's error text (never c->err, which the main loop owns)
};

// The worker's part: wait for the segment's compression job, lay out zoff and
// zlen over the pinned stage, and show the segment to the sink.
int stream_finish(const hbx_ctx* c, StreamSeg& s, bool zip, hbx_seg_sink_fn sink, void* user) {
  const uint8_t* z = nullptr;
  if (zip) {
    const auto& Z = c->zs[s.stage];
    if (s.zstarted) {
      (void)hipSetDevice(c->device);
      const hipError_t e = hipEventSynchronize(Z.done);
      if (e != hipSuccess) {
        s.err = std::string("hipEventSynchronize(compression stage): ") + hipGetErrorString(e);
        return HBX_ERR_HIP;
      }
    }
    // (the stage's length list holds the compressed chunks only, in order: zi)
    const uint64_t* ol = Z.lens.as<uint64_t>();
    uint64_t run = 0, zi = 0;
    for (uint64_t i = 0; i < s.k; i++) {
      const bool has = s.dst[i] != kNoStream;
      s.zoff[i] = has ? s.dst[i] : run;
      s.zlen[i] = has ? ol[zi++] : 0;
      run = s.zoff[i] + s.zlen[i];
    }
    z = Z.stage.as<uint8_t>();
  }
  if (!sink) return HBX_OK;
  hbx_seg_chunks sc{};
  sc.first_chunk = s.first_chunk;
  sc.n_chunks = s.k;
  sc.cut_ends = s.cuts.data();
  sc.ids = s.ids.data();
  sc.fresh = s.fresh.empty() ? nullptr : s.fresh.data();
  sc.z = z;
  sc.zoff = zip ? s.zoff.data() : nullptr;
  sc.zlen = zip ? s.zlen.data() : nullptr;
  sc.final = s.final ? 1 : 0;
  sc.summary = s.sum;
  if (const int rv = sink(user, &sc)) {
    s.err = "the sink returned " + std::to_string(rv) + " for the segment at file offset " + std::to_string(s.off);
    return HBX_ERR_SINK;
  }
  return HBX_OK;
}
}  // namespace

int hbx_store_file_stream(hbx_ctx* c, const char* path, uint64_t file_len, uint64_t seg_bytes, uint32_t io_threads,
                          uint32_t flags, hbx_idset* set, hbx_seg_sink_fn sink, void* user,
                          hbx_file_summary* summary) {
  // (every argument check that needs no context comes before the context is touched)
  if (!c || !path) return HBX_ERR_ARG;
  if (seg_bytes < HBX_SEG_MIN_BYTES || seg_bytes % HBX_ARENA_ALIGN) return HBX_ERR_ARG;
  if (flags & ~HBX_STREAM_COMPRESS) return HBX_ERR_ARG;
  const bool zip = (flags & HBX_STREAM_COMPRESS) != 0;
  if (zip && !sink) return HBX_ERR_ARG;
  hbx_seg* h = nullptr;
  {
    std::lock_guard<std::mutex> g(c->mu);
    if (set && std::find(c->idsets.begin(), c->idsets.end(), set) == c->idsets.end())
      return c->fail(HBX_ERR_ARG, "not an ID set of this context");
    if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  }
  int rc = hbx_seg_open(c, file_len, &h);
  if (rc) return rc;
  hbx_file_summary file_sum{};
  {
    std::lock_guard<std::mutex> g(c->mu);
    rc = [&]() -> int {
      if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
      HBX_TRY(c, hipSetDevice(c->device));
      uint64_t set_count0 = 0;  // a failed call puts the set back to this
      if (set)
        if (int r0 = idset_count(c, set, &set_count0, nullptr)) return r0;
      for (hipEvent_t& e : c->h2d_done)
        if (!e) HBX_TRY(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
      // Every buffer is sized by the segment, never by the file (hbxgpu.h)
      const uint32_t budget = c->md5_slice ? c->md5_slice : kBudgetAll;
      const size_t depth = ring_depth(c, budget);
      const uint64_t slot_bytes = std::min(seg_bytes, file_len) + 65536;
      if (c->d_ring.size() < depth) c->d_ring.resize(depth);
      for (PinBuf& p : c->h_read) HBX_TRY(c, p.ensure(slot_bytes));
      for (size_t i = 0; i < depth; i++)
        if (int r0 = ensure_shared(c, c->d_ring[i], slot_bytes)) return r0;
      if (int r0 = reserve_locked(c, (uint32_t)depth + 2u, 1, slot_bytes, set != nullptr)) return r0;
      if (zip) {  // both stages sized once, for one segment (the bounds of store_paths_impl)
        const uint64_t nch = max_chunks(slot_bytes), nsg = slot_bytes / hbxz::kSeg + nch;
        const uint64_t zbytes = slot_bytes + 5ull * (slot_bytes / hbxz::kSeg) + 31ull * nch + 64;
        for (auto& Z : c->zs) {
          HBX_TRY(c, Z.out.ensure(zbytes));
          HBX_TRY(c, Z.stage.ensure(zbytes));
          HBX_TRY(c, Z.desc.ensure(nch * sizeof(hbxz::ZBlock)));
          HBX_TRY(c, Z.lens.ensure(nch * 8));
          HBX_TRY(c, Z.blk.ensure(nch * sizeof(hbxz::ZBlock)));
          HBX_TRY(c, Z.info.ensure(nsg * sizeof(hbxz::SegInfo)));
          HBX_TRY(c, Z.off.ensure(nsg * 8));
          HBX_TRY(c, Z.len.ensure(nch * 8));
          HBX_TRY(c, Z.img.ensure(nsg * hbxz::kSlot));
        }
      }
      const int fd = file_len ? ::open(path, O_RDONLY | O_CLOEXEC) : -1;
      if (file_len && fd < 0)
        return c->fail(HBX_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
      auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
      // `flying`: submitted, not yet collected (the context's FIFO, in order);
      // `sinking`: collected, its worker not yet joined (at most one per stage)
      std::deque<std::unique_ptr<StreamSeg>> flying, sinking;
      std::vector<int> ring_stage(depth, -1);  // the stage whose job last read the arena
      std::atomic<int> worker_rc{0};           // the first failure of a worker
      uint64_t chunks_done = 0, zjobs = 0;
      bool from_worker = false;
      auto sdrain_one = [&]() -> int {
        const int r = sinking.front()->fin.get();
        if (r && !sinking.front()->err.empty()) c->err = sinking.front()->err;  // the worker's text, on this thread
        sinking.pop_front();
        return r;
      };
      // Collect the oldest segment and hand it to a worker: its compression job
      // goes on a stage's stream first, so the job and the sink call overlap
      // the reading, copying and hashing of the segments behind it.
      auto collect = [&]() -> int {
        StreamSeg* s = flying.front().get();
        s->prev_cut = h->last_cut;  // (the collect moves it on)
        int r = wait_oldest(c);
        if (r) return r;  // (the segment keeps its arrays until nothing is pending)
        std::unique_ptr<StreamSeg> u = std::move(flying.front());
        flying.pop_front();
        s->k = s->sum.n_chunks;
        s->first_chunk = chunks_done;
        chunks_done += s->k;
        if (s->final) {
          s->sum.n_chunks = (uint32_t)chunks_done;
          file_sum = s->sum;
        } else {
          s->sum = hbx_file_summary{};
        }
        while (!r && sinking.size() >= (size_t)hbx_ctx::kZStages) r = sdrain_one();  // the stage this one takes
        if (!r && zip) {
          s->stage = (int)(zjobs++ % (uint64_t)hbx_ctx::kZStages);
          std::vector<hbxz::ZBlock> zb;
          uint64_t d = 0, nseg = 0, start = s->prev_cut;
          for (uint64_t i = 0; i < s->k && !r; i++) {
            const uint64_t e = s->cuts[i];
            // a chunk lies inside its segment: it starts in the overlap at the earliest
            if (start < s->off || e < start || e > s->off + s->len) {
              r = c->fail(HBX_ERR_STATE, "a chunk outside its segment (internal)");
              break;
            }
            const uint64_t len = e - start, ns = (len + hbxz::kSeg - 1) / hbxz::kSeg;
            if (set && !s->fresh[i]) {  // seen before: nothing is sent for it
              s->dst.push_back(kNoStream);
            } else {
              zb.push_back(hbxz::ZBlock{reinterpret_cast<uint64_t>(s->arena + (start - s->off)), d, len,
                                        (uint32_t)nseg, (uint32_t)ns});
              s->dst.push_back(d);
              d += (hbx_deflate_bound(len) + 15) & ~uint64_t(15);
              nseg += ns;
            }
            start = e;
          }
          if (!r && !zb.empty()) {
            s->zstarted = true;
            ring_stage[s->ring] = s->stage;
            r = z_launch(c, s->stage, zb, d, nseg);
          }
        }
        if (r) return r;
        std::shared_future<int> prev = sinking.empty() ? std::shared_future<int>() : sinking.back()->fin;
        sinking.push_back(std::move(u));
        s->fin = std::async(std::launch::async, [c, s, prev, zip, sink, user, &worker_rc]() -> int {
                   if (prev.valid()) {  // FIFO: one sink call at a time, in segment order
                     const int r0 = prev.get();
                     if (r0) return r0;
                   }
                   const int r1 = stream_finish(c, *s, zip, sink, user);
                   if (r1) {
                     int none = 0;
                     worker_rc.compare_exchange_strong(none, r1);
                   }
                   return r1;
                 }).share();
        return HBX_OK;
      };
      bool slot_used[2] = {false, false};
      const uint64_t zero = 0;
      uint64_t prev_end = 0, k = 0;
      int r = HBX_OK;
      for (bool more = true; more && r == HBX_OK; k++) {
        if ((r = worker_rc.load())) {  // a sink or a stage failed: read no further
          from_worker = true;
          break;
        }
        uint64_t off = 0, len = 0;
        if ((r = hbx_seg_next(file_len, seg_bytes, prev_end, &off, &len))) {
          r = c->fail(r, "segment layout (internal)");
          break;
        }
        prev_end = off + len;
        more = prev_end < file_len;
        const int p = (int)(k & 1);
        const size_t ring = (size_t)(k % depth);
        DevBuf& arena = c->d_ring[ring];
        const double t0 = now();
        while (r == HBX_OK && flying.size() >= depth) r = collect();  // frees arena k % depth
        if (r) break;
        const double t1 = now();
        if (slot_used[p] && (r = c->hip(hipEventSynchronize(c->h2d_done[p]), "h2d wait"))) break;
        const double t2 = now();
        if (len) r = read_range(fd, path, off, len, c->h_read[p].as<uint8_t>(), std::max(1u, io_threads), c->err);
        c->io_s[0] += now() - t2;
        c->io_s[1] += t1 - t0;
        c->io_s[2] += t2 - t1;
        if (r) break;
        // the arena's previous segment may still be read by its compression job
        if (ring_stage[ring] >= 0 &&
            (r = c->hip(hipStreamWaitEvent(c->stream, c->zs[ring_stage[ring]].done, 0), "hipStreamWaitEvent")))
          break;
        ring_stage[ring] = -1;
        if (len) {
          const auto tc = std::chrono::steady_clock::now();
          if ((r = c->hip(hipMemcpyAsync(arena.p, c->h_read[p].p, len, hipMemcpyHostToDevice, c->stream), "hipMemcpyAsync")))
            break;
          c->max_copy_ms = std::max(c->max_copy_ms, ms_since(tc));
          if ((r = c->hip(hipEventRecord(c->h2d_done[p], c->stream), "hipEventRecord"))) break;
          slot_used[p] = true;
        }
        const uint64_t scap = max_chunks(len);
        std::unique_ptr<StreamSeg> u(new StreamSeg());
        StreamSeg* s = u.get();
        s->off = off;
        s->len = len;
        s->arena = arena.as<uint8_t>();
        s->ring = ring;
        s->final = !more;
        s->cuts.resize(scap);
        s->ids.resize(16 * scap);
        if (set) s->fresh.resize(scap);
        if (zip) {
          s->zoff.resize(scap);
          s->zlen.resize(scap);
        }
        r = seg_submit(c, 1, &h, arena.p, &zero, &len, s->cuts.data(), s->ids.data(), &zero, &scap, &s->sum, budget,
                       set, set ? s->fresh.data() : nullptr);
        if (r) break;
        flying.push_back(std::move(u));
        // hand over every segment whose results have already reached the host
        // (never waiting: neither for the device nor for a busy sink)
        while (r == HBX_OK && !flying.empty()) {
          const Batch* b = c->pending.front();
          if (!b->finalized || hipEventQuery(b->ev[4]) != hipSuccess) break;
          if (sinking.size() >= (size_t)hbx_ctx::kZStages &&
              sinking.front()->fin.wait_for(std::chrono::seconds(0)) != std::future_status::ready)
            break;
          r = collect();
        }
      }
      if (fd >= 0) ::close(fd);
      // collect everything in flight, also after a failure (the batches write
      // into the segments' arrays, which live until nothing is pending)
      const double td = now();
      while (!c->pending.empty()) {
        const std::string keep = c->err;
        const int r2 = r == HBX_OK ? collect() : wait_oldest(c);
        if (r == HBX_OK) r = r2;
        else c->err = keep;
      }
      flying.clear();
      // every worker joined (also after a failure: the stages and the arenas
      // must be idle when this call returns)
      while (!sinking.empty()) {
        if (r == HBX_OK) {
          r = sdrain_one();
        } else {
          const int w = sinking.front()->fin.get();
          if (w && from_worker && !sinking.front()->err.empty()) {
            c->err = sinking.front()->err;
            from_worker = false;
          }
          sinking.pop_front();
        }
      }
      if (r != HBX_OK && zip)
        for (auto& Z : c->zs)
          if (Z.stream) (void)hipStreamSynchronize(Z.stream);
      // the set forgets a failed call's chunks: what a sink already shipped is
      // fresh again next time, which costs only work
      if (r != HBX_OK && set && !c->broken) {
        const std::string keep = c->err;
        (void)idset_truncate(c, set, set_count0);
        c->err = keep;
      }
      c->io_s[1] += now() - td;
      return r;
    }();
  }
  if (rc == HBX_OK && summary) *summary = file_sum;
  const std::string keep = c->err;
  (void)hbx_seg_close(c, h);
  if (rc) c->err = keep;
  return rc;
}

int hbx_host_call_max(hbx_ctx* c, double ms[2], int reset) {
  if (!c || !ms) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  ms[0] = c->max_copy_ms;
  ms[1] = c->max_submit_ms;
  if (reset) c->max_copy_ms = c->max_submit_ms = 0.0;
  return HBX_OK;
}

int hbx_io_times(hbx_ctx* c, double s[3], int reset) {
  if (!c || !s) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  for (int i = 0; i < 3; i++) {
    s[i] = c->io_s[i];
    if (reset) c->io_s[i] = 0.0;
  }
  return HBX_OK;
}

int hbx_memcpy_h2d_async(hbx_ctx* c, void* d, const void* h, uint64_t n) {
  if (!c || (n && (!d || !h))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HBX_TRY(c, hipSetDevice(c->device));
  const auto t0 = std::chrono::steady_clock::now();
  if (int frc = flush_input_wait(c)) return frc;
  g_slow.call("h2d: input wait", t0, c->launches);
  const auto t1 = std::chrono::steady_clock::now();
  HBX_TRY(c, hipMemcpyAsync(d, h, n, hipMemcpyHostToDevice, c->stream));
  c->max_copy_ms = std::max(c->max_copy_ms, ms_since(t1));
  g_slow.call("h2d: hipMemcpyAsync", t1, c->launches);
  return HBX_OK;
}

int hbx_input_after_oldest(hbx_ctx* c) {
  if (!c) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  c->input_fence_set = false;
  if (c->pending.empty()) return HBX_OK;
  HBX_TRY(c, hipSetDevice(c->device));
  Batch* x = c->pending.front();
  // its last MD5 launch must have been issued: drain until it is (a caller
  // that reuses memory this early gets correct results, only slower)
  for (int k = 0; !x->finalized; k++) {
    const uint64_t l0 = c->launches;
    int rc = md5_step(c, kBudgetAll, true);
    if (rc) return rc;
    if (c->launches == l0 || k > 2) return c->fail(HBX_ERR_STATE, "drain launched nothing (internal)");
  }
  if (!x->joined || c->hstream == c->stream) return HBX_OK;  // (empty batch / one stream: in order already)
  // the completion event of the launch that finished it (or of a later one,
  // if that slot has been recorded again since)
  const uint64_t L = c->launches - x->final_launch <= kDoneRing ? x->final_launch : c->launches - 1;
  // (lean marks: nothing to enqueue once the host has seen it complete -- in
  // the steady state it finished two launches ago)
  if (c->lean_marks && hipEventQuery(c->order_free[L % kDoneRing]) == hipSuccess) return HBX_OK;
  c->input_fence_set = true;
  c->input_fence_L = L;
  if (c->lean_marks) {  // enqueued after the next plan (flush_input_wait), off the scan loop
    if (int frc = flush_input_wait(c)) return frc;  // (an earlier one not yet flushed goes first)
    c->input_wait_pending = true;
    c->input_wait_L = L;
    return HBX_OK;
  }
  HBX_TRY(c, hipStreamWaitEvent(c->stream, c->order_free[L % kDoneRing], 0));
  return HBX_OK;
}

int hbx_input_fence(hbx_ctx* c, void* stream) {
  if (!c) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  HBX_TRY(c, hipSetDevice(c->device));
  if (int frc = flush_input_wait(c)) return frc;
  if (!stream || !c->input_fence_set) return HBX_OK;
  // Nothing to wait for once launch L is known complete.  The ring slot of L
  // is recorded again by launch L + kDoneRing: a fence called that late waits for
  // that later launch instead (issued after L on the same stream, so it
  // completes after L: conservative, never early).
  const uint64_t L = c->input_fence_L;
  hipEvent_t e = c->order_free[L % kDoneRing];
  if (L < c->k3_done_upto || hipEventQuery(e) == hipSuccess) {
    c->input_fence_set = false;
    return HBX_OK;
  }
  HBX_TRY(c, hipStreamWaitEvent(static_cast<hipStream_t>(stream), e, 0));
  return HBX_OK;
}

int hbx_after_stream(hbx_ctx* c, void* stream) {
  if (!c) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HBX_TRY(c, hipSetDevice(c->device));
  if (!stream) {
    // The null stream: a blocking scan stream (the CU-masked default) is
    // already ordered after prior null-stream work by the legacy default-
    // stream rule, on the GPU.  Recording an event on the null stream instead
    // would hold the host until the scan stream drains (measured: every
    // submit then waited for the previous batch's K1/K2, 0.3 ms hash-stream
    // gaps per step).
    unsigned flags = 0;
    HBX_TRY(c, hipStreamGetFlags(c->stream, &flags));
    if (!(flags & hipStreamNonBlocking)) return HBX_OK;
  }
  if (!c->producer) HBX_TRY(c, hipEventCreateWithFlags(&c->producer, hipEventDisableTiming));
  HBX_TRY(c, hipEventRecord(c->producer, static_cast<hipStream_t>(stream)));
  HBX_TRY(c, hipStreamWaitEvent(c->stream, c->producer, 0));  // every input read starts on the scan stream
  return HBX_OK;
}

int hbx_alloc_pinned(uint64_t bytes, void** out) {
  if (!out) return HBX_ERR_ARG;
  return hipHostMalloc(out, bytes ? bytes : 1, hipHostMallocDefault) == hipSuccess ? HBX_OK
                                                                                  : HBX_ERR_HIP;
}

int hbx_free_pinned(void* p) {
  if (!p) return HBX_OK;
  return hipHostFree(p) == hipSuccess ? HBX_OK : HBX_ERR_HIP;
}

// ---- block formats (hbx_formats.h) ----------------------------
uint64_t hbx_file_entry_size(const hbx_file_entry* e) { return e ? hbxfmt::entry_size(*e) : 0; }

int hbx_file_entry_serialize(const hbx_file_entry* e, uint8_t* out, uint64_t cap, uint64_t* n) {
  if (!e || (cap && !out) || (e->name_len && !e->name) || (e->link_len && !e->link && e->content_type == 4))
    return HBX_ERR_ARG;
  hbxfmt::Writer w{out, cap};
  hbxfmt::write_entry(w, *e);
  if (!w.ok) return HBX_ERR_CAPACITY;
  if (n) *n = w.n;
  return HBX_OK;
}

int hbx_file_entry_parse(const uint8_t* in, uint64_t len, hbx_file_entry* e, uint64_t* used) {
  if (!e || (len && !in)) return HBX_ERR_ARG;
  hbxfmt::Reader r{in, len};
  if (!hbxfmt::read_entry(r, *e).empty()) return HBX_ERR_FORMAT;
  if (used) *used = r.n;
  return HBX_OK;
}

int hbx_chain_block_serialize(const uint8_t* ids, const uint8_t* keys, uint32_t k, uint8_t* out,
                              uint64_t cap, uint64_t* n) {
  if ((k && !ids) || (cap && !out)) return HBX_ERR_ARG;
  hbxfmt::Writer w{out, cap};
  hbxfmt::write_chain(w, ids, keys, k);
  if (!w.ok) return HBX_ERR_CAPACITY;
  if (n) *n = w.n;
  return HBX_OK;
}

int hbx_chain_block_parse(const uint8_t* in, uint64_t len, uint32_t* k, uint8_t* ids, uint8_t* keys,
                          uint32_t cap) {
  if (!k || (len && !in)) return HBX_ERR_ARG;
  hbxfmt::Reader r{in, len};
  const uint32_t magic = r.u32();
  const uint32_t cnt = r.u32();
  if (!r.ok) return HBX_ERR_FORMAT;
  if (magic != hbxfmt::kMagicChain) return HBX_ERR_FORMAT;  // "corrupted FileChainBlock"
  *k = cnt;
  if ((uint64_t)cnt * 32ull > len - r.n) return HBX_ERR_FORMAT;
  if (cnt > cap && (ids || keys)) return HBX_ERR_CAPACITY;
  for (uint32_t i = 0; i < cnt && (ids || keys); i++) {
    const uint8_t* pair = r.take(32);
    if (ids) std::memcpy(ids + 16ull * i, pair, 16);
    if (keys) std::memcpy(keys + 16ull * i, pair + 16, 16);
  }
  return HBX_OK;
}

uint64_t hbx_directory_block_size(const hbx_file_entry* es, uint32_t n) {
  return (es || !n) ? hbxfmt::dir_size(es, n) : 0;
}

int hbx_directory_block_serialize(const hbx_file_entry* es, uint32_t n, uint8_t* out, uint64_t cap,
                                  uint64_t* n_out, uint8_t* links, uint32_t* n_links) {
  if ((n && !es) || (cap && !out)) return HBX_ERR_ARG;
  hbxfmt::Writer w{out, cap};
  const uint32_t nl = hbxfmt::write_dir(w, es, n, links);
  if (!w.ok) return HBX_ERR_CAPACITY;
  if (n_out) *n_out = w.n;
  if (n_links) *n_links = nl;
  return HBX_OK;
}

int hbx_directory_block_parse(const uint8_t* in, uint64_t len, hbx_file_entry* es, uint32_t cap,
                              uint32_t* n) {
  if (!n || (len && !in)) return HBX_ERR_ARG;
  hbxfmt::Reader r{in, len};
  const uint32_t magic = r.u32();
  const uint32_t cnt = r.u32();
  if (!r.ok || magic != hbxfmt::kMagicDir) return HBX_ERR_FORMAT;  // "corrupted DirectoryBlock"
  *n = cnt;
  for (uint32_t i = 0; i < cnt; i++) {
    hbx_file_entry tmp;
    if (!hbxfmt::read_entry(r, tmp).empty()) return HBX_ERR_FORMAT;
    if (es && i < cap) es[i] = tmp;
  }
  return (es && cnt > cap) ? HBX_ERR_CAPACITY : HBX_OK;
}

int hbx_directory_block_ids(hbx_ctx* c, uint32_t n_dirs, const hbx_file_entry* entries,
                            const uint64_t* entry_base, const uint32_t* n_entries, uint8_t* ids) {
  if (!c || (n_dirs && (!entries || !entry_base || !n_entries || !ids))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (n_dirs == 0) return HBX_OK;
  HBX_TRY(c, hipSetDevice(c->device));
  // every directory block into one host image (256-B aligned, as hbx_verify_blocks
  // lays out its staging), one copy, one K6 launch
  std::vector<uint64_t> offs(n_dirs), lens(n_dirs), link_base(n_dirs);
  std::vector<uint32_t> nls(n_dirs);
  uint64_t total = 0, nlinks = 0;
  for (uint32_t d = 0; d < n_dirs; d++) {
    const hbx_file_entry* es = entries + entry_base[d];
    offs[d] = total;
    lens[d] = hbxfmt::dir_size(es, n_entries[d]);
    total += (lens[d] + 255) & ~uint64_t(255);
    link_base[d] = nlinks;
    for (uint32_t i = 0; i < n_entries[d]; i++) nlinks += hbxfmt::has_content(es[i].content_type) ? 1 : 0;
  }
  std::vector<uint8_t> img(total), links(16 * std::max<uint64_t>(nlinks, 1));
  for (uint32_t d = 0; d < n_dirs; d++) {
    hbxfmt::Writer w{img.data() + offs[d], lens[d]};
    nls[d] = hbxfmt::write_dir(w, entries + entry_base[d], n_entries[d], links.data() + 16 * link_base[d]);
    if (!w.ok) return c->fail(HBX_ERR_ARG, "directory " + std::to_string(d) + ": bad entry");
  }
  HBX_TRY(c, c->d_stage.ensure(total + 65536));
  uint8_t* arena = c->d_stage.as<uint8_t>();
  HBX_TRY(c, hipMemcpyAsync(arena, img.data(), total, hipMemcpyHostToDevice, c->stream));
  return verify_device(c, arena, n_dirs, offs.data(), lens.data(), links.data(), link_base.data(),
                       nls.data(), ids, nullptr, nullptr, nullptr);
}

// ---- zlib block compression (hbx_deflate.hip) -----------------
uint64_t hbx_deflate_bound(uint64_t len) {
  return 11ull + len + 5ull * ((len + hbxz::kSeg - 1) / hbxz::kSeg);
}

namespace {
// K7a -> K7s -> K7b over n blocks at device addresses src[i] (len[i] bytes,
// HBX_ARENA_SLACK readable after each) into device streams dst[i].
int deflate_device(hbx_ctx* c, uint64_t n, const uint64_t* src, const uint64_t* lens, const uint64_t* dst,
                   uint64_t* out_lens) {
  if (n == 0) return HBX_OK;
  if (n > 0xFFFFFFFFull) return c->fail(HBX_ERR_ARG, "too many blocks");
  std::vector<hbxz::ZBlock> zb(n);
  uint64_t nseg = 0;
  for (uint64_t i = 0; i < n; i++) {
    const uint64_t ns = (lens[i] + hbxz::kSeg - 1) / hbxz::kSeg;
    zb[i] = hbxz::ZBlock{src[i], dst[i], lens[i], (uint32_t)nseg, (uint32_t)ns};
    nseg += ns;
    if (nseg > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "too much data in one call");
  }
  hipStream_t s = c->stream;
  HBX_TRY(c, c->d_zblk.ensure(n * sizeof(hbxz::ZBlock)));
  HBX_TRY(c, c->d_zinfo.ensure(std::max<uint64_t>(nseg, 1) * sizeof(hbxz::SegInfo)));
  HBX_TRY(c, c->d_zoff.ensure(std::max<uint64_t>(nseg, 1) * 8));
  HBX_TRY(c, c->d_zlen.ensure(n * 8));
  HBX_TRY(c, c->d_zimg.ensure(std::max<uint64_t>(nseg, 1) * hbxz::kSlot));
  HBX_TRY(c, hipMemcpyAsync(c->d_zblk.p, zb.data(), n * sizeof(hbxz::ZBlock), hipMemcpyHostToDevice, s));
  const hbxz::ZBlock* dz = c->d_zblk.as<hbxz::ZBlock>();
  if (nseg) {
    hipLaunchKernelGGL(hbx_k7_deflate_entropy, dim3((uint32_t)nseg), dim3(hbxz::kEThreads), 0, s, dz, (uint32_t)n,
                       (uint32_t)nseg, c->d_zinfo.as<hbxz::SegInfo>());
    hipLaunchKernelGGL(hbx_k7_deflate_size, dim3((uint32_t)nseg), dim3(hbxz::kThreads), 0, s, dz, (uint32_t)n,
                       (uint32_t)nseg, c->d_zinfo.as<hbxz::SegInfo>(), c->d_zimg.as<uint32_t>());
    hipLaunchKernelGGL(hbx_k7_deflate_code, dim3((uint32_t)nseg), dim3(hbxz::kThreads), 0, s, dz, (uint32_t)n,
                       (uint32_t)nseg, c->d_zinfo.as<hbxz::SegInfo>(), c->d_zimg.as<uint32_t>());
    HBX_TRY(c, hipGetLastError());
  }
  hipLaunchKernelGGL(hbx_k7_deflate_plan, dim3((uint32_t)n), dim3(64), 0, s, dz, (uint32_t)n,
                     c->d_zinfo.as<hbxz::SegInfo>(), c->d_zoff.as<uint64_t>(), c->d_zlen.as<uint64_t>());
  HBX_TRY(c, hipGetLastError());
  if (nseg) {
    hipLaunchKernelGGL(hbx_k7_deflate_write, dim3((uint32_t)nseg), dim3(hbxz::kWThreads), 0, s, (uint32_t)nseg,
                       c->d_zinfo.as<hbxz::SegInfo>(), c->d_zimg.as<uint32_t>(), c->d_zoff.as<uint64_t>(), dz,
                       (uint32_t)n);
    HBX_TRY(c, hipGetLastError());
  }
  HBX_TRY(c, hipMemcpyAsync(out_lens, c->d_zlen.p, n * 8, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  return HBX_OK;
}
}  // namespace

int hbx_deflate_blocks_device(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                              const uint64_t* lens, void* d_out, const uint64_t* out_offs,
                              const uint64_t* out_caps, uint64_t* out_lens) {
  if (!c || (n && (!d_arena || !offs || !lens || !d_out || !out_offs || !out_caps || !out_lens)))
    return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  std::vector<uint64_t> src(n), dst(n);
  for (uint64_t i = 0; i < n; i++) {
    if (out_caps[i] < hbx_deflate_bound(lens[i]))
      return c->fail(HBX_ERR_CAPACITY, "output capacity below hbx_deflate_bound for block " + std::to_string(i));
    src[i] = reinterpret_cast<uint64_t>(d_arena) + offs[i];
    dst[i] = reinterpret_cast<uint64_t>(d_out) + out_offs[i];
  }
  return deflate_device(c, n, src.data(), lens, dst.data(), out_lens);
}

int hbx_deflate_blocks(hbx_ctx* c, uint64_t n, const uint8_t* const* datas, const uint64_t* lens,
                       uint8_t* const* outs, const uint64_t* caps, uint64_t* out_lens) {
  if (!c || (n && (!datas || !lens || !outs || !caps || !out_lens))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (n == 0) return HBX_OK;
  HBX_TRY(c, hipSetDevice(c->device));
  std::vector<uint64_t> soff(n), doff(n), src(n), dst(n);
  uint64_t sin = 0, sout = 0;
  for (uint64_t i = 0; i < n; i++) {
    if (lens[i] && !datas[i]) return c->fail(HBX_ERR_ARG, "null block data");
    if (caps[i] < hbx_deflate_bound(lens[i]))
      return c->fail(HBX_ERR_CAPACITY, "output capacity below hbx_deflate_bound for block " + std::to_string(i));
    soff[i] = sin;
    sin += (lens[i] + 255) & ~uint64_t(255);
    doff[i] = sout;
    sout += (hbx_deflate_bound(lens[i]) + 15) & ~uint64_t(15);
  }
  HBX_TRY(c, c->d_stage.ensure(sin + 65536));
  HBX_TRY(c, c->d_zout.ensure(sout + 64));
  uint8_t* arena = c->d_stage.as<uint8_t>();
  uint8_t* zo = c->d_zout.as<uint8_t>();
  for (uint64_t i = 0; i < n; i++) {
    if (lens[i]) HBX_TRY(c, hipMemcpyAsync(arena + soff[i], datas[i], lens[i], hipMemcpyHostToDevice, c->stream));
    src[i] = reinterpret_cast<uint64_t>(arena + soff[i]);
    dst[i] = reinterpret_cast<uint64_t>(zo + doff[i]);
  }
  const int rc = deflate_device(c, n, src.data(), lens, dst.data(), out_lens);
  if (rc) return rc;
  std::vector<uint8_t> host(sout);
  HBX_TRY(c, hipMemcpy(host.data(), zo, sout, hipMemcpyDeviceToHost));
  for (uint64_t i = 0; i < n; i++) std::memcpy(outs[i], host.data() + doff[i], out_lens[i]);
  return HBX_OK;
}

// ---- wire protocol framing (hbx_wire.h) -----------------------
int hbx_wire_encode_id(uint16_t num, uint32_t type, const uint8_t id[16], uint8_t out[22]) {
  if (!id || !out || !hbxwire::is_id_msg(type)) return HBX_ERR_ARG;
  hbxfmt::Writer w{out, 22};
  const uint8_t nb[2] = {(uint8_t)(num >> 8), (uint8_t)num};
  w.bytes(nb, 2);
  w.u32(type);
  w.bytes(id, 16);
  return w.ok ? HBX_OK : HBX_ERR_CAPACITY;
}

int hbx_wire_encode_block_header(uint16_t num, uint32_t type, const uint8_t id[16], const uint8_t* links,
                                 uint32_t n_links, uint8_t data_type, uint32_t data_len, uint8_t* out,
                                 uint64_t cap, uint64_t* n) {
  if (!id || (n_links && !links) || (cap && !out) || !hbxwire::is_block_msg(type)) return HBX_ERR_ARG;
  hbxfmt::Writer w{out, cap};
  const uint8_t nb[2] = {(uint8_t)(num >> 8), (uint8_t)num};
  w.bytes(nb, 2);
  w.u32(type);
  w.bytes(id, 16);  // HashboxBlock.Serialize, block.go:56-69
  w.u32(n_links);
  w.bytes(links, 16ull * n_links);
  w.u8(data_type);
  w.u32(data_len);
  if (!w.ok) return HBX_ERR_CAPACITY;
  if (n) *n = w.n;
  return HBX_OK;
}

int hbx_wire_parse(const uint8_t* in, uint64_t len, hbx_wire_msg* msg) {
  if (!msg || (len && !in)) return HBX_ERR_ARG;
  return hbxwire::parse(in, len, msg);
}

int hbx_verify_submit_device(hbx_ctx* c, const void* d_arena, uint64_t n, const uint64_t* offs,
                             const uint64_t* lens, const uint8_t* links, const uint64_t* link_base,
                             const uint32_t* n_links, uint8_t* ids, const uint8_t* expect, uint8_t* ok,
                             uint64_t* n_bad) {
  if (!c || (n && (!d_arena || !offs || !lens))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  HBX_TRY(c, hipSetDevice(c->device));
  if (n_bad) *n_bad = 0;
  return submit_verify(c, static_cast<const uint8_t*>(d_arena), n, offs, lens, links, link_base, n_links, ids,
                       expect, ok, n_bad, c->md5_slice ? c->md5_slice : kBudgetAll);
}

// ---- zlib inflate (hbx_inflate.hip) -----------------------------------------
// K8 / K8s over n streams (the context locked, nothing pending): what
// hbx_inflate_blocks_device and the restore path (hbx_restore_*) share.
// out_hint (NULL: out_caps) is what the choice of kernel and the split path's
// scratch are sized by: the restore path knows no stream's inflated size, so
// its capacities are all max_block and say nothing; it passes an estimate from
// the compressed length instead.  A stream that outgrows the estimate is
// inflated again by the wave kernel, as any split overflow is; the bounds every
// kernel checks are out_caps.  d_in (and d_out) may be NULL with absolute
// device addresses in in_offs (out_offs): only their integer sum is used.
static int inflate_device(hbx_ctx* c, const void* d_in, uint64_t n, const uint64_t* in_offs,
                          const uint64_t* in_lens, void* d_out, const uint64_t* out_offs,
                          const uint64_t* out_caps, uint64_t* out_lens, uint32_t* status,
                          const uint64_t* out_hint = nullptr) {
  if (n == 0) return HBX_OK;
  if (!out_hint) out_hint = out_caps;
  if (n > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "too many streams");
  HBX_TRY(c, hipSetDevice(c->device));
  // one wave per stream, longest first (the long ones start first)
  std::vector<uint32_t> perm(n);
  for (uint64_t i = 0; i < n; i++) {
    if (in_lens[i] > 0xFFFFFFFFull || out_caps[i] > 0xFFFFFFFFull) return c->fail(HBX_ERR_ARG, "stream too large");
    perm[i] = (uint32_t)i;
  }
  std::stable_sort(perm.begin(), perm.end(), [&](uint32_t a, uint32_t b) { return in_lens[a] > in_lens[b]; });
  // a wave per stream, except for tens of thousands of short compressible
  // streams, where 64 streams per wave (one per lane) keep more streams in
  // flight, and for long compressible streams when few of them fill the GPU:
  // those are split into regions decoded in parallel (hbx_inflate_split.hip).
  // HBX_K8_MODE=lane|wave|split forces one (tests; split then takes every
  // stream of >= 2 regions, compressible or not).
  uint64_t tin = 0, tcap = 0;
  for (uint64_t i = 0; i < n; i++) {
    tin += in_lens[i];
    tcap += out_hint[i];
  }
  bool lanes = n >= 8192 && tin * 10 < tcap * 7 && tcap / n <= (256u << 10);
  const char* mode = ab_env("HBX_K8_MODE");
  if (mode) lanes = std::strcmp(mode, "lane") == 0;
  const bool force_split = mode && std::strcmp(mode, "split") == 0;
  const bool no_split = lanes || (mode && std::strcmp(mode, "wave") == 0);
  auto splits = [&](uint32_t i) {
    if (no_split || in_lens[i] < 2ull * hbxs::kSplitRegion) return false;
    return force_split || in_lens[i] * 10 < out_hint[i] * 8;
  };
  // Scratch of one split stream: regions of kSplitRegion compressed bytes,
  // each with room for twice its share of the stream's output capacity in
  // 16-bit symbols, at most kSplitSymCap (a region that needs more overflows
  // and the stream is inflated again by the wave kernel).
  constexpr uint64_t kSplitSymCap = 4ull << 20;
  auto region_syms = [&](uint64_t len, uint64_t cap, uint32_t& cnt) {
    cnt = (uint32_t)((len + hbxs::kSplitRegion - 1) / hbxs::kSplitRegion);
    const uint64_t share = (2ull * cap + cnt - 1) / cnt;
    return std::min<uint64_t>(((share + 63) & ~63ull) + 4096, kSplitSymCap);
  };
  uint64_t long_streams = 0;
  for (uint64_t i = 0; i < n; i++) long_streams += splits(perm[i]) ? 1 : 0;
  // enough streams to fill the SIMDs on their own: no split (it costs a
  // second pass over 2 bytes per output byte)
  bool split_any = long_streams > 0 && (force_split || long_streams < 2048);
  // The split path's scratch has a budget (a quarter of the free device
  // memory, at most 16 GiB): the longest candidates take it in order, the
  // rest go to the wave kernel, which needs no scratch (advisor r04).
  std::vector<uint8_t> take(n, 0);
  if (split_any) {
    size_t fr = 0, tot = 0;
    uint64_t budget = 256ull << 20;
    if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::max<uint64_t>(budget, std::min<uint64_t>(fr / 4, 16ull << 30));
    uint64_t used = 0;
    long_streams = 0;
    for (uint64_t k = 0; k < n; k++) {
      const uint32_t i = perm[k];
      if (!splits(i)) continue;
      uint32_t cnt = 0;
      const uint64_t syms = region_syms(in_lens[i], out_hint[i], cnt);
      const uint64_t b = 2ull * syms * cnt;  // scratch bytes of its regions
      if (used + b > budget) continue;
      used += b;
      take[i] = 1;
      long_streams++;
    }
    split_any = long_streams > 0;
  }
  // split streams last, so the wave kernel takes the prefix [0, nw)
  if (split_any)
    std::stable_partition(perm.begin(), perm.end(), [&](uint32_t i) { return !take[i]; });
  uint64_t nw = split_any ? n - long_streams : n;
  std::vector<InflateDesc> desc(n);
  for (uint64_t k = 0; k < n; k++) {
    const uint32_t i = perm[k];
    desc[k].src = reinterpret_cast<uint64_t>(d_in) + in_offs[i];
    desc[k].dst = reinterpret_cast<uint64_t>(d_out) + out_offs[i];
    desc[k].len = (uint32_t)in_lens[i];
    desc[k].cap = (uint32_t)out_caps[i];
  }
  hipStream_t s = c->stream;
  HBX_TRY(c, c->d_idesc.ensure(n * sizeof(InflateDesc)));
  HBX_TRY(c, c->d_ires.ensure(n * 8));
  // The region table and every split buffer exist before the first kernel is
  // queued: a failure then leaves nothing running, and an allocation that
  // fails sends those streams to the wave kernel instead of failing the call.
  std::vector<SplitRegion> reg;
  std::vector<uint32_t> meta;
  if (split_any) {
    meta.assign(3 * (n - nw), 0u);
    uint64_t sym = 0;
    for (uint64_t k = nw; k < n; k++) {
      uint32_t cnt = 0;
      const uint32_t scap = (uint32_t)region_syms(desc[k].len, out_hint[perm[k]], cnt);
      meta[k - nw] = (uint32_t)k;
      meta[(n - nw) + (k - nw)] = (uint32_t)reg.size();
      meta[2 * (n - nw) + (k - nw)] = cnt;
      const uint32_t first = (uint32_t)reg.size();
      for (uint32_t r = 0; r < cnt; r++) {
        reg.push_back(SplitRegion{(uint32_t)k, r, first, cnt, sym, scap, 0u});
        sym += scap;
      }
    }
    const uint64_t nreg = reg.size();
    bool ok = nreg <= 0x7FFFFFFFull;
    for (auto [buf, bytes] : {std::pair<DevBuf*, uint64_t>{&c->d_sreg, nreg * sizeof(SplitRegion)},
                              {&c->d_sstart, nreg * 8}, {&c->d_sres, nreg * sizeof(SplitResult)},
                              {&c->d_sscratch, sym * 2 + 64}, {&c->d_smeta, meta.size() * 4}})
      if (ok && buf->ensure(bytes) != hipSuccess) {
        (void)hipGetLastError();  // the failed allocation is not an error of this call
        ok = false;
      }
    if (!ok) {  // every stream to the wave kernel
      split_any = false;
      nw = n;
    }
  }
  HBX_TRY(c, hipMemcpyAsync(c->d_idesc.p, desc.data(), n * sizeof(InflateDesc), hipMemcpyHostToDevice, s));
  uint32_t* dres = c->d_ires.as<uint32_t>();
  const InflateDesc* ddesc = c->d_idesc.as<InflateDesc>();
  if (nw && lanes)
    hipLaunchKernelGGL(hbx_k8_inflate_lanes, dim3((uint32_t)((nw + 63) / 64)), dim3(64), 0, s, ddesc, (uint32_t)nw,
                       dres, dres + n);
  else if (nw)
    hipLaunchKernelGGL(hbx_k8_inflate, dim3((uint32_t)nw), dim3(64), 0, s, ddesc, (uint32_t)nw, dres, dres + n);
  HBX_TRY(c, hipGetLastError());
  if (split_any) {
    const uint64_t nreg = reg.size(), ns = n - nw;
    HBX_TRY(c, hipMemcpyAsync(c->d_sreg.p, reg.data(), nreg * sizeof(SplitRegion), hipMemcpyHostToDevice, s));
    HBX_TRY(c, hipMemcpyAsync(c->d_smeta.p, meta.data(), meta.size() * 4, hipMemcpyHostToDevice, s));
    const SplitRegion* dreg = c->d_sreg.as<SplitRegion>();
    uint64_t* dstart = c->d_sstart.as<uint64_t>();
    SplitResult* dsres = c->d_sres.as<SplitResult>();
    const uint32_t* dmeta = c->d_smeta.as<uint32_t>();
    hipLaunchKernelGGL(hbx_k8s_find, dim3((uint32_t)nreg), dim3(64), 0, s, ddesc, dreg, (uint32_t)nreg, dstart);
    hipLaunchKernelGGL(hbx_k8s_decode, dim3((uint32_t)nreg), dim3(64), 0, s, ddesc, dreg, (uint32_t)nreg,
                       static_cast<const uint64_t*>(dstart), c->d_sscratch.as<uint16_t>(), dsres);
    hipLaunchKernelGGL(hbx_k8s_resolve, dim3((uint32_t)ns), dim3(256), 0, s, ddesc, dmeta, dmeta + ns, dmeta + 2 * ns,
                       (uint32_t)ns, dreg, static_cast<const uint64_t*>(dstart),
                       static_cast<const SplitResult*>(dsres), static_cast<const uint16_t*>(c->d_sscratch.as<uint16_t>()),
                       dres, dres + n);
    HBX_TRY(c, hipGetLastError());
  }
  std::vector<uint32_t> res(2 * n);
  HBX_TRY(c, hipMemcpyAsync(res.data(), dres, n * 8, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  if (split_any) {  // the streams the split path did not resolve: the wave kernel, from scratch
    std::vector<InflateDesc> again;
    std::vector<uint64_t> at;
    for (uint64_t k = nw; k < n; k++)
      if (res[n + k] != 0u) {
        again.push_back(desc[k]);
        at.push_back(k);
      }
    c->k8_split_fallbacks += again.size();
    c->k8_split_streams += n - nw;
    if (!again.empty()) {
      const uint64_t m = again.size();
      HBX_TRY(c, hipMemcpyAsync(c->d_idesc.p, again.data(), m * sizeof(InflateDesc), hipMemcpyHostToDevice, s));
      hipLaunchKernelGGL(hbx_k8_inflate, dim3((uint32_t)m), dim3(64), 0, s, ddesc, (uint32_t)m, dres, dres + m);
      HBX_TRY(c, hipGetLastError());
      std::vector<uint32_t> r2(2 * m);
      HBX_TRY(c, hipMemcpyAsync(r2.data(), dres, m * 8, hipMemcpyDeviceToHost, s));
      HBX_TRY(c, hipStreamSynchronize(s));
      for (uint64_t q = 0; q < m; q++) {
        res[at[q]] = r2[q];
        res[n + at[q]] = r2[m + q];
      }
    }
  }
  for (uint64_t k = 0; k < n; k++) {
    out_lens[perm[k]] = res[k];
    status[perm[k]] = res[n + k];
  }
  // the split scratch is not kept past the call once it is large (the stream
  // is idle here: everything above was synchronized)
  if (c->d_sscratch.cap > (256ull << 20)) c->d_sscratch.release();
  return HBX_OK;
}

int hbx_inflate_blocks_device(hbx_ctx* c, const void* d_in, uint64_t n, const uint64_t* in_offs,
                              const uint64_t* in_lens, void* d_out, const uint64_t* out_offs,
                              const uint64_t* out_caps, uint64_t* out_lens, uint32_t* status) {
  if (!c || (n && (!d_in || !in_offs || !in_lens || !d_out || !out_offs || !out_caps || !out_lens || !status)))
    return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  return inflate_device(c, d_in, n, in_offs, in_lens, d_out, out_offs, out_caps, out_lens, status);
}

}  // extern "C"

// ---- restore and diff (hbx_restore.hip, K10) ----------------------------------
namespace {

constexpr uint64_t kRestoreMaxBlock = 1ull << 30;  // largest max_block accepted (lengths stay well inside 32 bits)

inline uint64_t restore_mb(uint64_t max_block) { return max_block ? max_block : (uint64_t)HBX_MAX_BLOCK; }
// One inflate slot: the block's capacity, K6's read slack, a multiple of 256.
inline uint64_t restore_stride(uint64_t mb) { return (mb + 256ull + 255ull) & ~255ull; }

// One window of a block chain, its data fields already in device memory.
struct RestoreWin {
  uint64_t n = 0;
  const uint64_t* src = nullptr;   // device address of block i's data field
  const uint64_t* lens = nullptr;  // its length
  const uint8_t* types = nullptr;  // HBX_BLOCK_RAW / HBX_BLOCK_ZLIB
  const uint8_t* expect = nullptr; // 16 n: the expected BlockIDs
  const uint8_t* links = nullptr;  // as hbx_verify_blocks (may all be NULL)
  const uint64_t* link_base = nullptr;
  const uint32_t* n_links = nullptr;
  uint64_t max_block = HBX_MAX_BLOCK;
  uint64_t* offs = nullptr;     // out, n + 1: byte offsets in the window, valid up to offs[n_good]
  uint32_t* status = nullptr;   // in: 0, or 8 from the caller's pre-check; out: the block's status
  uint64_t n_good = 0;          // out: leading blocks with status 0
  uint64_t first_diff = hbxr::kNoDiff;  // out (diff): smallest differing offset inside the good prefix
};

// What the window's blocks are put into: a contiguous image (device or pinned
// host memory, `cap` bytes), or compared with: `local(total, &d, &avail)` must
// leave the local copy's bytes [0, avail) of this window at device address d
// on the result stream (avail <= total).  Neither: the blocks are only
// inflated and verified (the rest of a chain after its first bad block).
using RestoreLocalFn = std::function<int(uint64_t, const uint8_t**, uint64_t*)>;

// The image is the engine's own buffer and starts kImageLead bytes into it:
// the kImageGuard bytes before image[0] and after image[total) hold a pattern
// while K10 runs and are checked after it, so a gather that wrote outside
// [0, total) fails the call instead of passing unseen (the caller's buffer is
// filled by a copy of exactly the good prefix and could never show it).
constexpr uint64_t kImageLead = 256, kImageGuard = 64;
constexpr uint8_t kGuardByte = 0xC3;

// Inflate (K8 / K8s, on the scan stream), then VerifyBlock (K6, scan stream)
// beside the gather or diff (K10, result stream): both read the slots, neither
// waits for the other.  K10 covers the blocks that inflated; the caller keeps
// what lies before offs[n_good].  Synchronous: every stream it used is idle on
// return, also on failure.
int restore_window(hbx_ctx* c, RestoreWin& w, uint8_t* image, uint64_t cap, bool image_on_host,
                   const RestoreLocalFn* local) {
  const uint64_t n = w.n;
  w.n_good = 0;
  w.first_diff = hbxr::kNoDiff;
  w.offs[0] = 0;
  if (n == 0) return HBX_OK;
  const uint64_t stride = restore_stride(w.max_block);
  HBX_TRY(c, c->d_rword.ensure(4096));
  // 1. inflate the zlib blocks into their slots; the lengths come back to the host
  std::vector<uint64_t> zi, in_offs, in_lens, out_offs, out_caps, out_hint, out_lens;
  std::vector<uint32_t> zst;
  for (uint64_t i = 0; i < n; i++)
    if (w.status[i] == 0 && w.types[i] == HBX_BLOCK_ZLIB) {
      zi.push_back(i);
      in_offs.push_back(w.src[i]);
      in_lens.push_back(w.lens[i]);
      out_offs.push_back((zi.size() - 1) * stride);
      out_caps.push_back(w.max_block);
      // (text compresses 3:1 to 4:1; the split path leaves room for twice the hint)
      out_hint.push_back(std::min<uint64_t>(w.max_block, 8 * w.lens[i] + 4096));
    }
  const uint64_t nz = zi.size();
  const auto t_inflate = std::chrono::steady_clock::now();
  out_lens.assign(nz, 0);
  zst.assign(nz, 0);
  if (nz) {
    HBX_TRY(c, c->d_rslots.ensure(nz * stride + 65536));
    if (int rc = inflate_device(c, nullptr, nz, in_offs.data(), in_lens.data(), c->d_rslots.p, out_offs.data(),
                                out_caps.data(), out_lens.data(), zst.data(), out_hint.data()))
      return rc;
  }
  c->restore_ms[1] += ms_since(t_inflate);
  const auto t_verify = std::chrono::steady_clock::now();
  std::vector<uint64_t> addr(n), dlen(n);
  const uint64_t nowhere = reinterpret_cast<uint64_t>(c->d_rword.p);
  for (uint64_t i = 0; i < n; i++) {
    addr[i] = nowhere;
    dlen[i] = 0;
    if (w.status[i] == 0 && w.types[i] == HBX_BLOCK_RAW) {
      if (w.lens[i] > w.max_block) {
        w.status[i] = hbxi::kErrOutput;
      } else {
        addr[i] = w.src[i];
        dlen[i] = w.lens[i];
      }
    }
  }
  for (uint64_t k = 0; k < nz; k++) {
    const uint64_t i = zi[k];
    w.status[i] = zst[k];
    if (zst[k] == 0) {
      addr[i] = reinterpret_cast<uint64_t>(c->d_rslots.p) + out_offs[k];
      dlen[i] = out_lens[k];
    }
  }
  // 2. the prefix sum over the blocks that may still be good, and their pieces
  uint64_t m = 0;
  while (m < n && w.status[m] == 0) {
    w.offs[m + 1] = w.offs[m] + dlen[m];
    m++;
  }
  const uint64_t total = w.offs[m];
  hipStream_t rs = c->rstream;
  const uint8_t* d_local = nullptr;
  uint64_t avail = 0;
  const bool diff = local != nullptr && *local;
  if (diff) {
    if (int rc = (*local)(total, &d_local, &avail)) return rc;
    avail = std::min(avail, total);
  } else if (image && total > cap) {
    return c->fail(HBX_ERR_CAPACITY, "restore: the window's image is too small");
  }
  const uint64_t cover = diff ? avail : (image ? total : 0);  // bytes K10 touches
  std::vector<hbxr::Piece> pieces;
  for (uint64_t i = 0; i < m && w.offs[i] < cover; i++) {
    const uint64_t len = std::min(dlen[i], cover - w.offs[i]);
    for (uint64_t p = 0; p < len; p += hbxr::kPiece)
      pieces.push_back(hbxr::Piece{addr[i] + p, w.offs[i] + p, (uint32_t)std::min<uint64_t>(hbxr::kPiece, len - p), 0u});
  }
  if (pieces.size() > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "restore: window too large");
  uint64_t word = hbxr::kNoDiff;
  uint8_t guard[2 * kImageGuard];
  std::memset(guard, kGuardByte, sizeof guard);
  const bool guarded = !diff && image && !pieces.empty();
  int krc = HBX_OK;
  if (!pieces.empty()) {
    krc = [&]() -> int {
      HBX_TRY(c, c->d_rpiece.ensure(pieces.size() * sizeof(hbxr::Piece)));
      HBX_TRY(c, hipMemcpyAsync(c->d_rpiece.p, pieces.data(), pieces.size() * sizeof(hbxr::Piece),
                                hipMemcpyHostToDevice, rs));
      if (diff) {
        HBX_TRY(c, hipMemsetAsync(c->d_rword.p, 0xFF, 8, rs));
        hipLaunchKernelGGL(hbx_k10_diff, dim3((uint32_t)pieces.size()), dim3(hbxr::kThreads), 0, rs,
                           c->d_rpiece.as<hbxr::Piece>(), (uint32_t)pieces.size(), d_local,
                           c->d_rword.as<unsigned long long>());
        HBX_TRY(c, hipGetLastError());
        HBX_TRY(c, hipMemcpyAsync(&word, c->d_rword.p, 8, hipMemcpyDeviceToHost, rs));
      } else {
        if (image_on_host) {
          std::memset(image - kImageGuard, kGuardByte, kImageGuard);
          std::memset(image + total, kGuardByte, kImageGuard);
        } else {
          HBX_TRY(c, hipMemsetAsync(image - kImageGuard, kGuardByte, kImageGuard, rs));
          HBX_TRY(c, hipMemsetAsync(image + total, kGuardByte, kImageGuard, rs));
        }
        hipLaunchKernelGGL(hbx_k10_gather, dim3((uint32_t)pieces.size()), dim3(hbxr::kThreads), 0, rs,
                           c->d_rpiece.as<hbxr::Piece>(), (uint32_t)pieces.size(), image);
        HBX_TRY(c, hipGetLastError());
        if (!image_on_host) {
          HBX_TRY(c, hipMemcpyAsync(guard, image - kImageGuard, kImageGuard, hipMemcpyDeviceToHost, rs));
          HBX_TRY(c, hipMemcpyAsync(guard + kImageGuard, image + total, kImageGuard, hipMemcpyDeviceToHost, rs));
        }
      }
      return HBX_OK;
    }();
  }
  // 3. VerifyBlock of every block that inflated, links passed through
  std::vector<uint32_t> nl(n, 0u);
  if (w.n_links)
    for (uint64_t i = 0; i < n; i++)
      if (w.status[i] == 0) nl[i] = w.n_links[i];
  std::vector<uint8_t> ok(n, 0);
  int vrc = krc ? HBX_OK
                : verify_device(c, nullptr, n, addr.data(), dlen.data(), w.links, w.link_base, nl.data(), nullptr,
                                w.expect, ok.data(), nullptr);
  const std::string verr = c->err;
  const int src_ = c->hip(hipStreamSynchronize(rs), "hipStreamSynchronize(result stream)");
  c->restore_ms[2] += ms_since(t_verify);
  if (krc) return krc;
  if (vrc) return c->fail(vrc, verr);
  if (src_) return src_;
  if (guarded) {
    if (image_on_host) {
      std::memcpy(guard, image - kImageGuard, kImageGuard);
      std::memcpy(guard + kImageGuard, image + total, kImageGuard);
    }
    for (uint8_t b : guard)
      if (b != kGuardByte) return c->fail(HBX_ERR_STATE, "restore: K10 wrote outside the image");
  }
  for (uint64_t i = 0; i < n; i++)
    if (w.status[i] == 0 && !ok[i]) w.status[i] = 7;
  while (w.n_good < n && w.status[w.n_good] == 0) w.n_good++;
  if (word < w.offs[w.n_good]) w.first_diff = word;
  return HBX_OK;
}

}  // namespace

extern "C" {

uint64_t hbx_restore_in_bound(uint64_t max_block) {
  const uint64_t mb = restore_mb(max_block);
  return hbx_deflate_bound(mb) + 64;
}

int hbx_restore_blocks(hbx_ctx* c, uint64_t n, const uint8_t* const* datas, const uint64_t* lens,
                       const uint8_t* types, const uint8_t* expect, const uint8_t* links,
                       const uint64_t* link_base, const uint32_t* n_links, uint64_t max_block, uint8_t* out,
                       uint64_t out_cap, const uint8_t* local, uint64_t local_len, uint64_t* offs,
                       uint32_t* status, uint64_t* n_good, uint64_t* first_diff) {
  if (!c || !offs || !n_good || (n && (!datas || !lens || !types || !expect || !status))) return HBX_ERR_ARG;
  if ((out != nullptr) == (local != nullptr)) return HBX_ERR_ARG;  // exactly one target
  if (local && !first_diff) return HBX_ERR_ARG;
  const uint64_t mb = restore_mb(max_block);
  if (mb > kRestoreMaxBlock || n > 0x7FFFFFFFull) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  const uint64_t bound = hbx_restore_in_bound(mb), stride = restore_stride(mb);
  for (double& t : c->restore_ms) t = 0.0;
  offs[0] = 0;
  *n_good = 0;
  if (first_diff) *first_diff = hbxr::kNoDiff;
  for (uint64_t i = 0; i < n; i++) {
    const bool known = types[i] == HBX_BLOCK_RAW || types[i] == HBX_BLOCK_ZLIB;
    status[i] = (!known || lens[i] > bound) ? 8u : 0u;
    if (status[i] == 0 && lens[i] && !datas[i]) return c->fail(HBX_ERR_ARG, "null block data");
  }
  // Windows of as many blocks as a slot budget holds (a quarter of the free
  // device memory, at most 64 GiB): every zlib block needs a slot of max_block.
  size_t fr = 0, tot = 0;
  uint64_t budget = 1ull << 30;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess) budget = std::max<uint64_t>(budget, std::min<uint64_t>(fr / 4, 64ull << 30));
  const uint64_t per = std::max<uint64_t>(1, budget / stride);
  bool stopped = false;  // a bad block was met: the rest is only inflated and verified, for its status
  uint64_t found = hbxr::kNoDiff;
  std::vector<uint64_t> src, woffs;
  for (uint64_t a = 0; a < n; a += per) {
    const uint64_t b = std::min(n, a + per), wn = b - a;
    // stage the data fields: zlib streams at 16-byte boundaries (K8's vector
    // loads), raw blocks packed byte by byte behind whatever precedes them
    const auto t_stage = std::chrono::steady_clock::now();
    src.assign(wn, 0);
    uint64_t pos = 0;
    for (uint64_t i = a; i < b; i++) {
      if (status[i]) continue;
      if (types[i] == HBX_BLOCK_ZLIB) pos = (pos + 15) & ~15ull;
      src[i - a] = pos;
      pos += lens[i];
    }
    HBX_TRY(c, c->d_rin[0].ensure(pos + 65536));
    uint8_t* din = c->d_rin[0].as<uint8_t>();
    for (uint64_t i = a; i < b; i++) {
      if (status[i] == 0 && lens[i])
        HBX_TRY(c, hipMemcpyAsync(din + src[i - a], datas[i], lens[i], hipMemcpyHostToDevice, c->stream));
      src[i - a] += reinterpret_cast<uint64_t>(din);
    }
    HBX_TRY(c, hipStreamSynchronize(c->stream));
    c->restore_ms[0] += ms_since(t_stage);
    RestoreWin w;
    w.n = wn;
    w.src = src.data();
    w.lens = lens + a;
    w.types = types + a;
    w.expect = expect + 16 * a;
    w.links = links;
    w.link_base = link_base ? link_base + a : nullptr;
    w.n_links = n_links ? n_links + a : nullptr;
    w.max_block = mb;
    woffs.assign(wn + 1, 0);
    w.offs = woffs.data();
    w.status = status + a;
    const uint64_t base = offs[a];
    uint8_t* image = nullptr;
    uint64_t cap = 0;
    if (!stopped && out) {  // (the image's size is known only after the inflate: the window's upper bound)
      uint64_t ub = 0;
      for (uint64_t i = a; i < b; i++) ub += status[i] ? 0 : (types[i] == HBX_BLOCK_RAW ? lens[i] : mb);
      cap = std::min<uint64_t>(ub, wn * mb);
      HBX_TRY(c, c->d_rimg.ensure(kImageLead + cap + kImageGuard));
      image = c->d_rimg.as<uint8_t>() + kImageLead;
    }
    RestoreLocalFn lf;
    if (!stopped && local)
      lf = [&](uint64_t total, const uint8_t** d, uint64_t* avail) -> int {
        const uint64_t have = local_len > base ? std::min(total, local_len - base) : 0;
        HBX_TRY(c, c->d_rimg.ensure(have + 256));
        if (have) HBX_TRY(c, hipMemcpyAsync(c->d_rimg.p, local + base, have, hipMemcpyHostToDevice, c->rstream));
        *d = c->d_rimg.as<uint8_t>();
        *avail = have;
        return HBX_OK;
      };
    if (int rc = restore_window(c, w, image, cap, false, &lf)) return rc;
    if (stopped) continue;
    for (uint64_t i = 0; i < w.n_good; i++) offs[a + i + 1] = base + woffs[i + 1];
    *n_good = a + w.n_good;
    const uint64_t good = woffs[w.n_good];
    if (out && good) {
      if (base + good > out_cap) return c->fail(HBX_ERR_ARG, "out_cap is smaller than the restored prefix");
      const auto t_out = std::chrono::steady_clock::now();
      HBX_TRY(c, hipMemcpy(out + base, image, good, hipMemcpyDeviceToHost));
      c->restore_ms[3] += ms_since(t_out);
    }
    if (w.first_diff != hbxr::kNoDiff && found == hbxr::kNoDiff) found = base + w.first_diff;
    if (w.n_good < wn) stopped = true;
  }
  if (local) {
    const uint64_t total = offs[*n_good];
    *first_diff = found != hbxr::kNoDiff ? found : local_len != total ? std::min(local_len, total) : hbxr::kNoDiff;
  }
  return HBX_OK;
}

int hbx_restore_file_stream(hbx_ctx* c, uint64_t n_blocks, const uint8_t* ids, hbx_block_source_fn source,
                            void* user, uint64_t window_bytes, const char* out_path, hbx_restore_sink_fn sink,
                            const char* local_path, uint64_t max_block, uint64_t* bytes, uint64_t* bad_index,
                            uint32_t* bad_status, uint64_t* first_diff) {
  if (!c || (n_blocks && (!ids || !source))) return HBX_ERR_ARG;
  if ((out_path ? 1 : 0) + (sink ? 1 : 0) + (local_path ? 1 : 0) != 1) return HBX_ERR_ARG;  // exactly one target
  if (local_path && !first_diff) return HBX_ERR_ARG;
  const uint64_t mb = restore_mb(max_block);
  if (mb > kRestoreMaxBlock) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  for (double& t : c->restore_ms) t = 0.0;
  if (bytes) *bytes = 0;
  if (bad_index) *bad_index = ~0ull;
  if (bad_status) *bad_status = 0;
  if (first_diff) *first_diff = hbxr::kNoDiff;
  const uint64_t bound = hbx_restore_in_bound(mb), stride = restore_stride(mb);
  if (window_bytes == 0) window_bytes = 1ull << 30;
  const uint64_t per = std::min<uint64_t>(std::max<uint64_t>(1, window_bytes / stride), std::max<uint64_t>(n_blocks, 1));
  const uint64_t in_slot = ((bound + 15) & ~15ull);
  // every buffer is sized by the window, never by the chain
  for (int k = 0; k < 2; k++) {
    HBX_TRY(c, c->h_rin[k].ensure(per * in_slot + 64));
    HBX_TRY(c, c->d_rin[k].ensure(per * in_slot + 65536));
    HBX_TRY(c, c->h_rout[k].ensure(kImageLead + per * mb + kImageGuard));
  }
  HBX_TRY(c, c->d_rslots.ensure(per * stride + 65536));
  if (local_path) HBX_TRY(c, c->d_rimg.ensure(per * mb + 256));
  if (!c->fstream) HBX_TRY(c, hipStreamCreateWithFlags(&c->fstream, hipStreamNonBlocking));
  int fd = -1;
  uint64_t local_len = 0;
  if (out_path) {
    fd = ::open(out_path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
    if (fd < 0) return c->fail(HBX_ERR_IO, std::string("cannot create ") + out_path + ": " + std::strerror(errno));
  } else if (local_path) {
    fd = ::open(local_path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) return c->fail(HBX_ERR_IO, std::string("cannot open ") + local_path + ": " + std::strerror(errno));
    const off_t end = ::lseek(fd, 0, SEEK_END);
    if (end < 0) {
      ::close(fd);
      return c->fail(HBX_ERR_IO, std::string("cannot size ") + local_path);
    }
    local_len = (uint64_t)end;
  }
  struct Filled {  // one window's staged input
    uint64_t first = 0, n = 0;
    std::vector<uint64_t> src, lens;
    std::vector<uint8_t> types;
    std::vector<uint32_t> status;
    std::string err;
  };
  Filled fill[2];
  const uint64_t nwin = (n_blocks + per - 1) / per;
  // the source fills window k's pinned staging and the copy to the device runs
  // on a stream of its own, while the previous window inflates
  auto do_fill = [&](uint64_t k) -> int {
    Filled& f = fill[k & 1];
    f.first = k * per;
    f.n = std::min(per, n_blocks - f.first);
    f.src.assign(f.n, 0);
    f.lens.assign(f.n, 0);
    f.types.assign(f.n, 0);
    f.status.assign(f.n, 0);
    f.err.clear();
    if (hipSetDevice(c->device) != hipSuccess) {
      f.err = "hipSetDevice failed on the fill thread";
      return HBX_ERR_HIP;
    }
    uint8_t* h = c->h_rin[k & 1].as<uint8_t>();
    uint8_t* d = c->d_rin[k & 1].as<uint8_t>();
    uint64_t pos = 0;
    for (uint64_t i = 0; i < f.n; i++) {
      pos = (pos + 15) & ~15ull;
      uint64_t len = 0;
      uint8_t type = 0;
      if (source(user, f.first + i, h + pos, bound, &len, &type) != 0) {
        f.err = "the block source failed at block " + std::to_string(f.first + i);
        return HBX_ERR_IO;
      }
      f.types[i] = type;
      f.src[i] = reinterpret_cast<uint64_t>(d) + pos;
      if (len > bound || (type != HBX_BLOCK_RAW && type != HBX_BLOCK_ZLIB)) {
        f.status[i] = 8;
        continue;
      }
      f.lens[i] = len;
      pos += len;
    }
    hipError_t e = pos ? hipMemcpyAsync(d, h, pos, hipMemcpyHostToDevice, c->fstream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(c->fstream);
    if (e != hipSuccess) {
      f.err = std::string("restore input copy: ") + hipGetErrorString(e);
      return HBX_ERR_HIP;
    }
    return HBX_OK;
  };
  // window k's good prefix, gathered into pinned memory, to the file or the sink
  std::string out_err;
  auto do_out = [&](int slot, uint64_t file_off, uint64_t len) -> int {
    const uint8_t* p = c->h_rout[slot].as<uint8_t>() + kImageLead;
    if (sink) {
      if (len && sink(user, file_off, p, len) != 0) {
        out_err = "the restore sink failed at offset " + std::to_string(file_off);
        return HBX_ERR_IO;
      }
      return HBX_OK;
    }
    for (uint64_t done = 0; done < len;) {
      const ssize_t r = ::pwrite(fd, p + done, len - done, (off_t)(file_off + done));
      if (r < 0 && errno == EINTR) continue;
      if (r <= 0) {
        out_err = std::string("cannot write ") + out_path + ": " + std::strerror(errno);
        return HBX_ERR_IO;
      }
      done += (uint64_t)r;
    }
    return HBX_OK;
  };
  int rc = HBX_OK;
  uint64_t file_off = 0;
  std::future<int> filling, writing;
  std::vector<uint64_t> woffs;
  if (nwin) filling = std::async(std::launch::async, do_fill, (uint64_t)0);
  for (uint64_t k = 0; k < nwin && rc == HBX_OK; k++) {
    rc = filling.get();
    Filled& f = fill[k & 1];
    if (rc) {
      c->err = f.err;
      break;
    }
    if (k + 1 < nwin) filling = std::async(std::launch::async, do_fill, k + 1);
    RestoreWin w;
    w.n = f.n;
    w.src = f.src.data();
    w.lens = f.lens.data();
    w.types = f.types.data();
    w.expect = ids + 16 * f.first;
    w.max_block = mb;
    woffs.assign(f.n + 1, 0);
    w.offs = woffs.data();
    w.status = f.status.data();
    RestoreLocalFn lf;
    if (local_path)
      lf = [&](uint64_t total, const uint8_t** d, uint64_t* avail) -> int {
        const uint64_t have = local_len > file_off ? std::min(total, local_len - file_off) : 0;
        uint8_t* h = c->h_rout[k & 1].as<uint8_t>();
        for (uint64_t done = 0; done < have;) {
          const ssize_t r = ::pread(fd, h + done, have - done, (off_t)(file_off + done));
          if (r < 0 && errno == EINTR) continue;
          if (r <= 0) return c->fail(HBX_ERR_IO, std::string("short read of ") + local_path);
          done += (uint64_t)r;
        }
        if (have) HBX_TRY(c, hipMemcpyAsync(c->d_rimg.p, h, have, hipMemcpyHostToDevice, c->rstream));
        *d = c->d_rimg.as<uint8_t>();
        *avail = have;
        return HBX_OK;
      };
    // (the pinned output slot k & 1 is free: window k - 2's write was joined
    // before window k - 1's began)
    rc = restore_window(c, w, local_path ? nullptr : c->h_rout[k & 1].as<uint8_t>() + kImageLead, f.n * mb, true,
                        &lf);
    if (rc) break;
    const uint64_t good = woffs[w.n_good];
    if (writing.valid()) {
      rc = writing.get();
      if (rc) {
        c->err = out_err;
        break;
      }
    }
    if (!local_path) writing = std::async(std::launch::async, do_out, (int)(k & 1), file_off, good);
    if (local_path && w.first_diff != hbxr::kNoDiff) {  // the first event in chain order is a difference
      *first_diff = file_off + w.first_diff;
      file_off += good;
      break;
    }
    file_off += good;
    if (w.n_good < f.n) {
      if (bad_index) *bad_index = f.first + w.n_good;
      if (bad_status) *bad_status = f.status[w.n_good];
      rc = c->fail(HBX_ERR_VERIFY, "block " + std::to_string(f.first + w.n_good) + " failed with status " +
                                       std::to_string(f.status[w.n_good]));
      break;
    }
    if (local_path && file_off > local_len) {  // the local copy ended inside this window
      *first_diff = local_len;
      break;
    }
  }
  // drain: nothing of this call stays in flight, whatever happened
  if (filling.valid()) (void)filling.get();
  if (writing.valid()) {
    const int wrc = writing.get();
    if (wrc && rc == HBX_OK) rc = c->fail(wrc, out_err);
  }
  for (hipStream_t s : {c->stream, c->rstream, c->fstream}) (void)hipStreamSynchronize(s);
  if (fd >= 0 && ::close(fd) != 0 && out_path && rc == HBX_OK)
    rc = c->fail(HBX_ERR_IO, std::string("cannot close ") + out_path);
  if (bytes) *bytes = file_off;
  if (rc == HBX_OK && local_path && *first_diff == hbxr::kNoDiff && local_len != file_off)
    *first_diff = std::min(local_len, file_off);
  return rc;
}

}  // extern "C"

// ---- restore and diff of many files (hbx_restore_many.hip, K11) ---------------
namespace {

constexpr uint64_t kManyWindow = 1ull << 30;  // window_bytes = 0

// One block's share of a window: its capacity, K6's read slack, a multiple of 256.
inline uint64_t many_slot(uint64_t cap) {
  return ((std::min<uint64_t>(cap, 1ull << 62) + 255ull) & ~255ull) + 256ull;
}

// hbx_restore_many_window's rule: the blocks from `start` whose shares fit wb, at least one.
uint64_t many_window_end(uint64_t n, const uint64_t* caps, uint64_t wb, uint64_t start) {
  uint64_t sum = 0, e = start;
  while (e < n) {
    const uint64_t s = many_slot(caps[e]);
    if (e > start && (s > wb || sum > wb - s)) break;
    sum += s;
    e++;
  }
  return e;
}

// The staged input of a window may hold this many bytes: data fields are about
// as long as their capacities (a stored deflate block adds 5 bytes per 32 KiB),
// and one that is not (a tiny size hint in front of a long stream) ends the
// window early instead of growing the buffer.
inline uint64_t many_stage_cap(uint64_t wb, uint64_t in_slot) { return wb + wb / 512 + 2 * in_slot + 4096; }

// One window's blocks, their data fields in device memory.
struct ManyStaged {
  uint64_t first = 0, n = 0;  // global index of block 0; blocks
  bool last = false;          // (stream) nothing follows this window
  std::vector<uint64_t> src, lens, caps;  // device address and length of the data field; capacity (raw: its length)
  std::vector<uint8_t> types, hinted;     // DataType; the capacity comes from a size hint
  std::vector<uint32_t> status, file;     // 0 or 8 from the pre-check, then the block's status; its file
  std::string err;
  void clear(uint64_t at) {
    first = at;
    n = 0;
    last = false;
    for (auto* v : {&src, &lens, &caps}) v->clear();
    types.clear();
    hinted.clear();
    status.clear();
    file.clear();
    err.clear();
  }
  void push(uint64_t s, uint64_t len, uint64_t cap, uint8_t type, bool hint, uint32_t st, uint32_t f) {
    src.push_back(s);
    lens.push_back(len);
    caps.push_back(cap);
    types.push_back(type);
    hinted.push_back(hint ? 1 : 0);
    status.push_back(st);
    file.push_back(f);
    n++;
  }
};

// The blocks [b0, b1) of one file inside one K11 pass.
struct ManySeg {
  uint32_t file = 0;
  uint64_t b0 = 0, b1 = 0;  // in the staged window
  uint64_t img = 0;         // where its bytes start in the pass's packed image
  uint64_t foff0 = 0;       // the file offset they start at (the file's good bytes so far)
  uint64_t bytes = 0;       // what K11 touches: the blocks before the first that failed to inflate
  uint64_t good = 0;        // the bytes of its leading verified blocks
  bool was_bad = false;     // the file had a bad block in an earlier pass
  uint64_t have = 0, loff = 0;  // diff: bytes of the local copy in [foff0, foff0 + bytes), their place in the local image
};

using ManyLocalFn = std::function<int(std::vector<ManySeg>&, const uint8_t**, uint64_t*)>;
using ManyEmitFn = std::function<int(const std::vector<ManySeg>&, const uint8_t*)>;

// What one hbx_restore_files_* call carries from window to window.
struct ManyRun {
  uint64_t mb = HBX_MAX_BLOCK, wb = kManyWindow;
  const uint8_t* expect = nullptr;
  const uint8_t* links = nullptr;
  const uint64_t* link_base = nullptr;
  const uint32_t* n_links = nullptr;
  bool diff = false;
  std::vector<uint64_t> run, ngood, found;  // per file: good bytes and blocks so far, smallest differing offset
  std::vector<uint8_t> bad;                 // per file: a bad block was met
  std::vector<uint32_t> bad_status;
  uint64_t* blk_offs = nullptr;   // per global block (may be NULL)
  uint32_t* status_out = nullptr; // per global block (may be NULL)
  uint64_t pass = 0;
  ManyLocalFn local;  // diff: the local bytes of the pass's segments (have, loff) in pinned memory
  ManyEmitFn emit;    // gather: the pass's packed image (pinned memory), after its checks
  void init(uint64_t n_files) {
    run.assign(n_files, 0);
    ngood.assign(n_files, 0);
    found.assign(n_files, hbxr::kNoDiff);
    bad.assign(n_files, 0);
    bad_status.assign(n_files, 0);
  }
};

// One pass over the blocks [s, e) of a staged window, already inflated (addr,
// dlen, status): K11 (result stream) beside VerifyBlock (K6, scan stream), as
// restore_window does for one chain, with the image in pinned host memory and
// its guard bytes checked.  Every stream is idle on return, also on failure.
int many_pass(hbx_ctx* c, ManyRun& R, ManyStaged& S, uint64_t s, uint64_t e, const std::vector<uint64_t>& addr,
              const std::vector<uint64_t>& dlen) {
  const uint64_t n = e - s;
  if (n == 0) return HBX_OK;
  c->many_passes++;
  const auto t_verify = std::chrono::steady_clock::now();
  // the packed layout before VerifyBlock's answer: per file, the blocks before the first that did not inflate
  std::vector<ManySeg> segs;
  std::vector<uint64_t> bimg(n, 0), bfoff(n, 0);
  std::vector<uint8_t> live(n, 0);
  uint64_t total = 0;
  bool open = false;
  for (uint64_t i = s; i < e; i++) {
    const uint32_t f = S.file[i];
    if (segs.empty() || segs.back().file != f) {
      ManySeg g;
      g.file = f;
      g.b0 = i;
      g.img = total;
      g.foff0 = R.run[f];
      g.was_bad = R.bad[f] != 0;
      segs.push_back(g);
      open = !g.was_bad;
    }
    ManySeg& g = segs.back();
    g.b1 = i + 1;
    if (open && S.status[i] == 0) {
      live[i - s] = 1;
      bimg[i - s] = total;
      bfoff[i - s] = g.foff0 + g.bytes;
      g.bytes += dlen[i];
      total += dlen[i];
    } else {
      open = false;
    }
  }
  if (segs.size() > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "restore: window too large");
  hipStream_t rs = c->rstream;
  const uint8_t* h_local = nullptr;
  uint64_t local_total = 0;
  uint8_t* image = nullptr;
  if (R.diff) {
    if (int rc = R.local(segs, &h_local, &local_total)) return rc;
  } else {
    PinBuf& hb = c->h_rout[R.pass & 1];
    HBX_TRY(c, hb.ensure(kImageLead + total + kImageGuard));
    image = hb.as<uint8_t>() + kImageLead;
  }
  R.pass++;
  std::vector<hbxm::Piece> pieces;
  for (uint64_t k = 0; k < segs.size(); k++) {
    const ManySeg& g = segs[k];
    const uint64_t cover = R.diff ? std::min(g.have, g.bytes) : g.bytes;  // bytes of the segment K11 touches
    for (uint64_t i = g.b0; i < g.b1; i++) {
      if (!live[i - s]) continue;
      const uint64_t at = bfoff[i - s] - g.foff0;  // inside the segment
      if (at >= cover) break;
      const uint64_t len = std::min(dlen[i], cover - at);
      const uint64_t dst = R.diff ? g.loff + at : bimg[i - s];
      for (uint64_t p = 0; p < len; p += hbxm::kPieceMany)
        pieces.push_back(hbxm::Piece{addr[i] + p, dst + p, bfoff[i - s] + p,
                                     (uint32_t)std::min<uint64_t>(hbxm::kPieceMany, len - p), (uint32_t)k});
    }
  }
  if (pieces.size() > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "restore: window too large");
  std::vector<uint64_t> words(R.diff ? segs.size() : 0, hbxr::kNoDiff);
  const bool guarded = !R.diff && !pieces.empty();
  const uint32_t groups = (uint32_t)((pieces.size() + hbxm::kWaves - 1) / hbxm::kWaves);
  int krc = HBX_OK;
  if (!pieces.empty()) {
    krc = [&]() -> int {
      HBX_TRY(c, c->d_rpiece.ensure(pieces.size() * sizeof(hbxm::Piece)));
      HBX_TRY(c, hipMemcpyAsync(c->d_rpiece.p, pieces.data(), pieces.size() * sizeof(hbxm::Piece),
                                hipMemcpyHostToDevice, rs));
      if (R.diff) {
        HBX_TRY(c, c->d_rimg.ensure(local_total + 256));
        HBX_TRY(c, hipMemsetAsync(c->d_rword.p, 0xFF, 8 * segs.size(), rs));
        if (local_total)
          HBX_TRY(c, hipMemcpyAsync(c->d_rimg.p, h_local, local_total, hipMemcpyHostToDevice, rs));
        hipLaunchKernelGGL(hbx_k11_diff, dim3(groups), dim3(hbxm::kThreads), 0, rs, c->d_rpiece.as<hbxm::Piece>(),
                           (uint32_t)pieces.size(), c->d_rimg.as<uint8_t>(), c->d_rword.as<unsigned long long>());
        HBX_TRY(c, hipGetLastError());
        HBX_TRY(c, hipMemcpyAsync(words.data(), c->d_rword.p, 8 * segs.size(), hipMemcpyDeviceToHost, rs));
      } else {
        std::memset(image - kImageGuard, kGuardByte, kImageGuard);
        std::memset(image + total, kGuardByte, kImageGuard);
        hipLaunchKernelGGL(hbx_k11_gather, dim3(groups), dim3(hbxm::kThreads), 0, rs, c->d_rpiece.as<hbxm::Piece>(),
                           (uint32_t)pieces.size(), image);
        HBX_TRY(c, hipGetLastError());
      }
      return HBX_OK;
    }();
  }
  // VerifyBlock of every block that inflated, links passed through
  std::vector<uint32_t> nl(n, 0u);
  if (R.n_links)
    for (uint64_t i = s; i < e; i++)
      if (S.status[i] == 0) nl[i - s] = R.n_links[S.first + i];
  std::vector<uint8_t> ok(n, 0);
  int vrc = krc ? HBX_OK
                : verify_device(c, nullptr, n, addr.data() + s, dlen.data() + s, R.links,
                                R.link_base ? R.link_base + S.first + s : nullptr, nl.data(), nullptr,
                                R.expect + 16 * (S.first + s), ok.data(), nullptr);
  const std::string verr = c->err;
  const int src_ = c->hip(hipStreamSynchronize(rs), "hipStreamSynchronize(result stream)");
  c->restore_ms[2] += ms_since(t_verify);
  if (krc) return krc;
  if (vrc) return c->fail(vrc, verr);
  if (src_) return src_;
  if (guarded)
    for (uint64_t b = 0; b < kImageGuard; b++)
      if ((image - kImageGuard)[b] != kGuardByte || image[total + b] != kGuardByte)
        return c->fail(HBX_ERR_STATE, "restore: K11 wrote outside the image");
  for (uint64_t i = s; i < e; i++)
    if (S.status[i] == 0 && !ok[i - s]) S.status[i] = 7;
  // per file: its leading good blocks of this pass join its prefix
  for (uint64_t k = 0; k < segs.size(); k++) {
    ManySeg& g = segs[k];
    const uint32_t f = g.file;
    uint64_t i = g.b0;
    if (!g.was_bad) {
      while (i < g.b1 && S.status[i] == 0) {
        if (R.blk_offs) R.blk_offs[S.first + i] = g.foff0 + g.good;
        g.good += dlen[i];
        i++;
      }
      R.ngood[f] += i - g.b0;
      R.run[f] += g.good;
      if (i < g.b1) {
        R.bad[f] = 1;
        R.bad_status[f] = S.status[i];
      }
      if (R.diff && words[k] < g.foff0 + g.good) R.found[f] = std::min(R.found[f], words[k]);
    }
    for (; i < g.b1; i++)
      if (R.blk_offs) R.blk_offs[S.first + i] = ~0ull;
  }
  if (R.status_out)
    for (uint64_t i = s; i < e; i++) R.status_out[S.first + i] = S.status[i];
  if (!R.diff && R.emit) {
    const auto t_out = std::chrono::steady_clock::now();
    const int rc = R.emit(segs, image);
    c->restore_ms[3] += ms_since(t_out);
    return rc;
  }
  return HBX_OK;
}

// A staged window: inflate every zlib block into a slot of its (hinted)
// capacity, then K11 passes over it.  A size hint is never trusted: a stream
// that overflows a slot smaller than max_block is inflated again into a
// max_block slot, and the window is then cut into passes by the window rule
// over the corrected capacities, so no pass holds more than the window allows.
int many_process(hbx_ctx* c, ManyRun& R, ManyStaged& S) {
  const uint64_t n = S.n;
  if (n == 0) return HBX_OK;
  c->many_windows++;
  // (the diff words of a pass, one per file in it; also the address of a block that has no data: never
  // reallocated while a pass is under way)
  HBX_TRY(c, c->d_rword.ensure(std::max<uint64_t>(4096, 8 * n)));
  const uint64_t mb = R.mb;
  auto estimate = [&](uint64_t len) { return std::min<uint64_t>(mb, 8 * len + 4096); };  // as restore_window
  std::vector<uint64_t> zi, in_offs, in_lens, out_offs, out_caps, out_hint, out_lens;
  std::vector<uint32_t> zst;
  uint64_t slots = 0;
  for (uint64_t i = 0; i < n; i++)
    if (S.status[i] == 0 && S.types[i] == HBX_BLOCK_ZLIB) {
      zi.push_back(i);
      in_offs.push_back(S.src[i]);
      in_lens.push_back(S.lens[i]);
      out_offs.push_back(slots);
      out_caps.push_back(S.caps[i]);
      out_hint.push_back(S.hinted[i] ? S.caps[i] : estimate(S.lens[i]));
      slots += many_slot(S.caps[i]);
    }
  const uint64_t nz = zi.size();
  const auto t_inflate = std::chrono::steady_clock::now();
  out_lens.assign(nz, 0);
  zst.assign(nz, 0);
  if (nz) {
    HBX_TRY(c, c->d_rslots.ensure(slots + 65536));
    if (int rc = inflate_device(c, nullptr, nz, in_offs.data(), in_lens.data(), c->d_rslots.p, out_offs.data(),
                                out_caps.data(), out_lens.data(), zst.data(), out_hint.data()))
      return rc;
  }
  c->restore_ms[1] += ms_since(t_inflate);
  std::vector<uint64_t> addr(n), dlen(n, 0), newcaps(S.caps);
  std::vector<uint8_t> over(n, 0);
  const uint64_t nowhere = reinterpret_cast<uint64_t>(c->d_rword.p);
  for (uint64_t i = 0; i < n; i++) {
    addr[i] = nowhere;
    if (S.status[i] == 0 && S.types[i] == HBX_BLOCK_RAW) {
      if (S.lens[i] > mb) {
        S.status[i] = hbxi::kErrOutput;
      } else {
        addr[i] = S.src[i];
        dlen[i] = S.lens[i];
      }
    }
  }
  for (uint64_t k = 0; k < nz; k++) {
    const uint64_t i = zi[k];
    S.status[i] = zst[k];
    if (zst[k] == 0) {
      addr[i] = reinterpret_cast<uint64_t>(c->d_rslots.p) + out_offs[k];
      dlen[i] = out_lens[k];
    } else if (zst[k] == hbxi::kErrOutput && S.caps[i] < mb) {
      over[i] = 1;
      newcaps[i] = mb;
    }
  }
  const uint64_t stride = restore_stride(mb);
  for (uint64_t s = 0; s < n;) {
    const uint64_t e = many_window_end(n, newcaps.data(), R.wb, s);
    std::vector<uint64_t> ri, r_in, r_len, r_out, r_cap, r_hint, r_olen;
    for (uint64_t i = s; i < e; i++)
      if (over[i]) {
        r_out.push_back(ri.size() * stride);
        ri.push_back(i);
        r_in.push_back(S.src[i]);
        r_len.push_back(S.lens[i]);
        r_cap.push_back(mb);
        r_hint.push_back(estimate(S.lens[i]));
      }
    if (!ri.empty()) {
      const auto t_again = std::chrono::steady_clock::now();
      c->many_retries += ri.size();
      std::vector<uint32_t> rst(ri.size(), 0);
      r_olen.assign(ri.size(), 0);
      HBX_TRY(c, c->d_rretry.ensure(ri.size() * stride + 65536));
      if (int rc = inflate_device(c, nullptr, ri.size(), r_in.data(), r_len.data(), c->d_rretry.p, r_out.data(),
                                  r_cap.data(), r_olen.data(), rst.data(), r_hint.data()))
        return rc;
      for (uint64_t k = 0; k < ri.size(); k++) {
        const uint64_t i = ri[k];
        S.status[i] = rst[k];
        if (rst[k] == 0) {
          addr[i] = reinterpret_cast<uint64_t>(c->d_rretry.p) + r_out[k];
          dlen[i] = r_olen[k];
        }
      }
      c->restore_ms[1] += ms_since(t_again);
    }
    if (int rc = many_pass(c, R, S, s, e, addr, dlen)) return rc;
    s = e;
  }
  return HBX_OK;
}

// Up to `threads` threads over the jobs [0, n); the caller's thread is one of them.
template <class F>
void many_pool(uint32_t threads, uint64_t n, F&& job) {
  if (n == 0) return;
  std::atomic<uint64_t> next{0};
  auto work = [&] {
    for (uint64_t j = next.fetch_add(1); j < n; j = next.fetch_add(1)) job(j);
  };
  const uint64_t nt = std::min<uint64_t>(std::max<uint32_t>(threads, 1u), n);
  std::vector<std::thread> th;
  for (uint64_t t = 1; t < nt; t++) th.emplace_back(work);
  work();
  for (auto& t : th) t.join();
}

// The capacity of a block of file f: a zlib block's is min(max_block, hint), a raw block's its length.
inline uint64_t many_cap(uint64_t mb, const uint64_t* hint, uint64_t f, uint8_t type, uint64_t len, bool* hinted) {
  *hinted = false;
  if (type == HBX_BLOCK_RAW) return len;
  if (hint && hint[f]) {
    *hinted = true;
    return std::min(mb, hint[f]);
  }
  return mb;
}

bool many_first_ok(uint64_t n_files, const uint64_t* first) {
  if (n_files == 0) return true;
  if (!first || first[0] != 0) return false;
  for (uint64_t f = 0; f < n_files; f++)
    if (first[f + 1] < first[f]) return false;
  return true;
}

}  // namespace

extern "C" {

int hbx_restore_many_window(uint64_t n, const uint64_t* caps, uint64_t window_bytes, uint64_t start, uint64_t* end) {
  if (!end || start > n || (n && !caps)) return HBX_ERR_ARG;
  *end = many_window_end(n, caps, window_bytes ? window_bytes : kManyWindow, start);
  return HBX_OK;
}

int hbx_restore_files_blocks(hbx_ctx* c, uint64_t n_files, const uint64_t* first, const uint8_t* const* datas,
                             const uint64_t* lens, const uint8_t* types, const uint8_t* expect, const uint8_t* links,
                             const uint64_t* link_base, const uint32_t* n_links, const uint64_t* size_hint,
                             uint64_t max_block, uint8_t* out, uint64_t out_cap, uint64_t* out_offs,
                             const uint8_t* local, const uint64_t* local_offs, uint64_t* blk_offs, uint32_t* status,
                             uint64_t* n_good, uint64_t* first_diff) {
  if (!c || (n_files && (!first || !n_good))) return HBX_ERR_ARG;
  if ((out != nullptr) == (local != nullptr)) return HBX_ERR_ARG;  // exactly one target
  if (out && !out_offs) return HBX_ERR_ARG;
  if (local && (!local_offs || !first_diff)) return HBX_ERR_ARG;
  if (!many_first_ok(n_files, first)) return HBX_ERR_ARG;
  const uint64_t n = n_files ? first[n_files] : 0;
  if (n && (!datas || !lens || !types || !expect || !status)) return HBX_ERR_ARG;
  const uint64_t mb = restore_mb(max_block);
  if (mb > kRestoreMaxBlock || n > 0x7FFFFFFFull || n_files > 0x7FFFFFFFull) return HBX_ERR_ARG;
  if (local)
    for (uint64_t f = 0; f < n_files; f++)
      if (local_offs[f + 1] < local_offs[f]) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  for (double& t : c->restore_ms) t = 0.0;
  c->many_windows = c->many_passes = c->many_retries = 0;
  const uint64_t bound = hbx_restore_in_bound(mb), in_slot = (bound + 15) & ~15ull;
  ManyRun R;
  R.mb = mb;
  R.wb = kManyWindow;
  R.expect = expect;
  R.links = links;
  R.link_base = link_base;
  R.n_links = n_links;
  R.diff = local != nullptr;
  R.blk_offs = blk_offs;
  R.status_out = status;
  R.init(n_files);
  if (out_offs) out_offs[0] = 0;
  // per block: file, pre-check, capacity
  std::vector<uint32_t> file(n), pre(n);
  std::vector<uint64_t> caps(n);
  std::vector<uint8_t> hinted(n);
  for (uint64_t f = 0; f < n_files; f++)
    for (uint64_t i = first[f]; i < first[f + 1]; i++) {
      const bool known = types[i] == HBX_BLOCK_RAW || types[i] == HBX_BLOCK_ZLIB;
      pre[i] = (!known || lens[i] > bound) ? 8u : 0u;
      if (pre[i] == 0 && lens[i] && !datas[i]) return c->fail(HBX_ERR_ARG, "null block data");
      file[i] = (uint32_t)f;
      bool h = false;
      caps[i] = pre[i] ? 0 : many_cap(mb, size_hint, f, types[i], lens[i], &h);
      hinted[i] = h ? 1 : 0;
    }
  // gather: a file's bytes go to out + (the good bytes of the files before it) + its own offset
  std::vector<uint64_t> fbase(n_files + 1, 0);
  uint64_t done_files = 0;  // fbase[0 .. done_files] is final
  auto settle = [&](uint64_t upto) {  // every file before `upto` has all its blocks behind it
    for (; done_files < upto; done_files++) fbase[done_files + 1] = fbase[done_files] + R.run[done_files];
  };
  R.emit = [&](const std::vector<ManySeg>& segs, const uint8_t* image) -> int {
    for (const ManySeg& sg : segs) {
      if (sg.was_bad || sg.good == 0) continue;
      settle(sg.file);
      if (fbase[sg.file] + sg.foff0 + sg.good > out_cap)
        return c->fail(HBX_ERR_CAPACITY, "out_cap is smaller than the restored prefixes");
      std::memcpy(out + fbase[sg.file] + sg.foff0, image + sg.img, sg.good);
    }
    return HBX_OK;
  };
  R.local = [&](std::vector<ManySeg>& segs, const uint8_t** host, uint64_t* total) -> int {
    uint64_t pos = 0;
    for (ManySeg& sg : segs) {
      const uint64_t llen = local_offs[sg.file + 1] - local_offs[sg.file];
      sg.have = (sg.was_bad || llen <= sg.foff0) ? 0 : std::min(sg.bytes, llen - sg.foff0);
      sg.loff = pos;
      pos += sg.have;
    }
    HBX_TRY(c, c->h_rout[0].ensure(pos + 64));
    uint8_t* h = c->h_rout[0].as<uint8_t>();
    for (const ManySeg& sg : segs)
      if (sg.have) std::memcpy(h + sg.loff, local + local_offs[sg.file] + sg.foff0, sg.have);
    *host = h;
    *total = pos;
    return HBX_OK;
  };
  ManyStaged S;
  for (uint64_t a = 0; a < n;) {
    uint64_t b = many_window_end(n, caps.data(), R.wb, a);
    // stage the data fields through pinned memory, one copy per window: zlib streams at 16-byte
    // boundaries (K8's vector loads), raw blocks packed byte by byte behind whatever precedes them
    const auto t_stage = std::chrono::steady_clock::now();
    const uint64_t room = many_stage_cap(R.wb, in_slot);
    S.clear(a);
    uint64_t pos = 0;
    std::vector<uint64_t> at;
    for (uint64_t i = a; i < b; i++) {
      if (pre[i] == 0 && types[i] == HBX_BLOCK_ZLIB) pos = (pos + 15) & ~15ull;
      at.push_back(pos);
      if (pre[i] == 0) pos += lens[i];
      if (pos + 16 + bound > room) b = i + 1;  // the staging is full: the window ends here
    }
    HBX_TRY(c, c->h_rin[0].ensure(pos + 64));
    HBX_TRY(c, c->d_rin[0].ensure(pos + 65536));
    uint8_t* hin = c->h_rin[0].as<uint8_t>();
    const uint64_t din = reinterpret_cast<uint64_t>(c->d_rin[0].p);
    for (uint64_t i = a; i < b; i++) {
      if (pre[i] == 0 && lens[i]) std::memcpy(hin + at[i - a], datas[i], lens[i]);
      S.push(din + at[i - a], pre[i] ? 0 : lens[i], caps[i], types[i], hinted[i] != 0, pre[i], file[i]);
    }
    if (pos) HBX_TRY(c, hipMemcpyAsync(c->d_rin[0].p, hin, pos, hipMemcpyHostToDevice, c->stream));
    HBX_TRY(c, hipStreamSynchronize(c->stream));
    c->restore_ms[0] += ms_since(t_stage);
    if (int rc = many_process(c, R, S)) return rc;
    a = b;
  }
  settle(n_files);
  for (uint64_t f = 0; f < n_files; f++) {
    n_good[f] = R.ngood[f];
    if (out_offs) out_offs[f + 1] = fbase[f + 1];
    if (local) {
      const uint64_t llen = local_offs[f + 1] - local_offs[f];
      first_diff[f] = R.found[f] != hbxr::kNoDiff ? R.found[f]
                      : llen != R.run[f]          ? std::min(llen, R.run[f])
                                                  : hbxr::kNoDiff;
    }
  }
  return HBX_OK;
}

int hbx_restore_files_stream(hbx_ctx* c, uint64_t n_files, const uint64_t* first, const uint8_t* ids,
                             hbx_file_block_source_fn source, void* user, const uint64_t* size_hint,
                             uint64_t window_bytes, const char* const* out_paths, const char* const* local_paths,
                             uint32_t io_threads, uint64_t max_block, hbx_restored_file* results) {
  if (!c || (n_files && (!first || !results))) return HBX_ERR_ARG;
  if (n_files && (out_paths != nullptr) == (local_paths != nullptr)) return HBX_ERR_ARG;  // exactly one target
  if (!many_first_ok(n_files, first)) return HBX_ERR_ARG;
  const uint64_t n = n_files ? first[n_files] : 0;
  if (n && (!ids || !source)) return HBX_ERR_ARG;
  const uint64_t mb = restore_mb(max_block);
  if (mb > kRestoreMaxBlock || n_files > 0x7FFFFFFFull || io_threads > 16) return HBX_ERR_ARG;
  const char* const* paths = out_paths ? out_paths : local_paths;
  for (uint64_t f = 0; f < n_files; f++)
    if (!paths[f]) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  for (double& t : c->restore_ms) t = 0.0;
  c->many_windows = c->many_passes = c->many_retries = 0;
  const uint32_t threads = io_threads ? io_threads : 16u;
  const bool diff = local_paths != nullptr;
  for (uint64_t f = 0; f < n_files; f++) {
    hbx_restored_file& r = results[f];
    r.bytes = r.n_good = 0;
    r.bad_index = r.first_diff = ~0ull;
    r.bad_status = 0;
    r.err = 0;
  }
  const uint64_t bound = hbx_restore_in_bound(mb), in_slot = (bound + 15) & ~15ull;
  const uint64_t wb = window_bytes ? window_bytes : kManyWindow;
  const uint64_t room = many_stage_cap(wb, in_slot);
  // every buffer is sized by the window and max_block, never by the set of files
  for (int k = 0; k < 2; k++) {
    HBX_TRY(c, c->h_rin[k].ensure(room + 64));
    HBX_TRY(c, c->d_rin[k].ensure(room + 65536));
    HBX_TRY(c, c->h_rout[k].ensure(kImageLead + wb + mb + kImageGuard));
  }
  if (!c->fstream) HBX_TRY(c, hipStreamCreateWithFlags(&c->fstream, hipStreamNonBlocking));
  ManyRun R;
  R.mb = mb;
  R.wb = wb;
  R.expect = ids;
  R.diff = diff;
  R.init(n_files);
  std::vector<uint64_t> local_len(diff ? n_files : 0, 0);
  std::vector<uint8_t> sized(diff ? n_files : 0, 0);
  auto note = [&](uint64_t f, int e) {  // the first error of a file stays
    if (results[f].err == 0) results[f].err = e ? e : EIO;
  };
  auto size_local = [&](uint64_t f) {
    int fd = ::open(local_paths[f], O_RDONLY | O_CLOEXEC);
    if (fd < 0) return note(f, errno);
    const off_t end = ::lseek(fd, 0, SEEK_END);
    if (end < 0) note(f, errno);
    else local_len[f] = (uint64_t)end;
    ::close(fd);
  };
  // files without blocks: created empty, or sized for the diff's length rule
  {
    std::vector<uint64_t> empty;
    for (uint64_t f = 0; f < n_files; f++)
      if (first[f] == first[f + 1]) empty.push_back(f);
    many_pool(threads, empty.size(), [&](uint64_t j) {
      const uint64_t f = empty[j];
      if (diff) {
        sized[f] = 1;
        return size_local(f);
      }
      const int fd = ::open(out_paths[f], O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0666);
      if (fd < 0 || ::close(fd) != 0) note(f, errno);
    });
  }
  // diff: size the local copies met for the first time, then read the compared ranges into pinned memory
  R.local = [&](std::vector<ManySeg>& segs, const uint8_t** host, uint64_t* total) -> int {
    std::vector<uint64_t> fresh;
    for (uint64_t k = 0; k < segs.size(); k++)
      if (!sized[segs[k].file]) {
        sized[segs[k].file] = 1;
        fresh.push_back(segs[k].file);
      }
    many_pool(threads, fresh.size(), [&](uint64_t j) { size_local(fresh[j]); });
    uint64_t pos = 0;
    for (ManySeg& sg : segs) {
      const uint64_t llen = local_len[sg.file];
      sg.have = (sg.was_bad || results[sg.file].err || llen <= sg.foff0) ? 0 : std::min(sg.bytes, llen - sg.foff0);
      sg.loff = pos;
      pos += sg.have;
    }
    HBX_TRY(c, c->h_rout[0].ensure(pos + 64));
    uint8_t* h = c->h_rout[0].as<uint8_t>();
    many_pool(threads, segs.size(), [&](uint64_t k) {
      const ManySeg& sg = segs[k];
      if (!sg.have) return;
      const int fd = ::open(local_paths[sg.file], O_RDONLY | O_CLOEXEC);
      if (fd < 0) {
        std::memset(h + sg.loff, 0, sg.have);
        return note(sg.file, errno);
      }
      for (uint64_t done = 0; done < sg.have;) {
        const ssize_t r = ::pread(fd, h + sg.loff + done, sg.have - done, (off_t)(sg.foff0 + done));
        if (r < 0 && errno == EINTR) continue;
        if (r <= 0) {  // the file shrank under the call
          std::memset(h + sg.loff + done, 0, sg.have - done);
          note(sg.file, r < 0 ? errno : EIO);
          break;
        }
        done += (uint64_t)r;
      }
      ::close(fd);
    });
    *host = h;
    *total = pos;
    return HBX_OK;
  };
  // gather: the pool writes pass p's good prefixes from its pinned image while pass p + 1 runs
  std::future<void> writing;
  R.emit = [&](const std::vector<ManySeg>& segs, const uint8_t* image) -> int {
    if (writing.valid()) writing.get();
    writing = std::async(std::launch::async, [&, segs, image] {
      many_pool(threads, segs.size(), [&](uint64_t k) {
        const ManySeg& sg = segs[k];
        if (sg.was_bad || results[sg.file].err) return;
        const int fd = ::open(out_paths[sg.file], O_WRONLY | O_CLOEXEC | (sg.foff0 == 0 ? O_CREAT | O_TRUNC : 0), 0666);
        if (fd < 0) return note(sg.file, errno);
        for (uint64_t done = 0; done < sg.good;) {
          const ssize_t r = ::pwrite(fd, image + sg.img + done, sg.good - done, (off_t)(sg.foff0 + done));
          if (r < 0 && errno == EINTR) continue;
          if (r <= 0) {
            note(sg.file, r < 0 ? errno : EIO);
            break;
          }
          done += (uint64_t)r;
        }
        if (::close(fd) != 0) note(sg.file, errno);
      });
    });
    return HBX_OK;
  };
  // the fill thread: one source call at a time in (file, index) order into window k's pinned staging;
  // a block that no longer fits the window waits in `carry` for the next one
  ManyStaged fill[2];
  struct Carry {
    bool valid = false;
    uint64_t len = 0;
    uint8_t type = 0;
    std::vector<uint8_t> data;
  } carry;
  uint64_t next_blk = 0, next_file = 0;
  auto do_fill = [&](uint64_t k) -> int {
    ManyStaged& F = fill[k & 1];
    F.clear(next_blk);
    if (hipSetDevice(c->device) != hipSuccess) {
      F.err = "hipSetDevice failed on the fill thread";
      return HBX_ERR_HIP;
    }
    uint8_t* h = c->h_rin[k & 1].as<uint8_t>();
    const uint64_t d = reinterpret_cast<uint64_t>(c->d_rin[k & 1].p);
    uint64_t pos = 0, sum = 0;
    while (next_blk < n) {
      while (first[next_file + 1] <= next_blk) next_file++;
      pos = (pos + 15) & ~15ull;
      uint64_t len = 0;
      uint8_t type = 0;
      if (carry.valid) {
        len = carry.len;
        type = carry.type;
        if (len <= bound && len) std::memcpy(h + pos, carry.data.data(), len);
        carry.valid = false;
      } else if (source(user, next_file, next_blk - first[next_file], h + pos, bound, &len, &type) != 0) {
        F.err = "the block source failed at block " + std::to_string(next_blk - first[next_file]) + " of file " +
                std::to_string(next_file);
        return HBX_ERR_IO;
      }
      const bool bad = len > bound || (type != HBX_BLOCK_RAW && type != HBX_BLOCK_ZLIB);
      bool hinted = false;
      const uint64_t cap = bad ? 0 : many_cap(mb, size_hint, next_file, type, len, &hinted);
      const uint64_t share = many_slot(cap);
      if (F.n && (share > wb || sum > wb - share)) {  // hbx_restore_many_window's rule: the next window's first block
        carry.valid = true;
        carry.len = len;
        carry.type = type;
        if (!bad) carry.data.assign(h + pos, h + pos + len);
        break;
      }
      sum += share;
      F.push(d + pos, bad ? 0 : len, cap, type, hinted, bad ? 8u : 0u, (uint32_t)next_file);
      if (!bad) pos += len;
      next_blk++;
      if (pos + 16 + bound > room) break;  // the staging is full
    }
    F.last = next_blk >= n && !carry.valid;
    hipError_t e = pos ? hipMemcpyAsync(c->d_rin[k & 1].p, h, pos, hipMemcpyHostToDevice, c->fstream) : hipSuccess;
    if (e == hipSuccess) e = hipStreamSynchronize(c->fstream);
    if (e != hipSuccess) {
      F.err = std::string("restore input copy: ") + hipGetErrorString(e);
      return HBX_ERR_HIP;
    }
    return HBX_OK;
  };
  int rc = HBX_OK;
  std::future<int> filling;
  if (n) filling = std::async(std::launch::async, do_fill, (uint64_t)0);
  for (uint64_t k = 0; n && rc == HBX_OK; k++) {
    rc = filling.get();
    ManyStaged& F = fill[k & 1];
    if (rc) {
      c->err = F.err;
      break;
    }
    const bool last = F.last;
    if (!last) filling = std::async(std::launch::async, do_fill, k + 1);
    rc = many_process(c, R, F);
    if (last) break;
  }
  // drain: nothing of this call stays in flight, whatever happened
  if (filling.valid()) (void)filling.get();
  if (writing.valid()) writing.get();
  for (hipStream_t s : {c->stream, c->rstream, c->fstream}) (void)hipStreamSynchronize(s);
  for (uint64_t f = 0; f < n_files; f++) {
    hbx_restored_file& r = results[f];
    r.bytes = R.run[f];
    r.n_good = R.ngood[f];
    if (R.bad[f]) {
      r.bad_index = R.ngood[f];
      r.bad_status = R.bad_status[f];
    }
    if (diff && rc == HBX_OK && r.err == 0)
      r.first_diff = R.found[f] != hbxr::kNoDiff ? R.found[f]
                     : local_len[f] != R.run[f]  ? std::min(local_len[f], R.run[f])
                                                 : hbxr::kNoDiff;
  }
  return rc;
}

}  // extern "C"

// ---- storage data files (hbx_datfile.hip, K14; hbx_datfile.h) ----------------------
namespace {

constexpr uint64_t kDatCandidates = 1ull << 20;  // max_candidates = 0
constexpr uint64_t kDatStage = 32ull << 20;      // one pinned staging buffer of the path variants

// The slot a zlib entry gets before its inflated size is known (as restore_window's estimate).
inline uint64_t dat_share(uint64_t mb, uint64_t len) { return std::min<uint64_t>(mb, 8 * len + 4096); }

// K14's parse over n positions (host memory; the first n_entries are entry
// positions, the rest gap markers): the records come back in the same order.
int datfile_frame(hbx_ctx* c, const uint8_t* image, uint64_t size, uint64_t mb, const uint64_t* pos, uint64_t n,
                  uint64_t n_entries, std::vector<hbx_dat_record>& rec) {
  rec.resize(n);
  if (n == 0) return HBX_OK;
  if (n > 0x7FFFFFFFull * hbxf::kThreads) return c->fail(HBX_ERR_ARG, "data file: too many positions");
  hipStream_t s = c->stream;
  HBX_TRY(c, c->d_df[1].ensure(n * 8));
  HBX_TRY(c, c->d_df[2].ensure(n * sizeof(hbx_dat_record)));
  HBX_TRY(c, hipMemcpyAsync(c->d_df[1].p, pos, n * 8, hipMemcpyHostToDevice, s));
  const hbxf::ParseArgs pa{image, size, c->d_df[1].as<uint64_t>(), c->d_df[2].as<uint4>(), n, n_entries,
                           hbx_restore_in_bound(mb)};
  hipLaunchKernelGGL(hbx_k14_parse, dim3((uint32_t)((n + hbxf::kThreads - 1) / hbxf::kThreads)), dim3(hbxf::kThreads),
                     0, s, pa);
  HBX_TRY(c, hipGetLastError());
  HBX_TRY(c, hipMemcpyAsync(rec.data(), c->d_df[2].p, n * sizeof(hbx_dat_record), hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  return HBX_OK;
}

// Inflate (K8 / K8s) and VerifyBlock (K6, links read from the image) every
// record with status 0 that frames an entry, in place, in windows whose slots
// fit wb by hbx_restore_many_window's rule.  A zlib entry's slot is its
// share (dat_share); a stream that outgrows it is inflated again into a
// max_block slot, as hbx_restore_files_* treats a size hint.  rec[i].status
// becomes the entry's status (0..8), plain[i] its inflated length.
int datfile_verify(hbx_ctx* c, const uint8_t* image, uint64_t mb, uint64_t wb, std::vector<hbx_dat_record>& rec,
                   std::vector<uint32_t>& plain) {
  plain.assign(rec.size(), 0u);
  std::vector<uint64_t> v, caps;
  for (uint64_t i = 0; i < rec.size(); i++)
    if (!(rec[i].flags & HBX_DAT_F_GAP) && rec[i].status == 0) {
      // (K6 frames a message in 32 bits: links and data beyond that are not accepted)
      if (16ull * rec[i].n_links + rec[i].data_len + 136ull > 0xFFFFFFFFull) {
        rec[i].status = 8;
        continue;
      }
      v.push_back(i);
      caps.push_back(rec[i].type == HBX_BLOCK_ZLIB ? dat_share(mb, rec[i].data_len) : 0);
    }
  if (v.empty()) return HBX_OK;
  HBX_TRY(c, c->d_rword.ensure(4096));
  const uint64_t base = reinterpret_cast<uint64_t>(image), stride = restore_stride(mb);
  std::vector<uint64_t> addr, dlen, laddr;
  std::vector<uint32_t> st, nl;
  std::vector<uint8_t> expect, ok;
  // VerifyBlock of the window's blocks js (indices into v) at addr / dlen
  auto verify = [&](const std::vector<uint64_t>& js, uint64_t s0) -> int {
    const uint64_t m = js.size();
    if (m == 0) return HBX_OK;
    std::vector<uint64_t> a(m), l(m);
    laddr.resize(m);
    nl.resize(m);
    expect.resize(16 * m);
    ok.assign(m, 0);
    for (uint64_t q = 0; q < m; q++) {
      const hbx_dat_record& r = rec[v[js[q]]];
      a[q] = addr[js[q] - s0];
      l[q] = dlen[js[q] - s0];
      laddr[q] = base + r.links_off;
      nl[q] = r.n_links;
      std::memcpy(&expect[16 * q], r.id, 16);
    }
    if (int rc = verify_device(c, nullptr, m, a.data(), l.data(), nullptr, nullptr, nl.data(), nullptr,
                               expect.data(), ok.data(), nullptr, laddr.data()))
      return rc;
    for (uint64_t q = 0; q < m; q++)
      if (!ok[q]) st[js[q] - s0] = 7;
    return HBX_OK;
  };
  for (uint64_t s = 0; s < v.size();) {
    const uint64_t e = many_window_end(v.size(), caps.data(), wb, s), n = e - s;
    c->dat_windows++;
    std::vector<uint64_t> zi, in_offs, in_lens, out_offs, out_caps, out_lens, again, first;
    std::vector<uint32_t> zst;
    uint64_t slots = 0;
    addr.assign(n, reinterpret_cast<uint64_t>(c->d_rword.p));
    dlen.assign(n, 0);
    st.assign(n, 0u);
    for (uint64_t j = s; j < e; j++) {
      const hbx_dat_record& r = rec[v[j]];
      if (r.type == HBX_BLOCK_ZLIB) {
        zi.push_back(j);
        in_offs.push_back(base + r.data_off);
        in_lens.push_back(r.data_len);
        out_offs.push_back(slots);
        out_caps.push_back(caps[j]);
        slots += many_slot(caps[j]);
      } else if (r.data_len > mb) {
        st[j - s] = hbxi::kErrOutput;
      } else {
        addr[j - s] = base + r.data_off;
        dlen[j - s] = r.data_len;
      }
    }
    const uint64_t nz = zi.size();
    out_lens.assign(nz, 0);
    zst.assign(nz, 0u);
    if (nz) {
      HBX_TRY(c, c->d_rslots.ensure(slots + 65536));
      if (int rc = inflate_device(c, nullptr, nz, in_offs.data(), in_lens.data(), c->d_rslots.p, out_offs.data(),
                                  out_caps.data(), out_lens.data(), zst.data()))
        return rc;
    }
    for (uint64_t k = 0; k < nz; k++) {
      const uint64_t j = zi[k];
      st[j - s] = zst[k];
      if (zst[k] == 0) {
        addr[j - s] = reinterpret_cast<uint64_t>(c->d_rslots.p) + out_offs[k];
        dlen[j - s] = out_lens[k];
      } else if (zst[k] == hbxi::kErrOutput && caps[j] < mb) {
        again.push_back(j);
      }
    }
    for (uint64_t j = s; j < e; j++)
      if (st[j - s] == 0) first.push_back(j);
    if (int rc = verify(first, s)) return rc;
    // the streams that outgrew their share, as many at a time as max_block slots fit the window
    const uint64_t per = std::max<uint64_t>(1, wb / stride);
    for (uint64_t g = 0; g < again.size(); g += per) {
      const uint64_t m = std::min<uint64_t>(per, again.size() - g);
      c->dat_retries += m;
      std::vector<uint64_t> r_in(m), r_len(m), r_out(m), r_cap(m, mb), r_hint(m), r_olen(m, 0), js;
      std::vector<uint32_t> rst(m, 0u);
      for (uint64_t q = 0; q < m; q++) {
        const hbx_dat_record& r = rec[v[again[g + q]]];
        r_in[q] = base + r.data_off;
        r_len[q] = r.data_len;
        r_out[q] = q * stride;
        r_hint[q] = dat_share(mb, r.data_len);
      }
      HBX_TRY(c, c->d_rretry.ensure(m * stride + 65536));
      if (int rc = inflate_device(c, nullptr, m, r_in.data(), r_len.data(), c->d_rretry.p, r_out.data(), r_cap.data(),
                                  r_olen.data(), rst.data(), r_hint.data()))
        return rc;
      for (uint64_t q = 0; q < m; q++) {
        const uint64_t j = again[g + q];
        st[j - s] = rst[q];
        if (rst[q] == 0) {
          addr[j - s] = reinterpret_cast<uint64_t>(c->d_rretry.p) + r_out[q];
          dlen[j - s] = r_olen[q];
          js.push_back(j);
        }
      }
      if (int rc = verify(js, s)) return rc;
    }
    for (uint64_t j = s; j < e; j++) {
      rec[v[j]].status = st[j - s];
      plain[v[j]] = (uint32_t)dlen[j - s];
    }
    s = e;
  }
  return HBX_OK;
}

// The file at `path` into the context's image buffer through the two pinned
// staging buffers: chunk k is read while chunk k - 1 is copied.
int datfile_load(hbx_ctx* c, const char* path, const uint8_t** image, uint64_t* size) {
  const int fd = ::open(path, O_RDONLY | O_CLOEXEC);
  if (fd < 0) return c->fail(HBX_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
  hipEvent_t done[2] = {nullptr, nullptr};
  const int rc = [&]() -> int {
    const off_t end = ::lseek(fd, 0, SEEK_END);
    if (end < 0) return c->fail(HBX_ERR_IO, std::string("cannot size ") + path + ": " + std::strerror(errno));
    const uint64_t n = (uint64_t)end, need = n + 65536;
    if (need > c->d_dfimg.cap) {
      size_t fr = 0, tot = 0;
      HBX_TRY(c, hipMemGetInfo(&fr, &tot));
      if (need > (fr + c->d_dfimg.cap) / 3)
        return c->fail(HBX_ERR_CAPACITY, std::string(path) + " does not fit a third of the free device memory");
    }
    HBX_TRY(c, c->d_dfimg.ensure(need));
    uint8_t* img = c->d_dfimg.as<uint8_t>();
    hipStream_t s = c->stream;
    HBX_TRY(c, hipMemsetAsync(img + n, 0, 4096, s));
    for (int b = 0; b < 2 && (uint64_t)b * kDatStage < n; b++) {
      HBX_TRY(c, c->h_dfstage[b].ensure(std::min(kDatStage, n)));
      HBX_TRY(c, hipEventCreateWithFlags(&done[b], hipEventDisableTiming));
    }
    std::string err;
    for (uint64_t at = 0, k = 0; at < n; at += kDatStage, k++) {
      const uint64_t len = std::min(kDatStage, n - at);
      const int b = (int)(k & 1);
      if (k >= 2) HBX_TRY(c, hipEventSynchronize(done[b]));
      if (read_range(fd, path, at, len, c->h_dfstage[b].as<uint8_t>(), 8, err)) return c->fail(HBX_ERR_IO, err);
      HBX_TRY(c, hipMemcpyAsync(img + at, c->h_dfstage[b].p, len, hipMemcpyHostToDevice, s));
      HBX_TRY(c, hipEventRecord(done[b], s));
    }
    HBX_TRY(c, hipStreamSynchronize(s));
    *image = img;
    *size = n;
    return HBX_OK;
  }();
  if (rc) (void)hipStreamSynchronize(c->stream);  // (a copy may still read a staging buffer)
  for (hipEvent_t e : done)
    if (e) (void)hipEventDestroy(e);
  ::close(fd);
  return rc;
}

int datfile_check(hbx_ctx* c, const uint8_t* image, uint64_t size, uint64_t mb, uint64_t max_candidates, uint64_t wb,
                  hbx_dat_entry* entries, uint64_t entry_cap, hbx_dat_span* spans, uint64_t span_cap, uint8_t* links,
                  uint64_t link_cap, hbx_dat_summary* sum) {
  std::memset(sum, 0, sizeof *sum);
  sum->size = size;
  sum->truncate_at = ~0ull;
  c->dat_windows = c->dat_retries = 0;
  hipStream_t s = c->stream;
  uint8_t hdr[HBX_DAT_HEADER] = {0};
  const uint64_t hn = std::min<uint64_t>(size, HBX_DAT_HEADER);
  if (hn) {
    HBX_TRY(c, hipMemcpyAsync(hdr, image, hn, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
  }
  sum->header_ok = hbxdat::header_parse(hdr, hn, &sum->filetype, &sum->version, &sum->deadspace) == HBX_OK ? 1u : 0u;
  // 1. K14 scan: every "hblk" and "Cgap" at a position in [16, size - 4]
  const uint64_t cap = std::min<uint64_t>(max_candidates ? max_candidates : kDatCandidates, std::max<uint64_t>(size, 1));
  unsigned long long counts[2] = {0, 0};
  std::vector<uint64_t> pos;
  if (size >= HBX_DAT_HEADER + 4) {
    HBX_TRY(c, c->d_df[0].ensure(2 * cap * 8 + 16));
    uint64_t* lists = c->d_df[0].as<uint64_t>();
    unsigned long long* d_counts = reinterpret_cast<unsigned long long*>(lists + 2 * cap);
    HBX_TRY(c, hipMemsetAsync(d_counts, 0, 16, s));
    const hbxf::ScanArgs sa{image, size, lists, lists + cap, d_counts, cap};
    hipLaunchKernelGGL(hbx_k14_scan, dim3(hbxf::scan_grid(size, c->k14_wgs)), dim3(hbxf::kThreads), 0, s, sa);
    HBX_TRY(c, hipGetLastError());
    HBX_TRY(c, hipMemcpyAsync(counts, d_counts, 16, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
    sum->n_candidates = counts[0];
    sum->n_gap_markers = counts[1];
    if (counts[0] > cap || counts[1] > cap)
      return c->fail(HBX_ERR_CAPACITY, "data file: " + std::to_string(counts[0]) + " entry markers and " +
                                           std::to_string(counts[1]) + " gap markers, max_candidates is " +
                                           std::to_string(cap));
    pos.resize(counts[0] + counts[1]);
    if (counts[0]) HBX_TRY(c, hipMemcpyAsync(pos.data(), lists, counts[0] * 8, hipMemcpyDeviceToHost, s));
    if (counts[1])
      HBX_TRY(c, hipMemcpyAsync(pos.data() + counts[0], lists + cap, counts[1] * 8, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
    // the lists come in the order the waves' adds landed: sorted, the result is the same on every run
    std::sort(pos.begin(), pos.begin() + counts[0]);
    std::sort(pos.begin() + counts[0], pos.end());
  }
  // 2. K14 parse: a record per position
  std::vector<hbx_dat_record> rec;
  if (int rc = datfile_frame(c, image, size, mb, pos.data(), pos.size(), counts[0], rec)) return rc;
  std::vector<uint64_t> gap_offs;
  std::vector<int64_t> gap_skips;
  for (uint64_t i = counts[0]; i < rec.size(); i++)
    if (rec[i].status == 0) {
      gap_offs.push_back(rec[i].off);
      gap_skips.push_back((int64_t)rec[i].size);
    }
  rec.resize(counts[0]);
  for (const hbx_dat_record& r : rec) sum->n_valid += r.status == 0 ? 1 : 0;
  // 3. every structurally valid candidate inflated and verified in place
  std::vector<uint32_t> plain;
  if (int rc = datfile_verify(c, image, mb, wb, rec, plain)) return rc;
  // 4. the walk
  int rc = hbxdat::walk(size, rec.size(), rec.data(), plain.data(), gap_offs.size(), gap_offs.data(), gap_skips.data(),
                        entries, entry_cap, spans, span_cap, sum);
  sum->n_gap_markers = counts[1];  // (the walk saw only those with 12 bytes inside the file)
  if (rc) c->fail(rc, "data file: " + std::to_string(sum->n_entries) + " entries and " + std::to_string(sum->n_spans) +
                          " spans do not fit the output capacities");
  // 5. the good entries' links, flat: K11's gather out of the image, one copy back
  if (rc == HBX_OK && links && sum->n_links > link_cap)
    rc = c->fail(HBX_ERR_CAPACITY, "data file: " + std::to_string(sum->n_links) + " links, link_cap is " +
                                       std::to_string(link_cap));
  if (rc == HBX_OK && links && sum->n_links) {
    std::vector<hbxm::Piece> pieces;
    for (uint64_t i = 0; i < sum->n_entries; i++) {
      const hbx_dat_entry& e = entries[i];
      const uint64_t len = 16ull * e.n_links, src = reinterpret_cast<uint64_t>(image) + e.off + 24;
      for (uint64_t p = 0; p < len; p += hbxm::kPieceMany)
        pieces.push_back(hbxm::Piece{src + p, 16 * e.link_base + p, p,
                                     (uint32_t)std::min<uint64_t>(hbxm::kPieceMany, len - p), 0u});
    }
    if (pieces.size() > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "data file: too many links");
    HBX_TRY(c, c->d_rpiece.ensure(pieces.size() * sizeof(hbxm::Piece)));
    HBX_TRY(c, c->d_rimg.ensure(16 * sum->n_links + 256));
    HBX_TRY(c, hipMemcpyAsync(c->d_rpiece.p, pieces.data(), pieces.size() * sizeof(hbxm::Piece), hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(hbx_k11_gather, dim3((uint32_t)((pieces.size() + hbxm::kWaves - 1) / hbxm::kWaves)),
                       dim3(hbxm::kThreads), 0, s, c->d_rpiece.as<hbxm::Piece>(), (uint32_t)pieces.size(),
                       c->d_rimg.as<uint8_t>());
    HBX_TRY(c, hipGetLastError());
    HBX_TRY(c, hipMemcpyAsync(links, c->d_rimg.p, 16 * sum->n_links, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
  }
  return rc;
}

int datfile_verify_at(hbx_ctx* c, const uint8_t* image, uint64_t size, uint64_t n, const uint64_t* offs,
                      const uint8_t* expect_ids, int content, uint64_t mb, uint64_t wb, uint32_t* status) {
  c->dat_windows = c->dat_retries = 0;
  std::vector<hbx_dat_record> rec;
  if (int rc = datfile_frame(c, image, size, mb, offs, n, n, rec)) return rc;
  for (uint64_t i = 0; i < n; i++)
    if (rec[i].status == 0 && std::memcmp(rec[i].id, expect_ids + 16 * i, 16) != 0) rec[i].status = HBX_DAT_ST_WRONG_ID;
  if (content) {
    std::vector<uint32_t> plain;
    if (int rc = datfile_verify(c, image, mb, wb, rec, plain)) return rc;
  }
  for (uint64_t i = 0; i < n; i++) status[i] = rec[i].status;
  return HBX_OK;
}

// window_bytes = 0: an eighth of the free device memory, at least 1 GiB and at most 32 GiB.  Every window
// costs the serial time of its longest stream and its longest block (one wave, one lane), so few large windows
// are faster than many small ones; the retry slots may take as much again and the split scratch a quarter.
inline uint64_t dat_window(uint64_t wb) {
  if (wb) return wb;
  size_t fr = 0, tot = 0;
  uint64_t b = kManyWindow;
  if (hipMemGetInfo(&fr, &tot) == hipSuccess) b = std::max<uint64_t>(b, std::min<uint64_t>(fr / 8, 32ull << 30));
  return b;
}

// Argument checks shared by the three calls (before the context is touched).
inline bool datfile_args_ok(const void* d_image, uint64_t max_block) {
  return (reinterpret_cast<uintptr_t>(d_image) & (HBX_ARENA_ALIGN - 1)) == 0 && restore_mb(max_block) <= kRestoreMaxBlock;
}

// ---- K16: compact a data file (DESIGN.md §5 "K16", hbx_compact.hip, hbx_compact.h) ----
// hbx_ctx::d_cp
enum { kCpEnt, kCpKeep, kCpKlass, kCpMsz, kCpTsz, kCpCnt, kCpMsrc, kCpMstart, kCpTot, kCpMoved, kCpMeta, kCpIx, kCpBufs };
static_assert(kCpBufs == 12, "hbx_ctx::d_cp");

struct CompactOut {
  uint8_t* klass;
  uint64_t *new_off, *meta_off;
  uint8_t* moved;
  uint64_t moved_cap;
  uint8_t* meta;
  uint64_t meta_cap;
  uint8_t* ix;
  uint64_t ix_cap;
};

inline bool compact_out_ok(const CompactOut& o) {
  return !((o.moved_cap && !o.moved) || (o.meta_cap && !o.meta) || (o.ix_cap && !o.ix));
}

// Grow the named buffers of d_cp to need[], after checking the growth against the free device memory.
int compact_fits(hbx_ctx* c, const size_t* need, std::initializer_list<int> which) {
  uint64_t grow = 0;
  for (int b : which)
    if (need[b] > c->d_cp[b].cap) grow += need[b] + 4096 - c->d_cp[b].cap;
  size_t fr = 0, tot = 0;
  HBX_TRY(c, hipMemGetInfo(&fr, &tot));
  if (grow > fr)
    return c->fail(HBX_ERR_CAPACITY, "data file compaction needs " + std::to_string(grow) +
                                         " more bytes of device memory, " + std::to_string(fr) + " are free");
  for (int b : which) HBX_TRY(c, c->d_cp[b].ensure(need[b]));
  return HBX_OK;
}

// The arguments are checked (hbxcmp::args_ok gave entry_bytes), n > 0, the context is locked and idle.
int compact_run(hbx_ctx* c, const uint8_t* image, uint64_t size, uint64_t n, const hbx_dat_entry* ent,
                const uint8_t* keep, const hbx_dat_compact_args* a, uint64_t entry_bytes, const CompactOut& o,
                hbx_dat_compact_summary* sum) {
  hipStream_t s = c->rstream;
  // (targets of asynchronous copies: they outlive the body below, and a failure synchronises before they go)
  unsigned long long tot[hbxk::kTotWords] = {};
  uint8_t guard[4 * kImageGuard];
  std::memset(guard, kGuardByte, sizeof guard);
  const int rc = [&]() -> int {
  const uint64_t chunks = (n + hbxg::kScanChunk - 1) / hbxg::kScanChunk;
  size_t need[kCpBufs] = {};
  need[kCpEnt] = n * sizeof(hbx_dat_entry);
  need[kCpKeep] = need[kCpKlass] = n;
  need[kCpMsz] = need[kCpTsz] = need[kCpCnt] = (n + chunks) * 8;
  need[kCpMsrc] = need[kCpMstart] = (n + 1) * 8;
  need[kCpTot] = hbxk::kTotWords * 8;
  if (int rc = compact_fits(c, need, {kCpEnt, kCpKeep, kCpKlass, kCpMsz, kCpTsz, kCpCnt, kCpMsrc, kCpMstart, kCpTot}))
    return rc;
  unsigned long long* d_tot = c->d_cp[kCpTot].as<unsigned long long>();
  unsigned long long* scans[3] = {c->d_cp[kCpMsz].as<unsigned long long>(), c->d_cp[kCpTsz].as<unsigned long long>(),
                                  c->d_cp[kCpCnt].as<unsigned long long>()};
  const hbxk::PlanArgs pa{c->d_cp[kCpEnt].as<hbx_dat_entry>(), c->d_cp[kCpKeep].as<uint8_t>(),
                          c->d_cp[kCpKlass].as<uint8_t>(), scans[0], scans[1], scans[2],
                          c->d_cp[kCpMsrc].as<unsigned long long>(), c->d_cp[kCpMstart].as<unsigned long long>(),
                          d_tot, *a, (uint32_t)n};
  const dim3 block(hbxk::kThreads), rows((uint32_t)((n + hbxk::kThreads - 1) / hbxk::kThreads));
  // 1. the plan: the prefix break, class and sizes, three scans, the offsets and the movers' list
  HBX_TRY(c, hipMemcpyAsync(c->d_cp[kCpEnt].p, ent, n * sizeof(hbx_dat_entry), hipMemcpyHostToDevice, s));
  HBX_TRY(c, hipMemcpyAsync(c->d_cp[kCpKeep].p, keep, n, hipMemcpyHostToDevice, s));
  HBX_TRY(c, hipMemsetAsync(d_tot, 0, hbxk::kTotWords * 8, s));
  HBX_TRY(c, hipMemsetAsync(d_tot + hbxk::kTotPast, 0xFF, 8, s));
  if (a->flags & HBX_CMP_F_KEEP_PREFIX) {
    HBX_TRY(c, hipMemsetAsync(d_tot + hbxk::kTotBreak, 0xFF, 8, s));
    hipLaunchKernelGGL(hbx_k16_break, rows, block, 0, s, pa);
  }
  hipLaunchKernelGGL(hbx_k16_plan, rows, block, 0, s, pa);
  for (unsigned long long* x : scans) {
    hipLaunchKernelGGL(hbx_k15_scan_sums, dim3((uint32_t)chunks), block, 0, s, x, n, x + n);
    hipLaunchKernelGGL(hbx_k15_scan_top, dim3(1), block, 0, s, x + n, chunks);
    hipLaunchKernelGGL(hbx_k15_scan_add, dim3((uint32_t)chunks), block, 0, s, x, n, x + n);
  }
  hipLaunchKernelGGL(hbx_k16_place, rows, block, 0, s, pa);
  HBX_TRY(c, hipGetLastError());
  HBX_TRY(c, hipMemcpyAsync(tot, d_tot, sizeof tot, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  const uint64_t n_moved = tot[hbxk::kTotCounts] & 0xFFFFFFFFull, n_kept = tot[hbxk::kTotCounts] >> 32;
  const uint64_t moved_bytes = tot[hbxk::kTotMoved], meta_bytes = tot[hbxk::kTotMeta];
  if (n_moved > n_kept || n_kept > n || moved_bytes > entry_bytes)
    return c->fail(HBX_ERR_STATE, "data file compaction: the device plan is inconsistent");
  hbxcmp::summarize(size, n, ent, entry_bytes, n_kept - n_moved, n_moved, n_kept, moved_bytes, meta_bytes,
                    tot[hbxk::kTotPast], sum);
  auto plan_out = [&]() -> int {
    if (o.klass) HBX_TRY(c, hipMemcpyAsync(o.klass, pa.klass, n, hipMemcpyDeviceToHost, s));
    if (o.new_off) HBX_TRY(c, hipMemcpyAsync(o.new_off, pa.msz, n * 8, hipMemcpyDeviceToHost, s));
    if (o.meta_off) HBX_TRY(c, hipMemcpyAsync(o.meta_off, pa.tsz, n * 8, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
    return HBX_OK;
  };
  if (sum->first_past_limit != hbxcmp::kNever) {
    if (int rc = plan_out()) return rc;
    return c->fail(HBX_ERR_CAPACITY, "data file compaction: entry " + std::to_string(sum->first_past_limit) +
                                         " would lie above the 16 GiB offset limit");
  }
  const uint64_t ix_bytes = HBX_IX_ENTRY * n_kept;
  if ((o.moved && moved_bytes > o.moved_cap) || (o.meta && meta_bytes > o.meta_cap) || (o.ix && ix_bytes > o.ix_cap))
    return c->fail(HBX_ERR_CAPACITY, "data file compaction: " + std::to_string(moved_bytes) + " moved, " +
                                         std::to_string(meta_bytes) + " meta and " + std::to_string(ix_bytes) +
                                         " index bytes do not fit the output capacities");
  // 2. the streams, each between two guards
  const bool want_moved = o.moved && moved_bytes, want_meta = o.meta && meta_bytes, want_ix = o.ix && ix_bytes;
  need[kCpMoved] = want_moved ? moved_bytes + 2 * kImageGuard : 0;
  need[kCpMeta] = want_meta ? meta_bytes + 2 * kImageGuard : 0;
  need[kCpIx] = want_ix ? ix_bytes : 0;
  if (int rc = compact_fits(c, need, {kCpMoved, kCpMeta, kCpIx})) return rc;
  uint8_t* d_moved = want_moved ? c->d_cp[kCpMoved].as<uint8_t>() + kImageGuard : nullptr;
  uint8_t* d_meta = want_meta ? c->d_cp[kCpMeta].as<uint8_t>() + kImageGuard : nullptr;
  if (want_moved) {
    const uint64_t tiles = (moved_bytes + c->k16_tile - 1) / c->k16_tile;
    if (tiles > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "data file compaction: too many tiles");
    HBX_TRY(c, hipMemsetAsync(d_moved - kImageGuard, kGuardByte, kImageGuard, s));
    HBX_TRY(c, hipMemsetAsync(d_moved + moved_bytes, kGuardByte, kImageGuard, s));
    const hbxk::PackArgs ka{image, pa.msrc, pa.mstart, d_moved, moved_bytes, (uint32_t)n_moved, c->k16_tile};
    hipLaunchKernelGGL(hbx_k16_pack, dim3((uint32_t)tiles), block, 0, s, ka);
    HBX_TRY(c, hipGetLastError());
    HBX_TRY(c, hipMemcpyAsync(guard, d_moved - kImageGuard, kImageGuard, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipMemcpyAsync(guard + kImageGuard, d_moved + moved_bytes, kImageGuard, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipMemcpyAsync(o.moved, d_moved, moved_bytes, hipMemcpyDeviceToHost, s));
  }
  if (want_meta || want_ix) {
    if (want_meta) {
      HBX_TRY(c, hipMemsetAsync(d_meta - kImageGuard, kGuardByte, kImageGuard, s));
      HBX_TRY(c, hipMemsetAsync(d_meta + meta_bytes, kGuardByte, kImageGuard, s));
    }
    const hbxk::MetaArgs ma{image, pa.ent, pa.klass, pa.msz, pa.tsz, pa.cnt, d_meta,
                            want_ix ? c->d_cp[kCpIx].as<uint8_t>() : nullptr, *a, (uint32_t)n};
    hipLaunchKernelGGL(hbx_k16_meta, dim3(hbxg::grid(n, 0)), block, 0, s, ma);
    HBX_TRY(c, hipGetLastError());
    if (want_meta) {
      HBX_TRY(c, hipMemcpyAsync(guard + 2 * kImageGuard, d_meta - kImageGuard, kImageGuard, hipMemcpyDeviceToHost, s));
      HBX_TRY(c, hipMemcpyAsync(guard + 3 * kImageGuard, d_meta + meta_bytes, kImageGuard, hipMemcpyDeviceToHost, s));
      HBX_TRY(c, hipMemcpyAsync(o.meta, d_meta, meta_bytes, hipMemcpyDeviceToHost, s));
    }
    if (want_ix) HBX_TRY(c, hipMemcpyAsync(o.ix, c->d_cp[kCpIx].p, ix_bytes, hipMemcpyDeviceToHost, s));
  }
  if (int rc = plan_out()) return rc;
  for (uint8_t b : guard)
    if (b != kGuardByte) return c->fail(HBX_ERR_STATE, "data file compaction: K16 wrote outside a stream");
  return HBX_OK;
  }();
  if (rc != HBX_OK) {
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
  }
  return rc;
}

// Both entry points behind their argument checks: `path` or `d_image`.
int compact_call(hbx_ctx* c, const char* path, const void* d_image, uint64_t size, uint64_t n,
                 const hbx_dat_entry* ent, const uint8_t* keep, const hbx_dat_compact_args* a, const CompactOut& o,
                 hbx_dat_compact_summary* sum) {
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  HBX_TRY(c, hipSetDevice(c->device));
  const uint8_t* image = static_cast<const uint8_t*>(d_image);
  uint64_t entry_bytes = 0;
  if (path) {  // (only the file tells its size: the entries are checked against it before anything is launched)
    struct stat st;
    if (::stat(path, &st) != 0) return c->fail(HBX_ERR_IO, std::string("cannot open ") + path + ": " + std::strerror(errno));
    size = (uint64_t)st.st_size;
  }
  if (!hbxcmp::args_ok(size, n, ent, keep, a, &entry_bytes))
    return c->fail(HBX_ERR_ARG, "data file compaction: the entries do not ascend inside a file of " + std::to_string(size) +
                                    " bytes, a size is not 29 + 16 n_links + data_len or is above 2^32 - 1, or a file "
                                    "number or a base is out of range");
  if (n == 0) {
    hbxcmp::summarize(size, 0, ent, 0, 0, 0, 0, 0, 0, hbxcmp::kNever, sum);
    return HBX_OK;
  }
  int rc = HBX_OK;
  if (path) {
    uint64_t loaded = 0;
    rc = datfile_load(c, path, &image, &loaded);
    if (rc == HBX_OK && loaded != size) rc = c->fail(HBX_ERR_IO, std::string(path) + " changed its size while it was read");
  }
  if (rc == HBX_OK) rc = compact_run(c, image, size, n, ent, keep, a, entry_bytes, o, sum);
  if (rc != HBX_OK) {  // leave the streams idle and the error state clean: the context stays usable
    (void)hipStreamSynchronize(c->stream);
    (void)hipStreamSynchronize(c->rstream);
    (void)hipGetLastError();
  }
  return rc;
}

}  // namespace

extern "C" {

int hbx_datfile_compact_plan(uint64_t size, uint64_t n, const hbx_dat_entry* entries, const uint8_t* keep,
                             const hbx_dat_compact_args* args, uint8_t* klass, uint64_t* new_off, uint64_t* meta_off,
                             hbx_dat_compact_summary* summary) {
  return hbxcmp::plan(size, n, entries, keep, args, klass, new_off, meta_off, summary);
}

int hbx_datfile_compact_device(hbx_ctx* c, const void* d_image, uint64_t size, uint64_t n,
                               const hbx_dat_entry* entries, const uint8_t* keep, const hbx_dat_compact_args* args,
                               uint8_t* klass, uint64_t* new_off, uint64_t* meta_off, uint8_t* moved_out,
                               uint64_t moved_cap, uint8_t* meta_out, uint64_t meta_cap, uint8_t* ix_out,
                               uint64_t ix_cap, hbx_dat_compact_summary* summary) {
  const CompactOut o{klass, new_off, meta_off, moved_out, moved_cap, meta_out, meta_cap, ix_out, ix_cap};
  if (!c || !d_image || !summary || !args || !compact_out_ok(o) ||
      (reinterpret_cast<uintptr_t>(d_image) & (HBX_ARENA_ALIGN - 1)) != 0)
    return HBX_ERR_ARG;
  return compact_call(c, nullptr, d_image, size, n, entries, keep, args, o, summary);
}

int hbx_datfile_compact_path(hbx_ctx* c, const char* path, uint64_t n, const hbx_dat_entry* entries,
                             const uint8_t* keep, const hbx_dat_compact_args* args, uint8_t* klass,
                             uint64_t* new_off, uint64_t* meta_off, uint8_t* moved_out, uint64_t moved_cap,
                             uint8_t* meta_out, uint64_t meta_cap, uint8_t* ix_out, uint64_t ix_cap,
                             hbx_dat_compact_summary* summary) {
  const CompactOut o{klass, new_off, meta_off, moved_out, moved_cap, meta_out, meta_cap, ix_out, ix_cap};
  if (!c || !path || !summary || !args || !compact_out_ok(o)) return HBX_ERR_ARG;
  return compact_call(c, path, nullptr, 0, n, entries, keep, args, o, summary);
}

int hbx_datfile_header_parse(const uint8_t* in, uint64_t len, uint32_t* filetype, uint32_t* version,
                             uint64_t* deadspace) {
  if (!in && len) return HBX_ERR_ARG;
  return hbxdat::header_parse(in, len, filetype, version, deadspace);
}

int hbx_datfile_entry_parse(const uint8_t* image, uint64_t size, uint64_t off, uint64_t max_block,
                            hbx_dat_record* rec) {
  if (!rec || (!image && size) || restore_mb(max_block) > kRestoreMaxBlock) return HBX_ERR_ARG;
  hbxdat::entry_parse(image, size, off, hbx_restore_in_bound(max_block), rec);
  return HBX_OK;
}

int hbx_datfile_walk(uint64_t size, uint64_t n_cand, const hbx_dat_record* cand, const uint32_t* plain_len,
                     uint64_t n_gaps, const uint64_t* gap_offs, const int64_t* gap_skips, hbx_dat_entry* entries,
                     uint64_t entry_cap, hbx_dat_span* spans, uint64_t span_cap, hbx_dat_summary* summary) {
  if (!summary || (n_cand && !cand) || (n_gaps && (!gap_offs || !gap_skips)) || (entry_cap && !entries) ||
      (span_cap && !spans))
    return HBX_ERR_ARG;
  for (uint64_t i = 1; i < n_cand; i++)
    if (cand[i].off <= cand[i - 1].off) return HBX_ERR_ARG;
  for (uint64_t i = 1; i < n_gaps; i++)
    if (gap_offs[i] <= gap_offs[i - 1]) return HBX_ERR_ARG;
  return hbxdat::walk(size, n_cand, cand, plain_len, n_gaps, gap_offs, gap_skips, entries, entry_cap, spans, span_cap,
                      summary);
}

int hbx_datfile_check_device(hbx_ctx* c, const void* d_image, uint64_t size, uint64_t max_block,
                             uint64_t max_candidates, uint64_t window_bytes, hbx_dat_entry* entries,
                             uint64_t entry_cap, hbx_dat_span* spans, uint64_t span_cap, uint8_t* links,
                             uint64_t link_cap, hbx_dat_summary* summary) {
  if (!c || !d_image || !summary || (entry_cap && !entries) || (span_cap && !spans) || (link_cap && !links) ||
      !datfile_args_ok(d_image, max_block))
    return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  const int rc = datfile_check(c, static_cast<const uint8_t*>(d_image), size, restore_mb(max_block), max_candidates,
                               dat_window(window_bytes), entries, entry_cap, spans, span_cap, links,
                               link_cap, summary);
  if (rc) (void)hipStreamSynchronize(c->stream);
  return rc;
}

int hbx_datfile_check_path(hbx_ctx* c, const char* path, uint64_t max_block, uint64_t max_candidates,
                           uint64_t window_bytes, hbx_dat_entry* entries, uint64_t entry_cap, hbx_dat_span* spans,
                           uint64_t span_cap, uint8_t* links, uint64_t link_cap, hbx_dat_summary* summary) {
  if (!c || !path || !summary || (entry_cap && !entries) || (span_cap && !spans) || (link_cap && !links) ||
      !datfile_args_ok(nullptr, max_block))
    return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  const uint8_t* image = nullptr;
  uint64_t size = 0;
  int rc = datfile_load(c, path, &image, &size);
  if (rc == HBX_OK)
    rc = datfile_check(c, image, size, restore_mb(max_block), max_candidates, dat_window(window_bytes),
                       entries, entry_cap, spans, span_cap, links, link_cap, summary);
  if (rc) (void)hipStreamSynchronize(c->stream);
  return rc;
}

int hbx_datfile_verify_at(hbx_ctx* c, const void* d_image, uint64_t size, const char* path, uint64_t n,
                          const uint64_t* offs, const uint8_t* expect_ids, int content, uint64_t max_block,
                          uint64_t window_bytes, uint32_t* status) {
  if (!c || (d_image != nullptr) == (path != nullptr) || (n && (!offs || !expect_ids || !status)) ||
      !datfile_args_ok(d_image, max_block))
    return HBX_ERR_ARG;
  if (n == 0) return HBX_OK;
  std::lock_guard<std::mutex> g(c->mu);
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  HBX_TRY(c, hipSetDevice(c->device));
  const uint8_t* image = static_cast<const uint8_t*>(d_image);
  int rc = path ? datfile_load(c, path, &image, &size) : HBX_OK;
  if (rc == HBX_OK)
    rc = datfile_verify_at(c, image, size, n, offs, expect_ids, content, restore_mb(max_block),
                           dat_window(window_bytes), status);
  if (rc) (void)hipStreamSynchronize(c->stream);
  return rc;
}

}  // extern "C"

// ---- K17: the index files (DESIGN.md §5 "K17") -----------------------------
#include "hbx_index_calls.hip"
