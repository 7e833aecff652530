// hbx_index_calls.hip — the C-ABI of K17 (include/hbxgpu.h "Index files"):
// hbx_index_* over a handle in device memory and hbx_index_*_host over host
// images.  Included at the end of hbx_engine.hip: it uses the context, its
// lock, its result stream and its buffers' types.  Kernels: hbx_index.hip;
// the host statement of every operation: hbx_index.h.
#pragma once

namespace {

constexpr uint64_t kIxCallChunk = 1ull << 22;  // IDs per probe launch of a direct call: 64 MiB of IDs, 128 MiB of hits
constexpr uint64_t kIxSlack = 64;              // bytes behind an image's capacity

inline uint64_t ix_bytes(uint64_t columns) { return HBX_IX_HEADER + (uint64_t)HBX_IX_ENTRY * columns; }
inline uint64_t ix_chunks(uint64_t n) { return (n + hbxg::kScanChunk - 1) / hbxg::kScanChunk; }
constexpr uint64_t kIxWorkgroups = 2048;  // of the kernels whose workgroups stride over tiles
inline dim3 ix_grid(uint64_t items) { return dim3((uint32_t)((items + hbxx::kThreads - 1) / hbxx::kThreads)); }
inline unsigned long long* ix_counters(hbx_index* x) {
  return x->d_stat.as<unsigned long long>() + HBX_IX_FILES_MAX * hbxx::kStWords;
}

// The checks every call on a handle shares; the context's lock is held.
int ix_direct(hbx_ctx* c, hbx_index* x) {
  if (std::find(c->indexes.begin(), c->indexes.end(), x) == c->indexes.end())
    return c->fail(HBX_ERR_ARG, "not an index of this context");
  if (!c->pending.empty()) return c->fail(HBX_ERR_STATE, "submitted batches are still pending");
  if (c->broken) return c->fail(HBX_ERR_STATE, "context is unusable after a failed submit; destroy it");
  return c->hip(hipSetDevice(c->device), "hipSetDevice");
}

// Grow the named buffers to their sizes, after checking the growth against the free device memory.
int ix_fits(hbx_ctx* c, std::initializer_list<std::pair<DevBuf*, uint64_t>> want) {
  uint64_t grow = 0;
  for (const auto& w : want)
    if (w.second > w.first->cap) grow += w.second + 4096;  // (a buffer that grows is freed only after the check)
  if (grow) {
    size_t fr = 0, tot = 0;
    HBX_TRY(c, hipMemGetInfo(&fr, &tot));
    if (grow > fr)
      return c->fail(HBX_ERR_CAPACITY, "the index needs " + std::to_string(grow) + " more bytes of device memory, " +
                                           std::to_string(fr) + " are free");
  }
  for (const auto& w : want) HBX_TRY(c, w.first->ensure(w.second));
  return HBX_OK;
}

// The table of the files as they stand, on the host and on the device.
int ix_table(hbx_ctx* c, hbx_index* x, const uint64_t* live0 = nullptr) {
  hbxx::Tab& t = x->tab;
  std::memset(&t, 0, sizeof t);
  t.n = x->n;
  t.lim = ix_bytes(x->columns);
  uint64_t tiles = 0;
  for (uint32_t f = 0; f < x->n; f++) {
    t.f[f].live0 = live0 ? live0[f] : 0;
    t.f[f].img = x->img[f].as<uint8_t>();
    t.f[f].size = x->size[f];
    t.f[f].slots = (x->size[f] - HBX_IX_HEADER) / HBX_IX_ENTRY;
    t.f[f].tile0 = tiles;
    tiles += (t.f[f].slots + hbxx::kTile - 1) / hbxx::kTile;
  }
  x->tiles = tiles;
  HBX_TRY(c, hipMemcpyAsync(x->d_tab.p, &t, sizeof t, hipMemcpyHostToDevice, c->rstream));
  return HBX_OK;
}

// Every image to the capacity of `columns` slots (never less than it has): a
// new allocation, the file's bytes copied, zeros behind them.
int ix_grow(hbx_ctx* c, hbx_index* x, uint64_t columns) {
  if (columns <= x->columns) return HBX_OK;
  const uint64_t bytes = ix_bytes(columns) + kIxSlack;
  size_t fr = 0, tot = 0;
  HBX_TRY(c, hipMemGetInfo(&fr, &tot));
  if ((bytes + 4096) * x->n > fr)
    return c->fail(HBX_ERR_CAPACITY, "the index needs " + std::to_string((bytes + 4096) * x->n) +
                                         " more bytes of device memory, " + std::to_string(fr) + " are free");
  hipStream_t s = c->rstream;
  for (uint32_t f = 0; f < x->n; f++) {
    DevBuf nb;
    HBX_TRY(c, nb.ensure(bytes));
    hipError_t e = hipMemcpyAsync(nb.p, x->img[f].p, x->size[f], hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess) e = hipMemsetAsync(nb.as<uint8_t>() + x->size[f], 0, bytes - x->size[f], s);
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
      nb.release();
      return c->hip(e, "growing an index image");
    }
    x->img[f].release();
    x->img[f] = nb;
  }
  x->columns = columns;
  return HBX_OK;
}

// K15's exclusive scan of v[0 .. n) in place; v has ix_chunks(n) more words behind it.
void ix_excl_scan(hipStream_t s, unsigned long long* v, uint64_t n) {
  const uint64_t chunks = ix_chunks(n);
  const dim3 block(hbxg::kThreads);
  hipLaunchKernelGGL(hbx_k15_scan_sums, dim3((uint32_t)chunks), block, 0, s, v, n, v + n);
  hipLaunchKernelGGL(hbx_k15_scan_top, dim3(1), block, 0, s, v + n, chunks);
  hipLaunchKernelGGL(hbx_k15_scan_add, dim3((uint32_t)chunks), block, 0, s, v, n, v + n);
}

// What the count kernel found, per file and in all.
void ix_stats_out(const hbx_index* x, const unsigned long long* st, hbx_ix_file_stats* per_file, hbx_ix_summary* sum) {
  std::memset(sum, 0, sizeof *sum);
  sum->n_files = x->n;
  for (uint32_t f = 0; f < x->n; f++) {
    const unsigned long long* r = st + (uint64_t)f * hbxx::kStWords;
    hbx_ix_file_stats fs;
    fs.slots = (x->size[f] - HBX_IX_HEADER) / HBX_IX_ENTRY;
    fs.n_live = r[hbxx::kStLive];
    fs.n_invalid = r[hbxx::kStInvalid];
    fs.n_empty = r[hbxx::kStEmpty];
    fs.n_marked = r[hbxx::kStMarked];
    fs.n_nolinks = r[hbxx::kStNoLinks];
    fs.n_misplaced = r[hbxx::kStMisplaced];
    fs.first_misplaced = r[hbxx::kStFirstMisplaced];
    fs.trunc_point = ix_bytes(r[hbxx::kStLastLive]);
    if (per_file) per_file[f] = fs;
    sum->slots += fs.slots;
    sum->n_live += fs.n_live;
    sum->n_invalid += fs.n_invalid;
    sum->n_empty += fs.n_empty;
    sum->n_marked += fs.n_marked;
    sum->n_nolinks += fs.n_nolinks;
    sum->n_misplaced += fs.n_misplaced;
  }
  sum->n_obsolete = st[HBX_IX_FILES_MAX * hbxx::kStWords + hbxx::kCtObsolete];
  sum->n_cut_off = st[HBX_IX_FILES_MAX * hbxx::kStWords + hbxx::kCtCutOff];
}

// The scan on the device: the statistics into st[kStatWords] (host), the live
// table into d_live, the tiles' exclusive live counts into d_tiles.  The
// counters behind the files' rows are zeroed here, first_abort set to none.
int ix_scan(hbx_ctx* c, hbx_index* x, bool want_state, unsigned long long* st, uint64_t* max_home_end) {
  hipStream_t s = c->rstream;
  if (int rc = ix_table(c, x)) return rc;
  unsigned long long* d_stat = x->d_stat.as<unsigned long long>();
  HBX_TRY(c, hipMemsetAsync(d_stat, 0, hbxx::kStatWords * 8, s));
  for (uint32_t f = 0; f < x->n; f++)
    HBX_TRY(c, hipMemsetAsync(d_stat + (uint64_t)f * hbxx::kStWords + hbxx::kStFirstMisplaced, 0xFF, 8, s));
  HBX_TRY(c, hipMemsetAsync(ix_counters(x) + hbxx::kCtFirstAbort, 0xFF, 8, s));
  const uint64_t tiles = x->tiles;
  if (tiles > 0x7FFFFFFFull) return c->fail(HBX_ERR_ARG, "the index has too many tiles");
  if (tiles) {
    if (int rc = ix_fits(c, {{&x->d_tiles, (tiles + ix_chunks(tiles) + 1) * 8}})) return rc;
    const hbxx::ScanArgs a{x->d_tab.as<hbxx::Tab>(), d_stat, x->d_tiles.as<unsigned long long>(), nullptr, 0, tiles, 0};
    hipLaunchKernelGGL(hbx_k17_count, dim3((uint32_t)std::min(tiles, kIxWorkgroups)), dim3(hbxx::kThreads), 0, s, a);
    HBX_TRY(c, hipGetLastError());
  }
  HBX_TRY(c, hipMemcpyAsync(st, d_stat, hbxx::kStatWords * 8, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  uint64_t n_live = 0, mh = 0;
  for (uint32_t f = 0; f < x->n; f++) {
    n_live += st[(uint64_t)f * hbxx::kStWords + hbxx::kStLive];
    mh = std::max<uint64_t>(mh, st[(uint64_t)f * hbxx::kStWords + hbxx::kStMaxHome]);
  }
  if (max_home_end) *max_home_end = mh;
  if (n_live == 0) return HBX_OK;
  if (int rc = ix_fits(c, {{&x->d_live, n_live * sizeof(hbx_ix_live)}})) return rc;
  ix_excl_scan(s, x->d_tiles.as<unsigned long long>(), tiles);
  const hbxx::ScanArgs a{x->d_tab.as<hbxx::Tab>(), d_stat,     x->d_tiles.as<unsigned long long>(),
                         x->d_live.as<hbx_ix_live>(), n_live, tiles, want_state ? 1u : 0u};
  hipLaunchKernelGGL(hbx_k17_pack, dim3((uint32_t)tiles), dim3(hbxx::kThreads), 0, s, a);
  HBX_TRY(c, hipGetLastError());
  if (want_state) {
    HBX_TRY(c, hipMemcpyAsync(st, d_stat, hbxx::kStatWords * 8, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
  }
  return HBX_OK;
}

// n IDs (16 bytes each, host) probed in chunks; after(at, k) runs behind each chunk's probe, whose hits lie in d_hits.
int ix_probe(hbx_ctx* c, hbx_index* x, uint64_t n, const uint8_t* ids, bool stop_on_free,
             const std::function<int(uint64_t, uint64_t)>& after) {
  hipStream_t s = c->rstream;
  if (int rc = ix_table(c, x)) return rc;
  for (uint64_t at = 0; at < n; at += kIxCallChunk) {
    const uint64_t k = std::min(kIxCallChunk, n - at);
    if (int rc = ix_fits(c, {{&x->d_in, k * 16}, {&x->d_hits, k * sizeof(hbx_ix_hit)}})) return rc;
    HBX_TRY(c, hipMemcpyAsync(x->d_in.p, ids + 16 * at, k * 16, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(hbx_k17_probe, ix_grid(k), dim3(hbxx::kThreads), 0, s,
                       static_cast<const hbxx::Tab*>(x->d_tab.as<hbxx::Tab>()),
                       static_cast<const uint64_t*>(x->d_in.as<uint64_t>()), k, stop_on_free ? 1u : 0u,
                       x->d_hits.as<hbx_ix_hit>());
    HBX_TRY(c, hipGetLastError());
    if (int rc = after(at, k)) return rc;
    HBX_TRY(c, hipStreamSynchronize(s));
  }
  return HBX_OK;
}

// Leave the streams idle and the error state clean: the context stays usable.
int ix_done(hbx_ctx* c, int rc) {
  if (rc != HBX_OK) {
    (void)hipStreamSynchronize(c->rstream);
    (void)hipGetLastError();
  }
  return rc;
}

// hbx_index_open and _open_paths: image f comes from get(f, size), which may read it into `hold`.
int ix_open(hbx_ctx* c, uint32_t n_files, const uint64_t* sizes,
            const std::function<int(uint32_t, const uint8_t**)>& get, hbx_index** out) {
  for (uint32_t f = 0; f < n_files; f++)
    if (!hbxi::size_ok(sizes[f]))
      return c->fail(HBX_ERR_FORMAT, "index file " + std::to_string(f) + ": " + std::to_string(sizes[f]) +
                                         " bytes is no header and whole 24-byte slots within the size limit");
  HBX_TRY(c, hipSetDevice(c->device));
  uint64_t columns = 0;
  for (uint32_t f = 0; f < n_files; f++) columns = std::max(columns, (sizes[f] - HBX_IX_HEADER) / HBX_IX_ENTRY);
  const uint64_t bytes = ix_bytes(columns) + kIxSlack;
  size_t fr = 0, tot = 0;
  HBX_TRY(c, hipMemGetInfo(&fr, &tot));
  if ((bytes + 4096) * n_files + (1ull << 20) > fr)
    return c->fail(HBX_ERR_CAPACITY, "the index images need " + std::to_string((bytes + 4096) * n_files) +
                                         " bytes of device memory, " + std::to_string(fr) + " are free");
  hbx_index* x = new hbx_index();
  x->n = n_files;
  x->columns = columns;
  hipStream_t s = c->rstream;
  const int rc = [&]() -> int {
    HBX_TRY(c, x->d_tab.ensure(sizeof(hbxx::Tab)));
    HBX_TRY(c, x->d_stat.ensure(hbxx::kStatWords * 8));
    for (uint32_t f = 0; f < n_files; f++) {
      const uint8_t* image = nullptr;
      if (int rc = get(f, &image)) return rc;
      if (!hbxi::header_ok(image))
        return c->fail(HBX_ERR_FORMAT, "index file " + std::to_string(f) + ": not an \"HSIX\" header of version 1");
      x->size[f] = sizes[f];
      HBX_TRY(c, x->img[f].ensure(bytes));
      HBX_TRY(c, hipMemcpyAsync(x->img[f].p, image, sizes[f], hipMemcpyHostToDevice, s));
      HBX_TRY(c, hipMemsetAsync(x->img[f].as<uint8_t>() + sizes[f], 0, bytes - sizes[f], s));
      HBX_TRY(c, hipStreamSynchronize(s));  // (the image's memory may go before the next one comes)
    }
    return HBX_OK;
  }();
  if (rc != HBX_OK) {
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
    x->release();
    delete x;
    return rc;
  }
  c->indexes.push_back(x);
  *out = x;
  return HBX_OK;
}

int ix_sweep(hbx_ctx* c, hbx_index* x, uint8_t* action, uint64_t* moved_to, uint64_t live_cap, hbx_ix_killed* killed,
             uint64_t killed_cap, hbx_ix_sweep_summary* sum) {
  hipStream_t s = c->rstream;
  std::memset(sum, 0, sizeof *sum);
  sum->first_abort = hbxi::kNone;
  unsigned long long st[hbxx::kStatWords];
  uint64_t home_end = 0;
  if (int rc = ix_scan(c, x, false, st, &home_end)) return rc;
  hbx_ix_summary all;
  ix_stats_out(x, st, nullptr, &all);
  const uint64_t n_live = all.n_live, n_unmarked = all.n_live - all.n_marked;
  sum->n_live = n_live;
  if (n_live > live_cap || n_unmarked > killed_cap) {
    sum->n_deleted = sum->swept_records = n_unmarked;
    return c->fail(HBX_ERR_CAPACITY, "index sweep: " + std::to_string(n_live) + " live entries and " +
                                         std::to_string(n_unmarked) + " to delete do not fit the output capacities");
  }
  if (n_live == 0) return HBX_OK;
  // every column a move can name: home + 681 of every live entry
  const uint64_t columns = std::max<uint64_t>(
      x->columns, std::min<uint64_t>(home_end ? home_end - 1 + HBX_IX_PROBE_LIMIT : 0, HBX_IX_SLOTS_MAX));
  if (int rc = ix_grow(c, x, columns)) return rc;
  uint64_t live0[HBX_IX_FILES_MAX] = {};
  for (uint32_t f = 1; f < x->n; f++) live0[f] = live0[f - 1] + st[(uint64_t)(f - 1) * hbxx::kStWords + hbxx::kStLive];
  if (int rc = ix_table(c, x, live0)) return rc;
  // what a sweep that meets an abort puts back, and the buffers of the call
  const uint64_t link_words = columns + 1, kill_words = n_live;
  if (int rc = ix_fits(c, {{&x->d_link, (link_words + ix_chunks(link_words) + 1) * 8},
                           {&x->d_act, n_live},
                           {&x->d_moved, n_live * 16},
                           {&x->d_kflag, (kill_words + ix_chunks(kill_words) + 1) * 8},
                           {&x->d_killed, std::max<uint64_t>(n_unmarked, 1) * sizeof(hbx_ix_killed)}}))
    return rc;
  for (uint32_t f = 0; f < x->n; f++) {
    if (int rc = ix_fits(c, {{&x->save[f], x->size[f]}})) return rc;
    HBX_TRY(c, hipMemcpyAsync(x->save[f].p, x->img[f].p, x->size[f], hipMemcpyDeviceToDevice, s));
  }
  unsigned long long* d_link = x->d_link.as<unsigned long long>();
  unsigned long long* d_kflag = x->d_kflag.as<unsigned long long>();
  const hbx_ix_live* d_live = x->d_live.as<hbx_ix_live>();
  const dim3 block(hbxx::kThreads);
  HBX_TRY(c, hipMemsetAsync(d_link, 0, link_words * 8, s));
  hipLaunchKernelGGL(hbx_k17_spans, ix_grid(n_live), block, 0, s, d_live, n_live, columns, d_link);
  ix_excl_scan(s, d_link, link_words);
  const hbxx::SweepArgs a{x->d_tab.as<hbxx::Tab>(), d_live, d_link,
                          x->d_stat.as<unsigned long long>(), x->d_act.as<uint8_t>(),
                          x->d_moved.as<unsigned long long>(), n_live, columns};
  hipLaunchKernelGGL(hbx_k17_sweep, ix_grid(columns), block, 0, s, a);
  hipLaunchKernelGGL(hbx_k17_tally, dim3((uint32_t)std::min<uint64_t>(ix_grid(n_live).x, kIxWorkgroups)), block, 0, s,
                     static_cast<const uint8_t*>(a.action), n_live, d_kflag, x->d_stat.as<unsigned long long>());
  ix_excl_scan(s, d_kflag, kill_words);
  hipLaunchKernelGGL(hbx_k17_kill_put, ix_grid(n_live), block, 0, s, static_cast<const uint8_t*>(a.action), d_live, n_live,
                     static_cast<const unsigned long long*>(d_kflag), x->d_killed.as<hbx_ix_killed>());
  HBX_TRY(c, hipGetLastError());
  HBX_TRY(c, hipMemcpyAsync(st, x->d_stat.p, hbxx::kStatWords * 8, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipStreamSynchronize(s));
  const unsigned long long* ct = st + HBX_IX_FILES_MAX * hbxx::kStWords;
  sum->n_deleted = ct[hbxx::kCtAct + HBX_IX_ACT_DELETED];
  sum->n_stay = ct[hbxx::kCtAct + HBX_IX_ACT_STAY];
  sum->n_obsolete = ct[hbxx::kCtAct + HBX_IX_ACT_OBSOLETE];
  sum->n_moved = ct[hbxx::kCtAct + HBX_IX_ACT_MOVED];
  sum->n_abort = ct[hbxx::kCtAct + HBX_IX_ACT_ABORT];
  sum->first_abort = ct[hbxx::kCtFirstAbort];
  sum->swept_records = sum->n_deleted;
  if (sum->n_deleted != n_unmarked ||
      sum->n_deleted + sum->n_stay + sum->n_obsolete + sum->n_moved + sum->n_abort != n_live)
    return c->fail(HBX_ERR_STATE, "index sweep: the device's counts are inconsistent");
  HBX_TRY(c, hipMemcpyAsync(action, a.action, n_live, hipMemcpyDeviceToHost, s));
  HBX_TRY(c, hipMemcpyAsync(moved_to, a.moved_to, n_live * 16, hipMemcpyDeviceToHost, s));
  if (sum->n_deleted)
    HBX_TRY(c, hipMemcpyAsync(killed, x->d_killed.p, sum->n_deleted * sizeof(hbx_ix_killed), hipMemcpyDeviceToHost, s));
  if (sum->n_abort) {  // put the images back; a move past an end wrote behind a size: zeros again
    for (uint32_t f = 0; f < x->n; f++) {
      HBX_TRY(c, hipMemcpyAsync(x->img[f].p, x->save[f].p, x->size[f], hipMemcpyDeviceToDevice, s));
      HBX_TRY(c, hipMemsetAsync(x->img[f].as<uint8_t>() + x->size[f], 0, ix_bytes(columns) - x->size[f], s));
    }
  } else {
    for (uint32_t f = 0; f < x->n; f++)
      if (ct[hbxx::kCtSize + f] > x->size[f]) {
        x->size[f] = ct[hbxx::kCtSize + f];
        sum->n_grown++;
      }
  }
  HBX_TRY(c, hipStreamSynchronize(s));
  for (uint32_t f = 0; f < x->n; f++) x->save[f].release();
  if (sum->n_abort) {
    sum->n_grown = 0;
    return c->fail(HBX_ERR_FORMAT, "index sweep: findIXOffset names a later place for " + std::to_string(sum->n_abort) +
                                       " entries, the first is live entry " + std::to_string(sum->first_abort) +
                                       "; the index is unchanged");
  }
  return HBX_OK;
}

}  // namespace

extern "C" {

int hbx_index_open(hbx_ctx* c, uint32_t n_files, const uint8_t* const* images, const uint64_t* sizes, hbx_index** out) {
  if (!c || !out) return HBX_ERR_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> g(c->mu);
  if (n_files == 0 || n_files > HBX_IX_FILES_MAX || !images || !sizes)
    return c->fail(HBX_ERR_ARG, "hbx_index_open: 1 .. " + std::to_string(HBX_IX_FILES_MAX) + " index files");
  for (uint32_t f = 0; f < n_files; f++)
    if (!images[f]) return c->fail(HBX_ERR_ARG, "hbx_index_open: null image");
  return ix_open(c, n_files, sizes, [&](uint32_t f, const uint8_t** image) {
    *image = images[f];
    return (int)HBX_OK;
  }, out);
}

int hbx_index_open_paths(hbx_ctx* c, uint32_t n_files, const char* const* paths, hbx_index** out) {
  if (!c || !out) return HBX_ERR_ARG;
  *out = nullptr;
  std::lock_guard<std::mutex> g(c->mu);
  if (n_files == 0 || n_files > HBX_IX_FILES_MAX || !paths)
    return c->fail(HBX_ERR_ARG, "hbx_index_open_paths: 1 .. " + std::to_string(HBX_IX_FILES_MAX) + " index files");
  uint64_t sizes[HBX_IX_FILES_MAX] = {};
  for (uint32_t f = 0; f < n_files; f++) {
    if (!paths[f]) return c->fail(HBX_ERR_ARG, "hbx_index_open_paths: null path");
    struct stat st;
    if (::stat(paths[f], &st) != 0)
      return c->fail(HBX_ERR_IO, std::string("cannot open ") + paths[f] + ": " + std::strerror(errno));
    sizes[f] = (uint64_t)st.st_size;
  }
  std::vector<uint8_t> hold;
  return ix_open(c, n_files, sizes, [&](uint32_t f, const uint8_t** image) -> int {
    const int fd = ::open(paths[f], O_RDONLY | O_CLOEXEC);
    if (fd < 0) return c->fail(HBX_ERR_IO, std::string("cannot open ") + paths[f] + ": " + std::strerror(errno));
    hold.resize(sizes[f]);
    std::string err;
    const int rc = read_range(fd, paths[f], 0, sizes[f], hold.data(), 8, err);
    ::close(fd);
    if (rc) return c->fail(HBX_ERR_IO, err);
    *image = hold.data();
    return HBX_OK;
  }, out);
}

int hbx_index_close(hbx_ctx* c, hbx_index* x) {
  if (!c || !x) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  auto it = std::find(c->indexes.begin(), c->indexes.end(), x);
  if (it == c->indexes.end()) return c->fail(HBX_ERR_ARG, "not an index of this context");
  HBX_TRY(c, hipSetDevice(c->device));
  HBX_TRY(c, hipStreamSynchronize(c->rstream));
  c->indexes.erase(it);
  x->release();
  delete x;
  return HBX_OK;
}

int hbx_index_sizes(hbx_ctx* c, hbx_index* x, uint64_t* sizes) {
  if (!c || !x || !sizes) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = ix_direct(c, x)) return rc;
  for (uint32_t f = 0; f < x->n; f++) sizes[f] = x->size[f];
  return HBX_OK;
}

int hbx_index_export(hbx_ctx* c, hbx_index* x, uint32_t file, uint8_t* out, uint64_t cap, uint64_t* n) {
  if (!c || !x || !n) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = ix_direct(c, x)) return rc;
  if (file >= x->n) return c->fail(HBX_ERR_ARG, "hbx_index_export: no such file");
  *n = x->size[file];
  if (x->size[file] > cap)
    return c->fail(HBX_ERR_CAPACITY, "hbx_index_export: the file has " + std::to_string(x->size[file]) + " bytes");
  if (!out) return c->fail(HBX_ERR_ARG, "hbx_index_export: null output");
  return ix_done(c, [&]() -> int {
    HBX_TRY(c, hipMemcpyAsync(out, x->img[file].p, x->size[file], hipMemcpyDeviceToHost, c->rstream));
    HBX_TRY(c, hipStreamSynchronize(c->rstream));
    return HBX_OK;
  }());
}

int hbx_index_lookup(hbx_ctx* c, hbx_index* x, uint64_t n, const uint8_t* ids, int stop_on_free, hbx_ix_hit* hits) {
  if (!c || !x || (n && (!ids || !hits))) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = ix_direct(c, x)) return rc;
  if (n == 0) return HBX_OK;
  return ix_done(c, ix_probe(c, x, n, ids, stop_on_free != 0, [&](uint64_t at, uint64_t k) -> int {
    HBX_TRY(c, hipMemcpyAsync(hits + at, x->d_hits.p, k * sizeof(hbx_ix_hit), hipMemcpyDeviceToHost, c->rstream));
    return HBX_OK;
  }));
}

int hbx_index_scan(hbx_ctx* c, hbx_index* x, hbx_ix_live* live, uint64_t live_cap, hbx_ix_file_stats* per_file,
                   hbx_ix_summary* summary) {
  if (!c || !x || !summary || (live_cap && !live)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = ix_direct(c, x)) return rc;
  return ix_done(c, [&]() -> int {
    unsigned long long st[hbxx::kStatWords];
    if (int rc = ix_scan(c, x, true, st, nullptr)) return rc;
    ix_stats_out(x, st, per_file, summary);
    const uint64_t k = std::min<uint64_t>(summary->n_live, live_cap);
    if (live && k) {
      HBX_TRY(c, hipMemcpyAsync(live, x->d_live.p, k * sizeof(hbx_ix_live), hipMemcpyDeviceToHost, c->rstream));
      HBX_TRY(c, hipStreamSynchronize(c->rstream));
    }
    if (live && summary->n_live > live_cap)
      return c->fail(HBX_ERR_CAPACITY, "hbx_index_scan: the index holds " + std::to_string(summary->n_live) + " live entries");
    return HBX_OK;
  }());
}

int hbx_index_mark(hbx_ctx* c, hbx_index* x, uint64_t n, const uint8_t* ids, uint8_t* found, uint64_t* n_missing) {
  if (!c || !x || (n && !ids)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = ix_direct(c, x)) return rc;
  if (n_missing) *n_missing = 0;
  if (n == 0) return HBX_OK;
  return ix_done(c, [&]() -> int {
    hipStream_t s = c->rstream;
    unsigned long long missing = 0;
    HBX_TRY(c, hipMemsetAsync(ix_counters(x) + hbxx::kCtMissing, 0, 8, s));
    const int rc = ix_probe(c, x, n, ids, false, [&](uint64_t at, uint64_t k) -> int {
      if (int rc = ix_fits(c, {{&x->d_out, k}})) return rc;
      hipLaunchKernelGGL(hbx_k17_mark, ix_grid(k), dim3(hbxx::kThreads), 0, s,
                         static_cast<const hbxx::Tab*>(x->d_tab.as<hbxx::Tab>()),
                         static_cast<const hbx_ix_hit*>(x->d_hits.as<hbx_ix_hit>()), k, x->d_out.as<uint8_t>(),
                         x->d_stat.as<unsigned long long>());
      HBX_TRY(c, hipGetLastError());
      if (found) HBX_TRY(c, hipMemcpyAsync(found + at, x->d_out.p, k, hipMemcpyDeviceToHost, s));
      return HBX_OK;
    });
    if (rc) return rc;
    HBX_TRY(c, hipMemcpyAsync(&missing, ix_counters(x) + hbxx::kCtMissing, 8, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
    if (n_missing) *n_missing = missing;
    return HBX_OK;
  }());
}

int hbx_index_update(hbx_ctx* c, hbx_index* x, uint64_t n, const uint8_t* recs, uint8_t* status) {
  if (!c || !x || (n && !recs)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = ix_direct(c, x)) return rc;
  if (n == 0) return HBX_OK;
  if (!hbxi::ids_unique(n, recs + 2, HBX_IX_ENTRY)) return c->fail(HBX_ERR_ARG, "hbx_index_update: an ID occurs twice");
  std::vector<uint8_t> ids(n * 16);
  for (uint64_t i = 0; i < n; i++) std::memcpy(ids.data() + 16 * i, recs + HBX_IX_ENTRY * i + 2, 16);
  // the records behind the IDs' staging, each chunk's in its own buffer
  return ix_done(c, ix_probe(c, x, n, ids.data(), false, [&](uint64_t at, uint64_t k) -> int {
    hipStream_t s = c->rstream;
    if (int rc = ix_fits(c, {{&x->d_out, k}, {&x->d_kflag, k * HBX_IX_ENTRY}})) return rc;
    HBX_TRY(c, hipMemcpyAsync(x->d_kflag.p, recs + HBX_IX_ENTRY * at, k * HBX_IX_ENTRY, hipMemcpyHostToDevice, s));
    hipLaunchKernelGGL(hbx_k17_update, ix_grid(k), dim3(hbxx::kThreads), 0, s,
                       static_cast<const hbxx::Tab*>(x->d_tab.as<hbxx::Tab>()),
                       static_cast<const hbx_ix_hit*>(x->d_hits.as<hbx_ix_hit>()), k,
                       static_cast<const uint8_t*>(x->d_kflag.as<uint8_t>()), x->d_out.as<uint8_t>());
    HBX_TRY(c, hipGetLastError());
    if (status) HBX_TRY(c, hipMemcpyAsync(status + at, x->d_out.p, k, hipMemcpyDeviceToHost, s));
    return HBX_OK;
  }));
}

int hbx_index_sweep(hbx_ctx* c, hbx_index* x, uint8_t* action, uint64_t* moved_to, uint64_t live_cap,
                    hbx_ix_killed* killed, uint64_t killed_cap, hbx_ix_sweep_summary* summary) {
  if (!c || !x || !summary || (live_cap && (!action || !moved_to)) || (killed_cap && !killed)) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = ix_direct(c, x)) return rc;
  return ix_done(c, ix_sweep(c, x, action, moved_to, live_cap, killed, killed_cap, summary));
}

int hbx_index_compact(hbx_ctx* c, hbx_index* x, hbx_ix_compact_summary* summary) {
  if (!c || !x || !summary) return HBX_ERR_ARG;
  std::lock_guard<std::mutex> g(c->mu);
  if (int rc = ix_direct(c, x)) return rc;
  return ix_done(c, [&]() -> int {
    hipStream_t s = c->rstream;
    std::memset(summary, 0, sizeof *summary);
    summary->n_files = x->n;
    if (int rc = ix_table(c, x)) return rc;
    unsigned long long st[hbxx::kStatWords] = {};
    unsigned long long* d_stat = x->d_stat.as<unsigned long long>();
    HBX_TRY(c, hipMemsetAsync(d_stat, 0, hbxx::kStatWords * 8, s));
    if (x->tiles) {
      hipLaunchKernelGGL(hbx_k17_compact, dim3((uint32_t)std::min(x->tiles, kIxWorkgroups)), dim3(hbxx::kThreads), 0, s,
                         static_cast<const hbxx::Tab*>(x->d_tab.as<hbxx::Tab>()), x->tiles, d_stat);
      HBX_TRY(c, hipGetLastError());
    }
    HBX_TRY(c, hipMemcpyAsync(st, d_stat, hbxx::kStatWords * 8, hipMemcpyDeviceToHost, s));
    HBX_TRY(c, hipStreamSynchronize(s));
    summary->cleared = st[HBX_IX_FILES_MAX * hbxx::kStWords + hbxx::kCtCleared];
    for (uint32_t f = 0; f < x->n; f++) {
      const uint64_t size = ix_bytes(st[(uint64_t)f * hbxx::kStWords + hbxx::kStLastLive]);
      if (size > x->size[f]) return c->fail(HBX_ERR_STATE, "index compaction: the device's truncation point is inconsistent");
      // what the file loses is zero from now on, as everything behind a size
      if (size < x->size[f]) HBX_TRY(c, hipMemsetAsync(x->img[f].as<uint8_t>() + size, 0, x->size[f] - size, s));
      x->size[f] = size;
      summary->size[f] = size;
    }
    HBX_TRY(c, hipStreamSynchronize(s));
    return HBX_OK;
  }());
}

int hbx_index_lookup_host(uint32_t n_files, uint8_t* const* images, uint64_t* sizes, const uint64_t*, uint64_t n,
                          const uint8_t* ids, int stop_on_free, hbx_ix_hit* hits) {
  return hbxi::lookup(n_files, images, sizes, n, ids, stop_on_free, hits);
}

int hbx_index_scan_host(uint32_t n_files, uint8_t* const* images, uint64_t* sizes, const uint64_t*, hbx_ix_live* live,
                        uint64_t live_cap, hbx_ix_file_stats* per_file, hbx_ix_summary* summary) {
  return hbxi::scan(n_files, images, sizes, live, live_cap, per_file, summary);
}

int hbx_index_mark_host(uint32_t n_files, uint8_t* const* images, uint64_t* sizes, const uint64_t*, uint64_t n,
                        const uint8_t* ids, uint8_t* found, uint64_t* n_missing) {
  return hbxi::mark(n_files, images, sizes, n, ids, found, n_missing);
}

int hbx_index_update_host(uint32_t n_files, uint8_t* const* images, uint64_t* sizes, const uint64_t*, uint64_t n,
                          const uint8_t* recs, uint8_t* status) {
  return hbxi::update(n_files, images, sizes, n, recs, status);
}

int hbx_index_sweep_host(uint32_t n_files, uint8_t* const* images, uint64_t* sizes, const uint64_t* caps,
                         uint8_t* action, uint64_t* moved_to, uint64_t live_cap, hbx_ix_killed* killed,
                         uint64_t killed_cap, hbx_ix_sweep_summary* summary) {
  return hbxi::sweep(n_files, images, sizes, caps, action, moved_to, live_cap, killed, killed_cap, summary);
}

int hbx_index_compact_host(uint32_t n_files, uint8_t* const* images, uint64_t* sizes, const uint64_t*,
                           hbx_ix_compact_summary* summary) {
  return hbxi::compact(n_files, images, sizes, summary);
}

}  // extern "C"
