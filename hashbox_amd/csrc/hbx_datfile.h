// hbx_datfile.h — the storage data file on the host: its header, the
// structural rules of an entry and RecoverData's walk (host side of K14,
// hbx_datfile.hip; no device code, no HIP call).
//
// pkg/storagedb/storagedb.go:40-53, data.go:33-37, 142-164, integrity.go:74-143;
// include/hbxgpu.h states the format and the walk.  entry_parse restates
// hbx_k14_parse rule for rule: the two must give the same record for every
// position of every file.  The walk never looks at the file: it sees the
// sorted "hblk" positions with the status each one got, the sorted "Cgap"
// positions with their skips, and the file's size.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstring>

#include "../../include/hbxgpu.h"

namespace hbxdat {

inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | (uint32_t)p[3];
}
inline uint64_t be64(const uint8_t* p) { return ((uint64_t)be32(p) << 32) | be32(p + 4); }

inline int header_parse(const uint8_t* in, uint64_t len, uint32_t* filetype, uint32_t* version, uint64_t* deadspace) {
  const uint32_t ft = len >= 4 ? be32(in) : 0u, ver = len >= 8 ? be32(in + 4) : 0u;
  const uint64_t dead = len >= 16 ? be64(in + 8) : 0ull;
  if (filetype) *filetype = ft;
  if (version) *version = ver;
  if (deadspace) *deadspace = dead;
  return len >= HBX_DAT_HEADER && ft == HBX_DAT_FILETYPE && ver == HBX_DAT_VERSION ? HBX_OK : HBX_ERR_FORMAT;
}

// Rule 3.  Every read is preceded by a comparison of its end with `avail`.
inline void entry_parse(const uint8_t* image, uint64_t size, uint64_t off, uint64_t in_bound, hbx_dat_record* r) {
  std::memset(r, 0, sizeof *r);
  r->off = off;
  r->status = HBX_DAT_ST_INVALID;
  const uint64_t avail = off < size ? size - off : 0;
  if (avail < 4) return;
  const uint8_t* p = image + off;
  if (be32(p) != HBX_DAT_MARKER) return;
  r->flags = HBX_DAT_F_MARKER;
  if (avail < 24) return;
  const uint32_t nl = be32(p + 20);
  const uint64_t head = 24ull + 16ull * nl + 5ull;
  if (avail < head) return;
  const uint8_t type = p[head - 5];
  const uint32_t dl = be32(p + (head - 4));
  if (avail - head < dl || (type != HBX_BLOCK_RAW && type != HBX_BLOCK_ZLIB) || dl > in_bound) return;
  r->status = 0;
  r->size = head + dl;
  r->data_off = off + head;
  r->links_off = off + 24;
  r->data_len = dl;
  r->n_links = nl;
  r->type = type;
  std::memcpy(r->id, p + 4, 16);
}

// The gap marker at off: true with its skip if 12 bytes lie inside the file and say "Cgap".
inline bool gap_parse(const uint8_t* image, uint64_t size, uint64_t off, int64_t* skip) {
  if (off >= size || size - off < 12 || be32(image + off) != HBX_DAT_GAP) return false;
  *skip = (int64_t)be64(image + off + 4);
  return true;
}

inline int walk(uint64_t size, uint64_t n_cand, const hbx_dat_record* cand, const uint32_t* plain_len,
                uint64_t n_gaps, const uint64_t* gap_offs, const int64_t* gap_skips, hbx_dat_entry* entries,
                uint64_t entry_cap, hbx_dat_span* spans, uint64_t span_cap, hbx_dat_summary* s) {
  constexpr uint64_t kNone = ~0ull;
  s->size = size;
  s->n_candidates = n_cand;
  s->n_gap_markers = n_gaps;
  s->gap_past_eof = 0;
  s->n_unreached = s->n_entries = s->entry_bytes = s->n_gaps = s->gap_bytes = 0;
  s->n_broken = s->broken_bytes = s->n_spans = s->n_links = 0;
  s->truncate_at = kNone;
  uint64_t reached = 0;
  uint64_t broken = kNone, failed = 0;
  uint32_t first_status = 0;
  auto span = [&](uint64_t off, uint64_t len, uint32_t kind, uint32_t status, uint64_t nf) {
    if (s->n_spans < span_cap) spans[s->n_spans] = hbx_dat_span{off, len, kind, status, nf};
    s->n_spans++;
    (kind == HBX_DAT_SPAN_GAP ? s->n_gaps : s->n_broken)++;
    (kind == HBX_DAT_SPAN_GAP ? s->gap_bytes : s->broken_bytes) += len;
  };
  auto cand_at = [&](uint64_t off) {  // index of the first candidate at a position >= off
    return (uint64_t)(std::lower_bound(cand, cand + n_cand, off,
                                       [](const hbx_dat_record& r, uint64_t o) { return r.off < o; }) - cand);
  };
  uint64_t offset = HBX_DAT_HEADER;
  while (offset < size) {
    if (size - offset >= 12) {
      const uint64_t* g = std::lower_bound(gap_offs, gap_offs + n_gaps, offset);
      if (g != gap_offs + n_gaps && *g == offset && gap_skips[g - gap_offs] > 0) {
        const uint64_t skip = (uint64_t)gap_skips[g - gap_offs], left = size - offset;
        if (skip > left) s->gap_past_eof = 1;
        span(offset, std::min(skip, left), HBX_DAT_SPAN_GAP, 0u, 0u);
        offset += std::min(skip, left);
        if (offset >= size) break;
      }
    }
    const uint64_t block = offset;
    const uint64_t k = cand_at(block);
    const bool here = k < n_cand && cand[k].off == block;
    if (here) reached++;
    // (a record that claims to be good but does not fit the file is a failure: the walk always ends)
    const bool fits = here && cand[k].size >= HBX_DAT_ENTRY_MIN && cand[k].size <= size - block;
    if (here && cand[k].status == 0 && fits) {
      const hbx_dat_record& r = cand[k];
      if (broken != kNone) {
        span(broken, block - broken, HBX_DAT_SPAN_BROKEN, first_status, failed);
        broken = kNone;
      }
      if (s->n_entries < entry_cap) {
        hbx_dat_entry& e = entries[s->n_entries];
        std::memset(&e, 0, sizeof e);
        e.off = r.off;
        e.size = r.size;
        e.data_off = r.data_off;
        e.link_base = s->n_links;
        e.n_links = r.n_links;
        e.data_len = r.data_len;
        e.plain_len = plain_len ? plain_len[k] : (r.type == HBX_BLOCK_RAW ? r.data_len : 0u);
        e.type = r.type;
        std::memcpy(e.id, r.id, 16);
      }
      s->n_entries++;
      s->entry_bytes += r.size;
      s->n_links += r.n_links;
      offset = block + r.size;
      continue;
    }
    if (broken == kNone) {
      broken = block;
      first_status = here && cand[k].status ? cand[k].status : HBX_DAT_ST_INVALID;
      failed = 0;
    }
    if (here) failed++;
    const uint64_t nx = cand_at(block + 1);  // forwardToDataMarker from block + 1
    if (nx >= n_cand) break;
    offset = cand[nx].off;
  }
  if (broken != kNone) {
    span(broken, size - broken, HBX_DAT_SPAN_BROKEN, first_status, failed);
    s->truncate_at = broken;
  }
  s->n_unreached = n_cand - reached;
  return (s->n_entries > entry_cap || s->n_spans > span_cap) ? HBX_ERR_CAPACITY : HBX_OK;
}

}  // namespace hbxdat
