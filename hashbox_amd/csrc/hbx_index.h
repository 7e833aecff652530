// hbx_index.h — the store's open-addressed index files on the host (host side
// of K17, hbx_index.hip; no device code, no HIP call).
//
// pkg/storagedb/index.go, gc.go:24-206, integrity.go:354-410; include/hbxgpu.h
// "Index files" states the rules.  Every function here works in place over
// host images and is the exact statement of what the device calls compute:
// the two must agree byte for byte and word for word.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/hbxgpu.h"

namespace hbxi {

constexpr uint64_t kNone = ~0ull;

static_assert(sizeof(hbx_ix_hit) == 32 && sizeof(hbx_ix_live) == 48 && sizeof(hbx_ix_killed) == 32, "C-ABI");
static_assert(sizeof(hbx_ix_file_stats) == 72 && sizeof(hbx_ix_summary) == 80, "C-ABI");
static_assert(sizeof(hbx_ix_sweep_summary) == 72, "C-ABI");
static_assert(sizeof(hbx_ix_compact_summary) == 16 + 8 * HBX_IX_FILES_MAX, "C-ABI");

inline uint32_t be16(const uint8_t* p) { return ((uint32_t)p[0] << 8) | p[1]; }
inline void put_be16(uint8_t* p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}
inline uint32_t be32(const uint8_t* p) {
  return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3];
}
// sixByteLocation.Get (storagedb.go:102-106)
inline void location(const uint8_t* p, uint32_t* file, uint64_t* off) {
  uint64_t l = 0;
  for (int b = 0; b < 6; b++) l = (l << 8) | p[b];
  *file = (uint32_t)(l >> 34);
  *off = l & 0x3FFFFFFFFull;
}
// calculateIXEntryOffset (index.go:48-50) as a slot number
inline uint64_t home(const uint8_t* id) { return ((uint64_t)id[13] << 16) | ((uint64_t)id[14] << 8) | id[15]; }
inline uint64_t slot_off(uint64_t slot) { return HBX_IX_HEADER + HBX_IX_ENTRY * slot; }
inline bool live(uint32_t flags) { return (flags & HBX_IX_F_EXISTS) && !(flags & HBX_IX_F_INVALID); }

inline bool size_ok(uint64_t size) {
  return size >= HBX_IX_HEADER && (size - HBX_IX_HEADER) % HBX_IX_ENTRY == 0 && size <= HBX_IX_SIZE_MAX;
}
// The 16-byte header: "HSIX", version 1 (storagedb.go:40-49, 150-165).
inline bool header_ok(const uint8_t* h) { return be32(h) == HBX_IX_FILETYPE && be32(h + 4) == HBX_IX_VERSION; }

// What every call checks of its images.
inline int files_ok(uint32_t n_files, const uint8_t* const* images, const uint64_t* sizes) {
  if (n_files == 0 || n_files > HBX_IX_FILES_MAX || !images || !sizes) return HBX_ERR_ARG;
  for (uint32_t f = 0; f < n_files; f++) {
    if (!images[f]) return HBX_ERR_ARG;
    if (!size_ok(sizes[f]) || !header_ok(images[f])) return HBX_ERR_FORMAT;
  }
  return HBX_OK;
}

struct Place {
  bool found;
  uint32_t file;
  uint64_t off;
};

// findIXOffset (index.go:54-107): the rule.
inline Place find(uint32_t n_files, const uint8_t* const* images, const uint64_t* sizes, const uint8_t* id,
                  bool stop_on_free) {
  const uint64_t base = slot_off(home(id));
  uint32_t f = 0, free_f = 0;
  uint64_t o = base, free_o = base;
  bool have_free = false, stop = false;
  while (!stop) {
    if (f >= n_files) break;        // ran out of index files
    if (o > sizes[f]) break;
    for (uint32_t i = 0; i < HBX_IX_PROBE_LIMIT; i++) {
      if (o >= sizes[f]) {          // room at the end of the file
        stop = true;
        break;
      }
      const uint8_t* s = images[f] + o;
      const uint32_t flags = be16(s);
      if (live(flags)) {
        if (std::memcmp(s + 2, id, 16) == 0) return Place{true, f, o};
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
  return have_free ? Place{false, free_f, free_o} : Place{false, f, o};
}

inline void hit_of(const uint8_t* const* images, const Place& p, hbx_ix_hit* h) {
  std::memset(h, 0, sizeof *h);
  h->found = p.found ? 1u : 0u;
  h->file = p.file;
  h->offset = p.off;
  if (p.found) {
    const uint8_t* s = images[p.file] + p.off;
    h->flags = be16(s);
    location(s + 18, &h->meta_file, &h->meta_off);
  }
}

inline int lookup(uint32_t n_files, const uint8_t* const* images, const uint64_t* sizes, uint64_t n,
                  const uint8_t* ids, int stop_on_free, hbx_ix_hit* hits) {
  if (int rc = files_ok(n_files, images, sizes)) return rc;
  if (n && (!ids || !hits)) return HBX_ERR_ARG;
  for (uint64_t i = 0; i < n; i++)
    hit_of(images, find(n_files, images, sizes, ids + 16 * i, stop_on_free != 0), hits + i);
  return HBX_OK;
}

// The pass of CheckIndexes (integrity.go:354-410) with CompactIndexes' counters
// and the table of the live entries in (file, offset) order.
inline int scan(uint32_t n_files, const uint8_t* const* images, const uint64_t* sizes, hbx_ix_live* live_out,
                uint64_t live_cap, hbx_ix_file_stats* per_file, hbx_ix_summary* sum) {
  if (int rc = files_ok(n_files, images, sizes)) return rc;
  if (!sum || (live_cap && !live_out)) return HBX_ERR_ARG;
  std::memset(sum, 0, sizeof *sum);
  sum->n_files = n_files;
  uint64_t j = 0;
  for (uint32_t f = 0; f < n_files; f++) {
    hbx_ix_file_stats st;
    std::memset(&st, 0, sizeof st);
    st.slots = (sizes[f] - HBX_IX_HEADER) / HBX_IX_ENTRY;
    st.first_misplaced = kNone;
    st.trunc_point = HBX_IX_HEADER;
    for (uint64_t o = HBX_IX_HEADER; o < sizes[f]; o += HBX_IX_ENTRY) {
      const uint8_t* s = images[f] + o;
      const uint32_t flags = be16(s);
      if (flags & HBX_IX_F_INVALID) {
        st.n_invalid++;
      } else if (!(flags & HBX_IX_F_EXISTS)) {
        st.n_empty++;
      } else {
        st.n_live++;
        if (flags & HBX_IX_F_MARKED) st.n_marked++;
        if (flags & HBX_IX_F_NOLINKS) st.n_nolinks++;
        st.trunc_point = o + HBX_IX_ENTRY;
        if (o < slot_off(home(s + 2))) {  // integrity.go:387-390
          st.n_misplaced++;
          if (st.first_misplaced == kNone) st.first_misplaced = o;
        }
        const Place p = find(n_files, images, sizes, s + 2, false);
        const uint32_t state = !p.found ? 2u : (p.file == f && p.off == o) ? 0u : 1u;
        if (state == 1) sum->n_obsolete++;
        if (state == 2) sum->n_cut_off++;
        if (j < live_cap) {
          hbx_ix_live* e = live_out + j;
          std::memset(e, 0, sizeof *e);
          std::memcpy(e->id, s + 2, 16);
          e->flags = flags;
          e->ix_file = f;
          e->ix_offset = o;
          location(s + 18, &e->meta_file, &e->meta_off);
          e->state = state;
        }
        j++;
      }
    }
    if (per_file) per_file[f] = st;
    sum->slots += st.slots;
    sum->n_live += st.n_live;
    sum->n_invalid += st.n_invalid;
    sum->n_empty += st.n_empty;
    sum->n_marked += st.n_marked;
    sum->n_nolinks += st.n_nolinks;
    sum->n_misplaced += st.n_misplaced;
  }
  return j > live_cap && live_out ? HBX_ERR_CAPACITY : HBX_OK;
}

// The write half of MarkIndexes (gc.go:46-54).
inline int mark(uint32_t n_files, uint8_t* const* images, const uint64_t* sizes, uint64_t n, const uint8_t* ids,
                uint8_t* found, uint64_t* n_missing) {
  if (int rc = files_ok(n_files, images, sizes)) return rc;
  if (n && !ids) return HBX_ERR_ARG;
  uint64_t missing = 0;
  for (uint64_t i = 0; i < n; i++) {
    const Place p = find(n_files, images, sizes, ids + 16 * i, false);
    if (p.found) {
      uint8_t* s = images[p.file] + p.off;
      put_be16(s, be16(s) | HBX_IX_F_MARKED);
    } else {
      missing++;
    }
    if (found) found[i] = p.found ? 1 : 0;
  }
  if (n_missing) *n_missing = missing;
  return HBX_OK;
}

// True when no 16-byte ID occurs twice among n of them, `stride` bytes apart.
inline bool ids_unique(uint64_t n, const uint8_t* first, uint64_t stride) {
  std::vector<std::array<uint8_t, 16>> v(n);
  for (uint64_t i = 0; i < n; i++) std::memcpy(v[i].data(), first + stride * i, 16);
  std::sort(v.begin(), v.end());
  return std::adjacent_find(v.begin(), v.end()) == v.end();
}

// changeMetaLocation (meta.go:122-128) and RecoverData's repair of an existing
// entry (integrity.go:216-240) from 24-byte StorageIXEntry records.
inline int update(uint32_t n_files, uint8_t* const* images, const uint64_t* sizes, uint64_t n, const uint8_t* recs,
                  uint8_t* status) {
  if (int rc = files_ok(n_files, images, sizes)) return rc;
  if (n && !recs) return HBX_ERR_ARG;
  if (!ids_unique(n, recs + 2, HBX_IX_ENTRY)) return HBX_ERR_ARG;
  for (uint64_t i = 0; i < n; i++) {
    const uint8_t* r = recs + HBX_IX_ENTRY * i;
    const Place p = find(n_files, images, sizes, r + 2, false);
    if (p.found) {
      uint8_t* s = images[p.file] + p.off;
      put_be16(s, (be16(s) & ~HBX_IX_F_NOLINKS) | (be16(r) & HBX_IX_F_NOLINKS));
      std::memcpy(s + 18, r + 18, 6);
    }
    if (status) status[i] = p.found ? 0 : 1;
  }
  return HBX_OK;
}

// SweepIndexes (gc.go:70-151).  sizes[f] may grow up to caps[f].
inline int sweep(uint32_t n_files, uint8_t* const* images, uint64_t* sizes, const uint64_t* caps, uint8_t* action,
                 uint64_t* moved_to, uint64_t live_cap, hbx_ix_killed* killed, uint64_t killed_cap,
                 hbx_ix_sweep_summary* sum) {
  if (int rc = files_ok(n_files, images, sizes)) return rc;
  if (!sum || !caps || (live_cap && (!action || !moved_to)) || (killed_cap && !killed)) return HBX_ERR_ARG;
  for (uint32_t f = 0; f < n_files; f++)
    if (caps[f] < sizes[f]) return HBX_ERR_ARG;
  std::memset(sum, 0, sizeof *sum);
  sum->first_abort = kNone;
  // the capacities first: the live entries, and those of them without a mark
  uint64_t n_live = 0, n_unmarked = 0;
  for (uint32_t f = 0; f < n_files; f++)
    for (uint64_t o = HBX_IX_HEADER; o < sizes[f]; o += HBX_IX_ENTRY) {
      const uint32_t flags = be16(images[f] + o);
      if (!live(flags)) continue;
      n_live++;
      if (!(flags & HBX_IX_F_MARKED)) n_unmarked++;
    }
  sum->n_live = n_live;
  if (n_live > live_cap || n_unmarked > killed_cap) {
    sum->n_deleted = sum->swept_records = n_unmarked;
    return HBX_ERR_CAPACITY;
  }
  // what a failing call puts back
  std::vector<std::vector<uint8_t>> saved(n_files);
  const std::vector<uint64_t> saved_sizes(sizes, sizes + n_files);
  for (uint32_t f = 0; f < n_files; f++) saved[f].assign(images[f], images[f] + sizes[f]);
  auto restore = [&]() {
    for (uint32_t f = 0; f < n_files; f++) {
      std::memcpy(images[f], saved[f].data(), saved[f].size());
      sizes[f] = saved_sizes[f];
    }
  };
  uint64_t j = 0;
  for (uint32_t f = 0; f < n_files; f++) {
    const uint64_t size = sizes[f];  // (a move never lengthens the file being swept)
    for (uint64_t o = HBX_IX_HEADER; o < size; o += HBX_IX_ENTRY) {
      uint8_t* s = images[f] + o;
      uint32_t flags = be16(s);
      if (!live(flags)) continue;  // Invalid: skipped; Exists clear: not touched
      uint8_t act;
      moved_to[2 * j] = moved_to[2 * j + 1] = kNone;
      if (!(flags & HBX_IX_F_MARKED)) {
        hbx_ix_killed* k = killed + sum->n_deleted;
        std::memset(k, 0, sizeof *k);
        std::memcpy(k->id, s + 2, 16);
        location(s + 18, &k->meta_file, &k->meta_off);
        sum->n_deleted++;
        flags |= HBX_IX_F_INVALID;
        act = HBX_IX_ACT_DELETED;
      } else {
        flags &= ~HBX_IX_F_MARKED;
        const Place p = find(n_files, images, sizes, s + 2, true);
        if (p.file == f && p.off == o) {
          sum->n_stay++;
          act = HBX_IX_ACT_STAY;
        } else if (p.found) {
          flags |= HBX_IX_F_INVALID;
          sum->n_obsolete++;
          act = HBX_IX_ACT_OBSOLETE;
        } else if (p.file < f || (p.file == f && p.off < o)) {
          if (p.off + HBX_IX_ENTRY > caps[p.file]) {
            restore();
            return HBX_ERR_CAPACITY;
          }
          uint8_t* t = images[p.file] + p.off;
          if (p.off + HBX_IX_ENTRY > sizes[p.file]) {  // the file grows: zeros up to the new slot
            std::memset(images[p.file] + sizes[p.file], 0, p.off - sizes[p.file]);
            sizes[p.file] = p.off + HBX_IX_ENTRY;
          }
          std::memcpy(t, s, HBX_IX_ENTRY);  // writeIXEntry (index.go:117-132)
          put_be16(t, flags);
          moved_to[2 * j] = p.file;
          moved_to[2 * j + 1] = p.off;
          flags |= HBX_IX_F_INVALID;
          sum->n_moved++;
          act = HBX_IX_ACT_MOVED;
        } else {  // gc.go:129-131: left as it is, the mark too
          if (sum->first_abort == kNone) sum->first_abort = j;
          sum->n_abort++;
          action[j++] = HBX_IX_ACT_ABORT;
          continue;
        }
      }
      put_be16(s, flags);
      action[j++] = act;
    }
  }
  sum->swept_records = sum->n_deleted;
  for (uint32_t f = 0; f < n_files; f++)
    if (sizes[f] > saved_sizes[f]) sum->n_grown++;
  if (sum->n_abort) {
    restore();
    return HBX_ERR_FORMAT;
  }
  return HBX_OK;
}

// CompactIndexes (gc.go:153-206).
inline int compact(uint32_t n_files, uint8_t* const* images, uint64_t* sizes, hbx_ix_compact_summary* sum) {
  if (int rc = files_ok(n_files, images, sizes)) return rc;
  if (!sum) return HBX_ERR_ARG;
  std::memset(sum, 0, sizeof *sum);
  sum->n_files = n_files;
  for (uint32_t f = 0; f < n_files; f++) {
    uint64_t trunc = HBX_IX_HEADER;
    for (uint64_t o = HBX_IX_HEADER; o < sizes[f]; o += HBX_IX_ENTRY) {
      uint8_t* s = images[f] + o;
      const uint32_t flags = be16(s);
      if (flags & HBX_IX_F_INVALID) {
        std::memset(s, 0, HBX_IX_ENTRY);
        sum->cleared++;
      } else if (flags & HBX_IX_F_EXISTS) {
        trunc = o + HBX_IX_ENTRY;
      }
    }
    sizes[f] = trunc;
    sum->size[f] = trunc;
  }
  return HBX_OK;
}

}  // namespace hbxi
