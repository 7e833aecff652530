// hbx_compact.h — CompactFile's plan on the host (host side of K16,
// hbx_compact.hip; no device code, no HIP call).
//
// pkg/storagedb/gc.go:208-318; include/hbxgpu.h states the rules.  plan()
// restates hbx_k16_break / _plan / _place rule for rule, sequentially: the two
// must give the same class, offsets and summary for every table.
#pragma once

#include <cstdint>
#include <cstring>

#include "../../include/hbxgpu.h"

namespace hbxcmp {

constexpr uint64_t kNever = ~0ull;
constexpr uint64_t kBaseMax = 1ull << 62;  // a base above this could carry an offset out of 64 bits

// Rule 8 but for the context and the image; *entry_bytes = the sum of the sizes.
inline bool args_ok(uint64_t size, uint64_t n, const hbx_dat_entry* e, const uint8_t* keep,
                    const hbx_dat_compact_args* a, uint64_t* entry_bytes) {
  *entry_bytes = 0;
  if (!a || (n && (!e || !keep)) || n > 0x7FFFFFFFull) return false;
  if (a->file_no > HBX_DAT_FILE_MAX || a->dst_file_no > HBX_DAT_FILE_MAX || a->meta_file_no > HBX_DAT_FILE_MAX)
    return false;
  if (a->dst_base < HBX_DAT_HEADER || a->meta_base < HBX_DAT_HEADER || a->dst_base > kBaseMax ||
      a->meta_base > kBaseMax)
    return false;
  uint64_t end = HBX_DAT_HEADER;  // where the entry before ends: ascending and not overlapping
  for (uint64_t i = 0; i < n; i++) {
    if (e[i].size != 29ull + 16ull * e[i].n_links + e[i].data_len) return false;
    if (e[i].size > 0xFFFFFFFFull) return false;  // (a meta entry's DataSize is a uint32, in the reference too)
    if (e[i].off < end || e[i].off > size || e[i].size > size - e[i].off) return false;
    end = e[i].off + e[i].size;
    *entry_bytes += e[i].size;
  }
  return true;
}

// What the summary holds besides the device's totals.
inline void summarize(uint64_t size, uint64_t n, const hbx_dat_entry* e, uint64_t entry_bytes, uint64_t n_stay,
                      uint64_t n_moved, uint64_t n_kept, uint64_t moved_bytes, uint64_t meta_bytes, uint64_t past,
                      hbx_dat_compact_summary* s) {
  std::memset(s, 0, sizeof *s);
  s->n_entries = n;
  s->n_stay = n_stay;
  s->n_moved = n_moved;
  s->n_dropped = n - n_kept;
  s->stay_end = n_stay ? e[n_stay - 1].off + e[n_stay - 1].size : HBX_DAT_HEADER;
  s->moved_bytes = moved_bytes;
  const uint64_t stay_bytes = s->stay_end - HBX_DAT_HEADER;
  s->dropped_bytes = entry_bytes - stay_bytes - moved_bytes;
  s->deleted_bytes = size >= HBX_DAT_HEADER ? size - HBX_DAT_HEADER - stay_bytes - moved_bytes : 0;
  s->meta_bytes = meta_bytes;
  s->n_meta = n_kept;
  s->first_past_limit = past;
}

inline int plan(uint64_t size, uint64_t n, const hbx_dat_entry* e, const uint8_t* keep, const hbx_dat_compact_args* a,
                uint8_t* klass, uint64_t* new_off, uint64_t* meta_off, hbx_dat_compact_summary* s) {
  uint64_t entry_bytes = 0;
  if (!s || !args_ok(size, n, e, keep, a, &entry_bytes)) return HBX_ERR_ARG;
  bool prefix = (a->flags & HBX_CMP_F_KEEP_PREFIX) != 0;
  uint64_t mark = HBX_DAT_HEADER;  // the reference's highWaterMark
  uint64_t n_stay = 0, n_moved = 0, moved = 0, meta = 0, past = kNever;
  for (uint64_t i = 0; i < n; i++) {
    uint8_t k = HBX_CMP_DROP;
    uint64_t no = kNever, mo = kNever;
    if (!keep[i]) {
      prefix = false;
    } else {
      prefix = prefix && e[i].off == mark;
      if (prefix) {
        k = HBX_CMP_STAY;
        no = e[i].off;
        mark = e[i].off + e[i].size;
        n_stay++;
      } else {
        k = HBX_CMP_MOVE;
        no = a->dst_base + moved;
        moved += e[i].size;
        n_moved++;
      }
      mo = a->meta_base + meta;
      meta += HBX_META_HEAD + 16ull * e[i].n_links;
      if (past == kNever && (no > HBX_DAT_OFFSET_LIMIT || mo > HBX_DAT_OFFSET_LIMIT)) past = i;
    }
    if (klass) klass[i] = k;
    if (new_off) new_off[i] = no;
    if (meta_off) meta_off[i] = mo;
  }
  summarize(size, n, e, entry_bytes, n_stay, n_moved, n_stay + n_moved, moved, meta, past, s);
  return past == kNever ? HBX_OK : HBX_ERR_CAPACITY;
}

}  // namespace hbxcmp
