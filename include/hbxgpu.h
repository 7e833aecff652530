/*
 * hbxgpu.h — C-ABI of the MI355X rollsum-split + block-ID engine
 * (libhbxgpu.so).  Drop-in for Hashback's per-file chunker and block hashing.
 *
 * Reference interfaces replaced (fredli74/hashbox; the reference has no FFI
 * seam for this path, so the seam is cut at storeFile — SURVEY.md §8b):
 *
 *   hbx_chunk_hash        hashback/store.go:111-185  storeFile's split loop
 *                         (store.go:129-166) + the per-chunk
 *                         Client.StoreData -> NewHashboxBlock -> HashData
 *                         (pkg/core/client.go:556-560, block.go:39-43, 96-111)
 *   hbx_chunk_hash_batch  the same, for many files at once (tree walk order
 *                         store.go:201-397 is the caller's business)
 *   hbx_chunk_hash_device the same, files already resident in device memory
 *   hbx_submit_device /   asynchronous, pipelined form: any number of batches
 *   hbx_wait              in flight per context, completed in FIFO order
 *   hbx_store_paths       storeFile(path) for many files on disk, end to end
 *   hbx_block_id          HashboxBlock.HashData for an arbitrary block with
 *                         links (pkg/core/block.go:96-111), e.g. the
 *                         FileChainBlock of store.go:187-188
 *   hbx_file_summary      entry.ContentType / entry.ContentBlockID written by
 *                         store.go:187-196
 *   hbx_verify_blocks     HashboxBlock.VerifyBlock (block.go:152-174), batched
 *   hbx_file_entry_*,     FileEntry / FileChainBlock / DirectoryBlock
 *   hbx_chain_block_*,    Serialize + Unserialize (hashback/hashback.go:80-214)
 *   hbx_directory_block_* and storeDir's block id (store.go:201-234)
 *   hbx_deflate_blocks    HashboxBlock.CompressData, zlib (block.go:133-184)
 *   hbx_inflate_blocks_device  UncompressData (block.go:113-131), on the device
 *   hbx_restore_blocks    restoreFileData / diffFileData over a block chain
 *                         (hashback/restore.go:45-66, 249-277): UncompressData,
 *                         VerifyBlock and the file's bytes in one call
 *   hbx_restore_file_stream  the same for a chain of any length, in windows
 *   hbx_wire_*            ProtocolMessage framing of every message type
 *                         (pkg/core/protocol.go:184-264), block-store encoders
 *
 * Conventions
 *   - Every function returns an int status: 0 = OK, negative = error
 *     (HBX_ERR_*).  hbx_last_error(ctx) describes the last failure.  The
 *     library never aborts or exits (the Go wrapper turns a non-zero status
 *     into core.Abort, pkg/core/utils.go:22-37).
 *   - The caller owns every buffer passed in.  The library never frees caller
 *     memory and never keeps a caller pointer after the call returns, except
 *     between hbx_submit_device and the hbx_wait that completes the batch,
 *     where the device arena and the output arrays must stay valid (use
 *     hbx_alloc_pinned memory from cgo: cgo forbids C from retaining Go
 *     pointers).
 *   - One context = one GPU and its own HIP streams.  Calls on one context are
 *     serialised by an internal lock; use one context per GPU (or per
 *     goroutine) to run in parallel.  A context is safe to call from many
 *     threads, and distinct contexts run concurrently.  hbx_wait completes
 *     batches in submit order whichever thread calls it.  The text of
 *     hbx_last_error(ctx) is per context: with several threads on one context
 *     it may describe another thread's failure, so judge a call by its status
 *     and read the text right after it for diagnostics only.  The call takes
 *     the context's lock (it waits for a call in progress there, and must not
 *     be made from a callback) and returns a copy that stays valid until the
 *     calling thread's next hbx_last_error.  hbx_last_error(NULL) is per
 *     calling thread.
 *   - Block IDs are 16 raw MD5 bytes, exactly Go's core.Byte128 (core.go:26).
 *   - cut_ends[i] is the file offset where chunk i ends (exclusive); chunk i
 *     starts at cut_ends[i-1] (0 for i = 0).
 *   - Capacity: every chunk except the last is >= 64 KiB, so a file of len
 *     bytes has at most hbx_max_chunks(len) = len/65536 + 1 chunks.
 *   - Device inputs must be complete when the engine reads them: its HIP
 *     streams do not wait for the caller's streams.  Synchronize the producing
 *     stream first, or call hbx_after_stream(ctx, stream) before the submit
 *     (a GPU-side wait; the host does not block).
 */
#ifndef HBXGPU_H
#define HBXGPU_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HBX_OK 0
#define HBX_ERR_ARG (-1)
#define HBX_ERR_HIP (-2)
#define HBX_ERR_CAPACITY (-3)
#define HBX_ERR_IO (-4)
#define HBX_ERR_NODEV (-5)
#define HBX_ERR_STATE (-6)

#define HBX_MIN_BLOCK_SIZE 65536u   /* hashback/hashback.go:38 */
#define HBX_MAX_BLOCK_SIZE 8388608u /* hashback/hashback.go:37 */
#define HBX_CONTENT_FILE_DATA 2     /* ContentTypeFileData,  store.go:193 */
#define HBX_CONTENT_FILE_CHAIN 3    /* ContentTypeFileChain, store.go:189 */
/* Device arenas must be readable this many bytes past the end of every file
 * (loads are 16-byte granular and bounds-checked, never fault, but the last
 * granule of a file may straddle its end). */
#define HBX_ARENA_SLACK 64u
#define HBX_ARENA_ALIGN 16u

typedef struct hbx_ctx hbx_ctx;

/* Per-file result beside the chunk list (store.go:187-196). */
typedef struct {
  uint8_t content_id[16]; /* entry.ContentBlockID */
  int32_t content_type;   /* 2 = FileData (1 chunk), 3 = FileChain, 0 = empty */
  uint32_t n_chunks;
} hbx_file_summary;

int hbx_version(void);
int hbx_device_count(int *n);
uint64_t hbx_max_chunks(uint64_t len);

int hbx_ctx_create(int device, hbx_ctx **out);
void hbx_ctx_destroy(hbx_ctx *ctx);
const char *hbx_last_error(const hbx_ctx *ctx);

/* One file in host memory (the storeFile drop-in).  ids must hold 16*cap
 * bytes; *n_chunks receives the chunk count. */
int hbx_chunk_hash(hbx_ctx *ctx, const uint8_t *data, uint64_t len, uint64_t *cut_ends,
                   uint8_t *ids, uint64_t cap, uint64_t *n_chunks);

/* Many files in host memory.  File f's chunks go to cut_ends[out_base[f] ..]
 * and ids[16*out_base[f] ..], at most caps[f] of them; summaries[f] gets the
 * count and the file content id. */
int hbx_chunk_hash_batch(hbx_ctx *ctx, uint64_t n_files, const uint8_t *const *datas,
                         const uint64_t *lens, uint64_t *cut_ends, uint8_t *ids,
                         const uint64_t *out_base, const uint64_t *caps,
                         hbx_file_summary *summaries);

/* Files already in device memory: file f is d_arena[file_offs[f] ..
 * +file_lens[f]).  file_offs must be multiples of HBX_ARENA_ALIGN and each
 * file must be followed by HBX_ARENA_SLACK readable bytes. */
int hbx_chunk_hash_device(hbx_ctx *ctx, const void *d_arena, uint64_t n_files,
                          const uint64_t *file_offs, const uint64_t *file_lens,
                          uint64_t *cut_ends, uint8_t *ids, const uint64_t *out_base,
                          const uint64_t *caps, hbx_file_summary *summaries);

/* Asynchronous device form: enqueue on the context's stream and return at
 * once.  Batches pipeline: the block-MD5 stage is time-sliced
 * (hbx_set_md5_slice), so the chunks of a new batch join the chains of the
 * batches still in flight instead of waiting behind their longest chunk.
 * hbx_wait completes the OLDEST pending batch and fills the output arrays
 * given at its submit (it first drains every chain in flight if that batch's
 * chains are not yet guaranteed hashed).  The synchronous calls
 * (hbx_chunk_hash*, hbx_store_paths) fail with HBX_ERR_STATE while batches
 * are pending. */
int hbx_submit_device(hbx_ctx *ctx, const void *d_arena, uint64_t n_files,
                      const uint64_t *file_offs, const uint64_t *file_lens, uint64_t *cut_ends,
                      uint8_t *ids, const uint64_t *out_base, const uint64_t *caps,
                      hbx_file_summary *summaries);
int hbx_wait(hbx_ctx *ctx);
/* Number of submitted batches not yet completed by hbx_wait. */
int hbx_pending(hbx_ctx *ctx);
/* Time slice of the block-MD5 stage: full 64-byte MD5 blocks each chain in
 * flight advances per launch (default 16384 = 1 MiB; 0 = unlimited, one
 * launch per batch); a chain takes the part short of a whole slice in its
 * first launch and whole slices after.  A submitted batch is complete after join lag (below)
 * + ceil(min(longest file, 8 MiB)/64 / blocks) - 1 further launches; results are
 * identical for every setting.  Fails with HBX_ERR_STATE while batches are
 * pending (their launch counts were fixed at submit). */
int hbx_set_md5_slice(hbx_ctx *ctx, uint32_t blocks);
/* Reuse the input memory of the OLDEST pending batch: order the engine's
 * next input copies (hbx_memcpy_h2d_async) and submitted batches (chunking
 * and verify) after the MD5 launch that finishes that batch, with a GPU-side
 * wait, so they touch the memory only once the batch's last chain is hashed —
 * before the batch is collected with hbx_wait, and without blocking the
 * host.  A ring of device arenas then needs no slot for results still on
 * their way to the host.  If that batch's last launch has not been issued
 * yet, the chains in flight are drained first (correct, only slower).
 * The wait is enqueued lazily, just before the next engine-issued copy or
 * submit (it then sits after the next MD5 plan, off the scan loop), so ONLY
 * engine-issued work is ordered by this call.  A caller that writes the
 * memory itself (its own stream, kernel or copy) calls hbx_input_fence
 * first. */
int hbx_input_after_oldest(hbx_ctx *ctx);
/* Enqueue the wait of the latest hbx_input_after_oldest now: on the engine's
 * scan stream and, if `stream` (a hipStream_t) is not NULL, on that stream
 * too, so the caller's own writes into the old batch's memory are ordered
 * after the MD5 launch that finishes it.  Nothing is enqueued once the host
 * has seen that launch complete.  Never blocks the host. */
int hbx_input_fence(hbx_ctx *ctx, void *stream);
/* Optional: pre-size the pipeline for `batches` batches in flight of up to
 * `files` files and `bytes` bytes each.  The batch pool, the MD5 chain tables
 * and the slice summaries are allocated now, so the steady state never
 * allocates (growing a buffer the streams share drains both streams).  Fails
 * with HBX_ERR_STATE while batches are pending. */
int hbx_reserve(hbx_ctx *ctx, uint32_t batches, uint64_t files, uint64_t bytes);

/* Files on disk, end to end (storeFile over a list of paths, store.go:84-199
 * with the tree walk left to the caller): io_threads read batches of up to
 * batch_bytes straight into two pinned slots; each batch is copied into a
 * ring of device arenas and pipelined like hbx_submit_device, so reading
 * batch b+1 overlaps the copy of batch b and the hashing of every batch
 * still in flight.  lens[i] must be the file sizes (stat); a file that cannot be
 * read in full fails the call with HBX_ERR_IO.  Outputs as
 * hbx_chunk_hash_batch. */
int hbx_store_paths(hbx_ctx *ctx, uint64_t n_files, const char *const *paths,
                    const uint64_t *lens, uint64_t *cut_ends, uint8_t *ids,
                    const uint64_t *out_base, const uint64_t *caps, hbx_file_summary *summaries,
                    uint32_t io_threads, uint64_t batch_bytes);

/* ---- Files larger than a batch: segments ------------------------------------
 * storeFile (hashback/store.go:84-199) reads a file of any size through an
 * 8 MiB window; the calls above need a whole file resident in one arena.
 * These stream one file through the pipeline as a sequence of SEGMENTS that
 * overlap by HBX_SEG_OVERLAP bytes.  store.go:111-166 decides each cut from
 * file[s : s + min(MAX, N - s)] alone, so a segment's cut chain is exact for
 * every chunk start s with s + MAX <= the segment's length (or up to the end
 * of the file in the final segment); it stops at the first start beyond that,
 * which lies strictly inside the overlap, and the next segment resumes there.
 * That resume point (the file's CARRY, an absolute offset) goes from one
 * segment's cut kernel to the next in device memory, so the segments of a
 * file pipeline like independent batches: no host round trip, no drain, and
 * hbx_wait stays FIFO.  The overlap is scanned twice (K1); no byte is hashed
 * twice.  Results are those of the whole file in one piece. */
#define HBX_SEG_OVERLAP HBX_MAX_BLOCK_SIZE          /* segment j+1 starts this far before segment j's end */
#define HBX_SEG_MIN_BYTES (2u * HBX_MAX_BLOCK_SIZE) /* smallest non-final segment: the carried start is <=
                                                       OVERLAP into it, so at least one chunk completes */
typedef struct hbx_seg hbx_seg;

/* The next segment of a file of file_len bytes cut into segments of seg_bytes
 * (>= HBX_SEG_MIN_BYTES, a multiple of HBX_ARENA_ALIGN): *off = 0 for the
 * first (prev_end == 0), else prev_end - HBX_SEG_OVERLAP, where prev_end is
 * the previous segment's end (off + len); *len = min(seg_bytes, file_len -
 * off).  The segment with off + len == file_len is the final one.
 * HBX_ERR_ARG for a bad seg_bytes, or if prev_end > 0 and nothing is left.
 * Pure host arithmetic, no context. */
int hbx_seg_next(uint64_t file_len, uint64_t seg_bytes, uint64_t prev_end, uint64_t *off, uint64_t *len);
/* Open a file of file_len bytes for segmented submission.  The handle owns
 * the file's carry word (device memory) and the chunk IDs collected so far
 * (host memory, 16 bytes per chunk: the final FileChainBlock's links). */
int hbx_seg_open(hbx_ctx *ctx, uint64_t file_len, hbx_seg **out);
/* Close a handle: HBX_ERR_STATE while one of its segments is pending.
 * Closing before the final segment was submitted abandons the file. */
int hbx_seg_close(hbx_ctx *ctx, hbx_seg *seg);
/* Enqueue one batch of n >= 1 segments, segment i being the next one of the
 * open file segs[i] (distinct files) at d_arena[arena_offs[i] .. +seg_lens[i]):
 * otherwise as hbx_submit_device, completed by hbx_wait in FIFO order with
 * every other batch.  Each segment must be what hbx_seg_next gives for its
 * file (the handle tracks the previous end, so the offset is implied and only
 * the length is passed): a non-final segment shorter than HBX_SEG_MIN_BYTES
 * or not a multiple of HBX_ARENA_ALIGN, or one longer than the rest of the
 * file, is HBX_ERR_ARG; a segment after the final one is HBX_ERR_STATE;
 * caps[i] < hbx_max_chunks(seg_lens[i]) is HBX_ERR_CAPACITY; all before
 * anything is enqueued.  At completion cut_ends are ABSOLUTE file offsets,
 * summaries[i].n_chunks is the number of chunks this segment completed (a
 * segment's first chunk starts at the previous segment's last cut end), and
 * content_type is 0 for a non-final segment.  The final segment's summary
 * carries the whole file's content_type and content_id (store.go:187-196):
 * type 2 and the chunk's ID with one chunk in total, else type 3 and the ID
 * of the FileChainBlock over all the file's chunk IDs, hashed on the device
 * by that hbx_wait without draining the other batches (a file with more
 * chunks than one block's BE32 length framing holds fails that wait with
 * HBX_ERR_CAPACITY).  The "file too large" limits apply per segment. */
int hbx_seg_submit_device(hbx_ctx *ctx, uint64_t n, hbx_seg *const *segs, const void *d_arena,
                          const uint64_t *arena_offs, const uint64_t *seg_lens, uint64_t *cut_ends,
                          uint8_t *ids, const uint64_t *out_base, const uint64_t *caps,
                          hbx_file_summary *summaries);
/* storeFile(path) for a file of any size: io_threads read each segment's
 * byte range in parallel (ranged pread) into two pinned slots; each segment is
 * copied into a ring of device arenas and submitted as above, so reading
 * segment j+1 never waits for segment j's cuts.  file_len must be the file's
 * size (stat); a short read fails the call with HBX_ERR_IO.  cut_ends / ids
 * (cap entries; HBX_ERR_CAPACITY with summary->n_chunks set if the file has
 * more chunks) and *summary receive the whole file's results, as
 * hbx_chunk_hash_batch gives them for a file in memory.
 * Memory bound: with S = min(seg_bytes, file_len) + 64 KiB, pinned host
 * memory is 2 S and device memory is D S for the arena ring plus the
 * pipeline's per-batch buffers for D + 2 batches of S bytes, D being the ring
 * depth hbx_store_paths uses (2..64, from the MD5 slice, join lag and K3
 * period: 10 at the defaults).  None of it depends on file_len.  What grows
 * with the file is 24 bytes of pageable host memory per chunk (its ID and cut
 * end), and 48 bytes per chunk of host and device memory for the final
 * FileChainBlock message while its ID is hashed (about 11 MB per TiB).
 * Synchronous; refused (HBX_ERR_STATE) while batches are pending. */
int hbx_store_file_seg(hbx_ctx *ctx, const char *path, uint64_t file_len, uint64_t seg_bytes,
                       uint32_t io_threads, uint64_t *cut_ends, uint8_t *ids, uint64_t cap,
                       hbx_file_summary *summary);

/* Host seconds hbx_store_paths spent, cumulative per context: [0] reading
 * files into pinned memory, [1] waiting for batches to be collected (a device
 * arena's reuse, and the drain at the end of the call), [2] waiting for a
 * pinned slot's H2D copy.  reset != 0 zeroes them. */
int hbx_io_times(hbx_ctx *ctx, double s[3], int reset);
/* Host time of the slowest single call since the last reset, ms: [0] one H2D
 * copy call (hbx_memcpy_h2d_async and the disk path's copies), [1] one batch
 * submit (hbx_submit_device and the disk path's submits).  reset != 0 zeroes
 * them after reading.  No reference counterpart: diagnostics (the copy call
 * once held the host ~7 ms while the runtime created an SDMA engine's queue,
 * DESIGN.md §8). */
int hbx_host_call_max(hbx_ctx *ctx, double ms[2], int reset);

/* MD5(data) on the device: core.Hash (pkg/core/core.go:46-48), the primitive
 * under core.Hmac / DeepHmac (core.go:51-80). */
int hbx_md5(hbx_ctx *ctx, const uint8_t *data, uint64_t len, uint8_t out[16]);

/* MD5(BE32(n_links) || links || BE32(len) || data) on the device. */
int hbx_block_id(hbx_ctx *ctx, const uint8_t *links, uint32_t n_links, const uint8_t *data,
                 uint64_t len, uint8_t out[16]);

/* Batched HashboxBlock.HashData / VerifyBlock (pkg/core/block.go:96-111,
 * 152-174) for uncompressed blocks (BlockDataTypeRaw, or data already
 * inflated).  Block i's ID is MD5(BE32(n_links[i]) || links || BE32(lens[i])
 * || data), its links being the n_links[i] 16-byte IDs at
 * links[16*link_base[i] ..] (host memory; links, link_base and n_links may
 * be NULL when no block has links).  ids (16*n bytes, may be NULL) receives
 * the IDs.  With expect != NULL (16*n bytes), ok[i] (may be NULL) = 1 where
 * the ID equals expect[16*i ..], 0 elsewhere, and *n_bad (may be NULL)
 * counts the mismatches.  Callers in the reference: restore
 * (hashback/restore.go:52, 256), the server's write check
 * (server/server.go:182), verify -content (pkg/storagedb/integrity.go:117,
 * 282), show-block (util/commands.go:212).  Refused (HBX_ERR_STATE) while
 * batches are pending. */
int hbx_verify_blocks(hbx_ctx *ctx, uint64_t n, const uint8_t *const *datas, const uint64_t *lens,
                      const uint8_t *links, const uint64_t *link_base, const uint32_t *n_links,
                      uint8_t *ids, const uint8_t *expect, uint8_t *ok, uint64_t *n_bad);
/* The same for blocks in device memory: block i is d_arena[offs[i] ..
 * +lens[i]), followed by HBX_ARENA_SLACK readable bytes. */
int hbx_verify_blocks_device(hbx_ctx *ctx, const void *d_arena, uint64_t n, const uint64_t *offs,
                             const uint64_t *lens, const uint8_t *links, const uint64_t *link_base,
                             const uint32_t *n_links, uint8_t *ids, const uint8_t *expect,
                             uint8_t *ok, uint64_t *n_bad);

/* ---- Per-file and per-directory block formats ------------
 * hashback/hashback.go:80-214.  FileEntry is one directory entry; its
 * ContentBlockID is a chunk id (type 2), a FileChainBlock id (type 3, see
 * hbx_file_summary) or a DirectoryBlock id (type 1).  Strings are raw bytes
 * (core.String, pkg/core/core.go:95-109); integers big-endian
 * (pkg/core/utils.go:73-88); file_mode is Go's os.FileMode bit layout and
 * mod_time is UnixNano (store.go:243-251).  These functions are pure host
 * code and need no context. */
#define HBX_CONTENT_EMPTY 0     /* ContentTypeEmpty,     hashback.go:94 */
#define HBX_CONTENT_DIRECTORY 1 /* ContentTypeDirectory, hashback.go:95 */
#define HBX_CONTENT_SYMLINK 4   /* ContentTypeSymLink,   hashback.go:98 */
#define HBX_ERR_FORMAT (-7)     /* corrupted or truncated serialized block */

typedef struct {
  const char *name; /* FileName (not NUL-terminated) */
  uint32_t name_len;
  uint32_t file_mode;  /* FileMode */
  int64_t file_size;   /* FileSize */
  int64_t mod_time;    /* ModTime */
  uint8_t reference_id[16];
  uint8_t content_id[16];  /* written for types 1, 2, 3 */
  uint8_t decrypt_key[16]; /* written for type 2 */
  const char *link;        /* FileLink, written for type 4 */
  uint32_t link_len;
  uint8_t content_type; /* 0 empty, 1 dir, 2 file data, 3 file chain, 4 symlink */
  uint8_t pad[3];
} hbx_file_entry;

/* Serialized size of FileEntry.Serialize (hashback.go:113-132). */
uint64_t hbx_file_entry_size(const hbx_file_entry *e);
/* FileEntry.Serialize into out[0..cap); *n = bytes written.
 * HBX_ERR_CAPACITY if cap is too small (nothing useful written). */
int hbx_file_entry_serialize(const hbx_file_entry *e, uint8_t *out, uint64_t cap, uint64_t *n);
/* FileEntry.Unserialize (hashback.go:133-155) of in[0..len); *used = bytes
 * consumed.  name/link point into `in`.  HBX_ERR_FORMAT for a wrong magic
 * ("corrupted FileEntry") or a short buffer. */
int hbx_file_entry_parse(const uint8_t *in, uint64_t len, hbx_file_entry *e, uint64_t *used);

/* FileChainBlock.Serialize (hashback.go:162-170): "fchn", k, then k pairs
 * (id, decrypt key); keys may be NULL (all zero, as store.go:175-184 writes
 * them).  Size is 8 + 32k.  This is the block whose HashData with links =
 * ids is hbx_file_summary.content_id for type 3. */
int hbx_chain_block_serialize(const uint8_t *ids, const uint8_t *keys, uint32_t k, uint8_t *out,
                              uint64_t cap, uint64_t *n);
/* FileChainBlock.Unserialize (hashback.go:171-185): *k = chain length; ids
 * and keys (each 16*cap bytes, may be NULL) receive up to cap entries
 * (HBX_ERR_CAPACITY if *k > cap). */
int hbx_chain_block_parse(const uint8_t *in, uint64_t len, uint32_t *k, uint8_t *ids, uint8_t *keys,
                          uint32_t cap);

/* DirectoryBlock.Serialize (hashback.go:192-199) of n entries in the order
 * given (storeDir sorts by name, store.go:217).  links (16*n bytes, may be
 * NULL) receives storeDir's link list: the content_id of every entry of type
 * 1, 2 or 3, in order (store.go:221-228); *n_links its length.  Size:
 * hbx_directory_block_size. */
uint64_t hbx_directory_block_size(const hbx_file_entry *entries, uint32_t n);
int hbx_directory_block_serialize(const hbx_file_entry *entries, uint32_t n, uint8_t *out,
                                  uint64_t cap, uint64_t *n_out, uint8_t *links, uint32_t *n_links);
/* DirectoryBlock.Unserialize (hashback.go:200-214): *n = entry count;
 * entries[0..min(n, cap)) are filled (names/links point into `in`). */
int hbx_directory_block_parse(const uint8_t *in, uint64_t len, hbx_file_entry *entries, uint32_t cap,
                              uint32_t *n);

/* The IDs of many DirectoryBlocks at once, on the device: directory d holds
 * entries[entry_base[d] .. + n_entries[d]); ids[16*d ..] receives
 * NewHashboxBlock(dblk bytes, links).BlockID (store.go:230-231).  A tree's
 * directories are hashed level by level, deepest first, since a parent's
 * entry carries its child directory's id.  Refused (HBX_ERR_STATE) while
 * batches are pending. */
int hbx_directory_block_ids(hbx_ctx *ctx, uint32_t n_dirs, const hbx_file_entry *entries,
                            const uint64_t *entry_base, const uint32_t *n_entries, uint8_t *ids);

/* ---- zlib block compression ---------------------------------
 * HashboxBlock.CompressData for BlockDataTypeZlib (pkg/core/block.go:133-150,
 * 176-184; done by the client's workers before sending, client.go:249-258):
 * each block's data becomes one zlib stream (RFC 1950: 78 9C header, deflate
 * blocks, Adler-32).  Not byte-identical to Go's compress/zlib (the server
 * inflates and re-hashes, block.go:159-166; DataType is not hashed,
 * block.go:101) but every stream inflates to the block's data.  Each 32 KiB
 * segment is coded independently on the device (LZ77 within the segment +
 * fixed Huffman, or stored when that is not smaller), so any output is at
 * most hbx_deflate_bound(len) bytes. */
uint64_t hbx_deflate_bound(uint64_t len);
/* Blocks in device memory: block i = d_arena[offs[i] .. +lens[i]) (followed
 * by HBX_ARENA_SLACK readable bytes); its stream goes to d_out[out_offs[i] ..]
 * (out_caps[i] >= hbx_deflate_bound(lens[i]), else HBX_ERR_CAPACITY), its
 * length to out_lens[i] (host).  Synchronous.  Refused (HBX_ERR_STATE) while
 * batches are pending. */
int hbx_deflate_blocks_device(hbx_ctx *ctx, const void *d_arena, uint64_t n, const uint64_t *offs,
                              const uint64_t *lens, void *d_out, const uint64_t *out_offs,
                              const uint64_t *out_caps, uint64_t *out_lens);
/* The same for host blocks: datas[i] (lens[i] bytes) -> outs[i] (caps[i]
 * bytes), out_lens[i] = stream length. */
int hbx_deflate_blocks(hbx_ctx *ctx, uint64_t n, const uint8_t *const *datas, const uint64_t *lens,
                       uint8_t *const *outs, const uint64_t *caps, uint64_t *out_lens);

/* hbx_store_paths plus CompressData of every chunk on the device (the
 * client's send path: StoreData -> workers compress -> socket,
 * client.go:249-258).  sums is required.  Chunk i of file f (index
 * out_base[f] + i, like cut_ends) gets its zlib stream at zout[zoff[..]] with
 * length zlen[..]; file f's streams are packed from zout[zbase[f]], which
 * needs hbx_deflate_file_bound(lens[f]) bytes.
 * Device memory: each compression stage (two in flight) holds, besides its
 * output, 96 KiB of scratch per 32 KiB segment of the batch, about 3x the
 * batch's bytes (hbx_deflate.hip kSlot: the parse hand-off and the coded
 * image of every segment); hbx_deflate_blocks* hold the same per call.  Size
 * batch_bytes with that in mind. */
uint64_t hbx_deflate_file_bound(uint64_t len);
int hbx_store_paths_z(hbx_ctx *ctx, uint64_t n_files, const char *const *paths, const uint64_t *lens,
                      uint64_t *cut_ends, uint8_t *ids, const uint64_t *out_base, const uint64_t *caps,
                      hbx_file_summary *summaries, uint32_t io_threads, uint64_t batch_bytes,
                      uint8_t *zout, const uint64_t *zbase, uint64_t *zoff, uint64_t *zlen);

/* ---- wire protocol framing -----------------------------------
 * pkg/core/protocol.go: a message is u16 Num | u32 Type | its fields, big
 * endian (ProtocolMessage.Serialize, protocol.go:184-203).  Client types are
 * the lowercase constants; the server replies with Type & 0xDFDFDFDF
 * ("READ", "ACKN", "WRIT", "ERRS").  The StoreBlock exchange
 * (client.go:563-584, server.go:160-202): allo(id) -> READ(id) -> writ(block)
 * -> ACKN(id), or allo(id) -> ACKN(id) when the server has the block.  The
 * encoders cover that exchange; the parser frames every message type
 * protocol.go:204-264 knows.  Pure host code, no context. */
#define HBX_MSG_OLD_GREETING 0x686F6C61u /* "hola" */
#define HBX_MSG_GREETING 0x68616C6Fu    /* "halo" */
#define HBX_MSG_AUTHENTICATE 0x61757468u /* "auth" */
#define HBX_MSG_GOODBYE 0x71756974u     /* "quit" */
#define HBX_MSG_ACCOUNT_INFO 0x696E666Fu /* "info" */
#define HBX_MSG_ADD_DATASET_STATE 0x61646473u /* "adds" */
#define HBX_MSG_LIST_DATASET 0x6C697374u /* "list" */
#define HBX_MSG_REMOVE_DATASET_STATE 0x64656C73u /* "dels" */
#define HBX_MSG_ALLOCATE 0x616C6C6Fu    /* "allo" */
#define HBX_MSG_READ 0x72656164u        /* "read" */
#define HBX_MSG_WRITE 0x77726974u       /* "writ" */
#define HBX_MSG_ACKNOWLEDGE 0x61636B6Eu /* "ackn" */
#define HBX_MSG_ERROR 0x65727273u       /* "errs" (sent as "ERRS") */
#define HBX_SERVER_MASK 0xDFDFDFDFu
#define HBX_BLOCK_DATA_RAW 0xFFu  /* BlockDataTypeRaw,  block.go:21 */
#define HBX_BLOCK_DATA_ZLIB 0x01u /* BlockDataTypeZlib, block.go:22 */

typedef struct {
  uint16_t num;
  uint32_t type;
  uint8_t id[16];         /* allo/ACKN/read/READ/writ/WRIT: BlockID; HALO: nonce */
  uint32_t n_links;       /* writ/WRIT */
  const uint8_t *links;   /* writ/WRIT: into the input */
  uint8_t data_type;      /* writ/WRIT */
  uint32_t data_len;      /* writ/WRIT data; ERRS text; halo: version; others: payload bytes */
  const uint8_t *data;    /* writ/WRIT data, ERRS text, other payloads (after the 6-byte header): into the input */
  uint64_t header_len;    /* bytes before the data */
  uint64_t total_len;     /* bytes of the whole message */
} hbx_wire_msg;

/* allo / read (client) or ACKN / READ (server, pass type & HBX_SERVER_MASK):
 * 22 bytes. */
int hbx_wire_encode_id(uint16_t num, uint32_t type, const uint8_t id[16], uint8_t out[22]);
/* writ / WRIT up to (not including) the data: 31 + 16*n_links bytes; the
 * data_len bytes of block data follow on the wire as they are (for
 * BlockDataTypeZlib: the zlib stream, block.go:56-69). */
int hbx_wire_encode_block_header(uint16_t num, uint32_t type, const uint8_t id[16], const uint8_t *links,
                                 uint32_t n_links, uint8_t data_type, uint32_t data_len, uint8_t *out,
                                 uint64_t cap, uint64_t *n);
/* Parse one message at in[0..len) (ProtocolMessage.Unserialize,
 * protocol.go:204-264): HBX_OK, HBX_ERR_CAPACITY if the message is not
 * complete yet (msg->total_len is set once its header is), HBX_ERR_FORMAT for
 * an unknown type. */
int hbx_wire_parse(const uint8_t *in, uint64_t len, hbx_wire_msg *msg);

/* Pipelined VerifyBlock: the same inputs and outputs as
 * hbx_verify_blocks_device, enqueued like hbx_submit_device and completed by
 * hbx_wait in FIFO order with the chunking batches.  Each block's link prefix
 * is hashed first; the rest of its message joins the time-sliced MD5 chains
 * (hbx_set_md5_slice), so a bulk verification streams like the chunking path
 * instead of waiting on one launch's longest block.  ids, expect, ok and
 * n_bad must stay valid until the hbx_wait that completes the batch; links
 * are copied at submit. */
int hbx_verify_submit_device(hbx_ctx *ctx, const void *d_arena, uint64_t n, const uint64_t *offs,
                             const uint64_t *lens, const uint8_t *links, const uint64_t *link_base,
                             const uint32_t *n_links, uint8_t *ids, const uint8_t *expect,
                             uint8_t *ok, uint64_t *n_bad);

/* HashboxBlock.UncompressData for zlib blocks (pkg/core/block.go:113-131,
 * 186-201), many streams at once on the device: stream i =
 * d_in[in_offs[i] .. +in_lens[i]) inflates into d_out[out_offs[i] ..] (at most
 * out_caps[i] bytes); out_lens[i] (host) = inflated bytes, status[i] (host) =
 * 0, or 1 bad header / Adler-32, 2 truncated input, 3 output capacity,
 * 4 invalid code, 5 distance too far back, 6 bad stored length.  Any RFC
 * 1950 stream (Go's compress/zlib, K7's).  Status 4 covers what zlib and
 * Go's flate refuse in a block's codes: block type 3, more than 286
 * literal/length or 30 distance lengths, a repeat with nothing to repeat or
 * past the last length, no code for end-of-block, an over-subscribed code,
 * a symbol without a code, and an incomplete code: the code-length code must
 * be complete, a literal/length or distance code too unless it is a single
 * code of length 1, or a distance code of no codes at all (literals only).
 * A corrupt stream only sets its status; out_lens[i] is then what was
 * written before it was found, and no byte past it changes.  Then hbx_verify_blocks_device / hbx_verify_submit_device on the
 * output is VerifyBlock of compressed blocks (block.go:152-166).  This call
 * needs each stream's inflated size in advance; a block read back from a
 * server carries its compressed length only (Unserialize, block.go:82-94):
 * hbx_restore_blocks / hbx_restore_file_stream below inflate, verify and
 * assemble such blocks without it.
 * Synchronous; refused (HBX_ERR_STATE) while batches are pending. */
int hbx_inflate_blocks_device(hbx_ctx *ctx, const void *d_in, uint64_t n, const uint64_t *in_offs,
                              const uint64_t *in_lens, void *d_out, const uint64_t *out_offs,
                              const uint64_t *out_caps, uint64_t *out_lens, uint32_t *status);

/* hbx_store_paths_z with a callback per collected batch: ready(user, first,
 * count) runs as soon as files [first, first+count) have their cut_ends, ids,
 * summaries and zlib streams written, so a sender can put those blocks on the
 * wire while later batches are still read and hashed.  The calls come from
 * an engine worker thread (the one that unpacked the batch's compressed
 * streams), one at a time and in file order, all before this function
 * returns.  It must return quickly and must not call into the same context. */
typedef void (*hbx_batch_ready_fn)(void *user, uint64_t first_file, uint64_t n_files);
int hbx_store_paths_zcb(hbx_ctx *ctx, uint64_t n_files, const char *const *paths, const uint64_t *lens,
                        uint64_t *cut_ends, uint8_t *ids, const uint64_t *out_base, const uint64_t *caps,
                        hbx_file_summary *summaries, uint32_t io_threads, uint64_t batch_bytes,
                        uint8_t *zout, const uint64_t *zbase, uint64_t *zoff, uint64_t *zlen,
                        hbx_batch_ready_fn ready, void *user);

/* hbx_store_paths* with per-file outcomes (replaces the error handling of
 * storeFile/storePath/storeDir, hashback/store.go:85-94, 101-103, 221-224,
 * 356-359).  status (n_files int32, required) receives 0 for a file stored, or
 * the errno of a file the reference skips without stopping the tree walk:
 *   - open() failed (os.Open, store.go:101-103: storeDir logs "Skipping
 *     (ERROR)" and goes on with the next entry, :221-224);
 *   - a read failed with EBADF (minorPathError, hashback_unix.go:57-63:
 *     storePath keeps the previous backup's entry, store.go:356-359).
 * Such a file gets no chunks (summary n_chunks 0, content type 0); every other
 * file of its batch is stored as usual.  Any other read failure (an I/O error,
 * a file shorter than lens[i]) is what storeFile panics on (CopyNOrPanic,
 * pkg/core/utils.go:95-99): the call fails with HBX_ERR_IO and the path in
 * hbx_last_error, as hbx_store_paths does for every failure.  zout, zbase,
 * zoff, zlen all NULL: no compression (hbx_store_paths); else as
 * hbx_store_paths_zcb (ready may be NULL: hbx_store_paths_z). */
int hbx_store_paths_status(hbx_ctx *ctx, uint64_t n_files, const char *const *paths, const uint64_t *lens,
                           uint64_t *cut_ends, uint8_t *ids, const uint64_t *out_base, const uint64_t *caps,
                           hbx_file_summary *summaries, int32_t *status, uint32_t io_threads,
                           uint64_t batch_bytes, uint8_t *zout, const uint64_t *zbase, uint64_t *zoff,
                           uint64_t *zlen, hbx_batch_ready_fn ready, void *user);

/* ---- Block-ID set: skip the chunks already seen (K9) ------------------------
 * The reference compresses and sends a block only once it is known to be new:
 * StoreBlock drops an ID already in its queue map (pkg/core/client.go:571-576),
 * the server answers allo with ACKN for a block it holds (server/server.go:
 * 160-168), and a worker calls CompressData only for the blocks the server
 * asked for with READ (client.go:211-214, 249-258).  hbx_idset is that
 * knowledge as a set of 16-byte IDs in device memory, which the pipeline
 * consults in submit order: exactly one chunk per distinct ID is FRESH, the
 * first in submit order (file order, then chunk order, within a batch), however
 * the files fall into batches.  A caller seeds it with what the server is known
 * to hold (a previous backup's ID list).
 * Layout of a set of capacity C: the IDs in insertion order, and a table of
 * S = hbx_idset_slots(C) slots, the smallest power of two >= 2 C and at least
 * 64.  An ID's home slot is LE64(id[0..8]) & (S - 1) (its first 8 bytes as a
 * little-endian integer), with linear probing that wraps around.
 * A full set never reports an ID it could not insert as seen: such an ID is
 * counted in `dropped`, is fresh, and is fresh again the next time.  A wrong
 * "seen" would lose data; a wrong "fresh" costs only work.
 * The direct calls below are synchronous and, like the other synchronous
 * calls, refused (HBX_ERR_STATE) while batches are pending; a set used with a
 * context other than its own is HBX_ERR_ARG. */
typedef struct hbx_idset hbx_idset;
/* S for a capacity; 0 if the capacity is above 2^31.  Pure host arithmetic. */
uint64_t hbx_idset_slots(uint64_t capacity);
/* A set for up to `capacity` IDs (1..2^31): 16 bytes per ID + 4 per slot of
 * device memory. */
int hbx_idset_create(hbx_ctx *ctx, uint64_t capacity, hbx_idset **out);
/* HBX_ERR_STATE while pending batches still use the set. */
int hbx_idset_destroy(hbx_ctx *ctx, hbx_idset *set);
/* Test-and-insert n IDs (16 n bytes, host memory) in order: fresh[i] = 1
 * exactly for the first occurrence of an ID the set did not hold, else 0.
 * fresh may be NULL (bulk seeding). */
int hbx_idset_insert(hbx_ctx *ctx, hbx_idset *set, uint64_t n, const uint8_t *ids, uint8_t *fresh);
/* Read only: found[i] = 1 iff ids[16 i ..] is in the set. */
int hbx_idset_contains(hbx_ctx *ctx, hbx_idset *set, uint64_t n, const uint8_t *ids, uint8_t *found);
/* Any of the outputs may be NULL.  dropped: IDs not inserted because the set
 * was full, over the set's lifetime. */
int hbx_idset_stats(hbx_ctx *ctx, hbx_idset *set, uint64_t *count, uint64_t *capacity, uint64_t *slots,
                    uint64_t *dropped);
/* The set's IDs in insertion order into ids (16 cap bytes); *n = count
 * (HBX_ERR_CAPACITY if count > cap).  Across calls and across pipeline batches
 * the order is call / submit order; within one call or batch it is unspecified. */
int hbx_idset_export(hbx_ctx *ctx, hbx_idset *set, uint8_t *ids, uint64_t cap, uint64_t *n);
/* Keep the first `count` IDs of that order and forget the rest: a caller
 * notes the count before a send and rolls back when the send fails.
 * count above the set's is HBX_ERR_ARG. */
int hbx_idset_truncate(hbx_ctx *ctx, hbx_idset *set, uint64_t count);

/* hbx_submit_device with a set (NULL: exactly hbx_submit_device).  With a set,
 * fresh is required and runs parallel to ids: at the hbx_wait that completes
 * the batch, fresh[k] = 1 where ids[16 k ..] is the first occurrence of an ID
 * the set did not hold, and that ID is in the set; it must stay valid until
 * then.  The mark runs on the device when the batch's last chain is hashed, in
 * submit order (a batch with a set completes no earlier than the older batches
 * with one).  Verify batches never touch a set; segment batches take one through
 * hbx_seg_submit_device_dd.  Rolling back after a failed send is the caller's
 * job (hbx_idset_truncate). */
int hbx_submit_device_dd(hbx_ctx *ctx, const void *d_arena, uint64_t n_files, const uint64_t *file_offs,
                         const uint64_t *file_lens, uint64_t *cut_ends, uint8_t *ids, const uint64_t *out_base,
                         const uint64_t *caps, hbx_file_summary *summaries, hbx_idset *set, uint8_t *fresh);
/* hbx_store_paths_status with a set (NULL: exactly hbx_store_paths_status).
 * status may be NULL here: every read failure then fails the call, as in
 * hbx_store_paths.  fresh as above.  With compression, only fresh chunks are compressed, copied
 * back and placed: a chunk that is not fresh gets zlen = 0 (no real stream is
 * shorter than 11 bytes) and zoff = the running offset.  If the server answers
 * READ for such a chunk after all (a stale set: the server lost a block the
 * set was seeded with), compress it on demand with hbx_deflate_blocks.  With a
 * set, batch_bytes is honoured down to 1 MiB (without one it is raised to
 * 64 MiB).  If the call fails, the set is first truncated to the count it had
 * on entry: the caller saw none of those chunks. */
int hbx_store_paths_dd(hbx_ctx *ctx, uint64_t n_files, const char *const *paths, const uint64_t *lens,
                       uint64_t *cut_ends, uint8_t *ids, const uint64_t *out_base, const uint64_t *caps,
                       hbx_file_summary *summaries, int32_t *status, uint32_t io_threads, uint64_t batch_bytes,
                       uint8_t *zout, const uint64_t *zbase, uint64_t *zoff, uint64_t *zlen,
                       hbx_batch_ready_fn ready, void *user, hbx_idset *set, uint8_t *fresh);

/* ---- Segments with a set: one file of any size, deduplicated and compressed --
 * hbx_seg_submit_device with a set (NULL: exactly hbx_seg_submit_device).  With
 * a set, fresh is required, runs parallel to ids (fresh[out_base[i] + q] for
 * chunk q of segment i) and must stay valid until the hbx_wait that completes
 * the batch.  A chunk is marked in the segment that COMPLETES it.  Segment
 * batches and hbx_submit_device_dd batches share one submit order per context:
 * exactly one chunk per distinct ID is fresh, the first in submit order
 * (segment order within a batch, then chunk order), however segments and
 * ordinary batches interleave.  Closing a file before its final segment leaves
 * what its segments inserted in the set; rolling back is the caller's job
 * (hbx_idset_truncate).  A set of another context is HBX_ERR_ARG;
 * hbx_idset_destroy is refused while such a batch is pending. */
int hbx_seg_submit_device_dd(hbx_ctx *ctx, uint64_t n, hbx_seg *const *segs, const void *d_arena,
                             const uint64_t *arena_offs, const uint64_t *seg_lens, uint64_t *cut_ends,
                             uint8_t *ids, const uint64_t *out_base, const uint64_t *caps,
                             hbx_file_summary *summaries, hbx_idset *set, uint8_t *fresh);

#define HBX_ERR_SINK (-8)          /* the sink returned non-zero */
#define HBX_STREAM_COMPRESS 1u
/* What one segment of hbx_store_file_stream completed. */
typedef struct {
  uint64_t first_chunk;      /* index in the file of this segment's first chunk */
  uint64_t n_chunks;         /* chunks this segment completed */
  const uint64_t *cut_ends;  /* absolute file offsets */
  const uint8_t *ids;        /* 16 n_chunks bytes */
  const uint8_t *fresh;      /* NULL without a set */
  const uint8_t *z;          /* NULL without HBX_STREAM_COMPRESS: base of this segment's zlib streams */
  const uint64_t *zoff, *zlen; /* stream i = z[zoff[i] .. + zlen[i]); zlen 0 for a chunk that is not fresh */
  int final;                 /* 1 for the file's last segment */
  hbx_file_summary summary;  /* final: the whole file's content type, id and chunk count (else zero) */
} hbx_seg_chunks;
typedef int (*hbx_seg_sink_fn)(void *user, const hbx_seg_chunks *seg);
/* hbx_store_file_seg for a sender: storeFile(path) for a file of any size, with
 * the set consulted per segment (set may be NULL) and, with
 * HBX_STREAM_COMPRESS in flags, CompressData of every fresh chunk (of every
 * chunk without a set), each segment's finished chunks handed to `sink` as
 * soon as they are ready.
 * The sink runs once per segment, in segment order, one call at a time, on an
 * engine worker thread, and every call happens before this function returns.
 * It runs as soon as that segment's cut ends, IDs, flags and streams exist,
 * while later segments are still read, copied and hashed (a segment is
 * collected as soon as its results have reached the host, not only when its
 * arena is needed again).  Every pointer of *seg is valid only during the
 * call.  The streams are read in place from the engine's pinned compression
 * stage: nothing is copied into a caller buffer.  A stage is reused only after
 * its sink call has returned, so at most two segments wait for the sink while
 * the pipeline runs on.  The sink must not call into the same context.  An
 * empty file gives one call with n_chunks == 0 and final == 1.  sink may be
 * NULL without HBX_STREAM_COMPRESS (the set is filled and *summary written).
 * Failures: a non-zero return from the sink fails the call with HBX_ERR_SINK
 * (no later segment reaches the sink), a short read with HBX_ERR_IO, anything
 * else as hbx_store_file_seg.  In every failing case the pipeline is drained
 * (hbx_pending is 0 afterwards), a given set is first truncated to the count it
 * had on entry (chunks a sink already shipped are then fresh again, which costs
 * only work) and the context stays usable.  HBX_ERR_ARG for a NULL ctx or
 * path, a bad seg_bytes (as hbx_seg_next), unknown flags, HBX_STREAM_COMPRESS
 * without a sink (all before the context is touched) or a set of another
 * context; HBX_ERR_STATE while batches are pending.  *summary (may be NULL)
 * receives the file's summary.
 * Memory bound, none of it depending on file_len: with S = min(seg_bytes,
 * file_len) + 64 KiB, two pinned read slots of S; D ring arenas of S and the
 * pipeline's per-batch buffers for D + 2 batches of S bytes, D being the ring
 * depth hbx_store_paths uses (as hbx_store_file_seg); with
 * HBX_STREAM_COMPRESS the two compression stages sized for one segment (output
 * and pinned stage of about S each, plus 96 KiB of scratch per 32 KiB of S, as
 * hbx_store_paths_z documents); and 41 bytes of pageable host memory per
 * possible chunk (S / 64 KiB + 1) of each of the up to D + 3 segments between
 * submit and the end of their sink call.  What grows with the file is only the
 * handle's 16 bytes per chunk for the final FileChainBlock (and 48 bytes per
 * chunk while its ID is hashed); no cut end is kept.
 * Synchronous. */
int hbx_store_file_stream(hbx_ctx *ctx, const char *path, uint64_t file_len, uint64_t seg_bytes,
                          uint32_t io_threads, uint32_t flags, hbx_idset *set,
                          hbx_seg_sink_fn sink, void *user, hbx_file_summary *summary);

/* ---- Restore and diff: a file's block chain back into its bytes (K10) ---------
 * restoreFileData (hashback/restore.go:45-66) reads each block of a file's
 * chain, VerifyBlock()s it (restore.go:52-54; UncompressData + HashData,
 * block.go:113-131, 152-174) and appends its data to the file; diffFileData
 * (restore.go:249-277) compares each verified block with the local file at the
 * running offset instead.  These calls take the blocks as they come off the
 * wire (Unserialize, block.go:82-94: the data field, its DataType, and the
 * BlockID that was asked for; the inflated size is NOT known) and give the
 * file's bytes, or the first difference from a local copy.  The same path
 * serves the server's write check (server/server.go:182) and verify -content
 * (pkg/storagedb/integrity.go:117, 282) with directory and chain blocks: links
 * are passed through to the hash. */
#define HBX_BLOCK_RAW 0xff          /* BlockDataTypeRaw,  block.go:22-23 */
#define HBX_BLOCK_ZLIB 0x01         /* BlockDataTypeZlib */
#define HBX_MAX_BLOCK (8u << 20)    /* MAX_BLOCK_SIZE, hashback.go:37 */
#define HBX_ERR_VERIFY (-9)         /* hbx_restore_file_stream: a block of the chain is bad */
/* The largest data field accepted for a block whose data is at most max_block
 * bytes (0 = HBX_MAX_BLOCK): at least hbx_deflate_bound(max_block), so every
 * stream K7 or Go's compress/zlib writes for such a block fits.  Pure host
 * arithmetic. */
uint64_t hbx_restore_in_bound(uint64_t max_block);
/* n blocks of one chain, in file order, in host memory: block i's data field
 * is datas[i][0 .. lens[i]), of type types[i] (HBX_BLOCK_RAW: the data itself;
 * HBX_BLOCK_ZLIB: one zlib stream), and must hash to expect[16 i ..] with its
 * links (links / link_base / n_links as hbx_verify_blocks, all NULL when no
 * block has links).  max_block (0 = HBX_MAX_BLOCK) is the largest block data
 * accepted.  status[i] receives
 *   0      the block inflated and its ID matches (VerifyBlock true);
 *   1..6   exactly hbx_inflate_blocks_device's values; a stream (or a raw
 *          block) longer than max_block is 3;
 *   7      the ID does not match (VerifyBlock false);
 *   8      the data field is longer than hbx_restore_in_bound(max_block), or
 *          the type is neither raw nor zlib.
 * The reference stops at the first bad block (restore.go:52-54), so the
 * result is a PREFIX: *n_good = the number of leading blocks with status 0,
 * offs[0 .. *n_good] (offs holds n + 1) the file offset where each of them
 * starts (offs[i + 1] - offs[i] = block i's length) and, with out != NULL,
 * out[0 .. offs[*n_good]) the file's bytes.  Nothing past out[offs[*n_good]) is
 * written.  A corrupt block is a result, not an error: the call returns HBX_OK.
 * Diff mode (out NULL, local != NULL: the local copy's local_len bytes, host
 * memory): nothing is written; *first_diff = the smallest offset inside the
 * good prefix at which the two differ, comparing the bytes present on both
 * sides; else min(local_len, offs[*n_good]) if the lengths differ; else
 * UINT64_MAX.  (The caller compares file sizes first, restore.go:322, and
 * prints the 16-byte line.)
 * HBX_ERR_ARG: out and local both set or both NULL, out_cap smaller than the
 * good prefix, max_block above 1 GiB.  HBX_ERR_STATE while batches are
 * pending.  Device memory: a slot of max_block per zlib block, so long chains
 * run in windows of as many blocks as a quarter of the free device memory
 * holds.  Synchronous. */
int hbx_restore_blocks(hbx_ctx *ctx, uint64_t n, const uint8_t *const *datas, const uint64_t *lens,
                       const uint8_t *types, const uint8_t *expect, const uint8_t *links,
                       const uint64_t *link_base, const uint32_t *n_links, uint64_t max_block, uint8_t *out,
                       uint64_t out_cap, const uint8_t *local, uint64_t local_len, uint64_t *offs,
                       uint32_t *status, uint64_t *n_good, uint64_t *first_diff);
/* Block `index` of the chain into dst[0 .. cap) (pinned staging memory of the
 * engine): *len = its data field's length, *type = its DataType.  Non-zero =
 * failure.  A field longer than cap cannot be delivered: report its length
 * (the block then gets status 8) and write nothing. */
typedef int (*hbx_block_source_fn)(void *user, uint64_t index, uint8_t *dst, uint64_t cap, uint64_t *len,
                                   uint8_t *type);
/* The file's bytes [file_off, file_off + len), valid during the call. */
typedef int (*hbx_restore_sink_fn)(void *user, uint64_t file_off, const uint8_t *data, uint64_t len);
/* restoreFileData / diffFileData for a chain of any length (restore.go:45-66,
 * 249-277): block i has the ID ids[16 i ..] (the FileChainBlock's list, or
 * the one ContentBlockID of a single-block file) and is fetched with
 * source(user, i, ...).  Exactly one of out_path (the file is created or
 * truncated and written), sink (the bytes are handed over in file order) and
 * local_path (diff mode, as above, against that file; *first_diff required)
 * is set.  The chain runs in WINDOWS of as many blocks as fit window_bytes of
 * inflate slots (max_block + 256 each; 0 = 1 GiB; at least one block), two in
 * flight: the source fills window k + 1's pinned staging and its copy to the
 * device runs while window k inflates; window k's blocks are verified beside
 * their gather into a pinned buffer, whose good prefix is written (or sunk) by
 * a worker thread while window k + 1 inflates.  source runs on an engine
 * thread, one call at a time in index order; sink likewise, once per window
 * with contiguous ascending offsets; neither may call into the same context.
 * Memory depends on window_bytes and max_block only: with W blocks per window,
 * device W slots + 2 W hbx_restore_in_bound (+ W max_block in diff mode), pinned
 * host 2 W hbx_restore_in_bound + 2 W max_block (about 4.2 GiB pinned at the
 * defaults, W = 127).  The buffers are kept for the next call and freed by
 * hbx_ctx_destroy.
 * The first bad block ends the call with HBX_ERR_VERIFY, *bad_index its index
 * and *bad_status its status (as hbx_restore_blocks); the blocks before it
 * were written or sunk, nothing at or past it.  A failing source, sink or
 * write, or a local file that cannot be read, is HBX_ERR_IO.  Diff mode stops
 * at the first window that holds a difference.  *bytes = the bytes restored
 * (compared).  In every case the engine's streams are drained and the context
 * stays usable.  Synchronous; HBX_ERR_STATE while batches are pending. */
int hbx_restore_file_stream(hbx_ctx *ctx, uint64_t n_blocks, const uint8_t *ids, hbx_block_source_fn src,
                            void *user, uint64_t window_bytes, const char *out_path, hbx_restore_sink_fn sink,
                            const char *local_path, uint64_t max_block, uint64_t *bytes, uint64_t *bad_index,
                            uint32_t *bad_status, uint64_t *first_diff);

/* ---- Restore and diff of many files in one call (K11) --------------------------
 * restoreDir restores a directory's entries one after the other
 * (hashback/restore.go:137-162: restoreEntry per FileEntry, restore.go:68-135,
 * each file through restoreFileData, restore.go:45-66); diffDir / diffEntry
 * walk the same way and compare (restore.go:279-414, diffFileData 249-277).
 * The calls above take one chain per call, a round trip per file.  These are
 * the read side's counterpart of hbx_store_paths: the chains of MANY files in
 * one call, in WINDOWS formed across files, with a result per file.
 *
 * Blocks are listed in (file, index) order; file f owns the blocks
 * [first[f], first[f + 1]) (first holds n_files + 1 entries, first[0] = 0).  A
 * directory or chain block is a one-block "file" (links as hbx_verify_blocks).
 * Per-block statuses are exactly hbx_restore_blocks' (0-8) and its PREFIX rule
 * holds per file: file f's result is its n_good[f] leading good blocks,
 * nothing of it past its first bad block is written, and a bad block in one
 * file changes nothing in any other.  A corrupt block is a result: HBX_OK.
 *
 * Size hints (FileEntry.FileSize per file; NULL or 0 = unknown): a zlib block
 * of file f gets an inflate slot of min(max_block, hint[f]) bytes instead of
 * max_block, so a window holds thousands of small blocks and K8 can take its
 * lane-per-stream mode.  A hint is never trusted: a stream that overflows a
 * slot smaller than max_block is inflated again into a max_block slot while
 * its window is staged, and fails (status 3) only if it overflows that too.
 * Results are the same for every hint vector.
 *
 * hbx_restore_many_window is the window rule, pure host arithmetic: block i
 * takes caps[i] rounded up to 256, + 256 slack, of the window (caps: a zlib
 * block's slot capacity as above, a raw block's length, 0 for a status-8
 * block); *end = the first block after `start` that no longer fits
 * window_bytes (0 = 1 GiB), at least start + 1 (start == n: *end = n).  A
 * window also ends where its staged data fields reach window_bytes +
 * window_bytes / 512 + 2 hbx_restore_in_bound(max_block) + 4096 bytes (data
 * fields far longer than their hinted capacity).  Each window: K8 / K8s, then
 * K11 (hbx_k11_gather / hbx_k11_diff, a piece of at most 16 KiB per wave)
 * beside VerifyBlock (K6), guard bytes on both sides of the packed image
 * checked, every stream idle on return, also on failure.  When hints were
 * wrong the window runs as several K11 passes, cut by the same rule over the
 * corrected capacities. */
int hbx_restore_many_window(uint64_t n, const uint64_t *caps, uint64_t window_bytes, uint64_t start, uint64_t *end);
/* n_files chains in host memory (datas / lens / types / expect / links as
 * hbx_restore_blocks, over all first[n_files] blocks).  Exactly one of out and
 * local is set.  out: the PACKED image, file f's good prefix at
 * out[out_offs[f] .. out_offs[f + 1]) (out_offs holds n_files + 1); an out_cap
 * smaller than that is HBX_ERR_CAPACITY.  local (diff mode): the packed local
 * copies, file f's at local[local_offs[f] .. local_offs[f + 1]); first_diff[f]
 * is what hbx_restore_blocks defines, per file: the smallest offset inside the
 * file's good prefix at which the two differ, else the shorter length if the
 * lengths differ, else UINT64_MAX.  blk_offs (may be NULL) receives per block
 * its offset inside its file (UINT64_MAX at and past the file's first bad
 * block), status per block its status, n_good per file its leading good
 * blocks.  Windows are 1 GiB.  Contradictory arguments return HBX_ERR_ARG
 * before the context is touched; HBX_ERR_STATE while batches are pending.
 * Synchronous. */
int hbx_restore_files_blocks(hbx_ctx *ctx, uint64_t n_files, const uint64_t *first,
                             const uint8_t *const *datas, const uint64_t *lens, const uint8_t *types,
                             const uint8_t *expect, const uint8_t *links, const uint64_t *link_base,
                             const uint32_t *n_links, const uint64_t *size_hint, uint64_t max_block,
                             uint8_t *out, uint64_t out_cap, uint64_t *out_offs,
                             const uint8_t *local, const uint64_t *local_offs,
                             uint64_t *blk_offs, uint32_t *status, uint64_t *n_good, uint64_t *first_diff);
/* Block `index` of file `file`, otherwise as hbx_block_source_fn. */
typedef int (*hbx_file_block_source_fn)(void *user, uint64_t file, uint64_t index, uint8_t *dst, uint64_t cap,
                                        uint64_t *len, uint8_t *type);
typedef struct {
  uint64_t bytes;      /* the bytes of the file's good prefix (restored or compared) */
  uint64_t n_good;     /* its leading good blocks */
  uint64_t bad_index;  /* the index in the file of its first bad block, UINT64_MAX if none */
  uint64_t first_diff; /* diff mode, as hbx_restore_files_blocks; UINT64_MAX also when err != 0 */
  uint32_t bad_status; /* that block's status */
  int32_t err;         /* errno of a path that could not be created, written, opened or read; else 0 */
} hbx_restored_file;
/* The same for files of any number and size, two windows in flight as in
 * hbx_restore_file_stream: a fill thread calls src one call at a time in
 * (file, index) order into pinned staging (ids: the expected BlockIDs in the
 * same order); a pool of io_threads writers (0 = 16; more than 16 is
 * HBX_ERR_ARG) creates or truncates out_paths[f] and pwrites the file's good
 * prefix, a file that spans windows at its running offset; a file without
 * blocks is created empty.  With local_paths instead (diff mode; exactly one
 * of the two is set) the pool reads the local files and nothing is written.
 * A path that cannot be created, written, opened or read is that file's err
 * and the call goes on; a bad block is that file's bad_index / bad_status and
 * the call goes on (HBX_OK).  A failing src is HBX_ERR_IO.  After any failure
 * the streams are drained and the context is usable.
 * Memory depends on window_bytes (W; 0 = 1 GiB) and max_block (M) only.  With
 * S = W + W / 512 + 2 hbx_restore_in_bound(M) + 4096: device 2 S of staged
 * input + W of slots + max(W, M + 512) of slots for streams inflated again
 * (+ W + M in diff mode); pinned host 2 S + 2 (W + M) (about 4.1 GiB pinned at
 * the defaults).  The buffers are kept for the next call and freed by
 * hbx_ctx_destroy.  Synchronous; HBX_ERR_STATE while batches are pending;
 * contradictory arguments return HBX_ERR_ARG before the context is touched. */
int hbx_restore_files_stream(hbx_ctx *ctx, uint64_t n_files, const uint64_t *first, const uint8_t *ids,
                             hbx_file_block_source_fn src, void *user, const uint64_t *size_hint,
                             uint64_t window_bytes, const char *const *out_paths, const char *const *local_paths,
                             uint32_t io_threads, uint64_t max_block, hbx_restored_file *results);

/* ---- Diff and restore by block ID: local files against stored chains (K12) -----
 * diffEntry / diffFileData (hashback/restore.go:249-277, 317-367) fetch, verify
 * and compare every data block of every file whose size matches.  A file's
 * stored chain is its list of block IDs, and a block ID binds the block's
 * length and bytes (block.go:96-111): if cutting and hashing the LOCAL file
 * gives the same ID list, the file equals the stored one and none of its data
 * blocks needs to come off the wire.  The converse does not hold: a chain cut
 * by another chunker names equal bytes with other IDs, so a file that is not
 * `same` goes to the byte comparison (hbx_restore_files_stream in diff mode);
 * it is never reported as different on the strength of its IDs.
 * K12 (hbx_k12_chain_match) compares, per file, the local ID list with the
 * expected one: one wave per file, a 32-byte record per file. */
typedef struct {
  uint32_t n_match;     /* length of the common prefix of the local and the expected ID list */
  uint32_t n_local;     /* chunks the local file was cut into */
  uint32_t n_expect;    /* IDs in the expected chain */
  uint32_t same;        /* 1 iff n_match == n_local == n_expect */
  uint64_t match_bytes; /* local offset where chunk n_match starts: cut_ends[n_match - 1], 0 for n_match == 0
                           (so the file's length when n_match == n_local) */
  uint64_t reserved;    /* 0 */
} hbx_chain_match;
/* Short-cuts diffFileData / diffEntry (restore.go:249-277, 317-367) for ID lists
 * the caller already holds, in host memory: file f's local IDs are
 * local_ids[16 local_first[f] .. 16 local_first[f + 1]), its expected chain
 * expect_ids[16 expect_first[f] .. 16 expect_first[f + 1]) (*_first: n_files + 1
 * running counts from 0).  local_cut_ends (parallel to local_ids) may be NULL:
 * match_bytes is then 0.  match receives n_files records.  Runs K12 alone, as
 * hbx_idset_insert runs K9 alone.  Synchronous; HBX_ERR_STATE while batches are
 * pending; n_files == 0 is HBX_OK.  HBX_ERR_ARG: a NULL context, array or
 * match, running counts that decrease, a chain of 2^32 or more IDs, 2^32 or
 * more local IDs in all. */
int hbx_match_chains(hbx_ctx *ctx, uint64_t n_files, const uint64_t *local_first, const uint8_t *local_ids,
                     const uint64_t *local_cut_ends, const uint64_t *expect_first, const uint8_t *expect_ids,
                     hbx_chain_match *match);
/* hbx_submit_device with expected chains: short-cuts diffFileData / diffEntry
 * (restore.go:249-277, 317-367) for files in device memory.  expect_first ==
 * NULL is exactly hbx_submit_device.  Otherwise expect_first (n_files + 1
 * running counts, expect_first[0] need not be 0) and the IDs they index are
 * copied at submit (the caller's arrays are free on return), K12 runs on the
 * device once the batch's last chain is hashed, and match[f] (required; valid
 * until then) is filled by the hbx_wait that completes the batch.
 * VERDICT-ONLY mode: cut_ends, ids, out_base and caps all NULL together.  The
 * result slots are sized by hbx_max_chunks(len), and the batch brings back only
 * its per-file sections (content IDs, content types, match records: at most
 * 52 n_files + 768 bytes) instead of 24 bytes per result slot; summaries
 * (may be NULL) are filled as usual.
 * HBX_ERR_ARG: a NULL context; expect_first without match; expect_first
 * without expect_ids while the chains hold an ID; running counts that
 * decrease; a chain of 2^32 or more IDs; only some of cut_ends, ids, out_base
 * and caps NULL (out_base and caps are required unless all four are NULL;
 * without expect_first they are always required).  Verify batches and segment
 * batches take no match; match together with an ID set is not offered. */
int hbx_submit_device_match(hbx_ctx *ctx, const void *d_arena, uint64_t n_files, const uint64_t *file_offs,
                            const uint64_t *file_lens, uint64_t *cut_ends, uint8_t *ids, const uint64_t *out_base,
                            const uint64_t *caps, hbx_file_summary *summaries, const uint64_t *expect_first,
                            const uint8_t *expect_ids, hbx_chain_match *match);
/* hbx_store_paths_status (without compression) with expected chains: short-cuts
 * diffFileData / diffEntry (restore.go:249-277, 317-367) for files on disk, at
 * the store path's speed.  expect_first == NULL is exactly
 * hbx_store_paths_status without compression, except that status may be NULL
 * (every read failure then fails the call, as in hbx_store_paths_dd).  A file
 * with a non-zero status has n_local 0; its record means nothing more.
 * batch_bytes is honoured down to 1 MiB, as with a set; the records do not
 * depend on how the files fall into batches.  Verdict-only mode and the
 * argument checks as hbx_submit_device_match. */
int hbx_store_paths_match(hbx_ctx *ctx, uint64_t n_files, const char *const *paths, const uint64_t *lens,
                          uint64_t *cut_ends, uint8_t *ids, const uint64_t *out_base, const uint64_t *caps,
                          hbx_file_summary *summaries, int32_t *status, uint32_t io_threads, uint64_t batch_bytes,
                          const uint64_t *expect_first, const uint8_t *expect_ids, hbx_chain_match *match);

/* ---- Restore over an existing tree: where local files hold wanted blocks (K13) -----
 * restoreFileData (hashback/restore.go:45-66) fetches every block of every file
 * it writes.  A block ID binds the block's length and bytes (block.go:96-111)
 * and content-defined chunking leaves the IDs around a local change as they
 * were, so a chunk of ANY local file that carries a wanted ID is that block:
 * a file changed in one place, grown by a byte, renamed or copied needs only
 * the blocks no local file holds.  K13 (hbx_k13_build, hbx_k13_lookup) is that
 * join on the device: the pool's IDs go into a scratch slot table (K9's, with
 * the pool index as payload), every wanted ID is looked up in it.  The caller
 * reads the located bytes from the local file and hands them to VerifyBlock as
 * a raw block (hbx_restore_files_stream): a local file that changed since it
 * was hashed is found out there, never written. */
typedef struct {
  uint32_t file;     /* pool file holding the chunk; UINT32_MAX = not in the pool */
  uint32_t chunk;    /* its index among that file's chunks */
  uint64_t off;      /* where it starts in that file: the previous chunk's cut end, 0 for chunk 0 */
  uint64_t len;      /* its length */
  uint64_t reserved; /* 0 */
} hbx_block_loc;     /* 32 bytes; on a miss chunk = 0, off = len = 0 */
/* For each of n_want IDs (want_ids, 16 bytes each, host memory) the first place
 * the pool holds it: pool file f's chunk IDs are pool_ids[16 pool_first[f] ..
 * 16 pool_first[f + 1]) (pool_first: n_pool_files + 1 running counts, which need
 * not start at 0), pool_cut_ends runs parallel to pool_ids with offsets
 * relative to each file.  loc[j] names the LOWEST pool index whose 16 bytes
 * equal want_ids[j], so the answer does not depend on the run; *n_found (may
 * be NULL) is the number of hits.  Runs K13 alone on the result stream, as
 * hbx_match_chains runs K12 alone.  Synchronous; HBX_ERR_STATE while batches
 * are pending or after a failed submit; n_want == 0 is HBX_OK, nothing runs (*n_found = 0);
 * an empty pool makes every record a miss.  HBX_ERR_ARG, before the context is
 * touched: a NULL context; pool_first NULL with n_pool_files > 0; pool_ids or
 * pool_cut_ends NULL while the pool holds an ID; want_ids or loc NULL with
 * n_want > 0; running counts that decrease; more than 2^31 - 1 pool files, more
 * than 2^30 pool IDs, more than 2^32 - 1 wanted IDs.
 * Device memory, with np pool IDs, nw wanted IDs and S = hbx_idset_slots(np)
 * table slots: 16 (np + nw) + 8 np + 8 (n_pool_files + 1) + 4 S + 32 nw bytes
 * (+ 8 for the hit count), kept for the next call and freed by hbx_ctx_destroy. */
int hbx_locate_ids(hbx_ctx *ctx, uint64_t n_pool_files, const uint64_t *pool_first,
                   const uint8_t *pool_ids, const uint64_t *pool_cut_ends,
                   uint64_t n_want, const uint8_t *want_ids, hbx_block_loc *loc, uint64_t *n_found);

/* ---- Check a storage data file: scan, inflate, verify (K14) ---------------------
 * The server keeps its blocks in data files (*.dat, pkg/storagedb/data.go,
 * storagedb.go:40-53):
 *   header  BE32 filetype "HSDB" | BE32 version 1 | BE64 deadspace     (16 bytes)
 *   entry   "hblk" | BlockID[16] | BE32 n_links | n_links x 16 | DataType u8 |
 *           BE32 data_len | data            (data.go:33-37 around block.go:56-94;
 *           size = 29 + 16 n_links + data_len)
 *   gap     "Cgap" | BE64 skip, counted from the 'C'            (data.go:142-164)
 * RecoverData (integrity.go:74-143) walks a file from offset 16, one block at a
 * time on one goroutine, and resynchronises after damage on the next "hblk"
 * anywhere in the bytes; checkBlockFromIXEntry (integrity.go:259-296) reads the
 * entry at an offset the index names.  These calls do both on the device: K14
 * (hbx_k14_scan, hbx_k14_parse) finds and frames every "hblk" and "Cgap" of
 * the image, K8 / K8s and K6 inflate and VerifyBlock every framed entry in
 * place, links in the hash, and the walk is left with list lookups
 * (hbx_datfile_walk).  They report and write nothing: repairing index and meta
 * files, rewriting blocks and writing gap markers stay with the caller.
 *
 * The walk.  offset = 16; while offset < size:
 *   1. fewer than 12 bytes left: a failure at offset.  Else, "Cgap" at offset
 *      with skip > 0: a gap of skip bytes, offset += skip.  A skip past the end
 *      of the file ends the gap (and the walk) at the end and sets gap_past_eof.
 *      (The reference does not terminate on such a file: its reader discards
 *      nothing more at the end and the loop in skipDataGap goes on, data.go:157.)
 *      A gap that ends exactly at the end of the file ends the walk.  Only ONE
 *      marker is skipped per step: a gap behind a gap is read as an entry and
 *      fails, as it does in the reference.  skip <= 0 skips nothing.
 *   2. blockOffset = offset.
 *   3. The entry at blockOffset is STRUCTURALLY VALID if the marker is there,
 *      every field lies inside the file (n_links and data_len are untrusted:
 *      64-bit arithmetic), DataType is raw or zlib and data_len <=
 *      hbx_restore_in_bound(max_block).
 *   4. It is GOOD if it is structurally valid and VerifyBlock is true (status
 *      0 of hbx_restore_blocks); then offset = blockOffset + size.
 *   5. Any failure opens a broken span at blockOffset unless one is open, and
 *      the walk goes on at the first "hblk" at a position > blockOffset, also
 *      one inside the failed entry's claimed extent; without one it ends.
 *   6. A broken span runs to the next good entry's offset; consecutive failures
 *      merge; a walk that ends inside one sets truncate_at to its start
 *      (integrity.go:250-253).
 * Every result satisfies 16 + sum(entry sizes) + sum(gap lengths) + sum(broken
 * span lengths) = size (for size >= 16). */
#define HBX_DAT_FILETYPE 0x48534442u /* "HSDB" */
#define HBX_DAT_VERSION 1u
#define HBX_DAT_HEADER 16u
#define HBX_DAT_MARKER 0x68626C6Bu /* "hblk" */
#define HBX_DAT_GAP 0x43676170u    /* "Cgap" */
#define HBX_DAT_ENTRY_MIN 29u      /* an entry without links and data */
#define HBX_DAT_IMAGE_SLACK 64u    /* readable bytes a device image needs behind its size */
#define HBX_DAT_ST_INVALID 9u      /* no marker, or not structurally valid */
#define HBX_DAT_ST_WRONG_ID 10u    /* hbx_datfile_verify_at: not the expected BlockID */
#define HBX_DAT_F_MARKER 1u        /* hbx_dat_record.flags: the 4-byte marker is at off */
#define HBX_DAT_F_GAP 2u           /* the record frames a gap marker; size holds the skip */
#define HBX_DAT_SPAN_GAP 0u
#define HBX_DAT_SPAN_BROKEN 1u
typedef struct {
  uint64_t off;       /* the position framed */
  uint64_t size;      /* 29 + 16 n_links + data_len; a gap: its skip as two's complement */
  uint64_t data_off;  /* where the data field starts in the file */
  uint64_t links_off; /* where the links start (off + 24) */
  uint32_t data_len;
  uint32_t n_links;
  uint32_t status;    /* 0: structurally valid (after the check: the VerifyBlock status); 9 */
  uint8_t type;       /* DataType */
  uint8_t flags;      /* HBX_DAT_F_* */
  uint16_t pad;
  uint8_t id[16];     /* BlockID */
} hbx_dat_record;     /* 64 bytes, what hbx_k14_parse writes; but for off and flags all 0 when status is 9 */
typedef struct {
  uint64_t off, size, data_off;
  uint64_t link_base; /* index of its first link in the links output (16 bytes each) */
  uint32_t n_links, data_len;
  uint32_t plain_len; /* length of the block's data after inflating */
  uint8_t type;
  uint8_t pad[3];
  uint8_t id[16];
} hbx_dat_entry;      /* 64 bytes: a good entry on the walk */
typedef struct {
  uint64_t off, len;
  uint32_t kind;      /* HBX_DAT_SPAN_GAP / HBX_DAT_SPAN_BROKEN */
  uint32_t status;    /* broken: status of its first failure (1..8 as hbx_restore_blocks, 9); gap: 0 */
  uint64_t n_failed;  /* broken: failures inside at positions that carry the "hblk" marker */
} hbx_dat_span;       /* 32 bytes */
typedef struct {
  uint64_t size;
  uint32_t filetype, version; /* header fields (0 where the file is too short) */
  uint64_t deadspace;
  uint32_t header_ok;         /* 16 bytes, "HSDB", version 1 */
  uint32_t gap_past_eof;
  uint64_t n_candidates;      /* "hblk" markers at positions in [16, size - 4] */
  uint64_t n_gap_markers;     /* "Cgap" markers there */
  uint64_t n_valid;           /* structurally valid candidates: each was inflated and verified */
  uint64_t n_unreached;       /* candidates that never were the walk's block offset */
  uint64_t n_entries, entry_bytes;
  uint64_t n_gaps, gap_bytes;
  uint64_t n_broken, broken_bytes;
  uint64_t n_spans;           /* n_gaps + n_broken */
  uint64_t n_links;           /* links of all good entries */
  uint64_t truncate_at;       /* UINT64_MAX: the walk did not end inside a broken span */
} hbx_dat_summary;            /* 136 bytes */

/* Pure host functions (no context, no device): the header, the structural
 * rules and the walk, as the device path applies them.
 * header_parse: in[0 .. len) is the start of a file.  HBX_OK for 16 bytes of
 * "HSDB" version 1, HBX_ERR_FORMAT otherwise; the fields (each may be NULL)
 * are written as far as len allows, else 0. */
int hbx_datfile_header_parse(const uint8_t *in, uint64_t len, uint32_t *filetype, uint32_t *version,
                             uint64_t *deadspace);
/* Frame the entry at off of the file image[0 .. size) (host memory) by rule 3,
 * exactly as hbx_k14_parse: no byte at or past size is read, whatever n_links
 * and data_len claim.  rec->status is 0 or 9.  HBX_ERR_ARG for NULL arguments
 * or max_block above 1 GiB (0 = HBX_MAX_BLOCK). */
int hbx_datfile_entry_parse(const uint8_t *image, uint64_t size, uint64_t off, uint64_t max_block,
                            hbx_dat_record *rec);
/* The walk over a file of `size` bytes: cand[0 .. n_cand) the records of ALL
 * its "hblk" positions, ascending by off, status 0 (good), 1..8 or 9;
 * plain_len (may be NULL) parallel to cand; gap_offs ascending with gap_skips
 * the "Cgap" positions that have 12 bytes inside the file.  Writes up to
 * entry_cap entries and span_cap spans (both ascending by off; either array
 * may be NULL with capacity 0) and *summary's walk fields (n_unreached,
 * n_entries .. truncate_at, gap_past_eof, size, n_candidates, n_gap_markers;
 * the header fields and n_valid are left alone).  HBX_ERR_CAPACITY if a
 * capacity is too small: the summary then holds the needed counts.
 * HBX_ERR_ARG for NULL lists with a count, a NULL summary or lists that do not
 * ascend. */
int hbx_datfile_walk(uint64_t size, uint64_t n_cand, const hbx_dat_record *cand, const uint32_t *plain_len,
                     uint64_t n_gaps, const uint64_t *gap_offs, const int64_t *gap_skips,
                     hbx_dat_entry *entries, uint64_t entry_cap, hbx_dat_span *spans, uint64_t span_cap,
                     hbx_dat_summary *summary);
/* Check the data file whose `size` bytes lie at d_image in device memory (16-byte
 * aligned, HBX_DAT_IMAGE_SLACK readable bytes behind size; hbx_arena_alloc
 * gives both).  max_block (0 = HBX_MAX_BLOCK) is the largest block data
 * accepted; max_candidates (0 = 1 Mi) the capacity of each of K14's two
 * position lists; window_bytes (0 = an eighth of the free device memory, at
 * least 1 GiB, at most 32 GiB) bounds the inflate slots of one window by
 * hbx_restore_many_window's rule, a zlib entry's share being
 * min(max_block, 8 data_len + 4096): a stream that outgrows it is inflated
 * again into a max_block slot, so no result depends on that estimate.  EVERY
 * structurally valid candidate is inflated and verified, not only those the
 * walk reaches, so the walk does not wait for a verification.  Inflated bytes
 * are dropped after the hash.  Outputs: entries (entry_cap), spans (span_cap),
 * links (16-byte IDs, link_cap of them; NULL with link_cap 0: not wanted) and
 * *summary (required).  A damaged file is a result, not an error (HBX_OK).
 * HBX_ERR_CAPACITY: more markers of a kind than max_candidates (then
 * n_candidates / n_gap_markers hold the counts and nothing else is set), or
 * more entries, spans or links than their capacities (then the summary is
 * complete and the arrays hold what fitted).  HBX_ERR_ARG: NULL context,
 * image or summary, an unaligned image, max_block above 1 GiB.  Synchronous;
 * HBX_ERR_STATE while batches are pending; every stream is idle on return and
 * the context stays usable after any failure.  Device memory beside the image:
 * 16 bytes per list position + 72 per candidate + the window's slots, kept for
 * the next call and freed by hbx_ctx_destroy.  Replaces the loop of
 * RecoverData (integrity.go:94-143) up to its repairs, and CompactFile's
 * sequential read of a data file. */
int hbx_datfile_check_device(hbx_ctx *ctx, const void *d_image, uint64_t size, uint64_t max_block,
                             uint64_t max_candidates, uint64_t window_bytes, hbx_dat_entry *entries,
                             uint64_t entry_cap, hbx_dat_span *spans, uint64_t span_cap, uint8_t *links,
                             uint64_t link_cap, hbx_dat_summary *summary);
/* The same for the file at `path`: read through two pinned staging buffers
 * into one device image.  HBX_ERR_IO (with the path in hbx_last_error) if it
 * cannot be opened or read in full; HBX_ERR_CAPACITY if it does not fit a
 * third of the free device memory (segmenting is the caller's business). */
int hbx_datfile_check_path(hbx_ctx *ctx, const char *path, uint64_t max_block, uint64_t max_candidates,
                           uint64_t window_bytes, hbx_dat_entry *entries, uint64_t entry_cap,
                           hbx_dat_span *spans, uint64_t span_cap, uint8_t *links, uint64_t link_cap,
                           hbx_dat_summary *summary);
/* Entries at offsets the caller knows (checkBlockFromIXEntry, integrity.go:
 * 259-296): no scan, no walk.  The image is d_image (size bytes, as above) or,
 * with d_image NULL, the file at path (then size is ignored).  status[i] for
 * offs[i] with the expected BlockID expect_ids[16 i ..]:
 *   9   no structurally valid entry there;
 *   10  the entry's BlockID is not the expected one (integrity.go:292);
 *   else, content != 0: the VerifyBlock status (0..7; fullVerify,
 *   integrity.go:279-284); content == 0: 0, the header and ID check alone
 *   (integrity.go:287-295).
 * Errors and the contract as hbx_datfile_check_device / _path; n == 0 is
 * HBX_OK and nothing runs. */
int hbx_datfile_verify_at(hbx_ctx *ctx, const void *d_image, uint64_t size, const char *path, uint64_t n,
                          const uint64_t *offs, const uint8_t *expect_ids, int content, uint64_t max_block,
                          uint64_t window_bytes, uint32_t *status);

/* ---- Block graph: GC mark and block-tree check (K15) -----------------------------
 * hbx_datfile_check_* gives every good entry of a data file with its BlockID
 * and its links.  The server joins that table next, one index probe and one
 * meta read per block on one goroutine: MarkIndexes (pkg/storagedb/gc.go:24-69)
 * follows links breadth-first from the roots and marks what it reaches;
 * checkBlockFromIXEntry's link recursion (integrity.go:298-329, entered from
 * CheckBlockTree :346-352 and CheckIndexes :354-410) calls a block valid only
 * if its own check passed, every link exists and every linked block is valid.
 * hbx_block_graph does both joins on the device (K15, hbx_graph.hip).
 *
 * Input: a BLOCK TABLE of n rows, ids[16 n], n_links[n], link_base[n], and a
 * flat array of m link IDs.  Row i's links are links[16 (link_base[i] + k)] for
 * k < n_links[i]; bases may come in any order, lists may overlap or leave
 * holes.  bad[n] (may be NULL) is non-zero where the row's own check failed (a
 * VerifyBlock status, an invalid index flag).  root_ids[16 n_roots] are the
 * roots.  NONE = HBX_GRAPH_NONE.
 *  1. Representative.  The node of an ID is its LOWEST row (K13's rule, so
 *     every run answers the same); rep[i] is that row.  A row with rep[i] != i
 *     is an ALIAS: its bad flag and its links are ignored, and its two depth
 *     outputs are copies of its representative's.
 *  2. Resolve.  link_row[e] is the representative row of links[e], or NONE (a
 *     missing link), for every e < m, also for link slots no row owns;
 *     root_row[q] the same for the roots.  Equality is on all 16 bytes.
 *  3. Mark.  mark_depth[i] is the length of the shortest link path from any
 *     root to row i: 0 for a root, NONE if unreached.  The links of bad rows
 *     are followed too (the reference's mark does not look at validity).
 *     Missing links and missing roots are skipped and counted: where the
 *     reference aborts (gc.go:36-37) this call reports, and n_marked_faulty
 *     lets a caller refuse to sweep.
 *  4. Tree check.  A representative row is FAULTY if bad[i] is set or one of
 *     its links is missing.  fault_depth[i] is 0 for a faulty row, else the
 *     length of the shortest link path from row i down to a faulty row, else
 *     NONE: the block tree below the row is valid, what verifiedBlocks[id] ==
 *     true means in the reference.  Links that form a cycle cannot occur with
 *     real MD5 IDs but can in a crafted table, and the reference recurses
 *     without end on one; here a cycle from which no faulty row can be
 *     reached is valid, and one from which a faulty row can be reached is not.
 *  5. Summary.  Counts of rows count representatives only.  The levels of a
 *     sweep are its largest depth + 1 (0 when it claimed no row).
 * Every output is a function of the input alone: a depth is a BFS level,
 * whichever lane claimed the row. */
#define HBX_GRAPH_NONE 0xFFFFFFFFu
#define HBX_GRAPH_LANE_MAX 16u   /* a link list up to this long is walked by one lane, */
#define HBX_GRAPH_WAVE_MAX 4096u /* up to this long by its row's wave, a longer one by a workgroup */
typedef struct {
  uint64_t n_rows, n_links;  /* n and m as given */
  uint64_t n_alias;          /* rows with rep[i] != i */
  uint64_t n_missing_links;  /* e < m with link_row[e] == NONE */
  uint64_t n_roots, n_roots_missing;
  uint64_t n_marked;         /* representatives with mark_depth != NONE */
  uint64_t mark_levels;
  uint64_t n_faulty;         /* representatives with fault_depth == 0 */
  uint64_t n_invalid;        /* representatives with fault_depth != NONE */
  uint64_t fault_levels;
  uint64_t n_marked_faulty;  /* representatives with both depths != NONE: a live tree is damaged */
} hbx_graph_summary;         /* 96 bytes */
/* All pointers are host memory, as in hbx_locate_ids.  Any output array (rep
 * [n], link_row [m], root_row [n_roots], mark_depth [n], fault_depth [n]) may
 * be NULL: not wanted.  With mark_depth == NULL and n_roots == 0 the mark does
 * not run; with fault_depth == NULL the tree check does not run; the summary
 * fields of a stage that did not run are 0 (n_marked_faulty needs both).  The
 * transposed graph of the tree check is built only if a faulty row exists: a
 * healthy store answers all-NONE after one pass over its links.
 * Synchronous; HBX_ERR_STATE while batches are pending or after a failed
 * submit; runs alone on the result stream; every stream is idle on return and
 * the context stays usable after any failure.  n == 0 is HBX_OK with every
 * link and root missing.  HBX_ERR_ARG, before anything is launched: a NULL
 * context or summary; ids, n_links or link_base NULL with n > 0, links NULL
 * with m > 0, root_ids NULL with n_roots > 0; n above 2^31 - 1; a row with
 * link_base[i] + n_links[i] > m.  HBX_ERR_CAPACITY if the staging does not fit
 * the free device memory.  Device memory, kept for the next call and freed by
 * hbx_ctx_destroy, with S = hbx_idset_slots(n) table slots (8 to 16 bytes per
 * row): 49 bytes per row (ID, count, base, flag, rep, two depths, two frontier
 * words) + 4 S, 20 per link, 20 per root; with a faulty row 8 more per row
 * and 4 per link of the sum of n_links (the transposed graph).
 * Replaces the queue loop of MarkIndexes (gc.go:24-69) and the recursion of
 * checkBlockFromIXEntry (integrity.go:298-329) over a table in memory. */
int hbx_block_graph(hbx_ctx *ctx, uint64_t n, const uint8_t *ids, const uint32_t *n_links,
                    const uint64_t *link_base, uint64_t m, const uint8_t *links, const uint8_t *bad,
                    uint64_t n_roots, const uint8_t *root_ids, uint32_t *rep, uint32_t *link_row,
                    uint32_t *root_row, uint32_t *mark_depth, uint32_t *fault_depth,
                    hbx_graph_summary *summary);

/* ---- Compact a storage data file: pack, relocate, meta (K16) -----------------------
 * hbx_datfile_check_* gives a data file's good entries, hbx_block_graph which
 * of a store's rows the roots reach.  The server's next step is CompactFile
 * (pkg/storagedb/gc.go:208-318): it reads the file one entry at a time, drops
 * what no index entry points at, leaves the kept entries at the file's start
 * where they are, appends every other kept entry to the store's free file and
 * changes its location (changeDataLocation), and truncates the file at the
 * high-water mark.  These calls do that over one file image on the device
 * (K16, hbx_compact.hip) and also build the StorageMetaEntry (meta.go:21-39)
 * and the StorageIXEntry (index.go:24-38) each kept entry then needs.  They
 * report and return bytes; they open no store file for writing.
 *
 * Input: the image of `size` bytes (hbx_datfile_check_device's rules: 16-byte
 * aligned, HBX_DAT_IMAGE_SLACK readable bytes behind it), entries[n] as
 * hbx_datfile_check_* returns them (ascending, not overlapping), keep[n]
 * (non-zero: readIXEntry succeeds and VerifyLocation is true, gc.go:258-264)
 * and *args.
 *  1. Class.  klass[i] is HBX_CMP_DROP where keep[i] == 0; HBX_CMP_STAY where
 *     HBX_CMP_F_KEEP_PREFIX is set, every entry j <= i is kept and
 *     off[i] == 16 + sum of size[j] over j < i (the reference's readOffset ==
 *     highWaterMark with freeFileNum >= fileNumber, gc.go:266-268: a gap, a
 *     broken span or a dropped entry in front ends the prefix for good);
 *     HBX_CMP_MOVE for every other kept entry.  stay_end = 16 + the stayers'
 *     bytes: the reference's highWaterMark, where the source file is truncated.
 *  2. Moved stream.  The movers' bytes verbatim, in file order, back to back.
 *     new_off[i] = dst_base + the sizes of the movers before i; a stayer's
 *     new_off is its off, a dropped entry's UINT64_MAX.
 *  3. Meta stream.  One StorageMetaEntry per kept entry, in order, back to back
 *     from meta_base: "hblk" | id[16] | location[6] | BE32 DataSize | BE32
 *     n_links | links (34 + 16 n_links bytes).  location is sixByteLocation(file,
 *     new_off), the 48-bit big-endian file << 34 | off (storagedb.go:90-101),
 *     file = file_no for a stayer and dst_file_no for a mover; DataSize is the
 *     entry's size; the links are copied from the image at off + 24.
 *     meta_off[i] is where entry i's record starts (meta_base + the record
 *     sizes of the kept entries before i); a dropped entry's is UINT64_MAX.
 *  4. Index records.  One 24-byte StorageIXEntry per kept entry, in order, as
 *     a flat array: BE16 flags | id | sixByteLocation(meta_file_no, meta_off[i]);
 *     flags is HBX_IX_F_EXISTS, with HBX_IX_F_NOLINKS when n_links == 0
 *     (data.go:96-100).  hbx_index_update puts them into index files held on
 *     the device (entries that exist; inserting stays with the caller).
 *  5. Summary: the counts and bytes per class; deleted_bytes = size - 16 - the
 *     stayers' bytes - moved_bytes (the reference's `deleted` on a file without
 *     broken spans; 0 for size < 16).
 *  6. A location holds 34 bits of offset.  If a stayer's or a mover's new_off
 *     or a meta_off would lie above HBX_DAT_OFFSET_LIMIT the call returns
 *     HBX_ERR_CAPACITY: the summary is complete, first_past_limit is the first
 *     such entry, klass / new_off / meta_off are written and nothing is
 *     packed.  The caller cuts the list there and calls again with the next
 *     file as destination.  Otherwise first_past_limit is UINT64_MAX.
 *  7. Where the reference aborts on a damaged file (Unserialize panics), the
 *     entry list is the authority here: whatever it does not name is deleted.
 *     The free-space check (gc.go:269) and the index updates are the caller's.
 *  8. HBX_ERR_ARG, before anything is launched: a NULL context, image, args
 *     or summary, an unaligned image; entries or keep NULL with n > 0, n above
 *     2^31 - 1; entries that do not ascend, that overlap, that start below 16
 *     or end past size; size != 29 + 16 n_links + data_len, or a size above
 *     2^32 - 1 (DataSize is a uint32); a file number above
 *     0x3fff; dst_base or meta_base below 16 (or so large that an offset
 *     leaves 64 bits); an output NULL with a capacity.
 * Any output may be NULL with capacity 0: not wanted, and a stream nobody wants
 * is not built.  n == 0 is HBX_OK. */
#define HBX_DAT_OFFSET_LIMIT 0x3FFFFFFFFull /* 2^34 - 1: storageOffsetLimit (storagedb.go:52) */
#define HBX_DAT_FILE_MAX 0x3FFFu
#define HBX_CMP_DROP 0u
#define HBX_CMP_STAY 1u
#define HBX_CMP_MOVE 2u
#define HBX_CMP_F_KEEP_PREFIX 1u
#define HBX_IX_F_EXISTS 1u  /* entryFlagExists (storagedb.go:56) */
#define HBX_IX_F_NOLINKS 2u /* entryFlagNoLinks */
#define HBX_META_HEAD 34u   /* a StorageMetaEntry without links */
#define HBX_IX_ENTRY 24u    /* storageIXEntrySize */
typedef struct {
  uint32_t file_no;      /* the file compacted: a stayer's location */
  uint32_t dst_file_no;  /* the file the moved stream is appended to ... */
  uint64_t dst_base;     /* ... at this offset */
  uint32_t meta_file_no; /* the meta file the meta stream is appended to ... */
  uint32_t flags;        /* HBX_CMP_F_* */
  uint64_t meta_base;    /* ... at this offset */
} hbx_dat_compact_args;  /* 32 bytes */
typedef struct {
  uint64_t n_entries, n_stay, n_moved, n_dropped;
  uint64_t stay_end, moved_bytes, dropped_bytes, deleted_bytes;
  uint64_t meta_bytes, n_meta; /* n_meta = n_stay + n_moved: meta records, and index records */
  uint64_t first_past_limit;
} hbx_dat_compact_summary;     /* 88 bytes */
/* Rules 1-6 and 8 on the host (no context, no device), exactly as the device
 * applies them: klass [n] (uint8), new_off [n], meta_off [n] (each may be
 * NULL) and *summary.  HBX_OK, HBX_ERR_ARG (rule 8; `size` is the file's) or
 * HBX_ERR_CAPACITY (rule 6). */
int hbx_datfile_compact_plan(uint64_t size, uint64_t n, const hbx_dat_entry *entries, const uint8_t *keep,
                             const hbx_dat_compact_args *args, uint8_t *klass, uint64_t *new_off,
                             uint64_t *meta_off, hbx_dat_compact_summary *summary);
/* The whole of it for the image at d_image (device memory); every other pointer
 * is host memory.  moved_out (moved_cap bytes), meta_out (meta_cap bytes) and
 * ix_out (ix_cap bytes, 24 per kept entry) receive the three outputs.
 * HBX_ERR_CAPACITY if a wanted output's capacity is too small: the summary
 * then holds the needed sizes (moved_bytes, meta_bytes, 24 n_meta) and no
 * array is written.  Synchronous; HBX_ERR_STATE while batches are pending or
 * after a failed submit; runs alone on the result stream; every stream is idle
 * on return and the context stays usable after any failure; no part of a batch.
 * Device memory beside the image is checked against the free memory first
 * (HBX_ERR_CAPACITY), kept for the next call and freed by hbx_ctx_destroy: 106
 * bytes per entry (the table 64, keep and class 2, three scans 24, the movers'
 * list 16) + the wanted outputs + 128 guard bytes per stream.  Both packed streams lie between 64 guard bytes that hold
 * a pattern during the call and are checked after it (HBX_ERR_STATE on a
 * mismatch), as K10's and K11's images.  The device plan equals
 * hbx_datfile_compact_plan word for word. */
int hbx_datfile_compact_device(hbx_ctx *ctx, const void *d_image, uint64_t size, uint64_t n,
                               const hbx_dat_entry *entries, const uint8_t *keep,
                               const hbx_dat_compact_args *args, uint8_t *klass, uint64_t *new_off,
                               uint64_t *meta_off, uint8_t *moved_out, uint64_t moved_cap, uint8_t *meta_out,
                               uint64_t meta_cap, uint8_t *ix_out, uint64_t ix_cap,
                               hbx_dat_compact_summary *summary);
/* The same for the file at `path`, read through hbx_datfile_check_path's
 * reader into the kept device image (HBX_ERR_IO, HBX_ERR_CAPACITY as there);
 * `size` in rule 8 is the file's. */
int hbx_datfile_compact_path(hbx_ctx *ctx, const char *path, uint64_t n, const hbx_dat_entry *entries,
                             const uint8_t *keep, const hbx_dat_compact_args *args, uint8_t *klass,
                             uint64_t *new_off, uint64_t *meta_off, uint8_t *moved_out, uint64_t moved_cap,
                             uint8_t *meta_out, uint64_t meta_cap, uint8_t *ix_out, uint64_t ix_cap,
                             hbx_dat_compact_summary *summary);

/* ---- Index files on the device: probe, scan, mark, sweep, compact (K17) ------------
 * The store finds a block through its *.idx files (pkg/storagedb/index.go):
 * open-addressed tables of 24-byte StorageIXEntry records keyed by the last 24
 * bits of the block ID.  A GC run is MarkIndexes -> SweepIndexes ->
 * CompactIndexes (gc.go:24-206) and CheckIndexes reads every record
 * (integrity.go:354-410); the reference does all of it on one goroutine with a
 * seek and a read per probe.  An hbx_index holds the images of a store's index
 * files 0 .. n_files - 1 in device memory and applies the reference's
 * operations to them there (K17, hbx_index.hip), from hbx_index_open to
 * hbx_index_export; nothing is written to disk.  hbx_index_*_host are the same
 * operations over host images, in place, without a context or a device: what
 * a device call leaves in its images and outputs equals what the _host call
 * of the same name leaves, byte for byte and word for word.
 *
 * All integers are big-endian.
 *   File.  A 16-byte header (BE32 "HSIX", BE32 version 1, 8 more bytes;
 *     storagedb.go:40-49, as the data files'), then slots of 24 bytes: slot s
 *     lies at offset 16 + 24 s.  A valid size has (size - 16) % 24 == 0 and
 *     size <= HBX_IX_SIZE_MAX = 16 + 24 (2^24 + 682) (index.go:20-22).
 *   Slot.  BE16 flags | id[16] | sixByteLocation (48 bits, file << 34 | offset:
 *     where the block's meta entry lies; storagedb.go:90-106).
 *   Flags.  HBX_IX_F_EXISTS 1, _NOLINKS 2, _MARKED 4, _INVALID 8
 *     (storagedb.go:56-59).  A slot is LIVE if Exists is set and Invalid clear.
 *   Home.  home(id) = id[13] << 16 | id[14] << 8 | id[15]; base(id) = 16 + 24 home
 *     (calculateIXEntryOffset, index.go:48-50).
 *
 * THE RULE: findIXOffset(id, stop_on_free) (index.go:54-107).  Every call below
 * is defined through it.
 *   Start.  File f = 0, offset o = base(id).
 *   Per file.  If there is no file f: stop.  If o > size[f]: stop.  Otherwise
 *     make up to HBX_IX_PROBE_LIMIT (682) probes; each probe:
 *       if o >= size[f]: stop (the reference's "room at the end").
 *       Read the slot at o.
 *       Live and all 16 ID bytes equal: FOUND (f, o).
 *       Live with another ID: o += 24, next probe.
 *       Anything else: remember (f, o) as the free place if none is remembered
 *       yet; then stop if stop_on_free or the slot's Exists is clear, otherwise
 *       o += 24, next probe.
 *     After 682 probes: f++, o = base(id).
 *   On stop.  Not found; the PLACE is the remembered free one, else the current
 *     (f, o).  It may name a file that does not exist (f == n_files: "ran out
 *     of index files") or an offset at or past a file's end.
 * The semantics are those of that loop over a coherent image: the reference
 * flushes its writer before every probe (ixFile.Size, bufferedfile.go:88-93),
 * so a probe sees every earlier write.  readIXEntry(id) (index.go:109-115) is
 * the rule with stop_on_free = 0.
 *
 * Conventions of the device calls, as hbx_datfile_* and hbx_block_graph:
 * synchronous; HBX_ERR_STATE while batches are pending or after a failed
 * submit; a handle of another context is HBX_ERR_ARG; an output capacity too
 * small is HBX_ERR_CAPACITY with the needed counts in the summary and nothing
 * changed; device memory is checked against the free memory before it is
 * taken (HBX_ERR_CAPACITY); every stream is idle on return and the context
 * stays usable after any failure; n == 0 is HBX_OK.  A handle keeps, beside
 * its images, what its calls need (48 bytes per live entry for scan and sweep,
 * 8 bytes per column and a second copy of the images during a sweep) until
 * hbx_index_close; hbx_ctx_destroy closes what is still open. */
#define HBX_IX_F_MARKED 4u        /* entryFlagMarked (storagedb.go:58) */
#define HBX_IX_F_INVALID 8u       /* entryFlagInvalid */
#define HBX_IX_HEADER 16u         /* storageFileHeaderSize */
#define HBX_IX_PROBE_LIMIT 682u   /* storageIXEntryProbeLimit (index.go:21) */
#define HBX_IX_FILETYPE 0x48534958u /* "HSIX" */
#define HBX_IX_VERSION 1u
#define HBX_IX_SLOTS_MAX ((1u << 24) + HBX_IX_PROBE_LIMIT)
#define HBX_IX_SIZE_MAX (16ull + 24ull * HBX_IX_SLOTS_MAX) /* storageIXFileSize + the header */
#define HBX_IX_FILES_MAX 16u      /* index files in one hbx_index */
#define HBX_IX_SWEEP_TILE 256u    /* columns (slot numbers) per workgroup of the sweep kernel */
#define HBX_IX_ACT_DELETED 1u
#define HBX_IX_ACT_STAY 2u
#define HBX_IX_ACT_OBSOLETE 3u
#define HBX_IX_ACT_MOVED 4u
#define HBX_IX_ACT_ABORT 5u
typedef struct hbx_index hbx_index;
typedef struct {
  uint32_t found;     /* 1: the rule found the ID */
  uint32_t flags;     /* the slot's flags (found), else 0 */
  uint32_t file;      /* the rule's place, found or not; n_files = ran out of index files */
  uint32_t meta_file; /* the slot's location (found), else 0 */
  uint64_t offset;
  uint64_t meta_off;
} hbx_ix_hit;         /* 32 bytes */
typedef struct {
  uint8_t id[16];
  uint32_t flags;
  uint32_t ix_file;
  uint64_t ix_offset;
  uint32_t meta_file;
  uint32_t state;     /* 0: readIXEntry(id) returns this slot; 1: another slot (this one is an obsolete
                         duplicate); 2: none (the entry is cut off from its home) */
  uint64_t meta_off;
} hbx_ix_live;        /* 48 bytes */
typedef struct {
  uint64_t slots;
  uint64_t n_live, n_invalid, n_empty; /* Invalid set: invalid, whatever else; neither: empty */
  uint64_t n_marked, n_nolinks;        /* among the live ones */
  uint64_t n_misplaced;                /* live with offset < base(id): CheckIndexes aborts (integrity.go:387-390) */
  uint64_t first_misplaced;            /* the first such offset, UINT64_MAX without one */
  uint64_t trunc_point;                /* 16 + 24 (the last live slot + 1); 16 without one */
} hbx_ix_file_stats;                   /* 72 bytes */
typedef struct {
  uint64_t n_files, slots, n_live, n_invalid, n_empty, n_marked, n_nolinks, n_misplaced;
  uint64_t n_obsolete, n_cut_off; /* live entries of state 1 and 2 */
} hbx_ix_summary;                 /* 80 bytes */
typedef struct {
  uint8_t id[16];
  uint32_t meta_file;
  uint32_t reserved;
  uint64_t meta_off;
} hbx_ix_killed;      /* 32 bytes: killMetaEntry's arguments (gc.go:105-106) */
typedef struct {
  uint64_t n_live; /* live entries before the sweep: what action and moved_to must hold */
  uint64_t n_deleted, n_stay, n_obsolete, n_moved, n_abort;
  uint64_t first_abort;   /* the first live entry with HBX_IX_ACT_ABORT, UINT64_MAX without one */
  uint64_t swept_records; /* = n_deleted: what killed must hold */
  uint64_t n_grown;       /* files a move has lengthened */
} hbx_ix_sweep_summary;   /* 72 bytes */
typedef struct {
  uint64_t n_files;
  uint64_t cleared;                /* slots blanked */
  uint64_t size[HBX_IX_FILES_MAX]; /* each file's new size */
} hbx_ix_compact_summary;          /* 144 bytes */

/* Open: the images (host memory) of index files 0 .. n_files - 1 copied to the
 * device.  HBX_ERR_ARG: n_files == 0 or above HBX_IX_FILES_MAX, a NULL.
 * HBX_ERR_FORMAT: a size that is not valid (CheckIndexes aborts on it,
 * integrity.go:365-367), a header with another type or version (as
 * CheckStorageFiles, storagedb.go:150-165).  _paths reads each file through
 * the reader of hbx_datfile_check_path (HBX_ERR_IO). */
int hbx_index_open(hbx_ctx *ctx, uint32_t n_files, const uint8_t *const *images, const uint64_t *sizes,
                   hbx_index **out);
int hbx_index_open_paths(hbx_ctx *ctx, uint32_t n_files, const char *const *paths, hbx_index **out);
int hbx_index_close(hbx_ctx *ctx, hbx_index *ix);
/* sizes[n_files]: each file's current size (a sweep may lengthen, a compaction shorten it). */
int hbx_index_sizes(hbx_ctx *ctx, hbx_index *ix, uint64_t *sizes);
/* File `file`'s image as it stands into out (cap bytes), *n its size. */
int hbx_index_export(hbx_ctx *ctx, hbx_index *ix, uint32_t file, uint8_t *out, uint64_t cap, uint64_t *n);
/* The rule for n IDs (16 bytes each): hits[i].  With stop_on_free == 0 this is
 * readIXEntry.  The probe kernel: one lane per ID, a slot read as three 64-bit
 * words, the ID compared as two. */
int hbx_index_lookup(hbx_ctx *ctx, hbx_index *ix, uint64_t n, const uint8_t *ids, int stop_on_free,
                     hbx_ix_hit *hits);
/* One pass over every slot of every file: the pass of CheckIndexes, with
 * CompactIndexes' counters.  per_file[n_files] (may be NULL), *summary, and
 * live[j], the live entries in (file, offset) order (live may be NULL with
 * live_cap 0: only counted).  HBX_ERR_CAPACITY if live_cap < n_live: the
 * statistics are complete and live holds the first live_cap entries. */
int hbx_index_scan(hbx_ctx *ctx, hbx_index *ix, hbx_ix_live *live, uint64_t live_cap,
                   hbx_ix_file_stats *per_file, hbx_ix_summary *summary);
/* The write half of MarkIndexes (gc.go:46-54): for every ID readIXEntry finds,
 * Marked is set in that slot and nothing else changes (idempotent: an ID may
 * repeat).  found[i] (may be NULL) is 0 where the reference aborts
 * (gc.go:36-37); *n_missing (may be NULL) counts those.  The graph walk is
 * hbx_block_graph's: its mark selects the IDs. */
int hbx_index_mark(hbx_ctx *ctx, hbx_index *ix, uint64_t n, const uint8_t *ids, uint8_t *found,
                   uint64_t *n_missing);
/* changeMetaLocation (meta.go:122-128) and RecoverData's repair of an existing
 * entry (integrity.go:216-240) from n StorageIXEntry records (24 bytes each,
 * as hbx_datfile_compact_* returns them): where readIXEntry finds a record's ID, the
 * slot's location becomes the record's and its NoLinks bit the record's, every
 * other bit stays, status[i] = 0; where it does not, status[i] = 1 and nothing
 * is written.  INSERTING a new ID is not done here.  An ID that occurs twice in
 * one call is HBX_ERR_ARG, checked on the host before anything is launched. */
int hbx_index_update(hbx_ctx *ctx, hbx_index *ix, uint64_t n, const uint8_t *recs, uint8_t *status);
/* SweepIndexes (gc.go:70-151), the Marked bits read from the images.  The files
 * are walked in order, each from its first slot to the end it had when the
 * sweep began; an Invalid slot is skipped whatever else it holds, a slot with
 * Exists clear is not touched.  Live entry j (hbx_index_scan's order, before
 * the sweep) gets action[j]:
 *   HBX_IX_ACT_DELETED   Marked was clear: Invalid is set, the other bits stay;
 *     (id, meta_file, meta_off) is appended to killed, in live order.
 *   Otherwise Marked is cleared and the rule runs with stop_on_free = 1 over
 *   the images as they stand at that moment:
 *   HBX_IX_ACT_STAY      the place is this slot.
 *   HBX_IX_ACT_OBSOLETE  found elsewhere: Invalid is set.
 *   HBX_IX_ACT_MOVED     not found and the place lies in an earlier file, or
 *     earlier in this one (gc.go:121-128): the entry is written there without
 *     Marked, moved_to[2j] = its file, moved_to[2j + 1] = its offset, and the
 *     old slot gets Invalid.  A place past an earlier file's end lengthens that
 *     file to the end of the written slot; the bytes between are zero.
 *   HBX_IX_ACT_ABORT     any other place (gc.go:129-131, where the reference
 *     aborts): the entry is left as it is, Marked too, and the sweep goes on.
 * moved_to is UINT64_MAX twice for every other action.  If any entry got
 * HBX_IX_ACT_ABORT the call returns HBX_ERR_FORMAT: action, moved_to, killed
 * and the summary are as described and THE INDEX IS UNCHANGED.
 * HBX_ERR_CAPACITY: live_cap < n_live or killed_cap < n_deleted; the summary
 * holds n_live and n_deleted = swept_records, nothing else, and the index is
 * unchanged.  The _host form also returns it, index unchanged, when a file
 * would grow past its caps[f].
 * On the device the order-dependent loop runs in parallel over ranges of
 * columns (slot numbers shared by all files) no entry's reads and writes
 * cross: hbx_index.hip says how they are cut. */
int hbx_index_sweep(hbx_ctx *ctx, hbx_index *ix, uint8_t *action, uint64_t *moved_to, uint64_t live_cap,
                    hbx_ix_killed *killed, uint64_t killed_cap, hbx_ix_sweep_summary *summary);
/* CompactIndexes (gc.go:153-206): every slot with Invalid set becomes 24 zero
 * bytes; each file's size becomes 16 + 24 (its last live slot + 1), 16 without
 * one. */
int hbx_index_compact(hbx_ctx *ctx, hbx_index *ix, hbx_ix_compact_summary *summary);
/* The same operations over host images, in place (no context, no device; the
 * checks of hbx_index_open on every call).  sizes[f] is read, and written by
 * sweep and compact; caps[f] is what images[f] can hold (only the sweep reads
 * it; NULL elsewhere). */
int hbx_index_lookup_host(uint32_t n_files, uint8_t *const *images, uint64_t *sizes, const uint64_t *caps,
                          uint64_t n, const uint8_t *ids, int stop_on_free, hbx_ix_hit *hits);
int hbx_index_scan_host(uint32_t n_files, uint8_t *const *images, uint64_t *sizes, const uint64_t *caps,
                        hbx_ix_live *live, uint64_t live_cap, hbx_ix_file_stats *per_file,
                        hbx_ix_summary *summary);
int hbx_index_mark_host(uint32_t n_files, uint8_t *const *images, uint64_t *sizes, const uint64_t *caps,
                        uint64_t n, const uint8_t *ids, uint8_t *found, uint64_t *n_missing);
int hbx_index_update_host(uint32_t n_files, uint8_t *const *images, uint64_t *sizes, const uint64_t *caps,
                          uint64_t n, const uint8_t *recs, uint8_t *status);
int hbx_index_sweep_host(uint32_t n_files, uint8_t *const *images, uint64_t *sizes, const uint64_t *caps,
                         uint8_t *action, uint64_t *moved_to, uint64_t live_cap, hbx_ix_killed *killed,
                         uint64_t killed_cap, hbx_ix_sweep_summary *summary);
int hbx_index_compact_host(uint32_t n_files, uint8_t *const *images, uint64_t *sizes, const uint64_t *caps,
                           hbx_ix_compact_summary *summary);

/* Device arena helpers (allocations include HBX_ARENA_SLACK). */
int hbx_arena_alloc(hbx_ctx *ctx, uint64_t bytes, void **d_ptr);
int hbx_arena_free(hbx_ctx *ctx, void *d_ptr);
int hbx_memcpy_h2d(hbx_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
/* Enqueue an H2D copy on the context's stream and return at once: a
 * following hbx_submit_device on the same context runs after it.  h_src
 * should be hbx_alloc_pinned memory (pageable memory makes the copy
 * synchronous).  Use two contexts to overlap the next batch's copy with the
 * current batch's kernels. */
int hbx_memcpy_h2d_async(hbx_ctx *ctx, void *d_dst, const void *h_src, uint64_t bytes);
/* Order the context's next device work after everything enqueued so far on
 * `stream` (a hipStream_t of the same device, e.g. the stream that filled an
 * arena; NULL = the null stream).  The dependency is on the GPU (an event the
 * context's streams wait for): the host never blocks, so a caller can keep
 * submitting batches ahead of the device.  For the null stream and a blocking
 * scan stream (the default) the legacy default-stream ordering already holds
 * and nothing is recorded.  No reference counterpart: Go callers hand over
 * host buffers. */
int hbx_after_stream(hbx_ctx *ctx, void *stream);
int hbx_alloc_pinned(uint64_t bytes, void **out);
int hbx_free_pinned(void *p);

/* The context's effective pipeline knobs as one JSON object (NUL-terminated,
 * at most cap bytes): slice, join lag, K1 tile and run, K3 waves and placement,
 * and whether the HBX_* A/B environment switches were honoured (ab_env: they
 * are read only when HBX_AB=1); restore_ms: the host milliseconds the latest
 * hbx_restore_* call spent staging its input, inflating, verifying beside
 * K10 / K11, and copying out, each phase ending on a synchronization;
 * restore_many: the staged windows, K11 passes and streams inflated again of
 * the latest hbx_restore_files_* call; match_push_bytes: the total bytes of
 * the result pushes of match batches (hbx_submit_device_match,
 * hbx_store_paths_match) since the context was created.  No reference
 * counterpart: diagnostics. */
int hbx_knobs(hbx_ctx *ctx, char *out, uint64_t cap);

/* Device time (ms) of the last completed batch per stage:
 * [0] K1 window-digest scan, [1] K2 cut chain, [2] K2 end -> results ready
 * (the batch's share of the pipelined MD5 launches, K4 and the copy),
 * [3] 0, [4] whole batch.  For a synchronous call [2] is the plan and K3
 * and [3] is K4 + the result copy. */
int hbx_stage_times(hbx_ctx *ctx, float ms[5]);
/* Cumulative device time (ms) and launch count per kernel since the context
 * was created (or last reset), for completed launches (K3 launches are timed
 * on the device and counted once known complete: after the wait that
 * collects a batch they finished, or once the hash stream is idle):
 * [0] K1 scan, [1] K2 cut chain, [2] K2c chain plan, [3] K3 block MD5,
 * [4] K4 content id.  reset != 0 zeroes the totals after reading. */
int hbx_stage_totals(hbx_ctx *ctx, double ms[5], uint64_t launches[5], int reset);
/* Diagnostics: turn the per-wave K3 records below on (on != 0) or off.
 * Changes no result and no other knob.  Fails with HBX_ERR_STATE while
 * batches are pending. */
int hbx_set_k3_probe(hbx_ctx *ctx, int on);
/* Diagnostics: with the probe on (hbx_set_k3_probe),
 * every K3 launch records per wave {start, end of its start-up (first
 * group's loads and prologue block) | XCC id << 56, end, R | max count << 16
 * | HW_ID << 32, s_memtime (shader cycles) at the start and the end of the
 * first group's cooperative phase, s_memrealtime at its end, the blocks of
 * each chain it hashed (R - 1) | the polls (s_sleep 1 each) in which the wave
 * found its producer's next stage not yet written, over the launch, << 32}
 * (times in s_memrealtime ticks, 100 MHz; R and
 * the count saturate at 65535; the last four are 0 for a wave whose first
 * group took the lane path).  Copies the latest launch's records (8 x u64 per
 * wave, up to max_waves) after the hash stream drains; *n_waves = waves per
 * launch. */
int hbx_k3_wave_times(hbx_ctx *ctx, uint64_t *out, uint32_t max_waves, uint32_t *n_waves);
/* Diagnostics: the slice summaries K1 stored for the context's most recent
 * synchronous device batch (hbx_chunk_hash_device, hbx_chunk_hash_batch and
 * hbx_chunk_hash through it), copied from device memory.  K1 summarises every
 * 4,096 window positions of a file that has split candidates: a file of
 * len > 2 * HBX_MIN_BLOCK_SIZE has ceil(len / 4096) slices, any other file
 * none.  first[f] / count[f] (max_files entries each): file f's first slice
 * and its slice count in `pairs`, in the batch's file order.  pairs
 * (2 x uint32 per slice, max_slices slices): for slice j of a file, D(q) the
 * window digest of the 65,536 bytes ending at file position q (virtual zero
 * bytes before the file start),
 *   word 0  smax  = max D(q) over q in [4096 j, min(4096 (j + 1), len)),
 *   word 1  sprev = D(4096 j - 1), the digest K2 starts a re-scan of the
 *                   slice from; 0x80000000 for j == 0 (no byte rolled in).
 * *n_files and *n_slices are always set to the batch's counts.  The slot K1
 * gives the slices past a file's end is not returned.  HBX_ERR_CAPACITY if
 * max_files or max_slices is smaller than those counts (nothing copied; both
 * may be 0 with null arrays to ask for the counts), HBX_ERR_STATE while
 * batches are pending, before any synchronous batch has run, and once a
 * later submit of any kind or hbx_reserve / hbx_apply_plan may have reused
 * the summaries' memory; HBX_ERR_ARG for a null ctx, n_files or n_slices, or
 * a null array with a non-zero capacity.  Changes no result and no knob. */
int hbx_k1_summaries(hbx_ctx *ctx, uint64_t *first, uint64_t *count, uint64_t max_files, uint64_t *n_files,
                     uint32_t *pairs, uint64_t max_slices, uint64_t *n_slices);
/* Tile length of K1 in 64 KiB iterations, 1..1024; 0 (the default) sizes
 * tiles per batch: about two per CU, 16..256 iterations (1-16 MiB). */
int hbx_set_tile_iters(hbx_ctx *ctx, uint32_t iters);
/* Pipeline join lag, 1..4 (default 1): a batch's chains join the block-MD5
 * launch issued `lag` submits after it, so its cut stage (K1 scan + K2 cut
 * chain) has `lag` pipeline steps to finish before the hash stage needs it.
 * Lag 2 suits small batches, whose scan is latency- rather than
 * throughput-bound.  Results are identical for every setting; a batch is
 * complete `lag` - 1 launches later.  Fails with HBX_ERR_STATE while batches
 * are pending. */
int hbx_set_join_lag(hbx_ctx *ctx, uint32_t lag);
/* K3 period, 1..8 (default 1): one block-MD5 launch every `period` submits,
 * advancing every chain by `period` x the slice (hbx_set_md5_slice) and
 * joining every batch that is `lag` or more submits old (up to 8).  Each
 * launch has a fixed start-up and a tail (its slowest CU); a period > 1 pays
 * them once per `period` steps, which pays off for small batches (a rank's
 * 1 GiB share of configs[2] at N = 8).  Results are identical for every
 * setting; a batch completes up to `period` - 1 submits later.  Fails with
 * HBX_ERR_STATE while batches are pending. */
int hbx_set_k3_period(hbx_ctx *ctx, uint32_t period);

/* ---- Pipeline operating point ---------------------------------------------
 * Hashback calls storeFile once per file from its tree walk
 * (hashback/store.go:356 -> :84); a caller that batches those files for
 * hbx_submit_device reaches the engine's measured rate only with the
 * schedule below: R batches resident in device memory,
 * each MD5 launch advancing every chain by the slice, a join lag of 2, a
 * lead of 2 (3 below 64 files per batch) and, below 32 files per batch, one MD5
 * launch every 4 submits.
 * hbx_plan_pipeline computes that schedule (bench.py runs exactly this plan)
 * and hbx_apply_plan sets it on a context.  Request fields <= 0 (md5_slice:
 * < 0) are "auto"; a positive value overrides that knob. */
#define HBX_PLAN_HOST_INPUT 1u /* each batch is copied in from host memory per step: shallow pipeline */
#define HBX_PLAN_ARENA_SLACK (64ull << 20) /* planned per resident arena beyond its bytes (allocator rounding) */
typedef struct {
  uint64_t n_files;          /* files per batch on this device */
  uint64_t arena_bytes;      /* one batch's arena: last offset + last length + HBX_ARENA_SLACK (or more) */
  uint64_t longest_file;     /* bytes of the batch's longest file (its longest MD5 chain: min(this, 8 MiB)) */
  uint64_t free_bytes;       /* device memory to plan for; 0 = the context's device, free now */
  double hbm_frac;           /* share of free_bytes for resident arenas (<= 0: 0.95) */
  uint32_t ranks_per_device; /* processes sharing the device's memory (0: 1) */
  uint32_t steps;            /* submits the caller runs between drains (0: open-ended); an auto
                                period divides it */
  int32_t arenas;            /* resident batches R (<= 0: as many as hbm_frac of free_bytes holds) */
  int32_t md5_slice;         /* blocks per chain per submit (< 0: sized from R; 0: unlimited) */
  int32_t join_lag;          /* 1..4 (<= 0: 2) */
  int32_t lead;              /* steps an arena stays resident beyond its batch's launches (< 0: the join lag
                                at 64 or more files per batch with device input, else lag + 1) */
  int32_t k3_period;         /* 1..8 (<= 0: 4, or 2 if 4 does not divide steps, below 32 files; else 1) */
  uint32_t flags;            /* HBX_PLAN_HOST_INPUT */
} hbx_plan_request;
typedef struct {
  uint32_t resident;           /* R: batches in flight, one device arena each */
  uint32_t md5_slice;          /* for hbx_set_md5_slice (blocks per chain per submit; 0 = unlimited) */
  uint32_t join_lag;           /* for hbx_set_join_lag */
  uint32_t lead;               /* the arena of batch j is refilled for batch j + R (hbx_input_after_oldest) */
  uint32_t k3_period;          /* for hbx_set_k3_period */
  uint32_t launches_per_batch; /* MD5 launches a batch's longest chain needs */
  uint64_t hbm_bytes;          /* R x (arena_bytes + HBX_PLAN_ARENA_SLACK) */
} hbx_pipeline_plan;
/* Fill *plan from *req.  ctx may be NULL when req->free_bytes > 0 (pure
 * host arithmetic, no device call).  HBX_ERR_ARG for an impossible request
 * (no files, a knob out of range, or R too small for the launches a batch
 * needs: then hbx_last_error(ctx) says which; with ctx NULL,
 * hbx_last_error(NULL) describes the calling thread's last such failure). */
int hbx_plan_pipeline(hbx_ctx *ctx, const hbx_plan_request *req, hbx_pipeline_plan *plan);
/* Set the plan's slice, join lag and period on ctx and reserve R + 2 batches
 * of up to `files` files and `bytes` bytes (hbx_reserve).  The caller keeps R
 * arenas and, from the (R+1)-th submit on, calls hbx_input_after_oldest
 * before refilling the oldest one.  HBX_ERR_STATE while batches are pending. */
int hbx_apply_plan(hbx_ctx *ctx, const hbx_pipeline_plan *plan, uint64_t files, uint64_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* HBXGPU_H */
