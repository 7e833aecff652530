/* Plain-C threaded caller of libhbxgpu.so: pthreads and include/hbxgpu.h only,
 * the way cgo would call the library from goroutines.  It pins the threading
 * contract of hbxgpu.h ("a context is safe to call from many threads;
 * distinct contexts run concurrently") where the Python binding cannot: two
 * threads inside ONE context's pipeline.
 *
 *   (a) producer / consumer on one context: thread 1 calls hbx_submit_device
 *       for K batches, each with output arrays of its own, held to
 *       OUTSTANDING batches in flight by a semaphore; thread 2 calls hbx_wait
 *       K times, one per submit posted.  Right after the i-th wait returns it
 *       snapshots batch i's arrays (all arrays start as 0xEE): the i-th wait
 *       must have filled batch i, FIFO across threads.
 *   (b) two such pairs on two contexts at once.
 *
 * Batch i of pair p is ONE file: the bytes [off, off + len) of the input file
 * (batch_span below; tests/test_gpu_threads.py cuts the same spans for the
 * oracle).  Test infrastructure: tests/test_abi.py builds it and runs the
 * no-device mode, tests/test_gpu_threads.py compares its lines.
 *
 * usage: abi_threads <file> [--expect-nodev]
 * prints "<phase> ctx <p> batch <i>: <cut end> <32 hex digits>" per chunk,
 * "<phase> ctx <p> batch <i>= <content type> <hex> <n chunks>" per batch, then
 * "ok"; exits non-zero on any non-zero status. */
#define _POSIX_C_SOURCE 200809L
#include <pthread.h>
#include <semaphore.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include "hbxgpu.h"

enum { K = 24, OUTSTANDING = 4, SPAN_STEP = 65552 /* 16 x 4097 */ };

/* Where batch i of pair p lies in the input (offset a multiple of
 * HBX_ARENA_ALIGN): pair 0 walks the file forwards, pair 1 backwards with
 * other lengths, so no two batches of a run are the same bytes. */
static void batch_span(int pair, int i, uint64_t *off, uint64_t *len) {
  if (pair == 0) {
    *off = (uint64_t)i * SPAN_STEP;
    *len = 200000u + 4099u * (uint64_t)i;
  } else {
    *off = (uint64_t)(K - 1 - i) * SPAN_STEP + 32;
    *len = 150001u + 8191u * (uint64_t)i;
  }
}

typedef struct {
  uint64_t off, len, base, cap; /* hbx_submit_device's per-file arrays: alive until the wait */
  uint64_t *cuts;               /* pinned, cap entries */
  uint8_t *ids;                 /* pinned, 16 cap bytes */
  hbx_file_summary *sum;        /* pinned */
  void *pin;
  /* the consumer's snapshot, taken right after this batch's wait returned */
  uint64_t *got_cuts;
  uint8_t *got_ids;
  hbx_file_summary got_sum;
} batch_t;

typedef struct {
  int pair;
  hbx_ctx *ctx;
  void *arena;
  batch_t b[K];
  sem_t slots, items;
} pair_t;

static void die(const char *what, int rc, hbx_ctx *ctx) {
  fprintf(stderr, "%s failed: %d %s\n", what, rc, ctx ? hbx_last_error(ctx) : "");
  fflush(NULL);
  _exit(1); /* no further GPU work, and no destructors under the other threads */
}

static void *producer(void *arg) {
  pair_t *p = arg;
  for (int i = 0; i < K; i++) {
    batch_t *b = &p->b[i];
    sem_wait(&p->slots);
    const int rc = hbx_submit_device(p->ctx, p->arena, 1, &b->off, &b->len, b->cuts, b->ids, &b->base, &b->cap, b->sum);
    if (rc != HBX_OK) die("hbx_submit_device", rc, p->ctx);
    sem_post(&p->items);
  }
  return NULL;
}

static void *consumer(void *arg) {
  pair_t *p = arg;
  for (int i = 0; i < K; i++) {
    batch_t *b = &p->b[i];
    sem_wait(&p->items);
    const int rc = hbx_wait(p->ctx);
    if (rc != HBX_OK) die("hbx_wait", rc, p->ctx);
    memcpy(b->got_cuts, b->cuts, b->cap * 8);
    memcpy(b->got_ids, b->ids, b->cap * 16);
    b->got_sum = *b->sum;
    sem_post(&p->slots);
  }
  return NULL;
}

static void pair_open(pair_t *p, int pair, const uint8_t *data, uint64_t n) {
  int rc;
  memset(p, 0, sizeof *p);
  p->pair = pair;
  if ((rc = hbx_ctx_create(0, &p->ctx)) != HBX_OK) die("hbx_ctx_create", rc, NULL);
  if ((rc = hbx_set_join_lag(p->ctx, pair ? 1 : 2)) != HBX_OK) die("hbx_set_join_lag", rc, p->ctx);
  if ((rc = hbx_set_md5_slice(p->ctx, pair ? 512 : 256)) != HBX_OK) die("hbx_set_md5_slice", rc, p->ctx);
  if ((rc = hbx_arena_alloc(p->ctx, n, &p->arena)) != HBX_OK) die("hbx_arena_alloc", rc, p->ctx);
  if ((rc = hbx_memcpy_h2d(p->ctx, p->arena, data, n)) != HBX_OK) die("hbx_memcpy_h2d", rc, p->ctx);
  sem_init(&p->slots, 0, OUTSTANDING);
  sem_init(&p->items, 0, 0);
  for (int i = 0; i < K; i++) {
    batch_t *b = &p->b[i];
    batch_span(pair, i, &b->off, &b->len);
    if (b->off + b->len > n) die("input file too short for the batch spans", 0, NULL);
    b->base = 0;
    b->cap = hbx_max_chunks(b->len);
    const size_t need = b->cap * 24 + sizeof(hbx_file_summary);
    if ((rc = hbx_alloc_pinned(need, &b->pin)) != HBX_OK) die("hbx_alloc_pinned", rc, p->ctx);
    memset(b->pin, 0xEE, need);
    b->cuts = (uint64_t *)b->pin;
    b->ids = (uint8_t *)(b->cuts + b->cap);
    b->sum = (hbx_file_summary *)(b->ids + 16 * b->cap);
    b->got_cuts = calloc(b->cap, 8);
    b->got_ids = calloc(b->cap, 16);
  }
}

static void pair_report(pair_t *p, const char *phase) {
  char h[33];
  for (int i = 0; i < K; i++) {
    batch_t *b = &p->b[i];
    uint64_t k = b->got_sum.n_chunks;
    if (k > b->cap) k = 0; /* an unfilled summary (0xEE..): the "=" line below shows it */
    for (uint64_t q = 0; q < k; q++) {
      for (int j = 0; j < 16; j++) sprintf(h + 2 * j, "%02x", b->got_ids[16 * q + j]);
      printf("%s ctx %d batch %d: %llu %s\n", phase, p->pair, i, (unsigned long long)b->got_cuts[q], h);
    }
    for (int j = 0; j < 16; j++) sprintf(h + 2 * j, "%02x", b->got_sum.content_id[j]);
    printf("%s ctx %d batch %d= %d %s %u\n", phase, p->pair, i, b->got_sum.content_type, h, b->got_sum.n_chunks);
  }
}

static void pair_close(pair_t *p) {
  if (hbx_pending(p->ctx) != 0) die("hbx_pending after the last wait", hbx_pending(p->ctx), p->ctx);
  for (int i = 0; i < K; i++) {
    hbx_free_pinned(p->b[i].pin);
    free(p->b[i].got_cuts);
    free(p->b[i].got_ids);
  }
  hbx_arena_free(p->ctx, p->arena);
  hbx_ctx_destroy(p->ctx);
  sem_destroy(&p->slots);
  sem_destroy(&p->items);
}

static void run_pairs(pair_t *ps, int n_pairs, const char *phase) {
  pthread_t t[4];
  for (int i = 0; i < n_pairs; i++) {
    if (pthread_create(&t[2 * i], NULL, producer, &ps[i]) || pthread_create(&t[2 * i + 1], NULL, consumer, &ps[i]))
      die("pthread_create", 0, NULL);
  }
  for (int i = 0; i < 2 * n_pairs; i++) pthread_join(t[i], NULL);
  for (int i = 0; i < n_pairs; i++) pair_report(&ps[i], phase);
}

/* ---- without a GPU: every call reports from every thread, and the text of
 * hbx_last_error(NULL) belongs to the calling thread ---- */
typedef struct {
  int which, bad;
  pthread_barrier_t *bar;
} nodev_t;

static void *nodev_thread(void *arg) {
  nodev_t *a = arg;
  const char *want = a->which ? "K3 period" : "join lag", *other = a->which ? "join lag" : "K3 period";
  for (int r = 0; r < 200; r++) { /* (no early exit: the other thread waits at the barrier) */
    hbx_plan_request q;
    hbx_pipeline_plan pl;
    memset(&q, 0, sizeof q);
    q.n_files = 8;
    q.arena_bytes = q.longest_file = 1u << 20;
    q.free_bytes = 1ull << 30;
    if (a->which) q.k3_period = 99;
    else q.join_lag = 9;
    if (hbx_plan_pipeline(NULL, &q, &pl) != HBX_ERR_ARG) a->bad = 1;
    pthread_barrier_wait(a->bar); /* both threads have failed before either reads */
    const char *m = hbx_last_error(NULL);
    if (!strstr(m, want) || strstr(m, other)) a->bad = 2;
    pthread_barrier_wait(a->bar);
    hbx_ctx *ctx = NULL;
    if (hbx_ctx_create(0, &ctx) != HBX_ERR_NODEV || ctx) a->bad = 3;
    if (hbx_wait(NULL) != HBX_ERR_ARG || hbx_pending(NULL) != HBX_ERR_ARG) a->bad = 4;
    if (hbx_submit_device(NULL, NULL, 0, NULL, NULL, NULL, NULL, NULL, NULL, NULL) != HBX_ERR_ARG) a->bad = 5;
  }
  return NULL;
}

static int nodev(void) {
  int nd = -1;
  if (hbx_device_count(&nd) != HBX_ERR_NODEV || nd != 0) return 3;
  pthread_barrier_t bar;
  pthread_barrier_init(&bar, NULL, 2);
  nodev_t a[2] = {{0, 0, &bar}, {1, 0, &bar}};
  pthread_t t[2];
  for (int i = 0; i < 2; i++)
    if (pthread_create(&t[i], NULL, nodev_thread, &a[i])) return 4;
  for (int i = 0; i < 2; i++) pthread_join(t[i], NULL);
  pthread_barrier_destroy(&bar);
  if (a[0].bad || a[1].bad) return 10 + (a[0].bad ? a[0].bad : a[1].bad);
  printf("nodev ok\n");
  return 0;
}

int main(int argc, char **argv) {
  if (argc < 2) return 2;
  if (argc > 2 && strcmp(argv[2], "--expect-nodev") == 0) return nodev();

  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  fseek(f, 0, SEEK_END);
  const uint64_t n = (uint64_t)ftell(f);
  fseek(f, 0, SEEK_SET);
  uint8_t *data = malloc(n ? n : 1);
  if (n && fread(data, 1, n, f) != n) return 2;
  fclose(f);

  static pair_t ps[2];
  pair_open(&ps[0], 0, data, n);
  run_pairs(ps, 1, "a");
  pair_close(&ps[0]);

  pair_open(&ps[0], 0, data, n);
  pair_open(&ps[1], 1, data, n);
  run_pairs(ps, 2, "b");
  pair_close(&ps[0]);
  pair_close(&ps[1]);
  free(data);
  printf("ok\n");
  return 0;
}
