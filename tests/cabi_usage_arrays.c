/* A plain C99 translation unit that walks a flat problem it did not build, the way a caller who fills ks_problem by hand can check its own lengths
 * (INTEGRATION.md section 2): ks_debug_problem_array names every array of the struct with its element size, the length the problem states for it and where its
 * pointer sits.  The program copies every array into a malloc'ed buffer of EXACTLY that length -- an array of no elements becomes NULL --, uploads the copy and
 * the original, solves both and compares the results.  Run under AddressSanitizer (emulator build of the libraries), a read past a stated length is a report.
 * Compiled and run by tests/test_problem_arrays.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

typedef struct { ks_result r; void* mem[15]; } result_buf;

static void* take(result_buf* b, int slot, size_t bytes) { b->mem[slot] = malloc(bytes ? bytes : 1); return b->mem[slot]; }
static void result_alloc(result_buf* b, const ks_problem* p) {
  const size_t P = p->P, N = p->max_new_nodes, TW = KS_TW(p), R = p->R, K = p->K;
  memset(b, 0, sizeof *b);
  b->r.pod_node = (int32_t*)take(b, 0, 4 * P); b->r.pod_stage = (int32_t*)take(b, 1, 4 * P); b->r.pod_seq = (int32_t*)take(b, 2, 4 * P);
  b->r.pod_reason = (uint32_t*)take(b, 3, 4 * P); b->r.unscheduled = (int32_t*)take(b, 4, 4 * P); b->r.node_tmpl = (int32_t*)take(b, 5, 4 * N);
  b->r.node_types = (uint64_t*)take(b, 6, 8 * N * TW); b->r.node_requests = (int64_t*)take(b, 7, 8 * N * R); b->r.node_requests_present = (uint32_t*)take(b, 8, 4 * N);
  b->r.node_present = (uint32_t*)take(b, 9, 4 * N); b->r.node_complement = (uint32_t*)take(b, 10, 4 * N); b->r.node_mask = (uint64_t*)take(b, 11, 8 * N * K);
  b->r.node_gt = (int32_t*)take(b, 12, 4 * N * K); b->r.node_lt = (int32_t*)take(b, 13, 4 * N * K); b->r.node_it_state = (int32_t*)take(b, 14, 4 * N);
}
static void result_free(result_buf* b) { int i; for (i = 0; i < 15; ++i) free(b->mem[i]); }

/* upload + solve + free; 1 if a device took it, 0 if the upload was refused for want of one, -1 on any other failure */
static int solve(const ks_problem* p, result_buf* out) {
  ks_dev_problem* d = NULL;
  int rc = ks_problem_upload(p, 0, &d);
  if (rc == KS_ERR_DEVICE) { printf("upload refused: %d\n", rc); return 0; }
  if (rc != KS_OK) { fprintf(stderr, "upload: %s\n", ks_last_error()); return -1; }
  rc = ks_solve_dev(d, &out->r, NULL);
  ks_problem_free(d);
  if (rc != KS_OK) { fprintf(stderr, "solve: %s\n", ks_last_error()); return -1; }
  return 1;
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: cabi_usage_arrays <problem.ksp>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  const ks_problem* p = ksh_problem(h);

  /* the copy: the scalars as they are, every array an exact-length buffer of its own */
  ks_problem q = *p;
  const uint32_t rows = ks_debug_problem_array(p, 0, NULL, NULL, NULL, NULL, NULL);
  void** bufs = (void**)calloc(rows, sizeof(void*));
  uint32_t i, arrays = 0, unhashed = 0; size_t bytes = 0;
  for (i = 0; i < rows; ++i) {
    const char* name = NULL; uint32_t elem = 0, off = 0, marks = 0; uint64_t count = 0; const void* src = NULL;
    ks_debug_problem_array(p, i, &name, &elem, &count, &off, &marks);
    if (off % sizeof(void*) || off + sizeof(void*) > sizeof(ks_problem)) { fprintf(stderr, "%s: pointer at %u is outside ks_problem\n", name, off); return 1; }
    memcpy(&src, (const char*)p + off, sizeof src);
    if (!src && count && !(marks & KS_ARRAY_NULLABLE)) { fprintf(stderr, "%s: NULL with %lu elements\n", name, (unsigned long)count); return 1; }
    if (src && count) { bufs[i] = malloc((size_t)count * elem); memcpy(bufs[i], src, (size_t)count * elem); ++arrays; bytes += (size_t)count * elem; }
    memcpy((char*)&q + off, &bufs[i], sizeof(void*));
    if (marks & KS_ARRAY_NOT_FINGERPRINTED) ++unhashed;
  }
  printf("rows %u (%u not fingerprinted), %u arrays with elements, %lu bytes\n", rows, unhashed, arrays, (unsigned long)bytes);

  result_buf a, b; result_alloc(&a, p); result_alloc(&b, p);
  const int ra = solve(p, &a), rb = ra > 0 ? solve(&q, &b) : ra;
  if (ra < 0 || rb < 0) return 1;
  if (ra > 0) {
    const size_t N = a.r.n_new;
    if (a.r.n_new != b.r.n_new || a.r.n_unscheduled != b.r.n_unscheduled || memcmp(a.r.pod_node, b.r.pod_node, 4 * (size_t)p->P) || memcmp(a.r.pod_stage, b.r.pod_stage, 4 * (size_t)p->P) ||
        memcmp(a.r.node_tmpl, b.r.node_tmpl, 4 * N) || memcmp(a.r.node_types, b.r.node_types, 8 * N * KS_TW(p)) || memcmp(a.r.node_requests, b.r.node_requests, 8 * N * p->R)) {
      fprintf(stderr, "the exact-length copy solved differently\n"); return 1;
    }
    printf("exact-length copy: the same result, %u pods, %u new nodes, %u unscheduled\n", p->P, a.r.n_new, a.r.n_unscheduled);
  }
  result_free(&a); result_free(&b);
  for (i = 0; i < rows; ++i) free(bufs[i]);
  free(bufs); ksh_close(h); free(text);
  return 0;
}
