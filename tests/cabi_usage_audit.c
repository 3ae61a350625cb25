/* A plain C99 translation unit that gates a result the way a shim would ("the audit gate"): solve, audit the result where it lies on the device,
 * act only if nothing is flagged; then audit a result it CLAIMS -- the same arrays with one placed pod also listed as unscheduled -- and find exactly that; then
 * the same gate one layer up, over a libkshost handle.  Compiled and run by tests/test_audit_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: cabi_usage_audit <problem.ksp>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  const ks_problem* p = ksh_problem(h);
  const size_t P = p->P, N = p->max_new_nodes, TW = KS_TW(p), R = p->R, K = p->K;

  ks_result r; memset(&r, 0, sizeof r);
  r.pod_node = (int32_t*)take(4 * P); r.pod_stage = (int32_t*)take(4 * P); r.pod_seq = (int32_t*)take(4 * P); r.pod_reason = (uint32_t*)take(4 * P); r.unscheduled = (int32_t*)take(4 * P);
  r.node_tmpl = (int32_t*)take(4 * N); r.node_types = (uint64_t*)take(8 * N * TW); r.node_requests = (int64_t*)take(8 * N * R); r.node_requests_present = (uint32_t*)take(4 * N);
  r.node_present = (uint32_t*)take(4 * N); r.node_complement = (uint32_t*)take(4 * N); r.node_mask = (uint64_t*)take(8 * N * K); r.node_gt = (int32_t*)take(4 * N * K);
  r.node_lt = (int32_t*)take(4 * N * K); r.node_it_state = (int32_t*)take(4 * N);

  ks_dev_problem* d = NULL;
  int rc = ks_problem_upload(p, 0, &d);
  if (rc != KS_OK) { fprintf(stderr, "upload: %s\n", ks_last_error()); return 1; }

  /* the tables are the caller's: one word per pod, one per node the result can have */
  ks_audit a; memset(&a, 0, sizeof a);
  a.pod_flags = (uint32_t*)take(4 * P); a.node_flags = (uint32_t*)take(4 * ((size_t)p->E + N));
  rc = ks_audit_dev(d, NULL, &a);
  printf("before a solve: %d\n", rc);                                   /* KS_ERR_INVALID: nothing to audit */

  if (ks_solve_dev(d, &r, NULL) != KS_OK) { fprintf(stderr, "solve: %s\n", ks_last_error()); return 1; }
  if (ks_audit_dev(d, NULL, &a) != KS_OK) { fprintf(stderr, "audit: %s\n", ks_last_error()); return 1; }
  printf("genuine: %u of %u pods, %u of %u nodes flagged -> %s\n", a.n_pods_flagged, a.n_pods, a.n_nodes_flagged, a.n_nodes, (a.n_pods_flagged || a.n_nodes_flagged) ? "solve in Go" : "act");

  /* a result from anywhere: here the same one, with the first placed pod listed as unscheduled too */
  uint32_t i, victim = 0;
  for (i = 0; i < p->P; ++i) if (r.pod_node[i] >= 0) { victim = i; break; }
  r.unscheduled[r.n_unscheduled++] = (int32_t)victim;
  if (ks_audit_dev(d, &r, &a) != KS_OK) { fprintf(stderr, "audit (claimed): %s\n", ks_last_error()); return 1; }
  printf("claimed: %u pods flagged, pod %u carries %u (%u with KS_AUDIT_POD_UNSCHEDULED_LIST), %u nodes flagged -> %s\n", a.n_pods_flagged, victim, a.pod_flags[victim],
         a.pod_bit_count[1], a.n_nodes_flagged, (a.n_pods_flagged || a.n_nodes_flagged) ? "solve in Go" : "act");
  r.n_new = p->max_new_nodes + 1;
  printf("too many nodes claimed: %d\n", ks_audit_dev(d, &r, &a));      /* KS_ERR_INVALID */
  ks_problem_free(d);

  /* one layer up: the handle solves, ksh_audit gates.  Totals always; the flag rows only when the tables hold them */
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }
  ksh_audit_out o; memset(&o, 0, sizeof o);
  double ms[2];
  if (ksh_audit(&h, 1, &o, ms) != KS_OK) { fprintf(stderr, "ksh_audit: %s\n", ksh_last_error()); return 1; }
  printf("handle, totals only: %u pods %u nodes, %u + %u flagged, truncated %u\n", o.n_pods, o.n_nodes, o.n_pods_flagged, o.n_nodes_flagged, o.truncated);
  o.pod_flags = (uint32_t*)take(4 * (size_t)o.n_pods); o.cap_pods = o.n_pods; o.node_flags = (uint32_t*)take(4 * (size_t)o.n_nodes); o.cap_nodes = o.n_nodes;
  if (ksh_audit(&h, 1, &o, ms) != KS_OK) { fprintf(stderr, "ksh_audit: %s\n", ksh_last_error()); return 1; }
  printf("handle, with tables: truncated %u, %u + %u flagged\n", o.truncated, o.n_pods_flagged, o.n_nodes_flagged);
  free(o.pod_flags); free(o.node_flags); free(a.pod_flags); free(a.node_flags);
  ksh_close(h); free(text);
  return 0;
}
