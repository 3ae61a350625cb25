/* A plain C99 translation unit that gates a result the way a shim would ("the audit gate"), with the six passes: solve over a handle, ksh_audit,
 * ksh_audit_topology, ksh_audit_spread, ksh_audit_firstfit, ksh_audit_limits, then ksh_audit_hostfit, and act only if none flags anything.  Then the form for a result
 * from anywhere: the result's arrays (ksh_result_arrays_get) and its commit numbers, read through ksh_placement_rows (KS_PLC_STAGE_SEQ), audited back as CLAIMED --
 * clean --, and once more with pod argv[2], a pod under a hostname spread, claimed on existing node argv[3], later than the node whose count still admits it: exactly
 * that pod carries KS_AUDIT_POD_HFIT_EXISTING.  Compiled and run by tests/test_audit_hostfit_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: cabi_usage_audit_hostfit <problem.ksp> <pod> <existing node>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const uint32_t pod = (uint32_t)atoi(argv[2]); const int32_t node = (int32_t)atoi(argv[3]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the gate: the six passes over the result where it lies.  Totals always; the flag rows only when the tables hold them */
  ksh_audit_out a; memset(&a, 0, sizeof a);
  ksh_audit_topology_out t; memset(&t, 0, sizeof t);
  ksh_audit_spread_out s; memset(&s, 0, sizeof s);
  ksh_audit_firstfit_out ff; memset(&ff, 0, sizeof ff);
  ksh_audit_limits_out lm; memset(&lm, 0, sizeof lm);
  ksh_audit_hostfit_out hf; memset(&hf, 0, sizeof hf);
  if (ksh_audit(&h, 1, &a, NULL) != KS_OK) { fprintf(stderr, "ksh_audit: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_topology(&h, 1, &t, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_topology: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_spread(&h, 1, &s, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_spread: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_firstfit(&h, 1, &ff, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_firstfit: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_limits(&h, 1, &lm, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_limits: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_hostfit(&h, 1, &hf, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_hostfit: %s\n", ksh_last_error()); return 1; }
  const unsigned found = a.n_pods_flagged + a.n_nodes_flagged + t.n_pods_flagged + s.n_pods_flagged + ff.n_pods_flagged + lm.n_pods_flagged + lm.n_nodes_flagged + hf.n_pods_flagged;
  printf("genuine: %u + %u + %u + %u + %u + %u of %u pods, %u nodes flagged, truncated %u -> %s\n", a.n_pods_flagged, t.n_pods_flagged, s.n_pods_flagged, ff.n_pods_flagged,
         lm.n_pods_flagged, hf.n_pods_flagged, hf.n_pods, a.n_nodes_flagged + lm.n_nodes_flagged, hf.truncated, found ? "solve in Go" : "act");
  printf("the fourth pass examined %u pods, the sixth %u\n", ff.checked[1], hf.checked[1]);
  printf("evaluated: %u placed pods, %u pods examined, %u skipped, %u eligible groups, %u skipped, %u pairs, %u count tests, %u pairs admitting\n", hf.checked[0], hf.checked[1],
         hf.skipped_pods, hf.eligible_groups, hf.skipped_groups, hf.checked[2], hf.checked[3], hf.admitting_pairs);
  const uint32_t P = hf.n_pods;
  if (pod >= P) return 2;

  /* the commit numbers of that result: one placement row per pod */
  uint64_t id = 7, head[KS_PLC_HEAD_WORDS], total = 0;
  uint64_t* rows = (uint64_t*)take(8 * (size_t)P * KS_PLC_ROW_WORDS);
  if (ksh_placement_rows(&h, 1, &id, head, rows, P, &total, NULL) != KS_OK) { fprintf(stderr, "ksh_placement_rows: %s\n", ksh_last_error()); return 1; }
  int32_t* seq = (int32_t*)take(4 * (size_t)P);
  uint64_t k;
  for (k = 0; k < total; ++k) {
    const uint64_t* row = rows + k * KS_PLC_ROW_WORDS;
    seq[(uint32_t)row[KS_PLC_POD_WHERE]] = (int32_t)(uint32_t)(row[KS_PLC_STAGE_SEQ] >> 32);
  }
  ksh_result_arrays ra;
  if (ksh_result_arrays_get(h, &ra) != KS_OK) { fprintf(stderr, "ksh_result_arrays_get: %s\n", ksh_last_error()); return 1; }

  hf.pod_flags = (uint32_t*)take(4 * (size_t)P); hf.cap_pods = P;
  if (ksh_audit_hostfit_claimed(h, &ra, seq, &hf, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_hostfit_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u rows, %u pods flagged, truncated %u\n", (unsigned)total, hf.n_pods_flagged, hf.truncated);
  int32_t* where = (int32_t*)take(4 * (size_t)P);
  memcpy(where, ra.pod_node, 4 * (size_t)P);
  const int32_t was = where[pod];
  where[pod] = node; ra.pod_node = where;
  if (ksh_audit_hostfit_claimed(h, &ra, seq, &hf, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_hostfit_claimed: %s\n", ksh_last_error()); return 1; }
  printf("pod %u claimed on node %d instead of %d: %u pods flagged, the pod carries %u -> %s\n", pod, node, was, hf.n_pods_flagged, hf.pod_flags[pod], hf.n_pods_flagged ? "solve in Go" : "act");
  printf("no commit numbers: %d\n", ksh_audit_hostfit_claimed(h, &ra, NULL, &hf, NULL));      /* KS_ERR_INVALID */
  free(where); free(hf.pod_flags); free(seq); free(rows);
  ksh_close(h); free(text);
  return 0;
}
