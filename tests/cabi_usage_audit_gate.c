/* A plain C99 translation unit that gates a result the way a shim does now ("the audit gate"): solve over a handle, then ONE call, ksh_audit_gate,
 * with all six passes and no findings table -- the plain yes/no gate: act iff n_findings == 0.  Then the form for a result from anywhere: the result's arrays
 * (ksh_result_arrays_get) and its commit numbers, read through ksh_placement_rows (KS_PLC_STAGE_SEQ), gated as CLAIMED -- clean --, and once more with pod argv[2],
 * a pod under a hostname spread, claimed on existing node argv[3], later than the node whose count still admits it: the gate lists exactly one finding, the sixth
 * pass's, on that pod, and the sixth pass's own call says the same about its row.  Last a table of one record where two are found, and the refusals.
 * Compiled and run by tests/test_audit_gate_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: cabi_usage_audit_gate <problem.ksp> <pod> <existing node>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const uint32_t pod = (uint32_t)atoi(argv[2]); const int32_t node = (int32_t)atoi(argv[3]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the gate: one call, one struct per requested pass for its totals, no table */
  ksh_audit_out a; ksh_audit_topology_out t; ksh_audit_spread_out s; ksh_audit_firstfit_out ff; ksh_audit_limits_out lm; ksh_audit_hostfit_out hf;
  ksh_audit_gate_out g; memset(&g, 0, sizeof g);
  g.audit = &a; g.topology = &t; g.spread = &s; g.firstfit = &ff; g.limits = &lm; g.hostfit = &hf;
  double ms[2];
  if (ksh_audit_gate(&h, 1, KS_AUDIT_PASS_ALL, &g, ms) != KS_OK) { fprintf(stderr, "ksh_audit_gate: %s\n", ksh_last_error()); return 1; }
  printf("genuine: %u findings, truncated %u -> %s\n", g.n_findings, g.truncated, g.n_findings ? "solve in Go" : "act");
  printf("totals: %u pods, %u nodes, %u + %u + %u + %u + %u + %u pods and %u + %u nodes flagged\n", a.n_pods, a.n_nodes, a.n_pods_flagged, t.n_pods_flagged, s.n_pods_flagged,
         ff.n_pods_flagged, lm.n_pods_flagged, hf.n_pods_flagged, a.n_nodes_flagged, lm.n_nodes_flagged);
  printf("the fourth pass examined %u pods, the sixth %u: %u pairs, %u count tests, %u pairs admitting\n", ff.checked[1], hf.checked[1], hf.checked[2], hf.checked[3], hf.admitting_pairs);
  const uint32_t P = a.n_pods;
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

  ks_audit_finding found[4]; memset(found, 0xEE, sizeof found);
  g.findings = found; g.cap_findings = 4;
  if (ksh_audit_gate_claimed(h, &ra, seq, KS_AUDIT_PASS_ALL, &g, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u rows, %u findings, truncated %u\n", (unsigned)total, g.n_findings, g.truncated);
  int32_t* where = (int32_t*)take(4 * (size_t)P);
  memcpy(where, ra.pod_node, 4 * (size_t)P);
  const int32_t was = where[pod];
  where[pod] = node; ra.pod_node = where;
  if (ksh_audit_gate_claimed(h, &ra, seq, KS_AUDIT_PASS_ALL, &g, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate_claimed: %s\n", ksh_last_error()); return 1; }
  printf("pod %u claimed on node %d instead of %d: %u findings, truncated %u -> %s\n", pod, node, was, g.n_findings, g.truncated, g.n_findings ? "solve in Go" : "act");
  for (k = 0; k < g.n_findings && k < g.cap_findings; ++k)
    printf("finding %u: problem %u, pass %u, table %u, index %u, flags %u\n", (unsigned)k, found[k].problem, found[k].where >> 8, found[k].where & 255u, found[k].index, found[k].flags);
  printf("the record behind them untouched: %d\n", g.n_findings < 4 && found[g.n_findings].problem == 0xEEEEEEEEu);
  /* the rows remain the per-pass calls': the sixth pass alone, with its table */
  ksh_audit_hostfit_out own; memset(&own, 0, sizeof own);
  own.pod_flags = (uint32_t*)take(4 * (size_t)P); own.cap_pods = P;
  if (ksh_audit_hostfit_claimed(h, &ra, seq, &own, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_hostfit_claimed: %s\n", ksh_last_error()); return 1; }
  printf("the sixth pass's own call: %u pods flagged, the pod carries %u; the gate's totals say %u\n", own.n_pods_flagged, own.pod_flags[pod], hf.n_pods_flagged);

  /* a second pod moved as well, and a table of one record: the count is whole, the table holds the first */
  where[(pod + 1) % P] = node;
  memset(found, 0xEE, sizeof found); g.cap_findings = 1;
  if (ksh_audit_gate_claimed(h, &ra, seq, KS_AUDIT_PASS_HOSTFIT, &g, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate_claimed: %s\n", ksh_last_error()); return 1; }
  printf("two pods moved, a table of one: %u findings, truncated %u, the first on pod %u, the second record untouched: %d\n", g.n_findings, g.truncated, found[0].index, found[1].problem == 0xEEEEEEEEu);

  printf("no commit numbers: %d\n", ksh_audit_gate_claimed(h, &ra, NULL, KS_AUDIT_PASS_ALL, &g, NULL));      /* KS_ERR_INVALID */
  printf("no pass: %d\n", ksh_audit_gate(&h, 1, 0, &g, NULL));                                                  /* KS_ERR_INVALID */
  g.findings = NULL; g.cap_findings = 4;
  printf("no table for four records: %d\n", ksh_audit_gate(&h, 1, KS_AUDIT_PASS_ALL, &g, NULL));                /* KS_ERR_INVALID */
  free(own.pod_flags); free(where); free(seq); free(rows);
  ksh_close(h); free(text);
  return 0;
}
