/* A plain C99 translation unit that checks a result's relaxation stages the way a shim would ("the audit gate"): solve over a handle, the gate
 * (ksh_audit_gate, all six passes, no findings table), ksh_audit_stages beside it, and act only if neither finds anything.  Then the form for a result from anywhere:
 * the result's arrays (ksh_result_arrays_get) and its commit numbers, read through ksh_placement_rows (KS_PLC_STAGE_SEQ), audited back as CLAIMED -- clean --, and once
 * more with pod argv[2], which sits at stage 0 with a preference that holds, claimed one stage on: the gate stays clean, exactly that pod carries
 * KS_AUDIT_POD_STAGE_*.  Compiled and run by tests/test_audit_stages_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: cabi_usage_audit_stages <problem.ksp> <pod>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const uint32_t pod = (uint32_t)atoi(argv[2]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the gate, and the seventh pass beside it: totals always; the flag rows only when the table holds them */
  ksh_audit_out a; ksh_audit_topology_out t; ksh_audit_spread_out s; ksh_audit_firstfit_out ff; ksh_audit_limits_out l; ksh_audit_hostfit_out hf;
  memset(&a, 0, sizeof a); memset(&t, 0, sizeof t); memset(&s, 0, sizeof s); memset(&ff, 0, sizeof ff); memset(&l, 0, sizeof l); memset(&hf, 0, sizeof hf);
  ksh_audit_gate_out g; memset(&g, 0, sizeof g);
  g.audit = &a; g.topology = &t; g.spread = &s; g.firstfit = &ff; g.limits = &l; g.hostfit = &hf;
  ksh_audit_stages_out st; memset(&st, 0, sizeof st);
  if (ksh_audit_gate(&h, 1, KS_AUDIT_PASS_ALL, &g, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_stages(&h, 1, &st, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_stages: %s\n", ksh_last_error()); return 1; }
  printf("genuine: gate %u findings, stages %u of %u pods flagged, truncated %u -> %s\n", g.n_findings, st.n_pods_flagged, st.n_pods, st.truncated, (g.n_findings || st.n_pods_flagged) ? "solve in Go" : "act");
  printf("evaluated: %u placed pods, %u pods with an examined stage, %u skipped, %u stages, %u pairs, %u of them admitting\n", st.checked[0], st.checked[1], st.skipped_pods, st.checked[2],
         st.checked[3], st.admitting_pairs);
  const uint32_t P = st.n_pods;
  if (pod >= P) return 2;

  /* the commit numbers of that result: one placement row per pod */
  uint64_t id = 7, head[KS_PLC_HEAD_WORDS], total = 0;
  uint64_t* rows = (uint64_t*)take(8 * (size_t)P * KS_PLC_ROW_WORDS);
  if (ksh_placement_rows(&h, 1, &id, head, rows, P, &total, NULL) != KS_OK) { fprintf(stderr, "ksh_placement_rows: %s\n", ksh_last_error()); return 1; }
  int32_t* seq = (int32_t*)take(4 * (size_t)P);
  uint64_t k;
  for (k = 0; k < P; ++k) seq[k] = -1;
  for (k = 0; k < total; ++k) {
    const uint64_t* row = rows + k * KS_PLC_ROW_WORDS;
    seq[(uint32_t)row[KS_PLC_POD_WHERE]] = (int32_t)(uint32_t)(row[KS_PLC_STAGE_SEQ] >> 32);
  }
  ksh_result_arrays ra;
  if (ksh_result_arrays_get(h, &ra) != KS_OK) { fprintf(stderr, "ksh_result_arrays_get: %s\n", ksh_last_error()); return 1; }

  st.pod_flags = (uint32_t*)take(4 * (size_t)P); st.cap_pods = P;
  if (ksh_audit_stages_claimed(h, &ra, seq, &st, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_stages_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u rows, %u pods flagged, truncated %u\n", (unsigned)total, st.n_pods_flagged, st.truncated);
  int32_t* stage = (int32_t*)take(4 * (size_t)P);
  memcpy(stage, ra.pod_stage, 4 * (size_t)P);
  const int32_t was = stage[pod];
  stage[pod] = was + 1; ra.pod_stage = stage;
  if (ksh_audit_gate_claimed(h, &ra, seq, KS_AUDIT_PASS_ALL, &g, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate_claimed: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_stages_claimed(h, &ra, seq, &st, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_stages_claimed: %s\n", ksh_last_error()); return 1; }
  printf("pod %u claimed at stage %d instead of %d: gate %u findings, stages %u pods flagged, the pod carries %u -> %s\n", pod, was + 1, was, g.n_findings, st.n_pods_flagged, st.pod_flags[pod],
         (g.n_findings || st.n_pods_flagged) ? "solve in Go" : "act");
  printf("no commit numbers: %d\n", ksh_audit_stages_claimed(h, &ra, NULL, &st, NULL));      /* KS_ERR_INVALID */
  free(stage); free(st.pod_flags); free(seq); free(rows);
  ksh_close(h); free(text);
  return 0;
}
