/* A plain C99 translation unit that gates a result the way a shim does now ("the audit gate"): solve over a handle, then ONE call, ksh_audit_gate_ex,
 * with all EIGHT passes and no findings table -- the plain yes/no gate: act iff n_findings == 0.  Then the form for a result from anywhere: the result's arrays
 * (ksh_result_arrays_get, pod_reason among them) and its commit numbers, read through ksh_placement_rows, gated as CLAIMED -- clean --; once more with pod argv[2],
 * a pod that sits where its preference points, claimed one relaxation stage on: the old gate's six passes find nothing, the wide gate lists exactly one finding, the
 * seventh pass's; once more with a reason word on the placed pod argv[3]: one finding, the eighth pass's.  Last the growth rule -- a struct_size that ends before
 * `stages` does not know bit 64 -- and the refusals.  Compiled and run by tests/test_audit_gate_ex_cabi.py. */
#include <stddef.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: cabi_usage_audit_gate_ex <problem.ksp> <relaxing pod> <placed pod>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const uint32_t pod = (uint32_t)atoi(argv[2]), placed = (uint32_t)atoi(argv[3]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the gate: one call, one struct per requested pass for its totals, no table */
  ksh_audit_out a; ksh_audit_topology_out t; ksh_audit_spread_out s; ksh_audit_firstfit_out ff; ksh_audit_limits_out lm; ksh_audit_hostfit_out hf;
  ksh_audit_stages_out st; ksh_audit_reasons_out rs;
  ksh_audit_gate_ex_out g; memset(&g, 0, sizeof g);
  g.struct_size = (uint32_t)sizeof g;
  g.audit = &a; g.topology = &t; g.spread = &s; g.firstfit = &ff; g.limits = &lm; g.hostfit = &hf; g.stages = &st; g.reasons = &rs;
  double ms[2];
  if (ksh_audit_gate_ex(&h, 1, KS_AUDIT_PASS_ALL_EX, &g, ms) != KS_OK) { fprintf(stderr, "ksh_audit_gate_ex: %s\n", ksh_last_error()); return 1; }
  printf("genuine: %u findings, truncated %u -> %s\n", g.n_findings, g.truncated, g.n_findings ? "solve in Go" : "act");
  printf("totals: %u pods, %u + %u + %u + %u + %u + %u + %u + %u pods flagged\n", a.n_pods, a.n_pods_flagged, t.n_pods_flagged, s.n_pods_flagged, ff.n_pods_flagged,
         lm.n_pods_flagged, hf.n_pods_flagged, st.n_pods_flagged, rs.n_pods_flagged);
  printf("the seventh pass examined %u pods over %u stages and %u pairs; the eighth %u of %u unscheduled pods\n", st.checked[1], st.checked[2], st.checked[3], rs.checked[0], rs.n_unscheduled);
  const uint32_t P = a.n_pods;
  if (pod >= P || placed >= P) return 2;

  /* the commit numbers of that result: one placement row per pod */
  uint64_t id = 7, head[KS_PLC_HEAD_WORDS], total = 0;
  uint64_t* rows = (uint64_t*)take(8 * (size_t)P * KS_PLC_ROW_WORDS);
  if (ksh_placement_rows(&h, 1, &id, head, rows, P, &total, NULL) != KS_OK) { fprintf(stderr, "ksh_placement_rows: %s\n", ksh_last_error()); return 1; }
  int32_t* seq = (int32_t*)take(4 * (size_t)P);
  uint64_t k;
  for (k = 0; k < P; ++k) seq[k] = -1;
  for (k = 0; k < total; ++k) {
    const uint64_t* row = rows + k * KS_PLC_ROW_WORDS;
    seq[(uint32_t)row[KS_PLC_POD_WHERE]] = (int32_t)(uint32_t)(row[KS_PLC_STAGE_SEQ] >> 32);      /* (-1 for an unscheduled pod) */
  }
  ksh_result_arrays ra;
  if (ksh_result_arrays_get(h, &ra) != KS_OK) { fprintf(stderr, "ksh_result_arrays_get: %s\n", ksh_last_error()); return 1; }

  ks_audit_finding found[4]; memset(found, 0xEE, sizeof found);
  g.findings = found; g.cap_findings = 4;
  if (ksh_audit_gate_ex_claimed(h, &ra, seq, KS_AUDIT_PASS_ALL_EX, &g, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate_ex_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u findings, truncated %u\n", g.n_findings, g.truncated);

  /* the pod claimed one stage on: the six passes take pod_stage on trust */
  int32_t* stage = (int32_t*)take(4 * (size_t)P);
  memcpy(stage, ra.pod_stage, 4 * (size_t)P);
  const int32_t* genuine_stage = ra.pod_stage;
  stage[pod] += 1; ra.pod_stage = stage;
  ksh_audit_gate_out six; memset(&six, 0, sizeof six);
  six.audit = &a; six.topology = &t; six.spread = &s; six.firstfit = &ff; six.limits = &lm; six.hostfit = &hf;
  if (ksh_audit_gate_claimed(h, &ra, seq, KS_AUDIT_PASS_ALL, &six, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate_claimed: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_gate_ex_claimed(h, &ra, seq, KS_AUDIT_PASS_ALL_EX, &g, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate_ex_claimed: %s\n", ksh_last_error()); return 1; }
  printf("pod %u claimed at stage %d: the six passes find %u, the eight %u -> %s\n", pod, stage[pod], six.n_findings, g.n_findings, g.n_findings ? "solve in Go" : "act");
  for (k = 0; k < g.n_findings && k < g.cap_findings; ++k)
    printf("finding %u: problem %u, pass %u, table %u, index %u, flags %u\n", (unsigned)k, found[k].problem, found[k].where >> 8, found[k].where & 255u, found[k].index, found[k].flags);
  printf("the record behind them untouched: %d\n", g.n_findings < 4 && found[g.n_findings].problem == 0xEEEEEEEEu);
  /* the rows remain the per-pass calls': the seventh pass alone, with its table */
  ksh_audit_stages_out own; memset(&own, 0, sizeof own);
  own.pod_flags = (uint32_t*)take(4 * (size_t)P); own.cap_pods = P;
  if (ksh_audit_stages_claimed(h, &ra, seq, &own, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_stages_claimed: %s\n", ksh_last_error()); return 1; }
  printf("the seventh pass's own call: %u pods flagged, the pod carries %u; the gate's totals say %u\n", own.n_pods_flagged, own.pod_flags[pod], st.n_pods_flagged);
  ra.pod_stage = genuine_stage;

  /* a reason word on a placed pod: the column no earlier pass reads.  The first and the eighth pass take no commit numbers */
  uint32_t* why = (uint32_t*)take(4 * (size_t)P);
  memcpy(why, ra.pod_reason, 4 * (size_t)P);
  why[placed] = 7u; ra.pod_reason = why;
  memset(found, 0xEE, sizeof found);
  if (ksh_audit_gate_ex_claimed(h, &ra, NULL, KS_AUDIT_PASS_FIRST | KS_AUDIT_PASS_REASONS, &g, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_gate_ex_claimed: %s\n", ksh_last_error()); return 1; }
  printf("a word on placed pod %u, no commit numbers: %u findings: pass %u, index %u, flags %u\n", placed, g.n_findings, found[0].where >> 8, found[0].index, found[0].flags);

  /* the growth rule and the refusals */
  g.struct_size = (uint32_t)offsetof(ksh_audit_gate_ex_out, stages);
  printf("a struct that ends before stages, bit 64: %d\n", ksh_audit_gate_ex(&h, 1, KS_AUDIT_PASS_STAGES, &g, NULL));                    /* KS_ERR_INVALID */
  printf("the same struct, the six: %d\n", ksh_audit_gate_ex(&h, 1, KS_AUDIT_PASS_ALL, &g, NULL));                                        /* KS_OK */
  g.struct_size = (uint32_t)sizeof g;
  printf("bit 256: %d\n", ksh_audit_gate_ex(&h, 1, 256u, &g, NULL));                                                                      /* KS_ERR_INVALID */
  printf("bit 64 through the old gate: %d\n", ksh_audit_gate(&h, 1, KS_AUDIT_PASS_ALL | KS_AUDIT_PASS_STAGES, &six, NULL));               /* KS_ERR_INVALID */
  printf("no commit numbers for the seventh pass: %d\n", ksh_audit_gate_ex_claimed(h, &ra, NULL, KS_AUDIT_PASS_STAGES, &g, NULL));        /* KS_ERR_INVALID */
  ra.pod_reason = NULL;
  printf("no pod_reason for the eighth pass: %d\n", ksh_audit_gate_ex_claimed(h, &ra, seq, KS_AUDIT_PASS_ALL_EX, &g, NULL));              /* KS_ERR_INVALID */
  printf("no pod_reason, the eighth pass not asked: %d\n", ksh_audit_gate_ex_claimed(h, &ra, seq, KS_AUDIT_PASS_ALL | KS_AUDIT_PASS_STAGES, &g, NULL));   /* KS_OK */
  free(why); free(own.pod_flags); free(stage); free(seq); free(rows);
  ksh_close(h); free(text);
  return 0;
}
