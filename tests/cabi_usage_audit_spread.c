/* A plain C99 translation unit that gates a result the way a shim would ("the audit gate"), with the three passes: solve over a handle, ksh_audit,
 * ksh_audit_topology, then ksh_audit_spread, and act only if none flags anything.  Then the form for a result from anywhere: the result's arrays
 * (ksh_result_arrays_get) and its commit numbers, read through ksh_placement_rows (KS_PLC_STAGE_SEQ), audited back as CLAIMED -- clean --, and once more with the
 * commit numbers argv[2] and argv[3] exchanged between the two pods that hold them, so that a zone is chosen while another is still emptier by more than maxSkew:
 * exactly the pod that now holds argv[2] carries KS_AUDIT_POD_SPREAD.  Compiled and run by tests/test_audit_spread_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: cabi_usage_audit_spread <problem.ksp> <commit number> <commit number>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const int32_t first = (int32_t)atoi(argv[2]), second = (int32_t)atoi(argv[3]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the gate: the three passes over the result where it lies.  Totals always; the flag rows only when the tables hold them */
  ksh_audit_out a; memset(&a, 0, sizeof a);
  ksh_audit_topology_out t; memset(&t, 0, sizeof t);
  ksh_audit_spread_out s; memset(&s, 0, sizeof s);
  if (ksh_audit(&h, 1, &a, NULL) != KS_OK) { fprintf(stderr, "ksh_audit: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_topology(&h, 1, &t, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_topology: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_spread(&h, 1, &s, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_spread: %s\n", ksh_last_error()); return 1; }
  printf("genuine: %u + %u + %u of %u pods, %u nodes flagged, truncated %u -> %s\n", a.n_pods_flagged, t.n_pods_flagged, s.n_pods_flagged, s.n_pods, a.n_nodes_flagged, s.truncated,
         (a.n_pods_flagged || a.n_nodes_flagged || t.n_pods_flagged || s.n_pods_flagged) ? "solve in Go" : "act");
  printf("evaluated: %u placed pods, %u pairs, %u of them exactly, %u spread groups unattempted\n", s.checked[0], s.checked[1], s.exact_pairs, s.skipped_groups);
  const uint32_t P = s.n_pods;

  /* the commit numbers of that result: one placement row per pod */
  uint64_t id = 7, head[KS_PLC_HEAD_WORDS], total = 0;
  uint64_t* rows = (uint64_t*)take(8 * (size_t)P * KS_PLC_ROW_WORDS);
  if (ksh_placement_rows(&h, 1, &id, head, rows, P, &total, NULL) != KS_OK) { fprintf(stderr, "ksh_placement_rows: %s\n", ksh_last_error()); return 1; }
  int32_t* seq = (int32_t*)take(4 * (size_t)P);
  uint64_t k; uint32_t i, pa = P, pb = P;
  for (k = 0; k < total; ++k) {
    const uint64_t* row = rows + k * KS_PLC_ROW_WORDS;
    seq[(uint32_t)row[KS_PLC_POD_WHERE]] = (int32_t)(uint32_t)(row[KS_PLC_STAGE_SEQ] >> 32);
  }
  for (i = 0; i < P; ++i) { if (seq[i] == first) pa = i; if (seq[i] == second) pb = i; }
  if (pa >= P || pb >= P) return 2;
  ksh_result_arrays ra;
  if (ksh_result_arrays_get(h, &ra) != KS_OK) { fprintf(stderr, "ksh_result_arrays_get: %s\n", ksh_last_error()); return 1; }

  s.pod_flags = (uint32_t*)take(4 * (size_t)P); s.cap_pods = P;
  if (ksh_audit_spread_claimed(h, &ra, seq, &s, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_spread_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u rows, %u pods flagged, truncated %u\n", (unsigned)total, s.n_pods_flagged, s.truncated);
  seq[pa] = second; seq[pb] = first;
  if (ksh_audit_spread_claimed(h, &ra, seq, &s, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_spread_claimed: %s\n", ksh_last_error()); return 1; }
  printf("commit numbers exchanged: %u pods flagged, the pod that went first carries %u, the other %u -> %s\n", s.n_pods_flagged, s.pod_flags[pb], s.pod_flags[pa],
         s.n_pods_flagged ? "solve in Go" : "act");
  printf("no commit numbers: %d\n", ksh_audit_spread_claimed(h, &ra, NULL, &s, NULL));      /* KS_ERR_INVALID */
  free(s.pod_flags); free(seq); free(rows);
  ksh_close(h); free(text);
  return 0;
}
