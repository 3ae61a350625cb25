/* A plain C99 translation unit that gates a result the way a shim would ("the audit gate"), with both passes: solve over a handle, ksh_audit, then
 * ksh_audit_topology, and act only if neither flags anything.  Then the form for a result from anywhere: the result's arrays (ksh_result_arrays_get) and its commit
 * numbers, read through ksh_placement_rows (KS_PLC_STAGE_SEQ), audited back as CLAIMED -- clean --, and once more with two commit numbers exchanged, so that a
 * follower (argv[2]) is placed before the leader (argv[3]) its required affinity names: exactly that pod carries KS_AUDIT_POD_AFFINITY.  Compiled and run by
 * tests/test_audit_topology_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: cabi_usage_audit_topology <problem.ksp> <follower pod> <leader pod>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const uint32_t follower = (uint32_t)atoi(argv[2]), leader = (uint32_t)atoi(argv[3]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the gate: both passes over the result where it lies.  Totals always; the flag rows only when the tables hold them */
  ksh_audit_out a; memset(&a, 0, sizeof a);
  ksh_audit_topology_out t; memset(&t, 0, sizeof t);
  if (ksh_audit(&h, 1, &a, NULL) != KS_OK) { fprintf(stderr, "ksh_audit: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_topology(&h, 1, &t, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_topology: %s\n", ksh_last_error()); return 1; }
  printf("genuine: %u + %u of %u pods, %u nodes flagged, truncated %u -> %s\n", a.n_pods_flagged, t.n_pods_flagged, t.n_pods, a.n_nodes_flagged, t.truncated,
         (a.n_pods_flagged || a.n_nodes_flagged || t.n_pods_flagged) ? "solve in Go" : "act");
  printf("evaluated: %u commit numbers, anti-affinity %s, affinity %s, hostname spread %s, %u groups skipped\n", t.checked[0], t.checked[1] ? "yes" : "no", t.checked[2] ? "yes" : "no",
         t.checked[3] ? "yes" : "no", t.skipped_groups);
  const uint32_t P = t.n_pods;
  if (follower >= P || leader >= P) return 2;

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

  t.pod_flags = (uint32_t*)take(4 * (size_t)P); t.cap_pods = P;
  if (ksh_audit_topology_claimed(h, &ra, seq, &t, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_topology_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u rows, %u pods flagged, truncated %u\n", (unsigned)total, t.n_pods_flagged, t.truncated);
  printf("the leader was committed %s the follower\n", seq[leader] < seq[follower] ? "before" : "after");
  { const int32_t x = seq[leader]; seq[leader] = seq[follower]; seq[follower] = x; }
  if (ksh_audit_topology_claimed(h, &ra, seq, &t, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_topology_claimed: %s\n", ksh_last_error()); return 1; }
  printf("commit numbers exchanged: %u pods flagged, the follower carries %u (%u with KS_AUDIT_POD_AFFINITY) -> %s\n", t.n_pods_flagged, t.pod_flags[follower], t.pod_bit_count[9],
         t.n_pods_flagged ? "solve in Go" : "act");
  printf("no commit numbers: %d\n", ksh_audit_topology_claimed(h, &ra, NULL, &t, NULL));      /* KS_ERR_INVALID */
  free(t.pod_flags); free(seq); free(rows);
  ksh_close(h); free(text);
  return 0;
}
