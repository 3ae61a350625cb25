/* A plain C99 translation unit that checks a result's failure reasons the way a shim would before it synthesises PodFailedToSchedule events (INTEGRATION.md,
 * "Beside the gate: the failure reasons"): solve over a handle, ksh_audit_reasons over the resident result -- totals only --, and record events only if it finds
 * nothing.  Then the form for a result from anywhere: the result's arrays (ksh_result_arrays_get) audited back as CLAIMED -- clean --, and once more with the first
 * nibble of pod argv[2], an unscheduled pod no instance type holds, changed from KS_WHY_NO_INSTANCE_TYPE to KS_WHY_TOPOLOGY: the first pass stays clean, exactly that
 * pod carries KS_AUDIT_POD_REASON_STATIC.  Last, the refusal: a claimed result without pod_reason.  Compiled and run by tests/test_audit_reasons_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: cabi_usage_audit_reasons <problem.ksp> <pod>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const uint32_t pod = (uint32_t)atoi(argv[2]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the resident result: totals always; the flag rows only when the table holds them */
  ksh_audit_reasons_out rs; memset(&rs, 0, sizeof rs);
  if (ksh_audit_reasons(&h, 1, &rs, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_reasons: %s\n", ksh_last_error()); return 1; }
  printf("genuine: reasons %u of %u pods flagged, truncated %u -> %s\n", rs.n_pods_flagged, rs.n_pods, rs.truncated, rs.n_pods_flagged ? "solve in Go" : "record the events");
  printf("evaluated: %u placed pods, %u of %u unscheduled pods examined, %u skipped; nibbles: %u exact, %u bounded, %u not examined; %u classes, %u pairs\n", rs.n_placed, rs.checked[0],
         rs.n_unscheduled, rs.skipped_pods, rs.checked[1], rs.checked[2], rs.checked[3], rs.used_classes, rs.pairs);
  const uint32_t P = rs.n_pods;
  if (pod >= P) return 2;

  /* the same result, claimed back */
  ksh_result_arrays ra;
  if (ksh_result_arrays_get(h, &ra) != KS_OK) { fprintf(stderr, "ksh_result_arrays_get: %s\n", ksh_last_error()); return 1; }
  rs.pod_flags = (uint32_t*)take(4 * (size_t)P); rs.cap_pods = P;
  if (ksh_audit_reasons_claimed(h, &ra, &rs, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_reasons_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u pods flagged, truncated %u\n", rs.n_pods_flagged, rs.truncated);

  /* one nibble tampered: the first pass does not read the column */
  uint32_t* reason = (uint32_t*)take(4 * (size_t)P);
  memcpy(reason, ra.pod_reason, 4 * (size_t)P);
  const uint32_t was = reason[pod] & 15u;
  reason[pod] = (reason[pod] & ~15u) | (uint32_t)KS_WHY_TOPOLOGY; ra.pod_reason = reason;
  ksh_audit_out a; memset(&a, 0, sizeof a);
  if (ksh_audit_claimed(h, &ra, &a, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_claimed: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_reasons_claimed(h, &ra, &rs, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_reasons_claimed: %s\n", ksh_last_error()); return 1; }
  printf("pod %u claimed with reason %u instead of %u for the first template: first pass %u pods flagged, reasons %u pods flagged, the pod carries %u -> %s\n", pod, (unsigned)KS_WHY_TOPOLOGY, was,
         a.n_pods_flagged, rs.n_pods_flagged, rs.pod_flags[pod], rs.n_pods_flagged ? "solve in Go" : "record the events");

  /* the refusal */
  ra.pod_reason = NULL;
  const int rc = ksh_audit_reasons_claimed(h, &ra, &rs, NULL);
  printf("no pod_reason: %d %s\n", rc, ksh_last_error());      /* KS_ERR_INVALID */
  free(reason); free(rs.pod_flags);
  ksh_close(h); free(text);
  return 0;
}
