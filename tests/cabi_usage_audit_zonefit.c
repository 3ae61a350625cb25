/* A plain C99 translation unit that puts the three first-fit passes behind a result the way a shim would: solve over a handle, ksh_audit_firstfit, ksh_audit_hostfit,
 * then ksh_audit_zonefit -- the pods under zonal spread, which the other two leave out -- and act only if none flags anything.  Then the form for a result from
 * anywhere: the result's arrays (ksh_result_arrays_get) and its commit numbers, read through ksh_placement_rows (KS_PLC_STAGE_SEQ), audited back as CLAIMED -- clean --,
 * and once more with pod argv[2], a pod under a zonal spread, claimed on existing node argv[3], later than a node of a zone that admitted it at its moment: exactly
 * that pod carries KS_AUDIT_POD_ZFIT_EXISTING.  Compiled and run by tests/test_audit_zonefit_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

int main(int argc, char** argv) {
  if (argc < 4) { fprintf(stderr, "usage: cabi_usage_audit_zonefit <problem.ksp> <pod> <existing node>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const uint32_t pod = (uint32_t)atoi(argv[2]); const int32_t node = (int32_t)atoi(argv[3]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the three passes over the result where it lies.  Totals always; the flag rows only when the tables hold them */
  ksh_audit_firstfit_out ff; memset(&ff, 0, sizeof ff);
  ksh_audit_hostfit_out hf; memset(&hf, 0, sizeof hf);
  ksh_audit_zonefit_out zf; memset(&zf, 0, sizeof zf);
  if (ksh_audit_firstfit(&h, 1, &ff, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_firstfit: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_hostfit(&h, 1, &hf, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_hostfit: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_zonefit(&h, 1, &zf, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_zonefit: %s\n", ksh_last_error()); return 1; }
  const unsigned found = ff.n_pods_flagged + hf.n_pods_flagged + zf.n_pods_flagged;
  printf("genuine: %u + %u + %u of %u pods flagged, truncated %u -> %s\n", ff.n_pods_flagged, hf.n_pods_flagged, zf.n_pods_flagged, zf.n_pods, zf.truncated, found ? "solve in Go" : "act");
  printf("the fourth pass examined %u pods, the sixth %u, the ninth %u\n", ff.checked[1], hf.checked[1], zf.checked[1]);
  printf("evaluated: %u placed pods, %u pods examined, %u skipped, %u mixed, %u eligible groups, %u skipped, %u zone tests, %u passed, %u pairs admitting, %u pods exact\n", zf.checked[0],
         zf.checked[1], zf.skipped_pods, zf.mixed_pods, zf.eligible_groups, zf.skipped_groups, zf.checked[2], zf.checked[3], zf.admitting_pairs, zf.exact_pods);
  const uint32_t P = zf.n_pods;
  if (pod >= P || KS_AZ_GROUPS != 4u) return 2;

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

  zf.pod_flags = (uint32_t*)take(4 * (size_t)P); zf.cap_pods = P;
  if (ksh_audit_zonefit_claimed(h, &ra, seq, &zf, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_zonefit_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u rows, %u pods flagged, truncated %u\n", (unsigned)total, zf.n_pods_flagged, zf.truncated);
  int32_t* where = (int32_t*)take(4 * (size_t)P);
  memcpy(where, ra.pod_node, 4 * (size_t)P);
  const int32_t was = where[pod];
  where[pod] = node; ra.pod_node = where;
  if (ksh_audit_zonefit_claimed(h, &ra, seq, &zf, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_zonefit_claimed: %s\n", ksh_last_error()); return 1; }
  printf("pod %u claimed on node %d instead of %d: %u pods flagged, the pod carries %u -> %s\n", pod, node, was, zf.n_pods_flagged, zf.pod_flags[pod],
         (zf.pod_flags[pod] & KS_AUDIT_POD_ZFIT_EXISTING) ? "solve in Go" : "act");
  printf("no commit numbers: %d\n", ksh_audit_zonefit_claimed(h, &ra, NULL, &zf, NULL));      /* KS_ERR_INVALID */
  free(where); free(zf.pod_flags); free(seq); free(rows);
  ksh_close(h); free(text);
  return 0;
}
