/* A plain C99 translation unit for Provisioner.Reconcile's scheduling pass through kshost.h: a snapshot in (KSP1 text and the node of every bound pod -- the pending
 * pods are bound to the carrier node), the carrier and two nodes marked for deletion named on the command line; ksh_provision as a sizing call, then with tables of
 * exactly that size: the head, one line per placement row, one per machine with its launch pick.  A call with an unknown flag bit is refused.
 * Compiled and run by tests/test_provision_gpu.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: cabi_usage_provision <snapshot.ksp> <carrier> <deleting> <deleting> <node of pod 0> <node of pod 1> ...\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);

  void* snap = NULL;
  if (ksh_parse(text, (size_t)n, &snap) != KS_OK) { fprintf(stderr, "parse: %s\n", ksh_last_error()); return 1; }
  uint32_t n_pods = 0, n_nodes = 0, i;
  if (ksh_snapshot_bindings(snap, NULL, 0, &n_pods, &n_nodes) != KS_OK) return 1;
  if ((uint32_t)(argc - 5) != n_pods) { fprintf(stderr, "%u pods, %d bindings\n", n_pods, argc - 5); return 2; }
  uint32_t leaving[3];
  for (i = 0; i < 3; ++i) leaving[i] = (uint32_t)atoi(argv[2 + i]);
  int32_t* pod_node = (int32_t*)malloc(sizeof(int32_t) * (n_pods + 1));
  for (i = 0; i < n_pods; ++i) pod_node[i] = (int32_t)atoi(argv[5 + i]);

  /* how many instance types: the option words of a machine row */
  uint32_t T = 0; while (ksh_snapshot_name(snap, 4, T, 0)) ++T;
  const uint32_t words = (T + 63) / 64;

  ksh_provision_out out; double ms[5];
  memset(&out, 0, sizeof out); out.words = words;
  if (ksh_provision(snap, 1u << 30, pod_node, leaving, 3, 0, &out, ms) != KS_ERR_INVALID) { fprintf(stderr, "an unknown flag bit was taken\n"); return 1; }
  printf("refused: %s\n", ksh_last_error());

  /* the sizing call: capacities 0, tables NULL */
  if (ksh_provision(snap, 0, pod_node, leaving, 3, 0 /* device */, &out, ms) != KS_OK) { fprintf(stderr, "sizing: %s\n", ksh_last_error()); return 1; }
  printf("sizing: %lu rows, %lu machines\n", (unsigned long)out.total_rows, (unsigned long)out.total_machines);

  const uint64_t P = out.total_rows, M = out.total_machines; const size_t NW = KS_REP_NODE_WORDS(words);
  out.cap_rows = P; out.cap_machines = M;
  out.rows = (uint64_t*)calloc((size_t)P * KS_PLC_ROW_WORDS + 1, sizeof(uint64_t)); out.machines = (uint64_t*)calloc((size_t)M * NW + 1, sizeof(uint64_t));
  out.pick_type = (int32_t*)calloc((size_t)M + 1, sizeof(int32_t)); out.pick_zone = (int32_t*)calloc((size_t)M + 1, sizeof(int32_t));
  out.pick_ct = (int32_t*)calloc((size_t)M + 1, sizeof(int32_t)); out.pick_price = (double*)calloc((size_t)M + 1, sizeof(double));
  if (ksh_provision(snap, 0, pod_node, leaving, 3, 0, &out, ms) != KS_OK) { fprintf(stderr, "provision: %s\n", ksh_last_error()); return 1; }
  if (out.head[KS_PLC_FLAGS] != 0 || out.head[KS_PLC_N_EXISTING] != n_nodes) { fprintf(stderr, "flags %lu, %lu node slots\n", (unsigned long)out.head[KS_PLC_FLAGS], (unsigned long)out.head[KS_PLC_N_EXISTING]); return 1; }
  printf("head: %lu pods, %lu new, %lu unscheduled, route %u\n", (unsigned long)out.head[KS_PLC_P], (unsigned long)out.head[KS_PLC_N_NEW], (unsigned long)out.head[KS_PLC_N_UNSCHEDULED],
         (unsigned)out.route);
  uint64_t k;
  for (k = 0; k < P; ++k) {
    const uint64_t* row = out.rows + k * KS_PLC_ROW_WORDS;
    printf("pod %u where %d stage %d\n", (unsigned)(uint32_t)row[KS_PLC_POD_WHERE], (int)(int32_t)(uint32_t)(row[KS_PLC_POD_WHERE] >> 32), (int)(int32_t)(uint32_t)row[KS_PLC_STAGE_SEQ]);
  }
  for (k = 0; k < M; ++k) {
    const uint64_t* m = out.machines + k * NW;
    const char* type = out.pick_type[k] >= 0 ? ksh_snapshot_name(snap, 4, (uint32_t)out.pick_type[k], 0) : NULL;
    const char* zone = out.pick_zone[k] >= 0 ? ksh_snapshot_name(snap, 5, (uint32_t)out.pick_zone[k], 0) : NULL;
    const char* ct = out.pick_ct[k] >= 0 ? ksh_snapshot_name(snap, 6, (uint32_t)out.pick_ct[k], 0) : NULL;
    printf("machine %lu: %lu options, pick %s %s %s %.4f\n", (unsigned long)(m[KS_REP_NODE_ID] >> 32), (unsigned long)m[KS_REP_NODE_N_OPTIONS], type ? type : "-", zone ? zone : "-", ct ? ct : "-",
           out.pick_price[k]);
  }

  free(out.rows); free(out.machines); free(out.pick_type); free(out.pick_zone); free(out.pick_ct); free(out.pick_price);
  free(pod_node); ksh_parsed_free(snap); free(text);
  return 0;
}
