/* A plain C99 translation unit for the cluster the narrow selector form refuses: one PodDisruptionBudget per application, `matchLabels: {app: a<i>}`, 70 of them
 * -- more values of one label key than KS_CAND_MAX_VALUES.  A snapshot in (KSP1 text and the node of every bound pod), the 70 PDBs as a ksh_pdb_block built in a loop,
 * ksh_consolidation_candidates_ex without a flag (refused, both counts in the message), then with KSH_CAND_WIDE_SELECTORS: the order and every node's reason printed.
 * Every PDB allows no disruption except a1's.  Compiled and run by tests/test_candidates_wide_selectors.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

#define N_APPS 70

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: cabi_usage_candidates_wide <snapshot.ksp> <node of pod 0> <node of pod 1> ...\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);

  void* snap = NULL;
  if (ksh_parse(text, (size_t)n, &snap) != KS_OK) { fprintf(stderr, "parse: %s\n", ksh_last_error()); return 1; }
  uint32_t n_pods = 0, n_nodes = 0, i, k;
  if (ksh_snapshot_bindings(snap, NULL, 0, &n_pods, &n_nodes) != KS_OK) return 1;
  if ((uint32_t)(argc - 2) != n_pods) { fprintf(stderr, "%u pods, %d bindings\n", n_pods, argc - 2); return 2; }
  int32_t* pod_node = (int32_t*)malloc(sizeof(int32_t) * (n_pods + 1));
  for (i = 0; i < n_pods; ++i) pod_node[i] = (int32_t)atoi(argv[2 + i]);

  /* what the snapshot's objects do not carry: nothing nominated or annotated, no deletion costs or priorities, no ttl */
  uint32_t* node_flags = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); double* age = (double*)calloc(n_nodes + 1, sizeof(double));
  uint32_t* pod_flags = (uint32_t*)calloc(n_pods + 1, sizeof(uint32_t)); double* dcost = (double*)calloc(n_pods + 1, sizeof(double)); int32_t* prio = (int32_t*)calloc(n_pods + 1, sizeof(int32_t));
  const uint32_t enabled[2] = {1, 1}; const int64_t ttl[2] = {-1, -1};
  ksh_candidate_inputs in; memset(&in, 0, sizeof in);
  in.n_nodes = n_nodes; in.n_pods = n_pods; in.n_provisioners = 2;
  in.node_flags = node_flags; in.node_age_seconds = age; in.pod_flags = pod_flags; in.pod_deletion_cost = dcost; in.pod_priority = prio;
  in.prov_consolidation_enabled = enabled; in.prov_ttl_seconds_until_expired = ttl;

  /* the PDBs: strings 0 "default", 1 "app", 2 + i "a<i>"; per PDB namespace:S disruptions_allowed:I selector(0 = not nil, MAP of one pair, no expressions) */
  char strings[16 + 4 * N_APPS]; uint32_t str_off[3 + N_APPS]; uint32_t words[7 * N_APPS]; uint32_t at = 0;
  memcpy(strings, "defaultapp", 10); str_off[0] = 0; str_off[1] = 7; str_off[2] = at = 10;
  for (i = 0; i < N_APPS; ++i) {
    at += (uint32_t)sprintf(strings + at, "a%u", (unsigned)i); str_off[3 + i] = at;
    uint32_t* w = words + 7 * i;
    w[0] = 0; w[1] = i == 1 ? 1u : 0u; w[2] = 0; w[3] = 1; w[4] = 1; w[5] = 2 + i; w[6] = 0;
  }
  ksh_pdb_block pdbs; memset(&pdbs, 0, sizeof pdbs);
  pdbs.n_pdbs = N_APPS; pdbs.n_strings = 2 + N_APPS; pdbs.n_words = 7 * N_APPS; pdbs.str_off = str_off; pdbs.str_bytes = strings; pdbs.words = words; pdbs.str_bytes_len = at;

  ksh_candidates_out out; memset(&out, 0, sizeof out);
  out.order = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); out.empty = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); out.why = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t));
  out.detail = (int32_t*)calloc(n_nodes + 1, sizeof(int32_t)); out.n_node_pods = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); out.cost = (double*)calloc(n_nodes + 1, sizeof(double));

  /* without the flag: 70 values of one key do not fit the narrow form */
  if (ksh_consolidation_candidates_ex(snap, pod_node, NULL, 0, &in, &pdbs, 0 /* device */, 0 /* flags */, &out, NULL) != KS_ERR_UNSUPPORTED) { fprintf(stderr, "70 values were taken by the narrow form\n"); return 1; }
  printf("refused: %s\n", ksh_last_error());

  double ms[4];
  if (ksh_consolidation_candidates_ex(snap, pod_node, NULL, 0, &in, &pdbs, 0, KSH_CAND_WIDE_SELECTORS, &out, ms) != KS_OK) { fprintf(stderr, "candidates: %s\n", ksh_last_error()); return 1; }
  printf("order:");
  for (i = 0; i < out.n_candidates; ++i) printf(" %s", ksh_snapshot_name(snap, 3, out.order[i], 0));
  printf("\nempty: %u\n", (unsigned)out.n_empty);
  for (i = 0; i < n_nodes; ++i) {
    unsigned char b[8]; memcpy(b, &out.cost[i], 8);
    printf("%s: why %u detail %d pods %u cost ", ksh_snapshot_name(snap, 3, i, 0), (unsigned)out.why[i], (int)out.detail[i], (unsigned)out.n_node_pods[i]);
    for (k = 0; k < 8; ++k) printf("%02x", b[k]);
    printf("\n");
  }

  /* a flag bit the library does not know */
  if (ksh_consolidation_candidates_ex(snap, pod_node, NULL, 0, &in, &pdbs, 0, 2u, &out, NULL) != KS_ERR_INVALID) { fprintf(stderr, "an unknown flag bit was taken\n"); return 1; }
  printf("refused: %s\n", ksh_last_error());

  free(out.order); free(out.empty); free(out.why); free(out.detail); free(out.n_node_pods); free(out.cost);
  free(node_flags); free(age); free(pod_flags); free(dcost); free(prio); free(pod_node); ksh_parsed_free(snap); free(text);
  return 0;
}
