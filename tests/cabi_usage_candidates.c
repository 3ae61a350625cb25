/* A plain C99 translation unit that asks for the candidates of a consolidation pass the way a cgo shim would: a cluster snapshot in (KSP1 text
 * and the node of every bound pod), what the snapshot does not carry as arrays over its node and pod slots (ages, flags, the provisioners' ttl), one
 * PodDisruptionBudget as a ksh_pdb_block written by hand, ksh_consolidation_candidates, and the order and every node's reason printed.  Then one refusal: a ttl
 * of 0.  Compiled and run by tests/test_consolidation_candidates.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: cabi_usage_candidates <snapshot.ksp> <node of pod 0> <node of pod 1> ...\n"); return 2; }
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

  /* what the snapshot's objects do not carry: node 0 is 100 s old, nothing is nominated or annotated; no pod carries a deletion cost or a priority;
     provisioner 0 expires its nodes after 1000 s, provisioner 1 never */
  uint32_t* node_flags = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); double* age = (double*)calloc(n_nodes + 1, sizeof(double));
  uint32_t* pod_flags = (uint32_t*)calloc(n_pods + 1, sizeof(uint32_t)); double* dcost = (double*)calloc(n_pods + 1, sizeof(double)); int32_t* prio = (int32_t*)calloc(n_pods + 1, sizeof(int32_t));
  const uint32_t enabled[2] = {1, 1}; int64_t ttl[2] = {1000, -1};
  age[0] = 100.0;
  ksh_candidate_inputs in; memset(&in, 0, sizeof in);
  in.n_nodes = n_nodes; in.n_pods = n_pods; in.n_provisioners = 2;
  in.node_flags = node_flags; in.node_age_seconds = age; in.pod_flags = pod_flags; in.pod_deletion_cost = dcost; in.pod_priority = prio;
  in.prov_consolidation_enabled = enabled; in.prov_ttl_seconds_until_expired = ttl;

  /* one PDB in "default": matchLabels app=guarded, no disruptions allowed.  namespace:S disruptions_allowed:I selector(0 = not nil, MAP, N exprs) */
  static const char strings[] = "defaultappguarded";
  const uint32_t str_off[4] = {0, 7, 10, 17};
  const uint32_t words[7] = {0, 0, 0, 1, 1, 2, 0};
  ksh_pdb_block pdbs; memset(&pdbs, 0, sizeof pdbs);
  pdbs.n_pdbs = 1; pdbs.n_strings = 3; pdbs.n_words = 7; pdbs.str_off = str_off; pdbs.str_bytes = strings; pdbs.words = words; pdbs.str_bytes_len = 17;

  ksh_candidates_out out; memset(&out, 0, sizeof out);
  out.order = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); out.empty = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); out.why = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t));
  out.detail = (int32_t*)calloc(n_nodes + 1, sizeof(int32_t)); out.n_node_pods = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); out.cost = (double*)calloc(n_nodes + 1, sizeof(double));
  double ms[4];
  if (ksh_consolidation_candidates(snap, pod_node, NULL, 0, &in, &pdbs, 0 /* device */, &out, ms) != KS_OK) { fprintf(stderr, "candidates: %s\n", ksh_last_error()); return 1; }
  printf("order:");
  for (i = 0; i < out.n_candidates; ++i) printf(" %s", ksh_snapshot_name(snap, 3, out.order[i], 0));
  printf("\nempty: %u\n", (unsigned)out.n_empty);
  for (i = 0; i < n_nodes; ++i) {
    unsigned char b[8]; memcpy(b, &out.cost[i], 8);
    printf("%s: why %u detail %d pods %u cost ", ksh_snapshot_name(snap, 3, i, 0), (unsigned)out.why[i], (int)out.detail[i], (unsigned)out.n_node_pods[i]);
    for (k = 0; k < 8; ++k) printf("%02x", b[k]);
    printf("\n");
  }

  /* a ttl of 0: the reference divides by zero there; refused before anything is launched */
  ttl[0] = 0;
  if (ksh_consolidation_candidates(snap, pod_node, NULL, 0, &in, &pdbs, 0, &out, NULL) != KS_ERR_INVALID) { fprintf(stderr, "a ttl of 0 was taken\n"); return 1; }
  printf("refused: %s\n", ksh_last_error());

  free(out.order); free(out.empty); free(out.why); free(out.detail); free(out.n_node_pods); free(out.cost);
  free(node_flags); free(age); free(pod_flags); free(dcost); free(prio); free(pod_node); ksh_parsed_free(snap); free(text);
  return 0;
}
