/* A plain C99 translation unit for the cluster the dense per-node tables refuse: more than 1 024 topology groups among the bound pods (one per Deployment with a
 * spread constraint or a pod (anti-)affinity term).  A snapshot in (KSP1 text and the node of every bound pod); ksh_open_whatifs_derived without a flag (refused: the
 * message names the cap), then with KSH_DERIVE_GROUP_LISTS: three what-ifs -- node 0, nodes 1 and 2, the last node -- derived on the device, each handle's arena, the
 * groups active in it and its positive domain counts read back through ksh_debug_whatif_topology, solved in one launch, the summary printed.
 * Compiled and run by tests/test_whatif_group_lists.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: cabi_usage_group_lists <snapshot.ksp> <node of pod 0> <node of pod 1> ...\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);

  void* snap = NULL;
  if (ksh_parse(text, (size_t)n, &snap) != KS_OK) { fprintf(stderr, "parse: %s\n", ksh_last_error()); return 1; }
  uint32_t n_pods = 0, n_nodes = 0, i, w;
  if (ksh_snapshot_bindings(snap, NULL, 0, &n_pods, &n_nodes) != KS_OK) return 1;
  if ((uint32_t)(argc - 2) != n_pods || n_nodes < 3) { fprintf(stderr, "%u pods, %d bindings, %u nodes\n", n_pods, argc - 2, n_nodes); return 2; }
  int32_t* pod_node = (int32_t*)malloc(sizeof(int32_t) * (n_pods + 1));
  for (i = 0; i < n_pods; ++i) pod_node[i] = (int32_t)atoi(argv[2 + i]);

  /* the candidate sets, CSR: {0}, {1, 2}, {last} */
  uint32_t cand_off[4] = {0, 1, 3, 4}; uint32_t cand[4] = {0, 1, 2, 0}; void* h[3] = {NULL, NULL, NULL};
  cand[3] = n_nodes - 1;

  /* the self-check needs no device: with the flag the derivation is restated from the lists; without it the snapshot is refused */
  if (ksh_check_whatif_derivation(snap, KSH_DERIVE_GROUP_LISTS, cand + 1, 2, pod_node) != KS_OK) { fprintf(stderr, "check: %s\n", ksh_last_error()); return 1; }

  /* without the flag: more than 1 024 groups do not fit the dense tables -- nothing is opened */
  if (ksh_open_whatifs_derived(snap, 0, 3, cand_off, cand, pod_node, 0 /* device */, h) != KS_ERR_UNSUPPORTED) { fprintf(stderr, "more than 1024 groups were taken by the dense tables\n"); return 1; }
  printf("refused: %s\n", ksh_last_error());

  if (ksh_open_whatifs_derived(snap, KSH_DERIVE_GROUP_LISTS, 3, cand_off, cand, pod_node, 0, h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  uint32_t dims[10]; ksh_dims(h[0], dims);
  const uint32_t G = dims[7], GH = dims[8], words = (dims[2] + 63) / 64;
  printf("groups: %u\n", (unsigned)G);
  uint8_t* active = (uint8_t*)calloc(G + 1, 1); int32_t* count = (int32_t*)calloc((size_t)G * 64 + 1, sizeof(int32_t)); int32_t* extra = (int32_t*)calloc(GH + 1, sizeof(int32_t));
  uint64_t* sum = (uint64_t*)calloc(2 + words, sizeof(uint64_t));
  if (ksh_solve_batch(h, 3, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "solve: %s\n", ksh_last_error()); return 1; }
  for (w = 0; w < 3; ++w) {
    uint32_t n_active = 0, positive = 0; size_t c;
    if (ksh_debug_whatif_topology(h[w], active, count, extra) != KS_OK) { fprintf(stderr, "debug: %s\n", ksh_last_error()); return 1; }
    for (i = 0; i < G; ++i) n_active += active[i] ? 1u : 0u;
    for (c = 0; c < (size_t)G * 64; ++c) positive += count[c] > 0 ? 1u : 0u;
    if (ksh_result_summary(h[w], sum, words) != KS_OK) { fprintf(stderr, "summary: %s\n", ksh_last_error()); return 1; }
    printf("what-if %u: arena %lu bytes, active %u of %u groups, %u positive domain counts, %lu new nodes, %lu unscheduled\n", (unsigned)w,
           (unsigned long)ksh_whatifs_arena_bytes(h[w]), (unsigned)n_active, (unsigned)G, (unsigned)positive, (unsigned long)sum[0], (unsigned long)sum[1]);
  }

  /* a handle that is no derived what-if has no such state */
  if (ksh_debug_whatif_topology(NULL, active, count, extra) != KS_ERR_INVALID) { fprintf(stderr, "a null handle was taken\n"); return 1; }

  for (w = 0; w < 3; ++w) ksh_close(h[w]);
  free(sum); free(active); free(count); free(extra); free(pod_node); ksh_parsed_free(snap); free(text);
  return 0;
}
