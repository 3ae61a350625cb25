/* A plain C99 translation unit that asks for consolidation commands the way a cgo shim would: a cluster snapshot in (KSP1 text and
 * the node of every bound pod), one candidate set per state node, ksh_consolidation_commands, and every row printed with the names ksh_snapshot_name gives --
 * nodes to remove, replacement instance types, the replacement's requirements.  Then the single-node scan over the same candidates, and one refusal that cannot
 * be made through libkshost: a flat problem stripped of its prices.  Compiled and run by tests/test_consolidation_commands.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static const char* const ACTION[4] = {"do-nothing", "delete", "replace", "error"};

static void print_row(void* snap, const uint64_t* row, uint32_t words, const uint32_t* cand, uint32_t ncand) {
  const uint32_t action = (uint32_t)(row[KS_CMD_DECISION] & 0xffu), reason = (uint32_t)((row[KS_CMD_DECISION] >> 8) & 0xffu);
  uint32_t i, k, v;
  printf("%s", ACTION[action]);
  if (action == KS_CMD_DO_NOTHING || action == KS_CMD_ERROR) { printf(" (step %u)\n", reason); return; }
  printf(" remove");
  for (i = 0; i < ncand; ++i) printf(" %s", ksh_snapshot_name(snap, 3, cand[i], 0));
  if (action == KS_CMD_REPLACE) {
    const uint32_t present = (uint32_t)row[KS_CMD_PRESENT], complement = (uint32_t)(row[KS_CMD_PRESENT] >> 32);
    printf(" options %u:", (unsigned)row[KS_CMD_N_OPTIONS]);
    for (i = 0; i < words * 64u; ++i) if ((row[KS_CMD_OPTIONS + i / 64u] >> (i % 64u)) & 1u) printf(" %s", ksh_snapshot_name(snap, 4, i, 0));
    printf(" | requirements:");
    for (k = 0; k < KS_MAX_KEYS; ++k) if ((present >> k) & 1u) {
      printf(" %s %s [", ksh_snapshot_name(snap, 0, k, 0), ((complement >> k) & 1u) ? "NotIn" : "In");
      for (v = 0, i = 0; v < KS_MAX_VALUES; ++v) if ((row[KS_CMD_MASK + k] >> v) & 1u) printf("%s%s", i++ ? " " : "", ksh_snapshot_name(snap, 1, k, v));
      if (!row[KS_CMD_MASK + k] && (row[KS_CMD_DECISION] >> 16 & 1u) && !strcmp(ksh_snapshot_name(snap, 0, k, 0), "karpenter.sh/capacity-type")) printf("spot");
      printf("]");
    }
    if (row[KS_CMD_DECISION] >> 16 & 1u) printf(" (narrowed to spot)");
  }
  printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: cabi_usage_commands <snapshot.ksp> <node of pod 0> <node of pod 1> ...\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);

  void* snap = NULL;
  if (ksh_parse(text, (size_t)n, &snap) != KS_OK) { fprintf(stderr, "parse: %s\n", ksh_last_error()); return 1; }
  uint32_t n_pods = 0, n_nodes = 0, i;
  if (ksh_snapshot_bindings(snap, NULL, 0, &n_pods, &n_nodes) != KS_OK) return 1;
  if ((uint32_t)(argc - 2) != n_pods) { fprintf(stderr, "%u pods, %d bindings\n", n_pods, argc - 2); return 2; }
  int32_t* pod_node = (int32_t*)malloc(sizeof(int32_t) * (n_pods + 1));
  for (i = 0; i < n_pods; ++i) pod_node[i] = (int32_t)atoi(argv[2 + i]);

  /* the instance types are counted through the name accessor: a row's option masks need ceil(T/64) words */
  uint32_t T = 0; while (ksh_snapshot_name(snap, 4, T, 0)) ++T;
  const uint32_t words = (T + 63) / 64; const size_t W = KS_CMD_ROW_WORDS(words);

  /* one candidate set per state node */
  uint32_t* off = (uint32_t*)malloc(sizeof(uint32_t) * (n_nodes + 1)); uint32_t* cand = (uint32_t*)malloc(sizeof(uint32_t) * (n_nodes + 1));
  for (i = 0; i <= n_nodes; ++i) { off[i] = i; cand[i] = i; }
  uint64_t* rows = (uint64_t*)malloc(sizeof(uint64_t) * W * (n_nodes + 1));
  double ms[5];
  if (ksh_consolidation_commands(snap, 0, n_nodes, off, cand, pod_node, NULL, 0, 0 /* device */, 0 /* computeConsolidation alone */, rows, words, ms) != KS_OK) {
    fprintf(stderr, "commands: %s\n", ksh_last_error()); return 1;
  }
  for (i = 0; i < n_nodes; ++i) { printf("command %u: ", (unsigned)rows[i * W + KS_CMD_ID]); print_row(snap, rows + i * W, words, cand + i, 1); }

  if (ksh_single_node_option(snap, 0, cand, n_nodes, pod_node, NULL, 0, 0, rows, words, NULL) != KS_OK) { fprintf(stderr, "single: %s\n", ksh_last_error()); return 1; }
  printf("single node option: "); print_row(snap, rows, words, cand + rows[KS_CMD_ID], 1);

  /* a row one word too short is refused before anything is opened */
  if (words && ksh_consolidation_commands(snap, 0, n_nodes, off, cand, pod_node, NULL, 0, 0, 0, rows, words - 1, NULL) != KS_ERR_INVALID) { fprintf(stderr, "a short row was taken\n"); return 1; }
  printf("refused: %s\n", ksh_last_error());

  /* libksolve alone: the snapshot's flat problem without its prices is refused by the command call, nothing launched */
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  ks_problem bare = *ksh_problem(h); bare.it_price = NULL; bare.it_price_lo = NULL;
  ks_dev_problem* d = NULL;
  if (ks_problem_upload(&bare, 0, &d) != KS_OK) { fprintf(stderr, "upload: %s\n", ks_last_error()); return 1; }
  const uint64_t id0 = 0; const uint32_t flag0 = 0, toff[2] = {0, 0}; const double price0 = 1.0;
  ks_command_inputs in; memset(&in, 0, sizeof in); in.flags = &flag0; in.cand_price = &price0; in.type_off = toff;
  ks_dev_problem* ds[1]; ds[0] = d;
  if (ks_consolidation_commands_host(ds, 1, &id0, &in, words, rows, NULL) != KS_ERR_INVALID) { fprintf(stderr, "a problem without prices was taken\n"); return 1; }
  printf("refused without prices: %s\n", ks_last_error());
  ks_problem_free(d); ksh_close(h);

  free(rows); free(off); free(cand); free(pod_node); ksh_parsed_free(snap); free(text);
  return 0;
}
