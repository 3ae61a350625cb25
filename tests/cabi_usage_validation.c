/* A plain C99 translation unit that closes a consolidation pass the way a cgo shim would: commands at t0 (one candidate set per state node,
 * ksh_consolidation_commands), the cluster's events of the next 15 s applied to the same parsed snapshot (ksh_env_apply, KSD1 text from a file), then -- at
 * t0 + consolidationTTL -- candidates over the snapshot as it is now (ksh_consolidation_candidates) and every delete / replace of t0 validated against it in ONE call
 * (ksh_validate_commands).  Every verdict is printed with the names ksh_snapshot_name gives.  Compiled and run by tests/test_validate_commands.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static char* read_file(const char* path, size_t* len) {
  FILE* f = fopen(path, "rb"); long n; char* text;
  if (!f) return NULL;
  fseek(f, 0, SEEK_END); n = ftell(f); fseek(f, 0, SEEK_SET);
  text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) { fclose(f); return NULL; }
  text[n] = 0; fclose(f); *len = (size_t)n; return text;
}

int main(int argc, char** argv) {
  size_t n = 0, dn = 0; char *text, *delta; void* snap = NULL;
  uint32_t n_pods = 0, n_nodes = 0, i, t, T = 0, words, m = 0, info[4];
  if (argc < 3) { fprintf(stderr, "usage: cabi_usage_validation <snapshot.ksp> <events.ksd> <node of pod 0> <node of pod 1> ...\n"); return 2; }
  text = read_file(argv[1], &n); delta = read_file(argv[2], &dn); if (!text || !delta) return 2;
  if (ksh_parse(text, n, &snap) != KS_OK) { fprintf(stderr, "parse: %s\n", ksh_last_error()); return 1; }
  if (ksh_snapshot_bindings(snap, NULL, 0, &n_pods, &n_nodes) != KS_OK) return 1;
  if ((uint32_t)(argc - 3) != n_pods) { fprintf(stderr, "%u pods, %d bindings\n", n_pods, argc - 3); return 2; }
  {
    int32_t* pod_node = (int32_t*)malloc(sizeof(int32_t) * (n_pods + 1));
    uint32_t* off = (uint32_t*)malloc(sizeof(uint32_t) * (n_nodes + 1)); uint32_t* cand = (uint32_t*)malloc(sizeof(uint32_t) * (n_nodes + 1));
    uint64_t *rows, *vrows, *options; uint32_t *voff, *vnodes, *expect; size_t W, VW;
    for (i = 0; i < n_pods; ++i) pod_node[i] = (int32_t)atoi(argv[3 + i]);
    while (ksh_snapshot_name(snap, 4, T, 0)) ++T;
    words = (T + 63) / 64; W = KS_CMD_ROW_WORDS(words); VW = KS_VAL_ROW_WORDS(words);

    /* t0: one candidate set per state node */
    for (i = 0; i <= n_nodes; ++i) { off[i] = i; cand[i] = i; }
    rows = (uint64_t*)malloc(sizeof(uint64_t) * W * (n_nodes + 1));
    if (ksh_consolidation_commands(snap, 0, n_nodes, off, cand, pod_node, NULL, 0, 0, 0, rows, words, NULL) != KS_OK) { fprintf(stderr, "commands: %s\n", ksh_last_error()); return 1; }

    /* the deletes and replaces wait consolidationTTL; what a command keeps: its nodes (slots are stable across events) and its replacement's options */
    voff = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); vnodes = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t)); expect = (uint32_t*)calloc(n_nodes + 1, sizeof(uint32_t));
    options = (uint64_t*)calloc((size_t)(n_nodes + 1) * words, sizeof(uint64_t));
    for (i = 0; i < n_nodes; ++i) {
      const uint32_t action = (uint32_t)(rows[i * W + KS_CMD_DECISION] & 0xffu);
      if (action != KS_CMD_DELETE && action != KS_CMD_REPLACE) continue;
      vnodes[m] = i; expect[m] = action == KS_CMD_REPLACE;
      memcpy(options + (size_t)m * words, rows + i * W + KS_CMD_OPTIONS, sizeof(uint64_t) * words);
      ++m; voff[m] = m;
    }
    printf("%u commands wait\n", (unsigned)m);

    /* the 15 s in between: the cluster's events patch the same snapshot; from here on the library holds the bindings (pod_node = NULL) */
    if (ksh_env_apply(snap, pod_node, delta, dn, info) != KS_OK) { fprintf(stderr, "events: %s\n", ksh_last_error()); return 1; }
    printf("%u events applied: %u node slots, %u pod slots\n", (unsigned)info[0], (unsigned)info[1], (unsigned)info[2]);

    /* t0 + TTL: the candidates of the cluster as it is now, then every waiting command in one call */
    {
      const uint32_t nn = info[1], np = info[2], enabled = 1; const int64_t ttl = -1;
      uint32_t* zeros = (uint32_t*)calloc(nn + np + 1, sizeof(uint32_t)); double* dzeros = (double*)calloc(nn + np + 1, sizeof(double)); int32_t* izeros = (int32_t*)calloc(np + 1, sizeof(int32_t));
      uint32_t *order = (uint32_t*)calloc(nn + 1, sizeof(uint32_t)), *empty = (uint32_t*)calloc(nn + 1, sizeof(uint32_t)), *why = (uint32_t*)calloc(nn + 1, sizeof(uint32_t)),
               *npods = (uint32_t*)calloc(nn + 1, sizeof(uint32_t));
      int32_t* detail = (int32_t*)calloc(nn + 1, sizeof(int32_t)); double* cost = (double*)calloc(nn + 1, sizeof(double));
      ksh_candidate_inputs in; ksh_candidates_out out;
      memset(&in, 0, sizeof in); memset(&out, 0, sizeof out);
      in.n_nodes = nn; in.n_pods = np; in.n_provisioners = 1; in.node_flags = zeros; in.node_age_seconds = dzeros; in.pod_flags = zeros; in.pod_deletion_cost = dzeros;
      in.pod_priority = izeros; in.prov_consolidation_enabled = &enabled; in.prov_ttl_seconds_until_expired = &ttl;
      out.order = order; out.empty = empty; out.why = why; out.detail = detail; out.n_node_pods = npods; out.cost = cost;
      if (ksh_consolidation_candidates(snap, NULL, NULL, 0, &in, NULL, 0, &out, NULL) != KS_OK) { fprintf(stderr, "candidates: %s\n", ksh_last_error()); return 1; }
      vrows = (uint64_t*)malloc(sizeof(uint64_t) * VW * (m + 1));
      if (ksh_validate_commands(snap, 0, m, voff, vnodes, expect, options, why, zeros, NULL, NULL, 0, 0, vrows, words, NULL) != KS_OK) { fprintf(stderr, "validate: %s\n", ksh_last_error()); return 1; }
      for (i = 0; i < m; ++i) {
        const uint64_t* v = vrows + i * VW; const uint32_t verdict = (uint32_t)(v[KS_VAL_VERDICT] & 0xffu), step = (uint32_t)((v[KS_VAL_VERDICT] >> 8) & 0xffu);
        printf("validated %s: %s", ksh_snapshot_name(snap, 3, vnodes[v[KS_VAL_ID]], 0), verdict == KS_VAL_VALID ? "valid" : verdict == KS_VAL_ERROR ? "error" : "invalid");
        if (verdict != KS_VAL_VALID) printf(" (step %u)", (unsigned)step);
        if (v[KS_VAL_N_MISSING]) {
          printf(" missing %u:", (unsigned)v[KS_VAL_N_MISSING]);
          for (t = 0; t < T; ++t) if ((v[KS_VAL_OPTIONS + words + t / 64u] >> (t % 64u)) & 1u) printf(" %s", ksh_snapshot_name(snap, 4, t, 0));
        }
        printf("\n");
      }
      /* EmptyNodeConsolidation's own check over the same arrays: the waiting commands' nodes as one delete */
      { uint32_t retry = 0; if (ksh_validate_empty_nodes(vnodes, m, why, npods, zeros, &retry) != KS_OK) return 1; printf("as empty nodes: %s\n", retry ? "retry" : "delete"); }
      /* a row one word too short is refused before anything is simulated */
      if (words && m && ksh_validate_commands(snap, 0, m, voff, vnodes, expect, options, why, zeros, NULL, NULL, 0, 0, vrows, words - 1, NULL) != KS_ERR_INVALID) { fprintf(stderr, "a short row was taken\n"); return 1; }
      printf("refused: %s\n", ksh_last_error());
      free(zeros); free(dzeros); free(izeros); free(order); free(empty); free(why); free(npods); free(detail); free(cost); free(vrows);
    }
    free(rows); free(voff); free(vnodes); free(expect); free(options); free(off); free(cand); free(pod_node);
  }
  ksh_parsed_free(snap); free(text); free(delta);
  return 0;
}
