/* A plain C99 translation unit that gates a result the way a shim would ("the audit gate"), with the five passes: solve over a handle, ksh_audit,
 * ksh_audit_topology, ksh_audit_spread, ksh_audit_firstfit, then ksh_audit_limits, and act only if none flags anything.  Then the form for a result from anywhere: the
 * result's arrays (ksh_result_arrays_get) and its commit numbers, read through ksh_placement_rows (KS_PLC_STAGE_SEQ), audited back as CLAIMED -- clean --, and twice
 * more with an edit the first four passes say nothing about: new node argv[2] billed to template 0, the limited provisioner's (KS_AUDIT_NODE_LIMIT_EXTRA), and new node
 * argv[3] reduced to the one type argv[4] (KS_AUDIT_NODE_LIMIT_MISSING).  Compiled and run by tests/test_audit_limits_cabi.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

static void* take(size_t bytes) { return calloc(bytes ? bytes : 1, 1); }

/* the first four passes over a claimed result: the pods and nodes they flag, or -1 */
static int others(void* h, const ksh_result_arrays* ra, const int32_t* seq) {
  ksh_audit_out a; ksh_audit_topology_out t; ksh_audit_spread_out s; ksh_audit_firstfit_out ff;
  memset(&a, 0, sizeof a); memset(&t, 0, sizeof t); memset(&s, 0, sizeof s); memset(&ff, 0, sizeof ff);
  if (ksh_audit_claimed(h, ra, &a, NULL) != KS_OK || ksh_audit_topology_claimed(h, ra, seq, &t, NULL) != KS_OK || ksh_audit_spread_claimed(h, ra, seq, &s, NULL) != KS_OK ||
      ksh_audit_firstfit_claimed(h, ra, seq, &ff, NULL) != KS_OK) { fprintf(stderr, "claimed: %s\n", ksh_last_error()); return -1; }
  return (int)(a.n_pods_flagged + a.n_nodes_flagged + t.n_pods_flagged + s.n_pods_flagged + ff.n_pods_flagged);
}

int main(int argc, char** argv) {
  if (argc < 5) { fprintf(stderr, "usage: cabi_usage_audit_limits <problem.ksp> <new node to bill to template 0> <new node to reduce> <the type it keeps>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const uint32_t billed = (uint32_t)atoi(argv[2]), reduced = (uint32_t)atoi(argv[3]), kept = (uint32_t)atoi(argv[4]);
  void* h = NULL;
  if (ksh_open(text, (size_t)n, 0, &h) != KS_OK) { fprintf(stderr, "open: %s\n", ksh_last_error()); return 1; }
  if (ksh_solve(h, NULL, NULL, NULL) != KS_OK) { fprintf(stderr, "ksh_solve: %s\n", ksh_last_error()); return 1; }

  /* the gate: the five passes over the result where it lies.  Totals always; the flag rows only when the tables hold them */
  ksh_audit_out a; memset(&a, 0, sizeof a);
  ksh_audit_topology_out t; memset(&t, 0, sizeof t);
  ksh_audit_spread_out s; memset(&s, 0, sizeof s);
  ksh_audit_firstfit_out ff; memset(&ff, 0, sizeof ff);
  ksh_audit_limits_out lm; memset(&lm, 0, sizeof lm);
  if (ksh_audit(&h, 1, &a, NULL) != KS_OK) { fprintf(stderr, "ksh_audit: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_topology(&h, 1, &t, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_topology: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_spread(&h, 1, &s, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_spread: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_firstfit(&h, 1, &ff, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_firstfit: %s\n", ksh_last_error()); return 1; }
  if (ksh_audit_limits(&h, 1, &lm, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_limits: %s\n", ksh_last_error()); return 1; }
  const unsigned found = a.n_pods_flagged + a.n_nodes_flagged + t.n_pods_flagged + s.n_pods_flagged + ff.n_pods_flagged + lm.n_pods_flagged + lm.n_nodes_flagged;
  printf("genuine: %u + %u + %u + %u + %u of %u pods, %u + %u of %u nodes flagged, truncated %u -> %s\n", a.n_pods_flagged, t.n_pods_flagged, s.n_pods_flagged, ff.n_pods_flagged,
         lm.n_pods_flagged, lm.n_pods, a.n_nodes_flagged, lm.n_nodes_flagged, lm.n_nodes, lm.truncated, found ? "solve in Go" : "act");
  printf("evaluated: %u limited templates, %u placed pods, %u nodes, %u pods, %u pairs; %u exact, %u binding, %u + %u skipped\n", lm.limited_templates, lm.checked[0], lm.checked[1],
         lm.checked[2], lm.checked[3], lm.exact_nodes, lm.binding_nodes, lm.skipped_nodes, lm.skipped_pods);
  const uint32_t P = lm.n_pods, NS = lm.n_nodes;

  /* the commit numbers of that result: one placement row per pod */
  uint64_t id = 7, head[KS_PLC_HEAD_WORDS], total = 0;
  uint64_t* rows = (uint64_t*)take(8 * (size_t)P * KS_PLC_ROW_WORDS);
  if (ksh_placement_rows(&h, 1, &id, head, rows, P, &total, NULL) != KS_OK) { fprintf(stderr, "ksh_placement_rows: %s\n", ksh_last_error()); return 1; }
  int32_t* seq = (int32_t*)take(4 * (size_t)P);
  uint64_t k;
  for (k = 0; k < P; ++k) seq[k] = -1;
  for (k = 0; k < total; ++k) {
    const uint64_t* row = rows + k * KS_PLC_ROW_WORDS;
    seq[(uint32_t)row[KS_PLC_POD_WHERE]] = (int32_t)(uint32_t)(row[KS_PLC_STAGE_SEQ] >> 32);
  }
  ksh_result_arrays ra;
  if (ksh_result_arrays_get(h, &ra) != KS_OK) { fprintf(stderr, "ksh_result_arrays_get: %s\n", ksh_last_error()); return 1; }
  if (billed >= ra.n_new || reduced >= ra.n_new) return 2;

  lm.pod_flags = (uint32_t*)take(4 * (size_t)P); lm.cap_pods = P; lm.node_flags = (uint32_t*)take(4 * (size_t)NS); lm.cap_nodes = NS;
  if (ksh_audit_limits_claimed(h, &ra, seq, &lm, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_limits_claimed: %s\n", ksh_last_error()); return 1; }
  printf("claimed back: %u rows, %u pods and %u nodes flagged, truncated %u\n", (unsigned)total, lm.n_pods_flagged, lm.n_nodes_flagged, lm.truncated);

  /* a machine past the budget: new node `billed` charged to the limited provisioner */
  int32_t* tmpl = (int32_t*)take(4 * (size_t)ra.n_new);
  memcpy(tmpl, ra.node_tmpl, 4 * (size_t)ra.n_new);
  const int32_t* tmpl_was = ra.node_tmpl;
  tmpl[billed] = 0; ra.node_tmpl = tmpl;
  if (ksh_audit_limits_claimed(h, &ra, seq, &lm, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_limits_claimed: %s\n", ksh_last_error()); return 1; }
  printf("node %u billed to template 0: the other passes flag %d, this one %u nodes, the node carries %u -> %s\n", billed, others(h, &ra, seq), lm.n_nodes_flagged,
         lm.node_flags[ra.n_existing + billed], lm.n_nodes_flagged ? "solve in Go" : "act");
  ra.node_tmpl = tmpl_was;

  /* an option lost: new node `reduced` keeps type `kept` alone */
  uint64_t* types = (uint64_t*)take(8 * (size_t)ra.n_new * ra.types_words);
  memcpy(types, ra.node_types, 8 * (size_t)ra.n_new * ra.types_words);
  memset(types + (size_t)reduced * ra.types_words, 0, 8 * (size_t)ra.types_words);
  types[(size_t)reduced * ra.types_words + kept / 64] = (uint64_t)1 << (kept % 64);
  ra.node_types = types;
  if (ksh_audit_limits_claimed(h, &ra, seq, &lm, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_limits_claimed: %s\n", ksh_last_error()); return 1; }
  printf("node %u reduced to type %u: the other passes flag %d, this one %u nodes, the node carries %u -> %s\n", reduced, kept, others(h, &ra, seq), lm.n_nodes_flagged,
         lm.node_flags[ra.n_existing + reduced], lm.n_nodes_flagged ? "solve in Go" : "act");
  printf("no commit numbers: %d\n", ksh_audit_limits_claimed(h, &ra, NULL, &lm, NULL));      /* KS_ERR_INVALID */
  lm.cap_nodes = 1;      /* a node table too short: the totals still arrive */
  if (ksh_audit_limits_claimed(h, &ra, seq, &lm, NULL) != KS_OK) { fprintf(stderr, "ksh_audit_limits_claimed: %s\n", ksh_last_error()); return 1; }
  printf("a short node table: truncated %u, %u nodes flagged\n", lm.truncated, lm.n_nodes_flagged);
  free(types); free(tmpl); free(lm.pod_flags); free(lm.node_flags); free(seq); free(rows);
  ksh_close(h); free(text);
  return 0;
}
