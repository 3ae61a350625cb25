/* A plain C99 translation unit that asks for the candidates of the three methods the deprovisioning controller tries before consolidation, the way a cgo shim would
 * (INTEGRATION.md section 2): a cluster snapshot in (KSP1 text and the node of every bound pod), `now` and the nodes' creation and emptiness times as unix nanoseconds,
 * the annotation flags, the provisioners' ttls; ksh_deprovisioning_candidates once per method, every node's reason printed; Emptiness.ComputeCommand through
 * ksh_emptiness_command, Expiration's and Drift's through ksh_replacement_option (one what-if simulated each).  Then one refusal: a ttl at which Go's Duration wraps.  Compiled and run by tests/test_deprovisioning_candidates.py. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

int main(int argc, char** argv) {
  if (argc < 3) { fprintf(stderr, "usage: cabi_usage_deprovisioning <snapshot.ksp> <now, unix ns> <node of pod 0> <node of pod 1> ...\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);
  const int64_t now = (int64_t)strtoll(argv[2], NULL, 10), second = 1000000000;

  void* snap = NULL;
  if (ksh_parse(text, (size_t)n, &snap) != KS_OK) { fprintf(stderr, "parse: %s\n", ksh_last_error()); return 1; }
  uint32_t n_pods = 0, n_nodes = 0, i, k, m;
  if (ksh_snapshot_bindings(snap, NULL, 0, &n_pods, &n_nodes) != KS_OK) return 1;
  if ((uint32_t)(argc - 3) != n_pods || n_nodes != 4) { fprintf(stderr, "%u pods, %d bindings, %u nodes\n", n_pods, argc - 3, n_nodes); return 2; }
  int32_t* pod_node = (int32_t*)malloc(sizeof(int32_t) * (n_pods + 1));
  for (i = 0; i < n_pods; ++i) pod_node[i] = (int32_t)atoi(argv[3 + i]);

  /* what the snapshot's objects do not carry: n0 was created 100 s ago, n1 50 s, n2 5 s, n3 100 s; n2 carries karpenter.sh/voluntary-disruption=drifted and an
     emptiness timestamp of 100 s ago; provisioner 0: ttlSecondsUntilExpired 10, ttlSecondsAfterEmpty 30; provisioner 1: neither */
  uint32_t node_flags[4] = {0, 0, KSH_CAND_NODE_DRIFTED | KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP, 0}; double age[4] = {0.0, 0.0, 0.0, 0.0};
  int64_t creation[4], emptiness[4] = {0, 0, 0, 0};
  creation[0] = now - 100 * second; creation[1] = now - 50 * second; creation[2] = now - 5 * second; creation[3] = now - 100 * second; emptiness[2] = now - 100 * second;
  uint32_t* pod_flags = (uint32_t*)calloc(n_pods + 1, sizeof(uint32_t)); double* dcost = (double*)calloc(n_pods + 1, sizeof(double)); int32_t* prio = (int32_t*)calloc(n_pods + 1, sizeof(int32_t));
  int64_t ttl[2] = {10, -1}; const int64_t ttl_empty[2] = {30, -1};
  ksh_deprovisioning_inputs in; memset(&in, 0, sizeof in);
  in.base.n_nodes = n_nodes; in.base.n_pods = n_pods; in.base.n_provisioners = 2;
  in.base.node_flags = node_flags; in.base.node_age_seconds = age; in.base.pod_flags = pod_flags; in.base.pod_deletion_cost = dcost; in.base.pod_priority = prio;
  in.base.prov_ttl_seconds_until_expired = ttl;      /* (prov_consolidation_enabled is not read by these methods) */
  in.now_unix_nanos = now; in.node_creation_unix_nanos = creation; in.node_emptiness_unix_nanos = emptiness; in.prov_ttl_seconds_after_empty = ttl_empty; in.drift_enabled = 1;

  ksh_deprovisioning_out out; memset(&out, 0, sizeof out);
  out.base.order = (uint32_t*)calloc(n_nodes, sizeof(uint32_t)); out.base.empty = (uint32_t*)calloc(n_nodes, sizeof(uint32_t)); out.base.why = (uint32_t*)calloc(n_nodes, sizeof(uint32_t));
  out.base.detail = (int32_t*)calloc(n_nodes, sizeof(int32_t)); out.base.n_node_pods = (uint32_t*)calloc(n_nodes, sizeof(uint32_t)); out.base.cost = (double*)calloc(n_nodes, sizeof(double));
  static const uint32_t methods[3] = {KSH_METHOD_EXPIRATION, KSH_METHOD_DRIFT, KSH_METHOD_EMPTINESS};
  static const char* const names[3] = {"expiration", "drift", "emptiness"};
  for (m = 0; m < 3; ++m) {      /* the controller's order (controller.go:142-162 lists expiration, drift, emptiness ahead of consolidation) */
    double ms[4];
    if (ksh_deprovisioning_candidates(snap, methods[m], pod_node, NULL, 0, &in, NULL /* no PDBs */, 0 /* device */, &out, ms) != KS_OK) { fprintf(stderr, "%s: %s\n", names[m], ksh_last_error()); return 1; }
    printf("%s: in result %u order:", names[m], (unsigned)out.n_in_result);
    for (i = 0; i < out.base.n_candidates; ++i) printf(" %s", ksh_snapshot_name(snap, 3, out.base.order[i], 0));
    printf("\n");
    if (methods[m] != KSH_METHOD_EMPTINESS && out.n_in_result != 0) {
      /* ComputeCommand for expiration and drift: the first candidate of `order` that may be terminated and is not deleting is simulated, alone; its command comes
         back as one head and one fixed-size row per replacement node (words = 1: two instance types) */
      uint64_t head[KS_REP_HEAD_WORDS], rows[8 * (KS_REP_NODE_OPTIONS + 1)], total = 0; int32_t pos = -2;
      if (ksh_replacement_option(snap, 0, out.base.order, out.base.n_candidates, out.base.why, pod_node, NULL, 0, 0, head, rows, 8, &total, &pos, 1, NULL) != KS_OK) {
        fprintf(stderr, "%s option: %s\n", names[m], ksh_last_error()); return 1; }
      const unsigned action = (unsigned)(head[KS_REP_DECISION] & 0xff);
      printf("%s command: %s", names[m], action == KS_CMD_DELETE ? "delete" : action == KS_CMD_REPLACE ? "replace" : action == KS_CMD_DO_NOTHING ? "do-nothing" : "error");
      if (pos >= 0) printf(" %s with %u nodes", ksh_snapshot_name(snap, 3, out.base.order[pos], 0), (unsigned)head[KS_REP_N_NODES]);
      for (i = 0; i < (uint32_t)head[KS_REP_N_NODES] && i < 8; ++i) {      /* each row: the options as a bit mask over the catalogue, the requests by resource name */
        const uint64_t* row = rows + (size_t)(head[KS_REP_NODE_OFF] + i) * (KS_REP_NODE_OPTIONS + 1);
        printf(" [node %u: %u options, %s %ld]", (unsigned)(row[KS_REP_NODE_ID] >> 32), (unsigned)row[KS_REP_NODE_N_OPTIONS], ksh_snapshot_name(snap, 2, 2, 0), (long)row[KS_REP_NODE_REQ + 2]);
      }
      printf("\n");
    }
    for (i = 0; i < n_nodes; ++i) {
      unsigned char b[8]; memcpy(b, &out.base.cost[i], 8);
      printf("%s %s: why %u detail %d pods %u cost ", names[m], ksh_snapshot_name(snap, 3, i, 0), (unsigned)out.base.why[i], (int)out.base.detail[i], (unsigned)out.base.n_node_pods[i]);
      for (k = 0; k < 8; ++k) printf("%02x", b[k]);
      printf("\n");
    }
  }
  /* the last call was emptiness: its order is the whole command */
  uint32_t action = 99, n_remove = 0, remove[4];
  if (ksh_emptiness_command(out.base.order, out.base.n_candidates, out.base.n_node_pods, &action, remove, &n_remove) != KS_OK) return 1;
  printf("emptiness command: %s", action == KS_CMD_DELETE ? "delete" : "do-nothing");
  for (i = 0; i < n_remove; ++i) printf(" %s", ksh_snapshot_name(snap, 3, remove[i], 0));
  printf("\n");

  /* a ttl above 9 223 372 036 s: Duration(ttl) * time.Second wraps there; refused before anything is launched */
  ttl[0] = 9223372037;
  if (ksh_deprovisioning_candidates(snap, KSH_METHOD_EXPIRATION, pod_node, NULL, 0, &in, NULL, 0, &out, NULL) != KS_ERR_INVALID) { fprintf(stderr, "a wrapping ttl was taken\n"); return 1; }
  printf("refused: %s\n", ksh_last_error());

  free(out.base.order); free(out.base.empty); free(out.base.why); free(out.base.detail); free(out.base.n_node_pods); free(out.base.cost);
  free(pod_flags); free(dcost); free(prio); free(pod_node); ksh_parsed_free(snap); free(text);
  return 0;
}
