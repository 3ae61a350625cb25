/* A plain C99 translation unit that keeps a snapshot current through the BINARY events door (kshost.h ksh_env_apply_block) the way a cgo shim would
 * (INTEGRATION.md section 2): a block of two events -- a node joins, a pod is bound to it -- is built by hand and applied; the same two events go through
 * the text door (ksh_env_apply) into a twin, and the two snapshots must flatten alike.  A block whose n_events does not match its stream is refused with
 * nothing applied.  Compiled and run by tests/test_env_apply_block.py; no GPU is needed. */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "ksolve.h"
#include "kshost.h"

int main(int argc, char** argv) {
  if (argc < 2) { fprintf(stderr, "usage: cabi_usage_delta <environment.ksp>\n"); return 2; }
  FILE* f = fopen(argv[1], "rb"); if (!f) return 2;
  fseek(f, 0, SEEK_END); long n = ftell(f); fseek(f, 0, SEEK_SET);
  char* text = (char*)malloc((size_t)n + 1); if (fread(text, 1, (size_t)n, f) != (size_t)n) return 2; text[n] = 0; fclose(f);

  void* snap = NULL; void* twin = NULL;                 /* a snapshot with no state nodes and no bound pods yet */
  if (ksh_parse(text, (size_t)n, &snap) != KS_OK || ksh_parse(text, (size_t)n, &twin) != KS_OK) { fprintf(stderr, "parse: %s\n", ksh_last_error()); return 1; }

  /* string table: 0 "node-a", 1 "kubernetes.io/hostname", 2 "cpu", 3 "default", 4 "pod-a" */
  const char strs[] = "node-a" "kubernetes.io/hostname" "cpu" "default" "pod-a";
  const uint32_t str_off[6] = {0, 6, 28, 31, 38, 43};
  const uint32_t words[] = {
      KSH_EVENT_NODE_ADD, 0 /*name*/, 1 /*in state*/, 1 /*labels*/, 1, 0 /*hostname = node-a*/, 0 /*taints*/,
      1 /*available*/, 2 /*"cpu"*/, 4000, 0 /*4 cpu in milli-units, low and high word*/, 1 /*capacity*/, 2, 4000, 0, 0 /*daemonset requests*/,
      0 /*host ports*/, 0 /*volume limits*/, 0 /*volumes*/,
      KSH_EVENT_BIND, 0 /*node name*/, 20 /*words of the spec record*/,
      3 /*ns*/, 0 /*labels*/, 0 /*nodeSelector*/, 0 /*required terms*/, 0 /*preferred terms*/, 0 /*tolerations*/,
      1 /*containers*/, 1 /*requests*/, 2 /*"cpu"*/, 100, 0 /*100 milli*/, 0 /*limits*/, 0 /*ports*/,
      0 /*init containers*/, 0 /*spread*/, 0, 0, 0, 0 /*pod (anti-)affinity*/, 0 /*volumes*/,
      4 /*uid*/, 0, 0 /*creationTimestamp*/};
  ksh_delta_block d; memset(&d, 0, sizeof d);
  d.n_events = 2; d.n_strings = 5; d.n_words = (uint32_t)(sizeof words / sizeof words[0]); d.str_off = str_off; d.str_bytes = strs; d.words = words; d.str_bytes_len = sizeof strs - 1;

  uint32_t info[4];
  d.n_events = 3;                                       /* one event more than the stream holds: refused, nothing applied */
  if (ksh_env_apply_block(snap, NULL, &d, 0, info) != KS_ERR_INVALID || info[0] != 0) { fprintf(stderr, "a malformed block was taken\n"); return 1; }
  printf("refused: %s\n", ksh_last_error());
  uint32_t np = 9, nn = 9;
  if (ksh_snapshot_bindings(snap, NULL, 0, &np, &nn) != KS_OK || np != 0 || nn != 0) { fprintf(stderr, "the refused block left something behind\n"); return 1; }
  d.n_events = 2;
  if (ksh_env_apply_block(snap, NULL /* no pods yet: no bindings to hand over */, &d, 0, info) != KS_OK) { fprintf(stderr, "apply: %s\n", ksh_last_error()); return 1; }
  printf("applied %u events: %u nodes %u pods\n", info[0], info[1], info[2]);
  int32_t bind[1] = {-7};
  if (ksh_snapshot_bindings(snap, bind, 1, &np, &nn) != KS_OK || np != 1 || nn != 1 || bind[0] != 0) { fprintf(stderr, "bindings: %s\n", ksh_last_error()); return 1; }

  /* the text door takes the same two events; both snapshots flatten to the same arrays */
  const char ksd[] = "KSD1 2\n"
                     "NODE+ node-a 1 1 kubernetes.io/hostname node-a 0 1 cpu 4 1 cpu 4 0 0 VL 0 VU 0\n"
                     "BIND node-a POD pod-a default 0 L 0 NS 0 RA 0 PA 0 TOL 0 C 1 1 cpu 100m 0 0 I 0 TS 0 AFR 0 AFP 0 ANR 0 ANP 0 VOL 0\n"
                     "END\n";
  if (ksh_env_apply(twin, NULL, ksd, sizeof ksd - 1, info) != KS_OK) { fprintf(stderr, "text apply: %s\n", ksh_last_error()); return 1; }
  uint64_t fa = 0, fb = 1;
  if (ksh_snapshot_fingerprint(snap, NULL, 0, 0, &fa) != KS_OK || ksh_snapshot_fingerprint(twin, NULL, 0, 0, &fb) != KS_OK) { fprintf(stderr, "fingerprint: %s\n", ksh_last_error()); return 1; }
  printf("binary and text door: %s flattening\n", fa == fb ? "the same" : "ANOTHER");

  ksh_parsed_free(snap); ksh_parsed_free(twin); free(text);
  return fa == fb ? 0 : 1;
}
