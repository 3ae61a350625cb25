/* kshost.h -- C ABI of libkshost.so: the host half of the MI355X drop-in for karpenter-core's provisioning scheduler.
 *
 * libksolve.so (include/ksolve.h) takes a FLAT problem (structure-of-arrays bitmasks).  libkshost.so is what produces it from the
 * objects a caller holds, i.e. the part of the reference that needs strings and maps and therefore stays on the host:
 *
 *   ksh_parse                 the caller's objects in memory ([]*v1.Pod, []*cloudprovider.InstanceType, []v1alpha5.Provisioner,
 *                             []*state.Node, the cluster pods countDomains would list): KSP1 text -> C++ objects.  (A Go shim would
 *                             build the same objects from its own structs; KSP1 -- grammar in karpenter_core_amd/model.py -- is the
 *                             wire form the Python mirror and the tests use.)
 *   ksh_solve_from_pods       provisioning.(*Provisioner).NewScheduler + scheduling.NewTopology + (*Scheduler).Solve for that pod
 *                             list: provisioner.go:237-296,301-307 / topology.go:56-117 / scheduler.go:42-133 (queue.go:35 NewQueue
 *                             included).  Flatten -> ks_problem_upload -> ks_feasibility_grid -> ks_solve_dev.
 *   ksh_open / ksh_upload / ksh_solve / ksh_solve_batch
 *                             the same in separate steps (flatten once, keep the problem resident in HBM, solve repeatedly / in batches).
 *   ksh_open_whatifs          deprovisioning.simulateScheduling's problem construction for N candidate sets over ONE cluster snapshot
 *                             (helpers.go:42-99): candidates leave the state nodes, their pods become the batch.
 *   ksh_price_filter          filterByPrice / worstLaunchPrice on results still on the device (helpers.go:148-157,292-315).
 *   ksh_consolidation_commands / ksh_first_n_node_option / ksh_single_node_option
 *                             computeConsolidation (consolidation.go:190-274) and the two searches built on it (multinodeconsolidation.go:74-165,
 *                             singlenodeconsolidation.go:54-78): snapshot and candidate sets in, fixed-size command rows out, decided on the device.
 *   ksh_validate_commands / ksh_single_node_resume / ksh_validate_empty_nodes
 *                             Validation.IsValid / ValidateCommand on the cluster as it is after consolidationTTL (validation.go:63-172), the rest of the single-node
 *                             loop (singlenodeconsolidation.go:54-84) and EmptyNodeConsolidation's own check (emptynodeconsolidation.go:77-87).
 *   ksh_result_text / ksh_result_summary
 *                             what callers read from Solve's return values: KSR1 text (Node.Pods, InstanceTypeOptions,
 *                             Requirements, Requests, ExistingNode.Pods, unscheduled queue, relaxation stages), or the fixed-size record
 *                             consolidation needs of a simulation.
 *
 * Conventions: every function returns KS_OK (0) or a negative KS_ERR_* (ksolve.h); ksh_last_error() gives the thread-local message.
 * Handles are opaque; buffers passed in are only read during the call; strings returned through char** are malloc'ed -> ksh_free.
 * There is no CPU scheduling path behind this ABI: without a gfx950 device every solving entry point fails with KS_ERR_DEVICE.
 * Re-entrancy: handles are independent; two threads may solve different handles concurrently (the reference runs the provisioner and
 * the deprovisioner as two goroutines: provisioner.go:102-104, deprovisioning/controller.go:103-105).
 */
#ifndef KSHOST_H
#define KSHOST_H
#include <stddef.h>
#include <stdint.h>

#include "ksolve.h"

#ifdef __cplusplus
extern "C" {
#endif

const char* ksh_last_error(void);
void ksh_free(char* p);

/* ---- objects in memory ----
 * A parsed object also keeps, behind a mutex, what later calls derive from it once: the flattening of its ENVIRONMENT (instance types, provisioners,
 * state nodes, daemonsets -- everything but the pods) for the universe signature of the last batch, which the next batch with the same label keys /
 * values / bounds / resources adopts instead of encoding the catalogue again (KSH_NO_ENV_CACHE=1 turns that off); and, for a cluster snapshot, its
 * own flattening, shared by the what-ifs over it.  It is otherwise immutable: any number of threads may use it at once. */
int ksh_parse(const char* ksp_text, size_t len, void** out_parsed);
void ksh_parsed_free(void* parsed);

/* ---- Solve() for a pod list the caller holds: flatten + upload + HIP kernels + read-back.
 * ms[6] (may be NULL): flatten | upload | static tables + feasibility grid | pack kernel (HIP events) | ks_solve_dev incl. read-back | total.
 * out_handle (may be NULL) receives a ksh_open-style handle holding the problem and its result (ksh_result_text, ksh_solve again, ...). */
int ksh_solve_from_pods(void* parsed, int device, uint32_t flags /* KS_FLAG_* */, void** out_handle, double* ms);

/* ---- binary pod ingress: the pending pods as flat arrays (no text) ----
 * What provisioner.go:301-307 hands to NewScheduler / Solve is a []*v1.Pod.  A cgo shim walks its pods once (one goroutine per block) and
 * fills, per BLOCK: a table of interned strings, per pod one record of u32 words (string ids, counts, int64 milli-quantities as two words;
 * grammar in karpenter_core_amd/host/kspb.hpp, field for field the KSP1 POD record), the uid (a string id) and the creationTimestamp.
 * ksh_pods_ingest copies what it keeps (the buffers are only read during the call -- the cgo pointer rule) and never builds one object
 * per pod: records that are equal word for word share one decoded spec.  The environment -- instance types, provisioners, state nodes,
 * cluster pods, daemonsets -- comes from ksh_parse (of a KSP1 text with `PODS 0`); it changes far less often than the pending batch.
 * ksh_solve_from_batch == ksh_solve_from_pods for that batch: same flat problem (ksh_fingerprint), same result. */
typedef struct ksh_pod_block {
  uint32_t n_pods, n_strings;
  const uint32_t* str_off;      /* [n_strings + 1] byte offsets into str_bytes */
  const char* str_bytes;
  const uint32_t* spec_off;     /* [n_pods + 1] word offsets into spec_words */
  const uint32_t* spec_words;
  const uint32_t* uid;          /* [n_pods] string ids */
  const int64_t* creation_ts;   /* [n_pods] */
  uint64_t str_bytes_len;       /* bytes behind str_bytes, words behind spec_words: a block whose offsets reach beyond them is refused (round 6; ADVICE r05: without them */
  uint64_t spec_words_len;      /* the library could only check that the offsets ascend) */
} ksh_pod_block;
int ksh_pods_ingest(const ksh_pod_block* blocks, uint32_t n_blocks, void** out_batch, double* ms /* ingest time or NULL */);
/* ---- binary ingress for the ENVIRONMENT (round 5): instance types + offerings (cloudprovider/types.go:72-145), provisioners (machinetemplate.go:46-62), state nodes
 * (state/node.go:61-159), the cluster's pods with required anti-affinity (topology.go:231-276), daemonset pods, SimulationMode -- ONE stream of u32 words over ONE string
 * table (grammar: karpenter_core_amd/host/kspb.hpp, EnvReader).  The handle is what ksh_parse returns for the KSP1 text of the same objects with `PODS 0`: the environment
 * argument of ksh_solve_from_batch / ksh_open_batch, freed by ksh_parsed_free.  No text is written or parsed on this path. */
typedef struct ksh_env_block {
  uint32_t n_strings, n_words;
  const uint32_t* str_off;      /* [n_strings + 1] byte offsets into str_bytes */
  const char* str_bytes;
  const uint32_t* words;        /* [n_words] */
  uint64_t str_bytes_len;       /* bytes behind str_bytes: str_off[n_strings] must not reach beyond */
} ksh_env_block;
int ksh_env_ingest(const ksh_env_block* env, void** out_parsed, double* ms /* ingest time or NULL */);
void ksh_pods_free(void* batch);
int ksh_pods_count(void* batch, uint32_t* n_pods, uint32_t* n_specs);
int ksh_solve_from_batch(void* parsed_env, void* batch, int device, uint32_t flags, void** out_handle, double* ms /* as ksh_solve_from_pods */);
int ksh_open_batch(void* parsed_env, void* batch, uint32_t flags, void** out_handle);   /* flatten only (no GPU needed) */
int ksh_open_parsed(void* parsed, uint32_t flags, void** out_handle);                   /* ksh_open for objects already held (ksh_parse) */

/* ---- the same in steps ---- */
int ksh_open(const char* ksp_text, size_t len, uint32_t flags, void** out_handle);      /* parse + flatten (no GPU needed) */
void ksh_close(void* handle);
const ks_problem* ksh_problem(void* handle);                                           /* the flat problem (owned by the handle) */
/* ---- the result as arrays (round 5): what Scheduler.Solve returns (scheduler.go:96: []*Node, []*ExistingNode; Node.Pods / InstanceTypeOptions / Requirements / Requests,
 * machinetemplate.go:77-100 reads them) without the KSR1 text.  Pointers into the handle's result buffers, valid until the handle is solved again or closed.  Node n of the
 * CSR: existing node n (caller's state-node order) for n < n_existing, else new node n - n_existing (creation order); its pods are pod indices (caller's order) in COMMIT
 * order (Node.Pods).  node_types: bit i = the caller's instance type i (the shim keeps the provisioner's own order when it filters: lo.Filter, node.go:138).  Requirement
 * records are masks over a key's interned values: ksh_name(handle, 0, k, 0) names key k, ksh_name(handle, 1, k, v) value v (a key encoded over value classes names one
 * member per class: such keys -- only reachable through Gt / Lt on labels with more than 64 values -- are listed in full by ksh_result_text), ksh_name(handle, 2, r, 0)
 * resource r.  Not for what-ifs derived on the device (their consumer reads ksh_result_summaries' fixed-size records). */
typedef struct ksh_result_arrays {
  uint32_t n_pods, n_existing, n_new, n_unscheduled, types_words, n_resources, n_keys, pad;
  const int32_t* pod_node;                 /* [n_pods] -1 unscheduled | existing node e | n_existing + new node j */
  const int32_t* pod_stage;                /* [n_pods] the relaxation stage the pod ended at (Preferences.Relax, preferences.go:36-56: the shim applies it back to pod.Spec) */
  const uint32_t* pod_reason;              /* [n_pods] ks_result.pod_reason (KS_WHY_* per machine template) for recordSchedulingResults (scheduler.go:135-172) */
  const int32_t* unscheduled;              /* [n_unscheduled] the queue as Solve left it (queue.go:70-72) */
  const uint32_t* node_pods_off;           /* [n_existing + n_new + 1] */
  const int32_t* node_pods;                /* pod indices, node by node, commit order */
  const int32_t* node_tmpl;                /* [n_new] machine template = provisioner in weight order */
  const uint64_t* node_types;              /* [n_new][types_words] InstanceTypeOptions */
  const int64_t* node_requests; const uint32_t* node_requests_present;      /* [n_new][n_resources] milli-units | bit r: the resource is in the list */
  const uint32_t* node_present; const uint32_t* node_complement; const uint64_t* node_mask; const int32_t* node_gt; const int32_t* node_lt;   /* [n_new](*[n_keys]) Requirements after FinalizeScheduling */
  const int32_t* node_it_state;            /* [n_new] the requirement on the instance-type key as a lattice state (0: none; ksh_result_text spells it out) */
} ksh_result_arrays;
int ksh_result_arrays_get(void* handle, ksh_result_arrays* out);
const char* ksh_name(void* handle, int what /* 0 key, 1 value b of key a, 2 resource */, uint32_t a, uint32_t b);
int ksh_pack_width(void* handle, int* out);                                              /* ks_problem_pack_width of the handle's device problem: 4, 8 or 16 (the wide variants), 0 if ks_pack_rr took the last solve */
int ksh_pack_lean(void* handle, int* out);                                               /* ks_problem_pack_lean of the handle's device problem: 1 if the ks_pack variant of the last solve was a LEAN one (width 4, or 8 under KSH_ACTIVE_RESOURCES) */
int ksh_pack_row(void* handle, int* out);                                                /* ks_problem_pack_row of the handle's device problem: the row of the ks_pack instantiation table the last solve launched, -1 if ks_pack_rr took it or nothing ran */
int ksh_rr_status(void* handle, int out[2]);                                           /* ks_problem_rr_status of the handle's device problem: out[0] ks_pack_rr was launched, out[1] why it declined (0: it took the Solve) */
void ksh_dims(void* handle, uint32_t dims[10]);                                        /* P,C,T,M,E,K,R,G,GH,S */
uint64_t ksh_fingerprint(void* handle);                                                /* hash of every array of the flat problem */
int ksh_upload(void* handle, int device);                                              /* idempotent; a second call with another device is an error */
int ksh_upload_batch(void** handles, uint32_t n, int device, uint32_t nthreads);       /* the same for a batch, on host threads (0 = all usable cores) */
/* Solve / grid on a handle that was not uploaded yet use the calling thread's current HIP device. */
int ksh_solve(void* handle, char** out_text /* KSR1 or NULL */, float* kernel_ms, double* wall_ms);
int ksh_solve_batch(void** handles, uint32_t n, char** out_texts /* n entries or NULL */, float* kernel_ms, double* wall_ms);
int ksh_grid(void* handle, uint64_t* out /* [M][C][ceil(T/64)] or NULL */, float* kernel_ms);
/* The grid's rows split over GPUs (ks_feasibility_grid_rows / _install of ksolve.h for a handle): rows [row_lo, row_hi) of the M * C rows computed on the
 * handle's device and copied out (host and / or device destination, either may be NULL); rows computed elsewhere installed (complete != 0 with the last of them). */
int ksh_grid_rows(void* handle, uint32_t row_lo, uint32_t row_hi, uint64_t* out_rows, void* out_rows_dev, float* kernel_ms);
int ksh_grid_install(void* handle, uint32_t row_lo, uint32_t row_hi, const uint64_t* rows, const void* rows_dev, int complete);
/* Diagnostics.  ksh_debug_grid: ks_debug_grid of ksolve.h for a handle -- the grid as the last build left it (a batch's included), read-only, nothing launched;
 * KS_ERR_INVALID before an upload or while the grid is not built.  ksh_debug_pod_classes: out[i] = the pod class (grid row c, before relaxation) of pod i of the
 * handle's problem, in the caller's pod order; KS_ERR_UNSUPPORTED for a what-if derived on the device (it has no flattening of its own). */
int ksh_debug_grid(void* handle, uint64_t* out /* [M][C][ceil(T/64)] */);
int ksh_debug_pod_classes(void* handle, uint32_t* out /* [P] */);
/* ksh_debug_classes: the per-class records the pack kernels take their shortcuts from (csrc/ksolve.hip ClsBrief, 128 bytes each, and ClsPlan), as the last build left
 * them -- the handle's own, or the batch's it was solved in; built first only if nothing has built them yet.  Either destination may be NULL.  Returns sizeof(ClsPlan)
 * (> 0: a caller that mirrors the layout checks it against its own), or KS_ERR_INVALID before an upload. */
int ksh_debug_classes(void* handle, void* briefs /* [C] ClsBrief or NULL */, void* plans /* [C] ClsPlan or NULL */);
int ksh_solve_ksp(const char* ksp_text, size_t len, uint32_t flags, char** out_text);  /* one shot: KSP1 in, KSR1 out */

/* ---- results ---- */
int ksh_result_text(void* handle, char** out_text);
int ksh_result_summary(void* handle, uint64_t* out /* [2 + words]: n_new, n_unscheduled, new node 0's InstanceTypeOptions */, uint32_t words);
int ksh_result_summaries(void** handles, uint32_t n, uint64_t* out /* [n][2 + words] */, uint32_t words);

/* the batched launch with the results LEFT ON THE DEVICE (only error words come back), and the batch's fixed-size records built there into a
 * caller-owned device buffer d_out[n][3 + words] of uint64: [ids[i], n_new, n_unscheduled, new node 0's InstanceTypeOptions] -- the payload of
 * the one all-gather a what-if fan-out needs, with no host hop */
int ksh_solve_batch_resident(void** handles, uint32_t n, float* kernel_ms, double* wall_ms);
int ksh_result_records_dev(void** handles, uint32_t n, const uint64_t* ids, uint32_t words, void* d_out);
/* ... and the fan-out over several GPUs in one call (ks_solve_batch_sharded, include/ksolve.h): shard s = handles[shard_off[s] .. shard_off[s + 1]), all of a shard resident on
 * one device; ks_deal_lpt (ksolve.h) deals what-ifs to shards by predicted work.  out_rows[n][3 + words], ordered by id. */
int ksh_solve_whatifs_sharded(void** handles, const uint32_t* shard_off, uint32_t nshards, const uint64_t* ids, uint32_t words, uint64_t* out_rows, float* kernel_ms_max);

/* ---- consolidation ---- */
int ksh_open_whatifs(const char* snapshot_text, size_t len, uint32_t flags, uint32_t n, const uint32_t* cand_off /* [n+1] */, const uint32_t* cand,
                     const int32_t* pod_node /* node index of every snapshot pod */, uint32_t nthreads /* 0 = all usable cores */, void** out_handles /* [n] */);
int ksh_price_filter(void** handles, uint32_t n, const uint32_t* node, const double* max_price, const uint32_t* spot_only /* or NULL */,
                     uint64_t* out_masks, uint32_t stride_words, uint32_t* out_counts);

/* launch-time pick of the in-memory provider (fake/cloudprovider.go:79-84) / instanceTypesAreSubset (helpers.go:118-122), on device-resident results */
int ksh_launch_pick(void** handles, uint32_t n, const uint32_t* node, int32_t* out_type, int32_t* out_zone, int32_t* out_ct, double* out_price);
const char* ksh_key_value(void* handle, int which /* 0 zone, 1 capacity-type */, int32_t value_id);
int ksh_types_subset(void** handles, uint32_t n, const uint32_t* node, const uint64_t* lhs, uint32_t stride_words, uint32_t* out);
/* What-ifs DERIVED on the device from the resident snapshot (ksolve.h ks_whatifs_open; SURVEY 8b `ks_solve_batch(shared, whatif deltas, ...)`): no
 * per-what-if flattening on the host, an upload of KBs (candidate masks, remainingResources, descriptors); the handles come back already resident on
 * `device`.  Results read exactly like those of ksh_open_whatifs_parsed.  Bound pods may carry spread / affinity / preferred terms: which groups a
 * what-if starts with and what countDomains finds for it follow from per-node tables of the snapshot (ks_whatif_topo).  Required anti-affinity is covered as well: an inverse group
 * exists only while an owner is in the batch or stays bound (decided per what-if on the device; the evaluation skips a group that does not exist), and the
 * staying owners are counted per node.  KS_ERR_UNSUPPORTED -- nothing opened -- where a what-if depends on its candidate set in other ways: more than 1024
 * groups, one spread group shared by pods whose node filters differ, volume limits / claims (without KSH_DERIVE_VOLUMES).  Use ksh_open_whatifs_parsed then.
 *
 * KSH_DERIVE_VOLUMES (opt-in; a bit no KS_FLAG_* uses, never passed on to the flat problem): snapshots with CSI volume limits and / or claims are derived too.
 * The snapshot is then flattened with a partition of its claims that does not depend on the candidate set: a SOLO claim -- mounted by
 * exactly one bound pod and listed on no state node but that pod's -- is a per-driver count in the pod's volume entries; every other claim a bound pod mounts
 * is a MULTI claim, one bit over a snapshot-wide universe in the per-node sets.  Each derived what-if carries its own per-node volume counts and sets
 * (ks_whatifs_open_ex with KS_WHATIFS_VOLUMES).  This flattening is kept apart from the flag-0 one (which ksh_snapshot_fingerprint(flags 0) hashes and
 * ksh_open_whatifs_parsed uses); KS_ERR_UNSUPPORTED still for more than 64 limited drivers, 2^24 multi claims, or per-what-if volume state above 64 MiB. */
#define KSH_DERIVE_VOLUMES (1u << 16)
/* KSH_ACTIVE_RESOURCES (opt-in; a library flag like KSH_DERIVE_VOLUMES: a bit no KS_FLAG_* uses, stripped before the flat problem is built, so it is never hashed by
 * ksh_fingerprint nor passed to ks_problem_upload): flatten over the resource names the problem REQUESTS, not over all a catalogue lists.  Interned are cpu, memory, pods
 * (ids 0, 1, 2 as always) and, in the same first-use order as without the flag, every name that is NAMED -- present, a quantity of 0 included -- in
 *   a container's or init container's requests or limits of a pending pod, a daemonset pod or a bound pod of a snapshot; a provisioner's limits; a state node's
 *   daemonset_requests.
 * A name that only an instance type's capacity / overhead or a state node's available / capacity carries is INERT: it decides nothing (resources.Fits walks the requested
 * names, scheduler.go:273-309 the limited ones, a result's Requests hold requested names), so it gets no id and its quantities are not stored.  ksh_dims' R,
 * ksh_name(h, 2, r, 0), ksh_result_arrays' n_resources and KSR1 text then speak of the active names only, and the 16-name limit counts active names (a 20-name catalogue
 * whose pods request six opens; 17 active names are refused with both counts in the message).  The flat problem is byte for byte the one the same objects give without
 * the flag once the inert names are deleted from them, so every result is the same; with at most 8 (4) active names the narrow (LEAN, ks_pack_rr) kernels take a problem
 * the wide single-wave variants would otherwise run, and the LEAN variants take it at up to 8 names (ks_problem.lean_r8).
 * Accepted by every call that takes `flags` and flattens: ksh_open*, ksh_solve_from_pods / _batch, ksh_open_batch, ksh_open_whatifs*, ksh_open_whatifs_derived (with or
 * without KSH_DERIVE_VOLUMES; a snapshot's active set is the union over ALL its bound pods, so it does not depend on a candidate set), ksh_snapshot_fingerprint,
 * ksh_check_whatif_derivation.  A parsed object keeps the flag-on flattenings (environment cache, snapshot) apart from the flag-off ones; after ksh_env_apply / _block an
 * event that makes a new name active falls back to the full flattening, as a new label value does.  Without the flag nothing changes. */
#define KSH_ACTIVE_RESOURCES (1u << 17)
/* KSH_DERIVE_GROUP_LISTS (opt-in; a library flag like KSH_DERIVE_VOLUMES: a bit no KS_FLAG_* uses, stripped before the flat problem is built): what a derived what-if's
 * topology takes from its candidate set is held as LISTS PER NODE -- one entry (group, count, domain or stay count, owner bit) per (node, group) pair where a pod on
 * the node is counted by the group or owns it (ksolve.h ks_whatif_topo_lists) -- instead of two dense [groups][nodes] tables, and ANY number of topology groups is
 * accepted: the 1024 above are the dense kernel's shape (one thread per group in one block), not a property of the problem.  The host evaluates the node filter and
 * the key-present test for such pairs only; an open copies the lists (entries, not groups x nodes) into its arena; ks_derive_topology_lists walks a candidate node's
 * entries.  Every other refusal above stays, and the what-ifs are the dense route's cell by cell (the debug call below reads them).  The flag-on flattening of the
 * snapshot is kept apart from the flag-off one, so ksh_snapshot_fingerprint with flags 0 does not move; after ksh_env_apply / _block the lists are rebuilt where the tables are.
 * Accepted by ksh_open_whatifs_derived, ksh_consolidation_commands / ksh_first_n_node_option / ksh_single_node_option, ksh_replacement_commands / _option,
 * ksh_validate_commands, ksh_single_node_resume, ksh_check_whatif_derivation (which then restates the derivation from the lists) and ksh_snapshot_fingerprint; combines
 * with KSH_DERIVE_VOLUMES and KSH_ACTIVE_RESOURCES.  Where a command call falls back to flattening the what-ifs one by one the flag is dropped.  Without the flag nothing
 * changes, the refusal above 1024 groups included. */
#define KSH_DERIVE_GROUP_LISTS (1u << 18)
int ksh_open_whatifs_derived(void* parsed_snapshot, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand, const int32_t* pod_node, int device, void** out_handles);
/* Diagnostic: ks_debug_whatif_topology of ksolve.h for the handle of a derived what-if -- the group activity [G], domain counts [G][64] and positive-hostname
 * extras [GH] its derivation left (ksh_dims names G and GH; any destination may be NULL).  Read-only, launches nothing; KS_ERR_INVALID for any other handle. */
int ksh_debug_whatif_topology(void* handle, uint8_t* out_active, int32_t* out_count, int32_t* out_extra);
uint64_t ksh_whatifs_upload_bytes(void* handle);     /* a derived what-if: the bytes its batch's open copied to the device (ks_whatifs_upload_bytes); 0 for any other handle */
uint64_t ksh_whatifs_arena_bytes(void* handle);      /* a derived what-if: device bytes of the arena its batch shares (ks_whatifs_arena_bytes); 0 for any other handle */
int ksh_open_whatifs_parsed(void* parsed_snapshot, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand, const int32_t* pod_node, uint32_t nthreads, void** out_handles);
/* Diagnostic (no GPU needed, not on any solving path): what the device would derive for ONE candidate set -- group activity, domain counts, hostname rows --
 * restated in plain loops over the per-node tables (under KSH_DERIVE_GROUP_LISTS: over the per-node lists) and compared with that what-if flattened by itself.  KS_OK, or KS_ERR_INVALID with the first difference
 * in ksh_last_error(); KS_ERR_UNSUPPORTED for a snapshot ksh_open_whatifs_derived refuses.  With KSH_DERIVE_VOLUMES it also restates, for every node that
 * stays, the volume counts and limits per driver and the multi claims it lists, and for every pod of the batch on every such node whether the volume test
 * admits it and what it adds per driver -- against the what-if's own (candidate-dependent) partition. */
int ksh_check_whatif_derivation(void* parsed_snapshot, uint32_t flags, const uint32_t* cand, uint32_t ncand, const int32_t* pod_node);

/* ---- consolidation COMMANDS, decided on the device (deprovisioning/consolidation.go:190-274 computeConsolidation, multinodeconsolidation.go:74-165
 * firstNNodeConsolidationOption + filterOutSameType, singlenodeconsolidation.go:54-78 the scan of SingleNodeConsolidation.ComputeCommand): snapshot and candidate
 * sets in, one fixed-size row per candidate set out (layout: ksolve.h KS_CMD_*, KS_CMD_ROW_WORDS(words) uint64 each, words >= ceil(T/64)).
 * ksh_consolidation_commands opens the what-ifs derived on the device (flags: KS_FLAG_SIMULATION / _NO_RR / _ONE_WAVE / _NO_LEAN, KSH_DERIVE_VOLUMES,
 * KSH_ACTIVE_RESOURCES, KSH_DERIVE_GROUP_LISTS; any other bit is KS_ERR_INVALID) -- flattened one by one and uploaded where ksh_open_whatifs_derived answers KS_ERR_UNSUPPORTED --, solves
 * them resident in one launch, decides all of them in one more (ks_consolidation_commands_dev), reads the rows back and closes the handles.  Nothing but the rows
 * crosses back: no result is decoded on the host.  What the decision reads beside the simulation comes from the parsed nodes' labels:
 *   node.kubernetes.io/instance-type, topology.kubernetes.io/zone, karpenter.sh/capacity-type of every candidate: getNodePrices (the sum, in candidate order, of
 *     Offerings.Get -- the parsed offerings, available or not: types.go:117-124 does not consult availability), "all candidates are spot", and per distinct
 *     candidate type the lowest such price (0.0 if none of its candidates has an offering: Go's map miss) for filterOutSameType;
 *   karpenter.sh/initialized, karpenter.sh/provisioner-name and in_state of every node that STAYS: one owned, in-state node that is not initialised makes the
 *     simulation count as "not all pods scheduled" (helpers.go:102-113).
 * deleting[n_deleting]: nodes that leave EVERY what-if with their pods joining its batch.  Owned ones are the nodes marked for deletion (helpers.go:48-61,81-84):
 *   they leave last, and a candidate set that names one gets an error row (KS_CMD_ERROR, KS_CMD_WHY_DELETING: helpers.go:62-67) and is not simulated.  Pending pods
 *   stay the caller's business, as with ksh_open_whatifs*: bind them to ONE extra node of the snapshot that no provisioner owns (no labels, no cluster-pod records)
 *   and list that node here; an unowned node of `deleting` leaves first (the pending pods head the batch, helpers.go:76-79).
 * same_type != 0: also filterOutSameType on every replace (KS_CMD_F_SAME_TYPE; the row then carries both stages).  ms[5] (may be NULL): [0] open, [1] solve,
 * [2] command kernel (inputs up, launch, completion), [3] read-back of the rows, [4] the host work around them (the per-what-if inputs, closing the handles),
 * milliseconds: the five sum to the call.  Row i answers candidate set i; row[KS_CMD_ID] = i.
 * What the decision reads of the nodes' labels is tabulated by the first command call over a snapshot and kept with it until ksh_env_apply* changes the nodes.
 * Whole-call refusals, nothing opened: KS_ERR_INVALID for an unknown flag bit, words < ceil(T/64), offsets that do not ascend, a node index out of range, and for a
 * candidate (other than the unowned carrier of pending pods, which belongs in `deleting`) whose instance-type label names no type of the catalogue -- candidateNodes
 * never yields such a node (helpers.go:165-230), so it is a caller's mistake, not a per-set error row like a deleting candidate.  KS_ERR_UNSUPPORTED, after the
 * what-ifs were flattened but before anything is uploaded or launched: on the fallback route a what-if that needs instance-type requirement states of its own (a
 * row's KS_CMD_IT_STATE is read through the snapshot's lattice); such a batch goes through ksh_open_whatifs_parsed / ksh_result_text. */
int ksh_consolidation_commands(void* parsed_snapshot, uint32_t flags, uint32_t n, const uint32_t* cand_off /* [n+1] */, const uint32_t* cand, const int32_t* pod_node /* or NULL after ksh_env_apply */,
                               const uint32_t* deleting, uint32_t n_deleting, int device, int same_type, uint64_t* out_rows /* [n][KS_CMD_ROW_WORDS(words)] */, uint32_t words, double* ms /* [5] or NULL */);
/* firstNNodeConsolidationOption: every prefix candidates[0 .. mid] the binary search could probe (mid = 1 .. min(max_nodes, n - 1)) in ONE batch with same_type = 1,
 * then the search of multinodeconsolidation.go:86-114 replayed over the rows: out_row is the row of the longest prefix the search settled on (action delete or
 * replace; the launch options are the row's SECOND stage), all zero (do-nothing) if there is none, or the error row of a prefix the search probed (:92-95).
 * out_row[KS_CMD_ID] = the number of leading candidates the command removes. */
int ksh_first_n_node_option(void* parsed_snapshot, uint32_t flags, const uint32_t* candidates, uint32_t n, uint32_t max_nodes /* the reference passes 100 */, const int32_t* pod_node,
                            const uint32_t* deleting, uint32_t n_deleting, int device, uint64_t* out_row /* [KS_CMD_ROW_WORDS(words)] */, uint32_t words, double* ms /* [5] or NULL */);
/* The scan of SingleNodeConsolidation.ComputeCommand: every singleton in ONE batch; out_row is the first delete or replace in candidate order -- error rows are
 * passed over, as the reference logs and continues --, all zero (do-nothing) if there is none.  out_row[KS_CMD_ID] = the position of that candidate. */
int ksh_single_node_option(void* parsed_snapshot, uint32_t flags, const uint32_t* candidates, uint32_t n, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                           int device, uint64_t* out_row, uint32_t words, double* ms);
/* The rows of handles whose results are on the device (ksh_solve_batch_resident / ksh_solve / ...; derived or not), for a caller that keeps its what-ifs open or
 * shards them itself: ks_consolidation_commands_host (ksolve.h) over handles, the per-what-if inputs built by the caller. */
int ksh_command_rows(void** handles, uint32_t n, const uint64_t* ids, const ks_command_inputs* in, uint32_t words, uint64_t* out_rows, double* ms /* [2] or NULL */);
/* Turning a row into strings without a handle: what 0 = requirement key a (KS_CMD_MASK + a), 2 = resource a (KS_REP_NODE_REQ + a), 1 = value b of key a (bit b of that mask; a key encoded over value
 * classes names one member per class, as ksh_name does), 3 = state node a (a candidate index), 4 = instance type a (bit a of the option masks), 5 / 6 = value a of the
 * zone / capacity-type universe (the ids ksh_provision's launch pick gives).  Keys and values
 * are the snapshot's flattening's: available once a what-if call flattened it.  NULL when out of range; the strings live as long as the snapshot is neither
 * changed (ksh_env_apply*) nor freed.  A requirement reads: present bit k of row[KS_CMD_PRESENT], complement bit k of its high half, values = the mask's bits,
 * greaterThan / lessThan = the low / high half of row[KS_CMD_BOUNDS + k] unless KS_NO_BOUND_GT / KS_NO_BOUND_LT.  row[KS_CMD_IT_STATE] != 0: the node also carries
 * a requirement on node.kubernetes.io/instance-type, spelled out by ksh_snapshot_it_state (complement, number of values) / ksh_snapshot_it_state_value. */
const char* ksh_snapshot_name(void* parsed_snapshot, int what, uint32_t a, uint32_t b);
int ksh_snapshot_it_state(void* parsed_snapshot, uint32_t state, int* complement, uint32_t* n_values);
const char* ksh_snapshot_it_state_value(void* parsed_snapshot, uint32_t state, uint32_t i);

/* ---- consolidation commands VALIDATED, on the device: the last step of a pass -- snapshot -> candidates -> commands -> (events, consolidationTTL) -> validated
 * commands.  Validation.IsValid after its wait (deprovisioning/validation.go:63-100) and ValidateCommand (:109-172) with mapNodes (helpers.go:328-337), a second
 * simulateScheduling and instanceTypesAreSubset (helpers.go:118-122), for n commands against the snapshot as it is NOW (kept current by ksh_env_apply*; the wait
 * itself stays with the caller).  One fixed-size row per command (layout: ksolve.h KS_VAL_*, KS_VAL_ROW_WORDS(words) uint64 each); row i answers command i,
 * row[KS_VAL_ID] = i.
 *   node_off / nodes   each command's nodesToRemove as node slots of THIS snapshot (slots are stable across events; an empty list is allowed)
 *   expect_replacement len(cmd.replacementNodes) != 0;  options[i]: that node's InstanceTypeOptions -- of a command row, its launch options -- as a bit mask whose
 *                      bits are indices into the catalogue of the snapshot PASSED (the same catalogue unless the snapshot was ingested again); read only where a
 *                      replacement is expected; may be NULL if none is
 *   why / node_flags   [node slots] ksh_consolidation_candidates' out->why over THIS snapshot, and the node flags it was given (KSH_CAND_NODE_NOMINATED is read)
 *   pod_node, deleting, flags: as for ksh_consolidation_commands.
 * Host steps, the reference's order, first wins: (1) a node of the command is nominated -- over ALL its nodes, before the mapping (validation.go:87-91) -> invalid;
 * (2) mapping: a node maps iff why[node] is 0, 10, 11 or 12, i.e. it is in candidateNodes' result under Validation.ShouldDeprovision == consolidation.ShouldDeprovision
 * (sortAndFilterCandidates is NOT applied in validation); a tombstoned slot (13) and an empty list do not map; nothing maps -> invalid (:114); (3) a mapped node is
 * listed in `deleting` -> verdict KS_VAL_ERROR, the error of helpers.go:62-67 (reachable when `deleting` is newer than `why`: the reference's own race).  Rows 1-3 are
 * written by the library and not simulated.  Every other command's MAPPED nodes -- in ascending slot order, each once: mapNodes walks the candidates, and slot order is
 * the canonical order of DESIGN 7.16; NewQueue's order is total, so the order decides nothing -- leave the cluster in ONE batch of what-ifs on the route of
 * ksh_consolidation_commands (derived on the device, else flattened one by one; the carrier of pending pods first, owned deleting nodes last; KS_VAL_F_BLOCKED from the
 * same label table as KS_CMD_F_BLOCKED), and kernel ks_validate_commands writes steps 4-8 or valid.  Validation reads no requirement state, so the fallback route's
 * instance-type-state refusal does not apply here.
 * Whole-call refusals (nothing simulated, out_rows untouched): KS_ERR_INVALID for an unknown flag bit, words < ceil(T/64), offsets not ascending, a slot out of
 * range, a listed type index >= T, NULL arrays.  ms[5] as ksh_consolidation_commands ([2] = the validation kernel).  No CPU path: without a device KS_ERR_DEVICE. */
int ksh_validate_commands(void* parsed_snapshot_now, uint32_t flags, uint32_t n, const uint32_t* node_off /* [n+1] */, const uint32_t* nodes, const uint32_t* expect_replacement /* [n] */,
                          const uint64_t* options /* [n][words] */, const uint32_t* why /* [node slots] */, const uint32_t* node_flags /* [node slots] */,
                          const int32_t* pod_node /* or NULL after ksh_env_apply */, const uint32_t* deleting, uint32_t n_deleting, int device,
                          uint64_t* out_rows /* [n][KS_VAL_ROW_WORDS(words)] */, uint32_t words, double* ms /* [5] or NULL */);
/* SingleNodeConsolidation.ComputeCommand's loop (singlenodeconsolidation.go:54-84) AFTER a first validation has failed: candidates[0 .. n) are the candidates that
 * follow the one whose command failed, as slots of the CURRENT snapshot.  Their singleton commands are computed in one command batch, the deletes and replaces among
 * them validated in one validation batch, and the first VALID one in candidate order is returned: out_state = 1, out_row its command row (row[KS_CMD_ID] = its
 * position in `candidates`), out_vrow its validation row.  Error rows and validation errors are passed over, as the reference logs and continues.  If none is valid
 * both rows are zero and out_state = 2 (actionRetry) when failed_before != 0 or any validation here said invalid, else 0 (do-nothing).  A candidate whose slot has left
 * is an empty node to the command step and fails validation (nothing maps).  ms[5]: the sums over both batches. */
int ksh_single_node_resume(void* parsed_snapshot_now, uint32_t flags, const uint32_t* candidates, uint32_t n, int failed_before, const uint32_t* why, const uint32_t* node_flags,
                           const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, int device, uint64_t* out_row /* [KS_CMD_ROW_WORDS(words)] */,
                           uint64_t* out_vrow /* [KS_VAL_ROW_WORDS(words)] */, uint32_t* out_state, uint32_t words, double* ms /* [5] or NULL */);
/* EmptyNodeConsolidation's own, cheaper check (emptynodeconsolidation.go:77-87), literally; host only, no simulation.  nodes[0 .. n): the command's nodes as slots;
 * why / n_node_pods: ksh_consolidation_candidates' outputs over the snapshot NOW; node_flags as above ([node slots] each; every slot listed must be in range).  The
 * nodes are mapped as above; *out_retry = 1 iff a mapped node has pods and is not nominated.  A command none of whose nodes maps comes back with *out_retry = 0 -- the
 * reference returns such a command as it is, and so does this. */
int ksh_validate_empty_nodes(const uint32_t* nodes, uint32_t n, const uint32_t* why, const uint32_t* n_node_pods, const uint32_t* node_flags, uint32_t* out_retry);

/* ---- consolidation CANDIDATES, selected and ordered on the device: the first step of a consolidation pass, so that snapshot -> candidates -> commands runs through
 * this header alone.  candidateNodes (deprovisioning/helpers.go:171-249) with consolidation.ShouldDeprovision (consolidation.go:106-121) as its filter, then
 * sortAndFilterCandidates (consolidation.go:83-104): canBeTerminated with PDBLimits.CanEvictPods and PodsPreventEviction (helpers.go:339-366, pdblimits.go:55-70),
 * disruptionCost x calculateLifetimeRemaining (helpers.go:124-165,275-287), and the sort.  out->order is what ksh_first_n_node_option / ksh_single_node_option take as
 * `candidates`; out->empty is EmptyNodeConsolidation's nodesToRemove (emptynodeconsolidation.go:54).
 *
 * The snapshot's nodes and bound pods are the slots ksh_snapshot_bindings reports; its bound pods are GetNodePods' output (utils/node/node.go:30-49: daemonset-owned,
 * node-owned, terminal and terminating pods are not in it), so the skips of PodsPreventEviction are vacuous and "no pods" is "no bound pod".  `pod_node`: as for the
 * command calls (NULL after ksh_env_apply*).  `deleting`: the nodes that are MarkedForDeletion.
 * ksh_candidate_inputs: what the snapshot's objects do not carry.  n_nodes / n_pods / n_provisioners must equal the snapshot's slot counts and its provisioner count
 * (the provisioners in the snapshot's order).  age_seconds is what clock.Since(CreationTimestamp).Seconds() gave; deletion_cost is the parsed
 * controller.kubernetes.io/pod-deletion-cost annotation (parsing it, and dropping one that does not parse, stays with the caller); ttl_seconds_until_expired is -1 for nil.
 * KS_ERR_INVALID: a deletion cost that is not finite, an age that is not finite, a ttl of 0 -- the reference divides by zero there -- or below -1, a wrong array
 * length, an unknown flag bit (KSH_CAND_NODE_DO_NOT_CONSOLIDATE_TRUE without KSH_CAND_NODE_DO_NOT_CONSOLIDATE included), a deleting node out of range.
 * ksh_pdb_block: the PodDisruptionBudgets as one stream of u32 words over one string table (conventions of ksh_delta_block; grammar in
 * karpenter_core_amd/host/kspb.hpp, PdbReader): per PDB namespace:S disruptions_allowed:I selector.  The block is decoded completely before anything else happens: a
 * malformed one -- or a selector metav1.LabelSelectorAsSelector refuses -- is KS_ERR_INVALID with the PDB's index in ksh_last_error().  NULL means no PDBs.
 * Selectors are flattened for the device: the label keys some selector mentions, at most KS_CAND_MAX_KEYS, and per key the values some selector
 * mentions, at most KS_CAND_MAX_VALUES; beyond either, KS_ERR_UNSUPPORTED with both counts in the message and nothing written -- ksh_consolidation_candidates_ex with
 * KSH_CAND_WIDE_SELECTORS has neither limit.
 *
 * out->why[node] (0 = candidate; the first reason in the reference's own order wins), out->detail[node] (-1 unless stated):
 *    1  listed in `deleting` (helpers.go:186)                2  no provisioner-name label, or it names no provisioner of the snapshot (:190)
 *    3  the instance-type label names no type of that provisioner (:194-198)          4  no capacity-type label (:201)          5  no zone label (:205)
 *    6  not initialised (:211)          7  nominated (:215)          8  the do-not-consolidate annotation is "true" (consolidation.go:108-111: literally
 *       `return val != "true"` -- an annotation with any other value makes the node pass WITHOUT the provisioner checks)
 *    9  the provisioner has consolidation disabled (:116-119)          10  deletion timestamp set (helpers.go:340)
 *   11  a PDB prevents evictions; detail = the PDB's index (first pod in slot order, first PDB in order; a PDB with disruptions allowed never blocks)
 *   12  a pod has do-not-evict; detail = the pod slot          13  the slot's node left (NODE-, or a node that is not in state)
 * 1-9: not in candidateNodes' result; 10-12: in it, filtered by sortAndFilterCandidates.  out->cost[node] is the final disruption cost: the pods' eviction costs
 * summed sequentially in ascending slot order -- float64 addition is order-dependent and Go walks GetNodePods' list; the slot order is the canonical execution --
 * times the lifetime remaining.  It is written for 0 and 10-12 and is 0.0 for 1-9 and 13.  out->n_node_pods[node]: the bound pods of the slot.
 * out->order[0 .. n_candidates): the candidates by `cost <`, the reference's comparator (-0.0 and +0.0 tie); ties by ascending node slot -- Go's sort.Slice is
 * unstable and ForEachNode walks a map, the canonical execution is the stable sort over ascending slot.  out->empty[0 .. n_empty): the candidates without pods, in the
 * same order.  The arrays are the caller's, [node slots] each.
 * ms[4] (may be NULL): host tabulation | upload | kernels | read-back, milliseconds.  Reasons 2-6 are tabulated from the nodes' labels by the first call over a
 * snapshot and kept with it, next to the command calls' label table, until ksh_env_apply* changes the nodes.  There is no host path: without a device, KS_ERR_DEVICE. */
#define KSH_CAND_NODE_NOMINATED 1u
#define KSH_CAND_NODE_DO_NOT_CONSOLIDATE 2u         /* the karpenter.sh/do-not-consolidate annotation is present */
#define KSH_CAND_NODE_DO_NOT_CONSOLIDATE_TRUE 4u    /* ... and its value is "true" */
#define KSH_CAND_NODE_DELETION_TIMESTAMP 8u
#define KSH_CAND_POD_DO_NOT_EVICT KS_CAND_POD_DO_NOT_EVICT
#define KSH_CAND_POD_HAS_DELETION_COST KS_CAND_POD_HAS_DELETION_COST
#define KSH_CAND_POD_HAS_PRIORITY KS_CAND_POD_HAS_PRIORITY
typedef struct ksh_candidate_inputs {
  uint32_t n_nodes, n_pods, n_provisioners, pad;
  const uint32_t* node_flags;                 /* [n_nodes] KSH_CAND_NODE_* */
  const double* node_age_seconds;             /* [n_nodes] */
  const uint32_t* pod_flags;                  /* [n_pods] KSH_CAND_POD_* */
  const double* pod_deletion_cost;            /* [n_pods] read under KSH_CAND_POD_HAS_DELETION_COST */
  const int32_t* pod_priority;                /* [n_pods] read under KSH_CAND_POD_HAS_PRIORITY */
  const uint32_t* prov_consolidation_enabled; /* [n_provisioners] Spec.Consolidation != nil && *Enabled */
  const int64_t* prov_ttl_seconds_until_expired; /* [n_provisioners] -1: nil */
} ksh_candidate_inputs;
typedef struct ksh_pdb_block {
  uint32_t n_pdbs, n_strings, n_words;
  const uint32_t* str_off;      /* [n_strings + 1] byte offsets into str_bytes */
  const char* str_bytes;
  const uint32_t* words;        /* [n_words] */
  uint64_t str_bytes_len;       /* bytes behind str_bytes: str_off[n_strings] must not reach beyond */
} ksh_pdb_block;
typedef struct ksh_candidates_out {
  uint32_t n_candidates, n_empty;
  uint32_t* order; uint32_t* empty; uint32_t* why; int32_t* detail; uint32_t* n_node_pods; double* cost;      /* [node slots] each, the caller's */
} ksh_candidates_out;
int ksh_consolidation_candidates(void* parsed_snapshot, const int32_t* pod_node /* or NULL after ksh_env_apply* */, const uint32_t* deleting, uint32_t n_deleting,
                                 const ksh_candidate_inputs* in, const ksh_pdb_block* pdbs /* or NULL */, int device, ksh_candidates_out* out, double* ms /* [4] or NULL */);
/* The same call with `flags`; ksh_consolidation_candidates is this with flags 0, and with flags 0 the route, the results, the refusals and ms[4] are that call's.
 * KSH_CAND_WIDE_SELECTORS (opt-in, the only bit; any other is KS_ERR_INVALID): the selectors are flattened as LISTS (ksolve.h ks_selector_lists) -- per
 * bound pod the selector-mentioned keys it carries with a value id each, per requirement an operator and a sorted list of value ids -- and decided by kernel
 * ks_cand_pods_lists, so that label keys, values per key and values per set are unbounded: neither KS_CAND_MAX_KEYS nor KS_CAND_MAX_VALUES applies and no selector
 * size is KS_ERR_UNSUPPORTED (only a snapshot whose bound pods carry 2^32 selector-mentioned labels, or PDBs with 2^32 values in all, is -- both counts in the message).
 * The usual cluster, one PDB per application with `matchLabels: {app: <name>}`, needs this from its 63rd application on.  With the flag the wide route is always taken,
 * also for selectors the narrow form could hold; every output is bit for bit the narrow route's where both answer.  The tabulation walks each bound pod's labels once
 * (key, then value: two hash look-ups per label), not keys x pods.  Everything that is not a selector -- reasons 1-10 and 13, the provisioners' ttls, the per-node pod
 * lists, the cached label table, the behaviour after ksh_env_apply* -- is the same code as without the flag.  ms[4] as above; with the flag ms[1] also holds the
 * library's regrouping of PDBs and pods by namespace. */
#define KSH_CAND_WIDE_SELECTORS 1u
int ksh_consolidation_candidates_ex(void* parsed_snapshot, const int32_t* pod_node /* or NULL after ksh_env_apply* */, const uint32_t* deleting, uint32_t n_deleting,
                                    const ksh_candidate_inputs* in, const ksh_pdb_block* pdbs /* or NULL */, int device, uint32_t flags, ksh_candidates_out* out, double* ms /* [4] or NULL */);

/* ---- candidates of the methods the deprovisioning controller tries BEFORE consolidation (deprovisioning/controller.go:142-162): expiration, drift, emptiness.
 * ksh_consolidation_candidates' sibling: the snapshot, `pod_node`, `deleting`, the PDB block, the output arrays, ms[4] and reasons 1-7 and 10-13 mean what they mean
 * there; `method`'s ShouldDeprovision takes the place of 8 and 9, which never occur here (base.prov_consolidation_enabled is not read and may be NULL; the
 * do-not-consolidate flags are accepted and ignored).  1-7 come before the method's code, in the reference's order (helpers.go:171-249); 10-12 after it.
 *   14  expiration: the provisioner has no TTLSecondsUntilExpired (detail 0), or `now` is not after creation + ttl (detail 1)          expiration.go:56-58,120-127
 *   15  drift: drift_enabled == 0 (detail 0), or the node lacks KSH_CAND_NODE_DRIFTED -- the karpenter.sh/voluntary-disruption annotation is absent or not
 *       "drifted" (detail 1)                                                                                                             drift.go:50-56
 *   16  emptiness: no TTLSecondsAfterEmpty (detail 0), the node has bound pods (1), no emptiness timestamp annotation (2), the ttl is not reached (3).  An annotation
 *       that does not parse (KSH_CAND_NODE_EMPTINESS_UNPARSABLE) makes the node a candidate, as in the reference.  Daemonset pods are not bound pods of the snapshot
 *       (see ksh_consolidation_candidates), so a node that runs only those is empty.                                                    emptiness.go:52-70
 * Time is exact integer arithmetic, never age_seconds: a node is expired iff now_unix_nanos > node_creation_unix_nanos + ttl * 10^9 in int64 (time.Time.After is
 * strict: at the expiration time itself the node is not expired), empty long enough iff now > node_emptiness_unix_nanos + ttl * 10^9.  KS_ERR_INVALID for a ttl above
 * 9 223 372 036 s -- where Go's Duration(ttl) * time.Second wraps -- and for a sum the method needs that would overflow; plus every refusal of
 * ksh_consolidation_candidates, an unknown method, a ttlSecondsAfterEmpty below -1, UNPARSABLE without HAS_EMPTINESS_TIMESTAMP.  base.node_age_seconds is still read,
 * for disruptionCost's lifetime factor only; out->base.cost is written as there for 0 and 10-12.
 * The order.  Expiration: the nodes with code 0 by expiration time ascending, ties by ascending slot (SortCandidates, expiration.go:61-66, executed stably over slot
 * order: DESIGN.md 7.16).  Drift: the nodes with code 0 by ascending slot (candidateNodes walks a map; slot order is the canonical one).  Nodes with 10-12 are in
 * candidateNodes' result but ComputeCommand's canBeTerminated test passes them over, so they are not in `order`; out->n_in_result counts codes 0 and 10-12 -- the
 * controller moves to the next method when it is 0 (controller.go:167-170).  Emptiness: Emptiness.ComputeCommand never calls canBeTerminated, so 10 is not assigned
 * and 11 / 12 cannot occur (no pods); `order` and `empty` both list the code-0 nodes by ascending slot, which is the whole DELETE command (ksh_emptiness_command).
 * Under expiration and drift `empty` lists the nodes of `order` without pods.  No host path: without a device, KS_ERR_DEVICE. */
#define KSH_METHOD_EXPIRATION KS_METHOD_EXPIRATION
#define KSH_METHOD_DRIFT KS_METHOD_DRIFT
#define KSH_METHOD_EMPTINESS KS_METHOD_EMPTINESS
#define KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP 16u   /* the karpenter.sh/emptiness-timestamp annotation is present */
#define KSH_CAND_NODE_EMPTINESS_UNPARSABLE 32u      /* ... and time.Parse(time.RFC3339, ...) refuses it */
#define KSH_CAND_NODE_DRIFTED 64u                   /* karpenter.sh/voluntary-disruption == "drifted" */
typedef struct ksh_deprovisioning_inputs {
  ksh_candidate_inputs base;                      /* node_flags may carry the three bits above */
  int64_t now_unix_nanos;                         /* clock.Now() */
  const int64_t* node_creation_unix_nanos;        /* [n_nodes] CreationTimestamp */
  const int64_t* node_emptiness_unix_nanos;       /* [n_nodes] the parsed annotation; read under HAS_EMPTINESS_TIMESTAMP without UNPARSABLE */
  const int64_t* prov_ttl_seconds_after_empty;    /* [n_provisioners] -1: nil */
  uint32_t drift_enabled, pad;                    /* settings.DriftEnabled */
} ksh_deprovisioning_inputs;
typedef struct ksh_deprovisioning_out { ksh_candidates_out base; uint32_t n_in_result, pad; } ksh_deprovisioning_out;
int ksh_deprovisioning_candidates(void* parsed_snapshot, uint32_t method, const int32_t* pod_node /* or NULL after ksh_env_apply* */, const uint32_t* deleting, uint32_t n_deleting,
                                  const ksh_deprovisioning_inputs* in, const ksh_pdb_block* pdbs /* or NULL */, int device, ksh_deprovisioning_out* out, double* ms /* [4] or NULL */);
/* The same call with `flags` (KSH_CAND_WIDE_SELECTORS, as for ksh_consolidation_candidates_ex); ksh_deprovisioning_candidates is this with flags 0. */
int ksh_deprovisioning_candidates_ex(void* parsed_snapshot, uint32_t method, const int32_t* pod_node /* or NULL after ksh_env_apply* */, const uint32_t* deleting, uint32_t n_deleting,
                                     const ksh_deprovisioning_inputs* in, const ksh_pdb_block* pdbs /* or NULL */, int device, uint32_t flags, ksh_deprovisioning_out* out, double* ms /* [4] or NULL */);
/* Emptiness.ComputeCommand (emptiness.go:73-82), literally; host only, no simulation.  candidates[0 .. n): ksh_deprovisioning_candidates' out->base.order under
 * KSH_METHOD_EMPTINESS; n_node_pods: its out->base.n_node_pods ([node slots]).  out_nodes[0 .. *out_n_nodes) (room for n): the candidates without pods, in order --
 * the command's nodesToRemove; *out_action = KS_CMD_DELETE, or KS_CMD_DO_NOTHING when there is none. */
int ksh_emptiness_command(const uint32_t* candidates, uint32_t n, const uint32_t* n_node_pods, uint32_t* out_action, uint32_t* out_nodes, uint32_t* out_n_nodes);

/* ---- replacement commands with m -> n rows (deprovisioning/expiration.go:75-111, drift.go:64-96): Expiration / Drift.ComputeCommand's simulation and command for n
 * candidate sets over ONE snapshot.  `flags`, `pod_node`, `deleting`, the route (what-ifs derived on the device, else flattened one by one, solved resident in one
 * launch) and ms[5] are as for ksh_consolidation_commands ([2] = the two replacement kernels).  Two caller-owned tables come back (layout: ksolve.h KS_REP_*):
 * out_heads[n][KS_REP_HEAD_WORDS] -- head i answers candidate set i, head[KS_REP_ID] = i -- and out_nodes[cap_nodes][KS_REP_NODE_WORDS(words)], one fixed-size row per
 * replacement node in what-if order and then new-node order, found through the head's KS_REP_NODE_OFF.  A node row's requirement words decode as a command row's
 * (ksh_snapshot_name what 0 / 1, ksh_snapshot_it_state*); its KS_REP_NODE_REQ words are the node's resource requests, resource r named by ksh_snapshot_name(what = 2)
 * -- under KSH_ACTIVE_RESOURCES the active names.  The decision, in the reference's order: (1) a candidate listed in `deleting` -> an error head (KS_CMD_ERROR,
 * KS_CMD_WHY_DELETING), written here, not simulated; (2) blocked (KS_CMD_F_BLOCKED's rule: helpers.go:106-113 returns `nil, false, nil`) -> delete, n_nodes 0,
 * KS_REP_BLOCKED; (3) n_new == 0 -> delete; (4) replace with all n_new nodes.  n_unscheduled > 0 is reported and changes nothing (the reference logs it).  No price
 * stage and no narrowing: the reference applies neither here.
 * Capacity: *out_total_nodes = the sum of n_nodes; beyond cap_nodes the call still returns KS_OK with every head complete, rows written for the sets that fit entirely,
 * KS_REP_TRUNCATED on the others and nothing at or beyond cap_nodes touched -- call again with a larger table.  cap_nodes = 0 with out_nodes = NULL is the sizing call.
 * Whole-call refusals as ksh_consolidation_commands (without the instance-type one: nothing here is priced). */
int ksh_replacement_commands(void* parsed_snapshot, uint32_t flags, uint32_t n, const uint32_t* cand_off /* [n+1] */, const uint32_t* cand, const int32_t* pod_node /* or NULL after ksh_env_apply */,
                             const uint32_t* deleting, uint32_t n_deleting, int device, uint64_t* out_heads, uint64_t* out_nodes /* or NULL */, uint64_t cap_nodes, uint64_t* out_total_nodes,
                             uint32_t words, double* ms /* [5] or NULL */);
/* ComputeCommand's loop for expiration and drift.  candidates[0 .. n): ksh_deprovisioning_candidates' out->base.order (or any list of node slots); why: its out->base.why
 * ([node slots]).  The first candidate with why == 0 that is not in `deleting` decides (`continue` for both, drift.go:67-77); that ONE set is simulated and its head, its
 * node rows (from row 0) and *out_position (its index in `candidates`; out_head[KS_REP_ID] too) come back.  None: the head is all zero (do-nothing), *out_position = -1,
 * nothing is simulated.  Capacity as above. */
int ksh_replacement_option(void* parsed_snapshot, uint32_t flags, const uint32_t* candidates, uint32_t n, const uint32_t* why, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                           int device, uint64_t* out_head /* [KS_REP_HEAD_WORDS] */, uint64_t* out_nodes, uint64_t cap_nodes, uint64_t* out_total_nodes, int32_t* out_position, uint32_t words,
                           double* ms /* [5] or NULL */);
/* Diagnostic: how many what-ifs the calls that simulate for the caller -- ksh_consolidation_commands and the searches on it, ksh_validate_commands / ksh_single_node_resume,
 * ksh_replacement_commands / ksh_replacement_option -- have opened AND solved in this process so far (all threads).  The difference across one call is the number of
 * simulations it made: ksh_replacement_option adds 1, or 0 when no candidate is eligible; a batch of n live sets adds n. */
uint64_t ksh_whatifs_simulated(void);
/* The two tables of handles whose results are on the device, for a caller that keeps its what-ifs open or shards them itself: ks_replacement_commands_host (ksolve.h)
 * over handles, flags[i] = KS_REP_F_* built by the caller. */
int ksh_replacement_rows(void** handles, uint32_t n, const uint64_t* ids, const uint32_t* flags, uint32_t words, uint64_t* out_heads, uint64_t* out_nodes, uint64_t cap_nodes,
                         uint64_t* out_total_nodes, double* ms /* [2] or NULL */);

/* ---- provisioning over the snapshot kept by events (provisioning/provisioner.go:106-165 Provisioner.Reconcile): the OTHER reader of state.Cluster, through the same
 * snapshot as the deprovisioner's methods.  Reconcile's Solve (:117-150) takes the state nodes that are not marked for deletion; its pods are GetPendingPods plus the
 * pods of the nodes that are marked -- simulateScheduling (deprovisioning/helpers.go:48-93) with an empty candidate set.  ksh_provision builds that ONE what-if: the
 * nodes of `deleting` leave with their pods as the batch, under ksh_consolidation_commands' convention -- the carrier of the pending pods (ONE node of the snapshot
 * that no provisioner owns; pending pods are bound to it, BIND events keep it current) first, the nodes marked for deletion after it.  `flags`, `pod_node` and the
 * route are those of every simulating call: derived on the device (KSH_DERIVE_VOLUMES, KSH_ACTIVE_RESOURCES, KSH_DERIVE_GROUP_LISTS honoured), flattened by itself
 * where the derivation answers KS_ERR_UNSUPPORTED, solved resident either way; out->route says which.  The blocked rule (KS_CMD_F_BLOCKED) is NOT applied: Reconcile
 * has no check like helpers.go:102-113, and an uninitialised node that stays is an ordinary in-flight ExistingNode.  ksh_whatifs_simulated grows by 1, or by 0 when no
 * pod is pending and none sits on a deleting node: Reconcile returns before NewScheduler then (:145-147), and so does this -- route KSH_PROVISION_NOTHING, zero rows,
 * nothing flattened or launched.
 * What comes back (caller-owned tables, the KS_REP_* capacity convention: totals always, rows only when all fit, nothing at or beyond a capacity touched, KS_OK; a
 * capacity of 0 with a NULL table is the sizing call -- though total_rows never exceeds the pods bound to `deleting`, and total_machines never exceeds total_rows):
 *   head      ksolve.h KS_PLC_*: P, n_new, n_unscheduled, flags (KS_PLC_TRUNCATED: cap_rows was too small; KSH_PROVISION_MACHINES_TRUNCATED: cap_machines was)
 *   rows      [cap_rows][KS_PLC_ROW_WORDS], one per pod of the batch in queue order, named by the snapshot's own stable ids on BOTH routes: the pod's index (the
 *             order of `pod_node` / ksh_snapshot_bindings), and where it went -- -1, an existing node's SLOT (not its row in a flattening), or node slots + j for
 *             new node j; head[KS_PLC_N_EXISTING] is the number of node slots.  The relaxation stage is what a shim applies back to pod.Spec, ascending commit
 *             numbers within a node are Node.Pods (NominatePod, provisioner.go:352-357), the reason word feeds the failed-scheduling events (scheduler.go:135-172).
 *   machines  [cap_machines][KS_REP_NODE_WORDS(words)], new node j in row j: ksh_replacement_commands' node rows (requirements, InstanceTypeOptions, requests --
 *             what ToMachine needs), decoded the same way.
 *   pick_*    [cap_machines] each, or all NULL: ksh_launch_pick per machine -- type index, zone and capacity-type value ids (ksh_snapshot_name what 5 / 6 names
 *             them), price; written when the machine rows were.
 * ms[5] as ksh_consolidation_commands ([2] = the kernels behind the three tables, [3] their read-backs).  Refusals as there: KS_ERR_INVALID for an unknown flag bit,
 * words < ceil(T/64), a deleting node out of range, a NULL table with a capacity, pick arrays given in part.
 * Limits.  The derived what-if runs ks_pack's single-wave variant: a burst that opens thousands of machines is faster through ksh_solve_from_batch (ks_pack_rr),
 * which remains the door for such bursts (README has the measured crossover).  And the pending pods live in the snapshot's spare pod room: a full snapshot
 * refuses the BIND ("spare room ... used up"); ingest it again. */
#define KSH_PROVISION_NOTHING 0u
#define KSH_PROVISION_DERIVED 1u
#define KSH_PROVISION_FLATTENED 2u
#define KSH_PROVISION_MACHINES_TRUNCATED 2u      /* head[KS_PLC_FLAGS]: the machine table was too small (KS_PLC_TRUNCATED is the row table's) */
typedef struct ksh_provision_out {
  uint32_t words;                            /* in: option words of a machine row, >= ceil(T/64) */
  uint32_t route;                            /* out: KSH_PROVISION_* */
  uint64_t cap_rows, cap_machines;           /* in */
  uint64_t total_rows, total_machines;       /* out */
  uint64_t head[KS_PLC_HEAD_WORDS];          /* out */
  uint64_t* rows; uint64_t* machines;        /* in: the caller's tables, or NULL with a capacity of 0 */
  int32_t* pick_type; int32_t* pick_zone; int32_t* pick_ct; double* pick_price;      /* in: [cap_machines] each, or all NULL */
} ksh_provision_out;
int ksh_provision(void* parsed_snapshot, uint32_t flags, const int32_t* pod_node /* or NULL after ksh_env_apply */, const uint32_t* deleting, uint32_t n_deleting, int device,
                  ksh_provision_out* out, double* ms /* [5] or NULL */);
/* The placement tables of handles whose results are on the device (ksh_solve_batch_resident / ksh_solve / ...; derived or not), ksh_replacement_rows' sibling:
 * ks_placement_rows_host (ksolve.h KS_PLC_*) over handles -- with it the pods behind a replacement command are readable without text.  out_heads[n][KS_PLC_HEAD_WORDS],
 * out_rows[cap_rows][KS_PLC_ROW_WORDS], capacity as above.  A what-if over a snapshot -- derived on the device or flattened by itself -- comes back in the snapshot's
 * ids, as ksh_provision's rows do: snapshot pod index, node slot, node slots + j, head[KS_PLC_N_EXISTING] = node slots.  Any other handle keeps its own: the pod
 * indices and existing-node indices ksh_result_arrays_get speaks of.  ms[2] (may be NULL): kernels | read-back and renaming. */
int ksh_placement_rows(void** handles, uint32_t n, const uint64_t* ids, uint64_t* out_heads, uint64_t* out_rows, uint64_t cap_rows, uint64_t* out_total_rows, double* ms /* [2] or NULL */);

/* ---- the AUDIT of results (ksolve.h ks_audit_dev, KS_AUDIT_*): every placement, every new node's Requests and InstanceTypeOptions checked on the device against the
 * problem the result answers -- the shim's gate before it acts on a result: a finding means "do not act on this, solve in Go, file the problem" (INTEGRATION.md).
 * ksh_audit works over any handles whose results are on the device, derived or not, as one launch sequence.  The caller's tables are sized as for ksh_placement_rows:
 * the totals are always written, the flag rows only when they fit (pod_flags: cap_pods >= n_pods; node_flags: cap_nodes >= n_nodes; else KSH_AUDIT_TRUNCATED_* and the
 * caller calls again with larger tables; cap 0 with a NULL table asks for the totals alone).  Indices are the problem's own: pod i and node n as
 * ksh_result_arrays_get numbers them (existing node n < n_existing, else new node n - n_existing); a what-if derived on the device numbers its pods in the snapshot's
 * queue order (ksh_placement_rows' KS_PLC_POSITION) and its existing nodes by the snapshot flattening's rows.  ms[2] (may be NULL): kernels | read-back. */
#define KSH_AUDIT_TRUNCATED_PODS 1u
#define KSH_AUDIT_TRUNCATED_NODES 2u
typedef struct ksh_audit_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_* */
  uint32_t* node_flags; uint64_t cap_nodes;    /* [cap_nodes] KS_AUDIT_NODE_* */
  uint32_t n_pods, n_nodes, n_new, n_unscheduled;
  uint32_t n_pods_flagged, n_nodes_flagged, truncated /* KSH_AUDIT_TRUNCATED_* */, pad;
  uint32_t pod_bit_count[32], node_bit_count[32];
} ksh_audit_out;
int ksh_audit(void** handles, uint32_t n, ksh_audit_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* The same for a result the caller CLAIMS for one flattened handle (uploaded if it is not; KS_ERR_UNSUPPORTED for a what-if derived on the device): the arrays of
 * ksh_result_arrays as ksh_result_arrays_get lays them out -- unscheduled [n_unscheduled], the per-node arrays [n_new] -- from wherever the caller got them.
 * node_pods_off / node_pods and pod_reason are not read; ksh_result_arrays carries no commit numbers, so the pod_seq clause of KS_AUDIT_POD_RANGE is ks_audit_dev's alone.
 * KS_ERR_INVALID: a NULL table, dimensions that are not the handle's, n_new > max_new_nodes. */
int ksh_audit_claimed(void* handle, const ksh_result_arrays* claimed, ksh_audit_out* out, double* ms /* [2] or NULL */);
/* The audit's SECOND pass, opt-in (ksolve.h ks_audit_topology_dev, KS_AUDIT_POD_SEQ .. KS_AUDIT_POD_HOSTNAME_SPREAD): pod (anti-)affinity and hostname spread, decided
 * from the final state and the commit numbers.  The shim's gate is both passes: ksh_audit, then this, and on a finding of either, solve in Go.  The same conventions:
 * the totals always, pod_flags when cap_pods >= n_pods (else KSH_AUDIT_TRUNCATED_PODS), indices as ksh_audit's.  checked[] says what each rule evaluated -- [0] placed
 * pods whose commit number was examined, [1] anti-affinity, [2] affinity, [3] hostname spread (pod, group) pairs --, skipped_groups the groups no rule looked at. */
typedef struct ksh_audit_topology_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_SEQ .. */
  uint32_t n_pods, n_new, n_placed, skipped_groups;
  uint32_t n_pods_flagged, truncated /* KSH_AUDIT_TRUNCATED_PODS */;
  uint32_t checked[4];
  uint32_t pod_bit_count[32];
} ksh_audit_topology_out;
int ksh_audit_topology(void** handles, uint32_t n, ksh_audit_topology_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle, as ksh_audit_claimed -- with the commit numbers as an array of their own, [n_pods] (KS_PLC_STAGE_SEQ's high half for a
 * placed pod, -1 for an unscheduled one), because ksh_result_arrays carries none.  KS_ERR_INVALID: pod_seq NULL, and ksh_audit_claimed's refusals. */
int ksh_audit_topology_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, ksh_audit_topology_out* out, double* ms /* [2] or NULL */);
/* The audit's THIRD pass, opt-in (ksolve.h ks_audit_spread_dev, KS_AUDIT_POD_SPREAD): topology spread over narrow keys -- the zone -- decided from the final state and
 * the commit numbers.  The shim's gate is the three passes in order: ksh_audit, ksh_audit_topology, then this, and on a finding of any, solve in Go.  The second
 * pass's conventions: the totals always, pod_flags when cap_pods >= n_pods (else KSH_AUDIT_TRUNCATED_PODS), indices as ksh_audit's.  checked[0]: the placed pods;
 * checked[1]: the (pod, group) pairs examined; exact_pairs: those for which the rule was the reference's own test; skipped_groups: the spread groups left unattempted. */
typedef struct ksh_audit_spread_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_SPREAD */
  uint32_t n_pods, n_new, n_placed, skipped_groups;
  uint32_t n_pods_flagged, truncated /* KSH_AUDIT_TRUNCATED_PODS */;
  uint32_t checked[2];
  uint32_t exact_pairs, pad;
} ksh_audit_spread_out;
int ksh_audit_spread(void** handles, uint32_t n, ksh_audit_spread_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle, exactly as ksh_audit_topology_claimed takes it. */
int ksh_audit_spread_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, ksh_audit_spread_out* out, double* ms /* [2] or NULL */);
/* The audit's FOURTH pass, opt-in (ksolve.h ks_audit_firstfit_dev, KS_AUDIT_POD_FIT_*): first-fit order -- a pod may not have ended later than a node, new node or
 * template whose final state would still take it -- decided from the final state and the commit numbers.  The shim's gate is the four passes in order: ksh_audit,
 * ksh_audit_topology, ksh_audit_spread, then this, and on a finding of any, solve in Go.  The second pass's conventions: the totals always, pod_flags when
 * cap_pods >= n_pods (else KSH_AUDIT_TRUNCATED_PODS), indices as ksh_audit's.  checked[0]: the placed pods; checked[1]: the pods examined (skipped_pods: the others);
 * checked[2]: the (class, node-or-template) pairs evaluated; admitting_pairs: those that admitted -- a clean result with none of them proved little. */
typedef struct ksh_audit_firstfit_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_FIT_* */
  uint32_t n_pods, n_new, n_placed, skipped_pods;
  uint32_t n_pods_flagged, truncated /* KSH_AUDIT_TRUNCATED_PODS */;
  uint32_t checked[3];
  uint32_t admitting_pairs;
} ksh_audit_firstfit_out;
int ksh_audit_firstfit(void** handles, uint32_t n, ksh_audit_firstfit_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle, as ksh_audit_topology_claimed takes it; this pass also reads node_types, node_requests, node_requests_present and
 * node_it_state of the claimed arrays. */
int ksh_audit_firstfit_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, ksh_audit_firstfit_out* out, double* ms /* [2] or NULL */);
/* The audit's FIFTH pass, opt-in (ksolve.h ks_audit_limits_dev, KS_AUDIT_NODE_LIMIT_*, KS_AUDIT_POD_LIMIT_TEMPLATE): provisioner limits -- no machine of a limited
 * provisioner keeps a type above what can have remained when it opened, none lacks a type that must have remained, and no pod passed over a limited provisioner that
 * still had room for it -- decided from the final state and the commit numbers.  The shim's gate is the five passes in order: ksh_audit, ksh_audit_topology,
 * ksh_audit_spread, ksh_audit_firstfit, then this, and on a finding of any, solve in Go.  The fourth pass's conventions for the pods (cap_pods,
 * KSH_AUDIT_TRUNCATED_PODS) and ksh_audit's for the nodes (cap_nodes, KSH_AUDIT_TRUNCATED_NODES; node n as ksh_audit numbers it).  limited_templates == 0: the
 * problem has no limits and nothing but the commit numbers was examined.  checked[0]: the placed pods; [1]: the new nodes of limited templates examined; [2]: the pods
 * examined (skipped_pods: the others); [3]: the (class, template) pairs evaluated.  exact_nodes: the nodes for which the rule was the reference's own test;
 * binding_nodes: the nodes whose limit excluded a type -- a clean result with none of them proved little; skipped_nodes: the new nodes without an opening order. */
typedef struct ksh_audit_limits_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_LIMIT_TEMPLATE */
  uint32_t* node_flags; uint64_t cap_nodes;    /* [cap_nodes] KS_AUDIT_NODE_LIMIT_* */
  uint32_t n_pods, n_nodes, n_new, n_placed;
  uint32_t limited_templates, skipped_nodes, skipped_pods, truncated /* KSH_AUDIT_TRUNCATED_* */;
  uint32_t n_pods_flagged, n_nodes_flagged, exact_nodes, binding_nodes;
  uint32_t checked[4];
  uint32_t pod_bit_count[32], node_bit_count[32];
} ksh_audit_limits_out;
int ksh_audit_limits(void** handles, uint32_t n, ksh_audit_limits_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle, exactly as ksh_audit_firstfit_claimed takes it. */
int ksh_audit_limits_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, ksh_audit_limits_out* out, double* ms /* [2] or NULL */);
/* The audit's SIXTH pass, opt-in (ksolve.h ks_audit_hostfit_dev, KS_AUDIT_POD_HFIT_*): the fourth pass's first-fit order for the pods it leaves out because a
 * topology group constrains them, where every such group is hostname anti-affinity or unfiltered hostname spread -- per-node counts that only grow.  The two passes
 * partition the pods they examine.  The fourth pass's conventions (cap_pods, KSH_AUDIT_TRUNCATED_PODS, indices as ksh_audit's).  eligible_groups: the groups the rule
 * covers, skipped_groups: the others.  checked[0]: the placed pods; [1]: the pods examined (skipped_pods: the others); [2]: the (class, node-or-template) pairs
 * evaluated; [3]: the (pair, group) count tests evaluated; admitting_pairs: the pairs that admitted -- a clean result with none of them proved little. */
typedef struct ksh_audit_hostfit_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_HFIT_* */
  uint32_t n_pods, n_new, n_placed, skipped_pods;
  uint32_t n_pods_flagged, truncated /* KSH_AUDIT_TRUNCATED_PODS */;
  uint32_t eligible_groups, skipped_groups;
  uint32_t checked[4];
  uint32_t admitting_pairs, pad;
} ksh_audit_hostfit_out;
int ksh_audit_hostfit(void** handles, uint32_t n, ksh_audit_hostfit_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle, exactly as ksh_audit_firstfit_claimed takes it. */
int ksh_audit_hostfit_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, ksh_audit_hostfit_out* out, double* ms /* [2] or NULL */);
/* The audit's NINTH pass, opt-in and beside the gate (ksolve.h ks_audit_zonefit_dev, KS_AUDIT_POD_ZFIT_*): first-fit order for the pods whose constraining groups are
 * all eligible zonal spread groups -- the pods neither the fourth nor the sixth pass examines.  The final state together with the commit numbers gives, per pod, the
 * zones that certainly admitted it at its moment; an earlier existing node, or an earlier-opened machine, in such a zone that the fourth pass's predicate admits
 * cannot have been passed over.  The fourth pass's conventions (cap_pods, KSH_AUDIT_TRUNCATED_PODS, indices as ksh_audit's).  eligible_groups / skipped_groups as the
 * sixth pass's; mixed_pods: the skipped pods whose class mixes zonal and hostname groups; checked[0]: the placed pods; [1]: the pods examined (skipped_pods: the
 * others); [2]: the (pod, node) pairs whose zone test ran; [3]: those that passed it; admitting_pairs: the pairs that admitted; exact_pods: the examined pods whose
 * zone masks are the reference's own numbers. */
typedef struct ksh_audit_zonefit_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_ZFIT_* */
  uint32_t n_pods, n_new, n_placed, skipped_pods;
  uint32_t n_pods_flagged, truncated /* KSH_AUDIT_TRUNCATED_PODS */;
  uint32_t eligible_groups, skipped_groups;
  uint32_t mixed_pods, exact_pods;
  uint32_t checked[4];
  uint32_t admitting_pairs, pad;
} ksh_audit_zonefit_out;
int ksh_audit_zonefit(void** handles, uint32_t n, ksh_audit_zonefit_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle, exactly as ksh_audit_firstfit_claimed takes it. */
int ksh_audit_zonefit_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, ksh_audit_zonefit_out* out, double* ms /* [2] or NULL */);
/* The audit's SEVENTH pass, opt-in (ksolve.h ks_audit_stages_dev, KS_AUDIT_POD_STAGE_*): relaxation order -- no pod ended at a later stage of its chain than one at
 * which an existing node's final state, or a fresh machine of a provisioner without limits, would have taken it, and no unscheduled pod stopped short of its chain's
 * end.  It is the gate's seventh pass (KS_AUDIT_PASS_STAGES through ksh_audit_gate_ex); this call remains the way to its flag rows.  The fourth pass's conventions (cap_pods, KSH_AUDIT_TRUNCATED_PODS, indices
 * as ksh_audit's).  checked[0]: the placed pods; [1]: the pods with an examined earlier stage (skipped_pods: the others -- most pods never relax); [2]: the examined
 * stages; [3]: the (class, existing-node-or-template) pairs evaluated; admitting_pairs: the pairs that admitted -- none in a clean result. */
typedef struct ksh_audit_stages_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_STAGE_* */
  uint32_t n_pods, n_new, n_placed, skipped_pods;
  uint32_t n_pods_flagged, truncated /* KSH_AUDIT_TRUNCATED_PODS */;
  uint32_t checked[4];
  uint32_t admitting_pairs, pad;
} ksh_audit_stages_out;
int ksh_audit_stages(void** handles, uint32_t n, ksh_audit_stages_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle, exactly as ksh_audit_firstfit_claimed takes it. */
int ksh_audit_stages_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, ksh_audit_stages_out* out, double* ms /* [2] or NULL */);
/* The audit's EIGHTH pass, opt-in (ksolve.h ks_audit_reasons_dev, KS_AUDIT_POD_REASON_*): the failure reasons -- pod_reason, the column recordSchedulingResults turns
 * into PodFailedToSchedule events, against what a fresh node of every machine template answers the pod's class: a placed pod carries no word, an unscheduled pod a
 * reason for each of the first eight templates, and wherever the flat problem alone decides the reason (taints, requirements, no instance type) the nibble equals it.
 * It is the gate's eighth pass (KS_AUDIT_PASS_REASONS through ksh_audit_gate_ex), which the shim calls before it synthesises events; this call remains the way to its
 * flag rows.  The other passes' conventions (cap_pods,
 * KSH_AUDIT_TRUNCATED_PODS, indices as ksh_audit's).  checked[0]: the unscheduled pods examined; [1]: their nibbles decided exactly; [2]: bounded to a set (a
 * topology-constrained class: one of 5, 6, 7); [3]: not examined (KS_WHY_LIMITS on a limited template, a template without types). */
typedef struct ksh_audit_reasons_out {
  uint32_t* pod_flags; uint64_t cap_pods;      /* [cap_pods] KS_AUDIT_POD_REASON_* */
  uint32_t n_pods, n_new, n_placed, n_unscheduled;
  uint32_t skipped_pods, n_pods_flagged, truncated /* KSH_AUDIT_TRUNCATED_PODS */, used_classes;
  uint32_t checked[4];
  uint32_t pairs, pad;
} ksh_audit_reasons_out;
int ksh_audit_reasons(void** handles, uint32_t n, ksh_audit_reasons_out* outs /* [n] */, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle: pod_node, pod_stage and pod_reason are read -- here pod_reason IS read --, nothing else and no commit numbers; a null
 * pod_reason is KS_ERR_INVALID, the remaining refusals are ksh_audit_claimed's. */
int ksh_audit_reasons_claimed(void* handle, const ksh_result_arrays* claimed, ksh_audit_reasons_out* out, double* ms /* [2] or NULL */);
/* The GATE (ksolve.h ks_audit_gate_dev, KS_AUDIT_PASS_*): the passes of a mask in ONE call, their totals and a list of findings reduced on the device.  This is the
 * shim's gate: one call behind every result, and on a finding, solve in Go; the per-pass calls above remain the way to the flag rows.  No flag row is read back: for
 * every requested pass the caller gives an array of n of that pass's out structs and receives in each exactly the totals the pass's own call writes -- the tables and
 * their capacities are neither read nor written, truncated is 0 -- and the passes that are not requested are not looked at.  findings: ks_audit_finding records
 * (problem = the handle's position in the batch | pass << 8 | table | index | flag word), ordered by pass, problem, pods before nodes, index -- the same list every
 * run.  n_findings is always the full count; with more than cap_findings of them the first cap_findings are written, KS_AUDIT_GATE_TRUNCATED is set and the table
 * beyond them is untouched.  cap_findings == 0 with findings == NULL is the plain yes/no gate: the results are clean iff n_findings == 0.
 * Refusals (nothing launched, nothing written): KS_ERR_INVALID for a mask that is empty or names an unknown pass, for findings == NULL with cap_findings != 0, for a
 * requested pass without its array; then the requested passes' own refusals, the earliest pass of the mask first. */
typedef struct ksh_audit_gate_out {
  ks_audit_finding* findings; uint64_t cap_findings;
  ksh_audit_out* audit; ksh_audit_topology_out* topology; ksh_audit_spread_out* spread; ksh_audit_firstfit_out* firstfit; ksh_audit_limits_out* limits; ksh_audit_hostfit_out* hostfit;   /* [n] each, for the requested passes */
  uint32_t n_findings, truncated /* KS_AUDIT_GATE_TRUNCATED */;
} ksh_audit_gate_out;
int ksh_audit_gate(void** handles, uint32_t n, uint32_t passes /* KS_AUDIT_PASS_* */, ksh_audit_gate_out* out, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle through the gate: taken once and uploaded once, with the union of the arrays the requested passes read.  pod_seq as
 * ksh_audit_topology_claimed takes it -- it may be NULL only when KS_AUDIT_PASS_FIRST is the whole mask; the first pass reads the placed pods numbered in pod order,
 * as ksh_audit_claimed gives them to it, whatever pod_seq says.  out's arrays hold one struct each. */
int ksh_audit_gate_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, uint32_t passes, ksh_audit_gate_out* out, double* ms /* [2] or NULL */);
/* The gate over ALL EIGHT passes (ksolve.h ks_audit_gate_ex_dev, KS_AUDIT_PASS_STAGES, KS_AUDIT_PASS_REASONS, KS_AUDIT_PASS_ALL_EX): ONE call behind every result.
 * ksh_audit_gate_out above is pinned -- its layout and bit 64's refusal through the two calls above stay --, so the wide form is a struct that can grow:
 * struct_size leads, the caller's sizeof, and the passes after the sixth have their pointers at the END, in the order of their bits.  A mask bit is known iff it
 * lies within KS_AUDIT_PASS_ALL_EX and its pointer lies wholly within struct_size; any other bit is KS_ERR_INVALID "audit gate: unknown pass", as is a struct_size
 * below the offset of `stages`.  Everything else -- totals, findings (pass 6 and 7 in `where` for the two new passes, pod tables only), their order, n_findings,
 * the truncation bit, the untouched tail, capacity 0 -- is ksh_audit_gate's. */
typedef struct ksh_audit_gate_ex_out {
  uint32_t struct_size, pad;      /* in: sizeof(ksh_audit_gate_ex_out) as the caller was compiled */
  ks_audit_finding* findings; uint64_t cap_findings;
  ksh_audit_out* audit; ksh_audit_topology_out* topology; ksh_audit_spread_out* spread; ksh_audit_firstfit_out* firstfit; ksh_audit_limits_out* limits; ksh_audit_hostfit_out* hostfit;   /* [n] each, for the requested passes */
  uint32_t n_findings, truncated /* KS_AUDIT_GATE_TRUNCATED */;
  ksh_audit_stages_out* stages;   /* [n], for KS_AUDIT_PASS_STAGES */
  ksh_audit_reasons_out* reasons; /* [n], for KS_AUDIT_PASS_REASONS */
} ksh_audit_gate_ex_out;
int ksh_audit_gate_ex(void** handles, uint32_t n, uint32_t passes /* KS_AUDIT_PASS_* */, ksh_audit_gate_ex_out* out, double* ms /* [2] kernels | read-back, or NULL */);
/* A claimed result for one flattened handle through the wide gate: taken once and uploaded once, with the union of the arrays the requested passes read -- pod_reason
 * (ksh_result_arrays) among them only when KS_AUDIT_PASS_REASONS is requested; a null pod_reason is then that pass's refusal, after every earlier pass's.  pod_seq
 * may be NULL only when the mask lies within KS_AUDIT_PASS_FIRST | KS_AUDIT_PASS_REASONS, the two passes that take no commit numbers; the first pass reads the
 * placed pods numbered in pod order, as ksh_audit_claimed gives them to it, whatever pod_seq says. */
int ksh_audit_gate_ex_claimed(void* handle, const ksh_result_arrays* claimed, const int32_t* pod_seq /* [n_pods] */, uint32_t passes, ksh_audit_gate_ex_out* out, double* ms /* [2] or NULL */);

/* ---- the snapshot kept current by EVENTS ("cached incremental SoA builder fed from state.Cluster") ----
 * Replaces, for the snapshot consolidation simulates over, what the reference does between two passes of the deprovisioner (deprovisioning/controller.go:64,
 * every 10 s): state.Cluster hears UpdateNode / DeleteNode / UpdatePod / DeletePod (pkg/controllers/state/cluster.go:151-200) and patches its nodes in place
 * (state/node.go:161-182 updateForPod / cleanupForPod; Available() = Allocatable - the requests of the pods bound, node.go:113); the next pass then flattens
 * everything again (helpers.go:42-99 -> provisioner.go:237-296).  Here the events patch the objects ksh_parse holds AND the snapshot's flattening follows them.
 * `ksd_text`:  KSD1 <n>  { NODE+ <KSP1 NODE record without its keyword>  |  NODE= <the same record>  |  NODE- <node name>  |  BIND <node name> POD <KSP1 pod record>  |  UNBIND <pod uid>
 *                         |  IT= <KSP1 IT record without its keyword> }*  END
 *   NODE+   a state node joins (slot = the next node index; slots are never reused, candidate sets keep naming nodes by slot)
 *   NODE-   a state node leaves; the pods bound to it are unbound with it
 *   BIND    a pod is bound to a node: it joins the snapshot's pods (index = the next one), the node's available resources shrink by RequestsForPods(pod),
 *           its host ports and volumes join the node's usage
 *   UNBIND  the reverse
 *   NODE=   a state node that is in state already is replaced in place (state.Cluster.UpdateNode on every node reconciliation after the first sight of the node,
 *           cluster.go:151-166, newStateFromNode :227-255; NODE+ is the first sight).  The record's name must be a live state node -- a node that left is not --
 *           or the event is refused with "NODE=: no state node named X".  The node keeps its slot, the pods bound to it stay bound to that slot
 *           (ksh_snapshot_bindings does not change, the mirrored cluster pods name the same node).  Everything else the record carries REPLACES what the slot
 *           held: labels, taints, available, capacity, daemonset requests, host ports, volume limits, volumes -- taken as given: they are state.Node's own
 *           outputs at the moment of the event, already net of the pods bound; later BIND / UNBIND patch from there.  The provisioner-name label may change
 *           (owned <-> unowned, another provisioner).  The record's in_state word is not read: the node is in state.
 *   IT=     an instance type of the catalogue is replaced in place: what cloudProvider.GetInstanceTypes lists NOW (Provisioner.NewScheduler asks on every pass,
 *           provisioner.go:237-296) -- an offering unavailable or back, a price moved, the zone / capacity-type requirement values that follow availability.  The
 *           record's name must be the name of an instance type of the parsed object, or the event is refused with "IT=: no instance type named X".  The type
 *           keeps its index: provisioners' instance-type lists, nodes' instance-type labels and every InstanceTypeOptions bit keep their meaning.  Requirements,
 *           offerings, capacity and overhead of the record REPLACE what the slot held.  Types are neither added nor removed: one the provider no longer lists is
 *           a record with no available offering.  A record the ingest doors would refuse -- a requirement with Gt / Lt ("IT=: instance type requirement with
 *           Gt/Lt bounds"), one on kubernetes.io/hostname ("IT=: instance type requirement on hostname") -- ends the call with KS_ERR_UNSUPPORTED, nothing of
 *           that event applied (the events before it stay, info[0] counts them).  Continued (info[3] = 1) when the record differs from the one before in its
 *           offerings (availability, price, which pairs are listed) or in the values of its requirements, and the universes a run from scratch would build are
 *           the same: every zone, capacity type and requirement value it names is in them, no value it no longer names was the last use (other types, the
 *           provisioners, the batch and the nodes are asked), and the topology-domain universe NewScheduler builds from the types' requirement values is the
 *           same set.  The columns / rows of the touched types in the it_* arrays are then encoded anew, the others taken over.  The full run (info[3] = 0,
 *           same bytes) for anything else: a zone or value no universe has, the last use of one, a requirement key that comes or goes, a changed
 *           node.kubernetes.io/instance-type requirement, and ANY change of capacity or overhead (resource names, and everything made from the allocatable).
 *           A Solve over these objects (ksh_solve_from_batch) flattens its environment again after the event, as after every other.
 * The first call hands the snapshot's bindings over (`pod_node`, as the what-if calls take it); from then on the library holds them -- every call that takes a
 * `pod_node` accepts NULL for "the library's", ksh_snapshot_bindings reads them.  info[0] = events applied (an event that cannot be applied ends the call with
 * KS_ERR_INVALID; the ones before it stay), info[1] / info[2] = node / pod slots, info[3] = 1 when the snapshot's flattening was CONTINUED from the one before:
 * pods already seen keep their specs, the catalogue's arrays, the universes and the old nodes' requirement rows are taken over (possible while the events bring no
 * label key / value / resource name the universes lack; otherwise, and when no flattening existed yet, the next what-if call flattens from scratch -- same result
 * either way, tests/test_env_apply.py compares the two byte for byte).  A NODE= bumps the change stamp of its slot: the continuation rebuilds the requirement row
 * of such a slot and takes over the rows of the others (taints, remaining resources, volume counts and the per-node topology tables behind the device derivation
 * are worked out for every node on either road).  It is continued (info[3] = 1) while the universes stay put -- an initialised flip whose two values other nodes
 * carry, a taint of the known set added or removed, available / capacity changed, an ownership change among known provisioners.  It falls back to the full run
 * (info[3] = 0, same bytes) when the update brings a label value of a referenced key, a taint or a resource name (under KSH_ACTIVE_RESOURCES: a name in its
 * daemonset requests) that the flattening before did not have, when it removes the last use of a label value, and when it changes which resource names that only nodes
 * carry the node lists.  The objects are patched in place: do not call while another thread solves over this
 * snapshot; handles opened before the call keep what they were opened with.  KS_ERR_INVALID "spare room ... used up": the snapshot was parsed with room for a
 * quarter more nodes / pods (at least 256 / 4096); ingest it again. */
int ksh_env_apply(void* parsed_snapshot, const int32_t* pod_node /* first call: the bindings; later NULL */, const char* ksd_text, size_t len, uint32_t info[4] /* or NULL */);
/* ---- the same door without the text: the events as ONE stream of u32 words over ONE string table (conventions of ksh_env_block; grammar in
 * karpenter_core_amd/host/kspb.hpp, DeltaReader).  Per event a kind word, then its body: KSH_EVENT_NODE_ADD the state-node record of ksh_env_block, KSH_EVENT_NODE_REMOVE
 * the node's name, KSH_EVENT_BIND the node's name + the pod (word count, spec record of ksh_pod_block, uid, creationTimestamp as two words), KSH_EVENT_UNBIND the pod's uid,
 * KSH_EVENT_NODE_UPDATE (NODE=) the state-node record again, word for word what KSH_EVENT_NODE_ADD carries, KSH_EVENT_INSTANCE_TYPE_UPDATE (IT=) the
 * instance_type record of ksh_env_block.
 * A cgo caller fills it with the writer it has for the other two doors; quantities are int64 milli-units, nothing is quoted or printed.  Everything after the decoding is
 * ksh_env_apply's: same patching, same info[0..3], same bindings held by the library, same error texts for an event that cannot be applied (the events before it stay,
 * info[0] counts them).  Text and binary calls may be mixed on one snapshot in any order.
 * Stricter than the text door: the block is decoded completely before the first event is applied, so a MALFORMED block -- string id >= n_strings, offsets not ascending or
 * beyond str_bytes_len, a record running past n_words, words left over, an unknown kind, n_events not matching the stream -- is KS_ERR_INVALID with the event's index in
 * ksh_last_error() and NOTHING applied.
 * flags: 0, or KSH_APPLY_TRACK_CLUSTER_PODS -- BIND / UNBIND are mirrored into the snapshot's cluster pods (what countDomains lists, topology.go:231-276) whatever the
 * snapshot held at the first call.  Without it the door does what ksh_env_apply does: it mirrors iff the snapshot had cluster pods when the first event call was made, so a
 * topology-tracking snapshot that starts with no bound pod must pass the flag.  Any other bit: KS_ERR_INVALID. */
#define KSH_EVENT_NODE_ADD 1u
#define KSH_EVENT_NODE_REMOVE 2u
#define KSH_EVENT_BIND 3u
#define KSH_EVENT_UNBIND 4u
#define KSH_EVENT_NODE_UPDATE 5u
#define KSH_EVENT_INSTANCE_TYPE_UPDATE 6u
#define KSH_APPLY_TRACK_CLUSTER_PODS 1u
typedef struct ksh_delta_block {
  uint32_t n_events, n_strings, n_words;
  const uint32_t* str_off;      /* [n_strings + 1] byte offsets into str_bytes */
  const char* str_bytes;
  const uint32_t* words;        /* [n_words] */
  uint64_t str_bytes_len;       /* bytes behind str_bytes: str_off[n_strings] must not reach beyond */
} ksh_delta_block;
int ksh_env_apply_block(void* parsed_snapshot, const int32_t* pod_node /* first call: the bindings; later NULL */, const ksh_delta_block* delta, uint32_t flags, uint32_t info[4] /* or NULL */);
int ksh_snapshot_bindings(void* parsed_snapshot, int32_t* out /* [cap] or NULL */, uint32_t cap, uint32_t* n_pods /* or NULL */, uint32_t* n_nodes /* or NULL */);
/* Diagnostic (tests): FNV-1a over the snapshot's flattening -- the flat problem and the per-node tables behind the device derivation; `cold` != 0: of a
 * flattening made from scratch for the comparison (nothing cached is touched); flags with KSH_DERIVE_VOLUMES: of the flattening derived volume what-ifs use. */
int ksh_snapshot_fingerprint(void* parsed_snapshot, const int32_t* pod_node /* or NULL */, uint32_t flags, int cold, uint64_t* out);

#ifdef __cplusplus
}
#endif
#endif /* KSHOST_H */
