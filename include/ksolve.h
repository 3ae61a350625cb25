/* ksolve.h -- C ABI of libksolve.so: the MI355X (gfx950) drop-in for karpenter-core's provisioning
 * scheduler hot path.
 *
 * What it replaces (reference paths relative to aws/karpenter-core):
 *   ks_solve / ks_solve_dev      <->  (*Scheduler).Solve       pkg/controllers/provisioning/scheduling/scheduler.go:96-133
 *                                     called from provisioner.go:307 and deprovisioning/helpers.go:93
 *   ks_solve_batch               <->  N independent simulateScheduling what-ifs, deprovisioning/helpers.go:42-115
 *                                     (multinodeconsolidation.go:74-114, singlenodeconsolidation.go:43-78)
 *   ks_price_filter_dev          <->  filterByPrice / worstLaunchPrice on a what-if's replacement node,
 *                                     deprovisioning/helpers.go:148-157,292-315 (consolidation.go:238, multinodeconsolidation.go:164)
 *   ks_consolidation_commands_dev <-> computeConsolidation's decision over a what-if's result, deprovisioning/consolidation.go:190-274,
 *                                     and filterOutSameType, multinodeconsolidation.go:132-165
 *   ks_validate_commands_dev     <->  Validation.ValidateCommand's verdict over a re-simulation's result, deprovisioning/validation.go:118-171
 *   ks_feasibility_grid          <->  filterInstanceTypesByRequirements for a fresh node, node.go:137-159
 *                                     (compatible && fits && hasOffering over every instance type)
 *   ks_probe_*                   <->  Requirement.Intersection/Has/Operator/Len, Requirements.Compatible
 *                                     pkg/scheduling/requirement.go:117-204, requirements.go:123-206
 *
 * The reference has no FFI for this path (pure Go); a Go shim would flatten
 * []*v1.Pod / []*cloudprovider.InstanceType / []*state.Node into `ks_problem` (INTEGRATION.md shows
 * the cgo stub).  Everything crossing the boundary is plain pointers + sizes: no torch types, no C++
 * types, no callbacks.  Buffers are owned by the caller and only read during the call (cgo pointer
 * rules); results are written into caller-allocated arrays.
 *
 * Encoding (DESIGN.md "Data layout"):
 *   keys      K <= 32 "narrow" label keys, each with a universe of <= 64 values interned in ascending
 *             byte-wise string order (bit i of a mask == value i).  A requirement on key k is
 *             {present, complement, mask, gt, lt} == reference Requirement{complement, values,
 *             greaterThan, lessThan} (requirement.go:36-42).
 *   instance-type key  node-side states x pod-side requirement columns (tables its_inter / its_fail / its_types)
 *             because its universe is the whole catalogue.
 *   hostname key       implicit: new node n owns a placeholder hostname no pod can name (node.go:46);
 *             existing node e owns hostname e.  Pod classes carry {mode, list of existing-node ids}.
 *   resources R <= 16 int64 milli-units; index 0 = cpu, 1 = memory, 2 = pods.  A problem with more than 8 runs on
 *             the wide kernel variants; up to 8 take the same kernels as always.
 *   taints    <= 64 distinct (key,value,effect) triples -> u64 masks; tolerations pre-evaluated.
 *   offerings zone x capacity-type pairs (<= 64) -> u64 per instance type.
 *   pods      deduplicated into classes (one per distinct pod spec x relaxation stage); a pod is a
 *             chain of class ids, one per Preferences.Relax stage (preferences.go:36-56).
 *   topology  groups (spread / affinity / anti-affinity, inverse anti-affinity) with pre-counted
 *             domains (topology.go:231-276 needs the API server and therefore stays host-side).
 */
#ifndef KSOLVE_H
#define KSOLVE_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KS_MAX_KEYS 32
#define KS_MAX_RES 16
#define KS_MAX_VALUES 64
#define KS_MAX_ITSTATES 65535
#define KS_NO_BOUND_GT INT32_MIN /* "no greaterThan" */
#define KS_NO_BOUND_LT INT32_MAX /* "no lessThan"   */
#define KS_KEY_HOSTNAME (-2)
#define KS_KEY_NONE (-1)

/* error codes (Solve itself never fails: scheduler.go:132 always returns a nil error) */
#define KS_OK 0
#define KS_ERR_INVALID (-1)     /* malformed ks_problem */
#define KS_ERR_UNSUPPORTED (-2) /* feature outside the supported encoding */
#define KS_ERR_DEVICE (-3)      /* HIP failure / no gfx950 device: the library never falls back to a CPU path */
#define KS_ERR_CAPACITY (-4)    /* more new nodes than max_new_nodes */
#define KS_ERR_INTERNAL (-5)    /* device-side watchdog: the pack loop did not terminate within its step bound */

/* A family of requirement sets (reference scheduling.Requirements), n sets x K keys, SoA. */
typedef struct ks_reqsets {
  uint32_t n;
  const uint32_t* present;    /* [n]   bit k: key k has a requirement                         */
  const uint32_t* complement; /* [n]   bit k: requirement.go:38 `complement`                  */
  const uint64_t* mask;       /* [n*K] value set over the key's universe                      */
  const int32_t* gt;          /* [n*K] greaterThan or KS_NO_BOUND_GT                          */
  const int32_t* lt;          /* [n*K] lessThan    or KS_NO_BOUND_LT                          */
  const int32_t* it_state;    /* [n]   state of the instance-type key (0 == key absent)       */
} ks_reqsets;

/* The [..] comments below state each array's length for the reader; KS_PROBLEM_ARRAYS under the struct is the executable form of the same lengths. */
typedef struct ks_problem {
  /* ---- dimensions ---- */
  uint32_t P;  /* pods in the batch                                   */
  uint32_t C;  /* pod classes                                         */
  uint32_t T;  /* instance types (TW = ceil(T/64) mask words)         */
  uint32_t M;  /* machine templates == provisioners, weight order     */
  uint32_t E;  /* existing (owned, in-state) nodes, caller's order    */
  uint32_t K;  /* narrow keys                                         */
  uint32_t R;  /* resources                                           */
  uint32_t G;  /* topology groups (topologies first, then inverse)    */
  uint32_t GH; /* groups whose key is the hostname                    */
  uint32_t S;  /* instance-type-key states a node can be in (0 = key absent)                       */
  uint32_t SC; /* instance-type-key requirements a pod class / topology filter can carry (0 = none) */
  uint32_t max_new_nodes; /* capacity for scheduling.Node records (<= P is always enough) */
  uint32_t flags;         /* KS_FLAG_* */

  /* ---- keys ---- */
  uint32_t wellknown_mask;     /* bit k: key k in v1alpha5.WellKnownLabels (labels.go:84-92 + provider additions) */
  const uint32_t* key_nvalues; /* [K] */
  const int32_t* value_int;    /* [K*64] strconv.Atoi of the value or INT32_MIN when not an integer (requirement.go:232) */
  int32_t key_zone, key_ct;    /* narrow-key index of topology.kubernetes.io/zone, karpenter.sh/capacity-type, or -1 */
  uint32_t n_ct;               /* offering pair index = zone_value * n_ct + ct_value */

  /* ---- instance types (cloudprovider.InstanceType, types.go:72-89), SoA over T ---- */
  const uint32_t* it_present;    /* [T] */
  const uint32_t* it_complement; /* [T] */
  const uint64_t* it_mask;       /* [K*T]  it_mask[k*T+t] */
  const int64_t* it_alloc;       /* [R*T]  Allocatable() = Capacity - Overhead.Total(), types.go:87-102 */
  const int64_t* it_cap;         /* [R*T]  Capacity (provisioner limits, scheduler.go:273-309) */
  const uint64_t* it_offer;      /* [T]    available (zone,capacity-type) pairs, types.go:106-128 */
  const double* it_price;        /* [T*NP] Offering.Price of available pair p (NP = key_nvalues[key_zone] * n_ct; the highest one if a pair is offered
                                    twice): read by the consolidation price stage only (ks_price_filter_dev); may be NULL */
  const double* it_price_lo;     /* [T*NP] the LOWEST Offering.Price of available pair p (Offerings.Cheapest, types.go:141): read by ks_launch_pick_dev; NULL -> it_price */
  int32_t ct_spot, ct_ondemand;  /* value ids of "spot" / "on-demand" in the capacity-type key's universe, or -1 */
  /* instance-type key lattice */
  const uint16_t* its_inter; /* [S*SC] node state after intersecting node state a with pod-side req b  */
  const uint8_t* its_fail;   /* [S*SC] Requirements.Intersects error for existing=a, incoming=b        */
  const uint8_t* its_nidne;  /* [S]   operator in {NotIn, DoesNotExist}                                */
  const uint64_t* its_types; /* [S*TW] types whose own `instance-type In [name]` passes against state s */

  /* ---- machine templates (machinetemplate.go:46-62), order = OrderByWeight (provisioner.go:132-136) ---- */
  ks_reqsets tmpl;               /* n = M */
  const uint64_t* tmpl_taints;   /* [M] */
  const int64_t* tmpl_daemon;    /* [M*R] getDaemonOverhead, scheduler.go:250-267 */
  const uint32_t* tmpl_daemon_present; /* [M] resource presence bits of that ResourceList */
  const uint64_t* tmpl_types;    /* [M*TW] the provisioner's instance types */
  const uint32_t* tmpl_limit_present;  /* [M] bit r: resource r is limited; 0xFFFFFFFF == Spec.Limits nil (scheduler.go:71-75) */
  const int64_t* tmpl_remaining; /* [M*R] remainingResources after existing nodes (scheduler.go:244-246) */

  /* ---- existing nodes (existingnode.go:41-75) ---- */
  ks_reqsets en;               /* n = E : NewLabelRequirements(node.Labels) (hostname implicit) */
  const uint64_t* en_taints;   /* [E] */
  const int64_t* en_avail;     /* [E*R] state.Node.Available() */
  const int64_t* en_requests;  /* [E*R] remaining daemon requests, clamped at 0 (existingnode.go:44-53) */
  const uint32_t* en_requests_present; /* [E] */
  const uint32_t* en_port_off; /* [E+1] into ports[] */
  /* volume limits (existingnode.go:87-94, volumeusage.go:102-143; new nodes do not track volumes).  ND == 0: no class mounts a limited volume */
  uint32_t ND;                 /* CSI drivers some existing node limits (<= 64) */
  uint32_t SW;                 /* 64-bit words of the shared-claim sets: claims that can be on a node before the pod arrives */
  const int32_t* en_vol_limit; /* [E*ND] VolumeLimits()[driver], INT32_MAX == no limit */
  const int32_t* en_vol_count; /* [E*ND] distinct claims of the driver mounted on the node */
  const uint64_t* en_vol_set;  /* [E*SW] which shared claims those include */

  /* ---- pod classes ---- */
  ks_reqsets cls;                 /* n = C : NewPodRequirements, requirements.go:61-78 */
  const uint8_t* cls_hn_mode;     /* [C] hostname requirement: 0 none, 1 In list, 2 NotIn list (Exists = 2 + empty) */
  const uint32_t* cls_hn_off;     /* [C+1] into hn_list[] (existing-node indices) */
  const uint32_t* hn_list;        /* [cls_hn_off[C]] */
  const int64_t* cls_requests;    /* [C*R] resources.RequestsForPods(pod), resources.go:25-33 */
  const uint32_t* cls_requests_present; /* [C] */
  const uint64_t* cls_tolerated;  /* [C] bit i: some toleration ToleratesTaint(taint i) (taints.go:28-40) */
  const uint32_t* cls_port_off;   /* [C+1] into ports[] */
  const uint64_t* ports;          /* [cls_port_off[C]], or [en_port_off[E]] when C == 0: the existing nodes' reservations first, then the classes' ports.  proto<<56 | port<<32 | ip_id (ip_id 0 == unspecified 0.0.0.0/::), hostportusage.go:39-57 */
  const uint32_t* cls_vol_off;    /* [C+1] into vol_list[] */
  const uint32_t* vol_list;       /* [cls_vol_off[C]] the class's volumes, ordered by driver: driver<<24 | shared-claim bit        (bit 31 clear)
                                     1<<31 | driver<<24 | n : n claims no other pod or node mounts
                                     0xFFFFFFFF            : VolumeUsage.validate failed -> no existing node accepts the pod */
  /* topology membership of a class (CSR lists of group ids) */
  const uint32_t* cls_own_off;  /* [C+1] groups in Topology.topologies owned by the pod; entry = g | selfSelecting<<31 */
  const uint32_t* own_list;     /* [cls_own_off[C]] */
  const uint32_t* cls_sel_off;  /* [C+1] non-inverse groups whose selector selects the pod (Record, topology.go:120-133) */
  const uint32_t* sel_list;     /* [cls_sel_off[C]] */
  const uint32_t* cls_isel_off; /* [C+1] inverse groups selecting the pod (getMatchingTopologies, topology.go:358-362) */
  const uint32_t* isel_list;    /* [cls_isel_off[C]] */
  const uint32_t* cls_iown_off; /* [C+1] inverse groups owned by the pod (Record, topology.go:136-141) */
  const uint32_t* iown_list;    /* [cls_iown_off[C]] */

  /* ---- pods ---- */
  const uint32_t* pod_stage_off; /* [P+1] into stage_cls[]: one class per relaxation stage */
  const uint32_t* stage_cls;     /* [pod_stage_off[P]] class ids */
  const uint32_t* queue;         /* [P] initial queue order: byCPUAndMemoryDescending, queue.go:74-110 */

  /* ---- topology groups (topologygroup.go:53-86) ---- */
  const uint8_t* grp_type;      /* [G] 0 spread, 1 pod affinity, 2 pod anti-affinity */
  const int32_t* grp_key;       /* [G] narrow key index or KS_KEY_HOSTNAME */
  const int32_t* grp_max_skew;  /* [G] */
  const uint8_t* grp_active;    /* [G] 1: exists after NewTopology; 0: created by a later Topology.Update (topology.go:86-117) */
  const uint32_t* grp_filter_off; /* [G+1] TopologyNodeFilter terms (topologynodefilter.go:28-70) into `flt`; empty == always */
  ks_reqsets flt;               /* n = flt.n terms (grp_filter_off[G] of them are referenced) */
  const int32_t* grp_count;     /* [G*64] initial domain counts (countDomains, topology.go:231-276); -1 == not a registered domain */
  const int32_t* grp_hslot;     /* [G] row in the hostname tables or -1 */
  const int32_t* grph_count;    /* [GH*E] initial counts on the existing nodes' hostnames; -1 unregistered */
  const int32_t* grph_extra_pos;/* [GH] hostnames outside the state nodes with count > 0 (pod affinity options) */
  uint32_t n_topologies;        /* groups [0, n_topologies) are Topology.topologies, the rest inverseTopologies */
  uint32_t lean_r8;             /* != 0: the LEAN kernel variants may take this problem at up to 8 resources (their RM = 8 instantiations); 0 (every problem before this
                                   field existed): LEAN at R <= 4 only, so such a problem runs the kernel it always ran.  libkshost sets it for a problem flattened under
                                   KSH_ACTIVE_RESOURCES.  A kernel choice, not part of the problem: no fingerprint covers it, no result depends on it. */
} ks_problem;

/* ---- the arrays of ks_problem, each named ONCE.  For the library's own use (libksolve's upload, libkshost's flattening and fingerprint, ks_debug_problem_array): not
 * an interface.  Whoever adds an array to ks_problem adds its row here, and the wiring, the length check, the upload and the fingerprint follow.
 *   X(field, owner, count, share)   one array.
 *   XRS(field, n)                   one ks_reqsets member: its six arrays, present / complement / it_state of n elements, mask / gt / lt of n * K.
 * count: elements, over a `const ks_problem* p`; an offset array is listed before the list it measures, so a count never reads an array that was not checked yet.
 * owner: whose vector backs the pointer in libkshost's flattening -- SELF the flattening itself, CAT its catalogue() (a what-if over a shared snapshot points at the
 *        snapshot's), LAT its lattice().
 * share: the rule of ks_problem_upload_shared -- NEVER copied always; CAT not copied when the host pointer is the one `base` was uploaded from; LAT the same, and S / SC
 *        agree with base's; PRICE the same, and key_zone / key_ct / n_ct agree with base's -- such an array may be NULL and is then not uploaded;
 *        PRICE_LO as PRICE, NULL falls back to it_price, and the array is NOT FINGERPRINTED (the one row that is not): only ks_launch_pick_dev reads it, no Solve
 *        depends on it, and it arrived after the committed fingerprints were pinned.
 * The rows stand in the order libkshost's fingerprint hashes them, which is pinned (tests/golden); the upload packs its copied region in the same order. */
#define KS_TW(p) (((size_t)(p)->T + 63) / 64)
#define KS_NP(p) ((p)->key_zone >= 0 && (p)->key_ct >= 0 ? (size_t)(p)->key_nvalues[(p)->key_zone] * (p)->n_ct : (size_t)0) /* (zone, capacity-type) pairs */
#define KS_PROBLEM_ARRAYS(X, XRS) \
  X(key_nvalues, SELF, p->K, NEVER) \
  X(value_int, SELF, (size_t)p->K * 64, NEVER) \
  X(it_present, CAT, p->T, CAT) \
  X(it_complement, CAT, p->T, CAT) \
  X(it_mask, CAT, (size_t)p->K * p->T, CAT) \
  X(it_offer, CAT, p->T, CAT) \
  X(it_price, CAT, (size_t)p->T * KS_NP(p), PRICE) \
  X(it_price_lo, CAT, (size_t)p->T * KS_NP(p), PRICE_LO) \
  X(it_alloc, CAT, (size_t)p->R * p->T, CAT) \
  X(it_cap, CAT, (size_t)p->R * p->T, CAT) \
  X(its_inter, LAT, (size_t)p->S * p->SC, LAT) \
  X(its_fail, LAT, (size_t)p->S * p->SC, LAT) \
  X(its_nidne, LAT, p->S, LAT) \
  X(its_types, LAT, (size_t)p->S * KS_TW(p), LAT) \
  XRS(tmpl, p->M) \
  XRS(en, p->E) \
  XRS(cls, p->C) \
  XRS(flt, p->flt.n) \
  X(tmpl_taints, SELF, p->M, NEVER) \
  X(tmpl_types, SELF, (size_t)p->M * KS_TW(p), NEVER) \
  X(tmpl_daemon, SELF, (size_t)p->M * p->R, NEVER) \
  X(tmpl_remaining, SELF, (size_t)p->M * p->R, NEVER) \
  X(tmpl_daemon_present, SELF, p->M, NEVER) \
  X(tmpl_limit_present, SELF, p->M, NEVER) \
  X(en_taints, SELF, p->E, NEVER) \
  X(en_avail, SELF, (size_t)p->E * p->R, NEVER) \
  X(en_requests, SELF, (size_t)p->E * p->R, NEVER) \
  X(en_requests_present, SELF, p->E, NEVER) \
  X(en_port_off, SELF, (size_t)p->E + 1, NEVER) \
  X(cls_hn_mode, SELF, p->C, NEVER) \
  X(cls_hn_off, SELF, (size_t)p->C + 1, NEVER) \
  X(hn_list, SELF, p->C ? p->cls_hn_off[p->C] : 0, NEVER) \
  X(cls_requests, SELF, (size_t)p->C * p->R, NEVER) \
  X(cls_requests_present, SELF, p->C, NEVER) \
  X(cls_tolerated, SELF, p->C, NEVER) \
  X(cls_port_off, SELF, (size_t)p->C + 1, NEVER) \
  X(ports, SELF, p->C ? p->cls_port_off[p->C] : (p->E ? p->en_port_off[p->E] : 0), NEVER) \
  X(en_vol_limit, SELF, (size_t)p->E * p->ND, NEVER) \
  X(en_vol_count, SELF, (size_t)p->E * p->ND, NEVER) \
  X(en_vol_set, SELF, (size_t)p->E * p->SW, NEVER) \
  X(cls_vol_off, SELF, (size_t)p->C + 1, NEVER) \
  X(vol_list, SELF, p->C ? p->cls_vol_off[p->C] : 0, NEVER) \
  X(cls_own_off, SELF, (size_t)p->C + 1, NEVER) \
  X(own_list, SELF, p->C ? p->cls_own_off[p->C] : 0, NEVER) \
  X(cls_sel_off, SELF, (size_t)p->C + 1, NEVER) \
  X(sel_list, SELF, p->C ? p->cls_sel_off[p->C] : 0, NEVER) \
  X(cls_isel_off, SELF, (size_t)p->C + 1, NEVER) \
  X(isel_list, SELF, p->C ? p->cls_isel_off[p->C] : 0, NEVER) \
  X(cls_iown_off, SELF, (size_t)p->C + 1, NEVER) \
  X(iown_list, SELF, p->C ? p->cls_iown_off[p->C] : 0, NEVER) \
  X(pod_stage_off, SELF, (size_t)p->P + 1, NEVER) \
  X(stage_cls, SELF, p->P ? p->pod_stage_off[p->P] : 0, NEVER) \
  X(queue, SELF, p->P, NEVER) \
  X(grp_type, SELF, p->G, NEVER) \
  X(grp_active, SELF, p->G, NEVER) \
  X(grp_key, SELF, p->G, NEVER) \
  X(grp_max_skew, SELF, p->G, NEVER) \
  X(grp_count, SELF, (size_t)p->G * 64, NEVER) \
  X(grp_hslot, SELF, p->G, NEVER) \
  X(grph_count, SELF, (size_t)p->GH * p->E, NEVER) \
  X(grph_extra_pos, SELF, p->GH, NEVER) \
  X(grp_filter_off, SELF, (size_t)p->G + 1, NEVER)
/* The table covers the struct: the pointer members its rows name (a ks_reqsets member counts whole) plus the bytes of everything else -- the scalar members and the
 * padding after them -- are sizeof(ks_problem).  An array added to the struct without a row fails this; after adding a SCALAR member, add what it makes sizeof grow by. */
#define KS_PROBLEM_SCALAR_BYTES 96 /* 23 four-byte scalars and 4 bytes of padding after n_ct */
#define KS_PA_PTR_(field, owner, count, share) + sizeof(void*)
#define KS_PA_RS_(field, n) + sizeof(ks_reqsets)
#ifdef __cplusplus
static_assert(sizeof(void*) != 8 || (0 KS_PROBLEM_ARRAYS(KS_PA_PTR_, KS_PA_RS_)) + KS_PROBLEM_SCALAR_BYTES == sizeof(ks_problem), "KS_PROBLEM_ARRAYS does not cover ks_problem");
#endif

#define KS_FLAG_SIMULATION 1u /* SchedulerOptions.SimulationMode (scheduler.go:37-40); informational */
#define KS_FLAG_STATS 2u      /* also count the reference algorithm's attempts / scanned types (DESIGN.md roofline) */
/* kernel choice PER PROBLEM (round 5; the environment variables KS_NO_RR / KS_ONE_WAVE / KS_NO_LEAN still switch the whole process for A/B runs): for a library
 * two goroutines share -- the provisioner's Solve and a deprovisioner's what-ifs -- a choice has to travel with the problem, not with the process */
#define KS_FLAG_NO_RR 4u      /* do not start ks_pack_rr: ks_pack takes the Solve from the start */
#define KS_FLAG_ONE_WAVE 8u   /* ks_pack's single-wave variant (what a batch runs per what-if) for a single Solve */
#define KS_FLAG_NO_LEAN 16u   /* the general variant on a problem the LEAN one would take */

/* Result of one Solve: caller allocates the arrays (sizes below), the library fills them. */
typedef struct ks_result {
  /* per pod */
  int32_t* pod_node;   /* [P] -1 unscheduled, [0,E) existing node, E+j new node j */
  int32_t* pod_stage;  /* [P] relaxation stage the pod ended at */
  int32_t* pod_seq;    /* [P] commit sequence number (orders Node.Pods), -1 if unscheduled */
  uint32_t* pod_reason; /* [P] 0 if scheduled; else why the LAST scheduler.add failed (scheduler.go:193-217 keeps one error per provisioner):
                           4 bits per machine template m (weight order, m < 8) at bit 4m -- KS_WHY_* -- so a shim can synthesise the
                           reference's "incompatible with provisioner ..., <reason>" messages for recordSchedulingResults (scheduler.go:135-172) */
  /* unscheduled pods in final queue order (q.List(), queue.go:70-72) */
  uint32_t n_unscheduled;
  int32_t* unscheduled; /* [P] */
  /* per new node (creation order) -- what callers read from scheduling.Node */
  uint32_t n_new;
  int32_t* node_tmpl;      /* [max_new_nodes] */
  uint64_t* node_types;    /* [max_new_nodes*TW] InstanceTypeOptions as a bitmask */
  int64_t* node_requests;  /* [max_new_nodes*R] */
  uint32_t* node_requests_present; /* [max_new_nodes] */
  uint32_t* node_present;  /* [max_new_nodes] Requirements after FinalizeScheduling (node.go:111-115) */
  uint32_t* node_complement;
  uint64_t* node_mask;     /* [max_new_nodes*K] */
  int32_t* node_gt;        /* [max_new_nodes*K] */
  int32_t* node_lt;        /* [max_new_nodes*K] */
  int32_t* node_it_state;  /* [max_new_nodes] */
  /* counters */
  uint64_t stats[32];      /* KS_STAT_*; [8..31] are per-phase cycle counters of the pack kernel (tools/phase_profile.py) */
} ks_result;

enum {      /* per-template failure reasons in ks_result.pod_reason */
  KS_WHY_NONE = 0,
  KS_WHY_LIMITS = 1,           /* "all available instance types exceed provisioner limits" (scheduler.go:198-201)              */
  KS_WHY_TAINTS = 2,           /* Taints.Tolerates (node.go:64)                                                                 */
  KS_WHY_HOST_PORTS = 3,       /* HostPortUsage.Validate (node.go:69); cannot happen on a fresh node, kept for completeness     */
  KS_WHY_REQUIREMENTS = 4,     /* nodeRequirements.Compatible(podRequirements) (node.go:77)                                     */
  KS_WHY_TOPOLOGY = 5,         /* Topology.AddRequirements: unsatisfiable topology constraint (node.go:83)                      */
  KS_WHY_TOPOLOGY_REQS = 6,    /* nodeRequirements.Compatible(topologyRequirements) (node.go:87)                                */
  KS_WHY_NO_INSTANCE_TYPE = 7  /* filterInstanceTypesByRequirements left nothing (node.go:94-98)                                 */
};

enum {
  KS_STAT_POPS = 0,        /* queue pops                                             */
  KS_STAT_RELAX = 1,       /* relaxations                                            */
  KS_STAT_FULLCHECKS = 2,  /* candidate nodes that reached the instance-type filter  */
  KS_STAT_FULLFAILS = 3,   /* ... and failed it                                      */
  KS_STAT_REF_ATTEMPTS = 4,/* Node.Add/ExistingNode.Add calls the reference would make (KS_FLAG_STATS) */
  KS_STAT_REF_TYPES = 5,   /* instance types the reference would scan (KS_FLAG_STATS)  */
  KS_STAT_CYCLES = 6,      /* s_memtime ticks spent in the pack kernel (block 0)       */
  KS_STAT_ERR = 7          /* device-side error code (0 ok)                            */
};

/* ---- device-resident problem: upload once, solve many times (inputs resident in HBM) ---- */
typedef struct ks_dev_problem ks_dev_problem;

int ks_device_count(void);                                     /* number of gfx950 devices visible, 0 if none */
int ks_current_device(void);                                   /* the calling thread's current HIP device (hipGetDevice), 0 if none */
int ks_problem_device(const ks_dev_problem* d);                /* device an uploaded problem lives on */
/* Which pack kernel took the last solve of `d`.  A single LEAN Solve is first offered to the register-resident kernel (ks_pack_rr), which DECLINES what it does not
 * cover -- before or during its run, leaving no trace in the result -- whereupon the general kernel (ks_pack) solves it.  *started: ks_pack_rr was launched;
 * *decline_code: 0 it took the Solve, else why it declined (the codes are listed in karpenter_core_amd/csrc/ks_pack_rr.inc; e.g. 1 static limits, 4 more nodes than it
 * holds, 8 its watchdog).  Diagnostics only: the result is the same either way (scheduler.go:96-219). */
int ks_problem_rr_status(const ks_dev_problem* d, int* started, int* decline_code);
/* Which ks_pack variant took the last solve of `d`, by its compile-time resource bound: 4 (LEAN), 8 (general), 16 (wide: a problem with R > 8, or a
 * what-if batch holding one); 0 if ks_pack_rr took it.  Diagnostics only, like ks_problem_rr_status. */
int ks_problem_pack_width(const ks_dev_problem* d, int* rm);
int ks_problem_pack_lean(const ks_dev_problem* d, int* lean);      /* its neighbour: 1 if the ks_pack variant the last solve ran was a LEAN one (at width 4, or 8 under ks_problem.lean_r8), else 0 */
int ks_problem_pack_row(const ks_dev_problem* d, int* row);        /* and which instantiation exactly: the index into the library's table of ks_pack instantiations (ks_debug_pack_row names its FAST, BOUNDS, LEAN, waves, RM) that the last solve of `d` -- alone or as a member of a batch -- launched; -1 if ks_pack_rr took it or nothing ran */
int ks_problem_upload(const ks_problem* p, int device, ks_dev_problem** out);
/* Diagnostics: row i of the library's table of ks_problem's arrays (KS_PROBLEM_ARRAYS; a ks_reqsets member appears as its six arrays, "cls.mask"): its name, the
 * bytes of an element, the elements `p` states for it (*count: from p's dimensions and offset arrays, whether or not the pointer is set) and the byte offset of its
 * pointer in ks_problem; *marks: KS_ARRAY_*.  Any out-pointer may be NULL; p may be NULL when count is.  Returns the number of rows (for every i; nothing is written
 * for an i at or beyond it).  Needs no device.  What lets a caller -- or a test -- walk a problem it did not build without a list of its own. */
#define KS_ARRAY_NOT_FINGERPRINTED 1u /* libkshost's fingerprint leaves the array out */
#define KS_ARRAY_NULLABLE 2u          /* the pointer may be NULL whatever the count (offering prices) */
uint32_t ks_debug_problem_array(const ks_problem* p, uint32_t i, const char** name, uint32_t* elem_bytes, uint64_t* count, uint32_t* offset, uint32_t* marks);
void ks_problem_free(ks_dev_problem* d);
/* Consolidation what-ifs over ONE cluster snapshot (deprovisioning/helpers.go:42-99) differ in their pods and in which state nodes stay, not in
 * the catalogue.  `base` is a resident problem flattened from the same snapshot (ks_problem_prepare'd): arrays of `p` whose HOST pointers are
 * the very arrays `base` was uploaded from (instance types, offerings, prices, the instance-type-key lattice) are not copied again, and the
 * tables derived from the catalogue are shared with it.  `base` must outlive the returned problem.  Anything not shared is uploaded as usual. */
int ks_problem_upload_shared(const ks_problem* p, const ks_dev_problem* base, ks_dev_problem** out);
/* ---- consolidation what-ifs derived ON THE DEVICE from a resident cluster snapshot (SURVEY 8b `ks_solve_batch(shared, whatif deltas, ...)`;
 * deprovisioning/helpers.go:48-61,81-84: a what-if = the snapshot minus its candidate nodes plus their pods).  `base` is the snapshot flattened
 * as ONE problem -- every node an existing node, every bound pod in the batch -- resident with its tables built.  A what-if is then nothing but
 * its candidate set: ks_whatifs_open lays out the state of all n what-ifs in one arena, uploads KBs (candidate masks, remainingResources,
 * descriptors) and builds every batch on the device (the snapshot's queue order restricted to the candidates' pods).  ks_whatifs_problems are
 * ordinary device problems (views owned by the batch) for ks_solve_batch_dev / ks_batch_records_dev / ks_price_filter_dev / ...; in their
 * results pod i is the i-th pod of the what-if in the SNAPSHOT's queue order (ks_whatifs_pod_ids names the snapshot pod behind each) and
 * existing node e is the snapshot's row e (removed nodes receive nothing).  Not for snapshots with volume limits (base ND > 0: see ks_whatifs_open_ex)
 * or more than 1024 topology groups (KS_ERR_UNSUPPORTED: the caller flattens those what-ifs one by one). */
typedef struct ks_whatif_batch ks_whatif_batch;
/* Snapshots whose bound pods carry spread / affinity / anti-affinity terms (base G > 0, G <= 1024): what a what-if's topology takes from its
 * candidate set is derived on the device too -- which groups exist from the start (owned by a pod of the batch: topology.go:72-78) and countDomains over
 * the cluster pods that stay (topology.go:231-276) -- from per-node tables of the snapshot: */
typedef struct ks_whatif_topo {
  const int32_t* node_cnt;    /* [G][n_nodes] pods on the node that group g counts when they are NOT in the batch (selector, namespace, node filter, key present);
                                              inverse anti-affinity groups (g >= n_topologies): the bound pods on the node that OWN the group (topology.go:181-199) */
  const int32_t* node_dom;    /* [G][n_nodes] the node's domain for group g: value id of its label on the group's key, -1 if none; hostname-keyed groups: the
                                              pods on the node the group counts that are in NO batch (they count under its hostname even when the node is a candidate) */
  const uint64_t* node_own;   /* [n_nodes][ceil(G/64)] groups (bit g) some pod bound to the node owns at its first relaxation stage.  An inverse group EXISTS in a
                                              what-if only while an owner is in the batch (this bit) or stays bound (a positive count); a value-keyed one that does not
                                              exist is marked for the pack kernel's evaluation to skip, a hostname-keyed one without counts constrains nothing */
  const int32_t* tot;         /* [G][64]      node_cnt summed per domain over every node */
  const int32_t* extra_tot;   /* [GH]         hostname-keyed groups: nodes that are no existing row and count > 0 */
  const int32_t* grph_base;   /* [GH][E]      hostname-keyed groups: what every existing row counts while its node stays; 0 = registered without pods,
                                              -2 = registered only in a group a pod of the batch owns from the start (existingnode.go:73), else unknown (-1) */
} ks_whatif_topo;
int ks_whatifs_open(const ks_dev_problem* base, uint32_t n_nodes, const int32_t* pod_node /* [base P] node of every snapshot pod */,
                    const int32_t* node_row /* [n_nodes] existing-node row in base, -1 if none */, uint32_t n, const uint32_t* cand_off /* [n+1] */,
                    const uint32_t* cand /* node indices */, const uint32_t* n_pods /* [n] pods bound to each candidate set */,
                    const int64_t* remaining /* [n][M][R] remainingResources without the candidates */,
                    const ks_whatif_topo* topo /* NULL for a snapshot without topology groups */, ks_whatif_batch** out);
/* The same with options.  KS_WHATIFS_VOLUMES accepts a snapshot with volume drivers (base ND > 0): every what-if gets per-node volume counts [E][ND] and
 * claim sets [E][SW] of its own, initialised from the snapshot's en_vol_count / en_vol_set when it is solved.  That is exact only for a snapshot whose
 * claim partition does not depend on the candidate set -- a claim that is a count (0x80000000 entry) in some pod's vol_list must be mounted by no other
 * snapshot pod and listed on no existing row but that pod's node; libkshost flattens snapshots so under KSH_DERIVE_VOLUMES (kshost.h).  ks_whatifs_open
 * keeps refusing such a snapshot. */
#define KS_WHATIFS_VOLUMES 1u
typedef struct ks_whatifs_options {
  const ks_whatif_topo* topo;   /* as ks_whatifs_open's `topo` */
  uint32_t flags;               /* KS_WHATIFS_* */
  uint32_t reserved;            /* 0 */
} ks_whatifs_options;
int ks_whatifs_open_ex(const ks_dev_problem* base, uint32_t n_nodes, const int32_t* pod_node, const int32_t* node_row, uint32_t n, const uint32_t* cand_off,
                       const uint32_t* cand, const uint32_t* n_pods, const int64_t* remaining, const ks_whatifs_options* opt, ks_whatif_batch** out);
/* The same per-node facts as LISTS (libkshost: KSH_DERIVE_GROUP_LISTS): a CSR by node with one entry per (node, group) pair that matters -- a pod on the node
 * that the group counts, or that owns it -- instead of the two dense [G][n_nodes] tables and the [n_nodes][ceil(G/64)] owner words.  Any number of groups
 * (the 1024 of ks_whatif_topo came from the dense kernel's shape: one thread per group in one block); what is copied per open grows with the entries, not with G * n_nodes.
 * Entry k of node n, node_off[n] <= k < node_off[n + 1], ascending in g: */
typedef struct ks_whatif_topo_lists {
  const uint32_t* node_off;   /* [n_nodes + 1] ascending; node_off[n_nodes] = n_entries */
  const uint32_t* ent_g;      /* [n_entries]  the group id; bit 31 (KS_TOPO_ENT_OWN): some pod bound to the node owns the group (ks_whatif_topo::node_own's bit) */
  const int32_t* ent_cnt;     /* [n_entries]  ks_whatif_topo::node_cnt[g][n] */
  const int32_t* ent_dom;     /* [n_entries]  ks_whatif_topo::node_dom[g][n]: the domain's value id in [0, 64) wherever ent_cnt != 0, or -1; hostname-keyed groups: the stay count */
  uint64_t n_entries;
  const int32_t* tot;         /* [G][64]      as ks_whatif_topo */
  const int32_t* extra_tot;   /* [GH]         as ks_whatif_topo */
  const int32_t* grph_base;   /* [GH][E]      as ks_whatif_topo */
} ks_whatif_topo_lists;
#define KS_TOPO_ENT_OWN 0x80000000u
/* ks_whatifs_open_ex with the topology given as lists (`flags`: KS_WHATIFS_*).  The lists are checked before anything is launched (offsets, group ids, domains):
 * KS_ERR_INVALID.  The what-ifs it opens are what ks_whatifs_open / _ex open from the dense tables of the same snapshot, cell by cell (ks_debug_whatif_topology). */
int ks_whatifs_open_lists(const ks_dev_problem* base, uint32_t n_nodes, const int32_t* pod_node, const int32_t* node_row, uint32_t n, const uint32_t* cand_off,
                          const uint32_t* cand, const uint32_t* n_pods, const int64_t* remaining, const ks_whatif_topo_lists* lists, uint32_t flags, ks_whatif_batch** out);
/* Diagnostics: what the derivation left a derived what-if with -- grp_active [G], grp_count [G][64], grph_extra_pos [GH] (any of them NULL: not copied).  Read-only,
 * launches nothing; KS_ERR_INVALID for a problem that is no derived what-if over a snapshot with topology groups. */
int ks_debug_whatif_topology(ks_dev_problem* d, uint8_t* out_active, int32_t* out_count, int32_t* out_extra);
ks_dev_problem* const* ks_whatifs_problems(ks_whatif_batch* b);
uint64_t ks_whatifs_arena_bytes(const ks_whatif_batch* b);          /* device bytes of the batch's arena (diagnostics: tools/time_whatif_volumes.py) */
uint64_t ks_whatifs_upload_bytes(const ks_whatif_batch* b);         /* of those, the bytes the open copied from the host (one host-to-device copy): masks, descriptors, the per-node topology tables or lists */
uint32_t ks_whatifs_count(const ks_whatif_batch* b);
int ks_whatifs_pod_ids(ks_whatif_batch* b, uint32_t i, uint32_t* out /* [n_pods of what-if i] snapshot pod ids, what-if pod order */);
void ks_whatifs_free(ks_whatif_batch* b);
int ks_problem_prepare(ks_dev_problem* d);                     /* build the static tables + feasibility grid now (otherwise the first solve does) */
/* Solve on the uploaded problem; kernel time (ms, HIP events on the solve stream) is returned in *kernel_ms if non-NULL. */
int ks_solve_dev(ks_dev_problem* d, ks_result* out, float* kernel_ms);
/* Convenience: upload + solve + free. */
int ks_solve(const ks_problem* p, ks_result* out);
/* N independent problems (consolidation what-ifs): one workgroup each, one launch. */
/* out == NULL: the results stay on the device (only the error words are read back) for ks_batch_records_dev / ks_price_filter_dev / ... */
int ks_solve_batch_dev(ks_dev_problem* const* d, uint32_t n, ks_result* const* out, float* kernel_ms);
/* The fixed-size records a what-if fan-out exchanges (deprovisioning: what consolidation reads of a simulation, consolidation.go:190-260;
 * multinodeconsolidation.go:74-114 probes many candidate sets), built on the device from the results the last ks_solve*_dev left there, into a
 * caller-owned DEVICE buffer d_out[n][3 + words] of uint64: [ids[i], n_new, n_unscheduled, new node 0's InstanceTypeOptions (zero if none)].
 * The buffer is complete when the call returns -- it can be handed to RCCL as is (no host hop). */
int ks_batch_records_dev(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, uint32_t words, void* d_out);
/* ---- the what-if fan-out over several GPUs in ONE call (SURVEY 8b `ks_solve_batch(shared, whatifs, n, out, ngpus)`; deprovisioning/helpers.go:42-115 per what-if,
 * multinodeconsolidation.go:74-114 / singlenodeconsolidation.go:54-78 are the callers that would batch them).  The what-ifs are resident as shards, one list of device
 * problems per GPU (every problem of a shard on the same device: ks_whatifs_open over that GPU's copy of the snapshot, or ks_problem_upload).  Every shard is solved in one
 * batched launch on its own device and stream, concurrently (a thread per shard); the fixed-size decision records -- [id, n_new, n_unscheduled, new node 0's
 * InstanceTypeOptions (words)] -- are built on each device and gathered into out_rows[sum shard_n][3 + words], ordered by id.  kernel_ms_max: the slowest shard's launch.
 * ks_deal_lpt decides which shard a what-if goes to from a predicted weight (e.g. its pods): longest first, each to the least loaded shard. */
void ks_deal_lpt(const uint64_t* weight, uint32_t n, uint32_t nshards, uint32_t* shard_of);
int ks_solve_batch_sharded(ks_dev_problem* const* const* shards, const uint32_t* shard_n, const uint64_t* const* shard_ids, uint32_t nshards, uint32_t words,
                           uint64_t* out_rows, float* kernel_ms_max);
int ks_solve_batch(const ks_problem* const* p, uint32_t n, ks_result* const* out);

/* The static pod-class x instance-type feasibility grid for fresh nodes of every template:
 * out_grid[(m*C + c)*TW + w].  Exposed for parity tests and roofline measurement. */
int ks_feasibility_grid(ks_dev_problem* d, uint64_t* out_grid, float* kernel_ms);
/* Diagnostics: the M * C * TW words of the grid as the last build left it -- ks_feasibility_grid rebuilds before it copies, so the grid a batch built
 * (ks_solve_batch_dev) shows only here.  Read-only, launches nothing; KS_ERR_INVALID while the grid has not been built (or installed completely). */
int ks_debug_grid(ks_dev_problem* d, uint64_t* out_grid);
/* SURVEY 8e row 2 -- the static grid's rows split over GPUs (node.go:137-159 for a fresh node of template m and a pod of class c is row m * C + c, ceil(T/64) words):
 * ks_feasibility_grid_rows computes rows [row_lo, row_hi) on this device (every other static table in full) and copies them to host memory (out_rows) and / or into
 * device memory of the caller's (out_rows_dev: e.g. its slice of the buffer ONE all-gather fills); ks_feasibility_grid_install puts rows computed elsewhere in place
 * (from host or device memory; complete != 0: every row is in, the problem solves without building its grid again). */
int ks_feasibility_grid_rows(ks_dev_problem* d, uint32_t row_lo, uint32_t row_hi, uint64_t* out_rows, void* out_rows_dev, float* kernel_ms);
int ks_feasibility_grid_install(ks_dev_problem* d, uint32_t row_lo, uint32_t row_hi, const uint64_t* rows, const void* rows_dev, int complete);

/* Consolidation price stage on results that are still on the device (deprovisioning/helpers.go:148-157 filterByPrice over
 * :292-315 worstLaunchPrice; callers consolidation.go:238 and multinodeconsolidation.go:164): for problem i, of new node
 * node[i]'s InstanceTypeOptions (as left by the last ks_solve*_dev of ds[i]) keep the types whose worst launch price under
 * that node's zone / capacity-type requirements is < max_price[i].  out_types[i] receives ceil(T/64) words, out_counts[i]
 * the number of types kept.  spot_only[i] != 0 prices node i as if its capacity-type requirement had already been narrowed
 * to In [spot] (computeConsolidation does that before multi-node consolidation filters again, consolidation.go:262-265);
 * spot_only may be NULL.  One launch for the whole batch. */
int ks_price_filter_dev(ks_dev_problem* const* ds, uint32_t n, const uint32_t* node, const double* max_price,
                        const uint32_t* spot_only, uint64_t* const* out_types, uint32_t* out_counts);

/* ---- consolidation commands, decided on the device (deprovisioning/consolidation.go:190-274 computeConsolidation; multinodeconsolidation.go:132-165
 * filterOutSameType): for problem i, over the result the last ks_solve*_dev of ds[i] left on the device, ONE fixed-size row of uint64 in a caller-owned DEVICE
 * buffer d_out[n][KS_CMD_ROW_WORDS(words)] -- like ks_batch_records_dev's it can be handed to an all-gather without a host hop.  One launch for the batch (one wave
 * per what-if), on ds[0]'s stream; the buffer is complete when the call returns.  Every word of every row is written (words beyond a problem's ceil(T/64) are zero).
 *
 * The steps, in the reference's order: (1) blocked or n_unscheduled > 0 -> do-nothing; (2) n_new == 0 -> delete; (3) n_new != 1 -> do-nothing; (4) price error ->
 * error; (5) filterByPrice of new node 0's InstanceTypeOptions under its zone / capacity-type requirements against cand_price -- the arithmetic of
 * ks_price_filter_dev --; (6) nothing kept -> do-nothing; (7) all candidates spot and the capacity-type requirement Has(spot) -> do-nothing; (8) capacity type
 * Has(spot) and Has(on-demand) -> the command is narrowed to spot (:262-265); (9) with KS_CMD_F_SAME_TYPE, filterOutSameType: max_price = the lowest listed price
 * among the listed types that step 5 kept (MaxFloat64 if none is), the kept options priced again -- as spot only if step 8 narrowed -- against it; nothing left ->
 * do-nothing.  Prices are only compared on the device: getNodePrices' sum is made by the caller, in candidate order (float64 addition does not commute with a
 * reduction tree), and arrives as cand_price. */
#define KS_CMD_F_BLOCKED 1u      /* an owned, in-state node that is not initialised stays in the cluster: simulateScheduling reports "not all pods scheduled" (helpers.go:102-113) */
#define KS_CMD_F_ALL_SPOT 2u     /* every candidate's capacity type is spot (consolidation.go:250) */
#define KS_CMD_F_PRICE_ERROR 4u  /* getNodePrices failed for a candidate (consolidation.go:224-228, 277-287) */
#define KS_CMD_F_SAME_TYPE 8u    /* also run filterOutSameType (what firstNNodeConsolidationOption does with a replace, multinodeconsolidation.go:97-106) */
#define KS_CMD_F_ALL 15u
typedef struct ks_command_inputs {
  const uint32_t* flags;      /* [n]   KS_CMD_F_*; any other bit: KS_ERR_INVALID */
  const double* cand_price;   /* [n]   getNodePrices of the candidate set (ignored under KS_CMD_F_PRICE_ERROR) */
  const uint32_t* type_off;   /* [n+1] CSR into type_idx / type_price: one entry per DISTINCT instance type among what-if i's candidates (read under KS_CMD_F_SAME_TYPE) */
  const uint32_t* type_idx;   /*       instance-type index (< T) */
  const double* type_price;   /*       the lowest Offerings.Get price among the candidates of that type; 0.0 if none of them has an offering: the Go map miss of
                                       multinodeconsolidation.go:150-158 */
} ks_command_inputs;
/* the row: words of uint64 */
#define KS_CMD_ID 0                  /* ids[i] */
#define KS_CMD_DECISION 1            /* action | reason << 8 | narrowed << 16.  narrowed: step 8 replaced the capacity-type requirement by In [spot]; the requirement
                                        words below carry that.  (In a catalogue with no capacity type called spot the value has no bit: the mask is then empty
                                        and this flag alone says In [spot].)  Under KS_CMD_F_SAME_TYPE a row whose step 9 kept nothing reads do-nothing / KS_CMD_WHY_SAME_TYPE and
                                        KEEPS this bit and the narrowed requirement words: they describe the replace step 9 turned down. */
#define KS_CMD_N_NEW 2
#define KS_CMD_N_UNSCHEDULED 3
#define KS_CMD_N_OPTIONS 4           /* types step 5 kept */
#define KS_CMD_N_OPTIONS_SAME_TYPE 5 /* types step 9 kept (0 without KS_CMD_F_SAME_TYPE) */
#define KS_CMD_PRESENT 6             /* new node 0's Requirements (zero if there is none), after step 8's narrowing: present | complement << 32 */
#define KS_CMD_IT_STATE 7            /* ... its instance-type key state (ks_result.node_it_state) */
#define KS_CMD_MASK 8                /* ... [KS_MAX_KEYS] value masks, key k at KS_CMD_MASK + k (zero for k >= K) */
#define KS_CMD_BOUNDS 40             /* ... [KS_MAX_KEYS] (uint32_t)gt | (uint64_t)(uint32_t)lt << 32 */
#define KS_CMD_OPTIONS 72            /* [words] what step 5 kept: a plain computeConsolidation caller's replacement InstanceTypeOptions; then [words] what step 9 kept:
                                        what firstNNodeConsolidationOption launches.  Both zero where the step did not run. */
#define KS_CMD_ROW_WORDS(words) (KS_CMD_OPTIONS + 2 * (size_t)(words))
/* action (KS_CMD_DECISION & 0xff).  Under KS_CMD_F_SAME_TYPE the action is firstNNodeConsolidationOption's: a replace whose step 9 kept nothing reads do-nothing
 * with KS_CMD_WHY_SAME_TYPE, and step 5's options stay in the row. */
#define KS_CMD_DO_NOTHING 0
#define KS_CMD_DELETE 1
#define KS_CMD_REPLACE 2
#define KS_CMD_ERROR 3
/* reason ((KS_CMD_DECISION >> 8) & 0xff): the step that said do-nothing / error; 0 for delete and replace */
#define KS_CMD_WHY_NOT_ALL_SCHEDULED 1 /* step 1 */
#define KS_CMD_WHY_MANY_NODES 3        /* step 3 */
#define KS_CMD_WHY_PRICE_ERROR 4       /* step 4 (action error) */
#define KS_CMD_WHY_NOT_CHEAPER 6       /* step 6 */
#define KS_CMD_WHY_SPOT_TO_SPOT 7      /* step 7 */
#define KS_CMD_WHY_SAME_TYPE 9         /* step 9 left nothing */
#define KS_CMD_WHY_DELETING 10         /* written by libkshost, never by the kernel: a candidate is itself being deleted (action error, helpers.go:62-67) */
/* Refusals (KS_ERR_INVALID, nothing launched): a batch over two devices, a problem without prices or without zone / capacity-type keys, words < ceil(T/64),
 * type_off not ascending, a type index >= T, an unknown flag bit. */
int ks_consolidation_commands_dev(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, const ks_command_inputs* in, uint32_t words, void* d_out);
/* The same with the rows brought to HOST memory out_rows[n][KS_CMD_ROW_WORDS(words)] (one launch, one device-to-host copy); ms (may be NULL): [0] inputs up + launch +
 * completion, [1] the read-back, milliseconds.  The inputs are validated once, before any device work. */
int ks_consolidation_commands_host(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, const ks_command_inputs* in, uint32_t words, uint64_t* out_rows, double* ms);

/* ---- consolidation commands VALIDATED on the device (deprovisioning/validation.go:118-171 Validation.ValidateCommand after mapNodes and simulateScheduling): for
 * command i, over the result the last ks_solve*_dev of ds[i] -- the re-simulation of the command's nodes that are still candidates -- left on the device, ONE
 * fixed-size row of uint64 in a caller-owned DEVICE buffer d_out[n][KS_VAL_ROW_WORDS(words)].  ks_consolidation_commands_dev's sibling: one launch for the batch (one
 * wave per command), on ds[0]'s stream; the buffer is complete when the call returns; every word of every row is written (words beyond a problem's ceil(T/64) are zero).
 * The steps, in the reference's order, the first that applies decides: blocked or n_unscheduled > 0 -> invalid (4); n_new == 0 -> valid unless a replacement was
 * expected (5); n_new > 1 -> invalid (6); one new node but none expected -> invalid (7); instanceTypesAreSubset(the command's options, new node 0's options now) fails
 * -> invalid (8); else valid.  options[i] is read only under KS_VAL_F_EXPECT_REPLACEMENT (len(cmd.replacementNodes) != 0); its bits are instance-type indices of
 * ds[i]'s catalogue. */
#define KS_VAL_F_BLOCKED 1u              /* an owned, in-state node that is not initialised stays in the cluster (helpers.go:102-113), as KS_CMD_F_BLOCKED */
#define KS_VAL_F_EXPECT_REPLACEMENT 2u   /* the command carries a replacement node */
#define KS_VAL_F_ALL 3u
typedef struct ks_validate_inputs {
  const uint32_t* flags;      /* [n] KS_VAL_F_*; any other bit: KS_ERR_INVALID */
  const uint32_t* n_mapped;   /* [n] how many of the command's nodes were simulated (echoed into the row) */
  const uint64_t* options;    /* [n][words] the command's replacement InstanceTypeOptions; may be NULL when no command expects a replacement */
} ks_validate_inputs;
/* the row: words of uint64 */
#define KS_VAL_ID 0                  /* ids[i] */
#define KS_VAL_VERDICT 1             /* verdict | why << 8 */
#define KS_VAL_N_NEW 2
#define KS_VAL_N_UNSCHEDULED 3
#define KS_VAL_N_MAPPED 4            /* nodes of the command that were simulated (host-supplied, echoed) */
#define KS_VAL_N_OPTIONS 5           /* popcount of new node 0's options now (0 if there is no new node) */
#define KS_VAL_N_MISSING 6           /* popcount(command options & ~options now); 0 unless the subset test ran */
                                     /* word 7: reserved, zero */
#define KS_VAL_OPTIONS 8             /* [words] new node 0's InstanceTypeOptions now; then [words] the command's types the re-simulation no longer offers */
#define KS_VAL_ROW_WORDS(words) (KS_VAL_OPTIONS + 2 * (size_t)(words))
/* verdict (KS_VAL_VERDICT & 0xff) */
#define KS_VAL_INVALID 0
#define KS_VAL_VALID 1
#define KS_VAL_ERROR 2               /* ValidateCommand returned an error, not a verdict (written by libkshost only) */
/* why ((KS_VAL_VERDICT >> 8) & 0xff): the reference's step that decided.  1-3 are written by libkshost and never simulated; 0 and 4-8 by the kernel. */
#define KS_VAL_WHY_VALID 0
#define KS_VAL_WHY_NOMINATED 1          /* a node of the command is nominated (validation.go:87-91) */
#define KS_VAL_WHY_NO_CANDIDATES 2      /* no node of the command is still a candidate (:114) */
#define KS_VAL_WHY_DELETING 3           /* a mapped node is itself being deleted: verdict KS_VAL_ERROR (helpers.go:62-67) */
#define KS_VAL_WHY_NOT_ALL_SCHEDULED 4  /* :122, KS_VAL_F_BLOCKED included */
#define KS_VAL_WHY_NO_NEW_NODE 5        /* no new node but a replacement was expected (:139) */
#define KS_VAL_WHY_MANY_NODES 6         /* more than one new node (:143) */
#define KS_VAL_WHY_UNEXPECTED_NODE 7    /* one new node but the command is a delete (:148) */
#define KS_VAL_WHY_NOT_A_SUBSET 8       /* the command's options are not a subset of the re-simulation's (:164) */
/* Refusals (KS_ERR_INVALID, nothing launched): a null array, a batch over two devices, words < ceil(T/64), an unknown flag bit, a listed type index >= T. */
int ks_validate_commands_dev(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, const ks_validate_inputs* in, uint32_t words, void* d_out);
/* The same with the rows brought to HOST memory out_rows[n][KS_VAL_ROW_WORDS(words)] (one launch, one device-to-host copy); ms (may be NULL): [0] inputs up + launch +
 * completion, [1] the read-back, milliseconds. */
int ks_validate_commands_host(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, const ks_validate_inputs* in, uint32_t words, uint64_t* out_rows, double* ms);

/* ---- replacement commands with m -> n rows, decided on the device (deprovisioning/expiration.go:75-111, drift.go:64-96: Expiration / Drift.ComputeCommand after the
 * candidate has passed canBeTerminated): for problem i, over the result the last ks_solve*_dev of ds[i] left on the device, ONE head of KS_REP_HEAD_WORDS uint64 in
 * d_heads[n][KS_REP_HEAD_WORDS] and n_nodes rows of KS_REP_NODE_WORDS(words) uint64 in d_nodes[cap_nodes][...], both caller-owned DEVICE buffers of one width each (either
 * can go through one all-gather).  Two launches on ds[0]'s stream (ks_replacement_heads: one workgroup, the decisions and an exclusive scan for node_off, no atomics;
 * ks_replacement_nodes: one wave per what-if); both buffers are complete when the call returns.
 * The decision: KS_REP_F_BLOCKED -> delete with KS_REP_BLOCKED set and n_nodes 0 (simulateScheduling returns `nil, false, nil` when an owned, in-state node that stays is
 * not initialised, helpers.go:106-113, and ComputeCommand reads len(newNodes) only); n_new == 0 -> delete; else replace with all n_new nodes.  n_unscheduled never
 * changes the action (the reference only logs it).  No price stage, no narrowing.
 * Capacity: *out_total_nodes = the sum of n_nodes.  Beyond cap_nodes every head is still complete; node rows are written for the what-ifs whose rows fit entirely below
 * cap_nodes, the others carry KS_REP_TRUNCATED; no row at or beyond cap_nodes is touched; the call returns KS_OK and the caller calls again with a larger table.
 * cap_nodes = 0 with a NULL node table is the sizing call.
 * Refusals (KS_ERR_INVALID, nothing launched): a null array, a batch over two devices, words < ceil(T/64), K > KS_MAX_KEYS, R > KS_MAX_RES, an unknown flag bit. */
#define KS_REP_F_BLOCKED 1u          /* input flag: as KS_CMD_F_BLOCKED */
#define KS_REP_HEAD_WORDS 8
#define KS_REP_ID 0                  /* ids[i] */
#define KS_REP_DECISION 1            /* action (KS_CMD_DO_NOTHING / _DELETE / _REPLACE / _ERROR) | why << 8 (KS_CMD_WHY_DELETING, written by libkshost only) | flags << 16 */
#define KS_REP_N_NEW 2               /* as the simulation counted it */
#define KS_REP_N_UNSCHEDULED 3
#define KS_REP_N_NODES 4             /* the command's replacement count: 0 for a delete, a blocked set and an error */
#define KS_REP_NODE_OFF 5            /* index of its first row in the node table */
#define KS_REP_N_OPTIONS 6           /* the sum over its nodes of popcount(options) */
                                     /* word 7: reserved, zero */
#define KS_REP_BLOCKED 1u            /* flags (KS_REP_DECISION >> 16) */
#define KS_REP_TRUNCATED 2u
/* the node row: words of uint64 */
#define KS_REP_NODE_ID 0             /* (uint32) what-if id | node index << 32: what-if order, then new-node order */
#define KS_REP_NODE_PRESENT 1        /* the node's Requirements: present | complement << 32 */
#define KS_REP_NODE_IT_STATE 2
#define KS_REP_NODE_N_OPTIONS 3      /* popcount of its InstanceTypeOptions */
#define KS_REP_NODE_REQMASK 4        /* bit r: resource r is in the node's Requests */
#define KS_REP_NODE_MASK 5           /* [KS_MAX_KEYS] value masks, layout and meaning of KS_CMD_MASK */
#define KS_REP_NODE_BOUNDS 37        /* [KS_MAX_KEYS] as KS_CMD_BOUNDS */
#define KS_REP_NODE_REQ 69           /* [KS_MAX_RES] the node's resource requests (int64 milli-units, zero beyond R): what ToMachine needs */
#define KS_REP_NODE_OPTIONS 85       /* [words] InstanceTypeOptions */
#define KS_REP_NODE_WORDS(words) (KS_REP_NODE_OPTIONS + (size_t)(words))
int ks_replacement_commands_dev(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, const uint32_t* flags /* [n] KS_REP_F_* */, uint32_t words, void* d_heads, void* d_nodes,
                                uint64_t cap_nodes, uint64_t* out_total_nodes);
/* The same with both tables brought to HOST memory; of out_nodes only the rows that were written are touched.  ms (may be NULL): [0] inputs up + launches + completion,
 * [1] the read-back, milliseconds. */
int ks_replacement_commands_host(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, const uint32_t* flags, uint32_t words, uint64_t* out_heads, uint64_t* out_nodes,
                                 uint64_t cap_nodes, uint64_t* out_total_nodes, double* ms);

/* ---- placement rows: the PER-POD half of a result, as fixed-size rows (provisioner.go:352-357 NominatePod over Node.Pods, preferences.go:36-56 the relaxation a shim
 * applies back to pod.Spec, scheduler.go:135-172 the failed-scheduling events, ExistingNode.Pods).  For problem i, over the result the last ks_solve*_dev of ds[i] left
 * on the device -- a what-if derived on the device or an ordinary problem alike --, ONE head of KS_PLC_HEAD_WORDS uint64 in d_heads[n][KS_PLC_HEAD_WORDS] and P rows of
 * KS_PLC_ROW_WORDS uint64 in d_rows[cap_rows][KS_PLC_ROW_WORDS], one per pod of the batch in QUEUE order (queue.go:35 NewQueue's), found through the head's
 * KS_PLC_ROW_OFF; both caller-owned DEVICE buffers of one width each.  Two launches on ds[0]'s stream (ks_placement_heads: one workgroup, an exclusive scan of P for
 * row_off, no atomics -- ks_replacement_heads' way; ks_placement_rows: every problem's rows in one launch, lanes stride over a problem's pods); both buffers are
 * complete when the call returns.  A row is 32 bytes, 32-byte aligned, written by one lane as two aligned 16-byte stores (five 32-bit fields do not fit the widest
 * store there is); the pod it names is the pod's index in the problem it was flattened from -- for a derived what-if the SNAPSHOT's pod index (pod_gid), not the
 * position in the batch.  Ascending commit numbers within a node are Node.Pods' order (KS_PLC_SEQ is ks_result.pod_seq).
 * Capacity, the KS_REP_* convention: *out_total_rows = the sum of P.  Beyond cap_rows every head is still complete; rows are written for the problems whose rows fit
 * entirely below cap_rows, the others carry KS_PLC_TRUNCATED; nothing at or beyond cap_rows is touched; the call returns KS_OK.  cap_rows = 0 with a NULL table is
 * the sizing call.
 * Refusals (KS_ERR_INVALID, nothing launched): a null array, a batch over two devices, a problem that was never solved (or whose last solve failed). */
#define KS_PLC_HEAD_WORDS 8
#define KS_PLC_ID 0                  /* ids[i] */
#define KS_PLC_P 1                   /* pods of the batch = its rows */
#define KS_PLC_N_NEW 2
#define KS_PLC_N_UNSCHEDULED 3
#define KS_PLC_ROW_OFF 4             /* index of its first row in the row table */
#define KS_PLC_FLAGS 5               /* KS_PLC_TRUNCATED */
#define KS_PLC_N_EXISTING 6          /* E: KS_PLC_WHERE values below it name existing nodes, E + j new node j */
                                     /* word 7: reserved, zero */
#define KS_PLC_TRUNCATED 1u
/* the row: words of uint64, two 32-bit fields each */
#define KS_PLC_ROW_WORDS 4
#define KS_PLC_POD_WHERE 0           /* low: the pod's index | high: (int32) -1 unscheduled, existing node e, or E + new node j */
#define KS_PLC_STAGE_SEQ 1           /* low: (int32) the relaxation stage the pod ended at | high: (int32) its commit number, -1 if unscheduled */
#define KS_PLC_REASON_ID 2           /* low: ks_result.pod_reason (KS_WHY_* per machine template) | high: (uint32) ids[i] */
#define KS_PLC_POSITION 3            /* the pod's position in its problem's queue */
int ks_placement_rows_dev(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, void* d_heads, void* d_rows, uint64_t cap_rows, uint64_t* out_total_rows);
/* The same with both tables brought to HOST memory; of out_rows only the rows that were written are touched.  ms (may be NULL): [0] inputs up + launches + completion,
 * [1] the read-back, milliseconds. */
int ks_placement_rows_host(ks_dev_problem* const* ds, uint32_t n, const uint64_t* ids, uint64_t* out_heads, uint64_t* out_rows, uint64_t cap_rows, uint64_t* out_total_rows, double* ms);

/* ---- the AUDIT of a result against the problem it answers -- not against a second run of the algorithm.  Every placement, every new node's Requests and every new
 * node's InstanceTypeOptions are checked on the device, over the result where it lies, in time that does not matter next to the Solve; it works at any size, and for
 * what-ifs derived on the device.  A finding means: do not act on this result.  Each check is a bit; each bit is an invariant of the reference's algorithm that
 * holds in the FINAL state, whatever order the pods were placed in.  Throughout, a pod's class is the one of the stage it ended at,
 * stage_cls[pod_stage_off[p] + pod_stage[p]].
 * Pod bits (ks_audit.pod_flags[p]): */
#define KS_AUDIT_POD_RANGE 1u             /* pod_node outside [-1, E + n_new) (a derived what-if: or an existing node that left), pod_stage outside the pod's stages, pod_seq negative for a placed pod or != -1 for an unscheduled one */
#define KS_AUDIT_POD_UNSCHEDULED_LIST 2u  /* a pod with pod_node == -1 is not exactly once in unscheduled[0, n_unscheduled), or a placed pod is in it */
#define KS_AUDIT_POD_TAINTS 4u            /* (the node's taints & ~cls_tolerated) != 0 (taints.go:28-40) */
#define KS_AUDIT_POD_REQUIREMENTS 8u      /* existing node: Compatible(en, cls) fails or its_fail[en.it_state * SC + cls.it_state]; new node: Intersects(the node's final requirements, cls) fails on a narrow key, or the same lattice test with node_it_state.  ks_algebra.h's functions, not a restatement */
#define KS_AUDIT_POD_HOSTNAME 16u         /* cls_hn_mode against the node: In [list] on a node outside the list, NotIn [list] on a node inside it; a new node is in no list */
#define KS_AUDIT_POD_PORTS 32u            /* an entry of the class matches a reservation of the existing node, or an entry of another pod on the same node (hostportusage.go:45-57); both pods are flagged */
#define KS_AUDIT_POD_VOLUME_ERROR 64u     /* a class with the 0xFFFFFFFF volume entry sits on an existing node */
/* Node bits (ks_audit.node_flags[n]: existing node n < E, else new node n - E).  A node nothing was placed on is not examined beyond KS_AUDIT_NODE_EMPTY: no test of
 * the reference ever ran against it, so an existing node whose own daemon requests exceed what is available is as the caller gave it, not a finding. */
#define KS_AUDIT_NODE_RESOURCES 1u        /* existing node: en_requests plus the sum of its new pods' cls_requests does not Fit en_avail under resources.Fits' presence rule (existingnode.go:98-102) */
#define KS_AUDIT_NODE_VOLUMES 2u          /* existing node: for some driver a pod placed there mounts, the distinct claims after those pods (en_vol_set, en_vol_count, the classes' vol_list) exceed en_vol_limit */
#define KS_AUDIT_NODE_EMPTY 4u            /* a new node has no pod (nothing else of it is examined) */
#define KS_AUDIT_NODE_TEMPLATE 8u         /* node_tmpl outside [0, M) (nothing else of it is examined) */
#define KS_AUDIT_NODE_REQUESTS 16u        /* node_requests / node_requests_present is not exactly tmpl_daemon[m] merged with the sum of its pods' requests; int64, no tolerance */
#define KS_AUDIT_NODE_OPTIONS_EMPTY 32u   /* the node has no option */
#define KS_AUDIT_NODE_OPTIONS_EXTRA 64u   /* a set bit names a type outside T, outside tmpl_types[m], outside its_types[node_it_state], or one that fails compatible && fits && hasOffering (node.go:137-159) against the node's final requirements and requests */
#define KS_AUDIT_NODE_OPTIONS_MISSING 128u /* only for templates with tmpl_limit_present == 0xFFFFFFFF: a type that passes all of that is not set.  The filter is monotone -- requirements only narrow, requests only grow -- so the incremental filtering of node.go:94 equals one filtering by the final state; a limited template starts from an order-dependent subset (scheduler.go:199-208) and gets OPTIONS_EXTRA only */
/* NOT audited by this pass: anything about topology -- skew and affinity hold at the moment of placement, not at the end.  The part of them that the final state
 * decides together with the commit numbers is the second, opt-in pass below (ks_audit_topology_dev: pod (anti-)affinity, hostname spread).  Audited by neither:
 * spread over narrow keys, hostname spread under a node filter, self-selecting affinity, groups created by a later Topology.Update, provisioner limits (subtractMax
 * depends on the order), first-fit optimality (whether an earlier node would have taken the pod).  (Spread over narrow keys, unfiltered, is now the third pass's:
 * ks_audit_spread_dev; first-fit order, for the pods no topology group constrains, the fourth pass's: ks_audit_firstfit_dev; provisioner limits, bounded from
 * both sides in opening order, the fifth pass's: ks_audit_limits_dev -- KS_AUDIT_NODE_LIMIT_MISSING there is OPTIONS_MISSING for limited templates; first-fit
 * order for pods under hostname anti-affinity and unfiltered hostname spread, the sixth pass's: ks_audit_hostfit_dev.)
 * The caller owns the tables: pod_flags [P] and node_flags [E + max_new_nodes] (of which E + n_new are written), either may be NULL (totals only).  Flags are written
 * per index -- no list is appended through an atomic -- so the output is the same every run. */
typedef struct ks_audit {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_*, or NULL */
  uint32_t* node_flags;           /* [E + max_new_nodes] KS_AUDIT_NODE_*; entries [0, n_nodes) are written; or NULL */
  uint32_t n_pods, n_nodes;       /* out: P | E + n_new */
  uint32_t n_new, n_unscheduled;  /* out: the counts of the result that was audited */
  uint32_t n_pods_flagged, n_nodes_flagged;
  uint32_t pod_bit_count[32], node_bit_count[32];   /* out: pods / nodes carrying bit i */
  double kernel_ms, readback_ms;  /* out: inputs up + the launches + completion | the flags' way back and the totals (a batch: the batch's, in every member) */
} ks_audit;
/* claimed == NULL: the result the last ks_solve*_dev of `d` left on the device is audited where it lies -- the form for derived what-ifs.  claimed given: the caller's
 * arrays (ks_result's sizes; pod_reason and stats are not read) are uploaded and audited instead; for flattened problems only (KS_ERR_UNSUPPORTED for a derived view) --
 * how a shim audits a result it got from anywhere.  ks_audit_batch_dev: the resident form for a whole batch as one launch sequence (four launches on ds[0]'s stream).
 * Refusals (nothing launched): KS_ERR_INVALID for a NULL argument or table, a problem with nothing solved (resident form), a claimed n_new > max_new_nodes or
 * n_unscheduled > P, a batch over two devices. */
int ks_audit_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL */, ks_audit* out);
int ks_audit_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit* const* outs);
int ks_audit_sizes(const ks_dev_problem* d, uint32_t* n_pods /* P */, uint32_t* n_node_slots /* E + max_new_nodes */);   /* what the two tables of `d` must hold (a derived what-if has no ks_problem to read them from); either may be NULL */

/* ---- the audit's SECOND pass, opt-in: pod (anti-)affinity and hostname spread in COMMIT ORDER.  Nothing calls it unless asked; ks_audit_dev is unchanged by it.
 * The final state together with pod_seq decides these constraints one-sidedly, because a group's domain counts only grow (topologygroup.go:101-105) and a node's
 * requirements only narrow (node.go:80,90,103): every bit below flags only what no run of the reference can have produced.  The bits are a word of their own
 * (ks_audit_topology.pod_flags[p]), numbered on from the pod bits.
 * Definitions.  A pod's class is the one of the stage it ended at.  Group g CONSTRAINS pod P when g is in own_list (bit 31: selfSelecting) or isel_list of P's class;
 * g is RECORDED BY pod Q when g is in sel_list or iown_list of Q's class.  Groups with grp_active == 0 (created by a later Topology.Update: they never saw the earlier
 * commits) are skipped and counted in skipped_groups.  init = grp_count / grph_count as the pack kernels start from them (a derived what-if: its own tables).
 * Hostname-keyed groups are exact (a node is one domain): for P on node n, before = the pods Q != P on n that record g with seq(Q) < seq(P), c = init[g][n] (0 on a
 * new node).  Narrow-key groups of type 1 / 2: dom(n, k) = node n's final requirement on k as an In-set (an existing node's label; a new node's node_mask when the key
 * is present and no complement); a recorder is CERTAIN for k when its node was concrete on k at its own commit whatever happened later: an existing node with the
 * label, a template or a class with an In-set on k, or a group on k that constrains the recorder (topology.go:160-164). */
#define KS_AUDIT_POD_SEQ 128u               /* the pod_seq of the placed pods are not pairwise distinct and below their number: every pod of a collision, every pod out of range.  The other rules treat such a pod as unplaced */
#define KS_AUDIT_POD_ANTI_AFFINITY 256u     /* type 2, inverse groups included.  Hostname: c + before > 0.  Narrow key: for some d in dom(node(P), k), init[g][d] > 0 or a CERTAIN recorder Q != P with seq(Q) < seq(P) has d in dom(node(Q), k) (Q on P's own node counts) */
#define KS_AUDIT_POD_AFFINITY 512u          /* type 1, P not selfSelecting (the bootstrap branch, topologygroup.go:212-231, cannot be told from a violation).  Hostname: c + before == 0.  Narrow key: for some d in dom(node(P), k), init[g][d] <= 0 and no recorder Q != P, certain or not, with seq(Q) < seq(P) Has d in node(Q)'s final requirement on k (an absent key has every value) */
#define KS_AUDIT_POD_HOSTNAME_SPREAD 1024u  /* type 0 on the hostname with an empty node filter -- no term in grp_filter_off, or a term that requires nothing (present == 0, it_state == 0: what MakeTopologyNodeFilter gives a pod without node selectors, topologynodefilter.go:30-70) --: c + before + (selfSelecting ? 1 : 0) > grp_max_skew[g] (domainMinCount is 0 for the hostname, topologygroup.go:186) */
/* A pod constrained by a narrow-key group of type 1 / 2 whose own node is not concrete on the key carries the group's bit -- except on an existing node that lacks a
 * well-known label: such a node is Compatible with any requirement on it (requirements.go:123-133) and keeps its labels here, so the pair is not examined.
 * NOT attempted: spread over narrow keys (the chosen domain depends on a minimum at the time), hostname spread under a node filter (Counts depends on the node's
 * requirements at the time), self-selecting affinity, late-created groups, provisioner limits, first-fit optimality.  (Spread over narrow keys is now the third
 * pass's, ks_audit_spread_dev below: the minimum at the time is a prefix count over the commit order.  Provisioner limits are the fifth pass's,
 * ks_audit_limits_dev.) */
typedef struct ks_audit_topology {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_SEQ .. KS_AUDIT_POD_HOSTNAME_SPREAD, or NULL (totals only) */
  uint32_t n_pods, n_new;         /* out: P | the new nodes of the result that was audited */
  uint32_t n_placed;              /* out: pods on a node of the result */
  uint32_t skipped_groups;        /* out: groups no rule examined (grp_active == 0, or absent from a derived what-if) */
  uint32_t n_pods_flagged;
  uint32_t pod_bit_count[32];     /* out: pods carrying bit i */
  uint32_t checked[4];            /* out: what each rule actually evaluated -- [0] SEQ: placed pods; [1] ANTI_AFFINITY, [2] AFFINITY, [3] HOSTNAME_SPREAD: (pod, group) pairs.  A clean result with checked[i] == 0 was clean vacuously */
  double kernel_ms, readback_ms;  /* out: as ks_audit's */
} ks_audit_topology;
/* claimed == NULL: the resident result, where it lies (the form for derived what-ifs).  claimed given (flattened problems only, KS_ERR_UNSUPPORTED for a derived
 * view): pod_node, pod_stage, pod_seq, node_tmpl and the new nodes' requirement arrays are uploaded and read; every index is range-checked before it addresses
 * memory.  The batch form walks its problems in slices of at most 64 MiB of its per-group scratch table (G x 64 words per problem), five launches per slice.
 * Flags are written per index, no output through an atomic: the same flags every run.  Refusals as ks_audit_dev's. */
int ks_audit_topology_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL; pod_seq is read */, ks_audit_topology* out);
int ks_audit_topology_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_topology* const* outs);

/* ---- the audit's THIRD pass, opt-in: topology spread over NARROW keys (the zone) in COMMIT ORDER.  Nothing calls it unless asked; the first two passes are
 * unchanged by it.  "The minimum at the time" of nextDomainTopologySpread (topologygroup.go:159-200) is a prefix count over the commit order, and both monotonicities
 * above apply, so the skew inequality of topologygroup.go:171 can be tested one-sidedly: a LOWER bound of the chosen domain's count against an UPPER bound of the
 * minimum.  It flags only what no run of the reference can have produced, and it is the reference's own test wherever every recorder sits on a node that was already
 * pinned to one domain (a consolidation what-if: existing nodes with their zone label) -- exact_pairs counts those.  The bit shares its word with KS_AUDIT_POD_SEQ,
 * defined as in the second pass; a pod that fails SEQ counts as unplaced here.
 * ELIGIBLE group g: grp_type == 0, narrow key 0 <= k < K, not skipped (grp_active == 0, or absent from a derived what-if) and an empty node filter, both by the
 * second pass's definitions.  Every other spread group is unattempted and counted in skipped_groups.  init[e] = grp_count[g*64+e] (a derived what-if: its own
 * table); init[e] < 0: domain e is not registered.
 * RECORDER Q of g: g is in sel_list of Q's class (Counts() reduces to selects for an unfiltered group, topologygroup.go:109-111; Record counts a spread only when
 * Len() == 1, topology.go:129-132).  fd(Q): the final In-set of node(Q) on k (dom(n, k) above).
 * PIN TIME: pin[n][k] = the least pod_seq over the pods on node n whose class has an In-requirement on k with exactly one value, or a type-0 group on key k in its
 * own_list (any such group, filtered or skipped included: an owned group exists from the pod's own Topology.Update on, nextDomainTopologySpread returns one domain,
 * topologygroup.go:181, and node.go:80 / existingnode.go:110 add the pod's own requirement before Record).  From that commit on the node's requirement on k is a
 * single value, because requirements only narrow.
 * Q is CERTAIN when node(Q) is an existing node with the label, or its template has a single-value In on k, or pin[node(Q)][k] <= seq(Q).  Q is WILD when node(Q)
 * is an existing node whose requirement on k is absent: the reference may have pinned such a node through an earlier pod (existingnode.go:110-125), and the flat
 * problem keeps only its labels.
 * COUNTS at commit number s, per registered domain e:  L_s[e] = max(0, init[e]) + the certain Q with seq(Q) < s and fd(Q) == {e};  U_s[e] = max(0, init[e]) + the
 * Q, certain or not, with seq(Q) < s and fd(Q) == {e};  W_s = the wild Q with seq(Q) < s.  The true count lies in [L_s[e], U_s[e] + W_s]: whatever was recorded was
 * a single value, and that value is still the whole final set.
 * THE TEST for pod P (seq s, class c) and each eligible g in own_list of c (bit 31: self):
 *   1. mine = fd(P).  Absent on an existing node without a well-known label k: the pair is not examined (the second pass's exception).  Absent on any other node:
 *      flag.  popcount(mine) != 1: flag.  Else mine = {d}.
 *   2. init[d] < 0: flag.
 *   3. L_s[d] + self - min_e (U_s[e] + W_s) > grp_max_skew[g]: flag.  The minimum runs over the registered e that podDomains.Has: class c's requirement on k
 *      (kreq_has_mask), or every value when the class has none (topology.go:152-155, topologygroup.go:184-200); over no e it is INT32_MAX and nothing is flagged.
 * Only the skew inequality: whether d was the arg-min among the node's domains is first-fit optimality, which stays unattempted. */
#define KS_AUDIT_POD_SPREAD 2048u           /* a placed pod fails step 1, 2 or 3 above for some eligible group that constrains it */
typedef struct ks_audit_spread {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_SPREAD, or NULL (totals only) */
  uint32_t n_pods, n_new;         /* out: P | the new nodes of the result that was audited */
  uint32_t n_placed;              /* out: pods on a node of the result */
  uint32_t skipped_groups;        /* out: spread groups (grp_type == 0) that are not eligible: unattempted */
  uint32_t n_pods_flagged;
  uint32_t checked[2];            /* out: [0] the placed pods (SEQ); [1] the (pod, group) pairs examined.  A clean result with checked[1] == 0 was clean vacuously */
  uint32_t exact_pairs;           /* out: the pairs that reached step 3 with W_s == 0 and L_s[e] == U_s[e] on d and on every e of the minimum: there the rule is the reference's own test */
  double kernel_ms, readback_ms;  /* out: as ks_audit's */
} ks_audit_spread;
/* claimed == NULL: the resident result, where it lies (the form for derived what-ifs).  claimed given (flattened problems only, KS_ERR_UNSUPPORTED for a derived
 * view): the second pass's arrays are uploaded and read; every index a result supplies is range-checked before it addresses memory.  Five launches; the commit
 * order is cut into chunks of 256 commit numbers, the per-chunk table (chunks x G x 129 words per problem) is sized on the host, and the batch form walks its
 * problems in slices of at most 64 MiB of it (or one problem).  Flags are written per index, no output through an atomic, no float: the same flags every run.
 * Refusals as ks_audit_topology_dev's. */
int ks_audit_spread_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL; pod_seq is read */, ks_audit_spread* out);
int ks_audit_spread_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_spread* const* outs);

/* ---- the audit's FOURTH pass, opt-in: FIRST-FIT ORDER.  Nothing calls it unless asked; the first three passes are unchanged by it.  scheduler.add tries every
 * existing node, then every new node, then every template before it opens a machine (scheduler.go:174-219).  Between the moment a pod was tried and the end of the
 * Solve a node's requests only grow, its requirements only narrow, its InstanceTypeOptions only shrink, its port and volume sets only grow: a node whose FINAL state
 * would still take pod P in addition to everything on it would have taken P at any earlier moment it existed, so P cannot legally have ended anywhere later.  One-sided
 * like passes two and three: it flags only what no run of the reference can have produced.  The bits share their word with KS_AUDIT_POD_SEQ, defined as in the second
 * pass.
 * EXAMINED pod P: it does not fail SEQ (a placed pod), or it is unscheduled (pod_node == -1); its final-stage class c has an empty own_list and an empty isel_list
 * (no topology group constrains it: Topology.AddRequirements adds nothing; being RECORDED by others -- sel_list, iown_list -- is fine, Record runs after admission)
 * and no host ports.  Every other pod is counted in skipped_pods.  A class with any vol_list entry is examined against new nodes and templates only (new nodes track
 * no volumes), not against existing nodes.
 * admits_existing(c, e), existing node e of the view, not removed in a derived what-if.  The pair is examined only where every key the class names is labelled on e
 * -- cls.present & ~en.present == 0, and en.it_state[e] != 0 if the class carries an instance-type requirement: the flat problem keeps only an existing node's
 * labels, a label is a single-value In, so on those keys the node's requirement at any time IS the label and Compatible is exact; on an unlabelled key an earlier
 * topology pod may have narrowed the node in a way the result does not carry.  Then all of: en_taints[e] & ~cls_tolerated[c] == 0; the hostname mode admits e;
 * Compatible(en, cls) on every key (kreq_compatible_fail) and its_fail[en.it_state * SC + cls.it_state] == 0; Fits(en_requests[e] + the cls_requests of every pod the
 * result puts on e + cls_requests[c], en_avail[e]) under resources.Fits' presence rule, int64.
 * admits_new(c, j), new node j with template m in range.  All of: the template's taints are tolerated; cls_hn_mode[c] != 1 (a new node's placeholder hostname is in
 * no list); every non-well-known key the class names with an operator other than NotIn / DoesNotExist is present in tmpl.present[m] ("custom labels, if not defined,
 * are denied" looks at the node at the time, requirements.go:125-130; a later pod may have added the key to the final requirements, the template had it all along);
 * on every narrow key present in both the node's final requirements and the class the INTERSECTION IS NON-EMPTY -- the NotIn / DoesNotExist exception of
 * requirements.go:196-200 is not used: a final state that passes only through it can have failed earlier (a node at Exists refuses the DoesNotExist pod that the same
 * node, later narrowed to DoesNotExist, lets through); its_fail[node_it_state * SC + cls.it_state] == 0; and some type t in node_types[j] & its_types[its_inter[..]]
 * passes compatible && fits && hasOffering (node.go:137-159) against the node's final requirements intersected with the class and node_requests[j] + cls_requests[c].
 * admits_template(c, m), only for tmpl_limit_present[m] == 0xFFFFFFFF: admits_new against a fresh node -- the template's requirements, tmpl_daemon[m], tmpl_types[m].
 * open(j): the least pod_seq over the pods on new node j that do not fail SEQ.  first_e(c): the least e with admits_existing.  first_open(c): the least open(j) over
 * the j with admits_new.  first_m(c): the least m with admits_template. */
#define KS_AUDIT_POD_FIT_EXISTING 4096u     /* P is on existing node e and first_e(c) < e; or P is on a new node or unscheduled and first_e(c) exists */
#define KS_AUDIT_POD_FIT_NEW 8192u          /* P opened its new node (seq(P) == open(node(P))) and first_open(c) < seq(P) -- strictly: its own node opened at seq(P); or P is unscheduled and first_open(c) exists */
#define KS_AUDIT_POD_FIT_TEMPLATE 16384u    /* P opened a node of template m and first_m(c) < m; or P is unscheduled and first_m(c) exists */
/* A pod on a new node it did not open is checked against existing nodes only: the order among new nodes at the time depends on pod counts at the time (sort.Slice,
 * scheduler.go:183).  NOT attempted: topology-constrained pods (the next step would be hostname anti-affinity and unfiltered hostname spread, whose per-node counts
 * also only grow), pods with host ports, limited templates, existing nodes on keys they do not label, the order among new nodes, provisioner limits.  (Limited
 * templates and provisioner limits are the fifth pass's, ks_audit_limits_dev below: KS_AUDIT_POD_LIMIT_TEMPLATE is FIT_TEMPLATE for them.  Pods under hostname
 * anti-affinity and unfiltered hostname spread are the sixth pass's, ks_audit_hostfit_dev below: KS_AUDIT_POD_HFIT_* are FIT_* for them.) */
typedef struct ks_audit_firstfit {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_FIT_*, or NULL (totals only) */
  uint32_t n_pods, n_new;         /* out: P | the new nodes of the result that was audited */
  uint32_t n_placed;              /* out: pods on a node of the result */
  uint32_t skipped_pods;          /* out: the pods that are not examined */
  uint32_t n_pods_flagged;
  uint32_t checked[3];            /* out: [0] the placed pods (SEQ); [1] the pods examined; [2] the (class, node-or-template) pairs evaluated, over the distinct classes of the examined pods */
  uint32_t admitting_pairs;       /* out: how many of those pairs admitted.  A clean result with admitting_pairs == 0 proved little */
  double kernel_ms, readback_ms;  /* out: as ks_audit's */
} ks_audit_firstfit;
/* claimed == NULL: the resident result, where it lies (the form for derived what-ifs: removed nodes are skipped, the pods' classes are the snapshot's).  claimed given
 * (flattened problems only, KS_ERR_UNSUPPORTED for a derived view): what the first pass uploads but the unscheduled list -- pod_seq among it -- is uploaded and read;
 * every index a result supplies is range-checked before it addresses memory.  Six launches; the scratch of a problem is O(P + C + E x R + max_new_nodes) words, so a
 * batch is one slice.  The tables behind the verdict are built by integer min, add and or; flags are written per index, no output through an atomic, no float: the
 * same flags every run.  Refusals as ks_audit_spread_dev's. */
int ks_audit_firstfit_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL; pod_seq is read */, ks_audit_firstfit* out);
int ks_audit_firstfit_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_firstfit* const* outs);

/* ---- the audit's FIFTH pass, opt-in: PROVISIONER LIMITS in OPENING ORDER.  Nothing calls it unless asked; the first four passes are unchanged by it.  Before it
 * opens a machine of a provisioner with limits scheduler.add keeps only the types whose Capacity is within the provisioner's remaining resources
 * (filterByRemainingResources, scheduler.go:197-206,293-309), and after the opener's Add it takes the MaxResources of the node's options off them (subtractMax,
 * scheduler.go:215,273-290).  remainingResources depends on the order of opening -- but a node's options only shrink, so the final state and pod_seq bound it from
 * both sides, and every bit below flags only what no run of the reference can have produced.  The pod bit shares its word with KS_AUDIT_POD_SEQ, defined as in the
 * second pass; the node bits continue KS_AUDIT_NODE_* in a word of this pass's own (ks_audit_limits.node_flags).
 * Template m is LIMITED when lim = tmpl_limit_present[m] != 0xFFFFFFFF; lim == 0 (Spec.Limits non-nil and empty) is limited with no limited resource.  "On lim": over
 * the resources r whose bit is set in lim.  cap[t][r] = it_cap[r*T+t].  R0[m] = tmpl_remaining[m*R..] (a derived what-if: its own table).
 * open(j): the fourth pass's -- the least pod_seq over the pods on new node j that do not fail SEQ; that pod is j's OPENER.  A new node without such a pod, or with
 * node_tmpl outside [0, M), is UNORDERED and counted in skipped_nodes (where the problem has a limited template at all).  The ordered nodes of a limited template
 * are taken in the order of open(j), not of j (a result may come from a Go run, where sort.Slice has permuted newNodes); i < j: same template, opened earlier.  A
 * limited template with an unordered node gets the EXTRA rule only, over its ordered nodes: without that node a lower bound of its remaining is not one.
 *   mc(j)[r] = max(0, max over t in node_types[j], t < T, of cap[t][r]): the final options' MaxResources.
 *   U_j = R0[m] - sum over i < j of mc(i), on lim: an UPPER bound of the remaining just before j opened (the options at opening include the final ones, so what
 *         subtractMax took is at least mc(i)).  For an unordered node of a limited template U_j = R0[m].
 *   W_j = the t in tmpl_types[m] with cap[t] <= U_j on lim that pass compatible && fits && hasOffering (node.go:137-159) for a fresh node of m holding only j's
 *         opener: the fourth pass's per-type test of admits_template for the opener's final-stage class -- a superset of the options subtractMax saw (a
 *         topology-constrained opener only narrows further).  mw(j) = max(0, MaxResources over W_j).
 *   L_m[k] = R0[m] - the sum of mw over the first k openings of m, k = 0 .. n_m: a LOWER bound, non-increasing in k.  L_j = L_m[the openings before j].
 *   Node j is EXACT when mw(i) == mc(i) on lim for every i < j: there L_j == U_j and the rule is the reference's own test.
 * Sums are int64 and saturating; caps are taken as non-negative, a remaining that would pass below INT64_MIN stays there. */
#define KS_AUDIT_NODE_LIMIT_EXTRA 256u      /* new node j of a limited template: some t in node_types[j] has cap[t][r] > U_j[r] for an r in lim (filterByRemainingResources, scheduler.go:293-309) */
#define KS_AUDIT_NODE_LIMIT_MISSING 512u    /* new node j of an ordered limited template: some t in tmpl_types[m] is absent from node_types[j] although cap[t] <= L_j on lim and t passes the first pass's final-state filter for node j (the test behind KS_AUDIT_NODE_OPTIONS_MISSING; the filter is monotone): the equality the first pass grants unlimited templates, wherever the bound reaches */
#define KS_AUDIT_POD_LIMIT_TEMPLATE 32768u  /* P examined as in the fourth pass (no constraining group, no host ports; it does not fail SEQ, or it is unscheduled).  P opened a node of template m': for an ordered limited m < m', k = the openings of m with open < seq(P); P is unscheduled: for every ordered limited m, k = n_m (remaining only falls, so the end state bounds every attempt).  Flagged when admits_template's scalar clauses hold for (c, m) and some t in tmpl_types[m] has cap[t] <= L_m[k] on lim and passes the fresh-node type test: the fourth pass's FIT_TEMPLATE, extended to limited templates */
/* NOT attempted: pod_reason's KS_WHY_LIMITS nibble; tmpl_remaining itself (the caller's input); topology-constrained openers on the pod side. */
typedef struct ks_audit_limits {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_LIMIT_TEMPLATE, or NULL (totals only) */
  uint32_t* node_flags;           /* [E + max_new_nodes] KS_AUDIT_NODE_LIMIT_*; entries [0, n_nodes) are written (an existing node's is 0); or NULL */
  uint32_t n_pods, n_nodes;       /* out: P | E + n_new */
  uint32_t n_new, n_placed;       /* out: the new nodes of the result that was audited | pods on a node of the result */
  uint32_t limited_templates;     /* out: the limited templates of the problem; 0: nothing but SEQ was examined, and every count below is 0 */
  uint32_t skipped_nodes, skipped_pods;   /* out: the unordered new nodes | the pods that are not examined */
  uint32_t n_pods_flagged, n_nodes_flagged;
  uint32_t pod_bit_count[32], node_bit_count[32];   /* out: pods / nodes carrying bit i */
  uint32_t checked[4];            /* out: [0] the placed pods (SEQ); [1] the new nodes of limited templates examined; [2] the pods examined; [3] the (class, ordered limited template) pairs evaluated, over the distinct classes of the examined pods */
  uint32_t exact_nodes;           /* out: the exact nodes of the ordered limited templates */
  uint32_t binding_nodes;         /* out: the nodes whose U_j excluded at least one type of tmpl_types[m].  A clean result with binding_nodes == 0 proved little */
  double kernel_ms, readback_ms;  /* out: as ks_audit's */
} ks_audit_limits;
/* claimed == NULL: the resident result, where it lies (the form for derived what-ifs).  claimed given (flattened problems only, KS_ERR_UNSUPPORTED for a derived
 * view): the fourth pass's arrays are uploaded and read; every index a result supplies is range-checked before it addresses memory.  A problem without a limited
 * template returns KS_OK with limited_templates == 0 after the SEQ kernels alone (two launches); otherwise nine launches, the scratch of a problem is
 * O(P + C x M + max_new_nodes x R) words, so a batch is one slice.  The tables behind the verdict are built by integer min, add and or; flags are written per index,
 * no output through an atomic, no float: the same flags every run.  Refusals as ks_audit_firstfit_dev's. */
int ks_audit_limits_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL; pod_seq is read */, ks_audit_limits* out);
int ks_audit_limits_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_limits* const* outs);

/* ---- the audit's SIXTH pass, opt-in: FIRST-FIT ORDER for pods under HOSTNAME anti-affinity and unfiltered HOSTNAME SPREAD.  Nothing calls it unless asked; the first
 * five passes are unchanged by it.  For a pod whose constraining groups are all on the hostname Topology.AddRequirements (topology.go:149-167) adds a requirement on
 * the hostname only, and a node's hostname is one value for its whole life.  nextDomainAntiAffinity (topologygroup.go:235-243) allows the node iff its domain is
 * registered with count 0; nextDomainTopologySpread (topologygroup.go:155-182) has a hostname minimum of 0 (topologygroup.go:186) and allows it iff
 * count + self <= maxSkew.  Counts only grow (Record, topologygroup.go:101-105): a node whose FINAL counts admit the pod admitted it at every earlier moment, and the
 * fourth pass's argument carries over clause by clause.  Pod affinity (type 1) is NOT eligible: growing counts make affinity easier later, so a final state that
 * admits proves nothing about earlier moments.  One-sided like the passes before it; the bits share their word with KS_AUDIT_POD_SEQ, defined as in the second pass.
 * ELIGIBLE group g: grp_key[g] is the hostname (with a row of the hostname tables: 0 <= grp_hslot[g] < GH); g is not skipped by the second pass's definition
 * (grp_active == 0, or absent from a derived what-if); grp_type[g] == 2 (inverse groups included), or grp_type[g] == 0 with an empty node filter by the second pass's
 * definition.  eligible_groups counts them, skipped_groups every other group of the problem.
 * EXAMINED pod P: it does not fail SEQ, or it is unscheduled; its final-stage class c reserves no host port; own_list(c) U isel_list(c) is non-empty and every entry
 * of it is eligible.  A class with both lists empty is the fourth pass's: the two passes partition the pods they examine.  Every other pod is counted in skipped_pods.
 * fin[g][n] = init[g][n] -- as the second pass defines it: grph_count for an existing node (a derived what-if: its own tables), 0 for a new node -- plus the number of
 * pods the result puts on n whose final-stage class records g (sel_list or iown_list), the pods that fail SEQ included: a larger count only removes flags.
 * init < 0 (the hostname is not registered with g): n never admits on g.
 * ok(c, g, n), g constraining c: type 2: fin[g][n] == 0; type 0: fin[g][n] + self <= grp_max_skew[g], self = bit 31 of the own_list entry.
 * admits_existing / admits_new / admits_template: the fourth pass's predicate of the same name AND ok(c, g, n) for every g constraining c -- with its examined-pair
 * condition on labelled keys, its volume exception, its template-presence rule for custom labels, its non-empty-intersection rule and its exclusion of limited
 * templates unchanged.  A fresh node of a template has every count 0.  open(j), first_e(c), first_open(c), first_m(c): as in the fourth pass, over these predicates. */
#define KS_AUDIT_POD_HFIT_EXISTING 65536u   /* KS_AUDIT_POD_FIT_EXISTING's verdict: P is on existing node e and first_e(c) < e; or P is on a new node or unscheduled and first_e(c) exists */
#define KS_AUDIT_POD_HFIT_NEW 131072u       /* KS_AUDIT_POD_FIT_NEW's: P opened its new node (seq(P) == open(node(P))) and first_open(c) < seq(P); or P is unscheduled and first_open(c) exists */
#define KS_AUDIT_POD_HFIT_TEMPLATE 262144u  /* KS_AUDIT_POD_FIT_TEMPLATE's: P opened a node of template m and first_m(c) < m; or P is unscheduled and first_m(c) exists */
/* A pod on a new node it did not open is checked against existing nodes only, as in the fourth pass.  NOT attempted: pod affinity, groups on narrow keys, hostname
 * spread under a node filter, late-created groups, pods with host ports, limited templates, existing nodes on keys they do not label, the order among new nodes. */
typedef struct ks_audit_hostfit {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_HFIT_*, or NULL (totals only) */
  uint32_t n_pods, n_new;         /* out: P | the new nodes of the result that was audited */
  uint32_t n_placed;              /* out: pods on a node of the result */
  uint32_t eligible_groups, skipped_groups;   /* out: the eligible groups | the other groups of the problem */
  uint32_t skipped_pods;          /* out: the pods that are not examined */
  uint32_t n_pods_flagged;
  uint32_t checked[4];            /* out: [0] the placed pods (SEQ); [1] the pods examined; [2] the (class, node-or-template) pairs evaluated, over the distinct classes of the examined pods; [3] the (pair, group) count tests evaluated: every pair evaluates the test of every group that constrains its class */
  uint32_t admitting_pairs;       /* out: how many of those pairs admitted.  A clean result with admitting_pairs == 0 proved little */
  double kernel_ms, readback_ms;  /* out: as ks_audit's */
} ks_audit_hostfit;
/* claimed == NULL: the resident result, where it lies (the form for derived what-ifs).  claimed given (flattened problems only, KS_ERR_UNSUPPORTED for a derived
 * view): the fourth pass's arrays are uploaded and read; every index a result supplies is range-checked before it addresses memory.  Eight launches; fin is a dense
 * int32 table of (E + max_new_nodes) x GH words per problem, sized on the host, and the batch form walks its problems in slices of at most 64 MiB of it (or one
 * problem).  The tables behind the verdict are built by integer min, add and or; flags are written per index, no output through an atomic, no float: the same flags
 * every run.  Refusals as ks_audit_firstfit_dev's. */
int ks_audit_hostfit_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL; pod_seq is read */, ks_audit_hostfit* out);
int ks_audit_hostfit_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_hostfit* const* outs);

/* ---- the audit's SEVENTH pass, opt-in: RELAXATION ORDER -- the one column of a result the six passes above take on trust, pod_stage.  Nothing calls it unless
 * asked: the gate below runs it for KS_AUDIT_PASS_STAGES (ks_audit_gate_ex); the first six passes are unchanged by it.  Solve relaxes a pod one step per failed add (scheduler.go:118-127, preferences.go:36-145):
 * a pod P that ended at stage k = pod_stage[P], placed or unscheduled, was tried and refused at every stage j < k, each try at some moment before the end.  Let
 * c_j = stage_cls[pod_stage_off[gp] + j].  By the fourth pass's monotonicity two kinds of target need no knowledge of WHEN stage j was tried: an existing node was
 * there from the start and only filled up, and a fresh node of a template without limits is static data.  One-sided like passes two to six: it flags only what no run
 * of the reference can have produced.  The bits share their word with KS_AUDIT_POD_SEQ, defined as in the second pass.
 * EXAMINED stage j of pod P: j < k; P does not fail SEQ, or is unscheduled (pod_node == -1); pod_stage[P] lies inside P's chain; c_j is examinable in the fourth
 * pass's sense (empty own_list and isel_list, no host port).  A pod with k == 0 or without an examined stage is counted in skipped_pods.
 * admits_existing(c, e), admits_template(c, m): the fourth pass's predicates of those names, with its examined-pair condition on labelled keys, its volume exception
 * (a class with any vol_list entry is not examined against existing nodes), its skipping of the nodes that left a derived what-if and its exclusion of limited
 * templates.  When P itself sits on e its own requests are in e's sum and the class's are added again: that only removes flags. */
#define KS_AUDIT_POD_STAGE_EXISTING 524288u   /* for some examined stage j of P, some existing node e has admits_existing(c_j, e): the node took no less at the moment stage j was tried, so that add cannot have failed */
#define KS_AUDIT_POD_STAGE_TEMPLATE 1048576u  /* for some examined stage j of P, some template m without limits has admits_template(c_j, m): add would have opened a machine at stage j */
#define KS_AUDIT_POD_STAGE_UNRELAXED 2097152u /* P is unscheduled and pod_stage[P], in range, is not the last stage of its chain: the queue ends only on pods pushed back unrelaxed (queue.go:44-68), and Relax returns false only at the end of the chain */
/* NOT attempted: new nodes as targets (whether node j existed when stage j was tried is not in the result); earlier stages constrained by any topology group (the
 * hostname kinds are the next step, by the sixth pass's count tests: a fresh node's counts are 0); limited templates; classes with host ports; existing nodes on
 * keys they do not label. */
typedef struct ks_audit_stages {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_STAGE_*, or NULL (totals only) */
  uint32_t n_pods, n_new;         /* out: P | the new nodes of the result that was audited */
  uint32_t n_placed;              /* out: pods on a node of the result */
  uint32_t skipped_pods;          /* out: the pods without an examined stage */
  uint32_t n_pods_flagged;
  uint32_t checked[4];            /* out: [0] the placed pods (SEQ); [1] the pods with an examined stage; [2] the examined stages, summed over those pods; [3] the (class, existing-node-or-template) pairs evaluated, over the distinct classes of the examined stages */
  uint32_t admitting_pairs;       /* out: how many of those pairs admitted: 0 in a clean result */
  double kernel_ms, readback_ms;  /* out: as ks_audit's -- but kernel_ms holds one host wait more than the other passes': the read-back of the meta words between the second and the third launch, which decides whether the last four run */
} ks_audit_stages;
/* claimed == NULL: the resident result, where it lies (the form for derived what-ifs).  claimed given (flattened problems only, KS_ERR_UNSUPPORTED for a derived
 * view): the fourth pass's arrays are uploaded and read; every index a result supplies -- pod_stage above all -- is range-checked before it addresses memory.  Two
 * launches, then the meta words are read back: where no pod of the CALL has an examined stage (nothing relaxed) the flags are final; else -- for every problem of
 * the batch, the ones that relaxed nothing included: they evaluate no pair -- four more launches, three
 * of them the fourth pass's kernels over the distinct classes of the examined stages.  The scratch of a problem is the fourth pass's: a batch is one slice.  Integer
 * min, add and or; flags are written per index, no output through an atomic, no float: the same flags every run.  Refusals as ks_audit_firstfit_dev's. */
int ks_audit_stages_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL; pod_seq is read */, ks_audit_stages* out);
int ks_audit_stages_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_stages* const* outs);

/* ---- the audit's EIGHTH pass, opt-in: FAILURE REASONS -- the one column of a result the seven passes above do not read, pod_reason (ks_result above: KS_WHY_* per
 * machine template, four bits each, what the shim turns into PodFailedToSchedule events and "incompatible with provisioner ..., <reason>" lines).  Nothing calls it
 * unless asked: the gate below runs it for KS_AUDIT_PASS_REASONS (ks_audit_gate_ex); the first seven passes are unchanged by it.  A fresh node of a template is static data and Node.Add (node.go:62-107) runs
 * its steps in a fixed order -- taints, host ports, Compatible, topology, topology requirements, instance types --, so for many (pod, template) pairs the nibble has
 * exactly one right value: those get an EQUALITY check.  w = pod_reason[P]; M templates; MT = min(M, 8); c = the class of the stage the result claims (aud_class).
 * On the whole word: */
#define KS_AUDIT_POD_REASON_PLACED 4194304u    /* P names a node of the result and w != 0: both pack kernels and the oracle clear the word on every successful add */
#define KS_AUDIT_POD_REASON_MISSING 8388608u   /* P is unscheduled (pod_node == -1), pod_stage in range, and some template m < MT has nibble KS_WHY_NONE: add returns an error only after every template produced one (scheduler.go:193-218) */
#define KS_AUDIT_POD_REASON_SHAPE 16777216u    /* such a P, and: a nibble at m >= M is non-zero; or a nibble is above 7; or is KS_WHY_HOST_PORTS (a fresh node has no port in use); or is KS_WHY_LIMITS on a template without limits (tmpl_limit_present[m] == 0xFFFFFFFF) */
#define KS_AUDIT_POD_REASON_STATIC 33554432u   /* such a P, and a nibble at m < MT that neither MISSING nor SHAPE flags contradicts the static verdict s(c, m) below */
/* s(c, m), from the flat problem through ks_algebra.h alone (no mc_* table, no feasibility grid: those are the pack kernels' own), in Node.Add's order:
 *   1. tmpl_taints[m] & ~cls_tolerated[c] != 0                                                                 -> 2 (TAINTS)
 *   2. cls_hn_mode[c] == 1 (a fresh node's hostname is a placeholder no pod names, node.go:46); or kreq_compatible_fail(template, class) on any key -- the EXACT
 *      Compatible, with its custom-label rule and its NotIn / DoesNotExist exception; or the its_fail entry of the two it_states   -> 4 (REQUIREMENTS)
 *   3. c is not examinable in the fourth pass's sense (an own group, an inverse group or a host port)           -> U (undecided: topology speaks next)
 *   4. filterInstanceTypesByRequirements over the template's FULL type set, its daemon overhead plus the class's requests and the merged requirements:
 *      a type passes -> 0, none does -> 7 (NO_INSTANCE_TYPE)
 * The verdict on the nibble at m < MT of an unscheduled pod:
 *   template without limits:  s in {2, 4, 7, 0}: the nibble is exactly s (0: KS_WHY_NONE, which MISSING flags -- the fourth pass's FIT_TEMPLATE with the exact Compatible);
 *                             s == U: the nibble is one of {5, 6, 7}
 *   template with limits:     KS_WHY_LIMITS is always allowed and not examined (counted); otherwise s in {2, 4}: exactly s; s in {7, 0}: 7 (the limit only shrinks
 *                             the type set); s == U: one of {5, 6, 7}
 * NOT attempted: whether a LIMITS nibble on a limited template is true; which of {5, 6, 7} a topology-constrained class carries; templates from the ninth on (they
 * have no nibble); pods whose pod_stage is out of range (the first pass's RANGE); a template that lists no instance type at all (counted with the unexamined). */
typedef struct ks_audit_reasons {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_REASON_*, or NULL (totals only) */
  uint32_t n_pods, n_new;         /* out: P | the new nodes of the result that was audited */
  uint32_t n_placed;              /* out: pods on a node of the result: each examined for PLACED */
  uint32_t n_unscheduled;         /* out: pods with pod_node == -1 */
  uint32_t skipped_pods;          /* out: the pods neither placed nor examined: a stage out of range, a node the result does not have */
  uint32_t n_pods_flagged;
  uint32_t checked[4];            /* out: [0] the unscheduled pods examined; [1] their nibbles decided exactly; [2] their nibbles bounded to a set; [3] their nibbles not examined (LIMITS on a limited template, a template without types): [1] + [2] + [3] == min(M, 8) * [0] */
  uint32_t used_classes, pairs;   /* out: the distinct classes of the examined pods | the (class, template) verdicts computed: used_classes * min(M, 8) */
  double kernel_ms, readback_ms;  /* out: as ks_audit's */
} ks_audit_reasons;
/* claimed == NULL: the resident result, where it lies (the form for derived what-ifs).  claimed given (flattened problems only, KS_ERR_UNSUPPORTED for a derived
 * view): pod_node, pod_stage and pod_reason are uploaded and read, nothing else and no commit numbers; a null pod_reason is KS_ERR_INVALID "claimed result: null
 * array pod_reason"; the remaining refusals are ks_audit_dev's.  Four launches with no host wait between them: mark, the fourth pass's compaction, one wave per
 * (used class, template) pair, verdict; with no unscheduled pod the third finds an empty list and the fourth repeats the first one's words.  Integer only; flags are
 * written per index, no output through an atomic: the same flags every run. */
int ks_audit_reasons_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL; pod_node, pod_stage, pod_reason are read */, ks_audit_reasons* out);
int ks_audit_reasons_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_reasons* const* outs);

/* ---- the audit's NINTH pass, opt-in and beside the gate: FIRST-FIT ORDER for pods under ZONAL SPREAD -- the pods the fourth pass leaves out because a topology group
 * constrains them and the sixth leaves out because the group is on a narrow key.  Nothing calls it unless asked; the eight passes above and the gate are unchanged by
 * it.  A zonal group's minimum moves over time, so the final state alone decides nothing; the final state TOGETHER WITH the commit numbers does.  One-sided like the
 * passes before it; the bits share their word with KS_AUDIT_POD_SEQ, defined as in the second pass.
 * ELIGIBLE group g: the third pass's definition, unchanged: grp_type[g] == 0, a narrow key 0 <= grp_key[g] < K, not skipped, an empty node filter.  eligible_groups
 * counts them, skipped_groups every other group of the problem.
 * EXAMINED pod P: it does not fail SEQ, or it is unscheduled; its final-stage class c reserves no host port; isel_list(c) is empty; own_list(c) holds between one and
 * KS_AZ_GROUPS entries and every one of them is eligible.  Every other pod is counted in skipped_pods; of those, the pods whose class owns an eligible zonal group and
 * is also constrained by a hostname-keyed group (own_list or isel_list) are counted in mixed_pods as well: the named next step.  The fourth, the sixth and this pass
 * partition the pods they examine.
 * THE MOMENT s: a placed P was tried for the last time when exactly the pods with commit number < s = pod_seq[P] had committed (scheduler.add walks the existing nodes,
 * the new nodes and the templates, and nothing commits in between); an unscheduled P was tried last against the final state: s = n_placed (queue.go:52-66).
 * ADMISSIBLE DOMAINS at s, per g in own_list(c) on key k: the third pass's bounds at prefix s -- L_s[e] over the certain recorders with commit number < s, U_s[e]
 * over all of them, the wild count W_s --, its `among` (the registered domains e, grp_count[g][e] >= 0, for which the class's requirement on k Has e; an absent key
 * has every value) and self (bit 31 of the entry):
 *   OK_s[g] = { e registered : U_s[e] + W_s + self - min over e' in among of L_s[e'] <= grp_max_skew[g] }
 * The true count is at most U + W and the true minimum at least min L: e in OK_s[g] implies that the inequality of topologygroup.go:171 held at s -- the opposite
 * pairing of the bounds to the third pass's test, on purpose.  With `among` empty OK_s[g] is empty: Go's MaxInt32 minimum admits everything there and the pass proves
 * nothing from it.
 * TARGETS.  Existing node e (a class that mounts volumes has none): the fourth pass's admits_existing(c, e), with its condition on labelled keys and Fits over the
 * final sums, AND for every g of c: e carries the label of key(g) with the single value z, and z is in OK_s[g] (the node's nodeDomains is {z} for its whole life, so
 * the topology step admits iff z is admissible, existingnode.go:104-120).  New node j, only
 * for a pod that opened its node (s == open(node(P))) or is unscheduled: open(j) < s; for every g the requirement of j on key(g) was one value before s (the third
 * pass's `certain` at commit number s - 1) and its final single value z is in OK_s[g]; the fourth pass's admits_new(c, j) with its template-presence and
 * non-empty-intersection rules.  Requirements only narrow, so the value at s was z.  Templates are no targets: with several zones open the arg-min domain and Go's
 * map order decide. */
#define KS_AZ_GROUPS 4u                        /* the most eligible groups a class may own and still be examined */
#define KS_AUDIT_POD_ZFIT_EXISTING 67108864u   /* P is on existing node e_P and some target e < e_P admits at s; or P is on a new node or unscheduled and some existing node admits at s */
#define KS_AUDIT_POD_ZFIT_NEW 134217728u       /* P opened its new node or is unscheduled, and some new node j with open(j) < s admits at s */
/* A pod that joined a new node it did not open is checked against existing nodes only, as in the fourth pass.  NOT attempted: templates, limited templates, the order
 * among new nodes, classes mixing zonal and hostname groups, groups under a node filter, late-created groups, host ports, existing nodes on keys they do not label. */
typedef struct ks_audit_zonefit {
  uint32_t* pod_flags;            /* [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_ZFIT_*, or NULL (totals only) */
  uint32_t n_pods, n_new;         /* out: P | the new nodes of the result that was audited */
  uint32_t n_placed;              /* out: pods on a node of the result */
  uint32_t eligible_groups, skipped_groups;   /* out: the eligible groups | the other groups of the problem */
  uint32_t skipped_pods, mixed_pods;          /* out: the pods that are not examined | those of them whose class mixes eligible zonal groups with hostname groups */
  uint32_t n_pods_flagged;
  uint32_t checked[4];            /* out: [0] the placed pods (SEQ); [1] the pods examined; [2] the (pod, node) pairs whose zone test ran; [3] the pairs that passed the zone test and had the static predicate evaluated */
  uint32_t admitting_pairs;       /* out: the pairs that admitted -- in a clean result: existing nodes at or behind the pod's own.  A clean result with admitting_pairs == 0 proved little */
  uint32_t exact_pods;            /* out: the examined pods with W == 0 and L == U on every registered domain of every group they own, and a non-empty `among`: there the masks are the reference's own numbers */
  double kernel_ms, readback_ms;  /* out: as ks_audit's */
} ks_audit_zonefit;
/* claimed == NULL: the resident result, where it lies (the form for derived what-ifs).  claimed given (flattened problems only, KS_ERR_UNSUPPORTED for a derived
 * view): the fourth pass's arrays are uploaded and read; every index a result supplies is range-checked before it addresses memory.  Twelve launches with no host
 * wait between them, six of them the third and fourth passes' kernels as they are; a problem with no eligible group or no examined pod ends, as far as this pass's
 * own work goes, after the count and mark launches (four): the kernels behind them that are this pass's return after one load, and the last writes the SEQ bits.
 * The chunk table is the third pass's, so the batch form walks its problems in the third pass's slices.  Integer min, add and or; flags are written per index, no
 * output through an atomic, no float: the same flags every run.  Refusals as ks_audit_firstfit_dev's. */
int ks_audit_zonefit_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL; pod_seq is read */, ks_audit_zonefit* out);
int ks_audit_zonefit_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_zonefit* const* outs);

/* ---- the audit's GATE: chosen passes in ONE call, their totals and a list of FINDINGS reduced on the device.  The question a caller puts behind every result is
 * "is it clean?", and the answer is usually yes: the gate runs the chosen passes' own kernels, leaves their flag tables on the device, tallies them there and reads
 * back the totals alone -- no row of a flag table reaches the host.  The six passes and their entry points above are unchanged by it; they remain the way to the rows.
 * Every requested pass's out struct receives exactly what that pass's own entry point writes into it -- every count, bit count, `checked` entry and counter -- but
 * for its tables, which are neither read nor written (the pointers may be anything), and its two times, which are that pass's share of the gate's.
 * FINDINGS: one record per non-zero flag word, ordered by pass (the order of the mask bits), then by problem, then pods before nodes, then by index.  The order comes
 * from a scan on the device, not from an atomic append: the list is the same every run.  n_findings is always the full count; when it exceeds cap_findings the first
 * cap_findings records are written, KS_AUDIT_GATE_TRUNCATED is set and the table beyond them is untouched.  cap_findings == 0 with findings == NULL is the plain
 * yes/no gate: clean iff n_findings == 0. */
#define KS_AUDIT_PASS_FIRST 1u       /* ks_audit_dev */
#define KS_AUDIT_PASS_TOPOLOGY 2u    /* ks_audit_topology_dev */
#define KS_AUDIT_PASS_SPREAD 4u      /* ks_audit_spread_dev */
#define KS_AUDIT_PASS_FIRSTFIT 8u    /* ks_audit_firstfit_dev */
#define KS_AUDIT_PASS_LIMITS 16u     /* ks_audit_limits_dev */
#define KS_AUDIT_PASS_HOSTFIT 32u    /* ks_audit_hostfit_dev */
#define KS_AUDIT_PASS_ALL 63u
#define KS_AUDIT_GATE_TRUNCATED 1u
typedef struct ks_audit_finding {
  uint32_t problem;               /* the problem's position in the batch (0 for the single form) */
  uint32_t where;                 /* pass << 8 | table: pass = the index of its mask bit (0 first .. 5 hostfit; 6 stages, 7 reasons through ks_audit_gate_ex), table 0 = pod_flags, 1 = node_flags */
  uint32_t index;                 /* the pod, or the node slot */
  uint32_t flags;                 /* the flag word, as the pass's own table holds it */
} ks_audit_finding;
typedef struct ks_audit_gate {
  uint32_t passes;                /* in: KS_AUDIT_PASS_*, at least one */
  uint32_t cap_findings;          /* in: records `findings` holds */
  ks_audit_finding* findings;     /* in: the caller's table, or NULL with cap_findings == 0 */
  ks_audit* first; ks_audit_topology* topology; ks_audit_spread* spread; ks_audit_firstfit* firstfit; ks_audit_limits* limits; ks_audit_hostfit* hostfit;
                                  /* in: for every requested pass an array of one out struct per problem (the others are not looked at) */
  const int32_t* first_pod_seq;   /* in, claimed form only: the commit numbers the FIRST pass is to read instead of claimed->pod_seq, or NULL (kshost's claimed form
                                   * numbers the placed pods in pod order for it, as ksh_audit_claimed does, while the later passes read the caller's) */
  uint32_t n_findings, truncated; /* out: the non-zero flag words of all requested passes | KS_AUDIT_GATE_TRUNCATED */
  double kernel_ms, readback_ms;  /* out: the sums of the passes' times: uploads, launches (the reduction's among them) and completion | the totals' and the findings' way back */
} ks_audit_gate;
/* ks_audit_gate_dev: one problem -- the resident result (claimed == NULL) or the caller's arrays, taken once and uploaded once with the union of the arrays the
 * requested passes read.  ks_audit_gate_batch_dev: the resident results of a batch.  Refusals (nothing launched, no out struct written): nothing runs unless every
 * requested pass accepts the call; the refusals are the passes' own, code and text, and where two apply the earliest pass in the mask wins.  The gate's own, before
 * them: KS_ERR_INVALID for an empty mask, for a bit outside KS_AUDIT_PASS_ALL, and for findings == NULL with cap_findings != 0.  A sliced pass (topology, spread,
 * hostfit) reduces per slice; slices are consecutive runs of problems, so the findings keep their order. */
int ks_audit_gate_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL */, ks_audit_gate* gate);
int ks_audit_gate_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_gate* gate);
/* The gate over ALL EIGHT passes, in a struct that can grow.  ks_audit_gate above is pinned: its size, its six pointers and KS_AUDIT_PASS_ALL stay what they are, and
 * bit 64 through the two calls above stays "audit gate: unknown pass".  ks_audit_gate_ex carries everything ks_audit_gate carries -- same meaning, same rules, same
 * findings, where = 6 << 8 and 7 << 8 for the two new passes, which have a pod table only -- behind a leading struct_size, the caller's sizeof, and the later passes'
 * pointers AFTER everything else: a ninth pass appends a pointer and a bit, not a third family of entry points.  A mask bit is KNOWN iff it lies within
 * KS_AUDIT_PASS_ALL_EX and its pointer lies wholly within struct_size; anything else is KS_ERR_INVALID "audit gate: unknown pass" (so a caller compiled against a
 * shorter struct is refused a pass it has no pointer for, and never has memory behind its struct read).  struct_size below the offset of `stages` is KS_ERR_INVALID.
 * The two calls above are this gate restricted to the six bits and the old struct: one function.
 * Under the gate the seventh pass queues all six of its launches and meets the host once, like every other pass: the decision its own call takes on the host between
 * the second and the third launch is taken on the device, per problem -- a problem in which no pod relaxed compacts an empty class list, the two pair kernels make no
 * trip for it and the verdict repeats the mark kernel's words, whatever its neighbours in the batch do.
 * Claimed form: the upload carries the union of what the requested passes read; pod_reason travels (beside the block, as first_pod_seq does) only when
 * KS_AUDIT_PASS_REASONS is requested, and a null pod_reason is then that pass's own refusal, "claimed result: null array pod_reason", at its place in the mask order
 * -- the last.  Without that bit a null pod_reason is accepted as before. */
#define KS_AUDIT_PASS_STAGES 64u     /* ks_audit_stages_dev */
#define KS_AUDIT_PASS_REASONS 128u   /* ks_audit_reasons_dev */
#define KS_AUDIT_PASS_ALL_EX 255u
typedef struct ks_audit_gate_ex {
  uint32_t struct_size;           /* in: sizeof(ks_audit_gate_ex) as the caller was compiled */
  uint32_t passes;                /* in: KS_AUDIT_PASS_*, at least one, each of them known (above) */
  uint32_t cap_findings, pad;     /* in: records `findings` holds */
  ks_audit_finding* findings;     /* in: the caller's table, or NULL with cap_findings == 0 */
  ks_audit* first; ks_audit_topology* topology; ks_audit_spread* spread; ks_audit_firstfit* firstfit; ks_audit_limits* limits; ks_audit_hostfit* hostfit;
  const int32_t* first_pod_seq;   /* in, claimed form only: as ks_audit_gate's */
  uint32_t n_findings, truncated; /* out: as ks_audit_gate's */
  double kernel_ms, readback_ms;  /* out: as ks_audit_gate's */
  ks_audit_stages* stages;        /* in: bit 64's array of one out struct per problem.  The passes after the sixth follow here, in the order of their bits */
  ks_audit_reasons* reasons;      /* in: bit 128's */
} ks_audit_gate_ex;
int ks_audit_gate_ex_dev(ks_dev_problem* d, const ks_result* claimed /* or NULL */, ks_audit_gate_ex* gate);
int ks_audit_gate_ex_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_gate_ex* gate);
/* The gate's reduction over any table of words, so that its kernels can be tested apart from the passes: `rows` [n] (host memory) is uploaded to `device` and tallied
 * there both ways -- as a flag table (rows set, bit counts) and as a table of checked words with up to four bit fields (field_sum[i] = the sum of
 * (row >> shift[i]) & mask[i]).  All sums are modulo 2^32, as the totals' are. */
typedef struct ks_audit_fields { uint32_t n_fields; uint32_t shift[4], mask[4]; } ks_audit_fields;   /* n_fields <= 4, shift < 32 */
typedef struct ks_audit_row_totals { uint32_t n_set; uint32_t bit_count[32]; uint32_t field_sum[4]; } ks_audit_row_totals;
int ks_audit_reduce_rows(int device, const uint32_t* rows, uint32_t n, const ks_audit_fields* fields /* or NULL: none */, ks_audit_row_totals* out);

/* ---- consolidation CANDIDATES, selected and ordered on the device (deprovisioning/helpers.go:124-165,275-287 GetPodEvictionCost / disruptionCost /
 * calculateLifetimeRemaining, pdblimits.go:57-70 CanEvictPods, helpers.go:339-366 canBeTerminated / PodsPreventEviction, consolidation.go:83-104 the sort).
 * Flat arrays in, flat arrays out; three kernels (per pod, per node, rank), no host fallback.
 * Label selectors are flattened by the caller: it interns the label KEYS some PDB selector mentions (n_keys <= KS_CAND_MAX_KEYS) and, per key, the VALUES some
 * selector mentions as bits 0 .. KS_CAND_MAX_VALUES - 1; bit KS_CAND_BIT_OTHER = the pod has the key with a value no selector mentions, KS_CAND_BIT_ABSENT = the
 * pod lacks the key.  pod_val[k * n_pods + pod] is the pod's bit for key k (key-major: a wave reads it coalesced).  A PDB is a namespace id, disruptionsAllowed
 * and a CSR of (key, u64 allowed-set mask); it matches a pod iff the namespace ids are equal and (mask >> pod_val[key][pod]) & 1 for every requirement.  Only a
 * matching PDB with disruptionsAllowed == 0 blocks.
 * Per node slot: node_why (a reason the caller already decided, 0 = still in the running; KS_CAND_WHY_PDB / _DO_NOT_EVICT are the kernel's own and refused as
 * input), age in seconds, TTLSecondsUntilExpired (-1: none; 0 is refused -- the reference divides by zero there), and its pod slots in ASCENDING slot order
 * (node_pods_off / node_pods).  The disruption cost is the sum of the pods' eviction costs taken sequentially in that order as float64 -- deletion costs are
 * arbitrary doubles, so the sum depends on the order, and this is the canonical one -- times clamp(0, (ttl - age) / ttl, 1).  It is computed for nodes with
 * node_why 0 or KS_CAND_WHY_DELETING_NODE (they are in candidateNodes' result) and is 0.0 for every other code.
 * Out (caller-owned, [n_nodes] each): why (0 = candidate), detail (KS_CAND_WHY_PDB: the PDB's index -- first pod in slot order, lowest PDB index;
 * KS_CAND_WHY_DO_NOT_EVICT: the pod slot; else -1), n_node_pods, cost; order[0 .. n_candidates) = the candidates by `cost <` (so -0.0 and +0.0 tie), ties by
 * ascending node index (the stable sort over ascending index); empty[0 .. n_empty) = the candidates without pods, in the same order.
 * KS_ERR_INVALID (nothing launched, nothing written): a null array, a pod_val above 63, a requirement key >= n_keys, offsets that do not ascend, a pod slot out of
 * range / not ascending within its node / bound elsewhere according to pod_node, an unknown flag bit, a deletion cost or age that is not finite, a ttl of 0 or
 * below -1, a node_why above KS_CAND_WHY_LEFT or one of the kernel's own.  KS_ERR_UNSUPPORTED: n_keys > KS_CAND_MAX_KEYS (both counts in the message).
 * ms (may be NULL): [0] inputs up, [1] the three kernels, [2] read-back, milliseconds. */
#define KS_CAND_MAX_KEYS 16
#define KS_CAND_MAX_VALUES 62
#define KS_CAND_BIT_OTHER 62
#define KS_CAND_BIT_ABSENT 63
#define KS_CAND_POD_DO_NOT_EVICT 1u
#define KS_CAND_POD_HAS_DELETION_COST 2u
#define KS_CAND_POD_HAS_PRIORITY 4u
#define KS_CAND_WHY_DELETING_NODE 10   /* deletion timestamp set: in candidateNodes' result, filtered by canBeTerminated; its cost is still computed */
#define KS_CAND_WHY_PDB 11
#define KS_CAND_WHY_DO_NOT_EVICT 12
#define KS_CAND_WHY_LEFT 13
typedef struct ks_candidates_inputs {
  uint32_t n_pods, n_nodes, n_pdbs, n_keys;
  const int32_t* pod_node;            /* [n_pods] node slot, -1: unbound (ignored) */
  const uint32_t* pod_ns;             /* [n_pods] namespace id */
  const uint32_t* pod_flags;          /* [n_pods] KS_CAND_POD_* */
  const double* pod_deletion_cost;    /* [n_pods] read under KS_CAND_POD_HAS_DELETION_COST */
  const int32_t* pod_priority;        /* [n_pods] read under KS_CAND_POD_HAS_PRIORITY */
  const uint8_t* pod_val;             /* [n_keys][n_pods] */
  const uint32_t* pdb_ns;             /* [n_pdbs] */
  const int32_t* pdb_allowed;         /* [n_pdbs] disruptionsAllowed */
  const uint32_t* pdb_req_off;        /* [n_pdbs + 1] */
  const uint32_t* pdb_req_key; const uint64_t* pdb_req_mask;
  const uint32_t* node_why;           /* [n_nodes] */
  const double* node_age_seconds;     /* [n_nodes] */
  const int64_t* node_ttl_seconds;    /* [n_nodes] */
  const uint32_t* node_pods_off;      /* [n_nodes + 1] */
  const uint32_t* node_pods;
} ks_candidates_inputs;
typedef struct ks_candidates_outputs {
  uint32_t n_candidates, n_empty;
  uint32_t* order; uint32_t* empty; uint32_t* why; int32_t* detail; uint32_t* n_node_pods; double* cost;
} ks_candidates_outputs;
int ks_consolidation_candidates_host(const ks_candidates_inputs* in, ks_candidates_outputs* out, int device, double* ms /* [3] or NULL */);

/* ---- candidates of the other deprovisioning methods (deprovisioning/controller.go:142-162 tries them before consolidation): candidateNodes under
 * Expiration.ShouldDeprovision (expiration.go:56-58,120-127), Drift.ShouldDeprovision (drift.go:50-56) or Emptiness.ShouldDeprovision (emptiness.go:52-70), then the
 * order their ComputeCommand walks them in.  ks_consolidation_candidates_host's sibling: the same flat arrays (c), refusals and outputs; kernel ks_cand_pods is reused,
 * ks_deprov_nodes and ks_cand_order_key are the method's own.  No host fallback.
 * c.node_why carries the steps BEFORE the method's filter only: 0-7 or KS_CAND_WHY_LEFT (anything else is refused); the deletion timestamp arrives as
 * KS_DEPROV_NODE_DELETION_TIMESTAMP, because canBeTerminated runs after the filter.  c.node_ttl_seconds is the provisioner's TTLSecondsUntilExpired, read by
 * calculateLifetimeRemaining under every method and by the expiration filter.  Time is exact int64 arithmetic in unix nanoseconds: a node is expired iff
 * now > creation + ttl * 10^9, empty long enough iff now > emptiness + ttl * 10^9 (time.Time.After is strict).
 * why: c's codes 1-7, 10-13 and the method's own, with detail = the clause that decided:
 *   KS_DEPROV_WHY_NOT_EXPIRED  0 no TTLSecondsUntilExpired, 1 not after the expiration time
 *   KS_DEPROV_WHY_NOT_DRIFTED  0 drift_enabled == 0, 1 no KS_DEPROV_NODE_DRIFTED
 *   KS_DEPROV_WHY_NOT_EMPTY    0 no TTLSecondsAfterEmpty, 1 the node has pods, 2 no KS_DEPROV_NODE_HAS_EMPTINESS, 3 the ttl is not reached
 *                              (KS_DEPROV_NODE_EMPTINESS_UNPARSABLE makes the node a candidate, as the reference's parse error does)
 * Under expiration and drift a node the filter passes gets canBeTerminated's verdict (10-12) as under consolidation; under emptiness it does not
 * (Emptiness.ComputeCommand never asks).  cost: written for 0 and 10-12, 0.0 otherwise.  n_in_result: the nodes with 0 or 10-12, i.e. len(candidateNodes(...)).
 * order[0 .. n_candidates): the nodes with code 0 -- expiration: by expiration time ascending, ties by ascending slot (the stable execution of SortCandidates);
 * drift and emptiness: by ascending slot.  empty: those of them without pods, same order (under emptiness: all of them).
 * KS_ERR_INVALID beyond c's own: an unknown method or flag bit, UNPARSABLE without HAS_EMPTINESS, a ttl-after-empty below -1, either ttl above
 * KS_DEPROV_MAX_TTL_SECONDS (Go's Duration(ttl) * time.Second wraps there), a sum the method needs that overflows int64. */
#define KS_METHOD_EXPIRATION 1u
#define KS_METHOD_DRIFT 2u
#define KS_METHOD_EMPTINESS 3u
#define KS_DEPROV_WHY_NOT_EXPIRED 14
#define KS_DEPROV_WHY_NOT_DRIFTED 15
#define KS_DEPROV_WHY_NOT_EMPTY 16
#define KS_DEPROV_NODE_DELETION_TIMESTAMP 1u
#define KS_DEPROV_NODE_HAS_EMPTINESS 2u
#define KS_DEPROV_NODE_EMPTINESS_UNPARSABLE 4u
#define KS_DEPROV_NODE_DRIFTED 8u
#define KS_DEPROV_NODE_ALL 15u
#define KS_DEPROV_MAX_TTL_SECONDS 9223372036ll
typedef struct ks_deprov_inputs {
  ks_candidates_inputs c;
  uint32_t method, drift_enabled;
  int64_t now_unix_nanos;
  const uint32_t* node_dflags;                       /* [n_nodes] KS_DEPROV_NODE_* */
  const int64_t* node_creation_unix_nanos;           /* [n_nodes] */
  const int64_t* node_emptiness_unix_nanos;          /* [n_nodes] read under HAS_EMPTINESS without UNPARSABLE */
  const int64_t* node_ttl_seconds_after_empty;       /* [n_nodes] the provisioner's TTLSecondsAfterEmpty, -1: nil */
} ks_deprov_inputs;
typedef struct ks_deprov_outputs { ks_candidates_outputs c; uint32_t n_in_result, pad; } ks_deprov_outputs;
int ks_deprovisioning_candidates_host(const ks_deprov_inputs* in, ks_deprov_outputs* out, int device, double* ms /* [3] or NULL */);

/* ---- the same two calls over a second flat form of the selectors: LISTS instead of one byte per (key, pod) and one u64 mask per requirement, so that the number of
 * label keys, of values per key and of values per set is unbounded (one PDB per application, `matchLabels: {app: <name>}`, passes KS_CAND_MAX_VALUES at its 63rd
 * application).  Everything that is not a selector -- pods, nodes, costs, reasons, order, outputs, ms -- is ks_candidates_inputs / ks_deprov_inputs as above and
 * means what it means there; of `in` the fields n_keys, pod_val, pdb_req_key and pdb_req_mask are NOT read, pdb_ns / pdb_allowed / pdb_req_off are (pdb_req_off is
 * the CSR of requirements per PDB, into the req_* arrays below).  Kernel ks_cand_pods_lists takes ks_cand_pods' place; the node and rank kernels are the same.
 *   keys and values   the caller interns the label keys some selector mentions (n_keys) and, per key, the values some selector mentions: value ids
 *                     0 .. key_n_values[key] - 1; KS_CAND_VALUE_OTHER = the pod has the key with a value no selector mentions.
 *   pod side          a CSR per pod slot (pod_label_off) of (pod_label_key, pod_label_val) pairs: only the mentioned keys the pod CARRIES, in strictly ascending
 *                     key order.  A key the pod lacks is not listed.  Its size goes with the labels that matter, not with keys x pods.
 *   PDB side          per requirement req_key, req_op (KS_CAND_OP_*; matchLabels is IN with one value) and req_val[req_val_off[r] .. req_val_off[r + 1]): value ids
 *                     of that key, strictly ascending (sorted, each once).  The list is empty for EXISTS / DOES_NOT_EXIST and for them only.
 *   semantics         labels.Selector.Matches: IN present and a member; NOT_IN absent, or not a member (KS_CAND_VALUE_OTHER is never a member); EXISTS / DOES_NOT_EXIST
 *                     by presence; several requirements on one key must all hold.  A PDB matches a pod iff pdb_ns == pod_ns and every requirement holds: no
 *                     requirement matches every pod of the namespace; a nil selector is a pdb_ns no pod has.  Only a match with disruptionsAllowed == 0 blocks; per pod
 *                     the LOWEST PDB index that blocks is reported, exactly as by the narrow form.
 *   namespaces        pod_ns < n_namespaces for every bound pod slot, n_namespaces <= n_pods; a pdb_ns >= n_namespaces is a namespace without pods.  The library groups the blocking PDBs by
 *                     namespace (ascending index within one) and walks the pods through a permutation sorted by namespace: a pod meets only its own namespace's PDBs.
 * KS_ERR_INVALID (nothing launched, nothing written) beyond the narrow form's: offsets that do not start at 0 or do not ascend, a key or value id out of range, a
 * pod's keys not strictly ascending, a value list not strictly ascending, an unknown operator, an empty list under IN / NOT_IN or values under EXISTS /
 * DOES_NOT_EXIST, a bound pod's pod_ns >= n_namespaces, n_namespaces > n_pods.  No selector size is KS_ERR_UNSUPPORTED here: every count is a uint32_t and every uint32_t is accepted.
 * ms as above, with the regrouping by namespace and the packing of the lists counted in [0]. */
#define KS_CAND_VALUE_OTHER 0xFFFFFFFFu
#define KS_CAND_OP_IN 0u
#define KS_CAND_OP_NOT_IN 1u
#define KS_CAND_OP_EXISTS 2u
#define KS_CAND_OP_DOES_NOT_EXIST 3u
typedef struct ks_selector_lists {
  uint32_t n_keys, n_namespaces;
  const uint32_t* key_n_values;       /* [n_keys] */
  const uint32_t* pod_label_off;      /* [n_pods + 1] */
  const uint32_t* pod_label_key;      /* [pod_label_off[n_pods]] */
  const uint32_t* pod_label_val;      /* value id or KS_CAND_VALUE_OTHER */
  const uint32_t* req_key;            /* [pdb_req_off[n_pdbs]] */
  const uint32_t* req_op;             /* KS_CAND_OP_* */
  const uint32_t* req_val_off;        /* [pdb_req_off[n_pdbs] + 1] */
  const uint32_t* req_val;            /* [req_val_off[last]] */
} ks_selector_lists;
int ks_consolidation_candidates_lists_host(const ks_candidates_inputs* in, const ks_selector_lists* sel, ks_candidates_outputs* out, int device, double* ms /* [3] or NULL */);
int ks_deprovisioning_candidates_lists_host(const ks_deprov_inputs* in, const ks_selector_lists* sel, ks_deprov_outputs* out, int device, double* ms /* [3] or NULL */);

/* Launch-time instance-type pick of the reference's in-memory provider (cloudprovider/fake/cloudprovider.go:79-84: order the machine's
 * InstanceTypeOptions by `Offerings.Available().Requirements(reqs).Cheapest().Price`, types.go:126-145, and take the first): for problem i,
 * of new node node[i]'s InstanceTypeOptions (as left by the last ks_solve*_dev) the type whose cheapest available offering under the node's zone /
 * capacity-type requirements is cheapest -- a wave-wide arg-min over the surviving-type mask.  Ties go to the lowest instance-type index (the
 * reference's sort.Slice leaves them to pdqsort).  out_type[i] = -1 when no option has a compatible available offering; out_pair[i] is the
 * (zone, capacity-type) pair of that cheapest offering (zone_value * n_ct + ct_value), out_price[i] its price.  One launch for the batch. */
int ks_launch_pick_dev(ks_dev_problem* const* ds, uint32_t n, const uint32_t* node, int32_t* out_type, int32_t* out_pair, double* out_price);

/* instanceTypesAreSubset (deprovisioning/helpers.go:118-122; consolidation.go:177, validation.go:164): is lhs[i] (a host-held type mask of
 * ceil(T/64) words, row stride `stride_words`, e.g. a command's price-filtered replacement options) a subset of new node node[i]'s
 * InstanceTypeOptions on the device?  out[i] = 1 / 0. */
int ks_types_subset_dev(ks_dev_problem* const* ds, uint32_t n, const uint32_t* node, const uint64_t* lhs, uint32_t stride_words, uint32_t* out);

/* ---- requirement-algebra probes (one key); the same device functions the kernels use ---- */
typedef struct ks_req1 { uint64_t mask; int32_t gt, lt; uint8_t present, complement; } ks_req1;
/* value_int: [64] integer value of each universe entry or INT32_MIN.  on_device != 0 runs a 1-thread kernel. */
int ks_probe_intersection(const ks_req1* a, const ks_req1* b, const int32_t* value_int, uint32_t nvalues, int on_device, ks_req1* out);
int ks_probe_compatible(const ks_req1* a, const ks_req1* b, int well_known, const int32_t* value_int, uint32_t nvalues, int on_device, int* ok);

/* Requirement.Has over the key's universe (bit v: Has(value v)), Operator() (0 In, 1 NotIn, 2 Exists, 3 DoesNotExist), Len(), and the two
 * predicates of them the kernels branch on: nidne = operator in {NotIn, DoesNotExist}, len0 = Len() == 0 (requirement.go:171-204). */
typedef struct ks_req_facts { uint64_t has_mask; int64_t len; int32_t op; uint8_t nidne, len0; } ks_req_facts;
int ks_probe_has(const ks_req1* a, const int32_t* value_int, uint32_t nvalues, int on_device, ks_req_facts* out);

const char* ks_last_error(void); /* thread-local message of the last non-OK return */
const char* ks_version(void);
uint32_t ks_rr_run_max(void);       /* queue entries one RUN round of ks_pack_rr takes at most (the library's RR_RUN_MAX: a build-time choice, a multiple of 64) */
/* The cycle probes the library was compiled with (0: none -- the product).  ks_result.stats[12], [13], [21] and [25..31] hold another set of counters under each
 * (ks_pack_rr.inc, the end of ks_pack_rr): a profiling tool asks before it gives them names. */
#define KS_PROBE_BUILD_PROBES 1u    /* -DKS_PROBES: the phases of a normal round */
#define KS_PROBE_BUILD_WIN 2u       /* -DKS_PROBES_WIN: the head window's loop */
#define KS_PROBE_BUILD_RUN 4u       /* -DKS_PROBES_RUN: worker 1's phases of a RUN round's step */
uint32_t ks_probe_build(void);

#ifdef __cplusplus
}
#endif
#endif /* KSOLVE_H */
