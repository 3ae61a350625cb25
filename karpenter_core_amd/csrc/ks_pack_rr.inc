// ks_pack_rr.inc -- the register-resident pack kernel (included by ksolve.hip; round 4).
//
// Same Solve loop as ks_pack (scheduler.go:96-219), organised around two facts about the LEAN feature set:
//
//   1. The visiting order needs no array.  `sort.Slice(newNodes, len(Pods))` taken as a stable sort puts a node that takes
//      a pod at the FRONT of its next count bucket and a fresh node at the BACK of bucket 1; so the order is the order of the
//      keys   existing node e: e      new node: count << 22 | (count == 1 ? seq : 0x3FFFFF - seq)   (seq = commit number),
//      and "the first node in visiting order that accepts the pod" (scheduler.go:174-191) is an ARG-MIN over the accepting
//      nodes.  Every node is evaluated for every pod, one node per lane and slot; nothing moves.
//   2. What Node.Add reads of a node, besides its requests and its own hostname counters, is its requirement set -- and
//      nodes share those: the distinct sets ("node requirement classes", nrc: machine template x requirement record) are
//      few (one per template and what topology / selectors narrowed, 4 on BASELINE configs[2]).  Requirements.Compatible,
//      Topology.AddRequirements and the instance-type filter's requirement half are evaluated once per (pod class, nrc) --
//      and cached per class where no topology counter is read -- instead of once per node; the filter's resource half is
//      `requests <= per-resource maximum of the nrc's types`, exact whenever one type of the nrc holds every maximum
//      (checked when the nrc is interned; otherwise the leader runs the exact T-bit filter for the winner).
//
// One workgroup, 8 waves.  Wave 0 (the leader) owns the Solve's sequential state: the queue, topology counters, the nrc table,
// results.  Waves 1..7 (workers) hold the nodes in REGISTERS (8 node slots per lane: key, nrc, requested-resource mask,
// headroom per resource, 32 hostname counters) and do one thing per round: apply the order that precedes the evaluation
// (commit the last round's winner / a commit the leader decided / a fresh node), evaluate every node they hold against the
// round's pod, and publish their best key.  ONE barrier per round: the leader publishes the orders for round r+1 while the
// workers evaluate round r, speculating that round r's pod finds a node; everyone reads the 7 candidate keys after the barrier
// and agrees on the winner without the leader.  A pod that finds no node (a machine is opened), one whose winner needs the
// exact filter, or one whose evaluation reads a counter the unresolved pod may record into, costs an extra round.
// Nothing of the per-pod path touches L2 but the queue entry / class brief (prefetched) and two result stores.
//
// Round 5: the nodes at the front of the visiting order are LENT to the leader (the head window), which places the pods that are no plain replicas alone, barrier-free.
// Round 6: those pods reach the leader PREPARED (RRPx) -- the worker waves, which would otherwise sit at the barrier, lay down per pod and per requirement class what a
// node of that class answers (a zonal-spread pod's answers once per domain; the leader's loop only picks the domain from four counters) -- so that the leader's per-pod
// chain is the lanes' nodes against the pod, one wave minimum and the commit; and a census of the nodes whose hostname counter stands at 0 (RRLds::hz) says "nobody
// anywhere takes this anti-affinity pod" without the workers being asked.  What the measurements of the round say about sharing the leader's chain with other waves
// is written where it applies (RR_SMASK, DESIGN.md section 4.5).
//
// Problems outside what this kernel covers are DECLINED (stats[KS_STAT_ERR] = KS_RR_DECLINED, nothing of the inputs is
// modified): the host then runs ks_pack.  Covered: LEAN problems (no host ports / volumes / hostname or instance-type
// selectors / limits, R <= 4) without Gt/Lt bounds, G <= 64 groups, GH <= 32 hostname-keyed groups, K <= 16 keys, up to 64
// nrcs, 3584 nodes (existing + new), 1023 pods per node; no hostname-keyed affinity items, no node-filtered hostname-keyed
// groups.  InstanceTypeOptions are computed at the end, from each node's final nrc and requests (the filters are monotone:
// node.go:137-159 applied to the final state gives what the chain of filters gave).
#define KS_RR_DECLINED 0xDEC11EDull
// Why it declined (stats[14], ks_problem_rr_status): every code is a DECLINE -- the host runs ks_pack, which also raises the hard errors (capacity, ...) where they are real.
//   1 outside the static limits (before anything was written) | 2 more pods on a node than a key's count field holds | 3 more than 8 exact-filter exclusions for one pod |
//   4 more nodes than the workers' registers hold | 5 more requirement classes than the nrc table | 6 an anti-affinity group that does not exist yet decides the error |
//   7 a class outside the kernel's feature set reached the head of the queue | 8 the round watchdog (a protocol bug would otherwise hang the stream) | 9 max_new_nodes reached
#ifndef KS_SIM
// Within ONE wave the LDS executes its DS instructions in the order they were issued, so a lane reads what another lane of its wave wrote earlier without waiting for
// anything: the hand-off only has to keep the COMPILER from moving accesses across it (the fences of ksolve.hip's LSYNC also drain the wave's outstanding GLOBAL
// loads and stores -- a microsecond the leader does not have)
#undef LSYNC
#define LSYNC() asm volatile("" ::: "memory")
#endif
#ifdef KS_PROBES      /* per-phase cycle counters of a round (tools/phase_profile_rr.py): leader slots 0..5, worker wave 1 slots 8..12 */
#define RRP(i) do { const u64 t_ = __builtin_readcyclecounter(); rrp[(i)] += t_ - rrp_t; rrp_t = t_; } while (0)
#else
#define RRP(i) do { } while (0)
#endif
#ifndef RR_NWK
#define RR_NWK 7        /* worker waves (an experiment build may choose fewer: -DRR_NWK=3 is one wave per SIMD) */
#endif
#define RR_NW (RR_NWK + 1)
#define RR_NPL 8
#define RR_NWN RR_NWK             /* worker waves that hold nodes (all of them) */
#define RR_NODES (RR_NWN * 64 * RR_NPL)
// Where node n lives: slot n / 448, worker wave (n % 448) % 7, lane (n % 448) / 7 -- consecutive nodes on DIFFERENT waves, so that the pods of a run's step (which go to
// nodes that were opened one after the other) are committed by several waves side by side
#define RR_NODE_AT(slot, wk, ln) (((slot) * RR_NWN * 64u) + (u32)(ln) * RR_NWN + (wk))
#define RR_NODE_SLOT(n) ((n) / (64u * RR_NWN))
#define RR_NODE_WV(n) (((n) % (64u * RR_NWN)) % RR_NWN + 1u)
#define RR_NODE_LANE(n) (((n) % (64u * RR_NWN)) / RR_NWN)
#define RR_NRC 64
#define RR_GW 8
#define RR_KMAX 16
#define RR_HC_ZERO (RR_GW * 256u)          /* window hostname counters (RRLds::wn_hc, bytes): a row that is always 0 (an item that is not there) */
#define RR_HC_SINK ((RR_GW + 1u) * 256u)   /* ... and one nobody reads (a record that does not count) */
#define RR_MAXHREC 12
#define RR_MAXNREC 8
#define RR_CHILD 8
#define RR_SEQMAX 0x7FFFFu      /* a key: pods on the node << 22 | place within the count bucket << 3 | slot */
#define RR_CNTMAX 1023u

// What the leader reads of a pod class per pod: one 192-byte record (ks_build_rr, from the class plan).
struct alignas(16) RRBrief {
  i64 req[4];                   // words 0..7
  u32 prm, flags, ev, dyn1;     // 8..11   flags: 1 = the evaluation reads narrow-key topology counters (per pod, not cached) | 2 = outside this kernel | 4 = ... and its only such item is a spread
                                //          on a key the class has no requirement of its own on (dyn1 = 1 | g << 8 | key << 16 | self << 24): answered from the cached rest + the group's counts
  u64 tmask_n, rmask_n;         // 12..15  narrow-key groups (bit g) the evaluation reads / Topology.Record may update
  u32 nhost, nhrec, nnrec; i32 dyn_skew;// 16..19  (dyn1: maxSkew)
  u32 host_w[3]; i32 host_skew[3];   // 20..25  hostname-keyed items: type | self << 8 | hslot << 16 | g << 24; maxSkew
  u32 dyn_pd[2];                // 26..27  (dyn1: the pod's domains, PlanTopo::PD)
  u32 hrec[RR_MAXHREC];         // 28..39  hostname-keyed groups Topology.Record visits: hslot | g << 8 | owned_inverse << 16
  u32 nrec[RR_MAXNREC];         // 40..47  narrow-key groups it visits: g | key << 8 | type << 16 | owned_inverse << 24 | filtered << 25
};
static_assert(sizeof(RRBrief) == 192, "RRBrief layout");
// Per class, cached across pods (classes whose evaluation reads no topology counter): the answer of every nrc below n.
struct alignas(16) RRMemo { u64 acc, chg, vfy; u32 n, pad; u8 tr[64]; };      // acc: accepts | chg: the node's nrc changes (tr) | vfy: the winner needs the leader's exact check
static_assert(sizeof(RRMemo) == 96, "RRMemo layout");

__global__ __launch_bounds__(64) void ks_build_rr(const DevProb* probs) {
  const DevProb& P = probs[blockIdx.y];
  if (!P.rr_briefs) return;
  const ClsPlan* const plans = (const ClsPlan*)P.plans; const ClsBrief* const briefs = (const ClsBrief*)P.briefs; RRBrief* const out = (RRBrief*)P.rr_briefs;
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P.C) return;
  const ClsPlan& pl = plans[c]; RRBrief b; memset(&b, 0, sizeof b);
  bool bad = pl.overflow || pl.port_cnt || pl.vol_cnt || pl.hn_mode || pl.it_state != 0 || P.R > 4;
  for (u32 r = 0; r < 4; ++r) b.req[r] = r < P.R ? pl.req[r] : 0;
  b.prm = pl.reqmask; b.ev = briefs[c].ev;
  for (u32 j = 0; j < pl.ntopo; ++j) { if (pl.topo[j].g >= 64) bad = true; b.tmask_n |= 1ull << (pl.topo[j].g & 63); }
  b.nhost = pl.nhost;
  for (u32 j = 0; j < pl.nhost && j < 3; ++j) {
    const PlanTopo& t = pl.host[j];
    if (t.type == 1 || t.hslot >= 4 * RR_GW || t.g >= 64 || t.g < 0 || (t.type == 0 && (t.maxskew > 250 || t.maxskew < 0))) bad = true;
    b.host_w[j] = (u32)t.type | ((u32)t.self << 8) | ((u32)t.hslot << 16) | ((u32)(t.g & 63) << 24); b.host_skew[j] = t.maxskew;
  }
  for (u32 j = 0; j < pl.nrec; ++j) {
    const PlanRec& r = pl.rec[j];
    if (r.g < 0 || r.g >= 64) { bad = true; continue; }
    if (r.key == KS_KEY_HOSTNAME) {
      if (b.nhrec >= RR_MAXHREC || r.hslot >= 4 * RR_GW || r.filtered) { bad = true; continue; }
      b.hrec[b.nhrec++] = (u32)r.hslot | ((u32)r.g << 8) | ((u32)r.owned_inverse << 16);
    } else if (r.key >= 0 && r.key < RR_KMAX) {
      if (b.nnrec >= RR_MAXNREC) { bad = true; continue; }
      b.nrec[b.nnrec++] = (u32)r.g | ((u32)r.key << 8) | ((u32)r.type << 16) | ((u32)r.owned_inverse << 24) | ((u32)r.filtered << 25);
      b.rmask_n |= 1ull << r.g;
    } else bad = true;
  }
  if (!bad && pl.ntopo == 1 && pl.topo[0].type == 0) {
    for (u32 i = 0; i < pl.ntouch; ++i) {
      const PlanTouch& tl = pl.touch[i];
      if (tl.topo_begin == 0 && tl.topo_end == 1 && !tl.own && tl.key >= 0 && tl.key < RR_KMAX) {
        b.dyn1 = 1u | ((u32)(pl.topo[0].g & 63) << 8) | ((u32)tl.key << 16) | ((u32)pl.topo[0].self << 24); b.dyn_skew = pl.topo[0].maxskew; b.dyn_pd[0] = (u32)pl.topo[0].PD; b.dyn_pd[1] = (u32)(pl.topo[0].PD >> 32);
      }
    }
  }
  b.flags = (pl.ntopo ? 1u : 0u) | (bad ? 2u : 0u) | (b.dyn1 ? 4u : 0u);
  out[c] = b;
  // What the head window's straight-line loop reads (rr_window_fast), unpacked once: 0 simple | dyn1 << 1 ; 1, 2 hostname items: counter byte | limit << 16 (absent: the zero row,
  // never over the limit) ; 3, 4 hostname records: counter byte | group << 16 | owned inverse << 24 | there << 25 ; 5 the narrow record: group | key << 8 | there << 16
  if (P.rr_hot) {
    u32 h[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool simple = !bad && (!(b.flags & 1u) || b.dyn1) && b.nhost <= 2 && b.nhrec <= 2 && b.nnrec <= 1;
    for (u32 j = 0; j < 2; ++j) {
      u32 off = RR_HC_ZERO, lim = 0x7FFFu;
      if (j < b.nhost) { const u32 hw = b.host_w[j], hs = (hw >> 16) & 0xFFu; off = (hs >> 2) * 256u + (hs & 3u); lim = (u32)((hw & 0xFFu) == 0 ? b.host_skew[j] - (i32)((hw >> 8) & 0xFFu) : 0) & 0xFFFFu; }
      h[1 + j] = off | (lim << 16);
    }
    for (u32 j = 0; j < 2; ++j) if (j < b.nhrec) { const u32 w = b.hrec[j], hs = w & 0xFFu; h[3 + j] = ((hs >> 2) * 256u + (hs & 3u)) | (((w >> 8) & 63u) << 16) | (((w >> 16) & 1u) << 24) | (1u << 25); }
    if (b.nnrec == 1) { const u32 w = b.nrec[0]; if (((w >> 16) & 0xFFu) == 2u || ((w >> 24) & 3u)) simple = false; h[5] = (w & 0xFFFFu) | (1u << 16); }
    h[0] = (simple ? 1u : 0u) | (b.dyn1 ? 2u : 0u);
    for (int i = 0; i < 8; ++i) P.rr_hot[(size_t)c * 8 + i] = h[i];
  }
}

// Requirement classes: what the per-(class, nrc) answers depend on -- tolerations, the class's own requirements, its narrow-key topology items (for a
// dyn1 class: only that it is one; its spread is applied per pod from the brief) -- not its requests, hostname items or what it records.  Classes of
// one requirement class share one set of cached answers (rr_memo row of the first class interned): BASELINE configs[2] has 3 359 classes and a few dozen of these.
__device__ inline bool ks_rr_same(const ClsPlan& a, const ClsPlan& b, const u32 da, const u32 db) {
  if (a.tol != b.tol || a.present != b.present || a.complement != b.complement || a.it_state != b.it_state || a.ntouch != b.ntouch || a.tkeys != b.tkeys || (da != 0) != (db != 0)) return false;
  for (u32 i = 0; i < a.ntouch; ++i) { const PlanTouch& x = a.touch[i]; const PlanTouch& y = b.touch[i]; if (x.mask != y.mask || x.gt != y.gt || x.lt != y.lt || x.key != y.key || x.own != y.own || x.complement != y.complement || x.topo_begin != y.topo_begin || x.topo_end != y.topo_end) return false; }
  if (da) return true;
  if (a.ntopo != b.ntopo) return false;
  for (u32 j = 0; j < a.ntopo; ++j) { const PlanTopo& x = a.topo[j]; const PlanTopo& y = b.topo[j]; if (x.PD != y.PD || x.g != y.g || x.maxskew != y.maxskew || x.type != y.type || x.self != y.self || x.pod_has != y.pod_has) return false; }
  return true;
}
__device__ inline u64 ks_rr_hash(const ClsPlan& a, const u32 da) {
  u64 h = 0x9E3779B97F4A7C15ull;
  auto mix = [&](const u64 v) { h ^= v; h *= 0x9FB21C651E98DF25ull; h ^= h >> 29; };
  mix(a.tol); mix(a.present); mix(a.complement); mix((u32)a.it_state); mix(a.ntouch); mix(a.tkeys); mix(da ? 1 : 0);
  for (u32 i = 0; i < a.ntouch; ++i) { const PlanTouch& x = a.touch[i]; mix(x.mask); mix((u32)x.key | ((u32)x.own << 8) | ((u32)x.complement << 16) | ((u32)x.topo_begin << 20) | ((u32)x.topo_end << 26)); }
  if (!da) { mix(a.ntopo); for (u32 j = 0; j < a.ntopo; ++j) { const PlanTopo& x = a.topo[j]; mix(x.PD); mix((u32)x.g | ((u32)x.type << 16) | ((u32)x.self << 20) | ((u32)x.pod_has << 24)); mix((u32)x.maxskew); } }
  return h ^ (h >> 32);
}
__global__ __launch_bounds__(64) void ks_link_rr(const DevProb* probs) {
  const DevProb& P = probs[blockIdx.y];
  if (!P.rr_briefs || !P.rr_tab) return;
  const ClsPlan* const plans = (const ClsPlan*)P.plans; const RRBrief* const rb = (const RRBrief*)P.rr_briefs; u32* const tab = P.rr_tab; const u32 tab_size = P.ev_tab_size;
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P.C) return;
  const ClsPlan& me = plans[c]; const u32 dme = rb[c].dyn1;
  u32 slot = (u32)ks_rr_hash(me, dme) & (tab_size - 1), rep = c;
  for (u32 probes = 0; probes < tab_size; ++probes, slot = (slot + 1) & (tab_size - 1)) {
    const u32 prev = atomicCAS(&tab[slot], 0u, c + 1);
    if (prev == 0) { rep = c; break; }
    if (ks_rr_same(plans[prev - 1], me, rb[prev - 1].dyn1, dme)) { rep = prev - 1; break; }
  }
  P.rr_mi[c] = rep;
}

// Base classes: classes that share their cached answers (rr_mi) AND their requests -- what the resource / requirement half of an evaluation reads -- and carry at most two
// hostname-keyed items.  Consecutive pods of one base class form a RUN: evaluated once for that half, their hostname item applied per pod.  The id (a class index) goes
// into the brief's word 27 (dyn_pd[1], unused by classes that are not dyn1; dyn1 classes never run).
__global__ __launch_bounds__(64) void ks_link_rr2(const DevProb* probs) {
  const DevProb& P = probs[blockIdx.y];
  if (!P.rr_briefs || !P.rr_tab2) return;
  RRBrief* const rb = (RRBrief*)P.rr_briefs; u32* const tab = P.rr_tab2; const u32 tab_size = P.ev_tab_size;
  const u32 c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= P.C) return;
  const RRBrief& me = rb[c];
  if (me.dyn1) return;
  u32 rep = c;
  if (me.nhost <= 2 && !(me.flags & 3u)) {
    const u32 mi = P.rr_mi[c];
    u64 h = 0x9E3779B97F4A7C15ull ^ mi;
    for (int r = 0; r < 4; ++r) { h ^= (u64)me.req[r]; h *= 0x9FB21C651E98DF25ull; h ^= h >> 29; }
    h ^= me.prm; h *= 0xD6E8FEB86659FD93ull; h ^= h >> 32;
    u32 slot = (u32)h & (tab_size - 1);
    for (u32 probes = 0; probes < tab_size; ++probes, slot = (slot + 1) & (tab_size - 1)) {
      const u32 prev = atomicCAS(&tab[slot], 0u, c + 1);
      if (prev == 0) { rep = c; break; }
      const RRBrief& o = rb[prev - 1];
      if (P.rr_mi[prev - 1] == mi && o.req[0] == me.req[0] && o.req[1] == me.req[1] && o.req[2] == me.req[2] && o.req[3] == me.req[3] && o.prm == me.prm) { rep = prev - 1; break; }
    }
  }
  rb[c].dyn_pd[1] = rep;
}

// The nrc table (LDS, structure of arrays: lane = nrc reads are conflict free).
struct RRNrc {
  u64 taints[RR_NRC]; u32 present[RR_NRC], complement[RR_NRC]; i32 tmpl[RR_NRC]; i32 it[RR_NRC]; u32 dominant[RR_NRC];
  u64 mask[RR_KMAX][RR_NRC];
  i64 cap[4][RR_NRC];                       // per-resource maximum Allocatable over the nrc's instance types (new-node nrcs)
  u8 child[RR_CHILD][RR_NRC]; u32 cdiff[RR_CHILD][RR_NRC]; u32 nchild[RR_NRC];      // cache of transitions: child id / the keys on which it differs from this nrc
  u64 nmask[RR_KMAX]; u64 ntaints; u32 npresent, ncomplement; i32 ntmpl, nit;       // a candidate record being interned
};
struct RRCand { u64 kp; i64 room[4]; u64 meta; };     // a worker wave's best candidate: key << 32 | nrc << 16 | node, the node's headroom, its nrc | requested-resource mask << 8
#define RR_STEP (RR_NWK * 8u)     /* pods a run's step places at most (each worker wave publishes up to 8 keys) */
#define RR_B 8          /* pods per round */
#define RR_RING 32      /* class records (brief + cached answers) of queue entries, by queue index */
// One pod of a run: what differs between pods of one evaluation class -- the pod itself and the hostname-keyed groups Topology.Record counts it into
// (its hostname-keyed ITEMS are in RRLds::runitem: every wave reads those at every step)
struct alignas(8) RRRunPod { u32 pod, cls, nh; u8 hs[12]; };
static_assert(sizeof(RRRunPod) == 24, "RRRunPod layout");      // (the committing wave reads it as six words, lane i: word i)
#ifndef RR_RUN_MAX
#define RR_RUN_MAX 256u /* queue entries a RUN round takes at most: the leader looks at the queue 64 entries (one lane each) at a time, up to this many */
#endif
static_assert(RR_RUN_MAX >= 64u && RR_RUN_MAX % 64u == 0u, "a run's tables are filled 64 entries at a time");
struct alignas(16) RRCtl { u32 hdr[32]; u32 create[24]; u32 pbrief[48]; u32 pad[8]; };      // create: key | rm | room[4] (8 words) | hc[8]
// A queue entry prepared for its round: w[0..47] the class brief | w[48] stream position | w[49] class | w[50] pod | w[51] hostname records that count |
// w[52] requeued unrelaxed; m[0..23] what every nrc answers (RRMemo image: acc[2] | chg[2] | vfy[2] | n | pad | child[64 bytes])
struct alignas(16) RREntry { u32 w[64]; u32 m[32]; u32 t1[32]; };
// A pod PREPARED for the head window's loop (round 6): what rr_window_fast needs of the pod at stream position u[0], worked out by the worker waves (rr_px_static; they would
// otherwise sit at the barrier) from the class record and the cached answers, a few pods ahead, while the leader still places the pods before it.
//   u[0] stream position (written last) | u[1] flags (RR_PX_*) | u[2] the size of the nrc table it was made for
//   u[4..11] requests | u[12], u[13] hostname items: counter byte | limit << 16 | u[14] hostname records: counter byte (or the sink) | second << 16 | u[15] pod
//   u[16] requested-resource mask | dyn1 group << 8 | narrow record's group << 16 | u[17] base class of a plain replica (all ones: not one)
//   u[20..22] dyn1: the pod's own count (self) | maxSkew | the pod's domains
//   t[n]: what a node of requirement class n answers: the nrc it would have | accepts << 8 | needs the exact filter << 9 | not answered here << 10 | the narrow record
//   counts << 11 | ... into domain << 12 | dyn1: the domains (0..3) the class's requirement on the spread's key allows << 18 -- for a dyn1 pod all of this WITHOUT the spread
//   td[n * 4 + d] dyn1: ... and with the node's requirement on the key narrowed to domain d: nrc (6 bits) | not answered here << 6 | needs the exact filter << 7 |
//   the narrow record counts << 8 | ... into domain << 9.  Which d: nextDomainTopologySpread on the group's counters as they stand when the pod's turn comes -- the one
//   piece the leader's loop works out itself, per lane, from four counters (a group with a fifth registered domain is not answered here).
#define RR_PX 16u       /* ring of prepared pods: ten more slots than the workers run ahead, so that a wave would have to stall for ten pods' time in the middle of an entry for another to start on the slot's next tenant */
#define RR_PXA 6u       /* the workers keep the class records and the static parts of that many queue entries prepared ahead of the leader */
#define RR_PX_GO 1u
#define RR_PX_DYN 2u
#define RR_PX_CHG 4u    /* the class changes some nrc: the commit looks the capacity difference up */
#define RR_PX_STOP7 8u  /* not a pod of the straight-line loop: rr_window_gen's */
#define RR_PX_TWICE 16u /* its two hostname records count into one counter */
#define RR_PX_HREC 32u  /* some hostname record of the pod counts */
#define RR_PX_PLAIN 128u /* (the loop's control word only) the eighth plain replica of one base class in a row */
struct alignas(16) RRPx { u32 u[24]; u32 t[64]; u16 td[256]; };
struct alignas(16) RRLds {
  DevProb P; DevState S; FastTabs ft; LeaderShared ls; WaveShared sh; RRNrc nt;
  RRCtl ctl[2];                             // the orders of a round (by round parity)
  u64 win[2][RR_B];                         // per pod of the round: min over the workers of key << 32 | ambiguous << 31 | nrc << 16 | node
  u64 stepk[2][RR_NWK][8];                  // a run's step: per worker wave its accepting keys of one count bucket, at most eight (key << 32 | "the wave holds more" << 31 | nrc << 16 | node; all ones: none), by step parity
  u64 runitem[2][RR_RUN_MAX];               // ... and their hostname-keyed items (RR_ITEM_LIM), apart: every wave reads them at every step, lane = pod
  RRRunPod runtab[2][RR_RUN_MAX];           // a run's pods (by round parity: the workers still commit a round's last step while the leader forms the next round)
  u32 mrg_out[64], mrg_k[4];                // ... and what the leader's out-of-line copy hands back: the winners' payloads, kind | stop node | stop nrc
  u64 mrg[RR_NW][64];                       // rr_step_merge's scratch, one row per wave
  u32 runres[RR_RUN_MAX];                   // ... and where they went: child nrc << 16 | node
  RRCand ask;                               // the node the exact filter is asked about, as its owner holds it
  RREntry ring[RR_RING];
  u8 en_nrc[64]; u8 pkch[RR_B < 4 ? 4 : RR_B]; u32 scratch[64];
  u64 dy_nd[2][RR_NRC]; u64 vpair[RR_NRC]; u32 dynk[2];      // per nrc, for the head window's dyn1 answers: the domains its requirement on dyn key s allows (0: the key is a custom label the record does not define) | bit c: the transition to nrc c needs the exact filter | the dyn keys
  u8 t2[2][RR_NRC][64];                     // dyn1: nrc with key dynkey[s] narrowed to In [d] -> nrc (0xFF: not met yet)
  u64 lst[32], wst[16];                     // the leader's statistics / worker 1's probe counters, for the kernel's epilogue
  u32 n_nrc, staged_cls;                    // the nrc table's size; the class plan staged in sh.cls (leader and its out-of-line helpers)
  // The leader's HEAD WINDOW (round 5): the nodes at the front of the visiting order, lent by the workers -- place = worker wave * 8 + rank, the wave's 8 smallest
  // keys in order -- and the machines opened meanwhile (places 56..63), as a structure of arrays (lane = place).  Published by the workers, read by the leader,
  // written back by the leader at the end of the phase, read back by the owners at the next round's B1.
  u32 wn_key[64], wn_own[64], wn_meta[64]; u32 wn_hc[RR_GW + 2][64]; i64 wn_room[4][64];
  u32 wn_cut[8];                            // per worker wave: every key it holds and has not published is >= this
  u32 wn_qn, wn_qp, wn_qdone, wn_fn, wn_fnode, wn_fplace, wn_fdone, wn_pad2; u64 wq_win, wq_pad3;      // a question to the workers while the window stands: number / stream position of the pod / waves that have answered | a node to hand over: number / node / window place / done | the least accepting key among the nodes the workers hold (key << 32 | nrc << 16 | node)
  u32 wn_done, wn_qpos, wq_base, wq_head, wq_len, wq_pad; u64 wq_gam;      // while a window phase stands the workers keep class records prepared ahead of the leader: over / the leader's stream position | the phase's first position, queue index, queue length, the groups that exist
  u32 wn_mode, wn_pad;                      // (by the leader, before B0) 1: the workers lend their front nodes before the next round
  u32 wbrk[8];
  i32 hz[32];          // per hostname-keyed group (by its counter slot): the nodes whose counter stands at 0 -- a pod that needs a counter of 0 there and finds this at 0 is taken by no node anywhere (the workers are not asked: a machine at once).  Up by one per group that exists when a machine is opened (and per existing node at the start), down by one whenever a record takes a counter from 0 to 1 -- by whoever holds the node
  RRPx px[RR_PX];      // the pods prepared ahead of the leader's window loop || (older text:) per narrow-key group: records counted by the loop (a prepared dyn1 pod is as old as its group's version) | bumped by the leader whenever its tables may have changed under the prepared pods
  u32 wres[32][4]; u64 wsink[8]; u64 wsinkl[3][64];      // rr_window_fast: the results of the last pods (pod, node, commit number), flushed 32 at a time | where the stores of the lanes that are not the winner go | ... and the atomics of a record that does not count, a word PER LANE: 63 atomics on one LDS address are taken one after the other (664 against 208 cycles for the four of a narrow record, profiles/r06_pipe_costs.txt) | where the atomics of a record that does not count go
  u32 wstop[8]; u64 wpr[8];                 // rr_window: why the phases ended (by code) | (KS_PROBES) its cycle counters
  u32 wx[16]; u64 wx_gam, wx_act;           // leader <-> rr_window: queue head / stream position / length / commit number / pods placed / nrcs / T / fresh places / dyn keys / why it stopped; groups that exist; places that hold a node
  u32 init_err, fin[4];                     // words of their own: read by every wave after a barrier while the leader may already be writing scratch again
};
// ctl header words
#define RRH_PRE 0       /* 0 none | 2 commit pre_node | 3 create pre_node */
#define RRH_PNODE 1
#define RRH_PNRC 2
#define RRH_NB 3
#define RRH_SEQ 4
#define RRH_NSLOTS 5
#define RRH_PSEQ 6
#define RRH_PHMASK 7
#define RRH_NEXCL 8
#define RRH_EXIT 9
#define RRH_EXCL 10     /* 10..13: up to 8 excluded nodes, 16 bits each */
#define RRH_NB2 17      /* 17, 18 (by the parity of the pick): pods in the batch | same << 8, as of that pick's barrier -- pods join a running round */
#define RRH_RUN 16      /* > 0: the round is a RUN of that many pods of one evaluation class (no topology counters read): picked several per barrier */
#define RRH_SAME 15     /* bit j: pod j of the round is evaluated like pod j - 1 (same evaluation class, no topology counters read) */
#define RRH_POS 14      /* stream position of the round's first pod: its class record is ring[pos & (RR_RING - 1)] */
#define RRH_HINT 20     /* 1: a window phase follows this round (unless the leader decides otherwise): the workers prepare class records for it at the round's end */
#define RRH_QH 21       /* ... queue index of the round's first pod | 22: queue length with it | 23, 24: the groups that exist */
#define RRH_QL 22
#define RRH_GAM 23
#define RRH_RET 19      /* != 0: the leader's window hands its nodes back (RRLds::wn_*): 1 | fresh machines << 8 */
#ifndef RR_RUN_KEEP
#define RR_RUN_KEEP 3u  /* a run whose steps placed fewer pods than this on average hands the stretch back to the head window */
#endif
#ifndef RR_WIN_PLAIN
#define RR_WIN_PLAIN 8u /* that many plain replicas in a row end the window phase for RUN rounds */
#endif
#ifdef KS_SIM
#define RR_POLL_PAUSE() ks_sim::yield()
#define RR_LDS_LOAD(p) (*(volatile const u32*)(p))
#define RR_LDS_STORE(p, v) (*(volatile u32*)(p) = (v))
#else
#ifndef RR_SLEEP
#define RR_SLEEP 4
#endif
#define RR_POLL_PAUSE() __builtin_amdgcn_s_sleep(RR_SLEEP)
/* a word another wave writes / reads with no barrier in between: relaxed workgroup-scope atomics stay DS instructions (a volatile access through a cast becomes a FLAT one with a full wait) */
#define RR_LDS_LOAD(p) __hip_atomic_load((p), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#define RR_LDS_STORE(p, v) __hip_atomic_store((p), (v), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)
#endif
#ifdef KS_SIM
#define RR_SPIN_PAUSE() ks_sim::yield()
#else
#ifndef RR_SPIN_SLEEP
#define RR_SPIN_SLEEP 1
#endif
#define RR_SPIN_PAUSE() __builtin_amdgcn_s_sleep(RR_SPIN_SLEEP)
#endif
// A flag another wave published has been seen: what it stands for is read behind this.  (Within one wave the LDS executes its accesses in order and the producers write
// payload before flag, so the hardware needs nothing; the fence is for the COMPILER's benefit and costs one wait -- on the rare hand-offs only.  The leader's loop reads
// a prepared pod's stream position first and everything else behind it in ONE batch of loads, without a wait in between: that is its per-pod chain.)
#ifdef KS_SIM
#define RR_ACQUIRE() do { } while (0)
#else
#define RR_ACQUIRE() __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup")
#endif
#ifdef KS_SIM
#define RR_KEEP(v) do { } while (0)
#else
#define RR_KEEP(v) asm volatile("" : "+v"(v))      /* the value in its register HERE: a load is not moved behind this point */
#endif
#define RR_SPIN_MAX 400000u      /* the leader's wait for a prepared pod is bounded: behind it the pod is a round's (stop code 2), as it would be without the prepared pods */
// why a head-window phase ended (statistics; slot 25 of the kernel's figures, 12 bits each): 0 a stretch of plain replicas | 1 the loop's own stop (exact filter, the leader's business, the queue) |
// 2 the eight spare places are taken | 3 a pod that reads topology counters and nothing in the window takes | 4 no template works
// (slot 31, 16 bits each: machines opened by a ROUND for a pod that reads no topology counter | ... for one that does)
#define RR_BRK(i) do { if (lane == 0) L.wbrk[(i)] += 1; } while (0)
#ifndef RR_SMASK
#define RR_SMASK 0x77u   /* the worker waves (bit = wave - 1) that keep the class records and static parts prepared: all but wave 4, which shares the leader's SIMD (every instruction it issues there lengthens the leader's chain: 105.3 ms with it, 102.5 without) */
#endif
#ifndef RR_LPW
#define RR_LPW 8u       /* every worker wave lends its RR_LPW smallest keys */
#endif
#define RR_WLENT (RR_NWK * RR_LPW)      /* window places that hold lent nodes (56); the rest of the 64 -- the spare places -- take the machines opened and the nodes taken over while the window stands */
#define RR_WSPARE (64u - RR_WLENT)

// Node.Add up to the instance-type filter for ONE nrc per lane, without the per-node parts (resources, hostname counters):
// Taints.Tolerates, Requirements.Compatible + Add of the pod's own requirements, Topology.AddRequirements on the narrow keys and
// the Compatible + Add of its result (node.go:62-90; the same steps as eval_node above, read from the nrc table).  MERGED: the
// pod's own requirements are already folded into the record (a fresh node's template∩class record).
// Returns 2 (reaches the filter), 0 (refused before the topology step), or -KS_WHY_* (topology).
template <bool MERGED>
__device__ __forceinline__ int rr_eval(const Tabs& tb, WaveShared& sh, const RRNrc& nt, const u32 ni, const int lane, const ClsRT<4>& cr, const bool skip_topo, u32& tpres, u32& tcomp, u32& tchg) {
  const ClsPlan& c = sh.cls;
  tpres = 0; tcomp = 0; tchg = 0;
  if (nt.taints[ni] & ~cr.tol) return 0;
  const u32 present = nt.present[ni], complement = nt.complement[ni];
  for (u32 i = 0; i < cr.ntouch; ++i) {
    const PlanTouch& tl = c.touch[i]; const int k = (int)((u32)(cr.tkeys >> (5 * i)) & 31u);
    KReq a; a.present = (present >> k) & 1u; a.complement = (complement >> k) & 1u; a.mask = nt.mask[k][ni]; a.gt = KS_NOGT; a.lt = KS_NOLT;
    const KReq orig = a;
    const i32* vi = tb.value_int + k * 64; const u32 nv = tb.key_nvalues[k];
    if (tl.own && !MERGED) {
      KReq b; b.present = true; b.complement = tl.complement; b.mask = tl.mask; b.gt = KS_NOGT; b.lt = KS_NOLT;
      if (!a.present) { if (!((tb.wellknown >> k) & 1u) && !kreq_nidne(b)) return 0; a = b; }     // "label does not have known values"
      else {
        const KReq mg = kreq_intersect(b, a, vi, nv);
        if (kreq_len0(mg) && !(kreq_nidne(b) && kreq_nidne(a))) return 0;
        a = mg;
      }
    }
    if (!skip_topo && tl.topo_end > tl.topo_begin) {
      const KReq before = a;
      const KReq nd = before.present ? before : kreq_exists();
      const u64 ND = kreq_has_mask(nd, vi, nv);
      u64 dom = ~0ull; bool constrained = false;
      for (u32 j = tl.topo_begin; j < tl.topo_end; ++j) {
        const PlanTopo& tg = c.topo[j]; const TopoDyn& d = sh.dyn[j]; u64 options = 0;
        if (d.reg == 0 && d.pos == ~0ull) continue;
        constrained = true;
        if (tg.type == 0) {                                       // spread: nextDomainTopologySpread, topologygroup.go:155-182
          i32 best = INT32_MAX; int bestv = -1;
          for (u64 bits = d.reg & ND; bits; bits &= bits - 1) {
            const int dd = __builtin_ctzll(bits);
            const i32 cnt = tb.gcnt[(size_t)tg.g * 64 + dd] + tg.self;
            if ((i64)cnt - (i64)d.minc <= (i64)tg.maxskew && cnt < best) { best = cnt; bestv = dd; }
          }
          if (bestv >= 0) options = 1ull << bestv;
        } else if (tg.type == 1) {                                // affinity: nextDomainAffinity :202-233
          options = d.reg & tg.PD & d.pos;
          if (!options && tg.self) {
            KReq pd = kreq_exists();
            if (tg.pod_has) { pd.present = true; pd.complement = tl.complement; pd.mask = tl.mask; pd.gt = KS_NOGT; pd.lt = KS_NOLT; }
            const u64 I = kreq_has_mask(kreq_intersect(pd, nd, vi, nv), vi, nv);
            const u64 x = d.reg & I, y = d.reg & tg.PD;
            if (x) options |= x & (~x + 1);
            if (y) options |= y & (~y + 1);
          }
        } else options = d.reg & tg.PD & ~d.pos;                  // anti-affinity :235-243
        if (!options) return -KS_WHY_TOPOLOGY;                    // "unsatisfiable topology constraint"
        dom &= options;
      }
      if (constrained) {
        const KReq in = kreq_in(dom);
        if (!before.present) { if (!((tb.wellknown >> k) & 1u)) return -KS_WHY_TOPOLOGY_REQS; a = in; }
        else { const KReq mg = kreq_intersect(in, before, vi, nv); if (kreq_len0(mg) && !kreq_nidne(before)) return -KS_WHY_TOPOLOGY_REQS; a = mg; }
      }
    }
    if (a.present) tpres |= 1u << i;
    if (a.complement) tcomp |= 1u << i;
    if (kreq_differs(a, orig)) tchg |= 1u << i;
    sh.la_mask[i][lane] = a.mask;
  }
  return 2;
}

// What both roles derive from the descriptors in LDS (wave-uniform; no side effects)
#define RR_CTX \
  RRLds& L = g_rr_lds; \
  const DevProb& P = L.P; const DevState& S = L.S; WaveShared& sh = L.sh; RRNrc& nt = L.nt; LeaderShared& ls = L.ls; FastTabs& ft = L.ft; \
  Tabs tb; \
  tb.K = UF(P.K); tb.R = UF(P.R); tb.T = UF(P.T); tb.TW = UF(P.TW); tb.GH = UF(P.GH); tb.E = UF(P.E); tb.S = UF(P.S); tb.SC = UF(P.SC); tb.n_ct = UF(P.n_ct); tb.wellknown = UF(P.wellknown_mask); tb.key_zone = (i32)UF(P.key_zone); tb.key_ct = (i32)UF(P.key_ct); \
  tb.q = (GA u64*)UF64((u64)S.q); tb.pod_node = (GA i32*)UF64((u64)S.pod_node); tb.pod_seq = (GA i32*)UF64((u64)S.pod_seq); \
  tb.rec = (GA u8*)UF64((u64)S.rec); tb.rec_stride = UF(S.rec_stride); tb.hcnt = (GA i32*)UF64((u64)S.hcnt); tb.n_alive = (GA u64*)UF64((u64)S.n_alive); tb.ge_rows = (const GA u64*)UF64((u64)P.ge_rows); \
  const u32 nP = UF(P.P), nM = UF(P.M), nC = UF(P.C), nG = UF(P.G), nMAX = UF(P.NMAX), nE = tb.E, nK = tb.K, nR = tb.R, nTW = tb.TW; \
  i64* const ge = (i64*)ks_dyn_lds; const u32 gs = UF(P.ge_max); \
  tb.key_nvalues = ft.key_nvalues; tb.value_int = ft.value_int; tb.its_fail = ft.its_fail; tb.its_inter = ft.its_inter; \
  tb.gcnt = ft.gcnt; tb.g_reg = ft.g_reg; tb.g_pos = ft.g_pos; tb.g_active = ft.g_active; tb.g_hpos = ft.g_hpos; tb.g_hzero = ft.g_hzero; tb.ge_cnt = ft.ge_cnt; tb.ge_vals = ge; tb.ge_stride = gs; \
  const GA ClsPlan* const plans = (const GA ClsPlan*)UF64((u64)P.plans); \
  const GA u32* const rrb = (const GA u32*)UF64((u64)P.rr_briefs); \
  GA u32* const rrm = (GA u32*)UF64((u64)P.rr_memo); \
  GA u64* const rr_types = (GA u64*)UF64((u64)P.rr_types); \
  const GA u32* const rr_mi = (const GA u32*)UF64((u64)P.rr_mi); \
  (void)sh; (void)nt; (void)ls; (void)nP; (void)nM; (void)nC; (void)nG; (void)nMAX; (void)nK; (void)nR; (void)nTW; (void)plans; (void)rrb; (void)rrm; (void)rr_types; (void)rr_mi; (void)ge; (void)gs

__shared__ RRLds g_rr_lds;      // the workgroup's LDS (one workgroup per Solve); file scope so that the leader's and the workers' code can be separate functions,
                                // each with its own register allocation

// A run's pods share the resource / requirement half of their evaluation; their hostname-keyed items (at most two) may differ from pod to pod.  The pods from `done` on
// that carry the same items (RRLds::runitem, packed: RR_ITEM_LIM) are picked together: returns how many, and the items.
__device__ __forceinline__ u32 rr_run_group(const u64* items, const int lane, const u32 done, const u32 rem, u32& item0, u32& item1) {
  const bool in = (u32)lane < rem;
  const u64 ab = in ? items[done + lane] : 0ull;
  const u32 a = (u32)ab, b = (u32)(ab >> 32);
  item0 = RL(a, 0); item1 = RL(b, 0);
  const u64 diff = ~ballot64(in && a == item0 && b == item1);
  return diff ? (u32)__builtin_ctzll(diff) : 64u;
}
// a packed hostname item (RRLds::runitem): present << 31 | (limit & 0x1FF) << 16 | bit shift << 8 | counter word
#define RR_ITEM_LIM(p) ((i32)(((p) >> 16) & 0x1FFu) - (i32)((((p) >> 16) & 0x100u) << 1))

// A run's step, as every wave sees it after the barrier: the smallest accepting keys over the worker waves, in order, as long as they lie in ONE count bucket
// (the nodes that take a pod move to the next bucket, behind everything in this one: the pods of the step go to these keys in order, whatever the
// commits do), at most `rem`.  An existing node keeps its place when it takes a pod: a step that starts with one ends with it.  Lane j ends up holding
// winner j (o_key / o_pay = nrc << 16 | node); o_rank: lane l's published key (wave l / 8, its l % 8-th) is the o_rank-th smallest -- a winner iff o_rank < the return value.
// Returns the number of winners; kind = why the pod AFTER them stops the run (0: nothing does).
// What a wave publishes (rr_worker): up to eight entries key << 32 | flag << 31 | nrc << 16 | node, the rest all ones, in NO particular order among themselves.  A wave
// that holds at most eight accepting keys of its bucket publishes every one (each lane writes its own, at the place the ballots give it); one that holds more publishes
// its eight smallest and sets the FLAG on the eighth, the largest of them: behind that key the wave may hold keys smaller than what the other waves have left, so the step
// ends with it.  A wave whose smallest key is an existing node's publishes that one alone.  Every prefix of the merged order is exact; the flag only ends it early.
// By RANK (round 5) -- every lane counts the published keys below its own (56 compares against LDS broadcasts), the keys go to their ranks through the wave's scratch, and
// the stopping rules are ballots over the sorted lanes: about 2 450 cycles a step for a worker wave on config #3 (2 125 steps of 26.8 pods; profiles/r23_run_steps.txt), beside
// about 2 150 to publish, 1 750 at the barrier and 2 000 to commit and evaluate again.  `scratch`: 64 words of this wave's own.
__device__ __forceinline__ u32 rr_step_merge(const u64 (*stepk)[8], u64* const scratch, const int lane, const u32 rem, const u32 nE, const u64 vfy, u32& o_key, u32& o_pay, u32& kind, u32& stop_node, u32& stop_nrc, u32& o_rank) {
  const u64 v = (u32)lane < RR_NWK * 8u ? stepk[lane >> 3][lane & 7] : ~0ull;
  const u32 key = (u32)(v >> 32);
  const bool valid = key != 0xFFFFFFFFu;
  o_key = 0xFFFFFFFFu; o_pay = 0; kind = 0; stop_node = 0xFFFFFFFFu; stop_nrc = 0;
  u32 rank = 0;
  { const u32* const kw = (const u32*)&stepk[0][0];      // (key m is word 2m + 1; the keys are unique: count << 22 | place << 3 | slot)
#pragma unroll 4
    for (u32 m = 0; m < RR_NWK * 8u; ++m) rank += kw[2u * m + 1u] < key ? 1u : 0u; }
  o_rank = valid ? rank : 64u;
  const u32 nvalid = (u32)__builtin_popcountll(ballot64(valid));
  if (rem == 0) return 0;
  if (nvalid == 0) { kind = 2; return 0; }
  if (valid) scratch[rank] = v;      // (bit 31, set by the wave that published it: its eighth and largest key, and the wave holds more in this bucket -- smaller, maybe, than what the others have left)
  LSYNC();
  const bool in = (u32)lane < nvalid;
  const u64 sv = in ? scratch[lane] : ~0ull;
  LSYNC();
  const u32 skey = (u32)(sv >> 32), spay = (u32)sv & 0x7FFFFFFFu, node = spay & 0xFFFFu, nrc = (spay >> 16) & 0xFFu;
  const u32 b0 = RL(skey, 0) >> 22;
  const bool h_b = (skey >> 22) != b0, h_c = node >= nE && (skey >> 22) >= RR_CNTMAX, h_v = ((vfy >> nrc) & 1ull) != 0;
  const u64 hb = ballot64(in && (h_b || h_c || h_v)), sb = ballot64(in && (node < nE || (((u32)sv >> 31) & 1u)));
  const u64 cb = ballot64(in && !h_b && h_c), vb = ballot64(in && !h_b && !h_c && h_v);
  const u32 cap = min(min((u32)RR_STEP, rem), nvalid);
  u32 n = cap;
  bool by_hard = false;
  if (hb) { const u32 t = (u32)__builtin_ctzll(hb); if (t < n) { n = t; by_hard = true; } }
  if (sb) { const u32 t = (u32)__builtin_ctzll(sb) + 1u; if (t <= n) { if (t < n || by_hard) by_hard = false; n = min(n, t); } }
  if (by_hard) { kind = ((cb >> n) & 1ull) ? 4u : (((vb >> n) & 1ull) ? 3u : 0u); if (kind) { stop_node = RL(node, (int)n); stop_nrc = RL(nrc, (int)n); } }
  if ((u32)lane < n) { o_key = skey; o_pay = spay; }
  return n;
}

// (the leader's copy, out of line: rr_leader sits at the register limit, and what it needs of the step is four words)
__device__ __attribute__((noinline)) u32 rr_step_merge_leader(const u32 sp, const int lane, const u32 rem, const u32 nE, const u64 vfy) {
  RRLds& L = g_rr_lds;
  u32 wkey, wpay, kind, snode, snrc, mrank;
  const u32 n = rr_step_merge(L.stepk[sp], L.mrg[0], lane, rem, nE, vfy, wkey, wpay, kind, snode, snrc, mrank);
  L.mrg_out[lane] = wpay;
  if (lane == 0) { L.mrg_k[0] = kind; L.mrg_k[1] = snode; L.mrg_k[2] = snrc; }
  LSYNC();
  return n;
}

// One pick, as every wave sees it.  Returns 0 (placed: node / nrc / child / key are the winner's) or why the round stops here:
// 2 nothing accepts | 3 the winner needs the exact filter | 4 count field full.  mw: lane i holds word i of the pod's answers (RREntry::m)
__device__ __forceinline__ u32 rr_pick_decide(const u32 nE, const u32 mw, const u64 w, u32& node, u32& nrc, u32& child, u32& key) {
  node = 0xFFFFFFFFu; nrc = 0; child = 0; key = 0;
  if (w == ~0ull) return 2u;
  node = (u32)w & 0xFFFFu; nrc = ((u32)w >> 16) & 0xFFu; key = (u32)(w >> 32);
  const u64 chg = (u64)RL(mw, 2) | ((u64)RL(mw, 3) << 32), vfy = (u64)RL(mw, 4) | ((u64)RL(mw, 5) << 32);
  child = ((chg >> nrc) & 1ull) ? ((RL(mw, 8 + (int)(nrc >> 2)) >> (8u * (nrc & 3u))) & 0xFFu) : nrc;
  if (node >= nE && (key >> 22) >= RR_CNTMAX) return 4u;
  if ((vfy >> nrc) & 1ull) return 3u;
  return 0u;
}

// The STATIC part of a prepared pod (RRPx; round 6): from the pod's class record in the ring (prepared: E.w[48] == pos) -- its requests, its hostname items and records as
// LDS offsets, and per requirement class n = lane what a node of that class answers from the class's cached answers: accepts, the nrc it would have, whether the winner
// needs the exact filter, whether the narrow record counts and into which domain.  Built by the worker waves, a dozen pods ahead of the leader's loop (they would otherwise
// sit at the barrier), and by all waves for the first entries of a phase at the end of the round before.  It stands while the nrc table has `nn` entries (u[2]) and the
// groups that exist are those of `gam` (a relaxation clears every prepared record).  A dyn1 pod's answers depend on its group's counters through ONE choice, the domain
// nextDomainTopologySpread picks (topologygroup.go:155-182): the answers are laid down for each of the first four domains (td[]), the leader's loop picks.
__device__ __forceinline__ void rr_px_static(const int lane, const u32 pos, const u32 nn, const u64 gam, const GA u32* const rrm) {
  RRLds& L = g_rr_lds; const RRNrc& nt = L.nt;
  RREntry& E = L.ring[pos & (RR_RING - 1u)]; RRPx& X = L.px[pos & (RR_PX - 1u)];
  if (lane == 0) RR_LDS_STORE(&X.u[0], 0xFFFFFFFFu);
  LSYNC();
  const u32x4 we = *(const u32x4*)&E.w[48];              // stream position | class | pod | (hostname records that count)
  const u32x4 wq = *(const u32x4*)&E.w[52];              // requeued | shares the answers of | hot 0 (simple, dyn1) | hot 1 (item 0)
  const u32x4 wh = *(const u32x4*)&E.w[56];              // hot 2 (item 1) | hot 3, 4 (hostname records) | hot 5 (narrow record)
  u32x4 m0 = *(const u32x4*)&E.t1[0], m1 = *(const u32x4*)&E.t1[4];      // accepts | changes the nrc ; needs the exact filter | nrcs answered
  const bool cover = we.x == pos && wq.x == 0 && (wq.z & 1u);      // prepared, not requeued, a class of the straight-line loop
  if (UF((cover && m1.z < nn) ? 1u : 0u)) {
    // the class's cached answers are read again (another class that shares them may have met the new nrcs)
    const u32 mi = UF(wq.y); const u32 mw = (u32)lane < 24 ? rrm[(size_t)mi * 24 + lane] : 0u;
    LSYNC(); if ((u32)lane < 32) { E.m[lane] = mw; E.t1[lane] = mw; } LSYNC();
    m0 = *(const u32x4*)&E.t1[0]; m1 = *(const u32x4*)&E.t1[4];
  }
  const bool go = UF((cover && m1.z == nn) ? 1u : 0u) != 0;
  u32 flags = RR_PX_STOP7, dg = 0, ngrp = 0, ho = 0, plainb = 0xFFFFFFFFu, dself = 0, dskew = 0, dpd = 0;
  if (go) {
    const u32 it0 = wq.w, it1 = wh.x, hr0 = wh.y, hr1 = wh.z, nr0 = wh.w;
    const bool dyn = UF(wq.z & 2u) != 0;
    const bool cnt0 = ((hr0 >> 25) & 1u) && (((hr0 >> 24) & 1u) || ((gam >> ((hr0 >> 16) & 63u)) & 1ull)), cnt1 = ((hr1 >> 25) & 1u) && (((hr1 >> 24) & 1u) || ((gam >> ((hr1 >> 16) & 63u)) & 1ull));
    const u32 ho0 = cnt0 ? (hr0 & 0xFFFFu) : RR_HC_SINK, ho1 = cnt1 ? (hr1 & 0xFFFFu) : RR_HC_SINK;
    ho = ho0 | (ho1 << 16);
    // a plain replica (one base class: same requests, same answers; no hostname item, no topology counter read): RUN rounds place stretches of those several per barrier
    plainb = (!dyn && (it0 & 0xFFFFu) == RR_HC_ZERO && (it1 & 0xFFFFu) == RR_HC_ZERO) ? E.w[27] : 0xFFFFFFFFu;
    flags = RR_PX_GO | (dyn ? RR_PX_DYN : 0u) | ((dyn || (m0.z | m0.w) != 0) ? RR_PX_CHG : 0u) | ((ho1 == ho0 && cnt0 && cnt1) ? RR_PX_TWICE : 0u) | ((cnt0 || cnt1) ? RR_PX_HREC : 0u);
    ngrp = nr0 & 63u;
    {
      // ---- what a node of requirement class n = lane answers, and whether the narrow record counts there: spread / affinity count a node whose requirement on the key
      // has collapsed to one value (topology.go:120-143) ----
      const u32 n = (u32)lane;
      const u64 acc1 = (u64)m0.x | ((u64)m0.y << 32), chg1 = (u64)m0.z | ((u64)m0.w << 32), vfy1 = (u64)m1.x | ((u64)m1.y << 32);
      const u32 cbyte = ((const u8*)&E.t1[8])[n];
      const bool a_ok = n < nn && ((acc1 >> n) & 1ull), a_vfy = (vfy1 >> n) & 1ull; const u32 a_child = ((chg1 >> n) & 1ull) ? cbyte : n;
      const u32 nkey = (nr0 >> 8) & 0xFFu;
      auto rec_of = [&](const u32 ac) -> u32 {      // the narrow record on a node of requirement class ac: counts << 0 | into domain << 1
        const u32 npres = nt.present[ac], ncomp = nt.complement[ac]; const u64 nqm = nt.mask[nkey & (RR_KMAX - 1u)][ac];
        const bool rec = ((nr0 >> 16) & 1u) && ((gam >> ngrp) & 1ull) && ((npres >> nkey) & 1u) && !((ncomp >> nkey) & 1u) && __builtin_popcountll(nqm) == 1;
        return rec ? (1u | ((u32)__builtin_ctzll(nqm | (1ull << 63)) << 1)) : 0u; };
      const u32 r0 = rec_of(a_child & 63u);
      u32 tw = (a_child & 0xFFu) | (a_ok ? 1u << 8 : 0u) | (a_vfy ? 1u << 9 : 0u) | ((r0 & 1u) << 11) | (((r0 >> 1) & 63u) << 12);
      if (dyn) {
        // dyn1 (the answers above are the class's WITHOUT the spread): with the node's requirement on the spread's key narrowed to domain d, for each of the first four
        // domains -- the nrc it becomes (RRLds::t2; not met yet: not answered here), the exact-filter relation (vpair), the narrow record there
        const u32 dw = E.w[11], dk = (dw >> 16) & 0xFFu, dk0 = UF(L.wx[8]), dk1 = UF(L.wx[9]);
        dg = (dw >> 8) & 63u; dself = dw >> 24; dskew = E.w[19]; dpd = E.w[26];
        const u32 dks = dk == dk0 ? 0u : 1u, n1 = a_child & 63u;
        const u64 nd = L.dy_nd[dks][n1], vp = L.vpair[n];
        const u32 c4 = *(const u32*)&L.t2[dks][n1][0];      // (domains 0..3: one word)
        u32 tdw[2];
#pragma unroll
        for (int d = 0; d < 4; ++d) {
          const u32 c2 = (c4 >> (8 * d)) & 0xFFu, ac = c2 & 63u, rd = rec_of(ac);
          const u32 e = ac | (c2 == 0xFFu ? 1u << 6 : 0u) | ((u32)((vp >> ac) & 1ull) << 7) | ((rd & 1u) << 8) | (((rd >> 1) & 63u) << 9);
          if (d & 1) tdw[d >> 1] |= e << 16; else tdw[d >> 1] = e;
        }
        *(u32*)&X.td[n * 4u] = tdw[0]; *(u32*)&X.td[n * 4u + 2u] = tdw[1];
        tw |= ((dk != dk0 && dk != dk1) ? 1u << 10 : 0u) | (((u32)nd & 15u) << 18);      // (a dyn key without a column: not answered here)
      }
      X.t[lane] = tw;
    }
  }
  {
    const u32 l = (u32)lane;
    const u32 rqw = (l >= 4u && l < 12u) ? E.w[l - 4u] : 0u;
    const u32 v = l == 1u ? flags : l == 2u ? nn : l < 4u ? 0u : l < 12u ? rqw : l == 12u ? wq.w : l == 13u ? wh.x : l == 14u ? ho : l == 15u ? we.z
                : l == 16u ? ((E.w[8] & 0xFFu) | (dg << 8) | (ngrp << 16)) : l == 17u ? plainb : l == 20u ? dself : l == 21u ? dskew : l == 22u ? dpd : 0u;
    if (l >= 1u && l < 24u) X.u[l] = v;
    LSYNC();
    if (l == 0u) RR_LDS_STORE(&X.u[0], pos);      // (the stream position behind everything else: the leader reads it before everything else)
  }
  LSYNC();
}

// ---------------------------------------------------------------- the workers (waves 1..7): the nodes, in registers ----------------------------------------------------------------
__device__ __attribute__((noinline)) void rr_worker(const u32 wv, const int lane) {
  RR_CTX;
#ifdef KS_PROBES
  u64 rrp[16]; for (int i = 0; i < 16; ++i) rrp[i] = 0; u64 rrp_t = __builtin_readcyclecounter();
#endif
  u32 round = 0;
  __syncthreads();                         // the leader has interned the existing nodes' requirement records
  if (UF(L.init_err)) return;
  // ---------------- worker state: the nodes ----------------
  u32 n_key[RR_NPL], n_meta[RR_NPL], n_hc[RR_NPL][RR_GW]; i64 n_room[RR_NPL][4];      // meta: nrc | requested-resource mask << 8
#pragma unroll
  for (int i = 0; i < RR_NPL; ++i) {
    n_key[i] = 0xFFFFFFFFu; n_meta[i] = 0;
#pragma unroll
    for (int w = 0; w < RR_GW; ++w) n_hc[i][w] = 0xFFFFFFFFu;
#pragma unroll
    for (int r = 0; r < 4; ++r) n_room[i][r] = 0;
  }
  {
#pragma unroll
    for (int i = 0; i < RR_NPL; ++i) {
      const u32 n = RR_NODE_AT((u32)i, wv - 1u, lane);
      if (n < nE) {
        n_key[i] = (n << 3) | (u32)i; n_meta[i] = (u32)L.en_nrc[n] | (P.en_requests_present[n] << 8);
        bool over = false;      // a requested resource already beyond the node's allocatable: resources.Fits fails for every pod (existingnode.go:96-100)
#pragma unroll
        for (int r = 0; r < 4; ++r) { n_room[i][r] = (u32)r < nR ? P.en_avail[(size_t)n * nR + r] - P.en_requests[(size_t)n * nR + r] : 0; if ((u32)r < nR && ((P.en_requests_present[n] >> r) & 1u) && n_room[i][r] < 0) over = true; }
        if (over) n_meta[i] = 63u | (P.en_requests_present[n] << 8);
        for (u32 h = 0; h < tb.GH; ++h) {
          const i32 c = ks_host_count0(P, h, n); const u32 b = c < 0 ? 0xFFu : (c > 254 ? 254u : (u32)c);
          if (b == 0u) atomicAdd(&L.hz[h & 31u], 1);
#pragma unroll
          for (int w = 0; w < RR_GW; ++w) if ((h >> 2) == (u32)w) n_hc[i][w] = (n_hc[i][w] & ~(0xFFu << (8 * (h & 3u)))) | (b << (8 * (h & 3u)));
        }
      }
    }
  }

  // ================= rounds =================
  const u32 wk_i = wv - 1u;
  // the wave's candidate from the lanes' best keys: key << 32 | nrc << 16 | node (all ones: none)
  auto wave_cand = [&](const u32 best) -> u64 {
    const u32 kmin = wave_min_u32(best);
    u64 sub = ~0ull;
    if (kmin != 0xFFFFFFFFu) {
      const int wl = __builtin_ctzll(ballot64(best == kmin));
      const u32 ws = kmin & 7u;
      u32 bmeta = 0;
#pragma unroll
      for (int i = 0; i < RR_NPL; ++i) if ((u32)i == ws) bmeta = n_meta[i];
      bmeta = RL(bmeta, wl);
      sub = ((u64)kmin << 32) | ((u64)(bmeta & 0xFFu) << 16) | (u64)RR_NODE_AT(ws, wk_i, wl);
    }
    return sub;
  };
    // one slot against the current parameters (straight-line vector code; a resource the pod does not request asks for 0, and no live node has negative headroom)
#define RR_EVAL_SLOT(i) { bool rj = ((nacc >> (n_meta[i] & 63u)) & 1ull) != 0; rj |= rq0 > n_room[i][0]; rj |= rq1 > n_room[i][1]; rj |= rq2 > n_room[i][2]; rj |= rq3 > n_room[i][3]; rej |= rj ? (1u << (i)) : 0u; }
    // hostname-keyed items: this node's own counter (spread: count + self <= maxSkew, the minimum over hostnames being 0, topologygroup.go:184-188; anti-affinity: 0): refused iff the
    // counter (255: not a registered domain) exceeds lim.  item = word of the counter | bit shift << 8
#define RR_HOST_SLOT(i, w, sh, lim) rej |= ((u32)((lim) - (i32)((n_hc[i][w] >> (sh)) & 0xFFu)) >> 31) << (i);
#define RR_HOST_CASE(w, X, sh, lim) case w: X(w, sh, lim) break;
#define RR_HOST_ITEM(X, item, lim) { const u32 sh_ = (item) >> 8; switch ((item) & 0xFFu) { RR_HOST_CASE(0, X, sh_, lim) RR_HOST_CASE(1, X, sh_, lim) RR_HOST_CASE(2, X, sh_, lim) RR_HOST_CASE(3, X, sh_, lim) RR_HOST_CASE(4, X, sh_, lim) RR_HOST_CASE(5, X, sh_, lim) RR_HOST_CASE(6, X, sh_, lim) RR_HOST_CASE(7, X, sh_, lim) default: break; } }
#define RR_HOST_ALL(w, sh, lim) RR_HOST_SLOT(0, w, sh, lim) RR_HOST_SLOT(1, w, sh, lim) RR_HOST_SLOT(2, w, sh, lim) RR_HOST_SLOT(3, w, sh, lim) if (nslots > 4) { RR_HOST_SLOT(4, w, sh, lim) RR_HOST_SLOT(5, w, sh, lim) RR_HOST_SLOT(6, w, sh, lim) RR_HOST_SLOT(7, w, sh, lim) }
  u32 pf_n = 0, pf_pos = 0, pf_qi = 0; u64 pf_gam = 0;      // class records to prepare for the leader's window: how many queue entries there are behind the last round's, the first one's stream position / queue index
  u32 lent = 8u;                           // the slot this lane has lent to the leader's window (8: none) | its rank among the wave's published keys << 4
  for (;;) {
    u32 m1 = 0xFFFFFFFFu, myrank = 15u;
    {
      // ---- LEND, offered at the end of every round (while the leader resolves it; the order the leader may still decide -- a machine -- joins the window on its side):
      // the wave's 8 smallest keys (at most one per lane) go to the leader's window with their nodes' state; `cut`: every key the wave keeps is >= it ----
      u32 m2 = 0xFFFFFFFFu;
#pragma unroll
      for (int i = 0; i < RR_NPL; ++i) { const u32 k = n_key[i]; m2 = min(m2, max(m1, k)); m1 = min(m1, k); }
      const u32 ms = m1 & 7u;              // (a key names its slot)
      u32 cur = m1, nfound = 0;
      for (u32 r = 0; r < RR_LPW; ++r) {
        const u32 km = wave_min_u32(cur);
        if (km == 0xFFFFFFFFu) break;
        if (cur == km) { myrank = r; cur = 0xFFFFFFFFu; }
        nfound = r + 1u;
      }
      const u32 cut = min(wave_min_u32(cur), wave_min_u32(m2));
      if (myrank < RR_LPW) {                   // (word by word, a select chain each: nothing but the word in flight is held in registers beside the node arrays)
        const u32 ix = wk_i * RR_LPW + myrank;
        L.wn_key[ix] = m1; L.wn_own[ix] = RR_NODE_AT(ms, wk_i, lane);
        { u32 v = n_meta[0];
#pragma unroll
          for (int i = 1; i < RR_NPL; ++i) v = ms == (u32)i ? n_meta[i] : v;
          L.wn_meta[ix] = v; }
#pragma unroll
        for (int w = 0; w < RR_GW; ++w) { u32 v = n_hc[0][w];
#pragma unroll
          for (int i = 1; i < RR_NPL; ++i) v = ms == (u32)i ? n_hc[i][w] : v;
          L.wn_hc[w][ix] = v; }
#pragma unroll
        for (int r = 0; r < 4; ++r) { i64 v = n_room[0][r];
#pragma unroll
          for (int i = 1; i < RR_NPL; ++i) v = ms == (u32)i ? n_room[i][r] : v;
          L.wn_room[r][ix] = v; }
      }
      if ((u32)lane < RR_LPW && (u32)lane >= nfound) L.wn_key[wk_i * RR_LPW + (u32)lane] = 0xFFFFFFFFu;
      if (lane == 0) L.wn_cut[wk_i] = cut;
    }
    if (wk_i < UF(pf_n)) {
      // ... and one class record per wave: the queue entries behind the round's, for the window phase it announced (what the leader's ring_load / ring_store do)
      u32 idx = UF(pf_qi) + wk_i; if (idx >= nP) idx -= nP; if (idx >= nP) idx = 0;
      const u64 et = UF64(tb.q[idx]); const u32 cls = (u32)(et >> 32) & 0x7FFFFFFFu, mk = UF(rr_mi[cls]);
      u32 bb = (u32)lane < 48 ? rrb[(size_t)cls * 48 + lane] : ((u32)lane == 53 ? mk : (((u32)lane >= 54 && (u32)lane < 62) ? GC(u32, P.rr_hot)[(size_t)cls * 8 + lane - 54] : 0u));
      const u32 pm = (u32)lane < 24 ? rrm[(size_t)mk * 24 + lane] : 0u;
      const u32 pos = UF(pf_pos) + wk_i; RREntry& R = L.ring[pos & (RR_RING - 1u)];
      const u64 gamw = UF64(pf_gam);
      const u32 nh = RL(bb, 17); const bool hon = (u32)lane >= 28u && (u32)lane < 28u + nh && (((bb >> 16) & 1u) || ((gamw >> ((bb >> 8) & 63u)) & 1ull));
      const u32 hm = (u32)(ballot64(hon) >> 28);
      if ((u32)lane == 48) bb = pos; else if ((u32)lane == 49) bb = cls; else if ((u32)lane == 50) bb = (u32)et; else if ((u32)lane == 51) bb = hm; else if ((u32)lane == 52) bb = (u32)(et >> 63);
      R.w[lane] = bb; if ((u32)lane < 32) { R.m[lane] = pm; R.t1[lane] = pm; }
      LSYNC();
      if (pos - UF(pf_pos) < RR_PXA) rr_px_static(lane, pos, UF(L.wx[5]), gamw, rrm);      // (... with its static part for the window's loop)
    }
    pf_n = 0;
    __syncthreads();                       // B0: the leader has said whether a window phase precedes the round; every wave's keys and cuts are published
    if (UF(L.wn_mode)) {
      const u32 ms = m1 & 7u;
      u32 T = 0xFFFFFFFFu;
#pragma unroll
      for (int w = 0; w < RR_NWK; ++w) T = min(T, L.wn_cut[w]);
      // what lies below every wave's cut is lent: the leader holds the node until the next round's B1, the slot takes nothing meanwhile (nrc 63)
      if (myrank < RR_LPW && m1 < T) {
        lent = ms | (myrank << 4);
#pragma unroll
        for (int i = 0; i < RR_NPL; ++i) if (ms == (u32)i) n_meta[i] = (n_meta[i] & ~0xFFu) | 63u;
      }
      // ---- while the window stands: the class records ahead of the leader (entry t of the phase by wave t mod 6), prepared by the waves that would otherwise wait at B1.
      // No barrier: a record's tag -- its stream position -- is written behind everything else, the leader reads it before everything else. ----
      {
        const u32 base = UF(L.wq_base), qh0 = UF(L.wq_head), ql0 = UF(L.wq_len); const u64 gamw = UF64(L.wq_gam);
        u32 q_seen = 0, f_seen = 0;
        for (;;) {
          const u32 st = RL((RR_LDS_LOAD(&L.wn_qpos) << 1) | RR_LDS_LOAD(&L.wn_done), 0);
          if (st & 1u) break;
          const u32 sq = RL((RR_LDS_LOAD(&L.wn_qn) & 0xFFFFu) | (RR_LDS_LOAD(&L.wn_fn) << 16), 0);
          if ((sq & 0xFFFFu) != q_seen) {
            // ---- the leader asks: which of the nodes the workers hold is the first to accept the pod at stream position wn_qp?  (what a round's EVALUATE + PICK answer,
            // without the round: no node changes hands, the lent slots refuse by themselves) ----
            q_seen = sq & 0xFFFFu;
            RR_ACQUIRE();      // (the question's payload -- wn_qp, the ring entry -- behind its number)
            const RREntry& Eq = L.ring[UF(RR_LDS_LOAD(&L.wn_qp)) & (RR_RING - 1u)];
            const u32 bw = Eq.w[lane], mw = Eq.m[lane & 31];
            const u64 nacc = ~((u64)RL(mw, 0) | ((u64)RL(mw, 1) << 32));
            const i64 rq0 = (i64)((u64)RL(bw, 0) | ((u64)RL(bw, 1) << 32)), rq1 = (i64)((u64)RL(bw, 2) | ((u64)RL(bw, 3) << 32)), rq2 = (i64)((u64)RL(bw, 4) | ((u64)RL(bw, 5) << 32)), rq3 = (i64)((u64)RL(bw, 6) | ((u64)RL(bw, 7) << 32));
            const u32 nhost = RL(bw, 16), nslots = RR_NPL;
            u32 rej = 0;
            RR_EVAL_SLOT(0) RR_EVAL_SLOT(1) RR_EVAL_SLOT(2) RR_EVAL_SLOT(3) RR_EVAL_SLOT(4) RR_EVAL_SLOT(5) RR_EVAL_SLOT(6) RR_EVAL_SLOT(7)
            for (u32 hj = 0; hj < nhost && hj < 3u; ++hj) {
              const u32 hw = RL(bw, 20 + (int)hj), hit = ((hw >> 18) & 7u) | ((8u * ((hw >> 16) & 3u)) << 8); const i32 hlim = (hw & 0xFFu) == 0 ? (i32)RL(bw, 23 + (int)hj) - (i32)((hw >> 8) & 0xFFu) : 0;
              RR_HOST_ITEM(RR_HOST_ALL, hit, hlim)
            }
            u32 best = 0xFFFFFFFFu;
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) best = min(best, n_key[i] | (u32)(((i32)((~rej >> i) & 1u)) - 1));
            const u64 wsub = wave_cand(best);
            if (lane == 0) { if (wsub != ~0ull) atomicMin((unsigned long long*)&L.wq_win, (unsigned long long)wsub); __hip_atomic_fetch_add(&L.wn_qdone, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP); }
            continue;
          }
          if ((sq >> 16) != f_seen) {
            // ---- ... and takes the answer's node into its window (place wn_fplace; it comes back with the machines opened meanwhile): its owner publishes it, the slot takes nothing until then ----
            f_seen = sq >> 16;
            RR_ACQUIRE();
            const u32 fnode = UF(RR_LDS_LOAD(&L.wn_fnode)), ix = UF(RR_LDS_LOAD(&L.wn_fplace));
            if (RR_NODE_WV(fnode) == wv) {
              const u32 fs = RR_NODE_SLOT(fnode); const bool mine = (u32)lane == RR_NODE_LANE(fnode);
              if (mine) {
                L.wn_own[ix] = fnode;
                { u32 v = n_key[0];
#pragma unroll
                  for (int i = 1; i < RR_NPL; ++i) v = fs == (u32)i ? n_key[i] : v;
                  L.wn_key[ix] = v; }
                { u32 v = n_meta[0];
#pragma unroll
                  for (int i = 1; i < RR_NPL; ++i) v = fs == (u32)i ? n_meta[i] : v;
                  L.wn_meta[ix] = v; }
#pragma unroll
                for (int w = 0; w < RR_GW; ++w) { u32 v = n_hc[0][w];
#pragma unroll
                  for (int i = 1; i < RR_NPL; ++i) v = fs == (u32)i ? n_hc[i][w] : v;
                  L.wn_hc[w][ix] = v; }
#pragma unroll
                for (int r = 0; r < 4; ++r) { i64 v = n_room[0][r];
#pragma unroll
                  for (int i = 1; i < RR_NPL; ++i) v = fs == (u32)i ? n_room[i][r] : v;
                  L.wn_room[r][ix] = v; }
              }
#pragma unroll
              for (int i = 0; i < RR_NPL; ++i) if (mine && fs == (u32)i) n_meta[i] = (n_meta[i] & ~0xFFu) | 63u;
              LSYNC();
              if (lane == 0) __hip_atomic_store(&L.wn_fdone, f_seen, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            }
            continue;
          }
          // This wave's entries among the next RR_PXA (the waves of RR_SMASK share them), checked at every turn -- the class record for this stream position, the prepared
          // pod for this position and this nrc table: a relaxation clears the prepared records, a machine's requirement record grows the table, and either may happen
          // behind an entry this wave has already made.  Lane j looks at the wave's j-th entry; the nearest one that lacks something is made first.
          const u32 rel = (st >> 1) - base;
          const u32 nn = UF(RR_LDS_LOAD(&L.wx[5]));
          constexpr u32 NS_ = (u32)__builtin_popcount(RR_SMASK);
          const u32 has = (RR_SMASK >> wk_i) & 1u, rk = (u32)__builtin_popcount(RR_SMASK & ((1u << wk_i) - 1u)), rm = rel % NS_;
          const u32 tj = rel + (rk >= rm ? rk - rm : rk + NS_ - rm) + (u32)lane * NS_, posj = base + tj;
          const RRPx& Xj = L.px[posj & (RR_PX - 1u)];
          const u32 rtag = RR_LDS_LOAD(&L.ring[posj & (RR_RING - 1u)].w[48]), ptag = RR_LDS_LOAD(&Xj.u[0]), pnn = RR_LDS_LOAD(&Xj.u[2]);
          const u64 bad = ballot64(has && (u32)lane * NS_ < RR_PXA && tj < ql0 && tj < rel + RR_PXA && (rtag != posj || ptag != posj || pnn != nn));
          if (bad) {
            const int bj = (int)__builtin_ctzll(bad);
            const u32 t = RL(tj, bj), pos = base + t; RREntry& R = L.ring[pos & (RR_RING - 1u)];
            {
            if (RL(rtag, bj) != pos) {
              u32 idx = qh0 + t; if (idx >= nP) idx -= nP; if (idx >= nP) idx = 0;
              const u64 et = UF64(tb.q[idx]); const u32 cls = (u32)(et >> 32) & 0x7FFFFFFFu, mk = UF(rr_mi[cls]);
              u32 bb = (u32)lane < 48 ? rrb[(size_t)cls * 48 + lane] : ((u32)lane == 53 ? mk : (((u32)lane >= 54 && (u32)lane < 62) ? GC(u32, P.rr_hot)[(size_t)cls * 8 + lane - 54] : 0u));
              const u32 pm = (u32)lane < 24 ? rrm[(size_t)mk * 24 + lane] : 0u;
              const u32 nh = RL(bb, 17); const bool hon = (u32)lane >= 28u && (u32)lane < 28u + nh && (((bb >> 16) & 1u) || ((gamw >> ((bb >> 8) & 63u)) & 1ull));
              const u32 hm = (u32)(ballot64(hon) >> 28);
              if ((u32)lane == 48) bb = 0xFFFFFFFFu; else if ((u32)lane == 49) bb = cls; else if ((u32)lane == 50) bb = (u32)et; else if ((u32)lane == 51) bb = hm; else if ((u32)lane == 52) bb = (u32)(et >> 63);
              if ((u32)lane < 32) { R.m[lane] = pm; R.t1[lane] = pm; }
              R.w[lane] = bb;
              LSYNC();
              if ((u32)lane == 48) RR_LDS_STORE(&R.w[48], pos);
              LSYNC();
            }
            rr_px_static(lane, pos, nn, gamw, rrm);      // ... and the pod's static part for the leader's loop
            }
          } else RR_POLL_PAUSE();
        }
      }
    }
    __syncthreads();                       // B1: the round's header and class records are visible
    RRP(8);
    const u32 par = round & 1u;
    const u32 hdw = L.ctl[par].hdr[lane & 31];
    const u32 pre = RL(hdw, RRH_PRE), nslots = RL(hdw, RRH_NSLOTS), seq0 = RL(hdw, RRH_SEQ), nexcl = RL(hdw, RRH_NEXCL), pos0 = RL(hdw, RRH_POS);
    u32 nb = RL(hdw, RRH_NB), same = RL(hdw, RRH_SAME);      // (as of the round's start: pods may join while it runs, the leader says so at every pick's barrier)
    {
      const u32 rw = RL(hdw, RRH_RET);
      if (rw) {
        // ---- the window's nodes come back: the lent ones to the slots they left, the machines opened meanwhile to the slots they were numbered for ----
        if ((lent & 15u) < 8u) {
          const u32 ix = wk_i * RR_LPW + (lent >> 4), s_ = lent & 7u;
          { const u32 v = L.wn_key[ix];
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) n_key[i] = s_ == (u32)i ? v : n_key[i]; }
          { const u32 v = L.wn_meta[ix];
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) n_meta[i] = s_ == (u32)i ? v : n_meta[i]; }
#pragma unroll
          for (int w = 0; w < RR_GW; ++w) { const u32 v = L.wn_hc[w][ix];
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) n_hc[i][w] = s_ == (u32)i ? v : n_hc[i][w]; }
#pragma unroll
          for (int r = 0; r < 4; ++r) { const i64 v = L.wn_room[r][ix];
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) n_room[i][r] = s_ == (u32)i ? v : n_room[i][r]; }
          lent = 8u;
        }
        const u32 nfr = rw >> 8;
        for (u32 f = 0; f < nfr; ++f) {
          const u32 ix = RR_WLENT + f, node = UF(L.wn_own[ix]);
          if (RR_NODE_WV(node) != wv) continue;
          const u32 oslot = RR_NODE_SLOT(node); const bool mine = (u32)lane == RR_NODE_LANE(node);
          { const u32 v = L.wn_key[ix];
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) n_key[i] = (mine && oslot == (u32)i) ? v : n_key[i]; }
          { const u32 v = L.wn_meta[ix];
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) n_meta[i] = (mine && oslot == (u32)i) ? v : n_meta[i]; }
#pragma unroll
          for (int w = 0; w < RR_GW; ++w) { const u32 v = L.wn_hc[w][ix];
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) n_hc[i][w] = (mine && oslot == (u32)i) ? v : n_hc[i][w]; }
#pragma unroll
          for (int r = 0; r < 4; ++r) { const i64 v = L.wn_room[r][ix];
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) n_room[i][r] = (mine && oslot == (u32)i) ? v : n_room[i][r]; }
        }
      }
    }
    if (RL(hdw, RRH_EXIT)) break;
    const RRCtl& C = L.ctl[par];
    u32 stop_kind = 0, stop_node = 0;
    u32 hzm = 0;                             // per lane: the hostname counters a commit of this lane took from 0 to 1 (RRLds::hz, the census of zero counters)
#define RR_HZ_FLUSH() if (hzm) { for (u32 bits = hzm; bits; bits &= bits - 1) atomicAdd(&L.hz[__builtin_ctz(bits)], -1); hzm = 0; }
    // The pods of a round are taken one after the other.  A pod that is evaluated like the one before it (same evaluation class: a run of replicas) inherits the
    // lanes' accepting-slot masks; only the node that took the last pod is evaluated again, by the lane that holds it.
    // Parameters of the current evaluation (wave-uniform): requests, the nrcs that refuse, hostname-keyed items
    i64 rq0 = 0, rq1 = 0, rq2 = 0, rq3 = 0; u64 nacc = ~0ull; u32 nhost = 0, hit0 = 0, hit1 = 0, hit2 = 0; i32 hlim0 = 0, hlim1 = 0, hlim2 = 0;
    u32 okm = 0;                             // per lane: the slots that accept the current evaluation's pods
    u64 sub = ~0ull; bool fresh = false;
    // EVALUATE: every node this wave holds against the evaluation class of the pod at entry E (its answers in mw; j: its place in the round)
    auto do_eval = [&](const RREntry& E, const u32 mw, const u32 j, const bool nohost) {
      RRP(9);
      const u32 bw = E.w[lane];
      nacc = ~((u64)RL(mw, 0) | ((u64)RL(mw, 1) << 32));
      rq0 = (i64)((u64)RL(bw, 0) | ((u64)RL(bw, 1) << 32)); rq1 = (i64)((u64)RL(bw, 2) | ((u64)RL(bw, 3) << 32)); rq2 = (i64)((u64)RL(bw, 4) | ((u64)RL(bw, 5) << 32)); rq3 = (i64)((u64)RL(bw, 6) | ((u64)RL(bw, 7) << 32));
      nhost = nohost ? 0u : RL(bw, 16);
      if (nhost > 0) { const u32 hw = RL(bw, 20); hit0 = ((hw >> 18) & 7u) | ((8u * ((hw >> 16) & 3u)) << 8); hlim0 = (hw & 0xFFu) == 0 ? (i32)RL(bw, 23) - (i32)((hw >> 8) & 0xFFu) : 0; }
      if (nhost > 1) { const u32 hw = RL(bw, 21); hit1 = ((hw >> 18) & 7u) | ((8u * ((hw >> 16) & 3u)) << 8); hlim1 = (hw & 0xFFu) == 0 ? (i32)RL(bw, 24) - (i32)((hw >> 8) & 0xFFu) : 0; }
      if (nhost > 2) { const u32 hw = RL(bw, 22); hit2 = ((hw >> 18) & 7u) | ((8u * ((hw >> 16) & 3u)) << 8); hlim2 = (hw & 0xFFu) == 0 ? (i32)RL(bw, 25) - (i32)((hw >> 8) & 0xFFu) : 0; }
      const u32 slotmask = nslots >= RR_NPL ? 0xFFu : ((1u << nslots) - 1u);
      u32 rej = ~slotmask;
      RR_EVAL_SLOT(0) RR_EVAL_SLOT(1) RR_EVAL_SLOT(2) RR_EVAL_SLOT(3)
      if (nslots > 4) { RR_EVAL_SLOT(4) RR_EVAL_SLOT(5) RR_EVAL_SLOT(6) RR_EVAL_SLOT(7) }
      if (nhost > 0) RR_HOST_ITEM(RR_HOST_ALL, hit0, hlim0)
      if (nhost > 1) RR_HOST_ITEM(RR_HOST_ALL, hit1, hlim1)
      if (nhost > 2) RR_HOST_ITEM(RR_HOST_ALL, hit2, hlim2)
      if (j == 0 && nexcl) {
#pragma unroll
        for (int i = 0; i < RR_NPL; ++i) {
          const u32 n = RR_NODE_AT((u32)i, wk_i, lane);
          for (u32 x = 0; x < nexcl; ++x) if (((RL(hdw, RRH_EXCL + (int)(x >> 1)) >> (16u * (x & 1u))) & 0xFFFFu) == n) rej |= 1u << i;
        }
      }
      okm = ~rej & 0xFFu; fresh = true;
      RRP(10);
    };
    const u32 run = RL(hdw, RRH_RUN);
    for (int it = pre ? -1 : 0; it < (run ? 0 : (int)nb); ++it) {
      u32 node, nrc_new, pseq, phm; const u32* pbp; bool create = false;
      if (it < 0) { node = RL(hdw, RRH_PNODE); nrc_new = RL(hdw, RRH_PNRC); pseq = RL(hdw, RRH_PSEQ); phm = RL(hdw, RRH_PHMASK); pbp = C.pbrief; create = pre == 3; }
      else {
        const u32 j = (u32)it;
        const RREntry& E = L.ring[(pos0 + j) & (RR_RING - 1u)];
        const u32 mw = E.m[lane & 31];
        if (!((same >> j) & 1u)) do_eval(E, mw, j, false);
        if (fresh) {
          u32 best = 0xFFFFFFFFu;
#pragma unroll
          for (int i = 0; i < RR_NPL; ++i) best = min(best, n_key[i] | (u32)(((i32)((okm >> i) & 1u)) - 1));
          sub = wave_cand(best); fresh = false;
        }
        // ---- PICK: arg-min over the waves through one LDS atomic per wave, a barrier, everyone reads the winner ----
        if (lane == 0 && sub != ~0ull) atomicMin((unsigned long long*)&L.win[par][j], (unsigned long long)sub);
        RRP(11);
        __syncthreads();
        RRP(12);
        const u64 w = UF64(L.win[par][j]);
        { const u32 nb2 = UF(C.hdr[RRH_NB2 + (j & 1u)]); nb = nb2 & 0xFFu; same = nb2 >> 8; }
        u32 nrc, key;
        const u32 kind = rr_pick_decide(nE, mw, w, node, nrc, nrc_new, key);
        if (kind != 0) { stop_kind = kind; stop_node = node; break; }
        pseq = seq0 + j; phm = UF(E.w[51]); pbp = E.w;
        RRP(13);
      }
      // ---- COMMIT: Node.Add's writes to the node (node.go:100-107) by the lane that holds it: requests, requirements (nrc), Topology.Record on the hostname-keyed
      // groups (the node's own counters), its place in the order; a fresh node's first state.  Then the node against the current evaluation again. ----
      const u32 oslot = RR_NODE_SLOT(node), owv = RR_NODE_WV(node), olane = RR_NODE_LANE(node);
      if (owv == wv) {
        const bool mine = (u32)lane == olane;
        const u32 cbw = pbp[lane];             // the pod's class brief (lane i: word i); words 50.. of a prepared entry: the pod
        if (it >= 0 && mine) { const u32 pd = pbp[50]; tb.pod_node[pd] = (i32)node; tb.pod_seq[pd] = (i32)pseq; G_pod_reason[pd] = 0;
        }
        const i64 cq0 = (i64)((u64)RL(cbw, 0) | ((u64)RL(cbw, 1) << 32)), cq1 = (i64)((u64)RL(cbw, 2) | ((u64)RL(cbw, 3) << 32)), cq2 = (i64)((u64)RL(cbw, 4) | ((u64)RL(cbw, 5) << 32)), cq3 = (i64)((u64)RL(cbw, 6) | ((u64)RL(cbw, 7) << 32));
        const u32 prm = RL(cbw, 8), nhrec = RL(cbw, 17);
        const u32* const crp = C.create;
        u32 rej = 0;
#define RR_HREC_WORD(i, w) case w: { const u32 c = (n_hc[i][w] >> sh8) & 0xFFu; const u32 c2 = c == 0xFFu ? 1u : (c >= 254u ? 254u : c + 1u); if (mine) { n_hc[i][w] = (n_hc[i][w] & ~(0xFFu << sh8)) | (c2 << sh8); if (c == 0u) hzm |= 1u << (hs & 31u); } } break;
#define RR_COMMIT_SLOT(i) if (oslot == (i)) { \
          if (create) { \
            if (mine) { n_key[i] = UF(crp[0]); n_meta[i] = nrc_new | (UF(crp[1]) << 8); \
              n_room[i][0] = (i64)((u64)UF(crp[2]) | ((u64)UF(crp[3]) << 32)); n_room[i][1] = (i64)((u64)UF(crp[4]) | ((u64)UF(crp[5]) << 32)); \
              n_room[i][2] = (i64)((u64)UF(crp[6]) | ((u64)UF(crp[7]) << 32)); n_room[i][3] = (i64)((u64)UF(crp[8]) | ((u64)UF(crp[9]) << 32)); \
              n_hc[i][0] = UF(crp[10]); n_hc[i][1] = UF(crp[11]); n_hc[i][2] = UF(crp[12]); n_hc[i][3] = UF(crp[13]); n_hc[i][4] = UF(crp[14]); n_hc[i][5] = UF(crp[15]); n_hc[i][6] = UF(crp[16]); n_hc[i][7] = UF(crp[17]); } \
          } else { \
            const u32 nrc_old = RL(n_meta[i], (int)olane) & 0xFFu; \
            i64 d0 = cq0, d1 = cq1, d2 = cq2, d3 = cq3; \
            if (node >= nE && nrc_new != nrc_old) { d0 -= nt.cap[0][nrc_new] - nt.cap[0][nrc_old]; d1 -= nt.cap[1][nrc_new] - nt.cap[1][nrc_old]; d2 -= nt.cap[2][nrc_new] - nt.cap[2][nrc_old]; d3 -= nt.cap[3][nrc_new] - nt.cap[3][nrc_old]; } \
            if (mine) { \
              n_room[i][0] -= d0; n_room[i][1] -= d1; n_room[i][2] -= d2; n_room[i][3] -= d3; \
              if (node >= nE) n_key[i] = (((n_key[i] >> 22) + 1u) << 22) | ((RR_SEQMAX - pseq) << 3) | (n_key[i] & 7u); \
              n_meta[i] = nrc_new | ((((n_meta[i] >> 8) | prm) & 0xFFu) << 8); } \
          } \
          for (u32 t = 0; t < nhrec; ++t) if ((phm >> t) & 1u) {       /* Topology.Record on the hostname-keyed groups: this node's own counters */ \
            const u32 hs = RL(cbw, 28 + (int)t) & 0xFFu, sh8 = 8u * (hs & 3u); \
            switch (hs >> 2) { RR_HREC_WORD(i, 0) RR_HREC_WORD(i, 1) RR_HREC_WORD(i, 2) RR_HREC_WORD(i, 3) RR_HREC_WORD(i, 4) RR_HREC_WORD(i, 5) RR_HREC_WORD(i, 6) RR_HREC_WORD(i, 7) default: break; } \
          } \
          if (it >= 0) { RR_EVAL_SLOT(i) \
            if (nhost > 0) RR_HOST_ITEM(RR_HOST_AT_##i, hit0, hlim0) if (nhost > 1) RR_HOST_ITEM(RR_HOST_AT_##i, hit1, hlim1) if (nhost > 2) RR_HOST_ITEM(RR_HOST_AT_##i, hit2, hlim2) \
            okm = (okm & ~(1u << (i))) | (~rej & (1u << (i))); fresh = true; } }
#define RR_HOST_AT_0(w, sh, lim) RR_HOST_SLOT(0, w, sh, lim)
#define RR_HOST_AT_1(w, sh, lim) RR_HOST_SLOT(1, w, sh, lim)
#define RR_HOST_AT_2(w, sh, lim) RR_HOST_SLOT(2, w, sh, lim)
#define RR_HOST_AT_3(w, sh, lim) RR_HOST_SLOT(3, w, sh, lim)
#define RR_HOST_AT_4(w, sh, lim) RR_HOST_SLOT(4, w, sh, lim)
#define RR_HOST_AT_5(w, sh, lim) RR_HOST_SLOT(5, w, sh, lim)
#define RR_HOST_AT_6(w, sh, lim) RR_HOST_SLOT(6, w, sh, lim)
#define RR_HOST_AT_7(w, sh, lim) RR_HOST_SLOT(7, w, sh, lim)
        RR_COMMIT_SLOT(0) RR_COMMIT_SLOT(1) RR_COMMIT_SLOT(2) RR_COMMIT_SLOT(3) RR_COMMIT_SLOT(4) RR_COMMIT_SLOT(5) RR_COMMIT_SLOT(6) RR_COMMIT_SLOT(7)
        RR_HZ_FLUSH()
      }
    }
    if (run) {
      // ---- a RUN: pods of one evaluation class (no topology counters read).  They are evaluated once; per step every wave publishes its accepting keys of ONE count
      // bucket (all of them, lane by lane, if it holds at most eight: one wave minimum names the bucket, ballots do the rest; else its eight smallest), and after ONE
      // barrier everyone knows which nodes the next pods go to (rr_step_merge); the lanes that hold them commit side by side, slot by slot, and only those slots are
      // evaluated again. ----
      const RREntry& E = L.ring[pos0 & (RR_RING - 1u)];
      const u32 mw = E.m[lane & 31];
      do_eval(E, mw, 0u, true);              // (the shared half only: requests, requirements)
      u32 okb = okm, cur_item = 0, cur_item1 = 0;      // okb: the slots that pass the shared half; okm: ... and the current group's hostname item (none yet)
      const u32 rbw = E.w[lane];
      const u32 rprm = RL(rbw, 8);
      const u64 rchg = (u64)RL(mw, 2) | ((u64)RL(mw, 3) << 32), rvfy = (u64)RL(mw, 4) | ((u64)RL(mw, 5) << 32);
      u32 done = 0, stepno = 0;
#ifdef KS_PROBES
      const u64 trun0 = __builtin_readcyclecounter(); u64 tx = trun0;
#define RRT(i) do { const u64 t_ = __builtin_readcyclecounter(); rrp[(i)] += t_ - tx; tx = t_; } while (0)
#else
#define RRT(i) do { } while (0)
#endif
      RRT(0);
      while (done < run) {
        u32 g_i0, g_i1;
        const u32 glen = rr_run_group(L.runitem[par], lane, done, run - done, g_i0, g_i1);
        RRT(5);
        if (g_i0 != cur_item || g_i1 != cur_item1) {
          // the next pods carry other hostname items: they are applied to the shared half's masks
          cur_item = g_i0; cur_item1 = g_i1; nhost = (g_i0 >> 31) + (g_i1 >> 31);
          hit0 = g_i0 & 0xFFFFu; hlim0 = RR_ITEM_LIM(g_i0); hit1 = g_i1 & 0xFFFFu; hlim1 = RR_ITEM_LIM(g_i1);
          u32 rej = 0;
          if (nhost > 0) RR_HOST_ITEM(RR_HOST_ALL, hit0, hlim0)
          if (nhost > 1) RR_HOST_ITEM(RR_HOST_ALL, hit1, hlim1)
          okm = okb & ~rej;
        }
        RRT(6);
        const u32 rem = min(run - done, glen), sp = stepno & 1u;
        // this wave's smallest accepting keys, within the count bucket of its smallest
        u32 kk[RR_NPL];
#pragma unroll
        for (int i = 0; i < RR_NPL; ++i) kk[i] = n_key[i] | (u32)(((i32)((okm >> i) & 1u)) - 1);
        RRT(7);
        u32 lb = kk[0];
#pragma unroll
        for (int i = 1; i < RR_NPL; ++i) lb = min(lb, kk[i]);
        u32 km = wave_min_u32(lb);             // ONE wave minimum names the bucket
        const u32 b0 = km >> 22;
        u32 pubw = 0, pubm = 0;                // what THIS lane publishes: its slots (bits 0..7) and, three bits a slot from bit 8 on, their places among the wave's entries | pubm: the slots any lane of the wave publishes from
        bool one_by_one = true;
        if (km != 0xFFFFFFFFu && b0 != 0u) {
          // new nodes lead (an existing node's key has count field 0, a new node's is >= 1): which lanes hold an accepting key of the bucket, slot by slot
          u64 mb[RR_NPL]; u32 total = 0;
#pragma unroll
          for (int i = 0; i < RR_NPL; ++i) { mb[i] = ballot64(kk[i] != 0xFFFFFFFFu && (kk[i] >> 22) == b0); total += (u32)__builtin_popcountll(mb[i]); }
          if (total <= 8u) {
            // ... at most eight: every one is published by the lane that holds it, at the place the ballots give it (slot by slot, lane by lane -- NOT in key
            // order: the merge ranks by counting and does not mind).  Nothing here waits for the key before.
            one_by_one = false;
            const u64 below = (1ull << lane) - 1ull;
            u32 base = 0;
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) {
              if ((mb[i] >> lane) & 1ull) {
                const u32 pl = base + (u32)__builtin_popcountll(mb[i] & below);
                L.stepk[sp][wk_i][pl] = ((u64)kk[i] << 32) | (u64)(((n_meta[i] & 0xFFu) << 16) | RR_NODE_AT((u32)i, wk_i, lane));
                pubw |= (1u << i) | (pl << (8 + 3 * i));
              }
              base += (u32)__builtin_popcountll(mb[i]); pubm |= mb[i] ? 1u << i : 0u;
            }
            if (lane < 8 && (u32)lane >= total) L.stepk[sp][wk_i][lane] = ~0ull;
          }
        }
        if (one_by_one) {
          // an existing node leads (it alone is published: a step that starts with an existing node ends with it), or the wave holds more than eight of the bucket:
          // its eight smallest, one wave minimum each, the last of them flagged (bit 31 of the low word: the wave holds more in this bucket)
          u32 myk = 0xFFFFFFFFu, mypay = 0;
          if (km != 0xFFFFFFFFu) for (u32 r = 0;;) {
            const int wl = __builtin_ctzll(ballot64(lb == km));
            const u32 ws = km & 7u;
            u32 bm = 0;
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) if ((u32)i == ws) bm = n_meta[i];
            const u32 nd = RR_NODE_AT(ws, wk_i, wl);
            const u32 bmu = RL(bm, wl);
            if ((u32)lane == r) { myk = km; mypay = ((bmu & 0xFFu) << 16) | nd | (r == 7u ? 1u << 31 : 0u); }
            if (lane == wl) pubw |= (1u << ws) | (r << (8u + 3u * ws));
            pubm |= 1u << ws;
            if (b0 == 0u || ++r >= 8u || r >= rem) break;
#pragma unroll
            for (int i = 0; i < RR_NPL; ++i) if ((u32)i == ws) kk[i] = lane == wl ? 0xFFFFFFFFu : kk[i];      // (the key names its slot: one register to touch)
            lb = kk[0];
#pragma unroll
            for (int i = 1; i < RR_NPL; ++i) lb = min(lb, kk[i]);
            km = wave_min_u32(lb);
            if (km == 0xFFFFFFFFu || (km >> 22) != b0) break;
          }
          if (lane < 8) L.stepk[sp][wk_i][lane] = ((u64)myk << 32) | mypay;
        }
        RRT(1);
        __syncthreads();
        RRT(2);
        u32 wkey, wpay, kind, snode, snrc;
        u32 mrank;
        const u32 n_step = rr_step_merge(L.stepk[sp], L.mrg[wv], lane, rem, nE, rvfy, wkey, wpay, kind, snode, snrc, mrank);
        RRT(3);
        // ---- COMMIT the step's pods, each by the lane that holds its node: slot by slot (one, as a rule: the nodes of a bucket were opened one after the other),
        // all the winners a slot holds side by side.  A lane knows the place of what it published, the place names the entry, the merge has ranked the entry. ----
        u32 ts = 0;
        for (u32 sb = pubm; sb; sb &= sb - 1u) {
          const u32 oslot = (u32)__builtin_ctz(sb);
          const u32 j = __shfl(mrank, (int)(wk_i * 8u + ((pubw >> (8u + 3u * oslot)) & 7u)));      // (the step's j-th pod, if j < n_step)
          const bool mine = ((pubw >> oslot) & 1u) != 0u && j < n_step;
          if (!ballot64(mine)) continue;
          ts |= 1u << oslot;
          const u32* const rpw = (const u32*)&L.runtab[par][done + (mine ? j : 0u)];      // the pod's record (pod, class, nh, hs[12]), read by the lane that commits it
          const u32 pseq = seq0 + done + j, nh = mine ? rpw[2] : 0u;
          if (mine) { const u32 pd = rpw[0]; tb.pod_node[pd] = (i32)RR_NODE_AT(oslot, wk_i, (u32)lane); tb.pod_seq[pd] = (i32)pseq; G_pod_reason[pd] = 0; }
#define RR_RCOMMIT_SLOT(i) if (oslot == (i)) { \
            const u32 nrc = n_meta[i] & 0xFFu, chw = rchg ? __shfl(mw, (int)(8u + ((nrc >> 2) & 15u))) : 0u;      /* (the child byte of the run's answers, if any nrc has one) */ \
            if (mine) { \
              const u32 nrc_new = ((rchg >> nrc) & 1ull) ? ((chw >> (8u * (nrc & 3u))) & 0xFFu) : nrc; \
              n_room[i][0] -= rq0; n_room[i][1] -= rq1; n_room[i][2] -= rq2; n_room[i][3] -= rq3; \
              if (b0 != 0u) { \
                n_key[i] = (((n_key[i] >> 22) + 1u) << 22) | ((RR_SEQMAX - pseq) << 3) | (n_key[i] & 7u); \
                if (nrc_new != nrc) { n_room[i][0] += nt.cap[0][nrc_new] - nt.cap[0][nrc]; n_room[i][1] += nt.cap[1][nrc_new] - nt.cap[1][nrc]; n_room[i][2] += nt.cap[2][nrc_new] - nt.cap[2][nrc]; n_room[i][3] += nt.cap[3][nrc_new] - nt.cap[3][nrc]; } } \
              n_meta[i] = nrc_new | ((((n_meta[i] >> 8) | rprm) & 0xFFu) << 8); \
              for (u32 t = 0; t < nh; ++t) {       /* Topology.Record on the hostname-keyed groups that count the pod: this node's own counters */ \
                const u32 hs = ((const u8*)rpw)[12u + t], sh8 = 8u * (hs & 3u); \
                switch (hs >> 2) { RR_HREC_WORD(i, 0) RR_HREC_WORD(i, 1) RR_HREC_WORD(i, 2) RR_HREC_WORD(i, 3) RR_HREC_WORD(i, 4) RR_HREC_WORD(i, 5) RR_HREC_WORD(i, 6) RR_HREC_WORD(i, 7) default: break; } \
              } } }
          RR_RCOMMIT_SLOT(0) RR_RCOMMIT_SLOT(1) RR_RCOMMIT_SLOT(2) RR_RCOMMIT_SLOT(3) RR_RCOMMIT_SLOT(4) RR_RCOMMIT_SLOT(5) RR_RCOMMIT_SLOT(6) RR_RCOMMIT_SLOT(7)
        }
        RR_HZ_FLUSH()
        // the slots in which nodes of this wave took pods: against the run's class again, as they are now
        if (ts) {
          u32 rej = 0, rejh = 0;
#define RR_RETRY_SLOT(i) if ((ts >> (i)) & 1u) { RR_EVAL_SLOT(i) }
          RR_RETRY_SLOT(0) RR_RETRY_SLOT(1) RR_RETRY_SLOT(2) RR_RETRY_SLOT(3) RR_RETRY_SLOT(4) RR_RETRY_SLOT(5) RR_RETRY_SLOT(6) RR_RETRY_SLOT(7)
          okb = (okb & ~ts) | (~rej & ts);
          if (nhost) { rej = 0;
#define RR_RETRYH_SLOT(i) if ((ts >> (i)) & 1u) { RR_HOST_ITEM(RR_HOST_AT_##i, hit0, hlim0) if (nhost > 1) RR_HOST_ITEM(RR_HOST_AT_##i, hit1, hlim1) }
            RR_RETRYH_SLOT(0) RR_RETRYH_SLOT(1) RR_RETRYH_SLOT(2) RR_RETRYH_SLOT(3) RR_RETRYH_SLOT(4) RR_RETRYH_SLOT(5) RR_RETRYH_SLOT(6) RR_RETRYH_SLOT(7)
            rejh = rej; }
          okm = (okm & ~ts) | (okb & ~rejh & ts);
        }
        RRT(4);
        done += n_step; ++stepno;
        if (kind != 0) { stop_kind = kind; stop_node = snode; break; }
      }
    }
    if (stop_kind == 3) {
      // the winner needs the exact filter (the leader runs it): its owner says what the node has requested so far
      const u32 oslot = RR_NODE_SLOT(stop_node), owv = RR_NODE_WV(stop_node), olane = RR_NODE_LANE(stop_node);
      if (owv == wv) {
        u32 bmeta = 0; i64 broom[4] = {0, 0, 0, 0};
#pragma unroll
        for (int i = 0; i < RR_NPL; ++i) if ((u32)i == oslot) { bmeta = n_meta[i]; broom[0] = n_room[i][0]; broom[1] = n_room[i][1]; broom[2] = n_room[i][2]; broom[3] = n_room[i][3]; }
        if ((u32)lane == olane) { L.ask.meta = bmeta; L.ask.room[0] = broom[0]; L.ask.room[1] = broom[1]; L.ask.room[2] = broom[2]; L.ask.room[3] = broom[3]; }
      }
      __syncthreads();
    }
    if (RL(hdw, RRH_HINT)) { const u32 ql = RL(hdw, RRH_QL); pf_n = ql > nb ? min(ql - nb, RR_RING - 2u) : 0u; pf_pos = pos0 + nb; pf_qi = RL(hdw, RRH_QH) + nb; pf_gam = (u64)RL(hdw, RRH_GAM) | ((u64)RL(hdw, RRH_GAM + 1) << 32); }
    RRP(14);
    ++round;
  }
  // the workers hand their nodes over (new nodes only): nrc | requested-resource mask << 8, headroom
  {
    GA u64* const dump = (GA u64*)P.rr_nodes;      // [node][5]: meta, room[4]
#pragma unroll
    for (int i = 0; i < RR_NPL; ++i) {
      const u32 n = RR_NODE_AT((u32)i, wk_i, lane);
      if (n_key[i] != 0xFFFFFFFFu && n >= nE) { dump[(size_t)n * 5] = n_meta[i]; for (int r = 0; r < 4; ++r) dump[(size_t)n * 5 + 1 + r] = (u64)n_room[i][r]; }
    }
    __threadfence_block(); GSYNC();
  }
#if defined(KS_SIM) || defined(KS_CHECK)      /* self check of the census of zero counters: every node takes its zero counters out again -- what is left must be nothing */
#pragma unroll
  for (int i = 0; i < RR_NPL; ++i) if (n_key[i] != 0xFFFFFFFFu) for (u32 h = 0; h < tb.GH; ++h) {
    u32 b = 1;
#pragma unroll
    for (int w = 0; w < RR_GW; ++w) if ((h >> 2) == (u32)w) b = (n_hc[i][w] >> (8 * (h & 3u))) & 0xFFu;
    if (b == 0u) atomicAdd(&L.hz[h & 31u], -1);
  }
#endif
#ifdef KS_PROBES
  if (wv == 1 && lane == 0) for (int i = 0; i < 16; ++i) L.wst[i] = rrp[i];
#endif
}

// types / caps / dominance of nrc `id` (a new-node nrc): node.go:137-159 without the resource test
__device__ __attribute__((noinline)) void rr_build_types(const int lane, const u32 id) {
  RR_CTX;
    const i32 m = (i32)UF((u32)nt.tmpl[id]); const u32 pres = UF(nt.present[id]), comp = UF(nt.complement[id]); const i32 its = (i32)UF((u32)nt.it[id]);
    u64 allowZ = ~0ull, allowC = ~0ull;
    if (tb.key_zone >= 0 && ((pres >> tb.key_zone) & 1u)) { KReq z; z.present = true; z.complement = (comp >> tb.key_zone) & 1u; z.mask = nt.mask[tb.key_zone][id]; z.gt = KS_NOGT; z.lt = KS_NOLT; allowZ = kreq_has_mask(z, tb.value_int + tb.key_zone * 64, tb.key_nvalues[tb.key_zone]); }
    if (tb.key_ct >= 0 && ((pres >> tb.key_ct) & 1u)) { KReq z; z.present = true; z.complement = (comp >> tb.key_ct) & 1u; z.mask = nt.mask[tb.key_ct][id]; z.gt = KS_NOGT; z.lt = KS_NOLT; allowC = kreq_has_mask(z, tb.value_int + tb.key_ct * 64, tb.key_nvalues[tb.key_ct]); }
    for (u32 wbase = 0; wbase < nTW; wbase += 64) {
      const u32 w = wbase + lane;
      if (w < nTW) {
        u64 a = GC(u64, P.tmpl_types)[(size_t)m * nTW + w] & G_its_types[(size_t)its * nTW + w];
        for (u32 bits = pres; bits; bits &= bits - 1) {
          const int k = __builtin_ctz(bits);
          KReq B; B.present = true; B.complement = (comp >> k) & 1u; B.mask = nt.mask[k][id]; B.gt = KS_NOGT; B.lt = KS_NOLT;
          a &= pass_types_word(P, tb, k, B, w);
        }
        if (tb.n_ct != 0) {
          u64 acc = 0; const u64 cm = allowC & ((1ull << tb.n_ct) - 1);
          for (u64 zz = allowZ; zz; zz &= zz - 1) { const int z = __builtin_ctzll(zz); if ((u32)z * tb.n_ct >= 64) break; for (u64 cb = cm; cb; cb &= cb - 1) acc |= G_pair_types[((size_t)z * tb.n_ct + __builtin_ctzll(cb)) * nTW + w]; }
          a &= acc;
        }
        rr_types[(size_t)id * nTW + w] = a;
      }
    }
    GSYNC();
    i64 mx[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) mx[r] = INT64_MIN;
    for (u32 t = lane; t < nTW * 64; t += 64) {
      const bool on = t < tb.T && ((rr_types[(size_t)id * nTW + (t >> 6)] >> (t & 63)) & 1ull);
#pragma unroll
      for (int r = 0; r < 4; ++r) if ((u32)r < nR && on) { const i64 al = P.it_alloc[(size_t)r * tb.T + t]; if (al > mx[r]) mx[r] = al; }
    }
    i64 cap[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) { cap[r] = wave_max_i64(mx[r]); if ((u32)r >= nR) cap[r] = 0; if (lane == 0) nt.cap[r][id] = cap[r]; }      // (a resource the problem does not have: headroom 0, requests 0)
    bool dom = false;
    for (u32 t0 = 0; t0 < nTW * 64; t0 += 64) {
      const u32 t = t0 + lane;
      bool all = t < tb.T && ((rr_types[(size_t)id * nTW + (t >> 6)] >> (t & 63)) & 1ull);
#pragma unroll
      for (int r = 0; r < 4; ++r) if ((u32)r < nR && all && P.it_alloc[(size_t)r * tb.T + t] != cap[r]) all = false;
      if (ballot64(all)) dom = true;
    }
    if (lane == 0) nt.dominant[id] = dom ? 1u : 0u;
    LSYNC();
}

// the domains nrc n's requirement on key dk allows (Requirements.Get of a missing key is Exists: every domain -- unless the key is a custom label, which a record must define)
__device__ __forceinline__ u64 rr_dy_nd(const RRNrc& nt, const FastTabs& ft, const u32 n, const u32 dk, const u32 wellknown) {
  const bool pres = (nt.present[n] >> dk) & 1u;
  KReq nd = kreq_exists();
  if (pres) { nd.present = true; nd.complement = (nt.complement[n] >> dk) & 1u; nd.mask = nt.mask[dk][n]; nd.gt = KS_NOGT; nd.lt = KS_NOLT; }
  const u64 ND = kreq_has_mask(nd, ft.value_int + dk * 64, ft.key_nvalues[dk]);
  return (pres || ((wellknown >> dk) & 1u)) ? ND : 0ull;
}
// does a node of nrc a that becomes nrc c need the exact instance-type filter?  (what form_one's `v` says: c has no type holding every maximum, or other maxima than a)
__device__ __forceinline__ bool rr_vrel(const RRNrc& nt, const u32 a, const u32 c, const u32 nR) {
  if (nt.tmpl[a] < 0) return false;
  bool v = !nt.dominant[c];
  for (u32 r = 0; r < nR; ++r) if (nt.cap[r][c] != nt.cap[r][a]) v = true;
  return v;
}
// intern the candidate record nt.n* (wave-uniform): the id of an equal nrc, else a new one (0xFFFFFFFF: table full)
__device__ __attribute__((noinline)) u32 rr_intern(const int lane) {
  RR_CTX;
  const u32 n_nrc = UF(L.n_nrc);
    LSYNC();
    bool eq = (u32)lane < n_nrc && nt.taints[lane] == nt.ntaints && nt.present[lane] == nt.npresent && nt.complement[lane] == (nt.ncomplement & nt.npresent) && nt.tmpl[lane] == nt.ntmpl && nt.it[lane] == nt.nit;
    for (u32 k = 0; k < nK; ++k) if (eq && ((nt.npresent >> k) & 1u) && nt.mask[k][lane] != nt.nmask[k]) eq = false;
    const u64 hit = ballot64(eq);
    if (hit) return (u32)__builtin_ctzll(hit);
    if (n_nrc >= RR_NRC - 1) return 0xFFFFFFFFu;      // (id 63: "takes nothing", an existing node that is over its allocatable)
    const u32 id = n_nrc;
    if (lane == 0) { nt.taints[id] = nt.ntaints; nt.present[id] = nt.npresent; nt.complement[id] = nt.ncomplement & nt.npresent; nt.tmpl[id] = nt.ntmpl; nt.it[id] = nt.nit; nt.nchild[id] = 0; nt.dominant[id] = 1; }
    if ((u32)lane < RR_KMAX) nt.mask[lane][id] = ((u32)lane < nK && ((nt.npresent >> lane) & 1u)) ? nt.nmask[lane] : 0ull;
    if (lane < 4) nt.cap[lane][id] = 0;
    LSYNC();
    if (lane == 0) L.n_nrc = id + 1;
    LSYNC();
    if (UF((u32)nt.ntmpl) != 0xFFFFFFFFu) rr_build_types(lane, id);
    // the head window's per-nrc tables: the new record's row and column of the exact-filter relation, its allowed domains on the dyn keys
    {
      LSYNC();
      const bool in = (u32)lane <= id;
      const bool v_to = in && rr_vrel(nt, (u32)lane, id, nR), v_from = in && rr_vrel(nt, id, (u32)lane, nR);
      if (in && (u32)lane != id) L.vpair[lane] |= (u64)(v_to ? 1u : 0u) << id;
      const u64 row = ballot64(v_from);
      if (lane == 0) L.vpair[id] = row;
      if (lane < 2 && L.dynk[lane] != 0xFFu) L.dy_nd[lane][id] = rr_dy_nd(nt, ft, id, L.dynk[lane], tb.wellknown);
      LSYNC();
    }
    return id;
}

// The class plan cidx staged in LDS, evaluated against nrcs [lo, hi) -- or against the single nrc `single` on lane 0 (merged: a fresh node) -- and every accepting
// lane's transition resolved.  Per lane: child | accepts << 8 | (rc & 0xFF) << 16; bit 31 (every lane): the nrc table overflowed.  skip: the narrow-key
// topology items are left aside (the static half of a dyn1 class).
__device__ __attribute__((noinline)) u32 rr_phase_a(const int lane, const u32 cidx, const u32 lo, const u32 hi, const bool merged, const u32 single, const bool skip) {
  RR_CTX;
  ClsRT<4> cr;
  {
    if (UF(L.staged_cls) != cidx) {
      const GA u32x4* src = (const GA u32x4*)(plans + cidx); u32x4* dst = (u32x4*)&sh.cls;
      dst[lane] = src[lane]; if ((u32)lane + 64 < KS_PLAN_V) dst[lane + 64] = src[lane + 64];
      LSYNC(); if (lane == 0) L.staged_cls = cidx;
    }
    stage_class<false>(tb, sh, lane);      // (the per-pod, node-independent part of the topology items: domainMinCount; re-done every time: the counters move)
    const ClsPlan& c = sh.cls;
    cr.tol = UF64(c.tol); cr.reqmask = UF(c.reqmask); cr.ntouch = UF(c.ntouch); cr.nhost = 0; cr.hn_mode = 0; cr.port_cnt = 0; cr.vol_cnt = 0; cr.it_state = 0; cr.tkeys = UF64(c.tkeys); cr.eq = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) cr.req[i] = 0;
  }
  {
    const bool active = merged ? lane == 0 : ((u32)lane >= lo && (u32)lane < hi);
    const u32 ni = merged ? single : (u32)lane;
    u32 tpres = 0, tcomp = 0, tchg = 0; int rc = 0;
    if (active) rc = merged ? rr_eval<true>(tb, sh, nt, ni, lane, cr, false, tpres, tcomp, tchg) : rr_eval<false>(tb, sh, nt, ni, lane, cr, skip, tpres, tcomp, tchg);
    LSYNC();
    bool o_acc = active && rc == 2; u32 o_child = ni;
    u32 chgkeys = 0;
    for (u32 i = 0; i < cr.ntouch; ++i) if ((tchg >> i) & 1u) chgkeys |= 1u << ((u32)(cr.tkeys >> (5 * i)) & 31u);
    bool need = o_acc && chgkeys != 0;
    if (need) {      // the transition cache of this nrc
      const u32 nch = nt.nchild[ni];
      for (u32 cc = 0; cc < nch && need; ++cc) {
        if (nt.cdiff[cc][ni] != chgkeys) continue;
        const u32 cid = nt.child[cc][ni]; bool same = true;
        for (u32 i = 0; i < cr.ntouch; ++i) if ((tchg >> i) & 1u) {
          const u32 k = (u32)(cr.tkeys >> (5 * i)) & 31u;
          if (nt.mask[k][cid] != sh.la_mask[i][lane] || ((nt.present[cid] >> k) & 1u) != ((tpres >> i) & 1u) || ((nt.complement[cid] >> k) & 1u) != ((tcomp >> i) & 1u)) same = false;
        }
        if (same) { o_child = cid; need = false; }
      }
    }
    for (u64 todo = ballot64(need); todo; todo &= todo - 1) {      // transitions seen for the first time: intern the new record (one lane at a time)
      const int l = __builtin_ctzll(todo);
      if (lane == l) {
        u32 np = nt.present[ni], nc = nt.complement[ni];
        for (u32 k = 0; k < nK; ++k) nt.nmask[k] = nt.mask[k][ni];
        for (u32 i = 0; i < cr.ntouch; ++i) if ((tchg >> i) & 1u) {
          const u32 k = (u32)(cr.tkeys >> (5 * i)) & 31u, kb = 1u << k;
          nt.nmask[k] = sh.la_mask[i][lane];
          np = ((tpres >> i) & 1u) ? (np | kb) : (np & ~kb); nc = ((tcomp >> i) & 1u) ? (nc | kb) : (nc & ~kb);
        }
        nt.npresent = np; nt.ncomplement = nc; nt.ntaints = nt.taints[ni]; nt.ntmpl = nt.tmpl[ni]; nt.nit = nt.it[ni];
      }
      const u32 id = rr_intern(lane);
      if (id == 0xFFFFFFFFu) return 0x80000000u;
      if (lane == l) {
        o_child = id;
        const u32 nch = nt.nchild[ni];
        if (nch < RR_CHILD) { nt.child[nch][ni] = (u8)id; nt.cdiff[nch][ni] = chgkeys; nt.nchild[ni] = nch + 1; }
      }
      LSYNC();
    }
    return (o_child & 0xFFu) | (o_acc ? 0x100u : 0u) | (((u32)rc & 0xFFu) << 16);
  }
}

// the exact instance-type filter for nrc `id` with requests `tot` over the resources in `rm` (node.go:137-159): any type left?
__device__ __attribute__((noinline)) bool rr_exact_fit(const int lane, const u32 id, const i64 t0, const i64 t1, const i64 t2, const i64 t3, const u32 rm) {
  RR_CTX;
  const i64 tot[4] = {t0, t1, t2, t3};
    PubT<4> pbx;
#pragma unroll
    for (int i = 0; i < 4; ++i) { pbx.req_new[i] = tot[i]; pbx.room_new[i] = 0; }
    u32 ridx[4]; ge_row_indices(tb, pbx, rm, lane, ridx);
    bool none = false;
#pragma unroll
    for (int i = 0; i < 4; ++i) if (((rm >> i) & 1u) && ridx[i] >= tb.ge_cnt[i]) none = true;
    if (none) return false;
    bool any = false;
    for (u32 wbase = 0; wbase < nTW; wbase += 64) {
      const u32 w = wbase + lane; u64 a = 0;
      if (w < nTW) {
        a = rr_types[(size_t)id * nTW + w];
#pragma unroll
        for (int i = 0; i < 4; ++i) if ((rm >> i) & 1u) a &= tb.ge_rows[((size_t)i * tb.T + ridx[i]) * nTW + w];
      }
      if (ballot64(a != 0)) any = true;
    }
    return any;
}

// One recorded group of a placed pod (w: the record word of its class brief; child: the nrc its node has now): Topology.Record on a narrow key (topology.go:120-143),
// counters updated atomically (several lanes may record side by side); per lane, no wave collectives.
__device__ __forceinline__ void rr_record_word(const DevProb& P, const Tabs& tb, const RRNrc& nt, const u32 nK, const u64 gam, const u32 w, const u32 child) {
  const u32 g = w & 0xFFu, key = (w >> 8) & 0xFFu, ty = (w >> 16) & 0xFFu, oi = (w >> 24) & 1u, flt = (w >> 25) & 1u;
  bool go = oi || ((gam >> g) & 1ull);
  if (go && !oi && flt) {      // TopologyGroup.Counts: the node filter against the node's requirements (topologynodefilter.go:57-70)
    const u32 b = G_grp_filter_off[g], e = G_grp_filter_off[g + 1]; bool anyf = b == e;
    for (u32 f = b; f < e && !anyf; ++f) {
      bool okf = true; const u32 fp = P.flt.present[f], fc = P.flt.complement[f];
      for (u32 bits = fp; bits && okf; bits &= bits - 1) {
        const int k = __builtin_ctz(bits);
        KReq a; a.present = (nt.present[child] >> k) & 1u; a.complement = (nt.complement[child] >> k) & 1u; a.mask = nt.mask[k][child]; a.gt = KS_NOGT; a.lt = KS_NOLT;
        const KReq in = load_req(fp, fc, P.flt.mask + (size_t)f * nK, P.flt.gt + (size_t)f * nK, P.flt.lt + (size_t)f * nK, k);
        if (kreq_compatible_fail(a, in, (tb.wellknown >> k) & 1u, tb.value_int + k * 64, tb.key_nvalues[k])) okf = false;
      }
      if (okf && P.flt.it_state[f] != 0) okf = false;
      if (okf) anyf = true;
    }
    go = anyf;
  }
  if (go && ((nt.present[child] >> key) & 1u)) {
    const u64 qm = nt.mask[key][child]; const bool qc = (nt.complement[child] >> key) & 1u;
    if (oi || ty == 2) { for (u64 bb = qm; bb; bb &= bb - 1) grp_record<true>(tb, (int)g, __builtin_ctzll(bb)); }
    else if (!qc && __builtin_popcountll(qm) == 1) grp_record<true>(tb, (int)g, __builtin_ctzll(qm));
  }
}


__device__ __attribute__((noinline)) void rr_window_gen(const int lane) {
  RR_CTX;
  u32 q_head = UF(L.wx[0]), q_pos = UF(L.wx[1]), q_len = UF(L.wx[2]), seq = UF(L.wx[3]), wpods = 0, stop = 0;
  u32 n_nrc = UF(L.wx[5]); const u32 T = UF(L.wx[6]), dk0 = UF(L.wx[8]), dk1 = UF(L.wx[9]);
  const u64 gam = UF64(L.wx_gam);
  const bool w_act = (UF64(L.wx_act) >> lane) & 1ull;
  u32 w_key = w_act ? L.wn_key[lane] : 0xFFFFFFFFu, w_meta = L.wn_meta[lane]; const u32 w_node = L.wn_own[lane]; i64 w_room[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) w_room[r] = L.wn_room[r][lane];
  u8* const hcb = (u8*)L.wn_hc + ((u32)lane << 2);      // this lane's hostname counters: counter h at hcb[(h >> 2) * 256 + (h & 3)]
  const bool w_new = w_node >= nE;
#ifdef KS_PROBES
  u64 wrp[8]; for (int i = 0; i < 8; ++i) wrp[i] = 0; u64 wrp_t = __builtin_readcyclecounter();
#define WRP(i) do { const u64 t_ = __builtin_readcyclecounter(); wrp[(i)] += t_ - wrp_t; wrp_t = t_; } while (0)
#else
#define WRP(i) do { } while (0)
#endif
  // the class records of the next queue entries, 16 at once (what the leader's ring_load / ring_store do one at a time): every load of the block is in flight together
  auto wprep = [&]() {
    const u32 cnt = min(16u, q_len);
    u32 idx = q_head + (u32)lane; if (idx >= nP) idx -= nP; if (idx >= nP) idx = 0;
    const u64 e = (u32)lane < cnt ? tb.q[idx] : 0ull; const u32 cls = (u32)(e >> 32) & 0x7FFFFFFFu; const u32 mi = (u32)lane < cnt ? rr_mi[cls] : 0u;
    u32 b[16], m[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) { b[t] = 0; m[t] = 0; if ((u32)t < cnt) { const u32 ct = RL(cls, t), mt = RL(mi, t); b[t] = (u32)lane < 48 ? rrb[(size_t)ct * 48 + lane] : (((u32)lane >= 54 && (u32)lane < 62) ? GC(u32, P.rr_hot)[(size_t)ct * 8 + lane - 54] : 0u); m[t] = (u32)lane < 24 ? rrm[(size_t)mt * 24 + lane] : 0u; } }
#pragma unroll
    for (int t = 0; t < 16; ++t) if ((u32)t < cnt) {
      const u32 pos = q_pos + (u32)t; RREntry& R = L.ring[pos & (RR_RING - 1u)];
      u32 bb = b[t]; const u64 et = RL64(e, t); const u32 mit = RL(mi, t);
      const u32 nh = RL(bb, 17); const bool on = (u32)lane >= 28u && (u32)lane < 28u + nh && (((bb >> 16) & 1u) || ((gam >> ((bb >> 8) & 63u)) & 1ull));      // hostname records that count (lane 28 + i holds record word i)
      const u32 hm = (u32)(ballot64(on) >> 28);
      if ((u32)lane == 48) bb = pos; else if ((u32)lane == 49) bb = (u32)(et >> 32) & 0x7FFFFFFFu; else if ((u32)lane == 50) bb = (u32)et; else if ((u32)lane == 51) bb = hm; else if ((u32)lane == 52) bb = (u32)(et >> 63); else if ((u32)lane == 53) bb = mit;
      R.w[lane] = bb; if ((u32)lane < 32) { R.m[lane] = m[t]; R.t1[lane] = m[t]; }
    }
    LSYNC();
  };
  bool no_T = UF(L.wx[13]) != 0; u32 Tc = no_T ? 0xFFFFFFFFu : T;      // (the first pod against every node the window holds, whatever its key: the leader has asked the workers about theirs)
  const u32 wlimit = UF(L.wx[12]);        // (at most that many pods: the straight-line loop takes over again behind a pod it does not cover)
  for (;;) {
    if (q_len == 0) { stop = 1; break; }
    if (wpods >= wlimit) { stop = 8; break; }
    RREntry& E = L.ring[q_pos & (RR_RING - 1u)];
    // ---- the pod's parameters: LDS broadcast reads, all in flight together; ONE control word crosses to the scalar side:
    // 1 ready (prepared, not requeued, covered by this kernel, cached answers complete) | reads topology counters << 1 | ... through one spread << 2 | hostname items << 3 |
    // hostname records << 5 | narrow records << 9 | some nrc changes << 13 | prepared << 14 | answers incomplete << 15 ----
    u32x4 wa, wc, we, m0, m1; u32 c = 0;
    for (u32 attempt = 0; ; ++attempt) {
      wa = *(const u32x4*)&E.w[8];                   // requested-resource mask | flags | evaluation class | dyn1
      wc = *(const u32x4*)&E.w[16];                  // hostname items | hostname records | narrow records | dyn1: maxSkew
      we = *(const u32x4*)&E.w[48];                  // stream position | class | pod | hostname records that count
      const u32 rqd = E.w[52];
      m0 = *(const u32x4*)&E.t1[0]; m1 = *(const u32x4*)&E.t1[4];      // accepts | changes the nrc ; needs the exact filter | nrcs answered
      const bool prepared = we.x == q_pos, ready = prepared && rqd == 0 && !(wa.y & 2u) && m1.z == n_nrc;
      c = UF((ready ? 1u : 0u) | ((wa.y & 1u) << 1) | (((wa.y >> 2) & 1u) << 2) | ((wc.x & 3u) << 3) | ((wc.y & 15u) << 5) | ((wc.z & 15u) << 9) | ((m0.z | m0.w) ? 1u << 13 : 0u) | (prepared ? 1u << 14 : 0u) | (m1.z < n_nrc ? 1u << 15 : 0u));
      if ((c & 1u) || attempt) break;
      // not ready: the record is prepared now (a block of 16), or its class's cached answers are read again (another class that shares them may have met the new nrcs)
      if (!(c & (1u << 14))) wprep();
      else if (c & (1u << 15)) { const u32 mi = UF(E.w[53]); const u32 mw = (u32)lane < 24 ? rrm[(size_t)mi * 24 + lane] : 0u; LSYNC(); if ((u32)lane < 32) { E.m[lane] = mw; E.t1[lane] = mw; } LSYNC(); }
      else break;
      WRP(4);
    }
    if (!(c & 1u)) { stop = 2; break; }
    const u32 kind = (c >> 1) & 3u, nhost = (c >> 3) & 3u, nhrec = (c >> 5) & 15u, nnrec = (c >> 9) & 15u;
    if (kind == 1u) { stop = 2; break; }                 // a general topology class: the leader's formation answers it per pod
    WRP(0);
    const i64 rq0 = *(const i64*)&E.w[0], rq1 = *(const i64*)&E.w[2], rq2 = *(const i64*)&E.w[4], rq3 = *(const i64*)&E.w[6];
    const u32 nrc = w_meta & 63u;
    const u64 acc1 = (u64)m0.x | ((u64)m0.y << 32), chg1 = (u64)m0.z | ((u64)m0.w << 32), vfy1 = (u64)m1.x | ((u64)m1.y << 32);
    // what this lane's node answers: accepts | the nrc it would have | the winner would need the exact filter
    bool a_ok = (acc1 >> nrc) & 1ull; u32 a_child = nrc; bool a_vfy = (vfy1 >> nrc) & 1ull;
    if ((c >> 13) & 1u) a_child = ((chg1 >> nrc) & 1ull) ? (u32)((const u8*)&E.t1[8])[nrc] : nrc;
    if (kind == 3u) {
      // ---- dyn1: one spread on a narrow key, answered from the cached rest (above: without the item) and the group's counters -- nextDomainTopologySpread
      // (topologygroup.go:155-182) per lane for its node's requirement record, as form_one does per nrc ----
      const u32 dw = wa.w, dg = UF((dw >> 8) & 0xFFu), dk = UF((dw >> 16) & 0xFFu), dself = UF(dw >> 24); const i32 dskew = (i32)UF(wc.w);
      const u32 dks = dk == dk0 ? 0u : (dk == dk1 ? 1u : 2u);
      if (dks == 2u) { stop = 2; break; }
      const u64 dPD = UF64(*(const u64*)&E.w[26]);
      const u64 reg = UF64(ft.g_reg[dg]), gpos = UF64(ft.g_pos[dg]);
      if (!(reg == 0 && gpos == ~0ull)) {      // (a group that does not exist yet constrains nothing: the cached answers stand)
        const i32 cv = ft.gcnt[(size_t)dg * 64 + lane];      // lane d: domain d's count
        u32 mnc = 0x7FFFFFFFu;                               // domainMinCount over the pod's domains (:184-200)
        for (u64 bits = reg & dPD; bits; bits &= bits - 1) { const u32 cd = RL((u32)cv, (int)__builtin_ctzll(bits)); mnc = min(mnc, cd); }
        u64 EL = 0;
        for (u64 bits = reg; bits; bits &= bits - 1) { const int d = (int)__builtin_ctzll(bits); if ((i64)(i32)RL((u32)cv, d) + (i64)dself - (i64)(i32)mnc <= (i64)dskew) EL |= 1ull << d; }
        const u32 n1 = a_child;
        const bool pres = (nt.present[n1] >> dk) & 1u;
        KReq nd = kreq_exists();
        if (pres) { nd.present = true; nd.complement = (nt.complement[n1] >> dk) & 1u; nd.mask = nt.mask[dk][n1]; nd.gt = KS_NOGT; nd.lt = KS_NOLT; }
        const u64 ND = kreq_has_mask(nd, tb.value_int + dk * 64, tb.key_nvalues[dk]);
        const u64 mm = EL & ND;
        const bool ok = a_ok && mm != 0 && (pres || ((tb.wellknown >> dk) & 1u));
        i32 bestc = INT32_MAX; u32 dom = 0;
        for (u64 bits = EL; bits; bits &= bits - 1) {        // the least count, the first such domain
          const int d = (int)__builtin_ctzll(bits);
          const i32 cc = (i32)RL((u32)cv, d) + (i32)dself;
          if (((mm >> d) & 1ull) && cc < bestc) { bestc = cc; dom = (u32)d; }
        }
        const u32 child2 = ok ? (u32)L.t2[dks][n1][dom] : nrc;
        if (ballot64(w_act && w_key < Tc && ok && child2 == 0xFFu)) { stop = 2; break; }      // a narrowed record met for the first time: the leader interns it
        bool v = false;
        if (ok && nt.tmpl[nrc] >= 0) { if (!nt.dominant[child2 & 63u]) v = true; for (u32 r = 0; r < nR; ++r) if (nt.cap[r][child2 & 63u] != nt.cap[r][nrc]) v = true; }
        a_ok = ok; a_child = child2; a_vfy = v;
      }
    }
    WRP(1);
    bool rej = !a_ok || rq0 > w_room[0] || rq1 > w_room[1] || rq2 > w_room[2] || rq3 > w_room[3];
    if (nhost) {      // hostname-keyed items: the node's own counter against the item's limit (RR_HOST_SLOT)
      const u32x4 hw = *(const u32x4*)&E.w[20]; const u32x4 hk = *(const u32x4*)&E.w[24];      // items 0..2, maxSkew 0 | maxSkew 1, 2, ...
      { const u32 hs = (hw.x >> 16) & 0xFFu; const i32 lim = (hw.x & 0xFFu) == 0 ? (i32)hw.w - (i32)((hw.x >> 8) & 0xFFu) : 0; rej |= lim < (i32)(u32)hcb[(hs >> 2) * 256u + (hs & 3u)]; }
      if (nhost > 1u) { const u32 hs = (hw.y >> 16) & 0xFFu; const i32 lim = (hw.y & 0xFFu) == 0 ? (i32)hk.x - (i32)((hw.y >> 8) & 0xFFu) : 0; rej |= lim < (i32)(u32)hcb[(hs >> 2) * 256u + (hs & 3u)]; }
      if (nhost > 2u) { const u32 hs = (hw.z >> 16) & 0xFFu; const i32 lim = (hw.z & 0xFFu) == 0 ? (i32)hk.y - (i32)((hw.z >> 8) & 0xFFu) : 0; rej |= lim < (i32)(u32)hcb[(hs >> 2) * 256u + (hs & 3u)]; }
    }
    const bool inw = w_act && !rej && w_key < Tc;
    const u32 cand = inw ? w_key : 0xFFFFFFFFu;
    // (conservative: ANY candidate that would need the exact filter or has a full count field ends the phase -- decided beside the minimum, not behind it)
    const u64 odd = ballot64(inw && (a_vfy || (w_new && (w_key >> 22) >= RR_CNTMAX)));
    const u32 kmin = wave_min_u32(cand);
    WRP(2);
    if (kmin == 0xFFFFFFFFu) { stop = no_T ? 11u : 5u; break; }       // nothing in the window takes it: a round over all nodes decides
    if (odd) { stop = 6; break; }
    const bool mine = cand == kmin;
    // ---- COMMIT in the winner's lane (what RR_COMMIT_SLOT does in its owner's) ----
    const u32 pd = we.z;
    if (mine) {
      tb.pod_node[pd] = (i32)w_node; tb.pod_seq[pd] = (i32)seq; G_pod_reason[pd] = 0;
      i64 d0 = rq0, d1 = rq1, d2 = rq2, d3 = rq3;
      if (w_new && a_child != nrc) { d0 -= nt.cap[0][a_child] - nt.cap[0][nrc]; d1 -= nt.cap[1][a_child] - nt.cap[1][nrc]; d2 -= nt.cap[2][a_child] - nt.cap[2][nrc]; d3 -= nt.cap[3][a_child] - nt.cap[3][nrc]; }
      w_room[0] -= d0; w_room[1] -= d1; w_room[2] -= d2; w_room[3] -= d3;
      if (w_new) w_key = (((w_key >> 22) + 1u) << 22) | ((RR_SEQMAX - seq) << 3) | (w_key & 7u);
      w_meta = a_child | ((((w_meta >> 8) | wa.x) & 0xFFu) << 8);
    }
    for (u32 t = 0; t < nhrec; ++t) {      // Topology.Record on the hostname-keyed groups that count the pod: the node's own counters
      const u32 wd = E.w[28 + t], hs = wd & 0xFFu;
      if (mine && (((wd >> 16) & 1u) || ((gam >> ((wd >> 8) & 63u)) & 1ull))) { u8& cb = hcb[(hs >> 2) * 256u + (hs & 3u)]; const u32 cc = cb; cb = (u8)(cc == 0xFFu ? 1u : (cc >= 254u ? 254u : cc + 1u)); if (cc == 0u) atomicAdd(&L.hz[hs & 31u], -1); }
    }
    for (u32 t = 0; t < nnrec; ++t) {      // ... and on the narrow keys (topology.go:120-143)
      const u32 wd = E.w[40 + t];
      if (mine) rr_record_word(P, tb, nt, nK, gam, wd, a_child);
    }
    LSYNC();                              // (the winner's counters and records are what the other lanes read for the next pod)
    q_head = (q_head + 1 == nP) ? 0 : q_head + 1; ++q_pos; --q_len; ++seq; ++wpods; Tc = T; no_T = false;
    WRP(3);
  }
  // ---- the nodes' state back into the window's arrays (the leader hands them to their owners, or calls again) ----
  if (w_act) { L.wn_key[lane] = w_key; L.wn_meta[lane] = w_meta;
#pragma unroll
    for (int r = 0; r < 4; ++r) L.wn_room[r][lane] = w_room[r]; }
  if (lane == 0) { u32* const x = L.wx; x[0] = q_head; x[1] = q_pos; x[2] = q_len; x[3] = seq; x[4] += wpods; x[10] = stop; if (wpods) x[13] = 0;      // (the leader's "whatever its key" was for the FIRST pod: a call that placed pods has used it up -- the other window function, called next for the pod this one stopped at, must not read it again)
#ifdef KS_PROBES
    for (int i = 0; i < 8; ++i) L.wpr[i] += wrp[i];
#endif
  }
  LSYNC();
}

// The class records of the next 16 queue entries from (q_head, q_pos) on, every load of the block in flight together (what the leader's ring_load / ring_store do one at a time)
__device__ __attribute__((noinline)) void rr_wprep(const int lane, const u32 q_head, const u32 q_pos, const u32 q_len, const u64 gam) {
  RRLds& L = g_rr_lds; const DevProb& P = L.P; const DevState& S = L.S;
  const u32 nP = UF(P.P);
  const GA u64* const q = (const GA u64*)UF64((u64)S.q); const GA u32* const rrb = (const GA u32*)UF64((u64)P.rr_briefs); const GA u32* const rrm = (const GA u32*)UF64((u64)P.rr_memo);
  const GA u32* const rr_mi = (const GA u32*)UF64((u64)P.rr_mi); const GA u32* const hot = (const GA u32*)UF64((u64)P.rr_hot);
  const u32 cnt = min(16u, q_len);
  u32 idx = q_head + (u32)lane; if (idx >= nP) idx -= nP; if (idx >= nP) idx = 0;
  const u64 e = (u32)lane < cnt ? q[idx] : 0ull; const u32 cls = (u32)(e >> 32) & 0x7FFFFFFFu; const u32 mi = (u32)lane < cnt ? rr_mi[cls] : 0u;
  u32 b[16], m[16];
#pragma unroll
  for (int t = 0; t < 16; ++t) { b[t] = 0; m[t] = 0; if ((u32)t < cnt) { const u32 ct = RL(cls, t), mt = RL(mi, t); b[t] = (u32)lane < 48 ? rrb[(size_t)ct * 48 + lane] : (((u32)lane >= 54 && (u32)lane < 62) ? hot[(size_t)ct * 8 + lane - 54] : 0u); m[t] = (u32)lane < 24 ? rrm[(size_t)mt * 24 + lane] : 0u; } }
#pragma unroll
  for (int t = 0; t < 16; ++t) if ((u32)t < cnt) {
    const u32 pos = q_pos + (u32)t; RREntry& R = L.ring[pos & (RR_RING - 1u)];
    u32 bb = b[t]; const u64 et = RL64(e, t); const u32 mit = RL(mi, t);
    const u32 nh = RL(bb, 17); const bool on = (u32)lane >= 28u && (u32)lane < 28u + nh && (((bb >> 16) & 1u) || ((gam >> ((bb >> 8) & 63u)) & 1ull));      // hostname records that count (lane 28 + i holds record word i)
    const u32 hm = (u32)(ballot64(on) >> 28);
    if ((u32)lane == 48) bb = pos; else if ((u32)lane == 49) bb = (u32)(et >> 32) & 0x7FFFFFFFu; else if ((u32)lane == 50) bb = (u32)et; else if ((u32)lane == 51) bb = hm; else if ((u32)lane == 52) bb = (u32)(et >> 63); else if ((u32)lane == 53) bb = mit;
    R.w[lane] = bb; if ((u32)lane < 32) { R.m[lane] = m[t]; R.t1[lane] = m[t]; }
  }
  LSYNC();
}

// The head window's STRAIGHT-LINE loop (rr_window_gen above is the same algorithm for every class, written with control flow; this one takes the pods the class table
// marks simple -- no or one dyn1 topology item, at most two hostname items, two hostname records, one plain narrow record: every pod of BASELINE's generators -- and hands
// anything else to rr_window_gen, stop code 7).  Round 6: the pod arrives PREPARED (RRPx, by the worker waves, a few pods ahead): its requests, its hostname items
// and records as LDS offsets, and per requirement class what a node of that class answers -- what is left here is what depends on the pod before: the lanes' nodes against
// the requests and their own counters, the wave minimum over the accepting keys, the commit selected into the winner's lane (v_cndmask, no branch), the records.  A pod costs
// three branches: one on the control word, one on the wave minimum, the loop's.  The results (pod -> node, commit number) go to an LDS buffer and to memory 32 at a time.
__device__ __attribute__((noinline)) void rr_window_fast(const int lane) {
  RRLds& L = g_rr_lds; const DevProb& P = L.P; const DevState& S = L.S; const RRNrc& nt = L.nt; FastTabs& ft = L.ft;
  u32 q_head = UF(L.wx[0]), q_pos = UF(L.wx[1]), q_len = UF(L.wx[2]), seq = UF(L.wx[3]), wpods = 0, stop = 0, nres = 0;
  const u32 T = UF(L.wx[6]), nP = UF(P.P), nE = UF(P.E), n_nrc = UF(L.wx[5]);
  GA i32* const pod_node = (GA i32*)UF64((u64)S.pod_node); GA i32* const pod_seq = (GA i32*)UF64((u64)S.pod_seq); GA u32* const pod_reason = (GA u32*)UF64((u64)S.pod_reason);
  const bool w_act = (UF64(L.wx_act) >> lane) & 1ull;
  u32 w_key = w_act ? L.wn_key[lane] : 0xFFFFFFFFu, w_meta = L.wn_meta[lane]; const u32 w_node = L.wn_own[lane]; i64 w_room[4];
#pragma unroll
  for (int r = 0; r < 4; ++r) w_room[r] = L.wn_room[r][lane];
  u8* const hcb = (u8*)L.wn_hc + ((u32)lane << 2);      // this lane's hostname counters: counter h at hcb[(h >> 2) * 256 + (h & 3)]; RR_HC_ZERO / RR_HC_SINK: the zero row / the sink
  const bool w_new = w_node >= nE;
  u32 plain = 0, plain_base = 0xFFFFFFFFu, spins = 0;
  bool no_T = UF(L.wx[13]) != 0; u32 Tc = no_T ? 0xFFFFFFFFu : T;      // (the first pod against every node the window holds, whatever its key: the leader has asked the workers about theirs)
#ifndef KS_SIM
  __builtin_amdgcn_s_setprio(3);      // (the wave that shares the leader's SIMD yields the issue slot: 0.5 ms of 100)
#endif
#ifdef KS_PROBES
  u64 wrp[8]; for (int i = 0; i < 8; ++i) wrp[i] = 0; u64 wrp_t = __builtin_readcyclecounter();
#endif
  // results: the last pods' (pod, node, commit number) wait in LDS, 32 at a time go to memory (a store in the loop would have every pod wait for the one before it to reach memory)
  auto flush = [&]() { if ((u32)lane < nres) { const u32 pd = L.wres[lane][0]; pod_node[pd] = (i32)L.wres[lane][1]; pod_seq[pd] = (i32)L.wres[lane][2]; pod_reason[pd] = 0; } nres = 0; LSYNC(); };
  for (;;) {
    if (q_len == 0) { stop = 1; break; }
    RRPx& X = L.px[q_pos & (RR_PX - 1u)];
    RR_LDS_STORE(&L.wn_qpos, q_pos);      // (the assisting wave and the workers' class records follow this position)
    const u32 tag = RR_LDS_LOAD(&X.u[0]);      // the prepared pod's stream position before anything else of it: it is written last
    LSYNC();
    // ---- the prepared pod, all in flight together ----
    const u32 nrc = w_meta & 63u;
    u32x4 xa = *(const u32x4*)&X.u[0];                     // (stream position) | flags | nrcs it was made for | -
    i64 rq0 = *(const i64*)&X.u[4], rq1 = *(const i64*)&X.u[6], rq2 = *(const i64*)&X.u[8], rq3 = *(const i64*)&X.u[10];
    u32x4 xc = *(const u32x4*)&X.u[12];                    // hostname item 0 | item 1 | hostname records | pod
    u32 xg = X.u[16], plb = X.u[17];                       // requested-resource mask | dyn1 group << 8 | narrow record's group << 16 ; plain replica: its base class
    u32x4 xd = *(const u32x4*)&X.u[20];                    // dyn1: the pod's own count | maxSkew | the pod's domains
    u32 tw = X.t[nrc];                                     // what this lane's node answers, by its requirement class
    // (all of them requested HERE: left to itself the compiler sinks what only the pod's evaluation reads below the branch on the control word -- a second LDS round trip behind it)
    RR_KEEP(xa); RR_KEEP(rq0); RR_KEEP(rq1); RR_KEEP(rq2); RR_KEEP(rq3); RR_KEEP(xc); RR_KEEP(xg); RR_KEEP(plb); RR_KEEP(xd); RR_KEEP(tw);
    // a stretch of plain replicas: RUN rounds place those several per barrier (counted on the vector side: every lane holds the same numbers)
    const u32 plain_n = (plb != 0xFFFFFFFFu && plb == plain_base) ? plain + 1u : (plb != 0xFFFFFFFFu ? 1u : 0u);
    // ONE control word crosses to the scalar side (0: not prepared for this position and this nrc table; RR_PX_PLAIN: the eighth plain replica in a row)
    const u32 c = UF((tag == q_pos && xa.z == n_nrc) ? (xa.y | (plain_n >= RR_WIN_PLAIN ? RR_PX_PLAIN : 0u)) : 0u);
    if ((c & (RR_PX_GO | RR_PX_PLAIN)) != RR_PX_GO) {
      if (c & RR_PX_PLAIN) { stop = 9; break; }
      if (c & RR_PX_STOP7) { stop = 7; break; }      // rr_window_gen's (or the leader's)
      if (++spins > RR_SPIN_MAX) { stop = 2; break; }
#ifdef KS_PROBES      /* why the loop waits (tools/win_profile.py): the static part is not there | the dyn1 answers are not made | they are behind their group's version */
      { const u64 t_ = __builtin_readcyclecounter(); wrp[5] += t_ - wrp_t; wrp_t = t_; }
#endif
#ifdef KS_SIM
      if (lane == 0 && spins == 3000u && getenv("KS_SIM_DBG")) fprintf(stderr, "rr_window_fast waits: q_pos %u q_len %u tag %u flags %x nn %u (n_nrc %u) c %x ring tag %u\n", q_pos, q_len, tag, xa.y, xa.z, n_nrc, c, L.ring[q_pos & (RR_RING - 1u)].w[48]);
#endif
      RR_SPIN_PAUSE();
      continue;
    }
    WRP(0);
    plain = plain_n; plain_base = plb;
    // the counters the pod's items read and its records count into: this lane's bytes (the zero row / the sink where there is none) -- and, in the same trip, what a dyn1
    // pod's domain choice reads of its group (any pod: group 0's, unread)
    const u32 it0 = xc.x, it1 = xc.y, ho0 = xc.z & 0xFFFFu, ho1 = xc.z >> 16;
    u32 ci0 = hcb[it0 & 0xFFFFu], ci1 = hcb[it1 & 0xFFFFu];
    u32 ch0 = hcb[ho0], ch1 = hcb[ho1];
    const u32 dg = (xg >> 8) & 63u;
    u64 reg = ft.g_reg[dg], gpos = ft.g_pos[dg];
    u32x4 cnv = *(const u32x4*)&ft.gcnt[(size_t)dg * 64];
    RR_KEEP(ci0); RR_KEEP(ci1); RR_KEEP(ch0); RR_KEEP(ch1); RR_KEEP(reg); RR_KEEP(gpos); RR_KEEP(cnv);
    if (c & RR_PX_DYN) {
      // ---- dyn1: one spread on a narrow key.  The answers are prepared per domain (RRPx::td); WHICH domain is nextDomainTopologySpread (topologygroup.go:155-182) on the
      // group's counters as they stand now: the least count within the skew among the domains this lane's node allows, the first such -- over the first four domains
      // (every lane the same four counters; three zones are the common case), straight-line ----
      const i32 dself = (i32)xd.x, dskew = (i32)xd.y; const u32 dPD = xd.z;
      const bool exists = !(reg == 0 && gpos == ~0ull);      // (a group that does not exist yet constrains nothing: the cached answers stand)
      const i32 cn[4] = {(i32)cnv.x, (i32)cnv.y, (i32)cnv.z, (i32)cnv.w};
      const u32 regn = (u32)reg & 15u, inn = regn & dPD;
      i32 mnc = 0x7FFFFFFF;                                  // domainMinCount over the pod's domains (:184-200)
#pragma unroll
      for (int d = 0; d < 4; ++d) mnc = ((inn >> d) & 1u) && cn[d] < mnc ? cn[d] : mnc;
      const u32 ndr = regn & (tw >> 18);
      i32 bestc = INT32_MAX; u32 dom = 0; bool any = false;
#pragma unroll
      for (int d = 0; d < 4; ++d) {                          // (the counts are >= 0 and the pod's own 0 / 1: cc - mnc cannot leave 32 bits)
        const i32 cc = (i32)((u32)cn[d] + (u32)dself);
        const bool el = ((ndr >> d) & 1u) && (i32)((u32)cc - (u32)mnc) <= dskew;
        any = any || el; const bool better = el && cc < bestc; bestc = better ? cc : bestc; dom = better ? (u32)d : dom;
      }
      u32 te = X.td[nrc * 4u + dom]; RR_KEEP(te);            // the node narrowed to that domain: nrc | not answered << 6 | exact filter << 7 | narrow record counts << 8 | domain << 9
      const bool ok = ((tw >> 8) & 1u) && any;
      const u32 tn = ok ? ((te & 63u) | (1u << 8) | (((te >> 7) & 1u) << 9) | (((te >> 6) & 1u) << 10) | (((te >> 8) & 1u) << 11) | (((te >> 9) & 63u) << 12)) : nrc;      // (refused: nothing of the rest is read)
      const u32 unk = (tw & (1u << 10)) | ((exists && (reg >> 4) != 0) ? 1u << 10 : 0u);      // (a dyn key without a column; a fifth domain)
      tw = (exists ? tn : (tw & 0x3FFFFu)) | unk;
    }
    const bool a_ok = (tw >> 8) & 1u, a_vfy = (tw >> 9) & 1u, a_unk = (tw >> 10) & 1u; const u32 a_child = tw & 0xFFu;
    WRP(1);
    const bool rej = !a_ok || rq0 > w_room[0] || rq1 > w_room[1] || rq2 > w_room[2] || rq3 > w_room[3] || (i32)(int16_t)(it0 >> 16) < (i32)ci0 || (i32)(int16_t)(it1 >> 16) < (i32)ci1;
    const bool inw = w_act && !rej && w_key < Tc;
    const u32 cand = inw ? w_key : 0xFFFFFFFFu;
    // (conservative: ANY candidate that would need the exact filter or has a full count field, any node whose class is not answered here ends the phase -- decided beside the minimum, not behind it)
    const u64 odd = ballot64((inw && (a_vfy || (w_new && (w_key >> 22) >= RR_CNTMAX))) || (w_act && a_unk));
    const u32 kmin = wave_min_u32(cand);
    if (kmin == 0xFFFFFFFFu || odd) { stop = odd ? 6u : (no_T ? 11u : 5u); break; }      // nothing in the window takes it / the exact filter: a round over all nodes decides
    WRP(2);
    const bool mine = cand == kmin;
    // ---- COMMIT, selected into the winner's lane (what RR_COMMIT_SLOT does in its owner's) ----
    i64 d0 = rq0, d1 = rq1, d2 = rq2, d3 = rq3;
    if (c & RR_PX_CHG) {      // (a class that changes no nrc skips the capacity difference)
      const u32 ac = a_child & 63u; const bool moved = w_new && ac != nrc;
      const i64 e0 = nt.cap[0][ac] - nt.cap[0][nrc], e1 = nt.cap[1][ac] - nt.cap[1][nrc], e2 = nt.cap[2][ac] - nt.cap[2][nrc], e3 = nt.cap[3][ac] - nt.cap[3][nrc];
      d0 -= moved ? e0 : 0; d1 -= moved ? e1 : 0; d2 -= moved ? e2 : 0; d3 -= moved ? e3 : 0;
    }
    w_room[0] -= mine ? d0 : 0; w_room[1] -= mine ? d1 : 0; w_room[2] -= mine ? d2 : 0; w_room[3] -= mine ? d3 : 0;
    { const u32 nk = w_new ? ((((w_key >> 22) + 1u) << 22) | ((RR_SEQMAX - seq) << 3) | (w_key & 7u)) : w_key; w_key = mine ? nk : w_key; }
    w_meta = mine ? (a_child | ((((w_meta >> 8) | xg) & 0xFFu) << 8)) : w_meta;
    // Topology.Record on the hostname-keyed groups: the node's own counters (the sink where a record does not count, or in the other lanes) -- and the census of zero
    // counters (RRLds::hz; counter byte (h >> 2) * 256 + (h & 3) is slot h): a counter that leaves 0.  Behind ONE scalar flag: most pods have no such record.
    if (c & RR_PX_HREC) {
      const u32 o0 = mine ? ho0 : RR_HC_SINK, o1 = mine ? ho1 : RR_HC_SINK;
      const u32 c0n = ch0 == 0xFFu ? 1u : (ch0 >= 254u ? 254u : ch0 + 1u);
      hcb[o0] = (u8)c0n;
      const u32 ch1b = (c & RR_PX_TWICE) ? c0n : ch1;      // (two records on one counter)
      hcb[o1] = (u8)(ch1b == 0xFFu ? 1u : (ch1b >= 254u ? 254u : ch1b + 1u));
      i32* const z0 = (mine && ch0 == 0u && ho0 != RR_HC_SINK) ? &L.hz[((ho0 >> 8) * 4u + (ho0 & 3u)) & 31u] : (i32*)&L.wsinkl[0][lane];
      i32* const z1 = (mine && ch1b == 0u && ho1 != RR_HC_SINK) ? &L.hz[((ho1 >> 8) * 4u + (ho1 & 3u)) & 31u] : (i32*)&L.wsinkl[0][lane] + 1;
      atomicAdd(z0, -1); atomicAdd(z1, -1);
    }
    // ... and on the narrow key (topology.go:120-143), as prepared for the class the node now has
    // (by the winner's lane alone, behind a branch: four atomics of 64 lanes, 63 of them into a sink, keep the LDS busy for 200 cycles that the next pod's reads queue behind)
    if (mine && ((tw >> 11) & 1u)) {
      const u32 dd = (tw >> 12) & 63u, ngrp = (xg >> 16) & 63u;
      i32* const cp = &ft.gcnt[(size_t)ngrp * 64 + dd];
      atomicMax(cp, 0); atomicAdd(cp, 1); atomicOr((unsigned long long*)&ft.g_reg[ngrp], 1ull << dd); atomicOr((unsigned long long*)&ft.g_pos[ngrp], 1ull << dd); }
    // the result
    { u32* const rw = mine ? &L.wres[nres][0] : (u32*)&L.wsink[6]; rw[0] = xc.w; rw[1] = w_node; rw[2] = seq; }
    LSYNC();                              // (the winner's counters, records and result are what the other lanes read next)
    q_head = (q_head + 1 == nP) ? 0 : q_head + 1; ++q_pos; --q_len; ++seq; ++wpods; ++nres; Tc = T; no_T = false;
    if (nres == 32u) flush();
    WRP(3);
  }
  flush();
  // ---- the nodes' state back into the window's arrays (the leader hands them to their owners, or calls again) ----
  if (w_act) { L.wn_key[lane] = w_key; L.wn_meta[lane] = w_meta;
#pragma unroll
    for (int r = 0; r < 4; ++r) L.wn_room[r][lane] = w_room[r]; }
  if (lane == 0) { u32* const x = L.wx; x[0] = q_head; x[1] = q_pos; x[2] = q_len; x[3] = seq; x[4] += wpods; x[10] = stop; if (wpods) x[13] = 0;      // (the leader's "whatever its key" was for the FIRST pod: a call that placed pods has used it up -- the other window function, called next for the pod this one stopped at, must not read it again)
#ifdef KS_PROBES
    for (int i = 0; i < 8; ++i) L.wpr[i] += wrp[i];
#endif
  }
  LSYNC();
#ifndef KS_SIM
  __builtin_amdgcn_s_setprio(0);
#endif
}

// ---------------------------------------------------------------- the leader (wave 0): the Solve's sequential state ----------------------------------------------------------------
__device__ __attribute__((noinline)) void rr_leader(const int lane) {
  RR_CTX;
  const u32 wv = 0; (void)wv;
  u32 n_nrc = 0, err = 0;
  if (lane == 0) { L.n_nrc = 0; L.staged_cls = 0xFFFFFFFFu; }
  LSYNC();
#ifdef KS_PROBES
  u64 rrp[16]; for (int i = 0; i < 16; ++i) rrp[i] = 0; u64 rrp_t = __builtin_readcyclecounter();
#endif

  // ---------------- existing nodes: one nrc per distinct requirement record (leader), then the workers load them ----------------
  {
    for (u32 e = 0; e < nE && !err; ++e) {
      if (lane == 0) { nt.ntaints = P.en_taints[e]; nt.npresent = P.en.present[e]; nt.ncomplement = P.en.complement[e]; nt.ntmpl = -1; nt.nit = P.en.it_state[e]; }
      if ((u32)lane < nK) nt.nmask[lane] = P.en.mask[(size_t)e * nK + lane];
      const u32 id = rr_intern(lane); n_nrc = UF(L.n_nrc);
      if (id == 0xFFFFFFFFu) { err = 1; break; }
      if (lane == 0) L.en_nrc[e] = (u8)id;
    }
    if (lane == 0) L.init_err = err;
    LSYNC();
  }
  __syncthreads();
  if (UF(L.init_err)) return;
  // ---------------- rounds ----------------
  // A round places up to RR_B queued pods.
  //   leader : forms the batch (header: stream position of its first pod, count) | B1 | prepares the class records of the entries behind the batch |
  //            one barrier per pick | resolves: narrow-key Topology.Record, and whatever pod s needs (a machine, the exact filter, a relaxation)
  //   workers: B1 | apply the leader's order | EVALUATE every node they hold against every pod of the batch (per lane: accepting slots, best key) |
  //            PICK the pods one after the other: arg-min over the waves through one LDS atomic per wave, a barrier, everyone reads the winner; the
  //            lane that owns it moves the node's key to where the commit will put it at once | COMMIT headroom, counters, nrc of the winners
  // Picking in sequence keeps first-fit exact without re-evaluating: a node that took a pod of this round has moved back in the order (or, an existing
  // node, stayed) and takes LATER pods of the round only if it took them before -- headroom shrinks, hostname counters grow, requirements narrow --
  // so it stays a candidate with its new key, marked `ambiguous`; if such a candidate wins a pick, or a record a pod narrowed begins to accept a later
  // class (`flip`), the round stops there and the pod is issued again against exact state.  The narrow-key counters a pod's evaluation reads are not
  // recorded into by the pods before it in the round (tmask / rmask, checked when the batch is formed).
  u32 n_dyn_f = 0, n_run_pods = 0, n_run_steps = 0, n_runs = 0; u32 q_head = 0, q_pos = 0, q_len = nP, q_gen = 0, nnew = 0, seq = 0, round = 0, relaxations = 0, pops = 0, rounds_eval = 0, n_create = 0, n_vfy = 0, n_bubble = 0, n_phase_a = 0, n_again = 0;
  u64 g_active_mask = 0;
  g_active_mask = ballot64((u32)lane < nG && ft.g_active[lane] != 0);
  bool finished = false;
  u32 a_excl[8], a_nexcl = 0; bool re_a = false;
#pragma unroll
  for (int i = 0; i < 8; ++i) a_excl[i] = 0xFFFFu;
  // leader: the next 64 queue entries (lane i: entry pq_base + i), loaded ahead; a Push invalidates them
  u64 pq_e = 0; u32 pq_mi = 0, pq_off = 0, pq_base = 0; bool pq_ok = false;      // pq_mi: the class whose cached answers each entry's class shares (rr_mi)

  // ================= rounds =================
  // the queue entry at index idx (wave-uniform), through the 64-entry block held in registers
  auto q_entry = [&](const u32 idx) -> u64 {
    u32 off = idx >= pq_base ? idx - pq_base : idx + nP - pq_base;
    if (!pq_ok || off >= 64u) { u32 i2 = idx + (u32)lane; if (i2 >= nP) i2 -= nP; if (i2 >= nP) i2 = 0; pq_e = tb.q[i2]; pq_mi = rr_mi[(u32)(pq_e >> 32) & 0x7FFFFFFFu]; pq_base = idx; pq_ok = true; off = 0; }
    pq_off = off;
    return RL64(pq_e, (int)off);
  };
  // The class record of the queue entry at stream position pos (q_pos counts pops; a Push gets a position nothing was prepared for): brief, cached
  // answers, and what the entry itself adds -- the pod, whether it is a requeued unrelaxed one, which hostname records will count.
  auto ring_load = [&](const u32 cls, u32& b, u32& m) { const u32 mi = RL(pq_mi, (int)pq_off); b = (u32)lane < 48 ? rrb[(size_t)cls * 48 + lane] : ((u32)lane == 53 ? mi : (((u32)lane >= 54 && (u32)lane < 62 && P.rr_hot) ? GC(u32, P.rr_hot)[(size_t)cls * 8 + lane - 54] : 0u));      /* (word 53: the class whose cached answers it shares -- rr_window reads them again through it) */ m = (u32)lane < 24 ? rrm[(size_t)mi * 24 + lane] : 0u; };
  auto ring_store = [&](const u32 pos, const u64 e, u32 b, const u32 m) {
    RREntry& R = L.ring[pos & (RR_RING - 1u)];
    // hostname-keyed records that will count (the group exists, or the pod owns the inverse group)
    const u32 nh = RL(b, 17); const bool on = (u32)lane >= 28u && (u32)lane < 28u + nh && (((b >> 16) & 1u) || ((g_active_mask >> ((b >> 8) & 63u)) & 1ull));      // (lane 28 + i holds record word i)
    const u32 hm = (u32)(ballot64(on) >> 28);
    if ((u32)lane == 48) b = pos; else if ((u32)lane == 49) b = (u32)(e >> 32) & 0x7FFFFFFFu; else if ((u32)lane == 50) b = (u32)e; else if ((u32)lane == 51) b = hm; else if ((u32)lane == 52) b = (u32)(e >> 63);
    R.w[lane] = b; if ((u32)lane < 32) { R.m[lane] = m; R.t1[lane] = m; }
  };
  // Topology.Record on the narrow keys (topology.go:120-143) for a pod placed on a node whose requirements are nrc `child`
  auto narrow_record = [&](const u32 a_bw, const u32 child) {
    const u32 nnrec = RL(a_bw, 18);
    if (!nnrec) return;
    const u32 w = __shfl(a_bw, (40 + lane) & 63);      // lane i: record i
    if ((u32)lane < nnrec) {
      const u32 g = w & 0xFFu, key = (w >> 8) & 0xFFu, ty = (w >> 16) & 0xFFu, oi = (w >> 24) & 1u, flt = (w >> 25) & 1u;
      bool go = oi || ((g_active_mask >> g) & 1ull);
      if (go && !oi && flt) {      // TopologyGroup.Counts: the node filter against the node's requirements (topologynodefilter.go:57-70)
        const u32 b = G_grp_filter_off[g], e = G_grp_filter_off[g + 1]; bool anyf = b == e;
        for (u32 f = b; f < e && !anyf; ++f) {
          bool okf = true; const u32 fp = P.flt.present[f], fc = P.flt.complement[f];
          for (u32 bits = fp; bits && okf; bits &= bits - 1) {
            const int k = __builtin_ctz(bits);
            KReq a; a.present = (nt.present[child] >> k) & 1u; a.complement = (nt.complement[child] >> k) & 1u; a.mask = nt.mask[k][child]; a.gt = KS_NOGT; a.lt = KS_NOLT;
            const KReq in = load_req(fp, fc, P.flt.mask + (size_t)f * nK, P.flt.gt + (size_t)f * nK, P.flt.lt + (size_t)f * nK, k);
            if (kreq_compatible_fail(a, in, (tb.wellknown >> k) & 1u, tb.value_int + k * 64, tb.key_nvalues[k])) okf = false;
          }
          if (okf && P.flt.it_state[f] != 0) okf = false;      // (a filter on the instance-type key: not in the LEAN feature set; never matches here -- such problems are not LEAN)
          if (okf) anyf = true;
        }
        go = anyf;
      }
      if (go && ((nt.present[child] >> key) & 1u)) {
        const u64 qm = nt.mask[key][child]; const bool qc = (nt.complement[child] >> key) & 1u;
        if (oi || ty == 2) { for (u64 bb = qm; bb; bb &= bb - 1) grp_record<false>(tb, (int)g, __builtin_ctzll(bb)); }
        else if (!qc && __builtin_popcountll(qm) == 1) grp_record<false>(tb, (int)g, __builtin_ctzll(qm));
      }
    }
    LSYNC();
  };
  // the class record of the queue entry at index idx / stream position pos, prepared now if it is not
  auto ensure_entry = [&](const u32 pos, const u32 idx) {
    LSYNC();
    const u32 tg = L.ring[pos & (RR_RING - 1u)].w[lane];
    if (RL(tg, 48) != pos) { const u64 e = q_entry(idx); u32 b, m; ring_load((u32)(e >> 32) & 0x7FFFFFFFu, b, m); LSYNC(); ring_store(pos, e, b, m); LSYNC(); }
  };
  // One recorded group of a placed pod (w: the record word of its class brief; child: the nrc its node has now): Topology.Record on a narrow key (topology.go:120-143),
  // counters updated atomically (the pods of a run are recorded side by side, one lane each)
  auto record_word = [&](const u32 w, const u32 child) {
    const u32 g = w & 0xFFu, key = (w >> 8) & 0xFFu, ty = (w >> 16) & 0xFFu, oi = (w >> 24) & 1u, flt = (w >> 25) & 1u;
    bool go = oi || ((g_active_mask >> g) & 1ull);
    if (go && !oi && flt) {      // TopologyGroup.Counts: the node filter against the node's requirements (topologynodefilter.go:57-70)
      const u32 b = G_grp_filter_off[g], e = G_grp_filter_off[g + 1]; bool anyf = b == e;
      for (u32 f = b; f < e && !anyf; ++f) {
        bool okf = true; const u32 fp = P.flt.present[f], fc = P.flt.complement[f];
        for (u32 bits = fp; bits && okf; bits &= bits - 1) {
          const int k = __builtin_ctz(bits);
          KReq a; a.present = (nt.present[child] >> k) & 1u; a.complement = (nt.complement[child] >> k) & 1u; a.mask = nt.mask[k][child]; a.gt = KS_NOGT; a.lt = KS_NOLT;
          const KReq in = load_req(fp, fc, P.flt.mask + (size_t)f * nK, P.flt.gt + (size_t)f * nK, P.flt.lt + (size_t)f * nK, k);
          if (kreq_compatible_fail(a, in, (tb.wellknown >> k) & 1u, tb.value_int + k * 64, tb.key_nvalues[k])) okf = false;
        }
        if (okf && P.flt.it_state[f] != 0) okf = false;
        if (okf) anyf = true;
      }
      go = anyf;
    }
    if (go && ((nt.present[child] >> key) & 1u)) {
      const u64 qm = nt.mask[key][child]; const bool qc = (nt.complement[child] >> key) & 1u;
      if (oi || ty == 2) { for (u64 bb = qm; bb; bb &= bb - 1) grp_record<true>(tb, (int)g, __builtin_ctzll(bb)); }
      else if (!qc && __builtin_popcountll(qm) == 1) grp_record<true>(tb, (int)g, __builtin_ctzll(qm));
    }
  };
#ifdef KS_PROBES
  u64 cyc_runr = 0, cyc_norm = 0, t_round = __builtin_readcyclecounter(); u32 pods_runr = 0, pods_norm = 0, n_normr = 0;
#endif
  u32 dynkey[2] = {0xFFu, 0xFFu};      // dyn1: the (at most two) keys whose narrowing transitions are tabulated
  u32 n_pre = 0, pre_node = 0, pre_nrc = 0, pre_seq = 0, pre_hmask = 0, pre_bw = 0;      // the order the next round starts with
  bool prefer_run = false, ring_dirty = false; u32 n_wpods = 0, n_wphases = 0, n_wquery = 0;      // head window: off while RUN rounds serve a stretch of plain replicas | statistics
  u32 cr_key = 0, cr_rm = 0, cr_hc = 0; i64 cr_room[4] = {0, 0, 0, 0};
#ifdef KS_PROBES_WQ
  u64 wq_c[6] = {0, 0, 0, 0, 0, 0};      // around the window's loop: rr_window_fast | waiting for the workers' answer | the hand-over | a machine opened + joined | rr_window_gen | the rest
#endif
  // A new machine for the pod whose class brief is a_bw (lane i: word i), from the first template that works (scheduler.go:193-213): true -- the order for the workers / the
  // window is set (n_pre = 3, pre_*, cr_*), o_child the nrc the node has with the pod on it; false -- `why` says what each template refused (or err is set: declined)
  auto try_open = [&](const u32 a_bw, const u32 a_cls, const u32 a_seq, const u32 a_hmask, const i64* rq, const u32 prm, u32& why, u32& o_child) -> bool {
bool have = false;
    if (nE + nnew >= RR_NODES) err = 4; else if (nnew >= nMAX) err = 9;
    for (u32 m_t = 0; m_t < nM && !have && !err; ++m_t) {
      const size_t mc = (size_t)m_t * nC + a_cls;
      // (everything the template x class pair and the template's daemonsets contribute, requested at once: read one after the other -- a scalar each -- these were
      // eight trips to L2 per machine)
      u32 g_ok = GC(u8, P.mc_ok)[mc], g_base = ((const GA u8*)P.rr_mcnrc)[mc], g_chc = ((const GA u8*)P.rr_mcch)[mc], g_dp = GC(u32, P.tmpl_daemon_present)[m_t];
      i64 g_dm[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) g_dm[r] = (u32)r < nR ? GC(i64, P.tmpl_daemon)[(size_t)m_t * nR + r] : 0;
      RR_KEEP(g_ok); RR_KEEP(g_base); RR_KEEP(g_chc); RR_KEEP(g_dp); RR_KEEP(g_dm[0]); RR_KEEP(g_dm[1]); RR_KEEP(g_dm[2]); RR_KEEP(g_dm[3]);
      if (!UF(g_ok)) { if (m_t < 8) why |= (u32)UF(GC(u8, P.mc_why)[mc]) << (4 * m_t); continue; }
      // hostname-keyed items on a node nobody is on yet: its counters are 0 where the group exists, unregistered otherwise (evaluated first, like eval_node)
      const u32 nhost = RL(a_bw, 16); bool hok = true;
      for (u32 j = 0; j < nhost && hok; ++j) {
        const u32 w = RL(a_bw, 20 + (int)j); const i32 msk = (i32)RL(a_bw, 23 + (int)j); const u32 ty = w & 0xFFu, self = (w >> 8) & 0xFFu, g = w >> 24;
        const bool act = (g_active_mask >> g) & 1ull;
        if (ty == 0) { if (!act || (i32)self > msk) hok = false; }
        else if (!act) { hok = false; err = 6; }      // (an anti-affinity group that does not exist yet: which error the reference raises depends on a census this kernel does not keep -- declined)
      }
      if (err) break;
      if (!hok) { if (m_t < 8) why |= (u32)KS_WHY_TOPOLOGY << (4 * m_t); continue; }
      u32 base = UF(g_base);
      if (base == 0xFFu) {
        if (lane == 0) { nt.ntaints = GC(u64, P.tmpl_taints)[m_t]; nt.npresent = GC(u32, P.mc_present)[mc]; nt.ncomplement = GC(u32, P.mc_complement)[mc]; nt.ntmpl = (i32)m_t; nt.nit = GC(i32, P.mc_it)[mc]; }
        if ((u32)lane < nK) nt.nmask[lane] = GC(u64, P.mc_mask)[mc * nK + lane];
        base = rr_intern(lane); n_nrc = UF(L.n_nrc);
        if (base == 0xFFFFFFFFu) { err = 5; break; }
        if (lane == 0) ((GA u8*)P.rr_mcnrc)[mc] = (u8)base;
      }
      // a fresh node of this template with this class's pod on it: the nrc it ends up with, cached where the class reads no topology counter
      const bool cacheable = (RL(a_bw, 9) & 1u) == 0;
      u32 chc = cacheable ? UF(g_chc) : 0xFFu;
      int rc0 = 2; u32 ch = chc;
      if (chc == 0xFFu) {
        ++n_phase_a;
        const u32 pa = rr_phase_a(lane, a_cls, 0, 0, true, base, false); n_nrc = UF(L.n_nrc);
        if (UF(pa) >> 31) { err = 5; break; }
        const u32 pa0 = RL(pa, 0);
        rc0 = (int)(signed char)((pa0 >> 16) & 0xFFu); ch = pa0 & 0xFFu;
        if (cacheable && rc0 == 2 && lane == 0) ((GA u8*)P.rr_mcch)[mc] = (u8)ch;
      }
      if (rc0 != 2) { if (m_t < 8) why |= (u32)(rc0 < 0 ? -rc0 : KS_WHY_REQUIREMENTS) << (4 * m_t); continue; }
      const u32 rm = UF(g_dp) | prm;
      i64 tot[4]; bool fits = true;
#pragma unroll
      for (int r = 0; r < 4; ++r) { tot[r] = (u32)r < nR ? (i64)UF64((u64)g_dm[r]) + rq[r] : 0; if (((rm >> r) & 1u) && tot[r] > (i64)UF64((u64)nt.cap[r][ch])) fits = false; }
      if (fits && !UF(nt.dominant[ch])) fits = rr_exact_fit(lane, ch, tot[0], tot[1], tot[2], tot[3], rm);
      if (!fits) { if (m_t < 8) why |= (u32)KS_WHY_NO_INSTANCE_TYPE << (4 * m_t); continue; }
      have = true;
      n_pre = 3; pre_node = nE + nnew; pre_nrc = ch; pre_seq = a_seq; pre_hmask = a_hmask; pre_bw = a_bw;
      cr_key = (1u << 22) | (a_seq << 3) | ((nE + nnew) / (64u * RR_NWN)); cr_rm = rm;
#pragma unroll
      for (int r = 0; r < 4; ++r) cr_room[r] = (i64)UF64((u64)nt.cap[r][ch]) - tot[r];
      // Topology.Register(hostname), node.go:47: the hostname enters every group that exists with a count of 0 (lane w: counter word w)
      if (lane < 4 * RR_GW) L.scratch[lane] = 0xFFu;
      LSYNC();
      { const u32 hs = ls.hslot_of[lane]; if ((u32)lane < nG && hs < 4 * RR_GW && ((g_active_mask >> lane) & 1ull)) { L.scratch[hs] = 0u; atomicAdd(&L.hz[hs], 1); } }      // (... and the census of zero counters)
      LSYNC();
      cr_hc = lane < RR_GW ? (L.scratch[4 * lane] | (L.scratch[4 * lane + 1] << 8) | (L.scratch[4 * lane + 2] << 16) | (L.scratch[4 * lane + 3] << 24)) : 0u;
      LSYNC();
      if (lane == 0) G_n_tmpl[nnew] = (i32)m_t;
      o_child = ch; ++nnew; ++n_create;
    }
    return have;
  };
  // every iteration places a pod, opens a machine, or relaxes / requeues one: a Solve ends within this many (beyond: a protocol bug -- declined, ks_pack has its own watchdog)
  const u32 round_limit = 8u * nP + 4u * UF(G_pod_stage_off[nP]) + 4096u;
  for (;;) {
    // (the sequential state is wave-uniform; telling the compiler so at the head of every round keeps it in scalar registers and its branches scalar)
    q_head = UF(q_head); q_pos = UF(q_pos); q_len = UF(q_len); q_gen = UF(q_gen); nnew = UF(nnew); seq = UF(seq); round = UF(round); n_nrc = UF(n_nrc); err = UF(err);
    a_nexcl = UF(a_nexcl); n_pre = UF(n_pre); pre_node = UF(pre_node); pre_nrc = UF(pre_nrc); pre_seq = UF(pre_seq); pre_hmask = UF(pre_hmask); pq_base = UF(pq_base);
    g_active_mask = UF64(g_active_mask); dynkey[0] = UF(dynkey[0]); dynkey[1] = UF(dynkey[1]);
    finished = UF((u32)finished) != 0; re_a = UF((u32)re_a) != 0; pq_ok = UF((u32)pq_ok) != 0; prefer_run = UF((u32)prefer_run) != 0; ring_dirty = UF((u32)ring_dirty) != 0; n_wquery = UF(n_wquery); n_wpods = UF(n_wpods); n_wphases = UF(n_wphases);
    if (round > round_limit && !err) err = 8;
    const u32 par = round & 1u;
    RRCtl& C = L.ctl[par];
    // ---------- 1. form the batch ----------
    u32 nb = 0, same = 0, prev_ev = 0, prev_flags = 1, run = 0; u64 rmask_acc = 0;
    // A RUN?  The entries behind the head of its base class (ev0: same requests, same cached answers, at most one hostname-keyed item, no topology counters read): one lane
    // each, 64 entries of the queue at a time, up to RR_RUN_MAX.  The walk ends with the first 64 that hold an entry the run does not take: nothing behind it is read.
    auto try_run = [&](const u32 ev0) {
      u32 R = 0;
      for (u32 c0 = 0; c0 < RR_RUN_MAX; c0 += 64u) {
        const u32 t = c0 + (u32)lane; const bool valid = t < q_len;      // (t: the entry's place in the RUN -- what the tables are indexed by, and what the rule for requeued entries asks about)
        u32 ix = q_head + t; if (ix >= nP) ix -= nP;
        const u64 e = valid ? tb.q[ix] : 0ull;
        const u32 cls = (u32)(e >> 32) & 0x7FFFFFFFu;
        const u32 evt = valid ? rrb[(size_t)cls * 48 + 27] : ~ev0, flt = valid ? rrb[(size_t)cls * 48 + 9] : 2u;      // (word 27: the base class, ks_link_rr2)
        const bool okt = valid && (t == 0 || (e >> 63) == 0) && evt == ev0 && !(flt & 7u);      // (a requeued, unrelaxed entry only as the head of the run: queue.go:50-53 is tested there)
        const u64 bad = ~ballot64(okt);
        const u32 n = bad ? (u32)__builtin_ctzll(bad) : 64u;
        if (c0 + n < 2u) return;               // (a run of one is a round's pod)
        if ((u32)lane < n) {
          RRRunPod& rp = L.runtab[par][t];
          const u32 nh = rrb[(size_t)cls * 48 + 17]; u32 cnt = 0;
          for (u32 w = 0; w < nh && w < RR_MAXHREC; ++w) { const u32 word = rrb[(size_t)cls * 48 + 28 + w]; if (((word >> 16) & 1u) || ((g_active_mask >> ((word >> 8) & 63u)) & 1ull)) rp.hs[cnt++] = (u8)(word & 0xFFu); }
          rp.pod = (u32)e; rp.cls = cls; rp.nh = cnt;
          const u32 nho = rrb[(size_t)cls * 48 + 16];      // its hostname-keyed items (a base class has at most two), packed
          u32 it[2] = {0, 0};
          for (u32 q = 0; q < 2; ++q) if (q < nho) {
            const u32 hw = rrb[(size_t)cls * 48 + 20 + q]; const i32 lim = (hw & 0xFFu) == 0 ? (i32)rrb[(size_t)cls * 48 + 23 + q] - (i32)((hw >> 8) & 0xFFu) : 0;
            it[q] = 0x80000000u | (((u32)lim & 0x1FFu) << 16) | ((8u * ((hw >> 16) & 3u)) << 8) | ((hw >> 18) & 7u);
          }
          L.runitem[par][t] = (u64)it[0] | ((u64)it[1] << 32);
        }
        R = c0 + n;
        if (n < 64u) break;
      }
      LSYNC();
      run = R; nb = R;
    };
    u32 last_flags = 0, last_base = 0;
    auto form_one = [&](const u32 adv, bool& was_dyn) -> bool {
      nb = UF(nb); same = UF(same); prev_ev = UF(prev_ev); prev_flags = UF(prev_flags); rmask_acc = UF64(rmask_acc); n_nrc = UF(n_nrc);
      u32 idx = q_head + (nb - adv); if (idx >= nP) idx -= nP;
      const u32 pos = q_pos + (nb - adv), rs = pos & (RR_RING - 1u);
      LSYNC();
      u32 t_bw = L.ring[rs].w[lane];
      if (RL(t_bw, 48) != pos) {             // not prepared (the first rounds, after a relaxation changed the groups that exist)
        const u64 e = q_entry(idx); u32 b, m; ring_load((u32)(e >> 32) & 0x7FFFFFFFu, b, m); LSYNC(); ring_store(pos, e, b, m); LSYNC();
        t_bw = L.ring[rs].w[lane];
      }
      RRP(5);
      const u32 t_cls = RL(t_bw, 49), t_pod = RL(t_bw, 50);
      // a requeued, unrelaxed pod is tested for staleness against the exact queue state (queue.go:50-53): only at the head of a batch
      if (!re_a && RL(t_bw, 52) != 0) {
        if (nb > 0) return false;
        if (UF(G_lastgen[t_pod]) == q_gen && UF(G_lastlen[t_pod]) == q_len) { finished = true; return false; }
      }
      const u32 flags = RL(t_bw, 9);
      if (flags & 2u) { err = 7; return false; }
      const u64 tm = (u64)RL(t_bw, 12) | ((u64)RL(t_bw, 13) << 32), rmk = (u64)RL(t_bw, 14) | ((u64)RL(t_bw, 15) << 32);
      if ((flags & 1u) && (tm & rmask_acc)) { ++n_bubble; return false; }      // its evaluation reads counters an earlier pod of the batch records into
      // ---- what every nrc answers: cached per class (t1) but for the nrcs it has not met; classes that read topology counters are answered per pod --
      // in full (phase_a), or, where the only such item is one spread (dyn1), from the cached rest and the group's counts ----
      u32 dks = 2;      // dyn1: which of the two key slots
      if ((flags & 5u) == 5u) {
        const u32 dk = (RL(t_bw, 11) >> 16) & 0xFFu;
        if (dynkey[0] == dk) dks = 0; else if (dynkey[1] == dk) dks = 1; else if (dynkey[0] == 0xFFu) { dynkey[0] = dk; dks = 0; } else if (dynkey[1] == 0xFFu) { dynkey[1] = dk; dks = 1; }
        const u32 dk_have = UF(L.dynk[dks & 1u]);
        LSYNC();
        if (dks < 2 && dk_have != dk) {      // a dyn key met for the first time: the head window's per-nrc column for it
          if ((u32)lane < n_nrc) L.dy_nd[dks][lane] = rr_dy_nd(nt, ft, (u32)lane, dk, tb.wellknown);
          if (lane == 0) L.dynk[dks] = dk;
          LSYNC();
        }
      }
      const bool is_dyn = dks < 2, is_gen = (flags & 1u) && !is_dyn;
      RRP(6);
      u32 mn = UF(L.ring[rs].t1[6]);
      if (is_gen || mn < n_nrc) {
        u32 mw;
        if (is_gen) { mw = 0; mn = 0; }
        else { mw = (u32)lane < 24 ? rrm[(size_t)UF(rr_mi[t_cls]) * 24 + lane] : 0u; mn = RL(mw, 6); }      // (the ring's copy may be older than the class's cached answers)
        while (mn < n_nrc && !err) {
          const u32 hi = n_nrc;
          ++n_phase_a;
          const u32 pa = rr_phase_a(lane, t_cls, mn, hi, false, 0, is_dyn); n_nrc = UF(L.n_nrc);
          if (UF(pa) >> 31) { err = 5; break; }
          const bool acc_l = (pa >> 8) & 1u; const u32 child_l = pa & 0xFFu;
          const u64 acc = ballot64(acc_l), chg = ballot64(acc_l && child_l != (u32)lane);
          bool v = false;
          if (acc_l && nt.tmpl[lane] >= 0) { if (!nt.dominant[child_l]) v = true; for (u32 r = 0; r < nR; ++r) if (nt.cap[r][child_l] != nt.cap[r][lane]) v = true; }
          const u64 vfy = ballot64(v);
          if (lane < 24) L.scratch[lane] = mw;
          LSYNC();
          if ((u32)lane >= mn && (u32)lane < hi) ((u8*)&L.scratch[8])[lane] = (u8)child_l;
          if (lane == 0) { L.scratch[0] |= (u32)acc; L.scratch[1] |= (u32)(acc >> 32); L.scratch[2] |= (u32)chg; L.scratch[3] |= (u32)(chg >> 32); L.scratch[4] |= (u32)vfy; L.scratch[5] |= (u32)(vfy >> 32); L.scratch[6] = hi; }
          LSYNC();
          mw = lane < 24 ? L.scratch[lane] : 0u;
          LSYNC();
          mn = hi;
          if (!is_gen && lane < 24) rrm[(size_t)UF(rr_mi[t_cls]) * 24 + lane] = mw;
        }
        if (err) return false;
        if ((u32)lane < 24) { L.ring[rs].m[lane] = mw; if (!is_gen) L.ring[rs].t1[lane] = mw; }
        LSYNC();
      }
      RRP(7);
      if (is_dyn) {
        ++n_dyn_f;
        const u32 dw = RL(t_bw, 11); const u32 dg = (dw >> 8) & 0xFFu, dk = (dw >> 16) & 0xFFu, dself = dw >> 24; const i32 dskew = (i32)RL(t_bw, 19);
        const u64 dPD = (u64)RL(t_bw, 26) | ((u64)RL(t_bw, 27) << 32);
        const u64 reg = UF64(ft.g_reg[dg]), gpos = UF64(ft.g_pos[dg]);
        const u32 t1w = L.ring[rs].t1[lane & 31];
        const u64 acc1 = (u64)RL(t1w, 0) | ((u64)RL(t1w, 1) << 32), chg1 = (u64)RL(t1w, 2) | ((u64)RL(t1w, 3) << 32);
        if (!(reg == 0 && gpos == ~0ull)) {       // (a group that does not exist yet constrains nothing: the cached answers stand)
          const bool on = (u32)lane < n_nrc && ((acc1 >> lane) & 1ull);
          const u32 n1 = ((chg1 >> lane) & 1ull) ? (u32)((const u8*)&L.ring[rs].t1[8])[lane] : (u32)lane;      // the record after the pod's own requirements
          // nextDomainTopologySpread (topologygroup.go:155-182) for every record at once: lane d holds domain d's count
          const i32 cv = ft.gcnt[(size_t)dg * 64 + lane];
          const bool inmin = ((reg & dPD) >> lane) & 1ull;
          const u32 mnc = wave_min_u32(inmin ? (u32)cv : 0x7FFFFFFFu);      // domainMinCount over the pod's domains (:184-200)
          const u64 EL = ballot64(((reg >> lane) & 1ull) && (i64)cv + (i64)dself - (i64)(i32)mnc <= (i64)dskew);
          const u32 n1s = on ? n1 : 0u;
          const bool pres = (nt.present[n1s] >> dk) & 1u;
          KReq nd = kreq_exists();
          if (pres) { nd.present = true; nd.complement = (nt.complement[n1s] >> dk) & 1u; nd.mask = nt.mask[dk][n1s]; nd.gt = KS_NOGT; nd.lt = KS_NOLT; }
          const u64 ND = kreq_has_mask(nd, tb.value_int + dk * 64, tb.key_nvalues[dk]);
          const u64 mm = EL & ND;
          const bool ok = on && mm != 0 && (pres || ((tb.wellknown >> dk) & 1u));
          i32 bestc = INT32_MAX; u32 dom = 0;
          for (u64 bits = EL; bits; bits &= bits - 1) {      // the least count, the first such domain (EL is wave-uniform: the counts come by readlane)
            const int d = __builtin_ctzll(bits);
            const i32 c = (i32)RL((u32)cv, d) + (i32)dself;
            if (((mm >> d) & 1ull) && c < bestc) { bestc = c; dom = (u32)d; }
          }
          u32 child2 = ok ? (u32)L.t2[dks][n1s][dom] : (u32)lane;
          // narrowed records met for the first time: interned one lane at a time
          for (u64 todo = ballot64(ok && child2 == 0xFFu); todo; todo &= todo - 1) {
            const int l = __builtin_ctzll(todo);
            u32 id;
            const u32 n1u = RL(n1s, l), domu = RL(dom, l);
            const bool same = ((UF(nt.present[n1u]) >> dk) & 1u) && !((UF(nt.complement[n1u]) >> dk) & 1u) && UF64(nt.mask[dk][n1u]) == (1ull << domu);
            if (same) id = n1u;
            else {
              LSYNC();
              if (lane == 0) { nt.npresent = nt.present[n1u] | (1u << dk); nt.ncomplement = nt.complement[n1u] & ~(1u << dk); nt.ntaints = nt.taints[n1u]; nt.ntmpl = nt.tmpl[n1u]; nt.nit = nt.it[n1u]; }
              if ((u32)lane < nK) nt.nmask[lane] = (u32)lane == dk ? (1ull << domu) : nt.mask[lane][n1u];
              id = rr_intern(lane); n_nrc = UF(L.n_nrc);
              if (id == 0xFFFFFFFFu) { err = 5; break; }
            }
            if (lane == 0) L.t2[dks][n1u][domu] = (u8)id;
            if (lane == l) child2 = id;
            LSYNC();
          }
          if (err) return false;
          const u64 acc = ballot64(ok), chg = ballot64(ok && child2 != (u32)lane);
          bool v = false;
          if (ok && nt.tmpl[lane] >= 0) { if (!nt.dominant[child2]) v = true; for (u32 r = 0; r < nR; ++r) if (nt.cap[r][child2] != nt.cap[r][lane]) v = true; }
          const u64 vfy = ballot64(v);
          LSYNC();
          ((u8*)&L.ring[rs].m[8])[lane] = (u8)child2;
          if (lane == 0) { u32* mo = L.ring[rs].m; mo[0] = (u32)acc; mo[1] = (u32)(acc >> 32); mo[2] = (u32)chg; mo[3] = (u32)(chg >> 32); mo[4] = (u32)vfy; mo[5] = (u32)(vfy >> 32); mo[6] = n_nrc; }
          LSYNC();
        } else { if ((u32)lane < 24) L.ring[rs].m[lane] = t1w; LSYNC(); }
      }
      RRP(13);
      { const u32 ev = RL(t_bw, 10); if (nb > 0 && !(flags & 1u) && !(prev_flags & 1u) && ev == prev_ev) same |= 1u << nb; prev_ev = ev; prev_flags = flags; }
      rmask_acc |= rmk;
      ++nb;
      last_flags = flags; last_base = RL(t_bw, 27); was_dyn = is_dyn;
      return true;
    };
    // ---------- 0. the HEAD WINDOW (round 5; rr_window above) ----------
    // The workers lend the leader the nodes at the front of the visiting order; while the window stands the leader places pod after pod by itself (rr_window).  The pod it
    // stops at stays at the head of the queue for a round over all nodes, at whose B1 the owners take their nodes back.
    const bool do_win = !finished && !err && !re_a && n_pre != 2u && q_len > 0 && !prefer_run;
    if (lane == 0) { L.wn_mode = do_win ? 1u : 0u; L.wn_done = 0; L.wn_qn = 0; L.wn_fn = 0; L.wn_qdone = 0; L.wn_fdone = 0; L.wn_qpos = q_pos; L.wq_base = q_pos; L.wq_head = q_head; L.wq_len = q_len; L.wq_gam = g_active_mask; }
    LSYNC();
    __syncthreads();                       // B0
    if (ring_dirty) { if (lane < RR_RING) L.ring[lane].w[48] = 0xFFFFFFFFu; if (lane < (int)RR_PX) L.px[lane].u[0] = 0xFFFFFFFFu; LSYNC(); ring_dirty = false; }
    u32 ret_word = 0;
    if (do_win) {
      RRP(8);
      u32 T = 0xFFFFFFFFu;
#pragma unroll
      for (int w = 0; w < RR_NWK; ++w) T = min(T, UF(L.wn_cut[w]));
      const u64 act = ballot64((u32)lane < RR_WLENT && L.wn_key[lane] < T);      // (what was published at or above T stays with its owner)
      u32 nextra = 0;      // window places RR_WLENT.. in use: the machines opened for this phase, the nodes taken over from the workers during it
      // a machine the leader has just opened (the order n_pre = 3 it would give the workers): a window node from its first pod on, its owner learns of it when the window is handed back
      auto join_fresh = [&]() {
        const u32 pl = RR_WLENT + nextra;
        if (lane == 0) { L.wn_key[pl] = cr_key; L.wn_own[pl] = pre_node; L.wn_meta[pl] = pre_nrc | (cr_rm << 8); for (int r = 0; r < 4; ++r) L.wn_room[r][pl] = cr_room[r]; }
        if (lane < RR_GW) L.wn_hc[lane][pl] = cr_hc;
        if (lane < 48) L.scratch[lane] = pre_bw;      // (its first pod's class brief: the hostname records)
        LSYNC();
        if (lane == 0) {
          u8* const hcb = (u8*)L.wn_hc; const u32 nh = L.scratch[17];
          for (u32 t = 0; t < nh; ++t) if ((pre_hmask >> t) & 1u) { const u32 hs = L.scratch[28 + t] & 0xFFu; u8& c = hcb[(((hs >> 2) * 64u + pl) << 2) + (hs & 3u)]; if (c == 0u) atomicAdd(&L.hz[hs & 31u], -1); c = c == 0xFFu ? 1u : (c >= 254u ? 254u : c + 1u); }
          L.wx_act |= 1ull << pl;
        }
        LSYNC();
        ++nextra; n_pre = 0;
      };
      if (lane == 0) {
        u32* const x = L.wx; x[0] = q_head; x[1] = q_pos; x[2] = q_len; x[3] = seq; x[4] = 0; x[5] = n_nrc; x[6] = T; x[7] = 0; x[8] = dynkey[0]; x[9] = dynkey[1]; x[10] = 0; x[11] = n_wphases; x[13] = 0;
        L.wx_gam = g_active_mask; L.wx_act = act;
      }
      LSYNC();
      if (n_pre == 3u) join_fresh();
      RRP(9);
      u32 qn = 0, fn = 0; bool no_T = false;
#ifdef KS_PROBES_WQ
      u64 wq_t = __builtin_readcyclecounter();
#define WQP(i) do { const u64 t_ = __builtin_readcyclecounter(); wq_c[(i)] += t_ - wq_t; wq_t = t_; } while (0)
#else
#define WQP(i) do { } while (0)
#endif
      for (;;) {      // the straight-line loop; behind a pod it does not cover, the general one for that pod; a pod nothing in the window takes: ask the workers; and again
        if (lane == 0) { L.wx[13] = no_T ? 1u : 0u; L.wx[5] = n_nrc; }
        LSYNC();
        WQP(5);
        rr_window_fast(lane);
        LSYNC();
        WQP(0);
        u32 why = UF(L.wx[10]);
        no_T = false;
        if (why == 9u) { prefer_run = true; RR_BRK(0); break; }      // a stretch of plain replicas ahead: RUN rounds place those several per barrier
        if (why == 7u) {
          if (lane == 0) L.wx[12] = 1u;
          LSYNC();
          rr_window_gen(lane);
          LSYNC();
          WQP(4);
          why = UF(L.wx[10]);
          if (why == 8u) continue;
        }
        if ((why != 5u && why != 11u) || nextra >= RR_WSPARE) { RR_BRK((why != 5u && why != 11u) ? 1 : 2); break; }
        // ---- nothing in the window (below T: 5; at all, after the workers were asked: 11) takes the pod at the head of the queue ----
        const u32 xw = L.wx[lane & 15]; const u32 c_qh = RL(xw, 0), c_qp = RL(xw, 1), c_ql = RL(xw, 2), c_seq = RL(xw, 3);
        const u32 a_bw = L.ring[c_qp & (RR_RING - 1u)].w[lane];
        // (a class that reads topology counters in general is answered per pod and per nrc by the leader's formation: a round's.  Asking the workers about dyn1 pods with
        // answers worked out on the spot was measured twice, rounds 5 and 6: 3 972 questions instead of 1 320, 761 phases instead of 2 004, and 2 ms SLOWER -- a
        // question + hand-over + re-entry costs what the round + lend it replaces cost)
        if (RL(a_bw, 9) & 1u) { RR_BRK(3); break; }
        if (why == 5u && (RL(a_bw, 54) & 1u)) {
          // A pod one of whose hostname items needs its node's counter at 0 (anti-affinity; a spread whose skew leaves no room) when NO node's counter stands at 0 (the
          // census RRLds::hz) is taken by nobody, lent or not: the workers are not asked, the machine is opened at once (scheduler.go:193-213)
          bool none = false;
          for (int j = 0; j < 2; ++j) { const u32 it = RL(a_bw, 55 + j), off = it & 0xFFFFu; const i32 lim = (i32)(int16_t)(it >> 16);
            if (off < RR_HC_ZERO && (lim < 0 || (lim == 0 && UF((u32)L.hz[((off >> 8) * 4u + (off & 3u)) & 31u]) == 0u))) none = true; }
          if (none) { why = 11u; if (lane == 0) L.wstop[3] += 1; }
        }
        if (why == 5u) {
          // Which of the nodes the WORKERS hold is the first to accept it?  They answer from their polling loop (evaluate, wave minimum, one atomic each); the node joins
          // the window, and the pod is looked at once more against everything the window holds, whatever its key: the least accepting key of all nodes wins.
          ++qn; ++n_wquery;
          if (lane == 0) { L.wq_win = ~0ull; L.wn_qdone = 0; L.wn_qp = c_qp; }
          LSYNC();
          if (lane == 0) __hip_atomic_store(&L.wn_qn, qn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
          { u32 spin = 0; while (RL(RR_LDS_LOAD(&L.wn_qdone), 0) != RR_NWK) { RR_POLL_PAUSE(); if (++spin > RR_SPIN_MAX) { err = 8; break; } } }      // (bounded, like every wait of the leader: a lost answer declines the Solve to ks_pack instead of hanging the stream)
          if (err) break;
          LSYNC();
          WQP(1);
          const u64 w = UF64(L.wq_win);
          if (w != ~0ull) {
            ++fn;
            const u32 pl = RR_WLENT + nextra;
            if (lane == 0) { L.wn_fnode = (u32)w & 0xFFFFu; L.wn_fplace = pl; }
            LSYNC();
            if (lane == 0) __hip_atomic_store(&L.wn_fn, fn, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
            { u32 spin = 0; while (RL(RR_LDS_LOAD(&L.wn_fdone), 0) != fn) { RR_POLL_PAUSE(); if (++spin > RR_SPIN_MAX) { err = 8; break; } } }
            if (err) break;
            LSYNC();
            if (lane == 0) L.wx_act |= 1ull << pl;
            LSYNC();
            ++nextra;
          }
          WQP(2);
          no_T = true;
          continue;
        }
        // ---- no node anywhere: a machine (scheduler.go:193-213), opened here instead of in a round's resolve; it joins the window with its first pod on it ----
        {
          const u32 a_pod = RL(a_bw, 50), a_cls = RL(a_bw, 49), a_hmask = RL(a_bw, 51), prm = RL(a_bw, 8);
          i64 rq[4];
#pragma unroll
          for (int r = 0; r < 4; ++r) rq[r] = (i64)((u64)RL(a_bw, 2 * r) | ((u64)RL(a_bw, 2 * r + 1) << 32));
          u32 why_t = 0, child = 0;
          const bool have = try_open(a_bw, a_cls, c_seq, a_hmask, rq, prm, why_t, child);
          if (!have || err) { RR_BRK(4); break; }                       // (no template works: relaxation and requeue are the round's)
          if (lane == 0) {
            tb.pod_node[a_pod] = (i32)(nE + nnew - 1u); tb.pod_seq[a_pod] = (i32)c_seq; G_pod_reason[a_pod] = 0;
            u32* const x = L.wx; x[0] = (c_qh + 1 == nP) ? 0 : c_qh + 1; x[1] = c_qp + 1; x[2] = c_ql - 1; x[3] = c_seq + 1; x[4] += 1;
          }
          narrow_record(a_bw, child);
          join_fresh();
          LSYNC();
          WQP(3);
        }
      }
      if (lane == 0) RR_LDS_STORE(&L.wn_done, 1u);      // (the workers stop preparing records and come to B1)
      { const u32 xw = L.wx[lane & 15]; q_head = RL(xw, 0); q_pos = RL(xw, 1); q_len = RL(xw, 2); seq = RL(xw, 3); const u32 wp = RL(xw, 4); pops += wp; n_wpods += wp; ++n_wphases; const u32 why = RL(xw, 10) & 7u; if (lane == 0) L.wstop[why] += 1;
      }
      ret_word = 1u | (nextra << 8);
      RRP(10);
    }
    const bool runs_on = prefer_run;      // (with the head window on, a round only takes the pod the window could not place; RUN rounds while prefer_run)
    const u32 want = (re_a || !runs_on) ? 1u : RR_B;
    if (!finished && !err && !re_a) {
      // The head of the queue at a glance, one lane per entry: the leading entries that need nothing from the leader -- prepared, not requeued, no topology counters
      // read, cached answers complete -- join the batch at once (what they record still counts against the readers behind them)
      const u32 t = (u32)lane; const bool in = t < want && t < q_len;
      const RREntry& Et = L.ring[(q_pos + t) & (RR_RING - 1u)];
      LSYNC();
      const u32 tag = Et.w[48], rqd = Et.w[52], fl = Et.w[9], ev = Et.w[10], bs = Et.w[27], mnt = Et.t1[6]; const u64 rmk_t = (u64)Et.w[14] | ((u64)Et.w[15] << 32);
      const bool triv = in && tag == q_pos + t && rqd == 0 && (fl & 7u) == 0 && mnt == n_nrc;
      const u64 nt_ = ~ballot64(triv);
      const u32 ntriv = nt_ ? (u32)__builtin_ctzll(nt_) : 64u;
      if (ntriv > 0 && want == 1u) { nb = 1; prev_ev = RL(ev, 0); prev_flags = 0; rmask_acc = RL64(rmk_t, 0); }      // (the one pod the window left: nothing to compare it with)
      else if (ntriv > 0) {
        const u32 evp = __shfl(ev, (lane + 63) & 63);
        same = (u32)ballot64(t > 0 && t < ntriv && ev == evp);
        const u32 lo = wave_or_u32(t < ntriv ? (u32)rmk_t : 0u), hi = wave_or_u32(t < ntriv ? (u32)(rmk_t >> 32) : 0u);
        rmask_acc = (u64)lo | ((u64)hi << 32);
        nb = ntriv; prev_ev = RL(ev, (int)(ntriv - 1u)); prev_flags = 0;
        if (runs_on) try_run(RL(bs, 0));
      }
    }
    // One more pod joins the batch: the entry `nb - adv` places behind the head of the queue (adv: the pods of the batch that have left the queue already -- none while
    // the batch is formed before the round starts, all of them once it runs).  false: the batch ends before this pod.
    bool stream = false;      // the rest of the batch joins while the workers pick (one pod per pick, formed in the shadow of the pick before it)
    while (!run && !finished && !err && nb < want && nb < q_len) {
      bool dyn = false;
      if (!form_one(0u, dyn)) break;
      if (nb == 1 && !(last_flags & 7u) && !re_a && runs_on) { try_run(last_base); if (run) break; }      // (a head the glance above could not take -- not prepared yet, cached answers extended just now -- may still start a run)
      if (dyn && !re_a) { stream = true; break; }      // (a pod whose answers the leader computes from the counters: the workers start on it while the next one's are computed)
    }
    if (err) { if (lane == 0) { C.hdr[RRH_EXIT] = 1; C.hdr[RRH_RET] = 0; } LSYNC(); __syncthreads(); break; }
    const bool hint = !runs_on && !re_a && nb == 1u && !run;      // (a window phase will follow this one-pod round: the workers prepare class records for it)
    const bool exit_now = nb == 0 && n_pre == 0;      // (nothing left, or the head of the queue has seen this queue before: scheduler.go:110-114)
    if (lane == 0) {
      C.hdr[RRH_PRE] = n_pre; C.hdr[RRH_PNODE] = pre_node; C.hdr[RRH_PNRC] = pre_nrc; C.hdr[RRH_NB] = nb; C.hdr[RRH_SEQ] = seq; C.hdr[RRH_POS] = q_pos; C.hdr[RRH_SAME] = same; C.hdr[RRH_RUN] = run;
      C.hdr[RRH_NSLOTS] = (nE + nnew + 64u * RR_NWN - 1u) / (64u * RR_NWN); C.hdr[RRH_PSEQ] = pre_seq; C.hdr[RRH_PHMASK] = pre_hmask; C.hdr[RRH_RET] = ret_word;
      C.hdr[RRH_HINT] = hint ? 1u : 0u; C.hdr[RRH_QH] = q_head; C.hdr[RRH_QL] = q_len; C.hdr[RRH_GAM] = (u32)g_active_mask; C.hdr[RRH_GAM + 1] = (u32)(g_active_mask >> 32);
      C.hdr[RRH_NEXCL] = re_a ? a_nexcl : 0u; C.hdr[RRH_EXIT] = exit_now ? 1u : 0u; C.hdr[RRH_NB2] = nb | (same << 8); C.hdr[RRH_NB2 + 1] = nb | (same << 8);
      for (int i = 0; i < 4; ++i) C.hdr[RRH_EXCL + i] = (a_excl[2 * i] & 0xFFFFu) | ((a_excl[2 * i + 1] & 0xFFFFu) << 16);
      if (n_pre == 3) { C.create[0] = cr_key; C.create[1] = cr_rm; for (int r = 0; r < 4; ++r) { C.create[2 + 2 * r] = (u32)(u64)cr_room[r]; C.create[3 + 2 * r] = (u32)((u64)cr_room[r] >> 32); } }
    }
    if (n_pre == 3 && lane < RR_GW) C.create[10 + lane] = cr_hc;
    if (n_pre >= 2 && (u32)lane < 48) C.pbrief[lane] = pre_bw;
    if (lane < RR_B) L.win[par][lane] = ~0ull;
    // the batch leaves the queue (what is not placed goes back when the round is resolved)
    const u32 pos0 = q_pos;
    { q_head += nb; if (q_head >= nP) q_head -= nP; q_pos += nb; q_len -= nb; pops += nb; if (nb) ++rounds_eval; }
    RRP(0);
    __syncthreads();                       // B1
    if (exit_now) break;
    RRP(1);
    // ---------- 2. the class records of the entries behind the batch: prepared one per pick, in the time the leader spends waiting for the workers anyway ----------
    u32 pp_pos = q_pos, pend_pos = 0, pend_b = 0, pend_m = 0; u64 pend_e = 0; bool pend = false;      // pp_pos: the next stream position to look at (the head moves on while pods join a running round)
    auto prep_step = [&]() {
      if (pend) { LSYNC(); ring_store(pend_pos, pend_e, pend_b, pend_m); LSYNC(); pend = false; }      // (requested one call ago: it has arrived)
      if ((i32)(pp_pos - q_pos) < 0) pp_pos = q_pos;
      while (pp_pos - q_pos < RR_B) {
        const u32 t = pp_pos - q_pos; ++pp_pos;
        if (t >= q_len) { pp_pos = q_pos + RR_B; break; }
        const u32 pos = q_pos + t;
        if (pos - pos0 >= RR_RING) continue;                                           // (a long run: not into the ring slots the round's own entries sit in)
        if (UF(L.ring[pos & (RR_RING - 1u)].w[48]) == pos) continue;
        u32 idx = q_head + t; if (idx >= nP) idx -= nP;
        pend_e = q_entry(idx); ring_load((u32)(pend_e >> 32) & 0x7FFFFFFFu, pend_b, pend_m); pend_pos = pos; pend = true;
        break;
      }
    };
    RRP(2);
    // ---------- 3. the picks, as the workers see them ----------
    u32 s = nb, kind = 0;
    u32 wn = 0xFFFFFFFFu, wnrc_s = 0, child = 0;
    nb = UF(nb); run = UF(run);
    if (run) {
      // a RUN: the steps as the workers see them (one barrier each); where the pods went is kept for the records
      const u32 mw = L.ring[pos0 & (RR_RING - 1u)].m[lane & 31];
      const u64 rchg = (u64)RL(mw, 2) | ((u64)RL(mw, 3) << 32), rvfy = (u64)RL(mw, 4) | ((u64)RL(mw, 5) << 32);
      u32 done = 0, stepno = 0;
      while (done < run) {
        prep_step();
        __syncthreads();
        u32 wkey, wpay, snode, snrc, g_i0, g_i1;
        const u32 glen = rr_run_group(L.runitem[par], lane, done, run - done, g_i0, g_i1);
        const u32 n_step = rr_step_merge_leader(stepno & 1u, lane, min(run - done, glen), nE, rvfy);
        wpay = L.mrg_out[lane]; kind = UF(L.mrg_k[0]); snode = UF(L.mrg_k[1]); snrc = UF(L.mrg_k[2]);
        if ((u32)lane < n_step) { const u32 nrc = (wpay >> 16) & 0xFFu; const u32 ch = ((rchg >> nrc) & 1ull) ? (u32)((const u8*)&L.ring[pos0 & (RR_RING - 1u)].m[8])[nrc] : nrc; L.runres[done + lane] = (ch << 16) | (wpay & 0xFFFFu); }
        done += n_step; ++stepno;
        if (kind != 0) { wn = snode; wnrc_s = snrc; child = ((rchg >> snrc) & 1ull) ? ((RL(mw, 8 + (int)(snrc >> 2)) >> (8u * (snrc & 3u))) & 0xFFu) : snrc; break; }
      }
      s = done; n_run_pods += done; n_run_steps += stepno; ++n_runs;
      if (stepno * RR_RUN_KEEP > done) prefer_run = false;      // (steps of a pod or two: replicas whose hostname items differ -- the head window does those better)
      LSYNC();
      RRP(14);
      // Topology.Record on the narrow keys for the run's pods
      {
      for (u32 base = 0; base < s; base += 64) {
        const u32 t = base + (u32)lane;
        if (t < s) {
          const u32 cls = L.runtab[par][t].cls, ch = L.runres[t] >> 16;
          const GA u32* const cb = rrb + (size_t)cls * 48;      // (the count and every record word requested at once: one trip to L2 for the 64 pods, not one per record)
          const u32 nn = cb[18]; u32 rw[RR_MAXNREC];
#pragma unroll
          for (int r = 0; r < RR_MAXNREC; ++r) rw[r] = cb[40 + r];
#pragma unroll
          for (int r = 0; r < RR_MAXNREC; ++r) if ((u32)r < nn) record_word(rw[r], ch);
        }
      }
      }
      LSYNC();
      RRP(15);
      if (s < nb) { u32 ix = q_head >= (nb - s) ? q_head - (nb - s) : q_head + nP - (nb - s); ensure_entry(pos0 + s, ix); }      // (the pod the run stopped at: its class record, for what the leader does with it below)
    } else
    for (u32 j = 0; j < nb; ++j) {
      j = UF(j);
      const u32 mw = L.ring[(pos0 + j) & (RR_RING - 1u)].m[lane & 31];
      if (stream) {
        // the next pod joins the batch while the workers evaluate this one; they learn of it at this pick's barrier
        if (pend) { LSYNC(); ring_store(pend_pos, pend_e, pend_b, pend_m); LSYNC(); pend = false; }      // (not under the entry being formed)
        bool dyn = false;
        stream = !finished && !err && nb < want && q_len > 0 && form_one(nb, dyn);
        if (stream) { q_head = (q_head + 1 == nP) ? 0 : q_head + 1; ++q_pos; --q_len; ++pops; }
      }
      if (lane == 0) C.hdr[RRH_NB2 + (j & 1u)] = nb | (same << 8);
      LSYNC();
      if (!hint) { prep_step(); prep_step(); }      // (two entries per pick: a round of four picks leaves nothing for the end, where the workers would wait for it; a round that announces a window phase leaves the records to the workers)
      __syncthreads();
      const u64 w = UF64(L.win[par][j]);
      u32 node, nrc, ch, key;
      kind = rr_pick_decide(nE, mw, w, node, nrc, ch, key);
      if (kind != 0) { s = j; wn = node; wnrc_s = nrc; child = ch; break; }
      if (lane == 0) L.pkch[j] = (u8)ch;
    }
    if (!run && kind == 0) s = nb;      // (pods may have joined since the round started)
    if (!run) prefer_run = false;
    LSYNC();
    s = UF(s); kind = UF(kind); wn = UF(wn); wnrc_s = UF(wnrc_s); child = UF(child);
    // Topology.Record on the narrow keys for the pods the workers committed (topology.go:120-143)
    if (!run) {      // (one lane per pod, like a run's: the record words of its class from L2 at once, the counters updated atomically)
      const u32 t = (u32)lane;
      if (t < s) {
        const u32 cls = L.ring[(pos0 + t) & (RR_RING - 1u)].w[49], ch = (u32)L.pkch[t];
        const GA u32* const cb = rrb + (size_t)cls * 48;
        const u32 nn = cb[18]; u32 rw[RR_MAXNREC];
#pragma unroll
        for (int r = 0; r < RR_MAXNREC; ++r) rw[r] = cb[40 + r];
#pragma unroll
        for (int r = 0; r < RR_MAXNREC; ++r) if ((u32)r < nn) record_word(rw[r], ch);
      }
      LSYNC();
    }
#ifdef KS_SIM
    if (lane == 0 && getenv("KS_SIM_DBG")) fprintf(stderr, "round %u run=%u nb=%u s=%u kind=%u pos0=%u wn=%u pre=%u q_pos=%u q_len=%u seq=%u win0=%llx ch0=%u\n", round, run, nb, s, kind, pos0, wn, n_pre, q_pos, q_len, seq, (unsigned long long)L.win[par][0], (u32)L.pkch[0]);
#endif
    RRP(3);
    while (pend || (!hint && (i32)(pp_pos - q_pos) < (i32)RR_B)) prep_step();      // (what the picks left unprepared)
    // ---------- 4. resolve ----------
    n_pre = 0; re_a = false;
    seq += s;
    if (s) a_nexcl = 0;
    // what was not placed goes back to the head of the queue, in order
    { const u32 back = nb - s; q_head = q_head >= back ? q_head - back : q_head + nP - back; q_pos -= back; q_len += back; pops -= back; }
    if (s < nb) {
      // ---- pod s needs the leader ----
      const RREntry& E = L.ring[(pos0 + s) & (RR_RING - 1u)];
      const u32 a_bw = E.w[lane];
      const u32 a_pod = RL(a_bw, 50), a_cls = RL(a_bw, 49), a_seq = seq, a_hmask = RL(a_bw, 51);
      i64 rq[4];
#pragma unroll
      for (int r = 0; r < 4; ++r) rq[r] = (i64)((u64)RL(a_bw, 2 * r) | ((u64)RL(a_bw, 2 * r + 1) << 32));
      const u32 prm = RL(a_bw, 8);
      bool placed = false;
      if (kind == 4) err = 2;      // more pods on one node than the key's count field holds: declined
      else if (kind == 3) {
        // the winner passed the screen but the nrc it would get has no single type holding every maximum (or other maxima than
        // the nrc it has): the exact filter decides (node.go:94-98).  Its owner says what it has requested so far.
        ++n_vfy;
        __syncthreads();                     // (a stop of this kind costs one more barrier: the owner has written L.ask)
        const u32 wmeta = (u32)UF64(L.ask.meta), rmn = ((wmeta >> 8) | prm) & 0xFu;
        i64 tot[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) tot[r] = (i64)UF64((u64)nt.cap[r][wnrc_s]) - (i64)UF64((u64)L.ask.room[r]) + rq[r];
        bool fits = true;
        if (wn >= nE) fits = rr_exact_fit(lane, child, tot[0], tot[1], tot[2], tot[3], rmn);
        if (fits) { n_pre = 2; pre_node = wn; pre_nrc = child; pre_seq = a_seq; pre_hmask = a_hmask; pre_bw = a_bw; placed = true; }
        else if (a_nexcl < 8) { a_excl[a_nexcl++] = wn; re_a = true; }
        else err = 3;
      } else {
        // ---- nothing accepts: a new machine from the first template that works (scheduler.go:193-213) ----
        u32 why = 0;
        const u32 a_bw_flags9 = RL(a_bw, 9);
        const bool have = try_open(a_bw, a_cls, a_seq, a_hmask, rq, prm, why, child);
        if (have) { wn = nE + nnew - 1u; placed = true; RR_BRK((a_bw_flags9 & 1u) ? 6 : 5); }
        if (!have && !err) {
          // ---- Preferences.Relax + Queue.Push + Topology.Update (scheduler.go:116-123): the pod leaves the head of the queue and joins its tail ----
          q_head = (q_head + 1 == nP) ? 0 : q_head + 1; ++q_pos; q_len--; ++pops;
          const u32 nst = UF(G_pod_stage_off[a_pod + 1] - G_pod_stage_off[a_pod]);
          const i32 stg = (i32)UF((u32)G_pod_stage[a_pod]);
          const bool relaxed = (u32)stg + 1 < nst;
          u32 tail = q_head + q_len; if (tail >= nP) tail -= nP;
          q_len++; pq_ok = false;
          const u32 ncls = relaxed ? UF(G_stage_cls[G_pod_stage_off[a_pod] + stg + 1]) : a_cls;
          LSYNC();      // (every lane has read the pod's stage before lane 0 moves it on -- the order lockstep gives anyway; the lane-fibre emulator needs it said: ksolve.hip, the same path of ks_pack)
          if (lane == 0) {
            G_pod_reason[a_pod] = why;
            tb.q[tail] = (u64)a_pod | ((u64)ncls << 32) | (relaxed ? 0ull : (1ull << 63));
            if (relaxed) G_pod_stage[a_pod] = stg + 1; else { G_lastlen[a_pod] = q_len; G_lastgen[a_pod] = q_gen; }
          }
          if (relaxed) {
            for (u32 i = P.cls_own_off[ncls] + (u32)lane; i < P.cls_own_off[ncls + 1]; i += 64) tb.g_active[P.own_list[i] & 0x7FFFFFFFu] = 1;      // Topology.Update creates the group
            LSYNC();
            g_active_mask = ballot64((u32)lane < nG && ft.g_active[lane] != 0);
            q_gen++; ++relaxations;
            if (lane < RR_RING) L.ring[lane].w[48] = 0xFFFFFFFFu;      // (the prepared records carry which hostname records count: prepared again)
            if (lane < (int)RR_PX) L.px[lane].u[0] = 0xFFFFFFFFu;
            ring_dirty = true;                                             // (... and once more behind the next B0: the workers may be preparing records with the old groups right now)
          }
          __threadfence_block(); GSYNC();
          a_nexcl = 0;
        }
      }
      if (placed && !err) {
        // the pod leaves the queue; the workers apply the order at the start of the next round, the leader does its half now
        q_head = (q_head + 1 == nP) ? 0 : q_head + 1; ++q_pos; q_len--; ++pops;
        if (lane == 0) { tb.pod_node[a_pod] = (i32)wn; tb.pod_seq[a_pod] = (i32)a_seq; G_pod_reason[a_pod] = 0;
        }
        narrow_record(a_bw, child);
        ++seq; a_nexcl = 0;
      }
    }
    if (err) { ++round; continue; }      // declined mid-run (or a hard error): the next iteration's B0 / B1 tell the workers to leave; the host decides
#ifdef KS_PROBES
    { const u64 tn = __builtin_readcyclecounter(); if (run) { cyc_runr += tn - t_round; pods_runr += s; } else { cyc_norm += tn - t_round; pods_norm += s + (n_pre ? 1u : 0u); ++n_normr; } t_round = tn; }
#endif
    RRP(4);
    ++round;
  }
  if (lane == 0) {
    L.fin[0] = nnew; L.fin[1] = err; L.fin[2] = q_head; L.fin[3] = q_len;
    u64* const o = L.lst;
    for (int i = 0; i < 32; ++i) o[i] = 0;
    o[KS_STAT_POPS] = pops; o[KS_STAT_RELAX] = relaxations; o[KS_STAT_FULLCHECKS] = n_create + n_vfy; o[KS_STAT_FULLFAILS] = n_dyn_f;
    o[8] = round; o[9] = rounds_eval; o[10] = n_bubble; o[11] = n_phase_a; o[12] = n_nrc; o[13] = n_vfy;
    o[22] = n_run_pods; o[23] = n_run_steps; o[24] = n_runs; o[27] = n_wpods; o[28] = n_wphases; o[25] = (u64)L.wbrk[0] | ((u64)L.wbrk[1] << 12) | ((u64)L.wbrk[2] << 24) | ((u64)L.wbrk[3] << 36) | ((u64)L.wbrk[4] << 48); o[30] = n_wquery; o[31] = (u64)L.wbrk[5] | ((u64)L.wbrk[6] << 16); o[26] = L.wstop[3];      /* (26: questions the census of zero counters answered) */ o[29] = (u64)L.wstop[2] | ((u64)L.wstop[5] << 21) | ((u64)L.wstop[6] << 42);      // head window: pods placed | phases | why they ended: the leader's business / nothing in the window accepts / the exact filter
#ifdef KS_PROBES
    o[25] = rrp[14]; o[26] = rrp[15]; o[4] = cyc_runr; o[5] = cyc_norm; o[1] = ((u64)pods_runr << 32) | pods_norm; o[31] = n_normr;
#endif
#ifdef KS_PROBES
    for (int i = 0; i < 6; ++i) o[15 + i] = rrp[i];
    o[2] = rrp[6]; o[3] = rrp[7]; o[0] = rrp[13];      // (formation: flags | cached answers | dyn1 answers; o[20] = entry lookup)
#ifdef KS_PROBES_WIN      /* the head window: wait for the lend | set-up | rr_window in all || inside it: parameters + control word | dyn1 | evaluate + minimum | commit + records | preparing records */
    o[27] = rrp[8]; o[28] = rrp[9]; o[29] = rrp[10]; o[30] = L.wpr[0]; o[31] = L.wpr[1]; o[21] = L.wpr[2]; o[12] = L.wpr[3]; o[13] = L.wpr[4]; o[10] = n_wpods; o[11] = n_wphases;
    o[22] = L.wpr[5]; o[23] = L.wpr[6]; o[24] = L.wpr[7];      // (this build only: the loop's waits by cause, in the run statistics' slots)
    o[9] = (u64)L.wstop[2] | ((u64)L.wstop[5] << 21) | ((u64)L.wstop[6] << 42);
#endif
#ifdef KS_PROBES_WQ
    for (int i = 0; i < 5; ++i) o[15 + i] = wq_c[i]; o[20] = wq_c[5];
#endif
#endif
  }
}

__global__ __launch_bounds__(64 * RR_NW) void ks_pack_rr(const DevProb* probs, const DevState* states, u32 lds_bytes) {
  RRLds& L = g_rr_lds;
  const int lane = threadIdx.x & 63; const u32 wv = UF(threadIdx.x >> 6);
  { const u32* src = (const u32*)&probs[blockIdx.x]; u32* dst = (u32*)&L.P; for (u32 i = threadIdx.x; i < sizeof(DevProb) / 4; i += 64 * RR_NW) dst[i] = src[i]; }
  { const u32* src = (const u32*)&states[blockIdx.x]; u32* dst = (u32*)&L.S; for (u32 i = threadIdx.x; i < sizeof(DevState) / 4; i += 64 * RR_NW) dst[i] = src[i]; }
  __syncthreads();
  const u64 t_start = __builtin_readcyclecounter();
  const DevProb& P = L.P; const DevState& S = L.S; WaveShared& sh = L.sh; RRNrc& nt = L.nt; LeaderShared& ls = L.ls;
  Tabs tb;
  tb.K = UF(P.K); tb.R = UF(P.R); tb.T = UF(P.T); tb.TW = UF(P.TW); tb.GH = UF(P.GH); tb.E = UF(P.E); tb.S = UF(P.S); tb.SC = UF(P.SC); tb.n_ct = UF(P.n_ct); tb.wellknown = UF(P.wellknown_mask); tb.key_zone = (i32)UF(P.key_zone); tb.key_ct = (i32)UF(P.key_ct);
  tb.q = (GA u64*)UF64((u64)S.q); tb.pod_node = (GA i32*)UF64((u64)S.pod_node); tb.pod_seq = (GA i32*)UF64((u64)S.pod_seq);
  tb.rec = (GA u8*)UF64((u64)S.rec); tb.rec_stride = UF(S.rec_stride); tb.hcnt = (GA i32*)UF64((u64)S.hcnt); tb.n_alive = (GA u64*)UF64((u64)S.n_alive); tb.ge_rows = (const GA u64*)UF64((u64)P.ge_rows);
  const u32 nP = UF(P.P), nM = UF(P.M), nC = UF(P.C), nG = UF(P.G), nMAX = UF(P.NMAX), nE = tb.E, nK = tb.K, nR = tb.R, nTW = tb.TW;
  // ---- static eligibility (anything else: declined before a byte of state is written) ----
  const bool eligible = nK <= RR_KMAX && nR <= 4 && nG <= 64 && tb.GH <= 4 * RR_GW && nE <= 64 && nE <= RR_NODES && nTW <= 128 && nP <= RR_SEQMAX && tb.SC == 1 &&
                        P.pod_gid == nullptr && P.en_removed == nullptr && P.rr_briefs != nullptr && (size_t)nR * UF(P.ge_max) * 8 + 64 <= lds_bytes;
  if (!eligible) {
    if (threadIdx.x == 0) { for (int i = 0; i < 32; ++i) S.stats[i] = 0; S.stats[KS_STAT_ERR] = KS_RR_DECLINED; S.stats[14] = 1; S.out_counts[0] = 0; S.out_counts[1] = 0; }
    return;
  }
  // ---- small hot tables in LDS (the FAST layout of ks_pack) ----
  FastTabs& ft = L.ft;
  i64* const ge = (i64*)ks_dyn_lds; const u32 gs = UF(P.ge_max);
  if (wv == 0) {
    for (u32 i = lane; i < nK; i += 64) ft.key_nvalues[i] = P.key_nvalues[i];
    for (u32 i = lane; i < nK * 64; i += 64) ft.value_int[i] = P.value_int[i];
    for (u32 i = lane; i < nG * 64; i += 64) ft.gcnt[i] = P.grp_count[i];
    for (u32 g = lane; g < nG; g += 64) {
      u64 reg = 0, pos = 0; for (int d = 0; d < 64; ++d) { const i32 c = P.grp_count[(size_t)g * 64 + d]; if (c >= 0) reg |= 1ull << d; if (c > 0) pos |= 1ull << d; }
      ft.g_reg[g] = reg; ft.g_pos[g] = pos; ft.g_active[g] = P.grp_active[g];
    }
    for (u32 h = lane; h < KS_FAST_G; h += 64) { ft.g_hpos[h] = 0; ft.g_hzero[h] = 0; }
    for (u32 i = lane; i < nR; i += 64) ft.ge_cnt[i] = P.ge_cnt[i];
    for (u32 r = 0; r < nR; ++r) for (u32 i = lane; i < gs; i += 64) ge[(size_t)r * gs + i] = i < P.ge_cnt[r] ? P.ge_vals[(size_t)r * tb.T + i] : INT64_MAX;
    if (lane < 32) ls.ctr[lane] = 0;
    ls.hslot_of[lane] = ((u32)lane < nG && P.grp_hslot[lane] >= 0 && P.grp_hslot[lane] < 255) ? (u8)P.grp_hslot[lane] : (u8)0xFF;
    nt.nchild[lane] = 0;
    if (lane < 32) { L.ctl[0].hdr[lane] = 0; L.ctl[1].hdr[lane] = 0; }
    for (u32 i = lane; i < sizeof(L.t2) / 4; i += 64) ((u32*)L.t2)[i] = 0xFFFFFFFFu;
    L.vpair[lane] = 0; if (lane < 2) L.dynk[lane] = 0xFFu;
    L.ring[lane & (RR_RING - 1)].w[48] = 0xFFFFFFFFu;
    if (lane == 0) sh.cls.c = 0xFFFFFFFFu;
    if (lane < 8) { L.wstop[lane] = 0; L.wpr[lane] = 0; L.wsink[lane] = 0; }
    L.wn_hc[RR_GW][lane] = 0; L.wn_hc[RR_GW + 1][lane] = 0; L.wsinkl[0][lane] = 0; L.wsinkl[1][lane] = 0; L.wsinkl[2][lane] = 0; L.wn_key[lane] = 0xFFFFFFFFu;
    if (lane < (int)RR_PX) { for (int i = 0; i < 24; ++i) L.px[lane].u[i] = 0; L.px[lane].u[0] = 0xFFFFFFFFu; }
    if (lane < 32) L.hz[lane] = 0; if (lane < 8) L.wbrk[lane] = 0;
  }
  tb.key_nvalues = ft.key_nvalues; tb.value_int = ft.value_int; tb.its_fail = ft.its_fail; tb.its_inter = ft.its_inter;
  tb.gcnt = ft.gcnt; tb.g_reg = ft.g_reg; tb.g_pos = ft.g_pos; tb.g_active = ft.g_active; tb.g_hpos = ft.g_hpos; tb.g_hzero = ft.g_hzero; tb.ge_cnt = ft.ge_cnt; tb.ge_vals = ge; tb.ge_stride = gs;
  // ---- queue and per-pod results (every wave) ----
  for (u32 i = threadIdx.x; i < nP; i += 64 * RR_NW) {
    const u32 pd = P.queue ? P.queue[i] : i;
    tb.q[i] = (u64)pd | ((u64)P.stage_cls[P.pod_stage_off[pd]] << 32); G_lastgen[i] = 0xFFFFFFFFu; G_lastlen[i] = 0; G_pod_stage[i] = 0; tb.pod_node[i] = -1; tb.pod_seq[i] = -1; G_pod_reason[i] = 0;
  }
  const GA ClsPlan* const plans = (const GA ClsPlan*)UF64((u64)P.plans);
  const GA u32* const rrb = (const GA u32*)UF64((u64)P.rr_briefs);
  GA u32* const rrm = (GA u32*)UF64((u64)P.rr_memo);
  GA u64* const rr_types = (GA u64*)UF64((u64)P.rr_types);
  const GA u32* const rr_mi = (const GA u32*)UF64((u64)P.rr_mi);
  for (u32 i = threadIdx.x; i < nC * 24u; i += 64 * RR_NW) rrm[i] = 0;                                 // nothing is cached yet (a resident problem may be solved again)
  for (size_t i = threadIdx.x; i < (size_t)nM * nC; i += 64 * RR_NW) { ((GA u8*)P.rr_mcnrc)[i] = 0xFFu; ((GA u8*)P.rr_mcch)[i] = 0xFFu; }
  __threadfence_block();
  __syncthreads();

  if (wv == 0) rr_leader(lane); else rr_worker(wv, lane);
  if (UF(L.init_err)) {
    if (threadIdx.x == 0) { for (int i = 0; i < 32; ++i) S.stats[i] = 0; S.stats[KS_STAT_ERR] = KS_RR_DECLINED; S.stats[14] = 5; S.out_counts[0] = 0; S.out_counts[1] = 0; }
    return;
  }

  // ---------------- results ----------------
  __syncthreads();                         // (the leader's L.fin / L.lst and the workers' node hand-over are visible)
  const u32 f_nnew = UF(L.fin[0]), f_err = UF(L.fin[1]), f_qhead = UF(L.fin[2]), f_qlen = UF(L.fin[3]);
#if defined(KS_SIM) || defined(KS_CHECK)
  if (!f_err && threadIdx.x < 32 && L.hz[threadIdx.x] != 0) { printf("ks_pack_rr: the census of zero hostname counters is off by %d for slot %u\n", L.hz[threadIdx.x], threadIdx.x); S.stats[KS_STAT_ERR] = 0xBAD; }
#endif
  if (!f_err) {
    const GA u64* const dump = (const GA u64*)P.rr_nodes;
    for (u32 j = wv; j < f_nnew; j += RR_NW) {      // InstanceTypeOptions and the record of every new node, a wave per node
      const u32 n = nE + j;
      const u32 meta = (u32)UF64(dump[(size_t)n * 5]), nrc = meta & 0xFFu, rm = (meta >> 8) & 0xFFu;
      PubT<4> pbx;
#pragma unroll
      for (int r = 0; r < 4; ++r) { pbx.req_new[r] = (i64)UF64((u64)nt.cap[r][nrc]) - (i64)UF64(dump[(size_t)n * 5 + 1 + r]); pbx.room_new[r] = 0; }
      u32 ridx[4]; ge_row_indices(tb, pbx, rm, lane, ridx);
      for (u32 wbase = 0; wbase < nTW; wbase += 64) {
        const u32 w = wbase + lane;
        if (w < nTW) {
          u64 a = rr_types[(size_t)nrc * nTW + w];
#pragma unroll
          for (int i = 0; i < 4; ++i) if ((rm >> i) & 1u) a &= ridx[i] < tb.ge_cnt[i] ? tb.ge_rows[((size_t)i * tb.T + ridx[i]) * nTW + w] : 0ull;
          tb.n_alive[(size_t)j * nTW + w] = a;
        }
      }
      if ((u32)lane < nK) { S.o_mask[(size_t)j * nK + lane] = ((nt.present[nrc] >> lane) & 1u) ? nt.mask[lane][nrc] : 0ull; S.o_gt[(size_t)j * nK + lane] = KS_NOGT; S.o_lt[(size_t)j * nK + lane] = KS_NOLT; }
      if (lane >= 32 && (u32)lane < 32 + nR) S.o_req[(size_t)j * nR + lane - 32] = lane == 32 ? pbx.req_new[0] : lane == 33 ? pbx.req_new[1] : lane == 34 ? pbx.req_new[2] : pbx.req_new[3];
      if (lane == 63) { S.o_present[j] = nt.present[nrc]; S.o_complement[j] = nt.complement[nrc]; S.o_it[j] = nt.it[nrc]; S.o_reqmask[j] = rm; }
    }
    for (u32 i = threadIdx.x; i < f_qlen; i += 64 * RR_NW) { u32 idx = f_qhead + i; if (idx >= nP) idx -= nP; S.unscheduled[i] = (i32)tb.q[idx]; }
  }
  if (wv == 0 && lane == 0) {
    S.out_counts[0] = f_err ? 0 : f_nnew; S.out_counts[1] = f_err ? 0 : f_qlen;
    for (int i = 0; i < 32; ++i) S.stats[i] = L.lst[i];
    S.stats[14] = f_err;
#ifdef KS_PROBES
#ifdef KS_PROBES_WIN      /* the head window: leader's wait for the lend | load + hand-back | form_one | evaluate + minimum | commit + records; 21 / 12: pods / phases */
    /* (everything is in the leader's L.lst already) */
#elif defined(KS_PROBES_RUN)      /* the phases of a run's step instead of the normal rounds': extraction | barrier | merge | commit + retry; 31: B1 wait */
    S.stats[21] = L.wst[14]; S.stats[27] = L.wst[1]; S.stats[28] = L.wst[2]; S.stats[29] = L.wst[3]; S.stats[30] = L.wst[4]; S.stats[31] = L.wst[8]; S.stats[12] = L.wst[0]; S.stats[13] = L.wst[5]; S.stats[25] = L.wst[6]; S.stats[26] = L.wst[7];
#else
    S.stats[21] = L.wst[14]; S.stats[27] = L.wst[8]; S.stats[28] = L.wst[9]; S.stats[29] = L.wst[10]; S.stats[30] = L.wst[11]; S.stats[31] = L.wst[12]; S.stats[12] = L.wst[13];      // (worker 1: B1 wait | between pods (commit, loop) | EVAL | candidate + atomic | barrier | decide; 21: round tail incl. runs)
#endif
#endif
    S.stats[KS_STAT_CYCLES] = __builtin_readcyclecounter() - t_start;
    S.stats[KS_STAT_ERR] = f_err == 0 ? 0 : KS_RR_DECLINED;      // (every non-zero code is a decline: stats[14] says which)
    if (S.batch_meta) { S.batch_meta[0] = S.out_counts[0]; S.batch_meta[1] = S.out_counts[1]; for (int i = 0; i < 32; ++i) S.batch_meta[2 + i] = S.stats[i]; }
  }
}

#ifndef KS_SIM
// (this file's light LSYNC ends here: whatever follows the include in ksolve.hip gets the fenced hand-off back)
#undef LSYNC
#define LSYNC() do { __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront"); __builtin_amdgcn_wave_barrier(); __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront"); } while (0)
#endif
