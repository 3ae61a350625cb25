// ks_audit.inc -- the audit of a Solve's result against the problem it answers (ksolve.h ks_audit_dev / ks_audit_batch_dev, KS_AUDIT_*).  Included by ksolve.hip
// after the placement rows, outside the emulator's guards: the tests/sim build compiles and runs these kernels too.
//
// Every check is an invariant of the reference's algorithm that holds in the FINAL state whatever order the pods were placed in, so the audit needs neither the
// pack kernels nor a second run of them: it reads the problem's arrays and the result where it lies (a Solve's own DevState, or a claimed result uploaded for the
// call) and writes one flag word per pod and per node.  Four launches on the problems' stream, blockIdx.y = the problem:
//   ks_audit_count   one lane per pod: the unscheduled list marked in a P-sized scratch array, the pods of every node counted (a counting sort's first half; the
//                    atomics go to scratch only -- no output is appended through one, so the flags are the same every run).
//   ks_audit_scan    one workgroup per problem: the exclusive scan of the counts (Hillis-Steele over an LDS tile, ks_placement_heads' way) = the node -> pods CSR's offsets.
//   ks_audit_pods    one lane per pod: the pod bits that need no neighbour, and the pod's slot in its node's list (the counting sort's second half: the order within a
//                    node depends on the run, and nothing below depends on that order -- int64 sums, unions and all-pairs tests).
//   ks_audit_nodes   one wave per node: lanes stride the node's pods for the int64 sums and reduce across the wave; then one instance type per lane -- the per-type
//                    predicate every pass shares (AudNode, aud_node_type_ok below), over the node as the result leaves it -- and a ballot gives the 64-bit word that is
//                    compared with the node's InstanceTypeOptions.  Host ports and volumes are walked per node (rare and short).  The PORTS bit of a pod is added to its flag
//                    word by the one lane that holds the pod: a plain read-modify-write, after ks_audit_pods has finished.
struct AuditView {
  const i32* pod_node; const i32* pod_stage; const i32* pod_seq; const i32* unscheduled; const u32* counts;      // counts: [0] n_new, [1] n_unscheduled
  const i32* n_tmpl; const u64* n_types; const i64* o_req; const u32* o_reqmask; const u32* o_present; const u32* o_complement; const u64* o_mask; const i32* o_gt; const i32* o_lt; const i32* o_it;
  u32* meta; u32* pod_flags; u32* node_flags;      // outputs: meta [0] n_new, [1] n_unscheduled as the kernels read them | [P] | [E + NMAX]
  u32* mark; u32* cnt; u32* off; u32* fill; u32* pods;      // scratch, zeroed before the first launch: [P] | [E + NMAX] | [E + NMAX + 1] | [E + NMAX] | [P]
};
__device__ __forceinline__ u32 aud_n_new(const DevProb& P, const AuditView& V) { const u32 n = GC(u32, V.counts)[0]; return n < P.NMAX ? n : P.NMAX; }
__device__ __forceinline__ u32 aud_n_unsched(const DevProb& P, const AuditView& V) { const u32 n = GC(u32, V.counts)[1]; return n < P.P ? n : P.P; }
__device__ __forceinline__ u32 aud_n_stages(const DevProb& P, u32 p) { const u32 gp = P.pod_gid ? GC(u32, P.pod_gid)[p] : p; return GC(u32, P.pod_stage_off)[gp + 1] - GC(u32, P.pod_stage_off)[gp]; }
// the class of the stage the pod ended at; a stage outside the pod's chain (flagged RANGE) reads as stage 0 where a node still has to count the pod
__device__ __forceinline__ u32 aud_class(const DevProb& P, const AuditView& V, u32 p) {
  const u32 gp = P.pod_gid ? GC(u32, P.pod_gid)[p] : p; const u32 o = GC(u32, P.pod_stage_off)[gp], n = GC(u32, P.pod_stage_off)[gp + 1] - o;
  const i32 st = GC(i32, V.pod_stage)[p];
  return GC(u32, P.stage_cls)[o + ((st >= 0 && (u32)st < n) ? (u32)st : 0u)];
}
// the node a pod is on, or -1: unscheduled, outside [0, E + n_new), or an existing node that left the cluster (a derived what-if's candidate)
__device__ __forceinline__ i32 aud_where(const DevProb& P, const AuditView& V, u32 p, u32 NS) {
  const i32 nd = GC(i32, V.pod_node)[p];
  if (nd < 0 || (u32)nd >= NS) return -1;
  if ((u32)nd < P.E && P.en_removed && ((GC(u64, P.en_removed)[(u32)nd >> 6] >> ((u32)nd & 63u)) & 1ull)) return -1;
  return nd;
}
__device__ __forceinline__ u64 aud_xor64(u64 v, int x) { const u32 lo = __shfl_xor((u32)v, x), hi = __shfl_xor((u32)(v >> 32), x); return (u64)lo | ((u64)hi << 32); }
__device__ __forceinline__ u64 aud_wave_or(u64 v) { for (int x = 32; x > 0; x >>= 1) v |= aud_xor64(v, x); return v; }
__device__ __forceinline__ u64 aud_wave_add(u64 v) { for (int x = 32; x > 0; x >>= 1) v += aud_xor64(v, x); return v; }
// entry.matches, hostportusage.go:45-57: protocol and port equal, and the addresses equal or either unspecified
__device__ __forceinline__ bool aud_port_match(u64 a, u64 b) { if ((a >> 32) != (b >> 32)) return false; const u32 ia = (u32)a, ib = (u32)b; return ia == ib || ia == 0 || ib == 0; }
// ---- what the passes over the commit order (ks_audit_topo.inc and the files after it) share with this one ----
// is the placed pod's commit number one the rules may order by?  (below the number of placed pods, and no other placed pod's; seqcnt: the pass's own counts per commit number)
__device__ __forceinline__ bool aud_seq_ok(const AuditView& V, const u32* seqcnt, u32 p, u32 n_placed) {
  const i32 sq = GC(i32, V.pod_seq)[p];
  return sq >= 0 && (u32)sq < n_placed && seqcnt[sq] == 1u;
}
// the zone x capacity-type pairs a requirement set allows: bit z * n_ct + c of it_offer's words (z, ct: the set's requirements on the two keys, absent where the problem has no such key)
__device__ __forceinline__ u64 aud_pairs(const DevProb& P, const KReq& z, const KReq& ct) {
  u64 allowZ = ~0ull, allowC = ~0ull;
  if (P.key_zone >= 0 && z.present) allowZ = kreq_has_mask(z, P.value_int + P.key_zone * 64, GC(u32, P.key_nvalues)[P.key_zone]);
  if (P.key_ct >= 0 && ct.present) allowC = kreq_has_mask(ct, P.value_int + P.key_ct * 64, GC(u32, P.key_nvalues)[P.key_ct]);
  if (P.n_ct == 0) return ~0ull;
  u64 pairs = 0;
  for (u64 zz = allowZ; zz; zz &= zz - 1) { const int zi = __builtin_ctzll(zz); if ((u32)zi * P.n_ct >= 64) break; pairs |= (allowC & ((1ull << P.n_ct) - 1)) << (zi * P.n_ct); }
  return pairs;
}
// is existing node e in class c's hostname list?  (existing node e owns hostname e; a new node's placeholder is in no list, node.go:46)
__device__ __forceinline__ bool aud_hn_listed(const DevProb& P, u32 c, u32 e) {
  for (u32 i = GC(u32, P.cls_hn_off)[c]; i < GC(u32, P.cls_hn_off)[c + 1]; ++i) if (GC(u32, P.hn_list)[i] == e) return true;
  return false;
}
// ---- filterInstanceTypesByRequirements (node.go:137-159) as every pass evaluates it: one view of the node, one state meet, one predicate per type, one walk ----
__device__ __forceinline__ KReq aud_fit_cls_req(const DevProb& P, u32 c, u32 k) {
  return load_req(GC(u32, P.cls.present)[c], GC(u32, P.cls.complement)[c], P.cls.mask + (size_t)c * P.K, P.cls.gt + (size_t)c * P.K, P.cls.lt + (size_t)c * P.K, (int)k);
}
// what an instance type is filtered against: the node's requirements (presence and complement words; mask, gt and lt rows), its requests and their presence mask, its
// type set, its instance-type state and its template -- as the makers below leave it, or with one pod of class c on top (aud_node_add); pairs: aud_node_pairs
struct AudNode { u32 np_, nc_, rmask, c; const u64* nmask; const i32* ngt; const i32* nlt; const i64* nreq; const u64* ntypes; i32 it, m; u64 pairs; bool cls; };
// new node j as the result leaves it (m: as claimed -- the caller tests its range before it reads anything through it)
__device__ __forceinline__ AudNode aud_node_final(const DevProb& P, const AuditView& V, u32 j) {
  AudNode n; const u32 K = P.K;
  n.np_ = GC(u32, V.o_present)[j]; n.nc_ = GC(u32, V.o_complement)[j]; n.nmask = V.o_mask + (size_t)j * K; n.ngt = V.o_gt + (size_t)j * K; n.nlt = V.o_lt + (size_t)j * K;
  n.nreq = V.o_req + (size_t)j * P.R; n.rmask = GC(u32, V.o_reqmask)[j]; n.ntypes = V.n_types + (size_t)j * P.TW; n.it = GC(i32, V.o_it)[j]; n.m = GC(i32, V.n_tmpl)[j];
  n.c = 0; n.cls = false; n.pairs = 0;
  return n;
}
// a fresh node of template m: the template's requirements, its daemon overhead, its types
__device__ __forceinline__ AudNode aud_node_fresh(const DevProb& P, u32 m) {
  AudNode n; const u32 K = P.K;
  n.np_ = GC(u32, P.tmpl.present)[m]; n.nc_ = GC(u32, P.tmpl.complement)[m]; n.nmask = P.tmpl.mask + (size_t)m * K; n.ngt = P.tmpl.gt + (size_t)m * K; n.nlt = P.tmpl.lt + (size_t)m * K;
  n.nreq = P.tmpl_daemon + (size_t)m * P.R; n.rmask = GC(u32, P.tmpl_daemon_present)[m]; n.ntypes = P.tmpl_types + (size_t)m * P.TW; n.it = GC(i32, P.tmpl.it_state)[m]; n.m = (i32)m;
  n.c = 0; n.cls = false; n.pairs = 0;
  return n;
}
// the view's requirement on key k
__device__ __forceinline__ KReq aud_node_req(const DevProb& P, const AudNode& n, u32 k) {
  const KReq a = load_req(n.np_, n.nc_, n.nmask, n.ngt, n.nlt, (int)k);
  return n.cls ? kreq_add(a, aud_fit_cls_req(P, n.c, k), P.value_int + k * 64, GC(u32, P.key_nvalues)[k]) : a;
}
// the zone x capacity-type pairs the view allows: taken once per view, after the last change to it
__device__ __forceinline__ void aud_node_pairs(const DevProb& P, AudNode& n) {
  KReq rz = kreq_absent(), rc = kreq_absent();
  if (P.key_zone >= 0) rz = aud_node_req(P, n, (u32)P.key_zone);
  if (P.key_ct >= 0) rc = aud_node_req(P, n, (u32)P.key_ct);
  n.pairs = aud_pairs(P, rz, rc);
}
// one pod of class c on top: its requirements met with the node's, its requests added
__device__ __forceinline__ void aud_node_add(const DevProb& P, AudNode& n, u32 c) {
  n.c = c; n.cls = true; n.rmask |= GC(u32, P.cls_requests_present)[c];
  aud_node_pairs(P, n);
}
// the view's instance-type state met with class c's, or S where the lattice has no meet; aud_node_state_refuses: the two are not Compatible at all
__device__ __forceinline__ bool aud_node_state_refuses(const DevProb& P, const AudNode& n, u32 c) {
  const i32 sa = n.it, sb = GC(i32, P.cls.it_state)[c];
  return sa < 0 || (u32)sa >= P.S || (P.SC && (sb < 0 || (u32)sb >= P.SC || GC(u8, P.its_fail)[(size_t)sa * P.SC + sb]));
}
__device__ __forceinline__ u32 aud_node_state_meet(const DevProb& P, const AudNode& n, u32 c) {
  if (aud_node_state_refuses(P, n, c)) return P.S;
  if (!P.SC) return (u32)n.it;
  const u32 si = GC(u16, P.its_inter)[(size_t)n.it * P.SC + (u32)GC(i32, P.cls.it_state)[c]];
  return si < P.S ? si : P.S;
}
// compatible && fits && hasOffering (node.go:137-159) for type t
__device__ __forceinline__ bool aud_node_type_ok(const DevProb& P, const AudNode& n, u32 t) {
  const u32 K = P.K, R = P.R, T = P.T, tp = GC(u32, P.it_present)[t], tc = GC(u32, P.it_complement)[t], mp = n.cls ? (n.np_ | GC(u32, P.cls.present)[n.c]) : n.np_;
  bool ok = true;
  for (u32 k = 0; k < K && ok; ++k) {
    if (!((mp >> k) & 1u) || !((tp >> k) & 1u)) continue;
    KReq a; a.present = true; a.complement = (tc >> k) & 1u; a.mask = GC(u64, P.it_mask)[(size_t)k * T + t]; a.gt = KS_NOGT; a.lt = KS_NOLT;
    if (kreq_intersects_fail(a, aud_node_req(P, n, k), P.value_int + k * 64, GC(u32, P.key_nvalues)[k])) ok = false;
  }
  for (u32 r = 0; r < R && ok; ++r) {
    if (!((n.rmask >> r) & 1u)) continue;
    const i64 need = n.cls ? (i64)((u64)GC(i64, n.nreq)[r] + (u64)GC(i64, P.cls_requests)[(size_t)n.c * R + r]) : GC(i64, n.nreq)[r];
    if (need > GC(i64, P.it_alloc)[(size_t)r * T + t]) ok = false;
  }
  return ok && (GC(u64, P.it_offer)[t] & n.pairs) != 0;
}
// does any type of the view's set and of state si pass?  One type per lane, word by word -- it_mask[k*T+t] coalesced over t --; a ballot ends the walk at the first
// word a type passes in (the ballot is the same in all 64 lanes: they leave together)
__device__ __forceinline__ bool aud_node_any_type(const DevProb& P, const AudNode& n, u32 si, u32 lane) {
  bool any = false;
  for (u32 tw = 0; tw < P.TW && !any; ++tw) {
    const u32 t = tw * 64u + lane;
    bool ok = t < P.T && ((GC(u64, n.ntypes)[tw] >> lane) & 1ull) && ((GC(u64, P.its_types)[(size_t)si * P.TW + tw] >> lane) & 1ull);
    if (ok) ok = aud_node_type_ok(P, n, t);
    any = ballot64(ok) != 0;
  }
  return any;
}
// the sum of `mine` over the 256 threads of the workgroup, in s[0] for thread 0 (s: an LDS tile of 256 the caller owns and may use again after a barrier)
__device__ __forceinline__ void aud_block_sum(u32* s, u32 mine) {
  s[threadIdx.x] = mine;
  for (u32 o = 128u; o > 0; o >>= 1) { __syncthreads(); if (threadIdx.x < o) s[threadIdx.x] += s[threadIdx.x + o]; }
}

__global__ __launch_bounds__(256) void ks_audit_count(const DevProb* probs, const AuditView* views) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), nu = aud_n_unsched(P, V);
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < np; i += gridDim.x * 256u) {
    if (i < nu) { const i32 u = GC(i32, V.unscheduled)[i]; if (u >= 0 && (u32)u < np) atomicAdd(&V.mark[u], 1u); }
    const i32 nd = aud_where(P, V, i, NS);
    if (nd >= 0) atomicAdd(&V.cnt[nd], 1u);
  }
}
__global__ __launch_bounds__(256) void ks_audit_scan(const DevProb* probs, const AuditView* views) {
  __shared__ u32 s_sum[256];
  const DevProb& P = probs[blockIdx.x]; const AuditView& V = views[blockIdx.x];
  const u32 tid = threadIdx.x, NS = P.E + aud_n_new(P, V); u32 carry = 0;
  for (u32 base = 0; base < NS; base += 256u) {      // (NS is read from one address by every lane: every lane walks every tile and every scan step)
    const u32 i = base + tid; const u32 mine = i < NS ? V.cnt[i] : 0u;
    s_sum[tid] = mine;
    for (u32 o = 1; o < 256u; o <<= 1) {
      __syncthreads();
      const u32 x = tid >= o ? s_sum[tid - o] : 0u;
      __syncthreads();
      s_sum[tid] += x;
    }
    __syncthreads();
    if (i < NS) V.off[i] = carry + s_sum[tid] - mine;
    carry += s_sum[255];
    __syncthreads();
  }
  if (tid == 0) { V.off[NS] = carry; V.meta[0] = aud_n_new(P, V); V.meta[1] = aud_n_unsched(P, V); }
}
__global__ __launch_bounds__(256) void ks_audit_pods(const DevProb* probs, const AuditView* views) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y];
  const u32 np = P.P, E = P.E, NS = E + aud_n_new(P, V), K = P.K;
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    u32 f = 0;
    const i32 raw = GC(i32, V.pod_node)[p], st = GC(i32, V.pod_stage)[p], sq = GC(i32, V.pod_seq)[p];
    const i32 nd = aud_where(P, V, p, NS);
    const bool stage_ok = st >= 0 && (u32)st < aud_n_stages(P, p);
    if (raw != -1 && nd < 0) f |= KS_AUDIT_POD_RANGE;
    if (!stage_ok) f |= KS_AUDIT_POD_RANGE;
    if (raw == -1 ? sq != -1 : sq < 0) f |= KS_AUDIT_POD_RANGE;
    const u32 listed = V.mark[p];
    if (raw == -1 ? listed != 1u : listed != 0u) f |= KS_AUDIT_POD_UNSCHEDULED_LIST;
    if (nd >= 0) V.pods[V.off[nd] + atomicAdd(&V.fill[nd], 1u)] = p;      // (its node counts the pod whatever else is wrong with it)
    if (nd >= 0 && stage_ok) {
      const u32 c = aud_class(P, V, p); const bool existing = (u32)nd < E; const u32 j = (u32)nd - E;
      const u32 cp = GC(u32, P.cls.present)[c], cc = GC(u32, P.cls.complement)[c]; const i32 sb = GC(i32, P.cls.it_state)[c];
      const i32 m = existing ? 0 : GC(i32, V.n_tmpl)[j]; const bool tmpl_ok = existing || (m >= 0 && (u32)m < P.M);
      // Taints.Tolerates, taints.go:28-40 (a new node whose template is out of range is the node's finding: KS_AUDIT_NODE_TEMPLATE)
      if (tmpl_ok) { const u64 taints = existing ? GC(u64, P.en_taints)[nd] : GC(u64, P.tmpl_taints)[m]; if (taints & ~GC(u64, P.cls_tolerated)[c]) f |= KS_AUDIT_POD_TAINTS; }
      // existing node: Compatible(node, pod) (existingnode.go:104); new node: Intersects(the node's final requirements, pod) -- the requirements only narrowed since the pod arrived
      const u32 npres = existing ? GC(u32, P.en.present)[nd] : GC(u32, V.o_present)[j], ncomp = existing ? GC(u32, P.en.complement)[nd] : GC(u32, V.o_complement)[j];
      const u64* nmask = existing ? P.en.mask + (size_t)nd * K : V.o_mask + (size_t)j * K;
      const i32* ngt = existing ? P.en.gt + (size_t)nd * K : V.o_gt + (size_t)j * K; const i32* nlt = existing ? P.en.lt + (size_t)nd * K : V.o_lt + (size_t)j * K;
      bool bad = false;
      for (u32 k = 0; k < K; ++k) {
        if (!((cp >> k) & 1u)) continue;
        const KReq a = load_req(npres, ncomp, nmask, ngt, nlt, (int)k);
        const KReq b = load_req(cp, cc, P.cls.mask + (size_t)c * K, P.cls.gt + (size_t)c * K, P.cls.lt + (size_t)c * K, (int)k);
        const i32* vi = P.value_int + k * 64; const u32 nv = GC(u32, P.key_nvalues)[k];
        if (existing ? kreq_compatible_fail(a, b, (P.wellknown_mask >> k) & 1u, vi, nv) : kreq_intersects_fail(a, b, vi, nv)) bad = true;
      }
      const i32 sa = existing ? GC(i32, P.en.it_state)[nd] : GC(i32, V.o_it)[j];
      if (P.SC && (sa < 0 || (u32)sa >= P.S || sb < 0 || (u32)sb >= P.SC || GC(u8, P.its_fail)[(size_t)sa * P.SC + sb])) bad = true;
      if (bad) f |= KS_AUDIT_POD_REQUIREMENTS;
      // the hostname requirement: existing node e owns hostname e, a new node's placeholder is in no list (node.go:46)
      const u32 hm = GC(u8, P.cls_hn_mode)[c];
      if (hm) {
        const bool inlist = existing && aud_hn_listed(P, c, (u32)nd);
        if (hm == 1 ? !inlist : inlist) f |= KS_AUDIT_POD_HOSTNAME;
      }
      // VolumeUsage.validate failed for the pod: no existing node accepts it (existingnode.go:87-90)
      if (existing) for (u32 i = GC(u32, P.cls_vol_off)[c]; i < GC(u32, P.cls_vol_off)[c + 1]; ++i) if (GC(u32, P.vol_list)[i] == 0xFFFFFFFFu) { f |= KS_AUDIT_POD_VOLUME_ERROR; break; }
    }
    V.pod_flags[p] = f;
  }
}
__global__ __launch_bounds__(256) void ks_audit_nodes(const DevProb* probs, const AuditView* views) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, E = P.E, NS = E + aud_n_new(P, V), R = P.R, T = P.T, TW = P.TW;
  for (u32 s = blockIdx.x * 4u + (threadIdx.x >> 6); s < NS; s += gridDim.x * 4u) {      // (s, and everything read through it, is the same in all 64 lanes)
    const u32 b = V.off[s], e = V.off[s + 1]; const bool existing = s < E; const u32 j = s - E;
    u32 f = 0;
    if (e == b) {      // nothing placed here: an existing node is as the problem gave it (nothing of it was ever tested), a new node without a pod is not a node
      if (!existing) f = KS_AUDIT_NODE_EMPTY;
      if (lane == 0) V.node_flags[s] = f;
      continue;
    }
    // ---- the pods' requests, summed (int64, wrapping like the kernels' own additions: the order does not matter) ----
    i64 sum[KS_MAX_RES]; u32 pres = 0; u64 dmask = 0; bool ports = false;
#pragma unroll
    for (int r = 0; r < KS_MAX_RES; ++r) sum[r] = 0;
    for (u32 i = b + lane; i < e; i += 64u) {
      const u32 c = aud_class(P, V, V.pods[i]);
      pres |= GC(u32, P.cls_requests_present)[c];
#pragma unroll
      for (int r = 0; r < KS_MAX_RES; ++r) if ((u32)r < R) sum[r] = (i64)((u64)sum[r] + (u64)GC(i64, P.cls_requests)[(size_t)c * R + r]);
      if (GC(u32, P.cls_port_off)[c + 1] != GC(u32, P.cls_port_off)[c]) ports = true;
      if (existing && P.ND) for (u32 v = GC(u32, P.cls_vol_off)[c]; v < GC(u32, P.cls_vol_off)[c + 1]; ++v) { const u32 ent = GC(u32, P.vol_list)[v]; if (ent != 0xFFFFFFFFu) dmask |= 1ull << ((ent >> 24) & 63u); }
    }
#pragma unroll
    for (int r = 0; r < KS_MAX_RES; ++r) if ((u32)r < R) sum[r] = (i64)aud_wave_add((u64)sum[r]);
    pres = (u32)aud_wave_or(pres); dmask = aud_wave_or(dmask);
    const bool any_ports = __ballot(ports) != 0;
    // ---- host ports (hostportusage.go:81-93): every entry of a pod against the node's reservations and against every other pod's entries ----
    if (any_ports) for (u32 i = b + lane; i < e; i += 64u) {
      const u32 p = V.pods[i], c = aud_class(P, V, p); bool hit = false;
      for (u32 x = GC(u32, P.cls_port_off)[c]; x < GC(u32, P.cls_port_off)[c + 1] && !hit; ++x) {
        const u64 a = GC(u64, P.ports)[x];
        if (existing) for (u32 y = GC(u32, P.en_port_off)[s]; y < GC(u32, P.en_port_off)[s + 1]; ++y) if (aud_port_match(a, GC(u64, P.ports)[y])) { hit = true; break; }
        for (u32 i2 = b; i2 < e && !hit; ++i2) {
          if (i2 == i) continue;
          const u32 c2 = aud_class(P, V, V.pods[i2]);
          for (u32 y = GC(u32, P.cls_port_off)[c2]; y < GC(u32, P.cls_port_off)[c2 + 1]; ++y) if (aud_port_match(a, GC(u64, P.ports)[y])) { hit = true; break; }
        }
      }
      if (hit) V.pod_flags[p] |= KS_AUDIT_POD_PORTS;
    }
    if (existing) {
      // ---- resources.Fits(requests + the pods', Available()) under its presence rule: only a resource in the merged list is compared (existingnode.go:98-102) ----
      const u32 rp = GC(u32, P.en_requests_present)[s] | pres; bool over = false;
#pragma unroll
      for (int r = 0; r < KS_MAX_RES; ++r) if ((u32)r < R && ((rp >> r) & 1u)) { if ((i64)((u64)GC(i64, P.en_requests)[(size_t)s * R + r] + (u64)sum[r]) > GC(i64, P.en_avail)[(size_t)s * R + r]) over = true; }
      if (over) f |= KS_AUDIT_NODE_RESOURCES;
      // ---- volume limits (volumeusage.go:102-143): per driver some pod here mounts, the node's claims + the distinct claims the pods add, against the limit ----
      for (u64 dm = dmask; dm; dm &= dm - 1) {
        const u32 d = (u32)__builtin_ctzll(dm); u64 run = 0;
        for (u32 i = b + lane; i < e; i += 64u) {
          const u32 c = aud_class(P, V, V.pods[i]);
          for (u32 v = GC(u32, P.cls_vol_off)[c]; v < GC(u32, P.cls_vol_off)[c + 1]; ++v) { const u32 ent = GC(u32, P.vol_list)[v]; if (ent != 0xFFFFFFFFu && (ent >> 31) && ((ent >> 24) & 63u) == d) run += ent & 0xFFFFFFu; }
        }
        run = aud_wave_add(run);
        for (u32 w = 0; w < P.SW; ++w) {
          u64 bits = 0;
          for (u32 i = b + lane; i < e; i += 64u) {
            const u32 c = aud_class(P, V, V.pods[i]);
            for (u32 v = GC(u32, P.cls_vol_off)[c]; v < GC(u32, P.cls_vol_off)[c + 1]; ++v) { const u32 ent = GC(u32, P.vol_list)[v]; if (!(ent >> 31) && ((ent >> 24) & 63u) == d && ((ent & 0xFFFFFFu) >> 6) == w) bits |= 1ull << (ent & 63u); }
          }
          bits = aud_wave_or(bits) & ~GC(u64, P.en_vol_set)[(size_t)s * P.SW + w];
          run += (u64)__builtin_popcountll(bits);
        }
        if ((i64)GC(i32, P.en_vol_count)[(size_t)s * P.ND + d] + (i64)run > (i64)GC(i32, P.en_vol_limit)[(size_t)s * P.ND + d]) f |= KS_AUDIT_NODE_VOLUMES;
      }
      if (lane == 0) V.node_flags[s] = f;
      continue;
    }
    // ---- a new node ----
    const i32 m = GC(i32, V.n_tmpl)[j];
    if (m < 0 || (u32)m >= P.M) { if (lane == 0) V.node_flags[s] = KS_AUDIT_NODE_TEMPLATE; continue; }
    // Requests = the template's daemon overhead merged with the pods' (node.go:100-104), to the milli-unit
    const u32 rmask = GC(u32, V.o_reqmask)[j]; bool req_bad = rmask != (GC(u32, P.tmpl_daemon_present)[m] | pres);
#pragma unroll
    for (int r = 0; r < KS_MAX_RES; ++r) if ((u32)r < R) { if (GC(i64, V.o_req)[(size_t)j * R + r] != (i64)((u64)GC(i64, P.tmpl_daemon)[(size_t)m * R + r] + (u64)sum[r])) req_bad = true; }
    if (req_bad) f |= KS_AUDIT_NODE_REQUESTS;
    // InstanceTypeOptions against filterInstanceTypesByRequirements (node.go:137-159) by the node's final requirements and requests: one type per lane
    AudNode fn = aud_node_final(P, V, j); const i32 its = fn.it; const bool its_ok = its >= 0 && (u32)its < P.S;
    aud_node_pairs(P, fn);
    u64 extra = 0, missing = 0, any = 0;
    for (u32 w = 0; w < TW; ++w) {
      const u32 t = w * 64u + lane; bool ok = t < T && its_ok;
      if (ok) ok = ((GC(u64, P.tmpl_types)[(size_t)m * TW + w] >> lane) & 1ull) && ((GC(u64, P.its_types)[(size_t)its * TW + w] >> lane) & 1ull) && aud_node_type_ok(P, fn, t);
      const u64 pass = __ballot(ok), have = GC(u64, V.n_types)[(size_t)j * TW + w];
      extra |= have & ~pass; missing |= pass & ~have; any |= have;
    }
    if (!any) f |= KS_AUDIT_NODE_OPTIONS_EMPTY;
    if (extra) f |= KS_AUDIT_NODE_OPTIONS_EXTRA;
    if (missing && GC(u32, P.tmpl_limit_present)[m] == 0xFFFFFFFFu) f |= KS_AUDIT_NODE_OPTIONS_MISSING;      // (a limited template starts from an order-dependent subset, scheduler.go:199-208)
    if (lane == 0) V.node_flags[s] = f;
  }
}

#include "ks_audit_reduce.inc"      // the gate's kernels over the passes' flag tables: after aud_block_sum and ks_audit_scan, which they build on, and before the host half, whose tail launches them

// ---- host half ----
// The host path of all five passes.  A pass's own file keeps what is its own -- its view struct, the carve-up of its scratch, its launch list, the decoding of its
// meta and checked words -- and calls the plain functions below for the rest: the claimed upload, the resident prelude, the pooled work block, the launch rows, the
// wait and the two times, the flag tallies, the walk in slices, and the tail behind the launches -- the read-back and the host's counts for a pass's own entry points, the
// reduction on the device for the gate (ksolve.h ks_audit_gate_dev), whose entry points close this file.
// what the audit reads of a result: KS_RESULT_SEGS without the per-pod reasons.  Each entry has a bit (its place here); a pass names the set it reads as a mask
#define KS_AUDIT_SEGS(X) \
  X(pod_node, pod_node, i32, P) X(pod_stage, pod_stage, i32, P) X(pod_seq, pod_seq, i32, P) X(unscheduled, unscheduled, i32, P) \
  X(n_tmpl, node_tmpl, i32, N) X(n_alive, node_types, u64, N * TW) X(o_req, node_requests, i64, N * R) X(o_reqmask, node_requests_present, u32, N) \
  X(o_present, node_present, u32, N) X(o_complement, node_complement, u32, N) X(o_mask, node_mask, u64, N * K) X(o_gt, node_gt, i32, N * K) X(o_lt, node_lt, i32, N * K) \
  X(o_it, node_it_state, i32, N)
enum {
#define X(sf, rf, T, cnt) AUD_SEG_##rf,
  KS_AUDIT_SEGS(X)
#undef X
  AUD_N_SEGS
};
#define AUD_READS(rf) (1u << AUD_SEG_##rf)
static const u32 AUD_READS_ALL = (1u << AUD_N_SEGS) - 1u;                    // the first pass
static const u32 AUD_READS_ORDER = AUD_READS(pod_node) | AUD_READS(pod_stage) | AUD_READS(pod_seq) | AUD_READS(node_tmpl) | AUD_READS(node_present) | AUD_READS(node_complement) |
                                   AUD_READS(node_mask) | AUD_READS(node_gt) | AUD_READS(node_lt);      // topology and spread: where the pods are, at which stage, in which order; the new nodes' templates and final requirements
static const u32 AUD_READS_FIT = AUD_READS_ALL & ~AUD_READS(unscheduled);   // first-fit, limits, hostfit and stages
static const u32 AUD_READS_REASONS = AUD_READS(pod_node) | AUD_READS(pod_stage);      // the eighth pass: where the pods are and at which stage -- and pod_reason, a side array (below), no member of KS_AUDIT_SEGS
// a later pass's view of the result: the first pass's own outputs and scratch blanked, meta pointed at the pass's block
static AuditView audit_pass_view(const AuditView& result, u32* meta) {
  AuditView v = result;
  v.meta = meta; v.mark = nullptr; v.pod_flags = nullptr; v.node_flags = nullptr; v.cnt = nullptr; v.off = nullptr; v.fill = nullptr; v.pods = nullptr;
  return v;
}
// the result a solve left on the device
static AuditView audit_resident(const DevState& s) {
  AuditView v{};
  v.pod_node = s.pod_node; v.pod_stage = s.pod_stage; v.pod_seq = s.pod_seq; v.unscheduled = s.unscheduled; v.counts = s.out_counts;
  v.n_tmpl = s.n_tmpl; v.n_types = s.n_alive; v.o_req = s.o_req; v.o_reqmask = s.o_reqmask; v.o_present = s.o_present; v.o_complement = s.o_complement;
  v.o_mask = s.o_mask; v.o_gt = s.o_gt; v.o_lt = s.o_lt; v.o_it = s.o_it;
  return v;
}
// A claimed result for the one call: every refusal about it -- an array is refused only if the pass reads it --, then the arrays of `reads` in one block of `up`,
// every piece 8-byte aligned, then the two counts: one transfer.  An array the pass does not read stays null in the view.
static int audit_claimed_check(const ks_dev_problem* d, const ks_result* claimed, u32 reads) {
  if (d->view) return fail(KS_ERR_UNSUPPORTED, "a claimed result is audited against a flattened problem, not against a what-if derived on the device");
  const DevProb& h = d->h; const u64 P = h.P, K = h.K, R = h.R, TW = h.TW, N = claimed->n_new;
  if (N > h.NMAX) return fail(KS_ERR_INVALID, "claimed result: more new nodes than max_new_nodes");
  if (claimed->n_unscheduled > P) return fail(KS_ERR_INVALID, "claimed result: more unscheduled pods than pods");
#define X(sf, rf, T, cnt) if ((reads & AUD_READS(rf)) && (cnt) && !claimed->rf) return fail(KS_ERR_INVALID, "claimed result: null array " #rf);
  KS_AUDIT_SEGS(X)
#undef X
  return KS_OK;
}
// A SIDE array: [P] words of four bytes that travel behind the counts in the same transfer and are no member of KS_AUDIT_SEGS -- the commit numbers the gate's first
// pass reads in pod_seq's place, the pod_reason column the eighth pass audits.  src: the caller's array, or null: not carried; dev: its place on the device after
// the upload (null where it is not carried).  Each user makes a view of its own from `dev`; the block's views are untouched by a side array.
struct AuditSide { const void* src; const void* dev; };
static int audit_claimed_upload(ks_dev_problem* d, const ks_result* claimed, u32 reads, TmpDev& up, AuditView* view, AuditSide* sides = nullptr, u32 n_sides = 0) {
  const DevProb& h = d->h; const u64 P = h.P, K = h.K, R = h.R, TW = h.TW, N = claimed->n_new;
  size_t bytes = 0;
#define X(sf, rf, T, cnt) if (reads & AUD_READS(rf)) bytes += ks_pad8((cnt) * sizeof(T));
  KS_AUDIT_SEGS(X)
#undef X
  size_t all = bytes + 8;
  for (u32 k = 0; k < n_sides; ++k) if (sides[k].src) all += ks_pad8(P * sizeof(u32));
  std::vector<u64> blob(all / 8 + 1, 0); u8* hb = (u8*)blob.data();
  HIPCHK(hipSetDevice(d->device));
  TRY(up.alloc(all)); u8* db = up.as<u8>();
  DevState s{}; size_t at = 0;
#define X(sf, rf, T, cnt) if (reads & AUD_READS(rf)) { const size_t b_ = (cnt) * sizeof(T); if (b_) memcpy(hb + at, claimed->rf, b_); s.sf = (T*)(db + at); at += ks_pad8(b_); }
  KS_AUDIT_SEGS(X)
#undef X
  { u32 c2[2] = {claimed->n_new, claimed->n_unscheduled}; memcpy(hb + at, c2, 8); s.out_counts = (u32*)(db + at); at += 8; }
  for (u32 k = 0; k < n_sides; ++k) {
    sides[k].dev = nullptr;
    if (!sides[k].src) continue;
    if (P) memcpy(hb + at, sides[k].src, P * sizeof(u32));
    sides[k].dev = db + at; at += ks_pad8(P * sizeof(u32));
  }
  HIPCHK(hipMemcpy(db, hb, all, hipMemcpyHostToDevice));
  *view = audit_resident(s);
  return KS_OK;
}
static int audit_claimed(ks_dev_problem* d, const ks_result* claimed, u32 reads, TmpDev& up, AuditView* view) {
  TRY(audit_claimed_check(d, claimed, reads));
  return audit_claimed_upload(d, claimed, reads, up, view);
}
// The resident form of a pass over a batch: its refusals, then `run` over the results the solves left on the device.  own_device_check: the pass refuses a batch
// that spans devices here, before a problem that holds no result (the first pass leaves that refusal to BatchStage::open, after them all)
struct AuditGate;      // the gate's side of a pass's run (below): null for the pass's own entry points
// the refusals of the resident form, in the pass's order, and the views of the results (outs: null from the gate, whose tables are arrays it has looked at itself)
template <class Out> static int audit_resident_check(ks_dev_problem* const* ds, u32 n, Out* const* outs, bool own_device_check, AuditView* res) {
  TRY(BatchStage::not_null(ds, n));
  for (u32 i = 0; i < n; ++i) {
    if (outs && !outs[i]) return fail(KS_ERR_INVALID, "null audit table");
    if (own_device_check && ds[i]->device != ds[0]->device) return fail(KS_ERR_INVALID, "batch spans devices");
    if (!ds[i]->solved) return fail(KS_ERR_INVALID, "audit of a problem that holds no result: solve it first (or the last solve failed)");
    res[i] = audit_resident(ds[i]->hs);
  }
  return KS_OK;
}
template <class Out> static int audit_batch(ks_dev_problem* const* ds, u32 n, Out* const* outs, bool own_device_check, int (*run)(ks_dev_problem* const*, u32, const AuditView*, Out* const*, AuditGate*)) {
  if (!n) return KS_OK;
  if (!ds || !outs) return fail(KS_ERR_INVALID, "null argument");
  std::vector<AuditView> res(n);
  TRY(audit_resident_check(ds, n, outs, own_device_check, res.data()));
  return run(ds, n, res.data(), outs, nullptr);
}
// One problem: the result its solve left (claimed == NULL), or the caller's arrays, of which the pass reads `reads`
template <class Out> static int audit_one(ks_dev_problem* d, const ks_result* claimed, Out* out, u32 reads, bool own_device_check, int (*run)(ks_dev_problem* const*, u32, const AuditView*, Out* const*, AuditGate*)) {
  if (!d || !out) return fail(KS_ERR_INVALID, "null argument");
  if (!claimed) return audit_batch(&d, 1u, &out, own_device_check, run);
  TmpDev up(d->device); AuditView v{};
  TRY(audit_claimed(d, claimed, reads, up, &v));
  return run(&d, 1, &v, &out, nullptr);
}
// The pooled block of u32 a pass works in: [the words that are read back: meta, flag rows, checked rows | scratch], zeroed on the stream before the first launch.
// The output words are reserved first; a pass carves each problem's scratch up itself, from the offset it gets here.
struct AuditWork {
  TmpDev dev; size_t words = 0, n_out = 0; std::vector<u32> back;
  explicit AuditWork(int device) : dev(device) {}
  size_t out(size_t n) { const size_t at = words; words += n; n_out = words; return at; }
  size_t scratch(size_t n, bool align8 = false) { if (align8) words += words & 1; const size_t at = words; words += n; return at; }      // (align8: int64 tables come first in it)
  int alloc() { return dev.alloc(words * sizeof(u32)); }
  u32* w() const { return dev.as<u32>(); }
  int zero(hipStream_t stream) { HIPCHK(hipMemsetAsync(w(), 0, words * sizeof(u32), stream)); return KS_OK; }
  int read_back() { back.resize(n_out); HIPCHK(hipMemcpy(back.data(), w(), n_out * sizeof(u32), hipMemcpyDeviceToHost)); return KS_OK; }      // the output prefix, in one transfer
};
// a pass's launches, once per row of at most KS_GRID_Y_MAX problems: launches(base, ny)
template <class F> static void audit_rows(u32 n, F&& launches) {
  const u32 KS_GRID_Y_MAX = 65535u;
  for (u32 base = 0; base < n; base += KS_GRID_Y_MAX) launches(base, std::min(KS_GRID_Y_MAX, n - base));
}
template <class Out> static void audit_times(Out* const* outs, u32 n, double kernel_ms, double readback_ms) { for (u32 i = 0; i < n; ++i) { outs[i]->kernel_ms = kernel_ms; outs[i]->readback_ms = readback_ms; } }
// The two times of a pass: from before the upload of the views to the end of the last kernel | from there to the end of the host's tallies
struct AuditClock {
  std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now(), t1;
  int wait(hipStream_t stream) { HIPCHK(hipStreamSynchronize(stream)); HIPCHK(hipGetLastError()); t1 = std::chrono::steady_clock::now(); return KS_OK; }
  void add(double* kernel_ms, double* readback_ms) const {
    *kernel_ms += std::chrono::duration<double, std::milli>(t1 - t0).count(); *readback_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t1).count();
  }
  template <class Out> void store(Out* const* outs, u32 n) const { double kms = 0.0, rms = 0.0; add(&kms, &rms); audit_times(outs, n, kms, rms); }
};
// the rows of a flag table that are set, and (bit_count given) how often each bit is; the caller zeroes what it passes
static void audit_tally(const u32* rows, u32 n, u32* n_flagged, u32* bit_count /* [32] or NULL */) {
  for (u32 k = 0; k < n; ++k) if (rows[k]) { ++*n_flagged; if (bit_count) for (u32 x = rows[k]; x; x &= x - 1) ++bit_count[__builtin_ctz(x)]; }
}
// ---- what follows a pass's launches: the TAIL.  A pass says where its tables lie in its work block and which bit fields of a checked word its totals sum
// (AuditTail), and gives a function that writes a problem's out struct from the sums (AuditTotals).  Two tails produce the sums:
//   the pass's own entry points: wait, the output prefix read back, the rows counted on the host, the tables copied to the caller's;
//   the gate's (g given): the reduce kernels of ks_audit_reduce.inc over the same work block on the same stream, then wait and ONE read-back of the totals' block
//   [meta | sums] of every problem; the findings go to the gate's table on the device; no row of a flag table is copied to the host.
struct AuditTail {
  u32 n_meta;                                      // meta words per problem, at the head of the work block: problem i's at n_meta * i
  const size_t* o_pf; const size_t* o_ck; const size_t* o_nf;      // per problem: its pod flags | its checked words, or null | its node flags, or null (offsets in the work block)
  u32 n_fields, shift[4], mask[4];
};
struct AuditTotals {
  const u32* meta; u32 n_pods_flagged, n_nodes_flagged;
  const u32* pod_bits; const u32* node_bits;      // [32] each
  const u32* field;                                // [4]: the sums of the tail's fields over the checked words
};
struct AuditGate {
  ks_audit_finding* d_find; u32 cap;               // the findings' table on the device
  u32 found;                                       // findings so far: the passes before, and this pass's earlier slices
  u32 pass;                                        // a finding's pass
  const void* outs0;                               // the pass's array of out pointers: a slice's position in the batch is its distance from here
  const u32* const* reasons;                       // the eighth pass's column per problem on the device (a claimed result's side array), or null: the resident DevState's
};
// The reduce kernels over `probs` (device pointers inside), queued on `stream`: the totals' blocks come back in `tot` ([KS_AR_TOT] per problem) after the wait, which
// is `clock`'s where there is one.  R: the call's block for the descriptors, the partial sums, the findings' places and the totals.
static int audit_reduce(hipStream_t stream, const std::vector<AuditRedProb>& probs, u32 maxlen, ks_audit_finding* d_find, u32 cap, u32 before, TmpDev& R, AuditClock* clock, std::vector<u32>& tot) {
  const u32 n = (u32)probs.size(), runs = std::min(KS_AR_MAX_RUNS, std::max(1u, (maxlen + 255u) / 256u));
  const size_t nt = (size_t)n * KS_AR_TABS * runs;
  if (nt > 0x7FFFFFFFu / KS_AR_W) return fail(KS_ERR_UNSUPPORTED, "audit gate: the flag tables of the batch are too many runs for one reduction");
  const size_t b_probs = ks_pad8(n * sizeof(AuditRedProb)), w_part = nt * KS_AR_W, w_fbase = nt, w_tot = (size_t)n * KS_AR_TOT;
  TRY(R.alloc(b_probs + (w_part + w_fbase + w_tot) * sizeof(u32)));
  AuditRedView V{}; V.probs = R.as<const AuditRedProb>(); V.part = (u32*)(R.as<u8>() + b_probs); V.fbase = V.part + w_part; V.tot = V.fbase + w_fbase;
  V.find = d_find; V.n = n; V.runs = runs; V.cap = cap; V.before = before;
  HIPCHK(hipMemcpyAsync(R.p, probs.data(), n * sizeof(AuditRedProb), hipMemcpyHostToDevice, stream));
  const bool scatter = cap != 0u && before < cap;      // (a full table takes no more records: the count comes from the totals)
  const u32 KS_GRID_Y_PROBS = 65535u / KS_AR_TABS;
  for (u32 base = 0; base < n; base += KS_GRID_Y_PROBS) hipLaunchKernelGGL(ks_audit_tally, dim3(runs, std::min(KS_GRID_Y_PROBS, n - base) * KS_AR_TABS), dim3(256), 0, stream, V, base);
  hipLaunchKernelGGL(ks_audit_tally_finish, dim3(n), dim3(64), 0, stream, V);
  if (scatter) {
    hipLaunchKernelGGL(ks_audit_find_scan, dim3(1), dim3(256), 0, stream, V);
    for (u32 base = 0; base < n; base += KS_GRID_Y_PROBS) hipLaunchKernelGGL(ks_audit_find_scatter, dim3(runs, std::min(KS_GRID_Y_PROBS, n - base) * KS_AR_TABS), dim3(256), 0, stream, V, base);
  }
  if (clock) TRY(clock->wait(stream)); else { HIPCHK(hipStreamSynchronize(stream)); HIPCHK(hipGetLastError()); }
  tot.resize(w_tot);
  HIPCHK(hipMemcpy(tot.data(), V.tot, w_tot * sizeof(u32), hipMemcpyDeviceToHost));
  return KS_OK;
}
static AuditTotals audit_totals_of(const u32* tot) {      // a totals' block as the finish kernel lays it out
  AuditTotals T{}; T.meta = tot; T.pod_bits = tot + KS_AR_META; T.n_pods_flagged = tot[KS_AR_META + 32u]; T.node_bits = tot + KS_AR_META + 33u; T.n_nodes_flagged = tot[KS_AR_META + 65u]; T.field = tot + KS_AR_META + 66u;
  return T;
}
static int audit_tail_gate(hipStream_t stream, u32* w, AuditClock& clock, ks_dev_problem* const* ds, u32 n, const AuditTail& L, AuditGate& g, u32 position, const std::function<void(u32, const AuditTotals&)>& fill) {
  std::vector<AuditRedProb> probs(n); u32 maxlen = 0;
  for (u32 i = 0; i < n; ++i) {
    AuditRedProb& D = probs[i]; const DevProb& h = ds[i]->h;
    D.meta = w + (size_t)L.n_meta * i; D.n_meta = L.n_meta; D.pod_flags = w + L.o_pf[i]; D.node_flags = L.o_nf ? w + L.o_nf[i] : nullptr; D.chk = L.o_ck ? w + L.o_ck[i] : nullptr;
    D.P = h.P; D.E = h.E; D.NMAX = h.NMAX; D.n_fields = L.n_fields; memcpy(D.shift, L.shift, sizeof D.shift); memcpy(D.mask, L.mask, sizeof D.mask);
    D.problem = position + i; D.where = g.pass << 8;
    maxlen = std::max(maxlen, std::max(h.P, L.o_nf ? h.E + h.NMAX : 0u));
  }
  TmpDev R(ds[0]->device); std::vector<u32> tot;
  TRY(audit_reduce(stream, probs, maxlen, g.d_find, g.cap, g.found, R, &clock, tot));
  for (u32 i = 0; i < n; ++i) { const AuditTotals T = audit_totals_of(tot.data() + (size_t)i * KS_AR_TOT); fill(i, T); g.found += T.n_pods_flagged + T.n_nodes_flagged; }
  return KS_OK;
}
// fill(i, totals, pod flags, node flags): problem i's out struct from its sums; the two rows are the read-back's, for the caller's tables -- null from the gate
template <class Out, class F> static int audit_tail(BatchStage& st, AuditWork& W, AuditClock& clock, ks_dev_problem* const* ds, u32 n, Out* const* outs, const AuditTail& L, AuditGate* g, F&& fill) {
  if (g) return audit_tail_gate(st.stream(), W.w(), clock, ds, n, L, *g, (u32)(outs - (Out* const*)g->outs0), [&](u32 i, const AuditTotals& T) { fill(i, T, (const u32*)nullptr, (const u32*)nullptr); });
  TRY(clock.wait(st.stream()));
  TRY(W.read_back());
  for (u32 i = 0; i < n; ++i) {
    u32 pod_bits[32] = {0}, node_bits[32] = {0}, field[4] = {0, 0, 0, 0};
    AuditTotals T{}; T.meta = W.back.data() + (size_t)L.n_meta * i; T.pod_bits = pod_bits; T.node_bits = node_bits; T.field = field;
    const u32 Pn = ds[i]->h.P, NS = ds[i]->h.E + T.meta[0];
    const u32* pf = W.back.data() + L.o_pf[i]; const u32* nf = L.o_nf ? W.back.data() + L.o_nf[i] : nullptr;
    audit_tally(pf, Pn, &T.n_pods_flagged, pod_bits);
    if (nf) audit_tally(nf, NS, &T.n_nodes_flagged, node_bits);
    if (L.o_ck) { const u32* ck = W.back.data() + L.o_ck[i]; for (u32 k = 0; k < Pn; ++k) for (u32 f = 0; f < L.n_fields; ++f) field[f] += (ck[k] >> L.shift[f]) & L.mask[f]; }
    fill(i, T, pf, nf);
  }
  return KS_OK;
}
// A batch walked in slices for a pass whose scratch per problem can be large: a slice holds problems of at most `budget` words_of(problem) together, or one problem
template <class Out, class W, class S> static int audit_slices(ks_dev_problem* const* ds, u32 n, const AuditView* results, Out* const* outs, AuditGate* g, W&& words_of, size_t budget, S&& slice) {
  double kms = 0.0, rms = 0.0;
  for (u32 base = 0; base < n;) {
    u32 m = 0; size_t words = 0;
    while (base + m < n && (m == 0 || words + words_of(ds[base + m]) <= budget)) { words += words_of(ds[base + m]); ++m; }
    TRY(slice(ds + base, m, results + base, outs + base, g, &kms, &rms));
    base += m;
  }
  audit_times(outs, n, kms, rms);
  return KS_OK;
}

// every refusal about the out tables, then: scratch laid out and zeroed, four launches, then the tail: one read-back of [meta | pod flags | node flags] and the totals counted on the host, or (g given) the gate's reduction on the device
static int audit_run(ks_dev_problem* const* ds, u32 n, const AuditView* results /* the result pointers of every problem */, ks_audit* const* outs, AuditGate* g /* or null: the rows are read back */) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n);
  TRY(st.place());
  // [meta 2n | pod_flags of every problem | node_flags of every problem] (read back) then the scratch
  AuditWork W(ds[0]->device); std::vector<size_t> o_pf(n), o_nf(n), o_scr(n); u32 pmax = 0, nsmax = 0;
  W.out(2 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { o_pf[i] = W.out(ds[i]->h.P); pmax = std::max(pmax, ds[i]->h.P); }
  for (u32 i = 0; i < n; ++i) { o_nf[i] = W.out((size_t)ds[i]->h.E + ds[i]->h.NMAX); nsmax = std::max(nsmax, ds[i]->h.E + ds[i]->h.NMAX); }
  for (u32 i = 0; i < n; ++i) o_scr[i] = W.scratch(2 * (size_t)ds[i]->h.P + 3 * ((size_t)ds[i]->h.E + ds[i]->h.NMAX) + 1);
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditView v = results[i]; const size_t Pn = ds[i]->h.P, NS = (size_t)ds[i]->h.E + ds[i]->h.NMAX;
    v.meta = w + 2 * (size_t)i; v.pod_flags = w + o_pf[i]; v.node_flags = w + o_nf[i];
    u32* s = w + o_scr[i]; v.mark = s; v.cnt = s + Pn; v.off = s + Pn + NS; v.fill = s + Pn + 2 * NS + 1; v.pods = s + Pn + 3 * NS + 1;
    st.h<AuditView>(o_view)[i] = v;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_n = std::max(1u, std::min(4096u, (nsmax + 3u) / 4u));
  audit_rows(n, [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base);
    hipLaunchKernelGGL(ks_audit_scan, dim3(ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base);
    hipLaunchKernelGGL(ks_audit_pods, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base);
    hipLaunchKernelGGL(ks_audit_nodes, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base);
  });
  AuditTail tail{}; tail.n_meta = 2; tail.o_pf = o_pf.data(); tail.o_nf = o_nf.data();
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32* nf) {
    ks_audit* o = outs[i]; const u32* meta = t.meta; const u32 Pn = ds[i]->h.P, NS = ds[i]->h.E + meta[0];
    o->n_pods = Pn; o->n_nodes = NS; o->n_new = meta[0]; o->n_unscheduled = meta[1]; o->n_pods_flagged = t.n_pods_flagged; o->n_nodes_flagged = t.n_nodes_flagged;
    memcpy(o->pod_bit_count, t.pod_bits, sizeof o->pod_bit_count); memcpy(o->node_bit_count, t.node_bits, sizeof o->node_bit_count);
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
    if (nf && o->node_flags && NS) memcpy(o->node_flags, nf, (size_t)NS * sizeof(u32));
  }));
  clock.store(outs, n);
  return KS_OK;
}
extern "C" int ks_audit_sizes(const ks_dev_problem* d, uint32_t* n_pods, uint32_t* n_node_slots) {
  if (!d) return fail(KS_ERR_INVALID, "null argument");
  if (n_pods) *n_pods = d->h.P;
  if (n_node_slots) *n_node_slots = d->h.E + d->h.NMAX;
  return KS_OK;
}
extern "C" int ks_audit_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit* const* outs) { return audit_batch(ds, n, outs, false, audit_run); }
extern "C" int ks_audit_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit* out) { return audit_one(d, claimed, out, AUD_READS_ALL, false, audit_run); }

// ---- the gate (ksolve.h ks_audit_gate_ex_dev / ks_audit_gate_ex_batch_dev, and ks_audit_gate_dev / ks_audit_gate_batch_dev: the same function restricted to the
// six bits and the old struct): the passes a mask names, each through its own run with the gate's tail ----
// What the gate knows of a pass: X(the index of its mask bit, its member of ks_audit_gate_ex, what it reads of a claimed result's block, whether it refuses a batch
// over two devices itself, its run, the side array it reads of a claimed result).  The later passes' runs are defined in the files after this one.
static int audit_topo_run(ks_dev_problem* const*, u32, const AuditView*, ks_audit_topology* const*, AuditGate*);
static int audit_spread_run(ks_dev_problem* const*, u32, const AuditView*, ks_audit_spread* const*, AuditGate*);
static int audit_firstfit_run(ks_dev_problem* const*, u32, const AuditView*, ks_audit_firstfit* const*, AuditGate*);
static int audit_limits_run(ks_dev_problem* const*, u32, const AuditView*, ks_audit_limits* const*, AuditGate*);
static int audit_hostfit_run(ks_dev_problem* const*, u32, const AuditView*, ks_audit_hostfit* const*, AuditGate*);
static int audit_stages_run(ks_dev_problem* const*, u32, const AuditView*, ks_audit_stages* const*, AuditGate*);
static int audit_reasons_run(ks_dev_problem* const*, u32, const AuditView*, ks_audit_reasons* const*, AuditGate*);
enum { AUD_SIDE_NONE = -1, AUD_SIDE_SEQ = 0, AUD_SIDE_REASON = 1, AUD_N_SIDES = 2 };      // SEQ: first_pod_seq, where the caller gives one | REASON: claimed->pod_reason, required
#define KS_AUDIT_GATE_PASSES(X) \
  X(0, first, AUD_READS_ALL, false, audit_run, AUD_SIDE_SEQ) X(1, topology, AUD_READS_ORDER, true, audit_topo_run, AUD_SIDE_NONE) X(2, spread, AUD_READS_ORDER, true, audit_spread_run, AUD_SIDE_NONE) \
  X(3, firstfit, AUD_READS_FIT, true, audit_firstfit_run, AUD_SIDE_NONE) X(4, limits, AUD_READS_FIT, true, audit_limits_run, AUD_SIDE_NONE) X(5, hostfit, AUD_READS_FIT, true, audit_hostfit_run, AUD_SIDE_NONE) \
  X(6, stages, AUD_READS_FIT, true, audit_stages_run, AUD_SIDE_NONE) X(7, reasons, AUD_READS_REASONS, true, audit_reasons_run, AUD_SIDE_REASON)
// the least struct_size: everything ks_audit_gate carries; the passes after the sixth have their pointers behind it
static const u32 KS_AUDIT_GATE_EX_BASE = (u32)offsetof(ks_audit_gate_ex, stages);
// the bits a caller of this struct_size can ask for: within KS_AUDIT_PASS_ALL_EX, the pointer wholly within the struct
static u32 audit_gate_known(u32 struct_size) {
  u32 known = 0;
#define X(k, member, rd, own_check, run, side) if (offsetof(ks_audit_gate_ex, member) + sizeof(void*) <= struct_size) known |= 1u << k;
  KS_AUDIT_GATE_PASSES(X)
#undef X
  return known & KS_AUDIT_PASS_ALL_EX;
}
template <class Out> static int audit_gate_pass(AuditGate& g, u32 pass, ks_dev_problem* const* ds, u32 n, const AuditView* views, Out* outs, int (*run)(ks_dev_problem* const*, u32, const AuditView*, Out* const*, AuditGate*), ks_audit_gate_ex* gate) {
  std::vector<Out*> ptr(n); for (u32 i = 0; i < n; ++i) ptr[i] = outs + i;
  g.pass = pass; g.outs0 = ptr.data();
  TRY(run(ds, n, views, ptr.data(), &g));
  gate->kernel_ms += outs[0].kernel_ms; gate->readback_ms += outs[0].readback_ms;      // (a batch's times are in every member)
  return KS_OK;
}
// one problem with a claimed result (n == 1), or the resident results of n problems
static int audit_gate(ks_dev_problem* const* ds, u32 n, const ks_result* claimed, ks_audit_gate_ex* gate) {
  if (!gate) return fail(KS_ERR_INVALID, "null argument");
  if (gate->struct_size < KS_AUDIT_GATE_EX_BASE) return fail(KS_ERR_INVALID, "audit gate: struct_size is less than the struct's first version");
  if (!gate->passes) return fail(KS_ERR_INVALID, "audit gate: no pass requested");
  if (gate->passes & ~audit_gate_known(gate->struct_size)) return fail(KS_ERR_INVALID, "audit gate: unknown pass");
  if (gate->cap_findings && !gate->findings) return fail(KS_ERR_INVALID, "audit gate: null findings table");
  if (!n) { gate->n_findings = 0; gate->truncated = 0; gate->kernel_ms = gate->readback_ms = 0.0; return KS_OK; }
  // every refusal of every requested pass, in the order of the mask: nothing is launched and no out struct written unless they all accept
  std::vector<AuditView> views(n); AuditView first_view{}; u32 reads = 0;
  AuditSide sides[AUD_N_SIDES] = {{nullptr, nullptr}, {nullptr, nullptr}};
#define X(k, member, rd, own_check, run, side) if (gate->passes & (1u << k)) { \
    if (!ds || !gate->member) return fail(KS_ERR_INVALID, "null argument"); \
    if (claimed) { \
      if (!ds[0]) return fail(KS_ERR_INVALID, "null argument"); \
      TRY(audit_claimed_check(ds[0], claimed, rd)); reads |= rd; \
      if (side == AUD_SIDE_REASON) { if (ds[0]->h.P && !claimed->pod_reason) return fail(KS_ERR_INVALID, "claimed result: null array pod_reason"); sides[AUD_SIDE_REASON].src = claimed->pod_reason; } \
      if (side == AUD_SIDE_SEQ) sides[AUD_SIDE_SEQ].src = gate->first_pod_seq; \
    } else { \
      TRY(audit_resident_check<void>(ds, n, nullptr, own_check, views.data())); \
      if (!own_check) for (u32 i = 0; i < n; ++i) if (ds[i]->device != ds[0]->device) return fail(KS_ERR_INVALID, "batch spans devices"); \
    } }
  KS_AUDIT_GATE_PASSES(X)
#undef X
  const int device = ds[0]->device;
  HIPCHK(hipSetDevice(device));
  TmpDev up(device), F(device);
  if (claimed) TRY(audit_claimed_upload(ds[0], claimed, reads, up, &views[0], sides, AUD_N_SIDES));      // taken once, uploaded once: the union of what the passes read, the side arrays of the passes that have one
  const bool own_seq = sides[AUD_SIDE_SEQ].dev != nullptr;
  if (own_seq) { first_view = views[0]; first_view.pod_seq = (const i32*)sides[AUD_SIDE_SEQ].dev; }      // the first pass's view of its own
  const u32* reason_col = (const u32*)sides[AUD_SIDE_REASON].dev;                                        // the eighth pass's
  if (gate->cap_findings) TRY(F.alloc((size_t)gate->cap_findings * sizeof(ks_audit_finding)));
  AuditGate g{}; g.d_find = gate->cap_findings ? F.as<ks_audit_finding>() : nullptr; g.cap = gate->cap_findings; g.reasons = reason_col ? &reason_col : nullptr;
  gate->n_findings = 0; gate->truncated = 0; gate->kernel_ms = gate->readback_ms = 0.0;
#define X(k, member, rd, own_check, run, side) if (gate->passes & (1u << k)) TRY(audit_gate_pass(g, k, ds, n, (side == AUD_SIDE_SEQ && own_seq) ? &first_view : views.data(), gate->member, run, gate));
  KS_AUDIT_GATE_PASSES(X)
#undef X
  const auto t0 = std::chrono::steady_clock::now();
  gate->n_findings = g.found;
  if (g.found > g.cap) gate->truncated |= KS_AUDIT_GATE_TRUNCATED;
  if (const u32 m = std::min(g.found, g.cap)) HIPCHK(hipMemcpy(gate->findings, g.d_find, (size_t)m * sizeof(ks_audit_finding), hipMemcpyDeviceToHost));      // (the table beyond them is not touched)
  gate->readback_ms += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return KS_OK;
}
// the old struct as the wide one's first version: struct_size ends before `stages`, so the six bits are all it knows; what the gate wrote comes back on success alone
static int audit_gate_six(ks_dev_problem* const* ds, u32 n, const ks_result* claimed, ks_audit_gate* gate) {
  if (!gate) return fail(KS_ERR_INVALID, "null argument");
  ks_audit_gate_ex x{}; x.struct_size = KS_AUDIT_GATE_EX_BASE; x.passes = gate->passes; x.cap_findings = gate->cap_findings; x.findings = gate->findings;
  x.first = gate->first; x.topology = gate->topology; x.spread = gate->spread; x.firstfit = gate->firstfit; x.limits = gate->limits; x.hostfit = gate->hostfit; x.first_pod_seq = gate->first_pod_seq;
  TRY(audit_gate(ds, n, claimed, &x));
  gate->n_findings = x.n_findings; gate->truncated = x.truncated; gate->kernel_ms = x.kernel_ms; gate->readback_ms = x.readback_ms;
  return KS_OK;
}
extern "C" int ks_audit_gate_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_gate* gate) { return audit_gate_six(ds, n, nullptr, gate); }
extern "C" int ks_audit_gate_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_gate* gate) { if (!d) return fail(KS_ERR_INVALID, "null argument"); return audit_gate_six(&d, 1u, claimed, gate); }
extern "C" int ks_audit_gate_ex_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_gate_ex* gate) { return audit_gate(ds, n, nullptr, gate); }
extern "C" int ks_audit_gate_ex_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_gate_ex* gate) { if (!d) return fail(KS_ERR_INVALID, "null argument"); return audit_gate(&d, 1u, claimed, gate); }
extern "C" int ks_audit_reduce_rows(int device, const uint32_t* rows, uint32_t n, const ks_audit_fields* fields, ks_audit_row_totals* out) {
  if (!out || (n && !rows)) return fail(KS_ERR_INVALID, "null argument");
  if (fields && fields->n_fields > 4u) return fail(KS_ERR_INVALID, "audit reduce: more than four fields");
  if (fields) for (u32 f = 0; f < fields->n_fields; ++f) if (fields->shift[f] > 31u) return fail(KS_ERR_INVALID, "audit reduce: a field's shift is a bit of the word");
  int n_dev = 0; HIPCHK(hipGetDeviceCount(&n_dev));
  if (device < 0 || device >= n_dev) return fail(KS_ERR_INVALID, "no such device");
  HIPCHK(hipSetDevice(device));
  TmpDev T(device), R(device);
  TRY(T.alloc(((size_t)n + 2) * sizeof(u32)));
  u32* meta = T.as<u32>();      // [meta 2 | rows]: the one table is the pod flags and the checked words at once
  HIPCHK(hipMemsetAsync(meta, 0, 2 * sizeof(u32), nullptr));
  if (n) HIPCHK(hipMemcpyAsync(meta + 2, rows, (size_t)n * sizeof(u32), hipMemcpyHostToDevice, nullptr));
  std::vector<AuditRedProb> probs(1); AuditRedProb& D = probs[0];
  D = AuditRedProb{}; D.meta = meta; D.n_meta = 2; D.pod_flags = meta + 2; D.chk = meta + 2; D.P = n;
  if (fields) { D.n_fields = fields->n_fields; for (u32 f = 0; f < fields->n_fields; ++f) { D.shift[f] = fields->shift[f]; D.mask[f] = fields->mask[f]; } }
  std::vector<u32> tot;
  TRY(audit_reduce(nullptr, probs, n, nullptr, 0u, 0u, R, nullptr, tot));
  const AuditTotals t = audit_totals_of(tot.data());
  out->n_set = t.n_pods_flagged; memcpy(out->bit_count, t.pod_bits, sizeof out->bit_count); memcpy(out->field_sum, t.field, sizeof out->field_sum);
  return KS_OK;
}
