// ks_audit_hostfit.inc -- the audit's sixth, opt-in pass: FIRST-FIT ORDER for the pods whose constraining groups are all HOSTNAME-keyed anti-affinity or unfiltered
// hostname spread (ksolve.h ks_audit_hostfit_dev / ks_audit_hostfit_batch_dev, KS_AUDIT_POD_HFIT_*).  Included by ksolve.hip after ks_audit_limits.inc, outside the
// emulator's guards: the tests/sim build compiles and runs these kernels too.  The five earlier passes' kernels, views and outputs are untouched; their helpers
// (aud_where, aud_class, aud_n_new, aud_seq_ok, aud_fit_existing_pairs, aud_fit_admits_new, aud_fit_verdict, aud_topo_skipped, aud_topo_unfiltered) are called as they are,
// and two of the fourth pass's kernels -- ks_audit_ff_count and ks_audit_ff_compact, which know nothing of which pods are examined -- are launched as they are, over
// this pass's own AuditFitView.
//
// For such a pod Topology.AddRequirements adds a requirement on the hostname alone, a node's hostname is one value for its whole life, and a group's count on it only
// grows (topologygroup.go:101-105): a node whose FINAL counts admit the pod admitted it at every earlier moment, and the fourth pass's argument carries over clause by
// clause (DESIGN.md 7.27).  fin[n][s] -- the final count of eligible group slot s on node n -- is a dense int32 table [E + n_new][eligible groups], sized on the host at
// [E + max_new_nodes][GH].  Eight launches on the problems' stream, blockIdx.y = the problem:
//   ks_audit_ff_count     the fourth pass's: placed pods, pods per commit number, the existing nodes' request sums and presence masks; the tables set to "never".
//   ks_audit_hf_groups    one workgroup per problem: the eligible groups compacted into slots (the scan tile of ks_audit_ff_compact).
//   ks_audit_hf_mark      one lane per pod: used[c] = 1 for the class of every examined pod; open[j] by atomicMin.
//   ks_audit_ff_compact   the fourth pass's: used[] compacted into the class list.
//   ks_audit_hf_fin       one lane per pod walking its class's sel_list / iown_list: integer atomicAdd into fin; one lane per (existing node, slot): init added in
//                         (an unregistered hostname adds INT32_MIN: the entry stays negative whatever is counted on top, and a negative entry never admits).
//   ks_audit_hf_existing  one lane per (used class, existing node): the fourth pass's body (aud_fit_existing_pairs) with the group clauses -- a load per group -- first.
//   ks_audit_hf_new       one wave per (used class, 64 new nodes or templates): the group clauses a lane per pair -- most pairs end there --, then a wave per pair the
//                         counts admit: the fourth pass's aud_fit_admits_new.
//   ks_audit_hf_verdict   one lane per pod: the fourth pass's aud_fit_verdict with this pass's bits and its own "examinable".
// No float, no LDS beyond the scan tile, no dynamically indexed register array, no atomic on an output.
#define KS_AH_UNREGISTERED 0x80000000u
struct AuditHostView {
  u32* slot; u32* glist;      // scratch: [G] the group's slot + 1, 0: not eligible | [G] the eligible groups by slot
  i32* fin;                   // scratch: [(E + NMAX) * GH] used as [E + n_new][eligible groups]: init + the pods the result puts on the node that record the group
  u32* hcntr;                 // scratch: [2] eligible groups | count tests evaluated
};
// hostname-keyed, not skipped by the second pass's definition, and anti-affinity (inverse groups included) or spread with an empty node filter
__device__ __forceinline__ bool aud_hf_eligible(const DevProb& P, u32 g) {
  if (GC(i32, P.grp_key)[g] != KS_KEY_HOSTNAME || aud_topo_skipped(P, g)) return false;
  const i32 h = GC(i32, P.grp_hslot)[g];
  if (h < 0 || (u32)h >= P.GH) return false;
  const u32 type = GC(u8, P.grp_type)[g];
  return type == 2u || (type == 0u && aud_topo_unfiltered(P, g));
}
// the class reserves no host port, some group constrains it, and every group that does is eligible
__device__ __forceinline__ bool aud_hf_examinable(const DevProb& P, const AuditHostView& H, u32 c) {
  if (GC(u32, P.cls_port_off)[c + 1] != GC(u32, P.cls_port_off)[c]) return false;
  const u32 ob = GC(u32, P.cls_own_off)[c], no = GC(u32, P.cls_own_off)[c + 1] - ob, ib = GC(u32, P.cls_isel_off)[c], ne = no + (GC(u32, P.cls_isel_off)[c + 1] - ib);
  for (u32 i = 0; i < ne; ++i) { const u32 g = (i < no ? GC(u32, P.own_list)[ob + i] : GC(u32, P.isel_list)[ib + (i - no)]) & 0x7FFFFFFFu; if (g >= P.G || !H.slot[g]) return false; }
  return ne != 0u;
}
__device__ __forceinline__ u32 aud_hf_n_groups(const DevProb& P, u32 c) {
  return (GC(u32, P.cls_own_off)[c + 1] - GC(u32, P.cls_own_off)[c]) + (GC(u32, P.cls_isel_off)[c + 1] - GC(u32, P.cls_isel_off)[c]);
}
// ok(c, g, n) for every group that constrains examinable class c; row: the node's row of fin, or null for a fresh node of a template (every count 0).  Every test is
// evaluated: aud_hf_n_groups(c) of them per pair
__device__ __forceinline__ bool aud_hf_groups_ok(const DevProb& P, const AuditHostView& H, u32 c, const i32* row) {
  const u32 ob = GC(u32, P.cls_own_off)[c], no = GC(u32, P.cls_own_off)[c + 1] - ob, ib = GC(u32, P.cls_isel_off)[c], ne = no + (GC(u32, P.cls_isel_off)[c + 1] - ib);
  bool ok = true;
  for (u32 i = 0; i < ne; ++i) {
    const u32 ent = i < no ? GC(u32, P.own_list)[ob + i] : (GC(u32, P.isel_list)[ib + (i - no)] & 0x7FFFFFFFu);
    const u32 g = ent & 0x7FFFFFFFu, self = ent >> 31;
    const i32 v = row ? row[H.slot[g] - 1u] : 0;
    if (GC(u8, P.grp_type)[g] == 2u) ok = ok && v == 0;      // nextDomainAntiAffinity: the domain is registered with count 0
    else ok = ok && v >= 0 && (i64)v + (i64)self <= (i64)GC(i32, P.grp_max_skew)[g];      // nextDomainTopologySpread with the hostname's minimum of 0
  }
  return ok;
}

__global__ __launch_bounds__(256) void ks_audit_hf_groups(const DevProb* probs, const AuditHostView* hviews) {
  __shared__ u32 s_sum[256];
  const DevProb& P = probs[blockIdx.x]; const AuditHostView& H = hviews[blockIdx.x];
  const u32 tid = threadIdx.x, G = P.G, GH = P.GH; u32 carry = 0;
  for (u32 base = 0; base < G; base += 256u) {      // (G is read from one address by every lane: every lane walks every tile and every scan step)
    const u32 i = base + tid; const u32 mine = (i < G && aud_hf_eligible(P, i)) ? 1u : 0u;
    s_sum[tid] = mine;
    for (u32 o = 1; o < 256u; o <<= 1) {
      __syncthreads();
      const u32 x = tid >= o ? s_sum[tid - o] : 0u;
      __syncthreads();
      s_sum[tid] += x;
    }
    __syncthreads();
    if (mine) { const u32 u = carry + s_sum[tid] - 1u; if (u < GH) { H.glist[u] = i; H.slot[i] = u + 1u; } }      // (a row of fin holds GH entries: one hostname row per group, so never more)
    carry += s_sum[255];
    __syncthreads();
  }
  if (tid == 0) H.hcntr[0] = carry < GH ? carry : GH;
}
__global__ __launch_bounds__(256) void ks_audit_hf_mark(const DevProb* probs, const AuditView* views, const AuditFitView* fviews, const AuditHostView* hviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditHostView& H = hviews[blockIdx.y];
  const u32 np = P.P, E = P.E, NS = E + aud_n_new(P, V), n_placed = F.cntr[0];
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    const bool ok = nd >= 0 && aud_seq_ok(V, F.seqcnt, p, n_placed);
    if (!ok && GC(i32, V.pod_node)[p] != -1) continue;      // fails SEQ, or names no node of the result
    if (ok && (u32)nd >= E) atomicMin(&F.open[(u32)nd - E], (u32)GC(i32, V.pod_seq)[p]);
    const u32 c = aud_class(P, V, p);
    if (aud_hf_examinable(P, H, c)) F.used[c] = 1u;      // (every writer stores 1)
  }
}
__global__ __launch_bounds__(256) void ks_audit_hf_fin(const DevProb* probs, const AuditView* views, const AuditHostView* hviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditHostView& H = hviews[blockIdx.y];
  const u32 np = P.P, E = P.E, NS = E + aud_n_new(P, V), GE = H.hcntr[0];
  if (!GE) return;      // (the same in every thread of the launch's row)
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    if (nd < 0) continue;      // (a pod that fails SEQ is counted where the result puts it: a larger count only removes flags)
    const u32 c = aud_class(P, V, p);
    const u32 sb = GC(u32, P.cls_sel_off)[c], ns = GC(u32, P.cls_sel_off)[c + 1] - sb, wb = GC(u32, P.cls_iown_off)[c], nr = ns + (GC(u32, P.cls_iown_off)[c + 1] - wb);
    for (u32 i = 0; i < nr; ++i) {
      const u32 g = i < ns ? GC(u32, P.sel_list)[sb + i] : GC(u32, P.iown_list)[wb + (i - ns)];
      const u32 s = g < P.G ? H.slot[g] : 0u;
      if (s) atomicAdd((u32*)&H.fin[(size_t)(u32)nd * GE + (s - 1u)], 1u);
    }
  }
  const size_t seeds = (size_t)E * GE;
  for (size_t x = (size_t)blockIdx.x * 256u + threadIdx.x; x < seeds; x += (size_t)gridDim.x * 256u) {
    const u32 e = (u32)(x / GE), s = (u32)(x % GE);
    const i32 init = ks_host_count0(P, (u32)GC(i32, P.grp_hslot)[H.glist[s]], e);
    if (init) atomicAdd((u32*)&H.fin[x], init < 0 ? KS_AH_UNREGISTERED : (u32)init);
  }
}
__global__ __launch_bounds__(256) void ks_audit_hf_existing(const DevProb* probs, const AuditFitView* fviews, const AuditHostView* hviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditHostView& H = hviews[blockIdx.y];
  const u32 GE = H.hcntr[0];
  aud_fit_existing_pairs(P, fviews[blockIdx.y], [&](u32 c, u32 e) { return aud_hf_groups_ok(P, H, c, H.fin + (size_t)e * GE); },      // the counts first: a load per group
                         [&](u32 c, u32 nx) { atomicAdd(&H.hcntr[1], nx * aud_hf_n_groups(P, c)); });
}
// (probs is __restrict__ for the reason ks_audit_ff_new gives)
__global__ __launch_bounds__(256) void ks_audit_hf_new(const DevProb* __restrict__ probs, const AuditView* views, const AuditFitView* fviews, const AuditHostView* hviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditHostView& H = hviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, NN = aud_n_new(P, V), M = P.M, X = NN + M, tiles = (X + 63u) / 64u, n_used = F.cntr[1], GE = H.hcntr[0];
  const size_t total = (size_t)n_used * tiles;
  for (size_t w = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += (size_t)gridDim.x * 4u) {      // (w, u, c and x0 are the same in all 64 lanes)
    const u32 u = (u32)(w / tiles), x0 = (u32)(w % tiles) * 64u, c = UF(F.list[u]);      // (c is the same in all 64 lanes, and said so to the compiler: the class's rows are read through scalar registers)
    // ---- the group clauses, a lane per pair: most pairs end here (a node that holds a pod of the group), and a pair that ends here costs a few loads, not a wave ----
    const u32 xl = x0 + lane;
    bool valid = xl < X;
    if (valid) {
      if (xl >= NN) valid = GC(u32, P.tmpl_limit_present)[xl - NN] == 0xFFFFFFFFu;      // a limited template starts from an order-dependent subset (scheduler.go:199-208)
      else { const i32 ml = GC(i32, V.n_tmpl)[xl]; valid = ml >= 0 && (u32)ml < M; }
    }
    const bool gok = valid && aud_hf_groups_ok(P, H, c, xl >= NN ? nullptr : H.fin + (size_t)(P.E + xl) * GE);      // (a fresh node of a template has every count 0)
    const u64 bv = ballot64(valid);
    if (lane == 0 && bv) { const u32 nx = (u32)__builtin_popcountll(bv); atomicAdd(&F.cntr[2], nx); atomicAdd(&H.hcntr[1], nx * aud_hf_n_groups(P, c)); }
    // ---- the pairs the counts admit, a wave per pair: the fourth pass's admits_new ----
    for (u64 todo = ballot64(gok); todo; todo &= todo - 1) {      // (the ballot is the same in all 64 lanes: x, and everything read through it, is too)
      const u32 x = x0 + (u32)__builtin_ctzll(todo);
      const bool fresh = x >= NN;
      const AudNode n = fresh ? aud_node_fresh(P, x - NN) : aud_node_final(P, V, x);
      const bool adm = aud_fit_admits_new(P, n, c, lane);      // (every lane takes the walk's ballots)
      if (lane == 0 && adm) {
        atomicAdd(&F.cntr[3], 1u);
        if (fresh) atomicMin(&F.first_m[u], (u32)n.m);
        else { const u32 o = F.open[x]; if (o != KS_AF_NEVER) atomicMin(&F.first_open[u], o); }
      }
    }
  }
}
__global__ __launch_bounds__(256) void ks_audit_hf_verdict(const DevProb* probs, const AuditView* views, const AuditFitView* fviews, const AuditHostView* hviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditHostView& H = hviews[blockIdx.y];
  if (blockIdx.x == 0 && threadIdx.x == 0) { F.meta[5] = H.hcntr[0]; F.meta[6] = H.hcntr[1]; }
  aud_fit_verdict<KS_AUDIT_POD_HFIT_EXISTING, KS_AUDIT_POD_HFIT_NEW, KS_AUDIT_POD_HFIT_TEMPLATE>(P, views[blockIdx.y], F, [&](u32 c) { return aud_hf_examinable(P, H, c); });
}

// ---- host half ----
// The fourth pass's block [meta | flags | checked words | scratch] with this pass's tables behind it: slot and glist (G words each), two counters, and fin,
// (E + max_new_nodes) x GH words per problem -- max_new_nodes is P in the host's flattening, so a batch is walked in slices (audit_slices) of at most
// KS_AUDIT_HOSTFIT_FIN_WORDS of fin (64 MiB), or one problem.
#define KS_AUDIT_HOSTFIT_FIN_WORDS ((size_t)16 << 20)
static size_t audit_hostfit_fin_words(const ks_dev_problem* d) { return ((size_t)d->h.E + d->h.NMAX) * d->h.GH; }
static int audit_hostfit_slice(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_hostfit* const* outs, AuditGate* g, double* kernel_ms, double* readback_ms) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n), o_fview = st.add<AuditFitView>(n), o_hview = st.add<AuditHostView>(n);
  TRY(st.place());
  AuditWork W(ds[0]->device); std::vector<size_t> o_fl(n), o_ck(n), o_scr(n); u32 pmax = 0; size_t emax = 1, nmax = 1;
  W.out(8 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { o_fl[i] = W.out(ds[i]->h.P); o_ck[i] = W.out(ds[i]->h.P); pmax = std::max(pmax, ds[i]->h.P); }
  for (u32 i = 0; i < n; ++i) {
    const DevProb& h = ds[i]->h;
    o_scr[i] = W.scratch(audit_fit_words(h) + 2 * (size_t)h.G + 2 + audit_hostfit_fin_words(ds[i]), true);
    const size_t used = std::min<size_t>(h.C, h.P);      // (no more classes are used than there are pods)
    emax = std::max(emax, used * (((size_t)h.E + 255) / 256)); nmax = std::max(nmax, (used * (((size_t)h.NMAX + h.M + 63) / 64) + 3) / 4);
  }
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditFitView t{}; AuditHostView x{}; const DevProb& h = ds[i]->h;
    t.meta = w + 8 * (size_t)i; t.flags = w + o_fl[i]; t.chk = w + o_ck[i];
    u32* s = audit_fit_carve(t, h, w + o_scr[i]);
    x.slot = s; s += h.G; x.glist = s; s += h.G; x.hcntr = s; s += 2; x.fin = (i32*)s;
    const AuditView v = audit_pass_view(results[i], t.meta);
    st.h<AuditView>(o_view)[i] = v; st.h<AuditFitView>(o_fview)[i] = t; st.h<AuditHostView>(o_hview)[i] = x;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view); const AuditFitView* df = st.d<const AuditFitView>(o_fview); const AuditHostView* dh = st.d<const AuditHostView>(o_hview);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_e = (u32)std::min<size_t>(4096, emax), gx_n = (u32)std::min<size_t>(4096, nmax);
  audit_rows(n, [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_ff_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
    hipLaunchKernelGGL(ks_audit_hf_groups, dim3(ny), dim3(256), 0, st.stream(), st.probs() + base, dh + base);
    hipLaunchKernelGGL(ks_audit_hf_mark, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dh + base);
    hipLaunchKernelGGL(ks_audit_ff_compact, dim3(ny), dim3(256), 0, st.stream(), st.probs() + base, df + base);
    hipLaunchKernelGGL(ks_audit_hf_fin, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dh + base);
    hipLaunchKernelGGL(ks_audit_hf_existing, dim3(gx_e, ny), dim3(256), 0, st.stream(), st.probs() + base, df + base, dh + base);
    hipLaunchKernelGGL(ks_audit_hf_new, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dh + base);
    hipLaunchKernelGGL(ks_audit_hf_verdict, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dh + base);
  });
  const AuditTail tail{8, o_fl.data(), o_ck.data(), nullptr, 3, {30, 0, 29, 0}, {3u, 1u, 1u, 0u}};      // checked[0], checked[1], skipped_pods of a checked word
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32*) {
    ks_audit_hostfit* o = outs[i]; const u32 Pn = ds[i]->h.P; const u32* meta = t.meta;
    o->n_pods = Pn; o->n_new = meta[0]; o->n_placed = meta[1]; o->eligible_groups = meta[5]; o->skipped_groups = ds[i]->h.G - meta[5]; o->skipped_pods = t.field[2]; o->n_pods_flagged = t.n_pods_flagged;
    o->checked[0] = t.field[0]; o->checked[1] = t.field[1]; o->checked[2] = meta[3]; o->checked[3] = meta[6]; o->admitting_pairs = meta[4];
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
  }));
  clock.add(kernel_ms, readback_ms);
  return KS_OK;
}
static int audit_hostfit_run(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_hostfit* const* outs, AuditGate* g) {
  return audit_slices(ds, n, results, outs, g, audit_hostfit_fin_words, KS_AUDIT_HOSTFIT_FIN_WORDS, audit_hostfit_slice);
}
extern "C" int ks_audit_hostfit_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_hostfit* const* outs) { return audit_batch(ds, n, outs, true, audit_hostfit_run); }
extern "C" int ks_audit_hostfit_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_hostfit* out) { return audit_one(d, claimed, out, AUD_READS_FIT, true, audit_hostfit_run); }
