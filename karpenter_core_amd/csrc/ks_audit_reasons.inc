// ks_audit_reasons.inc -- the audit's eighth, opt-in pass: FAILURE REASONS (ksolve.h ks_audit_reasons_dev / ks_audit_reasons_batch_dev, KS_AUDIT_POD_REASON_*).
// Included by ksolve.hip after ks_audit_stages.inc, outside the emulator's guards: the tests/sim build compiles and runs these kernels too.  The seven earlier passes'
// kernels, views and outputs are untouched; their helpers (aud_where, aud_n_new, aud_n_stages, aud_fit_examinable, aud_fit_cls_req, aud_block_sum; AudNode with its
// state meet and its walk) are called as they are, and the fourth pass's ks_audit_ff_compact is launched as it is over this pass's own AuditFitView (its `used`,
// `list` and `cntr`).
//
// pod_reason carries, per unscheduled pod, the KS_WHY_* step at which the last scheduler.add refused the pod on a FRESH node of every template (four bits each, the
// first eight templates).  A fresh node of a template is static data and Node.Add runs its steps in a fixed order (node.go:62-107), so the step is decided by the
// flat problem alone for every (class, template) pair no topology group speaks about: s(c, m), from ks_algebra.h -- never from mc_ok / mc_why or the feasibility
// grid, which are the pack kernels' own tables (DESIGN.md 7.30 has the argument per clause).  The work is per DISTINCT class of an unscheduled pod.  Four launches on
// the problems' stream with no host wait between them, blockIdx.y = the problem:
//   ks_audit_rs_mark      one lane per pod: its flag word (PLACED) and its checked word; used[c] = 1 for the class of every unscheduled pod whose stage is in range
//                         (every class, not only the examinable ones: steps 1 and 2 are decided for all); the unscheduled pods counted (a block sum, one atomicAdd
//                         into a scratch counter).
//   ks_audit_ff_compact   the fourth pass's: used[] compacted into the class list; cntr[1] = the used classes.
//   ks_audit_rs_static    one wave per (used class, template m < min(M, 8)): this pass's own scalar part -- the EXACT Compatible, answers that are reasons -- is
//                         wave-uniform; then ks_audit.inc's state meet and walk over the types (aud_node_state_meet, aud_node_any_type), one instance type per lane.
//                         Lane 0 stores s into nib[u * 8 + m], a plain store.  With no unscheduled pod the list is empty: no trip.
//   ks_audit_rs_verdict   one lane per pod: the eight nibbles against nib[] by list index; one plain store each for the flag word and the checked word.
// Integer only: no float, no scratch, no dynamically indexed register array, no atomic on an output.
#define KS_AR_S_UNDECIDED 8u      // s(c, m): the class is not examinable -- topology speaks next (one of KS_WHY_TOPOLOGY, _TOPOLOGY_REQS, _NO_INSTANCE_TYPE)
#define KS_AR_S_NO_TYPES 9u       // the template lists no instance type at all: not examined
#define KS_AR_EXACT_SHIFT 1u      // a checked word: bit 0 examined, bits 1-4 the nibbles decided exactly, bits 5-8 the nibbles bounded to a set (0 .. 8 each), bit 30 placed
#define KS_AR_BOUND_SHIFT 5u
struct AuditReasonView {
  const u32* pod_reason;      // [P] the column under audit: the resident DevState's, or the claimed array uploaded beside the block
  u32* nib;                   // scratch: [C * 8] by list index: s(c, m) for m < min(M, 8)
};
// what ks_audit_rs_mark and ks_audit_rs_verdict agree on about pod p: its flag word so far, whether it is placed / unscheduled / examined, and its class
struct AudReasonPod { u32 f, chk, c, w; bool unsched, exam; };
__device__ __forceinline__ AudReasonPod aud_reason_pod(const DevProb& P, const AuditView& V, const AuditReasonView& Q, u32 p, u32 NS) {
  AudReasonPod s;
  const i32 nd = aud_where(P, V, p, NS);
  s.w = GC(u32, Q.pod_reason)[p]; s.unsched = GC(i32, V.pod_node)[p] == -1;
  s.f = (nd >= 0 && s.w) ? KS_AUDIT_POD_REASON_PLACED : 0u; s.chk = nd >= 0 ? 1u << 30 : 0u;
  const u32 gp = P.pod_gid ? GC(u32, P.pod_gid)[p] : p;
  const i32 st = GC(i32, V.pod_stage)[p];
  const bool in_range = st >= 0 && (u32)st < aud_n_stages(P, p);      // (a claimed stage addresses nothing before this test)
  s.c = (s.unsched && in_range) ? GC(u32, P.stage_cls)[GC(u32, P.pod_stage_off)[gp] + (u32)st] : 0xFFFFFFFFu;
  s.exam = s.c < P.C;      // (a class index is checked before it addresses anything)
  if (s.exam) s.chk |= 1u;
  return s;
}
__global__ __launch_bounds__(256) void ks_audit_rs_mark(const DevProb* probs, const AuditView* views, const AuditFitView* fviews, const AuditReasonView* rviews) {
  __shared__ u32 s_sum[256];
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditReasonView& Q = rviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V);
  u32 mine = 0;
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const AudReasonPod s = aud_reason_pod(P, V, Q, p, NS);
    if (s.unsched) ++mine;
    if (s.exam) F.used[s.c] = 1u;      // (every writer stores 1)
    F.flags[p] = s.f; F.chk[p] = s.chk;
  }
  aud_block_sum(s_sum, mine);
  if (threadIdx.x == 0 && s_sum[0]) atomicAdd(&F.cntr[0], s_sum[0]);
}
// s(c, m): what a fresh node of template m answers class c, in Node.Add's order.  Everything read here is the same in all 64 lanes up to the walk over the types.
__device__ __forceinline__ u32 aud_reason_static(const DevProb& P, u32 c, u32 m, u32 lane) {
  const u32 K = P.K, TW = P.TW;
  const u64* ntypes = P.tmpl_types + (size_t)m * TW;
  bool listed = false;
  for (u32 tw = 0; tw < TW; ++tw) if (GC(u64, ntypes)[tw]) listed = true;
  if (!listed) return KS_AR_S_NO_TYPES;
  if (GC(u64, P.tmpl_taints)[m] & ~GC(u64, P.cls_tolerated)[c]) return (u32)KS_WHY_TAINTS;      // Taints.Tolerates, node.go:64
  // (HostPortUsage.Validate, node.go:69: a fresh node has no port in use)
  AudNode n = aud_node_fresh(P, m);
  const u32 cp = GC(u32, P.cls.present)[c];
  bool ok = GC(u8, P.cls_hn_mode)[c] != 1;      // (a new node's placeholder hostname is in no list, node.go:46)
  for (u32 k = 0; k < K && ok; ++k) {      // nodeRequirements.Compatible(podRequirements), node.go:77: exact -- nothing here depends on a moment
    if (!((cp >> k) & 1u)) continue;
    if (kreq_compatible_fail(aud_node_req(P, n, k), aud_fit_cls_req(P, c, k), (P.wellknown_mask >> k) & 1u, P.value_int + k * 64, GC(u32, P.key_nvalues)[k])) ok = false;
  }
  if (!ok || aud_node_state_refuses(P, n, c)) return (u32)KS_WHY_REQUIREMENTS;
  if (!aud_fit_examinable(P, c)) return KS_AR_S_UNDECIDED;      // Topology.AddRequirements speaks next (node.go:83-87)
  const u32 si = aud_node_state_meet(P, n, c);
  if (si >= P.S) return (u32)KS_WHY_NO_INSTANCE_TYPE;            // (the lattice's meet names no state: no type)
  // ---- filterInstanceTypesByRequirements (node.go:137-159) over the template's FULL type set, the merged requirements, daemon overhead + the class's requests ----
  aud_node_add(P, n, c);
  return aud_node_any_type(P, n, si, lane) ? (u32)KS_WHY_NONE : (u32)KS_WHY_NO_INSTANCE_TYPE;
}
__global__ __launch_bounds__(256) void ks_audit_rs_static(const DevProb* probs, const AuditFitView* fviews, const AuditReasonView* rviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditReasonView& Q = rviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, MT = P.M < 8u ? P.M : 8u, n_used = F.cntr[1] < P.C ? F.cntr[1] : P.C;
  const size_t total = (size_t)n_used * MT;
  for (size_t w = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += (size_t)gridDim.x * 4u) {      // (w, and everything read through it, is the same in all 64 lanes)
    const u32 u = (u32)(w / MT), m = (u32)(w % MT), c = F.list[u];
    if (c >= P.C) continue;
    const u32 s = aud_reason_static(P, c, m, lane);
    if (lane == 0) { Q.nib[(size_t)u * 8u + m] = s; atomicAdd(&F.cntr[2], 1u); }
  }
}
__global__ __launch_bounds__(256) void ks_audit_rs_verdict(const DevProb* probs, const AuditView* views, const AuditFitView* fviews, const AuditReasonView* rviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditReasonView& Q = rviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), M = P.M;
  if (blockIdx.x == 0 && threadIdx.x == 0) { F.meta[0] = aud_n_new(P, V); F.meta[1] = F.cntr[0]; F.meta[2] = F.cntr[1]; F.meta[3] = F.cntr[2]; }
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const AudReasonPod s = aud_reason_pod(P, V, Q, p, NS);
    const u32 u1 = s.exam ? F.used[s.c] : 0u;      // (ks_audit_rs_mark marked the class of every examined pod: never 0 for one)
    if (!u1) { F.flags[p] = s.f; F.chk[p] = s.chk; continue; }      // placed, or skipped: the mark kernel's words
    u32 f = s.f, n_exact = 0, n_bound = 0;
#pragma unroll
    for (u32 m = 0; m < 8u; ++m) {
      const u32 nb = (s.w >> (4u * m)) & 15u;
      if (m >= M) { if (nb) f |= KS_AUDIT_POD_REASON_SHAPE; continue; }      // a template the problem does not have
      const u32 sv = Q.nib[(size_t)(u1 - 1u) * 8u + m];
      const bool limited = GC(u32, P.tmpl_limit_present)[m] != 0xFFFFFFFFu;
      bool said = false;      // MISSING or SHAPE has spoken: the nibble is not flagged a second time
      if (nb == (u32)KS_WHY_NONE) { f |= KS_AUDIT_POD_REASON_MISSING; said = true; }
      else if (nb > 7u || nb == (u32)KS_WHY_HOST_PORTS || (nb == (u32)KS_WHY_LIMITS && !limited)) { f |= KS_AUDIT_POD_REASON_SHAPE; said = true; }
      if (sv == KS_AR_S_NO_TYPES || (limited && nb == (u32)KS_WHY_LIMITS)) continue;      // not examined
      if (sv == KS_AR_S_UNDECIDED) {
        ++n_bound;
        if (!said && nb != (u32)KS_WHY_TOPOLOGY && nb != (u32)KS_WHY_TOPOLOGY_REQS && nb != (u32)KS_WHY_NO_INSTANCE_TYPE) f |= KS_AUDIT_POD_REASON_STATIC;
      } else {
        ++n_exact;
        const u32 want = (limited && sv == (u32)KS_WHY_NONE) ? (u32)KS_WHY_NO_INSTANCE_TYPE : sv;      // (a limit only shrinks the type set)
        if (!said && nb != want) f |= KS_AUDIT_POD_REASON_STATIC;
      }
    }
    F.flags[p] = f; F.chk[p] = s.chk | (n_exact << KS_AR_EXACT_SHIFT) | (n_bound << KS_AR_BOUND_SHIFT);
  }
}

// ---- host half ----
// One pooled block [meta | flags | checked words | scratch], one memset, the four launches with no host wait between them, then the common tail.  The scratch of a
// problem is 10 C + 4 words: used, list, nib (8 C) and the counters (unscheduled pods, used classes, pairs).  reasons: per problem the column under audit on the
// device, or null: the resident DevState's.
static int audit_reasons_run_on(ks_dev_problem* const* ds, u32 n, const AuditView* results, const u32* const* reasons, ks_audit_reasons* const* outs, AuditGate* g) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n), o_fview = st.add<AuditFitView>(n), o_rview = st.add<AuditReasonView>(n);
  TRY(st.place());
  AuditWork W(ds[0]->device); std::vector<size_t> o_fl(n), o_ck(n), o_scr(n); u32 pmax = 0; size_t smax = 1;
  W.out(8 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { o_fl[i] = W.out(ds[i]->h.P); o_ck[i] = W.out(ds[i]->h.P); pmax = std::max(pmax, ds[i]->h.P); }
  for (u32 i = 0; i < n; ++i) {
    const DevProb& h = ds[i]->h;
    o_scr[i] = W.scratch(10 * (size_t)h.C + 4);
    const size_t used = std::min<size_t>(h.C, h.P);      // (no more classes are used than there are pods)
    smax = std::max(smax, (used * std::min(h.M, 8u) + 3) / 4);      // the static kernel's grid is bounded here and read on the device from cntr[1]
  }
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditFitView t{}; AuditReasonView q{}; const DevProb& h = ds[i]->h; const size_t Cn = h.C;
    t.meta = w + 8 * (size_t)i; t.flags = w + o_fl[i]; t.chk = w + o_ck[i];
    u32* s = w + o_scr[i]; t.used = s; s += Cn; t.list = s; s += Cn; q.nib = s; s += 8 * Cn; t.cntr = s;
    q.pod_reason = reasons ? reasons[i] : ds[i]->hs.pod_reason;
    st.h<AuditView>(o_view)[i] = audit_pass_view(results[i], t.meta); st.h<AuditFitView>(o_fview)[i] = t; st.h<AuditReasonView>(o_rview)[i] = q;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view); const AuditFitView* df = st.d<const AuditFitView>(o_fview); const AuditReasonView* dq = st.d<const AuditReasonView>(o_rview);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_s = (u32)std::min<size_t>(4096, smax);
  audit_rows(n, [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_rs_mark, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dq + base);
    hipLaunchKernelGGL(ks_audit_ff_compact, dim3(ny), dim3(256), 0, st.stream(), st.probs() + base, df + base);
    hipLaunchKernelGGL(ks_audit_rs_static, dim3(gx_s, ny), dim3(256), 0, st.stream(), st.probs() + base, df + base, dq + base);
    hipLaunchKernelGGL(ks_audit_rs_verdict, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dq + base);
  });
  const AuditTail tail{8, o_fl.data(), o_ck.data(), nullptr, 4, {30, 0, KS_AR_EXACT_SHIFT, KS_AR_BOUND_SHIFT}, {1u, 1u, 15u, 15u}};      // n_placed, checked[0], checked[1], checked[2] of a checked word
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32*) {
    ks_audit_reasons* o = outs[i]; const u32 Pn = ds[i]->h.P, MT = std::min(ds[i]->h.M, 8u); const u32* m = t.meta;
    o->n_pods = Pn; o->n_new = m[0]; o->n_placed = t.field[0]; o->n_unscheduled = m[1]; o->skipped_pods = Pn - t.field[0] - t.field[1]; o->n_pods_flagged = t.n_pods_flagged;
    o->checked[0] = t.field[1]; o->checked[1] = t.field[2]; o->checked[2] = t.field[3]; o->checked[3] = MT * t.field[1] - t.field[2] - t.field[3];      // (every nibble at m < MT of an examined pod is one of the three)
    o->used_classes = m[2]; o->pairs = m[3];
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
  }));
  clock.store(outs, n);
  return KS_OK;
}
// the run function in the form every pass has: the resident column of every problem, or (from the gate's claimed form) the column the gate uploaded beside the block
static int audit_reasons_run(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_reasons* const* outs, AuditGate* g) { return audit_reasons_run_on(ds, n, results, g ? g->reasons : nullptr, outs, g); }
// What the claimed form reads: AUD_READS_REASONS (ks_audit.inc) -- and pod_reason, which is no member of KS_AUDIT_SEGS (AUD_READS_ALL stays the seven passes' set): it
// is uploaded beside the block as a side array, as the gate's second array of commit numbers is.
extern "C" int ks_audit_reasons_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_reasons* const* outs) { return audit_batch(ds, n, outs, true, audit_reasons_run); }
extern "C" int ks_audit_reasons_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_reasons* out) {
  if (!d || !out) return fail(KS_ERR_INVALID, "null argument");
  if (!claimed) return audit_batch(&d, 1u, &out, true, audit_reasons_run);
  TRY(audit_claimed_check(d, claimed, AUD_READS_REASONS));
  if (d->h.P && !claimed->pod_reason) return fail(KS_ERR_INVALID, "claimed result: null array pod_reason");
  TmpDev up(d->device); AuditView v{}; AuditSide side{claimed->pod_reason, nullptr};      // (null only where P == 0: nothing is carried, nothing is read)
  TRY(audit_claimed_upload(d, claimed, AUD_READS_REASONS, up, &v, &side, 1));
  const u32* reasons = (const u32*)side.dev;
  return audit_reasons_run_on(&d, 1, &v, &reasons, &out, nullptr);
}
