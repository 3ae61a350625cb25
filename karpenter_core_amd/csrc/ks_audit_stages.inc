// ks_audit_stages.inc -- the audit's seventh, opt-in pass: RELAXATION ORDER (ksolve.h ks_audit_stages_dev / ks_audit_stages_batch_dev, KS_AUDIT_POD_STAGE_*).
// Included by ksolve.hip after ks_audit_hostfit.inc, outside the emulator's guards: the tests/sim build compiles and runs these kernels too.  The six earlier passes'
// kernels, views and outputs are untouched; their helpers (aud_where, aud_n_new, aud_n_stages, aud_seq_ok, aud_fit_examinable) are called as they are, and four of the
// fourth pass's kernels are launched as they are over this pass's own AuditFitView: ks_audit_ff_count, ks_audit_ff_compact, ks_audit_ff_existing, and ks_audit_ff_new
// over a second AuditView whose `counts` point at two zero words -- it then sees no new node, its grid is the (used class, template) pairs, and its source is untouched.
//
// Solve relaxes a pod one step per failed add (scheduler.go:118-127): a pod that ended at stage k was tried and refused at every stage j < k, each try at some moment
// before the end.  An existing node was there at every such moment and only filled up; a fresh node of a template without limits is static data.  So if the FINAL
// state of an existing node, or a fresh node of such a template, admits the class of stage j, the try at stage j cannot have failed (DESIGN.md 7.29 has the argument
// per clause).  The work is per DISTINCT earlier-stage class in use, not per pod and stage.  Up to six launches on the problems' stream, blockIdx.y = the problem:
//   ks_audit_ff_count     the fourth pass's: placed pods, pods per commit number, the existing nodes' request sums and presence masks; the tables set to "never".
//   ks_audit_st_mark      one lane per pod walking its stages j < k: used[c_j] = 1 for the examinable ones; the pod's flag word (SEQ, UNRELAXED) and its checked word
//                         with the number of stages examined -- what the verdict would say if no pair admitted.  meta[5] = 1 where a class was marked.
//   -- the pass's own entry points read the meta words back here: where no problem of the call marked a class (no pod relaxed), the tables above are the answer and
//      nothing more is launched.  Under the gate (ks_audit_gate_ex) there is no wait: the four below are queued at once and decide per problem (host half) --
//   ks_audit_ff_compact   the fourth pass's: used[] compacted into the class list.
//   ks_audit_ff_existing  the fourth pass's: first_e[u] per used class.
//   ks_audit_ff_new       the fourth pass's, templates only: first_m[u] per used class.
//   ks_audit_st_verdict   one lane per pod walking the same stages: first_e / first_m looked up by list index; its flag word and its checked word, one plain store each.
// The walk's trip count differs from lane to lane -- a chain has at most 64 stages, most pods end at stage 0 -- and stays a plain loop: the lanes of a wave that relaxed
// further keep it for a few more trips of three loads each.  Integer min, add and or; no float, no scratch, no dynamically indexed register array, no atomic on an output.
#define KS_AS_STAGES_SHIFT 1u
#define KS_AS_STAGES_MASK 0x7Fu      // a chain has at most 64 stages: at most 63 of them lie before the one a pod ended at
// what ks_audit_st_mark and ks_audit_st_verdict agree on about pod p: where it is, whether its earlier stages are examined, and its chain
struct AudStagePod { i32 nd; bool ok, unsched, walk; u32 off, k, f, chk; };
__device__ __forceinline__ AudStagePod aud_stage_pod(const DevProb& P, const AuditView& V, const AuditFitView& F, u32 p, u32 NS, u32 n_placed) {
  AudStagePod s;
  s.nd = aud_where(P, V, p, NS);
  s.ok = s.nd >= 0 && aud_seq_ok(V, F.seqcnt, p, n_placed); s.unsched = GC(i32, V.pod_node)[p] == -1;
  const u32 gp = P.pod_gid ? GC(u32, P.pod_gid)[p] : p, n = aud_n_stages(P, p);
  const i32 st = GC(i32, V.pod_stage)[p];
  const bool in_range = st >= 0 && (u32)st < n;      // (a claimed stage addresses nothing before this test)
  s.off = GC(u32, P.pod_stage_off)[gp]; s.k = in_range ? (u32)st : 0u;
  s.f = (s.nd >= 0 && !s.ok) ? KS_AUDIT_POD_SEQ : 0u; s.chk = s.nd >= 0 ? 1u << 30 : 0u;
  if (s.unsched && in_range && (u32)st + 1u != n) s.f |= KS_AUDIT_POD_STAGE_UNRELAXED;      // the queue ends only on pods whose chain is used up (queue.go:44-68)
  s.walk = (s.ok || s.unsched) && in_range;
  return s;
}
__global__ __launch_bounds__(256) void ks_audit_st_mark(const DevProb* probs, const AuditView* views, const AuditFitView* fviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), n_placed = F.cntr[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) { F.meta[0] = aud_n_new(P, V); F.meta[1] = n_placed; }
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const AudStagePod s = aud_stage_pod(P, V, F, p, NS, n_placed);
    u32 n_exam = 0;
    if (s.walk) for (u32 j = 0; j < s.k; ++j) {
      const u32 c = GC(u32, P.stage_cls)[s.off + j];
      if (c < P.C && aud_fit_examinable(P, c)) { F.used[c] = 1u; ++n_exam; }      // (every writer stores 1)
    }
    if (n_exam) F.meta[5] = 1u;      // (every writer stores 1)
    F.flags[p] = s.f; F.chk[p] = s.chk | (n_exam ? 1u | (n_exam << KS_AS_STAGES_SHIFT) : 1u << 29);
  }
}
__global__ __launch_bounds__(256) void ks_audit_st_verdict(const DevProb* probs, const AuditView* views, const AuditFitView* fviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), n_placed = F.cntr[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) { F.meta[2] = F.cntr[1]; F.meta[3] = F.cntr[2]; F.meta[4] = F.cntr[3]; }
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const AudStagePod s = aud_stage_pod(P, V, F, p, NS, n_placed);
    u32 n_exam = 0, f = s.f;
    if (s.walk) for (u32 j = 0; j < s.k; ++j) {
      const u32 c = GC(u32, P.stage_cls)[s.off + j];
      if (!(c < P.C && aud_fit_examinable(P, c))) continue;
      ++n_exam;
      const u32 u1 = F.used[c];      // (ks_audit_st_mark marked the class of every examined stage: never 0 for one)
      if (!u1) continue;
      if (F.first_e[u1 - 1u] != KS_AF_NEVER) f |= KS_AUDIT_POD_STAGE_EXISTING;
      if (F.first_m[u1 - 1u] != KS_AF_NEVER) f |= KS_AUDIT_POD_STAGE_TEMPLATE;
    }
    F.flags[p] = f; F.chk[p] = s.chk | (n_exam ? 1u | (n_exam << KS_AS_STAGES_SHIFT) : 1u << 29);
  }
}

// ---- host half ----
// The fourth pass's block [meta | flags | checked words | scratch] and its scratch, plus two zero words per problem for the view ks_audit_ff_new reads its node count
// from.  After the first two launches the meta words -- the head of the block -- are read back: one small transfer that decides whether the pair kernels run at all
// (the pass's own entry points; the gate's form queues all six).
static int audit_stages_run(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_stages* const* outs, AuditGate* g) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n), o_tview = st.add<AuditView>(n), o_fview = st.add<AuditFitView>(n);
  TRY(st.place());
  AuditWork W(ds[0]->device); std::vector<size_t> o_fl(n), o_ck(n), o_scr(n); u32 pmax = 0; size_t emax = 1, nmax = 1;
  W.out(8 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { o_fl[i] = W.out(ds[i]->h.P); o_ck[i] = W.out(ds[i]->h.P); pmax = std::max(pmax, ds[i]->h.P); }
  for (u32 i = 0; i < n; ++i) {
    const DevProb& h = ds[i]->h;
    o_scr[i] = W.scratch(audit_fit_words(h) + 2, true);
    const size_t used = h.C;      // (a pod marks up to 63 classes: the classes bound the list)
    emax = std::max(emax, used * (((size_t)h.E + 255) / 256)); nmax = std::max(nmax, (used * (size_t)h.M + 3) / 4);
  }
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditFitView t{}; const DevProb& h = ds[i]->h;
    t.meta = w + 8 * (size_t)i; t.flags = w + o_fl[i]; t.chk = w + o_ck[i];
    const u32* s = audit_fit_carve(t, h, w + o_scr[i]);
    const AuditView v = audit_pass_view(results[i], t.meta);
    AuditView tv = v; tv.counts = s;      // (two words the memset zeroed: no new node, no unscheduled list)
    st.h<AuditView>(o_view)[i] = v; st.h<AuditView>(o_tview)[i] = tv; st.h<AuditFitView>(o_fview)[i] = t;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view); const AuditView* dt = st.d<const AuditView>(o_tview); const AuditFitView* df = st.d<const AuditFitView>(o_fview);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_e = (u32)std::min<size_t>(4096, emax), gx_n = (u32)std::min<size_t>(4096, nmax);
  const auto first_two = [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_ff_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
    hipLaunchKernelGGL(ks_audit_st_mark, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
  };
  const auto last_four = [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_ff_compact, dim3(ny), dim3(256), 0, st.stream(), st.probs() + base, df + base);
    hipLaunchKernelGGL(ks_audit_ff_existing, dim3(gx_e, ny), dim3(256), 0, st.stream(), st.probs() + base, df + base);
    hipLaunchKernelGGL(ks_audit_ff_new, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dt + base, df + base);
    hipLaunchKernelGGL(ks_audit_st_verdict, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
  };
  if (g) {
    // Under the gate: all six queued, no host wait between them (the gate's rule: one wait per pass and slice, in the tail).  The decision the read-back below takes
    // per CALL is taken on the device per PROBLEM, by the kernels as they are.  A problem whose meta[5] is 0 marked no class: its used[] is all zero, so
    //   ks_audit_ff_compact   finds `mine` 0 in every tile: it stores nothing to list[] or used[], and cntr[1] = 0 -- what the memset left;
    //   ks_audit_ff_existing  reads n_used = cntr[1] = 0: total = 0, its loop makes no trip, no atomic, no store;
    //   ks_audit_ff_new       the same: total = n_used * X = 0;
    //   ks_audit_st_verdict   walks the stages ks_audit_st_mark walked, through the same aud_stage_pod: no stage is examined (else the mark kernel had set meta[5]),
    //                         n_exam is 0, f is s.f, and the two stores repeat the mark kernel's words; meta[2 .. 4] = cntr[1 .. 3] = 0, what the memset left.
    // So its eight meta words, flag words and checked words are those of the pass's own call -- early-out or not, whatever its neighbours in the batch do -- and it
    // costs four workgroup dispatches that leave at once.  A problem that did mark classes takes exactly the launches its own call gives it.
    audit_rows(n, [&](u32 base, u32 ny) { first_two(base, ny); last_four(base, ny); });
  } else {
    audit_rows(n, first_two);
    std::vector<u32> meta(8 * (size_t)n);
    HIPCHK(hipMemcpyAsync(meta.data(), w, meta.size() * sizeof(u32), hipMemcpyDeviceToHost, st.stream()));
    HIPCHK(hipStreamSynchronize(st.stream()));
    bool relaxed = false;
    for (u32 i = 0; i < n && !relaxed; ++i) relaxed = meta[8 * (size_t)i + 5] != 0u;
    if (relaxed) audit_rows(n, last_four);
  }
  const AuditTail tail{8, o_fl.data(), o_ck.data(), nullptr, 4, {30, 0, 29, KS_AS_STAGES_SHIFT}, {1u, 1u, 1u, KS_AS_STAGES_MASK}};      // checked[0], checked[1], skipped_pods, checked[2] of a checked word
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32*) {
    ks_audit_stages* o = outs[i]; const u32 Pn = ds[i]->h.P; const u32* m = t.meta;
    o->n_pods = Pn; o->n_new = m[0]; o->n_placed = m[1]; o->skipped_pods = t.field[2]; o->n_pods_flagged = t.n_pods_flagged;
    o->checked[0] = t.field[0]; o->checked[1] = t.field[1]; o->checked[2] = t.field[3]; o->checked[3] = m[3]; o->admitting_pairs = m[4];
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
  }));
  clock.store(outs, n);
  return KS_OK;
}
extern "C" int ks_audit_stages_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_stages* const* outs) { return audit_batch(ds, n, outs, true, audit_stages_run); }
extern "C" int ks_audit_stages_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_stages* out) { return audit_one(d, claimed, out, AUD_READS_FIT, true, audit_stages_run); }
