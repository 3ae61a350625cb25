// ks_audit_firstfit.inc -- the audit's fourth, opt-in pass: FIRST-FIT ORDER (ksolve.h ks_audit_firstfit_dev / ks_audit_firstfit_batch_dev, KS_AUDIT_POD_FIT_*).
// Included by ksolve.hip after ks_audit_spread.inc, outside the emulator's guards: the tests/sim build compiles and runs these kernels too.  The first three passes'
// kernels, views and outputs are untouched; their helpers (aud_where, aud_class, aud_n_new, aud_wave_*) are called as they are, ks_algebra.h is as it was.
//
// scheduler.add tries every existing node, then every new node, then every template before it opens a machine (scheduler.go:174-219).  Between the moment a pod was
// tried and the end of the Solve a node's requests only grow, its requirements only narrow, its InstanceTypeOptions only shrink: a node whose FINAL state would take
// pod P on top of everything it holds would have taken P at any earlier moment it existed, so P cannot have ended anywhere later.  One-sided, as passes two and three:
// it flags only what no run of the reference can have produced (DESIGN.md 7.24 has the argument per clause).  The work is per DISTINCT final-stage class used by an
// examined pod -- a derived what-if shares its snapshot's thousands of classes and uses a few hundred.  Six launches on the problems' stream, blockIdx.y = the problem:
//   ks_audit_ff_count     one lane per pod: the placed pods counted, and counted per commit number (the second pass's SEQ rule); the existing nodes' request sums and
//                         presence masks by integer atomicAdd / atomicOr into scratch; open[] and the three first_* tables set to "never".
//   ks_audit_ff_mark      one lane per pod: used[c] = 1 for the class of every examined pod; open[j] = the least commit number on new node j (atomicMin).  Integer
//                         min, add and or: the same tables every run.
//   ks_audit_ff_compact   one workgroup per problem: used[] compacted into the class list (ks_audit_scan's Hillis-Steele tile).
//   ks_audit_ff_existing  one lane per (used class, existing node), a wave shares the class: the test is scalar per pair; a wave minimum, then atomicMin into first_e[u].
//   ks_audit_ff_new       one wave per (used class, new node or unlimited template): aud_fit_admits_new below -- the one-sided clauses, wave-uniform, then ks_audit.inc's
//                         walk over the types (AudNode, aud_node_any_type), one instance type per lane.  atomicMin into first_open[u] / first_m[u].
//   ks_audit_ff_verdict   one lane per pod: its flag word and its checked word, one writer each, a plain store.
// aud_fit_admits_new is THE new-node predicate of the audit: the sixth and the ninth pass call it for their own pairs, the fifth takes its clauses
// (aud_fit_new_clauses), the eighth the state meet and the walk.  The existing-node kernels of the fourth and sixth pass are one body (aud_fit_existing_pairs), their
// verdict kernels another (aud_fit_verdict); the ninth uses the body's predicates (aud_fit_mounts / _live / _labelled).
// No float, no LDS beyond the count kernel's reduction and the scan tile, no dynamically indexed register array, no atomic on an output.
#define KS_AF_NEVER 0xFFFFFFFFu
struct AuditFitView {
  u32* flags; u32* chk; u32* meta;      // outputs: [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_FIT_* | [P] bit 0 examined, bit 29 skipped, bit 30 placed | [8]: n_new, placed pods, used classes, pairs evaluated, pairs that admitted
  u64* esum; u32* epres;                // scratch: [E * R] the requests of the pods the result puts on existing node e | [E] their presence masks
  u32* seqcnt; u32* used; u32* list;    // scratch: [P] placed pods per commit number | [C] the class is used by an examined pod, then its index in the list + 1 | [C] the used classes
  u32* first_e; u32* first_open; u32* first_m; u32* open; u32* cntr;      // scratch: [C] by list index: the least admitting existing node | the least open() over the admitting new nodes | the least admitting unlimited template | [NMAX] the least commit number on new node j | [4] placed pods, used classes, pairs evaluated, pairs that admitted
};
// no topology group constrains the class (Topology.AddRequirements adds nothing) and it reserves no host port
__device__ __forceinline__ bool aud_fit_examinable(const DevProb& P, u32 c) {
  return GC(u32, P.cls_own_off)[c + 1] == GC(u32, P.cls_own_off)[c] && GC(u32, P.cls_isel_off)[c + 1] == GC(u32, P.cls_isel_off)[c] && GC(u32, P.cls_port_off)[c + 1] == GC(u32, P.cls_port_off)[c];
}
// the intersection of two present requirements is EMPTY.  Requirements.Intersects lets an empty intersection pass when both operators are NotIn / DoesNotExist
// (requirements.go:196-200); this pass does not: a final state that passes only through that exception can have failed earlier (a node at Exists refuses the
// DoesNotExist pod that the same node, later narrowed to DoesNotExist, lets through)
__device__ __forceinline__ bool aud_fit_meet_empty(const KReq& a, const KReq& b, const i32* vi, u32 nv) { return a.present && b.present && kreq_len0(kreq_intersect(a, b, vi, nv)); }
// admits_existing(c, e) for a pair that is examined (every key of the class is labelled on e): static facts of the flat problem plus one sum
__device__ __forceinline__ bool aud_fit_existing(const DevProb& P, const AuditFitView& F, u32 c, u32 e) {
  const u32 K = P.K, R = P.R;
  if (GC(u64, P.en_taints)[e] & ~GC(u64, P.cls_tolerated)[c]) return false;
  const u32 hm = GC(u8, P.cls_hn_mode)[c];
  if (hm && (hm == 1) != aud_hn_listed(P, c, e)) return false;
  const u32 cp = GC(u32, P.cls.present)[c], ep = GC(u32, P.en.present)[e], ec = GC(u32, P.en.complement)[e];
  for (u32 k = 0; k < K; ++k) {
    if (!((cp >> k) & 1u)) continue;
    const KReq a = load_req(ep, ec, P.en.mask + (size_t)e * K, P.en.gt + (size_t)e * K, P.en.lt + (size_t)e * K, (int)k);
    if (kreq_compatible_fail(a, aud_fit_cls_req(P, c, k), (P.wellknown_mask >> k) & 1u, P.value_int + k * 64, GC(u32, P.key_nvalues)[k])) return false;
  }
  const i32 sa = GC(i32, P.en.it_state)[e], sb = GC(i32, P.cls.it_state)[c];
  if (P.SC && (sa < 0 || (u32)sa >= P.S || sb < 0 || (u32)sb >= P.SC || GC(u8, P.its_fail)[(size_t)sa * P.SC + sb])) return false;
  // resources.Fits under its presence rule: only a resource in the merged list is compared (existingnode.go:98-102)
  const u32 rp = GC(u32, P.en_requests_present)[e] | F.epres[e] | GC(u32, P.cls_requests_present)[c];
  for (u32 r = 0; r < R; ++r) {
    if (!((rp >> r) & 1u)) continue;
    const u64 need = (u64)GC(i64, P.en_requests)[(size_t)e * R + r] + F.esum[(size_t)e * R + r] + (u64)GC(i64, P.cls_requests)[(size_t)c * R + r];
    if ((i64)need > GC(i64, P.en_avail)[(size_t)e * R + r]) return false;
  }
  return true;
}
// ---- admits_new(c, n): would new node n -- as the result leaves it, or a fresh one of a template (ks_audit.inc's views) -- have taken one more pod of class c? ----
// The clauses that make the test one-sided, the same in all 64 lanes.  n: the node WITHOUT the pod on top
__device__ __forceinline__ bool aud_fit_new_clauses(const DevProb& P, const AudNode& n, u32 c) {
  bool ok = (GC(u64, P.tmpl_taints)[n.m] & ~GC(u64, P.cls_tolerated)[c]) == 0ull && GC(u8, P.cls_hn_mode)[c] != 1;      // (a new node's placeholder hostname is in no list, node.go:46)
  const u32 cp = GC(u32, P.cls.present)[c], tmp = GC(u32, P.tmpl.present)[n.m];
  for (u32 k = 0; k < P.K && ok; ++k) {
    if (!((cp >> k) & 1u)) continue;
    const KReq b = aud_fit_cls_req(P, c, k);
    // "custom labels, if not defined, are denied" looks at the node AT THE TIME (requirements.go:125-130): a later pod may have added the key, the template had it all along
    if (!((P.wellknown_mask >> k) & 1u) && !kreq_nidne(b) && !((tmp >> k) & 1u)) ok = false;
    else if (aud_fit_meet_empty(aud_node_req(P, n, k), b, P.value_int + k * 64, GC(u32, P.key_nvalues)[k])) ok = false;
  }
  return ok;
}
// the clauses, the instance-type state's meet, then filterInstanceTypesByRequirements (node.go:137-159) against the requirements with the class added and the requests
// with the class's: one type per lane.  Wave-uniform up to the walk; every lane returns the same
__device__ __forceinline__ bool aud_fit_admits_new(const DevProb& P, AudNode n, u32 c, u32 lane) {
  const u32 si = aud_fit_new_clauses(P, n, c) ? aud_node_state_meet(P, n, c) : P.S;
  bool adm = false;
  if (si < P.S) { aud_node_add(P, n, c); adm = aud_node_any_type(P, n, si, lane); }
  return adm;
}
// ---- what the existing-node kernels share: the classes and nodes left out, the condition under which a pair is examined, and the tile's body ----
// a class that mounts volumes is examined against new nodes only: they track none
__device__ __forceinline__ bool aud_fit_mounts(const DevProb& P, u32 c) { return GC(u32, P.cls_vol_off)[c + 1] != GC(u32, P.cls_vol_off)[c]; }
__device__ __forceinline__ bool aud_fit_live(const DevProb& P, u32 e) { return e < P.E && !(P.en_removed && ((GC(u64, P.en_removed)[e >> 6] >> (e & 63u)) & 1ull)); }
// every key the class names is labelled on e: there the node's requirement at any time IS the label, and Compatible is exact
__device__ __forceinline__ bool aud_fit_labelled(const DevProb& P, u32 c, u32 e) {
  return (GC(u32, P.cls.present)[c] & ~GC(u32, P.en.present)[e]) == 0u && !(GC(i32, P.cls.it_state)[c] != 0 && GC(i32, P.en.it_state)[e] == 0);
}
// one lane per (used class, existing node), a workgroup shares the class.  more(c, e): what the pass tests before aud_fit_existing; counted(c, n): lane 0 of a wave,
// after n pairs of it were examined
template <class More, class Counted> __device__ __forceinline__ void aud_fit_existing_pairs(const DevProb& P, const AuditFitView& F, More&& more, Counted&& counted) {
  const u32 lane = threadIdx.x & 63u, E = P.E, tiles = (E + 255u) / 256u, n_used = F.cntr[1];
  const size_t total = (size_t)n_used * tiles;
  for (size_t w = blockIdx.x; w < total; w += gridDim.x) {      // (w, u and c are the same in all 256 threads)
    const u32 u = (u32)(w / tiles), e = (u32)(w % tiles) * 256u + threadIdx.x, c = F.list[u];
    if (aud_fit_mounts(P, c)) continue;
    const bool exam = aud_fit_live(P, e) && aud_fit_labelled(P, c, e), adm = exam && more(c, e) && aud_fit_existing(P, F, c, e);
    u32 best = adm ? e : KS_AF_NEVER;
    for (int x = 32; x > 0; x >>= 1) { const u32 o = __shfl_xor(best, x); best = o < best ? o : best; }
    const u64 bx = ballot64(exam), ba = ballot64(adm);
    if (lane == 0) {
      if (best != KS_AF_NEVER) atomicMin(&F.first_e[u], best);
      if (bx) { const u32 nx = (u32)__builtin_popcountll(bx); atomicAdd(&F.cntr[2], nx); counted(c, nx); }
      if (ba) atomicAdd(&F.cntr[3], (u32)__builtin_popcountll(ba));
    }
  }
}
// ---- the verdict of the fourth and the sixth pass: one lane per pod, its flag word and its checked word.  BE, BN, BT: the pass's three bits; examinable(c): its test ----
template <u32 BE, u32 BN, u32 BT, class Examinable> __device__ __forceinline__ void aud_fit_verdict(const DevProb& P, const AuditView& V, const AuditFitView& F, Examinable&& examinable) {
  const u32 np = P.P, E = P.E, NS = E + aud_n_new(P, V), n_placed = F.cntr[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) { F.meta[0] = aud_n_new(P, V); F.meta[1] = n_placed; F.meta[2] = F.cntr[1]; F.meta[3] = F.cntr[2]; F.meta[4] = F.cntr[3]; }
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    const bool ok = nd >= 0 && aud_seq_ok(V, F.seqcnt, p, n_placed), unsched = GC(i32, V.pod_node)[p] == -1;
    u32 f = (nd >= 0 && !ok) ? KS_AUDIT_POD_SEQ : 0u, chk = nd >= 0 ? 1u << 30 : 0u;
    const u32 c = aud_class(P, V, p);
    const u32 u1 = F.used[c];      // (the pass's mark kernel marked the class of every examined pod: never 0 for one)
    if (!(ok || unsched) || !u1 || !examinable(c)) { F.flags[p] = f; F.chk[p] = chk | (1u << 29); continue; }
    const u32 u = u1 - 1u;
    const u32 fe = F.first_e[u], fo = F.first_open[u], fm = F.first_m[u];
    if (unsched) {
      if (fe != KS_AF_NEVER) f |= BE;
      if (fo != KS_AF_NEVER) f |= BN;
      if (fm != KS_AF_NEVER) f |= BT;
    } else if ((u32)nd < E) {
      if (fe < (u32)nd) f |= BE;
    } else {
      const u32 j = (u32)nd - E, sq = (u32)GC(i32, V.pod_seq)[p];
      if (fe != KS_AF_NEVER) f |= BE;
      if (sq == F.open[j]) {      // the opener of its node; a pod that joined a new node later is checked against existing nodes only (the order among new nodes depends on pod counts at the time)
        if (fo < sq) f |= BN;      // (strictly: its own node opened at sq)
        const i32 m = GC(i32, V.n_tmpl)[j];
        if (m >= 0 && (u32)m < P.M && fm < (u32)m) f |= BT;
      }
    }
    F.flags[p] = f; F.chk[p] = chk | 1u;
  }
}

__global__ __launch_bounds__(256) void ks_audit_ff_count(const DevProb* probs, const AuditView* views, const AuditFitView* fviews) {
  __shared__ u32 s_sum[256];
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y];
  const u32 np = P.P, E = P.E, NS = E + aud_n_new(P, V), R = P.R;
  u32 mine = 0;
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < np; i += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, i, NS), sq = GC(i32, V.pod_seq)[i];
    if (nd < 0) continue;
    ++mine;
    if (sq >= 0 && (u32)sq < np) atomicAdd(&F.seqcnt[sq], 1u);
    if ((u32)nd < E) {      // (its node counts the pod whatever else is wrong with it, as the first pass does)
      const u32 c = aud_class(P, V, i), pres = GC(u32, P.cls_requests_present)[c];
      if (pres) atomicOr(&F.epres[nd], pres);
      for (u32 r = 0; r < R; ++r) { const i64 v = GC(i64, P.cls_requests)[(size_t)c * R + r]; if (v) atomicAdd((unsigned long long*)&F.esum[(size_t)nd * R + r], (unsigned long long)v); }
    }
  }
  aud_block_sum(s_sum, mine);
  if (threadIdx.x == 0 && s_sum[0]) atomicAdd(&F.cntr[0], s_sum[0]);
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < P.C; i += gridDim.x * 256u) { F.first_e[i] = KS_AF_NEVER; F.first_open[i] = KS_AF_NEVER; F.first_m[i] = KS_AF_NEVER; }
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < P.NMAX; i += gridDim.x * 256u) F.open[i] = KS_AF_NEVER;
}
__global__ __launch_bounds__(256) void ks_audit_ff_mark(const DevProb* probs, const AuditView* views, const AuditFitView* fviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y];
  const u32 np = P.P, E = P.E, NS = E + aud_n_new(P, V), n_placed = F.cntr[0];
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    const bool ok = nd >= 0 && aud_seq_ok(V, F.seqcnt, p, n_placed);
    if (!ok && GC(i32, V.pod_node)[p] != -1) continue;      // fails SEQ, or names no node of the result
    if (ok && (u32)nd >= E) atomicMin(&F.open[(u32)nd - E], (u32)GC(i32, V.pod_seq)[p]);
    const u32 c = aud_class(P, V, p);
    if (aud_fit_examinable(P, c)) F.used[c] = 1u;      // (every writer stores 1)
  }
}
__global__ __launch_bounds__(256) void ks_audit_ff_compact(const DevProb* probs, const AuditFitView* fviews) {
  __shared__ u32 s_sum[256];
  const DevProb& P = probs[blockIdx.x]; const AuditFitView& F = fviews[blockIdx.x];
  const u32 tid = threadIdx.x, C = P.C; u32 carry = 0;
  for (u32 base = 0; base < C; base += 256u) {      // (C is read from one address by every lane: every lane walks every tile and every scan step)
    const u32 i = base + tid; const u32 mine = i < C ? F.used[i] : 0u;
    s_sum[tid] = mine;
    for (u32 o = 1; o < 256u; o <<= 1) {
      __syncthreads();
      const u32 x = tid >= o ? s_sum[tid - o] : 0u;
      __syncthreads();
      s_sum[tid] += x;
    }
    __syncthreads();
    if (mine) { const u32 u = carry + s_sum[tid] - 1u; F.list[u] = i; F.used[i] = u + 1u; }
    carry += s_sum[255];
    __syncthreads();
  }
  if (tid == 0) F.cntr[1] = carry;
}
__global__ __launch_bounds__(256) void ks_audit_ff_existing(const DevProb* probs, const AuditFitView* fviews) {
  aud_fit_existing_pairs(probs[blockIdx.y], fviews[blockIdx.y], [](u32, u32) { return true; }, [](u32, u32) {});
}
// (probs is __restrict__: no store of this kernel reaches the problem descriptors, and said so their words stay in scalar registers across the atomics of the loop
//  -- without it the walk holds some twenty more vector registers and the kernel drops from seven waves a SIMD to five)
__global__ __launch_bounds__(256) void ks_audit_ff_new(const DevProb* __restrict__ probs, const AuditView* views, const AuditFitView* fviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, NN = aud_n_new(P, V), M = P.M, X = NN + M, n_used = F.cntr[1];
  const size_t total = (size_t)n_used * X;
  for (size_t w = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += (size_t)gridDim.x * 4u) {      // (w, and everything read through it, is the same in all 64 lanes)
    const u32 u = (u32)(w / X), x = (u32)(w % X), c = F.list[u];
    const bool fresh = x >= NN;
    bool adm;
    if (fresh) {
      if (GC(u32, P.tmpl_limit_present)[x - NN] != 0xFFFFFFFFu) continue;      // a limited template starts from an order-dependent subset (scheduler.go:199-208)
      adm = aud_fit_admits_new(P, aud_node_fresh(P, x - NN), c, lane);
    } else {
      const AudNode n = aud_node_final(P, V, x);
      if (n.m < 0 || (u32)n.m >= M) continue;      // a node of no template is the first pass's finding
      adm = aud_fit_admits_new(P, n, c, lane);
    }
    if (lane == 0) {
      atomicAdd(&F.cntr[2], 1u);
      if (adm) {
        atomicAdd(&F.cntr[3], 1u);
        if (fresh) atomicMin(&F.first_m[u], x - NN);
        else { const u32 o = F.open[x]; if (o != KS_AF_NEVER) atomicMin(&F.first_open[u], o); }
      }
    }
  }
}
__global__ __launch_bounds__(256) void ks_audit_ff_verdict(const DevProb* probs, const AuditView* views, const AuditFitView* fviews) {
  const DevProb& P = probs[blockIdx.y];
  aud_fit_verdict<KS_AUDIT_POD_FIT_EXISTING, KS_AUDIT_POD_FIT_NEW, KS_AUDIT_POD_FIT_TEMPLATE>(P, views[blockIdx.y], fviews[blockIdx.y], [&](u32 c) { return aud_fit_examinable(P, c); });
}

// ---- host half ----
// One pooled block [meta | flags | checked words | scratch], one memset, the six launches, one read-back, the totals counted on the host.  The scratch of a problem is
// audit_fit_words: no slicing is needed.  The sixth, seventh and ninth pass carve the same tables out of their own blocks.
static size_t audit_fit_words(const DevProb& h) { return 2 * (size_t)h.E * h.R + h.E + h.P + 5 * (size_t)h.C + h.NMAX + 4; }
// the scratch tables of `t` from s on (8-byte aligned: the int64 sums come first); returns the first word behind them
static u32* audit_fit_carve(AuditFitView& t, const DevProb& h, u32* s) {
  const size_t Cn = h.C;
  t.esum = (u64*)s; s += 2 * (size_t)h.E * h.R; t.epres = s; s += h.E; t.seqcnt = s; s += h.P; t.used = s; s += Cn; t.list = s; s += Cn;
  t.first_e = s; s += Cn; t.first_open = s; s += Cn; t.first_m = s; s += Cn; t.open = s; s += h.NMAX; t.cntr = s; s += 4;
  return s;
}
static int audit_firstfit_run(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_firstfit* const* outs, AuditGate* g) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n), o_fview = st.add<AuditFitView>(n);
  TRY(st.place());
  AuditWork W(ds[0]->device); std::vector<size_t> o_fl(n), o_ck(n), o_scr(n); u32 pmax = 0; size_t emax = 1, nmax = 1;
  W.out(8 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { o_fl[i] = W.out(ds[i]->h.P); o_ck[i] = W.out(ds[i]->h.P); pmax = std::max(pmax, ds[i]->h.P); }
  for (u32 i = 0; i < n; ++i) {
    const DevProb& h = ds[i]->h;
    o_scr[i] = W.scratch(audit_fit_words(h), true);
    const size_t used = std::min<size_t>(h.C, h.P);      // (no more classes are used than there are pods)
    emax = std::max(emax, used * (((size_t)h.E + 255) / 256)); nmax = std::max(nmax, (used * ((size_t)h.NMAX + h.M) + 3) / 4);
  }
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditFitView t{}; const DevProb& h = ds[i]->h;
    t.meta = w + 8 * (size_t)i; t.flags = w + o_fl[i]; t.chk = w + o_ck[i];
    audit_fit_carve(t, h, w + o_scr[i]);
    const AuditView v = audit_pass_view(results[i], t.meta);
    st.h<AuditView>(o_view)[i] = v; st.h<AuditFitView>(o_fview)[i] = t;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view); const AuditFitView* df = st.d<const AuditFitView>(o_fview);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_e = (u32)std::min<size_t>(4096, emax), gx_n = (u32)std::min<size_t>(4096, nmax);
  audit_rows(n, [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_ff_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
    hipLaunchKernelGGL(ks_audit_ff_mark, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
    hipLaunchKernelGGL(ks_audit_ff_compact, dim3(ny), dim3(256), 0, st.stream(), st.probs() + base, df + base);
    hipLaunchKernelGGL(ks_audit_ff_existing, dim3(gx_e, ny), dim3(256), 0, st.stream(), st.probs() + base, df + base);
    hipLaunchKernelGGL(ks_audit_ff_new, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
    hipLaunchKernelGGL(ks_audit_ff_verdict, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
  });
  const AuditTail tail{8, o_fl.data(), o_ck.data(), nullptr, 3, {30, 0, 29, 0}, {3u, 1u, 1u, 0u}};      // checked[0], checked[1], skipped_pods of a checked word
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32*) {
    ks_audit_firstfit* o = outs[i]; const u32 Pn = ds[i]->h.P; const u32* meta = t.meta;
    o->n_pods = Pn; o->n_new = meta[0]; o->n_placed = meta[1]; o->skipped_pods = t.field[2]; o->n_pods_flagged = t.n_pods_flagged; o->checked[0] = t.field[0]; o->checked[1] = t.field[1]; o->checked[2] = meta[3]; o->admitting_pairs = meta[4];
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
  }));
  clock.store(outs, n);
  return KS_OK;
}
extern "C" int ks_audit_firstfit_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_firstfit* const* outs) { return audit_batch(ds, n, outs, true, audit_firstfit_run); }
extern "C" int ks_audit_firstfit_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_firstfit* out) { return audit_one(d, claimed, out, AUD_READS_FIT, true, audit_firstfit_run); }
