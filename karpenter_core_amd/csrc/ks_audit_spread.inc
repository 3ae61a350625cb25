// ks_audit_spread.inc -- the audit's third, opt-in pass: topology spread over NARROW keys (the zone), checked in COMMIT ORDER (ksolve.h ks_audit_spread_dev /
// ks_audit_spread_batch_dev, KS_AUDIT_POD_SPREAD).  Included by ksolve.hip after ks_audit_topo.inc, outside the emulator's guards: the tests/sim build compiles and
// runs these kernels too.  The first two passes' kernels, views and outputs are untouched; their helpers (aud_where, aud_class, aud_topo_skipped, aud_topo_unfiltered,
// aud_topo_dom) are called as they are.
//
// nextDomainTopologySpread (topologygroup.go:159-200) admits domain d only if count[d] + self - min <= maxSkew, with counts "at the time": prefix counts over the
// commit order, which pod_seq gives.  A recorder's contribution is known exactly only where its node was already pinned to one domain when it committed, so the
// rule compares a LOWER bound of count[d] (the certain recorders) with an UPPER bound of the minimum (every recorder, plus the wild ones in every domain): it flags
// only what no run of the reference can have produced, and is the reference's own test where the bounds meet (exact_pairs).  DESIGN.md 7.23 has the argument.
// Five launches on the problems' stream, blockIdx.y = the problem; the commit order is cut into chunks of KS_AS_CHUNK commit numbers:
//   ks_audit_spread_count   one lane per pod: the placed pods counted, and counted per commit number (the second pass's SEQ rule); the pin table set to "never";
//                           elig[g] decided once per group, the unattempted spread groups counted.  Atomics go to scratch and add integers: the same sums every run.
//   ks_audit_spread_order   one lane per pod: SEQ, ord[seq] = pod, and atomicMin of its commit number into pin[node][key] for every key its class pins (a minimum
//                           of integers: the same table every run).  Writes every pod's flag and checked word (SEQ, placed).
//   ks_audit_spread_chunks  one lane per commit number: the recorder adds itself to tab[chunk][group][domain][any | certain] or to the chunk's wild count.
//   ks_audit_spread_scan    one lane per (group, domain, kind): the exclusive prefix along the chunks, in place; lanes are neighbours in memory.
//   ks_audit_spread_pods    one wave per chunk.  For every tile of 64 commit numbers and every distinct eligible group a pod of the tile is constrained by
//                           (__ballot, __shfl from the first set lane): the chunk's tiles up to that one are walked in order with lane = DOMAIN holding the running
//                           L, U (and every lane W); inside the pod's own tile a lane = POD gets its prefix from __ballot(records && dom == e) & lanes-below.  The
//                           one lane that holds the pod adds its bit and its checked word: a plain read-modify-write, after ks_audit_spread_order has finished.
// No float, no atomic on an output, no dynamically indexed register array, no LDS beyond the count kernel's reduction.
#define KS_AS_CHUNK 256u                 // commit numbers per chunk: four tiles of one wave
#define KS_AS_ROW 129u                   // words per (chunk, group): [64 domains][any | certain] | wild
struct AuditSpreadView {
  u32* flags; u32* chk; u32* meta;       // outputs: [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_SPREAD | [P] bits 0-9 the (pod, group) pairs examined, 10-19 those of them that were exact, bit 30 placed | [4]: n_new, placed pods, unattempted spread groups
  u32* seqcnt; u32* ord; u32* pin;       // scratch: [P] placed pods per commit number | [P] commit number -> pod + 1 (0: none) | [(E + NMAX) * K] the commit number from which the node's requirement on k is one value
  u32* elig; u32* cntr; u32* tab;        // scratch: [G] the group is examined | [1] placed pods | [chunks][G][KS_AS_ROW] the chunk's recorders, then (scanned) those of the chunks before it
};
__device__ __forceinline__ u32 aud_spr_chunks(u32 np) { const u32 n = (np + KS_AS_CHUNK - 1u) / KS_AS_CHUNK; return n ? n : 1u; }
// was the requirement of node nd on key k one value when the pod with commit number sq was recorded?
__device__ __forceinline__ bool aud_spr_certain(const DevProb& P, const AuditView& V, const AuditSpreadView& S, u32 nd, u32 k, u32 sq) {
  if (nd < P.E) { if (((GC(u32, P.en.present)[nd] >> k) & 1u) && !((GC(u32, P.en.complement)[nd] >> k) & 1u)) return true; }
  else {
    const i32 m = GC(i32, V.n_tmpl)[nd - P.E];
    if (m >= 0 && (u32)m < P.M && ((GC(u32, P.tmpl.present)[m] >> k) & 1u) && !((GC(u32, P.tmpl.complement)[m] >> k) & 1u) && __builtin_popcountll(GC(u64, P.tmpl.mask)[(size_t)m * P.K + k]) == 1) return true;
  }
  return S.pin[(size_t)nd * P.K + k] <= sq;
}
// what recorder q (class c, node nd, commit number sq) adds to eligible group g on key k: 0 nothing | 1 domain *e, uncertain | 2 domain *e, certain | 3 wild
__device__ __forceinline__ u32 aud_spr_record(const DevProb& P, const AuditView& V, const AuditSpreadView& S, u32 c, u32 nd, u32 sq, u32 g, u32 k, u32* e) {
  bool rec = false;
  for (u32 i = GC(u32, P.cls_sel_off)[c]; i < GC(u32, P.cls_sel_off)[c + 1]; ++i) if (GC(u32, P.sel_list)[i] == g) { rec = true; break; }
  if (!rec) return 0u;
  u64 dom = 0;
  if (aud_topo_dom(P, V, nd, k, &dom)) {
    if (__builtin_popcountll(dom) != 1) return 0u;      // (Record counts a spread only when Len() == 1, and the set was no smaller then)
    *e = (u32)__builtin_ctzll(dom);
    return aud_spr_certain(P, V, S, nd, k, sq) ? 2u : 1u;
  }
  return (nd < P.E && !((GC(u32, P.en.present)[nd] >> k) & 1u)) ? 3u : 0u;      // (an existing node the reference may have pinned through an earlier pod; the problem keeps only its labels)
}

__global__ __launch_bounds__(256) void ks_audit_spread_count(const DevProb* probs, const AuditView* views, const AuditSpreadView* sviews) {
  __shared__ u32 s_sum[256];
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), npin = (P.E + P.NMAX) * P.K;
  u32 mine = 0;
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < np; i += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, i, NS), sq = GC(i32, V.pod_seq)[i];
    if (nd >= 0) { ++mine; if (sq >= 0 && (u32)sq < np) atomicAdd(&S.seqcnt[sq], 1u); }
  }
  aud_block_sum(s_sum, mine);
  if (threadIdx.x == 0 && s_sum[0]) atomicAdd(&S.cntr[0], s_sum[0]);
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < npin; i += gridDim.x * 256u) S.pin[i] = KS_AT_NEVER;
  if (blockIdx.x == 0) {      // (the same in all 256 threads: every thread takes the barriers below)
    u32 un = 0;
    for (u32 g = threadIdx.x; g < P.G; g += 256u) {
      const i32 k = GC(i32, P.grp_key)[g];
      const bool spread = GC(u8, P.grp_type)[g] == 0, ok = spread && k >= 0 && (u32)k < P.K && !aud_topo_skipped(P, g) && aud_topo_unfiltered(P, g);
      S.elig[g] = ok ? 1u : 0u;
      if (spread && !ok) ++un;
    }
    __syncthreads();
    aud_block_sum(s_sum, un);
    if (threadIdx.x == 0) S.meta[2] = s_sum[0];
  }
}
__global__ __launch_bounds__(256) void ks_audit_spread_order(const DevProb* probs, const AuditView* views, const AuditSpreadView* sviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), K = P.K, n_placed = S.cntr[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) { S.meta[0] = aud_n_new(P, V); S.meta[1] = n_placed; }
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    const bool ok = nd >= 0 && aud_seq_ok(V, S.seqcnt, p, n_placed);
    S.flags[p] = (nd >= 0 && !ok) ? KS_AUDIT_POD_SEQ : 0u; S.chk[p] = nd >= 0 ? 1u << 30 : 0u;
    if (!ok) continue;
    const u32 sq = (u32)GC(i32, V.pod_seq)[p], c = aud_class(P, V, p);
    S.ord[sq] = p + 1u;
    // the keys the pod pins its node on: a single-value In of its class, or a spread group it owns on the key (its own topology requirement is one domain, topologygroup.go:181)
    const u32 cp = GC(u32, P.cls.present)[c] & ~GC(u32, P.cls.complement)[c]; u32 pk = 0;
    for (u32 k = 0; k < K; ++k) if (((cp >> k) & 1u) && __builtin_popcountll(GC(u64, P.cls.mask)[(size_t)c * K + k]) == 1) pk |= 1u << k;
    for (u32 i = GC(u32, P.cls_own_off)[c]; i < GC(u32, P.cls_own_off)[c + 1]; ++i) {
      const u32 g = GC(u32, P.own_list)[i] & 0x7FFFFFFFu; const i32 k = GC(i32, P.grp_key)[g];
      if (GC(u8, P.grp_type)[g] == 0 && k >= 0 && (u32)k < K) pk |= 1u << k;
    }
    for (; pk; pk &= pk - 1) atomicMin(&S.pin[(size_t)nd * K + (u32)__builtin_ctz(pk)], sq);
  }
}
__global__ __launch_bounds__(256) void ks_audit_spread_chunks(const DevProb* probs, const AuditView* views, const AuditSpreadView* sviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), G = P.G;
  if (!G) return;
  for (u32 s = blockIdx.x * 256u + threadIdx.x; s < np; s += gridDim.x * 256u) {
    const u32 q1 = S.ord[s];
    if (!q1) continue;
    const u32 q = q1 - 1u, ch = s / KS_AS_CHUNK; const i32 nd = aud_where(P, V, q, NS);
    if (nd < 0) continue;
    const u32 c = aud_class(P, V, q);
    for (u32 i = GC(u32, P.cls_sel_off)[c]; i < GC(u32, P.cls_sel_off)[c + 1]; ++i) {
      const u32 g = GC(u32, P.sel_list)[i];
      if (g >= G || !S.elig[g]) continue;
      u32 e = 0; const u32 what = aud_spr_record(P, V, S, c, (u32)nd, s, g, (u32)GC(i32, P.grp_key)[g], &e);
      u32* row = S.tab + ((size_t)ch * G + g) * KS_AS_ROW;
      if (what == 3u) atomicAdd(&row[128], 1u);
      else if (what) { atomicAdd(&row[e * 2u], 1u); if (what == 2u) atomicAdd(&row[e * 2u + 1u], 1u); }
    }
  }
}
__global__ __launch_bounds__(256) void ks_audit_spread_scan(const DevProb* probs, const AuditSpreadView* sviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y];
  const u32 nch = aud_spr_chunks(P.P); const size_t width = (size_t)P.G * KS_AS_ROW;
  for (size_t i = (size_t)blockIdx.x * 256u + threadIdx.x; i < width; i += (size_t)gridDim.x * 256u) {
    if (!S.elig[i / KS_AS_ROW]) continue;
    u32 run = 0;
    for (u32 ch = 0; ch < nch; ++ch) { u32* w = S.tab + (size_t)ch * width + i; const u32 v = *w; *w = run; run += v; }
  }
}
__global__ __launch_bounds__(64) void ks_audit_spread_pods(const DevProb* probs, const AuditView* views, const AuditSpreadView* sviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, np = P.P, E = P.E, NS = E + aud_n_new(P, V), G = P.G, K = P.K, nch = aud_spr_chunks(np);
  const u64 below = (1ull << lane) - 1ull;
  if (!G) return;
  for (u32 ch = blockIdx.x; ch < nch; ch += gridDim.x) {      // (ch, and every loop bound below, is the same in all 64 lanes)
    const u32 base = ch * KS_AS_CHUNK;
    for (u32 t = 0; t < KS_AS_CHUNK / 64u && base + t * 64u < np; ++t) {
      const u32 s = base + t * 64u + lane, p1 = s < np ? S.ord[s] : 0u, p = p1 - 1u;
      i32 nd = -1; u32 c = 0, ob = 0, no = 0;
      if (p1) { nd = aud_where(P, V, p, NS); if (nd >= 0) { c = aud_class(P, V, p); ob = GC(u32, P.cls_own_off)[c]; no = GC(u32, P.cls_own_off)[c + 1] - ob; } }
      u32 maxo = no; for (int x = 32; x > 0; x >>= 1) { const u32 o = __shfl_xor(maxo, x); maxo = o > maxo ? o : maxo; }
      u32 f = 0, chk = 0;
      for (u32 oi = 0; oi < maxo; ++oi) {
        u32 g = 0, self = 0; bool valid = false;
        if (oi < no) { const u32 ent = GC(u32, P.own_list)[ob + oi]; g = ent & 0x7FFFFFFFu; self = ent >> 31; valid = g < G && S.elig[g] != 0u; }
        for (u64 pending = ballot64(valid); pending;) {
          const u32 gl = (u32)__shfl((int)g, (int)__builtin_ctzll(pending));      // a group some pod of the tile is constrained by; its pods are examined together
          const bool member = valid && g == gl;
          pending &= ~ballot64(member);
          const u32 k = (u32)GC(i32, P.grp_key)[gl];
          // steps 1 and 2 for the member pods: the pod's own domain d
          bool counts = false; u32 d = 0; u64 among = 0;
          if (member) {
            u64 mine = 0;
            if (!aud_topo_dom(P, V, (u32)nd, k, &mine)) {
              if (!((u32)nd < E && ((P.wellknown_mask >> k) & 1u) && !((GC(u32, P.en.present)[nd] >> k) & 1u))) { f |= KS_AUDIT_POD_SPREAD; chk += 1u; }      // (else: 7.22's exception, not examined)
            } else {
              chk += 1u;
              if (__builtin_popcountll(mine) != 1) f |= KS_AUDIT_POD_SPREAD;
              else {
                d = (u32)__builtin_ctzll(mine);
                if (GC(i32, P.grp_count)[(size_t)gl * 64 + d] < 0) f |= KS_AUDIT_POD_SPREAD;
                else {
                  counts = true;
                  const u32 cp = GC(u32, P.cls.present)[c];
                  among = ((cp >> k) & 1u) ? kreq_has_mask(load_req(cp, GC(u32, P.cls.complement)[c], P.cls.mask + (size_t)c * K, P.cls.gt + (size_t)c * K, P.cls.lt + (size_t)c * K, (int)k), P.value_int + k * 64, GC(u32, P.key_nvalues)[k]) : ~0ull;
                }
              }
            }
          }
          if (!ballot64(counts)) continue;
          // lane = domain: the counts at the chunk's first commit number
          const i32 init = GC(i32, P.grp_count)[(size_t)gl * 64 + lane]; const u32* row = S.tab + ((size_t)ch * G + gl) * KS_AS_ROW;
          const u64 reg = ballot64(init >= 0);
          i64 U = (i64)(init > 0 ? init : 0) + row[lane * 2u], L = (i64)(init > 0 ? init : 0) + row[lane * 2u + 1u], W = row[128];
          among &= reg;
          for (u32 t2 = 0; t2 <= t; ++t2) {
            // lane = recorder: what the pod with commit number base + t2 * 64 + lane adds to gl
            const u32 s2 = base + t2 * 64u + lane, q1 = s2 < np ? S.ord[s2] : 0u; u32 what = 0, re = 0;
            if (q1) { const i32 n2 = aud_where(P, V, q1 - 1u, NS); if (n2 >= 0) what = aud_spr_record(P, V, S, aud_class(P, V, q1 - 1u), (u32)n2, s2, gl, k, &re); }
            const u64 bw = ballot64(what == 3u);
            if (t2 < t) {
              for (u64 ds = aud_wave_or((what == 1u || what == 2u) ? 1ull << re : 0ull); ds; ds &= ds - 1) {
                const u32 e = (u32)__builtin_ctzll(ds); const u64 ba = ballot64((what == 1u || what == 2u) && re == e), bc = ballot64(what == 2u && re == e);
                if (lane == e) { U += __builtin_popcountll(ba); L += __builtin_popcountll(bc); }
              }
              W += __builtin_popcountll(bw);
            } else {
              // the pod's own tile: lane = pod, its prefix from the lanes below it
              const i64 Wl = W + __builtin_popcountll(bw & below); i64 least = INT32_MAX, Ld = 0; bool exact = Wl == 0;
              for (u64 ds = reg; ds; ds &= ds - 1) {
                const u32 e = (u32)__builtin_ctzll(ds); const u64 ba = ballot64((what == 1u || what == 2u) && re == e), bc = ballot64(what == 2u && re == e);
                const u32 ulo = (u32)__shfl((int)(u32)U, (int)e), llo = (u32)__shfl((int)(u32)L, (int)e);      // (counts of pods and int32 initial counts: below 2^32)
                const i64 Ue = (i64)ulo + __builtin_popcountll(ba & below), Le = (i64)llo + __builtin_popcountll(bc & below);
                if (counts && e == d) { Ld = Le; if (Le != Ue) exact = false; }
                if (counts && ((among >> e) & 1ull)) { if (Ue + Wl < least) least = Ue + Wl; if (Le != Ue) exact = false; }
              }
              if (counts) {
                if (Ld + (i64)self - least > (i64)GC(i32, P.grp_max_skew)[gl]) f |= KS_AUDIT_POD_SPREAD;
                if (exact) chk += 1u << 10;
              }
            }
          }
        }
      }
      if (p1 && nd >= 0 && (f | chk)) { S.flags[p] |= f; S.chk[p] += chk; }
    }
  }
}

// ---- host half ----
// A batch is walked in slices (audit_slices), as the second pass walks it with `first`: the chunk table is chunks x G x KS_AS_ROW words per problem (sized here, from
// P and G), and a slice holds at most KS_AUDIT_SPREAD_TAB_WORDS of them (64 MiB), or one problem.
#define KS_AUDIT_SPREAD_TAB_WORDS ((size_t)16 << 20)
static size_t audit_spread_tab_words(const ks_dev_problem* d) { const size_t nch = std::max<size_t>(1, ((size_t)d->h.P + KS_AS_CHUNK - 1) / KS_AS_CHUNK); return nch * d->h.G * KS_AS_ROW; }
static int audit_spread_slice(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_spread* const* outs, AuditGate* g, double* kernel_ms, double* readback_ms) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n), o_sview = st.add<AuditSpreadView>(n);
  TRY(st.place());
  AuditWork W(ds[0]->device); std::vector<size_t> o_fl(n), o_ck(n), o_scr(n); u32 pmax = 0, chmax = 1; size_t wmax = 1;
  W.out(4 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { o_fl[i] = W.out(ds[i]->h.P); o_ck[i] = W.out(ds[i]->h.P); pmax = std::max(pmax, ds[i]->h.P); wmax = std::max(wmax, (size_t)ds[i]->h.G * KS_AS_ROW); }
  chmax = std::max(1u, (pmax + KS_AS_CHUNK - 1u) / KS_AS_CHUNK);
  for (u32 i = 0; i < n; ++i) { const DevProb& h = ds[i]->h; o_scr[i] = W.scratch(2 * (size_t)h.P + ((size_t)h.E + h.NMAX) * h.K + h.G + 1 + audit_spread_tab_words(ds[i])); }
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditSpreadView t{}; const DevProb& h = ds[i]->h; const size_t Pn = h.P, npin = ((size_t)h.E + h.NMAX) * h.K;
    t.meta = w + 4 * (size_t)i; t.flags = w + o_fl[i]; t.chk = w + o_ck[i];
    u32* s = w + o_scr[i]; t.seqcnt = s; t.ord = s + Pn; t.pin = s + 2 * Pn; t.elig = s + 2 * Pn + npin; t.cntr = s + 2 * Pn + npin + h.G; t.tab = s + 2 * Pn + npin + h.G + 1;
    st.h<AuditView>(o_view)[i] = audit_pass_view(results[i], t.meta); st.h<AuditSpreadView>(o_sview)[i] = t;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view); const AuditSpreadView* dt = st.d<const AuditSpreadView>(o_sview);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_c = std::min(4096u, chmax), gx_s = (u32)std::max<size_t>(1, std::min<size_t>(1024, (wmax + 255) / 256));
  audit_rows(n, [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_spread_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_spread_order, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_spread_chunks, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_spread_scan, dim3(gx_s, ny), dim3(256), 0, st.stream(), st.probs() + base, dt + base);
    hipLaunchKernelGGL(ks_audit_spread_pods, dim3(gx_c, ny), dim3(64), 0, st.stream(), st.probs() + base, dv + base, dt + base);
  });
  const AuditTail tail{4, o_fl.data(), o_ck.data(), nullptr, 3, {30, 0, 10, 0}, {3u, 1023u, 1023u, 0u}};      // checked[0], checked[1], exact_pairs of a checked word
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32*) {
    ks_audit_spread* o = outs[i]; const u32 Pn = ds[i]->h.P; const u32* meta = t.meta;
    o->n_pods = Pn; o->n_new = meta[0]; o->n_placed = meta[1]; o->skipped_groups = meta[2]; o->n_pods_flagged = t.n_pods_flagged; o->checked[0] = t.field[0]; o->checked[1] = t.field[1]; o->exact_pairs = t.field[2];
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
  }));
  clock.add(kernel_ms, readback_ms);
  return KS_OK;
}
static int audit_spread_run(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_spread* const* outs, AuditGate* g) {
  size_t budget = KS_AUDIT_SPREAD_TAB_WORDS;
  if (const char* e = getenv("KS_AUDIT_SPREAD_SLICE_WORDS")) budget = (size_t)strtoull(e, nullptr, 0);      // (diagnostic, as KS_POISON: lets a test walk a small batch in slices; the flags must not depend on it)
  return audit_slices(ds, n, results, outs, g, audit_spread_tab_words, budget, audit_spread_slice);
}
extern "C" int ks_audit_spread_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_spread* const* outs) { return audit_batch(ds, n, outs, true, audit_spread_run); }
extern "C" int ks_audit_spread_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_spread* out) { return audit_one(d, claimed, out, AUD_READS_ORDER, true, audit_spread_run); }
