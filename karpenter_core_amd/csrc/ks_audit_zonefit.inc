// ks_audit_zonefit.inc -- an opt-in pass beside the gate's eight: FIRST-FIT ORDER for the pods whose constraining groups are all eligible ZONAL spread groups -- topology
// spread over a narrow key with an empty node filter (ksolve.h ks_audit_zonefit_dev / ks_audit_zonefit_batch_dev, KS_AUDIT_POD_ZFIT_*).  Included by ksolve.hip after
// ks_audit_reasons.inc, outside the emulator's guards: the tests/sim build compiles and runs these kernels too.  The earlier passes' kernels, views and outputs are
// untouched.  Four of the third pass's kernels (ks_audit_spread_count / _order / _chunks / _scan: elig, ord, pin and the scanned chunk table) and two of the fourth's
// (ks_audit_ff_count / ks_audit_ff_mark: the existing nodes' request sums and presence masks, open[]) are launched as they are, over this pass's own views of them, and
// their helpers (aud_where, aud_class, aud_n_new, aud_seq_ok, aud_spr_record, aud_spr_certain, aud_topo_dom, aud_fit_existing, aud_fit_mounts / _live / _labelled, aud_fit_admits_new) are
// called as they are.
//
// A zonal group's minimum moves over time, so the final counts alone decide nothing; the final state TOGETHER WITH the commit numbers does.  Pod P was tried for the
// last time when exactly the pods with commit number < s had committed (s = pod_seq[P]; an unscheduled pod: s = n_placed).  At that prefix the third pass's bounds
// L_s <= count <= U_s + W_s give, per group g of P's class, a mask OK_s[g] of domains the skew inequality CERTAINLY admitted (the upper bound of the count against the
// lower bound of the minimum: the opposite pairing to the third pass's test).  A node whose domain on key(g) was one value z at s, with z in OK_s[g] for every g, passed
// the topology step at s; the fourth pass's monotone half of admission (requests only grow, requirements only narrow, options only shrink) says the rest from the
// final state (DESIGN.md 7.32).  Twelve launches on the problems' stream, blockIdx.y = the problem:
//   ks_audit_spread_count   the third pass's: elig[g], pin set to "never", the placed pods per commit number.
//   ks_audit_ff_count       the fourth pass's: the existing nodes' request sums and presence masks, open[] set to "never".
//   ks_audit_ff_mark        the fourth pass's: open[j] by atomicMin.
//   ks_audit_zf_mark        one lane per pod: the examined pods listed (and of them the openers and the unscheduled: the pods checked against new nodes), the per-pod
//                           minima set to "never"; the eligible groups counted.  A problem with no examined pod does no more than this: the kernels below that are this
//                           pass's own return after one load (the verdict kernel still writes every pod's SEQ bit and checked word).
//   ks_audit_spread_order / _chunks / _scan   the third pass's: ord, pin, the chunk table and its exclusive prefix.
//   ks_audit_zf_totals      one wave per eligible group: lane = domain, the prefix at n_placed (the last chunk's row plus its recorders): the row the unscheduled pods read.
//   ks_audit_zf_window      one wave per chunk, the walk of ks_audit_spread_pods: lane = domain holds the running L / U, lane = pod takes its prefix by ballot and popcount;
//                           all 64 domains are kept: okmask[P][g] and the exact bit.  Then the unscheduled pods, a lane each, from the totals row.
//   ks_audit_zf_existing    one lane per (examined pod, existing node): the bit test of the node's label value against the pod's masks first -- a lane ends the pairs the
//                           zone refuses, not a wave --, then the fourth pass's aud_fit_existing; a wave minimum, then atomicMin into the pod's scratch word.
//   ks_audit_zf_new         one lane per (opener or unscheduled pod, new node): open(j) < s, the key already one value at s - 1, the value in the mask; then a wave per
//                           surviving pair: the fourth pass's aud_fit_admits_new.
//   ks_audit_zf_verdict     one lane per pod: its flag word and its checked word, one writer each, a plain store.
// No float, no LDS beyond the reused kernels' and the count of the eligible groups, no dynamically indexed register array, no atomic on an output; the lists are
// appended by integer atomicAdd into scratch and only minima and sums are taken over them: the same flags and counters every run.
struct AuditZoneView {
  u64* okmask;                             // scratch: [P * KS_AZ_GROUPS] the domains of key(g) that certainly admitted the pod at its moment, by the place of g in own_list(c)
  u32* zst;                                // scratch: [P] bit 0 examined | bit 1 exact | bit 2 checked against new nodes (it opened its node, or is unscheduled)
  u32* first_e; u32* first_open;           // scratch: [P] the least admitting existing node | the least open() over the admitting new nodes
  u32* xlist; u32* nlist;                  // scratch: [P] the examined pods | those of them with bit 2
  u32* zcntr;                              // scratch: [8] examined pods, pods in nlist, zone tests, static predicates evaluated, admitting pairs, eligible groups
  u32* ztot;                               // scratch: [G * KS_AS_ROW] the third pass's row at prefix n_placed
};
// the class reserves no host port, no inverse group constrains it, it owns between one and KS_AZ_GROUPS groups and every one of them is eligible (elig: as ks_audit_spread_count wrote it)
__device__ __forceinline__ bool aud_zf_examinable(const DevProb& P, const u32* elig, u32 c) {
  if (GC(u32, P.cls_port_off)[c + 1] != GC(u32, P.cls_port_off)[c] || GC(u32, P.cls_isel_off)[c + 1] != GC(u32, P.cls_isel_off)[c]) return false;
  const u32 ob = GC(u32, P.cls_own_off)[c], no = GC(u32, P.cls_own_off)[c + 1] - ob;
  if (no == 0u || no > KS_AZ_GROUPS) return false;
  for (u32 i = 0; i < no; ++i) { const u32 g = GC(u32, P.own_list)[ob + i] & 0x7FFFFFFFu; if (g >= P.G || !elig[g]) return false; }
  return true;
}
// the class owns an eligible zonal group and a hostname-keyed group constrains it too: the named next step, counted apart
__device__ __forceinline__ bool aud_zf_mixed(const DevProb& P, const u32* elig, u32 c) {
  bool zonal = false, host = false;
  for (u32 i = GC(u32, P.cls_own_off)[c]; i < GC(u32, P.cls_own_off)[c + 1]; ++i) {
    const u32 g = GC(u32, P.own_list)[i] & 0x7FFFFFFFu; if (g >= P.G) continue;
    if (elig[g]) zonal = true;
    if (GC(i32, P.grp_key)[g] == KS_KEY_HOSTNAME) host = true;
  }
  for (u32 i = GC(u32, P.cls_isel_off)[c]; i < GC(u32, P.cls_isel_off)[c + 1]; ++i) { const u32 g = GC(u32, P.isel_list)[i] & 0x7FFFFFFFu; if (g < P.G && GC(i32, P.grp_key)[g] == KS_KEY_HOSTNAME) host = true; }
  return zonal && host;
}
// podDomains.Has over the registered domains is taken by the caller: bit e = the class's requirement on k has value e (an absent key has every value)
__device__ __forceinline__ u64 aud_zf_among(const DevProb& P, u32 c, u32 k) {
  const u32 cp = GC(u32, P.cls.present)[c];
  return ((cp >> k) & 1u) ? kreq_has_mask(aud_fit_cls_req(P, c, k), P.value_int + k * 64, GC(u32, P.key_nvalues)[k]) : ~0ull;
}

__global__ __launch_bounds__(256) void ks_audit_zf_mark(const DevProb* probs, const AuditView* views, const AuditFitView* fviews, const AuditSpreadView* sviews, const AuditZoneView* zviews) {
  __shared__ u32 s_sum[256];
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y]; const AuditZoneView& Z = zviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, np = P.P, E = P.E, NS = E + aud_n_new(P, V), n_placed = F.cntr[0];
  const u64 below = (1ull << lane) - 1ull;
  if (blockIdx.x == 0) {      // (the same in all 256 threads: every thread takes the barriers)
    u32 ne = 0;
    for (u32 g = threadIdx.x; g < P.G; g += 256u) ne += S.elig[g];
    aud_block_sum(s_sum, ne);
    if (threadIdx.x == 0) Z.zcntr[5] = s_sum[0];
  }
  for (u32 p0 = blockIdx.x * 256u; p0 < np; p0 += gridDim.x * 256u) {      // (p0 is the same in all 256 threads: every lane reaches the ballots)
    const u32 p = p0 + threadIdx.x; bool ex = false, nw = false;
    if (p < np) {
      const i32 nd = aud_where(P, V, p, NS);
      const bool ok = nd >= 0 && aud_seq_ok(V, F.seqcnt, p, n_placed), unsched = GC(i32, V.pod_node)[p] == -1;
      ex = (ok || unsched) && aud_zf_examinable(P, S.elig, aud_class(P, V, p));
      nw = ex && (unsched || ((u32)nd >= E && (u32)GC(i32, V.pod_seq)[p] == F.open[(u32)nd - E]));
      Z.first_e[p] = KS_AF_NEVER; Z.first_open[p] = KS_AF_NEVER; Z.zst[p] = (ex ? 1u : 0u) | (nw ? 4u : 0u);
    }
    const u64 bx = ballot64(ex), bn = ballot64(nw);
    u32 xb = 0, nb = 0;
    if (lane == 0) { if (bx) xb = atomicAdd(&Z.zcntr[0], (u32)__builtin_popcountll(bx)); if (bn) nb = atomicAdd(&Z.zcntr[1], (u32)__builtin_popcountll(bn)); }
    xb = (u32)__shfl((int)xb, 0); nb = (u32)__shfl((int)nb, 0);
    if (ex) Z.xlist[xb + (u32)__builtin_popcountll(bx & below)] = p;
    if (nw) Z.nlist[nb + (u32)__builtin_popcountll(bn & below)] = p;
  }
}
__global__ __launch_bounds__(64) void ks_audit_zf_totals(const DevProb* probs, const AuditView* views, const AuditSpreadView* sviews, const AuditZoneView* zviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y]; const AuditZoneView& Z = zviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, np = P.P, NS = P.E + aud_n_new(P, V), G = P.G, ch = aud_spr_chunks(np) - 1u, base = ch * KS_AS_CHUNK;
  if (!G || !Z.zcntr[0]) return;
  for (u32 g = blockIdx.x; g < G; g += gridDim.x) {      // (g, and every loop bound below, is the same in all 64 lanes)
    if (!S.elig[g]) continue;
    const u32 k = (u32)GC(i32, P.grp_key)[g];
    const i32 init = GC(i32, P.grp_count)[(size_t)g * 64 + lane]; const u32* row = S.tab + ((size_t)ch * G + g) * KS_AS_ROW;
    u32 U = (u32)(init > 0 ? init : 0) + row[lane * 2u], L = (u32)(init > 0 ? init : 0) + row[lane * 2u + 1u], W = row[128];
    for (u32 t2 = 0; t2 < KS_AS_CHUNK / 64u && base + t2 * 64u < np; ++t2) {
      const u32 s2 = base + t2 * 64u + lane, q1 = s2 < np ? S.ord[s2] : 0u; u32 what = 0, re = 0;
      if (q1) { const i32 n2 = aud_where(P, V, q1 - 1u, NS); if (n2 >= 0) what = aud_spr_record(P, V, S, aud_class(P, V, q1 - 1u), (u32)n2, s2, g, k, &re); }
      for (u64 ds = aud_wave_or((what == 1u || what == 2u) ? 1ull << re : 0ull); ds; ds &= ds - 1) {
        const u32 e = (u32)__builtin_ctzll(ds); const u64 ba = ballot64((what == 1u || what == 2u) && re == e), bc = ballot64(what == 2u && re == e);
        if (lane == e) { U += (u32)__builtin_popcountll(ba); L += (u32)__builtin_popcountll(bc); }
      }
      W += (u32)__builtin_popcountll(ballot64(what == 3u));
    }
    u32* out = Z.ztot + (size_t)g * KS_AS_ROW;
    out[lane * 2u] = U; out[lane * 2u + 1u] = L;
    if (lane == 0) out[128] = W;
  }
}
__global__ __launch_bounds__(64) void ks_audit_zf_window(const DevProb* probs, const AuditView* views, const AuditSpreadView* sviews, const AuditZoneView* zviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y]; const AuditZoneView& Z = zviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, np = P.P, NS = P.E + aud_n_new(P, V), G = P.G, nch = aud_spr_chunks(np);
  const u64 below = (1ull << lane) - 1ull;
  if (!G || !Z.zcntr[0]) return;
  for (u32 ch = blockIdx.x; ch < nch; ch += gridDim.x) {      // (ch, and every loop bound below, is the same in all 64 lanes)
    const u32 base = ch * KS_AS_CHUNK;
    for (u32 t = 0; t < KS_AS_CHUNK / 64u && base + t * 64u < np; ++t) {
      const u32 s = base + t * 64u + lane, p1 = s < np ? S.ord[s] : 0u, p = p1 - 1u;
      u32 c = 0, ob = 0, no = 0;
      if (p1 && (Z.zst[p] & 1u)) { c = aud_class(P, V, p); ob = GC(u32, P.cls_own_off)[c]; no = GC(u32, P.cls_own_off)[c + 1] - ob; }      // (an examined pod in ord is on a node and owns 1 .. KS_AZ_GROUPS groups)
      u32 maxo = no; for (int x = 32; x > 0; x >>= 1) { const u32 o = __shfl_xor(maxo, x); maxo = o > maxo ? o : maxo; }
      bool exact_all = true;
      for (u32 oi = 0; oi < maxo; ++oi) {
        u32 g = 0, self = 0; const bool valid = oi < no;
        if (valid) { const u32 ent = GC(u32, P.own_list)[ob + oi]; g = ent & 0x7FFFFFFFu; self = ent >> 31; }
        for (u64 pending = ballot64(valid); pending;) {
          const u32 gl = (u32)__shfl((int)g, (int)__builtin_ctzll(pending));      // a group some examined pod of the tile owns; its pods take their masks together
          const bool member = valid && g == gl;
          pending &= ~ballot64(member);
          const u32 k = (u32)GC(i32, P.grp_key)[gl];
          // lane = domain: the counts at the chunk's first commit number
          const i32 init = GC(i32, P.grp_count)[(size_t)gl * 64 + lane]; const u32* row = S.tab + ((size_t)ch * G + gl) * KS_AS_ROW;
          const u64 reg = ballot64(init >= 0);
          i64 U = (i64)(init > 0 ? init : 0) + row[lane * 2u], L = (i64)(init > 0 ? init : 0) + row[lane * 2u + 1u], W = row[128];
          const u64 among = member ? aud_zf_among(P, c, k) & reg : 0ull;
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
              // the pod's own tile: lane = pod, its prefix from the lanes below it.  First the least certain count among the pod's domains, then every registered domain against it
              const i64 Wl = W + __builtin_popcountll(bw & below); i64 minL = INT32_MAX; bool exact = Wl == 0;
              for (u64 ds = reg; ds; ds &= ds - 1) {
                const u32 e = (u32)__builtin_ctzll(ds); const u64 ba = ballot64((what == 1u || what == 2u) && re == e), bc = ballot64(what == 2u && re == e);
                const u32 ulo = (u32)__shfl((int)(u32)U, (int)e), llo = (u32)__shfl((int)(u32)L, (int)e);      // (counts of pods and int32 initial counts: below 2^32)
                const i64 Ue = (i64)ulo + __builtin_popcountll(ba & below), Le = (i64)llo + __builtin_popcountll(bc & below);
                if (Le != Ue) exact = false;
                if (((among >> e) & 1ull) && Le < minL) minL = Le;
              }
              u64 mask = 0;
              for (u64 ds = reg; ds; ds &= ds - 1) {
                const u32 e = (u32)__builtin_ctzll(ds); const u64 ba = ballot64((what == 1u || what == 2u) && re == e);
                const i64 Ue = (i64)(u32)__shfl((int)(u32)U, (int)e) + __builtin_popcountll(ba & below);
                if (Ue + Wl + (i64)self - minL <= (i64)GC(i32, P.grp_max_skew)[gl]) mask |= 1ull << e;
              }
              if (member) { Z.okmask[(size_t)p * KS_AZ_GROUPS + oi] = among ? mask : 0ull; if (!among || !exact) exact_all = false; }      // (no domain of the pod's is registered: nothing is proved from Go's MaxInt32 minimum)
            }
          }
        }
      }
      if (no && exact_all) Z.zst[p] |= 2u;      // (the one lane that holds the pod: a plain read-modify-write, after ks_audit_zf_mark has finished)
    }
  }
  // ---- the unscheduled pods, a lane each: the prefix at n_placed is the totals row
  const u32 nn = Z.zcntr[1];
  for (u32 x = blockIdx.x * 64u + lane; x < nn; x += gridDim.x * 64u) {
    const u32 p = Z.nlist[x];
    if (GC(i32, V.pod_node)[p] != -1) continue;
    const u32 c = aud_class(P, V, p), ob = GC(u32, P.cls_own_off)[c], no = GC(u32, P.cls_own_off)[c + 1] - ob;
    bool exact_all = true;
    for (u32 oi = 0; oi < no; ++oi) {
      const u32 ent = GC(u32, P.own_list)[ob + oi], g = ent & 0x7FFFFFFFu, self = ent >> 31, k = (u32)GC(i32, P.grp_key)[g];
      const u32* row = Z.ztot + (size_t)g * KS_AS_ROW; const i64 Wl = row[128];
      const u64 has = aud_zf_among(P, c, k); u64 among = 0, mask = 0; i64 minL = INT32_MAX; bool exact = Wl == 0;
      for (u32 e = 0; e < 64u; ++e) {
        if (GC(i32, P.grp_count)[(size_t)g * 64 + e] < 0) continue;
        const i64 Ue = row[e * 2u], Le = row[e * 2u + 1u];
        if (Le != Ue) exact = false;
        if ((has >> e) & 1ull) { among |= 1ull << e; if (Le < minL) minL = Le; }
      }
      for (u32 e = 0; e < 64u; ++e) {
        if (GC(i32, P.grp_count)[(size_t)g * 64 + e] < 0) continue;
        if ((i64)row[e * 2u] + Wl + (i64)self - minL <= (i64)GC(i32, P.grp_max_skew)[g]) mask |= 1ull << e;
      }
      Z.okmask[(size_t)p * KS_AZ_GROUPS + oi] = among ? mask : 0ull;
      if (!among || !exact) exact_all = false;
    }
    if (exact_all) Z.zst[p] |= 2u;
  }
}
__global__ __launch_bounds__(256) void ks_audit_zf_existing(const DevProb* probs, const AuditView* views, const AuditFitView* fviews, const AuditZoneView* zviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditZoneView& Z = zviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, E = P.E, K = P.K, tiles = (E + 63u) / 64u, n_exam = Z.zcntr[0];
  const size_t total = (size_t)n_exam * tiles;
  for (size_t w = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += (size_t)gridDim.x * 4u) {      // (w, p and c are the same in all 64 lanes)
    const u32 p = Z.xlist[w / tiles], e = (u32)(w % tiles) * 64u + lane, c = aud_class(P, V, p);
    if (aud_fit_mounts(P, c)) continue;
    const bool live = aud_fit_live(P, e);
    // ---- the zone test, a lane per pair: the node carries the label of key(g) with the single value z, and z is in the pod's mask
    bool zok = live;
    if (zok) {
      const u32 ob = GC(u32, P.cls_own_off)[c], no = GC(u32, P.cls_own_off)[c + 1] - ob, ep = GC(u32, P.en.present)[e] & ~GC(u32, P.en.complement)[e];
      for (u32 i = 0; i < no && zok; ++i) {
        const u32 k = (u32)GC(i32, P.grp_key)[GC(u32, P.own_list)[ob + i] & 0x7FFFFFFFu]; const u64 lab = GC(u64, P.en.mask)[(size_t)e * K + k];
        zok = ((ep >> k) & 1u) && __builtin_popcountll(lab) == 1 && ((Z.okmask[(size_t)p * KS_AZ_GROUPS + i] >> __builtin_ctzll(lab)) & 1ull);
      }
    }
    // ---- the fourth pass's predicate, under its condition on labelled keys
    const bool adm = zok && aud_fit_labelled(P, c, e) && aud_fit_existing(P, F, c, e);
    u32 best = adm ? e : KS_AF_NEVER;
    for (int x = 32; x > 0; x >>= 1) { const u32 o = __shfl_xor(best, x); best = o < best ? o : best; }
    const u64 bl = ballot64(live), bz = ballot64(zok), ba = ballot64(adm);
    if (lane == 0) {
      if (best != KS_AF_NEVER) atomicMin(&Z.first_e[p], best);
      if (bl) atomicAdd(&Z.zcntr[2], (u32)__builtin_popcountll(bl));
      if (bz) atomicAdd(&Z.zcntr[3], (u32)__builtin_popcountll(bz));
      if (ba) atomicAdd(&Z.zcntr[4], (u32)__builtin_popcountll(ba));
    }
  }
}
// (probs is __restrict__ for the reason ks_audit_ff_new gives)
__global__ __launch_bounds__(256) void ks_audit_zf_new(const DevProb* __restrict__ probs, const AuditView* views, const AuditFitView* fviews, const AuditSpreadView* sviews, const AuditZoneView* zviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y]; const AuditZoneView& Z = zviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, E = P.E, NN = aud_n_new(P, V), M = P.M, tiles = (NN + 63u) / 64u, nn = Z.zcntr[1], n_placed = F.cntr[0];
  const size_t total = (size_t)nn * tiles;
  for (size_t w = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += (size_t)gridDim.x * 4u) {      // (w, p, c and s are the same in all 64 lanes)
    const u32 p = Z.nlist[w / tiles], j0 = (u32)(w % tiles) * 64u, c = UF(aud_class(P, V, p));      // (c is the same in all 64 lanes, and said so to the compiler: the class's rows are read through scalar registers)
    const u32 s = GC(i32, V.pod_node)[p] == -1 ? n_placed : (u32)GC(i32, V.pod_seq)[p];      // (an opener does not fail SEQ: its commit number is below n_placed)
    if (s == 0u) continue;      // nothing had committed: no new node existed
    // ---- the lane-level filter: the node existed at s, its requirement on every key(g) was one value before s, and its final value is in the pod's mask
    const u32 jl = j0 + lane;
    bool live = jl < NN;
    u32 opened = KS_AF_NEVER;
    if (live) { const i32 ml = GC(i32, V.n_tmpl)[jl]; opened = F.open[jl]; live = ml >= 0 && (u32)ml < M && opened < s; }      // ("never" is above every commit number)
    bool zok = live;
    if (zok) {
      const u32 ob = GC(u32, P.cls_own_off)[c], no = GC(u32, P.cls_own_off)[c + 1] - ob;
      for (u32 i = 0; i < no && zok; ++i) {
        const u32 k = (u32)GC(i32, P.grp_key)[GC(u32, P.own_list)[ob + i] & 0x7FFFFFFFu]; u64 dom = 0;
        zok = aud_spr_certain(P, V, S, E + jl, k, s - 1u) && aud_topo_dom(P, V, E + jl, k, &dom) && __builtin_popcountll(dom) == 1 && ((Z.okmask[(size_t)p * KS_AZ_GROUPS + i] >> __builtin_ctzll(dom)) & 1ull);
      }
    }
    const u64 bl = ballot64(live), bz = ballot64(zok);
    if (lane == 0) { if (bl) atomicAdd(&Z.zcntr[2], (u32)__builtin_popcountll(bl)); if (bz) atomicAdd(&Z.zcntr[3], (u32)__builtin_popcountll(bz)); }
    // ---- the pairs the zone admits, a wave per pair: the fourth pass's admits_new for a node of the result
    for (u64 todo = bz; todo; todo &= todo - 1) {      // (the ballot is the same in all 64 lanes: j, and everything read through it, is too)
      const u32 j = j0 + (u32)__builtin_ctzll(todo);
      const bool adm = aud_fit_admits_new(P, aud_node_final(P, V, j), c, lane);      // (every lane takes the walk's ballots)
      if (lane == 0 && adm) { atomicAdd(&Z.zcntr[4], 1u); atomicMin(&Z.first_open[p], F.open[j]); }
    }
  }
}
__global__ __launch_bounds__(256) void ks_audit_zf_verdict(const DevProb* probs, const AuditView* views, const AuditFitView* fviews, const AuditSpreadView* sviews, const AuditZoneView* zviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditFitView& F = fviews[blockIdx.y]; const AuditSpreadView& S = sviews[blockIdx.y]; const AuditZoneView& Z = zviews[blockIdx.y];
  const u32 np = P.P, E = P.E, NS = E + aud_n_new(P, V), n_placed = F.cntr[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) { F.meta[0] = aud_n_new(P, V); F.meta[1] = n_placed; F.meta[2] = Z.zcntr[5]; F.meta[3] = Z.zcntr[2]; F.meta[4] = Z.zcntr[3]; F.meta[5] = Z.zcntr[4]; }
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    const bool ok = nd >= 0 && aud_seq_ok(V, F.seqcnt, p, n_placed), unsched = GC(i32, V.pod_node)[p] == -1;
    u32 f = (nd >= 0 && !ok) ? KS_AUDIT_POD_SEQ : 0u, chk = nd >= 0 ? 1u << 30 : 0u;
    const u32 st = Z.zst[p];
    if (!(st & 1u)) { F.flags[p] = f; F.chk[p] = chk | (1u << 29) | (aud_zf_mixed(P, S.elig, aud_class(P, V, p)) ? 1u << 28 : 0u); continue; }
    const u32 fe = Z.first_e[p], fo = Z.first_open[p];
    if (nd >= 0 && (u32)nd < E ? fe < (u32)nd : fe != KS_AF_NEVER) f |= KS_AUDIT_POD_ZFIT_EXISTING;      // (a pod on existing node e_P: only a node before e_P)
    if ((st & 4u) && fo != KS_AF_NEVER) f |= KS_AUDIT_POD_ZFIT_NEW;      // (only the nodes with open(j) < s were targets; a pod that joined a new node it did not open is checked against existing nodes only)
    F.flags[p] = f; F.chk[p] = chk | 1u | (st & 2u);
  }
}

// ---- host half ----
// The fourth pass's block [meta | flags | checked words | scratch], the third pass's tables and this pass's own behind it.  The chunk table is the large piece, so
// a batch is walked in slices (audit_slices) by the third pass's budget: at most KS_AUDIT_SPREAD_TAB_WORDS of chunk table, or one problem; KS_AUDIT_SPREAD_SLICE_WORDS
// is honoured as the third pass honours it.
static int audit_zonefit_slice(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_zonefit* const* outs, AuditGate* g, double* kernel_ms, double* readback_ms) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n), o_fview = st.add<AuditFitView>(n), o_sview = st.add<AuditSpreadView>(n), o_zview = st.add<AuditZoneView>(n);
  TRY(st.place());
  AuditWork W(ds[0]->device); std::vector<size_t> o_fl(n), o_ck(n), o_scr(n); u32 pmax = 0, gmax = 1; size_t wmax = 1, emax = 1, nmax = 1;
  W.out(8 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { o_fl[i] = W.out(ds[i]->h.P); o_ck[i] = W.out(ds[i]->h.P); pmax = std::max(pmax, ds[i]->h.P); }
  for (u32 i = 0; i < n; ++i) {
    const DevProb& h = ds[i]->h; const size_t Pn = h.P;
    // the int64 tables first (8-byte aligned): the masks, then the fourth pass's tables with the request sums at their head | the third pass's | this pass's
    o_scr[i] = W.scratch(2 * KS_AZ_GROUPS * Pn + audit_fit_words(h) + (4 * Pn + ((size_t)h.E + h.NMAX) * h.K + h.G + 1 + 4 + audit_spread_tab_words(ds[i])) + (5 * Pn + 8 + (size_t)h.G * KS_AS_ROW), true);
    wmax = std::max(wmax, (size_t)h.G * KS_AS_ROW); gmax = std::max(gmax, h.G);
    emax = std::max(emax, (Pn * (((size_t)h.E + 63) / 64) + 3) / 4); nmax = std::max(nmax, (Pn * (((size_t)h.NMAX + 63) / 64) + 3) / 4);
  }
  const u32 chmax = std::max(1u, (pmax + KS_AS_CHUNK - 1u) / KS_AS_CHUNK);
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditFitView t{}; AuditSpreadView x{}; AuditZoneView z{}; const DevProb& h = ds[i]->h; const size_t Pn = h.P, npin = ((size_t)h.E + h.NMAX) * h.K;
    t.meta = w + 8 * (size_t)i; t.flags = w + o_fl[i]; t.chk = w + o_ck[i];
    u32* s = w + o_scr[i]; z.okmask = (u64*)s; s += 2 * KS_AZ_GROUPS * Pn;      // (an even number of words: the request sums behind it stay 8-byte aligned)
    s = audit_fit_carve(t, h, s);      // (of the fourth pass's tables ks_audit_ff_count sets the three per-class ones to "never" and ks_audit_ff_mark marks used[]; nothing here reads those four, and list[] is neither written nor read: this pass keeps its minima per pod)
    x.seqcnt = s; s += Pn; x.ord = s; s += Pn; x.flags = s; s += Pn; x.chk = s; s += Pn;      // (the third pass's flag and checked words: scratch here)
    x.pin = s; s += npin; x.elig = s; s += h.G; x.cntr = s; s += 1; x.meta = s; s += 4; x.tab = s; s += audit_spread_tab_words(ds[i]);
    z.zst = s; s += Pn; z.first_e = s; s += Pn; z.first_open = s; s += Pn; z.xlist = s; s += Pn; z.nlist = s; s += Pn; z.zcntr = s; s += 8; z.ztot = s;
    st.h<AuditView>(o_view)[i] = audit_pass_view(results[i], t.meta); st.h<AuditFitView>(o_fview)[i] = t; st.h<AuditSpreadView>(o_sview)[i] = x; st.h<AuditZoneView>(o_zview)[i] = z;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view); const AuditFitView* df = st.d<const AuditFitView>(o_fview); const AuditSpreadView* dt = st.d<const AuditSpreadView>(o_sview); const AuditZoneView* dz = st.d<const AuditZoneView>(o_zview);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_c = std::min(4096u, chmax), gx_s = (u32)std::max<size_t>(1, std::min<size_t>(1024, (wmax + 255) / 256)), gx_g = std::min(1024u, gmax);
  const u32 gx_e = (u32)std::min<size_t>(4096, emax), gx_n = (u32)std::min<size_t>(4096, nmax);
  audit_rows(n, [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_spread_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_ff_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
    hipLaunchKernelGGL(ks_audit_ff_mark, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
    hipLaunchKernelGGL(ks_audit_zf_mark, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dt + base, dz + base);
    hipLaunchKernelGGL(ks_audit_spread_order, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_spread_chunks, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_spread_scan, dim3(gx_s, ny), dim3(256), 0, st.stream(), st.probs() + base, dt + base);
    hipLaunchKernelGGL(ks_audit_zf_totals, dim3(gx_g, ny), dim3(64), 0, st.stream(), st.probs() + base, dv + base, dt + base, dz + base);
    hipLaunchKernelGGL(ks_audit_zf_window, dim3(gx_c, ny), dim3(64), 0, st.stream(), st.probs() + base, dv + base, dt + base, dz + base);
    hipLaunchKernelGGL(ks_audit_zf_existing, dim3(gx_e, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dz + base);
    hipLaunchKernelGGL(ks_audit_zf_new, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dt + base, dz + base);
    hipLaunchKernelGGL(ks_audit_zf_verdict, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base, dt + base, dz + base);
  });
  const AuditTail tail{8, o_fl.data(), o_ck.data(), nullptr, 4, {0, 29, 28, 1}, {1u, 1u, 1u, 1u}};      // checked[1], skipped_pods, mixed_pods, exact_pods of a checked word
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32*) {
    ks_audit_zonefit* o = outs[i]; const u32 Pn = ds[i]->h.P; const u32* meta = t.meta;
    o->n_pods = Pn; o->n_new = meta[0]; o->n_placed = meta[1]; o->eligible_groups = meta[2]; o->skipped_groups = ds[i]->h.G - meta[2]; o->skipped_pods = t.field[1]; o->mixed_pods = t.field[2]; o->n_pods_flagged = t.n_pods_flagged;
    o->checked[0] = meta[1]; o->checked[1] = t.field[0]; o->checked[2] = meta[3]; o->checked[3] = meta[4]; o->admitting_pairs = meta[5]; o->exact_pods = t.field[3];
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
  }));
  clock.add(kernel_ms, readback_ms);
  return KS_OK;
}
static int audit_zonefit_run(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_zonefit* const* outs, AuditGate* g) {
  size_t budget = KS_AUDIT_SPREAD_TAB_WORDS;
  if (const char* e = getenv("KS_AUDIT_SPREAD_SLICE_WORDS")) budget = (size_t)strtoull(e, nullptr, 0);      // (the third pass's diagnostic switch: the flags must not depend on it)
  return audit_slices(ds, n, results, outs, g, audit_spread_tab_words, budget, audit_zonefit_slice);
}
extern "C" int ks_audit_zonefit_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_zonefit* const* outs) { return audit_batch(ds, n, outs, true, audit_zonefit_run); }
extern "C" int ks_audit_zonefit_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_zonefit* out) { return audit_one(d, claimed, out, AUD_READS_FIT, true, audit_zonefit_run); }
