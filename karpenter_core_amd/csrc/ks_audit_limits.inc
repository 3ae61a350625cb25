// ks_audit_limits.inc -- the audit's fifth, opt-in pass: PROVISIONER LIMITS in opening order (ksolve.h ks_audit_limits_dev / ks_audit_limits_batch_dev,
// KS_AUDIT_NODE_LIMIT_*, KS_AUDIT_POD_LIMIT_TEMPLATE).  Included by ksolve.hip after ks_audit_firstfit.inc, outside the emulator's guards: the tests/sim build compiles
// and runs these kernels too.  The four passes' kernels, views and outputs are untouched; their helpers (aud_where, aud_class, aud_n_new, aud_wave_*, aud_fit_*) and
// ks_audit.inc's view of a node and its per-type predicate (AudNode, aud_node_state_meet, aud_node_type_ok) are called as they are, ks_algebra.h is as it was.
//
// Before it opens a machine of a limited provisioner scheduler.add keeps the types whose Capacity is within the remaining resources (scheduler.go:197-206,293-309);
// after the opener's Add it takes the MaxResources of the node's options off them (scheduler.go:215,273-290).  A node's options only shrink, so per limited template,
// in OPENING order, the final options give an upper bound U of the remaining before every opening and the types the opener could have kept give a lower bound L
// (DESIGN.md 7.25 has the argument per clause).  Nine launches on the problems' stream, blockIdx.y = the problem; a problem without a limited template leaves
// every kernel but the first and the last at once:
//   ks_audit_lim_count    one lane per pod: the placed pods counted, and counted per commit number (the second pass's SEQ rule); open[] set to "never".
//   ks_audit_lim_mark     one lane per pod: used[c] = 1 for the class of every examined pod; open[j] = the least (commit number, pod) on new node j (64-bit atomicMin).
//   ks_audit_lim_cap      one wave per new node of a limited template: it is counted, its opening commit number is flagged in seqnode[] (or the template is marked
//                         as holding an unordered node), mc(j) = the MaxResources of its final options, one type per lane and a wave maximum per limited resource.
//   ks_audit_lim_order    one workgroup per (problem, limited template), and one more per problem that compacts used[] (ks_audit_ff_compact's way): the flags per
//                         commit number scanned in 256-wide tiles (ks_audit_scan's tile) give every node its rank among its template's and the template's list in
//                         opening order; then the exclusive, saturating prefix sum of mc over that list, carried across the tiles: U_j.
//   ks_audit_lim_upper    one wave per new node of a limited template: EXTRA (a final option above U_j), whether U_j excludes a type of the template, and for an
//                         ordered template W_j -- filterByRemainingResources by U_j, then the fourth pass's per-type test for the opener alone on a fresh node --
//                         and mw(j), its MaxResources.
//   ks_audit_lim_lower    one workgroup per (problem, ordered limited template): the prefix sum of mw: L_m[0 .. n_m]; the first node whose mw differs from mc.
//   ks_audit_lim_missing  one wave per new node of a limited template: MISSING (a type within L_j that passes the first pass's final-state filter and is not an
//                         option); the node's flag word, one writer, a plain store.
//   ks_audit_lim_pairs    one wave per (used class, ordered limited template): the fourth pass's clauses (aud_fit_new_clauses), then one type per lane: a binary search in
//                         L_m[] per limited resource for the last opening count the type is still within, and a wave maximum.
//   ks_audit_lim_verdict  one lane per pod: its flag word and its checked word, one writer each, a plain store.
// No float, no LDS beyond the reductions' and the scans' tiles, no dynamically indexed register array, no atomic on an output.
#define KS_AL_NEVER64 0xFFFFFFFFFFFFFFFFull
struct AuditLimView {
  u32* pflags; u32* pchk; u32* nflags; u32* meta;      // outputs: [P] KS_AUDIT_POD_SEQ | KS_AUDIT_POD_LIMIT_TEMPLATE | [P] bit 0 examined, bit 29 skipped, bit 30 placed | [E + NMAX] KS_AUDIT_NODE_LIMIT_* | [8]: n_new, placed pods, skipped nodes, nodes examined, pairs evaluated, exact nodes, binding nodes
  i64* mcv; i64* mwv; i64* uv; i64* lv;                // scratch: [NMAX * R] mc(j) | mw(j) | U_j, by node | [(NMAX + M) * R] L_m[k] at row tbase[m] + m + k
  u64* open;                                           // scratch: [NMAX] (the least commit number on new node j) << 32 | the pod that carries it
  u32* seqcnt; u32* used; u32* list; u32* seqnode; u32* rank; u32* ord; u32* nx;      // scratch: [P] placed pods per commit number | [C] as the fourth pass's | [C] | [P] 1 + the node of a limited template that opened at this commit number | [NMAX] the node's rank among its template's | [NMAX] the templates' lists in opening order | [NMAX] bit 0 EXTRA, bit 1 examined
  u32* tcnt; u32* tunord; u32* tbase; u32* kadm; u32* cntr;      // scratch: [M] ordered nodes | [M] the template holds an unordered node | [M] where its list starts in ord[] | [min(C, P) * M] 1 + the largest admitting k | [8] placed pods, used classes, skipped nodes, nodes examined, pairs, exact nodes, binding nodes
  u32 n_limited, pad;                                  // the problem's limited templates (counted on the host when the problem was uploaded)
};
__device__ __forceinline__ i64 aud_lim_sat_add(i64 a, i64 b) { return a > INT64_MAX - b ? INT64_MAX : a + b; }      // (both non-negative)
__device__ __forceinline__ i64 aud_lim_sat_sub(i64 a, i64 b) { return a < INT64_MIN + b ? INT64_MIN : a - b; }      // (b non-negative)
__device__ __forceinline__ i64 aud_lim_wave_max(i64 v) { for (int x = 32; x > 0; x >>= 1) { const i64 o = (i64)aud_xor64((u64)v, x); v = o > v ? o : v; } return v; }
// a fresh node of template m with one pod of class c on it (ks_audit.inc's view)
__device__ __forceinline__ AudNode aud_lim_fresh(const DevProb& P, u32 m, u32 c) { AudNode n = aud_node_fresh(P, m); aud_node_add(P, n, c); return n; }
// Capacity of type t within bound[r] on every limited resource; the bound's rows are global memory
__device__ __forceinline__ bool aud_lim_within(const DevProb& P, u32 lim, u32 t, const i64* bound) {
  for (u32 bits = lim; bits; bits &= bits - 1) { const u32 r = (u32)__builtin_ctz(bits); if (r < P.R && GC(i64, P.it_cap)[(size_t)r * P.T + t] > bound[r]) return false; }
  return true;
}
// a limited template in range for new node j, or -1
__device__ __forceinline__ i32 aud_lim_tmpl(const DevProb& P, const AuditView& V, u32 j) {
  const i32 m = GC(i32, V.n_tmpl)[j];
  if (m < 0 || (u32)m >= P.M || GC(u32, P.tmpl_limit_present)[m] == 0xFFFFFFFFu) return -1;
  return m;
}

__global__ __launch_bounds__(256) void ks_audit_lim_count(const DevProb* probs, const AuditView* views, const AuditLimView* lviews) {
  __shared__ u32 s_sum[256];
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V);
  u32 mine = 0;
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < np; i += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, i, NS), sq = GC(i32, V.pod_seq)[i];
    if (nd < 0) continue;
    ++mine;
    if (sq >= 0 && (u32)sq < np) atomicAdd(&F.seqcnt[sq], 1u);
  }
  aud_block_sum(s_sum, mine);
  if (threadIdx.x == 0 && s_sum[0]) atomicAdd(&F.cntr[0], s_sum[0]);
  if (F.n_limited) for (u32 i = blockIdx.x * 256u + threadIdx.x; i < P.NMAX; i += gridDim.x * 256u) F.open[i] = KS_AL_NEVER64;
}
__global__ __launch_bounds__(256) void ks_audit_lim_mark(const DevProb* probs, const AuditView* views, const AuditLimView* lviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  if (!F.n_limited) return;
  const u32 np = P.P, E = P.E, NS = E + aud_n_new(P, V), n_placed = F.cntr[0];
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    const bool ok = nd >= 0 && aud_seq_ok(V, F.seqcnt, p, n_placed);
    if (!ok && GC(i32, V.pod_node)[p] != -1) continue;      // fails SEQ, or names no node of the result
    if (ok && (u32)nd >= E) atomicMin((unsigned long long*)&F.open[(u32)nd - E], (unsigned long long)(((u64)(u32)GC(i32, V.pod_seq)[p] << 32) | p));
    const u32 c = aud_class(P, V, p);
    if (aud_fit_examinable(P, c)) F.used[c] = 1u;      // (every writer stores 1)
  }
}
__global__ __launch_bounds__(256) void ks_audit_lim_cap(const DevProb* probs, const AuditView* views, const AuditLimView* lviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  if (!F.n_limited) return;
  const u32 lane = threadIdx.x & 63u, NN = aud_n_new(P, V), R = P.R, T = P.T, TW = P.TW;
  for (u32 j = blockIdx.x * 4u + (threadIdx.x >> 6); j < NN; j += gridDim.x * 4u) {      // (j, and everything read through it, is the same in all 64 lanes)
    const i32 mr = GC(i32, V.n_tmpl)[j];
    if (mr < 0 || (u32)mr >= P.M) { if (lane == 0) atomicAdd(&F.cntr[2], 1u); continue; }      // unordered: it belongs to no template
    const i32 m = aud_lim_tmpl(P, V, j);
    if (m < 0) continue;
    const u32 lim = GC(u32, P.tmpl_limit_present)[m]; const u64 o = F.open[j];
    if (lane == 0) {
      atomicAdd(&F.cntr[3], 1u);
      if (o == KS_AL_NEVER64) { atomicAdd(&F.cntr[2], 1u); atomicOr(&F.tunord[m], 1u); }      // unordered: no pod on it has a commit number of its own
      else { F.seqnode[(u32)(o >> 32)] = j + 1u; atomicAdd(&F.tcnt[m], 1u); }      // (commit numbers that pass SEQ are distinct: one writer)
    }
    for (u32 bits = lim; bits; bits &= bits - 1) {
      const u32 r = (u32)__builtin_ctz(bits); if (r >= R) break;
      i64 mx = 0;
      for (u32 tw = 0; tw < TW; ++tw) { const u32 t = tw * 64u + lane; if (t < T && ((GC(u64, V.n_types)[(size_t)j * TW + tw] >> lane) & 1ull)) { const i64 cp = GC(i64, P.it_cap)[(size_t)r * T + t]; mx = cp > mx ? cp : mx; } }
      mx = aud_lim_wave_max(mx);
      if (lane == 0) F.mcv[(size_t)j * R + r] = mx;
    }
  }
}
// the exclusive, saturating prefix sum of val[ord[k] * R + r] over the template's list, k = 0 .. n_m - 1, taken off R0: out(k) receives it; returns the total
template <class Out> __device__ __forceinline__ i64 aud_lim_prefix(i64* s64, const u32* ord, const i64* val, u32 n_m, u32 R, u32 r, i64 r0, Out&& out) {
  const u32 tid = threadIdx.x; i64 carry = 0;
  for (u32 base = 0; base < n_m; base += 256u) {      // (n_m is the same in every lane: every lane walks every tile and every scan step)
    const u32 k = base + tid; const i64 mine = k < n_m ? val[(size_t)ord[k] * R + r] : 0;
    s64[tid] = mine;
    for (u32 o = 1; o < 256u; o <<= 1) {
      __syncthreads();
      const i64 x = tid >= o ? s64[tid - o] : 0;
      __syncthreads();
      s64[tid] = aud_lim_sat_add(s64[tid], x);
    }
    __syncthreads();
    if (k < n_m) out(k, aud_lim_sat_sub(r0, aud_lim_sat_add(carry, tid ? s64[tid - 1] : 0)));
    carry = aud_lim_sat_add(carry, s64[255]);
    __syncthreads();
  }
  return carry;
}
__global__ __launch_bounds__(256) void ks_audit_lim_order(const DevProb* probs, const AuditView* views, const AuditLimView* lviews) {
  __shared__ u32 s_sum[256]; __shared__ i64 s64[256];
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  if (!F.n_limited) return;
  const u32 tid = threadIdx.x, M = P.M, R = P.R;
  if (blockIdx.x >= M) {      // the used classes, compacted (ks_audit_ff_compact)
    if (blockIdx.x > M) return;
    const u32 C = P.C; u32 carry = 0;
    for (u32 base = 0; base < C; base += 256u) {
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
    return;
  }
  const u32 m = blockIdx.x, lim = GC(u32, P.tmpl_limit_present)[m];
  if (lim == 0xFFFFFFFFu) return;
  u32 tb = 0; for (u32 x = 0; x < m; ++x) tb += F.tcnt[x];      // (an unlimited template counts no node)
  if (tid == 0) F.tbase[m] = tb;
  // ---- the flags per commit number, scanned: the rank of every node among its template's, and the template's list in opening order ----
  const u32 n_placed = F.cntr[0], NN = aud_n_new(P, V); u32 carry = 0;
  for (u32 base = 0; base < n_placed; base += 256u) {
    const u32 s = base + tid; u32 j1 = s < n_placed ? F.seqnode[s] : 0u;
    if (j1 && (j1 > NN || GC(i32, V.n_tmpl)[j1 - 1u] != (i32)m)) j1 = 0u;
    s_sum[tid] = j1 ? 1u : 0u;
    for (u32 o = 1; o < 256u; o <<= 1) {
      __syncthreads();
      const u32 x = tid >= o ? s_sum[tid - o] : 0u;
      __syncthreads();
      s_sum[tid] += x;
    }
    __syncthreads();
    if (j1) { const u32 pos = carry + s_sum[tid] - 1u; F.ord[tb + pos] = j1 - 1u; F.rank[j1 - 1u] = pos; }
    carry += s_sum[255];
    __syncthreads();
  }
  const u32 n_m = carry;      // (== tcnt[m])
  __syncthreads();      // (the list is read back below by other lanes of this workgroup)
  // ---- U_j = R0[m] - the mc of the nodes opened before j ----
  for (u32 bits = lim; bits; bits &= bits - 1) {
    const u32 r = (u32)__builtin_ctz(bits); if (r >= R) break;
    const u32* ord = F.ord + tb;
    aud_lim_prefix(s64, ord, F.mcv, n_m, R, r, GC(i64, P.tmpl_remaining)[(size_t)m * R + r], [&](u32 k, i64 v) { F.uv[(size_t)ord[k] * R + r] = v; });
  }
}
__global__ __launch_bounds__(256) void ks_audit_lim_upper(const DevProb* probs, const AuditView* views, const AuditLimView* lviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  if (!F.n_limited) return;
  const u32 lane = threadIdx.x & 63u, NN = aud_n_new(P, V), R = P.R, T = P.T, TW = P.TW;
  for (u32 j = blockIdx.x * 4u + (threadIdx.x >> 6); j < NN; j += gridDim.x * 4u) {      // (j, and everything read through it, is the same in all 64 lanes)
    const i32 m = aud_lim_tmpl(P, V, j);
    if (m < 0) continue;
    const u32 lim = GC(u32, P.tmpl_limit_present)[m]; const u64 o = F.open[j]; const bool ordered = o != KS_AL_NEVER64;
    const i64* U = ordered ? F.uv + (size_t)j * R : P.tmpl_remaining + (size_t)m * R;      // (an unordered node: nothing is known to have opened before it)
    const bool whole = ordered && F.tunord[m] == 0u;      // W_j feeds the lower bound, which an unordered node of the template voids
    AudNode fn{}; u32 si = P.S;
    if (whole) { const u32 c = aud_class(P, V, (u32)o); fn = aud_lim_fresh(P, (u32)m, c); si = aud_node_state_meet(P, fn, c); }
    bool extra = false, binding = false;
    i64 mx[KS_MAX_RES];
#pragma unroll
    for (int r = 0; r < KS_MAX_RES; ++r) mx[r] = 0;
    for (u32 tw = 0; tw < TW; ++tw) {
      const u32 t = tw * 64u + lane; const bool in = t < T;
      const bool tm = in && ((GC(u64, P.tmpl_types)[(size_t)m * TW + tw] >> lane) & 1ull), have = in && ((GC(u64, V.n_types)[(size_t)j * TW + tw] >> lane) & 1ull);
      const bool over = in && !aud_lim_within(P, lim, t, U);
      if (have && over) extra = true;
      if (tm && over) binding = true;
      if (whole && tm && !over && si < P.S && ((GC(u64, P.its_types)[(size_t)si * TW + tw] >> lane) & 1ull) && aud_node_type_ok(P, fn, t)) {      // t is in W_j
#pragma unroll
        for (int r = 0; r < KS_MAX_RES; ++r) if ((u32)r < R) { const i64 cp = GC(i64, P.it_cap)[(size_t)r * T + t]; mx[r] = cp > mx[r] ? cp : mx[r]; }
      }
    }
    const bool any_extra = ballot64(extra) != 0, any_binding = ballot64(binding) != 0;
    if (whole) {
#pragma unroll
      for (int r = 0; r < KS_MAX_RES; ++r) if ((u32)r < R && ((lim >> r) & 1u)) { const i64 v = aud_lim_wave_max(mx[r]); if (lane == 0) F.mwv[(size_t)j * R + r] = v; }
    }
    if (lane == 0) { F.nx[j] = (any_extra ? 1u : 0u) | 2u; if (any_binding) atomicAdd(&F.cntr[6], 1u); }
  }
}
__global__ __launch_bounds__(256) void ks_audit_lim_lower(const DevProb* probs, const AuditLimView* lviews) {
  __shared__ u32 s_min[256]; __shared__ i64 s64[256];
  const DevProb& P = probs[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  if (!F.n_limited || blockIdx.x >= P.M) return;
  const u32 tid = threadIdx.x, m = blockIdx.x, R = P.R, lim = GC(u32, P.tmpl_limit_present)[m];
  if (lim == 0xFFFFFFFFu || F.tunord[m]) return;
  const u32 n_m = F.tcnt[m], tb = F.tbase[m]; const u32* ord = F.ord + tb; i64* L = F.lv + ((size_t)tb + m) * R;
  for (u32 bits = lim; bits; bits &= bits - 1) {
    const u32 r = (u32)__builtin_ctz(bits); if (r >= R) break;
    const i64 r0 = GC(i64, P.tmpl_remaining)[(size_t)m * R + r];
    const i64 total = aud_lim_prefix(s64, ord, F.mwv, n_m, R, r, r0, [&](u32 k, i64 v) { L[(size_t)k * R + r] = v; });
    if (tid == 0) L[(size_t)n_m * R + r] = aud_lim_sat_sub(r0, total);
  }
  // ---- the nodes up to the first whose mw differs from mc are exact: there L_j == U_j ----
  u32 first = n_m;
  for (u32 k = tid; k < n_m; k += 256u) {
    const u32 j = ord[k]; bool diff = false;
    for (u32 bits = lim; bits; bits &= bits - 1) { const u32 r = (u32)__builtin_ctz(bits); if (r < R && F.mcv[(size_t)j * R + r] != F.mwv[(size_t)j * R + r]) diff = true; }
    if (diff && k < first) first = k;
  }
  s_min[tid] = first;
  for (u32 o = 128u; o > 0; o >>= 1) { __syncthreads(); if (tid < o) s_min[tid] = s_min[tid + o] < s_min[tid] ? s_min[tid + o] : s_min[tid]; }
  if (tid == 0) { const u32 ex = s_min[0] + 1u < n_m ? s_min[0] + 1u : n_m; if (ex) atomicAdd(&F.cntr[5], ex); }
}
__global__ __launch_bounds__(256) void ks_audit_lim_missing(const DevProb* probs, const AuditView* views, const AuditLimView* lviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  if (!F.n_limited) return;
  const u32 lane = threadIdx.x & 63u, E = P.E, NN = aud_n_new(P, V), R = P.R, T = P.T, TW = P.TW;
  for (u32 j = blockIdx.x * 4u + (threadIdx.x >> 6); j < NN; j += gridDim.x * 4u) {      // (wave-uniform)
    const i32 m = aud_lim_tmpl(P, V, j);
    if (m < 0) continue;
    const u32 lim = GC(u32, P.tmpl_limit_present)[m]; u32 f = (F.nx[j] & 1u) ? KS_AUDIT_NODE_LIMIT_EXTRA : 0u;
    const i32 its = GC(i32, V.o_it)[j];
    if (F.open[j] != KS_AL_NEVER64 && F.tunord[m] == 0u && its >= 0 && (u32)its < P.S) {
      const i64* L = F.lv + ((size_t)F.tbase[m] + m + F.rank[j]) * R;
      AudNode fn = aud_node_final(P, V, j);
      aud_node_pairs(P, fn);
      bool missing = false;
      for (u32 tw = 0; tw < TW; ++tw) {
        const u32 t = tw * 64u + lane;
        if (t < T && ((GC(u64, P.tmpl_types)[(size_t)m * TW + tw] >> lane) & 1ull) && !((GC(u64, V.n_types)[(size_t)j * TW + tw] >> lane) & 1ull) &&
            ((GC(u64, P.its_types)[(size_t)its * TW + tw] >> lane) & 1ull) && aud_lim_within(P, lim, t, L) && aud_node_type_ok(P, fn, t)) missing = true;
      }
      if (ballot64(missing)) f |= KS_AUDIT_NODE_LIMIT_MISSING;
    }
    if (lane == 0) F.nflags[E + j] = f;
  }
}
__global__ __launch_bounds__(256) void ks_audit_lim_pairs(const DevProb* probs, const AuditLimView* lviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  if (!F.n_limited) return;
  const u32 lane = threadIdx.x & 63u, M = P.M, R = P.R, T = P.T, TW = P.TW, n_used = F.cntr[1];
  const size_t total = (size_t)n_used * M;
  for (size_t w = (size_t)blockIdx.x * 4u + (threadIdx.x >> 6); w < total; w += (size_t)gridDim.x * 4u) {      // (w, and everything read through it, is the same in all 64 lanes)
    const u32 u = (u32)(w / M), m = (u32)(w % M), c = F.list[u], lim = GC(u32, P.tmpl_limit_present)[m];
    if (lim == 0xFFFFFFFFu || F.tunord[m]) continue;
    const u32 n_m = F.tcnt[m]; const i64* L = F.lv + ((size_t)F.tbase[m] + m) * R;
    // ---- admits_template: the fourth pass's clauses and state meet, then a walk of this kernel's own ----
    AudNode fn = aud_node_fresh(P, m);
    const u32 si = aud_fit_new_clauses(P, fn, c) ? aud_node_state_meet(P, fn, c) : P.S;
    i32 best = -1;
    if (si < P.S) {
      aud_node_add(P, fn, c);
      for (u32 tw = 0; tw < TW; ++tw) {
        const u32 t = tw * 64u + lane;
        if (!(t < T && ((GC(u64, P.tmpl_types)[(size_t)m * TW + tw] >> lane) & 1ull) && ((GC(u64, P.its_types)[(size_t)si * TW + tw] >> lane) & 1ull) && aud_node_type_ok(P, fn, t))) continue;
        i32 kt = (i32)n_m;      // the last opening count at which t is within L_m[k] on every limited resource (L_m falls with k)
        for (u32 bits = lim; bits && kt >= 0; bits &= bits - 1) {
          const u32 r = (u32)__builtin_ctz(bits); if (r >= R) break;
          const i64 cap = GC(i64, P.it_cap)[(size_t)r * T + t];
          if (cap > L[r]) { kt = -1; break; }
          u32 lo = 0, hi = (u32)kt;      // L[lo] admits; the answer is in [lo, hi]
          while (lo < hi) { const u32 mid = lo + (hi - lo + 1u) / 2u; if (cap <= L[(size_t)mid * R + r]) lo = mid; else hi = mid - 1u; }
          kt = (i32)lo;
        }
        best = kt > best ? kt : best;
      }
      for (int x = 32; x > 0; x >>= 1) { const i32 o = __shfl_xor(best, x); best = o > best ? o : best; }
    }
    if (lane == 0) { atomicAdd(&F.cntr[4], 1u); F.kadm[(size_t)u * M + m] = (u32)(best + 1); }
  }
}
__global__ __launch_bounds__(256) void ks_audit_lim_verdict(const DevProb* probs, const AuditView* views, const AuditLimView* lviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditLimView& F = lviews[blockIdx.y];
  const u32 np = P.P, E = P.E, M = P.M, NS = E + aud_n_new(P, V), n_placed = F.cntr[0];
  if (blockIdx.x == 0 && threadIdx.x == 0) { F.meta[0] = aud_n_new(P, V); F.meta[1] = n_placed; F.meta[2] = F.cntr[2]; F.meta[3] = F.cntr[3]; F.meta[4] = F.cntr[4]; F.meta[5] = F.cntr[5]; F.meta[6] = F.cntr[6]; }
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    const bool ok = nd >= 0 && aud_seq_ok(V, F.seqcnt, p, n_placed), unsched = GC(i32, V.pod_node)[p] == -1;
    u32 f = (nd >= 0 && !ok) ? KS_AUDIT_POD_SEQ : 0u; const u32 chk = nd >= 0 ? 1u << 30 : 0u;
    if (!F.n_limited) { F.pflags[p] = f; F.pchk[p] = chk; continue; }
    const u32 c = aud_class(P, V, p);
    const u32 u1 = F.used[c];      // (ks_audit_lim_mark marked the class of every examined pod: never 0 for one)
    if (!(ok || unsched) || !aud_fit_examinable(P, c) || !u1) { F.pflags[p] = f; F.pchk[p] = chk | (1u << 29); continue; }
    const u32 u = u1 - 1u;
    if (unsched) {      // the end state bounds every attempt: remaining only falls
      for (u32 m = 0; m < M; ++m) if (GC(u32, P.tmpl_limit_present)[m] != 0xFFFFFFFFu && !F.tunord[m] && F.kadm[(size_t)u * M + m] >= F.tcnt[m] + 1u) f |= KS_AUDIT_POD_LIMIT_TEMPLATE;
    } else if ((u32)nd >= E) {
      const u32 j = (u32)nd - E, sq = (u32)GC(i32, V.pod_seq)[p]; const i32 mine = GC(i32, V.n_tmpl)[j];
      if ((u32)(F.open[j] >> 32) == sq && mine >= 0 && (u32)mine < M) {      // the opener of its node: the templates before its own were tried first
        for (u32 m = 0; m < (u32)mine; ++m) {
          if (GC(u32, P.tmpl_limit_present)[m] == 0xFFFFFFFFu || F.tunord[m]) continue;
          const u32* ord = F.ord + F.tbase[m]; u32 lo = 0, hi = F.tcnt[m];      // k = the openings of m before sq: the list is in opening order
          while (lo < hi) { const u32 mid = (lo + hi) / 2u; if ((u32)(F.open[ord[mid]] >> 32) < sq) lo = mid + 1u; else hi = mid; }
          if (F.kadm[(size_t)u * M + m] >= lo + 1u) f |= KS_AUDIT_POD_LIMIT_TEMPLATE;
        }
      }
    }
    F.pflags[p] = f; F.pchk[p] = chk | 1u;
  }
}

// ---- host half ----
// One pooled block [meta | pod flags | checked words | node flags | scratch], one memset, the launches, one read-back, the totals counted on the host.
static int audit_limits_run(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_limits* const* outs, AuditGate* g) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n), o_lview = st.add<AuditLimView>(n);
  TRY(st.place());
  AuditWork W(ds[0]->device); std::vector<size_t> o_fl(n), o_ck(n), o_nf(n), o_scr(n); u32 pmax = 0, nnmax = 1, mmax = 0; size_t prmax = 1; bool any_limited = false;
  W.out(8 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { const DevProb& h = ds[i]->h; o_fl[i] = W.out(h.P); o_ck[i] = W.out(h.P); o_nf[i] = W.out((size_t)h.E + h.NMAX); pmax = std::max(pmax, h.P); }
  for (u32 i = 0; i < n; ++i) {
    const DevProb& h = ds[i]->h;      // (the int64 tables come first in the scratch: 8-byte aligned)
    if (!ds[i]->n_limited) { o_scr[i] = W.scratch((size_t)h.P + 8, true); continue; }      // (SEQ alone: the counts per commit number and the counters)
    any_limited = true;
    const size_t used = std::min<size_t>(h.C, h.P), NM = h.NMAX, R = h.R;
    o_scr[i] = W.scratch(2 * (3 * NM * R + (NM + h.M) * R + NM) + 2 * (size_t)h.P + 2 * (size_t)h.C + 3 * NM + 3 * (size_t)h.M + used * h.M + 8, true);
    nnmax = std::max(nnmax, h.NMAX); mmax = std::max(mmax, h.M); prmax = std::max(prmax, (used * h.M + 3) / 4);
  }
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditLimView t{}; const DevProb& h = ds[i]->h; const size_t Pn = h.P, Cn = h.C, NM = h.NMAX, R = h.R, Mn = h.M;
    t.meta = w + 8 * (size_t)i; t.pflags = w + o_fl[i]; t.pchk = w + o_ck[i]; t.nflags = w + o_nf[i]; t.n_limited = ds[i]->n_limited;
    u32* s = w + o_scr[i];
    if (!t.n_limited) { t.seqcnt = s; s += Pn; t.cntr = s; }
    else {
      t.mcv = (i64*)s; s += 2 * NM * R; t.mwv = (i64*)s; s += 2 * NM * R; t.uv = (i64*)s; s += 2 * NM * R; t.lv = (i64*)s; s += 2 * (NM + Mn) * R; t.open = (u64*)s; s += 2 * NM;
      t.seqcnt = s; s += Pn; t.seqnode = s; s += Pn; t.used = s; s += Cn; t.list = s; s += Cn; t.rank = s; s += NM; t.ord = s; s += NM; t.nx = s; s += NM;
      t.tcnt = s; s += Mn; t.tunord = s; s += Mn; t.tbase = s; s += Mn; t.kadm = s; s += std::min<size_t>(Cn, Pn) * Mn; t.cntr = s;
    }
    st.h<AuditView>(o_view)[i] = audit_pass_view(results[i], t.meta); st.h<AuditLimView>(o_lview)[i] = t;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view); const AuditLimView* df = st.d<const AuditLimView>(o_lview);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_n = std::max(1u, std::min(4096u, (nnmax + 3u) / 4u)), gx_r = (u32)std::min<size_t>(4096, prmax);
  audit_rows(n, [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_lim_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
    if (any_limited) {      // (no limited template anywhere in the batch: SEQ alone)
      hipLaunchKernelGGL(ks_audit_lim_mark, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
      hipLaunchKernelGGL(ks_audit_lim_cap, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
      hipLaunchKernelGGL(ks_audit_lim_order, dim3(mmax + 1u, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
      hipLaunchKernelGGL(ks_audit_lim_upper, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
      hipLaunchKernelGGL(ks_audit_lim_lower, dim3(mmax, ny), dim3(256), 0, st.stream(), st.probs() + base, df + base);
      hipLaunchKernelGGL(ks_audit_lim_missing, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
      hipLaunchKernelGGL(ks_audit_lim_pairs, dim3(gx_r, ny), dim3(256), 0, st.stream(), st.probs() + base, df + base);
    }
    hipLaunchKernelGGL(ks_audit_lim_verdict, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, df + base);
  });
  const AuditTail tail{8, o_fl.data(), o_ck.data(), o_nf.data(), 3, {30, 0, 29, 0}, {3u, 1u, 1u, 0u}};      // checked[0], checked[2], skipped_pods of a checked word
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32* nf) {
    ks_audit_limits* o = outs[i]; const u32 Pn = ds[i]->h.P; const u32* meta = t.meta; const u32 NS = ds[i]->h.E + meta[0];
    o->n_pods = Pn; o->n_nodes = NS; o->n_new = meta[0]; o->n_placed = meta[1]; o->limited_templates = ds[i]->n_limited; o->skipped_nodes = meta[2]; o->skipped_pods = t.field[2];
    o->n_pods_flagged = t.n_pods_flagged; o->n_nodes_flagged = t.n_nodes_flagged; o->checked[0] = t.field[0]; o->checked[1] = meta[3]; o->checked[2] = t.field[1]; o->checked[3] = meta[4]; o->exact_nodes = meta[5]; o->binding_nodes = meta[6];
    memcpy(o->pod_bit_count, t.pod_bits, sizeof o->pod_bit_count); memcpy(o->node_bit_count, t.node_bits, sizeof o->node_bit_count);
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
    if (nf && o->node_flags && NS) memcpy(o->node_flags, nf, (size_t)NS * sizeof(u32));
  }));
  clock.store(outs, n);
  return KS_OK;
}
extern "C" int ks_audit_limits_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_limits* const* outs) { return audit_batch(ds, n, outs, true, audit_limits_run); }
extern "C" int ks_audit_limits_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_limits* out) { return audit_one(d, claimed, out, AUD_READS_FIT, true, audit_limits_run); }
