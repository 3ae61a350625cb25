// ks_audit_topo.inc -- the audit's second, opt-in pass: pod (anti-)affinity and hostname spread, checked in COMMIT ORDER (ksolve.h ks_audit_topology_dev /
// ks_audit_topology_batch_dev, KS_AUDIT_POD_SEQ .. KS_AUDIT_POD_HOSTNAME_SPREAD).  Included by ksolve.hip after ks_audit.inc, outside the emulator's guards: the
// tests/sim build compiles and runs these kernels too.  ks_audit.inc's kernels, views and outputs are untouched; ks_audit_scan is launched as it is (over this
// pass's own counts), nothing else of the first pass runs here.
//
// The final state alone does not decide these constraints; the final state with the commit numbers (pod_seq) decides the part below soundly, because a topology
// group's domain counts only grow (TopologyGroup.Record, topologygroup.go:101-105) and a node's requirements only narrow (node.go:80,90,103).  Every rule is
// one-sided: it flags only what no run of the reference can have produced (DESIGN.md 7.22 has the argument per rule, and what is not attempted).
// Five launches on the problems' stream, blockIdx.y = the problem:
//   ks_audit_topo_count  one lane per pod: the pods of every node counted (the counting sort's first half), the placed pods counted per commit number (the SEQ rule
//                        compares counts only, so the atomics -- into scratch -- give the same answer every run); `first` set to "never"; the skipped groups counted.
//   ks_audit_scan        ks_audit.inc's: the node -> pods CSR's offsets.
//   ks_audit_topo_order  one lane per pod: its slot in its node's list, and atomicMin of its commit number into first[g][d] for every narrow-key group of type 1 / 2
//                        its class is recorded by, over the bits of its node's mask (a minimum of integers: the same table every run).
//   ks_audit_topo_pods   one lane per pod: SEQ, and the narrow-key rules over own_list / isel_list of the pod's class against `first` and the initial counts.
//   ks_audit_topo_nodes  one wave per node, for the hostname-keyed groups (exact: a node is one domain): the node's pods staged as (seq, class) tiles of 256 in LDS,
//                        each lane takes one constrained pod and walks the tiles, counting the recorders with a smaller commit number.  Four nodes share a
//                        workgroup, and every loop that holds a __syncthreads runs the same number of times in all four waves (sized by the longest list of the four).
//                        The bits join the pod's word by the one lane that holds the pod: a plain read-modify-write, after ks_audit_topo_pods has finished.
struct AuditTopoView {
  u32* flags; u32* chk; u32* meta;      // outputs: [P] KS_AUDIT_POD_SEQ.. | [P] pairs evaluated: bits 0-9 anti-affinity, 10-19 affinity, 20-29 hostname spread, bit 30 the commit number | [4]: n_new, n_unscheduled (ks_audit_scan), skipped groups, placed pods
  u32* seqcnt; u32* first;              // scratch: [P] placed pods per commit number | [G * 64] the least commit number that recorded domain d of group g (type 2: of the certain recorders)
};
#define KS_AT_NEVER 0xFFFFFFFFu
__device__ __forceinline__ bool aud_topo_skipped(const DevProb& P, u32 g) {
  if (!GC(u8, P.grp_active)[g]) return true;
  return GC(i32, P.grp_key)[g] >= 0 && GC(i32, P.grp_count)[(size_t)g * 64] == INT32_MIN;      // (a derived what-if: the group does not exist in it)
}
// an empty node filter: no term, or a term that requires nothing -- what MakeTopologyNodeFilter gives a pod without node selectors, Compatible with every node
// (topologynodefilter.go:30-70; ks_pack's dynamic-spread test reads the same two words)
__device__ __forceinline__ bool aud_topo_unfiltered(const DevProb& P, u32 g) {
  const u32 b = GC(u32, P.grp_filter_off)[g], e = GC(u32, P.grp_filter_off)[g + 1];
  for (u32 f = b; f < e; ++f) if (GC(u32, P.flt.present)[f] == 0 && GC(i32, P.flt.it_state)[f] == 0) return true;
  return b == e;
}
// node nd's final requirement on narrow key k as an In-set: an existing node's label value, a new node's node_mask when the key is present and no complement
__device__ __forceinline__ bool aud_topo_dom(const DevProb& P, const AuditView& V, u32 nd, u32 k, u64* dom) {
  const bool existing = nd < P.E; const u32 j = nd - P.E;
  const u32 pres = existing ? GC(u32, P.en.present)[nd] : GC(u32, V.o_present)[j], comp = existing ? GC(u32, P.en.complement)[nd] : GC(u32, V.o_complement)[j];
  if (!((pres >> k) & 1u) || ((comp >> k) & 1u)) return false;
  *dom = existing ? GC(u64, P.en.mask)[(size_t)nd * P.K + k] : GC(u64, V.o_mask)[(size_t)j * P.K + k];
  return true;
}
// bit d: Requirement.Has(d) on node nd's final requirement on key k; an absent key has every value
__device__ __forceinline__ u64 aud_topo_has(const DevProb& P, const AuditView& V, u32 nd, u32 k) {
  const bool existing = nd < P.E; const u32 j = nd - P.E, K = P.K;
  const u32 pres = existing ? GC(u32, P.en.present)[nd] : GC(u32, V.o_present)[j], comp = existing ? GC(u32, P.en.complement)[nd] : GC(u32, V.o_complement)[j];
  if (!((pres >> k) & 1u)) return ~0ull;
  const KReq r = existing ? load_req(pres, comp, P.en.mask + (size_t)nd * K, P.en.gt + (size_t)nd * K, P.en.lt + (size_t)nd * K, (int)k)
                          : load_req(pres, comp, V.o_mask + (size_t)j * K, V.o_gt + (size_t)j * K, V.o_lt + (size_t)j * K, (int)k);
  return kreq_has_mask(r, P.value_int + k * 64, GC(u32, P.key_nvalues)[k]);
}
// was the requirement of recorder (class c, node nd) on key k a concrete set at its own commit, whatever happened later?
__device__ __forceinline__ bool aud_topo_certain(const DevProb& P, const AuditView& V, u32 c, u32 nd, u32 k) {
  if (nd < P.E) { if (((GC(u32, P.en.present)[nd] >> k) & 1u) && !((GC(u32, P.en.complement)[nd] >> k) & 1u)) return true; }
  else { const i32 m = GC(i32, V.n_tmpl)[nd - P.E]; if (m >= 0 && (u32)m < P.M && ((GC(u32, P.tmpl.present)[m] >> k) & 1u) && !((GC(u32, P.tmpl.complement)[m] >> k) & 1u)) return true; }
  if (((GC(u32, P.cls.present)[c] >> k) & 1u) && !((GC(u32, P.cls.complement)[c] >> k) & 1u)) return true;
  // a group on key k constrains the recorder: its topology requirement made the node concrete (topology.go:160-164).  An owned group exists from the pod's own
  // Topology.Update on; an inverse group that was created later may not have existed yet
  for (u32 i = GC(u32, P.cls_own_off)[c]; i < GC(u32, P.cls_own_off)[c + 1]; ++i) if (GC(i32, P.grp_key)[GC(u32, P.own_list)[i] & 0x7FFFFFFFu] == (i32)k) return true;
  for (u32 i = GC(u32, P.cls_isel_off)[c]; i < GC(u32, P.cls_isel_off)[c + 1]; ++i) { const u32 g = GC(u32, P.isel_list)[i] & 0x7FFFFFFFu; if (GC(i32, P.grp_key)[g] == (i32)k && !aud_topo_skipped(P, g)) return true; }
  return false;
}
// is group g recorded by a pod of class c?  (sel_list: the non-inverse groups that select it; iown_list: the inverse groups it owns -- topology.go:120-142)
__device__ __forceinline__ bool aud_topo_records(const DevProb& P, u32 c, u32 g) {
  for (u32 i = GC(u32, P.cls_sel_off)[c]; i < GC(u32, P.cls_sel_off)[c + 1]; ++i) if (GC(u32, P.sel_list)[i] == g) return true;
  for (u32 i = GC(u32, P.cls_iown_off)[c]; i < GC(u32, P.cls_iown_off)[c + 1]; ++i) if (GC(u32, P.iown_list)[i] == g) return true;
  return false;
}

__global__ __launch_bounds__(256) void ks_audit_topo_count(const DevProb* probs, const AuditView* views, const AuditTopoView* tviews) {
  __shared__ u32 s_skip[256];
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditTopoView& T = tviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), nf = P.G * 64u;
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < np; i += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, i, NS), sq = GC(i32, V.pod_seq)[i];
    if (nd >= 0) { atomicAdd(&V.cnt[nd], 1u); if (sq >= 0 && (u32)sq < np) atomicAdd(&T.seqcnt[sq], 1u); }
  }
  for (u32 i = blockIdx.x * 256u + threadIdx.x; i < nf; i += gridDim.x * 256u) T.first[i] = KS_AT_NEVER;
  if (blockIdx.x == 0) {
    u32 mine = 0;
    for (u32 g = threadIdx.x; g < P.G; g += 256u) if (aud_topo_skipped(P, g)) ++mine;
    aud_block_sum(s_skip, mine);
    if (threadIdx.x == 0) T.meta[2] = s_skip[0];
  }
}
__global__ __launch_bounds__(256) void ks_audit_topo_order(const DevProb* probs, const AuditView* views, const AuditTopoView* tviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditTopoView& T = tviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), n_placed = V.off[NS];
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    const i32 nd = aud_where(P, V, p, NS);
    if (nd < 0) continue;
    V.pods[V.off[nd] + atomicAdd(&V.fill[nd], 1u)] = p;
    if (!aud_seq_ok(V, T.seqcnt, p, n_placed)) continue;
    const u32 c = aud_class(P, V, p), sq = (u32)GC(i32, V.pod_seq)[p];
    const u32 sb = GC(u32, P.cls_sel_off)[c], se = GC(u32, P.cls_sel_off)[c + 1], wb = GC(u32, P.cls_iown_off)[c], we = GC(u32, P.cls_iown_off)[c + 1];
    for (u32 i = 0; i < (se - sb) + (we - wb); ++i) {
      const u32 g = i < se - sb ? GC(u32, P.sel_list)[sb + i] : GC(u32, P.iown_list)[wb + (i - (se - sb))];
      const i32 k = GC(i32, P.grp_key)[g]; const u32 type = GC(u8, P.grp_type)[g];
      if (k < 0 || (u32)k >= P.K || type == 0 || aud_topo_skipped(P, g)) continue;
      u64 bits = 0;
      if (type == 2) { if (!aud_topo_certain(P, V, c, (u32)nd, (u32)k) || !aud_topo_dom(P, V, (u32)nd, (u32)k, &bits)) bits = 0; }      // only a certain recorder's final set is within what Record counted
      else bits = aud_topo_has(P, V, (u32)nd, (u32)k);                                                                                    // every domain the recorder can have counted
      for (; bits; bits &= bits - 1) atomicMin(&T.first[(size_t)g * 64 + (u32)__builtin_ctzll(bits)], sq);
    }
  }
}
__global__ __launch_bounds__(256) void ks_audit_topo_pods(const DevProb* probs, const AuditView* views, const AuditTopoView* tviews) {
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditTopoView& T = tviews[blockIdx.y];
  const u32 np = P.P, NS = P.E + aud_n_new(P, V), n_placed = V.off[NS];
  if (blockIdx.x == 0 && threadIdx.x == 0) T.meta[3] = n_placed;
  for (u32 p = blockIdx.x * 256u + threadIdx.x; p < np; p += gridDim.x * 256u) {
    u32 f = 0, chk = 0;
    const i32 nd = aud_where(P, V, p, NS);
    if (nd >= 0) {
      chk = 1u << 30;
      if (!aud_seq_ok(V, T.seqcnt, p, n_placed)) f = KS_AUDIT_POD_SEQ;
      else {
        const u32 c = aud_class(P, V, p), sq = (u32)GC(i32, V.pod_seq)[p];
        const u32 ob = GC(u32, P.cls_own_off)[c], oe = GC(u32, P.cls_own_off)[c + 1], ib = GC(u32, P.cls_isel_off)[c], ie = GC(u32, P.cls_isel_off)[c + 1];
        for (u32 i = 0; i < (oe - ob) + (ie - ib); ++i) {
          const u32 ent = i < oe - ob ? GC(u32, P.own_list)[ob + i] : (GC(u32, P.isel_list)[ib + (i - (oe - ob))] & 0x7FFFFFFFu);
          const u32 g = ent & 0x7FFFFFFFu, self = ent >> 31;
          const i32 k = GC(i32, P.grp_key)[g]; const u32 type = GC(u8, P.grp_type)[g];
          if (k < 0 || (u32)k >= P.K || type == 0 || (type == 1 && self) || aud_topo_skipped(P, g)) continue;
          const u32 bit = type == 2 ? KS_AUDIT_POD_ANTI_AFFINITY : KS_AUDIT_POD_AFFINITY;
          u64 dom = 0;
          if (!aud_topo_dom(P, V, (u32)nd, (u32)k, &dom)) {
            // its topology requirement made its node concrete on k (topology.go:160-164) -- but an existing node keeps its labels here, and one without a
            // well-known label is Compatible with any requirement on it (requirements.go:123-133): not examined
            if ((u32)nd < P.E && ((P.wellknown_mask >> k) & 1u) && !((GC(u32, P.en.present)[nd] >> k) & 1u)) continue;
            f |= bit; chk += type == 2 ? 1u : 1u << 10; continue;
          }
          chk += type == 2 ? 1u : 1u << 10;
          for (u64 b = dom; b; b &= b - 1) {
            const u32 d = (u32)__builtin_ctzll(b); const i32 init = GC(i32, P.grp_count)[(size_t)g * 64 + d]; const bool earlier = T.first[(size_t)g * 64 + d] < sq;
            if (type == 2 ? (init > 0 || earlier) : (init <= 0 && !earlier)) f |= bit;
          }
        }
      }
    }
    T.flags[p] = f; T.chk[p] = chk;
  }
}
__global__ __launch_bounds__(256) void ks_audit_topo_nodes(const DevProb* probs, const AuditView* views, const AuditTopoView* tviews) {
  __shared__ u32 s_seq[4][256]; __shared__ u32 s_cls[4][256]; __shared__ u32 s_max[4];
  const DevProb& P = probs[blockIdx.y]; const AuditView& V = views[blockIdx.y]; const AuditTopoView& T = tviews[blockIdx.y];
  const u32 lane = threadIdx.x & 63u, wv = threadIdx.x >> 6, E = P.E, NS = E + aud_n_new(P, V), n_placed = V.off[NS];
  if (!P.GH) return;      // (the same in every thread of the launch's row: no hostname-keyed group, nothing to do)
  for (u32 s0 = blockIdx.x * 4u; s0 < NS; s0 += gridDim.x * 4u) {      // (s0 and maxlen are the same in all 256 threads: every wave takes every barrier below)
    u32 maxlen = 0;
    for (u32 w = 0; w < 4u; ++w) if (s0 + w < NS) { const u32 l = V.off[s0 + w + 1] - V.off[s0 + w]; maxlen = l > maxlen ? l : maxlen; }
    const u32 s = s0 + wv; const bool node = s < NS; const u32 b = node ? V.off[s] : 0u, e = node ? V.off[s + 1] : 0u, len = e - b;
    const bool single = maxlen <= 256u;      // the usual case: the node's whole list is one tile, staged once
    if (single) {
      __syncthreads();
      for (u32 t = lane; t < 256u; t += 64u) if (t < len) { const u32 q = V.pods[b + t]; s_seq[wv][t] = aud_seq_ok(V, T.seqcnt, q, n_placed) ? (u32)GC(i32, V.pod_seq)[q] : KS_AT_NEVER; s_cls[wv][t] = aud_class(P, V, q); }
      __syncthreads();
    }
    for (u32 i0 = 0; i0 < maxlen; i0 += 64u) {
      const bool mine = i0 + lane < len; u32 p = 0, c = 0, sq = 0, ob = 0, no = 0, ib = 0, ne = 0;
      if (mine) {
        p = V.pods[b + i0 + lane];
        if (aud_seq_ok(V, T.seqcnt, p, n_placed)) {
          c = aud_class(P, V, p); sq = (u32)GC(i32, V.pod_seq)[p];
          ob = GC(u32, P.cls_own_off)[c]; no = GC(u32, P.cls_own_off)[c + 1] - ob; ib = GC(u32, P.cls_isel_off)[c]; ne = no + (GC(u32, P.cls_isel_off)[c + 1] - ib);
        }
      }
      u32 m = ne; for (int x = 32; x > 0; x >>= 1) { const u32 o = __shfl_xor(m, x); m = o > m ? o : m; }
      if (lane == 0) s_max[wv] = m;
      __syncthreads();
      u32 maxe = s_max[0]; for (u32 w = 1; w < 4u; ++w) maxe = s_max[w] > maxe ? s_max[w] : maxe;
      __syncthreads();
      u32 f = 0, chk = 0;
      for (u32 gi = 0; gi < maxe; ++gi) {
        // this lane's gi-th entry: a hostname-keyed group the rules examine, or nothing
        bool act = false; u32 g = 0, rule = 0; i32 c0 = 0, skew = 0;
        if (gi < ne) {
          const u32 ent = gi < no ? GC(u32, P.own_list)[ob + gi] : (GC(u32, P.isel_list)[ib + (gi - no)] & 0x7FFFFFFFu);
          g = ent & 0x7FFFFFFFu; const u32 self = ent >> 31, type = GC(u8, P.grp_type)[g]; const i32 h = GC(i32, P.grp_hslot)[g];
          if (GC(i32, P.grp_key)[g] == KS_KEY_HOSTNAME && h >= 0 && (u32)h < P.GH && !aud_topo_skipped(P, g)) {
            if (type == 2) { act = true; rule = 2; }
            else if (type == 1) { if (!self) { act = true; rule = 1; } }      // (self-selecting: the bootstrap branch, topologygroup.go:212-231, cannot be told from a violation)
            else if (aud_topo_unfiltered(P, g)) { act = true; rule = 0; skew = GC(i32, P.grp_max_skew)[g]; c0 = (i32)self; }      // (under a node filter Counts depends on the node's requirements at the time)
            if (act && s < E) { const i32 ini = ks_host_count0(P, (u32)h, s); if (ini > 0) c0 += ini; }
          }
        }
        u32 before = 0, lastc = KS_AT_NEVER; bool lastrec = false;
        for (u32 tb = 0; tb < maxlen; tb += 256u) {
          if (!single) {
            __syncthreads();
            for (u32 t = lane; t < 256u; t += 64u) if (tb + t < len) { const u32 q = V.pods[b + tb + t]; s_seq[wv][t] = aud_seq_ok(V, T.seqcnt, q, n_placed) ? (u32)GC(i32, V.pod_seq)[q] : KS_AT_NEVER; s_cls[wv][t] = aud_class(P, V, q); }
            __syncthreads();
          }
          if (act && tb < len) {
            const u32 n = len - tb < 256u ? len - tb : 256u;
            for (u32 t = 0; t < n; ++t) if (s_seq[wv][t] < sq) { const u32 c2 = s_cls[wv][t]; if (c2 != lastc) { lastc = c2; lastrec = aud_topo_records(P, c2, g); } if (lastrec) ++before; }
          }
        }
        if (act) {
          const i64 total = (i64)c0 + (i64)before;
          if (rule == 2) { chk += 1u; if (total > 0) f |= KS_AUDIT_POD_ANTI_AFFINITY; }
          else if (rule == 1) { chk += 1u << 10; if (total == 0) f |= KS_AUDIT_POD_AFFINITY; }
          else { chk += 1u << 20; if (total > (i64)skew) f |= KS_AUDIT_POD_HOSTNAME_SPREAD; }
        }
      }
      if (mine && (f | chk)) { T.flags[p] |= f; T.chk[p] += chk; }
    }
  }
}

// ---- host half ----
// A batch is walked in slices (audit_slices): `first` is G x 64 words per problem (G can exceed 1 024 for what-ifs with per-node group lists), and a slice holds at
// most KS_AUDIT_TOPO_FIRST_WORDS of them (64 MiB), or one problem.
#define KS_AUDIT_TOPO_FIRST_WORDS ((size_t)16 << 20)
// ks_audit.inc's audit_run pattern per slice: scratch laid out, one memset, the launches, one read-back of [meta | flags | chk], the totals counted on the host
static int audit_topo_slice(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_topology* const* outs, AuditGate* g, double* kernel_ms, double* readback_ms) {
  BatchStage st; TRY(st.open(ds, n, nullptr, false));
  const size_t o_view = st.add<AuditView>(n), o_tview = st.add<AuditTopoView>(n);
  TRY(st.place());
  AuditWork W(ds[0]->device); std::vector<size_t> o_fl(n), o_ck(n), o_scr(n); u32 pmax = 0, nsmax = 0;
  W.out(4 * (size_t)n);
  for (u32 i = 0; i < n; ++i) { o_fl[i] = W.out(ds[i]->h.P); o_ck[i] = W.out(ds[i]->h.P); pmax = std::max(pmax, ds[i]->h.P); nsmax = std::max(nsmax, ds[i]->h.E + ds[i]->h.NMAX); }
  for (u32 i = 0; i < n; ++i) o_scr[i] = W.scratch(2 * (size_t)ds[i]->h.P + 3 * ((size_t)ds[i]->h.E + ds[i]->h.NMAX) + 1 + (size_t)ds[i]->h.G * 64);
  TRY(W.alloc());
  u32* w = W.w();
  for (u32 i = 0; i < n; ++i) {
    AuditTopoView t{}; const size_t Pn = ds[i]->h.P, NS = (size_t)ds[i]->h.E + ds[i]->h.NMAX;
    t.meta = w + 4 * (size_t)i; t.flags = w + o_fl[i]; t.chk = w + o_ck[i];
    AuditView v = audit_pass_view(results[i], t.meta);      // (its node -> pods CSR is this pass's own: set below)
    u32* s = w + o_scr[i]; t.seqcnt = s; v.pods = s + Pn; v.cnt = s + 2 * Pn; v.off = s + 2 * Pn + NS; v.fill = s + 2 * Pn + 2 * NS + 1; t.first = s + 2 * Pn + 3 * NS + 1;
    st.h<AuditView>(o_view)[i] = v; st.h<AuditTopoView>(o_tview)[i] = t;
  }
  AuditClock clock;
  TRY(st.upload(st.bytes));
  TRY(W.zero(st.stream()));
  const AuditView* dv = st.d<const AuditView>(o_view); const AuditTopoView* dt = st.d<const AuditTopoView>(o_tview);
  const u32 gx_p = std::max(1u, std::min(1024u, (pmax + 255u) / 256u)), gx_n = std::max(1u, std::min(4096u, (nsmax + 3u) / 4u));
  audit_rows(n, [&](u32 base, u32 ny) {
    hipLaunchKernelGGL(ks_audit_topo_count, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_scan, dim3(ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base);
    hipLaunchKernelGGL(ks_audit_topo_order, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_topo_pods, dim3(gx_p, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
    hipLaunchKernelGGL(ks_audit_topo_nodes, dim3(gx_n, ny), dim3(256), 0, st.stream(), st.probs() + base, dv + base, dt + base);
  });
  const AuditTail tail{4, o_fl.data(), o_ck.data(), nullptr, 4, {30, 0, 10, 20}, {3u, 1023u, 1023u, 1023u}};      // checked[0..3] of a checked word
  TRY(audit_tail(st, W, clock, ds, n, outs, tail, g, [&](u32 i, const AuditTotals& t, const u32* pf, const u32*) {
    ks_audit_topology* o = outs[i]; const u32 Pn = ds[i]->h.P; const u32* meta = t.meta;
    o->n_pods = Pn; o->n_new = meta[0]; o->n_placed = meta[3]; o->skipped_groups = meta[2]; o->n_pods_flagged = t.n_pods_flagged;
    memcpy(o->pod_bit_count, t.pod_bits, sizeof o->pod_bit_count); memcpy(o->checked, t.field, sizeof o->checked);
    if (pf && o->pod_flags && Pn) memcpy(o->pod_flags, pf, (size_t)Pn * sizeof(u32));
  }));
  clock.add(kernel_ms, readback_ms);
  return KS_OK;
}
static int audit_topo_run(ks_dev_problem* const* ds, u32 n, const AuditView* results, ks_audit_topology* const* outs, AuditGate* g) {
  return audit_slices(ds, n, results, outs, g, [](const ks_dev_problem* d) { return (size_t)d->h.G * 64; }, KS_AUDIT_TOPO_FIRST_WORDS, audit_topo_slice);
}
extern "C" int ks_audit_topology_batch_dev(ks_dev_problem* const* ds, uint32_t n, ks_audit_topology* const* outs) { return audit_batch(ds, n, outs, true, audit_topo_run); }
extern "C" int ks_audit_topology_dev(ks_dev_problem* d, const ks_result* claimed, ks_audit_topology* out) { return audit_one(d, claimed, out, AUD_READS_ORDER, true, audit_topo_run); }
