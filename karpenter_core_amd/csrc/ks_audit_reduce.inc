// ks_audit_reduce.inc -- the audit's GATE on the device (ksolve.h ks_audit_gate_dev / ks_audit_gate_batch_dev / ks_audit_reduce_rows): the flag tables a pass left
// in its work block are tallied where they lie, and their non-zero words compacted into a list of findings, so that a caller who asks "is it clean?" reads back the
// totals and never a row.  Included by ksolve.hip after ks_audit.inc's device half and before its host half's users, outside the emulator's guards: the tests/sim
// build compiles and runs these kernels too.
//
// A pass hands over one AuditRedProb per problem: where its meta words, its pod flags, its node flags (or none) and its checked words (or none) lie, and the bit
// fields of a checked word that its totals sum.  Every problem has KS_AR_TABS tables -- 0 the pod flags, 1 the node flags, 2 the checked words; an absent one has no
// rows -- and a table is cut into gridDim.x runs of consecutive rows, whole tiles of 256 (as many runs as the longest table of the call has tiles, at most
// KS_AR_MAX_RUNS), one workgroup each: blockIdx.y = the table, blockIdx.x = the run.  Four launches on the problems' stream:
//   ks_audit_tally         one workgroup per (table, run).  A flag table: 32 ballots per 64 rows give the wave's count of every bit, lane b keeps bit b's and lane 32
//                          the non-zero rows'; the four waves' counts meet in LDS.  A checked table: every lane sums its rows' fields, aud_block_sum adds them up.
//                          The run's KS_AR_W sums go to the partial table: a plain store per word.
//   ks_audit_tally_finish  one workgroup per problem: lane w adds word w over the runs of each table (the second step), and the totals' block of the problem is
//                          [meta | pods: bits, rows set | nodes: bits, rows set | fields] -- what the host reads back.
//   ks_audit_find_scan     one workgroup: the exclusive scan of the runs' non-zero counts over all flag tables in the order (problem, table, run) = where each run's
//                          findings begin (ks_audit_scan's Hillis-Steele over an LDS tile).  The findings before this launch sequence are the scan's first carry.
//   ks_audit_find_scatter  one workgroup per (flag table, run) that has findings below the cap: per 256 rows an LDS scan of the non-zero marks, one 16-byte record
//                          per non-zero row at its place in the list.  The place comes from the scans, never from an atomic: the list is the same every run.
// A node table's length is E + meta[0]: the pass's own kernels left n_new there, and the kernels here read it there (bounded by the table's capacity).
#define KS_AR_TABS 3u
#define KS_AR_MAX_RUNS 64u                               // the most workgroups on one table
#define KS_AR_W 37u                                      // a run's sums: [0, 32) the bits | 32 the rows set | [33, 37) the fields
#define KS_AR_META 8u                                    // the most meta words a pass keeps per problem
#define KS_AR_TOT (KS_AR_META + 33u + 33u + 4u)          // a problem's totals: [meta | pods: bits, rows set | nodes: bits, rows set | fields]
struct AuditRedProb {
  const u32* meta; const u32* pod_flags; const u32* node_flags; const u32* chk;      // node_flags, chk: null where the pass has none
  u32 n_meta, P, E, NMAX;                                                              // pod_flags, chk: [P] | node_flags: [E + min(meta[0], NMAX)]
  u32 n_fields, shift[4], mask[4];                                                     // the totals' fields of a checked word: (chk >> shift) & mask
  u32 problem, where;                                                                  // a finding's first two words: the problem's position in the batch | pass << 8 (| table)
};
struct AuditRedView { const AuditRedProb* probs; u32* part; u32* fbase; u32* tot; ks_audit_finding* find; u32 n, runs, cap, before; };
__device__ __forceinline__ const u32* aud_red_rows(const AuditRedProb& D, u32 tab, u32* len) {
  if (tab == 0u) { *len = D.pod_flags ? D.P : 0u; return D.pod_flags; }
  if (tab == 2u) { *len = D.chk ? D.P : 0u; return D.chk; }
  if (!D.node_flags) { *len = 0u; return nullptr; }
  const u32 nn = D.meta[0]; *len = D.E + (nn < D.NMAX ? nn : D.NMAX);
  return D.node_flags;
}
// run r of `runs` over a table of len rows: [*b, *e), whole tiles of 256 but for the table's end
__device__ __forceinline__ void aud_red_run(u32 len, u32 runs, u32 r, u32* b, u32* e) {
  const u32 per = ((len + runs - 1u) / runs + 255u) & ~255u; const u64 at = (u64)r * per;
  *b = at < len ? (u32)at : len; *e = at + per < len ? (u32)(at + per) : len;
}

__global__ __launch_bounds__(256) void ks_audit_tally(AuditRedView V, u32 first) {
  __shared__ u32 s[256];
  const u32 tab = first * KS_AR_TABS + blockIdx.y, t = tab % KS_AR_TABS, tid = threadIdx.x, lane = tid & 63u;
  const AuditRedProb& D = V.probs[tab / KS_AR_TABS];
  u32 len; const u32* rows = aud_red_rows(D, t, &len);
  u32 b, e; aud_red_run(len, V.runs, blockIdx.x, &b, &e);      // (b, e: the same in every lane -- every lane walks every tile, every ballot is a whole wave's)
  u32* out = V.part + ((size_t)tab * V.runs + blockIdx.x) * KS_AR_W;
  if (t != 2u) {
    u32 mine = 0;
    for (u32 base = b; base < e; base += 256u) {
      const u32 i = base + tid; const u32 w = i < e ? rows[i] : 0u;
      const u64 nz = __ballot(w != 0u);
      if (!nz) continue;
      if (lane == 32u) mine += (u32)__builtin_popcountll(nz);
#pragma unroll
      for (u32 k = 0; k < 32u; ++k) { const u64 m = __ballot((w >> k) & 1u); if (lane == k) mine += (u32)__builtin_popcountll(m); }
    }
    s[tid] = mine;
    __syncthreads();
    if (tid < 33u) out[tid] = s[tid] + s[tid + 64u] + s[tid + 128u] + s[tid + 192u];
    else if (tid < KS_AR_W) out[tid] = 0u;
    return;
  }
  u32 f0 = 0, f1 = 0, f2 = 0, f3 = 0; const u32 nf = D.n_fields;
  for (u32 i = b + tid; i < e; i += 256u) {
    const u32 w = rows[i];
    f0 += (w >> D.shift[0]) & D.mask[0]; f1 += (w >> D.shift[1]) & D.mask[1]; f2 += (w >> D.shift[2]) & D.mask[2]; f3 += (w >> D.shift[3]) & D.mask[3];
  }
  if (tid < 33u) out[tid] = 0u;
  aud_block_sum(s, nf > 0u ? f0 : 0u); if (tid == 0) out[33] = s[0]; __syncthreads();
  aud_block_sum(s, nf > 1u ? f1 : 0u); if (tid == 0) out[34] = s[0]; __syncthreads();
  aud_block_sum(s, nf > 2u ? f2 : 0u); if (tid == 0) out[35] = s[0]; __syncthreads();
  aud_block_sum(s, nf > 3u ? f3 : 0u); if (tid == 0) out[36] = s[0];
}
__global__ __launch_bounds__(64) void ks_audit_tally_finish(AuditRedView V) {
  const u32 i = blockIdx.x, w = threadIdx.x; const AuditRedProb& D = V.probs[i];
  u32* tot = V.tot + (size_t)i * KS_AR_TOT;
  if (w < KS_AR_META) tot[w] = w < D.n_meta ? D.meta[w] : 0u;
  if (w >= KS_AR_W) return;
  const u32* p = V.part + (size_t)i * KS_AR_TABS * V.runs * KS_AR_W + w;
  u32 sum[KS_AR_TABS];
#pragma unroll
  for (u32 t = 0; t < KS_AR_TABS; ++t) { sum[t] = 0; for (u32 r = 0; r < V.runs; ++r) sum[t] += p[((size_t)t * V.runs + r) * KS_AR_W]; }
  if (w < 33u) { tot[KS_AR_META + w] = sum[0]; tot[KS_AR_META + 33u + w] = sum[1]; }
  else tot[KS_AR_META + 66u + (w - 33u)] = sum[2];
}
__global__ __launch_bounds__(256) void ks_audit_find_scan(AuditRedView V) {
  __shared__ u32 s_sum[256];
  const u32 tid = threadIdx.x, total = V.n * KS_AR_TABS * V.runs; u32 carry = V.before;
  for (u32 base = 0; base < total; base += 256u) {      // (total is a kernel argument: every lane walks every tile and every scan step)
    const u32 i = base + tid; const u32 mine = (i < total && (i / V.runs) % KS_AR_TABS != 2u) ? V.part[(size_t)i * KS_AR_W + 32u] : 0u;
    s_sum[tid] = mine;
    for (u32 o = 1; o < 256u; o <<= 1) {
      __syncthreads();
      const u32 x = tid >= o ? s_sum[tid - o] : 0u;
      __syncthreads();
      s_sum[tid] += x;
    }
    __syncthreads();
    if (i < total) V.fbase[i] = carry + s_sum[tid] - mine;
    carry += s_sum[255];
    __syncthreads();
  }
}
__global__ __launch_bounds__(256) void ks_audit_find_scatter(AuditRedView V, u32 first) {
  __shared__ u32 s_sum[256];
  const u32 tab = first * KS_AR_TABS + blockIdx.y, t = tab % KS_AR_TABS, tid = threadIdx.x;
  if (t == 2u) return;
  const size_t run = (size_t)tab * V.runs + blockIdx.x;
  u32 at = V.fbase[run];      // (the run's count and place are read from one address by every lane: the workgroup leaves as one, or walks every tile and every scan step as one)
  if (V.part[run * KS_AR_W + 32u] == 0u || at >= V.cap) return;
  const AuditRedProb& D = V.probs[tab / KS_AR_TABS];
  u32 len; const u32* rows = aud_red_rows(D, t, &len);
  u32 b, e; aud_red_run(len, V.runs, blockIdx.x, &b, &e);
  for (u32 base = b; base < e && at < V.cap; base += 256u) {
    const u32 i = base + tid; const u32 w = i < e ? rows[i] : 0u; const u32 mine = w != 0u ? 1u : 0u;
    s_sum[tid] = mine;
    for (u32 o = 1; o < 256u; o <<= 1) {
      __syncthreads();
      const u32 x = tid >= o ? s_sum[tid - o] : 0u;
      __syncthreads();
      s_sum[tid] += x;
    }
    __syncthreads();
    const u32 pos = at + s_sum[tid] - mine;
    if (mine && pos < V.cap) { ks_audit_finding r; r.problem = D.problem; r.where = D.where | t; r.index = i; r.flags = w; V.find[pos] = r; }
    at += s_sum[255];
    __syncthreads();
  }
}
