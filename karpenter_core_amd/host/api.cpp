// api.cpp -- C entry points of libkshost.so: the host-side mirror of the reference call sites
//   scheduler := provisioner.NewScheduler(ctx, pods, stateNodes, opts)   (provisioner.go:301, helpers.go:85)
//   nodes, existing, err := scheduler.Solve(ctx, pods)                   (provisioner.go:307, helpers.go:93)
// ksh_open == NewScheduler (+NewTopology) + flattening + upload; ksh_solve == Solve through the
// libksolve C ABI (HIP kernels).  There is no CPU scheduling path in this library.
#include <atomic>
#include <mutex>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <thread>
#include <type_traits>
#include <unordered_map>

#include "encode.hpp"

// The caller's objects in memory.  A cluster snapshot additionally keeps its flattening (ksh::SnapshotBase) once a what-if batch asked for
// it: a consolidation pass probes many candidate sets against the same snapshot (multinodeconsolidation.go:86-114 binary search,
// singlenodeconsolidation.go:54 scan), and everything that does not depend on the candidate set is flattened once.
struct Parsed {
  std::shared_ptr<const ksp::Problem> pr;
  std::mutex mu; std::shared_ptr<const ksh::SnapshotBase> sb; std::vector<int32_t> sb_pod_node; uint32_t sb_flags = 0;
  ksh::EnvCache env;      // the flattening of everything but the pods, reused by the next batch with the same universe signature
  std::shared_ptr<const void> cmd_nodes;      // what the consolidation commands read of the nodes' labels (CmdSnapshot below), made once; ksh_env_apply* drops it
  std::shared_ptr<const void> cand_nodes;     // what candidate selection reads of them (CandSnapshot below), likewise
  // ksh_env_apply (round 6): once events were applied the library holds the bindings itself -- bind[i] = the node pod i is bound to, -1 for a pod that was unbound
  // (it stays in place: nothing that points into the problem may move) -- and the names of what is alive
  std::unordered_map<std::string, uint32_t> type_index;      // instance-type name -> index, made by the first IT= event (types are never added, removed or renamed)
  bool bind_set = false, had_cluster_pods = false; std::vector<int32_t> bind; std::unordered_map<std::string, uint32_t> live_node, live_pod; uint64_t tombstones = 0; uint32_t applied = 0;
};
namespace {
// A batch of what-ifs derived on the device (ks_whatifs_open): the arena, the resident snapshot it points into and what the candidate sets were
struct DeltaBatch {
  ks_whatif_batch* b = nullptr; std::shared_ptr<void> base_dev; std::shared_ptr<const ksh::SnapshotBase> sb; std::vector<uint32_t> cand_off, cand;
  ~DeltaBatch() { if (b) ks_whatifs_free(b); }
};
struct Handle {
  std::unique_ptr<ksh::Encoded> enc; ks_dev_problem* dev = nullptr; std::unique_ptr<ksh::Encoded::ResultBuf> rb;
  std::shared_ptr<DeltaBatch> delta; uint32_t delta_index = 0;      // a derived what-if: `dev` is a view the batch owns; result pod ids follow the snapshot's queue order
  std::shared_ptr<void> base_dev;      // what-ifs over a snapshot: the snapshot's own flattening, resident on the device (shared catalogue + derived tables)
  bool solved = false;                 // rb holds the result of a successful solve (the result buffers are raw memory until then)
  bool dev_result = false;             // the device holds the result of a successful solve (price filter / launch pick / records read it there)
  bool snapshot_whatif = false;        // a what-if over a cluster snapshot (ksh_open_whatifs* / ksh_open_whatifs_derived): ksh_placement_rows renames its rows to the snapshot's ids.  Said by the calls that open one, never inferred: a Solve flattened over the environment cache shares an Encoded and names a source problem too
  std::vector<uint32_t> pod_ids;       // a what-if flattened by itself over a snapshot: batch pod i is the snapshot's pod pod_ids[i] (candidate order, then pod order; ksh_placement_rows names pods by it)
  std::vector<uint32_t> csr_off; std::vector<int32_t> csr_pods;      // ksh_result_arrays: the pods of every node in commit order (built on demand from pod_seq)
  ~Handle() { if (dev && !delta) ks_problem_free(dev); }
};
// KSR1 text of the result in h->rb.  A derived what-if numbers its pods in the snapshot's queue order; callers number a what-if's pods in
// candidate order, then pod order (ksh_open_whatifs): translate before decoding.
static std::string decode_handle(Handle* h, double dt) {
  if (!h->delta) return h->enc->decode(h->rb->r, dt);
  const DeltaBatch& D = *h->delta; const ksh::DeltaInputs in = ksh::delta_inputs(*D.sb); const uint32_t w = h->delta_index;
  std::vector<std::pair<uint32_t, uint32_t>> byrank;      // (rank in the snapshot's queue, candidate-order index)
  for (uint32_t i = D.cand_off[w]; i < D.cand_off[w + 1]; ++i) for (uint32_t p : (*in.by_node)[D.cand[i]]) byrank.push_back({in.pod_rank[p], (uint32_t)byrank.size()});
  std::sort(byrank.begin(), byrank.end());
  const uint32_t P = (uint32_t)byrank.size(); const ks_result& r = h->rb->r;
  std::vector<int32_t> pn(P + 1), ps(P + 1), pq(P + 1), un(P + 1); std::vector<uint32_t> pr(P + 1);
  for (uint32_t k = 0; k < P; ++k) { const uint32_t c = byrank[k].second; pn[c] = r.pod_node[k]; ps[c] = r.pod_stage[k]; pq[c] = r.pod_seq[k]; pr[c] = r.pod_reason[k]; }
  for (uint32_t i = 0; i < r.n_unscheduled; ++i) un[i] = (int32_t)byrank[(uint32_t)r.unscheduled[i]].second;
  ks_result t = r; t.pod_node = pn.data(); t.pod_stage = ps.data(); t.pod_seq = pq.data(); t.pod_reason = pr.data(); t.unscheduled = un.data();
  return h->enc->decode(t, dt);
}
thread_local std::string g_err;
int set_err(int code, const std::string& m) { g_err = m; return code; }
// what a call into libksolve returned: KS_OK, or its code with its message
int dev_rc(int rc) { return rc == KS_OK ? KS_OK : set_err(rc, ks_last_error()); }
// The one error boundary: every extern "C" function that can throw runs its body through here, so that no exception -- a std::bad_alloc included -- leaves the library
template <class F> int guarded(F&& body) {
  try { return body(); }
  catch (const ksh::Unsupported& e) { return set_err(KS_ERR_UNSUPPORTED, e.what()); }
  catch (const std::exception& e) { return set_err(KS_ERR_INVALID, e.what()); }
}
using clk = std::chrono::steady_clock;
double ms_since(clk::time_point t) { return std::chrono::duration<double, std::milli>(clk::now() - t).count(); }
void zero(double* ms, int n) { if (ms) std::fill(ms, ms + n, 0.0); }
bool timing() { return getenv("KSH_TIMING") != nullptr; }      // (asked at every call: a caller may set it after loading the library)
// a flattening as a handle, its result buffers allocated
Handle* new_handle(std::unique_ptr<ksh::Encoded> enc) {
  auto h = std::make_unique<Handle>();
  h->enc = std::move(enc); h->rb = h->enc->make_result();
  return h.release();
}
// not uploaded yet: to the calling thread's current HIP device
int ensure_resident(Handle* h) { return h->dev ? KS_OK : ksh_upload(h, ks_current_device()); }
// ds = the device problems of hv[0 .. n).  A handle without one -- or, with `need_result`, without a solve's result on the device -- is refused in the caller's words
int device_problems(void** hv, uint32_t n, bool need_result, const char* refusal, std::vector<ks_dev_problem*>& ds) {
  ds = std::vector<ks_dev_problem*>(n);
  for (uint32_t i = 0; i < n; ++i) {
    Handle* h = (Handle*)hv[i];
    if (!h || !h->dev || (need_result && !h->dev_result)) return set_err(KS_ERR_INVALID, refusal);
    ds[i] = h->dev;
  }
  return KS_OK;
}
// The string table of a binary block (env / delta / pdb), checked: the offsets ascend and stay within str_bytes_len.  As the ksh_pod_block the readers take.
ksh_pod_block string_table(const char* what, uint32_t n_strings, const uint32_t* str_off, const char* str_bytes, uint64_t str_bytes_len) {
  for (uint32_t i = 0; i < n_strings; ++i) if (str_off[i + 1] < str_off[i]) throw ksp::Error(std::string(what) + " block: string offsets not ascending");
  if (n_strings && str_off[n_strings] > str_bytes_len) throw ksp::Error(std::string(what) + " block: string offsets reach beyond str_bytes_len");
  ksh_pod_block strings{}; strings.n_strings = n_strings; strings.str_off = str_off; strings.str_bytes = str_bytes; strings.str_bytes_len = str_bytes_len;
  return strings;
}
// the bindings a what-if call means: the caller's array, or -- after ksh_env_apply -- the library's own
const int32_t* bindings_of(Parsed* P, const int32_t* pod_node) { return pod_node ? pod_node : (P->bind_set ? P->bind.data() : nullptr); }
// The snapshot's flattening for these bindings (the caller's, else the library's own) and flags: the one kept if it fits them, else a new one, which is kept.  P->mu is
// held.  `may_continue`: a new one is continued from the one kept when the flags agree (ksh::make_snapshot_base `before`).  *made (may be NULL): a new one was made.
std::shared_ptr<const ksh::SnapshotBase> flattening_of(Parsed* P, const int32_t* pod_node, uint32_t flags, bool may_continue, bool* made = nullptr) {
  pod_node = bindings_of(P, pod_node);
  const size_t np = P->pr->pods.size();
  if (!pod_node && np) throw ksp::Error("no bindings (pod_node)");
  const bool fits = P->sb && P->sb_flags == flags && P->sb_pod_node.size() == np && std::equal(pod_node, pod_node + np, P->sb_pod_node.begin());
  if (made) *made = !fits;
  if (fits) return P->sb;
  P->sb = ksh::make_snapshot_base(P->pr, pod_node, flags, may_continue && P->sb_flags == flags ? P->sb.get() : nullptr);
  P->sb_flags = flags; P->sb_pod_node.assign(pod_node, pod_node + np);
  return P->sb;
}
// The snapshot's own flattening resident on `device` with its tables built (once per snapshot and device; shared by every what-if over it).
int resident_base(const ksh::Encoded* base, int device, std::shared_ptr<void>* out) {
  std::lock_guard<std::mutex> g(base->dev_mu);
  auto it = base->dev_resident.find(device);
  if (it != base->dev_resident.end()) { *out = it->second; return KS_OK; }
  ks_dev_problem* raw = nullptr;
  int rc = ks_problem_upload(&base->prob, device, &raw);
  if (rc == KS_OK) rc = ks_problem_prepare(raw);
  if (rc != KS_OK) { if (raw) ks_problem_free(raw); return set_err(rc, ks_last_error()); }
  *out = std::shared_ptr<void>(raw, [](void* p) { ks_problem_free((ks_dev_problem*)p); });
  base->dev_resident[device] = *out;
  return KS_OK;
}
// FNV-1a over every array behind a flattening's ks_problem: two construction routes produced the same flat problem iff equal.
uint64_t fingerprint_of(const ksh::Encoded& E) {
  uint64_t h = 1469598103934665603ull;
  auto mix = [&](const void* p, size_t bytes) { const unsigned char* c = (const unsigned char*)p; for (size_t i = 0; i < bytes; ++i) { h ^= c[i]; h *= 1099511628211ull; } };
  auto vec = [&](const auto& v) { uint64_t n = v.size(); mix(&n, 8); if (n) mix(v.data(), n * sizeof(v[0])); };
  auto rs = [&](const ksh::ReqSetsStore& r) { vec(r.present); vec(r.complement); vec(r.mask); vec(r.gt); vec(r.lt); vec(r.it_state); };
  const ks_problem& p = E.prob; const uint32_t dims[16] = {p.P, p.C, p.T, p.M, p.E, p.K, p.R, p.G, p.GH, p.S, p.SC, p.max_new_nodes, p.flags, p.wellknown_mask, p.n_ct, p.n_topologies}; mix(dims, sizeof dims);
  // the arrays in the table's order (include/ksolve.h KS_PROBLEM_ARRAYS), which is the order the committed fingerprints were hashed in; a PRICE_LO row is left out
  const ksh::Encoded& own_SELF = E; const ksh::Encoded& own_CAT = E.catalogue(); const ksh::Encoded& own_LAT = E.lattice();
  enum { SKIP_NEVER = 0, SKIP_CAT = 0, SKIP_LAT = 0, SKIP_PRICE = 0, SKIP_PRICE_LO = 1 };
#define X(f, owner, count, share) if (!SKIP_##share) vec(own_##owner.f);
#define XRS(f, n) rs(E.f);
  KS_PROBLEM_ARRAYS(X, XRS)
#undef X
#undef XRS
  return h;
}
}  // namespace

extern "C" {

const char* ksh_last_error(void) { return g_err.c_str(); }
void ksh_free(char* p) { free(p); }

// Parse KSP1, run the host half of NewScheduler/NewTopology, flatten.  No GPU needed.
int ksh_open(const char* ksp_text, size_t len, uint32_t flags, void** out) {
  *out = nullptr;
  return guarded([&] {
    auto t0 = clk::now();
    ksp::Problem pr = ksp::Parser(ksp_text, len).parse();
    const double parse_ms = ms_since(t0); t0 = clk::now();
    auto enc = ksh::encode(std::move(pr), flags);
    const double encode_ms = ms_since(t0); t0 = clk::now();
    *out = new_handle(std::move(enc));
    if (timing()) fprintf(stderr, "ksh_open: parse %.2f ms, encode %.2f ms, result buffers %.2f ms\n", parse_ms, encode_ms, ms_since(t0));
    return KS_OK;
  });
}
void ksh_close(void* h) { delete (Handle*)h; }
const ks_problem* ksh_problem(void* h) { return &((Handle*)h)->enc->prob; }

// ---- the pod list in memory ----
// ksh_parse turns KSP1 text into the C++ objects (the analogue of the []*v1.Pod, []*cloudprovider.InstanceType, []*state.Node a Go
// caller holds); ksh_solve_from_pods then does what the reference does from that point: NewScheduler's flattening incl. NewQueue's
// sort and every per-pod computation, upload, the HIP kernels, read-back -- the window bench.py times as "solve_from_pods".
int ksh_parse(const char* ksp_text, size_t len, void** out) {
  *out = nullptr;
  return guarded([&] { auto p = std::make_unique<Parsed>(); p->pr = std::make_shared<const ksp::Problem>(ksp::Parser(ksp_text, len).parse()); *out = p.release(); return KS_OK; });
}
int ksh_env_ingest(const ksh_env_block* env, void** out, double* ms) {
  if (out) *out = nullptr;
  if (!out || !env || !env->str_off || !env->words || (!env->str_bytes && env->n_strings)) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    const auto t0 = clk::now();
    const ksh_pod_block strings = string_table("env", env->n_strings, env->str_off, env->str_bytes, env->str_bytes_len);
    auto p = std::make_unique<Parsed>();
    p->pr = std::make_shared<const ksp::Problem>(ksp::EnvReader(strings, env->words, env->words + env->n_words).read_env());
    if (ms) *ms = ms_since(t0);
    *out = p.release(); return KS_OK;
  });
}
void ksh_parsed_free(void* p) { delete (Parsed*)p; }
// ms[0..5]: flatten (host) | upload | static tables + feasibility grid | pack kernel (HIP events) | whole ks_solve_dev incl. read-back | total wall
}  // extern "C"
template <class ENC> static int solve_from(ENC&& make_encoded, int device, void** out_handle, double* ms) {
  if (out_handle) *out_handle = nullptr;
  return guarded([&] {
    const auto t0 = clk::now();      // (every lap below is read off this one start: the parts add up to the total)
    auto enc = make_encoded();
    const double encoded = ms_since(t0);
    std::unique_ptr<Handle> h(new_handle(std::move(enc)));
    const double flat = ms_since(t0);
    if (timing()) fprintf(stderr, "  solve_from: encode %.2f ms, make_result %.2f ms\n", encoded, flat - encoded);
    int rc = dev_rc(ks_problem_upload(&h->enc->prob, device, &h->dev)); if (rc != KS_OK) return rc;
    const double uploaded = ms_since(t0);
    float grid_ms = 0; rc = dev_rc(ks_feasibility_grid(h->dev, nullptr, &grid_ms)); if (rc != KS_OK) return rc;
    const double gridded = ms_since(t0);
    float kms = 0; rc = dev_rc(ks_solve_dev(h->dev, &h->rb->r, &kms)); if (rc != KS_OK) return rc;
    h->solved = true; h->dev_result = true;
    const double solved = ms_since(t0);
    if (ms) { ms[0] = flat; ms[1] = uploaded - flat; ms[2] = gridded - uploaded; ms[3] = kms; ms[4] = solved - gridded; ms[5] = solved; }
    if (out_handle) *out_handle = h.release();
    return KS_OK;
  });
}
extern "C" {
int ksh_solve_from_pods(void* parsed, int device, uint32_t flags, void** out_handle, double* ms) {
  return solve_from([&] { return ksh::encode(((Parsed*)parsed)->pr, flags, &((Parsed*)parsed)->env); }, device, out_handle, ms);
}

// ---- binary pod ingress (kshost.h): flat pod records -> the batch in compact form; then Solve for that batch against an environment ----
struct Batch { std::shared_ptr<const ksp::PodBatch> b; };
int ksh_pods_ingest(const ksh_pod_block* blocks, uint32_t n_blocks, void** out_batch, double* ms) {
  if (out_batch) *out_batch = nullptr;
  if (!out_batch || (n_blocks && !blocks)) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    const auto t0 = clk::now();
    auto b = std::make_unique<Batch>(); b->b = ksh::ingest_pod_blocks(blocks, n_blocks);
    if (ms) *ms = ms_since(t0);
    *out_batch = b.release(); return KS_OK;
  });
}
void ksh_pods_free(void* batch) { delete (Batch*)batch; }
int ksh_pods_count(void* batch, uint32_t* n_pods, uint32_t* n_specs) {
  if (!batch) return set_err(KS_ERR_INVALID, "null argument");
  if (n_pods) *n_pods = (uint32_t)((Batch*)batch)->b->size();
  if (n_specs) *n_specs = (uint32_t)((Batch*)batch)->b->specs.size();
  return KS_OK;
}
int ksh_solve_from_batch(void* parsed_env, void* batch, int device, uint32_t flags, void** out_handle, double* ms) {
  if (!parsed_env || !batch) return set_err(KS_ERR_INVALID, "null argument");
  return solve_from([&] { return ksh::encode(((Parsed*)parsed_env)->pr, ((Batch*)batch)->b, flags, &((Parsed*)parsed_env)->env); }, device, out_handle, ms);
}
// flatten only (no GPU needed) the problem a ksh_parse holds: ksh_open without the text
int ksh_open_parsed(void* parsed, uint32_t flags, void** out) {
  if (out) *out = nullptr;
  if (!parsed || !out) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] { *out = new_handle(ksh::encode(((Parsed*)parsed)->pr, flags, &((Parsed*)parsed)->env)); return KS_OK; });
}
int ksh_open_batch(void* parsed_env, void* batch, uint32_t flags, void** out) {
  if (out) *out = nullptr;
  if (!parsed_env || !batch || !out) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] { *out = new_handle(ksh::encode(((Parsed*)parsed_env)->pr, ((Batch*)batch)->b, flags, &((Parsed*)parsed_env)->env)); return KS_OK; });
}
// KSR1 text of the result a handle holds (after ksh_solve / ksh_solve_from_pods)
int ksh_result_text(void* hv, char** out_text) {
  Handle* h = (Handle*)hv; if (out_text) *out_text = nullptr;
  if (!h || !out_text) return set_err(KS_ERR_INVALID, "null argument");
  if (!h->solved) return set_err(KS_ERR_INVALID, "the handle holds no result: solve it first (or the last solve failed)");
  return guarded([&] { std::string s = decode_handle(h, 0.0); *out_text = strdup(s.c_str()); return KS_OK; });
}

// Fixed-size record of the result a handle holds -- what consolidation reads of a simulation (consolidation.go:190-260):
// out[0] = number of new nodes, out[1] = number of unscheduled pods, out[2..2+words) = InstanceTypeOptions of new node 0 as a bitmask
// (zero if there is none).  No text, no per-pod data: this is what the ranks all-gather.
int ksh_result_summary(void* hv, uint64_t* out, uint32_t words) {
  Handle* h = (Handle*)hv; if (!h || !out) return set_err(KS_ERR_INVALID, "null argument");
  if (!h->solved) return set_err(KS_ERR_INVALID, "the handle holds no result: solve it first (or the last solve failed)");
  const ks_result& r = h->rb->r; const uint32_t TW = (h->enc->prob.T + 63) / 64;
  if (words < TW) return set_err(KS_ERR_INVALID, "summary row too short");
  out[0] = r.n_new; out[1] = r.n_unscheduled;
  for (uint32_t w = 0; w < words; ++w) out[2 + w] = (r.n_new && w < TW) ? r.node_types[w] : 0;
  return KS_OK;
}

// Consolidation what-ifs over ONE cluster snapshot (deprovisioning/helpers.go:42-115 simulateScheduling): the snapshot is
// parsed once -- `base` lists every state node and, as its pod batch, every bound pod with its full spec; pod_node[i] is the
// node (index into base nodes) pod i runs on -- and what-if w is derived natively: its candidate nodes cand[cand_off[w] ..
// cand_off[w+1]) leave the state-node list (helpers.go:48-61), their pods, in candidate order, become the pending batch, the
// flattening (NewScheduler / NewTopology host half) runs on `nthreads` host threads.  out_handles[w] is a ksh_open handle.
static int open_whatifs_over(std::shared_ptr<const ksp::Problem> snapshot, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand,
                             const int32_t* pod_node, uint32_t nthreads, void** out_handles, Parsed* cache = nullptr) {
  for (uint32_t w = 0; w < n; ++w) out_handles[w] = nullptr;
  return guarded([&] {
    for (uint32_t i = 0; i < cand_off[n]; ++i) if (cand[i] >= snapshot->nodes.size()) return set_err(KS_ERR_INVALID, "candidate node out of range");
    // the snapshot is flattened ONCE (catalogue, universes, templates, every state node's row); a what-if adds only what its candidate set decides
    auto t0 = clk::now();
    std::shared_ptr<const ksh::SnapshotBase> sb;
    if (cache) { std::lock_guard<std::mutex> g(cache->mu); sb = flattening_of(cache, pod_node, flags, true); }
    else { if (!pod_node && !snapshot->pods.empty()) return set_err(KS_ERR_INVALID, "no bindings (pod_node)"); sb = ksh::make_snapshot_base(snapshot, pod_node, flags); }
    if (timing()) { fprintf(stderr, "  what-ifs: snapshot base %8.2f ms\n", ms_since(t0)); t0 = clk::now(); }
    std::atomic<uint32_t> next{0}; std::atomic<int> rc{KS_OK}; std::vector<std::string> errs(n);
    const std::vector<std::vector<uint32_t>>* by_node = ksh::delta_inputs(*sb).by_node;
    auto work = [&]() {
      for (;;) {
        const uint32_t w = next.fetch_add(1); if (w >= n) return;
        try {
          Handle* h = new_handle(ksh::encode_whatif(*sb, cand + cand_off[w], cand_off[w + 1] - cand_off[w], flags)); out_handles[w] = h; h->snapshot_whatif = true;
          for (uint32_t i = cand_off[w]; i < cand_off[w + 1]; ++i) for (uint32_t p : (*by_node)[cand[i]]) h->pod_ids.push_back(p);      // (the batch's own order: encode.cpp Builder)
        } catch (const ksh::Unsupported& e) { errs[w] = e.what(); rc = KS_ERR_UNSUPPORTED;
        } catch (const std::exception& e) { errs[w] = e.what(); rc = KS_ERR_INVALID; }
      }
    };
    const uint32_t nt = std::max(1u, std::min(nthreads ? nthreads : ksh::host_threads(), n));
    std::vector<std::thread> pool; for (uint32_t t = 1; t < nt; ++t) pool.emplace_back(work);
    work(); for (auto& t : pool) t.join();
    if (timing()) fprintf(stderr, "  what-ifs: %u flattened on %u threads %8.2f ms\n", n, nt, ms_since(t0));
    if (rc != KS_OK) { std::string m; for (auto& e : errs) if (!e.empty()) { m = e; break; } for (uint32_t w = 0; w < n; ++w) { delete (Handle*)out_handles[w]; out_handles[w] = nullptr; } return set_err(rc, m); }
    return KS_OK;
  });
}
int ksh_open_whatifs(const char* base_text, size_t len, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand,
                     const int32_t* pod_node, uint32_t nthreads, void** out_handles) {
  for (uint32_t w = 0; w < n; ++w) out_handles[w] = nullptr;
  return guarded([&] {
    auto snapshot = std::make_shared<ksp::Problem>(ksp::Parser(base_text, len).parse());
    for (auto& nd : snapshot->nodes) nd.in_state = true;
    snapshot->simulation_mode = true;
    return open_whatifs_over(std::shared_ptr<const ksp::Problem>(snapshot), flags, n, cand_off, cand, pod_node, nthreads, out_handles);
  });
}
// The same over a snapshot the caller already holds as objects (ksh_parse): every node of it is a state node, every pod a bound pod.
int ksh_open_whatifs_parsed(void* parsed, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand, const int32_t* pod_node, uint32_t nthreads, void** out_handles) {
  return open_whatifs_over(((Parsed*)parsed)->pr, flags, n, cand_off, cand, pod_node, nthreads, out_handles, (Parsed*)parsed);
}

uint64_t ksh_fingerprint(void* hv) { return fingerprint_of(*((Handle*)hv)->enc); }

// ---- the snapshot kept current by events instead of re-ingested (state.Cluster's UpdateNode / DeleteNode / UpdatePod / DeletePod, cluster.go) ----
// The problem object is patched in place -- new nodes and pods are appended (the vectors were parsed with room: nothing moves), a node that is updated is replaced
// in its slot (NODE=), an instance type likewise (IT=), what leaves stays as a tombstone
// (a node out of state, a pod bound nowhere) -- and the snapshot's flattening, if there is one, is continued from the one before (ksh::make_snapshot_base `before`).
// Not to be called while another thread uses handles opened over this snapshot; handles opened BEFORE the call keep solving what they were opened for.
// What both doors do once the events are objects (`ev` is consumed): the text door (ksh_env_apply) and the binary one (ksh_env_apply_block) differ in the decoding alone.
// `track_cluster_pods`: mirror BIND / UNBIND into the snapshot's cluster pods whatever the first call found there (KSH_APPLY_TRACK_CLUSTER_PODS); otherwise iff it found some.
static int apply_events(Parsed* P, const int32_t* pod_node, std::vector<ksp::DeltaEvent>& ev, bool track_cluster_pods, uint32_t info[4]) {
  {
    std::lock_guard<std::mutex> g(P->mu);
    ksp::Problem& pr = const_cast<ksp::Problem&>(*P->pr);      // (the only writer; see above)
    if (!P->bind_set) {
      if (!pod_node && !pr.pods.empty()) return set_err(KS_ERR_INVALID, "the first ksh_env_apply needs the bindings (pod_node) of the snapshot's pods");
      P->bind.assign(pod_node, pod_node + pr.pods.size());
      for (size_t i = 0; i < pr.pods.size(); ++i) if (P->bind[i] >= (int32_t)pr.nodes.size()) return set_err(KS_ERR_INVALID, "pod_node out of range");
      for (size_t i = 0; i < pr.nodes.size(); ++i) if (pr.nodes[i].in_state && !P->live_node.emplace(pr.nodes[i].name, (uint32_t)i).second) { P->live_node.clear(); return set_err(KS_ERR_INVALID, "two state nodes share a name"); }
      for (size_t i = 0; i < pr.pods.size(); ++i) if (P->bind[i] >= 0 && !P->live_pod.emplace(pr.pods[i].uid, (uint32_t)i).second) { P->live_node.clear(); P->live_pod.clear(); return set_err(KS_ERR_INVALID, "two bound pods share a uid"); }
      P->had_cluster_pods = !pr.cluster_pods.empty(); P->bind_set = true;
    } else if (pod_node && !std::equal(pod_node, pod_node + pr.pods.size(), P->bind.begin())) return set_err(KS_ERR_INVALID, "the bindings passed differ from the ones the library holds since the last ksh_env_apply (pass NULL)");
    const bool mirror = track_cluster_pods || P->had_cluster_pods;
    auto unbind = [&](uint32_t i) {
      ksp::Pod& p = pr.pods[i]; ksp::StateNode& n = pr.nodes[P->bind[i]];
      const ksp::ResList req = ksh::RequestsForPod(p);      // state.Node.cleanupForPod (node.go:175-182): Available() = Allocatable - the requests of the pods still there
      for (auto& kv : n.available) { auto r = req.find(kv.first); if (r != req.end()) kv.second += r->second; }
      for (auto& c : p.containers) for (auto& hp : c.ports) if (hp.port != 0) for (size_t k = 0; k < n.host_ports.size(); ++k) if (n.host_ports[k].ip == hp.ip && n.host_ports[k].port == hp.port && n.host_ports[k].proto == hp.proto) { n.host_ports.erase(n.host_ports.begin() + k); break; }
      for (auto& v : p.volumes) for (size_t k = 0; k < n.volumes.size(); ++k) if (n.volumes[k].driver == v.driver && n.volumes[k].pvc == v.pvc) { n.volumes.erase(n.volumes.begin() + k); break; }
      if (mirror) for (size_t k = 0; k < pr.cluster_pods.size(); ++k) if (pr.cluster_pods[k].uid == p.uid) { pr.cluster_pods.erase(pr.cluster_pods.begin() + k); break; }
      P->live_pod.erase(p.uid); P->bind[i] = -1;
      p.uid = std::string("\1unbound-") + std::to_string(++P->tombstones);      // (uids stay unique: the same pod may be bound again)
    };
    uint32_t done = 0; std::string why; int why_rc = KS_ERR_INVALID;
    std::vector<ksh::ReplacedNode> replaced;      // NODE=: the nodes as the flattening before saw them (the first replacement of a slot in this call)
    std::vector<ksh::ReplacedType> replaced_types;      // IT=: the instance types likewise
    for (auto& e : ev) {
      if (e.kind == ksp::DeltaEvent::NodeAdd) {
        if (P->live_node.count(e.node.name)) { why = "NODE+: a state node named " + e.node.name + " exists"; break; }
        if (pr.nodes.size() == pr.nodes.capacity()) { why = "NODE+: the snapshot's spare room for nodes is used up (ingest it again)"; break; }
        e.node.in_state = true; P->live_node.emplace(e.node.name, (uint32_t)pr.nodes.size()); pr.nodes.push_back(std::move(e.node));
      } else if (e.kind == ksp::DeltaEvent::NodeRemove) {
        auto it = P->live_node.find(e.name); if (it == P->live_node.end()) { why = "NODE-: no state node named " + e.name; break; }
        const uint32_t nd = it->second;
        for (uint32_t i = 0; i < P->bind.size(); ++i) if (P->bind[i] == (int32_t)nd) unbind(i);      // (its pods go with it)
        pr.nodes[nd].in_state = false; P->live_node.erase(it);
        pr.nodes[nd].name = std::string("\1gone-") + std::to_string(++P->tombstones) + ":" + pr.nodes[nd].name;      // (the name may come back)
      } else if (e.kind == ksp::DeltaEvent::PodBind) {
        auto it = P->live_node.find(e.name); if (it == P->live_node.end()) { why = "BIND: no state node named " + e.name; break; }
        if (P->live_pod.count(e.pod.uid)) { why = "BIND: pod " + e.pod.uid + " is bound already (UNBIND it first)"; break; }
        if (pr.pods.size() == pr.pods.capacity()) { why = "BIND: the snapshot's spare room for pods is used up (ingest it again)"; break; }
        ksp::StateNode& n = pr.nodes[it->second];
        const ksp::ResList req = ksh::RequestsForPod(e.pod);      // state.Node.updateForPod (node.go:161-173)
        for (auto& kv : n.available) { auto r = req.find(kv.first); if (r != req.end()) kv.second -= r->second; }
        for (auto& c : e.pod.containers) for (auto& hp : c.ports) if (hp.port != 0) n.host_ports.push_back(hp);
        for (auto& v : e.pod.volumes) n.volumes.push_back(v);
        if (mirror) { ksp::ClusterPod cp; cp.uid = e.pod.uid; cp.ns = e.pod.ns; cp.node_name = n.name; cp.labels = e.pod.labels; cp.anti_required = e.pod.anti_required; pr.cluster_pods.push_back(std::move(cp)); }
        P->live_pod.emplace(e.pod.uid, (uint32_t)pr.pods.size()); pr.pods.push_back(std::move(e.pod)); P->bind.push_back((int32_t)it->second);
      } else if (e.kind == ksp::DeltaEvent::NodeUpdate) {
        // state.Cluster.UpdateNode for a node already in state (cluster.go:151-166): the node object is replaced, slot and bindings stay; what the record carries is
        // state.Node's own output, already net of the pods bound -- taken as given
        auto it = P->live_node.find(e.node.name); if (it == P->live_node.end()) { why = "NODE=: no state node named " + e.node.name; break; }
        const uint32_t nd = it->second; ksp::StateNode& n = pr.nodes[nd];
        e.node.in_state = true; e.node.stamp = n.stamp + 1;
        bool first = true; for (auto& r : replaced) if (r.slot == nd) first = false;
        if (first) replaced.push_back(ksh::ReplacedNode{nd, std::move(n)});
        n = std::move(e.node);
      } else if (e.kind == ksp::DeltaEvent::TypeUpdate) {
        // the catalogue as cloudProvider.GetInstanceTypes lists it NOW (provisioner.go:237-296 asks on every pass): the record replaces the type in its slot -- the
        // index stays, and with it the provisioners' lists, the nodes' instance-type labels and every bit of an InstanceTypeOptions row
        if (P->type_index.empty()) for (size_t t = 0; t < pr.instance_types.size(); ++t) P->type_index.emplace(pr.instance_types[t].name, (uint32_t)t);
        auto it = P->type_index.find(e.type.name); if (it == P->type_index.end()) { why = "IT=: no instance type named " + e.type.name; break; }
        // what the ingest doors refuse of an instance type (encode.cpp collect_passive / encode_instance_types) is refused here, before anything is touched
        for (auto& x : e.type.requirements) {
          if (x.op == ksp::Op::Gt || x.op == ksp::Op::Lt) { why = "IT=: instance type requirement with Gt/Lt bounds"; why_rc = KS_ERR_UNSUPPORTED; break; }
          if (ksp::normalize_key(x.key) == ksp::kHostname) { why = "IT=: instance type requirement on hostname"; why_rc = KS_ERR_UNSUPPORTED; break; }
        }
        if (!why.empty()) break;
        const uint32_t t = it->second; ksp::InstanceType& ty = pr.instance_types[t];
        e.type.stamp = ty.stamp + 1;
        bool first = true; for (auto& r : replaced_types) if (r.slot == t) first = false;
        if (first) replaced_types.push_back(ksh::ReplacedType{t, std::move(ty)});
        ty = std::move(e.type);
      } else {
        auto it = P->live_pod.find(e.name); if (it == P->live_pod.end()) { why = "UNBIND: no bound pod with uid " + e.name; break; }
        unbind(it->second);
      }
      ++done;
    }
    P->applied += done; P->cmd_nodes.reset(); P->cand_nodes.reset(); { std::lock_guard<std::mutex> ge(P->env.mu); P->env.base.reset(); }      // (a Solve over these objects flattens its environment again)
    // the snapshot's flattening follows, continued from the one before when there is one
    bool continued = false;
    if (P->sb) {
      std::shared_ptr<const ksh::SnapshotBase> before = P->sb;
      try { P->sb = ksh::make_snapshot_base(P->pr, P->bind.data(), P->sb_flags, before.get(), &replaced, &replaced_types); P->sb_pod_node = P->bind; continued = ksh::snapshot_continued(*P->sb); }
      catch (...) { P->sb.reset(); P->sb_pod_node.clear(); throw; }
      ksh::dispose_later(std::move(before));      // (the flattening before: torn down off this thread, once the handles that still use it are closed)
    }
    if (info) { info[0] = done; info[1] = (uint32_t)pr.nodes.size(); info[2] = (uint32_t)pr.pods.size(); info[3] = continued ? 1u : 0u; }
    if (done != ev.size()) return set_err(why_rc, "event " + std::to_string(done) + ": " + why + " (the events before it were applied)");
    return KS_OK;
  }
}
int ksh_env_apply(void* parsed, const int32_t* pod_node, const char* ksd_text, size_t len, uint32_t info[4]) {
  if (info) info[0] = info[1] = info[2] = info[3] = 0;
  if (!parsed || !ksd_text) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    std::vector<ksp::DeltaEvent> ev = ksp::Parser(ksd_text, len).parse_delta();
    return apply_events((Parsed*)parsed, pod_node, ev, false, info);
  });
}
// The same events without the text (kshost.h ksh_delta_block; grammar in kspb.hpp DeltaReader).  The block is decoded COMPLETELY before the first event is applied:
// a malformed block changes nothing, not even the hand-over of the bindings on a first call.
int ksh_env_apply_block(void* parsed, const int32_t* pod_node, const ksh_delta_block* d, uint32_t flags, uint32_t info[4]) {
  if (info) info[0] = info[1] = info[2] = info[3] = 0;
  if (!parsed || !d || !d->str_off || (!d->words && d->n_words) || (!d->str_bytes && d->n_strings)) return set_err(KS_ERR_INVALID, "null argument");
  if (flags & ~(uint32_t)KSH_APPLY_TRACK_CLUSTER_PODS) return set_err(KS_ERR_INVALID, "ksh_env_apply_block: unknown flag bit");
  return guarded([&] {
    const ksh_pod_block strings = string_table("delta", d->n_strings, d->str_off, d->str_bytes, d->str_bytes_len);
    std::vector<ksp::DeltaEvent> ev = ksp::DeltaReader(strings, d->words, d->words + d->n_words).read_delta(d->n_events);
    return apply_events((Parsed*)parsed, pod_node, ev, (flags & KSH_APPLY_TRACK_CLUSTER_PODS) != 0, info);
  });
}
// the bindings the library holds after ksh_env_apply: out[0 .. n_pods) (cap entries at most); the sizes either way
int ksh_snapshot_bindings(void* parsed, int32_t* out, uint32_t cap, uint32_t* n_pods, uint32_t* n_nodes) {
  if (!parsed) return set_err(KS_ERR_INVALID, "null argument");
  Parsed* P = (Parsed*)parsed; std::lock_guard<std::mutex> g(P->mu);
  if (n_pods) *n_pods = (uint32_t)P->pr->pods.size();
  if (n_nodes) *n_nodes = (uint32_t)P->pr->nodes.size();
  if (out) { if (!P->bind_set) return set_err(KS_ERR_INVALID, "no ksh_env_apply yet: the caller holds the bindings"); std::copy_n(P->bind.begin(), std::min<size_t>(cap, P->bind.size()), out); }
  return KS_OK;
}
// FNV-1a over the snapshot's flattening (the flat problem + the tables the device derivation reads); `cold` != 0: of a flattening made from scratch for the comparison
// (tests: a continued flattening must equal it).  The snapshot must have been flattened (a what-if batch opened) or is flattened now.
int ksh_snapshot_fingerprint(void* parsed, const int32_t* pod_node, uint32_t flags, int cold, uint64_t* out) {
  if (!parsed || !out) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    Parsed* P = (Parsed*)parsed; std::lock_guard<std::mutex> g(P->mu);
    const int32_t* pn = bindings_of(P, pod_node); if (!pn && !P->pr->pods.empty()) return set_err(KS_ERR_INVALID, "no bindings");
    // a flattening made here is never continued from the one kept: the tests compare what this call makes with a cold one
    std::shared_ptr<const ksh::SnapshotBase> sb = cold ? ksh::make_snapshot_base(P->pr, pn, flags) : flattening_of(P, pn, flags, false);
    *out = fingerprint_of(*ksh::delta_inputs(*sb).base) ^ (ksh::snapshot_fingerprint(*sb) * 0x9E3779B97F4A7C15ull);
    return KS_OK;
  });
}

// What-ifs DERIVED on the device from the resident snapshot (include/ksolve.h ks_whatifs_open): no per-what-if flattening, an upload of KBs.
// Same contract as ksh_open_whatifs_parsed, with the problems already resident on `device`; KS_ERR_UNSUPPORTED (nothing opened) when the
// snapshot's what-ifs do not differ by their candidate sets alone -- the caller then uses ksh_open_whatifs_parsed.
int ksh_open_whatifs_derived(void* parsed, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand, const int32_t* pod_node, int device, void** out_handles) {
  for (uint32_t w = 0; w < n; ++w) out_handles[w] = nullptr;
  return guarded([&] {
    Parsed* P = (Parsed*)parsed; std::shared_ptr<const ksp::Problem> snapshot = P->pr;
    for (uint32_t i = 0; i < cand_off[n]; ++i) if (cand[i] >= snapshot->nodes.size()) return set_err(KS_ERR_INVALID, "candidate node out of range");
    if (flags & KS_FLAG_STATS) return set_err(KS_ERR_UNSUPPORTED, "derived what-ifs carry no reference-algorithm statistics");
    const bool timed = timing(); auto t0 = clk::now();
    auto lap = [&](const char* what) { if (!timed) return; fprintf(stderr, "  derived what-ifs: %-28s %8.2f ms\n", what, ms_since(t0)); t0 = clk::now(); };
    std::shared_ptr<const ksh::SnapshotBase> sb; bool made = false;
    { std::lock_guard<std::mutex> g(P->mu); sb = flattening_of(P, pod_node, flags, true, &made); }
    if (made) lap("snapshot flattened (once)");
    t0 = clk::now();
    const ksh::DeltaInputs in = ksh::delta_inputs(*sb);
    if (!in.eligible) return set_err(KS_ERR_UNSUPPORTED, "what-ifs of this snapshot cannot be derived on the device: " + in.why);
    auto D = std::make_shared<DeltaBatch>(); D->sb = sb; D->cand_off.assign(cand_off, cand_off + n + 1); D->cand.assign(cand, cand + cand_off[n]);
    int rc = resident_base(in.base.get(), device, &D->base_dev); if (rc != KS_OK) return rc;
    lap("snapshot resident");
    const ks_problem& bp = in.base->prob; const uint32_t M = bp.M, R = bp.R;
    std::vector<uint32_t> npods(n, 0); std::vector<int64_t> rem((size_t)n * M * R);
    for (uint32_t w = 0; w < n; ++w) {
      int64_t* rw = &rem[(size_t)w * M * R]; std::copy(bp.tmpl_remaining, bp.tmpl_remaining + (size_t)M * R, rw);
      for (uint32_t i = cand_off[w]; i < cand_off[w + 1]; ++i) {
        const uint32_t nd = cand[i]; npods[w] += (uint32_t)(*in.by_node)[nd].size();
        const int32_t m = in.node_tmpl[nd]; if (m >= 0) for (uint32_t r = 0; r < R; ++r) rw[(size_t)m * R + r] += in.node_cap[(size_t)nd * R + r];      // remainingResources: the node's capacity comes back (scheduler.go:244-246)
      }
    }
    lap("masks / remaining (host)");
    if (in.lists || (flags & KSH_DERIVE_GROUP_LISTS)) {      // (KSH_DERIVE_GROUP_LISTS: the per-node topology facts as lists, any number of groups; a snapshot without groups has none)
      rc = ks_whatifs_open_lists((const ks_dev_problem*)D->base_dev.get(), in.n_nodes, P->sb_pod_node.data(), in.node_row, n, cand_off, cand, npods.data(), rem.data(), in.lists, in.volumes ? KS_WHATIFS_VOLUMES : 0u, &D->b);
    } else if (in.volumes) {      // (KSH_DERIVE_VOLUMES: the snapshot was flattened with the candidate-independent claim partition; every what-if carries its own volume state)
      ks_whatifs_options opt{}; opt.topo = in.topo; opt.flags = KS_WHATIFS_VOLUMES;
      rc = ks_whatifs_open_ex((const ks_dev_problem*)D->base_dev.get(), in.n_nodes, P->sb_pod_node.data(), in.node_row, n, cand_off, cand, npods.data(), rem.data(), &opt, &D->b);
    } else rc = ks_whatifs_open((const ks_dev_problem*)D->base_dev.get(), in.n_nodes, P->sb_pod_node.data(), in.node_row, n, cand_off, cand, npods.data(), rem.data(), in.topo, &D->b);
    if (rc != KS_OK) return dev_rc(rc);
    lap("ks_whatifs_open (device)");
    ks_dev_problem* const* views = ks_whatifs_problems(D->b);
    for (uint32_t w = 0; w < n; ++w) {
      auto h = std::make_unique<Handle>();
      h->enc = std::make_unique<ksh::Encoded>(); h->enc->src = snapshot; h->enc->shared = in.base; h->enc->shared_lattice = true; h->enc->view = true;
      h->enc->prob = bp; h->enc->prob.P = npods[w]; h->enc->prob.max_new_nodes = npods[w] ? npods[w] : 1;
      h->dev = views[w]; h->delta = D; h->delta_index = w; h->base_dev = D->base_dev; h->snapshot_whatif = true;
      out_handles[w] = h.release();
    }
    lap("handles");
    return KS_OK;
  });
}

int ksh_debug_whatif_topology(void* hv, uint8_t* out_active, int32_t* out_count, int32_t* out_extra) {
  Handle* h = (Handle*)hv;
  if (!h || !h->delta || !h->dev) return set_err(KS_ERR_INVALID, "not the handle of a derived what-if");
  return dev_rc(ks_debug_whatif_topology(h->dev, out_active, out_count, out_extra));
}
uint64_t ksh_whatifs_upload_bytes(void* hv) { const Handle* h = (const Handle*)hv; return h && h->delta ? ks_whatifs_upload_bytes(h->delta->b) : 0; }
uint64_t ksh_whatifs_arena_bytes(void* hv) { const Handle* h = (const Handle*)hv; return h && h->delta ? ks_whatifs_arena_bytes(h->delta->b) : 0; }

// CPU self-check of what ksh_open_whatifs_derived would derive on the device for ONE candidate set (kshost.h).
int ksh_check_whatif_derivation(void* parsed, uint32_t flags, const uint32_t* cand, uint32_t ncand, const int32_t* pod_node) {
  return guarded([&] {
    Parsed* P = (Parsed*)parsed;
    std::shared_ptr<const ksh::SnapshotBase> sb;
    { std::lock_guard<std::mutex> g(P->mu); sb = flattening_of(P, pod_node, flags, true); }
    const std::string why = ksh::check_derived_topology(*sb, cand, ncand, flags);
    return why.empty() ? KS_OK : set_err(why.rfind("not derivable", 0) == 0 ? KS_ERR_UNSUPPORTED : KS_ERR_INVALID, why);
  });
}

// Upload the flat problem to HBM (idempotent).
int ksh_upload(void* hv, int device) {
  return guarded([&] {
    Handle* h = (Handle*)hv;
    if (h->dev) return ks_problem_device(h->dev) == device ? KS_OK : set_err(KS_ERR_INVALID, "problem already resident on another device");
    const ksh::Encoded* base = h->enc->shared.get();
    if (!base) return dev_rc(ks_problem_upload(&h->enc->prob, device, &h->dev));
    // A what-if flattened over a shared snapshot: the snapshot's flattening goes to the device once (catalogue, prices, lattice, the tables
    // derived from them); the what-if then uploads only what its candidate set decides.
    std::shared_ptr<void> bd;
    int rc = resident_base(base, device, &bd); if (rc != KS_OK) return rc;
    rc = ks_problem_upload_shared(&h->enc->prob, (const ks_dev_problem*)bd.get(), &h->dev);
    if (rc == KS_OK) h->base_dev = bd;
    return dev_rc(rc);
  });
}

// Upload a batch (what-ifs of one snapshot) on host threads: the per-problem cost is packing its arrays into the pinned staging buffer.
int ksh_upload_batch(void** handles, uint32_t n, int device, uint32_t nthreads) {
  if (!n) return KS_OK;
  int rc0 = ksh_upload(handles[0], device); if (rc0 != KS_OK) return rc0;      // the first one also makes the snapshot resident (once)
  return guarded([&] {
    std::atomic<uint32_t> next{1}; std::atomic<int> rc{KS_OK}; std::mutex emu; std::string emsg;
    auto work = [&]() {
      for (;;) {
        const uint32_t i = next.fetch_add(1); if (i >= n) return;
        try {      // (nothing may leave a worker thread; ksh_upload catches its own, keeping the message is what can still throw)
          const int r = ksh_upload(handles[i], device);
          if (r != KS_OK) { rc = r; std::lock_guard<std::mutex> g(emu); if (emsg.empty()) emsg = g_err; }
        } catch (const std::exception&) { rc = KS_ERR_INVALID; }
      }
    };
    const uint32_t nt = std::max(1u, std::min(nthreads ? nthreads : ksh::host_threads(), n - 1));
    std::vector<std::thread> pool; for (uint32_t t = 1; t < nt; ++t) pool.emplace_back(work);
    work(); for (auto& t : pool) t.join();
    return rc != KS_OK ? set_err(rc, emsg) : KS_OK;
  });
}
// The fixed-size records of a batch in one call: out[i*(2+words) ..] as ksh_result_summary.
int ksh_result_summaries(void** handles, uint32_t n, uint64_t* out, uint32_t words) {
  for (uint32_t i = 0; i < n; ++i) { const int rc = ksh_result_summary(handles[i], out + (size_t)i * (2 + words), words); if (rc != KS_OK) return rc; }
  return KS_OK;
}

// Solve (device-resident inputs).  out_text may be NULL (skip decode).
int ksh_solve(void* hv, char** out_text, float* kernel_ms, double* wall_ms) {
  return guarded([&] {
    Handle* h = (Handle*)hv;
    int rc = ensure_resident(h); if (rc != KS_OK) return rc;
    const auto t0 = clk::now();
    h->solved = false; h->dev_result = false;
    if (!h->rb) h->rb = h->enc->make_result();
    rc = ks_solve_dev(h->dev, &h->rb->r, kernel_ms);
    const double dt = std::chrono::duration<double>(clk::now() - t0).count();      // (seconds: what the KSR1 text carries)
    if (wall_ms) *wall_ms = dt * 1e3;
    if (rc != KS_OK) return dev_rc(rc);
    h->solved = true; h->dev_result = true;
    if (out_text) { std::string s = decode_handle(h, dt); *out_text = strdup(s.c_str()); }
    return KS_OK;
  });
}

// N independent problems in one launch (consolidation what-ifs, deprovisioning/helpers.go:42-115).
int ksh_solve_batch(void** hv, uint32_t n, char** out_texts, float* kernel_ms, double* wall_ms) {
  return guarded([&] {
    std::vector<ks_dev_problem*> ds(n); std::vector<ks_result*> rs(n);
    for (uint32_t i = 0; i < n; ++i) { Handle* h = (Handle*)hv[i]; if (!h->rb) h->rb = h->enc->make_result(); }      // (derived what-ifs allocate their result buffers on first use)
    for (uint32_t i = 0; i < n; ++i) { Handle* h = (Handle*)hv[i]; int rc = ensure_resident(h); if (rc != KS_OK) return rc; ds[i] = h->dev; rs[i] = &h->rb->r; }
    const auto t0 = clk::now();
    for (uint32_t i = 0; i < n; ++i) { ((Handle*)hv[i])->solved = false; ((Handle*)hv[i])->dev_result = false; }
    int rc = ks_solve_batch_dev(ds.data(), n, rs.data(), kernel_ms);
    const double dt = std::chrono::duration<double>(clk::now() - t0).count();
    if (wall_ms) *wall_ms = dt * 1e3;
    if (rc != KS_OK) return dev_rc(rc);
    for (uint32_t i = 0; i < n; ++i) { ((Handle*)hv[i])->solved = true; ((Handle*)hv[i])->dev_result = true; }
    if (out_texts) for (uint32_t i = 0; i < n; ++i) { std::string s = decode_handle((Handle*)hv[i], dt); out_texts[i] = strdup(s.c_str()); }
    return KS_OK;
  });
}

// The same launch with the results left on the device (no read-back but the error words), and the fixed-size records of the batch built there
// into a caller-owned DEVICE buffer [n][3 + words] of uint64 -- [ids[i], n_new, n_unscheduled, new node 0's InstanceTypeOptions] -- which a
// fan-out hands to its one all-gather as is (multinodeconsolidation.go:74-114: many candidate sets, one decision record each).
int ksh_solve_batch_resident(void** hv, uint32_t n, float* kernel_ms, double* wall_ms) {
  return guarded([&] {
    std::vector<ks_dev_problem*> ds(n);
    for (uint32_t i = 0; i < n; ++i) { Handle* h = (Handle*)hv[i]; int rc = ensure_resident(h); if (rc != KS_OK) return rc; ds[i] = h->dev; }
    const auto t0 = clk::now();
    for (uint32_t i = 0; i < n; ++i) { ((Handle*)hv[i])->solved = false; ((Handle*)hv[i])->dev_result = false; }
    int rc = ks_solve_batch_dev(ds.data(), n, nullptr, kernel_ms);
    if (wall_ms) *wall_ms = ms_since(t0);
    if (rc != KS_OK) return dev_rc(rc);
    for (uint32_t i = 0; i < n; ++i) ((Handle*)hv[i])->dev_result = true;
    return KS_OK;
  });
}
int ksh_result_records_dev(void** hv, uint32_t n, const uint64_t* ids, uint32_t words, void* d_out) {
  return guarded([&] {
    std::vector<ks_dev_problem*> ds;
    int rc = device_problems(hv, n, true, "records before solve", ds); if (rc != KS_OK) return rc;
    return dev_rc(ks_batch_records_dev(ds.data(), n, ids, words, d_out));
  });
}

// Consolidation price stage on the results of the last ksh_solve / ksh_solve_batch, which are still on the device:
// for handle i, of new node node[i]'s InstanceTypeOptions keep the types whose worst launch price is < max_price[i]
// (filterByPrice, deprovisioning/helpers.go:148-157).  out_masks: n * ceil(T_max/64) words with row stride `stride_words`.
int ksh_price_filter(void** hv, uint32_t n, const uint32_t* node, const double* max_price, const uint32_t* spot_only, uint64_t* out_masks, uint32_t stride_words, uint32_t* out_counts) {
  return guarded([&] {
    std::vector<ks_dev_problem*> ds; std::vector<uint64_t*> outs(n);
    int rc = device_problems(hv, n, true, "price filter before solve", ds); if (rc != KS_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) {
      if ((((Handle*)hv[i])->enc->prob.T + 63) / 64 > stride_words) return set_err(KS_ERR_INVALID, "mask row too short");
      outs[i] = out_masks + (size_t)i * stride_words;
    }
    return dev_rc(ks_price_filter_dev(ds.data(), n, node, max_price, spot_only, outs.data(), out_counts));
  });
}

// Launch-time pick of the in-memory provider (fake/cloudprovider.go:79-84) and instanceTypesAreSubset (helpers.go:118-122) on results that are
// still on the device.  launch pick: out_type = instance-type index (into the problem's catalogue) or -1, out_zone / out_ct = value ids in the zone /
// capacity-type universes (ksh_key_value resolves them), out_price.
int ksh_launch_pick(void** hv, uint32_t n, const uint32_t* node, int32_t* out_type, int32_t* out_zone, int32_t* out_ct, double* out_price) {
  return guarded([&] {
    std::vector<ks_dev_problem*> ds; std::vector<int32_t> pair(n);
    int rc = device_problems(hv, n, true, "launch pick before solve", ds); if (rc != KS_OK) return rc;
    rc = dev_rc(ks_launch_pick_dev(ds.data(), n, node, out_type, pair.data(), out_price)); if (rc != KS_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) { const uint32_t nct = ((Handle*)hv[i])->enc->prob.n_ct; out_zone[i] = pair[i] < 0 ? -1 : pair[i] / (int32_t)nct; out_ct[i] = pair[i] < 0 ? -1 : pair[i] % (int32_t)nct; }
    return KS_OK;
  });
}
// value `v` of the zone (which = 0) or capacity-type (which = 1) universe of the handle's problem; NULL when out of range (owned by the handle)
const char* ksh_key_value(void* hv, int which, int32_t v) {
  const ksh::Encoded& E = ((Handle*)hv)->enc->names(); const int32_t k = which == 0 ? E.prob.key_zone : E.prob.key_ct;
  if (k < 0 || v < 0 || (size_t)v >= E.key_values[k].size()) return nullptr;
  return E.key_values[k][v].c_str();
}
int ksh_types_subset(void** hv, uint32_t n, const uint32_t* node, const uint64_t* lhs, uint32_t stride_words, uint32_t* out) {
  return guarded([&] {
    std::vector<ks_dev_problem*> ds;
    int rc = device_problems(hv, n, true, "subset test before solve", ds); if (rc != KS_OK) return rc;
    return dev_rc(ks_types_subset_dev(ds.data(), n, node, lhs, stride_words, out));
  });
}

// Static feasibility grid [M][C][TW]; `out` may be NULL (timing only).
int ksh_grid(void* hv, uint64_t* out, float* kernel_ms) {
  Handle* h = (Handle*)hv; int rc = ensure_resident(h); if (rc != KS_OK) return rc;
  return dev_rc(ks_feasibility_grid(h->dev, out, kernel_ms));
}

// The grid's rows split over GPUs: a range of rows computed on the handle's device / rows computed elsewhere installed.
int ksh_grid_rows(void* hv, uint32_t row_lo, uint32_t row_hi, uint64_t* out_rows, void* out_rows_dev, float* kernel_ms) {
  Handle* h = (Handle*)hv; int rc = ensure_resident(h); if (rc != KS_OK) return rc;
  return dev_rc(ks_feasibility_grid_rows(h->dev, row_lo, row_hi, out_rows, out_rows_dev, kernel_ms));
}
int ksh_grid_install(void* hv, uint32_t row_lo, uint32_t row_hi, const uint64_t* rows, const void* rows_dev, int complete) {
  Handle* h = (Handle*)hv; int rc = ensure_resident(h); if (rc != KS_OK) return rc;
  return dev_rc(ks_feasibility_grid_install(h->dev, row_lo, row_hi, rows, rows_dev, complete));
}

// Diagnostics: the grid as the last build left it (nothing launched), and the class row of every pod as submitted (stage 0 of its relaxation chain).
int ksh_debug_grid(void* hv, uint64_t* out) {
  Handle* h = (Handle*)hv; if (!h || !h->dev) return set_err(KS_ERR_INVALID, "grid of a handle that was not uploaded");
  return dev_rc(ks_debug_grid(h->dev, out));
}
int ksh_debug_pod_classes(void* hv, uint32_t* out) {
  Handle* h = (Handle*)hv; if (!h || !out) return set_err(KS_ERR_INVALID, "null argument");
  if (h->enc->view) return set_err(KS_ERR_UNSUPPORTED, "a what-if derived on the device has no flattening of its own");
  const ks_problem& p = h->enc->prob;
  for (uint32_t i = 0; i < p.P; ++i) out[i] = p.stage_cls[p.pod_stage_off[i]];
  return KS_OK;
}

// One-shot convenience: KSP1 text in, KSR1 text out.
int ksh_solve_ksp(const char* ksp_text, size_t len, uint32_t flags, char** out_text) {
  void* h = nullptr; int rc = ksh_open(ksp_text, len, flags, &h); if (rc != KS_OK) return rc;
  rc = ksh_solve(h, out_text, nullptr, nullptr); ksh_close(h); return rc;
}

extern "C" int ks_debug_classes(ks_dev_problem*, void*, void*);
int ksh_debug_classes(void* hv, void* briefs, void* plans) {
  Handle* h = (Handle*)hv; if (!h || !h->dev) return set_err(KS_ERR_INVALID, "class tables of a handle that was not uploaded");
  const int rc = ks_debug_classes(h->dev, briefs, plans);
  if (rc < 0) return set_err(rc, ks_last_error());
  return rc;
}

// dims for tests / bench: [P,C,T,M,E,K,R,G,GH,S]
// The result as ARRAYS (round 5): what scheduler.Solve returns -- Node.Pods in commit order, InstanceTypeOptions, Requests, Requirements, the relaxation stage every pod
// ended at, the per-pod failure reasons -- without a text round trip.  Pointers into the handle's own result buffers: valid until the handle is solved again or closed.
int ksh_result_arrays_get(void* hv, ksh_result_arrays* out) {
  Handle* h = (Handle*)hv;
  if (!h || !out) return set_err(KS_ERR_INVALID, "null argument");
  if (!h->solved || !h->rb) return set_err(KS_ERR_INVALID, "result arrays before a solve");
  if (h->delta) return set_err(KS_ERR_UNSUPPORTED, "a what-if derived on the device numbers its pods in the snapshot's queue order: read it through ksh_result_text / ksh_result_summaries");
  return guarded([&] {
    const ks_problem& p = h->enc->prob; const ks_result& r = h->rb->r;
    const uint32_t nn = p.E + r.n_new;
    h->csr_off.assign((size_t)nn + 1, 0);
    uint32_t placed = 0;
    for (uint32_t i = 0; i < p.P; ++i) if (r.pod_node[i] >= 0) { h->csr_off[(size_t)r.pod_node[i] + 1]++; ++placed; }
    for (uint32_t n = 0; n < nn; ++n) h->csr_off[n + 1] += h->csr_off[n];
    // commit order within a node = ascending commit number; the numbers are unique over the Solve, so one pass in that order fills every node's list in place
    std::vector<int32_t> by_seq(placed, -1);
    for (uint32_t i = 0; i < p.P; ++i) if (r.pod_node[i] >= 0) { const int32_t sq = r.pod_seq[i]; if (sq < 0 || (uint32_t)sq >= placed || by_seq[sq] >= 0) return set_err(KS_ERR_INTERNAL, "commit numbers are not a permutation"); by_seq[sq] = (int32_t)i; }
    h->csr_pods.assign(placed, -1);
    { std::vector<uint32_t> fill(h->csr_off.begin(), h->csr_off.end() - 1); for (uint32_t sq = 0; sq < placed; ++sq) { const int32_t i = by_seq[sq]; h->csr_pods[fill[r.pod_node[i]]++] = i; } }
    memset(out, 0, sizeof *out);
    out->n_pods = p.P; out->n_existing = p.E; out->n_new = r.n_new; out->n_unscheduled = r.n_unscheduled; out->types_words = (p.T + 63) / 64; out->n_resources = p.R; out->n_keys = p.K;
    out->pod_node = r.pod_node; out->pod_stage = r.pod_stage; out->pod_reason = r.pod_reason; out->unscheduled = r.unscheduled;
    out->node_pods_off = h->csr_off.data(); out->node_pods = h->csr_pods.data();
    out->node_tmpl = r.node_tmpl; out->node_types = r.node_types; out->node_requests = r.node_requests; out->node_requests_present = r.node_requests_present;
    out->node_present = r.node_present; out->node_complement = r.node_complement; out->node_mask = r.node_mask; out->node_gt = r.node_gt; out->node_lt = r.node_lt; out->node_it_state = r.node_it_state;
    return KS_OK;
  });
}
// the names behind the arrays: requirement key k, its interned value v (a value class names its first member; ksh_result_text lists every member), resource r;
// NULL when out of range (owned by the handle)
const char* ksh_name(void* hv, int what /* 0 key, 1 value of key a, 2 resource */, uint32_t a, uint32_t b) {
  const ksh::Encoded& E = ((Handle*)hv)->enc->names();
  if (what == 0) return a < E.key_names.size() ? E.key_names[a].c_str() : nullptr;
  if (what == 1) return (a < E.key_values.size() && b < E.key_values[a].size()) ? E.key_values[a][b].c_str() : nullptr;
  if (what == 2) return a < E.res_names.size() ? E.res_names[a].c_str() : nullptr;
  return nullptr;
}
// The what-if fan-out in one call (ks_solve_batch_sharded): shard s = handles[shard_off[s] .. shard_off[s + 1]) (every handle of a shard uploaded to the same device),
// ids[] names each handle's what-if; out_rows[n][3 + words] comes back ordered by id.
int ksh_solve_whatifs_sharded(void** hv, const uint32_t* shard_off, uint32_t nshards, const uint64_t* ids, uint32_t words, uint64_t* out_rows, float* kernel_ms_max) {
  if (!hv || !shard_off || !ids || !out_rows) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    const uint32_t n = shard_off[nshards];
    std::vector<ks_dev_problem*> ds;
    int rc = device_problems(hv, n, false, "a what-if that is not resident (ksh_upload / ksh_upload_batch / ksh_open_whatifs_derived first)", ds); if (rc != KS_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) { ((Handle*)hv[i])->solved = false; ((Handle*)hv[i])->dev_result = false; }
    std::vector<ks_dev_problem* const*> sp(nshards); std::vector<uint32_t> sn(nshards); std::vector<const uint64_t*> si(nshards);
    for (uint32_t s = 0; s < nshards; ++s) { sp[s] = ds.data() + shard_off[s]; sn[s] = shard_off[s + 1] - shard_off[s]; si[s] = ids + shard_off[s]; }
    rc = dev_rc(ks_solve_batch_sharded(sp.data(), sn.data(), si.data(), nshards, words, out_rows, kernel_ms_max)); if (rc != KS_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) ((Handle*)hv[i])->dev_result = true;
    return KS_OK;
  });
}

// ---- consolidation commands (kshost.h): computeConsolidation / firstNNodeConsolidationOption / SingleNodeConsolidation.ComputeCommand over a snapshot ----
// The rows of handles that hold a result on the device (any route: derived, flattened one by one, a plain Solve): ks_consolidation_commands_host for handles.
int ksh_command_rows(void** hv, uint32_t n, const uint64_t* ids, const ks_command_inputs* in, uint32_t words, uint64_t* out_rows, double* ms) {
  if (n && !hv) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    std::vector<ks_dev_problem*> ds;
    int rc = device_problems(hv, n, true, "command rows before solve", ds); if (rc != KS_OK) return rc;
    return dev_rc(ks_consolidation_commands_host(ds.data(), n, ids, in, words, out_rows, ms));
  });
}
// The two tables of handles that hold a result on the device: ks_replacement_commands_host for handles.
int ksh_replacement_rows(void** hv, uint32_t n, const uint64_t* ids, const uint32_t* flags, uint32_t words, uint64_t* out_heads, uint64_t* out_nodes, uint64_t cap_nodes, uint64_t* out_total_nodes, double* ms) {
  if (n && !hv) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    std::vector<ks_dev_problem*> ds;
    int rc = device_problems(hv, n, true, "replacement rows before solve", ds); if (rc != KS_OK) return rc;
    return dev_rc(ks_replacement_commands_host(ds.data(), n, ids, flags, words, out_heads, out_nodes, cap_nodes, out_total_nodes, ms));
  });
}
// The placement tables of handles that hold a result on the device: ks_placement_rows_host for handles, then -- on the host, a pass over the rows that came back --
// the rows of a what-if over a snapshot renamed to the snapshot's own stable ids: existing-node row e -> the node's slot (a derived what-if: the snapshot's
// flattening's rows; a what-if flattened by itself: its own), new node j -> node slots + j, and for a what-if flattened by itself batch pod i -> the snapshot's pod
// (a derived one's rows name snapshot pods already: pod_gid).  The head's KS_PLC_N_EXISTING becomes the number of node slots, so `where` reads the same way.
int ksh_placement_rows(void** hv, uint32_t n, const uint64_t* ids, uint64_t* out_heads, uint64_t* out_rows, uint64_t cap_rows, uint64_t* out_total_rows, double* ms) {
  if (ms) ms[0] = ms[1] = 0.0;
  if (!out_total_rows || (n && (!hv || !ids || !out_heads)) || (cap_rows && !out_rows)) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    std::vector<ks_dev_problem*> ds;
    int rc = device_problems(hv, n, true, "placement rows before solve", ds); if (rc != KS_OK) return rc;
    rc = dev_rc(ks_placement_rows_host(ds.data(), n, ids, out_heads, out_rows, cap_rows, out_total_rows, ms)); if (rc != KS_OK) return rc;
    const auto t0 = clk::now();
    for (uint32_t i = 0; i < n; ++i) {
      const Handle* h = (const Handle*)hv[i]; uint64_t* head = out_heads + (size_t)i * KS_PLC_HEAD_WORDS;
      if (!h->snapshot_whatif) continue;      // any other problem -- a Solve over the environment cache included -- keeps its own pod and existing-node indices, as ksh_result_arrays_get gives them
      const std::vector<int>& slot_of = h->enc->view ? h->enc->shared->existing : h->enc->existing;
      const uint32_t E = (uint32_t)head[KS_PLC_N_EXISTING], slots = (uint32_t)h->enc->src->nodes.size();
      if (!h->enc->shared || !h->enc->src || slot_of.size() != E || (!h->enc->view && h->pod_ids.size() != head[KS_PLC_P])) return set_err(KS_ERR_INTERNAL, "placement rows: the what-if's tables do not match its flattening");
      head[KS_PLC_N_EXISTING] = slots;
      if (head[KS_PLC_FLAGS] & KS_PLC_TRUNCATED) continue;
      uint64_t* row = out_rows + (size_t)head[KS_PLC_ROW_OFF] * KS_PLC_ROW_WORDS;
      for (uint64_t k = 0; k < head[KS_PLC_P]; ++k, row += KS_PLC_ROW_WORDS) {
        uint32_t pod = (uint32_t)row[KS_PLC_POD_WHERE]; int32_t where = (int32_t)(uint32_t)(row[KS_PLC_POD_WHERE] >> 32);
        if (!h->enc->view) { if (pod >= h->pod_ids.size()) return set_err(KS_ERR_INTERNAL, "placement rows: pod index out of range"); pod = h->pod_ids[pod]; }
        if (where >= 0) where = (uint32_t)where < E ? (int32_t)slot_of[(uint32_t)where] : (int32_t)(slots + ((uint32_t)where - E));
        row[KS_PLC_POD_WHERE] = (uint64_t)pod | ((uint64_t)(uint32_t)where << 32);
      }
    }
    if (ms) ms[1] += ms_since(t0);
    return KS_OK;
  });
}
}  // extern "C"
// The audit's eight passes (kshost.h ksh_audit* / ksh_audit*_claimed).  What a pass is to this file: its table in libksolve and in kshost.h, whether it has a node
// table beside the pod table, its two entry points in libksolve, whether its claimed form comes without commit numbers, and the totals it copies.
namespace {
struct AuditFirst {
  using Dev = ks_audit; using Out = ksh_audit_out; static constexpr bool nodes = true, no_pod_seq = true;
  static constexpr auto batch_dev = ks_audit_batch_dev; static constexpr auto one_dev = ks_audit_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_nodes = r.n_nodes; o->n_new = r.n_new; o->n_unscheduled = r.n_unscheduled; o->n_pods_flagged = r.n_pods_flagged; o->n_nodes_flagged = r.n_nodes_flagged; o->pad = 0;
    memcpy(o->pod_bit_count, r.pod_bit_count, sizeof o->pod_bit_count); memcpy(o->node_bit_count, r.node_bit_count, sizeof o->node_bit_count);
  }
};
struct AuditTopology {
  using Dev = ks_audit_topology; using Out = ksh_audit_topology_out; static constexpr bool nodes = false, no_pod_seq = false;
  static constexpr auto batch_dev = ks_audit_topology_batch_dev; static constexpr auto one_dev = ks_audit_topology_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_new = r.n_new; o->n_placed = r.n_placed; o->skipped_groups = r.skipped_groups; o->n_pods_flagged = r.n_pods_flagged;
    memcpy(o->checked, r.checked, sizeof o->checked); memcpy(o->pod_bit_count, r.pod_bit_count, sizeof o->pod_bit_count);
  }
};
struct AuditSpread {
  using Dev = ks_audit_spread; using Out = ksh_audit_spread_out; static constexpr bool nodes = false, no_pod_seq = false;
  static constexpr auto batch_dev = ks_audit_spread_batch_dev; static constexpr auto one_dev = ks_audit_spread_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_new = r.n_new; o->n_placed = r.n_placed; o->skipped_groups = r.skipped_groups; o->n_pods_flagged = r.n_pods_flagged;
    memcpy(o->checked, r.checked, sizeof o->checked); o->exact_pairs = r.exact_pairs; o->pad = 0;
  }
};
struct AuditFirstFit {
  using Dev = ks_audit_firstfit; using Out = ksh_audit_firstfit_out; static constexpr bool nodes = false, no_pod_seq = false;
  static constexpr auto batch_dev = ks_audit_firstfit_batch_dev; static constexpr auto one_dev = ks_audit_firstfit_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_new = r.n_new; o->n_placed = r.n_placed; o->skipped_pods = r.skipped_pods; o->n_pods_flagged = r.n_pods_flagged;
    memcpy(o->checked, r.checked, sizeof o->checked); o->admitting_pairs = r.admitting_pairs;
  }
};
struct AuditLimits {
  using Dev = ks_audit_limits; using Out = ksh_audit_limits_out; static constexpr bool nodes = true, no_pod_seq = false;
  static constexpr auto batch_dev = ks_audit_limits_batch_dev; static constexpr auto one_dev = ks_audit_limits_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_nodes = r.n_nodes; o->n_new = r.n_new; o->n_placed = r.n_placed; o->limited_templates = r.limited_templates; o->skipped_nodes = r.skipped_nodes;
    o->skipped_pods = r.skipped_pods; o->n_pods_flagged = r.n_pods_flagged; o->n_nodes_flagged = r.n_nodes_flagged; o->exact_nodes = r.exact_nodes; o->binding_nodes = r.binding_nodes;
    memcpy(o->checked, r.checked, sizeof o->checked); memcpy(o->pod_bit_count, r.pod_bit_count, sizeof o->pod_bit_count); memcpy(o->node_bit_count, r.node_bit_count, sizeof o->node_bit_count);
  }
};
struct AuditHostFit {
  using Dev = ks_audit_hostfit; using Out = ksh_audit_hostfit_out; static constexpr bool nodes = false, no_pod_seq = false;
  static constexpr auto batch_dev = ks_audit_hostfit_batch_dev; static constexpr auto one_dev = ks_audit_hostfit_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_new = r.n_new; o->n_placed = r.n_placed; o->skipped_pods = r.skipped_pods; o->n_pods_flagged = r.n_pods_flagged;
    o->eligible_groups = r.eligible_groups; o->skipped_groups = r.skipped_groups; memcpy(o->checked, r.checked, sizeof o->checked); o->admitting_pairs = r.admitting_pairs; o->pad = 0;
  }
};
struct AuditZoneFit {
  using Dev = ks_audit_zonefit; using Out = ksh_audit_zonefit_out; static constexpr bool nodes = false, no_pod_seq = false;
  static constexpr auto batch_dev = ks_audit_zonefit_batch_dev; static constexpr auto one_dev = ks_audit_zonefit_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_new = r.n_new; o->n_placed = r.n_placed; o->skipped_pods = r.skipped_pods; o->n_pods_flagged = r.n_pods_flagged;
    o->eligible_groups = r.eligible_groups; o->skipped_groups = r.skipped_groups; o->mixed_pods = r.mixed_pods; o->exact_pods = r.exact_pods;
    memcpy(o->checked, r.checked, sizeof o->checked); o->admitting_pairs = r.admitting_pairs; o->pad = 0;
  }
};
struct AuditStages {
  using Dev = ks_audit_stages; using Out = ksh_audit_stages_out; static constexpr bool nodes = false, no_pod_seq = false;
  static constexpr auto batch_dev = ks_audit_stages_batch_dev; static constexpr auto one_dev = ks_audit_stages_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_new = r.n_new; o->n_placed = r.n_placed; o->skipped_pods = r.skipped_pods; o->n_pods_flagged = r.n_pods_flagged;
    memcpy(o->checked, r.checked, sizeof o->checked); o->admitting_pairs = r.admitting_pairs; o->pad = 0;
  }
};
struct AuditReasons {
  using Dev = ks_audit_reasons; using Out = ksh_audit_reasons_out; static constexpr bool nodes = false, no_pod_seq = true, reads_reason = true;
  static constexpr auto batch_dev = ks_audit_reasons_batch_dev; static constexpr auto one_dev = ks_audit_reasons_dev;
  static void totals(const Dev& r, Out* o) {
    o->n_pods = r.n_pods; o->n_new = r.n_new; o->n_placed = r.n_placed; o->n_unscheduled = r.n_unscheduled; o->skipped_pods = r.skipped_pods; o->n_pods_flagged = r.n_pods_flagged;
    o->used_classes = r.used_classes; memcpy(o->checked, r.checked, sizeof o->checked); o->pairs = r.pairs; o->pad = 0;
  }
};
// does the pass's claimed form read pod_reason (and neither the unscheduled list nor commit numbers)?  Only a pass that says so
template <class P, class = void> struct audit_reads_reason : std::false_type {};
template <class P> struct audit_reads_reason<P, std::void_t<decltype(P::reads_reason)>> : std::true_type {};
// A pass's tables: libksolve fills tables of the library's own, sized from the device problems; the totals always reach the caller, the flag rows only when they fit
template <class P> struct AuditTables {
  using Dev = typename P::Dev;
  std::vector<Dev> a; std::vector<Dev*> ptr; std::vector<std::vector<uint32_t>> pf, nf;
  int size(const std::vector<ks_dev_problem*>& ds) {
    const size_t n = ds.size(); a.assign(n, Dev{}); ptr.resize(n); pf.resize(n); nf.resize(n);
    for (size_t i = 0; i < n; ++i) {
      uint32_t np = 0, ns = 0; int rc = dev_rc(ks_audit_sizes(ds[i], &np, P::nodes ? &ns : nullptr)); if (rc != KS_OK) return rc;
      pf[i].assign(np, 0); a[i].pod_flags = pf[i].data(); ptr[i] = &a[i];
      if constexpr (P::nodes) { nf[i].assign(ns, 0); a[i].node_flags = nf[i].data(); }
    }
    return KS_OK;
  }
  void give(size_t i, typename P::Out* o, double* ms) const {
    const Dev& r = a[i];
    P::totals(r, o); o->truncated = 0;
    if (o->cap_pods >= r.n_pods) { if (r.n_pods) memcpy(o->pod_flags, r.pod_flags, (size_t)r.n_pods * sizeof(uint32_t)); } else o->truncated |= KSH_AUDIT_TRUNCATED_PODS;
    if constexpr (P::nodes) { if (o->cap_nodes >= r.n_nodes) { if (r.n_nodes) memcpy(o->node_flags, r.node_flags, (size_t)r.n_nodes * sizeof(uint32_t)); } else o->truncated |= KSH_AUDIT_TRUNCATED_NODES; }
    if (ms) { ms[0] = r.kernel_ms; ms[1] = r.readback_ms; }
  }
};
template <class P> bool audit_out_ok(const typename P::Out* o) {
  if (!o || (o->cap_pods && !o->pod_flags)) return false;
  if constexpr (P::nodes) return !o->cap_nodes || o->node_flags;
  return true;
}
// the results the last solves left on the device, for handles of any kind
template <class P> int audit_resident(void** hv, uint32_t n, typename P::Out* outs, double* ms) {
  zero(ms, 2);
  if (n && (!hv || !outs)) return set_err(KS_ERR_INVALID, "null argument");
  for (uint32_t i = 0; i < n; ++i) if (!audit_out_ok<P>(&outs[i])) return set_err(KS_ERR_INVALID, "null audit table");
  if (!n) return KS_OK;
  return guarded([&] {
    std::vector<ks_dev_problem*> ds;
    int rc = device_problems(hv, n, true, "audit before solve", ds); if (rc != KS_OK) return rc;
    AuditTables<P> t; rc = t.size(ds); if (rc != KS_OK) return rc;
    rc = dev_rc(P::batch_dev(ds.data(), n, t.ptr.data())); if (rc != KS_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) t.give(i, &outs[i], ms);
    return KS_OK;
  });
}
// The refusals about a claimed result's dimensions, then ks_result's shape over the caller's arrays.  lists_unscheduled: the pass reads the unscheduled list
int claimed_result(const ks_problem& p, const ksh_result_arrays* c, bool lists_unscheduled, const int32_t* pod_seq, ks_result* r) {
  const uint32_t TW = (p.T + 63) / 64;
  if (c->n_pods != p.P || c->n_existing != p.E || c->types_words != TW || c->n_resources != p.R || c->n_keys != p.K) return set_err(KS_ERR_INVALID, "claimed result: its dimensions are not the handle's");
  if (c->n_new > p.max_new_nodes) return set_err(KS_ERR_INVALID, "claimed result: more new nodes than max_new_nodes");
  if (c->n_unscheduled > p.P) return set_err(KS_ERR_INVALID, "claimed result: more unscheduled pods than pods");
  if ((p.P && (!c->pod_node || !c->pod_stage)) || (lists_unscheduled && c->n_unscheduled && !c->unscheduled)) return set_err(KS_ERR_INVALID, "claimed result: null array");
  *r = ks_result{}; r->pod_node = (int32_t*)c->pod_node; r->pod_stage = (int32_t*)c->pod_stage; r->pod_seq = (int32_t*)pod_seq;
  r->n_new = c->n_new; r->n_unscheduled = c->n_unscheduled;
  r->node_tmpl = (int32_t*)c->node_tmpl; r->node_types = (uint64_t*)c->node_types; r->node_requests = (int64_t*)c->node_requests; r->node_requests_present = (uint32_t*)c->node_requests_present;
  r->node_present = (uint32_t*)c->node_present; r->node_complement = (uint32_t*)c->node_complement; r->node_mask = (uint64_t*)c->node_mask; r->node_gt = (int32_t*)c->node_gt; r->node_lt = (int32_t*)c->node_lt;
  r->node_it_state = (int32_t*)c->node_it_state;
  return KS_OK;
}
// a claimed result for one flattened handle; pod_seq: the commit numbers, for every pass but the first
template <class P> int audit_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, typename P::Out* out, double* ms) {
  zero(ms, 2);
  Handle* h = (Handle*)hv;
  if (!h || !c || (!P::no_pod_seq && !pod_seq)) return set_err(KS_ERR_INVALID, "null argument");
  if (!audit_out_ok<P>(out)) return set_err(KS_ERR_INVALID, "null audit table");
  if (h->delta || h->enc->view) return set_err(KS_ERR_UNSUPPORTED, "a claimed result is audited against a flattened problem, not against a what-if derived on the device");
  return guarded([&] {
    const ks_problem& p = h->enc->prob; ks_result r;
    constexpr bool reasons = audit_reads_reason<P>::value;
    int rc = claimed_result(p, c, P::no_pod_seq && !reasons, pod_seq, &r); if (rc != KS_OK) return rc;
    if (reasons) r.pod_reason = (uint32_t*)c->pod_reason;
    rc = ensure_resident(h); if (rc != KS_OK) return rc;
    std::vector<int32_t> seq, un;
    if (P::no_pod_seq && !reasons) {
      // ks_result's shape: the unscheduled list in an array of P, and commit numbers -- ksh_result_arrays has none, so placed pods are numbered in pod order
      seq.assign((size_t)p.P + 1, -1); un.assign((size_t)p.P + 1, -1);
      { int32_t k = 0; for (uint32_t i = 0; i < p.P; ++i) if (c->pod_node[i] != -1) seq[i] = k++; }
      for (uint32_t i = 0; i < c->n_unscheduled; ++i) un[i] = c->unscheduled[i];
      r.pod_seq = seq.data(); r.unscheduled = un.data();
    }
    std::vector<ks_dev_problem*> ds{h->dev};
    AuditTables<P> t; rc = t.size(ds); if (rc != KS_OK) return rc;
    rc = dev_rc(P::one_dev(h->dev, &r, t.ptr[0])); if (rc != KS_OK) return rc;
    t.give(0, out, ms);
    return KS_OK;
  });
}
// The gate (kshost.h ksh_audit_gate_ex / ksh_audit_gate_ex_claimed, and ksh_audit_gate / ksh_audit_gate_claimed: the same bodies over the old struct as the wide one's
// first version): X(the pass's mask bit, its traits, its member of ks_audit_gate_ex, its member of ksh_audit_gate_ex_out).
// libksolve fills out structs of the library's own -- no tables in them -- and every requested pass's totals reach the caller through the pass's own `totals`.
#define KSH_AUDIT_GATE_PASSES(X) \
  X(KS_AUDIT_PASS_FIRST, AuditFirst, first, audit) X(KS_AUDIT_PASS_TOPOLOGY, AuditTopology, topology, topology) X(KS_AUDIT_PASS_SPREAD, AuditSpread, spread, spread) \
  X(KS_AUDIT_PASS_FIRSTFIT, AuditFirstFit, firstfit, firstfit) X(KS_AUDIT_PASS_LIMITS, AuditLimits, limits, limits) X(KS_AUDIT_PASS_HOSTFIT, AuditHostFit, hostfit, hostfit) \
  X(KS_AUDIT_PASS_STAGES, AuditStages, stages, stages) X(KS_AUDIT_PASS_REASONS, AuditReasons, reasons, reasons)
const uint32_t KSH_AUDIT_GATE_EX_BASE = (uint32_t)offsetof(ksh_audit_gate_ex_out, stages);      // the least struct_size: everything ksh_audit_gate_out carries
// the bits a caller of this struct_size can ask for: within KS_AUDIT_PASS_ALL_EX, the pointer wholly within the struct
uint32_t audit_gate_known(uint32_t struct_size) {
  uint32_t known = 0;
#define X(bit, P, km, hm) if (offsetof(ksh_audit_gate_ex_out, hm) + sizeof(void*) <= struct_size) known |= bit;
  KSH_AUDIT_GATE_PASSES(X)
#undef X
  return known & KS_AUDIT_PASS_ALL_EX;
}
// the gate's own refusals, before any pass's
int audit_gate_ok(uint32_t passes, const ksh_audit_gate_ex_out* out) {
  if (!out) return set_err(KS_ERR_INVALID, "null argument");
  if (out->struct_size < KSH_AUDIT_GATE_EX_BASE) return set_err(KS_ERR_INVALID, "audit gate: struct_size is less than the struct's first version");
  if (!passes) return set_err(KS_ERR_INVALID, "audit gate: no pass requested");
  if (passes & ~audit_gate_known(out->struct_size)) return set_err(KS_ERR_INVALID, "audit gate: unknown pass");
  if (out->cap_findings && !out->findings) return set_err(KS_ERR_INVALID, "audit gate: null findings table");
#define X(bit, P, km, hm) if ((passes & bit) && !out->hm) return set_err(KS_ERR_INVALID, "null argument");
  KSH_AUDIT_GATE_PASSES(X)
#undef X
  return KS_OK;
}
// dev_call(gate): the call into libksolve, over tables of n structs per requested pass
template <class F> int audit_gate_call(uint32_t n, uint32_t passes, ksh_audit_gate_ex_out* out, double* ms, F&& dev_call) {
  ks_audit_gate_ex g{}; g.struct_size = (uint32_t)sizeof g; g.passes = passes; g.findings = out->findings; g.cap_findings = (uint32_t)std::min<uint64_t>(out->cap_findings, 0xFFFFFFFFu);
#define X(bit, P, km, hm) std::vector<P::Dev> v_##km; if (passes & bit) { v_##km.assign(n, P::Dev{}); g.km = v_##km.data(); }
  KSH_AUDIT_GATE_PASSES(X)
#undef X
  int rc = dev_rc(dev_call(&g)); if (rc != KS_OK) return rc;
#define X(bit, P, km, hm) if (passes & bit) for (uint32_t i = 0; i < n; ++i) { P::totals(v_##km[i], &out->hm[i]); out->hm[i].truncated = 0; }
  KSH_AUDIT_GATE_PASSES(X)
#undef X
  out->n_findings = g.n_findings; out->truncated = g.truncated;
  if (ms) { ms[0] = g.kernel_ms; ms[1] = g.readback_ms; }
  return KS_OK;
}
// the two entry bodies, over the wide struct
int audit_gate_resident(void** hv, uint32_t n, uint32_t passes, ksh_audit_gate_ex_out* out, double* ms) {
  zero(ms, 2);
  int rc = audit_gate_ok(passes, out); if (rc != KS_OK) return rc;
  if (n && !hv) return set_err(KS_ERR_INVALID, "null argument");
  if (!n) { out->n_findings = 0; out->truncated = 0; return KS_OK; }
  return guarded([&] {
    std::vector<ks_dev_problem*> ds;
    int rc = device_problems(hv, n, true, "audit before solve", ds); if (rc != KS_OK) return rc;
    return audit_gate_call(n, passes, out, ms, [&](ks_audit_gate_ex* g) { return ks_audit_gate_ex_batch_dev(ds.data(), n, g); });
  });
}
int audit_gate_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, uint32_t passes, ksh_audit_gate_ex_out* out, double* ms) {
  zero(ms, 2);
  int rc = audit_gate_ok(passes, out); if (rc != KS_OK) return rc;
  Handle* h = (Handle*)hv; const bool first = passes & KS_AUDIT_PASS_FIRST;
  if (!h || !c || ((passes & ~(KS_AUDIT_PASS_FIRST | KS_AUDIT_PASS_REASONS)) && !pod_seq)) return set_err(KS_ERR_INVALID, "null argument");      // (the two passes that take no commit numbers)
  if (h->delta || h->enc->view) return set_err(KS_ERR_UNSUPPORTED, "a claimed result is audited against a flattened problem, not against a what-if derived on the device");
  return guarded([&] {
    const ks_problem& p = h->enc->prob; ks_result r;
    int rc = claimed_result(p, c, first, pod_seq, &r); if (rc != KS_OK) return rc;
    if (passes & KS_AUDIT_PASS_REASONS) r.pod_reason = (uint32_t*)c->pod_reason;      // (read by that pass alone; its null is that pass's refusal, in libksolve's order)
    rc = ensure_resident(h); if (rc != KS_OK) return rc;
    std::vector<int32_t> seq, un;
    if (first) {      // (what ksh_audit_claimed gives the first pass: the unscheduled list in an array of P, the placed pods numbered in pod order)
      seq.assign((size_t)p.P + 1, -1); un.assign((size_t)p.P + 1, -1);
      { int32_t k = 0; for (uint32_t i = 0; i < p.P; ++i) if (c->pod_node[i] != -1) seq[i] = k++; }
      for (uint32_t i = 0; i < c->n_unscheduled; ++i) un[i] = c->unscheduled[i];
      r.unscheduled = un.data(); if (!pod_seq) r.pod_seq = seq.data();
    }
    return audit_gate_call(1, passes, out, ms, [&](ks_audit_gate_ex* g) { g->first_pod_seq = first && pod_seq ? seq.data() : nullptr; return ks_audit_gate_ex_dev(h->dev, &r, g); });
  });
}
// the old struct as the wide one's first version: struct_size ends before `stages`, so the six bits are all it knows; the counts come back on success alone
template <class F> int audit_gate_six(ksh_audit_gate_out* out, double* ms, F&& body) {
  if (!out) { zero(ms, 2); return set_err(KS_ERR_INVALID, "null argument"); }
  ksh_audit_gate_ex_out x{}; x.struct_size = KSH_AUDIT_GATE_EX_BASE; x.findings = out->findings; x.cap_findings = out->cap_findings;
  x.audit = out->audit; x.topology = out->topology; x.spread = out->spread; x.firstfit = out->firstfit; x.limits = out->limits; x.hostfit = out->hostfit;
  int rc = body(&x); if (rc != KS_OK) return rc;
  out->n_findings = x.n_findings; out->truncated = x.truncated;
  return KS_OK;
}
}  // namespace
extern "C" {
int ksh_audit_gate(void** hv, uint32_t n, uint32_t passes, ksh_audit_gate_out* out, double* ms) {
  return audit_gate_six(out, ms, [&](ksh_audit_gate_ex_out* x) { return audit_gate_resident(hv, n, passes, x, ms); });
}
int ksh_audit_gate_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, uint32_t passes, ksh_audit_gate_out* out, double* ms) {
  return audit_gate_six(out, ms, [&](ksh_audit_gate_ex_out* x) { return audit_gate_claimed(hv, c, pod_seq, passes, x, ms); });
}
int ksh_audit_gate_ex(void** hv, uint32_t n, uint32_t passes, ksh_audit_gate_ex_out* out, double* ms) { return audit_gate_resident(hv, n, passes, out, ms); }
int ksh_audit_gate_ex_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, uint32_t passes, ksh_audit_gate_ex_out* out, double* ms) { return audit_gate_claimed(hv, c, pod_seq, passes, out, ms); }
int ksh_audit(void** hv, uint32_t n, ksh_audit_out* outs, double* ms) { return audit_resident<AuditFirst>(hv, n, outs, ms); }
int ksh_audit_claimed(void* hv, const ksh_result_arrays* c, ksh_audit_out* out, double* ms) { return audit_claimed<AuditFirst>(hv, c, nullptr, out, ms); }
int ksh_audit_topology(void** hv, uint32_t n, ksh_audit_topology_out* outs, double* ms) { return audit_resident<AuditTopology>(hv, n, outs, ms); }
int ksh_audit_topology_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, ksh_audit_topology_out* out, double* ms) { return audit_claimed<AuditTopology>(hv, c, pod_seq, out, ms); }
int ksh_audit_spread(void** hv, uint32_t n, ksh_audit_spread_out* outs, double* ms) { return audit_resident<AuditSpread>(hv, n, outs, ms); }
int ksh_audit_spread_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, ksh_audit_spread_out* out, double* ms) { return audit_claimed<AuditSpread>(hv, c, pod_seq, out, ms); }
int ksh_audit_firstfit(void** hv, uint32_t n, ksh_audit_firstfit_out* outs, double* ms) { return audit_resident<AuditFirstFit>(hv, n, outs, ms); }
int ksh_audit_firstfit_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, ksh_audit_firstfit_out* out, double* ms) { return audit_claimed<AuditFirstFit>(hv, c, pod_seq, out, ms); }
int ksh_audit_limits(void** hv, uint32_t n, ksh_audit_limits_out* outs, double* ms) { return audit_resident<AuditLimits>(hv, n, outs, ms); }
int ksh_audit_limits_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, ksh_audit_limits_out* out, double* ms) { return audit_claimed<AuditLimits>(hv, c, pod_seq, out, ms); }
int ksh_audit_hostfit(void** hv, uint32_t n, ksh_audit_hostfit_out* outs, double* ms) { return audit_resident<AuditHostFit>(hv, n, outs, ms); }
int ksh_audit_hostfit_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, ksh_audit_hostfit_out* out, double* ms) { return audit_claimed<AuditHostFit>(hv, c, pod_seq, out, ms); }
int ksh_audit_zonefit(void** hv, uint32_t n, ksh_audit_zonefit_out* outs, double* ms) { return audit_resident<AuditZoneFit>(hv, n, outs, ms); }
int ksh_audit_zonefit_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, ksh_audit_zonefit_out* out, double* ms) { return audit_claimed<AuditZoneFit>(hv, c, pod_seq, out, ms); }
int ksh_audit_stages(void** hv, uint32_t n, ksh_audit_stages_out* outs, double* ms) { return audit_resident<AuditStages>(hv, n, outs, ms); }
int ksh_audit_stages_claimed(void* hv, const ksh_result_arrays* c, const int32_t* pod_seq, ksh_audit_stages_out* out, double* ms) { return audit_claimed<AuditStages>(hv, c, pod_seq, out, ms); }
int ksh_audit_reasons(void** hv, uint32_t n, ksh_audit_reasons_out* outs, double* ms) { return audit_resident<AuditReasons>(hv, n, outs, ms); }
int ksh_audit_reasons_claimed(void* hv, const ksh_result_arrays* c, ksh_audit_reasons_out* out, double* ms) { return audit_claimed<AuditReasons>(hv, c, nullptr, out, ms); }
}  // extern "C"
// What getNodePrices / filterOutSameType / simulateScheduling's readiness rule read of the snapshot's nodes, once per call
namespace {
struct CmdNode { int32_t type = -1; bool spot = false, has_price = false, unready = false, owned = false; double price = 0.0; };
struct CmdSnapshot {
  std::vector<CmdNode> nodes; uint32_t unready = 0;
  explicit CmdSnapshot(const ksp::Problem& pr) : nodes(pr.nodes.size()) {
    std::unordered_map<std::string, int32_t> tindex; for (size_t t = 0; t < pr.instance_types.size(); ++t) tindex.emplace(pr.instance_types[t].name, (int32_t)t);
    for (size_t i = 0; i < pr.nodes.size(); ++i) {
      const ksp::StateNode& nd = pr.nodes[i]; CmdNode& c = nodes[i];
      auto lab = [&](const char* k) -> const std::string& { static const std::string none; auto it = nd.labels.find(k); return it == nd.labels.end() ? none : it->second; };
      c.owned = nd.owned();
      auto init = nd.labels.find("karpenter.sh/initialized");
      c.unready = nd.in_state && c.owned && !(init != nd.labels.end() && init->second == "true");      // helpers.go:102-111
      unready += c.unready ? 1u : 0u;
      auto t = tindex.find(lab(ksp::kInstanceType)); if (t == tindex.end()) continue;
      c.type = t->second; const std::string& ct = lab(ksp::kCapacityType); const std::string& zone = lab(ksp::kZone); c.spot = ct == "spot";
      for (auto& o : pr.instance_types[c.type].offerings) if (o.capacity_type == ct && o.zone == zone) { c.has_price = true; c.price = o.price; break; }      // Offerings.Get (types.go:117-124): availability is not consulted
    }
  }
};
// What the command call and the validation call share: the whole-call refusals, the label table, the nodes that leave EVERY what-if, per what-if its own node list and
// readiness, and the route -- open (derived on the device, else flattened one by one), solve resident.  The handles are closed with the object.
std::atomic<uint64_t> g_whatifs_simulated{0};      // ksh_whatifs_simulated: what-ifs SimBatch has opened and solved in this process
struct SimBatch {
  Parsed* P = nullptr; std::shared_ptr<const void> held; const CmdSnapshot* cs = nullptr;
  std::vector<uint8_t> is_del, seen; std::vector<uint32_t> first, last, off2{0}, cand2; uint32_t del_unready = 0; std::vector<void*> hs;
  ~SimBatch() { close(); }
  void close() { for (void*& h : hs) if (h) { ksh_close(h); h = nullptr; } }
  // KS_ERR_INVALID for an unknown flag bit, a row too short, offsets that do not ascend, a node out of range; then the label table and the deleting nodes.  `call` / `row` word the messages
  int begin(Parsed* P_, const char* call, const char* row, uint32_t flags, uint32_t n, const uint32_t* off, const uint32_t* nodes, const uint32_t* deleting, uint32_t n_deleting, uint32_t words) {
    P = P_;
    const uint32_t known = KS_FLAG_SIMULATION | KS_FLAG_NO_RR | KS_FLAG_ONE_WAVE | KS_FLAG_NO_LEAN | KSH_DERIVE_VOLUMES | KSH_ACTIVE_RESOURCES | KSH_DERIVE_GROUP_LISTS;
    if (flags & ~known) return set_err(KS_ERR_INVALID, std::string(call) + ": unknown flag bit");
    if (!n) return KS_OK;
    const ksp::Problem& pr = *P->pr; const size_t NN = pr.nodes.size(); const uint32_t TW = ((uint32_t)pr.instance_types.size() + 63) / 64;
    if (words < TW) return set_err(KS_ERR_INVALID, std::string(row) + " row too short: " + std::to_string(words) + " words for " + std::to_string(pr.instance_types.size()) + " instance types");
    for (uint32_t i = 0; i < n; ++i) if (off[i + 1] < off[i]) return set_err(KS_ERR_INVALID, "candidate offsets not ascending");
    if (off[n] && !nodes) return set_err(KS_ERR_INVALID, "null argument");
    for (uint32_t i = 0; i < off[n]; ++i) if (nodes[i] >= NN) return set_err(KS_ERR_INVALID, "candidate node out of range");
    for (uint32_t i = 0; i < n_deleting; ++i) if (deleting[i] >= NN) return set_err(KS_ERR_INVALID, "deleting node out of range");
    // the label table: made by the first command call over this snapshot, kept until events change the nodes
    { std::lock_guard<std::mutex> g(P->mu); if (!P->cmd_nodes) P->cmd_nodes = std::make_shared<const CmdSnapshot>(pr); held = P->cmd_nodes; }
    cs = static_cast<const CmdSnapshot*>(held.get());
    // nodes that leave EVERY what-if: the carrier of the pending pods (a node no provisioner owns) first -- the pending pods head simulateScheduling's batch,
    // helpers.go:76-79 --, the nodes marked for deletion last (:81-84); a candidate that is itself being deleted is an error, not a simulation (:62-67)
    is_del.assign(NN, 0); seen.assign(NN, 0);
    for (uint32_t i = 0; i < n_deleting; ++i) { if (is_del[deleting[i]]) continue; is_del[deleting[i]] = 1; (cs->nodes[deleting[i]].owned ? last : first).push_back(deleting[i]); del_unready += cs->nodes[deleting[i]].unready ? 1u : 0u; }
    return KS_OK;
  }
  bool names_deleting(const uint32_t* nodes, uint32_t count) const { for (uint32_t k = 0; k < count; ++k) if (is_del[nodes[k]]) return true; return false; }
  // one more what-if: these nodes leave (a node listed twice leaves once; `distinct` sees each once, in order).  True when an owned, in-state node that is not
  // initialised STAYS: simulateScheduling then reports "not all pods scheduled" (helpers.go:102-113)
  template <class F> bool add(const uint32_t* nodes, uint32_t count, F&& distinct) {
    cand2.insert(cand2.end(), first.begin(), first.end());
    uint32_t gone_unready = del_unready;
    for (uint32_t k = 0; k < count; ++k) {
      const uint32_t nd = nodes[k]; cand2.push_back(nd);
      if (seen[nd]) continue;
      seen[nd] = 1; gone_unready += cs->nodes[nd].unready ? 1u : 0u; distinct(cs->nodes[nd]);
    }
    for (uint32_t k = 0; k < count; ++k) seen[nodes[k]] = 0;
    cand2.insert(cand2.end(), last.begin(), last.end());
    off2.push_back((uint32_t)cand2.size());
    return cs->unready > gone_unready;
  }
  uint32_t size() const { return (uint32_t)off2.size() - 1; }
  // ms[0] open, ms[1] solve.  `rows_name_it_states`: the rows to come carry instance-type requirement states, read through the snapshot's lattice
  int open_and_solve(uint32_t flags, const int32_t* pod_node, int device, bool rows_name_it_states, double* ms) {
    const uint32_t m = size(); hs.assign(m, nullptr);
    if (cand2.empty()) cand2.push_back(0);
    auto t0 = clk::now();
    int rc = ksh_open_whatifs_derived(P, flags, m, off2.data(), cand2.data(), pod_node, device, hs.data());
    if (rc == KS_ERR_UNSUPPORTED) {      // what scheduler.open_whatifs(derive=None) does: flatten the what-ifs one by one, then make them resident
      rc = ksh_open_whatifs_parsed(P, flags & ~(uint32_t)(KSH_DERIVE_VOLUMES | KSH_DERIVE_GROUP_LISTS), m, off2.data(), cand2.data(), pod_node, 0, hs.data());
      // KS_CMD_IT_STATE is spelled out through the snapshot's lattice (ksh_snapshot_it_state): a what-if flattened by itself that needed instance-type states of
      // its own cannot be read that way -- refused here, before anything is uploaded or launched
      for (uint32_t k = 0; rows_name_it_states && k < m && rc == KS_OK; ++k) { const ksh::Encoded& e = *((Handle*)hs[k])->enc; if (!(e.shared && e.shared_lattice)) rc = set_err(KS_ERR_UNSUPPORTED, "a what-if carries instance-type requirement states of its own: simulate it through ksh_open_whatifs_parsed and read it through ksh_result_text"); }
      if (rc == KS_OK) rc = ksh_upload_batch(hs.data(), m, device, 0);
    }
    if (rc != KS_OK) { close(); return rc; }
    if (ms) ms[0] = ms_since(t0);
    t0 = clk::now();
    rc = ksh_solve_batch_resident(hs.data(), m, nullptr, nullptr);
    if (rc != KS_OK) { close(); return rc; }
    if (ms) ms[1] = ms_since(t0);
    g_whatifs_simulated += m;
    return KS_OK;
  }
};
// all the what-ifs of one call: open, solve resident, decide on the device, rows back.  ms[5]: open | solve | command kernel | read-back | the host work around them
int commands_over(Parsed* P, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                  int device, bool same_type, const uint64_t* ids, uint64_t* out_rows, uint32_t words, double* ms) {
  zero(ms, 5);
  if (!P || (n && (!cand_off || !out_rows)) || (n_deleting && !deleting)) return set_err(KS_ERR_INVALID, "null argument");
  SimBatch B; int rc = B.begin(P, "consolidation commands", "command", flags, n, cand_off, cand, deleting, n_deleting, words);
  if (rc != KS_OK || !n) return rc;
  const ksp::Problem& pr = *P->pr;
  const auto t_call = clk::now();
  const size_t W = KS_CMD_ROW_WORDS(words);
  std::vector<uint32_t> live; std::vector<uint32_t> cflags; std::vector<double> cprice, tprice; std::vector<uint32_t> toff{0}, tidx; std::vector<uint64_t> lids;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* mine = cand + cand_off[i]; const uint32_t count = cand_off[i + 1] - cand_off[i];
    uint64_t* row = out_rows + (size_t)i * W;
    if (B.names_deleting(mine, count)) { std::fill(row, row + W, 0ull); row[KS_CMD_ID] = ids ? ids[i] : i; row[KS_CMD_DECISION] = (uint64_t)KS_CMD_ERROR | ((uint64_t)KS_CMD_WHY_DELETING << 8); continue; }
    for (uint32_t k = 0; k < count; ++k) if (B.cs->nodes[mine[k]].type < 0) return set_err(KS_ERR_INVALID, "candidate node " + pr.nodes[mine[k]].name + " carries no instance type of the snapshot's catalogue");
    live.push_back(i); lids.push_back(ids ? ids[i] : i);
    uint32_t f = same_type ? KS_CMD_F_SAME_TYPE : 0u; bool all_spot = true; double price = 0.0; const size_t t0 = tidx.size();
    const bool blocked = B.add(mine, count, [&](const CmdNode& c) {
      all_spot = all_spot && c.spot;
      if (c.has_price) price += c.price; else f |= KS_CMD_F_PRICE_ERROR;      // getNodePrices, consolidation.go:277-287: summed in candidate order
      size_t at = t0; while (at < tidx.size() && tidx[at] != (uint32_t)c.type) ++at;
      if (at == tidx.size()) { tidx.push_back((uint32_t)c.type); tprice.push_back(c.has_price ? c.price : -1.0); }      // (-1: no candidate of the type has an offering yet)
      else if (c.has_price && (tprice[at] < 0.0 || c.price < tprice[at])) tprice[at] = c.price;
    });
    for (size_t at = t0; at < tprice.size(); ++at) if (tprice[at] < 0.0) tprice[at] = 0.0;      // the Go map miss of multinodeconsolidation.go:150-158
    if (all_spot) f |= KS_CMD_F_ALL_SPOT;
    if (blocked) f |= KS_CMD_F_BLOCKED;
    cflags.push_back(f); cprice.push_back(price); toff.push_back((uint32_t)tidx.size());
  }
  const uint32_t m = (uint32_t)live.size(); if (!m) return KS_OK;
  rc = B.open_and_solve(flags, pod_node, device, true, ms);
  if (rc != KS_OK) return rc;
  ks_command_inputs in{}; in.flags = cflags.data(); in.cand_price = cprice.data(); in.type_off = toff.data(); in.type_idx = tidx.data(); in.type_price = tprice.data();
  std::vector<uint64_t> rows; uint64_t* dst = out_rows;
  if (m != n) { rows.resize((size_t)m * W); dst = rows.data(); }      // (refused candidate sets keep their rows: the live ones are scattered around them)
  rc = ksh_command_rows(B.hs.data(), m, lids.data(), &in, words, dst, ms ? ms + 2 : nullptr);
  B.close();
  if (rc != KS_OK) return rc;
  if (m != n) for (uint32_t k = 0; k < m; ++k) std::copy(rows.begin() + (size_t)k * W, rows.begin() + (size_t)(k + 1) * W, out_rows + (size_t)live[k] * W);
  if (ms) ms[4] = ms_since(t_call) - ms[0] - ms[1] - ms[2] - ms[3];      // the host work around the four: the per-what-if inputs, closing the handles
  return KS_OK;
}
// Expiration / Drift.ComputeCommand for n candidate sets: open, solve resident, both tables written on the device, read back.  A set that names a deleting node gets an
// error head here and is not simulated; its node_off is the next simulated set's, so the offsets stay ascending.  ms[5] as commands_over.
int replacement_over(Parsed* P, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                     int device, uint64_t* out_heads, uint64_t* out_nodes, uint64_t cap_nodes, uint64_t* out_total, uint32_t words, double* ms) {
  zero(ms, 5);
  if (!P || !out_total || (n && (!cand_off || !out_heads)) || (n_deleting && !deleting) || (cap_nodes && !out_nodes)) return set_err(KS_ERR_INVALID, "null argument");
  SimBatch B; int rc = B.begin(P, "replacement commands", "replacement", flags, n, cand_off, cand, deleting, n_deleting, words);
  if (rc != KS_OK) return rc;
  *out_total = 0;
  if (!n) return KS_OK;
  const auto t_call = clk::now();
  std::vector<uint32_t> live, rflags; std::vector<uint64_t> lids;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* mine = cand + cand_off[i]; const uint32_t count = cand_off[i + 1] - cand_off[i];
    if (B.names_deleting(mine, count)) continue;
    live.push_back(i); lids.push_back(i);
    rflags.push_back(B.add(mine, count, [](const CmdNode&) {}) ? KS_REP_F_BLOCKED : 0u);
  }
  const uint32_t m = (uint32_t)live.size();
  std::vector<uint64_t> heads((size_t)m * KS_REP_HEAD_WORDS);
  if (m) {
    rc = B.open_and_solve(flags, pod_node, device, true, ms);
    if (rc != KS_OK) return rc;
    rc = ksh_replacement_rows(B.hs.data(), m, lids.data(), rflags.data(), words, heads.data(), out_nodes, cap_nodes, out_total, ms ? ms + 2 : nullptr);
    B.close();
    if (rc != KS_OK) return rc;
  }
  uint64_t next_off = *out_total;      // (walking backwards: an error head points at the next simulated set's first row)
  for (uint32_t i = n, k = m; i-- > 0;) {
    uint64_t* h = out_heads + (size_t)i * KS_REP_HEAD_WORDS;
    if (k && live[k - 1] == i) { --k; std::copy(heads.begin() + (size_t)k * KS_REP_HEAD_WORDS, heads.begin() + (size_t)(k + 1) * KS_REP_HEAD_WORDS, h); next_off = h[KS_REP_NODE_OFF]; continue; }
    std::fill(h, h + KS_REP_HEAD_WORDS, 0ull);
    h[KS_REP_ID] = i; h[KS_REP_DECISION] = (uint64_t)KS_CMD_ERROR | ((uint64_t)KS_CMD_WHY_DELETING << 8); h[KS_REP_NODE_OFF] = next_off;
  }
  if (ms) ms[4] = ms_since(t_call) - ms[0] - ms[1] - ms[2] - ms[3];
  return KS_OK;
}
// Provisioner.Reconcile's Solve (provisioning/provisioner.go:117-150) over the snapshot: ONE what-if with no candidate -- the carrier of the pending pods and the nodes
// marked for deletion leave, their pods are the batch --, on SimBatch's route, then three tables off the result on the device: placement rows, machine rows
// (ks_replacement_nodes' rows, every new node), the launch pick per machine.  ms[5] as commands_over: [2] the kernels of all three, [3] their read-backs.
int provision_over(Parsed* P, uint32_t flags, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, int device, ksh_provision_out* out, double* ms) {
  zero(ms, 5);
  if (!P || !out || (n_deleting && !deleting) || (out->cap_rows && !out->rows) || (out->cap_machines && !out->machines)) return set_err(KS_ERR_INVALID, "null argument");
  const bool picks = out->pick_type || out->pick_zone || out->pick_ct || out->pick_price;
  if (picks && !(out->pick_type && out->pick_zone && out->pick_ct && out->pick_price)) return set_err(KS_ERR_INVALID, "null argument");
  out->route = KSH_PROVISION_NOTHING; out->total_rows = out->total_machines = 0; std::fill(out->head, out->head + KS_PLC_HEAD_WORDS, 0ull);
  const uint32_t words = out->words, none[2] = {0, 0};
  SimBatch B; int rc = B.begin(P, "provision", "machine", flags, 1, none, nullptr, deleting, n_deleting, words);
  if (rc != KS_OK) return rc;
  const auto t_call = clk::now();
  // nothing pending, nothing on a node that is going: Reconcile returns before NewScheduler (provisioner.go:145-147) -- no flattening, no launch
  const int32_t* bound = bindings_of(P, pod_node); const size_t np = P->pr->pods.size(), NN = P->pr->nodes.size(); size_t batch = 0;
  if (!bound && np) return set_err(KS_ERR_INVALID, "no bindings (pod_node)");
  for (size_t p = 0; p < np; ++p) { if (bound[p] < 0) continue; if ((size_t)bound[p] >= NN) return set_err(KS_ERR_INVALID, "pod_node out of range"); batch += B.is_del[bound[p]]; }
  if (!batch) return KS_OK;
  B.add(nullptr, 0, [](const CmdNode&) {});      // (its answer -- an uninitialised node stays -- is not read: Reconcile has no check like helpers.go:102-113, such a node is an in-flight ExistingNode)
  rc = B.open_and_solve(flags, pod_node, device, true, ms);
  if (rc != KS_OK) return rc;
  out->route = ((Handle*)B.hs[0])->delta ? KSH_PROVISION_DERIVED : KSH_PROVISION_FLATTENED;
  const uint64_t id = 0; const uint32_t no_flags = 0; double part[2] = {0.0, 0.0};
  rc = ksh_placement_rows(B.hs.data(), 1, &id, out->head, out->rows, out->cap_rows, &out->total_rows, part);
  if (rc != KS_OK) return rc;
  if (ms) { ms[2] += part[0]; ms[3] += part[1]; }
  uint64_t rep_head[KS_REP_HEAD_WORDS];
  rc = ksh_replacement_rows(B.hs.data(), 1, &id, &no_flags, words, rep_head, out->machines, out->cap_machines, &out->total_machines, part);
  if (rc != KS_OK) return rc;
  if (ms) { ms[2] += part[0]; ms[3] += part[1]; }
  if ((rep_head[KS_REP_DECISION] >> 16) & KS_REP_TRUNCATED) out->head[KS_PLC_FLAGS] |= KSH_PROVISION_MACHINES_TRUNCATED;
  else if (picks && out->total_machines) {
    const auto t0 = clk::now(); const uint32_t nm = (uint32_t)out->total_machines;
    std::vector<void*> same(nm, B.hs[0]); std::vector<uint32_t> node(nm); for (uint32_t j = 0; j < nm; ++j) node[j] = j;
    rc = ksh_launch_pick(same.data(), nm, node.data(), out->pick_type, out->pick_zone, out->pick_ct, out->pick_price);
    if (rc != KS_OK) return rc;
    if (ms) ms[2] += ms_since(t0);
  }
  B.close();
  if (ms) ms[4] = ms_since(t_call) - ms[0] - ms[1] - ms[2] - ms[3];
  return KS_OK;
}
// mapNodes (helpers.go:328-337) by reason code: a node of a command is still a candidate iff candidateNodes yields it under consolidation.ShouldDeprovision -- reasons
// 0 and 10-12 (sortAndFilterCandidates is not applied in validation)
inline bool still_candidate(uint32_t why) { return why == 0 || (why >= KS_CAND_WHY_DELETING_NODE && why <= KS_CAND_WHY_DO_NOT_EVICT); }
// Validation.IsValid after the wait (validation.go:84-96) and ValidateCommand (:109-172) for n commands: nomination, mapping and the deleting error on the host; the
// mapped subsets re-simulated in ONE batch and judged on the device.  ms[5] as commands_over.
int validate_over(Parsed* P, uint32_t flags, uint32_t n, const uint32_t* node_off, const uint32_t* nodes, const uint32_t* expect, const uint64_t* options, const uint32_t* why,
                  const uint32_t* node_flags, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, int device, const uint64_t* ids, uint64_t* out_rows, uint32_t words, double* ms) {
  zero(ms, 5);
  if (!P || (n && (!node_off || !out_rows || !expect)) || (n_deleting && !deleting)) return set_err(KS_ERR_INVALID, "null argument");
  SimBatch B; int rc = B.begin(P, "validate commands", "validation", flags, n, node_off, nodes, deleting, n_deleting, words);
  if (rc != KS_OK || !n) return rc;
  if (node_off[n] && (!why || !node_flags)) return set_err(KS_ERR_INVALID, "null argument");
  const uint32_t T = (uint32_t)P->pr->instance_types.size();
  for (uint32_t i = 0; i < n; ++i) if (expect[i]) {
    if (!options) return set_err(KS_ERR_INVALID, "null argument");
    const uint64_t* o = options + (size_t)i * words;      // option bits are indices into THIS snapshot's catalogue
    for (uint32_t w = T / 64; w < words; ++w) if (w * 64 >= T ? o[w] != 0 : (o[w] >> (T % 64)) != 0) return set_err(KS_ERR_INVALID, "command " + std::to_string(i) + ": type index out of range");
  }
  const auto t_call = clk::now();
  const size_t W = KS_VAL_ROW_WORDS(words);
  struct HostRow { uint32_t i, verdict, why, n_mapped; };
  std::vector<HostRow> decided; std::vector<uint32_t> live, vflags, nmapped, mapped; std::vector<uint64_t> lids, lopts;
  for (uint32_t i = 0; i < n; ++i) {
    const uint32_t* mine = nodes + node_off[i]; const uint32_t count = node_off[i + 1] - node_off[i];
    bool nominated = false; mapped.clear();
    for (uint32_t k = 0; k < count; ++k) { nominated = nominated || (node_flags[mine[k]] & KSH_CAND_NODE_NOMINATED); if (still_candidate(why[mine[k]])) mapped.push_back(mine[k]); }
    std::sort(mapped.begin(), mapped.end()); mapped.erase(std::unique(mapped.begin(), mapped.end()), mapped.end());      // mapNodes walks the candidates: slot order, each once
    if (nominated) { decided.push_back({i, KS_VAL_INVALID, KS_VAL_WHY_NOMINATED, 0}); continue; }                          // validation.go:87-91, before the mapping
    if (mapped.empty()) { decided.push_back({i, KS_VAL_INVALID, KS_VAL_WHY_NO_CANDIDATES, 0}); continue; }                 // :114
    if (B.names_deleting(mapped.data(), (uint32_t)mapped.size())) { decided.push_back({i, KS_VAL_ERROR, KS_VAL_WHY_DELETING, (uint32_t)mapped.size()}); continue; }      // helpers.go:62-67
    live.push_back(i); lids.push_back(ids ? ids[i] : i); nmapped.push_back((uint32_t)mapped.size());
    const bool blocked = B.add(mapped.data(), (uint32_t)mapped.size(), [](const CmdNode&) {});
    vflags.push_back((blocked ? KS_VAL_F_BLOCKED : 0u) | (expect[i] ? KS_VAL_F_EXPECT_REPLACEMENT : 0u));
    lopts.resize(lopts.size() + words, 0ull);
    if (expect[i]) std::copy(options + (size_t)i * words, options + (size_t)(i + 1) * words, lopts.end() - words);
  }
  const uint32_t m = (uint32_t)live.size();
  std::vector<uint64_t> rows((size_t)m * W);
  if (m) {
    rc = B.open_and_solve(flags, pod_node, device, false, ms);      // (validation reads no requirement state: the fallback route's instance-type-state refusal does not apply)
    if (rc != KS_OK) return rc;
    std::vector<ks_dev_problem*> ds(m); for (uint32_t k = 0; k < m; ++k) ds[k] = ((Handle*)B.hs[k])->dev;
    ks_validate_inputs in{}; in.flags = vflags.data(); in.n_mapped = nmapped.data(); in.options = lopts.data();
    rc = dev_rc(ks_validate_commands_host(ds.data(), m, lids.data(), &in, words, rows.data(), ms ? ms + 2 : nullptr));
    B.close();
    if (rc != KS_OK) return rc;
  }
  // nothing was written so far: a refusal leaves the caller's rows as they were
  for (uint32_t k = 0; k < m; ++k) std::copy(rows.begin() + (size_t)k * W, rows.begin() + (size_t)(k + 1) * W, out_rows + (size_t)live[k] * W);
  for (const HostRow& h : decided) {
    uint64_t* row = out_rows + (size_t)h.i * W; std::fill(row, row + W, 0ull);
    row[KS_VAL_ID] = ids ? ids[h.i] : h.i; row[KS_VAL_VERDICT] = (uint64_t)h.verdict | ((uint64_t)h.why << 8); row[KS_VAL_N_MAPPED] = h.n_mapped;
  }
  if (ms) ms[4] = ms_since(t_call) - ms[0] - ms[1] - ms[2] - ms[3];
  return KS_OK;
}
}  // namespace
extern "C" {
int ksh_consolidation_commands(void* parsed, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                               int device, int same_type, uint64_t* out_rows, uint32_t words, double* ms) {
  return guarded([&] { return commands_over((Parsed*)parsed, flags, n, cand_off, cand, pod_node, deleting, n_deleting, device, same_type != 0, nullptr, out_rows, words, ms); });
}
// firstNNodeConsolidationOption (multinodeconsolidation.go:74-114): every prefix the binary search could probe in one batch, filterOutSameType included, then the search
// replayed over the rows.  out_row[KS_CMD_ID] = how many leading candidates the command removes.
int ksh_first_n_node_option(void* parsed, uint32_t flags, const uint32_t* candidates, uint32_t n, uint32_t max_nodes, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                            int device, uint64_t* out_row, uint32_t words, double* ms) {
  if (!out_row || (n && !candidates)) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    const size_t W = KS_CMD_ROW_WORDS(words); std::fill(out_row, out_row + W, 0ull);
    zero(ms, 5);
    if (n < 2) return KS_OK;                                   // :75-77
    uint32_t lo = 1, hi = max_nodes; if (n <= hi) hi = n - 1;      // :78-84
    if (hi < lo) return KS_OK;
    const uint32_t np = hi - lo + 1;
    std::vector<uint32_t> off(np + 1, 0), cand; std::vector<uint64_t> ids(np);
    for (uint32_t mid = lo; mid <= hi; ++mid) { cand.insert(cand.end(), candidates, candidates + mid + 1); off[mid - lo + 1] = (uint32_t)cand.size(); ids[mid - lo] = mid + 1; }
    std::vector<uint64_t> rows((size_t)np * W);
    int rc = commands_over((Parsed*)parsed, flags, np, off.data(), cand.data(), pod_node, deleting, n_deleting, device, true, ids.data(), rows.data(), words, ms);
    if (rc != KS_OK) return rc;
    int64_t l = lo, h = hi;
    while (l <= h) {
      const int64_t mid = (l + h) / 2; const uint64_t* row = rows.data() + (size_t)(mid - lo) * W; const uint32_t action = (uint32_t)(row[KS_CMD_DECISION] & 0xffu);
      if (action == KS_CMD_ERROR) { std::copy(row, row + W, out_row); return KS_OK; }      // the probed prefix's error is the search's (:92-95)
      if (action == KS_CMD_REPLACE || action == KS_CMD_DELETE) { std::copy(row, row + W, out_row); l = mid + 1; } else h = mid - 1;
    }
    return KS_OK;
  });
}
// SingleNodeConsolidation.ComputeCommand's scan (singlenodeconsolidation.go:54-78): every singleton in one batch; the first delete or replace in candidate order, errors
// passed over.  out_row[KS_CMD_ID] = the position of that candidate.
int ksh_single_node_option(void* parsed, uint32_t flags, const uint32_t* candidates, uint32_t n, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                           int device, uint64_t* out_row, uint32_t words, double* ms) {
  if (!out_row || (n && !candidates)) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    const size_t W = KS_CMD_ROW_WORDS(words); std::fill(out_row, out_row + W, 0ull);
    zero(ms, 5);
    if (!n) return KS_OK;
    std::vector<uint32_t> off(n + 1); for (uint32_t i = 0; i <= n; ++i) off[i] = i;
    std::vector<uint64_t> rows((size_t)n * W);
    int rc = commands_over((Parsed*)parsed, flags, n, off.data(), candidates, pod_node, deleting, n_deleting, device, false, nullptr, rows.data(), words, ms);
    if (rc != KS_OK) return rc;
    for (uint32_t i = 0; i < n; ++i) {
      const uint64_t* row = rows.data() + (size_t)i * W; const uint32_t action = (uint32_t)(row[KS_CMD_DECISION] & 0xffu);
      if (action == KS_CMD_REPLACE || action == KS_CMD_DELETE) { std::copy(row, row + W, out_row); return KS_OK; }
    }
    return KS_OK;
  });
}
uint64_t ksh_whatifs_simulated(void) { return g_whatifs_simulated.load(); }
// ---- replacement commands (kshost.h): Expiration / Drift.ComputeCommand's simulation and m -> n command ----
int ksh_replacement_commands(void* parsed, uint32_t flags, uint32_t n, const uint32_t* cand_off, const uint32_t* cand, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                             int device, uint64_t* out_heads, uint64_t* out_nodes, uint64_t cap_nodes, uint64_t* out_total_nodes, uint32_t words, double* ms) {
  return guarded([&] { return replacement_over((Parsed*)parsed, flags, n, cand_off, cand, pod_node, deleting, n_deleting, device, out_heads, out_nodes, cap_nodes, out_total_nodes, words, ms); });
}
// ComputeCommand's loop (expiration.go:75-111, drift.go:64-96): the first candidate canBeTerminated lets through (why == 0) that is not deleting decides, and only it is
// simulated -- which one that is is known before any simulation.
int ksh_replacement_option(void* parsed, uint32_t flags, const uint32_t* candidates, uint32_t n, const uint32_t* why, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting,
                           int device, uint64_t* out_head, uint64_t* out_nodes, uint64_t cap_nodes, uint64_t* out_total_nodes, int32_t* out_position, uint32_t words, double* ms) {
  if (!parsed || !out_head || !out_total_nodes || !out_position || (n && (!candidates || !why)) || (n_deleting && !deleting)) return set_err(KS_ERR_INVALID, "null argument");
  zero(ms, 5);
  const size_t NN = ((Parsed*)parsed)->pr->nodes.size();
  for (uint32_t i = 0; i < n; ++i) if (candidates[i] >= NN) return set_err(KS_ERR_INVALID, "candidate node out of range");
  for (uint32_t i = 0; i < n_deleting; ++i) if (deleting[i] >= NN) return set_err(KS_ERR_INVALID, "deleting node out of range");
  std::fill(out_head, out_head + KS_REP_HEAD_WORDS, 0ull); *out_total_nodes = 0; *out_position = -1;
  for (uint32_t i = 0; i < n; ++i) {
    if (why[candidates[i]] != 0) continue;                                                             // canBeTerminated said no: `continue`
    if (std::find(deleting, deleting + n_deleting, candidates[i]) != deleting + n_deleting) continue;  // errCandidateNodeDeleting: "just retry" with the next one
    const uint32_t off[2] = {0, 1};
    int rc = ksh_replacement_commands(parsed, flags, 1, off, candidates + i, pod_node, deleting, n_deleting, device, out_head, out_nodes, cap_nodes, out_total_nodes, words, ms);
    if (rc != KS_OK) return rc;
    out_head[KS_REP_ID] = i; *out_position = (int32_t)i;
    return KS_OK;
  }
  return KS_OK;
}
// ---- provisioning (kshost.h): Provisioner.Reconcile's Solve over the snapshot kept by events ----
int ksh_provision(void* parsed, uint32_t flags, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, int device, ksh_provision_out* out, double* ms) {
  return guarded([&] { return provision_over((Parsed*)parsed, flags, pod_node, deleting, n_deleting, device, out, ms); });
}
// ---- validation (kshost.h): Validation.IsValid / ValidateCommand over the snapshot as it is NOW, and the two loops built on it ----
int ksh_validate_commands(void* parsed, uint32_t flags, uint32_t n, const uint32_t* node_off, const uint32_t* nodes, const uint32_t* expect_replacement, const uint64_t* options,
                          const uint32_t* why, const uint32_t* node_flags, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, int device,
                          uint64_t* out_rows, uint32_t words, double* ms) {
  return guarded([&] { return validate_over((Parsed*)parsed, flags, n, node_off, nodes, expect_replacement, options, why, node_flags, pod_node, deleting, n_deleting, device, nullptr, out_rows, words, ms); });
}
// SingleNodeConsolidation.ComputeCommand's loop (singlenodeconsolidation.go:54-84) from the candidate AFTER the one whose validation failed: the remaining singletons in
// one command batch, the deletes and replaces among them in one validation batch, the first valid one in candidate order.
int ksh_single_node_resume(void* parsed, uint32_t flags, const uint32_t* candidates, uint32_t n, int failed_before, const uint32_t* why, const uint32_t* node_flags, const int32_t* pod_node,
                           const uint32_t* deleting, uint32_t n_deleting, int device, uint64_t* out_row, uint64_t* out_vrow, uint32_t* out_state, uint32_t words, double* ms) {
  if (!out_row || !out_vrow || !out_state || (n && !candidates)) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    const size_t W = KS_CMD_ROW_WORDS(words), VW = KS_VAL_ROW_WORDS(words);
    zero(ms, 5);
    std::vector<uint64_t> rows((size_t)n * W), vrows; std::vector<uint32_t> off(n + 1); for (uint32_t i = 0; i <= n; ++i) off[i] = i;
    double ms1[5] = {0, 0, 0, 0, 0}, ms2[5] = {0, 0, 0, 0, 0};
    int rc = commands_over((Parsed*)parsed, flags, n, off.data(), candidates, pod_node, deleting, n_deleting, device, false, nullptr, rows.data(), words, ms1);
    if (rc != KS_OK) return rc;
    // the commands the loop would validate (:62-64 passes do-nothing over, :57-60 an error), each a command over its one node
    std::vector<uint32_t> pos, voff{0}, vnodes, expect; std::vector<uint64_t> vopts, vids;
    for (uint32_t i = 0; i < n; ++i) {
      const uint64_t* row = rows.data() + (size_t)i * W; const uint32_t action = (uint32_t)(row[KS_CMD_DECISION] & 0xffu);
      if (action != KS_CMD_REPLACE && action != KS_CMD_DELETE) continue;
      pos.push_back(i); vids.push_back(i); vnodes.push_back(candidates[i]); voff.push_back((uint32_t)vnodes.size()); expect.push_back(action == KS_CMD_REPLACE ? 1u : 0u);
      vopts.insert(vopts.end(), row + KS_CMD_OPTIONS, row + KS_CMD_OPTIONS + words);
    }
    const uint32_t m = (uint32_t)pos.size(); vrows.resize((size_t)m * VW);
    if (m) {
      rc = validate_over((Parsed*)parsed, flags, m, voff.data(), vnodes.data(), expect.data(), vopts.data(), why, node_flags, pod_node, deleting, n_deleting, device, vids.data(), vrows.data(), words, ms2);
      if (rc != KS_OK) return rc;
    }
    if (ms) for (int k = 0; k < 5; ++k) ms[k] = ms1[k] + ms2[k];
    std::fill(out_row, out_row + W, 0ull); std::fill(out_vrow, out_vrow + VW, 0ull);
    bool failed = failed_before != 0;
    for (uint32_t k = 0; k < m; ++k) {
      const uint64_t* vrow = vrows.data() + (size_t)k * VW; const uint32_t verdict = (uint32_t)(vrow[KS_VAL_VERDICT] & 0xffu);
      if (verdict == KS_VAL_ERROR) continue;                       // "validating consolidation": logged, next candidate (:67-70)
      if (verdict == KS_VAL_INVALID) { failed = true; continue; }  // :71-74
      std::copy(rows.begin() + (size_t)pos[k] * W, rows.begin() + (size_t)(pos[k] + 1) * W, out_row); std::copy(vrow, vrow + VW, out_vrow);
      *out_state = 1; return KS_OK;                                // :76-78
    }
    *out_state = failed ? 2u : 0u;                                 // :82-85
    return KS_OK;
  });
}
// EmptyNodeConsolidation's own check (emptynodeconsolidation.go:77-87), literally: map the nodes; retry iff a mapped node has pods and is not nominated.
int ksh_validate_empty_nodes(const uint32_t* nodes, uint32_t n, const uint32_t* why, const uint32_t* n_node_pods, const uint32_t* node_flags, uint32_t* out_retry) {
  if (!out_retry || (n && (!nodes || !why || !n_node_pods || !node_flags))) return set_err(KS_ERR_INVALID, "null argument");
  *out_retry = 0;
  for (uint32_t i = 0; i < n; ++i) if (still_candidate(why[nodes[i]]) && n_node_pods[nodes[i]] != 0 && !(node_flags[nodes[i]] & KSH_CAND_NODE_NOMINATED)) *out_retry = 1;
  return KS_OK;
}
// ---- consolidation candidates (kshost.h): candidateNodes + ShouldDeprovision + sortAndFilterCandidates over a snapshot ----
}  // extern "C"
namespace {
// What candidateNodes reads of the nodes' labels, once per snapshot: the reason a node is skipped for (2-6, 13; 0: none) and its provisioner
struct CandSnapshot {
  std::vector<uint8_t> why; std::vector<int32_t> prov;
  explicit CandSnapshot(const ksp::Problem& pr) : why(pr.nodes.size(), 0), prov(pr.nodes.size(), -1) {
    std::unordered_map<std::string, int32_t> pindex; for (size_t m = 0; m < pr.provisioners.size(); ++m) pindex.emplace(pr.provisioners[m].name, (int32_t)m);
    std::vector<std::unordered_map<std::string, int32_t>> types(pr.provisioners.size());      // buildProvisionerMap: provName -> instanceName -> instance type
    for (size_t m = 0; m < pr.provisioners.size(); ++m) for (int32_t t : pr.provisioners[m].instance_types) types[m].emplace(pr.instance_types[t].name, t);
    for (size_t i = 0; i < pr.nodes.size(); ++i) {
      const ksp::StateNode& nd = pr.nodes[i];
      auto lab = [&](const char* k) -> const std::string* { auto it = nd.labels.find(k); return it == nd.labels.end() ? nullptr : &it->second; };
      static const std::string none;
      if (!nd.in_state) { why[i] = KS_CAND_WHY_LEFT; continue; }
      const std::string* pn = lab(ksp::kProvisionerName); auto pm = pn ? pindex.find(*pn) : pindex.end();
      if (pm == pindex.end()) { why[i] = 2; continue; }                                         // helpers.go:181-192
      prov[i] = pm->second;
      const std::string* it = lab(ksp::kInstanceType);
      if (!types[pm->second].count(it ? *it : none)) { why[i] = 3; continue; }                  // :194-198
      if (!lab(ksp::kCapacityType)) { why[i] = 4; continue; }                                   // :201
      if (!lab(ksp::kZone)) { why[i] = 5; continue; }                                           // :205
      const std::string* init = lab("karpenter.sh/initialized");
      if (!(init && *init == "true")) { why[i] = 6; continue; }                                 // :211, state/node.go:80-82
    }
  }
};
// `dx` = NULL: consolidation (`in`, codes 8 / 9).  Else `in` == &dx->base and `method`'s ShouldDeprovision takes the place of 8 / 9: the host gives reasons 1-7 and 13 and
// the flags, the device decides the rest (ks_deprovisioning_candidates_host); *n_in_result = len(candidateNodes(...)).
// `flags`: KSH_CAND_WIDE_SELECTORS tabulates the selectors as lists (ksolve.h ks_selector_lists) instead of bytes and masks; everything that is not a selector is one path.
int candidates_over(Parsed* P, uint32_t method, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, const ksh_candidate_inputs* in, const ksh_deprovisioning_inputs* dx,
                    const ksh_pdb_block* pb, int device, uint32_t flags, ksh_candidates_out* out, uint32_t* n_in_result, double* ms) {
  const auto t_call = clk::now();
  zero(ms, 4);
  if (!P || !in || !out || (n_deleting && !deleting)) return set_err(KS_ERR_INVALID, "null argument");
  const std::string what = dx ? "deprovisioning candidates" : "consolidation candidates";
  if (flags & ~(uint32_t)KSH_CAND_WIDE_SELECTORS) return set_err(KS_ERR_INVALID, what + ": unknown flag bit (KSH_CAND_WIDE_SELECTORS is the only one)");
  const bool wide = (flags & KSH_CAND_WIDE_SELECTORS) != 0;
  if (dx && (method < KSH_METHOD_EXPIRATION || method > KSH_METHOD_EMPTINESS)) return set_err(KS_ERR_INVALID, what + ": unknown method " + std::to_string(method));
  // the PDBs first, completely: a malformed block changes and launches nothing
  std::vector<ksp::Pdb> pdbs;
  if (pb) {
    if (!pb->str_off || (!pb->words && pb->n_words) || (!pb->str_bytes && pb->n_strings)) return set_err(KS_ERR_INVALID, "null argument");
    pdbs = ksp::PdbReader(string_table("pdb", pb->n_strings, pb->str_off, pb->str_bytes, pb->str_bytes_len), pb->words, pb->words + pb->n_words).read_pdbs(pb->n_pdbs);
  }
  std::shared_ptr<const void> held; std::vector<int32_t> bind;
  const ksp::Problem& pr = *P->pr;
  { std::lock_guard<std::mutex> g(P->mu);
    const int32_t* pn = bindings_of(P, pod_node); if (!pn && !pr.pods.empty()) return set_err(KS_ERR_INVALID, "no bindings (pod_node)");
    bind.assign(pn, pn + pr.pods.size());
    if (!P->cand_nodes) P->cand_nodes = std::make_shared<const CandSnapshot>(pr);
    held = P->cand_nodes; }
  const CandSnapshot& cs = *static_cast<const CandSnapshot*>(held.get());
  const uint32_t NN = (uint32_t)pr.nodes.size(), NP = (uint32_t)pr.pods.size(), NM = (uint32_t)pr.provisioners.size();
  if (in->n_nodes != NN || in->n_pods != NP || in->n_provisioners != NM)
    return set_err(KS_ERR_INVALID, what + ": the input arrays are for " + std::to_string(in->n_nodes) + " nodes / " + std::to_string(in->n_pods) + " pods / " + std::to_string(in->n_provisioners) +
                                   " provisioners, the snapshot has " + std::to_string(NN) + " / " + std::to_string(NP) + " / " + std::to_string(NM));
  if ((NN && (!in->node_flags || !in->node_age_seconds || !out->order || !out->empty || !out->why || !out->detail || !out->n_node_pods || !out->cost)) ||
      (NP && (!in->pod_flags || !in->pod_deletion_cost || !in->pod_priority)) || (NM && ((!dx && !in->prov_consolidation_enabled) || !in->prov_ttl_seconds_until_expired)) ||
      (dx && ((NN && (!dx->node_creation_unix_nanos || !dx->node_emptiness_unix_nanos)) || (NM && !dx->prov_ttl_seconds_after_empty)))) return set_err(KS_ERR_INVALID, "null argument");
  for (uint32_t i = 0; i < n_deleting; ++i) if (deleting[i] >= NN) return set_err(KS_ERR_INVALID, "deleting node out of range");
  for (uint32_t p = 0; p < NP; ++p) if (bind[p] >= (int32_t)NN || bind[p] < -1) return set_err(KS_ERR_INVALID, "pod_node out of range");
  for (uint32_t n = 0; n < NN; ++n) {
    const uint32_t f = in->node_flags[n];
    if ((f & KSH_CAND_NODE_EMPTINESS_UNPARSABLE) && !(f & KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP) && dx)
      return set_err(KS_ERR_INVALID, what + ": node " + std::to_string(n) + ": KSH_CAND_NODE_EMPTINESS_UNPARSABLE without KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP");
    if ((f & ~(dx ? 127u : 15u)) || ((f & KSH_CAND_NODE_DO_NOT_CONSOLIDATE_TRUE) && !(f & KSH_CAND_NODE_DO_NOT_CONSOLIDATE))) return set_err(KS_ERR_INVALID, what + ": node " + std::to_string(n) + ": unknown flag bit");
    if (!std::isfinite(in->node_age_seconds[n])) return set_err(KS_ERR_INVALID, what + ": node " + std::to_string(n) + ": age is not finite");
  }
  for (uint32_t p = 0; p < NP; ++p) {
    if (in->pod_flags[p] & ~7u) return set_err(KS_ERR_INVALID, what + ": pod " + std::to_string(p) + ": unknown flag bit");
    if ((in->pod_flags[p] & KSH_CAND_POD_HAS_DELETION_COST) && !std::isfinite(in->pod_deletion_cost[p])) return set_err(KS_ERR_INVALID, what + ": pod " + std::to_string(p) + ": deletion cost is not finite");
  }
  for (uint32_t m = 0; m < NM; ++m) {
    const int64_t ttl = in->prov_ttl_seconds_until_expired[m];
    if (ttl == 0 || ttl < -1) return set_err(KS_ERR_INVALID, what + ": provisioner " + pr.provisioners[m].name + ": ttlSecondsUntilExpired " + std::to_string(ttl) + " (the reference divides by a ttl of 0; -1 means none)");
    const int64_t ttl_e = dx ? dx->prov_ttl_seconds_after_empty[m] : -1;
    if (ttl_e < -1) return set_err(KS_ERR_INVALID, what + ": provisioner " + pr.provisioners[m].name + ": ttlSecondsAfterEmpty " + std::to_string(ttl_e) + " (-1 means none)");
    if (dx && (ttl > KS_DEPROV_MAX_TTL_SECONDS || ttl_e > KS_DEPROV_MAX_TTL_SECONDS))
      return set_err(KS_ERR_INVALID, what + ": provisioner " + pr.provisioners[m].name + ": a ttl above " + std::to_string(KS_DEPROV_MAX_TTL_SECONDS) + " s wraps as a Duration (Duration(ttl) * time.Second)");
  }
  // selectors -> (key, allowed-set mask): the keys and values some selector mentions
  std::vector<std::string> keys; std::unordered_map<std::string, uint32_t> kindex; std::vector<std::unordered_map<std::string, uint32_t>> vindex;
  auto key_of = [&](const std::string& k) { auto it = kindex.find(k); if (it != kindex.end()) return it->second; const uint32_t id = (uint32_t)keys.size(); kindex.emplace(k, id); keys.push_back(k); vindex.emplace_back(); return id; };
  auto bit_of = [&](uint32_t k, const std::string& v) { auto& m = vindex[k]; auto it = m.find(v); if (it != m.end()) return it->second; const uint32_t id = (uint32_t)m.size(); m.emplace(v, id); return id; };
  for (const ksp::Pdb& b : pdbs) if (!b.selector.nil) {
    for (auto& kv : b.selector.match_labels) bit_of(key_of(kv.first), kv.second);
    for (auto& x : b.selector.match_exprs) { const uint32_t k = key_of(x.key); for (auto& v : x.values) bit_of(k, v); }
  }
  if (!wide && keys.size() > KS_CAND_MAX_KEYS) return set_err(KS_ERR_UNSUPPORTED, what + ": the PDB selectors mention " + std::to_string(keys.size()) + " label keys, " + std::to_string(KS_CAND_MAX_KEYS) + " are supported");
  for (size_t k = 0; !wide && k < keys.size(); ++k) if (vindex[k].size() > KS_CAND_MAX_VALUES)
    return set_err(KS_ERR_UNSUPPORTED, what + ": the PDB selectors mention " + std::to_string(vindex[k].size()) + " values of label key " + keys[k] + ", " + std::to_string(KS_CAND_MAX_VALUES) + " are supported");
  const uint32_t NK = (uint32_t)keys.size(), NB = (uint32_t)pdbs.size();
  // namespaces: the bound pods' get ids; a PDB in a namespace no pod has, and a nil selector (LabelSelectorAsSelector(nil) selects nothing), get an id no pod has
  const uint32_t kNoNs = 0xFFFFFFFFu; std::unordered_map<std::string, uint32_t> nsindex;
  std::vector<uint32_t> pod_ns(NP, 0); std::vector<uint8_t> pod_val(wide ? 0 : (size_t)NK * NP, (uint8_t)KS_CAND_BIT_ABSENT);
  std::vector<uint32_t> lab_off(wide ? (size_t)NP + 1 : 0, 0), lab_key, lab_val;      // the wide route's pod side: per pod the mentioned keys it carries, ascending
  std::vector<std::pair<uint32_t, uint32_t>> mine;
  if (wide) { lab_key.reserve(NP); lab_val.reserve(NP); }
  for (uint32_t p = 0; p < NP; ++p) {
    if (wide) lab_off[p + 1] = lab_off[p];
    if (bind[p] < 0) continue;
    const ksp::Pod& pod = pr.pods[p];
    pod_ns[p] = nsindex.emplace(pod.ns, (uint32_t)nsindex.size()).first->second;
    if (wide) {      // the pod's labels once, key then value: the work goes with the labels, not with keys x pods
      mine.clear();
      for (auto& kv : pod.labels) {
        auto k = kindex.find(kv.first); if (k == kindex.end()) continue;
        auto v = vindex[k->second].find(kv.second);
        mine.emplace_back(k->second, v == vindex[k->second].end() ? (uint32_t)KS_CAND_VALUE_OTHER : v->second);
      }
      if (mine.size() > 1) std::sort(mine.begin(), mine.end());
      if (lab_key.size() + mine.size() > 0xFFFFFFFFull)
        return set_err(KS_ERR_UNSUPPORTED, what + ": " + std::to_string(lab_key.size() + mine.size()) + " selector-mentioned pod labels, " + std::to_string(0xFFFFFFFFull) + " are supported");
      for (auto& kv : mine) { lab_key.push_back(kv.first); lab_val.push_back(kv.second); }
      lab_off[p + 1] = (uint32_t)lab_key.size();
      continue;
    }
    for (uint32_t k = 0; k < NK; ++k) {
      auto it = pod.labels.find(keys[k]); if (it == pod.labels.end()) continue;
      auto v = vindex[k].find(it->second);
      pod_val[(size_t)k * NP + p] = v == vindex[k].end() ? (uint8_t)KS_CAND_BIT_OTHER : (uint8_t)v->second;
    }
  }
  std::vector<uint32_t> pdb_ns(NB), req_off(NB + 1, 0), req_key; std::vector<int32_t> pdb_allowed(NB); std::vector<uint64_t> req_mask;
  std::vector<uint32_t> req_op, req_val; std::vector<size_t> req_val_off(1, 0);      // (the wide route's PDB side)
  const uint64_t kAbsent = 1ull << KS_CAND_BIT_ABSENT;
  for (uint32_t b = 0; b < NB; ++b) {
    const ksp::Pdb& d = pdbs[b]; auto ns = nsindex.find(d.ns);
    pdb_ns[b] = (d.selector.nil || ns == nsindex.end()) ? kNoNs : ns->second; pdb_allowed[b] = d.disruptions_allowed;
    if (!d.selector.nil && wide) {      // per requirement an operator and the value ids, sorted and each once, in one pool
      auto list = [&](uint32_t k, uint32_t op, const std::vector<uint32_t>& ids) {
        req_key.push_back(k); req_op.push_back(op); req_val.insert(req_val.end(), ids.begin(), ids.end()); req_val_off.push_back(req_val.size());
      };
      std::vector<uint32_t> ids;
      for (auto& kv : d.selector.match_labels) { const uint32_t k = kindex[kv.first]; ids.assign(1, vindex[k][kv.second]); list(k, KS_CAND_OP_IN, ids); }
      for (auto& x : d.selector.match_exprs) {
        const uint32_t k = kindex[x.key]; ids.clear();
        if (x.op == ksp::Op::In || x.op == ksp::Op::NotIn) { for (auto& v : x.values) ids.push_back(vindex[k][v]); std::sort(ids.begin(), ids.end()); ids.erase(std::unique(ids.begin(), ids.end()), ids.end()); }
        list(k, x.op == ksp::Op::In ? KS_CAND_OP_IN : x.op == ksp::Op::NotIn ? KS_CAND_OP_NOT_IN : x.op == ksp::Op::Exists ? KS_CAND_OP_EXISTS : KS_CAND_OP_DOES_NOT_EXIST, ids);
      }
    } else if (!d.selector.nil) {
      for (auto& kv : d.selector.match_labels) { const uint32_t k = kindex[kv.first]; req_key.push_back(k); req_mask.push_back(1ull << vindex[k][kv.second]); }
      for (auto& x : d.selector.match_exprs) {
        const uint32_t k = kindex[x.key]; uint64_t bits = 0; for (auto& v : x.values) bits |= 1ull << vindex[k][v];
        req_key.push_back(k);
        req_mask.push_back(x.op == ksp::Op::In ? bits : x.op == ksp::Op::NotIn ? ~bits : x.op == ksp::Op::Exists ? ~kAbsent : kAbsent);
      }
    }
    req_off[b + 1] = (uint32_t)req_key.size();
  }
  // nodes: the reason the host can give (the reference's order), the provisioner's ttl, the pods in ascending slot order
  std::vector<uint8_t> is_del(NN, 0); for (uint32_t i = 0; i < n_deleting; ++i) is_del[deleting[i]] = 1;
  std::vector<uint32_t> node_why(NN, 0), pods_off(NN + 1, 0), node_pods, node_dflags(dx ? NN : 0, 0); std::vector<int64_t> node_ttl(NN, -1), node_ttl_e(dx ? NN : 0, -1);
  for (uint32_t n = 0; n < NN; ++n) {
    const uint32_t f = in->node_flags[n]; uint32_t w = 0;
    if (cs.why[n] == KS_CAND_WHY_LEFT) w = KS_CAND_WHY_LEFT;
    else if (is_del[n]) w = 1;                                                                   // helpers.go:186
    else if (cs.why[n]) w = cs.why[n];                                                           // :190-211
    else if (f & KSH_CAND_NODE_NOMINATED) w = 7;                                                 // :215
    node_why[n] = w;      // codes 1-7 and 13 are the same under every method
    if (w != 0) continue;
    if (dx) {      // the method's ShouldDeprovision and canBeTerminated are the device's: it needs the provisioner's ttls and the node's flags
      node_dflags[n] = ((f & KSH_CAND_NODE_DELETION_TIMESTAMP) ? KS_DEPROV_NODE_DELETION_TIMESTAMP : 0u) | ((f & KSH_CAND_NODE_HAS_EMPTINESS_TIMESTAMP) ? KS_DEPROV_NODE_HAS_EMPTINESS : 0u) |
                       ((f & KSH_CAND_NODE_EMPTINESS_UNPARSABLE) ? KS_DEPROV_NODE_EMPTINESS_UNPARSABLE : 0u) | ((f & KSH_CAND_NODE_DRIFTED) ? KS_DEPROV_NODE_DRIFTED : 0u);
      node_ttl[n] = in->prov_ttl_seconds_until_expired[cs.prov[n]]; node_ttl_e[n] = dx->prov_ttl_seconds_after_empty[cs.prov[n]];
    } else {       // consolidation.ShouldDeprovision, then the deletion timestamp of canBeTerminated
      if (f & KSH_CAND_NODE_DO_NOT_CONSOLIDATE) w = (f & KSH_CAND_NODE_DO_NOT_CONSOLIDATE_TRUE) ? 8 : 0;      // consolidation.go:108-111: `return val != "true"`
      else if (!in->prov_consolidation_enabled[cs.prov[n]]) w = 9;                                           // :116-119
      if (w == 0 && (f & KSH_CAND_NODE_DELETION_TIMESTAMP)) w = KS_CAND_WHY_DELETING_NODE;                   // helpers.go:340
      node_why[n] = w;
      if (w == 0 || w == KS_CAND_WHY_DELETING_NODE) node_ttl[n] = in->prov_ttl_seconds_until_expired[cs.prov[n]];
    }
  }
  for (uint32_t p = 0; p < NP; ++p) if (bind[p] >= 0) pods_off[(size_t)bind[p] + 1]++;
  for (uint32_t n = 0; n < NN; ++n) pods_off[n + 1] += pods_off[n];
  node_pods.resize(pods_off[NN]);
  { std::vector<uint32_t> fill(pods_off.begin(), pods_off.end() - 1); for (uint32_t p = 0; p < NP; ++p) if (bind[p] >= 0) node_pods[fill[bind[p]]++] = p; }
  ks_candidates_inputs ki{}; ki.n_pods = NP; ki.n_nodes = NN; ki.n_pdbs = NB; ki.n_keys = NK;
  ki.pod_node = bind.data(); ki.pod_ns = pod_ns.data(); ki.pod_flags = in->pod_flags; ki.pod_deletion_cost = in->pod_deletion_cost; ki.pod_priority = in->pod_priority; ki.pod_val = pod_val.data();
  ki.pdb_ns = pdb_ns.data(); ki.pdb_allowed = pdb_allowed.data(); ki.pdb_req_off = req_off.data(); ki.pdb_req_key = req_key.data(); ki.pdb_req_mask = req_mask.data();
  ki.node_why = node_why.data(); ki.node_age_seconds = in->node_age_seconds; ki.node_ttl_seconds = node_ttl.data(); ki.node_pods_off = pods_off.data(); ki.node_pods = node_pods.data();
  ks_selector_lists sl{}; std::vector<uint32_t> key_nv, val_off32;
  if (wide) {
    if (req_val.size() > 0xFFFFFFFFull) return set_err(KS_ERR_UNSUPPORTED, what + ": " + std::to_string(req_val.size()) + " selector values in all, " + std::to_string(0xFFFFFFFFull) + " are supported");
    key_nv.resize(NK); for (uint32_t k = 0; k < NK; ++k) key_nv[k] = (uint32_t)vindex[k].size();
    val_off32.assign(req_val_off.begin(), req_val_off.end());
    ki.n_keys = 0; ki.pod_val = nullptr; ki.pdb_req_key = nullptr; ki.pdb_req_mask = nullptr;
    sl.n_keys = NK; sl.n_namespaces = (uint32_t)nsindex.size(); sl.key_n_values = key_nv.data(); sl.pod_label_off = lab_off.data(); sl.pod_label_key = lab_key.data(); sl.pod_label_val = lab_val.data();
    sl.req_key = req_key.data(); sl.req_op = req_op.data(); sl.req_val_off = val_off32.data(); sl.req_val = req_val.data();
  }
  ks_candidates_outputs ko{}; ko.order = out->order; ko.empty = out->empty; ko.why = out->why; ko.detail = out->detail; ko.n_node_pods = out->n_node_pods; ko.cost = out->cost;
  const double host_ms = ms_since(t_call);
  double kms[3] = {0, 0, 0};
  int rc;
  if (dx) {
    ks_deprov_inputs di{}; di.c = ki; di.method = method; di.drift_enabled = dx->drift_enabled; di.now_unix_nanos = dx->now_unix_nanos; di.node_dflags = node_dflags.data();
    di.node_creation_unix_nanos = dx->node_creation_unix_nanos; di.node_emptiness_unix_nanos = dx->node_emptiness_unix_nanos; di.node_ttl_seconds_after_empty = node_ttl_e.data();
    ks_deprov_outputs dout{}; dout.c = ko;
    rc = wide ? ks_deprovisioning_candidates_lists_host(&di, &sl, &dout, device, kms) : ks_deprovisioning_candidates_host(&di, &dout, device, kms);
    ko = dout.c; if (n_in_result) *n_in_result = dout.n_in_result;
  } else rc = wide ? ks_consolidation_candidates_lists_host(&ki, &sl, &ko, device, kms) : ks_consolidation_candidates_host(&ki, &ko, device, kms);
  if (rc != KS_OK) return dev_rc(rc);
  out->n_candidates = ko.n_candidates; out->n_empty = ko.n_empty;
  if (ms) { ms[0] = host_ms; ms[1] = kms[0]; ms[2] = kms[1]; ms[3] = kms[2]; }
  return KS_OK;
}
}  // namespace
extern "C" {
int ksh_consolidation_candidates(void* parsed, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, const ksh_candidate_inputs* in, const ksh_pdb_block* pdbs, int device,
                                 ksh_candidates_out* out, double* ms) {
  return ksh_consolidation_candidates_ex(parsed, pod_node, deleting, n_deleting, in, pdbs, device, 0, out, ms);
}
int ksh_consolidation_candidates_ex(void* parsed, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, const ksh_candidate_inputs* in, const ksh_pdb_block* pdbs, int device,
                                    uint32_t flags, ksh_candidates_out* out, double* ms) {
  return guarded([&] { return candidates_over((Parsed*)parsed, 0, pod_node, deleting, n_deleting, in, nullptr, pdbs, device, flags, out, nullptr, ms); });
}
// candidateNodes under Expiration / Drift / Emptiness.ShouldDeprovision and the order their ComputeCommand walks (kshost.h)
int ksh_deprovisioning_candidates(void* parsed, uint32_t method, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, const ksh_deprovisioning_inputs* in,
                                  const ksh_pdb_block* pdbs, int device, ksh_deprovisioning_out* out, double* ms) {
  return ksh_deprovisioning_candidates_ex(parsed, method, pod_node, deleting, n_deleting, in, pdbs, device, 0, out, ms);
}
int ksh_deprovisioning_candidates_ex(void* parsed, uint32_t method, const int32_t* pod_node, const uint32_t* deleting, uint32_t n_deleting, const ksh_deprovisioning_inputs* in,
                                     const ksh_pdb_block* pdbs, int device, uint32_t flags, ksh_deprovisioning_out* out, double* ms) {
  if (!in || !out) return set_err(KS_ERR_INVALID, "null argument");
  return guarded([&] {
    uint32_t n_in_result = 0;
    const int rc = candidates_over((Parsed*)parsed, method, pod_node, deleting, n_deleting, &in->base, in, pdbs, device, flags, &out->base, &n_in_result, ms);
    if (rc == KS_OK) out->n_in_result = n_in_result;
    return rc;
  });
}
// Emptiness.ComputeCommand (emptiness.go:73-82), literally: of the candidates those without pods, all deleted in one command; none -> do-nothing.  Host only.
int ksh_emptiness_command(const uint32_t* candidates, uint32_t n, const uint32_t* n_node_pods, uint32_t* out_action, uint32_t* out_nodes, uint32_t* out_n_nodes) {
  if (!out_action || !out_n_nodes || (n && (!candidates || !n_node_pods || !out_nodes))) return set_err(KS_ERR_INVALID, "null argument");
  uint32_t k = 0;
  for (uint32_t i = 0; i < n; ++i) if (n_node_pods[candidates[i]] == 0) out_nodes[k++] = candidates[i];
  *out_n_nodes = k; *out_action = k ? KS_CMD_DELETE : KS_CMD_DO_NOTHING;
  return KS_OK;
}
// The names behind a row, without a handle: what 0 = requirement key a, 1 = value b of key a (the flattening's universes: available once a what-if call flattened the
// snapshot), 3 = state node a, 4 = instance type a, 5 / 6 = value a of the zone / capacity-type universe (a launch pick's ids).  NULL when out of range.
const char* ksh_snapshot_name(void* parsed, int what, uint32_t a, uint32_t b) {
  Parsed* P = (Parsed*)parsed; if (!P) return nullptr;
  std::lock_guard<std::mutex> g(P->mu);
  if (what == 3) return a < P->pr->nodes.size() ? P->pr->nodes[a].name.c_str() : nullptr;
  if (what == 4) return a < P->pr->instance_types.size() ? P->pr->instance_types[a].name.c_str() : nullptr;
  if (!P->sb) return nullptr;
  const char* name = nullptr;
  guarded([&] {
    const ksh::Encoded& E = *ksh::delta_inputs(*P->sb).base;
    if (what == 0 && a < E.key_names.size()) name = E.key_names[a].c_str();
    if (what == 1 && a < E.key_values.size() && b < E.key_values[a].size()) name = E.key_values[a][b].c_str();
    if (what == 2 && a < E.res_names.size()) name = E.res_names[a].c_str();
    if (what == 5 || what == 6) { const int32_t k = what == 5 ? E.prob.key_zone : E.prob.key_ct; if (k >= 0 && a < E.key_values[k].size()) name = E.key_values[k][a].c_str(); }
    return KS_OK;
  });
  return name;
}
// the instance-type key's requirement of a row (KS_CMD_IT_STATE), spelled out: *complement, the number of values; value i through ksh_snapshot_it_state_value
int ksh_snapshot_it_state(void* parsed, uint32_t state, int* complement, uint32_t* n_values) {
  Parsed* P = (Parsed*)parsed; if (!P || !complement || !n_values) return set_err(KS_ERR_INVALID, "null argument");
  std::lock_guard<std::mutex> g(P->mu);
  if (!P->sb) return set_err(KS_ERR_INVALID, "the snapshot was not flattened yet");
  return guarded([&] {
    const ksh::Encoded& L = ksh::delta_inputs(*P->sb).base->lattice();
    if (state == 0 || state >= L.it_states.size()) return set_err(KS_ERR_INVALID, "instance-type state out of range");
    *complement = L.it_states[state].complement ? 1 : 0; *n_values = (uint32_t)L.it_states[state].values.size(); return KS_OK;
  });
}
const char* ksh_snapshot_it_state_value(void* parsed, uint32_t state, uint32_t i) {
  Parsed* P = (Parsed*)parsed; if (!P) return nullptr;
  std::lock_guard<std::mutex> g(P->mu);
  if (!P->sb) return nullptr;
  const char* value = nullptr;
  guarded([&] {
    const ksh::Encoded& L = ksh::delta_inputs(*P->sb).base->lattice();
    if (state == 0 || state >= L.it_states.size() || i >= L.it_states[state].values.size()) return KS_OK;
    auto it = L.it_states[state].values.begin(); std::advance(it, i); value = it->c_str(); return KS_OK;
  });
  return value;
}
int ksh_pack_width(void* hv, int* out) { Handle* h = (Handle*)hv; if (!h || !h->dev) return KS_ERR_INVALID; return ks_problem_pack_width(h->dev, out); }
int ksh_pack_lean(void* hv, int* out) { Handle* h = (Handle*)hv; if (!h || !h->dev) return KS_ERR_INVALID; return ks_problem_pack_lean(h->dev, out); }
int ksh_pack_row(void* hv, int* out) { Handle* h = (Handle*)hv; if (!h || !h->dev) return KS_ERR_INVALID; return ks_problem_pack_row(h->dev, out); }
int ksh_rr_status(void* hv, int* out2) { Handle* h = (Handle*)hv; if (!h || !h->dev) return KS_ERR_INVALID; return ks_problem_rr_status(h->dev, out2, out2 + 1); }
void ksh_dims(void* hv, uint32_t* d) { const ks_problem& p = ((Handle*)hv)->enc->prob; uint32_t v[10] = {p.P, p.C, p.T, p.M, p.E, p.K, p.R, p.G, p.GH, p.S}; memcpy(d, v, sizeof v); }

}  // extern "C"
