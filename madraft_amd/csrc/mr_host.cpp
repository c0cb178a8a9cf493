// mr_host.cpp — C ABI of include/madraft_sim.h on one MI355X: allocates the
// cluster-minor SoA of mr_dev.h in HBM (sized for the config, hundreds of
// GB fit on a 288 GB part), and drives the step kernel in bounded launches
// on the batch's own HIP stream, timing each launch with HIP events on that
// stream.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "mr_dev.h"

namespace mr {
// ---- one map from (scenario, servers, kernel family) to the kernel instance that runs it
enum Family : uint32_t { F_STEP, F_POOL, F_TAPE };
template <uint32_t S_, uint32_t NB_, Family F_>
struct Inst { static constexpr uint32_t S = S_, NB = NB_, F = F_; };
// scenarios this library holds instances of: all of the table's, or the few of a dev variant
// (build.py scns=); a debug library may also lack the decision-tape kernels (build.build_guard)
#ifdef MR_DEV_SCNS
#define MR_BUILT_SCNS MR_DEV_SCNS
#else
#define MR_BUILT_SCNS MR_ALL_SCNS
#endif
#if MR_NO_TAPE
constexpr bool k_has_tape = false;
#else
constexpr bool k_has_tape = true;
#endif
template <uint32_t S, uint32_t NB, class Fn>
static bool visit_exact(uint32_t n, Family fam, Fn& fn) {
  if (n != NB) return false;
  if constexpr (has_pool(S, NB)) if (fam == F_POOL) return fn(Inst<S, NB, F_POOL>{}), true;
  if constexpr (has_exact(S, NB)) if (fam == F_STEP) return fn(Inst<S, NB, F_STEP>{}), true;
  return false;
}
// Calls fn(Inst<S, NB, F>{}) with the instance of scenario `scn` for n servers in family `fam`: the
// exact-size one where it is built (mr_dev.h has_exact / has_pool), else for the step kernel the
// 8-server one; tape kernels exist at 8 only. False, and no call, if the library holds none.
template <class Fn>
static bool visit_instance(uint32_t scn, uint32_t n, Family fam, Fn fn) {
  switch (scn) {
#define MR_INST(S)                                                                        \
  case S:                                                                                 \
    if constexpr (k_has_tape)                                                             \
      if (fam == F_TAPE) return fn(Inst<S, MR_MAX_NODES, F_TAPE>{}), true;                \
    if (fam == F_TAPE) return false;                                                      \
    return visit_exact<S, 3>(n, fam, fn) || visit_exact<S, 5>(n, fam, fn) ||              \
           visit_exact<S, 7>(n, fam, fn) ||                                               \
           (fam == F_STEP && (fn(Inst<S, MR_MAX_NODES, F_STEP>{}), true));
    MR_BUILT_SCNS
#undef MR_INST
    default: return false;
  }
}
static Family family_of(const Dev& D) { return D.tape_mode ? F_TAPE : D.pool ? F_POOL : F_STEP; }
// the kernel instance of scenario `scn` for this batch
hipError_t launch_step(const Dev& D, uint32_t scn, uint32_t budget, hipStream_t s) {
  hipError_t r = hipErrorInvalidValue;
  visit_instance(scn, D.n, family_of(D), [&](auto i) {
    using I = decltype(i);
    if constexpr (I::F == F_TAPE) r = launch_step_tape_t<I::S, I::NB>(D, budget, s);
    else if constexpr (I::F == F_POOL) r = launch_pool_t<I::S, I::NB>(D, budget, s);
    else r = launch_step_t<I::S, I::NB>(D, budget, s);
  });
  return r;
}
// clusters the scenario's pool / step kernel keeps resident (0: unknown)
static uint32_t step_capacity(const Dev& D, uint32_t scn, int device) {
  uint32_t cap = 0;
  visit_instance(scn, D.n, D.pool ? F_POOL : F_STEP, [&](auto i) {
    using I = decltype(i);
    if constexpr (I::F == F_POOL) cap = pool_capacity_t<I::S, I::NB>(device, D.M);
    else cap = step_capacity_t<I::S, I::NB>(device, D.M);
  });
  return cap;
}
// the pool kernel serves this batch: an instance exists, the key rows fit (pool_max_slots), and the
// environment does not turn it off (MR_POOL=0: the per-lane step kernel, for A/B runs)
static bool use_pool(uint32_t scn, uint32_t n, uint32_t M) {
  if (const char* e = std::getenv("MR_POOL")) if (e[0] == '0') return false;
  bool fits = false;
  visit_instance(scn, n, F_POOL, [&](auto i) { fits = M <= pool_max_slots(i.S, i.NB); });
  return fits;
}
hipError_t launch_reset(const Dev& D, hipStream_t s);
hipError_t launch_reduce(const Dev& D, unsigned long long* out, uint64_t cluster_base,
                         hipStream_t s);
hipError_t launch_tape_pack(const uint4* tape, const uint32_t* used, uint32_t dcap, uint32_t first,
                            uint32_t count, const uint64_t* off, uint32_t* out, hipStream_t s);
}  // namespace mr

using namespace mr;

namespace {
thread_local std::string g_err;

int set_err(const std::string& s) {
  g_err = s;
  return -1;
}
#define HIPCHK(expr)                                                                  \
  do {                                                                                \
    hipError_t e_ = (expr);                                                           \
    if (e_ != hipSuccess)                                                             \
      return set_err(std::string(#expr) + ": " + hipGetErrorString(e_));              \
  } while (0)

constexpr uint32_t STEP_LANES = 64;  // lanes per step-kernel block (one wave)

// who installed a batch's decision tables: what the lifetime rules ask (variants_enter drops only a
// variant's, a seed list and variants exclude each other, set_variant_masks needs a variant's)
enum Owner : uint32_t { OWN_NONE, OWN_REPLAY, OWN_RECORD, OWN_VARIANTS };

// A batch's decision tables on the device, each its own allocation, whoever made them: the record
// tape (MR_F_RECORD), or what stage_slices built, the sorted slices and the clusters' descriptors
// of a replay, and with them a variant batch's edits and masks. All null: Philox draws.
struct Tables {
  uint4* tape = nullptr;      // keyed decisions: the record tape, or the groups' sorted slices
  uint4* tdesc = nullptr;     // slices: the clusters' group descriptors;
  uint32_t* vedit = nullptr;  // variants: the base records' edit indices within their group,
  uint2* vwords = nullptr;    // the edits' words,
  uint32_t* vmask = nullptr;  // and the clusters' mask rows (set_variant_masks rewrites them)
  uint32_t dcap = 0, vW = 0;  // Dev's dcap and vW with these tables
  Owner mode = OWN_NONE;
};

void free_tables(Tables& t) {
  for (void* p : {(void*)t.tape, (void*)t.tdesc, (void*)t.vedit, (void*)t.vwords, (void*)t.vmask})
    if (p) (void)hipFree(p);
  t = Tables{};
}

// *dst = a new device array of max(count, 1) elements: src[0 .. count), or zeros for a null src
template <class T>
hipError_t upload(T** dst, const T* src, size_t count) {
  const hipError_t e = hipMalloc(dst, (count ? count : 1) * sizeof(T));
  if (e != hipSuccess || !count) return e;
  return src ? hipMemcpy(*dst, src, count * sizeof(T), hipMemcpyHostToDevice)
             : hipMemset(*dst, 0, count * sizeof(T));
}
}  // namespace

struct mr_batch {
  mr_cfg cfg;
  Dev D;
  void* base = nullptr;
  DevLayout lay;  // where `base` holds D's arrays, and what a reset zeroes
  unsigned long long* red = nullptr;
  uint32_t* h_remaining = nullptr;  // [2]: remaining, next unclaimed cluster (D.remaining)
  uint32_t* h_ctl0 = nullptr;       // [2]: {0, L}, copied to D.remaining before each launch
  uint32_t c_open = 0;              // first cluster of the first chunk not yet finished
  uint32_t* held[2] = {nullptr, nullptr};  // streaming: clusters held at a launch's end (ping-pong)
  uint32_t hsel = 0;                // held[hsel] = the next launch's held_in
  bool resume = false;              // streaming: the next launch continues the current chunk
  hipStream_t stream = nullptr;
  hipEvent_t ev0 = nullptr, ev1 = nullptr;
  uint32_t budget = 16384;  // events per cluster per launch (MR_STEP_BUDGET)
  Tables dec;                // the decision tables D draws from (install_tables)
  uint32_t* sof = nullptr;   // the seed list (mr_batch_set_seeds): the batch's, not its tables'
  bool submitted = false;    // mr_batch_submit enqueued a step not yet finished
  uint32_t kern = 0;         // kernel family of the launches since the reset: 1 pool, 2 step / tape
  std::chrono::steady_clock::time_point t_submit;
};

// traced cluster k's row of `rows` ([trace_clusters][trace_cap]): its records so far, at most cap
template <class T>
static int copy_trace_row(mr_batch* b, uint32_t k, const T* rows, T* out, size_t cap, size_t* n) {
  uint32_t tn = 0;
  HIPCHK(hipMemcpy(&tn, b->D.cs32 + CS_IDX(CS_TRACEN, k, b->D.C), 4, hipMemcpyDeviceToHost));
  size_t m = tn < b->D.trace_cap ? tn : b->D.trace_cap;
  if (m > cap) m = cap;
  HIPCHK(hipMemcpy(out, rows + (size_t)k * b->D.trace_cap, m * sizeof(T), hipMemcpyDeviceToHost));
  *n = m;
  return 0;
}

// Dev's tape_mode: what a draw does with the owner's tables, or with a seed list and no tables
static TapeMode tape_mode_of(const mr_batch* b) {
  if (b->dec.mode == OWN_RECORD) return TAPE_RECORD;
  return b->dec.mode != OWN_NONE ? TAPE_LOOKUP : b->sof ? TAPE_SEEDS : TAPE_OFF;
}

// `t` (staged whole by the caller) becomes the batch's decision tables, the previous ones are
// freed, and the kernels' view of them is published into D
static void install_tables(mr_batch* b, const Tables& t) {
  free_tables(b->dec);
  b->dec = t;
  Dev& D = b->D;
  D.dtab = t.tape; D.dcap = t.dcap;
  D.tdesc = t.tdesc; D.vedit = t.vedit; D.vwords = t.vwords; D.vmask = t.vmask; D.vW = t.vW;
  D.tape_mode = tape_mode_of(b);
}

// A C entry point whose host allocations may throw: an error code across the C ABI, never an
// exception
template <class Fn>
static int no_throw(const char* name, Fn fn) {
  try {
    return fn();
  } catch (const std::exception& e) {
    return set_err(std::string(name) + ": " + e.what());
  }
}

extern "C" {

const char* mr_last_error(void) { return g_err.c_str(); }

const char* mr_scenario_name(uint32_t s) {
  switch (s) {
#define MR_ROW_(id, sym, name, n, kind, slots, exact, pool) case id: return name;
    MR_SCENARIO_TABLE(MR_ROW_)
#undef MR_ROW_
    default: return "";
  }
}

uint32_t mr_scenario_from_name(const char* name) {
  if (!name) return 0;
  for (uint32_t i = 1; i < MR_SCN_COUNT_; i++)
    if (std::strcmp(name, mr_scenario_name(i)) == 0) return i;
  return 0;
}

const char* mr_fail_message(uint32_t code) {
  switch (code) {
#define MR_ROW_(code, sym, msg) case code: return msg;
    MR_FAIL_TABLE(MR_ROW_)
#undef MR_ROW_
    default: return "unknown";
  }
}

int mr_cfg_init(mr_cfg* c, uint32_t scn) {
  if (!c) return set_err("null cfg");
  return mr_cfg_defaults(c, scn) == 0 ? 0 : set_err("unknown scenario");
}

static int validate(const mr_cfg* c) {
  if (!c) return set_err("null cfg");
  if (c->abi_version != MR_ABI_VERSION) return set_err("abi_version mismatch");
  if (mr_scn_servers(c->scenario) == 0) return set_err("unknown scenario");
  if (const char* bad = mr_cfg_check_caps(c)) return set_err(bad);  // shared with the oracle
  if (c->n_clusters == 0 || c->n_clusters > (1ull << 31)) return set_err("bad n_clusters");
  if (c->elect_hi_us <= c->elect_lo_us || c->hb_us == 0) return set_err("bad timers");
  if (c->max_events == 0) return set_err("max_events must be > 0");
  if ((c->flags & MR_F_TRACE) && (c->trace_cap == 0 || c->trace_clusters > c->n_clusters))
    return set_err("bad trace config");
  if (c->lanes_per_wave != 0 && c->lanes_per_wave != 16 && c->lanes_per_wave != 32 &&
      c->lanes_per_wave != 64)
    return set_err("lanes_per_wave must be 0 (auto), 16, 32 or 64");
  if ((c->flags & MR_F_RECORD) && c->tape_cap < 1)
    return set_err("MR_F_RECORD needs tape_cap >= 1 (decisions kept per cluster)");
  return 0;
}

static int mr_batch_create_impl(const mr_cfg* cfg, mr_batch** out) {
  if (!out) return set_err("null out");
  *out = nullptr;
  if (validate(cfg) != 0) return -1;
  const uint32_t scn = cfg->scenario;

  mr_batch* b = new mr_batch();
  b->cfg = *cfg;
  Dev& D = b->D;
  std::memset(&D, 0, sizeof D);
  const uint64_t C = cfg->n_clusters, n = cfg->n_nodes, M = cfg->msg_slots;
  D.C = (uint32_t)C;
  D.L = cfg->lanes && cfg->lanes < C ? cfg->lanes : (uint32_t)C;  // no tape: capacity (below)
  D.stream = (cfg->flags & MR_F_STREAM) ? 1u : 0u;
  D.n = (uint32_t)n; D.log_cap = cfg->log_cap; D.apply_cap = cfg->apply_cap;
  D.M = (uint32_t)M; D.K = cfg->ae_max; D.hb = cfg->hb_us; D.elo = cfg->elect_lo_us;
  D.ehi = cfg->elect_hi_us; D.max_events = cfg->max_events;
  D.null_raft = (cfg->flags & MR_F_NULL_RAFT) ? 1u : 0u;
  D.unrel_flag = (cfg->flags & MR_F_UNRELIABLE) ? 1u : 0u;
  D.safety = (cfg->flags & MR_F_SAFETY) ? 1u : 0u;
  D.bugs = cfg->flags & (MR_F_BUG_VOTE_TWICE | MR_F_BUG_VOTE_STALE | MR_F_BUG_NO_PREV_CHECK |
                         MR_F_BUG_NO_DEDUP | MR_F_BUG_STALE_READ | MR_F_BUG_NO_APPLY_CHECK);
  scenario_fixed(D, scn);
  D.trace_clusters = (cfg->flags & MR_F_TRACE) ? cfg->trace_clusters : 0u;
  D.trace_cap = cfg->trace_cap;
  D.scenario = scn;
  // loop counts of the test bodies (tests.rs): many_election 10, figure_8 1000, snap_common 30
  uint32_t def_iters = scn == MR_SCN_MANY_ELECTION_2A ? 10 : mr_scn_is_snap2d(scn) ? 30 : 1000;
  D.iters = cfg->iters ? cfg->iters : def_iters;
  D.seed0 = cfg->seed_base + cfg->cluster_base;
  D.pool = !(cfg->flags & MR_F_RECORD) && use_pool(scn, (uint32_t)n, (uint32_t)M) ? 1u : 0u;

  // field matrices use 32-bit element offsets in the kernels
  const uint64_t lim = 1ull << 32;
  if ((uint64_t)CS_STRIDE * C >= lim || (uint64_t)C64_STRIDE * C >= lim || M * C >= lim) {
    delete b;
    return set_err("n_clusters too large for one batch (32-bit field offsets)");
  }
  b->lay = dev_layout(*cfg);  // one allocation; every array 256-B aligned (mr_dev.h MR_DEV_ARRAYS)
  hipError_t e = hipSetDevice(cfg->device);
  if (e == hipSuccess) e = hipMalloc(&b->base, b->lay.off[A__N]);
  if (e == hipSuccess) e = hipMalloc(&b->red, RED_N * sizeof(unsigned long long));
  if (e == hipSuccess) e = hipHostMalloc(&b->h_remaining, 2 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipHostMalloc(&b->h_ctl0, 2 * sizeof(uint32_t));
  if (e == hipSuccess) e = hipStreamCreateWithFlags(&b->stream, hipStreamNonBlocking);
  if (e == hipSuccess) e = hipEventCreate(&b->ev0);
  if (e == hipSuccess) e = hipEventCreate(&b->ev1);
  if (e != hipSuccess) {
    std::string msg = std::string("allocation of ") + std::to_string(b->lay.off[A__N]) + " B failed: " +
                      hipGetErrorString(e);
    mr_batch_destroy(b);
    return set_err(msg);
  }
  dev_carve(D, b->lay, static_cast<char*>(b->base));
  if (cfg->flags & MR_F_RECORD) {
    Tables t;  // (the tape is written before it is read: not filled)
    e = hipMalloc(&t.tape, (size_t)C * cfg->tape_cap * sizeof(uint4));
    if (e != hipSuccess) {
      mr_batch_destroy(b);
      return set_err(std::string("tape allocation failed: ") + hipGetErrorString(e));
    }
    t.dcap = cfg->tape_cap;
    t.mode = OWN_RECORD;
    install_tables(b, t);
  }
  if (hipMemset(b->D.prof, 0, PROF_SLOTS * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(b->D.guard, 0, 4 * sizeof(uint32_t)) != hipSuccess) {
    mr_batch_destroy(b);
    return set_err("hipMemset failed");
  }
  // lanes per wave: as configured, else 32 when the batch (or its chunk) fills at most half of
  // the resident lanes — two half-full waves per SIMD hide the latency chains better than one
  // full one — else 64
  const uint32_t cap = step_capacity(b->D, scn, cfg->device);  // resident lanes (64 per wave)
  b->D.lpw = cfg->lanes_per_wave ? cfg->lanes_per_wave
             : (cap && (uint64_t)(cfg->lanes && cfg->lanes < C ? cfg->lanes : C) * 2u <= cap) ? 32u : 64u;
  if (!cfg->lanes) {  // a batch bigger than the resident waves runs as chunks of that size
    const uint32_t capc = (uint32_t)((uint64_t)cap * b->D.lpw / STEP_LANES);
    if (capc && capc < b->D.C) {
      b->D.L = capc;
      // a pool kernel refills its slots from the rest of the batch (streaming) instead of
      // draining once per chunk (config 3's whole job on one GPU +10 %)
      if (b->D.pool && !b->D.tape_mode) b->D.stream = 1u;
    }
  }
  if (b->D.stream) {  // held-cluster lists, L entries each (L <= C)
    e = hipMalloc(&b->held[0], (size_t)b->D.C * sizeof(uint32_t));
    if (e == hipSuccess) e = hipMalloc(&b->held[1], (size_t)b->D.C * sizeof(uint32_t));
    if (e != hipSuccess) {
      mr_batch_destroy(b);
      return set_err(std::string("held-list allocation failed: ") + hipGetErrorString(e));
    }
  }
  // the 7-server Raft pool's LDS key rows (32); MR_KEY_ROWS (tests) puts more slots' keys in HBM
  b->D.krows = 32u;
  if (const char* s = std::getenv("MR_KEY_ROWS")) {
    const int r = std::atoi(s);
    if (r >= 1 && r <= 32) b->D.krows = (uint32_t)r;
  }
  if (const char* s = std::getenv("MR_STEP_BUDGET")) b->budget = (uint32_t)std::atoi(s);
  if (b->budget == 0) b->budget = 16384;
  if (mr_batch_reset(b, cfg->seed_base) != 0) {
    std::string msg = g_err;
    mr_batch_destroy(b);
    return set_err(msg);
  }
  *out = b;
  return 0;
}

static int enqueue_reset(mr_batch* b, uint64_t seed_base) {
  b->cfg.seed_base = seed_base;
  b->kern = 0;
  b->c_open = 0;
  b->resume = false;
  b->D.seed0 = seed_base + b->cfg.cluster_base;
  HIPCHK(hipSetDevice(b->cfg.device));
  for (int k = 0; k < (int)A__N; k++)  // the table's ZERO rows this batch has, by their place k
    for (uint32_t a = 0; a < A__N; a++)
      if (k_dev_reset[a] == k && b->lay.bytes[a])
        HIPCHK(hipMemsetAsync(static_cast<char*>(b->base) + b->lay.off[a], 0, b->lay.bytes[a], b->stream));
#if MR_GUARD
  b->D.gprobe = std::getenv("MR_GUARD_PROBE") ? 1u : 0u;
#endif
  HIPCHK(launch_reset(b->D, b->stream));
  return 0;
}

// one step-kernel launch on the batch stream, bracketed by the timing events;
// the remaining-cluster count is copied back asynchronously
static int enqueue_step(mr_batch* b, uint32_t budget) {
  // the pool kernel's message keys (32-bit, AppendEntries bit) and the step / tape kernels' are
  // different HBM formats: a run does not switch family between its launches
  const uint32_t kern = b->D.pool && !b->D.tape_mode ? 1u : 2u;
  if (b->kern && b->kern != kern)
    return set_err("decisions set or dropped in the middle of a pool-kernel run: mr_batch_reset first");
  b->kern = kern;
  b->h_ctl0[0] = 0;
  if (b->D.stream && b->resume) {  // continue: the held clusters first, the claim pointer kept
    b->h_ctl0[1] = b->h_remaining[1];
    b->D.nheld = b->h_remaining[0];
    b->D.resume = 1;
  } else {
    b->h_ctl0[1] = b->D.c0 + b->D.L;  // lanes start with clusters c0 .. c0+L-1 (streaming: claim on)
    b->D.nheld = 0;
    b->D.resume = 0;
  }
  b->D.held_in = b->held[b->hsel];
  b->D.held_out = b->held[b->hsel ^ 1u];
  b->hsel ^= 1u;
  b->resume = b->D.stream != 0;
  HIPCHK(hipMemcpyAsync(b->D.remaining, b->h_ctl0, 2 * sizeof(uint32_t), hipMemcpyHostToDevice,
                        b->stream));
  HIPCHK(hipEventRecord(b->ev0, b->stream));
  HIPCHK(launch_step(b->D, b->D.scenario, budget, b->stream));
  HIPCHK(hipEventRecord(b->ev1, b->stream));
  HIPCHK(hipMemcpyAsync(b->h_remaining, b->D.remaining, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost,
                        b->stream));
  return 0;
}

// clusters of the launched chunk without a verdict: those the lanes held, plus (streaming)
// those never claimed
static uint64_t remaining_after(const mr_batch* b) {
  const uint32_t next = b->h_remaining[1];
  return (uint64_t)b->h_remaining[0] + (b->D.stream && next < b->D.C ? b->D.C - next : 0u);
}

// MR_GUARD builds: the run fails with the first out-of-range index its launches recorded
static int guard_check(mr_batch* b) {
#if MR_GUARD
  uint32_t g[4];
  HIPCHK(hipMemcpy(g, b->D.guard, sizeof g, hipMemcpyDeviceToHost));
  if (g[0])
    return set_err("MR_GUARD: index " + std::to_string(g[2]) + " out of range " + std::to_string(g[3]) +
                   " (tag " + std::to_string(g[0]) + ", cluster " + std::to_string(g[1]) + ")");
#else
  (void)b;
#endif
  return 0;
}

int mr_batch_reset(mr_batch* b, uint64_t seed_base) {
  if (!b) return set_err("null batch");
  if (b->submitted) return set_err("batch has a submitted step: mr_batch_finish it first");
  if (enqueue_reset(b, seed_base) != 0) return -1;
  HIPCHK(hipStreamSynchronize(b->stream));
  return 0;
}

int mr_batch_run(mr_batch* b, uint64_t max_events_per_call, mr_run_stats* st) {
  if (!b) return set_err("null batch");
  if (b->submitted) return set_err("batch has a submitted step: mr_batch_finish it first");
  HIPCHK(hipSetDevice(b->cfg.device));
  auto t0 = std::chrono::steady_clock::now();
  mr_run_stats s;
  std::memset(&s, 0, sizeof s);
  uint64_t done_events = 0;
  bool stop = false;
  // chunks of D.L clusters, one after another (a streaming batch is one chunk of all clusters);
  // a call cut short by max_events_per_call resumes with the chunk it stopped in
  const uint32_t chunk = b->D.stream ? b->D.C : b->D.L;
  for (uint32_t c0 = b->c_open; c0 < b->D.C && !stop; c0 += chunk) {
    b->D.c0 = c0;
    for (;;) {
      uint32_t budget = b->budget;
      if (max_events_per_call) {
        if (done_events >= max_events_per_call) { stop = true; break; }
        uint64_t left = max_events_per_call - done_events;
        if (left < budget) budget = (uint32_t)left;
      }
      if (enqueue_step(b, budget) != 0) { b->D.c0 = 0; return -1; }
      HIPCHK(hipStreamSynchronize(b->stream));
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
      s.kernel_ms += ms;
      s.launches++;
      done_events += budget;
      if (remaining_after(b) == 0) {
        b->c_open = c0 + chunk;
        break;
      }
    }
  }
  b->D.c0 = 0;
  if (guard_check(b) != 0) return -1;
  s.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  // events processed and clusters left: sums over the per-cluster counters (cheap reduce)
  mr_counters c;
  if (mr_batch_counters(b, &c) != 0) return -1;
  s.events = c.events;
  s.remaining = c.clusters - c.done;
  if (st) *st = s;
  return 0;
}

// Pipelined steps (bench.py): reset + the first step-kernel launch are only
// enqueued, so the host can queue the next batch's step on its own stream and
// that batch's waves take the CUs this batch's early-finishing waves free.
int mr_batch_submit(mr_batch* b, uint64_t seed_base) {
  if (!b) return set_err("null batch");
  if (b->submitted) return set_err("batch already has a submitted step");
  b->t_submit = std::chrono::steady_clock::now();
  if (enqueue_reset(b, seed_base) != 0) return -1;
  if (enqueue_step(b, b->budget) != 0) return -1;
  b->submitted = true;
  return 0;
}

int mr_batch_finish(mr_batch* b, mr_run_stats* st, mr_counters* cnt) {
  if (!b) return set_err("null batch");
  if (!b->submitted) return set_err("no submitted step");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  b->submitted = false;
  mr_run_stats s;
  std::memset(&s, 0, sizeof s);
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, b->ev0, b->ev1));
  s.kernel_ms = ms;
  s.launches = 1;
  s.remaining = remaining_after(b);
  if (s.remaining == 0) b->c_open = b->D.stream ? b->D.C : b->D.L;  // the submitted chunk is done
  if (b->c_open < b->D.C) s.remaining = 1;  // later chunks: run them below
  if (s.remaining != 0) {  // clusters past the per-launch budget: finish them synchronously
    mr_run_stats more;
    if (mr_batch_run(b, 0, &more) != 0) return -1;
    s.kernel_ms += more.kernel_ms;
    s.launches += more.launches;
    s.remaining = more.remaining;
  }
  if (guard_check(b) != 0) return -1;  // (mr_batch_run above checked its own launches)
  mr_counters c;
  if (mr_batch_counters(b, &c) != 0) return -1;
  s.events = c.events;
  s.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() -
                                                        b->t_submit).count();
  if (st) *st = s;
  if (cnt) *cnt = c;
  return 0;
}

static int mr_batch_verdicts_impl(mr_batch* b, uint16_t* code, uint32_t* time_us, uint64_t* digest) {
  if (!b) return set_err("null batch");
  HIPCHK(hipSetDevice(b->cfg.device));
  size_t C = b->D.C;
  std::vector<uint32_t> c32;
  // one field of every cluster: a strided row (cluster-major records) or a contiguous one
  auto row = [&](void* dst, const void* base, size_t f, size_t width, bool wide) -> hipError_t {
    const char* p = static_cast<const char*>(base) + (wide ? C64_IDX(f, 0, C) : CS_IDX(f, 0, C)) * width;
    const size_t pitch = (wide ? C64_IDX(f, 1, C) - C64_IDX(f, 0, C) : CS_IDX(f, 1, C) - CS_IDX(f, 0, C)) * width;
    return hipMemcpy2DAsync(dst, width, p, pitch, width, C, hipMemcpyDeviceToHost, b->stream);
  };
  if (code) {
    c32.resize(C);
    HIPCHK(row(c32.data(), b->D.cs32, CS_CODE, 4, false));
  }
  if (time_us) HIPCHK(row(time_us, b->D.cs32, CS_VTIME, 4, false));
  if (digest) HIPCHK(row(digest, b->D.cs64, C64_DIGEST, 8, true));
  HIPCHK(hipStreamSynchronize(b->stream));
  for (size_t i = 0; i < c32.size(); i++) code[i] = (uint16_t)c32[i];
  return 0;
}

int mr_batch_counters(mr_batch* b, mr_counters* out) {
  if (!b || !out) return set_err("null argument");
  HIPCHK(hipSetDevice(b->cfg.device));
  std::vector<unsigned long long> h(RED_N, 0);
  h[RED_FIRST_FAIL] = ~0ull;
  HIPCHK(hipMemcpyAsync(b->red, h.data(), RED_N * 8, hipMemcpyHostToDevice, b->stream));
  HIPCHK(launch_reduce(b->D, b->red, b->cfg.cluster_base, b->stream));
  HIPCHK(hipMemcpyAsync(h.data(), b->red, RED_N * 8, hipMemcpyDeviceToHost, b->stream));
  HIPCHK(hipStreamSynchronize(b->stream));
  std::memset(out, 0, sizeof *out);
  out->clusters = b->D.C;
#define MR_ROW_(sym, field, red, who) out->field = h[CNT_##sym];
  MR_COUNTER_TABLE(MR_ROW_)
#undef MR_ROW_
  out->events = h[RED_EVENTS]; out->msgs_sent = h[RED_MSGS]; out->virt_time_us = h[RED_VTIME];
  out->done = h[RED_DONE]; out->passed = h[RED_PASSED]; out->failed = out->done - out->passed;
  out->first_fail_cluster = h[RED_FIRST_FAIL];
  for (int i = 0; i < 64; i++) out->fail_hist[i] = h[RED_FAIL_HIST + i];
  for (int i = 0; i < 16; i++) {
    out->cov_leaders[i] = h[RED_COV_LEADERS + i];
    out->cov_events[i] = h[RED_COV_EVENTS + i];
  }
  out->kv_ops = h[RED_KV_OPS];
  out->kv_checked = h[RED_KV_CHECKED];
  out->kv_lin_checked = h[RED_KV_LIN];
  out->first_fail_code = 0;
  if (out->first_fail_cluster != ~0ull) {
    uint32_t code = 0;
    size_t idx = out->first_fail_cluster - b->cfg.cluster_base;
    HIPCHK(hipMemcpy(&code, b->D.cs32 + CS_IDX(CS_CODE, idx, b->D.C), 4, hipMemcpyDeviceToHost));
    out->first_fail_code = code;
  }
  return 0;
}

int mr_trace_get(mr_batch* b, uint32_t k, mr_event* out, size_t cap, size_t* n) {
  if (!b || !out || !n) return set_err("null argument");
  if (k >= b->D.trace_clusters) return set_err("cluster not traced");
  HIPCHK(hipSetDevice(b->cfg.device));
  return copy_trace_row(b, k, b->D.trace, out, cap, n);
}

int mr_trace_digests(mr_batch* b, uint32_t k, uint64_t* out, size_t cap, size_t* n) {
  if (!b || !out || !n) return set_err("null argument");
  if (k >= b->D.trace_clusters) return set_err("cluster not traced");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  return copy_trace_row(b, k, b->D.tdig, out, cap, n);
}

int mr_trace_applies(mr_batch* b, uint32_t k, uint64_t* out, size_t cap, size_t* n) {
  if (!b || !out || !n) return set_err("null argument");
  if (k >= b->D.trace_clusters) return set_err("cluster not traced");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  size_t m = cap < b->D.trace_cap ? cap : b->D.trace_cap;
  HIPCHK(hipMemcpy(out, b->D.tapp + (size_t)k * b->D.trace_cap * 2u, m * 2u * sizeof(uint64_t),
                   hipMemcpyDeviceToHost));
  while (m && !out[2 * (m - 1)]) m--;
  *n = m;
  return 0;
}

const char* mr_batch_kernel(const mr_batch* b) {
  if (!b) return "";
  return b->D.tape_mode ? "step_kernel_tape" : b->D.pool ? "pool_kernel" : "step_kernel";
}

uint32_t mr_decision_word(uint32_t v, uint32_t lo, uint32_t hi) {
  if (hi <= lo || v < lo || v >= hi) return 0;
  // ceil((v - lo) * 2^32 / (hi - lo)): the first w whose range image is v
  const uint64_t span = hi - lo, num = (uint64_t)(v - lo) << 32;
  return (uint32_t)((num + span - 1) / span);
}

// the batch's decision tables (whoever installed them) freed; Philox draws
static void drop_decisions(mr_batch* b) { install_tables(b, Tables{}); }

// `t`, staged by a chain of upload()s that ended with `e`: installed, or on an error freed, the
// batch keeping its previous tables (`what` names them in the message)
static int install_staged(mr_batch* b, Tables& t, hipError_t e, const char* what) {
  if (e != hipSuccess) {
    free_tables(t);
    return set_err(std::string(what) + ": " + hipGetErrorString(e));
  }
  install_tables(b, t);
  return 0;
}

// (a variant batch's messages name the group only where there are groups)
static std::string in_group(bool many, size_t g) {
  return many ? " (group " + std::to_string(g) + ")" : std::string();
}

// The lookup tables of mr_batch_set_decisions, mr_batch_set_variants and mr_batch_set_variant_groups:
// the groups' base tapes base[base_off .. +n_base) one after the other, each slice packed, sorted
// once and checked for duplicate keys, and one 16-B descriptor per cluster copied from its group.
// Replay (`who` = OWN_REPLAY) is a variant batch of C one-cluster groups without edits: cluster c is
// in group c, and no edit array exists. A variant batch's cluster c is in group group_of[c] (null:
// group 0); it has each base record's edit index within its group beside it, the edits' words in
// group order, and one mask row per cluster. The groups' ranges are the caller's to check.
// Validated and staged whole before the previous tables are dropped, so a rejected call leaves the
// batch as it was.
static int stage_slices(mr_batch* b, Owner who, const mr_variant_group* groups, size_t n_groups,
                        const mr_decision* base, const mr_decision* edits, const uint32_t* group_of,
                        const uint32_t* masks) {
  const size_t C = b->D.C;
  const bool replay = who == OWN_REPLAY, many = !replay && group_of != nullptr;
  size_t rows = 0, words = 0, widest = 0;
  for (size_t g = 0; g < n_groups; g++) {
    rows += groups[g].n_base;
    words += groups[g].n_edits;
    if (groups[g].n_edits > widest) widest = groups[g].n_edits;
  }
  if (rows >= (1ull << 32) || words >= (1ull << 32))
    return set_err("too many decisions for one batch (2^32 - 1 at most)");
  auto key_of = [](const mr_decision& r) { return make_uint2(((uint32_t)r.stream << 16) | r.entity, r.seq); };
  auto bad_stream = [](const mr_decision& r) { return r.stream < MR_DS_TESTER || r.stream > MR_DS_NET; };
  auto lt = [](const uint4& a, const uint4& c) { return a.x < c.x || (a.x == c.x && a.y < c.y); };
  std::vector<uint4> tab(rows), desc(n_groups);
  std::vector<uint32_t> ved(replay ? 0 : rows, ~0u);
  std::vector<uint2> vw(words);
  size_t r0 = 0, w0 = 0;  // the group's first row of tab / ved, its first edit of vw
  for (size_t g = 0; g < n_groups; g++) {
    const mr_variant_group& G = groups[g];
    uint4* row = tab.data() + r0;
    for (size_t i = 0; i < G.n_base; i++) {
      const mr_decision& r = base[G.base_off + i];
      if (bad_stream(r)) return set_err("bad decision stream" + in_group(many, g));
      const uint2 k = key_of(r);
      row[i] = make_uint4(k.x, k.y, r.w0, r.w1);
    }
    std::sort(row, row + G.n_base, lt);
    for (size_t k = 1; k < G.n_base; k++)
      if (row[k].x == row[k - 1].x && row[k].y == row[k - 1].y)
        return set_err(replay ? "duplicate decision key (cluster " + std::to_string(g) + ")"
                              : "duplicate decision key in the base tape" + in_group(many, g));
    for (size_t j = 0; j < G.n_edits; j++) {
      const mr_decision& r = edits[G.edit_off + j];
      if (bad_stream(r)) return set_err("bad decision stream (edit " + std::to_string(j) + ")" + in_group(many, g));
      const uint2 k = key_of(r);
      const uint4* it = std::lower_bound(row, row + G.n_base, make_uint4(k.x, k.y, 0, 0), lt);
      if (it == row + G.n_base || it->x != k.x || it->y != k.y)
        return set_err("edit " + std::to_string(j) + ": its key is not in the base tape" + in_group(many, g));
      uint32_t& e = ved[r0 + (it - row)];
      if (e != ~0u)
        return set_err("duplicate edit key (edits " + std::to_string(e) + " and " + std::to_string(j) + ")" +
                       in_group(many, g));
      e = (uint32_t)j;
      vw[w0 + j] = make_uint2(r.w0, r.w1);
    }
    desc[g] = make_uint4((uint32_t)r0, G.n_base, (uint32_t)w0, G.seed_cluster);
    r0 += G.n_base;
    w0 += G.n_edits;
  }
  std::vector<uint4> cdesc(C);
  for (size_t c = 0; c < C; c++) cdesc[c] = desc[replay ? c : many ? group_of[c] : 0];
  const size_t W = (widest + 31) / 32;
  Tables t;
  t.vW = (uint32_t)W;
  t.mode = who;
  hipError_t e = upload(&t.tape, tab.data(), rows);
  if (e == hipSuccess) e = upload(&t.tdesc, cdesc.data(), C);
  if (!replay) {  // (null in a replay: no record has an edit)
    if (e == hipSuccess) e = upload(&t.vedit, ved.data(), rows);
    if (e == hipSuccess) e = upload(&t.vwords, vw.data(), words);
    if (e == hipSuccess) e = upload(&t.vmask, masks, C * W);
  }
  return install_staged(b, t, e, replay ? "decision table" : "variant tables");
}

// Keyed decisions in any order: a counting sort by cluster makes cluster c's records the base tape
// of group c, whose seed_cluster is c and which has no edits (a row may be empty: every draw of
// that cluster misses). The table is O(n + C) whatever the longest row.
static int set_decisions_impl(mr_batch* b, const mr_decision* d, size_t n) {
  const size_t C = b->D.C;
  if (n >= (1ull << 32)) return set_err("too many decisions for one batch (2^32 - 1 at most)");
  std::vector<mr_variant_group> rows(C);  // (value-initialised: zeros)
  for (size_t i = 0; i < n; i++) {
    if (d[i].cluster >= C) return set_err("decision for a cluster outside the batch");
    rows[d[i].cluster].n_base++;
  }
  uint32_t at = 0;
  for (size_t c = 0; c < C; c++) {  // (n_base counts again below, as the row's fill)
    rows[c].seed_cluster = (uint32_t)c;
    rows[c].base_off = at;
    at += rows[c].n_base;
    rows[c].n_base = 0;
  }
  std::vector<mr_decision> tab(n);
  for (size_t i = 0; i < n; i++) {
    mr_variant_group& G = rows[d[i].cluster];
    tab[G.base_off + G.n_base++] = d[i];
  }
  return stage_slices(b, OWN_REPLAY, rows.data(), C, tab.data(), nullptr, nullptr, nullptr);
}

int mr_batch_set_decisions(mr_batch* b, const mr_decision* d, size_t n) {
  if (!b) return set_err("null batch");
  if (n && !d) return set_err("null decisions");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (!n) { drop_decisions(b); return 0; }
  return no_throw("decision table", [&] { return set_decisions_impl(b, d, n); });  // host staging
}

// A variant batch (madraft_sim.h mr_batch_set_variant_groups; mr_batch_set_variants is its
// one-group case, group_of == nullptr = every cluster in group 0): what a variant's entry points
// ask of their ranges, then stage_slices
static int set_variants_impl(mr_batch* b, const mr_variant_group* groups, size_t n_groups,
                             const mr_decision* base, size_t n, const mr_decision* edits,
                             size_t n_edits, const uint32_t* group_of, const uint32_t* masks) {
  if (n >= (1ull << 32) || n_edits >= (1ull << 32) || n_groups >= (1ull << 32))
    return set_err("too many decisions for one batch (2^32 - 1 at most)");
  const bool many = group_of != nullptr;
  for (size_t g = 0; g < n_groups; g++) {
    const mr_variant_group& G = groups[g];
    if (G.n_base == 0) return set_err("a variant group needs a base tape, n_base >= 1" + in_group(many, g));
    if ((uint64_t)G.base_off + G.n_base > n) return set_err("base range overruns n" + in_group(many, g));
    if ((uint64_t)G.edit_off + G.n_edits > n_edits)
      return set_err("edit range overruns n_edits" + in_group(many, g));
  }
  if (many)
    for (size_t c = 0; c < b->D.C; c++)
      if (group_of[c] >= n_groups)
        return set_err("group_of[" + std::to_string(c) + "] = " + std::to_string(group_of[c]) +
                       ": no such group");
  return stage_slices(b, OWN_VARIANTS, groups, n_groups, base, edits, group_of, masks);
}

// what the two variant calls share before their tables are looked at; 1 = go on
static int variants_enter(mr_batch* b, bool drop) {
  if (!b) return set_err("null batch");
  if (b->cfg.flags & MR_F_RECORD) return set_err("variants on a MR_F_RECORD batch");
  if (!drop && b->sof) return set_err("variants on a batch with a seed list (mr_batch_set_seeds)");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  if (!drop) return 1;
  if (b->dec.mode == OWN_VARIANTS) drop_decisions(b);  // (another kind of table is not a variant's to drop)
  return 0;
}

int mr_batch_set_variants(mr_batch* b, const mr_decision* base, size_t n, const mr_decision* edits,
                          size_t n_edits, const uint32_t* masks) {
  if (n && !base) return set_err("null decisions");
  if (n && n_edits && !edits) return set_err("null edits");
  if (n >= (1ull << 32) || n_edits >= (1ull << 32))
    return set_err("too many decisions for one batch (2^32 - 1 at most)");
  if (const int rc = variants_enter(b, n == 0); rc <= 0) return rc;
  const mr_variant_group one{0u, 0u, (uint32_t)n, 0u, (uint32_t)n_edits};
  return no_throw("variant tables",
                  [&] { return set_variants_impl(b, &one, 1, base, n, edits, n_edits, nullptr, masks); });
}

int mr_batch_set_variant_groups(mr_batch* b, const mr_variant_group* groups, size_t n_groups,
                                const mr_decision* base, size_t n, const mr_decision* edits,
                                size_t n_edits, const uint32_t* group_of, const uint32_t* masks) {
  if (n_groups && (!groups || !group_of)) return set_err("null groups");
  if (n_groups && n && !base) return set_err("null decisions");
  if (n_groups && n_edits && !edits) return set_err("null edits");
  if (const int rc = variants_enter(b, n_groups == 0); rc <= 0) return rc;
  return no_throw("variant tables", [&] {
    return set_variants_impl(b, groups, n_groups, base, n, edits, n_edits, group_of, masks);
  });
}

int mr_batch_set_variant_masks(mr_batch* b, const uint32_t* masks) {
  if (!b) return set_err("null batch");
  if (b->dec.mode != OWN_VARIANTS) return set_err("mr_batch_set_variant_masks without variants");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  const size_t mw = (size_t)b->D.C * b->D.vW;
  if (!mw) return 0;
  if (masks) HIPCHK(hipMemcpy(b->dec.vmask, masks, mw * sizeof(uint32_t), hipMemcpyHostToDevice));
  else HIPCHK(hipMemset(b->dec.vmask, 0, mw * sizeof(uint32_t)));
  return 0;
}

static int mr_batch_get_decisions_impl(mr_batch* b, uint32_t k, mr_decision* out, size_t cap, size_t* n) {
  if (!b || !n) return set_err("null argument");
  if (k >= b->D.C) return set_err("cluster out of range");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  uint32_t used = 0;
  HIPCHK(hipMemcpy(&used, b->D.cs32 + CS_IDX(CS_TAPE, k, b->D.C), 4, hipMemcpyDeviceToHost));
  *n = used;
  if (b->D.tape_mode != TAPE_RECORD || !out) return 0;
  size_t m = used < b->D.dcap ? used : b->D.dcap;
  if (m > cap) m = cap;
  std::vector<uint4> rows(m);
  if (m)
    HIPCHK(hipMemcpy(rows.data(), b->dec.tape + (size_t)k * b->D.dcap, m * sizeof(uint4),
                     hipMemcpyDeviceToHost));
  for (size_t i = 0; i < m; i++)
    out[i] = mr_decision{k, (uint16_t)(rows[i].x >> 16), (uint16_t)(rows[i].x & 0xFFFFu), rows[i].y,
                         rows[i].z, rows[i].w};
  return 0;
}

// The recorded tapes of clusters [first, first + count): one copy of the CS_TAPE row slice (the row is
// cluster-minor, so the slice is contiguous), a scan on the host, one tape_pack_kernel launch into a
// scratch buffer that starts with the offsets, one copy back. The host touches no record.
static int get_decisions_packed_impl(mr_batch* b, uint32_t first, uint32_t count, uint64_t* drawn,
                                     uint64_t* off, mr_decision* out, size_t cap) {
  if (!b || !off) return set_err("null argument");
  if ((uint64_t)first + count > b->D.C) return set_err("clusters out of range");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  const uint32_t* used_d = b->D.cs32 + CS_IDX(CS_TAPE, first, b->D.C);
  std::vector<uint32_t> used(count);
  if (count) HIPCHK(hipMemcpy(used.data(), used_d, (size_t)count * 4, hipMemcpyDeviceToHost));
  const bool rec = b->D.tape_mode == TAPE_RECORD;  // (with decisions set the counts are misses: no records)
  off[0] = 0;
  for (size_t i = 0; i < count; i++) {
    if (drawn) drawn[i] = used[i];
    off[i + 1] = off[i] + (rec ? std::min(used[i], b->D.dcap) : 0u);
  }
  const uint64_t total = off[count];
  if (!out || !total) return 0;
  if (cap < total)
    return set_err("mr_batch_get_decisions_packed: out holds " + std::to_string(cap) + " records, " +
                   std::to_string(total) + " are kept");
  const size_t head = ((size_t)(count + 1) * sizeof(uint64_t) + 255) & ~size_t(255);
  char* scratch = nullptr;
  HIPCHK(hipMalloc(&scratch, head + total * sizeof(mr_decision)));
  hipError_t e = hipMemcpyAsync(scratch, off, (size_t)(count + 1) * sizeof(uint64_t),
                                hipMemcpyHostToDevice, b->stream);
  if (e == hipSuccess)
    e = launch_tape_pack(b->dec.tape, used_d, b->D.dcap, first, count,
                         reinterpret_cast<const uint64_t*>(scratch),
                         reinterpret_cast<uint32_t*>(scratch + head), b->stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(out, scratch + head, total * sizeof(mr_decision), hipMemcpyDeviceToHost, b->stream);
  if (e == hipSuccess) e = hipStreamSynchronize(b->stream);
  (void)hipFree(scratch);
  if (e != hipSuccess) return set_err(std::string("tape pack: ") + hipGetErrorString(e));
  return 0;
}

static int mr_replay_impl(const mr_cfg* cfg, const mr_decision* d, size_t n, mr_event* out, size_t cap,
              size_t* n_out, uint16_t* code, uint32_t* time_us, uint64_t* misses) {
  if (!cfg || !n_out) return set_err("null argument");
  if (n && !d) return set_err("null decisions");
  mr_cfg c = *cfg;
  c.n_clusters = 1;
  c.flags = (c.flags | MR_F_TRACE) & ~MR_F_RECORD;
  c.trace_clusters = 1;
  c.trace_cap = cap ? (uint32_t)cap : 1u;
  mr_batch* b = nullptr;
  int rc = mr_batch_create(&c, &b);
  if (rc) return rc;
  std::vector<mr_decision> one(d, d + n);
  for (auto& r : one) r.cluster = 0;
  // keyed replay runs the MR_TAPE kernels even for an empty trace (every draw then misses)
  const mr_decision none{0, MR_DS_TESTER, 0xFFFFu, 0xFFFFFFFFu, 0u, 0u};
  if (one.empty()) one.push_back(none);
  rc = mr_batch_set_decisions(b, one.data(), one.size());
  mr_run_stats st;
  if (!rc) rc = mr_batch_run(b, 0, &st);
  uint16_t cd = 0;
  uint32_t t = 0;
  if (!rc) rc = mr_batch_verdicts(b, &cd, &t, nullptr);
  if (!rc && out && cap) rc = mr_trace_get(b, 0, out, cap, n_out);
  else if (!rc) *n_out = 0;
  size_t ms = 0;
  if (!rc && misses) rc = mr_batch_get_decisions(b, 0, nullptr, 0, &ms);
  if (!rc && misses) *misses = ms;
  if (!rc && code) *code = cd;
  if (!rc && time_us) *time_us = t;
  mr_batch_destroy(b);
  return rc;
}

void mr_batch_destroy(mr_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->cfg.device);
  if (b->stream) (void)hipStreamSynchronize(b->stream);
#ifdef MR_PROF
  if (b->base) {  // development profile: wave cycles per kernel section (mr_kernel.hip PROF_*)
    unsigned long long h[PROF_SLOTS];
    if (hipMemcpy(h, b->D.prof, sizeof h, hipMemcpyDeviceToHost) == hipSuccess) {
      std::fprintf(stderr, "MRPROF");
      for (uint32_t k = 0; k < PROF_SLOTS; k++) std::fprintf(stderr, " %llu", h[k]);
      std::fprintf(stderr, "\n");
    }
  }
#endif
  if (b->base) (void)hipFree(b->base);
  free_tables(b->dec);
  // the seed list and the streaming held-cluster lists belong to the batch, not to its decision tables
  if (b->sof) (void)hipFree(b->sof);
  for (uint32_t h = 0; h < 2; h++)
    if (b->held[h]) { (void)hipFree(b->held[h]); b->held[h] = nullptr; }
  if (b->red) (void)hipFree(b->red);
  if (b->h_remaining) (void)hipHostFree(b->h_remaining);
  if (b->h_ctl0) (void)hipHostFree(b->h_ctl0);
  if (b->ev0) (void)hipEventDestroy(b->ev0);
  if (b->ev1) (void)hipEventDestroy(b->ev1);
  if (b->stream) (void)hipStreamDestroy(b->stream);
  delete b;
}

int mr_batch_create(const mr_cfg* cfg, mr_batch** out) {
  return no_throw("mr_batch_create", [&] { return mr_batch_create_impl(cfg, out); });
}

int mr_batch_verdicts(mr_batch* b, uint16_t* code, uint32_t* time_us, uint64_t* digest) {
  return no_throw("mr_batch_verdicts", [&] { return mr_batch_verdicts_impl(b, code, time_us, digest); });
}

int mr_batch_get_decisions(mr_batch* b, uint32_t k, mr_decision* out, size_t cap, size_t* n) {
  return no_throw("mr_batch_get_decisions",
                  [&] { return mr_batch_get_decisions_impl(b, k, out, cap, n); });
}

int mr_batch_get_decisions_packed(mr_batch* b, uint32_t first, uint32_t count, uint64_t* drawn,
                                  uint64_t* off, mr_decision* out, size_t cap) {
  return no_throw("mr_batch_get_decisions_packed",
                  [&] { return get_decisions_packed_impl(b, first, count, drawn, off, out, cap); });
}

// The batch's seed list: uploaded whole before the previous one is freed; the tables stay, and with
// them what a draw does (a list alone: TAPE_SEEDS; dropped without tables: the batch's pool / step kernel again)
int mr_batch_set_seeds(mr_batch* b, const uint32_t* seed_cluster) {
  if (!b) return set_err("null batch");
  if (b->submitted) return set_err("batch has a submitted step: mr_batch_finish it first");
  if (seed_cluster && b->dec.mode == OWN_VARIANTS)
    return set_err("a seed list on a batch with variants set");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream));
  uint32_t* list = nullptr;
  if (seed_cluster) {
    const hipError_t e = upload(&list, seed_cluster, (size_t)b->D.C);
    if (e != hipSuccess) {
      if (list) (void)hipFree(list);
      return set_err(std::string("seed list: ") + hipGetErrorString(e));
    }
  }
  if (b->sof) (void)hipFree(b->sof);
  b->sof = list;
  b->D.sof = list;
  b->D.tape_mode = tape_mode_of(b);
  return 0;
}

int mr_replay(const mr_cfg* cfg, const mr_decision* d, size_t n, mr_event* out, size_t cap,
              size_t* n_out, uint16_t* code, uint32_t* time_us, uint64_t* misses) {
  return no_throw("mr_replay", [&] {
    return mr_replay_impl(cfg, d, n, out, cap, n_out, code, time_us, misses);
  });
}

}  // extern "C"
