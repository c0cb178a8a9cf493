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
#include <memory>
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
hipError_t launch_group_reduce(const Dev& D, const uint32_t* gof, uint32_t n_groups,
                               unsigned long long* out, uint64_t cluster_base, hipStream_t s);
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

// Move-only owners of the HIP handles a batch keeps, one per kind: released with their holder
template <auto Release>
struct Releaser {
  template <class P> void operator()(P p) const { (void)Release(p); }
};
template <class T> using DevMem = std::unique_ptr<T[], Releaser<hipFree>>;      // device memory
template <class T> using PinMem = std::unique_ptr<T[], Releaser<hipHostFree>>;  // pinned host memory
using Stream = std::unique_ptr<ihipStream_t, Releaser<hipStreamDestroy>>;
using Event = std::unique_ptr<ihipEvent_t, Releaser<hipEventDestroy>>;

// own = the handle `make(&raw)` creates (null where that fails)
template <class Own, class Make>
hipError_t acquire(Own& own, Make make) {
  typename Own::pointer p = nullptr;
  const hipError_t e = make(&p);
  own.reset(p);
  return e;
}
// m = a new device array of `count` elements
template <class T>
hipError_t dev_alloc(DevMem<T>& m, size_t count) {
  return acquire(m, [&](T** p) { return hipMalloc(p, count * sizeof(T)); });
}

// dst = a new device array of max(count, 1) elements: src[0 .. count), or zeros for a null src
template <class T>
hipError_t upload(DevMem<T>& dst, const T* src, size_t count) {
  const hipError_t e = dev_alloc(dst, count ? count : 1);
  if (e != hipSuccess || !count) return e;
  return src ? hipMemcpy(dst.get(), src, count * sizeof(T), hipMemcpyHostToDevice)
             : hipMemset(dst.get(), 0, count * sizeof(T));
}

// A batch's decision tables on the device, each its own allocation, whoever made them: the record
// tape (MR_F_RECORD), or what stage_slices built, the sorted slices and the clusters' descriptors
// of a replay, and with them a variant batch's edits and masks. All null: Philox draws.
struct Tables {
  DevMem<uint4> tape;         // keyed decisions: the record tape, or the groups' sorted slices
  DevMem<uint4> tdesc;        // slices: the clusters' group descriptors;
  DevMem<uint32_t> vedit;     // variants: the base records' edit indices within their group,
  DevMem<uint2> vwords;       // the edits' words,
  DevMem<uint32_t> vmask;     // and the clusters' mask rows (set_variant_masks rewrites them)
  uint32_t dcap = 0, vW = 0;  // Dev's dcap and vW with these tables
  Owner mode = OWN_NONE;
};

// A batch's parameter groups on the device (mr_batch_set_param_groups), each array its own
// allocation, staged whole and moved in as one. All null: every cluster runs the batch's cfg.
struct ParamGroups {
  DevMem<uint32_t> rec;             // [C][PG_W] the clusters' parameter records (Dev::pgrp)
  DevMem<uint32_t> gof;             // [C] the clusters' groups, for the grouped reduce
  DevMem<unsigned long long> red;   // [n][RED_N] the groups' reduce rows (group_reduce_kernel)
  std::vector<uint64_t> positions;  // [n] clusters of each group
  bool fresh = false;               // red holds the reduce of the clusters as they stand
  size_t n() const { return positions.size(); }
};

// the HBM format of a run's message keys: the pool kernel's (32-bit, AppendEntries bit), or the one
// the step and tape kernels share
enum KeyFormat : uint32_t { KEYS_UNSET, KEYS_POOL, KEYS_STEP };

// Where a batch's run stands: a reset starts it over, enqueue_step and the launch loop (advance)
// move it on
struct RunState {
  uint32_t c_open = 0;         // first cluster of the first chunk not yet finished
  bool resume = false;         // streaming: the next launch continues the current chunk
  KeyFormat keys = KEYS_UNSET; // of the launches since the reset
  bool submitted = false;      // mr_batch_submit enqueued a step not yet waited for
  std::chrono::steady_clock::time_point t_submit;
};
}  // namespace

struct mr_batch {
  Stream stream;  // (first: released last, after the events and the memory its work used)
  Event ev0, ev1;
  mr_cfg cfg;
  Dev D;  // the kernels' view: raw pointers into what the owners below hold
  DevMem<char> base;
  DevLayout lay;  // where `base` holds D's arrays, and what a reset zeroes
  DevMem<unsigned long long> red;
  PinMem<uint32_t> h_remaining;  // [2]: remaining, next unclaimed cluster (D.remaining)
  PinMem<uint32_t> h_ctl0;       // [2]: {0, L}, copied to D.remaining before each launch
  DevMem<uint32_t> held[2];      // streaming: clusters held at a launch's end (ping-pong)
  uint32_t hsel = 0;             // held[hsel] = the next launch's held_in
  uint32_t budget = 16384;       // events per cluster per launch (MR_STEP_BUDGET)
  Tables dec;                    // the decision tables D draws from (install_tables)
  DevMem<uint32_t> sof;          // the seed list (mr_batch_set_seeds): the batch's, not its tables'
  ParamGroups pg;                // the parameter groups (mr_batch_set_param_groups): the batch's too
  RunState run;
  bool fork_timed = false;  // ev0 / ev1 bracket a fork_kernel: no reset or step since (mr_batch_fork_ms)
};
struct BatchDestroy {
  void operator()(mr_batch* b) const { mr_batch_destroy(b); }
};
using Batch = std::unique_ptr<mr_batch, BatchDestroy>;

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

// Dev's tape_mode: what a draw does with the owner's tables, or without tables on a batch that
// needs the tape kernels all the same: for a seed list, or for parameter groups (TAPE_SEEDS with a
// null list is Philox from the cluster's own seed)
static TapeMode tape_mode_of(const mr_batch* b) {
  if (b->dec.mode == OWN_RECORD) return TAPE_RECORD;
  return b->dec.mode != OWN_NONE ? TAPE_LOOKUP : b->sof || b->pg.rec ? TAPE_SEEDS : TAPE_OFF;
}

// `t` (staged whole by the caller) becomes the batch's decision tables, the previous ones are
// freed by the move, and the kernels' view of them is published into D
static void install_tables(mr_batch* b, Tables&& t) {
  b->dec = std::move(t);
  const Tables& d = b->dec;
  Dev& D = b->D;
  D.dtab = d.tape.get(); D.dcap = d.dcap;
  D.tdesc = d.tdesc.get(); D.vedit = d.vedit.get(); D.vwords = d.vwords.get();
  D.vmask = d.vmask.get(); D.vW = d.vW;
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

static int group_reduce(mr_batch* b);
static int fill_counters(mr_batch* b, const unsigned long long* h, uint64_t clusters, mr_counters* out);

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
  const uint64_t C = cfg->n_clusters, n = cfg->n_nodes, M = cfg->msg_slots;
  // field matrices use 32-bit element offsets in the kernels
  const uint64_t lim = 1ull << 32;
  if ((uint64_t)CS_STRIDE * C >= lim || (uint64_t)C64_STRIDE * C >= lim || M * C >= lim)
    return set_err("n_clusters too large for one batch (32-bit field offsets)");

  Batch b(new mr_batch());  // (every exit below releases what the batch holds by then)
  b->cfg = *cfg;
  Dev& D = b->D;
  std::memset(&D, 0, sizeof D);
  const uint64_t per_chunk = cfg->lanes && cfg->lanes < C ? cfg->lanes : C;  // clusters, as configured
  D.C = (uint32_t)C;
  D.L = (uint32_t)per_chunk;  // no tape: capacity (below)
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

  b->lay = dev_layout(*cfg);  // one allocation; every array 256-B aligned (mr_dev.h MR_DEV_ARRAYS)
  hipError_t e = hipSetDevice(cfg->device);
  if (e == hipSuccess) e = dev_alloc(b->base, b->lay.off[A__N]);
  if (e == hipSuccess) e = dev_alloc(b->red, RED_N);
  const auto pinned2 = [](uint32_t** p) { return hipHostMalloc(p, 2 * sizeof(uint32_t)); };
  const auto stream = [](hipStream_t* p) { return hipStreamCreateWithFlags(p, hipStreamNonBlocking); };
  if (e == hipSuccess) e = acquire(b->h_remaining, pinned2);
  if (e == hipSuccess) e = acquire(b->h_ctl0, pinned2);
  if (e == hipSuccess) e = acquire(b->stream, stream);
  if (e == hipSuccess) e = acquire(b->ev0, hipEventCreate);
  if (e == hipSuccess) e = acquire(b->ev1, hipEventCreate);
  if (e != hipSuccess)
    return set_err(std::string("allocation of ") + std::to_string(b->lay.off[A__N]) + " B failed: " +
                   hipGetErrorString(e));
  dev_carve(D, b->lay, b->base.get());
  if (cfg->flags & MR_F_RECORD) {
    Tables t;  // (the tape is written before it is read: not filled)
    e = dev_alloc(t.tape, (size_t)C * cfg->tape_cap);
    if (e != hipSuccess) return set_err(std::string("tape allocation failed: ") + hipGetErrorString(e));
    t.dcap = cfg->tape_cap;
    t.mode = OWN_RECORD;
    install_tables(b.get(), std::move(t));
  }
  if (hipMemset(D.prof, 0, PROF_SLOTS * sizeof(unsigned long long)) != hipSuccess ||
      hipMemset(D.guard, 0, 4 * sizeof(uint32_t)) != hipSuccess)
    return set_err("hipMemset failed");
  // lanes per wave: as configured, else 32 when the batch (or its chunk) fills at most half of
  // the resident lanes — two half-full waves per SIMD hide the latency chains better than one
  // full one — else 64
  const uint32_t cap = step_capacity(D, scn, cfg->device);  // resident lanes (64 per wave)
  D.lpw = cfg->lanes_per_wave ? cfg->lanes_per_wave : (cap && per_chunk * 2u <= cap) ? 32u : 64u;
  if (!cfg->lanes) {  // a batch bigger than the resident waves runs as chunks of that size
    const uint32_t capc = (uint32_t)((uint64_t)cap * D.lpw / STEP_LANES);
    if (capc && capc < D.C) {
      D.L = capc;
      // a pool kernel refills its slots from the rest of the batch (streaming) instead of
      // draining once per chunk (config 3's whole job on one GPU +10 %)
      if (family_of(D) == F_POOL) D.stream = 1u;
    }
  }
  if (D.stream) {  // held-cluster lists, L entries each (L <= C)
    e = dev_alloc(b->held[0], D.C);
    if (e == hipSuccess) e = dev_alloc(b->held[1], D.C);
    if (e != hipSuccess) return set_err(std::string("held-list allocation failed: ") + hipGetErrorString(e));
  }
  // the 7-server Raft pool's LDS key rows (32); MR_KEY_ROWS (tests) puts more slots' keys in HBM
  D.krows = 32u;
  if (const char* s = std::getenv("MR_KEY_ROWS")) {
    const int r = std::atoi(s);
    if (r >= 1 && r <= 32) D.krows = (uint32_t)r;
  }
  if (const char* s = std::getenv("MR_STEP_BUDGET")) b->budget = (uint32_t)std::atoi(s);
  if (b->budget == 0) b->budget = 16384;
  if (mr_batch_reset(b.get(), cfg->seed_base) != 0) return -1;  // (its message stands: a destroy sets none)
  *out = b.release();
  return 0;
}

// the key format the batch's next launch reads and writes: its kernel family's
static KeyFormat key_format_of(const Dev& D) { return family_of(D) == F_POOL ? KEYS_POOL : KEYS_STEP; }
static const char* key_format_name(KeyFormat k) {
  return k == KEYS_POOL ? "pool_kernel" : "step_kernel / step_kernel_tape";
}

static int enqueue_reset(mr_batch* b, uint64_t seed_base) {
  b->fork_timed = false;
  b->cfg.seed_base = seed_base;
  b->run = RunState{};
  b->pg.fresh = false;
  b->D.seed0 = seed_base + b->cfg.cluster_base;
  HIPCHK(hipSetDevice(b->cfg.device));
  for (int k = 0; k < (int)A__N; k++)  // the table's ZERO rows this batch has, by their place k
    for (uint32_t a = 0; a < A__N; a++)
      if (k_dev_reset[a] == k && b->lay.bytes[a])
        HIPCHK(hipMemsetAsync(b->base.get() + b->lay.off[a], 0, b->lay.bytes[a], b->stream.get()));
#if MR_GUARD
  b->D.gprobe = std::getenv("MR_GUARD_PROBE") ? 1u : 0u;
#endif
  HIPCHK(launch_reset(b->D, b->stream.get()));
  return 0;
}

// one step-kernel launch on the batch stream for the chunk that starts at cluster c0, bracketed by
// the timing events; the remaining-cluster count is copied back asynchronously
static int enqueue_step(mr_batch* b, uint32_t c0, uint32_t budget) {
  RunState& r = b->run;
  Dev& D = b->D;
  b->fork_timed = false;
  // a run does not switch key format between its launches
  const KeyFormat keys = key_format_of(D);
  if (r.keys != KEYS_UNSET && r.keys != keys)
    return set_err("decisions set or dropped in the middle of a pool-kernel run: mr_batch_reset first");
  r.keys = keys;
  D.c0 = c0;
  b->h_ctl0[0] = 0;
  if (D.stream && r.resume) {  // continue: the held clusters first, the claim pointer kept
    b->h_ctl0[1] = b->h_remaining[1];
    D.nheld = b->h_remaining[0];
    D.resume = 1;
  } else {
    b->h_ctl0[1] = c0 + D.L;  // lanes start with clusters c0 .. c0+L-1 (streaming: claim on)
    D.nheld = 0;
    D.resume = 0;
  }
  D.held_in = b->held[b->hsel].get();
  D.held_out = b->held[b->hsel ^ 1u].get();
  b->hsel ^= 1u;
  r.resume = D.stream != 0;
  hipStream_t stream = b->stream.get();
  HIPCHK(hipMemcpyAsync(D.remaining, b->h_ctl0.get(), 2 * sizeof(uint32_t), hipMemcpyHostToDevice, stream));
  HIPCHK(hipEventRecord(b->ev0.get(), stream));
  HIPCHK(launch_step(D, D.scenario, budget, stream));
  HIPCHK(hipEventRecord(b->ev1.get(), stream));
  HIPCHK(hipMemcpyAsync(b->h_remaining.get(), D.remaining, 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, stream));
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
  if (b->run.submitted) return set_err("batch has a submitted step: mr_batch_finish it first");
  if (enqueue_reset(b, seed_base) != 0) return -1;
  HIPCHK(hipStreamSynchronize(b->stream.get()));
  return 0;
}

// The one launch loop. Chunks of D.L clusters, one after another (a streaming batch is one chunk of
// all clusters), each by launches of at most the budget's events per cluster: enqueue a step (a
// submitted batch has its first one in flight), wait, account it, close the chunk when nothing of
// it remains. A call cut short by max_events (0: no bound) resumes with the chunk it stopped in.
static int advance(mr_batch* b, uint64_t max_events, mr_run_stats& s) {
  RunState& r = b->run;
  const uint32_t chunk = b->D.stream ? b->D.C : b->D.L;
  for (uint64_t done_events = 0; r.c_open < b->D.C;) {
    uint32_t budget = b->budget;
    if (!r.submitted) {
      if (max_events) {
        if (done_events >= max_events) break;
        budget = (uint32_t)std::min<uint64_t>(budget, max_events - done_events);
      }
      if (enqueue_step(b, r.c_open, budget) != 0) return -1;
    }
    HIPCHK(hipStreamSynchronize(b->stream.get()));
    r.submitted = false;
    float ms = 0.f;
    HIPCHK(hipEventElapsedTime(&ms, b->ev0.get(), b->ev1.get()));
    s.kernel_ms += ms;
    s.launches++;
    done_events += budget;
    if (remaining_after(b) == 0) r.c_open += chunk;
  }
  return 0;
}

// mr_batch_run and mr_batch_finish: the loop, then once per call the guard's verdict and the counter
// reduce (events processed and clusters left are sums over the per-cluster counters)
static int run_from(mr_batch* b, uint64_t max_events, std::chrono::steady_clock::time_point t0,
                    mr_run_stats* st, mr_counters* cnt) {
  HIPCHK(hipSetDevice(b->cfg.device));
  mr_run_stats s;
  std::memset(&s, 0, sizeof s);
  const int rc = advance(b, max_events, s);
  b->D.c0 = 0;  // (a launch's argument: 0 between calls, whichever way the loop ended)
  if (rc != 0 || guard_check(b) != 0) return -1;
  mr_counters c;
  if (mr_batch_counters(b, &c) != 0) return -1;
  if (b->pg.rec && group_reduce(b) != 0) return -1;  // every group's row, one pass
  s.events = c.events;
  s.remaining = c.clusters - c.done;
  s.wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  if (st) *st = s;
  if (cnt) *cnt = c;
  return 0;
}

int mr_batch_run(mr_batch* b, uint64_t max_events_per_call, mr_run_stats* st) {
  if (!b) return set_err("null batch");
  if (b->run.submitted) return set_err("batch has a submitted step: mr_batch_finish it first");
  return run_from(b, max_events_per_call, std::chrono::steady_clock::now(), st, nullptr);
}

// Pipelined steps (bench.py): reset + the first step-kernel launch are only
// enqueued, so the host can queue the next batch's step on its own stream and
// that batch's waves take the CUs this batch's early-finishing waves free.
int mr_batch_submit(mr_batch* b, uint64_t seed_base) {
  if (!b) return set_err("null batch");
  if (b->run.submitted) return set_err("batch already has a submitted step");
  const auto t0 = std::chrono::steady_clock::now();
  if (enqueue_reset(b, seed_base) != 0) return -1;
  if (enqueue_step(b, 0, b->budget) != 0) return -1;
  b->run.submitted = true;
  b->run.t_submit = t0;
  return 0;
}

// the loop from the submitted launch on: clusters past its budget, and later chunks, run here
int mr_batch_finish(mr_batch* b, mr_run_stats* st, mr_counters* cnt) {
  if (!b) return set_err("null batch");
  if (!b->run.submitted) return set_err("no submitted step");
  return run_from(b, 0, b->run.t_submit, st, cnt);
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
    return hipMemcpy2DAsync(dst, width, p, pitch, width, C, hipMemcpyDeviceToHost, b->stream.get());
  };
  if (code) {
    c32.resize(C);
    HIPCHK(row(c32.data(), b->D.cs32, CS_CODE, 4, false));
  }
  if (time_us) HIPCHK(row(time_us, b->D.cs32, CS_VTIME, 4, false));
  if (digest) HIPCHK(row(digest, b->D.cs64, C64_DIGEST, 8, true));
  HIPCHK(hipStreamSynchronize(b->stream.get()));
  for (size_t i = 0; i < c32.size(); i++) code[i] = (uint16_t)c32[i];
  return 0;
}

int mr_batch_counters(mr_batch* b, mr_counters* out) {
  if (!b || !out) return set_err("null argument");
  HIPCHK(hipSetDevice(b->cfg.device));
  std::vector<unsigned long long> h(RED_N, 0);
  h[RED_FIRST_FAIL] = ~0ull;
  HIPCHK(hipMemcpyAsync(b->red.get(), h.data(), RED_N * 8, hipMemcpyHostToDevice, b->stream.get()));
  HIPCHK(launch_reduce(b->D, b->red.get(), b->cfg.cluster_base, b->stream.get()));
  HIPCHK(hipMemcpyAsync(h.data(), b->red.get(), RED_N * 8, hipMemcpyDeviceToHost, b->stream.get()));
  HIPCHK(hipStreamSynchronize(b->stream.get()));
  return fill_counters(b, h.data(), b->D.C, out);
}

// the parameter groups' reduce rows as of now: preset, one group_reduce_kernel pass, on the stream
static int group_reduce(mr_batch* b) {
  ParamGroups& pg = b->pg;
  std::vector<unsigned long long> h(pg.n() * RED_N, 0);
  for (size_t g = 0; g < pg.n(); g++) h[g * RED_N + RED_FIRST_FAIL] = ~0ull;
  HIPCHK(hipMemcpyAsync(pg.red.get(), h.data(), h.size() * 8, hipMemcpyHostToDevice, b->stream.get()));
  HIPCHK(launch_group_reduce(b->D, pg.gof.get(), (uint32_t)pg.n(), pg.red.get(), b->cfg.cluster_base,
                             b->stream.get()));
  HIPCHK(hipStreamSynchronize(b->stream.get()));  // (h is read until the copy is done)
  pg.fresh = true;
  return 0;
}

// mr_counters of `clusters` clusters from a reduce vector h[RED_N] (mr_dev.h CNT_* and RED_*)
static int fill_counters(mr_batch* b, const unsigned long long* h, uint64_t clusters, mr_counters* out) {
  std::memset(out, 0, sizeof *out);
  out->clusters = clusters;
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

// what the trace getters ask before they copy: a traced cluster, and the batch's stream at rest
// (it is non-blocking, so the null stream's copies are not ordered after it)
static int trace_enter(mr_batch* b, uint32_t k, const void* out, const size_t* n) {
  if (!b || !out || !n) return set_err("null argument");
  if (k >= b->D.trace_clusters) return set_err("cluster not traced");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream.get()));
  return 0;
}

int mr_trace_get(mr_batch* b, uint32_t k, mr_event* out, size_t cap, size_t* n) {
  if (trace_enter(b, k, out, n) != 0) return -1;
  return copy_trace_row(b, k, b->D.trace, out, cap, n);
}

int mr_trace_digests(mr_batch* b, uint32_t k, uint64_t* out, size_t cap, size_t* n) {
  if (trace_enter(b, k, out, n) != 0) return -1;
  return copy_trace_row(b, k, b->D.tdig, out, cap, n);
}

int mr_trace_applies(mr_batch* b, uint32_t k, uint64_t* out, size_t cap, size_t* n) {
  if (trace_enter(b, k, out, n) != 0) return -1;
  size_t m = cap < b->D.trace_cap ? cap : b->D.trace_cap;
  HIPCHK(hipMemcpy(out, b->D.tapp + (size_t)k * b->D.trace_cap * 2u, m * 2u * sizeof(uint64_t),
                   hipMemcpyDeviceToHost));
  while (m && !out[2 * (m - 1)]) m--;
  *n = m;
  return 0;
}

const char* mr_batch_kernel(const mr_batch* b) {
  if (!b) return "";
  switch (family_of(b->D)) {
    case F_TAPE: return "step_kernel_tape";
    case F_POOL: return "pool_kernel";
    default: return "step_kernel";
  }
}

uint32_t mr_decision_word(uint32_t v, uint32_t lo, uint32_t hi) {
  if (hi <= lo || v < lo || v >= hi) return 0;
  // ceil((v - lo) * 2^32 / (hi - lo)): the first w whose range image is v
  const uint64_t span = hi - lo, num = (uint64_t)(v - lo) << 32;
  return (uint32_t)((num + span - 1) / span);
}

// the batch's decision tables (whoever installed them) freed; Philox draws
static void drop_decisions(mr_batch* b) { install_tables(b, Tables{}); }

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
  hipError_t e = upload(t.tape, tab.data(), rows);
  if (e == hipSuccess) e = upload(t.tdesc, cdesc.data(), C);
  if (!replay) {  // (null in a replay: no record has an edit)
    if (e == hipSuccess) e = upload(t.vedit, ved.data(), rows);
    if (e == hipSuccess) e = upload(t.vwords, vw.data(), words);
    if (e == hipSuccess) e = upload(t.vmask, masks, C * W);
  }
  if (e != hipSuccess)  // (t goes, the batch keeps its previous tables)
    return set_err(std::string(replay ? "decision table" : "variant tables") + ": " + hipGetErrorString(e));
  install_tables(b, std::move(t));
  return 0;
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
  HIPCHK(hipStreamSynchronize(b->stream.get()));
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
  HIPCHK(hipStreamSynchronize(b->stream.get()));
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
  HIPCHK(hipStreamSynchronize(b->stream.get()));
  const size_t mw = (size_t)b->D.C * b->D.vW;
  if (!mw) return 0;
  if (masks) HIPCHK(hipMemcpy(b->dec.vmask.get(), masks, mw * sizeof(uint32_t), hipMemcpyHostToDevice));
  else HIPCHK(hipMemset(b->dec.vmask.get(), 0, mw * sizeof(uint32_t)));
  return 0;
}

// The recorded tapes of clusters [first, first + count), of each at most `limit` records: one copy of
// the CS_TAPE row slice (the row is cluster-minor, so the slice is contiguous), a scan on the host,
// one tape_pack_kernel launch into a scratch buffer that starts with the offsets, one copy back. The
// host touches no record: the kernel is the one place where a tape row becomes an mr_decision.
static int read_tapes(mr_batch* b, uint32_t first, uint32_t count, uint64_t* drawn, uint64_t* off,
                      mr_decision* out, size_t cap, uint64_t limit) {
  HIPCHK(hipSetDevice(b->cfg.device));
  hipStream_t stream = b->stream.get();
  HIPCHK(hipStreamSynchronize(stream));
  const uint32_t* used_d = b->D.cs32 + CS_IDX(CS_TAPE, first, b->D.C);
  std::vector<uint32_t> used(count);
  if (count) HIPCHK(hipMemcpy(used.data(), used_d, (size_t)count * 4, hipMemcpyDeviceToHost));
  // (with decisions set the counts are misses: no records)
  const uint64_t keep = b->D.tape_mode == TAPE_RECORD ? std::min<uint64_t>(b->D.dcap, limit) : 0u;
  off[0] = 0;
  for (size_t i = 0; i < count; i++) {
    if (drawn) drawn[i] = used[i];
    off[i + 1] = off[i] + std::min<uint64_t>(used[i], keep);
  }
  const uint64_t total = off[count];
  if (!out || !total) return 0;
  if (cap < total)
    return set_err("mr_batch_get_decisions_packed: out holds " + std::to_string(cap) + " records, " +
                   std::to_string(total) + " are kept");
  const size_t head = ((size_t)(count + 1) * sizeof(uint64_t) + 255) & ~size_t(255);
  DevMem<char> scratch;
  HIPCHK(dev_alloc(scratch, head + total * sizeof(mr_decision)));
  char* recs = scratch.get() + head;
  hipError_t e = hipMemcpyAsync(scratch.get(), off, (size_t)(count + 1) * sizeof(uint64_t),
                                hipMemcpyHostToDevice, stream);
  if (e == hipSuccess)
    e = launch_tape_pack(b->dec.tape.get(), used_d, b->D.dcap, first, count,
                         reinterpret_cast<const uint64_t*>(scratch.get()),
                         reinterpret_cast<uint32_t*>(recs), stream);
  if (e == hipSuccess)
    e = hipMemcpyAsync(out, recs, total * sizeof(mr_decision), hipMemcpyDeviceToHost, stream);
  if (e == hipSuccess) e = hipStreamSynchronize(stream);
  if (e != hipSuccess) return set_err(std::string("tape pack: ") + hipGetErrorString(e));
  return 0;
}

static int get_decisions_packed_impl(mr_batch* b, uint32_t first, uint32_t count, uint64_t* drawn,
                                     uint64_t* off, mr_decision* out, size_t cap) {
  if (!b || !off) return set_err("null argument");
  if ((uint64_t)first + count > b->D.C) return set_err("clusters out of range");
  return read_tapes(b, first, count, drawn, off, out, cap, ~0ull);
}

// one cluster: the packed read-back of [k, k + 1) with the caller's cap as the limit, so *n tells
// all it drew and out gets what fits
static int mr_batch_get_decisions_impl(mr_batch* b, uint32_t k, mr_decision* out, size_t cap, size_t* n) {
  if (!b || !n) return set_err("null argument");
  if (k >= b->D.C) return set_err("cluster out of range");
  uint64_t drawn = 0, off[2];
  if (read_tapes(b, k, 1, &drawn, off, out, cap, cap) != 0) return -1;
  *n = drawn;
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
  mr_batch* made = nullptr;
  if (const int rc = mr_batch_create(&c, &made)) return rc;
  const Batch b(made);
  std::vector<mr_decision> one(d, d + n);
  for (auto& r : one) r.cluster = 0;
  // keyed replay runs the MR_TAPE kernels even for an empty trace (every draw then misses)
  const mr_decision none{0, MR_DS_TESTER, 0xFFFFu, 0xFFFFFFFFu, 0u, 0u};
  if (one.empty()) one.push_back(none);
  mr_run_stats st;
  uint16_t cd = 0;
  uint32_t t = 0;
  size_t ms = 0;
  if (const int rc = mr_batch_set_decisions(b.get(), one.data(), one.size())) return rc;
  if (const int rc = mr_batch_run(b.get(), 0, &st)) return rc;
  if (const int rc = mr_batch_verdicts(b.get(), &cd, &t, nullptr)) return rc;
  if (!out || !cap) *n_out = 0;
  else if (const int rc = mr_trace_get(b.get(), 0, out, cap, n_out)) return rc;
  if (misses) {
    if (const int rc = mr_batch_get_decisions(b.get(), 0, nullptr, 0, &ms)) return rc;
    *misses = ms;
  }
  if (code) *code = cd;
  if (time_us) *time_us = t;
  return 0;
}

void mr_batch_destroy(mr_batch* b) {
  if (!b) return;
  (void)hipSetDevice(b->cfg.device);
  if (b->stream) (void)hipStreamSynchronize(b->stream.get());
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
  delete b;  // its owners release the memory, the events and last the stream
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
  if (b->run.submitted) return set_err("batch has a submitted step: mr_batch_finish it first");
  if (seed_cluster && b->dec.mode == OWN_VARIANTS)
    return set_err("a seed list on a batch with variants set");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream.get()));
  DevMem<uint32_t> list;
  if (seed_cluster)
    if (const hipError_t e = upload(list, seed_cluster, (size_t)b->D.C); e != hipSuccess)
      return set_err(std::string("seed list: ") + hipGetErrorString(e));
  b->sof = std::move(list);
  b->D.sof = b->sof.get();
  b->D.tape_mode = tape_mode_of(b);
  return 0;
}

// The batch's parameter groups (madraft_sim.h): every group resolved against the batch's cfg and
// checked, every position's group checked, then one 32-B record per cluster (its group's values, as
// the kernels' accessors read them), the clusters' groups and the groups' reduce rows staged whole
// before the previous groups are freed by the move, so a rejected call leaves the batch as it was.
static int set_param_groups_impl(mr_batch* b, const mr_param_group* g, size_t n_groups,
                                 const uint32_t* group_of) {
  const size_t C = b->D.C;
  const mr_cfg& cfg = b->cfg;
  if (n_groups >= (1ull << 32)) return set_err("too many parameter groups (2^32 - 1 at most)");
  std::vector<uint32_t> val(n_groups * PG_W);
  for (size_t i = 0; i < n_groups; i++) {
    const mr_param_group& G = g[i];
    const std::string at = " (parameter group " + std::to_string(i) + ")";
    if (G.flags & ~MR_F_SWEEPABLE) return set_err("a flag bit outside MR_F_SWEEPABLE" + at);
    if (G.reserved[0] || G.reserved[1]) return set_err("reserved words must be 0" + at);
    uint32_t* v = val.data() + i * PG_W;
    v[PG_HB] = G.hb_us ? G.hb_us : cfg.hb_us;
    v[PG_ELO] = G.elect_lo_us ? G.elect_lo_us : cfg.elect_lo_us;
    v[PG_EHI] = G.elect_hi_us ? G.elect_hi_us : cfg.elect_hi_us;
    v[PG_K] = G.ae_max ? G.ae_max : cfg.ae_max;
    v[PG_ITERS] = G.iters ? G.iters : b->D.iters;  // (the batch's: cfg's, or the test body's own)
    v[PG_BUGS] = G.flags & MR_F_SWEEPABLE & ~(MR_F_UNRELIABLE | MR_F_NULL_RAFT);
    v[PG_UNREL] = (G.flags & MR_F_UNRELIABLE) ? 1u : 0u;
    v[PG_NULL] = (G.flags & MR_F_NULL_RAFT) ? 1u : 0u;
    if (v[PG_EHI] <= v[PG_ELO]) return set_err("elect_hi_us <= elect_lo_us" + at);
    if (v[PG_K] > cfg.ae_max) return set_err("ae_max above the batch's" + at);
  }
  ParamGroups pg;
  pg.positions.assign(n_groups, 0);
  std::vector<uint32_t> rec(C * PG_W);
  for (size_t c = 0; c < C; c++) {
    if (group_of[c] >= n_groups)
      return set_err("group_of[" + std::to_string(c) + "] = " + std::to_string(group_of[c]) +
                     ": no such parameter group");
    pg.positions[group_of[c]]++;
    std::memcpy(rec.data() + c * PG_W, val.data() + (size_t)group_of[c] * PG_W, PG_W * sizeof(uint32_t));
  }
  hipError_t e = upload(pg.rec, rec.data(), rec.size());
  if (e == hipSuccess) e = upload(pg.gof, group_of, C);
  if (e == hipSuccess) e = dev_alloc(pg.red, n_groups * RED_N);
  if (e != hipSuccess)  // (pg goes, the batch keeps its previous groups)
    return set_err(std::string("parameter groups: ") + hipGetErrorString(e));
  b->pg = std::move(pg);
  return 0;
}

int mr_batch_set_param_groups(mr_batch* b, const mr_param_group* g, size_t n_groups,
                              const uint32_t* group_of) {
  if (!b) return set_err("null batch");
  if (n_groups && (!g || !group_of)) return set_err("null parameter groups");
  if (b->run.submitted) return set_err("batch has a submitted step: mr_batch_finish it first");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipStreamSynchronize(b->stream.get()));
  if (!n_groups) b->pg = ParamGroups{};
  else if (const int rc = no_throw("parameter groups", [&] { return set_param_groups_impl(b, g, n_groups, group_of); }))
    return rc;
  b->D.pgrp = b->pg.rec.get();
  b->D.tape_mode = tape_mode_of(b);
  return 0;
}

int mr_batch_group_counters(mr_batch* b, uint32_t group, mr_counters* out) {
  if (!b || !out) return set_err("null argument");
  if (!b->pg.rec) return set_err("mr_batch_group_counters without parameter groups");
  if (group >= b->pg.n())
    return set_err("parameter group " + std::to_string(group) + " of " + std::to_string(b->pg.n()));
  if (b->run.submitted) return set_err("batch has a submitted step: mr_batch_finish it first");
  HIPCHK(hipSetDevice(b->cfg.device));
  if (!b->pg.fresh && group_reduce(b) != 0) return -1;
  unsigned long long h[RED_N];
  HIPCHK(hipMemcpy(h, b->pg.red.get() + (size_t)group * RED_N, sizeof h, hipMemcpyDeviceToHost));
  return fill_counters(b, h, b->pg.positions[group], out);
}

// bytes of one element of each array, by DevArray
#define MR_ROW_(m, elements, present, reset) (uint32_t)sizeof(*Dev().m),
static constexpr uint32_t k_dev_esz[A__N] = {MR_DEV_ARRAYS(MR_ROW_)};
#undef MR_ROW_

// mr_batch_fork (madraft_sim.h): everything is checked, the plan laid out and the sources uploaded
// before fork_kernel writes, so every error leaves both batches as they were. The plan is the walk
// of MR_DEV_ARRAYS that the reset and dev_layout make: every row that is a cluster's state
// (k_dev_own) and that both batches hold, by its per-owner size in each (DevLayout::per).
static int fork_impl(mr_batch* dst, mr_batch* src, const uint32_t* src_of) {
  const mr_cfg &d = dst->cfg, &s = src->cfg;
  const std::pair<const char*, bool> differs[] = {
      {"device", d.device != s.device}, {"scenario", d.scenario != s.scenario},
      {"n_nodes", d.n_nodes != s.n_nodes}, {"log_cap", d.log_cap != s.log_cap},
      {"apply_cap", d.apply_cap != s.apply_cap}, {"msg_slots", d.msg_slots != s.msg_slots},
      {"ae_max", d.ae_max != s.ae_max}, {"MR_F_SAFETY", ((d.flags ^ s.flags) & MR_F_SAFETY) != 0},
      {"MR_KEY_ROWS", dst->D.krows != src->D.krows}};  // (which message keys the 7-server pool keeps in HBM)
  for (const auto& [what, bad] : differs)
    if (bad) return set_err(std::string("mr_batch_fork: the batches differ in ") + what);
  const uint32_t Cd = dst->D.C, Cs = src->D.C, Td = dst->D.trace_clusters, Ts = src->D.trace_clusters;
  const bool in_place = src == dst;
  std::vector<uint32_t> of(src_of, src_of + Cd);  // as the kernel takes it: identity in place = skip
  std::vector<uint32_t> tracen;                   // the source's CS_TRACEN of its traced clusters
  bool any = false;
  for (uint32_t c = 0; c < Cd; c++) {
    const uint32_t from = src_of[c];
    const std::string at = "mr_batch_fork: src_of[" + std::to_string(c) + "] = " + std::to_string(from);
    if (from == FORK_SKIP) continue;
    if (from >= Cs) return set_err(at + ": the source has " + std::to_string(Cs) + " clusters");
    if (in_place && from == c) { of[c] = FORK_SKIP; continue; }
    if (in_place && src_of[from] != FORK_SKIP && src_of[from] != from)
      return set_err(at + ": that source is itself overwritten (src_of[" + std::to_string(from) + "] = " +
                     std::to_string(src_of[from]) + ")");
    if (c < Td) {
      if (from >= Ts) return set_err(at + ": a traced position from a source that is not traced");
      if (tracen.empty()) {
        tracen.resize(Ts);
        HIPCHK(hipMemcpy(tracen.data(), src->D.cs32 + CS_IDX(CS_TRACEN, 0, Cs), (size_t)Ts * 4,
                         hipMemcpyDeviceToHost));
      }
      const uint32_t held = std::min(tracen[from], src->D.trace_cap);
      // (a source past its own cap has dropped records a destination of another cap would hold)
      if (tracen[from] > src->D.trace_cap && src->D.trace_cap != dst->D.trace_cap)
        return set_err(at + ": the source drew " + std::to_string(tracen[from]) + " trace records past its "
                       "trace_cap " + std::to_string(src->D.trace_cap) + ", the destination's is " +
                       std::to_string(dst->D.trace_cap));
      if (held > dst->D.trace_cap)
        return set_err(at + ": the source holds " + std::to_string(held) +
                       " trace records, the destination's trace_cap is " + std::to_string(dst->D.trace_cap));
    }
    any = true;
  }
  if (!any) return 0;  // nothing to copy: both batches stay bit for bit what they were
  if ((d.flags & MR_F_RECORD) && !(s.flags & MR_F_RECORD))
    return set_err("mr_batch_fork: a recording destination needs a recording source (MR_F_RECORD)");
  // the message keys in HBM keep the format of the kernels that wrote them
  const KeyFormat had = src->run.keys, next = key_format_of(dst->D);
  if (had != KEYS_UNSET && (had != next || (dst->run.keys != KEYS_UNSET && dst->run.keys != had)))
    return set_err(std::string("mr_batch_fork: source ran on ") + key_format_name(had) +
                   ", destination continues on " + key_format_name(next) + " (another message-key format)");

  const bool keep_tape = dst->dec.mode == OWN_RECORD && src->dec.mode == OWN_RECORD;
  ForkPlan P{};
  P.Cd = Cd; P.Cs = Cs;
  uint64_t blocks = 0;
  auto add = [&](ForkRow r) {
    if (!r.owners || !r.dper || !r.sper) return true;
    if (r.kind != FK_MINOR && ((r.dper | r.sper) & 15u)) return false;
    r.blk0 = (uint32_t)blocks;
    blocks += fork_blocks(r);
    if (blocks >= (1ull << 31) || P.n_rows == FORK_ROWS) return false;
    P.row[P.n_rows++] = r;
    return true;
  };
  bool ok = true;
  for (uint32_t a = 0; a < A__N && ok; a++) {
    const OwnKind own = k_dev_own[a];
    if (!own_is_cluster(own) || !dst->lay.bytes[a] || !src->lay.bytes[a]) continue;
    if ((dst->lay.per[a] | src->lay.per[a]) >> 32) { ok = false; break; }
    ForkRow r{};
    r.dst = dst->base.get() + dst->lay.off[a];
    r.src = src->base.get() + src->lay.off[a];
    r.zfield = ~0u;
    if (own == OWN_MINOR) {  // (n and msg_slots are equal: the same fields on both sides)
      r.kind = FK_MINOR; r.owners = Cd; r.esz = k_dev_esz[a];
      r.dper = r.sper = (uint32_t)(dst->lay.per[a] / r.esz);
      if (src->lay.per[a] != dst->lay.per[a] || (r.esz != 4 && r.esz != 8)) { ok = false; break; }
      if (a == A_cs32 && !keep_tape) r.zfield = CS_TAPE;  // no tape comes along: none drawn
    } else {
      r.kind = FK_MAJOR; r.owners = own == OWN_TRACED ? Td : Cd;
      r.dper = (uint32_t)dst->lay.per[a]; r.sper = (uint32_t)src->lay.per[a];
      if (own == OWN_MAJOR && r.dper != r.sper) { ok = false; break; }
    }
    ok = add(r);
  }
  if (ok && keep_tape) {  // the records drawn so far: a forked position's tape is its whole history
    ForkRow r{};
    r.dst = reinterpret_cast<char*>(dst->dec.tape.get());
    r.src = reinterpret_cast<const char*>(src->dec.tape.get());
    r.kind = FK_TAPE; r.owners = Cd; r.zfield = ~0u;
    if (((uint64_t)dst->dec.dcap | src->dec.dcap) >> 28) ok = false;
    r.dper = dst->dec.dcap * 16u; r.sper = src->dec.dcap * 16u;
    P.tape_used = src->D.cs32 + CS_IDX(CS_TAPE, 0, Cs);
    ok = ok && add(r);
  }
  if (!ok) return set_err("mr_batch_fork: the batches' arrays do not fit one fork launch");
  P.blocks = (uint32_t)blocks;
  DevMem<uint32_t> of_d;
  if (const hipError_t e = upload(of_d, of.data(), of.size()); e != hipSuccess)
    return set_err(std::string("mr_batch_fork: ") + hipGetErrorString(e));
  P.src_of = of_d.get();
  hipStream_t stream = dst->stream.get();
  HIPCHK(hipEventRecord(dst->ev0.get(), stream));
  HIPCHK(launch_fork(P, stream));
  HIPCHK(hipEventRecord(dst->ev1.get(), stream));
  HIPCHK(hipStreamSynchronize(stream));
  // the destination's launch loop starts over: a position with a verdict costs its lane one load
  // (launch_begin / cluster_claim), whether the batch runs whole, in chunks or streaming
  dst->run.c_open = 0;
  dst->run.resume = false;
  if (dst->run.keys == KEYS_UNSET) dst->run.keys = had;
  dst->pg.fresh = false;
  dst->fork_timed = true;
  return 0;
}

int mr_batch_fork(mr_batch* dst, mr_batch* src, const uint32_t* src_of) {
  if (!dst || !src || !src_of) return set_err("null argument");
  if (dst->run.submitted || src->run.submitted)
    return set_err("batch has a submitted step: mr_batch_finish it first");
  HIPCHK(hipSetDevice(dst->cfg.device));
  HIPCHK(hipStreamSynchronize(src->stream.get()));
  HIPCHK(hipStreamSynchronize(dst->stream.get()));
  return no_throw("mr_batch_fork", [&] { return fork_impl(dst, src, src_of); });
}

int mr_batch_fork_ms(mr_batch* b, float* ms) {
  if (!b || !ms) return set_err("null argument");
  if (!b->fork_timed) return set_err("mr_batch_fork_ms: the batch's last work was not a fork");
  HIPCHK(hipSetDevice(b->cfg.device));
  HIPCHK(hipEventElapsedTime(ms, b->ev0.get(), b->ev1.get()));
  return 0;
}

int mr_replay(const mr_cfg* cfg, const mr_decision* d, size_t n, mr_event* out, size_t cap,
              size_t* n_out, uint16_t* code, uint32_t* time_us, uint64_t* misses) {
  return no_throw("mr_replay", [&] {
    return mr_replay_impl(cfg, d, n, out, cap, n_out, code, time_us, misses);
  });
}

}  // extern "C"
