// mr_pool.inc — the cluster-pool step kernel (included by mr_kernel.hip in MR_POOL units;
// DESIGN.md §6.10).
//
// step_kernel binds a cluster to a lane for the whole launch, so a wave iteration issues the
// union of the paths its 64 clusters' next events take (measured: 12.9 of 64 lanes active per
// VALU instruction). Here a workgroup of POOL_WAVES waves (two per SIMD) owns a pool of up to
// POOL_SLOTS clusters. Between its events a cluster's run state — what step_kernel keeps in
// registers — is a record in LDS (px_record), its message keys a column of the LDS key rows, and its
// slot an entry in the queue of its next event's kind (PK_*: a tester step, an AppendEntries
// request delivery, any other node event); the entry, lap << 16 | decision | slot (mr_qentry.h),
// also names that event (class, node, spawned thread), decided once, when it is published. A wave that is free reads the queues' lengths, takes up
// to 64 ready clusters of one kind (a compare-and-swap of the queue's head: an entry is claimed by
// exactly one wave), runs their events with the state in registers through the same handlers as
// step_kernel, and publishes each cluster's next kind. A cluster runs on one lane at a time, its events in its own order, so
// every result equals step_kernel's and the oracle's; only which lanes run together changes.
// What the two kernels do to a cluster between HBM and registers is one piece of code
// (mr_kernel.hip: cluster_load / cluster_store / cluster_claim, launch_begin / launch_end,
// next_event / run_event); here are the LDS record, the kinds and the queues.
// The modelled gain (tools/bin_sim.py, oracle traces, r04 section costs): 1.55-1.77x.
//
// MR_POOL 2 units build the same kernel for the kvraft / shard_ctrler test bodies: 4 waves and
// 256 clusters per workgroup (64 message slots of keys; their handlers take one wave per SIMD of
// registers), the spawned tester threads' scheduler key in the record, and queues for a tester or
// clerk-thread step, an AppendEntries request to a server, another server event, a reply to a
// clerk host and (the 15-client linearizable body, ap_cont) an applier continuation. Measured
// (profiles/r05_ab_svcpool.txt): config 5 +26 %, its linearizable variants +25 % / +19 % over the
// step kernel; the continuation +36 % on C5-lin 3A (profiles/r06_ab_kvap.txt).
//
// The 7-server Raft bodies (NB = 7, KEYS_HBM) keep 512 clusters per workgroup by holding LDS key
// rows for message slots 0..31 only (D.krows) and the keys of slots 32..63 in HBM (D.mkey):
// profiles/r06_ab_c4.txt, config 4 +12.4 %.
//
// Statistics counters: a lane adds the sums of the events it runs in registers (x.cnt) and the
// workgroup adds them, as 64-bit sums, to the batch's pool sums D.pcnt at the end (reduce_kernel
// adds those to the per-cluster counters: a workgroup that streams a large batch sums more events
// than 32 bits hold);
// the two counters read per cluster (leaders elected: the coverage histogram; the largest
// applied index: the leader-completeness check) travel in the cluster's record.

// The record's words are the rows of px_record below, the one description that the store, the load
// and the word count PX_W walk. Word 0 is the cluster id; PX_EMPTY there: the slot holds no cluster
constexpr uint32_t PX_EMPTY = ~0u;
// bins: a tester step (PK_TESTER); an AppendEntries request delivery (key bit 3, PK_AE); every
// other node event (PK_NODE); and, for test bodies that crash and restart servers
// (restarts_servers), bins of their own for RequestVote request / reply deliveries (key bit 4),
// deliveries to a server that is down or disconnected (dropped there) and node timers
// (heartbeats and elections, whose sends go to every peer). Same-box A/B (r05ab3): the finer
// bins +5.5 % on figure_8_unreliable_crash, -3.5 % on figure_8_unreliable_2c. The service pool
// (MR_POOL 2): a tester or spawned-thread step (clerk calls), an AppendEntries request to a
// server (x.aem), another server event, a reply delivered to a clerk host (PK_CLERK)
// (Round 6: AppendEntries requests whose payload takes more than one batch of loads in a kind of
// their own: figure_8_unreliable_2c -1.8 %, its crash variant -2.2 %, config 4 +1.1 %,
// profiles/r06_ab_ael.txt — the short deliveries' waves run fewer clusters. Not kept.)
enum : uint32_t { PK_TESTER, PK_AE, PK_NODE, PK_RV, PK_DROP, PK_TMR };
constexpr uint32_t PK_CLERK = 3u;  // the service pool's fourth kind
constexpr uint32_t PK_APPLY = 4u;  // the service pool's fifth: an applier continuation (AP_CAP)
constexpr uint32_t PK__N = MR_POOL == 2 ? 5u : 6u;
static_assert(PK__N <= 8, "MR_PROF keeps 8 kinds of statistics");
// (Round 6 on the queue claim, same box, profiles/r06_ab_fine_sleep.txt: the fine kinds for every
// body -2.7 % on figure_8_unreliable_2c, none for its crash variant -8.6 %: kept by restarts.)
template <uint32_t S>
constexpr bool pool_fine_bins() { return restarts_servers(S); }
constexpr uint32_t PS = POOL_SLOTS;
// a queue entry (mr_qentry.h): the slot, next_event's decision for the cluster's next event, and
// the lap tag. The fields hold what this unit's next_event can choose
using QE = QEntry<MR_POOL>;
static_assert(QE::SLOT_N == POOL_SLOTS, "queue positions wrap at the pool size");
static_assert(CLS_MSG < QE::CLS_N && CLS_TIMER < QE::CLS_N && CLS_TESTER < QE::CLS_N, "an entry's class field");
static_assert(NB <= QE::NODE_N && KEY_DST < QE::NODE_N, "an entry's node field: a timer's server, a key's destination");
static_assert(MR_POOL == 2 || QE::TCLI_B == 0u, "the Raft pool runs no spawned threads (pool_kernel asserts nthr)");
static_assert(MR_POOL != 2 || CLERK_HOST + 16u <= QE::NODE_N, "the service pool's clerk hosts are nodes 8 ..");

// The ready clusters of a kind are a FIFO ring of slot ids: per kind a {head, tail} pair of
// positions and PS entries (a kind never holds more than the pool), each entry tagged with the
// lap of its position so a stale one is never taken. Between the tag and the slot an entry carries
// what next_event decided when it was published (class, node, spawned thread: mr_qentry.h), so the
// claiming wave runs that event with its key from the record (event_key) and does not decide again:
// next_event runs once per event, in pool_kind, off the path from the claim to the event's loads. A wave claims min(64, queued) entries of
// the fullest kind with one compare-and-swap of the head and lane i reads entry head + i; a wave
// publishes its lanes' next kinds with one atomic add of a tail per kind present. Same-box A/B
// against round 5's 512-bit bins with a per-wave claim list (r06_q, profiles/r06_ab_queue.txt):
// figure_8_unreliable_2c 104.3 -> 102.8 ms, its crash variant 43.40 -> 41.75 ms, VALU
// instructions per event 40.1 -> 34.9.
//
// LDS after the key rows [key_rows][POOL_SLOTS] and the per-wave staging (mr_kernel.hip: lds_layout)
struct PoolL {
  uint32_t* xr;    // [PX_W][POOL_SLOTS] cluster records
  uint32_t* qc;    // [PK__N][2] the queues' head and tail positions (8-B aligned pairs)
  uint32_t* q;     // [PK__N][PS] queue entries (QE): lap << 16 | decision | slot
  uint32_t* live;  // clusters running and within the launch's budget
};

// A walk of the record: PX_PUT stores the lane's registers to its slot's column r[word * PS],
// PX_GET loads them, PX_COUNT only counts the words. bits(f, w) is the one primitive: the next w
// bits of the current word hold f (w = 32: a whole word); the others are encodings on top of it
enum PxMode { PX_PUT, PX_GET, PX_COUNT };
// mmin (32-bit keys: t << 32 | the key's low five bits, ~0 = no message) as one word: the key
constexpr uint32_t mmin_pack(uint64_t m) { return m == ~0ull ? ~0u : ((uint32_t)(m >> 32) << 5) | ((uint32_t)m & 31u); }
constexpr uint64_t mmin_unpack(uint32_t w) { return w == ~0u ? ~0ull : ((uint64_t)(w >> 5) << 32) | (w & 31u); }
template <PxMode M>
struct Px {
  uint32_t* r = nullptr;
  uint32_t n = 0, sh = 0, cur = 0;  // words done, bits done of the current word, that word
  bool ok = true;                   // (PX_COUNT) no field straddles a word
  // (cut: f may hold higher bits, which the record drops; otherwise f fits its w bits as it is)
  template <class T>
  constexpr __forceinline__ void bits(T& f, uint32_t w, bool cut = false) {
    const uint32_t m = w < 32u ? (1u << w) - 1u : ~0u;
    if constexpr (M == PX_GET) {
      if (sh == 0u) cur = r[n * PS];
      f = (cur >> sh) & m;
    }
    if constexpr (M == PX_PUT) cur |= (cut ? (uint32_t)f & m : (uint32_t)f) << sh;
    if constexpr (M == PX_COUNT) ok = ok && sh + w <= 32u;
    if ((sh += w) < 32u) return;
    if constexpr (M == PX_PUT) r[n * PS] = cur;
    n++;
    sh = cur = 0u;
  }
  template <class... T>
  constexpr __forceinline__ void words(T&... f) { (bits(f, 32u), ...); }  // a whole word each
  template <class T>
  constexpr __forceinline__ void half(T& f, uint32_t s) {  // bits s .. s + 31 of a 64-bit value
    uint32_t w = 0u;
    if constexpr (M == PX_PUT) w = (uint32_t)(f >> s);
    bits(w, 32u);
    if constexpr (M == PX_GET) f = s ? f | (uint64_t)w << 32 : (uint64_t)w;
  }
  template <class T>
  constexpr __forceinline__ void wide(T& f) { half(f, 0u), half(f, 32u); }  // 64 bits: low, high
  template <class T>
  constexpr __forceinline__ void mmin(T& f) {
    uint32_t w = 0u;
    if constexpr (M == PX_PUT) w = mmin_pack(f);
    bits(w, 32u);
    if constexpr (M == PX_GET) f = mmin_unpack(w);
  }
  constexpr void reserve(uint32_t words) { n += words; }
};
// THE RECORD: what a pool slot keeps of its cluster between two events (X, and the launch's budget
// end), row by row in the order of its words. Every position, width and condition is here only
template <uint32_t S, class V, class XT>
constexpr __forceinline__ void px_record(V& v, XT& x, uint32_t& evend) {
  // (word 0, the cluster id: PX_EMPTY, px_clear / px_held)
  v.words(x.c, x.now, x.events, x.msgs_sent, x.t_ctr, x.twake, x.trace_n);
  v.wide(x.digest);
  v.mmin(x.mmin);
  v.half(x.free_mask[0], 0u);  // free message slots 0..31
  v.bits(x.code, 16u, true), v.bits(x.inflight, 8u), v.bits(x.mslot, 8u);
  // (conn: servers 0..7 only; the service pool keeps its clerk hosts', 8 + k, in the whole word below)
  v.bits(x.netmode, 8u), v.bits(x.conn, 8u, true), v.bits(x.alive, 8u), v.bits(x.lmask, 8u);
  // the two counters that travel; where the launch's event budget ends for the cluster
  v.words(x.cnt[CNT_LEADERS], x.cnt[CNT_MAX_INDEX], evend);
  constexpr bool SVC = MR_POOL == 2;
  if constexpr (KEYS_HBM || SVC) v.half(x.free_mask[0], 32u);  // free message slots 32..63
  if constexpr (SVC) {
    v.wide(x.aem);
    v.words(x.cwake, x.ctid, x.cslot, x.conn);
    if constexpr (ap_cont(S)) v.words(x.ap0, x.ap1, x.ap2, x.ap3);  // (node_event AP_CAP)
    else v.reserve(4u);  // (the continuation's words stay: one PX_W per unit)
  }
#pragma unroll
  for (uint32_t d = 0; d < NB; d++) v.bits(x.timer[d], 32u);
}
template <uint32_t S>
constexpr Px<PX_COUNT> px_count() {
  Px<PX_COUNT> v{};
  X x{};
  uint32_t evend = 0;
  px_record<S>(v, x, evend);
  return v;
}
static_assert(px_count<0>().ok && px_count<0>().sh == 0u, "px_record: the fields of a shared word fill its 32 bits");
constexpr uint32_t PX_W = px_count<0>().n;  // (the same for every scenario: pool_kernel asserts it)
// registers <-> the cluster's LDS record (x.ls is its slot)
template <uint32_t S>
DI void px_put(const PoolL& L, const X& x, uint32_t evend) {
  Px<PX_PUT> v{L.xr + x.ls};
  px_record<S>(v, x, evend);
}
template <uint32_t S>
DI uint32_t px_get(const PoolL& L, X& x) {  // returns the launch's budget end
  // what no record holds: said here, and the rows whose condition holds load over it
  x.sleep_us = 0; x.yield = 0;
  x.cwake = INF_T; x.ctid = 0; x.cslot = 0; x.ap0 = 0;
  Px<PX_GET> v{L.xr + x.ls};
  uint32_t evend = 0;
  px_record<S>(v, x, evend);
  return evend;
}
DI void px_clear(const PoolL& L, uint32_t slot) { L.xr[slot] = PX_EMPTY; }
DI bool px_held(const PoolL& L, uint32_t slot) { return L.xr[slot] != PX_EMPTY; }
// a launch's budget for a cluster that enters it at x.events
DI uint32_t budget_end(const X& x, uint32_t budget) { return x.events > ~0u - budget ? ~0u : x.events + budget; }

constexpr LdsLayout pool_layout(uint32_t M) { return lds_layout(key_rows(M), PX_W, PK__N); }
DI PoolL pool_l(const Dev& D) {
  const LdsLayout l = pool_layout(D.M);
  return PoolL{lds_words() + l.xr, lds_words() + l.qc, lds_words() + l.q, lds_words() + l.live};
}
constexpr size_t pool_lds_bytes(uint32_t M) { return (size_t)pool_layout(M).total * 4u; }
DI unsigned long long qc_pair(const PoolL& L, uint32_t k) {  // {head, tail} of kind k, one 8-B load
  return __hip_atomic_load(reinterpret_cast<unsigned long long*>(L.qc) + k, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the cluster's next event, decided here and nowhere else in the pool: next_event's decision `dc`,
// which travels in the queue entry to the wave that claims it, and its kind (the queue). The key
// of a decision is event_key's (mr_kernel.hip), here and at the claim
template <uint32_t S>
DI uint32_t pool_kind(const X& x, QDec& dc) {
  constexpr bool FINE = pool_fine_bins<S>();
  uint64_t key;
  next_event<S>(x, key, dc.cls, dc.node, dc.tcli);
  const uint32_t cls = dc.cls, node = dc.node;
  if constexpr (ap_cont(S))
    if (x.ap0 >> 31) return PK_APPLY;  // the current event's applier continues (AP_CAP)
  if (cls == CLS_TESTER) return PK_TESTER;
  if constexpr (MR_POOL == 2) {
    if (cls != CLS_MSG) return PK_NODE;
    if (node >= CLERK_HOST) return PK_CLERK;
    return ((x.aem >> x.mslot) & 1ull) ? PK_AE : PK_NODE;
  }
  // node timers in a kind of their own also where a heartbeat or an election sends to six peers
  // (the 7-server bodies, config 4: +4.0 / +5.8 % same box, the fine kinds +3.7 %,
  // profiles/r06_ab_c4k.txt); at 5 servers it measured +0.1 % (profiles/r06_ab_tmr.txt)
  if (cls != CLS_MSG) return (FINE || NB >= 7) ? PK_TMR : PK_NODE;
  if (FINE && !(bit(x.alive, node) && bit(x.conn, node))) return PK_DROP;
  if (key & 8u) return PK_AE;
  if (FINE && (key & 16u)) return PK_RV;
  return PK_NODE;
}
// which kind a free wave runs (a scheduling policy: results do not depend on it): the fullest.
// (Weighting the AppendEntries queue by 3/4, verdict r5 item 7, re-measured on the queue claim:
// figure_8_unreliable_2c -0.1 / +0.0 %, its crash variant +0.2 / -0.0 %, profiles/r06_ab_queue.txt
// QW3 — not kept.)
DI uint32_t pool_pick(const uint32_t (&n)[PK__N]) {
  uint32_t k = 0;
#pragma unroll
  for (uint32_t q = 1; q < PK__N; q++)
    if (n[q] > n[k]) k = q;
  return k;
}
// the lanes with `pub` append their slots, with their next events' decisions `dc`, to the queue of
// their kind `kd`: one atomic add of the
// kind's tail per kind present, then each lane writes its entry at tail + its rank (a claimer that
// reserved that position before the entry lands waits for its lap tag). The event's global stores
// and the record's LDS writes land before another wave can claim the slot (workgroup scope: the
// waves share the CU's vector L1)
DI void pool_publish(const PoolL& L, bool pub, uint32_t kd, const QDec& dc, uint32_t slot) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
#pragma unroll
  for (uint32_t k = 0; k < PK__N; k++) {
    const uint64_t m = __ballot(pub && kd == k);
    if (!m) continue;
    const uint32_t ld = (uint32_t)__builtin_ctzll(m);
    uint32_t base = 0;
    if (lane64() == ld) base = atomicAdd(&L.qc[2u * k + 1u], (uint32_t)__popcll(m));
    base = rl(base, ld);
    if (pub && kd == k) {
      const uint32_t pos = base + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
      __hip_atomic_store(&L.q[k * PS + (pos & (PS - 1u))], QE::pack(pos, slot, dc), __ATOMIC_RELAXED,
                         __HIP_MEMORY_SCOPE_WORKGROUP);
    }
  }
}

template <uint32_t S, uint32_t NBT>
__global__ void __launch_bounds__(POOL_SLOTS, POOL_WAVES / 4) pool_kernel(Dev Din, uint32_t budget) {
  static_assert(NBT == NB, "one node bound per translation unit");
  static_assert(MR_POOL == 2 ? is_svc(S) : nthr(S) == 0 && !is_svc(S),
                "MR_POOL 1 units run Raft-only test bodies, MR_POOL 2 units the service ones");
  static_assert(EXACT_N, "exact-size instances only (has_pool)");
  static_assert(pool_lds_bytes(pool_max_slots(S, NB)) <= 160u * 1024u,
                "the pool's LDS passes the CU's 160 KiB: a record word (px_record) costs 4 * POOL_SLOTS bytes");
  static_assert(px_count<S>().n == PX_W, "px_record: the record's width does not depend on the scenario");
  Dev D = Din;
  fix_scenario<S>(D);
  const PoolL P = pool_l(D);
  const uint32_t tid = threadIdx.x, lane = lane64();
  X x;
#pragma unroll
  for (uint32_t k = 0; k < CNT__N; k++) x.cnt[k] = 0u;
#ifdef MR_PROF
  if (lane == 0) {
    for (uint32_t k = 0; k < 2 * P__N; k++) s_prof[tid >> 6][k] = 0;
    s_prof[tid >> 6][2 * P__N] = wall_clock64();
  }
  // per kind: iterations, clusters run, wave cycles from the claim to the publish; idle spins,
  // lost claims (wave-uniform, added to D.prof once at the end: no atomics in the loop)
  unsigned long long pst[3 * 8 + 2] = {};  // [kind] iterations, [8 + kind] clusters, [16 + kind] cycles; idle, lost
  const unsigned long long t_start = wall_clock64();
#endif
  if (tid < 2u * PK__N) P.qc[tid] = 0u;
  for (uint32_t i = tid; i < PK__N * PS; i += POOL_SLOTS) P.q[i] = ~0u;  // no lap's tag
  if (tid == 0) *P.live = 0u;
  __syncthreads();
  {  // prologue: slot tid takes its lane of this launch
    x.ls = tid;
    const bool held = launch_begin<S>(D, x);
    uint32_t kd = 0;
    QDec dc{};
    if (held) {
      kd = pool_kind<S>(x, dc);
      px_put<S>(P, x, budget_end(x, budget));
    } else {
      px_clear(P, tid);
    }
    pool_publish(P, held, kd, dc, tid);
    const uint32_t nh = (uint32_t)__popcll(__ballot(held));
    if (lane == 0 && nh) atomicAdd(P.live, nh);
  }
  __syncthreads();
  for (;;) {
    PROF(P_TAIL);
    uint32_t kind;
    QDec dc{};  // the claimed cluster's event, as its publisher decided it
#ifdef MR_PROF
    unsigned long long t_claim = 0;
#endif
    {
      // the kinds' queue lengths: lane k < PK__N reads kind k's {head, tail}
      const unsigned long long ht = lane < PK__N ? qc_pair(P, lane) : 0ull;
      const uint32_t hd = (uint32_t)ht, len = (uint32_t)(ht >> 32) - hd;
      uint32_t nk[PK__N], nall = 0;
#pragma unroll
      for (uint32_t q = 0; q < PK__N; q++) { nk[q] = rl(len, q); nall += nk[q]; }
      if (nall == 0u) {  // every ready cluster is held by another wave, or none is left
        if (__hip_atomic_load(P.live, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) == 0u) break;
#ifdef MR_PROF
        pst[24]++;
#endif
        __builtin_amdgcn_s_sleep(2);  // (1 / 6: +-0.2 %, profiles/r06_ab_fine_sleep.txt)
        continue;
      }
      kind = pool_pick(nk);
      // reserve queue positions [h, h + n) of the kind: the head moves only by this compare-and-
      // swap, the tail only grows, so every reserved position holds (or is about to hold) a
      // published slot
      const uint32_t h = rl(hd, kind), n = nk[kind] < 64u ? nk[kind] : 64u;
      uint32_t won = 0;
      if (lane == 0) won = atomicCAS(&P.qc[2u * kind], h, h + n) == h ? 1u : 0u;
      if (!rl(won, 0)) {  // another wave moved the head first
#ifdef MR_PROF
        pst[25]++;
#endif
        continue;
      }
      PROF(P_SEL);
#ifdef MR_PROF
      t_claim = wall_clock64();
#pragma unroll
      for (uint32_t k = 0; k < PK__N; k++)
        if (kind == k) { pst[k]++; pst[8 + k] += n; }
#endif
      if (lane >= n) continue;
      const uint32_t pos = h + lane, tag = QE::tag_of(pos);
      uint32_t e;
      do {  // the publisher's entry write follows its tail add
        e = __hip_atomic_load(&P.q[kind * PS + (pos & (PS - 1u))], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
      } while (QE::tag(e) != tag);
      x.ls = QE::slot(e);
      dc = QE::dec(e);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
    const uint32_t evend = px_get<S>(P, x);
    if (ap_cont(S) && (x.ap0 >> 31)) {  // not a new event: the current one's applier goes on
      node_event<S>(D, x, false, x.ap0 & 7u, 0u, 0u);
    } else {  // the event the entry names: its key from the record, no second next_event
      run_event<S>(D, x, event_key<S>(x, dc.cls, dc.node, dc.tcli), dc.cls, dc.node, dc.tcli,
                   0u);  // (32-bit keys: no sequence number)
    }
    // the cluster back to the pool: its next kind's queue, or out of the running (a verdict, or
    // the launch's budget reached: the epilogue stores it)
    uint32_t fin = x.code != RUN;
    // (a cluster inside an applier continuation stays in the pool past the launch's budget)
    bool cont = !fin && (x.events < evend || (ap_cont(S) && (x.ap0 >> 31)));
    if (D.stream && fin) {  // streaming: the finished cluster to HBM, the slot takes the next one
      cluster_store<S>(D, x);
      const uint32_t slot = x.ls;
      const bool got_new = cluster_claim<S>(D, x, true);
      x.ls = slot;
      if (got_new) {
        cont = true;
        px_put<S>(P, x, budget_end(x, budget));
      } else {
        px_clear(P, slot);
      }
    } else {
      px_put<S>(P, x, evend);
    }
    const uint32_t kd = cont ? pool_kind<S>(x, dc) : 0u;
    pool_publish(P, cont, kd, dc, x.ls);
#ifdef MR_PROF
    {
      const unsigned long long dt = __shfl(wall_clock64() - t_claim, 0);
#pragma unroll
      for (uint32_t k = 0; k < PK__N; k++)
        if (kind == k) pst[16 + k] += dt;
    }
#endif
    const uint64_t out = __ballot(!cont);
    if (out && lane == (uint32_t)__builtin_ctzll(out)) {
      [[maybe_unused]] const uint32_t was = atomicSub(P.live, (uint32_t)__popcll(out));
#ifdef MR_PROF  // the tail: when the pool's running clusters fell below 3/4, 1/2, 1/8, 1/64
      const uint32_t now_live = was - (uint32_t)__popcll(out);
      const uint32_t cut[4] = {384u, 256u, 64u, 8u};
#pragma unroll
      for (uint32_t q = 0; q < 4; q++)
        if (was >= cut[q] && now_live < cut[q]) atomicAdd(&D.prof[90 + q], wall_clock64() - t_start);
#endif
    }
  }
#ifdef MR_PROF
  PROF(P_TAIL);
  if (lane == 0)
    for (uint32_t k = 0; k < 26; k++) atomicAdd(&D.prof[64 + k], pst[k]);
  if (tid == 0) atomicAdd(&D.prof[94], wall_clock64() - t_start);  // per block: its lifetime
  if (lane == 0)
    for (uint32_t k = 0; k < P__N; k++) {
      atomicAdd(&D.prof[k], s_prof[tid >> 6][k]);
      atomicAdd(&D.prof[32 + k], s_prof[tid >> 6][P__N + k]);
    }
#endif
  __syncthreads();
  // epilogue: every slot's cluster back to HBM (still running: counted, and resumed first by the
  // next launch of a streaming batch)
  x.ls = tid;
  if (px_held(P, tid)) {
    px_get<S>(P, x);
    launch_end<S>(D, x);
  }
  __syncthreads();
  // the lanes' counter sums: reduced in LDS (64-bit), then added to the batch's pool sums
  unsigned long long* const red = reinterpret_cast<unsigned long long*>(P.xr);
  if (tid < CNT__N) red[tid] = 0ull;
  __syncthreads();
#pragma unroll
  for (uint32_t k = 0; k < CNT__N; k++) {
    if (k == CNT_LEADERS || k == CNT_MAX_INDEX || x.cnt[k] == 0u) continue;
    if (cnt_is_max(k)) atomicMax(&red[k], (unsigned long long)x.cnt[k]);
    else atomicAdd(&red[k], (unsigned long long)x.cnt[k]);
  }
  __syncthreads();
  if (tid < CNT__N && red[tid]) {
    if (cnt_is_max(tid)) atomicMax(&D.pcnt[tid], red[tid]);
    else atomicAdd(&D.pcnt[tid], red[tid]);
  }
}

// dynamic LDS above 64 KiB: the kernel attribute is per device, set once per (instance, device)
template <uint32_t S, uint32_t NBT>
hipError_t pool_attr_t() {
  static std::atomic<uint64_t> done{0};  // devices 0..63 that have it
  int dev = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e != hipSuccess) return e;
  const uint64_t bitd = dev < 64 ? 1ull << dev : 0ull;
  if (bitd && (done.load(std::memory_order_acquire) & bitd)) return hipSuccess;
  e = hipFuncSetAttribute((const void*)pool_kernel<S, NBT>, hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)pool_lds_bytes(pool_max_slots(S, NBT)));
  if (e == hipSuccess && bitd) done.fetch_or(bitd, std::memory_order_acq_rel);
  return e;
}
template <uint32_t S, uint32_t NBT>
hipError_t launch_pool_t(const Dev& D, uint32_t budget, hipStream_t s) {
  const uint32_t np = D.lpw * POOL_WAVES;
  dim3 blk(POOL_SLOTS), grd((D.L + np - 1) / np);
  if (const hipError_t e = pool_attr_t<S, NBT>(); e != hipSuccess) return e;
  hipLaunchKernelGGL((pool_kernel<S, NBT>), grd, blk, pool_lds_bytes(D.M), s, D, budget);
  return hipGetLastError();
}
// clusters the pool kernel keeps resident: workgroups per CU x CUs x POOL_SLOTS
template <uint32_t S, uint32_t NBT>
uint32_t pool_capacity_t(int device, uint32_t M) {
  int blocks = 0, cus = 0;
  if (hipSetDevice(device) != hipSuccess || pool_attr_t<S, NBT>() != hipSuccess) return 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&blocks, (const void*)pool_kernel<S, NBT>, POOL_SLOTS,
                                                   pool_lds_bytes(M)) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) != hipSuccess)
    return 0;
  return (uint32_t)blocks * (uint32_t)cus * POOL_SLOTS;
}
