// mr_kv.inc — spawned tester threads (docs/SEMANTICS.md §8) and kvraft on the
// device (§9): the build's completion of the todo!() KV server
// (src/kvraft/server.rs:68-87) and clerk (src/kvraft/client.rs:49-62), the
// generic_test client tasks (src/kvraft/tests.rs:109-131) as resumable tester
// threads, and the clerk hosts of the simulated net. Included by
// mr_kernel.hip after the network and node helpers; thread code is compiled
// into the instances of scenarios that spawn (nthr(S) > 0), KV code into the
// kvraft instances only.

// thread slot s's record: cluster-major (one per-lane base and a word offset per field, instead of
// one loop-invariant field base per field that the compiler keeps in scalar registers)
#define KT(f, s) D.kt32[((size_t)x.c * D.nthr + GI(s, D.nthr, G_KT_SLOT)) * KT_STRIDE + GI(f, KT_STRIDE, G_KT_FIELD)]
#define KVP(d) (D.kv32 + ((size_t)x.c * D.n + GI(d, D.n, G_KV)) * KVREC)

// the scheduler's key of thread slot s, (wake, tid), as one packed pair of words per slot
// (kwk: {tid, wake}, a 64-bit (wake << 32 | tid) in memory order) — a rescan reads every
// slot's key in one batch of 16-B loads instead of two scattered words per slot of kt32
#define KWT(s) D.kwk[((size_t)x.c * kws(D.nthr) + GI(s, kws(D.nthr), G_KWK)) * 2u]
#define KWW(s) D.kwk[((size_t)x.c * kws(D.nthr) + GI(s, kws(D.nthr), G_KWK)) * 2u + 1u]

// the running thread slot's record in registers (thr_step, MR_KT_CACHE): one batch of 16-B loads
// at the step's start instead of a round trip per field read; reads of the slot's fields come from
// it, writes go to it and through to kt32 (other slots and other events read memory)
struct KC {
  uint32_t w[KT_STRIDE];
  uint32_t kvdone;  // the cluster's CS_KVDONE, loaded with the record (no thread step changes it)
};
DI void kc_load(const Dev& D, X& x, uint32_t slot, KC& kc) {
  const uint4* q = reinterpret_cast<const uint4*>(&KT(0, slot));
#pragma unroll
  for (uint32_t i = 0; i < KT_STRIDE / 4; i++) {
    const uint4 v = q[i];
    kc.w[4 * i] = v.x; kc.w[4 * i + 1] = v.y; kc.w[4 * i + 2] = v.z; kc.w[4 * i + 3] = v.w;
  }
}
// the cache of a call chain, or none (`on` is a compile-time constant at every call site; a
// test of the pointer itself does not fold: a private-memory address may be 0)
struct KCR {
  KC* p = nullptr;
  bool on = false;
};
DI uint32_t ktr(const Dev& D, const X& x, KCR kc, uint32_t f, uint32_t s) {
  if (kc.on) return kc.p->w[f];
  return KT(f, s);
}
DI void ktw(const Dev& D, const X& x, KCR kc, uint32_t f, uint32_t s, uint32_t v) {
  if (kc.on) kc.p->w[f] = v;
  KT(f, s) = v;
}
// field f of thread `slot` (the functions below take the cache kc of that slot, or nullptr)
#define KR(f) ktr(D, x, kc, (f), slot)
#define KS(f, v) ktw(D, x, kc, (f), slot, (v))
#define KVDONE() (kc.on ? kc.p->kvdone : CS(CS_KVDONE))

// the earliest runnable spawned thread (slots 1..nthr-1): key (wake, tid); INF = none
DI void thr_rescan(const Dev& D, X& x) {
  uint64_t best = ~0ull;
  uint32_t bs = 0;
  const uint4* kq = reinterpret_cast<const uint4*>(&KWT(0));
  constexpr uint32_t NQ = 12;  // quads per batch of independent loads (up to 24 slots: one batch)
  for (uint32_t q0 = 0; q0 < kws(D.nthr) / 2u; q0 += NQ) {
    uint4 kk[NQ];
#pragma unroll
    for (uint32_t q = 0; q < NQ; q++) kk[q] = q0 + q < kws(D.nthr) / 2u ? kq[q0 + q] : make_uint4(~0u, ~0u, ~0u, ~0u);
#pragma unroll
    for (uint32_t q = 0; q < NQ; q++) {  // slot 0 and the pad slot hold ~0: never below best
      const uint64_t k0 = ((uint64_t)kk[q].y << 32) | kk[q].x, k1 = ((uint64_t)kk[q].w << 32) | kk[q].z;
      if (k0 < best) { best = k0; bs = 2u * (q0 + q); }
      if (k1 < best) { best = k1; bs = 2u * (q0 + q) + 1u; }
    }
  }
  x.cwake = (uint32_t)(best >> 32);
  x.ctid = (uint32_t)best;
  x.cslot = bs;
}

// thread `slot` (tid known) becomes runnable at t
DI void thr_wake_tid(const Dev& D, X& x, uint32_t slot, uint32_t t, uint32_t tid) {
  KWW(slot) = t;
  if (t < x.cwake || (t == x.cwake && tid < x.ctid)) {  // new minimum
    x.cwake = t; x.ctid = tid; x.cslot = slot;
  } else if (slot == x.cslot) {  // the minimum moved later
    thr_rescan(D, x);
  }
}
// thread `slot` becomes runnable at t (slot 0 = the test body)
DI void thr_wake(const Dev& D, X& x, uint32_t slot, uint32_t t) {
  if (slot == 0) { x.twake = t; return; }
  thr_wake_tid(D, x, slot, t, KWT(slot));
}

// task::spawn_local: thread tid in slot `slot`, runnable now
DI void thr_spawn(const Dev& D, X& x, uint32_t slot, uint32_t tid) {
#pragma unroll 1  // a rolled loop: unrolled, its addresses crowd the test body's registers
  for (uint32_t f = 0; f < KT__N; f++) KT(f, slot) = 0u;
  KT(KT_TID, slot) = tid;
  KT(KT_LIVE, slot) = 1u;
  KT(KT_OWN, slot) = slot;
  KWT(slot) = tid;
  CS(CS_NLIVE) = CS(CS_NLIVE) + 1u;
  thr_wake_tid(D, x, slot, x.now, tid);
}

// a spawned thread ended (its last segment record is written): wake a joining test body
DI void thr_finish(const Dev& D, X& x, uint32_t slot) {
  KT(KT_LIVE, slot) = 0u;
  KWW(slot) = INF_T;
  const uint32_t nl = CS(CS_NLIVE) - 1u;
  CS(CS_NLIVE) = nl;
  if (slot == x.cslot) thr_rescan(D, x);
  const uint32_t mj = CS(CS_MJOIN);
  if (mj == slot || mj == JOIN_ANY || (mj == JOIN_ALL && nl == 0u)) x.twake = x.now;
}

// one call_timeout attempt of the clerk of `slot` (client.rs:52-57)
DI void clerk_send(const Dev& D, X& x, uint32_t slot, KCR kc = KCR{}) {
  const uint32_t tag = KR(KT_TAG) + 1u, id = KR(KT_ID);
  uint32_t nctr = KR(KT_NCTR);
  KS(KT_TAG, tag);
  net_send(D, x, CLERK_HOST + slot, nctr, KR(KT_LH), M_KV_REQ, id, tag,
           KR(KT_OP) | (KR(KT_KEY) << 2), KR(KT_SEQ), KR(KT_ELEM), 0ull,
           0u, CLERK_HOST + id);
  KS(KT_NCTR, nctr);
  KS(KT_WAITING, 1u);
  KS(KT_GOT, 0u);
  const uint32_t own = KR(KT_OWN);
  if (kc.on && own == slot && slot != 0)  // a task's own clerk: its tid is cached
    thr_wake_tid(D, x, slot, x.now + 500000u, KR(KT_TID));  // Duration::from_millis(500)
  else
    thr_wake(D, x, own, x.now + 500000u);
}

// ---- the linearizability checker (SEMANTICS §9a): each key is an append / get register;
// per (key, appender) the tester counts the appends called and acknowledged and the largest
// count a returned Get observed, and bounds every Get's observed count by the call / return
// order: at least the appends acknowledged (and the count Gets that returned saw) before it
// was called, at most the appends called before it returned, tokens in order, once each
// keys as the command carries them: 6 bits (kv_request)
#define LINP(k) (D.lin32 + ((size_t)x.c * KV_KEYS + ((k) & (KV_KEYS - 1u))) * (KV_APP * LINW))
DI uint32_t* lin_ent(const Dev& D, X& x, uint32_t key, uint32_t cli) {
  uint32_t* e = LINP(key);
  for (uint32_t a = 0; a < KV_APP; a++, e += LINW) {
    if (e[0] == cli + 1u) return e;
    if (e[0] == 0u) { e[0] = cli + 1u; e[1] = 0u; e[2] = 0u; e[3] = 0u; e[4] = 0u; return e; }
  }
  fail(D, x, MR_FAIL_SIM_CAPACITY);
  return nullptr;
}
// generic_test_linearizability's checker (SEMANTICS §9b), sound with concurrent Puts: per key a
// Put epoch (Puts called) and the Puts pending, per (key, client) the Appends / Puts called and
// the Appends acknowledged that no Put can be ordered after (called with no Put pending, no Put
// called since); a Get of (key, a) is bounded below by that count unless a Put was called while
// it ran, above by the calls
#define LIN15P(k) (D.lin32 + (size_t)x.c * (KV_KEYS * KV_APP * LINW) + KV_KW15 * ((k) & 15u))
DI void lin15_call(const Dev& D, X& x, uint32_t slot, uint32_t op, uint32_t key, uint32_t elem, KCR kc = KCR{}) {
  uint32_t* e = LIN15P(key);
  if (op == KV_PUT) {
    e[30]++;
    e[31]++;
    e[(elem >> 19) % LIN_CLI]++;
    uint4* a = reinterpret_cast<uint4*>(e + 12);  // acked[0..14] = words 15..29
    a[0].w = 0u;
    for (uint32_t w = 1; w < 4; w++) a[w] = make_uint4(0u, 0u, 0u, 0u);
    e[28] = 0u; e[29] = 0u;
  } else if (op == KV_APPEND) {
    e[(elem >> 19) % LIN_CLI]++;
    KS(KT_LEP, e[30]);
    KS(KT_LNP, e[31] == 0u ? 1u : 0u);
  } else {
    KS(KT_LLO, e[LIN_CLI + elem % LIN_CLI]);
    KS(KT_LEP, e[30]);
  }
}
DI void lin15_return(const Dev& D, X& x, uint32_t slot, KCR kc = KCR{}) {
  const uint32_t op = KR(KT_OP), elem = KR(KT_ELEM);
  uint32_t* e = LIN15P(KR(KT_KEY));
  if (op == KV_PUT) { e[31]--; return; }
  if (op == KV_APPEND) {
    if (KR(KT_LNP) && e[30] == KR(KT_LEP)) e[LIN_CLI + (elem >> 19) % LIN_CLI]++;
    return;
  }
  CS(CS_KV_LIN) = CS(CS_KV_LIN) + 1u;
  const uint32_t v = KR(KT_RVAL), n = v & 0xFFFFFFu;
  const uint32_t lo = e[30] == KR(KT_LEP) ? KR(KT_LLO) : 0u;
  if (!(v >> 31) || n < lo || n > e[elem % LIN_CLI]) fail(D, x, MR_FAIL_KV_NOT_LINEARIZABLE);
}
DI void lin_call(const Dev& D, X& x, uint32_t slot, uint32_t op, uint32_t key, uint32_t elem, KCR kc = KCR{}) {
  if (!D.lin32) return;  // kvraft tests only
  if (D.lin15) { lin15_call(D, x, slot, op, key, elem, kc); return; }
  if (op == KV_PUT) {  // a new value: every appender of the key starts again
    uint4* e = reinterpret_cast<uint4*>(LINP(key));
    for (uint32_t w = 0; w < KV_APP * LINW / 4; w++) e[w] = make_uint4(0u, 0u, 0u, 0u);
  } else if (op == KV_APPEND) {
    if (uint32_t* e = lin_ent(D, x, key, elem >> 19)) e[1]++;
  } else if (elem == KV_ALL) {  // appenders 0..4: each one's bound, kept in its entry
    for (uint32_t cli = 0; cli < KV_APP; cli++)
      if (uint32_t* e = lin_ent(D, x, key, cli)) e[4] = e[2] > e[3] ? e[2] : e[3];
  } else if (uint32_t* e = lin_ent(D, x, key, elem)) {
    KS(KT_LLO, e[2] > e[3] ? e[2] : e[3]);
  }
}
DI void lin_return(const Dev& D, X& x, uint32_t slot, KCR kc = KCR{}) {
  if (!D.lin32) return;  // kvraft tests only
  if (D.lin15) { lin15_return(D, x, slot, kc); return; }
  const uint32_t op = KR(KT_OP), key = KR(KT_KEY), elem = KR(KT_ELEM);
  const uint32_t v = KR(KT_RVAL);
  if (op == KV_APPEND) {
    if (uint32_t* e = lin_ent(D, x, key, elem >> 19)) e[2]++;
    return;
  }
  if (op != KV_GET) return;
  CS(CS_KV_LIN) = CS(CS_KV_LIN) + 1u;
  if (elem == KV_ALL) {  // count (5 bits, 31 = saturated) | ok << 5 per appender
    for (uint32_t cli = 0; cli < KV_APP; cli++) {
      uint32_t* e = lin_ent(D, x, key, cli);
      if (!e) return;
      const uint32_t st = (v >> (6 * cli)) & 63u, n = st & 31u;
      if (!(st >> 5) || (n < 31u && (n < e[4] || n > e[1]))) {  // 31 = saturated count
        fail(D, x, MR_FAIL_KV_NOT_LINEARIZABLE);
        return;
      }
      if (n > e[3]) e[3] = n;
    }
    return;
  }
  uint32_t* e = lin_ent(D, x, key, elem);
  if (!e) return;
  const uint32_t n = v & 0xFFFFFFu;
  if (!(v >> 31) || n < KR(KT_LLO) || n > e[1]) { fail(D, x, MR_FAIL_KV_NOT_LINEARIZABLE); return; }
  if (n > e[3]) e[3] = n;
}

DI void clerk_begin(const Dev& D, X& x, uint32_t slot, uint32_t op, uint32_t key, uint32_t elem, KCR kc = KCR{}) {
  KS(KT_SEQ, KR(KT_SEQ) + 1u);
  KS(KT_OP, op); KS(KT_KEY, key); KS(KT_ELEM, elem);
  lin_call(D, x, slot, op, key, elem, kc);
  if (x.code != RUN) return;
  clerk_send(D, x, slot, kc);
}

// the clerk's thread woke (reply or timeout): true = the call is done
DI bool clerk_resume(const Dev& D, X& x, uint32_t slot, KCR kc = KCR{}) {
  KS(KT_WAITING, 0u);
  // as shipped, ClerkCore::call is todo!() once call_timeout returns (kvraft/client.rs:59)
  if (p_null_raft(D, x)) { fail(D, x, MR_FAIL_TODO_RPC_RESULTS); return false; }
  uint32_t lh = KR(KT_LH);
  if (KR(KT_GOT)) {
    const uint32_t st = KR(KT_RSTAT);
    if (st == KV_OK) {
      CS(CS_KV_OPS) = CS(CS_KV_OPS) + 1u;
      lin_return(D, x, slot, kc);
      return x.code == RUN;
    }
    lh = st == KV_WRONG_LEADER ? KR(KT_RHINT) : (lh + 1u) % D.n;
  } else {
    lh = (lh + 1u) % D.n;
  }
  KS(KT_LH, lh);
  clerk_send(D, x, slot, kc);
  return false;
}

// trace record of an event at a clerk host
DI void rec_host(const Dev& D, X& x, uint32_t kind, uint32_t host, uint32_t aux) {
  rec8(D, x, x.now, 0u | (kind << 8) | (host << 16), aux, 0, 0, 0, 0, 0);
}

// KV_REP delivered to clerk host `host` (the clerk of thread slot host - 8), for clerk `clerk`
DI void clerk_deliver(const Dev& D, X& x, uint32_t host, uint32_t src, uint32_t clerk, uint32_t tag,
                      uint32_t st, uint32_t hint, uint32_t val, uint64_t vh, uint32_t seq) {
  const uint32_t slot = host - CLERK_HOST;
  if (!bit(x.conn, src) || link_cut(D, x, src, host)) {
    CADD(CNT_DROP_DELIVER, 1u);
    rec_host(D, x, 16, host, seq);
    return;
  }
  // the slot's record and its scheduler key as one batch of loads (MR_KT_CACHE), not a round
  // trip per condition of the test below
  const bool inb = slot < D.nthr;
  KC c;
  uint32_t ktid = 0;
  if (inb) { kc_load(D, x, slot, c); ktid = KWT(slot); }
  const KCR kc{&c, true};
  if (!inb || !(KR(KT_LIVE) || KR(KT_MCL)) || KR(KT_ID) != clerk || !KR(KT_WAITING) || KR(KT_GOT) ||
      KR(KT_TAG) != tag) {
    CADD(CNT_DROP_STALE, 1u);
    rec_host(D, x, 17, host, seq);
    return;
  }
  KS(KT_GOT, 1u); KS(KT_RSTAT, st); KS(KT_RHINT, hint);
  KS(KT_RVAL, val);
  KS(KT_RVH0, (uint32_t)vh); KS(KT_RVH1, (uint32_t)(vh >> 32));
  const uint32_t own = KR(KT_OWN);
  if (own == slot && slot != 0) thr_wake_tid(D, x, slot, x.now, ktid);  // a task's own clerk
  else thr_wake(D, x, own, x.now);
  rec_host(D, x, M_KV_REP, host, seq);
}

DI void kv_send_rep(const Dev& D, X& x, uint32_t me, NC& d, uint32_t host, uint32_t clerk,
                    uint32_t tag, uint32_t st, uint32_t hint, uint32_t val, uint64_t vh) {
  net_send(D, x, me, d.nctr, host, M_KV_REP, clerk, tag, st, hint, val, vh, 0u);
}

DI uint32_t kv_get_value(const uint32_t* kr, uint32_t elem);
// generic_test_linearizability (§9b): client a's state of a 32-word key record: count | ok << 31
DI uint32_t kv_lin15_state(const uint32_t* kr, uint32_t a) {
  const uint32_t w = a < LIN_CLI ? kr[3 + a] : 0u;
  return (w & 0xFFFu) | ((~w >> 31) << 31);
}

// KV_REQ at server me (server.rs:48-56 handler): reject, or start() and wait for the apply
DI void kv_request(const Dev& D, X& x, uint32_t me, NC& d, uint32_t src, uint32_t clerk,
                   uint32_t tag, uint32_t opkey, uint32_t seq, uint32_t elem, uint2 prange) {
  if (p_null_raft(D, x)) { fail(D, x, MR_FAIL_TODO_APPLY); return; }  // as shipped: kvraft/server.rs:69
  if (f_role(d.f) != R_L) {
    kv_send_rep(D, x, me, d, src, clerk, tag, KV_WRONG_LEADER, (me + 1u) % D.n, 0u, 0ull);
    return;
  }
  if ((p_bugs(D, x) & MR_F_BUG_STALE_READ) && D.lin32 && (opkey & 3u) == KV_GET) {
    // the buggy leader answers from its own state at once: no log entry, no quorum
    const uint32_t key = (opkey >> 2) & 63u, e = elem & 0xFFFFFFu;
    const uint32_t* kr = KVP(me) + KVR_KEYS + (D.lin15 ? KV_KW15 * (key & 15u) : KV_KW * key);
    const uint32_t val = D.lin15 ? kv_lin15_state(kr, e) : kv_get_value(kr, e);
    kv_send_rep(D, x, me, d, src, clerk, tag, KV_OK, me, val, ((uint64_t)kr[1] << 32) | kr[0]);
    return;
  }
  uint32_t* kp = KVP(me);
  const uint32_t pm = kp[KVR_PMASK];  // occupied pending slots
  // (MR_KV_REQ_BATCH: the run start loaded beside it, and the pending payload range the event
  // loaded with the node record — unchanged until the event's sends — instead of a reload)
  const uint32_t lrs0 = LRS(me);
  const uint32_t p = pm == (1u << KV_PEND) - 1u ? KV_PEND : (uint32_t)__builtin_ctz(~pm);  // lowest free
  if (p == KV_PEND) { kv_send_rep(D, x, me, d, src, clerk, tag, KV_FAILED, 0u, 0u, 0ull); return; }
  const uint32_t i = d.last + 1u;
  // command: 1 | op << 61 | key << 55 | clerk << 48 | seq24 << 24 | elem24
  const uint64_t cmd = (1ull << 63) | ((uint64_t)(opkey & 3u) << 61) |
                       ((uint64_t)((opkey >> 2) & 63u) << 55) | ((uint64_t)clerk << 48) |
                       ((uint64_t)(seq & 0xFFFFFFu) << 24) | (elem & 0xFFFFFFu);
  if (i - d.snap > D.log_cap) { fail(D, x, MR_FAIL_SIM_CAPACITY); return; }  // start(), raft.rs:238-244
  guard_log_write(D, x, me, d.pexp, i, prange.x, prange.y);
  const uint32_t rs = d.term == d.lastt ? lrs0 : i;  // run start (le_at)
  D.log[logi(D, x, me, i)] = LE{d.term, rs, cmd};
  LRS(me) = rs;
  CADD(CNT_LOG_WRITES, 1u);
  d.last = i;
  d.lastt = d.term;
  CMAX(CNT_MAX_LOG, i - d.snap);
  uint4* pp = reinterpret_cast<uint4*>(kp + KVR_PEND + 8 * p);
  pp[0] = make_uint4(i, clerk | (src << 16), seq & 0xFFFFFFu, tag);
  pp[1] = make_uint4(0u, 0u, 0u, 0u);
  kp[KVR_PMASK] = pm | (1u << p);
}

// ---- shard_ctrler (SEMANTICS §10)
#define CFGP(s, j) (D.cfg32 + (((size_t)x.c * D.n + GI(s, D.n, G_CFG_S)) * CFG_CAP + GI(j, CFG_CAP, G_CFG_J)) * CFGW)  // server s, config j
#define OPP(id) (D.op32 + ((size_t)x.c * OP_CAP + GI(id, OP_CAP, G_OP)) * OPW)

// every shard assigned, group loads differ by <= 1, a shard moves only off a
// removed or over-target group (the same rule as the oracle's ctl_rebalance)
DI void ctl_rebalance(uint32_t* c) {
  const uint32_t ng = c[CF_NG];
  if (ng == 0) {
    for (uint32_t j = 0; j < N_SHARDS; j++) c[CF_SHARDS + j] = 0u;
    return;
  }
  uint32_t cnt[CFG_G];
  for (uint32_t g = 0; g < ng; g++) cnt[g] = 0;
  for (uint32_t j = 0; j < N_SHARDS; j++) {
    const uint32_t sg = c[CF_SHARDS + j];
    uint32_t g = 0;
    while (g < ng && c[CF_GID + g] != sg) g++;
    if (g < ng) cnt[g]++;
    else c[CF_SHARDS + j] = 0u;
  }
  const uint32_t base = N_SHARDS / ng, extra = N_SHARDS % ng;
  uint32_t tgt[CFG_G];
  for (uint32_t g = 0; g < ng; g++) {  // base + 1 for the most-loaded groups (ties: smaller gid)
    uint32_t r = 0;
    for (uint32_t h = 0; h < ng; h++) r += (cnt[h] > cnt[g] || (cnt[h] == cnt[g] && h < g)) ? 1u : 0u;
    tgt[g] = base + (r < extra ? 1u : 0u);
  }
  for (uint32_t g = 0; g < ng; g++)  // release over-target shards, highest shard first
    for (int j = N_SHARDS - 1; j >= 0 && cnt[g] > tgt[g]; j--)
      if (c[CF_SHARDS + j] == c[CF_GID + g]) { c[CF_SHARDS + j] = 0u; cnt[g]--; }
  for (uint32_t j = 0; j < N_SHARDS; j++) {  // free shards, ascending, to the first group below target
    if (c[CF_SHARDS + j] != 0u) continue;
    uint32_t g = 0;
    while (cnt[g] >= tgt[g]) g++;
    c[CF_SHARDS + j] = c[CF_GID + g];
    cnt[g]++;
  }
}

// ShardInfo::apply (shard_ctrler/server.rs:8-19, the build's completion) at server me;
// returns the output (Query: index of the answered config in me's store)
DI uint32_t ctl_apply(const Dev& D, X& x, uint32_t me, uint32_t clerk, uint32_t seq, uint32_t id) {
  const uint32_t* op = OPP(id);
  uint32_t* kp = KVP(me);
  const uint32_t nc = kp[KVR_NCFG], type = op[OP_TYPE];
  if (type == CT_QUERY) return op[OP_A] >= nc ? nc - 1u : op[OP_A];
  if (seq <= kp[KVR_DEDUP + clerk]) return 0u;  // duplicate
  kp[KVR_DEDUP + clerk] = seq;
  if (nc >= CFG_CAP) { fail(D, x, MR_FAIL_SIM_CAPACITY); return 0u; }
  uint32_t* c = CFGP(me, nc);
  const uint32_t* p = CFGP(me, nc - 1u);
  for (uint32_t w = 0; w < CFGW; w++) c[w] = p[w];
  c[CF_NUM] = nc;
  const uint32_t nk = op[OP_NG];
  if (type == CT_JOIN) {
    for (uint32_t k = 0; k < nk; k++) {
      const uint32_t gid = op[OP_GID + k], ad = op[OP_ADDR + k], ng = c[CF_NG];
      uint32_t g = 0;
      while (g < ng && c[CF_GID + g] < gid) g++;
      if (g < ng && c[CF_GID + g] == gid) { c[CF_ADDR + g] = ad; continue; }
      if (ng >= CFG_G) { fail(D, x, MR_FAIL_SIM_CAPACITY); return 0u; }
      for (uint32_t h = ng; h > g; h--) { c[CF_GID + h] = c[CF_GID + h - 1]; c[CF_ADDR + h] = c[CF_ADDR + h - 1]; }
      c[CF_GID + g] = gid; c[CF_ADDR + g] = ad; c[CF_NG] = ng + 1u;
    }
    ctl_rebalance(c);
  } else if (type == CT_LEAVE) {
    for (uint32_t k = 0; k < nk; k++) {
      const uint32_t gid = op[OP_GID + k], ng = c[CF_NG];
      uint32_t g = 0;
      while (g < ng && c[CF_GID + g] != gid) g++;
      if (g == ng) continue;
      for (uint32_t h = g; h + 1 < ng; h++) { c[CF_GID + h] = c[CF_GID + h + 1]; c[CF_ADDR + h] = c[CF_ADDR + h + 1]; }
      c[CF_NG] = ng - 1u;
    }
    ctl_rebalance(c);
  } else if (op[OP_A] < N_SHARDS) {
    c[CF_SHARDS + op[OP_A]] = op[OP_B];  // Move
  }
  kp[KVR_NCFG] = nc + 1u;
  return 0u;
}

DI uint32_t ndig(uint32_t v) { uint32_t d = 1; while (v >= 10u) { v /= 10u; d++; } return d; }
// a Put value token: 0 = "", t < 2^20 = the decimal string of t - 1, else one letter
DI uint32_t put_len(uint32_t t) { return t == 0 ? 0u : t < (1u << 20) ? ndig(t - 1u) : 1u; }
// appender `cli` of key record kr: count | ok << 31
DI uint32_t kv_app_state(const uint32_t* kr, uint32_t cli) {
  uint32_t st = 1u << 31;
#pragma unroll
  for (uint32_t a = 0; a < KV_APP; a++) {
    const uint32_t w = kr[3 + a];
    if ((w & 0xFFu) == cli + 1u) st = ((w >> 8) & 0x7FFFFFu) | ((~w >> 31) << 31);
  }
  return st;
}

// a Get's reply value: the state of appender elem, or (KV_ALL) of appenders 0..4 packed as
// count (5 bits, saturating at 31) | ok << 5 each
DI uint32_t kv_get_value(const uint32_t* kr, uint32_t elem) {
  if (elem != KV_ALL) return kv_app_state(kr, elem);
  uint32_t out = 0;
#pragma unroll
  for (uint32_t c = 0; c < KV_APP; c++) {
    const uint32_t st = kv_app_state(kr, c), n = st & 0xFFFFFFu;
    out |= ((n > 31u ? 31u : n) | ((st >> 31) ? 32u : 0u)) << (6 * c);
  }
  return out;
}

// Kv::apply of generic_test_linearizability (SEMANTICS §9b): Put / Append of token
// "x {cli} {j} y" (elem = cli << 19 | j) on a 32-word key record; a Get answers client elem's
// state. out / outh: the Get's value and hash.
DI void kv_apply_lin15(const Dev& D, X& x, uint32_t me, uint32_t* kp, uint32_t key, uint32_t op,
                       uint32_t clerk, uint32_t seq, uint32_t elem, uint32_t& out, uint64_t& outh) {
  uint32_t* kr = kp + KVR_KEYS + KV_KW15 * key;
  const uint32_t cli = elem >> 19, j = elem & 0x7FFFFu;
  // what the entry reads — the key record's first quad, the clerk's dedup word, and the state
  // word of the client it names (a Get: elem; a Put / Append: its token's client) — as one batch
  // of independent loads instead of a round trip per decision
  const uint32_t cs = op == KV_GET ? elem : cli;
  const uint4 k0 = reinterpret_cast<const uint4*>(kr)[0];  // hash lo, hi, length, client 0
  const uint32_t ded = kp[KVR_DEDUP + clerk];
  const uint32_t ws = cs < LIN_CLI ? kr[3 + cs] : 0u;
  if (op == KV_GET) {
    outh = ((uint64_t)k0.y << 32) | k0.x;
    out = (ws & 0xFFFu) | ((~ws >> 31) << 31);
    return;
  }
  if (!(seq > ded || (p_bugs(D, x) & MR_F_BUG_NO_DEDUP))) return;  // a duplicate
  if (cli >= LIN_CLI) { fail(D, x, MR_FAIL_SIM_CAPACITY); return; }
  const uint32_t len = 5u + ndig(cli) + ndig(j);
  if (op == KV_PUT) {  // the value is this one token
    uint4* q = reinterpret_cast<uint4*>(kr);
    q[0] = make_uint4(elem + 1u, 0u, len, 0u);
    for (uint32_t w = 1; w < 5; w++) q[w] = make_uint4(0u, 0u, 0u, 0u);
    kr[3 + cli] = 1u | (j << 12);
  } else {
    const uint32_t w = ws, n = w & 0xFFFu;
    if (!(w >> 31) && (n == 0u || j > ((w >> 12) & 0x7FFFFu))) {
      if (n + 1u > 0xFFFu) { fail(D, x, MR_FAIL_SIM_CAPACITY); return; }
      kr[3 + cli] = (n + 1u) | (j << 12);
    } else {
      kr[3 + cli] = w | (1u << 31);
    }
    const uint64_t h = (((uint64_t)k0.y << 32) | k0.x) * KV_HP + elem + 1u;
    kr[0] = (uint32_t)h; kr[1] = (uint32_t)(h >> 32);
    kr[2] = k0.z + len;
  }
  kp[KVR_DEDUP + clerk] = seq;
}

// Server::apply + Kv::apply (or ShardInfo::apply) of log entry i (value v) at
// server me; values are token sequences kept as (hash, length, appenders)
// (SEMANTICS §9); answers are marked ready and sent at the end of the event (kv_flush)
// pm: the server's occupied pending slots (KVR_PMASK; constant while its applier runs: slots
// are taken by kv_request and freed by kv_flush, both outside it)
template <bool CTRL>
DI void kv_apply(const Dev& D, X& x, uint32_t me, uint32_t i, uint64_t v, uint32_t& ready, uint32_t pm) {
  const uint32_t op = (uint32_t)(v >> 61) & 3u, key = (uint32_t)(v >> 55) & 63u;
  const uint32_t clerk = (uint32_t)(v >> 48) & 127u, seq = (uint32_t)(v >> 24) & 0xFFFFFFu;
  const uint32_t elem = (uint32_t)v & 0xFFFFFFu;
  uint32_t* kp = KVP(me);
  uint32_t* kr = kp + KVR_KEYS + KV_KW * key;
  uint32_t out = 0;
  uint64_t outh = 0;
  bool query = op == KV_GET;
  if (CTRL) {  // elem = the operation's id
    out = ctl_apply(D, x, me, clerk, seq, elem);
    if (x.code != RUN) return;
    query = OPP(elem)[OP_TYPE] == CT_QUERY;
  } else {
    if (D.lin15) {  // generic_test_linearizability (SEMANTICS §9b): 32-word key records
      kv_apply_lin15(D, x, me, kp, key & 15u, op, clerk, seq, elem, out, outh);
      if (x.code != RUN) return;
    } else {
      // the key record {hash lo, hash hi, length, appenders 0..4} in registers
      const uint4 kra = reinterpret_cast<const uint4*>(kr)[0];
      const uint4 krb = reinterpret_cast<const uint4*>(kr)[1];
      const uint32_t pded = kp[KVR_DEDUP + clerk];
      uint32_t k[KV_KW] = {kra.x, kra.y, kra.z, kra.w, krb.x, krb.y, krb.z, krb.w};
      if (op == KV_GET) {
        outh = ((uint64_t)k[1] << 32) | k[0];
        out = kv_get_value(k, elem);
      } else if (seq > pded || (p_bugs(D, x) & MR_F_BUG_NO_DEDUP)) {
        if (op == KV_PUT) {  // elem = the value's token (0 = "")
          const uint64_t h = elem ? (elem + 1ull) * 0x9E3779B97F4A7C15ull : 0ull;
          reinterpret_cast<uint4*>(kr)[0] = make_uint4((uint32_t)h, (uint32_t)(h >> 32), put_len(elem), 0u);
          reinterpret_cast<uint4*>(kr)[1] = make_uint4(0u, 0u, 0u, 0u);
        } else {  // Append of token "x {cli} {j} y": elem = cli << 19 | j
          const uint32_t cli = elem >> 19, j = elem & 0x7FFFFu;
          uint32_t a = KV_APP, w = 0;  // the first appender slot that is cli's or empty
#pragma unroll
          for (int q = KV_APP - 1; q >= 0; q--) {
            const uint32_t wq = k[3 + q];
            if ((wq & 0xFFu) == cli + 1u || (wq & 0xFFu) == 0u) { a = (uint32_t)q; w = wq; }
          }
          if (a == KV_APP) { fail(D, x, MR_FAIL_SIM_CAPACITY); return; }
          const uint32_t n = (w >> 8) & 0xFFFFFFu;
          kr[3 + a] = (!(w >> 31) && n == j) ? ((cli + 1u) | ((n + 1u) << 8))
                                             : ((cli + 1u) | (n << 8) | (1u << 31));
          const uint64_t h = (((uint64_t)k[1] << 32) | k[0]) * KV_HP + elem + 1u;
          kr[0] = (uint32_t)h; kr[1] = (uint32_t)(h >> 32);
          kr[2] = k[2] + 5u + ndig(cli) + ndig(j);
        }
        kp[KVR_DEDUP + clerk] = seq;
      }
    }
  }
  if (!CTRL && x.c < D.trace_clusters && i < D.trace_cap) {  // mr_trace_applies: first applier
    const uint32_t* kh = kp + KVR_KEYS + (D.lin15 ? KV_KW15 * (key & 15u) : KV_KW * key);
    uint64_t* p = D.tapp + ((size_t)x.c * D.trace_cap + i) * 2u;
    if (!p[0]) { p[0] = v; p[1] = ((uint64_t)kh[1] << 32) | kh[0]; }
  }
  PROF(P_AP_KV);
  for (uint32_t m = pm; m; m &= m - 1u) {  // followers hold none: no loads
    const uint32_t p = (uint32_t)__builtin_ctz(m);
    uint4* pp = reinterpret_cast<uint4*>(kp + KVR_PEND + 8 * p);
    uint4 e = pp[0];
    if (e.x != i || (e.y >> 8) & 1u) continue;
    const bool ok = (e.y & 0xFFu) == clerk && e.z == seq;
    e.y |= (1u << 8) | ((ok ? KV_OK : KV_FAILED) << 9);
    pp[0] = e;
    const bool val = ok && query;
    pp[1] = make_uint4(val ? out : 0u, val ? (uint32_t)outh : 0u, val ? (uint32_t)(outh >> 32) : 0u, 0u);
    ready |= 1u << p;
  }
  PROF(P_AP_PEND);
}

// ---- KV snapshots (maxraftstate): the persisted snapshot of server s, a ring entry
#define KVSP(s) (D.kvs32 + ((size_t)x.c * D.n + GI(s, D.n, G_KV)) * KVS_W)
#define KRP(r) (D.kring + ((size_t)x.c * KV_RING + (r)) * KRW)

// snapshot image (dedup[128] + key records) -> live state (a restarted server, start1)
DI void kv_state_put(const Dev& D, X& x, uint32_t me, const uint32_t* src) {
  uint32_t* kp = KVP(me);
  const uint4* s = reinterpret_cast<const uint4*>(src);
  for (uint32_t w = 0; w < KVS_W / 4; w += 4) {
    uint4* live = reinterpret_cast<uint4*>(kp) +
                  (w < MAX_CLERKS / 4 ? KVR_DEDUP / 4 + w : KVR_KEYS / 4 + (w - MAX_CLERKS / 4));
    uint4 v[4];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) v[k] = s[w + k];
#pragma unroll
    for (uint32_t k = 0; k < 4; k++) live[k] = v[k];
  }
}

// the service snapshots at applied index i (Raft's part is done by the caller): the
// persisted KV snapshot and the ring entry (equal states at equal indices, or APPLY_MISMATCH).
// The 640-word image moves in chunks of KV_CHUNK quads (kv_chunk(S): 4 or 8; InstallSnapshot's
// copy 4) whose loads issue together: a chunk costs one round trip where a quad at a time cost
// one each (the image is 160 quads)
DI const uint4* kv_image_src(const uint32_t* kp, uint32_t w) {  // image quad w of the live state
  const uint4* q = reinterpret_cast<const uint4*>(kp);
  return w < MAX_CLERKS / 4 ? q + KVR_DEDUP / 4 + w : q + KVR_KEYS / 4 + (w - MAX_CLERKS / 4);
}
template <uint32_t KV_CHUNK>
DI void kv_snapshot(const Dev& D, X& x, uint32_t me, uint32_t i) {
  static_assert(MAX_CLERKS / 4 % KV_CHUNK == 0 && KVS_W / 4 % KV_CHUNK == 0, "whole chunks");
  const uint32_t* kp = KVP(me);
  uint4* sp = reinterpret_cast<uint4*>(KVSP(me));
  uint32_t* rp = KRP((i / KV_SNAP_EVERY) % KV_RING);
  uint4* b = reinterpret_cast<uint4*>(rp + 4);
  const bool cmp = rp[0] == i;
  bool same = true;
  // (round 6: the next chunk's loads issued before this chunk's stores, -14 % on the snapshotting
  // 15-client 3B body, profiles/r06_ab_kv47.txt — not kept)
  for (uint32_t w = 0; w < KVS_W / 4; w += KV_CHUNK) {
    const uint4* src = kv_image_src(kp, w);
    uint4 v[KV_CHUNK], q[KV_CHUNK];
#pragma unroll
    for (uint32_t k = 0; k < KV_CHUNK; k++) v[k] = src[k];
#pragma unroll
    for (uint32_t k = 0; k < KV_CHUNK; k++) q[k] = cmp ? b[w + k] : make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
    for (uint32_t k = 0; k < KV_CHUNK; k++) sp[w + k] = v[k];
#pragma unroll
    for (uint32_t k = 0; k < KV_CHUNK; k++) {
      if (cmp) same = same && v[k].x == q[k].x && v[k].y == q[k].y && v[k].z == q[k].z && v[k].w == q[k].w;
      else b[w + k] = v[k];
    }
  }
  if (cmp) {
    if (!same) fail(D, x, MR_FAIL_APPLY_MISMATCH);
  } else {
    rp[0] = i;
  }
}

// InstallSnapshot(idx) at server me: the KV state of index idx from the ring; requests
// pending at or below idx are answered FAILED (their entries are never applied here)
// (its copy stays at 4 quads per chunk for every body: 8, as the 15-client body's snapshot copy,
// measured -0.9 % there, profiles/r06_ab_ki.txt)
DI void kv_install(const Dev& D, X& x, uint32_t me, uint32_t idx, uint32_t& ready) {
  constexpr uint32_t KV_CHUNK = 4;
  const uint32_t* rp = KRP((idx / KV_SNAP_EVERY) % KV_RING);
  if (rp[0] != idx) { fail(D, x, MR_FAIL_SIM_CAPACITY); return; }
  const uint4* a = reinterpret_cast<const uint4*>(rp + 4);
  uint4* sp = reinterpret_cast<uint4*>(KVSP(me));
  uint32_t* kpw = KVP(me);
  for (uint32_t w = 0; w < KVS_W / 4; w += KV_CHUNK) {  // the persisted snapshot and the live state
    uint4* live = const_cast<uint4*>(kv_image_src(kpw, w));
    uint4 v[KV_CHUNK];
#pragma unroll
    for (uint32_t k = 0; k < KV_CHUNK; k++) v[k] = a[w + k];
#pragma unroll
    for (uint32_t k = 0; k < KV_CHUNK; k++) { sp[w + k] = v[k]; live[k] = v[k]; }
  }
  uint32_t* kp = KVP(me);
  for (uint32_t m = kp[KVR_PMASK]; m; m &= m - 1u) {
    const uint32_t p = (uint32_t)__builtin_ctz(m);
    uint4* pp = reinterpret_cast<uint4*>(kp + KVR_PEND + 8 * p);
    uint4 e = pp[0];
    if (e.x == 0u || ((e.y >> 8) & 1u) || e.x > idx) continue;
    e.y |= (1u << 8) | (KV_FAILED << 9);
    pp[0] = e;
    pp[1] = make_uint4(0u, 0u, 0u, 0u);
    ready |= 1u << p;
  }
}

// answered requests of server me, in slot order, after the event's Raft sends. ready: the slots
// answered in this event (kv_apply / kv_install; MR_KV_RMASK), so only they are read — not a round
// trip per occupied slot to find them
DI void kv_flush(const Dev& D, X& x, uint32_t me, NC& d, uint32_t ready) {
  uint32_t* kp = KVP(me);
  uint32_t pm = kp[KVR_PMASK];
  for (uint32_t m = ready; m; m &= m - 1u) {
    const uint32_t p = (uint32_t)__builtin_ctz(m);
    uint4* pp = reinterpret_cast<uint4*>(kp + KVR_PEND + 8 * p);
    const uint4 e = pp[0];
    const uint4 r = pp[1];
    pp[0] = make_uint4(0u, 0u, 0u, 0u);
    pm &= ~(1u << p);
    kp[KVR_PMASK] = pm;
    kv_send_rep(D, x, me, d, e.y >> 16, e.y & 0xFFu, e.w, (e.y >> 9) & 3u, me, r.x,
                ((uint64_t)r.z << 32) | r.y);  // hint = server
    if (x.code != RUN) return;
  }
}

// client task of generic_test (kvraft/tests.rs:109-131) in slot `slot`, one segment
DI void kv_client_step(const Dev& D, X& x, uint32_t slot, KCR kc = KCR{}) {
  uint32_t pc = KR(KT_PC), j = KR(KT_J);
  const uint32_t cli = KR(KT_CLI), tid = KR(KT_TID);
  bool fin = false;
  for (int guard = 0;; guard++) {
    if (guard > 64) { fail(D, x, MR_FAIL_SIM_BAD_PROGRAM); return; }
    if (pc == 0) {  // ck.put(&key, "")
      clerk_begin(D, x, slot, KV_PUT, cli, 0u, kc);
      KS(KT_HL0, 0u); KS(KT_HL1, 0u);
      pc = 1;
      break;
    }
    if (pc == 2) {
      if (KVDONE()) { fin = true; break; }
      const uint32_t tc = KR(KT_TCTR);
      KS(KT_TCTR, tc + 1u);
      uint32_t w0, w1;
      philox(D, x, tc, tid, ST_TESTER, w0, w1);
      if (w0 < 0x80000000u) {  // gen_bool(0.5): append "x {cli} {j} y"; last += &nv
        const uint32_t e = (cli << 19) | j;
        const uint64_t h = (((uint64_t)KR(KT_HL1) << 32) | KR(KT_HL0)) * KV_HP + e + 1u;
        KS(KT_HL0, (uint32_t)h); KS(KT_HL1, (uint32_t)(h >> 32));
        clerk_begin(D, x, slot, KV_APPEND, cli, e, kc);
        pc = 3;
      } else {
        clerk_begin(D, x, slot, KV_GET, cli, cli, kc);
        pc = 4;
      }
      break;
    }
    if (!clerk_resume(D, x, slot, kc)) break;  // pc 1, 3, 4: the call's reply or timeout
    if (x.code != RUN) return;
    if (pc == 3) j++;
    if (pc == 4) CS(CS_KV_CHECKED) = CS(CS_KV_CHECKED) + 1u;
    if (pc == 4 && (KR(KT_RVH0) != KR(KT_HL0) || KR(KT_RVH1) != KR(KT_HL1))) {
      fail(D, x, MR_FAIL_KV_GET_WRONG);  // kvraft/tests.rs:127
      return;
    }
    pc = 2;
  }
  if (x.code != RUN) return;
  rec_simple(D, x, 2, tid & 0xFFu);
  KS(KT_PC, pc);
  KS(KT_J, j);
  if (fin) thr_finish(D, x, slot);
}

// client task of generic_test_linearizability (SEMANTICS §9b) in slot `slot`, one segment:
// random key, Append (1/2), Put (1/20) or Get reporting a random client (the rest)
DI uint32_t thr_range(const Dev& D, X& x, uint32_t slot, uint32_t lo, uint32_t hi, KCR kc = KCR{}) {
  const uint32_t tc = KR(KT_TCTR);
  KS(KT_TCTR, tc + 1u);
  uint32_t w0, w1;
  philox(D, x, tc, KR(KT_TID), ST_TESTER, w0, w1);
  return u_range(w0, lo, hi);
}
DI void lin_client_step(const Dev& D, X& x, uint32_t slot, KCR kc = KCR{}) {
  uint32_t pc = KR(KT_PC), j = KR(KT_J);
  const uint32_t cli = KR(KT_CLI), tid = KR(KT_TID);
  bool fin = false;
  for (int guard = 0;; guard++) {
    if (guard > 64) { fail(D, x, MR_FAIL_SIM_BAD_PROGRAM); return; }
    if (pc == 0) {
      if (KVDONE()) { fin = true; break; }
      const uint32_t key = thr_range(D, x, slot, 0, LIN_CLI, kc), e = (cli << 19) | j;
      if (thr_range(D, x, slot, 0, 1000, kc) < 500u) {
        clerk_begin(D, x, slot, KV_APPEND, key, e, kc);
        pc = 1;
      } else if (thr_range(D, x, slot, 0, 1000, kc) < 100u) {
        clerk_begin(D, x, slot, KV_PUT, key, e, kc);
        pc = 1;
      } else {
        clerk_begin(D, x, slot, KV_GET, key, thr_range(D, x, slot, 0, LIN_CLI, kc), kc);
        pc = 2;
      }
      break;
    }
    if (!clerk_resume(D, x, slot, kc)) break;  // pc 1, 2: the call's reply or timeout
    if (x.code != RUN) return;
    if (pc == 1) j++;
    pc = 0;
  }
  if (x.code != RUN) return;
  rec_simple(D, x, 2, tid & 0xFFu);
  KS(KT_PC, pc);
  KS(KT_J, j);
  if (fin) thr_finish(D, x, slot);
}

// the partitioner task of generic_test (kvraft/tests.rs:135-157): while !done,
// shuffle `all` (rand 0.8 SliceRandom::shuffle), split at gen_range(0..n),
// partition, sleep RAFT_ELECTION_TIMEOUT + gen_range(0..200) ms
DI void part_step(const Dev& D, X& x, uint32_t slot, KCR kc = KCR{}) {
  const uint32_t tid = KR(KT_TID);
  if (KVDONE()) {
    rec_simple(D, x, 2, tid & 0xFFu);
    thr_finish(D, x, slot);
    return;
  }
  uint32_t perm = KR(KT_PERM);
  for (uint32_t i = D.n - 1; i >= 1; i--) {  // swap(i, gen_range(0..i+1))
    const uint32_t j = thr_range(D, x, slot, 0, i + 1, kc);
    const uint32_t ai = (perm >> (4 * i)) & 15u, aj = (perm >> (4 * j)) & 15u;
    perm = (perm & ~(15u << (4 * i)) & ~(15u << (4 * j))) | (aj << (4 * i)) | (ai << (4 * j));
  }
  KS(KT_PERM, perm);
  const uint32_t k = thr_range(D, x, slot, 0, D.n, kc);
  uint32_t left = 0;
  for (uint32_t i = 0; i < k; i++) left |= 1u << ((perm >> (4 * i)) & 15u);
  // t.partition(left, right) with left | right = all: link i~j up iff same side
  uint32_t cut0 = 0, cut1 = 0;
  for (uint32_t i = 0; i < D.n; i++)
    for (uint32_t j = 0; j < D.n; j++)
      if (bit(left, i) != bit(left, j)) {
        if (i < 4) cut0 |= 1u << (8 * i + j);
        else cut1 |= 1u << (8 * (i - 4) + j);
      }
  CS(CS_CUT) = cut0; CS(CS_CUT + 1) = cut1;
  const uint32_t ms = thr_range(D, x, slot, 0, 200, kc);
  rec_simple(D, x, 2, tid & 0xFFu);
  thr_wake(D, x, slot, x.now + 1000000u + 1000u * ms);
}

// ---- kvraft tests with their own bodies (kvraft/tests.rs:240-342, 396-492)
DI void set_ccut(const Dev& D, X& x, uint32_t k, uint32_t to) {  // connect_client(k, to)
  const uint32_t w = CS_CCUT + (k >> 2), sh = 8u * (k & 3u);
  CS(w) = (CS(w) & ~(0xFFu << sh)) | ((~to & 0xFFu) << sh);
}
// make_client(to) for the test body (slot 0, or slot k != 0 that is not a thread)
DI void main_clerk(const Dev& D, X& x, uint32_t k, uint32_t id, uint32_t to) {
  for (uint32_t f = KT_ID; f <= KT_ELEM; f++) KT(f, k) = 0u;
  KT(KT_RVH0, k) = 0u; KT(KT_RVH1, k) = 0u;
  KT(KT_ID, k) = id; KT(KT_OWN, k) = 0u; KT(KT_MCL, k) = k != 0 ? 1u : 0u;
  set_ccut(D, x, k, to);
}
// task::spawn_local of a task over a fresh clerk `id` of its slot: `cnt` calls
DI void kv_task_spawn(const Dev& D, X& x, uint32_t slot, uint32_t tid, uint32_t kind, uint32_t cli,
                      uint32_t id, uint32_t op, uint32_t key, uint32_t elem, uint32_t cnt) {
  thr_spawn(D, x, slot, tid);
  KT(KT_KIND, slot) = kind; KT(KT_CLI, slot) = cli; KT(KT_ID, slot) = id;
  KT(KT_TOP, slot) = op; KT(KT_TKEY, slot) = key; KT(KT_TELEM, slot) = elem; KT(KT_TCNT, slot) = cnt;
}
// a one-key appender (kind 2, kvraft/tests.rs:255-262) or a single-call task (kind 3, :309-314)
DI void kv_task_step(const Dev& D, X& x, uint32_t slot, KCR kc = KCR{}) {
  const uint32_t tid = KR(KT_TID);
  uint32_t j = KR(KT_J);
  if (KR(KT_PC) == 1u) {
    if (!clerk_resume(D, x, slot, kc)) {
      if (x.code == RUN) rec_simple(D, x, 2, tid & 0xFFu);
      return;
    }
    j++;
    KS(KT_J, j);
    KS(KT_PC, 0u);
  }
  if (j < KR(KT_TCNT)) {
    const uint32_t elem = KR(KT_KIND) == 2u ? (KR(KT_CLI) << 19) | j : KR(KT_TELEM);
    clerk_begin(D, x, slot, KR(KT_TOP), KR(KT_TKEY), elem, kc);
    if (x.code != RUN) return;
    KS(KT_PC, 1u);
    rec_simple(D, x, 2, tid & 0xFFu);
    return;
  }
  rec_simple(D, x, 2, tid & 0xFFu);
  thr_finish(D, x, slot);
}
// the persisted KV snapshot's size (snapshot_size(), kvraft/tester.rs:69-76; SEMANTICS §9)
DI uint32_t kv_snap_size(const Dev& D, X& x, uint32_t s) {
  const uint32_t* sp = KVSP(s);
  uint32_t sz = 16;
  for (uint32_t c = 0; c < MAX_CLERKS; c++) sz += sp[c] ? 16u : 0u;
  const uint32_t nk = D.lin15 ? LIN_CLI : KV_KEYS, kw = D.lin15 ? KV_KW15 : KV_KW;
  for (uint32_t key = 0; key < nk; key++) {
    const uint32_t* kr = sp + MAX_CLERKS + kw * key;
    if (kr[0] | kr[1] | kr[2]) sz += 16u + (key < 50u ? ndig(key) : 1u) + kr[2];
  }
  return sz;
}

// task::spawn_local of client `cli` as thread tid in slot `slot`, with a new clerk (id = tid)
DI void kv_spawn(const Dev& D, X& x, uint32_t slot, uint32_t tid, uint32_t cli) {
  thr_spawn(D, x, slot, tid);
  KT(KT_CLI, slot) = cli;
  KT(KT_ID, slot) = tid;
}
