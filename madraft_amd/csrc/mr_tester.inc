// mr_tester.inc — the tester (src/raft/tester.rs) and the test bodies
// (src/raft/tests.rs) as resumable state machines for the step kernel
// (mr_kernel.hip, one lane per cluster; the lanes of a wave cooperate only in the
// applier, DESIGN.md §6.5). Included after the kernel defines its cluster
// context X, philox(), fail(), TV(k) (the u64 script arrays) and the tester
// primitives that touch nodes (t_started, t_connected, t_conn, t_crash1,
// t_start1, t_start, t_new, t_term, t_log_size, t_check_terms,
// t_check_no_leader, t_end, nd_role, nd_term, n_committed). Everything here is
// control flow over those primitives.

// a tester loop that calls start() on every server runs the start path once per server index
// that is some lane's leader; walking each lane's own leaders runs it once per wave
// (t_start_round, one_step; A/B in DESIGN.md §6.8)
// the same walk in one()'s round-robin start (one_step): fail_agree_2b +5.8 %. (Round 3 kept it
// out of the 8-server instances after step_kernel<18, 8> faulted with it; that fault needed the
// instance's scratch spills, and the 8-server instances now run without any: DESIGN.md §6.9)

struct T {  // the tester coroutine frame, in registers during a tester event
  uint32_t pc, res, helper;
  uint32_t l[T_NL];
  uint32_t h[T_NH];
  uint64_t hv;
};

DI uint32_t t_draw(const Dev& D, X& x, uint32_t& w1) {
  uint32_t w0;
  philox(D, x, x.t_ctr++, 0, ST_TESTER, w0, w1);
  return w0;
}
DI uint32_t t_range(const Dev& D, X& x, uint32_t lo, uint32_t hi) {
  uint32_t w1, w0 = t_draw(D, x, w1);
  return u_range(w0, lo, hi);
}
DI bool t_bool(const Dev& D, X& x, uint32_t p_q32) {
  uint32_t w1;
  return t_draw(D, x, w1) < p_q32;
}
DI uint64_t t_entry(const Dev& D, X& x) {  // tests.rs:943-951 gen_entry
  uint32_t w1, w0 = t_draw(D, x, w1);
  return ((uint64_t)w1 << 32) | w0;
}
// gen_entry for start(i) on server i: only a leader's start() reads its command, so for any
// other server the draw only advances the tester's counter (draw k is keyed by k alone,
// SEMANTICS §2; MR_TAPE builds record every draw and take it)
DI uint64_t t_entry_for_start(const Dev& D, X& x, uint32_t i, uint32_t lm) {
  if (!MR_TAPE && !(bit(x.alive, i) && !p_null_raft(D, x) && bit(lm, i))) {
    x.t_ctr++;
    return 0;
  }
  return t_entry(D, x);
}
// ---- multi-event tester calls: step() returns true when done, false after
// scheduling a sleep or failing. Frame: t.h[0..4], t.hv; result in t.res / t.hv.

// check_one_leader, tester.rs:64-92. h0 iteration, h4 phase
DI void col_init(T& t) { t.h[0] = 0; t.h[4] = 1; }
DI bool col_step(const Dev& D, X& x, T& t) {
  for (;;) {
    if (t.h[4] == 1) {
      if (t.h[0] >= 10) { fail(D, x, MR_FAIL_ONE_LEADER_NONE); return false; }
      t_sleep(x, t_range(D, x, 450000u, 550000u));
      t.h[4] = 2;
      return false;
    }
    uint32_t best_term = 0, best = NONE, terms_seen = 0;
    uint32_t tm[NB];  // every server's term, one batch of loads
    t_terms(D, x, tm);
    for (uint32_t i = 0; i < D.n; i++) {
      if (!t_connected(D, x, i)) continue;
      if (!t_started(D, x, i)) { fail(D, x, MR_FAIL_UNWRAP_NONE); return false; }
      if (p_null_raft(D, x) || !bit(t_leaders(D, x), i)) continue;
      uint32_t ti = sel_nb(tm, i);
      for (uint32_t j = 0; j < i; j++) {  // >1 leaders in one term?
        if (t_connected(D, x, j) && bit(t_leaders(D, x), j) &&
            sel_nb(tm, j) == ti) {
          fail(D, x, MR_FAIL_MULTI_LEADER_TERM);
          return false;
        }
      }
      terms_seen++;
      if (best == NONE || ti > best_term) { best_term = ti; best = i; }
    }
    if (terms_seen) { t.res = best; return true; }
    t.h[0]++;
    t.h[4] = 1;
  }
}

// one(cmd, expected, retry), tester.rs:216-262.
// h0 t0, h1 starts, h2 index, h3 t1, h4 phase | expected << 8 | retry << 16; hv cmd
DI void one_init(const Dev& D, X& x, T& t, uint64_t cmd, uint32_t expected, bool retry) {
  t.hv = cmd;
  t.h[0] = x.now;
  t.h[1] = 0;
  t.h[4] = 1u | (expected << 8) | (retry ? 1u << 16 : 0u);
}
DI bool one_step(const Dev& D, X& x, T& t) {
  uint32_t expected = (t.h[4] >> 8) & 255u;
  bool retry = (t.h[4] >> 16) & 1u;
  for (;;) {
    if ((t.h[4] & 255u) == 1) {
      if (!(x.now - t.h[0] < 10000000u)) { fail(D, x, MR_FAIL_ONE_NO_AGREEMENT); return false; }
      uint32_t starts = t.h[1], index = 0, term;
      bool have = false;
      const uint32_t lm = t_leaders(D, x);
      {
        // the first connected, started leader in the rotation h1 + 1, h1 + 2, ... (mod n): the
        // servers before it answer Err(NotLeader) with no effect, so one start() per lane — one
        // copy of its path per wave, not one per server index (t_start_round)
        const uint32_t all = (1u << D.n) - 1u, cand = lm & x.conn & x.alive & all;
        if (cand && !p_null_raft(D, x)) {
          const uint32_t r = (starts + 1u) % D.n;  // rotate so that server r is bit 0
          const uint32_t rot = ((cand >> r) | (cand << (D.n - r))) & all;
          starts = (r + (uint32_t)__builtin_ctz(rot)) % D.n;
          have = t_start(D, x, starts, t.hv, index, term, true);
          if (x.code != RUN) return false;
        }
      }
      t.h[1] = starts;
      if (!have) { t_sleep(x, 50000); return false; }
      t.h[2] = index;
      t.h[3] = x.now;
      t.h[4] = (t.h[4] & ~255u) | 2u;
    }
    if (!(x.now - t.h[3] < 2000000u)) {
      if (!retry) { fail(D, x, MR_FAIL_ONE_NO_AGREEMENT); return false; }
      t.h[4] = (t.h[4] & ~255u) | 1u;
      continue;
    }
    uint64_t v;
    uint32_t cnt = n_committed(D, x, t.h[2], v);
    if (cnt > 0 && cnt >= expected && v == t.hv) { t.res = t.h[2]; return true; }
    t_sleep(x, 20000);
    return false;
  }
}

// wait(index, n, start_term), tester.rs:175-201.
// h0 to, h1 iteration, h2 index, h3 start term, h4 phase | n << 8 | has_st << 16
// result: t.res = Some?, t.hv = value
DI void wait_init(T& t, uint32_t index, uint32_t nn, bool has_st, uint32_t st) {
  t.h[0] = 10000; t.h[1] = 0; t.h[2] = index; t.h[3] = st;
  t.h[4] = 1u | (nn << 8) | (has_st ? 1u << 16 : 0u);
}
DI bool wait_step(const Dev& D, X& x, T& t) {
  uint32_t nn = (t.h[4] >> 8) & 255u;
  uint64_t v;
  if ((t.h[4] & 255u) == 2) {
    if ((t.h[4] >> 16) & 1u) {
      uint32_t tm[NB];  // every server's term, one batch of loads
      t_terms(D, x, tm);
      for (uint32_t i = 0; i < D.n; i++)
        if (t_started(D, x, i) && sel_nb(tm, i) > t.h[3]) {
          t.res = 0;
          return true;
        }
    }
    t.h[1]++;
    t.h[4] = (t.h[4] & ~255u) | 1u;
  }
  uint32_t cnt = n_committed(D, x, t.h[2], v);
  if (t.h[1] < 30 && cnt < nn) {
    t_sleep(x, t.h[0]);
    if (t.h[0] < 1000000u) t.h[0] *= 2;
    t.h[4] = (t.h[4] & ~255u) | 2u;
    return false;
  }
  if (cnt < nn) { fail(D, x, MR_FAIL_WAIT_TOO_FEW); return false; }
  t.res = cnt > 0 ? 1u : 0u;
  t.hv = v;
  return true;
}

// ---- scenario state machines. Each test body (tests.rs) is split at its
// suspension points into numbered states; a state ends by sleeping (SLEEP_TO),
// by starting a multi-event tester call (ONE_TO / COL_TO / WAIT_TO) that the
// dispatcher in tester() runs before resuming at the given state, by jumping
// to another state (GO), or with the verdict. The dispatch loop over a switch
// keeps the control flow reducible (protothread-style resumption into the
// middle of loops made the AMDGPU structurizer blow up register pressure).
// Persistent locals live in t.l[].
enum : uint32_t { H_NONE = 0, H_ONE, H_COL, H_WAIT, H_CALL, H_JOIN };  // H_CALL: kvraft clerk call
#define CK() do { if (x.code != RUN) return; } while (0)
#define GO(s) { t.pc = (s); continue; }
#define SLEEP_TO(us, s) { t_sleep(x, (us)); t.pc = (s); return; }
#define ONE_TO(cmd, e, r, s) \
  { one_init(D, x, t, (cmd), (e), (r)); t.helper = H_ONE; t.pc = (s); return; }
#define COL_TO(s) { col_init(t); t.helper = H_COL; t.pc = (s); return; }
#define WAIT_TO(idx, nn, has, st, s) \
  { wait_init(t, (idx), (nn), (has), (st)); t.helper = H_WAIT; t.pc = (s); return; }
#define END() { t_end(D, x); return; }
#define BAD() default: fail(D, x, MR_FAIL_SIM_BAD_PROGRAM); return;

DI void scn_initial_election(const Dev& D, X& x, T& t) {  // tests.rs:20-46
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); COL_TO(1)
    case 1: SLEEP_TO(50000, 2)
    case 2: t_check_terms(D, x); CK(); SLEEP_TO(2 * ELECTION_US, 3)
    case 3: t_check_terms(D, x); CK(); COL_TO(4)  // term1 != term2 only warns
    case 4: END()
    BAD()
  }
}

DI void scn_reelection(const Dev& D, X& x, T& t) {  // tests.rs:48-78
  const uint32_t n = D.n;
  uint32_t& l1 = t.l[0];
  uint32_t& l2 = t.l[1];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); COL_TO(1)
    case 1: l1 = t.res; t_conn(D, x, l1, 0); COL_TO(2)
    case 2: t_conn(D, x, l1, 1); COL_TO(3)
    case 3:
      l2 = t.res;
      t_conn(D, x, l2, 0);
      t_conn(D, x, (l2 + 1) % n, 0);
      SLEEP_TO(2 * ELECTION_US, 4)
    case 4: t_check_no_leader(D, x); CK(); t_conn(D, x, (l2 + 1) % n, 1); COL_TO(5)
    case 5: t_conn(D, x, l2, 1); COL_TO(6)
    case 6: END()
    BAD()
  }
}

DI void scn_many_election(const Dev& D, X& x, T& t) {  // tests.rs:80-112
  const uint32_t n = D.n;
  uint32_t& it = t.l[0];
  uint32_t& i1 = t.l[1];
  uint32_t& i2 = t.l[2];
  uint32_t& i3 = t.l[3];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); COL_TO(1)
    case 1: it = 0; GO(2)
    case 2:
      if (it >= p_iters(D, x)) COL_TO(4)
      i1 = t_range(D, x, 0, n); i2 = t_range(D, x, 0, n); i3 = t_range(D, x, 0, n);
      t_conn(D, x, i1, 0); t_conn(D, x, i2, 0); t_conn(D, x, i3, 0);
      COL_TO(3)
    case 3:
      t_conn(D, x, i1, 1); t_conn(D, x, i2, 1); t_conn(D, x, i3, 1);
      it++;
      GO(2)
    case 4: END()
    BAD()
  }
}

DI void scn_basic_agree(const Dev& D, X& x, T& t) {  // tests.rs:114-130
  uint32_t& index = t.l[0];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); index = 1; GO(1)
    case 1: {
      if (index > 3) END()
      uint64_t v;
      if (n_committed(D, x, index, v) != 0) { fail(D, x, MR_FAIL_BASIC_PRECOMMIT); return; }
      ONE_TO((uint64_t)index * 100, D.n, false, 2)
    }
    case 2:
      if (t.res != index) { fail(D, x, MR_FAIL_BASIC_INDEX); return; }
      index++;
      GO(1)
    BAD()
  }
}

DI void scn_fail_agree(const Dev& D, X& x, T& t) {  // tests.rs:132-161
  const uint32_t n = D.n;
  uint32_t& leader = t.l[0];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); ONE_TO(101, n, false, 1)
    case 1: COL_TO(2)
    case 2: leader = t.res; t_conn(D, x, (leader + 1) % n, 0); ONE_TO(102, n - 1, false, 3)
    case 3: ONE_TO(103, n - 1, false, 4)
    case 4: SLEEP_TO(ELECTION_US, 5)
    case 5: ONE_TO(104, n - 1, false, 6)
    case 6: ONE_TO(105, n - 1, false, 7)
    case 7: t_conn(D, x, (leader + 1) % n, 1); ONE_TO(106, n, true, 8)
    case 8: SLEEP_TO(ELECTION_US, 9)
    case 9: ONE_TO(107, n, true, 10)
    case 10: END()
    BAD()
  }
}

DI void scn_fail_no_agree(const Dev& D, X& x, T& t) {  // tests.rs:163-209
  const uint32_t n = D.n;
  uint32_t& leader = t.l[0];
  uint32_t& index = t.l[1];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); ONE_TO(10, n, false, 1)
    case 1: COL_TO(2)
    case 2: {
      leader = t.res;
      t_conn(D, x, (leader + 1) % n, 0);
      t_conn(D, x, (leader + 2) % n, 0);
      t_conn(D, x, (leader + 3) % n, 0);
      uint32_t term;
      bool ok = t_start(D, x, leader, 20, index, term);
      CK();
      if (!ok) { fail(D, x, MR_FAIL_LEADER_REJECTED); return; }
      if (index != 2) { fail(D, x, MR_FAIL_EXPECTED_INDEX2); return; }
      SLEEP_TO(2 * ELECTION_US, 3)
    }
    case 3: {
      uint64_t v;
      if (n_committed(D, x, index, v) != 0) { fail(D, x, MR_FAIL_NO_MAJORITY_COMMIT); return; }
      t_conn(D, x, (leader + 1) % n, 1);
      t_conn(D, x, (leader + 2) % n, 1);
      t_conn(D, x, (leader + 3) % n, 1);
      COL_TO(4)
    }
    case 4: {
      uint32_t idx2, term;
      bool ok = t_start(D, x, t.res, 30, idx2, term);
      CK();
      if (!ok) { fail(D, x, MR_FAIL_LEADER_REJECTED); return; }
      if (idx2 < 2 || idx2 > 3) { fail(D, x, MR_FAIL_UNEXPECTED_INDEX); return; }
      ONE_TO(1000, n, true, 5)
    }
    case 5: END()
    BAD()
  }
}

// (0..servers).any(|j| t.term(j) != term) with unwrap() semantics
DI bool any_term_changed(const Dev& D, X& x, uint32_t term) {
  for (uint32_t j = 0; j < D.n; j++) {
    uint32_t tj = t_term(D, x, j);
    if (x.code != RUN) return false;
    if (tj != term) return true;
  }
  return false;
}

DI void scn_concurrent_starts(const Dev& D, X& x, T& t) {  // tests.rs:211-275
  const uint32_t n = D.n;
  uint32_t& tried = t.l[0];
  uint32_t& term = t.l[1];
  uint32_t& ni = t.l[2];  // idxes in TV(0..5)
  uint32_t& q = t.l[3];
  uint32_t& nc = t.l[4];  // cmds in TV(8..13)
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); tried = 0; GO(1)
    case 1:
      if (tried >= 5) { fail(D, x, MR_FAIL_TERM_CHANGED); return; }  // assert!(success)
      if (tried > 0) SLEEP_TO(3000000, 2)
      GO(2)
    case 2: COL_TO(3)
    case 3: {
      uint32_t leader = t.res, idx, st;
      bool ok = t_start(D, x, leader, 1, idx, term);
      CK();
      if (!ok) { tried++; GO(1) }
      ni = 0;
      for (uint32_t ii = 0; ii < 5; ii++) {
        bool ok2 = t_start(D, x, leader, 100 + ii, idx, st);
        CK();
        if (ok2 && st == term) { TV(ni) = idx; ni++; }
      }
      bool ch = any_term_changed(D, x, term);
      CK();
      if (ch) { tried++; GO(1) }
      nc = 0;
      q = 0;
      GO(4)
    }
    case 4:
      if (q >= ni) GO(6)
      WAIT_TO((uint32_t)TV(q), n, true, term, 5)
    case 5:
      if (t.res) { TV(8 + nc) = t.hv; nc++; }
      q++;
      GO(4)
    case 6:
      for (uint32_t ii = 0; ii < 5; ii++) {
        bool ok = false;
        for (uint32_t k = 0; k < nc; k++)
          if (TV(8 + k) == 100 + ii) ok = true;
        if (!ok) { fail(D, x, MR_FAIL_CMD_MISSING); return; }
      }
      END()
    BAD()
  }
}

DI void scn_rejoin(const Dev& D, X& x, T& t) {  // tests.rs:277-313
  const uint32_t n = D.n;
  uint32_t& l1 = t.l[0];
  uint32_t& l2 = t.l[1];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); ONE_TO(101, n, true, 1)
    case 1: COL_TO(2)
    case 2:
      l1 = t.res;
      t_conn(D, x, l1, 0);
      t_start(D, x, l1, 102); CK();
      t_start(D, x, l1, 103); CK();
      t_start(D, x, l1, 104); CK();
      ONE_TO(103, 2, true, 3)
    case 3: COL_TO(4)
    case 4: l2 = t.res; t_conn(D, x, l2, 0); t_conn(D, x, l1, 1); ONE_TO(104, 2, true, 5)
    case 5: t_conn(D, x, l2, 1); ONE_TO(105, n, true, 6)
    case 6: END()
    BAD()
  }
}

DI void scn_backup(const Dev& D, X& x, T& t) {  // tests.rs:315-386
  const uint32_t n = D.n;
  uint32_t& l1 = t.l[0];
  uint32_t& l2 = t.l[1];
  uint32_t& other = t.l[2];
  uint32_t& i = t.l[3];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); ONE_TO(t_entry(D, x), n, true, 1)
    case 1: COL_TO(2)
    case 2:
      l1 = t.res;
      t_conn(D, x, (l1 + 2) % n, 0); t_conn(D, x, (l1 + 3) % n, 0); t_conn(D, x, (l1 + 4) % n, 0);
      for (uint32_t k = 0; k < 50; k++) {
        uint64_t e = t_entry(D, x);
        t_start(D, x, l1, e); CK();
      }
      SLEEP_TO(ELECTION_US / 2, 3)
    case 3:
      t_conn(D, x, (l1 + 0) % n, 0); t_conn(D, x, (l1 + 1) % n, 0);
      t_conn(D, x, (l1 + 2) % n, 1); t_conn(D, x, (l1 + 3) % n, 1); t_conn(D, x, (l1 + 4) % n, 1);
      i = 0;
      GO(4)
    case 4:
      if (i >= 50) COL_TO(6)
      ONE_TO(t_entry(D, x), 3, true, 5)
    case 5: i++; GO(4)
    case 6:
      l2 = t.res;
      other = (l1 + 2) % n;
      if (l2 == other) other = (l2 + 1) % n;
      t_conn(D, x, other, 0);
      for (uint32_t k = 0; k < 50; k++) {
        uint64_t e = t_entry(D, x);
        t_start(D, x, l2, e); CK();
      }
      SLEEP_TO(ELECTION_US / 2, 7)
    case 7:
      for (uint32_t k = 0; k < n; k++) t_conn(D, x, k, 0);
      t_conn(D, x, (l1 + 0) % n, 1); t_conn(D, x, (l1 + 1) % n, 1); t_conn(D, x, other, 1);
      i = 0;
      GO(8)
    case 8:
      if (i >= 50) {
        for (uint32_t k = 0; k < n; k++) t_conn(D, x, k, 1);
        ONE_TO(t_entry(D, x), n, true, 10)
      }
      ONE_TO(t_entry(D, x), 3, true, 9)
    case 9: i++; GO(8)
    case 10: END()
    BAD()
  }
}

DI void scn_count(const Dev& D, X& x, T& t) {  // tests.rs:388-479
  const uint32_t n = D.n;
  uint32_t& total1 = t.l[0];
  uint32_t& total2 = t.l[1];
  uint32_t& tried = t.l[2];
  uint32_t& starti = t.l[3];
  uint32_t& term = t.l[4];
  uint32_t& i = t.l[5];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); COL_TO(1)
    case 1:
      total1 = x.msgs_sent / 2;
      if (total1 < 1 || total1 > 30) { fail(D, x, MR_FAIL_RPC_INITIAL); return; }
      total2 = 0;
      tried = 0;
      GO(2)
    case 2:
      if (tried >= 5) { fail(D, x, MR_FAIL_TERM_CHANGED); return; }
      if (tried > 0) SLEEP_TO(3000000, 3)
      GO(3)
    case 3: COL_TO(4)
    case 4: {
      total1 = x.msgs_sent / 2;
      uint32_t leader = t.res, idx, st;
      bool ok = t_start(D, x, leader, 1, starti, term);
      CK();
      if (!ok) { tried++; GO(2) }
      bool outer = false;
      for (uint32_t k = 1; k < 10 + 2; k++) {
        uint64_t xv = t_entry(D, x);  // random.gen::<u64>()
        TV(k - 1) = xv;
        bool ok2 = t_start(D, x, leader, xv, idx, st);
        CK();
        if (!ok2 || st != term) { outer = true; break; }
        if (starti + k != idx) { fail(D, x, MR_FAIL_START_FAILED); return; }
      }
      if (outer) { tried++; GO(2) }
      i = 1;
      GO(5)
    }
    case 5:
      if (i > 10) GO(7)
      WAIT_TO(starti + i, n, true, term, 6)
    case 6:
      if (t.res && t.hv != TV(i - 1)) { fail(D, x, MR_FAIL_WRONG_VALUE); return; }
      i++;
      GO(5)
    case 7: {
      bool ch = any_term_changed(D, x, term);
      CK();
      if (ch) { tried++; GO(2) }
      total2 = x.msgs_sent / 2;
      if (total2 - total1 > (10 + 1 + 3) * 3) { fail(D, x, MR_FAIL_RPC_TOO_MANY); return; }
      SLEEP_TO(ELECTION_US, 8)
    }
    case 8:
      if (x.msgs_sent / 2 - total2 > 3 * 20) { fail(D, x, MR_FAIL_RPC_IDLE); return; }
      END()
    BAD()
  }
}

DI void scn_persist1(const Dev& D, X& x, T& t) {  // tests.rs:481-526
  const uint32_t n = D.n;
  uint32_t& l = t.l[0];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); ONE_TO(11, n, true, 1)
    case 1:
      for (uint32_t i = 0; i < n; i++) t_start1(D, x, i);
      for (uint32_t i = 0; i < n; i++) { t_conn(D, x, i, 0); t_conn(D, x, i, 1); }
      ONE_TO(12, n, true, 2)
    case 2: COL_TO(3)
    case 3:
      l = t.res;
      t_conn(D, x, l, 0); t_start1(D, x, l); t_conn(D, x, l, 1);
      ONE_TO(13, n, true, 4)
    case 4: COL_TO(5)
    case 5: l = t.res; t_conn(D, x, l, 0); ONE_TO(14, n - 1, true, 6)
    case 6: t_start1(D, x, l); t_conn(D, x, l, 1); WAIT_TO(4, n, false, 0, 7)
    case 7: COL_TO(8)
    case 8: l = (t.res + 1) % n; t_conn(D, x, l, 0); ONE_TO(15, n - 1, true, 9)
    case 9: t_start1(D, x, l); t_conn(D, x, l, 1); ONE_TO(16, n, true, 10)
    case 10: END()
    BAD()
  }
}

DI void scn_persist2(const Dev& D, X& x, T& t) {  // tests.rs:528-572
  const uint32_t n = D.n;
  uint32_t& index = t.l[0];
  uint32_t& k = t.l[1];
  uint32_t& l1 = t.l[2];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); index = 1; k = 0; GO(1)
    case 1:
      if (k >= 5) ONE_TO(1000, n, true, 7)
      ONE_TO(10 + index, n, true, 2)
    case 2: index++; COL_TO(3)
    case 3:
      l1 = t.res;
      t_conn(D, x, (l1 + 1) % n, 0); t_conn(D, x, (l1 + 2) % n, 0);
      ONE_TO(10 + index, n - 2, true, 4)
    case 4:
      index++;
      t_conn(D, x, (l1 + 0) % n, 0); t_conn(D, x, (l1 + 3) % n, 0); t_conn(D, x, (l1 + 4) % n, 0);
      t_start1(D, x, (l1 + 1) % n); t_start1(D, x, (l1 + 2) % n);
      t_conn(D, x, (l1 + 1) % n, 1); t_conn(D, x, (l1 + 2) % n, 1);
      SLEEP_TO(ELECTION_US, 5)
    case 5:
      t_start1(D, x, (l1 + 3) % n); t_conn(D, x, (l1 + 3) % n, 1);
      ONE_TO(10 + index, n - 2, true, 6)
    case 6:
      index++;
      t_conn(D, x, (l1 + 4) % n, 1); t_conn(D, x, (l1 + 0) % n, 1);
      k++;
      GO(1)
    case 7: END()
    BAD()
  }
}

DI void scn_persist3(const Dev& D, X& x, T& t) {  // tests.rs:574-602
  const uint32_t n = D.n;
  uint32_t& leader = t.l[0];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); ONE_TO(101, 3, true, 1)
    case 1: COL_TO(2)
    case 2: leader = t.res; t_conn(D, x, (leader + 2) % n, 0); ONE_TO(102, 2, true, 3)
    case 3:
      t_crash1(D, x, (leader + 0) % n); t_crash1(D, x, (leader + 1) % n);
      t_conn(D, x, (leader + 2) % n, 1);
      t_start1(D, x, (leader + 0) % n); t_conn(D, x, (leader + 0) % n, 1);
      ONE_TO(103, 2, true, 4)
    case 4:
      t_start1(D, x, (leader + 1) % n); t_conn(D, x, (leader + 1) % n, 1);
      ONE_TO(104, n, true, 5)
    case 5: END()
    BAD()
  }
}

DI uint32_t fig8_delay(const Dev& D, X& x) {  // tests.rs:631-635 / 711-715
  // the same two draws as `if t_bool { range(0, E/2) } else { range(0, 13 ms) }`, through one
  // draw site: the lanes of a wave that took either branch share one Philox copy
  const bool lng = t_bool(D, x, LOSS_Q32);
  return t_range(D, x, 0, lng ? ELECTION_US / 2 : 13000u);
}

// figure_8's start(gen_entry()) round (tests.rs:617-627 / 701-709): the servers of `iter` in
// ascending order, each taking one tester draw (gen_entry); only a leader's start() reads its
// entry and writes (t_entry_for_start). A wave's lanes have their leaders at different server
// indices, so a loop over every index runs the start path once per index that is some lane's
// leader — one record round trip each. Walking each lane's own leaders instead (ascending;
// a second one only where two servers both believe they lead) runs it once per wave: the
// draws keep their counters (server i's is the round's first + the iterated servers below i)
// and a non-leader's start() has no effect on a live server. Returns the last server, in
// ascending order, whose start succeeded (and is connected, `need_conn`), or NONE.
DI uint32_t t_start_round(const Dev& D, X& x, uint32_t iter, bool need_conn) {
  const uint32_t lm = t_leaders(D, x), ctr0 = x.t_ctr;
  uint32_t res = NONE;
  if (MR_TAPE || p_null_raft(D, x) || (iter & ~x.alive)) {  // server by server
    for (uint32_t i = 0; i < D.n; i++) {
      if (!bit(iter, i)) continue;
      const uint64_t e = t_entry_for_start(D, x, i, lm);
      uint32_t ix, tm;
      const bool ok = t_start(D, x, i, e, ix, tm, bit(lm, i));
      if (x.code != RUN) return NONE;
      if (ok && (!need_conn || t_connected(D, x, i))) res = i;
    }
    return res;
  }
  for (uint32_t lead = lm & iter; lead; lead &= lead - 1u) {
    const uint32_t i = (uint32_t)__builtin_ctz(lead);
    x.t_ctr = ctr0 + (uint32_t)__builtin_popcount(iter & ((1u << i) - 1u));
    const uint64_t e = t_entry(D, x);
    uint32_t ix, tm;
    const bool ok = t_start(D, x, i, e, ix, tm, true);
    if (x.code != RUN) return NONE;
    if (ok && (!need_conn || t_connected(D, x, i))) res = i;
  }
  x.t_ctr = ctr0 + (uint32_t)__builtin_popcount(iter);
  return res;
}

// figure_8_2c (tests.rs:612-660); with `unreliable` the config-3 literal variant
DI void scn_figure_8(const Dev& D, X& x, T& t, bool unreliable) {
  const uint32_t n = D.n;
  uint32_t& nup = t.l[0];
  uint32_t& it = t.l[1];
  uint32_t& leader = t.l[2];
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, false);
      if (unreliable) t_set_unrel(x, true);
      ONE_TO(t_entry(D, x), 1, true, 1)
    case 1: nup = n; it = 0; GO(2)
    case 2:
      if (it >= p_iters(D, x)) {
        for (uint32_t i = 0; i < n; i++)
          if (!t_started(D, x, i)) t_start1(D, x, i);
        ONE_TO(t_entry(D, x), n, true, 4)
      }
      leader = t_start_round(D, x, x.alive & ((1u << n) - 1u), false);  // started servers
      CK();
      SLEEP_TO(fig8_delay(D, x), 3)
    case 3:
      if (leader != NONE) { t_crash1(D, x, leader); nup--; }
      if (nup < 3) {
        uint32_t s = t_range(D, x, 0, n);
        if (!t_started(D, x, s)) { t_start1(D, x, s); nup++; }
      }
      it++;
      GO(2)
    case 4: END()
    BAD()
  }
}

DI void scn_figure_8_unreliable(const Dev& D, X& x, T& t) {  // tests.rs:688-741
  const uint32_t n = D.n;
  uint32_t& nup = t.l[0];
  uint32_t& it = t.l[1];
  uint32_t& leader = t.l[2];
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, false);
      t_set_unrel(x, true);
      ONE_TO(t_entry(D, x), 1, true, 1)
    case 1: nup = n; it = 0; GO(2)
    case 2:
      if (it >= p_iters(D, x)) {
        for (uint32_t i = 0; i < n; i++) t_conn(D, x, i, 1);
        ONE_TO(t_entry(D, x), n, true, 4)
      }
      leader = t_start_round(D, x, (1u << n) - 1u, true);
      CK();
      SLEEP_TO(fig8_delay(D, x), 3)
    case 3:
      if (leader != NONE && t_range(D, x, 0, 1000) < ELECTION_US / 1000 / 2) {
        t_conn(D, x, leader, 0);
        nup--;
      }
      if (nup < 3) {
        uint32_t s = t_range(D, x, 0, n);
        if (!t_connected(D, x, s)) { t_conn(D, x, s, 1); nup++; }
      }
      it++;
      GO(2)
    case 4: END()
    BAD()
  }
}

DI void scn_snap_common(const Dev& D, X& x, T& t, bool disconnect, bool reliable, bool crash) {
  // tests.rs:858-911
  const uint32_t n = D.n;
  uint32_t& leader1 = t.l[0];
  uint32_t& i = t.l[1];
  uint32_t& victim = t.l[2];
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, true);
      t_set_unrel(x, !reliable);
      ONE_TO(t_entry(D, x), n, true, 1)
    case 1: COL_TO(2)
    case 2: leader1 = t.res; i = 0; GO(3)
    case 3:
      if (i >= p_iters(D, x)) END()
      victim = (i % 3 == 1) ? leader1 : (leader1 + 1) % n;
      if (disconnect) { t_conn(D, x, victim, 0); ONE_TO(t_entry(D, x), n - 1, true, 4) }
      GO(4)
    case 4:
      if (crash) { t_crash1(D, x, victim); ONE_TO(t_entry(D, x), n - 1, true, 5) }
      GO(5)
    case 5: {
      uint32_t sender = (i % 3 == 1) ? (leader1 + 1) % n : leader1;
      t_start_burst(D, x, sender, 11);  // for _ in 0..=10 { start(sender, gen_entry()) }
      CK();
      ONE_TO(t_entry(D, x), n - 1, true, 6)
    }
    case 6:
      if (t_log_size(D, x) >= 2000) { fail(D, x, MR_FAIL_LOG_SIZE); return; }
      if (disconnect) { t_conn(D, x, victim, 1); ONE_TO(t_entry(D, x), n, true, 7) }
      GO(9)
    case 7: COL_TO(8)
    case 8: leader1 = t.res; GO(9)
    case 9:
      if (crash) {
        t_start1(D, x, victim);
        t_conn(D, x, victim, 1);
        ONE_TO(t_entry(D, x), n, true, 10)
      }
      GO(12)
    case 10: COL_TO(11)
    case 11: leader1 = t.res; GO(12)
    case 12: i++; GO(3)
    BAD()
  }
}

// S = the scenario, a template constant: each step-kernel instance holds one
// test body only (the union of all 21 spilled to scratch: DESIGN.md §6)
// ---- kvraft generic_test (kvraft/tests.rs:65-220; SEMANTICS §8-9)
// the test body's clerk call on ck (slot 0): t.res = the reply value
DI bool call_step(const Dev& D, X& x, T& t) {  // through the clerk of slot t.h[0]
  const uint32_t k = t.h[0];
  if (clerk_resume(D, x, k)) { t.res = KT(KT_RVAL, k); t.hv = KT(KT_RHINT, k); return true; }
  x.yield = 2;  // re-sent: blocked until the reply or the new deadline (x.twake)
  return false;
}
// JoinHandle.await: only the joined thread's finish wakes the test body
DI bool join_step(const Dev& D, X& x, T& t) {
  CS(CS_MJOIN) = 0xFFFFFFFFu;
  return true;
}
#define CALLK_TO(k, op, key, elem, s)                                                   \
  {                                                                                     \
    t.h[0] = (k); clerk_begin(D, x, (k), (op), (key), (elem));                          \
    t.helper = H_CALL; t.pc = (s); x.yield = 2; return;                                 \
  }
#define CALL_TO(op, key, elem, s) CALLK_TO(0u, op, key, elem, s)
#define JOINALL_TO(s)                                                                      \
  {                                                                                        \
    if (CS(CS_NLIVE) == 0u) GO(s)                                                          \
    CS(CS_MJOIN) = JOIN_ALL; x.twake = INF_T; t.helper = H_JOIN; t.pc = (s); x.yield = 2; return; \
  }
// select! over the spawned tasks and sleep(us): the first task to finish, or the deadline
#define JOINANY_TO(us, s) \
  { CS(CS_MJOIN) = JOIN_ANY; x.twake = x.now + (us); t.helper = H_JOIN; t.pc = (s); x.yield = 2; return; }
#define JOIN_TO(slot, s)                                                           \
  {                                                                                \
    if (!KT(KT_LIVE, (slot))) GO(s)                                                \
    CS(CS_MJOIN) = (slot); x.twake = INF_T; t.helper = H_JOIN; t.pc = (s); x.yield = 2; return; \
  }

// kvraft/tester.rs:153-169: shutdown_server = crash1; start_server = start1 with an
// empty KV state machine (rebuilt by re-applying the log) and dedup table
DI void t_start_server(const Dev& D, X& x, uint32_t i) {
  t_start1(D, x, i);
  if (D.kvs32) { kv_state_put(D, x, i, KVSP(i)); return; }  // restore from the snapshot
  uint32_t* kp = D.kv32 + ((size_t)x.c * D.n + i) * KVREC;
  for (uint32_t w = KVR_DEDUP; w < KVR_DEDUP + MAX_CLERKS; w++) kp[w] = 0u;
  for (uint32_t w = KVR_KEYS; w < KVREC; w++) kp[w] = 0u;
}
DI void t_connect_all(const Dev& D, X& x) { CS(CS_CUT) = 0u; CS(CS_CUT + 1) = 0u; }

// generic_test (kvraft/tests.rs:65-220) with the scenario's (nclients, unreliable, crash, partitions)
template <uint32_t S>
DI void scn_kv_generic(const Dev& D, X& x, T& t) {
  constexpr KvGen g = kv_gen(S);
  constexpr uint32_t nc = g.nc, ps = 1 + g.nc;  // the partitioner's slot
  uint32_t& it = t.l[0];
  uint32_t& cli = t.l[1];
  uint32_t& jj = t.l[2];
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, false);  // Tester::new (kvraft/tester.rs:27-56)
      if (g.unrel) t_set_unrel(x, true);
      x.conn |= 0xFFFFFF00u;  // clerk hosts (connect_client, kvraft/tester.rs:140-150)
      it = 0;
      GO(1)
    case 1:
      if (it >= 3) END()
      CS(CS_KVDONE) = 0u;
      for (uint32_t c = 0; c < nc; c++) {
        kv_spawn(D, x, 1 + c, 1 + nc * it + c, c);
        if constexpr (mr_scn_is_lin15(S)) {  // §9b: a client's token counter continues over iterations
          KT(KT_KIND, 1 + c) = 4u;
          KT(KT_J, 1 + c) = D.lin32[(size_t)x.c * (KV_KEYS * KV_APP * LINW) + LIN15_J + GI(c, LIN_CLI, G_LINJ)];
        }
      }
      if (g.part) SLEEP_TO(ELECTION_US, 6)  // let the clients work uninterrupted for 1 s
      GO(7)
    case 6: {  // spawn the partitioner (tests.rs:135-157)
      thr_spawn(D, x, ps, 1 + 3 * nc + it);
      uint32_t perm = 0;
      for (uint32_t k = 0; k < D.n; k++) perm |= k << (4 * k);  // t.all()
      KT(KT_KIND, ps) = 1u;
      KT(KT_PERM, ps) = perm;
      KT(KT_ID, ps) = 0xFFFFu;  // no clerk
      GO(7)
    }
    case 7: SLEEP_TO(5000000u, 2)
    case 2:
      CS(CS_KVDONE) = 1u;
      if (g.part) JOIN_TO(ps, 8)
      GO(9)
    case 8: t_connect_all(D, x); SLEEP_TO(ELECTION_US, 9)
    case 9:
      if (!g.crash) { cli = 0; GO(3) }
      for (uint32_t k = 0; k < D.n; k++) t_crash1(D, x, k);  // shutdown_server
      SLEEP_TO(ELECTION_US, 10)
    case 10:
      for (uint32_t k = 0; k < D.n; k++) t_start_server(D, x, k);
      t_connect_all(D, x);
      cli = 0;
      GO(3)
    case 3:
      if (cli >= nc) {
        if (g.maxraft && t_log_size(D, x) > 2 * g.maxraft) {  // kvraft/tests.rs:207-215
          fail(D, x, MR_FAIL_KV_LOG_SIZE);
          return;
        }
        it++;
        GO(1)
      }
      JOIN_TO(1 + cli, 4)
    case 4:
      if constexpr (mr_scn_is_lin15(S)) {  // no predicted values: the checker judged every Get (§9b)
        D.lin32[(size_t)x.c * (KV_KEYS * KV_APP * LINW) + LIN15_J + GI(cli, LIN_CLI, G_LINJ)] = KT(KT_J, 1 + cli);
        cli++;
        GO(3)
      }
      jj = KT(KT_J, 1 + cli); CALL_TO(KV_GET, cli, cli, 5)  // check_clnt_appends(cli, &v, j)
    case 5: {
      const uint32_t v = t.res;
      CS(CS_KV_CHECKED) = CS(CS_KV_CHECKED) + 1u;
      if (!(v >> 31)) { fail(D, x, MR_FAIL_KV_APPEND_BAD); return; }        // kvraft/tests.rs:31-39
      if ((v & 0x7FFFFFFFu) < jj) { fail(D, x, MR_FAIL_KV_MISSING); return; }  // kvraft/tests.rs:25-30
      cli++;
      GO(3)
    }
    BAD()
  }
}

// ---- kvraft tests with their own bodies (kvraft/tests.rs:240-342, 396-492)
DI bool kv_check_ok(const Dev& D, X& x, uint32_t k, uint32_t tok) {  // Clerk::check's assert_eq
  CS(CS_KV_CHECKED) = CS(CS_KV_CHECKED) + 1u;
  const uint64_t h = tok ? (tok + 1ull) * 0x9E3779B97F4A7C15ull : 0ull;
  return KT(KT_RVH0, k) == (uint32_t)h && KT(KT_RVH1, k) == (uint32_t)(h >> 32);
}
#define CHECK_OK(k, tok) \
  if (!kv_check_ok(D, x, (k), (tok))) { fail(D, x, MR_FAIL_KV_CHECK); return; }
// t.partition(left, all \ left): link i~j up iff same side
DI void t_partition_left(const Dev& D, X& x, uint32_t left) {
  uint32_t cut0 = 0, cut1 = 0;
  for (uint32_t i = 0; i < D.n; i++)
    for (uint32_t j = 0; j < D.n; j++)
      if (bit(left, i) != bit(left, j)) {
        if (i < 4) cut0 |= 1u << (8 * i + j);
        else cut1 |= 1u << (8 * (i - 4) + j);
      }
  CS(CS_CUT) = cut0; CS(CS_CUT + 1) = cut1;
}
DI bool t_log_ok(const Dev& D, X& x) { return t_log_size(D, x) <= 2000u; }  // 2 * maxraftstate

DI void scn_kv_one_key(const Dev& D, X& x, T& t) {  // unreliable_one_key_3a, tests.rs:240-274
  constexpr uint32_t K = key_letter('k');
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, false);
      t_set_unrel(x, true);
      x.conn |= 0xFFFFFF00u;
      main_clerk(D, x, 0, 0, 0xFFu);
      CALL_TO(KV_PUT, K, 0u, 1)
    case 1:
      for (uint32_t i = 0; i < 5; i++) {  // make_client(&t.all()), spawn its 10 appends
        set_ccut(D, x, 1 + i, 0xFFu);
        kv_task_spawn(D, x, 1 + i, 1 + i, 2, i, 1 + i, KV_APPEND, K, 0u, 10u);
      }
      JOINALL_TO(2)
    case 2: CALL_TO(KV_GET, K, KV_ALL, 3)
    case 3:
      CS(CS_KV_CHECKED) = CS(CS_KV_CHECKED) + 1u;
      for (uint32_t i = 0; i < 5; i++) {  // check_concurrent_appends(&vx, &counts)
        const uint32_t f = (t.res >> (6 * i)) & 63u;
        if (!(f >> 5)) { fail(D, x, MR_FAIL_KV_APPEND_BAD); return; }
        if ((f & 31u) < 10u) { fail(D, x, MR_FAIL_KV_MISSING); return; }
      }
      END()
    BAD()
  }
}

DI void scn_kv_one_partition(const Dev& D, X& x, T& t) {  // one_partition_3a, tests.rs:276-342
  uint32_t& p2 = t.l[0];
  const uint32_t all = (1u << D.n) - 1u;
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, false);
      x.conn |= 0xFFFFFF00u;
      main_clerk(D, x, 0, 0, all);
      CALL_TO(KV_PUT, 1u, tok_num(13), 1)
    case 1: {  // make_partition (kvraft/tester.rs:184-192): leader to the minority
      uint32_t leader = 0xFFu;
      for (uint32_t i = D.n; i-- > 0;)
        if (bit(x.alive, i) && bit(t_leaders(D, x), i)) leader = i;
      if (leader == 0xFFu) leader = 0;
      uint32_t a[MR_MAX_NODES], m = D.n, p1 = 0;
      for (uint32_t i = 0; i < D.n; i++) a[i] = i;
      a[leader] = a[m - 1]; m--;  // swap_remove(leader)
      p2 = 1u << leader;
      for (uint32_t i = 0; i < m; i++) {
        if (i < D.n / 2 + 1) p1 |= 1u << a[i];
        else p2 |= 1u << a[i];
      }
      t_partition_left(D, x, p1);
      main_clerk(D, x, 1, 1, p1);  // ckp1
      set_ccut(D, x, 2, p2);       // ckp2a
      set_ccut(D, x, 3, p2);       // ckp2b
      CALLK_TO(1u, KV_PUT, 1u, tok_num(14), 2)
    }
    case 2: CALLK_TO(1u, KV_GET, 1u, 0u, 3)
    case 3:
      CHECK_OK(1, tok_num(14))
      kv_task_spawn(D, x, 2, 1, 3, 0, 2, KV_PUT, 1u, tok_num(15), 1u);  // ckp2a.put("1", "15")
      kv_task_spawn(D, x, 3, 2, 3, 0, 3, KV_GET, 1u, 0u, 1u);           // ckp2b.get("1")
      JOINANY_TO(1000000u, 4)
    case 4:
      if (!KT(KT_LIVE, 2) || !KT(KT_LIVE, 3)) { fail(D, x, MR_FAIL_KV_MINORITY_PROGRESS); return; }
      CALLK_TO(1u, KV_GET, 1u, 0u, 5)
    case 5: CHECK_OK(1, tok_num(14)) CALLK_TO(1u, KV_PUT, 1u, tok_num(16), 6)
    case 6: CALLK_TO(1u, KV_GET, 1u, 0u, 7)
    case 7:
      CHECK_OK(1, tok_num(16))
      t_connect_all(D, x);
      set_ccut(D, x, 2, all);
      set_ccut(D, x, 3, all);
      SLEEP_TO(ELECTION_US, 8)
    case 8:
      if (KT(KT_LIVE, 2) && KT(KT_LIVE, 3)) JOINANY_TO(3000000u, 9)
      GO(10)
    case 9:
      if (KT(KT_LIVE, 2) && KT(KT_LIVE, 3)) { fail(D, x, MR_FAIL_KV_NO_COMPLETION); return; }
      GO(10)
    case 10: CALL_TO(KV_GET, 1u, 0u, 11)
    case 11: CHECK_OK(0, tok_num(15)) END()
    BAD()
  }
}

DI void scn_kv_snapshot_rpc(const Dev& D, X& x, T& t) {  // snapshot_rpc_3b, tests.rs:396-454
  uint32_t& i = t.l[0];
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, false);
      x.conn |= 0xFFFFFF00u;
      main_clerk(D, x, 0, 0, 7u);
      CALL_TO(KV_PUT, key_letter('a'), tok_letter('A'), 1)
    case 1: CALL_TO(KV_GET, key_letter('a'), 0u, 2)
    case 2:
      CHECK_OK(0, tok_letter('A'))
      t_partition_left(D, x, 3u);  // [0, 1] | [2]
      main_clerk(D, x, 1, 1, 3u);
      i = 0;
      GO(3)
    case 3:
      if (i >= 50u) SLEEP_TO(ELECTION_US, 5)
      CALLK_TO(1u, KV_PUT, i, tok_num(i), 4)
    case 4: i++; GO(3)
    case 5: CALLK_TO(1u, KV_PUT, key_letter('b'), tok_letter('B'), 6)
    case 6:
      if (!t_log_ok(D, x)) { fail(D, x, MR_FAIL_KV_LOG_SIZE); return; }
      t_partition_left(D, x, 5u);  // [0, 2] | [1]
      main_clerk(D, x, 2, 2, 5u);
      CALLK_TO(2u, KV_PUT, key_letter('c'), tok_letter('C'), 7)
    case 7: CALLK_TO(2u, KV_PUT, key_letter('d'), tok_letter('D'), 8)
    case 8: CALLK_TO(2u, KV_GET, key_letter('a'), 0u, 9)
    case 9: CHECK_OK(2, tok_letter('A')) CALLK_TO(2u, KV_GET, key_letter('b'), 0u, 10)
    case 10: CHECK_OK(2, tok_letter('B')) CALLK_TO(2u, KV_GET, 1u, 0u, 11)
    case 11: CHECK_OK(2, tok_num(1)) CALLK_TO(2u, KV_GET, 49u, 0u, 12)
    case 12:
      CHECK_OK(2, tok_num(49))
      t_partition_left(D, x, 7u);
      CALL_TO(KV_PUT, key_letter('e'), tok_letter('E'), 13)
    case 13: CALL_TO(KV_GET, key_letter('c'), 0u, 14)
    case 14: CHECK_OK(0, tok_letter('C')) CALL_TO(KV_GET, key_letter('e'), 0u, 15)
    case 15: CHECK_OK(0, tok_letter('E')) CALL_TO(KV_GET, 1u, 0u, 16)
    case 16: CHECK_OK(0, tok_num(1)) END()
    BAD()
  }
}

DI void scn_kv_snapshot_size(const Dev& D, X& x, T& t) {  // snapshot_size_3b, tests.rs:456-492
  constexpr uint32_t X_ = key_letter('x');
  uint32_t& i = t.l[0];
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, false);
      x.conn |= 0xFFFFFF00u;
      main_clerk(D, x, 0, 0, 7u);
      i = 0;
      GO(1)
    case 1:
      if (i >= 200u) {
        if (!t_log_ok(D, x)) { fail(D, x, MR_FAIL_KV_LOG_SIZE); return; }
        uint32_t mx = 0;
        for (uint32_t s = 0; s < D.n; s++) { const uint32_t z = kv_snap_size(D, x, s); mx = z > mx ? z : mx; }
        if (mx > 500u) { fail(D, x, MR_FAIL_KV_SNAPSHOT_SIZE); return; }
        END()
      }
      CALL_TO(KV_PUT, X_, tok_num(0), 2)
    case 2: CALL_TO(KV_GET, X_, 0u, 3)
    case 3: CHECK_OK(0, tok_num(0)) CALL_TO(KV_PUT, X_, tok_num(1), 4)
    case 4: CALL_TO(KV_GET, X_, 0u, 5)
    case 5: CHECK_OK(0, tok_num(1)) i++; GO(1)
    BAD()
  }
}

// ---- raft tests with spawned tasks: unreliable_agree_2c (tests.rs:662-686),
// reliable / unreliable_churn_2c (tests.rs:743-856)

// one(cmd, expected, retry) as a spawned task: the same one_step over a frame kept in the thread slot
DI void agree_thr_step(const Dev& D, X& x, uint32_t slot) {
  T f;
#pragma unroll
  for (uint32_t k = 0; k < T_NH; k++) f.h[k] = KT(KT_W + k, slot);
  f.hv = ((uint64_t)KT(KT_W + T_NH + 1, slot) << 32) | KT(KT_W + T_NH, slot);
  const uint32_t tid = KT(KT_TID, slot);
  const bool done = one_step(D, x, f);
  if (x.code != RUN) return;
  rec_simple(D, x, 2, tid & 0xFFu);
  if (done) { thr_finish(D, x, slot); return; }
#pragma unroll
  for (uint32_t k = 0; k < T_NH; k++) KT(KT_W + k, slot) = f.h[k];
  thr_wake(D, x, slot, x.now + x.sleep_us);
}

// cfn, the churn client (tests.rs:763-797), slot 1 + me. Frame: x (W0, W1),
// index (W2), timeout step (W3), values recorded (W4).
template <uint32_t S>
DI void churn_step(const Dev& D, X& x, uint32_t slot) {
  const uint32_t me = slot - 1u, tid = KT(KT_TID, slot);
  uint32_t pc = KT(KT_PC, slot), sleep_ms = 0;
  uint64_t xv = ((uint64_t)KT(KT_W + 1, slot) << 32) | KT(KT_W, slot);
  uint32_t idx = KT(KT_W + 2, slot), toi = KT(KT_W + 3, slot);
  for (int guard = 0;; guard++) {
    if (guard > 4096) { fail(D, x, MR_FAIL_SIM_BAD_PROGRAM); return; }  // as the oracle
    if (pc == 0) {
      if (CS(CS_KVDONE)) {  // stop
        rec_simple(D, x, 2, tid & 0xFFu);
        thr_finish(D, x, slot);
        return;
      }
      const uint32_t tc = KT(KT_TCTR, slot);  // random.gen_entry() on the thread's stream
      KT(KT_TCTR, slot) = tc + 1u;
      uint32_t w0, w1;
      philox(D, x, tc, tid, ST_TESTER, w0, w1);
      xv = ((uint64_t)w1 << 32) | w0;
      bool has = false;
      const uint32_t lm = t_leaders(D, x);
      for (uint32_t i = 0; i < D.n; i++) {  // try them all, maybe one of them is a leader
        if (!t_started(D, x, i)) continue;
        uint32_t ix, tm;
        if (t_start(D, x, i, xv, ix, tm, bit(lm, i))) { idx = ix; has = true; }
        if (x.code != RUN) return;
      }
      if (!has) { sleep_ms = 79u + me * 17u; break; }
      toi = 0;
      pc = 1;
    }
    // for to in [10, 20, 50, 100, 200] { if let Some(cmd) = n_committed(index) ...; sleep(to) }
    uint64_t v;
    const uint32_t cnt = n_committed(D, x, idx, v);
    if (cnt > 0) {
      if (v == xv) {
        const uint32_t nv = KT(KT_W + 4, slot);
        if (nv >= CHURN_VCAP) { fail(D, x, MR_FAIL_SIM_CAPACITY); return; }
        const size_t vi = ((size_t)x.c * 3 + GI(me, 3, G_CHURN)) * CHURN_VCAP + nv;
        D.cval[vi] = v;
        D.cidx[vi] = idx;
        KT(KT_W + 4, slot) = nv + 1u;
      }
      pc = 0;
      continue;
    }
    sleep_ms = toi == 0 ? 10u : toi == 1 ? 20u : toi == 2 ? 50u : toi == 3 ? 100u : 200u;
    toi++;
    if (toi == 5) pc = 0;
    break;
  }
  rec_simple(D, x, 2, tid & 0xFFu);
  KT(KT_PC, slot) = pc;
  KT(KT_W, slot) = (uint32_t)xv; KT(KT_W + 1, slot) = (uint32_t)(xv >> 32);
  KT(KT_W + 2, slot) = idx; KT(KT_W + 3, slot) = toi;
  thr_wake(D, x, slot, x.now + sleep_ms * 1000u);
}

// ---- shard_ctrler tests (src/shard_ctrler/tests.rs, tester.rs; SEMANTICS §10)
constexpr uint32_t Q_LATEST = 0xFFFFFFFFu;  // Op::Query { num: u64::MAX }
DI uint32_t ct_op(const Dev& D, X& x, uint32_t type, uint32_t a, uint32_t b) {
  const uint32_t id = CS(CS_NOPS);
  if (id >= OP_CAP) { fail(D, x, MR_FAIL_SIM_CAPACITY); return 0u; }
  uint32_t* op = OPP(id);
  op[OP_TYPE] = type; op[OP_A] = a; op[OP_B] = b; op[OP_NG] = 0u;
  CS(CS_NOPS) = id + 1u;
  return id;
}
DI void ct_grp(const Dev& D, X& x, uint32_t id, uint32_t gid, uint32_t addr) {  // groups! / gids entry
  uint32_t* op = OPP(id);
  const uint32_t ng = op[OP_NG];
  op[OP_GID + ng] = gid; op[OP_ADDR + ng] = addr; op[OP_NG] = ng + 1u;
}
DI uint32_t addrs(uint32_t n, uint32_t a0, uint32_t a1, uint32_t a2) {  // addrs![..] (`as u8`)
  return n | (a0 & 255u) << 8 | (n > 1 ? (a1 & 255u) << 16 : 0u) | (n > 2 ? (a2 & 255u) << 24 : 0u);
}
// a config reference: (answering server << 8) | index in its store
DI const uint32_t* cref(const Dev& D, const X& x, uint32_t r) { return CFGP(r >> 8, r & 255u); }
DI bool cfg_has(const uint32_t* c, uint32_t gid) {
  for (uint32_t g = 0; g < c[CF_NG]; g++) if (c[CF_GID + g] == gid) return true;
  return false;
}
DI bool cfg_eq(const uint32_t* a, const uint32_t* b) {
  if (a[CF_NUM] != b[CF_NUM] || a[CF_NG] != b[CF_NG]) return false;
  for (uint32_t j = 0; j < N_SHARDS; j++) if (a[CF_SHARDS + j] != b[CF_SHARDS + j]) return false;
  for (uint32_t g = 0; g < a[CF_NG]; g++)
    if (a[CF_GID + g] != b[CF_GID + g] || a[CF_ADDR + g] != b[CF_ADDR + g]) return false;
  return true;
}
// Clerk::check (tester.rs:113-150) on a queried config; gids = first + k * step
DI void ct_check(const Dev& D, X& x, uint32_t r, uint32_t ng, uint32_t first, uint32_t step) {
  const uint32_t* c = cref(D, x, r);
  if (c[CF_NG] != ng) { fail(D, x, MR_FAIL_CTRL_NGROUPS); return; }
  for (uint32_t k = 0; k < ng; k++)
    if (!cfg_has(c, first + k * step)) { fail(D, x, MR_FAIL_CTRL_MISSING); return; }
  if (ng == 0)
    for (uint32_t j = 0; j < N_SHARDS; j++)
      if (c[CF_SHARDS + j] != 0u && !cfg_has(c, c[CF_SHARDS + j])) { fail(D, x, MR_FAIL_CTRL_INVALID); return; }
  if (c[CF_NG]) {
    uint32_t mn = ~0u, mx = 0;
    for (uint32_t g = 0; g < c[CF_NG]; g++) {
      uint32_t k = 0;
      for (uint32_t j = 0; j < N_SHARDS; j++) k += c[CF_SHARDS + j] == c[CF_GID + g] ? 1u : 0u;
      mn = k < mn ? k : mn;
      mx = k > mx ? k : mx;
    }
    if (mx > mn + 1) fail(D, x, MR_FAIL_CTRL_IMBALANCED);
  }
}
DI void ct_servers(const Dev& D, X& x, uint32_t r, uint32_t gid, uint32_t addr) {  // cfx.groups[&gid] == addr
  const uint32_t* c = cref(D, x, r);
  for (uint32_t g = 0; g < c[CF_NG]; g++)
    if (c[CF_GID + g] == gid) {
      if (c[CF_ADDR + g] != addr) fail(D, x, MR_FAIL_CTRL_SERVERS);
      return;
    }
  fail(D, x, MR_FAIL_CTRL_SERVERS);  // HashMap index panics
}
// !(b.shards[j] == i && a.shards[j] != i) for i in 1..=npara (tests.rs:133-159)
DI void ct_minimal(const Dev& D, X& x, uint32_t ra, uint32_t rb, uint32_t npara, uint32_t code) {
  const uint32_t *a = cref(D, x, ra), *b = cref(D, x, rb);
  for (uint32_t i = 1; i <= npara; i++)
    for (uint32_t j = 0; j < N_SHARDS; j++)
      if (b[CF_SHARDS + j] == i && a[CF_SHARDS + j] != i) { fail(D, x, code); return; }
}
DI uint32_t ct_leader(const Dev& D, X& x) {  // Tester::leader (tester.rs:76-87); NONE if none
  for (uint32_t i = 0; i < D.n; i++)
    if (bit(x.alive, i) && bit(t_leaders(D, x), i)) return i;
  return NONE;
}
#define CT_TO(idexpr, s)                                                                  \
  {                                                                                       \
    const uint32_t id_ = (idexpr);                                                        \
    if (x.code != RUN) return;                                                            \
    t.h[0] = 0u; clerk_begin(D, x, 0, 0, 0, id_); t.helper = H_CALL; t.pc = (s); x.yield = 2; return; \
  }
#define QUERY_TO(num, s) CT_TO(ct_op(D, x, CT_QUERY, (num), 0u), s)
#define REF (((uint32_t)t.hv << 8) | t.res)
#define JOIN1_TO(gid, ad, s)                                                             \
  {                                                                                      \
    const uint32_t jid_ = ct_op(D, x, CT_JOIN, 0u, 0u);                                  \
    CK();                                                                                \
    ct_grp(D, x, jid_, (gid), (ad));                                                     \
    CT_TO(jid_, s)                                                                       \
  }
#define LEAVE1_TO(gid, s)                                                                \
  {                                                                                      \
    const uint32_t lid_ = ct_op(D, x, CT_LEAVE, 0u, 0u);                                 \
    CK();                                                                                \
    ct_grp(D, x, lid_, (gid), 0u);                                                       \
    CT_TO(lid_, s)                                                                       \
  }

// a concurrent client task (tests.rs:110-117 / 224-233) with its own clerk (slot 1 + i)
template <uint32_t S>
DI void ctl_client_step(const Dev& D, X& x, uint32_t slot) {
  constexpr bool multi = S == MR_SCN_CTRL_MULTI_4A;
  constexpr uint32_t nops = multi ? 2u : 3u;
  const uint32_t tid = KT(KT_TID, slot), gid = KT(KT_CLI, slot);
  uint32_t pc = KT(KT_PC, slot);
  if (pc == 0 || clerk_resume(D, x, slot)) {
    if (x.code != RUN) return;
    if (pc == nops) {
      rec_simple(D, x, 2, tid & 0xFFu);
      thr_finish(D, x, slot);
      return;
    }
    uint32_t id;
    if (!multi) {
      id = ct_op(D, x, pc < 2 ? CT_JOIN : CT_LEAVE, 0u, 0u);
      if (x.code != RUN) return;
      if (pc == 0) ct_grp(D, x, id, gid + 1000u, addrs(1, gid + 1u, 0, 0));
      else if (pc == 1) ct_grp(D, x, id, gid, addrs(1, gid + 2u, 0, 0));
      else ct_grp(D, x, id, gid + 1000u, 0u);
    } else {
      id = ct_op(D, x, pc == 0 ? CT_JOIN : CT_LEAVE, 0u, 0u);
      if (x.code != RUN) return;
      if (pc == 0) {
        ct_grp(D, x, id, gid, addrs(3, gid + 1u, gid + 2u, gid + 3u));
        ct_grp(D, x, id, gid + 1000u, addrs(1, gid + 1001u, 0, 0));
        ct_grp(D, x, id, gid + 2000u, addrs(1, gid + 2001u, 0, 0));
      } else {
        ct_grp(D, x, id, gid + 1000u, 0u);
        ct_grp(D, x, id, gid + 2000u, 0u);
      }
    }
    KT(KT_PC, slot) = pc + 1u;
    clerk_begin(D, x, slot, 0, 0, id);
  }
  if (x.code != RUN) return;
  rec_simple(D, x, 2, tid & 0xFFu);
}

DI void ct_init(const Dev& D, X& x, T& t) {  // Tester::new(3, false) + ck = make_client()
  t_new(D, x, false);
  x.conn |= 0xFFFFFF00u;  // clerk hosts
}

DI void scn_ctrl_basic(const Dev& D, X& x, T& t) {  // basic_4a, shard_ctrler/tests.rs:24-166
  constexpr uint32_t npara = 10;
  uint32_t& i = t.l[0];
  uint32_t& k = t.l[1];
  uint32_t& cf = t.l[2];
  uint32_t& c1 = t.l[3];
  uint32_t& c2 = t.l[4];
  for (;;) switch (t.pc) {
    case 0: ct_init(D, x, t); QUERY_TO(Q_LATEST, 1)
    case 1: TV(0) = REF; QUERY_TO(Q_LATEST, 2)
    case 2: ct_check(D, x, REF, 0, 0, 0); CK(); JOIN1_TO(1u, addrs(3, 11, 12, 13), 3)
    case 3: QUERY_TO(Q_LATEST, 4)
    case 4: ct_check(D, x, REF, 1, 1, 1); CK(); QUERY_TO(Q_LATEST, 5)
    case 5: TV(1) = REF; JOIN1_TO(2u, addrs(3, 21, 22, 23), 6)
    case 6: QUERY_TO(Q_LATEST, 7)
    case 7: ct_check(D, x, REF, 2, 1, 1); CK(); QUERY_TO(Q_LATEST, 8)
    case 8: TV(2) = REF; QUERY_TO(Q_LATEST, 9)
    case 9:
      ct_servers(D, x, REF, 1u, addrs(3, 11, 12, 13)); CK();
      ct_servers(D, x, REF, 2u, addrs(3, 21, 22, 23)); CK();
      LEAVE1_TO(1u, 10)
    case 10: QUERY_TO(Q_LATEST, 11)
    case 11: ct_check(D, x, REF, 1, 2, 0); CK(); QUERY_TO(Q_LATEST, 12)
    case 12: TV(3) = REF; LEAVE1_TO(2u, 13)
    case 13: QUERY_TO(Q_LATEST, 14)
    case 14: TV(4) = REF; i = 0; GO(15)
    case 15:  // Historical queries: each server down in turn
      if (i >= D.n) JOIN1_TO(503u, addrs(3, 31, 32, 33), 18)
      t_crash1(D, x, i);
      k = 0;
      GO(16)
    case 16:
      if (k >= 5) { t_start1(D, x, i); i++; GO(15) }
      QUERY_TO(cref(D, x, (uint32_t)TV(k))[CF_NUM], 17)
    case 17:
      if (!cfg_eq(cref(D, x, REF), cref(D, x, (uint32_t)TV(k)))) { fail(D, x, MR_FAIL_CTRL_HISTORY); return; }
      k++;
      GO(16)
    case 18: JOIN1_TO(504u, addrs(3, 41, 42, 43), 19)
    case 19: i = 0; GO(20)
    case 20:  // Move
      if (i >= N_SHARDS) QUERY_TO(Q_LATEST, 24)
      QUERY_TO(Q_LATEST, 21)
    case 21: cf = REF; CT_TO(ct_op(D, x, CT_MOVE, i, i < N_SHARDS / 2 ? 503u : 504u), 22)
    case 22:
      if (cref(D, x, cf)[CF_SHARDS + i] != (i < N_SHARDS / 2 ? 503u : 504u)) QUERY_TO(Q_LATEST, 23)
      i++;
      GO(20)
    case 23:
      if (!(cref(D, x, REF)[CF_NUM] > cref(D, x, cf)[CF_NUM])) { fail(D, x, MR_FAIL_CTRL_MOVE_NUM); return; }
      i++;
      GO(20)
    case 24:
      for (uint32_t j = 0; j < N_SHARDS; j++)
        if (cref(D, x, REF)[CF_SHARDS + j] != (j < N_SHARDS / 2 ? 503u : 504u)) {
          fail(D, x, MR_FAIL_CTRL_MOVE_WRONG);
          return;
        }
      LEAVE1_TO(503u, 25)
    case 25: LEAVE1_TO(504u, 26)
    case 26:  // Concurrent leave/join
      for (uint32_t q = 0; q < npara; q++) kv_spawn(D, x, 1 + q, 1 + q, q * 10u + 100u);
      JOINALL_TO(27)
    case 27: QUERY_TO(Q_LATEST, 28)
    case 28: ct_check(D, x, REF, npara, 100, 10); CK(); QUERY_TO(Q_LATEST, 29)
    case 29: c1 = REF; i = 0; GO(30)
    case 30:  // Minimal transfers after joins
      if (i >= 5) QUERY_TO(Q_LATEST, 32)
      JOIN1_TO(npara + 1 + i, addrs(3, npara + 2 + i, npara + 3 + i, npara + 3 + i), 31)
    case 31: i++; GO(30)
    case 32: c2 = REF; ct_minimal(D, x, c1, c2, npara, MR_FAIL_CTRL_MINIMAL_JOIN); CK(); i = 0; GO(33)
    case 33:  // Minimal transfers after leaves
      if (i >= 5) QUERY_TO(Q_LATEST, 35)
      LEAVE1_TO(npara + 1 + i, 34)
    case 34: i++; GO(33)
    case 35: ct_minimal(D, x, REF, c2, npara, MR_FAIL_CTRL_MINIMAL_LEAVE); CK(); END()
    BAD()
  }
}

DI void scn_ctrl_multi(const Dev& D, X& x, T& t) {  // multi_4a, shard_ctrler/tests.rs:168-299
  constexpr uint32_t npara = 10;
  uint32_t& c1 = t.l[0];
  uint32_t& c2 = t.l[1];
  uint32_t& cc = t.l[2];
  uint32_t& att = t.l[3];
  for (;;) switch (t.pc) {
    case 0: ct_init(D, x, t); QUERY_TO(Q_LATEST, 1)
    case 1: QUERY_TO(Q_LATEST, 2)
    case 2: {
      ct_check(D, x, REF, 0, 0, 0); CK();
      const uint32_t id = ct_op(D, x, CT_JOIN, 0u, 0u); CK();
      ct_grp(D, x, id, 1u, addrs(3, 11, 12, 13)); ct_grp(D, x, id, 2u, addrs(3, 21, 22, 23));
      CT_TO(id, 3)
    }
    case 3: QUERY_TO(Q_LATEST, 4)
    case 4: ct_check(D, x, REF, 2, 1, 1); CK(); QUERY_TO(Q_LATEST, 5)
    case 5: JOIN1_TO(3u, addrs(3, 31, 32, 33), 6)
    case 6: QUERY_TO(Q_LATEST, 7)
    case 7: ct_check(D, x, REF, 3, 1, 1); CK(); QUERY_TO(Q_LATEST, 8)
    case 8: QUERY_TO(Q_LATEST, 9)
    case 9: {
      ct_servers(D, x, REF, 1u, addrs(3, 11, 12, 13)); CK();
      ct_servers(D, x, REF, 2u, addrs(3, 21, 22, 23)); CK();
      ct_servers(D, x, REF, 3u, addrs(3, 31, 32, 33)); CK();
      const uint32_t id = ct_op(D, x, CT_LEAVE, 0u, 0u); CK();
      ct_grp(D, x, id, 1u, 0u); ct_grp(D, x, id, 3u, 0u);
      CT_TO(id, 10)
    }
    case 10: QUERY_TO(Q_LATEST, 11)
    case 11: ct_check(D, x, REF, 1, 2, 0); CK(); QUERY_TO(Q_LATEST, 12)
    case 12: QUERY_TO(Q_LATEST, 13)
    case 13: ct_servers(D, x, REF, 2u, addrs(3, 21, 22, 23)); CK(); LEAVE1_TO(2u, 14)
    case 14:  // Concurrent multi leave/join
      for (uint32_t q = 0; q < npara; q++) kv_spawn(D, x, 1 + q, 1 + q, q + 1000u);
      JOINALL_TO(15)
    case 15: QUERY_TO(Q_LATEST, 16)
    case 16: ct_check(D, x, REF, npara, 1000, 1); CK(); QUERY_TO(Q_LATEST, 17)
    case 17: {  // Minimal transfers after multijoins
      c1 = REF;
      const uint32_t id = ct_op(D, x, CT_JOIN, 0u, 0u); CK();
      for (uint32_t q = 0; q < 5; q++) {
        const uint32_t gid = npara + 1 + q;
        ct_grp(D, x, id, gid, addrs(2, gid + 1, gid + 2, 0));
      }
      CT_TO(id, 18)
    }
    case 18: QUERY_TO(Q_LATEST, 19)
    case 19: {
      c2 = REF;
      ct_minimal(D, x, c1, c2, npara, MR_FAIL_CTRL_MINIMAL_JOIN); CK();
      const uint32_t id = ct_op(D, x, CT_LEAVE, 0u, 0u); CK();
      for (uint32_t q = 0; q < 5; q++) ct_grp(D, x, id, npara + 1 + q, 0u);
      CT_TO(id, 20)
    }
    case 20: QUERY_TO(Q_LATEST, 21)
    case 21:
      ct_minimal(D, x, REF, c2, npara, MR_FAIL_CTRL_MINIMAL_LEAVE); CK();
      att = ct_leader(D, x);  // Check Same config on servers
      if (att == NONE) { fail(D, x, MR_FAIL_CTRL_NO_LEADER); return; }
      QUERY_TO(Q_LATEST, 22)
    case 22: cc = REF; t_crash1(D, x, att); att = 0; GO(23)
    case 23:
      if (ct_leader(D, x) == NONE) QUERY_TO(Q_LATEST, 24)
      att++;
      if (!(att < 3)) { fail(D, x, MR_FAIL_CTRL_NO_LEADER); return; }
      SLEEP_TO(1000000u, 23)
    case 24:
      if (!cfg_eq(cref(D, x, cc), cref(D, x, REF))) { fail(D, x, MR_FAIL_CTRL_SAME_CONFIG); return; }
      END()
    BAD()
  }
}

template <uint32_t S>
DI void thr_step(const Dev& D, X& x, uint32_t slot) {
  if constexpr (is_kv(S)) {
    KC c;
    const KCR kc{&c, true};
    kc_load(D, x, slot, c);
    c.kvdone = CS(CS_KVDONE);
    const uint32_t kind = KR(KT_KIND);
    if (kv_gen(S).part && kind == 1u) part_step(D, x, slot, kc);
    else if (mr_scn_is_lin15(S)) lin_client_step(D, x, slot, kc);  // kind 4 (§9b)
    else if (kind >= 2u) kv_task_step(D, x, slot, kc);
    else kv_client_step(D, x, slot, kc);
  }
  else if constexpr (is_ctrl(S)) ctl_client_step<S>(D, x, slot);
  else if constexpr (mr_scn_is_churn(S)) churn_step<S>(D, x, slot);
  else agree_thr_step(D, x, slot);
}

DI void scn_unreliable_agree(const Dev& D, X& x, T& t) {  // tests.rs:662-686
  constexpr uint32_t NT = nthr(MR_SCN_UNRELIABLE_AGREE_2C);
  uint32_t& it = t.l[0];
  uint32_t& ntid = t.l[1];
  for (;;) switch (t.pc) {
    case 0: t_new(D, x, false); t_set_unrel(x, true); it = 1; ntid = 1; GO(1)
    case 1:
      if (it >= 50) { t_set_unrel(x, false); JOINALL_TO(3) }
      for (uint32_t j = 0; j < 4; j++) {  // dones.push(task::spawn_local(one(100 * iters + j)))
        uint32_t slot = NT;
        for (uint32_t s = NT - 1; s >= 1; s--)
          if (!KT(KT_LIVE, s)) slot = s;
        if (slot == NT) { fail(D, x, MR_FAIL_SIM_CAPACITY); return; }
        thr_spawn(D, x, slot, ntid++);
        T f;
        one_init(D, x, f, 100ull * it + j, 1, true);
#pragma unroll
        for (uint32_t k = 0; k < T_NH; k++) KT(KT_W + k, slot) = f.h[k];
        KT(KT_W + T_NH, slot) = (uint32_t)f.hv;
        KT(KT_W + T_NH + 1, slot) = (uint32_t)(f.hv >> 32);
      }
      ONE_TO(it, 1, true, 2)
    case 2: it++; GO(1)
    case 3: ONE_TO(100, D.n, true, 4)
    case 4: END()
    BAD()
  }
}

DI void scn_churn(const Dev& D, X& x, T& t, bool unreliable) {  // internal_churn, tests.rs:755-856
  const uint32_t n = D.n;
  uint32_t& it = t.l[0];
  uint32_t& last = t.l[1];
  uint32_t& index = t.l[2];
  for (;;) switch (t.pc) {
    case 0:
      t_new(D, x, false);
      t_set_unrel(x, unreliable);
      CS(CS_KVDONE) = 0u;  // stop
      for (uint32_t i = 0; i < 3; i++) thr_spawn(D, x, 1 + i, 1 + i);  // ncli = 3
      it = 0;
      GO(1)
    case 1:
      if (it >= 20) SLEEP_TO(ELECTION_US, 3)
      if (t_bool(D, x, 858993459u)) t_conn(D, x, t_range(D, x, 0, n), 0);  // gen_bool(0.2)
      if (t_bool(D, x, 0x80000000u)) {
        const uint32_t i = t_range(D, x, 0, n);
        if (!t_started(D, x, i)) t_start1(D, x, i);
        t_conn(D, x, i, 1);
      }
      if (t_bool(D, x, 858993459u)) {
        const uint32_t i = t_range(D, x, 0, n);
        if (t_started(D, x, i)) t_crash1(D, x, i);
      }
      SLEEP_TO(ELECTION_US * 7 / 10, 2)
    case 2: it++; GO(1)
    case 3:
      t_set_unrel(x, false);
      for (uint32_t i = 0; i < n; i++) {
        if (!t_started(D, x, i)) t_start1(D, x, i);
        t_conn(D, x, i, 1);
      }
      CS(CS_KVDONE) = 1u;
      SLEEP_TO(ELECTION_US, 4)
    case 4: ONE_TO(t_entry(D, x), n, true, 5)
    case 5: last = t.res; index = 1; GO(6)
    case 6:
      if (index > last) JOINALL_TO(8)
      WAIT_TO(index, n, false, 0, 7)
    case 7: index++; GO(6)
    case 8:
      for (uint32_t c = 0; c < 3; c++) {  // really.contains(v1), tests.rs:851-853
        const uint32_t nv = KT(KT_W + 4, 1 + c);
        for (uint32_t k = 0; k < nv; k++) {
          const size_t vi = ((size_t)x.c * 3 + c) * CHURN_VCAP + k;
          const uint64_t v1 = D.cval[vi];
          uint64_t w;
          uint32_t ix = D.cidx[vi];
          bool found = ix <= last && n_committed(D, x, ix, w) > 0 && w == v1;  // where it was seen
          for (ix = 1; ix <= last && !found; ix++) found = n_committed(D, x, ix, w) > 0 && w == v1;
          if (!found) { fail(D, x, MR_FAIL_CHURN_VALUE); return; }
        }
      }
      END()
    BAD()
  }
}

template <uint32_t S>
DI void run_scenario(const Dev& D, X& x, T& t) {
  switch (S) {
    case MR_SCN_INITIAL_ELECTION_2A: scn_initial_election(D, x, t); break;
    case MR_SCN_REELECTION_2A: scn_reelection(D, x, t); break;
    case MR_SCN_MANY_ELECTION_2A: scn_many_election(D, x, t); break;
    case MR_SCN_BASIC_AGREE_2B: scn_basic_agree(D, x, t); break;
    case MR_SCN_FAIL_AGREE_2B: scn_fail_agree(D, x, t); break;
    case MR_SCN_FAIL_NO_AGREE_2B: scn_fail_no_agree(D, x, t); break;
    case MR_SCN_CONCURRENT_STARTS_2B: scn_concurrent_starts(D, x, t); break;
    case MR_SCN_REJOIN_2B: scn_rejoin(D, x, t); break;
    case MR_SCN_BACKUP_2B: scn_backup(D, x, t); break;
    case MR_SCN_COUNT_2B: scn_count(D, x, t); break;
    case MR_SCN_PERSIST1_2C: scn_persist1(D, x, t); break;
    case MR_SCN_PERSIST2_2C: scn_persist2(D, x, t); break;
    case MR_SCN_PERSIST3_2C: scn_persist3(D, x, t); break;
    case MR_SCN_FIGURE_8_2C: scn_figure_8(D, x, t, false); break;
    case MR_SCN_FIGURE_8_UNRELIABLE_CRASH: scn_figure_8(D, x, t, true); break;
    case MR_SCN_FIGURE_8_UNRELIABLE_2C: scn_figure_8_unreliable(D, x, t); break;
    case MR_SCN_SNAPSHOT_BASIC_2D: scn_snap_common(D, x, t, false, true, false); break;
    case MR_SCN_SNAPSHOT_INSTALL_2D: scn_snap_common(D, x, t, true, true, false); break;
    case MR_SCN_SNAPSHOT_INSTALL_UNRELIABLE_2D: scn_snap_common(D, x, t, true, false, false); break;
    case MR_SCN_SNAPSHOT_INSTALL_CRASH_2D: scn_snap_common(D, x, t, false, true, true); break;
    case MR_SCN_SNAPSHOT_INSTALL_UNRELIABLE_CRASH_2D:
      scn_snap_common(D, x, t, false, false, true);
      break;
    case MR_SCN_UNRELIABLE_AGREE_2C: scn_unreliable_agree(D, x, t); break;
    case MR_SCN_RELIABLE_CHURN_2C: scn_churn(D, x, t, false); break;
    case MR_SCN_UNRELIABLE_CHURN_2C: scn_churn(D, x, t, true); break;
    case MR_SCN_CTRL_BASIC_4A: scn_ctrl_basic(D, x, t); break;
    case MR_SCN_CTRL_MULTI_4A: scn_ctrl_multi(D, x, t); break;
    case MR_SCN_KV_UNRELIABLE_ONE_KEY_3A: scn_kv_one_key(D, x, t); break;
    case MR_SCN_KV_ONE_PARTITION_3A: scn_kv_one_partition(D, x, t); break;
    case MR_SCN_KV_SNAPSHOT_RPC_3B: scn_kv_snapshot_rpc(D, x, t); break;
    case MR_SCN_KV_SNAPSHOT_SIZE_3B: scn_kv_snapshot_size(D, x, t); break;
    default:
      if constexpr (is_kv(S)) { scn_kv_generic<S>(D, x, t); break; }
      fail(D, x, MR_FAIL_SIM_BAD_PROGRAM);
      return;
  }
}

