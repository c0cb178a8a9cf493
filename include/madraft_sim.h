/*
 * madraft_sim.h — C ABI of the MI355X batched deterministic Raft simulator.
 *
 * This is the drop-in boundary for the reference's hot path: the single-seed
 * MadSim executor + simulated network + Raft node + persister + tester that
 * `MADSIM_TEST_NUM=N cargo test <name>` runs once per seed
 * (/root/reference/README.md:44-66). One `mr_batch` runs `n_clusters`
 * independent seeds of one reference test in lockstep on one GPU.
 *
 * Interfaces replaced (reference file:line):
 *   - `#[madsim::test]` seed loop + MADSIM_TEST_SEED/NUM  (README.md:44-66)
 *       -> mr_batch_create / mr_batch_run / mr_batch_verdicts
 *   - RaftTester::new/one/wait/check_* / end                (src/raft/tester.rs:34-358)
 *       -> scenario programs executed inside mr_batch_run
 *   - RaftHandle::{new,start,term,is_leader,snapshot,cond_install_snapshot}
 *                                                            (src/raft/raft.rs:107-168)
 *       -> device Raft node state machine inside mr_batch_run
 *   - madsim net stat().msg_count, fs get_file_size          (src/raft/tester.rs:147-158)
 *       -> mr_counters, persisted-size model
 *   - panic!(...) + "MADSIM_TEST_SEED=" report               (README.md:44-48)
 *       -> per-cluster fail code (MR_FAIL_*) + fail time; mr_fail_message()
 *
 * Conventions: plain C types, caller-owned buffers, int status (0 = ok,
 * <0 = error, message in mr_last_error()). One mr_batch per device; a batch is
 * not thread-safe. The exact simulation semantics are in docs/SEMANTICS.md.
 */
#ifndef MADRAFT_SIM_H
#define MADRAFT_SIM_H

#include <stddef.h>
#include <stdint.h>
#include <string.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MR_ABI_VERSION 7u
#define MR_MAX_NODES 8u
#define MR_MAX_MSG_SLOTS 256u
#define MR_MAX_AE 32u

/* ---- scenarios: one id per reference #[madsim::test] (src/raft/tests.rs) ----
 * The one place that describes a scenario; enum mr_scenario, the names, the defaults of mr_cfg_init
 * and of the oracle's mro_cfg_init (mr_cfg_defaults below), the kernel instances built and
 * dispatched to and the Python mirror are generated from these rows:
 *   X(id, SYMBOL, "test name", servers, kind, slots, exact, pool)
 *   kind   RAFT, KV (kvraft generic_test and its variants) or CTRL (shard_ctrler)
 *   slots  default mr_cfg.msg_slots: 32, 64, or 256 (clerks keep more than 64 messages in flight)
 *   exact  server counts with a kernel instance of exactly that size: bit n set for n servers
 *          (0x08 = 3, 0x20 = 5, 0x80 = 7); any other count runs the 8-server instance
 *   pool   pool-kernel family built at those counts: NONE, RAFT (Raft-only test bodies without
 *          spawned threads) or SVC (kvraft / shard_ctrler bodies)
 * `exact` is a hex literal and `pool` a bare word so that _abi.py reads the rows as text. */
#define MR_SCENARIO_TABLE(X) \
  X(1, INITIAL_ELECTION_2A, "initial_election_2a", 3, RAFT, 32, 0x08, RAFT)   /* tests.rs:20-46   */ \
  X(2, REELECTION_2A, "reelection_2a", 3, RAFT, 32, 0x08, RAFT)               /* tests.rs:48-78   */ \
  X(3, MANY_ELECTION_2A, "many_election_2a", 7, RAFT, 32, 0x80, RAFT)         /* tests.rs:80-112  */ \
  X(4, BASIC_AGREE_2B, "basic_agree_2b", 5, RAFT, 32, 0x20, RAFT)             /* tests.rs:114-130 */ \
  X(5, FAIL_AGREE_2B, "fail_agree_2b", 3, RAFT, 32, 0x28, RAFT)               /* tests.rs:132-161 */ \
  X(6, FAIL_NO_AGREE_2B, "fail_no_agree_2b", 5, RAFT, 32, 0x20, RAFT)         /* tests.rs:163-209 */ \
  X(7, CONCURRENT_STARTS_2B, "concurrent_starts_2b", 3, RAFT, 32, 0x08, RAFT) /* tests.rs:211-275 */ \
  X(8, REJOIN_2B, "rejoin_2b", 3, RAFT, 32, 0x08, RAFT)                       /* tests.rs:277-313 */ \
  X(9, BACKUP_2B, "backup_2b", 5, RAFT, 32, 0x20, RAFT)                       /* tests.rs:315-386 */ \
  X(10, COUNT_2B, "count_2b", 3, RAFT, 32, 0x08, RAFT)                        /* tests.rs:388-479 */ \
  X(11, PERSIST1_2C, "persist1_2c", 3, RAFT, 32, 0x08, RAFT)                  /* tests.rs:481-526 */ \
  X(12, PERSIST2_2C, "persist2_2c", 5, RAFT, 32, 0x20, RAFT)                  /* tests.rs:528-572 */ \
  X(13, PERSIST3_2C, "persist3_2c", 3, RAFT, 32, 0x08, RAFT)                  /* tests.rs:574-602 */ \
  X(14, FIGURE_8_2C, "figure_8_2c", 5, RAFT, 32, 0x20, RAFT)                  /* tests.rs:612-660 */ \
  /* spawned tester threads (one() tasks, churn clients): no pool kernel */ \
  X(15, UNRELIABLE_AGREE_2C, "unreliable_agree_2c", 5, RAFT, 32, 0x20, NONE)  /* tests.rs:662-686 */ \
  X(16, FIGURE_8_UNRELIABLE_2C, "figure_8_unreliable_2c", 5, RAFT, 32, 0x20, RAFT) /* tests.rs:688-741 */ \
  X(17, RELIABLE_CHURN_2C, "reliable_churn_2c", 5, RAFT, 32, 0x20, NONE)      /* tests.rs:743-747 */ \
  X(18, UNRELIABLE_CHURN_2C, "unreliable_churn_2c", 5, RAFT, 32, 0x20, NONE)  /* tests.rs:749-753 */ \
  X(19, SNAPSHOT_BASIC_2D, "snapshot_basic_2d", 3, RAFT, 32, 0x88, RAFT)      /* tests.rs:913-917 */ \
  X(20, SNAPSHOT_INSTALL_2D, "snapshot_install_2d", 3, RAFT, 32, 0x88, RAFT)  /* tests.rs:919-923 */ \
  X(21, SNAPSHOT_INSTALL_UNRELIABLE_2D, "snapshot_install_unreliable_2d", 3, RAFT, 32, 0x88, RAFT) /* tests.rs:925-929 */ \
  X(22, SNAPSHOT_INSTALL_CRASH_2D, "snapshot_install_crash_2d", 3, RAFT, 32, 0x88, RAFT) /* tests.rs:931-935 */ \
  X(23, SNAPSHOT_INSTALL_UNRELIABLE_CRASH_2D, "snapshot_install_unreliable_crash_2d", 3, RAFT, 32, 0x88, RAFT) /* tests.rs:937-941 */ \
  /* BASELINE.json config 3 read literally: figure_8_unreliable_2c's loop with \
   * crash1/start1 (figure_8_2c, tests.rs:638-649) in place of disconnect. */ \
  X(24, FIGURE_8_UNRELIABLE_CRASH, "figure_8_unreliable_crash", 5, RAFT, 32, 0x20, RAFT) \
  /* kvraft generic_test (src/kvraft/tests.rs:65-220) over 5 servers; BASELINE config 5 */ \
  X(25, KV_BASIC_3A, "basic_3a", 5, KV, 64, 0x20, SVC)             /* kvraft/tests.rs:222-226: 1 client      */ \
  X(26, KV_CONCURRENT_3A, "concurrent_3a", 5, KV, 64, 0x20, SVC)   /* kvraft/tests.rs:228-232: 5 clients     */ \
  X(27, KV_UNRELIABLE_3A, "unreliable_3a", 5, KV, 64, 0x20, SVC)   /* kvraft/tests.rs:234-238: 5, unreliable */ \
  /* shard_ctrler (src/shard_ctrler/tests.rs) over 3 servers */ \
  X(28, CTRL_BASIC_4A, "basic_4a", 3, CTRL, 32, 0x08, SVC)         /* shard_ctrler/tests.rs:24-166  */ \
  X(29, CTRL_MULTI_4A, "multi_4a", 3, CTRL, 32, 0x08, SVC)         /* shard_ctrler/tests.rs:168-299 */ \
  /* kvraft generic_test with partitions / restarts (src/kvraft/tests.rs:344-385) */ \
  X(30, KV_MANY_PARTITIONS_ONE_CLIENT_3A, "many_partitions_one_client_3a", 5, KV, 64, 0x20, SVC)     /* kvraft/tests.rs:344-348 */ \
  X(31, KV_MANY_PARTITIONS_MANY_CLIENTS_3A, "many_partitions_many_clients_3a", 5, KV, 64, 0x20, SVC) /* kvraft/tests.rs:350-354 */ \
  X(32, KV_PERSIST_ONE_CLIENT_3A, "persist_one_client_3a", 5, KV, 64, 0x20, SVC)                     /* kvraft/tests.rs:356-360 */ \
  X(33, KV_PERSIST_CONCURRENT_3A, "persist_concurrent_3a", 5, KV, 64, 0x20, SVC)                     /* kvraft/tests.rs:362-366 */ \
  X(34, KV_PERSIST_CONCURRENT_UNRELIABLE_3A, "persist_concurrent_unreliable_3a", 5, KV, 64, 0x20, SVC) /* kvraft/tests.rs:368-372 */ \
  X(35, KV_PERSIST_PARTITION_3A, "persist_partition_3a", 5, KV, 64, 0x20, SVC)                       /* kvraft/tests.rs:374-378 */ \
  X(36, KV_PERSIST_PARTITION_UNRELIABLE_3A, "persist_partition_unreliable_3a", 5, KV, 64, 0x20, SVC) /* kvraft/tests.rs:380-384 */ \
  X(37, KV_UNRELIABLE_ONE_KEY_3A, "unreliable_one_key_3a", 3, KV, 64, 0x08, SVC)                     /* kvraft/tests.rs:240-274 */ \
  X(38, KV_ONE_PARTITION_3A, "one_partition_3a", 5, KV, 64, 0x20, SVC)                               /* kvraft/tests.rs:276-342 */ \
  /* kvraft 3B: services snapshot under maxraftstate = 1000 */ \
  X(39, KV_SNAPSHOT_RPC_3B, "snapshot_rpc_3b", 3, KV, 64, 0x08, SVC)           /* kvraft/tests.rs:396-454 */ \
  X(40, KV_SNAPSHOT_SIZE_3B, "snapshot_size_3b", 3, KV, 64, 0x08, SVC)         /* kvraft/tests.rs:456-492 */ \
  X(41, KV_SNAPSHOT_RECOVER_3B, "snapshot_recover_3b", 5, KV, 64, 0x20, SVC)   /* kvraft/tests.rs:494-498 */ \
  /* 20 clerks: 256 message slots and clerk hosts that do not fit the service pool */ \
  X(42, KV_SNAPSHOT_RECOVER_MANY_CLIENTS_3B, "snapshot_recover_many_clients_3b", 5, KV, 256, 0x20, NONE) /* kvraft/tests.rs:500-504 */ \
  X(43, KV_SNAPSHOT_UNRELIABLE_3B, "snapshot_unreliable_3b", 5, KV, 64, 0x20, SVC)                 /* kvraft/tests.rs:506-510 */ \
  X(44, KV_SNAPSHOT_UNRELIABLE_RECOVER_3B, "snapshot_unreliable_recover_3b", 5, KV, 64, 0x20, SVC) /* kvraft/tests.rs:512-516 */ \
  X(45, KV_SNAPSHOT_UNRELIABLE_RECOVER_CONCURRENT_PARTITION_3B, "snapshot_unreliable_recover_concurrent_partition_3b", 5, KV, 64, 0x20, SVC) /* kvraft/tests.rs:518-522 */ \
  /* generic_test_linearizability (15 clients, 7 servers): the reference's commented-out \
   * kvraft/tests.rs:386-390 and 524-528, defined by the build (docs/SEMANTICS.md §9b) */ \
  X(46, KV_PERSIST_PARTITION_UNRELIABLE_LINEARIZABLE_3A, "persist_partition_unreliable_linearizable_3a", 7, KV, 64, 0x80, SVC) \
  X(47, KV_SNAPSHOT_UNRELIABLE_RECOVER_CONCURRENT_PARTITION_LINEARIZABLE_3B, "snapshot_unreliable_recover_concurrent_partition_linearizable_3b", 7, KV, 64, 0x80, SVC)

enum mr_scn_kind { MR_KIND_RAFT = 1, MR_KIND_KV = 2, MR_KIND_CTRL = 3 };  /* 0: no such scenario */
enum mr_scn_pool { MR_POOL_FAMILY_NONE = 0, MR_POOL_FAMILY_RAFT = 1, MR_POOL_FAMILY_SVC = 2 };  /* = MR_POOL */

enum mr_scenario {
  MR_SCN_NONE = 0,
#define MR_ROW_(id, sym, name, n, kind, slots, exact, pool) MR_SCN_##sym = id,
  MR_SCENARIO_TABLE(MR_ROW_)
#undef MR_ROW_
  MR_SCN_COUNT_ /* 1 + the last row's id: rows stay in id order (checked in mr_dev.h) */
};

/* Column lookups by id (0 for an id without a row); constant expressions in C++, so the kernels'
 * compile-time predicates (madraft_amd/csrc/mr_dev.h) read the same rows. */
#ifdef __cplusplus
#define MR_TABLE_FN_ static constexpr
#else
#define MR_TABLE_FN_ static inline
#endif
#define MR_COLUMN_(fn, ROW) \
  MR_TABLE_FN_ uint32_t fn(uint32_t s) { switch (s) { MR_SCENARIO_TABLE(ROW) default: return 0; } }
#define MR_ROW_N_(id, sym, name, n, kind, slots, exact, pool) case id: return n;
#define MR_ROW_KIND_(id, sym, name, n, kind, slots, exact, pool) case id: return MR_KIND_##kind;
#define MR_ROW_SLOTS_(id, sym, name, n, kind, slots, exact, pool) case id: return slots;
#define MR_ROW_EXACT_(id, sym, name, n, kind, slots, exact, pool) case id: return exact;
#define MR_ROW_POOL_(id, sym, name, n, kind, slots, exact, pool) case id: return MR_POOL_FAMILY_##pool;
MR_COLUMN_(mr_scn_servers, MR_ROW_N_)
MR_COLUMN_(mr_scn_kind, MR_ROW_KIND_)
MR_COLUMN_(mr_scn_msg_slots, MR_ROW_SLOTS_)
MR_COLUMN_(mr_scn_exact_mask, MR_ROW_EXACT_)
MR_COLUMN_(mr_scn_pool, MR_ROW_POOL_)
#undef MR_ROW_N_
#undef MR_ROW_KIND_
#undef MR_ROW_SLOTS_
#undef MR_ROW_EXACT_
#undef MR_ROW_POOL_
#undef MR_COLUMN_

/* kvraft scenarios (generic_test and its variants) */
MR_TABLE_FN_ int mr_scn_is_kv(uint32_t s) { return mr_scn_kind(s) == MR_KIND_KV; }
/* generic_test_linearizability scenarios (SEMANTICS §9b) */
MR_TABLE_FN_ int mr_scn_is_lin15(uint32_t s) {
  return s == MR_SCN_KV_PERSIST_PARTITION_UNRELIABLE_LINEARIZABLE_3A ||
         s == MR_SCN_KV_SNAPSHOT_UNRELIABLE_RECOVER_CONCURRENT_PARTITION_LINEARIZABLE_3B;
}
/* scenarios whose clerks keep more than 64 messages in flight: 256 message slots */
MR_TABLE_FN_ int mr_scn_wide_slots(uint32_t s) { return mr_scn_msg_slots(s) > 64u; }
/* the figure_8 bodies, snap_common's five 2D tests (tests.rs:913-941), the churn tests */
MR_TABLE_FN_ int mr_scn_is_fig8(uint32_t s) {
  return s == MR_SCN_FIGURE_8_2C || s == MR_SCN_FIGURE_8_UNRELIABLE_2C ||
         s == MR_SCN_FIGURE_8_UNRELIABLE_CRASH;
}
MR_TABLE_FN_ int mr_scn_is_snap2d(uint32_t s) {
  return s >= MR_SCN_SNAPSHOT_BASIC_2D && s <= MR_SCN_SNAPSHOT_INSTALL_UNRELIABLE_CRASH_2D;
}
MR_TABLE_FN_ int mr_scn_is_churn(uint32_t s) {
  return s == MR_SCN_RELIABLE_CHURN_2C || s == MR_SCN_UNRELIABLE_CHURN_2C;
}
/* default log / apply capacity of a kvraft scenario (no snapshots: every op stays in the log),
 * from the oracle's maxima: the bodies named here need more than 2048; 0 for any other id */
MR_TABLE_FN_ uint32_t mr_kv_log_cap(uint32_t s) {
  if (!mr_scn_is_kv(s)) return 0u;
  switch (s) {
    case MR_SCN_KV_SNAPSHOT_RECOVER_MANY_CLIENTS_3B: return 16384u;
    case MR_SCN_KV_CONCURRENT_3A:
    case MR_SCN_KV_MANY_PARTITIONS_MANY_CLIENTS_3A:
    case MR_SCN_KV_PERSIST_CONCURRENT_3A:
    case MR_SCN_KV_PERSIST_PARTITION_3A: return 8192u;
    default: return 2048u;
  }
}
#undef MR_TABLE_FN_

/* ---- flags ---- */
#define MR_F_UNRELIABLE 0x1u /* set_unreliable(true) right after RaftTester::new (C2) */
#define MR_F_NULL_RAFT 0x2u  /* skeleton node: never campaigns (as-shipped raft.rs) */
#define MR_F_TRACE 0x4u      /* capture per-event trace for the first trace_clusters */
#define MR_F_SAFETY 0x8u     /* Raft invariant checks at every election (SEMANTICS §11) */
/* Known-buggy Raft variants (SEMANTICS §11), so the checkers can be shown to catch bugs the
 * way the reference tester grades a student's raft.rs */
#define MR_F_BUG_VOTE_TWICE 0x10u /* voters ignore votedFor: two leaders per term possible */
#define MR_F_BUG_VOTE_STALE 0x20u /* voters skip the up-to-date check (Raft §5.4.1) */
#define MR_F_BUG_NO_PREV_CHECK 0x40u /* followers skip AppendEntries' prevLogTerm check (§5.3) */
#define MR_F_RECORD 0x80u    /* record every random decision of each cluster (mr_batch_get_decisions) */
/* Known-buggy kvraft servers (SEMANTICS §9): the linearizability checker must catch them */
#define MR_F_BUG_NO_DEDUP 0x100u   /* servers re-apply a retried Put / Append (no per-clerk dedup) */
#define MR_F_BUG_STALE_READ 0x200u /* a leader answers Get from its local state, not via the log */
#define MR_F_STREAM 0x400u   /* with lanes < n_clusters: a lane whose cluster has its verdict takes
                              * the next unstarted cluster (default: chunks of `lanes` clusters) */
/* Test-only (ABI 4): the tester's apply checker records values but does not compare them
 * (tester.rs:384-388 disabled), so a diverging Raft runs on and the traces' apply digests
 * (mr_trace_digests) are what must catch it */
#define MR_F_BUG_NO_APPLY_CHECK 0x800u

/* ---- verdicts: one code per tester panic site ----
 * X(code, SYMBOL, "message"): enum mr_fail { MR_<SYMBOL> = code }, mr_fail_message(code), the
 * oracle's mro_fail_message and the Python mirror's FAIL_NAMES come from these rows. The comments cite the panic and, where the
 * message shortens it, its format string. */
#define MR_FAIL_TABLE(X) \
  X(0, PASS, "ok") \
  X(1, FAIL_ONE_LEADER_NONE, "expected one leader, got none")               /* tester.rs:91 */ \
  X(2, FAIL_MULTI_LEADER_TERM, "term has (>1) leaders")                     /* tester.rs:83  "term {} has {:?} (>1) leaders" */ \
  X(3, FAIL_TERM_DISAGREE, "servers disagree on term")                      /* tester.rs:105 */ \
  X(4, FAIL_UNEXPECTED_LEADER, "expected no leader, but claims to be leader") /* tester.rs:119 "expected no leader, but {} claims..." */ \
  X(5, FAIL_WAIT_TOO_FEW, "only decided for index; wanted more")            /* tester.rs:198 "only {} decided for index {}; wanted {}" */ \
  X(6, FAIL_ONE_NO_AGREEMENT, "one() failed to reach agreement")            /* tester.rs:255,261 "one({:?}) failed to reach agreement" */ \
  X(7, FAIL_TIMEOUT_120S, "test took longer than 120 seconds")              /* tester.rs:356 */ \
  X(8, FAIL_APPLY_MISMATCH, "commit index mismatch between servers")        /* tester.rs:384-388 "commit index=.. server=.. != .." */ \
  X(9, FAIL_APPLY_OUT_OF_ORDER, "server apply out of order")                /* tester.rs:393 "server {} apply out of order {}" */ \
  X(10, FAIL_COMMIT_MISMATCH, "committed values do not match")              /* tester.rs:411-415 */ \
  X(11, FAIL_UNWRAP_NONE, "called `Option::unwrap()` on a `None` value")    /* tester.rs:76,101,118,144,166 unwrap() on a crashed raft */ \
  X(12, FAIL_LOG_SIZE, "log size too large")                                /* tests.rs:894 */ \
  X(13, FAIL_BASIC_PRECOMMIT, "some have committed before start()")         /* tests.rs:123 */ \
  X(14, FAIL_BASIC_INDEX, "got index but expected another")                 /* tests.rs:126 "got index {} but expected {}" */ \
  X(15, FAIL_LEADER_REJECTED, "leader rejected start")                      /* tests.rs:180,202 (expect) */ \
  X(16, FAIL_EXPECTED_INDEX2, "expected index 2")                           /* tests.rs:183 "expected index 2, got {}" */ \
  X(17, FAIL_NO_MAJORITY_COMMIT, "committed but no majority")               /* tests.rs:189 "{} committed but no majority" */ \
  X(18, FAIL_UNEXPECTED_INDEX, "unexpected index")                          /* tests.rs:204 "unexpected index {}" */ \
  X(19, FAIL_CMD_MISSING, "cmd missing")                                    /* tests.rs:266 "cmd {} missing in {:?}" */ \
  X(20, FAIL_TERM_CHANGED, "term changed too often")                        /* tests.rs:272,468 */ \
  X(21, FAIL_RPC_INITIAL, "too many or few RPCs to elect initial leader")   /* tests.rs:397-401 */ \
  X(22, FAIL_START_FAILED, "start failed")                                  /* tests.rs:434 */ \
  X(23, FAIL_WRONG_VALUE, "wrong value committed")                          /* tests.rs:445-452 "wrong value {:?} committed..." */ \
  X(24, FAIL_RPC_TOO_MANY, "too many RPCs for entries")                     /* tests.rs:462 "too many RPCs ({}) for {} entries" */ \
  X(25, FAIL_RPC_IDLE, "too many RPCs for 1 second of idleness")            /* tests.rs:472-476 */ \
  X(26, FAIL_CHURN_VALUE, "didn't find a value")                            /* tests.rs:852 */ \
  X(27, FAIL_KV_GET_WRONG, "get wrong value")                               /* kvraft/tests.rs:127 "get wrong value, key {:?}" */ \
  X(28, FAIL_KV_MISSING, "missing element in Append result")                /* kvraft/tests.rs:25-30 "missing element {:?} in Append result" */ \
  X(29, FAIL_KV_APPEND_BAD, "duplicate or wrong order element in Append result") /* kvraft/tests.rs:31-39 */ \
  X(30, FAIL_CTRL_NGROUPS, "assertion failed: c.groups.len() == groups.len()")   /* shard_ctrler/tester.rs:117 assert_eq!(c.groups.len(), ..) */ \
  X(31, FAIL_CTRL_MISSING, "missing group")                                 /* shard_ctrler/tester.rs:120 "missing group {}" */ \
  X(32, FAIL_CTRL_INVALID, "shard -> invalid group")                        /* shard_ctrler/tester.rs:125-130 "shard {} -> invalid group {}" */ \
  X(33, FAIL_CTRL_IMBALANCED, "imbalanced sharding")                        /* shard_ctrler/tester.rs:142-148 */ \
  X(34, FAIL_CTRL_SERVERS, "wrong servers for gid")                         /* shard_ctrler/tests.rs:51,53,198-202,210 */ \
  X(35, FAIL_CTRL_HISTORY, "historical query differs")                      /* shard_ctrler/tests.rs:70 historical query != config */ \
  X(36, FAIL_CTRL_MOVE_NUM, "Move should increase Tester.Num")              /* shard_ctrler/tests.rs:91 */ \
  X(37, FAIL_CTRL_MOVE_WRONG, "shard wrong group")                          /* shard_ctrler/tests.rs:97 "shard {} wrong group" */ \
  X(38, FAIL_CTRL_MINIMAL_JOIN, "non-minimal transfer after Join()s")       /* shard_ctrler/tests.rs:135,251 */ \
  X(39, FAIL_CTRL_MINIMAL_LEAVE, "non-minimal transfer after Leave()s")     /* shard_ctrler/tests.rs:154,269 */ \
  X(40, FAIL_CTRL_NO_LEADER, "Leader not found")                            /* shard_ctrler/tests.rs:282,289 */ \
  X(41, FAIL_CTRL_SAME_CONFIG, "config differs after leader shutdown")      /* shard_ctrler/tests.rs:294 assert_eq!(c, c1) */ \
  /* Raft invariants (MR_F_SAFETY; Raft paper Fig. 3), not reference panic sites */ \
  X(42, FAIL_SAFETY_ELECTION, "election safety: two leaders in one term") \
  X(43, FAIL_SAFETY_COMPLETENESS, "leader completeness: new leader lacks a committed entry") /* committed = applied */ \
  X(44, FAIL_KV_LOG_SIZE, "logs were not trimmed")                          /* kvraft/tests.rs:208-215, :422-428, :475-481 */ \
  X(45, FAIL_KV_SNAPSHOT_SIZE, "snapshot too large")                        /* kvraft/tests.rs:483-489 */ \
  X(46, FAIL_KV_MINORITY_PROGRESS, "put/get in minority completed")         /* kvraft/tests.rs:315-319 */ \
  X(47, FAIL_KV_NO_COMPLETION, "put/get did not complete")                  /* kvraft/tests.rs:333-337 */ \
  X(48, FAIL_KV_CHECK, "get(key) check failed")                             /* kvraft/tester.rs:266-271 Clerk::check */ \
  X(49, FAIL_SAFETY_LOG_MATCHING, "log matching: same index and term, different entries") /* MR_F_SAFETY */ \
  /* the as-shipped service skeleton (MR_F_NULL_RAFT on kvraft / shard_ctrler tests) */ \
  X(50, FAIL_TODO_APPLY, "not yet implemented: apply command")              /* kvraft/server.rs:69 */ \
  X(51, FAIL_TODO_RPC_RESULTS, "not yet implemented: handle RPC results")   /* kvraft/client.rs:59 */ \
  /* the build's linearizability checker (SEMANTICS §9a; the reference's are commented out, \
   * kvraft/tests.rs:386-390,524-528): a Get's result fits no linearization of the key's history */ \
  X(52, FAIL_KV_NOT_LINEARIZABLE, "history is not linearizable") \
  /* simulator limits (not reference panics): a cluster that hits one is reported, never passed */ \
  X(60, FAIL_SIM_CAPACITY, "simulator capacity exceeded")       /* a log / apply / sequence capacity of the config */ \
  X(61, FAIL_SIM_EVENT_LIMIT, "simulator event limit exceeded") /* cfg.max_events processed without a verdict */ \
  X(62, FAIL_SIM_BAD_PROGRAM, "scenario program error")         /* interpreter budget, bad op */ \
  X(0xFFFF, RUNNING, "running")                                 /* verdict not reached yet */

enum mr_fail {
#define MR_ROW_(code, sym, msg) MR_##sym = code,
  MR_FAIL_TABLE(MR_ROW_)
#undef MR_ROW_
};

typedef struct mr_cfg {
  uint32_t abi_version;   /* = MR_ABI_VERSION */
  uint32_t scenario;      /* enum mr_scenario */
  uint32_t n_nodes;       /* servers, 3..8 (reference default per test if 0) */
  uint32_t flags;         /* MR_F_* */
  uint64_t seed_base;     /* cluster c runs seed  seed_base + cluster_base + c */
  uint64_t cluster_base;  /* global id of this batch's first cluster (multi-GPU shard) */
  uint64_t n_clusters;    /* clusters in this batch */
  uint32_t iters;         /* scenario loop count override (0 = the reference's) */
  uint32_t log_cap;       /* Raft log ring capacity per node, power of two */
  uint32_t apply_cap;     /* apply-checker index capacity per cluster */
  uint32_t msg_slots;     /* max in-flight messages per cluster (<= 64; <= 256 for
                           * snapshot_recover_many_clients_3b); more in flight = MR_FAIL_SIM_CAPACITY */
  uint32_t ae_max;        /* max entries per AppendEntries (<= 32) */
  uint32_t hb_us;         /* leader heartbeat period */
  uint32_t elect_lo_us;   /* election timeout U[lo, hi) (raft.rs:262: 150..300 ms) */
  uint32_t elect_hi_us;
  uint32_t max_events;    /* per-cluster event cap -> MR_FAIL_SIM_EVENT_LIMIT */
  uint32_t trace_clusters;/* with MR_F_TRACE: the first K clusters keep a trace */
  uint32_t trace_cap;     /* trace records per traced cluster */
  int32_t device;         /* HIP device ordinal */
  uint32_t tape_cap;      /* with MR_F_RECORD: decisions kept per cluster */
  uint32_t lanes;         /* clusters in flight per launch (0 = what the GPU keeps resident:
                           * waves / SIMD x SIMDs x 64). A bigger batch runs as consecutive
                           * chunks of `lanes` clusters (or streams them, MR_F_STREAM) instead of
                           * queueing waves behind the resident ones. Results do not depend on it. */
  uint32_t lanes_per_wave;/* lanes of each 64-lane wave that hold a cluster: 64, 32 or 16 (0 = auto:
                           * 32 when the batch fills at most half the resident lanes, so a small
                           * batch still runs two waves per SIMD; else 64). Results do not depend
                           * on it. */
  uint32_t reserved[3];
} mr_cfg;

/* The reference's defaults for scenario `scn` (mr_cfg_init and the oracle's mro_cfg_init are this);
 * -1 and cfg untouched for an id without a row. */
static inline int mr_cfg_defaults(mr_cfg* c, uint32_t scn) {
  if (mr_scn_servers(scn) == 0) return -1;
  memset(c, 0, sizeof *c);
  c->abi_version = MR_ABI_VERSION;
  c->scenario = scn;
  c->n_nodes = mr_scn_servers(scn); /* tests.rs `let servers = ..` */
  c->seed_base = 1629626496ull;     /* README.md:48 */
  c->n_clusters = 1;
  /* capacities sized from the oracle's maxima over 2000 seeds */
  uint32_t cap = mr_scn_is_fig8(scn) ? 2048 : mr_scn_is_kv(scn) ? mr_kv_log_cap(scn)
               : mr_scn_is_churn(scn) ? 4096 : scn == MR_SCN_UNRELIABLE_AGREE_2C ? 1024 : 0;
  c->log_cap = cap ? cap : 256;
  c->apply_cap = cap ? cap : (mr_scn_is_snap2d(scn) ? 1024 : 512);
  /* in-flight maxima over 64K / 1K seeds: 20 (figure_8), <= 45 (7 / 8 servers,
   * kvraft), 229 (20 clerks); a send past msg_slots fails the cluster (MR_FAIL_SIM_CAPACITY) */
  c->msg_slots = mr_scn_msg_slots(scn);
  c->ae_max = 16;
  c->hb_us = 50000;
  c->elect_lo_us = 150000; /* raft.rs:262 */
  c->elect_hi_us = 300000;
  c->max_events = 4u << 20;
  c->trace_cap = 1u << 16;
  return 0;
}
/* The capacity limits the kernels and the oracle share: what is wrong with cfg, or NULL. */
static inline const char* mr_cfg_check_caps(const mr_cfg* c) {
  if (c->n_nodes < 3 || c->n_nodes > MR_MAX_NODES) return "n_nodes must be 3..8";
  if (c->log_cap < 16 || (c->log_cap & (c->log_cap - 1))) return "log_cap: power of 2 >= 16";
  if (c->apply_cap < 16) return "apply_cap too small";
  if (c->msg_slots < 1 || c->msg_slots > MR_MAX_MSG_SLOTS ||
      (c->msg_slots > 64 && !mr_scn_wide_slots(c->scenario)))
    return "msg_slots must be 1..64 (1..256 for snapshot_recover_many_clients_3b)";
  if (c->ae_max < 1 || c->ae_max > MR_MAX_AE) return "ae_max must be 1..32";
  return NULL;
}

/* Whole-batch counters (sums over clusters unless named max/first). */
typedef struct mr_counters {
  uint64_t clusters, done, passed, failed;
  uint64_t events, ev_msg, ev_timer, ev_tester;
  uint64_t msgs_sent;      /* every send: madsim stat().msg_count (tester.rs:147-149) */
  uint64_t drop_clog;      /* endpoint disconnected at send */
  uint64_t drop_loss;      /* Bernoulli(packet_loss_rate) */
  uint64_t drop_overflow;  /* a send found msg_slots in flight: the cluster fails MR_FAIL_SIM_CAPACITY */
  uint64_t drop_deliver;   /* endpoint disconnected / crashed at delivery */
  uint64_t drop_stale;     /* RPC reply to a killed incarnation */
  uint64_t elections, leaders_elected, applies, snapshots, installs;
  uint64_t entries_shipped;/* AppendEntries entries read by their receiver (counted at delivery,
                            * past the prevLogIndex/prevLogTerm check; clogged, lost and rejected
                            * appends carry none: payloads are zero-copy until delivery) */
  uint64_t virt_time_us;   /* sum of per-cluster virtual end time */
  uint64_t max_inflight, max_log, max_index;
  uint64_t first_fail_cluster; /* global cluster id (UINT64_MAX if none) */
  uint64_t first_fail_code;
  uint64_t fail_hist[64];  /* verdict histogram by code (index 63 = >= 63) */
  /* coverage histograms over clusters, bucket b = 0 for 0, else min(15, 1 + floor(log2 v)) */
  uint64_t cov_leaders[16]; /* leaders elected per cluster */
  uint64_t cov_events[16];  /* events per cluster */
  /* services (kvraft / shard_ctrler; BASELINE config 5 "linearizability-check counters") */
  uint64_t kv_ops;          /* clerk calls completed */
  uint64_t kv_checked;      /* Get results the tester verified against their linearizable value */
  /* ABI 3 */
  uint64_t log_writes;      /* log entries written (leader start() appends + follower appends) */
  uint64_t entries_materialized; /* zero-copy payload entries copied before their log slot was
                                  * overwritten (HIP path only; the oracle copies at send) */
  uint64_t kv_lin_checked;  /* Get results the linearizability checker verified (SEMANTICS §9a) */
  /* ABI 4 */
  uint64_t coop_entries;    /* HIP path only: AppendEntries entries a receiver's wave wrote for it
                             * (the cooperative receive of the 7- / 8-server step kernels) */
} mr_counters;

/* ---- per-cluster counters: what the kernels keep per cluster (mr_dev.h x.cnt[]) ----
 *   X(SYMBOL, field, reduction, who)
 * CNT_<SYMBOL> indexes the cluster's counter, mr_counters.<field> is its reduction over the batch
 * (SUM, or MAX: the MAX rows come last), and `who` says whether the oracle keeps it too (BOTH:
 * mro_result.<field>) or only the HIP path does (HIP). The CNT_ enum, the reduce kernel's rule,
 * mr_batch_counters, the oracle's sums and the Python key lists (dist.py, the tests) come from these
 * rows; the struct above stays written out, because its field order is ABI. */
#define MR_COUNTER_TABLE(X) \
  X(EV_MSG, ev_msg, SUM, BOTH) \
  X(EV_TIMER, ev_timer, SUM, BOTH) \
  X(EV_TESTER, ev_tester, SUM, BOTH) \
  X(DROP_CLOG, drop_clog, SUM, BOTH) \
  X(DROP_LOSS, drop_loss, SUM, BOTH) \
  X(DROP_OVERFLOW, drop_overflow, SUM, BOTH) \
  X(DROP_DELIVER, drop_deliver, SUM, BOTH) \
  X(DROP_STALE, drop_stale, SUM, BOTH) \
  X(ELECTIONS, elections, SUM, BOTH) \
  X(LEADERS, leaders_elected, SUM, BOTH) \
  X(APPLIES, applies, SUM, BOTH) \
  X(SNAPSHOTS, snapshots, SUM, BOTH) \
  X(INSTALLS, installs, SUM, BOTH) \
  X(SHIPPED, entries_shipped, SUM, BOTH) \
  X(LOG_WRITES, log_writes, SUM, BOTH) \
  X(MATERIALIZED, entries_materialized, SUM, HIP) \
  X(COOP, coop_entries, SUM, HIP) \
  X(MAX_INFLIGHT, max_inflight, MAX, BOTH) \
  X(MAX_LOG, max_log, MAX, BOTH) \
  X(MAX_INDEX, max_index, MAX, BOTH)

typedef struct mr_run_stats {
  uint64_t launches;       /* step-kernel launches */
  double kernel_ms;        /* summed step-kernel time (HIP events, batch stream) */
  double wall_ms;          /* host wall time of mr_batch_run */
  uint64_t events;         /* events processed in this call */
  uint64_t remaining;      /* clusters without verdict after the call */
} mr_run_stats;

/* One trace record per processed event (32 B); docs/SEMANTICS.md §Trace. */
typedef struct mr_event {
  uint32_t time_us;
  uint8_t cls;     /* 0 message, 1 node timer, 2 tester, 3 verdict */
  uint8_t kind;    /* message type / drop reason / fail code */
  uint8_t node;    /* destination or timer node (0xFF for tester) */
  uint8_t role;    /* node role after the event (0 F, 1 C, 2 L, 3 down) */
  uint32_t aux;    /* message seq / msgs_sent for tester events */
  uint32_t term, commit, applied, last, snap;
} mr_event;

typedef struct mr_batch mr_batch;

const char* mr_last_error(void);
const char* mr_fail_message(uint32_t code);
const char* mr_scenario_name(uint32_t scenario);
/* Name as in tests.rs (e.g. "figure_8_unreliable_2c") -> id; 0 if unknown. */
uint32_t mr_scenario_from_name(const char* name);
/* Fill cfg with the reference's defaults for `scenario`. */
int mr_cfg_init(mr_cfg* cfg, uint32_t scenario);

int mr_batch_create(const mr_cfg* cfg, mr_batch** out);
/* Re-seed and reset every cluster to RaftTester::new state (device-side). */
int mr_batch_reset(mr_batch* b, uint64_t seed_base);
/* Run until every cluster has a verdict or max_events_per_call events per
 * cluster were processed in this call (0 = no per-call bound). */
int mr_batch_run(mr_batch* b, uint64_t max_events_per_call, mr_run_stats* st);
/* Pipelined steps (the benchmark's double-buffered batches): mr_batch_submit enqueues
 * mr_batch_reset(seed_base) and the first step-kernel launch on the batch's own stream and
 * returns at once; mr_batch_finish waits for them, runs any clusters left past the per-launch
 * budget to their verdict, and returns the run stats and (cnt != NULL) the counters.
 * A second batch's step submitted meanwhile fills the CUs this batch's finished waves free.
 * Results are those of mr_batch_reset + mr_batch_run. */
int mr_batch_submit(mr_batch* b, uint64_t seed_base);
int mr_batch_finish(mr_batch* b, mr_run_stats* st, mr_counters* cnt);
/* Per-cluster verdict code, fail/end time (virtual us) and trace digest. */
int mr_batch_verdicts(mr_batch* b, uint16_t* code, uint32_t* time_us, uint64_t* digest);
int mr_batch_counters(mr_batch* b, mr_counters* out);
/* Trace of traced cluster `k` (k < trace_clusters). *n = records written. */
int mr_trace_get(mr_batch* b, uint32_t k, mr_event* out, size_t cap, size_t* n);
/* ABI 4: the apply-digest term of log entry i with command value v (splitmix64's finalizer of
 * v ^ i * golden ratio); the kernels compute the same in device code */
static inline uint64_t mr_apply_mix(uint32_t i, uint64_t v) {
  uint64_t z = v ^ ((uint64_t)i * 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
/* ABI 4: the apply digest of each of those records (docs/SEMANTICS.md §7): for a node event,
 * the sum mod 2^64 of mr_apply_mix(i, value_i) over the entries i = 1..applied the node applied
 * one by one; UINT64_MAX once it installed a snapshot or restarted above index 0; 0 for other
 * records. Equal applied indices with different digests = state-machine safety broken by
 * value, checkable from the trace alone (tests/test_trace_properties.py). */
int mr_trace_digests(mr_batch* b, uint32_t k, uint64_t* out, size_t cap, size_t* n);
/* ABI 4: the key-value commands of traced cluster k as the service applied them (kvraft
 * scenarios; zero rows elsewhere): out[2 i] = log entry i's command (SEMANTICS §9 layout), out[2 i
 * + 1] = the hash of its key's value right after the first server to apply entry i applied it
 * (a Get: the hash it answers). Rows i < min(cap, trace_cap); *n = 1 + the highest index
 * recorded. The log by value and the servers' state machine, checkable against a replay of
 * the real strings (tests/test_kv_trace.py). */
int mr_trace_applies(mr_batch* b, uint32_t k, uint64_t* out, size_t cap, size_t* n);
/* ABI 4: the kernel the batch's launches run: "pool_kernel", "step_kernel" or
 * "step_kernel_tape" (keyed decisions, variants or a seed list set, or decisions recorded) */
const char* mr_batch_kernel(const mr_batch* b);
void mr_batch_destroy(mr_batch* b);

/* ---- keyed decision traces and replay (docs/SEMANTICS.md §12) ----
 * Every random choice of a cluster is one decision, keyed by WHO makes it, not by when:
 *   stream MR_DS_NET    entity = sending host (server i, clerk 8 + k), seq = that host's
 *                       send index -> w0 < loss_q32 drops the message, w1 picks its latency
 *                       (madsim net send: drop + latency, tester.rs:127-137);
 *   stream MR_DS_ELECT  entity = server, seq = its timeout index -> w0 picks the election
 *                       timeout (raft.rs:260-263, U[150, 300) ms);
 *   stream MR_DS_TESTER entity = tester thread (0 = the test body), seq = its draw index ->
 *                       (w0, w1) is the rand::rng() value (tests.rs gen_range / gen_bool /
 *                       gen_entry as SEMANTICS §2 maps it).
 * A range choice v in [lo, hi) is the word mr_decision_word(v, lo, hi). A trace is a set:
 * any order, any subset; a draw whose key is absent takes the seed's own Philox draw and
 * counts as a miss. A recorder of another simulator's run (a MadSim seed) emits these
 * records and mr_replay plays them. */
enum mr_decision_stream { MR_DS_TESTER = 1, MR_DS_ELECT = 2, MR_DS_NET = 3 };
typedef struct mr_decision {
  uint32_t cluster; /* batch-relative cluster (mr_replay: ignored) */
  uint16_t stream;  /* enum mr_decision_stream */
  uint16_t entity;
  uint32_t seq;
  uint32_t w0, w1;
} mr_decision;
/* The smallest draw word w with lo + floor(w * (hi - lo) / 2^32) == v (lo <= v < hi). */
uint32_t mr_decision_word(uint32_t v, uint32_t lo, uint32_t hi);
/* Drive the batch's clusters by `d` (n records, any order; duplicate keys are an error);
 * n = 0 = Philox again. Call after create / reset and before run. */
int mr_batch_set_decisions(mr_batch* b, const mr_decision* d, size_t n);
/* Cluster k: with MR_F_RECORD its decisions so far in draw order (*n = decisions drawn, up to
 * cap copied); with decisions set, *n = its draws that found no record (misses). */
int mr_batch_get_decisions(mr_batch* b, uint32_t k, mr_decision* out, size_t cap, size_t* n);
/* ABI 5: every cluster of the batch is a variant of cluster 0's seed (seed_base + cluster_base):
 * base decisions (d.cluster ignored), edits (key must be in base; w0, w1 replace the record's),
 * masks[c * W + j / 32] bit j % 32 = cluster c applies edit j, W = (n_edits + 31) / 32
 * (masks == NULL: no cluster applies any). n == 0 drops the variants (Philox again); tables of
 * another kind (mr_batch_set_decisions) are not a variant's to drop and stay as they are.
 * A draw whose key is not in base takes that seed's Philox draw, whatever the cluster, and counts
 * as a miss (mr_batch_get_decisions(b, k, NULL, 0, &n)). Errors, which leave the batch's tables
 * as they were: a duplicate key in base or in edits, an edit key absent from base, a bad stream,
 * a MR_F_RECORD batch. The tables survive mr_batch_reset (docs/SEMANTICS.md §12.1). */
int mr_batch_set_variants(mr_batch* b, const mr_decision* base, size_t n,
                          const mr_decision* edits, size_t n_edits, const uint32_t* masks);
/* New masks for the same base and edits (of either kind of variant batch, with the batch's W):
 * the only upload of a shrinking round. An error without variants set. */
int mr_batch_set_variant_masks(mr_batch* b, const uint32_t* masks);
/* ABI 6: a variant batch of groups (docs/SEMANTICS.md §12.2). Each group is one seed with its own
 * base tape and edits; cluster c is a variant of group group_of[c]'s seed. */
typedef struct mr_variant_group {
  uint32_t seed_cluster;      /* the group's runs are runs of the seed seed_base + cluster_base + seed_cluster
                               * (batch-relative; need not be < n_clusters); its misses draw from that seed */
  uint32_t base_off, n_base;  /* its base tape: base[base_off .. base_off + n_base), n_base >= 1 */
  uint32_t edit_off, n_edits; /* its edits: edits[edit_off .. +n_edits); keys must be in ITS base tape */
} mr_variant_group;
/* masks[c * W + j / 32] bit j % 32 = cluster c applies edit j of its group (j counts within the
 * group's edits), W = (max over groups of n_edits + 31) / 32; masks == NULL: no cluster applies
 * any. n_groups == 0 drops variants of either kind, as mr_batch_set_variants(.., n = 0, ..) does;
 * tables of mr_batch_set_decisions stay. mr_batch_set_variants is the one-group case: group
 * {0, 0, n, 0, n_edits}, group_of all 0. Misses: mr_batch_get_decisions(b, k, NULL, 0, &n).
 * Errors, validated before anything is freed, so the batch's tables stay as they were: a duplicate
 * key inside one group's base or edits, an edit key absent from its own group's base (another
 * group's does not count), a bad stream, a range that overruns n or n_edits, n_base == 0, a
 * group_of[c] >= n_groups, a MR_F_RECORD batch, more than 2^32 - 1 records. The tables survive
 * mr_batch_reset. */
int mr_batch_set_variant_groups(mr_batch* b, const mr_variant_group* groups, size_t n_groups,
                                const mr_decision* base, size_t n, const mr_decision* edits,
                                size_t n_edits, const uint32_t* group_of /* [n_clusters] */,
                                const uint32_t* masks);
/* ---- seed lists (ABI 7, docs/SEMANTICS.md §12.3) ----
 * Cluster c runs the seed seed_base + cluster_base + seed_cluster[c] (any order, duplicates
 * allowed, values need not be < n_clusters). NULL = cluster c runs seed c again. Call after create /
 * reset and before run. The list is the batch's, not its decision tables': it survives
 * mr_batch_reset (the same offsets from the new base), mr_batch_submit and mr_batch_set_decisions
 * (n = 0 too); only NULL here or mr_batch_destroy drops it. While it is set the batch runs
 * "step_kernel_tape". With MR_F_RECORD the tape of position c is that seed's; with decisions set,
 * d.cluster is the position and a miss draws from the position's seed. Verdicts, counters,
 * first_fail_cluster, traces and d.cluster speak of positions, whatever seed runs there. Errors,
 * which leave the batch as it was: a list on a batch with variants set (and mr_batch_set_variants /
 * mr_batch_set_variant_groups on a batch with a list), a submitted step not yet finished. */
int mr_batch_set_seeds(mr_batch* b, const uint32_t* seed_cluster /* [n_clusters] or NULL */);
/* ABI 7: the recorded tapes of clusters [first, first + count) in one call. drawn[i] (optional) =
 * decisions cluster first + i drew; off[count + 1] = CSR offsets into out of the records kept,
 * min(drawn, tape_cap) each, in draw order, cluster = batch position. out == NULL: only drawn and
 * off are filled (size the buffer, call again). With decisions set instead of MR_F_RECORD: drawn =
 * misses, off all 0. An error if out != NULL and cap < off[count]. */
int mr_batch_get_decisions_packed(mr_batch* b, uint32_t first, uint32_t count, uint64_t* drawn,
                                  uint64_t* off, mr_decision* out, size_t cap);
/* ---- parameter groups (an addition within ABI 7, docs/SEMANTICS.md §12.4) ----
 * One batch sweeps the settings of the system under test: position c is in group group_of[c], and
 * runs exactly what a batch created from cfg_g runs at that position's seed, where cfg_g is the
 * batch's cfg with the group's non-zero numeric fields and with the sweepable flag bits
 * (MR_F_SWEEPABLE) taken from the group's flags: they REPLACE cfg.flags' sweepable bits, so an
 * all-zero group inherits the numbers and clears those bits. MR_F_SAFETY, MR_F_TRACE, MR_F_RECORD,
 * MR_F_STREAM, n_nodes, every capacity and max_events stay the batch's: they size arrays or select
 * kernels. The groups are the batch's, as a seed list is: they survive mr_batch_reset,
 * mr_batch_submit and every set_decisions / set_variants* / set_seeds call; only n_groups == 0 here
 * or mr_batch_destroy drops them. Call after create / reset and before run. While they are set the
 * batch runs "step_kernel_tape"; they compose with every decision source (a seed list gives the
 * paired design: the same seeds in every group; MR_F_RECORD records position c's tape under its
 * group; replay and variants look draws up as before). Errors, each of which leaves the batch as it
 * was: a group_of[c] >= n_groups, a flag bit outside MR_F_SWEEPABLE, non-zero reserved,
 * elect_hi_us <= elect_lo_us after inheritance, ae_max > cfg.ae_max, a submitted step not yet
 * finished. */
#define MR_F_SWEEPABLE                                                                             \
  (MR_F_UNRELIABLE | MR_F_NULL_RAFT | MR_F_BUG_VOTE_TWICE | MR_F_BUG_VOTE_STALE |                  \
   MR_F_BUG_NO_PREV_CHECK | MR_F_BUG_NO_DEDUP | MR_F_BUG_STALE_READ | MR_F_BUG_NO_APPLY_CHECK)
typedef struct mr_param_group {
  uint32_t flags;        /* the group's MR_F_SWEEPABLE bits: they replace cfg.flags' */
  uint32_t hb_us;        /* 0 = cfg's, likewise below */
  uint32_t elect_lo_us, elect_hi_us;
  uint32_t ae_max;       /* <= cfg.ae_max: payloads are sized and strided by the batch's */
  uint32_t iters;
  uint32_t reserved[2];  /* 0 */
} mr_param_group;        /* 32 B */
int mr_batch_set_param_groups(mr_batch* b, const mr_param_group* g, size_t n_groups,
                              const uint32_t* group_of /* [n_clusters] */);
/* mr_batch_counters restricted to the positions of one group, as of the batch's last run (one
 * grouped reduce pass fills every group's row; this call copies one): sums, maxima, fail_hist, both
 * coverage histograms, the service counters, clusters = the group's positions, and
 * first_fail_cluster = its first failing position + cluster_base (UINT64_MAX: none). An error if
 * `group` is out of range or no groups are set. */
int mr_batch_group_counters(mr_batch* b, uint32_t group, mr_counters* out);
/* ---- fork (an addition within ABI 7, docs/SEMANTICS.md §12.5) ----
 * Position c of dst becomes a copy of position src_of[c] of src as that cluster stands now; src may
 * be dst. src_of[c] == UINT32_MAX leaves c as it is (and so does src_of[c] == c when src == dst).
 * Every later draw of c follows c's own rule in dst: its seed seed_base + cluster_base + c, or its
 * seed-list entry, its lookup slice or its parameter group. The whole run of c then equals the run
 * of c's seed with the decisions the source had drawn (what MR_F_RECORD records of it) set as keyed
 * decisions: verdict, time, digest, trace and per-cluster counters. The batches may differ in
 * n_clusters, trace_clusters, trace_cap, tape_cap, seeds, timers, iters and lanes. The call blocks;
 * afterwards dst's launch loop starts over (positions with a verdict are skipped at one load each).
 * When both batches record, the source's tape comes along, so a forked position's tape is its whole
 * history; otherwise the position's count of draws (mr_batch_get_decisions' n) restarts at 0.
 * Counters: events, msgs_sent, virt_time_us, done / passed / failed, fail_hist, first_fail_*, both
 * coverage histograms and the kv_* counters are kept per cluster, are copied, and speak of each
 * position's whole history. So do the rows of MR_COUNTER_TABLE when the prefix ran on "step_kernel"
 * or "step_kernel_tape". "pool_kernel" sums those rows per workgroup into the batch that ran them:
 * a prefix run there stays counted once, in the source's batch, and the destination adds the
 * futures to whatever its own earlier launches since its reset summed (nothing, for a destination
 * not launched before the fork); leaders_elected and max_index travel with the cluster there too.
 * Errors, all found before anything is written, so both batches stay as they were: a null
 * argument; a submitted step not yet finished on either batch; different device, scenario, n_nodes,
 * log_cap, apply_cap, msg_slots, ae_max, MR_F_SAFETY or the MR_KEY_ROWS they were created under;
 * src_of[c] >= src's n_clusters; src == dst
 * and a source that is itself overwritten; src's launches since its reset wrote the message keys
 * in one format ("pool_kernel"'s, or the one "step_kernel" and "step_kernel_tape" share) and dst's
 * kernel reads the other ("source ran on ..., destination continues on ..."; a source not launched
 * since its reset is always accepted); a traced position of dst (c < trace_clusters) whose source is
 * not traced, holds more records than dst's trace_cap, or has drawn more than its own trace_cap
 * when the two caps differ (it dropped records dst would hold); a recording dst with a src that does not
 * record. */
int mr_batch_fork(mr_batch* dst, mr_batch* src, const uint32_t* src_of /* [dst n_clusters] */);
/* A measurement aid: the device time of fork_kernel in b's last mr_batch_fork as destination.
 * Meaningful only directly after that fork: an error once b has been reset or launched since, or if
 * it was never forked into (or the fork copied nothing). */
int mr_batch_fork_ms(mr_batch* b, float* ms);
/* One cluster of cfg (cluster_base selects the seed for misses) driven by the n decisions:
 * its per-event trace (per-node term / role / commit / applied / last / snapshot after every
 * event), its verdict and verdict time, and (misses != NULL) its draws not in `d`. */
int mr_replay(const mr_cfg* cfg, const mr_decision* d, size_t n, mr_event* out, size_t cap,
              size_t* n_out, uint16_t* code, uint32_t* time_us, uint64_t* misses);

#ifdef __cplusplus
}
#endif
#endif /* MADRAFT_SIM_H */
