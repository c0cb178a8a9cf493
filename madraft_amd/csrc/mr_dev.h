// mr_dev.h — device state layout shared by the HIP kernels (mr_kernel.hip)
// and the C++ batch driver (mr_host.cpp).
//
// Layout: one lane simulates one cluster. Two kinds of arrays:
//  * cluster-minor matrices [field][...][C] for what every lane of a wave
//    touches at the same field index (cluster scalars, tester frame, message
//    keys in the launch prologue / epilogue): 64 lanes read 64 consecutive
//    words;
//  * cluster-major records for what a lane touches at a per-lane index — a
//    node (the event's destination differs per lane), a message slot, log
//    entries, apply-checker indices: one node's whole state is one 128-B
//    record (scalars + next[] + match[]), one message one 32-B record, so an
//    event touches one or two lines per object instead of one line per field
//    (a [field][node][C] layout costs a line per field per lane once the
//    lanes' node indices differ).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/madraft_sim.h"

namespace mr {

// ---- node flag word (one u32 per node): role[0:2) voted[4:8) (15 = none)
//      inc[8:16) votes[16:24); started / connected are cluster bit masks (CS_ALIVE, CS_CONN)
enum : uint32_t { R_F = 0, R_C = 1, R_L = 2, R_DOWN = 3 };
enum : uint32_t { M_RV_REQ = 1, M_RV_REP, M_AE_REQ, M_AE_REP, M_IS_REQ, M_IS_REP, M_KV_REQ, M_KV_REP };
enum : uint32_t { ST_TESTER = 1, ST_ELECT = 2, ST_NET = 3 };

// per-cluster u32 counters (part of cs32): the rows of madraft_sim.h's MR_COUNTER_TABLE
enum : uint32_t {
#define MR_ROW_(sym, field, red, who) CNT_##sym,
  MR_COUNTER_TABLE(MR_ROW_)
#undef MR_ROW_
  CNT__N
};
// counter k reduces over clusters as a maximum, not a sum: the table's MAX rows, its tail
enum : uint32_t { CNT_RED_SUM, CNT_RED_MAX };
constexpr bool cnt_is_max(uint32_t k) { return k >= CNT_MAX_INFLIGHT; }
#define MR_ROW_(sym, field, red, who) \
  static_assert(cnt_is_max(CNT_##sym) == (CNT_RED_##red == CNT_RED_MAX), #sym ": MAX rows come last");
MR_COUNTER_TABLE(MR_ROW_)
#undef MR_ROW_
// reduce_kernel's output vector: the CNT__N counters, then these (two unused slots after
// RED_FIRST_FAIL; the histograms take 64, 16 and 16 slots)
enum : uint32_t {
  RED_EVENTS = CNT__N, RED_MSGS, RED_VTIME, RED_DONE, RED_PASSED, RED_FIRST_FAIL,
  RED_FAIL_HIST = RED_FIRST_FAIL + 3, RED_COV_LEADERS = RED_FAIL_HIST + 64,
  RED_COV_EVENTS = RED_COV_LEADERS + 16, RED_KV_OPS = RED_COV_EVENTS + 16, RED_KV_CHECKED,
  RED_KV_LIN, RED_N
};

// tester coroutine frame (per cluster): program counter, script locals,
// helper frame of the multi-event tester calls (one / wait / check_one_leader)
constexpr uint32_t T_NL = 8;   // u32 script locals
constexpr uint32_t T_NH = 5;   // u32 helper frame
constexpr uint32_t T_NV = 16;  // u64 script arrays (count_2b / concurrent_starts)

// cs32 [CS__N][C]: per-cluster u32 scalars
enum : uint32_t {
  CS_CODE, CS_VTIME, CS_NOW, CS_EVENTS, CS_MSGS, CS_INFLIGHT, CS_NETMODE, CS_TCTR, CS_TRACEN,
  CS_MSLOT, CS_CONN, CS_ALIVE, CS_TWAKE, CS_CNT,  // (the tester frame is the tfr record)
  CS_KVDONE = CS_CNT + CNT__N, CS_MJOIN, CS_CWAKE, CS_CTID, CS_CSLOT,  // tester threads (SEMANTICS §8-9)
  CS_NLIVE,  // live spawned threads
  CS_NOPS,   // shard_ctrler: clerk operations so far
  CS_CUT,    // server links cut (disconnect2): bit 8 (i mod 4) + j of word CS_CUT + i / 4
  CS_CUT_END = CS_CUT + 2,
  CS_CCUT,   // clerk links cut: bit 8 (k mod 4) + j of word CS_CCUT + k / 4 = clerk host 8 + k !~ server j
  CS_CCUT_END = CS_CCUT + 6,
  CS_TAPE,   // keyed decisions: recorded so far (record) / draws without a record (replay)
  CS_KV_OPS, CS_KV_CHECKED,  // service clerk calls completed / Get results verified
  CS_KV_LIN,                 // Get results the linearizability checker verified
  CS_LMASK,                  // servers whose record holds role leader (x.lmask, store_node)
  CS_LRS,                    // per node: run start of its last log entry (mr_kernel.hip le_at)
  CS_LRS_END = CS_LRS + 8,
  CS__N
};
// cs64 [C64__N][C]: per-cluster u64 scalars
// C64_FREE1..3: free-slot mask words 1..3 (slots 64..255, MR_MW = 4 units)
enum : uint32_t { C64_FREE, C64_DIGEST, C64_MMIN, C64_TV, C64_FREE1 = C64_TV + T_NV,
                  C64__N = C64_FREE1 + 3 };
// Cluster scalars: cluster-minor matrices [field][C] (a wave's lanes read 64 consecutive words
// of one field; cluster-major records measured -5 % in round 4). The strides pad the field
// counts; the host reads rows through these index macros.
constexpr uint32_t CS_STRIDE = (CS__N + 3u) & ~3u, C64_STRIDE = (C64__N + 1u) & ~1u;
#define CS_IDX(f, c, C) ((size_t)(f) * (C) + (c))
#define C64_IDX(f, c, C) ((size_t)(f) * (C) + (c))
// nd32 [C][n][NREC]: one 128-B record per node. Words 0..11 are the scalars
// an event loads / stores as a block (load_node), 12..13 the pending payload
// range, 14..15 the snapshot value (u64), 16..23 next[p], 24..31 match[p]
// (leader -> peer p). match[me] holds the leader's base: its last index when it
// won its term (every entry above it, and none at or below, has the current
// term), or LBASE_NONE once it has taken entries or a snapshot from another leader of
// its term (two leaders in a term: MR_F_BUG_VOTE_TWICE), after which no index tells an
// entry's term. LASTT caches term_at(last). Node timers live in tmr [n][C].
enum : uint32_t {
  NF_FLAGS, NF_TERM, NF_COMMIT, NF_APPLIED, NF_LAST, NF_SNAP, NF_SNAPT, NF_ECTR, NF_NCTR,
  NF_PEXP, NF_SLEN, NF_LASTT, NF_PLO, NF_PHI, NF_SNAPV, NF__N = 16
};
enum : uint32_t { PF_NEXT, PF_MATCH, PF__N };
constexpr uint32_t LBASE_NONE = ~0u;
constexpr uint32_t NR_PEER = 16;  // next[] at 16, match[] at 16 + MR_MAX_NODES
constexpr uint32_t NREC = 32;
// ms32 [C][M][MREC]: one 32-B record per in-flight message (value at 6..7);
// mkey [M][C]: message keys (time, seq, dst), cluster-minor
enum : uint32_t { MF_HDR, MF_TERM, MF_A, MF_B, MF_C, MF_PAD, MF_V, MREC = 8 };

// one Raft log entry (raft.rs Log: term + command), 16 B so an entry moves as
// one 128-bit access; message payloads (AppendEntries entries) use the same form
struct alignas(16) LE {
  uint32_t term, rs;  // rs: first index of the run of entries of this term that ends here
  uint64_t val;       // (device log only; <= the snapshot index when the run reaches it)
};

// ---- kvraft (SEMANTICS §8-9); arrays allocated for the kvraft scenarios only
enum : uint32_t { KV_GET = 0, KV_PUT = 1, KV_APPEND = 2 };
enum : uint32_t { KV_OK = 0, KV_WRONG_LEADER = 1, KV_FAILED = 2 };
constexpr uint32_t CLERK_HOST = 8;  // clerk c is host 8 + c
constexpr uint32_t KV_PEND = 8;     // pending requests per server
// kt32 [C][nthr(S)][KT_STRIDE]: a spawned tester thread (+ its clerk, kvraft) per slot.
// Words KT_W.. are the thread's own frame: kvraft clerk fields, churn client
// (x lo/hi, index, timeout step, values), or a one() task (helper frame h[0..4], cmd).
enum : uint32_t {
  KT_TID, KT_LIVE, KT_PC, KT_J, KT_CLI, KT_TCTR, KT_ID, KT_LH, KT_SEQ, KT_TAG, KT_NCTR,  // (wake: kwk)
  KT_WAITING, KT_GOT, KT_RSTAT, KT_RHINT, KT_RVAL, KT_OP, KT_KEY, KT_ELEM,
  KT_KIND,  // 1 = generic_test partitioner (KT_PERM: its shuffled `all`, 4 bits per server)
  KT_PERM,
  KT_RVH0, KT_RVH1,  // the reply's value hash
  KT_HL0, KT_HL1,    // generic_test client: hash of its predicted value `last`
  KT_OWN,            // the thread the clerk's calls wake (0 = the test body)
  KT_MCL,            // 1 = a clerk of the test body in a slot that is not a thread
  KT_LLO,            // a Get's linearizability lower bound at its call (SEMANTICS §9a)
  KT_TOP, KT_TKEY, KT_TELEM, KT_TCNT,  // a task's call: op, key, elem (or appender), calls
  KT_LEP, KT_LNP,    // generic_test_linearizability (§9b): the key's Put epoch at the call, no
                     // Put pending at the call
  KT__N
};
constexpr uint32_t KT_W = KT_ID;
constexpr uint32_t KT_STRIDE = (KT__N + 3u) & ~3u;  // words per thread-slot record (16-B multiple)
constexpr uint32_t JOIN_ALL = 0xFFFFFFFEu;
constexpr uint32_t JOIN_ANY = 0xFFFFFFFDu;  // select! over spawned tasks: the first finish wakes
// kvraft key ids / Put value tokens of the test bodies (SEMANTICS §9)
constexpr uint32_t key_letter(char c) { return 50u + (uint32_t)(c - 'a'); }
constexpr uint32_t tok_num(uint32_t v) { return v + 1u; }
constexpr uint32_t tok_letter(char c) { return (1u << 20) + (uint32_t)(c - 'A'); }
constexpr uint32_t CHURN_VCAP = 512;  // values one churn client may record (tests.rs:763-797)
// kv32 [C][n][KVREC]: per-server KV state (SEMANTICS §9): dedup[clerk] at 0..127, pending
// request p at 128 + 8p: {index (0 = free), clerk | ready << 8 | status << 9 | host << 16,
// seq, tag, value, hash lo, hash hi, -}, the shard_ctrler config count at 192, the mask of
// occupied pending slots at 193, and key k at 256 + 8k: {hash lo, hash hi, byte length,
// appender 0..4 (cli + 1 | count << 8 | bad << 31)}
constexpr uint32_t KVR_DEDUP = 0, KVR_PEND = 128, KVR_NCFG = 192, KVR_PMASK = 193, KVR_KEYS = 256,
                   KVREC = 768;
constexpr uint32_t KV_KEYS = 64, KV_KW = 8, KV_APP = 5, MAX_CLERKS = 128;
constexpr uint32_t KV_ALL = 0xFFFFFFu;  // Get elem: appenders 0..4, packed
constexpr uint64_t KV_HP = 0x100000001B3ull;  // value hash multiplier
// a KV snapshot (SEMANTICS §9): dedup[128] then the 64 key records; the ring entry for
// index i (slot i / 16 mod 16) holds i at word 0 and the snapshot from word 4
constexpr uint32_t KVS_W = MAX_CLERKS + KV_KEYS * KV_KW, KV_RING = 16, KRW = 4 + KVS_W;
constexpr uint32_t KV_SNAP_EVERY = 16;
// linearizability bookkeeping per (key, appender): tag (cli + 1), appends called, appends
// acknowledged, largest count a returned Get observed, an all-appenders Get's lower bound
constexpr uint32_t LINW = 8;
// generic_test_linearizability (SEMANTICS §9b): 15 clients share keys 0..14, each key record
// is 32 words (hash lo, hi, length, the states of clients 0..14 by id: count | last j << 12 |
// bad << 31), and the tester keeps per key 32 words of lin32: called[15], acked[15], the Put
// epoch and the Puts pending; word 512 + cli of the cluster's lin32: client cli's next j
constexpr uint32_t LIN_CLI = 15, KV_KW15 = 32, LIN15_J = 512;
// ---- shard_ctrler (SEMANTICS §10): per-server append-only config store and a
// per-cluster table of clerk operations (the log command names an operation)
constexpr uint32_t N_SHARDS = 10;  // shard_ctrler/mod.rs:9
constexpr uint32_t CFG_CAP = 128, CFG_G = 32, OP_CAP = 256;
// cfg32 [C][n][CFG_CAP][CFGW]: num, shards[10], ng, gid[32], addr[32]
enum : uint32_t { CF_NUM = 0, CF_SHARDS = 1, CF_NG = 11, CF_GID = 12, CF_ADDR = 44, CFGW = 80 };
// op32 [C][OP_CAP][OPW]: type, a (num / shard), b (gid), ng, gid[5], addr[5]
enum : uint32_t { OP_TYPE = 0, OP_A, OP_B, OP_NG, OP_GID, OP_ADDR = 9, OPW = 16 };
enum : uint32_t { CT_QUERY = 0, CT_JOIN = 1, CT_LEAVE = 2, CT_MOVE = 3 };

// one tester apply-checker index (StorageHandle, tester.rs:366-428): the value
// the first applier stored, the mask of servers whose log holds it, and the
// entry's term (for the MR_F_SAFETY leader-completeness check)
struct alignas(16) SE {
  uint64_t val;
  uint32_t mask, term;
};

// Dev::tape_mode (SEMANTICS §12): what a draw does in the decision-tape kernels, which run whenever
// it is not TAPE_OFF. Whatever the mode, the draw's seed is the one seed rule of philox()
enum TapeMode : uint32_t {
  TAPE_OFF = 0,  // Philox from the cluster's own seed: the pool / step kernels
  TAPE_LOOKUP,   // look the key up in my slice (replay, variants); a miss is counted and drawn
  TAPE_RECORD,   // draw and append {key, words} to my tape
  TAPE_SEEDS     // only take my seed from the list (no tables)
};

// ---- everything the kernels see (passed by value as a kernel argument)
struct Dev {
  // config
  uint32_t C, n, log_cap, apply_cap, M, K, hb, elo, ehi, max_events;
  uint32_t null_raft, unrel_flag, trace_clusters, trace_cap, scenario, iters, safety, bugs, links;
  uint64_t seed0;  // seed of cluster 0 = seed_base + cluster_base
  // the batch's arrays, these and those below without a shape: the rows of MR_DEV_ARRAYS
  uint32_t* cs32; uint64_t* cs64; uint32_t* nd32;
  uint32_t* tmr;    // node timers (registers during a launch)
  uint32_t* ms32; uint64_t* mkey;
  LE* log;          // ring per node
  LE* pay;          // AppendEntries payload per message slot
  SE* stor;         // tester storage (tester.rs:366-428)
  uint32_t* kt32; uint32_t* kv32;
  uint32_t* kvs32;  // persisted KV snapshots (maxraftstate)
  uint32_t* kring;  // recent KV snapshots by index (maxraftstate)
  uint4* dtab;      // keyed decisions {stream << 16 | entity, seq, w0, w1}, else null:
                    // lookup: the groups' tapes one after the other, each slice sorted by key;
                    // record: [C][dcap], appended in draw order
  // a seed list (mr_batch_set_seeds, SEMANTICS §12.3), else null: [C] cluster c draws from the seed
  // seed0 + sof[c]. Read by the tape kernels' philox() only; the batch's own allocation beside its
  // decision tables, no row of MR_DEV_ARRAYS: it outlives a reset untouched and most batches have none
  const uint32_t* sof;
  uint32_t dcap;       // record: decisions kept per cluster
  uint32_t tape_mode;  // a TapeMode: what a draw of the tape kernels does (0: the pool / step kernels run)
  // lookup (TAPE_LOOKUP, SEMANTICS §12 - §12.2): a cluster looks its draws up in its group's slice of
  // dtab, takes its group's edits where its mask row says so, and draws its misses from its group's
  // seed, seed0 + seed_cluster. Replay is a variant batch of C one-cluster groups without edits:
  // cluster c's slice is its row, its seed_cluster is c, and vedit, vwords, vmask are null, vW 0
  // (mr_batch_set_variants: one group, slice = the table, seed_cluster 0)
  uint4* tdesc;     // [C] the cluster's group: {slice offset, slice records (0: every draw misses),
                    // its first edit in vwords, seed_cluster} (one load per draw, no group_of ->
                    // groups indirection)
  uint32_t* vedit;  // [records] the record's edit within its group, ~0u = none; null: no record has one
  uint2* vwords;    // [edits] an edit's replacement words (w0, w1), the groups' one after the other
  uint32_t* vmask;  // [C][vW] bit j of cluster c's row: c takes its group's edit j
  uint32_t vW;      // mask words per cluster = ceil(the widest group's edits / 32)
  uint64_t* cval;   // churn clients' committed values
  uint32_t* cidx;   // ... and the index each was seen at
  uint32_t* cfg32;  // shard_ctrler config stores
  uint32_t* op32;   // shard_ctrler operations
  uint32_t nthr;    // thread slots of kt32 (0 = none)
  mr_event* trace;
  uint64_t* tdig;   // apply digest of each record (ABI 4)
  uint64_t* tapp;   // KV command, key hash after it (ABI 4)
  uint64_t* adig;   // per node: digest sum, invalid flag
  uint32_t* led;    // MR_F_SAFETY: bit t = a leader was elected in term t
  uint32_t* lin32;  // kvraft linearizability bookkeeping (§9a, §9b)
  uint32_t lin15;   // generic_test_linearizability layout (§9b): key records / bookkeeping
  uint32_t* remaining;  // clusters without verdict after a step launch; next unclaimed cluster
  uint32_t L;           // clusters per launch: lane l starts with cluster c0 + l (chunk [c0, c0 + L))
  uint32_t lpw;         // lanes of each 64-lane block that hold a cluster (64, 32, 16; the rest idle)
  uint32_t c0;          // first cluster of this launch's chunk
  uint32_t stream;      // MR_F_STREAM: a lane that finishes takes the next unclaimed cluster
  uint32_t resume;      // streaming, not the chunk's first launch: lanes first take held_in[]
  uint32_t nheld;       // ... the clusters the previous launch's lanes still held
  uint32_t* held_in;    // [L] those clusters (streaming)
  uint32_t* held_out;   // [L] this launch's (index = its remaining[0] count)
  unsigned long long* prof;  // wave-cycle profile (MR_PROF builds only)
  uint4* tfr;       // the tester coroutine frame, one cluster-major 80-B record
  uint32_t* kwk;    // thread slots' {tid, wake}: the scheduler's keys, packed
  uint32_t pool;    // the batch runs on pool_kernel (has_pool): 32-bit keys with the AE bit
  uint32_t* guard;  // MR_GUARD builds: an out-of-range index {tag, cluster, index, bound}
  uint32_t gprobe;  // MR_GUARD builds, MR_GUARD_PROBE set: cluster 0's first delivery reads slot M
  unsigned long long* pcnt;  // pool_kernel: the workgroups' counter sums (64-bit; reduce adds them)
  uint32_t krows;   // the 7-server Raft pool: message slots whose keys live in LDS (the rest in HBM)
  // parameter groups (mr_batch_set_param_groups, SEMANTICS §12.4), else null: [C] one PG_W-word
  // record per cluster, its group's values of the eight parameters above that a group may set
  // (PG_*; one load, no group_of -> groups indirection, as tdesc). Read by the tape kernels'
  // accessors only (mr_kernel.hip p_hb() ..); the batch's own allocation beside sof, no row of
  // MR_DEV_ARRAYS. Last, so that no field the step and pool kernels read moves
  const uint32_t* pgrp;
};
// a cluster's parameter record (Dev::pgrp): the group's value of Dev's field of the same name
enum : uint32_t { PG_HB, PG_ELO, PG_EHI, PG_K, PG_ITERS, PG_BUGS, PG_UNREL, PG_NULL, PG_W };
static_assert(PG_W * 4 == sizeof(mr_param_group), "one 32-B record per cluster");
// words-pairs per cluster of kwk: the thread slots rounded up to whole 16-B quads (two slots each;
// slot 0 = the test body and the pad slot hold ~0, so they never win a rescan)
constexpr uint32_t kws(uint32_t nthr) { return (nthr + 1u) & ~1u; }
// tester frame record (tester() in mr_kernel.hip): pc | helper << 24, result, locals l[0..7],
// helper frame h[0..4], u64 argument hv — 17 words in five 16-B quads, loaded and stored whole
constexpr uint32_t TF_Q = 5;
constexpr uint32_t PROF_SLOTS = 96;  // 64..94: pool_kernel statistics (MR_PROF, tools/prof.py)
// election-safety term bitmap (MR_F_SAFETY): terms 0..LED_TERMS-1; a leader elected in a
// later term is a simulator limit (MR_FAIL_SIM_CAPACITY); figure_8 peaks at term 177
constexpr uint32_t LED_W = 64, LED_TERMS = 32 * LED_W;

// The kind column of madraft_sim.h's MR_SCENARIO_TABLE (0 for an id without a row: no service)
constexpr bool is_kv(uint32_t s) { return mr_scn_is_kv(s); }
constexpr bool is_ctrl(uint32_t s) { return mr_scn_kind(s) == MR_KIND_CTRL; }
// scenarios served by the clerk / server request path (kvraft + shard_ctrler)
constexpr bool is_svc(uint32_t s) { return is_kv(s) || is_ctrl(s); }
#define MR_ROW_(id, sym, name, n, kind, slots, exact, pool) static_assert(id < MR_SCN_COUNT_, name);
MR_SCENARIO_TABLE(MR_ROW_)
#undef MR_ROW_
// generic_test(nclients, unreliable, crash, partitions, maxraftstate) of a kvraft scenario
// (kvraft/tests.rs:222-384, 494-522); snapshot_rpc / snapshot_size use maxraftstate too
struct KvGen { uint32_t nc; bool unrel, crash, part; uint32_t maxraft; };
constexpr KvGen kv_gen(uint32_t s) {
  switch (s) {
    case MR_SCN_KV_BASIC_3A: return {1, false, false, false};
    case MR_SCN_KV_CONCURRENT_3A: return {5, false, false, false};
    case MR_SCN_KV_UNRELIABLE_3A: return {5, true, false, false};
    case MR_SCN_KV_MANY_PARTITIONS_ONE_CLIENT_3A: return {1, false, false, true};
    case MR_SCN_KV_MANY_PARTITIONS_MANY_CLIENTS_3A: return {5, false, false, true};
    case MR_SCN_KV_PERSIST_ONE_CLIENT_3A: return {1, false, true, false};
    case MR_SCN_KV_PERSIST_CONCURRENT_3A: return {5, false, true, false};
    case MR_SCN_KV_PERSIST_CONCURRENT_UNRELIABLE_3A: return {5, true, true, false};
    case MR_SCN_KV_PERSIST_PARTITION_3A: return {5, false, true, true};
    case MR_SCN_KV_PERSIST_PARTITION_UNRELIABLE_3A: return {5, true, true, true};
    case MR_SCN_KV_UNRELIABLE_ONE_KEY_3A: return {5, true, false, false};
    case MR_SCN_KV_ONE_PARTITION_3A: return {0, false, false, true};
    case MR_SCN_KV_SNAPSHOT_RPC_3B: return {0, false, false, true, 1000};
    case MR_SCN_KV_SNAPSHOT_SIZE_3B: return {0, false, false, false, 1000};
    case MR_SCN_KV_SNAPSHOT_RECOVER_3B: return {1, false, true, false, 1000};
    case MR_SCN_KV_SNAPSHOT_RECOVER_MANY_CLIENTS_3B: return {20, false, true, false, 1000};
    case MR_SCN_KV_SNAPSHOT_UNRELIABLE_3B: return {5, true, false, false, 1000};
    case MR_SCN_KV_SNAPSHOT_UNRELIABLE_RECOVER_3B: return {5, true, true, false, 1000};
    case MR_SCN_KV_SNAPSHOT_UNRELIABLE_RECOVER_CONCURRENT_PARTITION_3B: return {5, true, true, true, 1000};
    // generic_test_linearizability (15 clients, 7 servers; SEMANTICS §9b): mr_scn_is_lin15
    case MR_SCN_KV_PERSIST_PARTITION_UNRELIABLE_LINEARIZABLE_3A: return {15, true, true, true, 0};
    case MR_SCN_KV_SNAPSHOT_UNRELIABLE_RECOVER_CONCURRENT_PARTITION_LINEARIZABLE_3B:
      return {15, true, true, true, 1000};
    default: return {0, false, false, false, 0};
  }
}
// the service pool's applier continuation (mr_kernel.hip AP_CAP) is built for the 15-client
// linearizable body without service snapshots, whose reconnected followers apply long backlogs:
// same box (profiles/r06_ab_kvap.txt) C5-lin 3A 76.4 K -> 103.8 K seeds/s (+36 %), while built for
// every service body config 5 (unreliable_3a) lost 21 % and the snapshotting 3B body 2 % (short
// backlogs: the extra kind and the registers cost more than the balance gains)
// (the snapshotting linearizable 3B body with it, cap 5: 89.8 K -> 88.5 K seeds/s, -1.4 %,
// profiles/r06_ab_kv47.txt)
constexpr bool ap_cont(uint32_t s) { return mr_scn_is_lin15(s) && kv_gen(s).maxraft == 0; }
// the KV snapshot copy's chunk (quads whose loads issue together, kv_snapshot): 8 for
// the 15-client linearizable body, 4 for the others. Same box (profiles/r06_ab_kc.txt): the
// snapshotting linearizable 3B body 89.7 K -> 93.6 K seeds/s with 8 (+4.4 %; 16: -5 %), the 5-client
// 3B body 238 K -> 220 K (-7.5 %: its kernel spills the larger chunk)
constexpr uint32_t kv_chunk(uint32_t s) { return mr_scn_is_lin15(s) ? 8u : 4u; }
// tester thread slots (slot 0 = the test body): kvraft 1 + 5 clients, churn 1 + 3
// clients, unreliable_agree_2c up to 63 concurrent one() tasks
constexpr uint32_t nthr(uint32_t s) {
  return is_kv(s) ? (kv_gen(s).nc + 2u > 6u ? kv_gen(s).nc + 2u : 6u)  // + test body, partitioner
         : is_ctrl(s) ? 11u : mr_scn_is_churn(s) ? 4u
         : s == MR_SCN_UNRELIABLE_AGREE_2C ? 64u : 0u;
}

// step-kernel instances (mr_kernel.hip launch_step_t<S, NB>): per scenario, one
// per exact server count (has_exact) and one for up to 8 servers
template <uint32_t S, uint32_t NB>
hipError_t launch_step_t(const Dev& D, uint32_t budget, hipStream_t s);
// the pool kernel of scenario S (has_pool(S, NB); mr_kernel.hip MR_POOL units)
template <uint32_t S, uint32_t NB>
hipError_t launch_pool_t(const Dev& D, uint32_t budget, hipStream_t s);
template <uint32_t S, uint32_t NB>
uint32_t pool_capacity_t(int device, uint32_t M);
// lanes the step kernel of scenario S keeps resident on the device (occupancy x CUs x block)
template <uint32_t S, uint32_t NB>
uint32_t step_capacity_t(int device, uint32_t M);
// the same kernels built with decision-tape draws (MR_TAPE=1 translation units, NB = 8):
// replay and record runs only, so the common draw path carries no tape branch
template <uint32_t S, uint32_t NB>
hipError_t launch_step_tape_t(const Dev& D, uint32_t budget, hipStream_t s);
// exact-size step-kernel instances (NB = n < 8): the node count is a compile-time constant there
// (every `q < n` over the unrolled node loops folds away, and with it the loop-invariant lane
// masks the compiler otherwise keeps in scalar registers); any other n runs the generic 8-server
// instance. Built: the table's `exact` column — each scenario at its default n, BASELINE config 2
// (fail_agree_2b at 5 servers) and config 4 (the 2D tests at 7: arrays sized for 7 keep fewer
// registers live than the 8-server instance)
constexpr bool has_exact(uint32_t s, uint32_t n) { return n < 8u && (mr_scn_exact_mask(s) >> n & 1u); }
// pool-kernel instances (mr_kernel.hip pool_kernel), the table's `pool` column:
// Raft-only test bodies without spawned threads at an exact server count of 3, 5 or 7
// (512-cluster pools, up to 64 message slots: the 32-bit keys of slots 0..31 take 64 KiB of LDS,
// slots 32..63 — 7-server bodies, BASELINE config 4 — keep theirs in HBM), and the kvraft /
// shard_ctrler test bodies at their exact server count (256-cluster pools, up to 64 message
// slots, all keys in LDS; not the 20-clerk snapshot_recover_many_clients_3b, whose 256 slots and
// clerk hosts do not fit)
constexpr bool has_pool(uint32_t s, uint32_t n) {
  return has_exact(s, n) && mr_scn_pool(s) != MR_POOL_FAMILY_NONE;
}
constexpr uint32_t pool_max_slots(uint32_t s, uint32_t n) { return is_svc(s) || n > 5u ? 64u : 32u; }
// why a row may say what it says: a bad row fails here, not at the first launch
#define MR_ROW_(id, sym, name, n, kind, slots, exact, pool)                                        \
  static_assert(MR_POOL_FAMILY_##pool != MR_POOL_FAMILY_RAFT || (nthr(id) == 0 && !is_svc(id)),    \
                name ": the Raft pool runs no spawned tester threads and no service");             \
  static_assert(MR_POOL_FAMILY_##pool != MR_POOL_FAMILY_SVC || (is_svc(id) && slots <= 64),        \
                name ": the service pool runs kvraft / shard_ctrler bodies of up to 64 slots");    \
  static_assert(MR_POOL_FAMILY_##pool == MR_POOL_FAMILY_NONE || exact != 0,                        \
                name ": pool kernels exist at exact server counts only");                          \
  static_assert((exact & ~0xA8) == 0,                                                              \
                name ": exact-size units are built and dispatched for 3, 5 and 7 servers (< 8)");  \
  static_assert(n >= 3 && n <= MR_MAX_NODES && (n >= 8 || (exact >> n & 1)),                       \
                name ": the default server count below 8 has its exact instance");
MR_SCENARIO_TABLE(MR_ROW_)
#undef MR_ROW_
// scenarios in which a log can be compacted: the service snapshots of snap_common (mr_scn_is_snap2d:
// t_new(snapshot = true), tester.rs:303-325 SNAPSHOT_INTERVAL; node_apply_coop specializes on it
// at compile time and checks it against the runtime mode, x.netmode bit 1) or a kvraft
// maxraftstate. Everywhere else snap stays 0, so no InstallSnapshot is ever sent (the node
// event compiles that path out of its send loop)
constexpr bool has_snaps(uint32_t s) { return mr_scn_is_snap2d(s) || kv_gen(s).maxraft > 0; }
// test bodies that crash and restart servers (crash1 / start1, tester.rs:293-333): persist1-3,
// figure_8 and its unreliable crash variant, the 2D crash variants, the churn tests
constexpr bool restarts_servers(uint32_t s) {
  return (s >= MR_SCN_PERSIST1_2C && s <= MR_SCN_FIGURE_8_2C) || s == MR_SCN_RELIABLE_CHURN_2C ||
         s == MR_SCN_UNRELIABLE_CHURN_2C || s == MR_SCN_SNAPSHOT_INSTALL_CRASH_2D ||
         s == MR_SCN_SNAPSHOT_INSTALL_UNRELIABLE_CRASH_2D || s == MR_SCN_FIGURE_8_UNRELIABLE_CRASH;
}
// ---- the batch's device arrays, one row each, in the order they are carved from the batch's one
// allocation (every array 256-B aligned): X(Dev member, owner(elements per owner), present, reset)
//   owner     whose state the row is, and with it how many times its elements repeat:
//             MR_MINOR(w): a cluster-minor matrix [w][C], field f of cluster c at f * C + c;
//             MR_MAJOR(w): cluster-major records [C][w], cluster c's slab at c * w;
//             MR_TRACED(w): as MR_MAJOR for the traced clusters only, [trace_clusters][w];
//             MR_SHARED(w): w elements of the batch, no cluster's state
//             (the first three are what mr_batch_fork copies; a row without an owner does not compile:
//             its element count names no C, and is no OwnKind for k_dev_own)
//   elements  per owner, over the config: n servers, M message slots, K = ae_max, log_cap, apply_cap,
//             trace_cap, safety (1 with MR_F_SAFETY, else 0), and the scenario s (nthr(s) thread slots,
//             kws() of them for the scheduler keys). The array holds them x C clusters, or x
//             trace_clusters (0 unless MR_F_TRACE), or once (dev_layout)
//   present   over s; an absent or empty array is a null pointer
//   reset     ZERO(k): the k-th memset of mr_batch_reset; KERNEL: reset_kernel initialises it; NONE: a
//             run writes it before it reads it (the row says why); GUARD: ZERO in MR_GUARD builds
#define MR_DEV_ARRAYS(X)                                                                          \
  X(cs32, MR_MINOR(CS_STRIDE), true, KERNEL)                                                      \
  X(cs64, MR_MINOR(C64_STRIDE), true, KERNEL)                                                     \
  X(nd32, MR_MAJOR(NREC * n), true, KERNEL)                                                       \
  X(tmr, MR_MINOR(n), true, KERNEL)                                                               \
  X(ms32, MR_MAJOR(MREC * M), true, NONE) /* a slot's record is written when its key is: at the send */ \
  X(mkey, MR_MINOR(M), true, KERNEL)                                                              \
  X(log, MR_MAJOR(n * log_cap), true, NONE) /* entries up to NF_LAST, each written by its append */ \
  X(pay, MR_MAJOR(M * K), true, NONE)       /* written when the slot's message takes a payload */  \
  X(stor, MR_MAJOR(apply_cap), true, ZERO(2))                                                     \
  X(kt32, MR_MAJOR(KT_STRIDE * nthr(s)), nthr(s) > 0, KERNEL)                                     \
  X(kwk, MR_MAJOR(2 * kws(nthr(s))), nthr(s) > 0, KERNEL)                                         \
  X(kv32, MR_MAJOR(KVREC * n), is_svc(s), ZERO(7))                                                \
  X(lin32, MR_MAJOR(KV_KEYS * KV_APP * LINW), is_kv(s), ZERO(8))                                  \
  X(kvs32, MR_MAJOR(KVS_W * n), kv_gen(s).maxraft > 0, ZERO(9))                                   \
  X(kring, MR_MAJOR(KRW * KV_RING), kv_gen(s).maxraft > 0, ZERO(10))                              \
  X(cfg32, MR_MAJOR(CFG_CAP * CFGW * n), is_ctrl(s), KERNEL)                                      \
  X(op32, MR_MAJOR(OP_CAP * OPW), is_ctrl(s), NONE) /* rows below CS_NOPS, each written by its clerk */ \
  X(cval, MR_MAJOR(3 * CHURN_VCAP), mr_scn_is_churn(s), NONE) /* up to the client's own count */  \
  X(cidx, MR_MAJOR(3 * CHURN_VCAP), mr_scn_is_churn(s), NONE) /* as cval */                       \
  X(led, MR_MAJOR(safety * LED_W), true, ZERO(3))                                                 \
  X(trace, MR_TRACED(trace_cap), true, NONE) /* records below CS_TRACEN */                        \
  X(tdig, MR_TRACED(trace_cap), true, ZERO(4))                                                    \
  X(tapp, MR_TRACED(trace_cap * 2), true, ZERO(5))                                                \
  X(adig, MR_TRACED(MR_MAX_NODES * 2), true, ZERO(6))                                             \
  X(remaining, MR_SHARED(2), true, NONE)  /* copied from the host before every launch */          \
  X(prof, MR_SHARED(PROF_SLOTS), true, NONE) /* zeroed at create: a profile sums over the batch's runs */ \
  X(guard, MR_SHARED(4), true, GUARD)        /* zeroed at create */                               \
  X(pcnt, MR_SHARED(CNT__N), true, ZERO(0))                                                       \
  X(tfr, MR_MAJOR(TF_Q), true, KERNEL)
#define MR_ROW_(m, elements, present, reset) A_##m,
enum DevArray : uint32_t { MR_DEV_ARRAYS(MR_ROW_) A__N };
#undef MR_ROW_
constexpr int RST_NONE = -2, RST_KERNEL = -1;  // (a ZERO row: its place k)
#define RST_ZERO(k) (k)
#if MR_GUARD
#define RST_GUARD RST_ZERO(1)  // a violation belongs to the run it happened in
#else
#define RST_GUARD RST_NONE
#endif
#define MR_ROW_(m, elements, present, reset) RST_##reset,
constexpr int k_dev_reset[A__N] = {MR_DEV_ARRAYS(MR_ROW_)};  // by DevArray
#undef MR_ROW_
// whose state a row is (its owner column), by DevArray: the one place the fork, the layout and the
// checks read it from
enum OwnKind : uint32_t { OWN_MINOR, OWN_MAJOR, OWN_TRACED, OWN_SHARED };
#define MR_MINOR(w) OWN_MINOR
#define MR_MAJOR(w) OWN_MAJOR
#define MR_TRACED(w) OWN_TRACED
#define MR_SHARED(w) OWN_SHARED
#define MR_ROW_(m, elements, present, reset) elements,
constexpr OwnKind k_dev_own[A__N] = {MR_DEV_ARRAYS(MR_ROW_)};  // by DevArray
#undef MR_ROW_
#undef MR_MINOR
#undef MR_MAJOR
#undef MR_TRACED
#undef MR_SHARED
// a cluster's state between launches is the rows owned per cluster or per traced cluster
constexpr bool own_is_cluster(OwnKind k) { return k != OWN_SHARED; }
// a batch of scenario s has array a: the kernels' template constant S folds it, so an array's
// presence is typed out in its row only
constexpr bool dev_has(uint32_t s, DevArray a) {
#define MR_ROW_(m, elements, present, reset) if (a == A_##m) return present;
  MR_DEV_ARRAYS(MR_ROW_)
#undef MR_ROW_
  return false;
}
// Dev's fields the scenario alone fixes: set by the host at create, and by fix_scenario<S>, where they fold
constexpr void scenario_fixed(Dev& D, uint32_t s) {
  D.nthr = nthr(s);
  D.links = kv_gen(s).part ? 1u : 0u;      // server-link cuts (CS_CUT) can exist
  D.lin15 = mr_scn_is_lin15(s) ? 1u : 0u;  // generic_test_linearizability layout (SEMANTICS §9b)
}
// Where a batch of config c keeps its arrays: a function of the config alone, so it is checked
// without a device (tests/test_abi.py, tests/test_fork_host.py). per: the bytes one owner has of the
// array (a cluster, a traced cluster, or the batch for an OWN_SHARED row); bytes = per x the row's
// owners, 0: absent or empty; off[A__N]: the allocation's size
struct DevLayout { size_t per[A__N], bytes[A__N], off[A__N + 1]; };
// owners of a row of kind k in a batch of C clusters of which trace_clusters are traced
constexpr uint64_t dev_owners(OwnKind k, uint64_t C, uint64_t trace_clusters) {
  return k == OWN_SHARED ? 1u : k == OWN_TRACED ? trace_clusters : C;
}
inline DevLayout dev_layout(const mr_cfg& c) {
  const uint64_t C = c.n_clusters, n = c.n_nodes, M = c.msg_slots, K = c.ae_max, log_cap = c.log_cap,
                 apply_cap = c.apply_cap, trace_cap = c.trace_cap, trace_clusters = (c.flags & MR_F_TRACE) ? c.trace_clusters : 0u;
  const uint32_t s = c.scenario, safety = (c.flags & MR_F_SAFETY) ? 1u : 0u;
  DevLayout L{};
#define MR_MINOR(w) (w)
#define MR_MAJOR(w) (w)
#define MR_TRACED(w) (w)
#define MR_SHARED(w) (w)
#define MR_ROW_(m, elements, present, reset) \
  L.per[A_##m] = dev_has(s, A_##m) ? (uint64_t)(elements) * sizeof(*Dev().m) : 0u;
  MR_DEV_ARRAYS(MR_ROW_)
#undef MR_ROW_
#undef MR_MINOR
#undef MR_MAJOR
#undef MR_TRACED
#undef MR_SHARED
  for (uint32_t a = 0; a < A__N; a++) {
    L.bytes[a] = L.per[a] * dev_owners(k_dev_own[a], C, trace_clusters);
    if (!L.bytes[a]) L.per[a] = 0;  // (no owner: absent)
    L.off[a + 1] = L.off[a] + ((L.bytes[a] + 255) & ~size_t(255));
  }
  return L;
}
// D's array members point into the allocation at `base` as L lays it out
inline void dev_carve(Dev& D, const DevLayout& L, char* base) {
#define MR_ROW_(m, elements, present, reset) \
  D.m = L.bytes[A_##m] ? reinterpret_cast<decltype(D.m)>(base + L.off[A_##m]) : nullptr;
  MR_DEV_ARRAYS(MR_ROW_)
#undef MR_ROW_
}

// ---- mr_batch_fork (SEMANTICS §12.5): what fork_kernel (mr_fork.inc) is told, its own argument —
// Dev does not change for it. One ForkRow per array of the table that both batches have and that
// is some cluster's state, as the host walks the table, and one for the record tape.
enum ForkKind : uint32_t { FK_MINOR, FK_MAJOR, FK_TAPE };  // (OWN_TRACED rows are FK_MAJOR over the traced)
constexpr uint32_t FORK_SKIP = ~0u;  // src_of[c]: position c stays as it is
constexpr uint32_t FORK_BLOCK = 256, FORK_QUADS = 4 * FORK_BLOCK, FORK_FIELDS = 8;
struct ForkRow {
  char* dst;
  const char* src;
  uint32_t kind;    // a ForkKind
  uint32_t owners;  // destination owners: its clusters, or its traced clusters
  uint32_t dper;    // FK_MINOR: fields; else the bytes one owner has in the destination (16-B quads)
  uint32_t sper;    // ... in the source
  uint32_t esz;     // FK_MINOR: bytes of an element, 4 or 8
  uint32_t zfield;  // FK_MINOR: the field that becomes 0 in every forked position, ~0u: none
  uint32_t blk0;    // the row's first block of the launch
  uint32_t pad;
};
constexpr uint32_t FORK_ROWS = A__N + 1;
struct ForkPlan {
  const uint32_t* src_of;     // [Cd] the destination positions' sources, FORK_SKIP: none
  const uint32_t* tape_used;  // FK_TAPE: the source's CS_TAPE row, [Cs]
  uint32_t Cd, Cs;            // clusters of the destination and of the source: the FK_MINOR strides
  uint32_t n_rows, blocks;    // rows in use; the launch's blocks = the last row's end
  ForkRow row[FORK_ROWS];
};
// blocks of FORK_BLOCK threads a row takes (mr_fork.inc says how they divide it)
constexpr uint64_t fork_blocks(const ForkRow& r) {
  if (r.kind == FK_MINOR)
    return (uint64_t)((r.dper + FORK_FIELDS - 1) / FORK_FIELDS) * ((r.owners + FORK_BLOCK - 1) / FORK_BLOCK);
  const uint32_t q = r.dper / 16u;
  if (q >= FORK_QUADS || r.kind == FK_TAPE) return (uint64_t)r.owners * ((q + FORK_QUADS - 1) / FORK_QUADS);
  const uint32_t opb = FORK_QUADS / q;  // owners per block
  return ((uint64_t)r.owners + opb - 1) / opb;
}
hipError_t launch_fork(const ForkPlan& P, hipStream_t s);

#define MR_INST_ROW_(id, sym, name, n, kind, slots, exact, pool) MR_INST(id)
#define MR_ALL_SCNS MR_SCENARIO_TABLE(MR_INST_ROW_)  // MR_INST(id) for every row of the table

}  // namespace mr
