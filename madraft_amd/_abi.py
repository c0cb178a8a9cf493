"""ctypes mirror of include/madraft_sim.h (structs, enums, numpy trace dtype).

Plain data definitions only; loading a library is done by madraft_amd.sim
(the HIP product) or by the tests (the CPU oracle).
"""
import collections
import ctypes as C
import os
import re

import numpy as np

MR_ABI_VERSION = 7
MR_MAX_NODES = 8
MR_RUNNING = 0xFFFF
MR_PASS = 0

MR_F_UNRELIABLE = 0x1
MR_F_NULL_RAFT = 0x2
MR_F_TRACE = 0x4
MR_F_SAFETY = 0x8
MR_F_BUG_VOTE_TWICE = 0x10
MR_F_BUG_VOTE_STALE = 0x20
MR_F_BUG_NO_PREV_CHECK = 0x40
MR_F_RECORD = 0x80
MR_F_BUG_NO_DEDUP = 0x100
MR_F_BUG_STALE_READ = 0x200
MR_F_STREAM = 0x400  # lanes < clusters: finished lanes take the next cluster (mr_cfg.lanes)
MR_F_BUG_NO_APPLY_CHECK = 0x800  # test-only: apply checker compares no values (ABI 4)
DIGEST_INVALID = (1 << 64) - 1  # mr_trace_digests: the node's prefix was not applied entry by entry


def apply_mix(i, v):
    """include/madraft_sim.h mr_apply_mix: the apply-digest term of entry i with value v."""
    m = (1 << 64) - 1
    z = (v ^ (i * 0x9E3779B97F4A7C15)) & m
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & m
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & m
    return z ^ (z >> 31)

README_SEED = 1629626496  # /root/reference/README.md:48


HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                      "include", "madraft_sim.h")
_ROW = re.compile(r'\s*X\((\w+), (\w+), "((?:[^"\\]|\\.)*)"'
                  r'(?:, (\d+), (\w+), (\d+), (0x[0-9A-Fa-f]+), (\w+))?\)')
_COUNTER_ROW = re.compile(r'\s*X\(([A-Z_]+), ([a-z_]+), (SUM|MAX), (BOTH|HIP)\)')


def _table(name, row=_ROW):
    """The rows of the header's X-macro `name`, fields as written: X(id, SYMBOL, "text"[, servers,
    kind, slots, exact mask, pool]), or what `row` reads, up to the first line that does not
    continue."""
    with open(HEADER) as f:
        lines = f.read().split(f"#define {name}(X) \\\n", 1)[1].split("\n")
    rows = []
    for line in lines:
        m = row.match(line)
        if m:
            rows.append(m.groups())
        elif line.lstrip().startswith("X("):
            raise ValueError(f"{name}: cannot read the row {line.strip()!r}")
        if not line.endswith("\\"):
            break
    return rows


Scenario = collections.namedtuple("Scenario", "id symbol name servers kind slots exact pool")
# MR_SCENARIO_TABLE: one row per scenario (exact: bit n = an n-server kernel instance is built;
# pool: the pool-kernel family, NONE / RAFT / SVC)
SCENARIO_ROWS = [Scenario(int(i), sym, name, int(n), kind, int(slots), int(exact, 16), pool)
                 for i, sym, name, n, kind, slots, exact, pool in _table("MR_SCENARIO_TABLE")]
SCENARIOS = [""] * (1 + max(r.id for r in SCENARIO_ROWS))  # enum mr_scenario -> tests.rs name
for _r in SCENARIO_ROWS:
    SCENARIOS[_r.id] = _r.name
SCENARIO_ID = {n: i for i, n in enumerate(SCENARIOS) if n}
# tests that still need multi-threaded tester programs (spawn_local); not built yet
UNSUPPORTED = set()
# kvraft generic_test (src/kvraft/tests.rs:65-238), BASELINE config 5
KV_TESTS = [r.name for r in SCENARIO_ROWS if r.kind == "KV"]
# generic_test_linearizability (SEMANTICS §9b): the symbols the header's mr_scn_is_lin15 names
with open(HEADER) as _f:
    _LIN15 = re.findall(r"MR_SCN_(\w+)", re.search(r"mr_scn_is_lin15\(uint32_t s\) \{(.*?)\n\}",
                                                   _f.read(), re.S).group(1))
LIN_TESTS = [r.name for r in SCENARIO_ROWS if r.symbol in _LIN15]
GPU_UNSUPPORTED = set(UNSUPPORTED)

# MR_FAIL_TABLE: verdict code -> symbol without its MR_ / MR_FAIL_ prefix
FAIL_NAMES = {int(code, 0): sym[5:] if sym.startswith("FAIL_") else sym
              for code, sym, *_ in _table("MR_FAIL_TABLE")}

# MR_COUNTER_TABLE: the per-cluster counters in CNT_ order (reduce: SUM / MAX over the batch; who:
# BOTH = the oracle keeps it too, HIP = the HIP path only)
Counter = collections.namedtuple("Counter", "symbol field reduce who")
COUNTER_ROWS = [Counter(*r) for r in _table("MR_COUNTER_TABLE", _COUNTER_ROW)]
# mr_counters fields that are no per-cluster counter but sums over the batch all the same
BATCH_SUMS = ["clusters", "done", "passed", "failed", "events", "msgs_sent", "virt_time_us",
              "kv_ops", "kv_checked", "kv_lin_checked"]


class MrCfg(C.Structure):
    _fields_ = [
        ("abi_version", C.c_uint32), ("scenario", C.c_uint32), ("n_nodes", C.c_uint32),
        ("flags", C.c_uint32), ("seed_base", C.c_uint64), ("cluster_base", C.c_uint64),
        ("n_clusters", C.c_uint64), ("iters", C.c_uint32), ("log_cap", C.c_uint32),
        ("apply_cap", C.c_uint32), ("msg_slots", C.c_uint32), ("ae_max", C.c_uint32),
        ("hb_us", C.c_uint32), ("elect_lo_us", C.c_uint32), ("elect_hi_us", C.c_uint32),
        ("max_events", C.c_uint32), ("trace_clusters", C.c_uint32), ("trace_cap", C.c_uint32),
        ("device", C.c_int32), ("tape_cap", C.c_uint32), ("lanes", C.c_uint32),
        ("lanes_per_wave", C.c_uint32), ("reserved", C.c_uint32 * 3),
    ]


class MrCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in (
        "clusters", "done", "passed", "failed", "events", "ev_msg", "ev_timer", "ev_tester",
        "msgs_sent", "drop_clog", "drop_loss", "drop_overflow", "drop_deliver", "drop_stale",
        "elections", "leaders_elected", "applies", "snapshots", "installs", "entries_shipped",
        "virt_time_us", "max_inflight", "max_log", "max_index", "first_fail_cluster",
        "first_fail_code")] + [("fail_hist", C.c_uint64 * 64), ("cov_leaders", C.c_uint64 * 16),
                               ("cov_events", C.c_uint64 * 16), ("kv_ops", C.c_uint64),
                               ("kv_checked", C.c_uint64), ("log_writes", C.c_uint64),
                               ("entries_materialized", C.c_uint64),
                               ("kv_lin_checked", C.c_uint64),
                               ("coop_entries", C.c_uint64)]  # ABI 4

    def to_dict(self):
        d = {n: getattr(self, n) for n, _ in self._fields_
             if n not in ("fail_hist", "cov_leaders", "cov_events")}
        d["fail_hist"] = {FAIL_NAMES.get(i, str(i)): int(v)
                          for i, v in enumerate(self.fail_hist) if v}
        d["cov_leaders"] = [int(v) for v in self.cov_leaders]
        d["cov_events"] = [int(v) for v in self.cov_events]
        return d


def cov_bucket(v):
    """Coverage-histogram bucket of a per-cluster count (mr_counters.cov_*)."""
    return 0 if v == 0 else min(15, int(v).bit_length())


class MrRunStats(C.Structure):
    _fields_ = [("launches", C.c_uint64), ("kernel_ms", C.c_double), ("wall_ms", C.c_double),
                ("events", C.c_uint64), ("remaining", C.c_uint64)]


EVENT_DTYPE = np.dtype([
    ("time_us", "<u4"), ("cls", "u1"), ("kind", "u1"), ("node", "u1"), ("role", "u1"),
    ("aux", "<u4"), ("term", "<u4"), ("commit", "<u4"), ("applied", "<u4"), ("last", "<u4"),
    ("snap", "<u4"),
])
assert EVENT_DTYPE.itemsize == 32

# keyed decisions (mr_decision, docs/SEMANTICS.md §12)
MR_DS_TESTER, MR_DS_ELECT, MR_DS_NET = 1, 2, 3
DECISION_DTYPE = np.dtype([("cluster", "<u4"), ("stream", "<u2"), ("entity", "<u2"), ("seq", "<u4"),
                           ("w0", "<u4"), ("w1", "<u4")])
assert DECISION_DTYPE.itemsize == 20
LOSS_Q32 = 429496729  # floor(0.1 * 2^32), tester.rs:130
# mr_variant_group (ABI 6): one seed of a grouped variant batch, its slices of base and edits
VARIANT_GROUP_DTYPE = np.dtype([("seed_cluster", "<u4"), ("base_off", "<u4"), ("n_base", "<u4"),
                                ("edit_off", "<u4"), ("n_edits", "<u4")])
assert VARIANT_GROUP_DTYPE.itemsize == 20
# mr_param_group (parameter groups, docs/SEMANTICS.md §12.4): one setting of a sweep; 0 = the batch's
PARAM_GROUP_DTYPE = np.dtype([("flags", "<u4"), ("hb_us", "<u4"), ("elect_lo_us", "<u4"),
                              ("elect_hi_us", "<u4"), ("ae_max", "<u4"), ("iters", "<u4"),
                              ("reserved", "<u4", (2,))])
assert PARAM_GROUP_DTYPE.itemsize == 32
# MR_F_SWEEPABLE: the flag bits a group sets for its positions (they replace the batch's)
SWEEPABLE_FLAGS = (MR_F_UNRELIABLE | MR_F_NULL_RAFT | MR_F_BUG_VOTE_TWICE | MR_F_BUG_VOTE_STALE |
                   MR_F_BUG_NO_PREV_CHECK | MR_F_BUG_NO_DEDUP | MR_F_BUG_STALE_READ |
                   MR_F_BUG_NO_APPLY_CHECK)
# the buggy Raft variants by the names the command line takes (--bug, --sweep bug=)
BUG_FLAGS = {"none": 0, "vote_twice": MR_F_BUG_VOTE_TWICE, "vote_stale": MR_F_BUG_VOTE_STALE,
             "no_prev_check": MR_F_BUG_NO_PREV_CHECK}


def decision_word(v, lo, hi):
    """The smallest draw word w with lo + floor(w * (hi - lo) / 2^32) == v (mr_decision_word)."""
    assert lo <= v < hi
    return ((v - lo) << 32) // (hi - lo) + (1 if ((v - lo) << 32) % (hi - lo) else 0)


def net_decision(dropped, latency_us=1000, unreliable=True):
    """(w0, w1) of a send: dropped (by loss) or delivered after latency_us (tester.rs:127-137)."""
    hi = 27000 if unreliable else 10000
    return (0 if dropped else 0xFFFFFFFF), decision_word(latency_us, 1000, hi)

# symbols the product library exports (include/madraft_sim.h)
EXPORTS = [
    "mr_last_error", "mr_fail_message", "mr_scenario_name", "mr_scenario_from_name",
    "mr_cfg_init", "mr_batch_create", "mr_batch_reset", "mr_batch_run", "mr_batch_verdicts",
    "mr_batch_counters", "mr_trace_get", "mr_batch_destroy", "mr_batch_set_decisions",
    "mr_batch_get_decisions", "mr_decision_word", "mr_replay", "mr_batch_submit", "mr_batch_finish",
    "mr_trace_digests", "mr_trace_applies", "mr_batch_kernel",  # ABI 4
    "mr_batch_set_variants", "mr_batch_set_variant_masks",  # ABI 5
    "mr_batch_set_variant_groups",  # ABI 6
    "mr_batch_set_seeds", "mr_batch_get_decisions_packed",  # ABI 7
    "mr_batch_set_param_groups", "mr_batch_group_counters",  # parameter groups (within ABI 7)
    "mr_batch_fork", "mr_batch_fork_ms",  # fork (within ABI 7)
]
FORK_SKIP = 0xFFFFFFFF  # mr_batch_fork's src_of[c]: position c stays as it is
