"""CPU: the C-ABI library loads and exports every symbol include/madraft_sim.h
declares; the ctypes mirror matches the C struct layout; host-only entry
points (no GPU needed) behave."""
import ctypes as C
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from madraft_amd import _abi, build, sim
from madraft_amd import dist as mdist
from tests import oracle_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "madraft_sim.h")


@pytest.fixture(scope="module")
def L():
    build.build_hip()
    return sim.lib()


def header_functions():
    txt = open(HEADER).read()
    return sorted(set(re.findall(r"^\s*(?:const\s+)?\w+\**\s+\**(mr_\w+)\s*\(", txt, re.M)))


def test_exports_every_header_symbol(L):
    names = header_functions()
    assert set(names) == set(_abi.EXPORTS), names
    out = subprocess.run(["nm", "-D", "--defined-only", sim.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r" T (mr_\w+)$", out, re.M))
    for n in names:
        assert n in exported, n
        assert hasattr(L, n)


# the key lists as they were typed out before the counter table (include/madraft_sim.h) named them
PINNED_SUM_KEYS = ["clusters", "done", "passed", "failed", "events", "ev_msg", "ev_timer",
                   "ev_tester", "msgs_sent", "drop_clog", "drop_loss", "drop_overflow",
                   "drop_deliver", "drop_stale", "elections", "leaders_elected", "applies",
                   "snapshots", "installs", "entries_shipped", "virt_time_us", "kv_ops",
                   "kv_checked", "log_writes", "entries_materialized", "kv_lin_checked",
                   "coop_entries"]
PINNED_MAX_KEYS = ["max_inflight", "max_log", "max_index"]
PINNED_PARITY_KEYS = ["events", "ev_msg", "ev_timer", "ev_tester", "msgs_sent", "drop_clog",
                      "drop_loss", "drop_overflow", "drop_deliver", "drop_stale", "elections",
                      "leaders_elected", "applies", "snapshots", "installs", "entries_shipped",
                      "max_inflight", "max_log", "max_index", "kv_ops", "kv_checked", "log_writes",
                      "kv_lin_checked"]


def test_struct_layout_matches_c():
    """sizeof / offsetof as the C compiler sees them against the ctypes mirrors, every counter-table
    field of mr_counters and every counter of the oracle's mro_result among them."""
    cnt = [r.field for r in _abi.COUNTER_ROWS]
    assert cnt and set(cnt) <= {n for n, _ in _abi.MrCounters._fields_}
    offs = [f"offsetof(mr_counters, {f})" for f in cnt] + \
           [f"offsetof(mro_result, {f})" for f in oracle_lib.COUNTER_KEYS]
    src = f"""
#include <stdio.h>
#include <stddef.h>
#include "{os.path.join(ROOT, "oracle", "mr_oracle.h")}"
int main(void) {{
  size_t v[] = {{sizeof(mr_cfg), sizeof(mr_counters), sizeof(mr_run_stats), sizeof(mr_event),
                offsetof(mr_cfg, device), offsetof(mr_counters, fail_hist), sizeof(mro_result),
                {", ".join(offs)}}};
  for (size_t i = 0; i < sizeof v / sizeof *v; i++) printf("%zu ", v[i]);
  return 0;
}}"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-o", exe, c], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True,
                                           check=True).stdout.split()))
    assert got == [C.sizeof(_abi.MrCfg), C.sizeof(_abi.MrCounters), C.sizeof(_abi.MrRunStats),
                   _abi.EVENT_DTYPE.itemsize, _abi.MrCfg.device.offset,
                   _abi.MrCounters.fail_hist.offset, C.sizeof(oracle_lib.MroResult)] + \
        [getattr(_abi.MrCounters, f).offset for f in cnt] + \
        [getattr(oracle_lib.MroResult, f).offset for f in oracle_lib.COUNTER_KEYS]


def test_counter_table_names_the_key_lists():
    """The counter table's MAX rows are its tail, and the key lists derived from it (dist.py's
    reductions, the parity tests' comparison) hold exactly the keys they held when typed out."""
    red = [r.reduce for r in _abi.COUNTER_ROWS]
    assert red == sorted(red, reverse=True) and red.count("MAX") == 3  # "SUM" rows, then "MAX"
    assert set(mdist.SUM_KEYS) == set(PINNED_SUM_KEYS) and len(mdist.SUM_KEYS) == len(PINNED_SUM_KEYS)
    assert mdist.MAX_KEYS == PINNED_MAX_KEYS
    assert sorted(oracle_lib.COUNTER_KEYS) == sorted(PINNED_PARITY_KEYS)
    assert {r.field for r in _abi.COUNTER_ROWS if r.who == "HIP"} == \
        {"entries_materialized", "coop_entries"}


def test_scenario_names_roundtrip(L):
    for i, n in enumerate(_abi.SCENARIOS):
        if not n:
            continue
        assert L.mr_scenario_from_name(n.encode()) == i
        assert L.mr_scenario_name(i).decode() == n
    assert L.mr_scenario_from_name(b"no_such_test") == 0


def test_cfg_init_defaults_match_oracle(L, oracle):
    for n in _abi.SCENARIOS:
        if not n:
            continue
        cfg = sim.make_cfg(n)
        ocfg = oracle.cfg(n)
        for f, _ in _abi.MrCfg._fields_:
            if f == "reserved":
                continue
            assert getattr(cfg, f) == getattr(ocfg, f), (n, f)
    assert sim.make_cfg("initial_election_2a").n_nodes == 3   # tests.rs:22
    assert sim.make_cfg("many_election_2a").n_nodes == 7      # tests.rs:82
    assert sim.make_cfg("figure_8_unreliable_2c").n_nodes == 5  # tests.rs:690


def test_fail_messages(L):
    assert sim.fail_message(1) == "expected one leader, got none"      # tester.rs:91
    assert sim.fail_message(7) == "test took longer than 120 seconds"  # tester.rs:356
    assert sim.fail_message(0) == "ok"


def test_bad_config_is_an_error_not_a_crash(L):
    cfg = sim.make_cfg("initial_election_2a")
    cfg.n_nodes = 9
    with pytest.raises(sim.SimError, match="n_nodes"):
        sim.Batch(cfg=cfg)
    cfg = sim.make_cfg("initial_election_2a")
    cfg.log_cap = 1000
    with pytest.raises(sim.SimError, match="log_cap"):
        sim.Batch(cfg=cfg)


def test_fail_table_matches_library(L):
    """Every verdict row of the header has a Python name and a message; other codes have none."""
    body = open(HEADER).read().split("#define MR_FAIL_TABLE(X)", 1)[1].split("enum mr_fail", 1)[0]
    rows = re.findall(r'^\s*X\((0x[0-9A-Fa-f]+|\d+), (\w+), "', body, re.M)
    codes = {int(c, 0) for c, _ in rows}
    assert len(codes) == len(rows) >= 57 and {0, 62, 0xFFFF} <= codes
    assert codes == set(_abi.FAIL_NAMES)
    for c, sym in rows:
        assert _abi.FAIL_NAMES[int(c, 0)] in (sym, sym[len("FAIL_"):])
        assert sim.fail_message(int(c, 0)) not in ("", "unknown"), sym
    assert _abi.FAIL_NAMES[0] == "PASS" and _abi.FAIL_NAMES[0xFFFF] == "RUNNING"
    for c in (set(range(64)) | {0xFFFE, 0x10000, 1 << 31}) - codes:
        assert sim.fail_message(c) == "unknown", c


def test_table_parser_rejects_a_row_it_cannot_read(tmp_path, monkeypatch):
    bad = tmp_path / "bad.h"
    bad.write_text('#define MR_FAIL_TABLE(X) \\\n  X(0, PASS, "ok") \\\n  X(1,FAIL_X, "x")\n')
    monkeypatch.setattr(_abi, "HEADER", str(bad))
    with pytest.raises(ValueError, match="FAIL_X"):
        _abi._table("MR_FAIL_TABLE")
    bad.write_text('#define MR_COUNTER_TABLE(X) \\\n  X(EV_MSG, ev_msg, SUM, BOTH) \\\n'
                   '  X(EV_TIMER, ev_timer, MIN, BOTH)\n')
    with pytest.raises(ValueError, match="EV_TIMER"):
        _abi._table("MR_COUNTER_TABLE", _abi._COUNTER_ROW)


def test_scenario_table_matches_library(L):
    """Every row of the header's scenario table: the library's name, id and default config."""
    assert [r.id for r in _abi.SCENARIO_ROWS] == list(range(1, len(_abi.SCENARIOS)))
    for r in _abi.SCENARIO_ROWS:
        assert L.mr_scenario_name(r.id).decode() == r.name
        assert L.mr_scenario_from_name(r.name.encode()) == r.id
        cfg = _abi.MrCfg()
        assert L.mr_cfg_init(C.byref(cfg), r.id) == 0
        assert (cfg.scenario, cfg.n_nodes, cfg.msg_slots) == (r.id, r.servers, r.slots), r.name
    assert L.mr_scenario_name(len(_abi.SCENARIOS)).decode() == ""
    assert L.mr_cfg_init(C.byref(_abi.MrCfg()), len(_abi.SCENARIOS)) != 0


def test_oracle_reads_the_scenario_and_verdict_tables(oracle):
    """The oracle twin of test_scenario_table_matches_library / test_fail_table_matches_library:
    its names and messages are the header's rows."""
    msg = oracle.L.mro_fail_message
    msg.argtypes, msg.restype = [C.c_uint32], C.c_char_p
    for r in _abi.SCENARIO_ROWS:
        assert oracle.L.mro_scenario_from_name(r.name.encode()) == r.id
    assert oracle.L.mro_scenario_from_name(b"no_such_test") == 0
    rows = _abi._table("MR_FAIL_TABLE")
    assert len(rows) >= 57
    for code, _, text, *_ in rows:
        assert msg(int(code, 0)).decode() == text
    for c in (set(range(64)) | {0xFFFE, 0x10000}) - {int(r[0], 0) for r in rows}:
        assert msg(c) == b"unknown", c


@pytest.mark.parametrize("field,value,message", [
    ("n_nodes", 9, "n_nodes must be 3..8"), ("log_cap", 1000, "log_cap: power of 2 >= 16"),
    ("apply_cap", 8, "apply_cap too small"), ("ae_max", 33, "ae_max must be 1..32"),
    ("msg_slots", 65, "msg_slots must be 1..64 (1..256 for snapshot_recover_many_clients_3b)")])
def test_capacity_checks_are_shared_with_the_oracle(L, oracle, field, value, message):
    """mr_cfg_check_caps: the library refuses the config with the message it always gave, and
    the oracle refuses it too (a raw call: oracle_lib.run_cluster asserts)."""
    cfg = sim.make_cfg("initial_election_2a")
    setattr(cfg, field, value)
    with pytest.raises(sim.SimError, match=re.escape(message)):
        sim.Batch(cfg=cfg)
    assert oracle.L.mro_run_cluster(C.byref(cfg), 0, None, None, 0, None) != 0


def test_oracle_accepts_wide_slots_where_the_library_does(oracle):
    """More than 64 message slots are for snapshot_recover_many_clients_3b alone, on both sides."""
    cfg = oracle.cfg("snapshot_recover_many_clients_3b", msg_slots=65, flags=_abi.MR_F_NULL_RAFT)
    assert oracle.L.mro_run_cluster(C.byref(cfg), 0, None, None, 0, None) == 0


PREDICATES_SRC = """
#include <cstdio>
#include "{dev}"
int main() {{
  for (uint32_t s = 1; s < MR_SCN_COUNT_; s++)
    for (uint32_t n = 3; n <= 8; n++)
      std::printf("%u %u %d %d %u %d %d\\n", s, n, (int)mr::has_exact(s, n), (int)mr::has_pool(s, n),
                  mr_scn_pool(s), mr_scn_wide_slots(s), mr_scn_is_lin15(s));
  return 0;
}}"""


@pytest.fixture(scope="module")
def predicates():
    """mr_dev.h's instance predicates, evaluated by a host program: {(id, n): (has_exact,
    has_pool, pool family, wide slots, lin15)} for every id and n = 3..8."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "p.cpp"), os.path.join(d, "p")
        open(src, "w").write(PREDICATES_SRC.format(dev=os.path.join(ROOT, "madraft_amd", "csrc",
                                                                    "mr_dev.h")))
        subprocess.run(["g++", "-std=c++17", "-D__HIP_PLATFORM_AMD__", "-I", inc, "-o", exe, src],
                       check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    rows = [tuple(map(int, line.split())) for line in out.splitlines()]
    return {(s, n): (bool(e), bool(p), fam, bool(w), bool(lin)) for s, n, e, p, fam, w, lin in rows}


def unit_instances(units):
    """(unit kind, id, NB) of every kernel instance the translation units `units` hold."""
    inst = []
    for src, name, flags in units:
        if not src.endswith(".hip"):
            continue
        d = dict(f[2:].split("=", 1) for f in flags)
        kind = ("tape" if d.get("MR_TAPE") == "1" else
                {None: "step", "1": "pool", "2": "svcpool"}[d.get("MR_POOL")])
        ids = [int(i) for i in re.findall(r"MR_INST\((\d+)\)", d["MR_SCN_LIST"])]
        assert (d["MR_COMMON"] == "1") == (not ids) == (name == "common"), (name, flags)
        inst += [(kind, i, int(d["MR_NB"]), d.get("MR_MW") == "4") for i in ids]
    return inst


@pytest.mark.parametrize("plan", ["full", "guard", "dev"])
def test_build_plan_matches_the_kernels_predicates(predicates, plan):
    """build.py compiles exactly the kernel instances mr_dev.h's has_exact() / has_pool() name,
    which are the ones the host dispatches to: a difference is an undefined symbol when the
    library loads, or a missing kernel at the first launch."""
    scns, tape = {"full": (None, True), "guard": (build.GUARD_SCNS, False),
                  "dev": ([16], True)}[plan]
    ids = list(scns or build.SCN_IDS)
    if plan == "full":
        assert sorted({s for s, _ in predicates}) == ids == list(_abi.SCENARIO_ID.values())
        assert [_abi.SCENARIOS[i] for i in ids if predicates[i, 8][4]] == _abi.LIN_TESTS
    inst = unit_instances(build._units(os.path.join(ROOT, "madraft_amd", "csrc"), scns, tape))
    assert len(set(i[:3] for i in inst)) == len(inst)  # no instance in two units
    for kind, i, nb, wide in inst:
        assert wide == predicates[i, nb][3], (kind, i, nb)  # 256-slot kernels: MR_MW=4 units
    want = {("step", i, 8) for i in ids}
    want |= {("tape", i, 8) for i in ids if tape}
    for i in ids:
        for n in range(3, 9):
            exact, pool, fam = predicates[i, n][:3]
            want |= {("step", i, n)} if exact else set()
            want |= {({1: "pool", 2: "svcpool"}[fam], i, n)} if pool else set()
            assert not pool or exact  # pool instances at exact sizes only
            assert build.has_exact(i, n) == exact and build.has_pool(i, n) == pool
    assert {i[:3] for i in inst} == want


def test_pinned_exact_instances(predicates):
    """The instances the BASELINE configs run on exist: config 2 (fail_agree_2b at 5 servers),
    config 4 (the 2D tests at 7), each scenario's default count; none is "exact" at 8."""
    assert _abi.SCENARIO_ID["fail_agree_2b"] == 5 and predicates[5, 5][0] and build.has_exact(5, 5)
    for t in ("snapshot_basic_2d", "snapshot_install_2d", "snapshot_install_unreliable_2d",
              "snapshot_install_crash_2d", "snapshot_install_unreliable_crash_2d"):
        assert predicates[_abi.SCENARIO_ID[t], 7][0] and build.has_exact(_abi.SCENARIO_ID[t], 7)
    for i in build.SCN_IDS:
        assert build.has_exact(i, build.DEFAULT_N[i]) == (build.DEFAULT_N[i] < 8)
        assert predicates[i, build.DEFAULT_N[i]][0] == (build.DEFAULT_N[i] < 8)
        assert not build.has_exact(i, 8) and not predicates[i, 8][0]


# the batches of tests/golden/dev_layout.json, 64 clusters each: scenario, flags, traced clusters
LAYOUT_CONFIGS = [
    ("initial_election_2a", "0", 0), ("reliable_churn_2c", "0", 0), ("unreliable_agree_2c", "0", 0),
    ("unreliable_3a", "0", 0),
    ("snapshot_unreliable_recover_concurrent_partition_linearizable_3b",
     "MR_F_SAFETY | MR_F_TRACE", 2),
    ("multi_4a", "0", 0)]
LAYOUT_SRC = """
#include <cstdio>
#include "{dev}"
#define MR_ROW_(m, elements, present, reset) #m,
static const char* const names[] = {{MR_DEV_ARRAYS(MR_ROW_)}};
static void one(uint32_t scn, uint32_t flags, uint32_t traced) {{
  mr_cfg c;
  mr_cfg_defaults(&c, scn);
  c.n_clusters = 64; c.flags = flags; c.trace_clusters = traced;
  const mr::DevLayout L = mr::dev_layout(c);
  for (uint32_t a = 0; a < mr::A__N; a++)
    std::printf("%s %lld ", names[a], L.bytes[a] ? (long long)L.off[a] : -1ll);
  std::printf("total %zu reset", L.off[mr::A__N]);
  for (int k = 0; k < (int)mr::A__N; k++)  // mr_batch_reset's walk: the ZERO rows by their place
    for (uint32_t a = 0; a < mr::A__N; a++)
      if (mr::k_dev_reset[a] == k && L.bytes[a]) std::printf(" %s %zu", names[a], L.bytes[a]);
  std::printf("\\n");
}}
int main() {{
{calls}
  return 0;
}}"""


@pytest.mark.parametrize("guard", [False, True], ids=["product", "guard"])
def test_dev_layout_matches_golden(guard):
    """mr_dev.h's array table gives every array of a batch the byte offset (-1: a null pointer) it
    had when mr_batch_create typed the carve out, the same total, and mr_batch_reset the memsets
    it issued then, byte counts and order (MR_GUARD builds: `guard` too), for six batches of 64
    clusters. The expected numbers are a replay of that code."""
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "dev_layout.json")))
    assert list(golden) == [t for t, _, _ in LAYOUT_CONFIGS]
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    calls = "\n".join(f"  one({_abi.SCENARIO_ID[t]}, {flags}, {traced});"
                      for t, flags, traced in LAYOUT_CONFIGS)
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "l.cpp"), os.path.join(d, "l")
        open(src, "w").write(LAYOUT_SRC.format(
            dev=os.path.join(ROOT, "madraft_amd", "csrc", "mr_dev.h"), calls=calls))
        subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                        f"-DMR_GUARD={int(guard)}", "-I", inc, "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout
    lines = out.splitlines()
    assert len(lines) == len(LAYOUT_CONFIGS)
    for (test, _, _), line in zip(LAYOUT_CONFIGS, lines):
        w = line.split()
        t, r = w.index("total"), w.index("reset")
        want = golden[test]
        assert list(zip(w[:t:2], map(int, w[1:t:2]))) == list(want["offsets"].items()), test
        assert int(w[t + 1]) == want["total"], test
        assert [[m, int(b)] for m, b in zip(w[r + 1::2], w[r + 2::2])] == \
            want["reset_guard" if guard else "reset"], test
