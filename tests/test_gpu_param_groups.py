"""GPU: parameter groups (mr_batch_set_param_groups, docs/SEMANTICS.md §12.4). Position c of group g
runs exactly what a batch created from cfg_g runs at that position's seed, so every position is
checked against the oracle's mro_run_cluster(cfg_g, seed), bit for bit, and every group's counters
against the oracle's sums over the group. The oracle's results are computed once per case and shared.

Seeds: 0 .. 8 of the README seed. The guards against a vacuous pass (test_the_fixture_is_not_vacuous)
hold with seed 8 as the ninth, so no other ninth seed was picked."""
import contextlib
import functools
import io
import json

import numpy as np
import pytest

from madraft_amd import _abi
from tests import oracle_lib

pytestmark = pytest.mark.gpu
SEED = _abi.README_SEED
NONE = (1 << 64) - 1
# (test, servers, iters): a pool-family body, one with u64 script arrays, one that restarts servers
CASES = {"fail_agree": ("fail_agree_2b", 3, 0), "count": ("count_2b", 3, 0),
         "figure_8": ("figure_8_unreliable_2c", 5, 20)}
GROUPS = [{}, {"hb_us": 200000}, {"hb_us": 10000}, {"elect_lo_us": 50000, "elect_hi_us": 60000},
          {"ae_max": 1}, {"flags": _abi.MR_F_BUG_VOTE_STALE}, {"flags": _abi.MR_F_BUG_NO_PREV_CHECK},
          {"flags": _abi.MR_F_UNRELIABLE}]
G_NO_PREV, G_UNREL = 6, 7
SEEDS = list(range(9))  # 72 positions: one full wave mixing all eight groups, a partial second one
KV_CASE = ("unreliable_3a", 5, 0)
KV_GROUPS = [{}, {"flags": _abi.MR_F_BUG_NO_DEDUP}, {"hb_us": 200000}]
KV_SEEDS = list(range(4))
MAX_KEYS = {r.field for r in _abi.COUNTER_ROWS if r.reduce == "MAX"}


def cfg_g(hip, case, g, clusters=1, seed=SEED, **kw):
    """The batch's cfg with group g's non-zero numbers and its sweepable flag bits."""
    test, nodes, iters = case
    cfg = hip.make_cfg(test, clusters, seed, nodes=nodes, iters=iters, safety=True, **kw)
    cfg.flags = (cfg.flags & ~_abi.SWEEPABLE_FLAGS) | g.get("flags", 0)
    for k, v in g.items():
        if k != "flags" and v:
            setattr(cfg, k, v)
    return cfg


def positions(n_groups, seeds):
    """Group-minor order: position p is group p % G at seed p // G."""
    return [(p % n_groups, seeds[p // n_groups]) for p in range(n_groups * len(seeds))]


@functools.lru_cache(maxsize=None)
def oracle_runs(case, groups_key, seeds, seed=SEED):
    """mro_run_cluster(cfg_g, seed) of every position, as result dicts, by position."""
    from madraft_amd import sim
    o = oracle_lib.Oracle()
    case_t, groups = (CASES.get(case) or KV_CASE), json.loads(groups_key)
    return [o.run_cluster(cfg_g(sim, case_t, groups[g], seed=seed), k)[0]
            for g, k in positions(len(groups), list(seeds))]


def want_of(case, groups=GROUPS, seeds=SEEDS, seed=SEED):
    return oracle_runs(case, json.dumps(groups), tuple(seeds), seed)


def triple(r):
    return int(r["code"]), int(r["time_us"]), int(r["digest"])


def verdicts(b):
    code, t, dig = b.verdicts()
    return [(int(code[k]), int(t[k]), int(dig[k])) for k in range(b.clusters)]


def run(b):
    assert b.run()["remaining"] == 0
    return verdicts(b)


def sweep_batch(hip, case_t, groups, seeds, seed=SEED, **kw):
    test, nodes, iters = case_t
    b = hip.Batch(test, len(groups) * len(seeds), seed, nodes=nodes, iters=iters, safety=True, **kw)
    pos = positions(len(groups), seeds)
    b.set_seeds([seed + k for _, k in pos])
    b.set_param_groups(groups, [g for g, _ in pos])
    return b


def group_sums(want, n_groups, g):
    """What group_counters(g) must say, from the oracle's per-position results."""
    mine = [(p, r) for p, r in enumerate(want) if p % n_groups == g]
    out = {k: (max if k in MAX_KEYS else sum)(int(r[k]) for _, r in mine) for k in oracle_lib.COUNTER_KEYS}
    out["clusters"] = out["done"] = len(mine)
    out["passed"] = sum(r["code"] == 0 for _, r in mine)
    out["failed"] = len(mine) - out["passed"]
    hist = {}
    for _, r in mine:
        name = _abi.FAIL_NAMES[int(r["code"])]
        hist[name] = hist.get(name, 0) + 1
    out["fail_hist"] = hist
    out["first_fail_cluster"] = next((p for p, r in mine if r["code"] != 0), NONE)
    return out


def assert_group_counters(b, want, n_groups):
    for g in range(n_groups):
        got, exp = b.group_counters(g), group_sums(want, n_groups, g)
        for k, v in exp.items():
            assert got[k] == v, (g, k, got[k], v)


@pytest.fixture(scope="module")
def ran(hip):
    """Per case: (the oracle's per-position results, the sweep batch's verdicts, group_counters of
    every group, counters()), each batch run once."""
    out = {}
    for case, case_t in CASES.items():
        with sweep_batch(hip, case_t, GROUPS, SEEDS) as b:
            kernel = b.kernel
            got = run(b)
            out[case] = (want_of(case), got, [b.group_counters(g) for g in range(len(GROUPS))],
                         b.counters(), kernel)
    return out


def test_the_fixture_is_not_vacuous(hip):
    """On the oracle's results: at least three verdict codes, no simulator limit, and every group but
    no_prev_check and unreliable differs from the inherit group in some seed's digest somewhere in
    the fixture (count_2b, for one, never reaches what vote_stale changes)."""
    codes, differs = set(), set()
    G = len(GROUPS)
    for case in CASES:
        want = want_of(case)
        codes |= {int(r["code"]) for r in want}
        differs |= {g for g in range(G) for s in range(len(SEEDS))
                    if want[s * G + g]["digest"] != want[s * G]["digest"]}
    assert differs >= set(range(1, G)) - {G_NO_PREV, G_UNREL}, differs
    assert len(codes) >= 3, codes
    assert not codes & {60, 61}, codes  # MR_FAIL_SIM_CAPACITY, MR_FAIL_SIM_EVENT_LIMIT


@pytest.mark.parametrize("case", list(CASES))
def test_every_position_equals_the_oracle_under_its_groups_cfg(hip, ran, case):
    want, got, gcnt, _, kernel = ran[case]
    assert kernel == "step_kernel_tape"
    assert len(got) == 72
    for p in range(72):
        assert got[p] == triple(want[p]), (p, p % 8, p // 8, got[p], triple(want[p]))
    for g in range(len(GROUPS)):
        exp = group_sums(want, len(GROUPS), g)
        for k, v in exp.items():
            assert gcnt[g][k] == v, (g, k, gcnt[g][k], v)
    # the inherit group against a plain batch of the same seeds, on whatever kernel that picks
    test, nodes, iters = CASES[case]
    with hip.Batch(test, len(SEEDS), SEED, nodes=nodes, iters=iters, safety=True) as b:
        assert run(b) == got[0::8]


def test_a_service_body(hip):
    want = want_of("kv", KV_GROUPS, KV_SEEDS)
    G = len(KV_GROUPS)
    with sweep_batch(hip, KV_CASE, KV_GROUPS, KV_SEEDS) as b:
        got = run(b)
        for p in range(len(got)):
            assert got[p] == triple(want[p]), (p, got[p], triple(want[p]))
        assert_group_counters(b, want, G)
        for g in range(G):
            gc = b.group_counters(g)
            for k in ("kv_ops", "kv_lin_checked"):
                assert gc[k] == sum(int(want[s * G + g][k]) for s in range(len(KV_SEEDS))), (g, k)
    assert len({triple(want[g])[2] for g in range(G)}) == G  # the three settings are three runs


def merged(rows):
    """counters() of the batch from its groups' rows: sums, maxima for the MAX rows, the first fail."""
    out = {}
    for k, v in rows[0].items():
        if k in ("fail_hist",):
            out[k] = {}
            for r in rows:
                for n, c in r[k].items():
                    out[k][n] = out[k].get(n, 0) + c
        elif k in ("cov_leaders", "cov_events"):
            out[k] = [sum(r[k][i] for r in rows) for i in range(16)]
        elif k == "first_fail_cluster":
            out[k] = min(r[k] for r in rows)
        elif k == "first_fail_code":
            continue
        else:
            out[k] = (max if k in MAX_KEYS else sum)(r[k] for r in rows)
    return out


def assert_merges_to(rows, whole):
    m = merged(rows)
    for k, v in m.items():
        assert whole[k] == v, (k, whole[k], v)
    first = min(rows, key=lambda r: r["first_fail_cluster"])
    assert whole["first_fail_code"] == first["first_fail_code"]


def test_group_rows_merge_to_the_batch_counters(hip, ran):
    for case in CASES:
        _, _, gcnt, whole, _ = ran[case]
        assert_merges_to(gcnt, whole)
        assert sum(g["clusters"] for g in gcnt) == 72


def test_the_grouped_reduce_on_a_skewed_partition(hip):
    """40 groups (more than the reduce keeps in LDS): one with a single position, one with none,
    the last index used, the rest in group 0 and in a group past the LDS rows."""
    n = 40
    of = [0 if p % 3 else 33 for p in range(72)]
    of[0], of[71], of[17] = 5, n - 1, n - 1
    with sweep_batch(hip, CASES["count"], GROUPS, SEEDS) as b:
        run(b)
        whole = b.counters()
        code = b.verdicts()[0]
        b.set_param_groups([{}] * n, of)  # (not run again: the rows of the clusters as they stand)
        rows = [b.group_counters(g) for g in range(n)]
    assert_merges_to(rows, whole)
    assert [g for g in range(n) if rows[g]["clusters"]] == [0, 5, 33, n - 1]
    assert rows[5]["clusters"] == 1 and rows[n - 1]["clusters"] == 2
    assert rows[5]["done"] == 1 and rows[5]["failed"] == int(code[0] != 0)
    assert rows[6]["clusters"] == 0 and rows[6]["first_fail_cluster"] == NONE
    assert all(v == 0 for k, v in rows[6].items() if isinstance(v, int) and k != "first_fail_cluster")
    assert rows[6]["fail_hist"] == {} and not any(rows[6]["cov_events"])
    for g in (0, 33, n - 1):
        mine = [p for p in range(72) if of[p] == g]
        assert rows[g]["failed"] == int((code[mine] != 0).sum())
        bad = [p for p in mine if code[p] != 0]
        assert rows[g]["first_fail_cluster"] == (bad[0] if bad else NONE)


def test_lifetime_and_composition(hip):
    seeds, shift = [0, 1], 3
    G = len(GROUPS)
    want = want_of("count", GROUPS, seeds)
    want_shifted = want_of("count", GROUPS, seeds, SEED + shift)
    with sweep_batch(hip, CASES["count"], GROUPS, seeds) as b:
        assert b.kernel == "step_kernel_tape"
        assert run(b) == [triple(r) for r in want]
        b.reset(SEED + shift)  # the groups (and the list) survive: the same settings at the new base
        assert b.kernel == "step_kernel_tape"
        assert run(b) == [triple(r) for r in want_shifted]
        assert_group_counters(b, want_shifted, G)
        b.set_param_groups(None)  # dropped: the seed list alone, every position the batch's cfg
        b.reset(SEED)
        plain = run(b)
        assert plain == [triple(want[(p // G) * G]) for p in range(len(plain))]
        with pytest.raises(hip.SimError, match="without parameter groups"):
            b.group_counters(0)
    # recording under groups, then the tapes replayed under the same groups: no miss, the same runs
    with sweep_batch(hip, CASES["count"], GROUPS, seeds, flags=_abi.MR_F_RECORD, tape_cap=1 << 15) as b:
        assert run(b) == [triple(r) for r in want]
        drawn, off, rec = b.decisions_all()
        assert int(off[-1]) == int(drawn.sum())  # every draw kept
    with sweep_batch(hip, CASES["count"], GROUPS, seeds) as b:
        b.set_decisions(rec)
        assert b.kernel == "step_kernel_tape"
        assert run(b) == [triple(r) for r in want]
        assert not b.decisions_all()[0].any()
        b.set_decisions(None)  # the groups outlive the tables
        b.reset(SEED)
        assert run(b) == [triple(r) for r in want]


def test_errors_leave_the_batch_as_it_was(hip):
    seeds = [0, 1]
    G = len(GROUPS)
    want = [triple(r) for r in want_of("count", GROUPS, seeds)]
    of = [p % G for p in range(G * len(seeds))]
    bad = [
        (GROUPS, of[:-1] + [G], "no such parameter group"),
        ([{"flags": _abi.MR_F_SAFETY}] + GROUPS[1:], of, "MR_F_SWEEPABLE"),
        ([{"flags": _abi.MR_F_RECORD}] + GROUPS[1:], of, "MR_F_SWEEPABLE"),
        ([{"elect_lo_us": 400000}] + GROUPS[1:], of, "elect_hi_us <= elect_lo_us"),
        ([{"elect_hi_us": 100}] + GROUPS[1:], of, "elect_hi_us <= elect_lo_us"),
        ([{"ae_max": 1 << 20}] + GROUPS[1:], of, "ae_max"),
    ]
    with sweep_batch(hip, CASES["count"], GROUPS, seeds) as b:
        for groups, group_of, msg in bad:
            with pytest.raises(hip.SimError, match=msg):
                b.set_param_groups(groups, group_of)
        g = hip.param_group_records(GROUPS)
        g["reserved"][2][1] = 1
        ofa = np.array(of, np.uint32)
        assert hip.lib().mr_batch_set_param_groups(b._b, g.ctypes.data, g.size, ofa.ctypes.data) != 0
        assert b"reserved" in hip.lib().mr_last_error()
        with pytest.raises(hip.SimError, match="parameter group 8 of 8"):
            b.group_counters(G)
        b.submit(SEED)
        with pytest.raises(hip.SimError, match="submitted"):
            b.set_param_groups(GROUPS, of)
        b.finish()
        assert verdicts(b) == want  # the submitted step ran under the groups set before the errors
        b.reset(SEED)
        assert run(b) == want
    test, nodes, iters = CASES["count"]
    with hip.Batch(test, 4, SEED, nodes=nodes, safety=True) as b:
        with pytest.raises(hip.SimError, match="without parameter groups"):
            b.group_counters(0)
        fresh = b.kernel
        with pytest.raises(hip.SimError):
            b.set_param_groups([{"hb_us": 10000}], [0, 0, 0, 1])
        assert b.kernel == fresh  # a rejected first call sets nothing


def test_run_sweep_and_the_command_line(hip, oracle):
    from madraft_amd import __main__ as cli
    res = hip.run_sweep("count_2b", {"hb_us": [10000, 50000]}, num=8, safety=True)
    assert [r["params"] for r in res] == [{"hb_us": 10000}, {"hb_us": 50000}]
    for r, hb in zip(res, (10000, 50000)):
        cfg = hip.make_cfg("count_2b", 1, SEED, safety=True, hb_us=hb)
        want = [oracle.run_cluster(cfg, k)[0] for k in range(8)]
        assert [int(c) for c in r["codes"]] == [w["code"] for w in want]
        assert [int(d) for d in r["digests"]] == [w["digest"] for w in want]
        assert r["counters"]["failed"] == sum(w["code"] != 0 for w in want)
    out = io.StringIO()
    with contextlib.redirect_stdout(out), pytest.raises(SystemExit) as e:
        cli.main(["count_2b", "--clusters", "8", "--safety", "--sweep", "hb_us=10000,50000"])
    assert e.value.code == 1
    lines = [json.loads(x) for x in out.getvalue().splitlines()]
    assert [x["params"] for x in lines] == [{"hb_us": 10000}, {"hb_us": 50000}]
    assert lines[0]["failed"] == 8 and lines[0]["fail_hist"] == {"RPC_INITIAL": 8}
    assert lines[0]["first_fail_seed"] == SEED
    assert lines[1]["failed"] == 0 and lines[1]["passed"] == 8 and lines[1]["first_fail_seed"] is None
