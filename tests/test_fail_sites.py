"""The tester's failing verdicts (MR_FAIL_TABLE's rows, one per reference panic site) on record:
which a case of tests/golden/fail_cases.json reaches (tests/test_gpu_fail_sites.py then holds the
HIP path to the oracle there, bit for bit), which an older GPU test reaches, and which nothing
reaches yet. A new verdict code fails test_every_verdict_code_is_classified until it is in one of
the three lists."""
import collections
import os
import re

import numpy as np
import pytest

from madraft_amd import _abi, sim
from tests.parity_util import default_kernel, fail_cases, hist_of, pool_family

CASES = fail_cases()
MIN_HITS, THIN_HITS = 8, 2  # tests/golden/make_fail_cases.py

# 1. a case of fail_cases.json expects the code and ends at least MIN_HITS clusters with it
#    (THIN_HITS for the thin codes: a few clusters in a thousand under any configuration tried)
REACHED = [2, 3, 4, 7, 17, 19, 20, 21, 24, 25, 26, 30, 31, 34, 36, 40, 46, 47, 48]
REACHED_THIN = [35, 41]

# 2. an existing GPU test reaches the code: code -> (test file, test)
EXISTING = {
    0: ("test_gpu_parity.py", "test_scenario_bit_exact"),
    1: ("test_gpu_parity.py", "test_null_node_kat"),  # (and count_2b+elect_fixed: a real Raft)
    6: ("test_gpu_parity.py", "test_config2_verdict_histogram"),
    8: ("test_gpu_parity.py", "test_apply_checker_failures_bit_exact"),
    9: ("test_gpu_parity.py", "test_apply_checker_failures_bit_exact"),
    42: ("test_gpu_parity.py", "test_safety_checks_bit_exact"),
    43: ("test_gpu_parity.py", "test_safety_checks_bit_exact"),
    49: ("test_gpu_parity.py", "test_safety_checks_bit_exact"),
    50: ("test_gpu_parity.py", "test_null_service_kat"),
    51: ("test_gpu_parity.py", "test_null_service_kat"),
    52: ("test_gpu_parity.py", "test_linearizability_checker_bit_exact"),
    60: ("test_gpu_parity.py", "test_small_capacities_fail_identically"),
    61: ("test_gpu_parity.py", "test_eight_servers"),
}

# 3. nothing reaches the code on the GPU: code -> why, or what was tried. "the sweeps": the oracle
#    over every supported scenario x one changed field (each MR_F_BUG_* flag and pairs of them with
#    BUG_NO_APPLY_CHECK / UNRELIABLE, hb_us 5 / 20 / 150 / 250 / 400 ms, election timeouts 20-40 ms
#    .. 1.5-3 s and 150000-150001 us, ae_max 1 / 2, 3 / 7 servers, log_cap 16), 48 or 96 seeds a
#    cell
_SWEEPS = "no cluster of the sweeps ended with it"
UNREACHED = {
    5: _SWEEPS,
    10: _SWEEPS,
    11: _SWEEPS,
    12: _SWEEPS,
    13: _SWEEPS,
    14: _SWEEPS,
    15: _SWEEPS,
    16: _SWEEPS,
    18: _SWEEPS,
    22: _SWEEPS,
    23: _SWEEPS,
    27: _SWEEPS,
    28: _SWEEPS,
    29: _SWEEPS,
    32: _SWEEPS,
    33: _SWEEPS,
    37: "5 of the 384 clusters of basic_4a+all_bugs+elect_40ms end with it (equal on the GPU, as "
        "every cluster of a case is), under the 8-cluster minimum",
    38: "1 of the 384 clusters of basic_4a+all_bugs+elect_40ms; 1-3 in 2048 seeds elsewhere",
    39: "1 in 2048 seeds of basic_4a with all Raft bugs, elections of 40-80 ms",
    44: _SWEEPS,
    45: _SWEEPS,
    62: "an interpreter guard (bad op, loop budget): no scenario program trips it",
    0xFFFF: "MR_RUNNING is no final verdict: every parity test runs until nothing remains",
}


def test_every_verdict_code_is_classified():
    """Every row of MR_FAIL_TABLE is in exactly one of the three lists above; list 1 against
    fail_cases.json (expected by a case that ends enough clusters with it), list 2 against the
    named test's file."""
    codes = [int(code, 0) for code, *_ in _abi._table("MR_FAIL_TABLE")]
    listed = REACHED + REACHED_THIN + list(EXISTING) + list(UNREACHED)
    assert sorted(listed) == sorted(codes), (sorted(set(codes) - set(listed)),
                                             [c for c, n in collections.Counter(listed).items()
                                              if n > 1 or c not in codes])
    best = collections.Counter()
    for c in CASES:
        for code in c["expect"]:
            best[code] = max(best[code], c["hist"].get(str(code), 0))
    for code in REACHED:
        assert best[code] >= MIN_HITS, (code, best[code])
    for code in REACHED_THIN:
        assert best[code] >= THIN_HITS, (code, best[code])
    # and nothing a case expects is missing from list 1 (code 1 is list 2's: the null node)
    assert set(best) - {1} == set(REACHED + REACHED_THIN)
    here = os.path.dirname(os.path.abspath(__file__))
    for code, (path, name) in EXISTING.items():
        src = open(os.path.join(here, path)).read()
        assert re.search(rf"^def {name}\(", src, re.M), (code, name)
    for code, why in UNREACHED.items():
        assert why.strip(), code


def test_cases_meet_their_conditions():
    """The conditions tests/golden/make_fail_cases.py checks before it writes, on the file as
    committed: size, event cap, no unexpected SIM_EVENT_LIMIT, histogram over every cluster."""
    assert len({c["name"] for c in CASES}) == len(CASES)
    for c in CASES:
        assert 128 <= c["clusters"] <= 512, c["name"]
        assert c["clusters"] * c["events_per_seed"] <= 2500000, c["name"]
        assert c["kw"]["max_events"] == 200000, c["name"]
        assert sum(c["hist"].values()) == c["clusters"], c["name"]
        assert "61" not in c["hist"] or 61 in c["expect"], c["name"]
        assert c["expect"] and all(c["hist"].get(str(e), 0) > 0 for e in c["expect"]), c["name"]
        assert c["test"] not in _abi.GPU_UNSUPPORTED, c["name"]


def test_cases_run_on_every_pool_family():
    """What the kernel assertion of tests/test_gpu_fail_sites.py test_case_bit_exact then means:
    cases whose default is the pool kernel cover the 5-server and 7-server Raft pools, the kvraft
    and the shard_ctrler pools."""
    on_pool = {pool_family(c) for c in CASES if default_kernel(c) == "pool_kernel"}
    assert {"raft5", "raft7", "kv", "ctrl"} <= on_pool, on_pool


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_oracle_reproduces_case(oracle, case):
    """The oracle against the committed histogram, the events per seed, and the traced clusters:
    one of the first four (those the GPU test compares record by record) fails as expected."""
    cfg = sim.make_cfg(case["test"], case["clusters"], cluster_base=case["cluster_base"],
                       **case["kw"])
    code, _, _, s = oracle.run_batch(cfg, 0, case["clusters"])
    assert hist_of(code) == case["hist"]
    assert s["events"] // case["clusters"] == case["events_per_seed"]
    assert np.isin(code[:4], case["expect"]).any()
