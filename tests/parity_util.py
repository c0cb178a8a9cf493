"""What the GPU parity tests share (tests/test_gpu_parity.py, tests/test_gpu_fail_sites.py): one
batch on the HIP path against the CPU oracle, bit for bit."""
import numpy as np
import pytest

from madraft_amd import _abi
from tests.oracle_lib import COUNTER_KEYS


def first_diff(a, b):
    n = min(len(a), len(b))
    for i in range(n):
        if a[i] != b[i]:
            return i, a[i], b[i]
    return n, (a[n] if n < len(a) else None), (b[n] if n < len(b) else None)


def compare(hip, oracle, test, clusters, traced=4, first=0, oracle_codes=False, kernel=None,
            **kw):
    with hip.Batch(test, clusters, trace_clusters=traced, cluster_base=first, **kw) as b:
        st = b.run()
        assert st["remaining"] == 0
        assert kernel is None or b.kernel == kernel, (test, b.kernel)
        code, t, dig = b.verdicts()
        cnt = b.counters()
        traces = [b.trace(k) for k in range(traced)]
        tdigs = [b.trace_digests(k) for k in range(traced)]
        cfg = b.cfg
    ocode, ot, odig, osum = oracle.run_batch(cfg, 0, clusters)
    for k in range(traced):
        _, otr, odg = oracle.run_cluster_dig(cfg, k, int(cfg.trace_cap))
        if not np.array_equal(traces[k], otr):
            i, g, o = first_diff(traces[k], otr)
            pytest.fail(f"{test} cluster {k}: trace differs at record {i}: gpu={g} oracle={o}")
        if not np.array_equal(tdigs[k], odg):
            i = int(np.nonzero(tdigs[k] != odg)[0][0])
            pytest.fail(f"{test} cluster {k}: apply digest differs at record {i}: {traces[k][i]}")
    bad = np.nonzero((code != ocode) | (t != ot) | (dig != odig))[0]
    assert bad.size == 0, (f"{test}: {bad.size} clusters differ, first {bad[0]}: "
                           f"gpu=({code[bad[0]]},{t[bad[0]]}) oracle=({ocode[bad[0]]},{ot[bad[0]]})")
    for k in COUNTER_KEYS:
        assert cnt[k] == osum[k], (test, k, cnt[k], osum[k])
    assert cnt["done"] == clusters
    return (code, cnt, ocode) if oracle_codes else (code, cnt)


def hist_of(code):
    vals, cnt = np.unique(code, return_counts=True)
    return {str(int(v)): int(n) for v, n in zip(vals, cnt)}


def fail_cases():
    """The cases of tests/golden/fail_cases.json (tests/golden/make_fail_cases.py)."""
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "fail_cases.json")
    return json.load(open(path))["cases"]


ROWS = {r.name: r for r in _abi.SCENARIO_ROWS}


def default_kernel(case):
    """The kernel the library chooses for the case (mr_dev.h has_pool, pool_max_slots): the pool
    kernel where the scenario has a pool family and a kernel instance of exactly that many
    servers, and the message slots fit its key rows."""
    r = ROWS[case["test"]]
    n = case["kw"].get("nodes", r.servers)
    slots = case["kw"].get("msg_slots", 64 if n > 5 else r.slots)
    fits = slots <= (64 if r.pool == "SVC" or n > 5 else 32)
    return "pool_kernel" if r.pool != "NONE" and n < 8 and r.exact >> n & 1 and fits \
        else "step_kernel"


def pool_family(case):
    r = ROWS[case["test"]]
    n = case["kw"].get("nodes", r.servers)
    return {"RAFT": f"raft{n}", "SVC": "ctrl" if r.kind == "CTRL" else "kv"}[r.pool]
