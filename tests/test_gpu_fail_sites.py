"""GPU parity where the tester fails: the cases of tests/golden/fail_cases.json (a real Raft,
misconfigured or deliberately buggy, that ends clusters at the reference's panic sites) on the HIP
path against the CPU oracle, bit for bit — verdict code, verdict time and trace digest of every
cluster, the first four clusters record by record up to the failing event, every shared counter —
through the pool kernel and the step kernel, through the reduce kernel, and across a store and a
load. tests/test_fail_sites.py says which verdict codes this reaches and which nothing does."""
import numpy as np
import pytest

from madraft_amd import _abi
from tests.oracle_lib import COUNTER_KEYS
from tests.parity_util import compare, default_kernel, fail_cases, hist_of

pytestmark = pytest.mark.gpu

CASES = {c["name"]: c for c in fail_cases()}
RUNS = [(name, k) for name, c in CASES.items()
        for k in dict.fromkeys([default_kernel(c), "step_kernel"])]


@pytest.mark.parametrize("name,kernel", RUNS, ids=[f"{n}-{k}" for n, k in RUNS])
def test_case_bit_exact(hip, oracle, monkeypatch, name, kernel):
    """Every case GPU == oracle (verdicts, times, digests, four traced clusters with their apply
    digests, counters) on the kernel the library chooses and on the step kernel (MR_POOL=0), the
    verdict histogram equal to the committed one, and every expected code reached."""
    c = CASES[name]
    if kernel != default_kernel(c):
        monkeypatch.setenv("MR_POOL", "0")
    code, _ = compare(hip, oracle, c["test"], c["clusters"], traced=4, first=c["cluster_base"],
                      kernel=kernel, **c["kw"])
    assert hist_of(code) == c["hist"]
    assert np.isin(code[:4], c["expect"]).any()  # a traced cluster failed as the case expects


@pytest.mark.parametrize("name", ["snapshot_install_unreliable_2d+vote_twice",
                                  "fail_no_agree_2b+vote_twice", "basic_4a+all_bugs+elect_40ms"])
def test_reduce_mixed_histogram(hip, name):
    """The reduce kernel over a batch that ends with three or more verdict codes (mr_dev.h
    RED_FAIL_HIST, RED_PASSED, RED_FIRST_FAIL, RED_VTIME), against the batch's own verdict arrays:
    test_reduce_vector_scalars has one code per batch."""
    c = CASES[name]
    assert len(c["hist"]) >= 3
    with hip.Batch(c["test"], c["clusters"], cluster_base=c["cluster_base"], **c["kw"]) as b:
        assert b.run()["remaining"] == 0
        code, t, _ = b.verdicts()
        cnt = b.counters()
    assert hist_of(code) == c["hist"]
    assert cnt["fail_hist"] == {_abi.FAIL_NAMES[int(k)]: n for k, n in c["hist"].items()}
    assert cnt["clusters"] == cnt["done"] == c["clusters"]
    assert cnt["passed"] == int((code == 0).sum()) == c["hist"]["0"]
    assert cnt["failed"] == c["clusters"] - cnt["passed"]
    bad = np.nonzero(code != 0)[0]
    assert cnt["first_fail_cluster"] == c["cluster_base"] + int(bad[0])
    assert cnt["first_fail_code"] == int(code[bad[0]])
    assert cnt["virt_time_us"] == int(t.astype(np.int64).sum())


@pytest.mark.parametrize("name,kernel", [
    ("one_partition_3a+stale_read", "pool_kernel"),                  # the service pool
    ("snapshot_install_unreliable_2d+vote_twice", "pool_kernel"),   # the 3-server Raft pool
])
def test_failing_verdict_in_a_resumed_launch(hip, name, kernel):
    """A cluster that fails after a store at the end of one launch and a load by the next
    (test_resumed_cluster_equals_uninterrupted resumes passing runs only): with a launch budget
    of a fifth of the case's events per seed, the verdicts, times, digests and counters of the
    uninterrupted run, which test_case_bit_exact holds to the oracle's."""
    c = CASES[name]
    args = dict(cluster_base=c["cluster_base"], **c["kw"])
    with hip.Batch(c["test"], c["clusters"], **args) as b:
        assert b.run()["remaining"] == 0 and b.kernel == kernel
        ref, rcnt = b.verdicts(), b.counters()
    assert hist_of(ref[0]) == c["hist"]
    with hip.Batch(c["test"], c["clusters"], **args) as b:
        launches = 0
        while True:
            st = b.run(max_events=max(1, c["events_per_seed"] // 5))
            launches += st["launches"]
            if not st["remaining"]:
                break
        got, cnt = b.verdicts(), b.counters()
        assert b.kernel == kernel
    assert launches >= 2
    for a_, c_ in zip(ref, got):
        assert np.array_equal(a_, c_)
    for k in COUNTER_KEYS:
        assert cnt[k] == rcnt[k], k
    assert cnt["done"] == c["clusters"] and cnt["fail_hist"] == rcnt["fail_hist"]
