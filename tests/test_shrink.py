"""CPU: ddmin over fault sets (madraft_amd/shrink.py) on synthetic predicates, and over the
oracle's replay of edited tapes (docs/SEMANTICS.md §12.1): the shrunk set fails with the
recorded verdict and no single fault can be taken from it."""
import numpy as np
import pytest

from madraft_amd import _abi, shrink
from tests import variants_util as vu

N = 87
T = 43


def _predicate(fn):
    calls = []

    def evaluate(keep):
        assert keep.dtype == np.bool_ and keep.shape[1] == N
        assert keep.shape[0] <= shrink.max_candidates(N)
        calls.append(keep.shape[0])
        return np.array([T if fn(set(np.nonzero(k)[0].tolist())) else 0 for k in keep])
    return evaluate, calls


def test_shrink_finds_the_three_faults_that_matter():
    evaluate, calls = _predicate(lambda s: {3, 17, 40} <= s)
    r = shrink.shrink(evaluate, N, T)
    assert r.kept.tolist() == [3, 17, 40]
    assert r.rounds == len(calls) and r.candidates == sum(calls)
    assert calls[0] == 2  # the empty set and the full set come first


def test_shrink_of_a_failure_without_faults_is_empty():
    evaluate, calls = _predicate(lambda s: True)
    r = shrink.shrink(evaluate, N, T)
    assert r.kept.size == 0 and calls == [2]


def test_shrink_needs_a_failing_run():
    evaluate, _ = _predicate(lambda s: False)
    with pytest.raises(ValueError):
        shrink.shrink(evaluate, N, T)


@pytest.mark.parametrize("fn", [
    lambda s: len(s & {1, 2, 3, 4, 5}) % 2 == 1,                  # parity: not monotone
    lambda s: {10, 60} <= s and not (20 in s and 30 not in s),   # a fault that needs another
    lambda s: len(s) >= 80 or {7, 8} <= s,                        # two unrelated causes
])
def test_shrink_is_one_minimal_on_non_monotone_predicates(fn):
    evaluate, _ = _predicate(fn)
    kept = set(shrink.shrink(evaluate, N, T).kept.tolist())
    assert fn(kept) and kept
    for j in kept:
        assert not fn(kept - {j}), j


def test_shrink_is_a_function_of_the_verdicts():
    evaluate, calls = _predicate(lambda s: {3, 17, 40} <= s)
    a = shrink.shrink(evaluate, N, T)
    n = len(calls)
    b = shrink.shrink(evaluate, N, T)
    assert a.kept.tolist() == b.kept.tolist() and calls[:n] == calls[n:]


def test_edit_kinds():
    d = np.array([(0, 3, 1, 0, 5, 7), (0, 3, 1, 1, _abi.LOSS_Q32, 1 << 31),
                  (0, 3, 2, 0, 0xFFFFFFFF, (1 << 31) - 1), (0, 2, 1, 0, 0, 0xFFFFFFFF),
                  (0, 3, 9, 4, 1, 0xFFFFFFFF)], _abi.DECISION_DTYPE)
    idx, e = shrink.find_edits(d, "drop")
    assert idx.tolist() == [0, 4] and e["w0"].tolist() == [0xFFFFFFFF] * 2
    assert e["w1"].tolist() == [7, 0xFFFFFFFF] and e["seq"].tolist() == [0, 4]
    idx, e = shrink.find_edits(d, "delay")
    assert idx.tolist() == [1] and e["w1"].tolist() == [0] and e["w0"].tolist() == [_abi.LOSS_Q32]
    idx, e, kind = shrink.edit_list(d, ("delay", "drop"))
    assert idx.tolist() == [0, 4, 1] and kind.tolist() == ["drop", "drop", "delay"]
    out = shrink.apply_edits(d, idx, e, [True, False, True])
    assert out["w0"].tolist() == [0xFFFFFFFF, _abi.LOSS_Q32, 0xFFFFFFFF, 0, 1]
    assert out["w1"].tolist() == [7, 0, (1 << 31) - 1, 0xFFFFFFFF, 0xFFFFFFFF]


def test_oracle_shrinks_figure_8_to_a_one_minimal_drop_set():
    base, code, _ = vu.recorded("figure_8")
    assert code == 43
    assert shrink.find_edits(base, "drop")[0].size == 87
    p = vu.oracle_passes("figure_8", ("drop",))
    assert p.kind == "drop" and p.faults == 87
    assert 0 < p.kept.size < 87
    vu.assert_one_minimal("figure_8", p)


def test_oracle_many_election_fails_without_drops_then_shrinks_delays():
    base, code, _ = vu.recorded("many_election")
    assert code == 42 and base.size == 50
    assert shrink.find_edits(base, "drop")[0].size == 3
    p = vu.oracle_passes("many_election", ("drop",))
    assert p.kept.size == 0 and p.applied.all()  # latency, not loss
    p = vu.oracle_passes("many_election", ("drop", "delay"))
    assert p.kind == "delay" and p.applied[:3].all()  # every drop delivered
    assert p.faults == shrink.find_edits(base, "delay")[0].size
    vu.assert_one_minimal("many_election", p)


def test_merged_helper_at_seed_0_is_the_cluster_0_fixture():
    """The helpers take a seed index k and run seed k with cluster_base = k. At k = 0 that is
    what they did before they took one: cluster 0 of a config whose cluster_base is left at its
    default, every candidate replayed directly (no memo)."""
    o = vu.oracle()
    test, ckw = vu.FIXTURES["figure_8"]
    cfg = o.cfg(test, **ckw)
    with o.recording(1, vu.CAP) as (count, rec):
        code = int(o.run_batch(cfg, 0, 1)[0][0])
    base = rec[0, : int(count[0])].copy()
    idx, edits, _ = shrink.edit_list(base, ("drop",))

    def evaluate_masks(applied):
        out = []
        for a in applied:
            with o.replaying(shrink.apply_edits(base, idx, edits, a), 1):
                out.append(int(o.run_batch(cfg, 0, 1)[0][0]))
        return np.array(out)

    q = shrink.shrink_passes(evaluate_masks, base, ("drop",), code)
    p = vu.oracle_passes("figure_8", ("drop",), k=0)
    assert np.array_equal(vu.recorded("figure_8", 0)[0], base)
    assert vu.recorded("figure_8", 0)[1] == code == 43
    assert p.faults == q.faults == 87 and p.kind == q.kind == "drop"
    assert np.array_equal(p.kept, q.kept) and np.array_equal(p.applied, q.applied)
    assert (p.rounds, p.candidates) == (q.rounds, q.candidates)
    assert np.array_equal(p.idx, q.idx) and np.array_equal(p.edits, q.edits)
    assert np.array_equal(vu.oracle_passes("figure_8", ("drop",)).kept, p.kept)  # k left out
