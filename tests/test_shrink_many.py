"""CPU: ddmin for several failing seeds in lockstep (madraft_amd/shrink.py shrink_many,
docs/SEMANTICS.md §12.2) over the oracle's replay of edited tapes: each seed gets exactly the
Passes of shrinking it alone, the joint rounds are the longest seed's, and a seed that is done
is given nothing more."""
import numpy as np

from madraft_amd import shrink
from tests import variants_util as vu


def _joint():
    """shrink_many over the oracle evaluators of vu.SEEDS: (passes, calls, the groups of every
    evaluate_groups call, the candidates of every per-seed evaluation)."""
    rounds, counts = [], {g: [] for g in range(len(vu.SEEDS))}
    evals = [vu.evaluator(vu.NAME, vu.KINDS, k, counts[g]) for g, k in enumerate(vu.SEEDS)]

    def evaluate_groups(rows):
        rounds.append(sorted(rows))
        return {g: evals[g](applied) for g, applied in rows.items()}

    bases = [vu.recorded(vu.NAME, k)[0] for k in vu.SEEDS]
    targets = [vu.recorded(vu.NAME, k)[1] for k in vu.SEEDS]
    passes, calls = shrink.shrink_many(evaluate_groups, bases, vu.KINDS, targets)
    return passes, calls, rounds, counts


def test_the_fixture_seeds_fail_and_differ_in_rounds():
    alone = [vu.oracle_passes(vu.NAME, vu.KINDS, k) for k in vu.SEEDS]
    assert all(vu.recorded(vu.NAME, k)[1] != 0 for k in vu.SEEDS)
    assert len({p.rounds for p in alone}) > 2  # long, short and one-round walks side by side
    assert min(p.rounds for p in alone) == 1 and max(p.rounds for p in alone) > 8


def test_shrink_many_gives_each_seed_the_passes_of_shrinking_it_alone():
    passes, calls, rounds, counts = _joint()
    alone = [vu.oracle_passes(vu.NAME, vu.KINDS, k) for k in vu.SEEDS]
    for g, (p, q) in enumerate(zip(passes, alone)):
        assert p.kind == q.kind and p.faults == q.faults, g
        assert np.array_equal(p.kept, q.kept) and np.array_equal(p.applied, q.applied), g
        assert (p.rounds, p.candidates) == (q.rounds, q.candidates), g
        assert np.array_equal(p.idx, q.idx) and np.array_equal(p.edits, q.edits), g
        assert len(counts[g]) == q.rounds and sum(counts[g]) == q.candidates, g
    # one joint call per round of the longest walk
    assert calls == len(rounds) == max(q.rounds for q in alone)


def test_a_finished_seed_is_given_no_further_candidates():
    _, _, rounds, _ = _joint()
    alone = [vu.oracle_passes(vu.NAME, vu.KINDS, k) for k in vu.SEEDS]
    for g, q in enumerate(alone):
        assert [g in r for r in rounds] == [i < q.rounds for i in range(len(rounds))], g
    one_round = [g for g, q in enumerate(alone) if q.rounds == 1]
    assert one_round and all(g not in r for g in one_round for r in rounds[1:])


def test_each_result_is_one_minimal_at_its_own_seed():
    passes = _joint()[0]
    for k, p in zip(vu.SEEDS, passes):
        vu.assert_one_minimal(vu.NAME, p, k)
        assert p.kept.size < p.faults or p.faults == 0


def test_walks_are_resumable_and_drive_is_shrink():
    """The walk yields what shrink() would submit and takes the verdicts from outside."""
    fails = lambda keep: np.array([43 if k[[3, 17]].all() else 0 for k in keep])
    w = shrink.shrink_walk(40, 43)
    keep, sent = next(w), []
    try:
        while True:
            sent.append(keep.shape[0])
            keep = w.send(fails(keep))
    except StopIteration as stop:
        r = stop.value
    calls = []
    q = shrink.shrink(lambda keep: (calls.append(keep.shape[0]), fails(keep))[1], 40, 43)
    assert r.kept.tolist() == q.kept.tolist() == [3, 17]
    assert sent == calls and (r.rounds, r.candidates) == (q.rounds, q.candidates)
