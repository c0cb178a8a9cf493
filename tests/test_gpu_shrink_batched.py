"""GPU: shrink_seeds as three batches whatever the number of seeds (docs/SEMANTICS.md §12.3) — one
MR_F_RECORD batch over the seed list read back at once, the variant batch, one replay_many — with
the results of the oracle shrinking each seed alone."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from madraft_amd import _abi, shrink, trace
from tests import variants_util as vu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = _abi.README_SEED
TRACE_CAP = 1 << 16
PASSING = 1
KS = tuple(sorted(vu.SEEDS + (PASSING,)))  # 0, 1, 3, 13, 15, 19


def _check(res):
    """`res` = shrink_seeds' results for the seeds KS: the oracle's ddmin of each seed alone."""
    assert len(res) == len(KS)
    for k, r in zip(KS, res):
        if k == PASSING:
            assert r == "passes" and str(SEED + k) in r.error
            continue
        p = vu.oracle_passes(vu.NAME, vu.KINDS, k)
        base, code, _ = vu.recorded(vu.NAME, k)
        assert (r.code, r.kind, r.faults) == (code, p.kind, p.faults), k
        assert (r.rounds, r.candidates) == (p.rounds, p.candidates), k
        assert np.array_equal(r.kept, base[p.idx[p.kept]]), k
        tape = shrink.apply_edits(base, p.idx, p.edits, p.applied)
        assert np.array_equal(r.tape, tape), k
        assert np.array_equal(r.trace, vu.replay(vu.NAME, tape, k, trace_cap=TRACE_CAP)[4]), k


def _counting(hip, monkeypatch):
    made, replays = [], []

    class Counted(hip.Batch):
        def __init__(self, *a, **kw):
            made.append(kw.get("flags", 0))
            super().__init__(*a, **kw)

    def replay(*a, **kw):
        replays.append(a)
        raise AssertionError("shrink_seeds replays in one batch, not seed by seed")

    monkeypatch.setattr(hip, "Batch", Counted)
    monkeypatch.setattr(hip, "replay", replay)
    return made, replays


def test_shrink_seeds_is_three_batches(hip, monkeypatch):
    assert vu.plain(vu.NAME, PASSING)[0] == 0
    test, ckw = vu.FIXTURES[vu.NAME]
    made, replays = _counting(hip, monkeypatch)
    res, launches = shrink.shrink_seeds(test, [SEED + k for k in KS], kinds=vu.KINDS, **ckw)
    assert len(made) == 3 and not replays
    assert [bool(f & _abi.MR_F_RECORD) for f in made] == [True, False, False]
    _check(res)
    assert launches == max(vu.oracle_passes(vu.NAME, vu.KINDS, k).rounds for k in vu.SEEDS)


def test_record_chunks_give_the_same_results(hip, monkeypatch):
    test, ckw = vu.FIXTURES[vu.NAME]
    made, replays = _counting(hip, monkeypatch)
    # 1 MiB of tape per seed: three seeds per record batch; 2 MiB of trace: one seed per replay
    res, launches = shrink.shrink_seeds(test, [SEED + k for k in KS], kinds=vu.KINDS,
                                        record_bytes=3 << 20, **ckw)
    assert [bool(f & _abi.MR_F_RECORD) for f in made] == [True, True] + [False] * (1 + len(vu.SEEDS))
    assert not replays
    _check(res)
    assert launches == max(vu.oracle_passes(vu.NAME, vu.KINDS, k).rounds for k in vu.SEEDS)


@functools.lru_cache(maxsize=None)
def _kept_events(k):
    base = vu.recorded(vu.NAME, k)[0]
    p = vu.oracle_passes(vu.NAME, vu.KINDS, k)
    return trace.events_from_decisions(base[p.idx[p.kept]], unreliable=True, raw=False)


def test_cli_seeds_with_shrink_prints_one_line_per_seed(hip, tmp_path):
    order = (19, 1, 0, 13)  # as given, not sorted
    f = tmp_path / "seeds.txt"
    f.write_text("".join(f"{SEED + k}\n" for k in order))
    args = [sys.executable, "-m", "madraft_amd", "figure_8_unreliable_2c", "--iters", "100",
            "--bug", "vote_stale", "--safety", "--seeds", "@" + str(f)]
    out = subprocess.run(args + ["--shrink"], cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(s) for s in out.stdout.splitlines()]
    assert [j["seed"] - SEED for j in lines] == list(order)
    for k, j in zip(order, lines):
        if k == PASSING:
            assert j == {"seed": SEED + k, "skipped": "passes"}
            continue
        p = vu.oracle_passes(vu.NAME, vu.KINDS, k)
        assert j["code"] == vu.recorded(vu.NAME, k)[1] and j["kind"] == p.kind
        assert (j["faults_before"], j["faults_after"]) == (p.faults, int(p.kept.size))
        assert j["kept"] == json.loads(json.dumps(_kept_events(k))), k
    # without --shrink: the counters line and each failure's own seed
    out = subprocess.run(args, cwd=ROOT, capture_output=True, text=True)
    assert out.returncode == 1, out.stderr
    so = out.stdout.splitlines()
    cnt = json.loads(so[-1])
    assert (cnt["clusters"], cnt["failed"], cnt["first_fail_cluster"]) == (4, 3, 0)
    assert [s for s in so if s.startswith("MADSIM_TEST_SEED=")] == \
        [f"MADSIM_TEST_SEED={SEED + k}" for k in order if k != PASSING]
