"""Shared by test_shrink_many.py and test_gpu_variant_groups.py: the figure_8 fixture
(variants_util.FIXTURES) at any seed of its batch, by the oracle. Seed k (cluster k of the README
seed's batch) is run with cluster_base = k, so it is the oracle's row 0: recorded with cluster 0,
replayed from a tape whose records say cluster 0. Results are computed once per session."""
import functools

import numpy as np

from madraft_amd import shrink
from tests import variants_util as vu

NAME = "figure_8"
KINDS = ("drop",)
# failing clusters of the fixture's first 20: many drops and many rounds, a failure that is no
# drop's doing (one round), few drops
SEEDS = (0, 3, 13, 15, 19)


def cfg_of(k):
    return vu.cfg_of(NAME, cluster_base=int(k))


@functools.lru_cache(maxsize=None)
def plain(k):
    """(code, time, digest) of seed k's own run."""
    code, t, dig, _ = vu.oracle().run_batch(cfg_of(k), 0, 1)
    return int(code[0]), int(t[0]), int(dig[0])


@functools.lru_cache(maxsize=None)
def recorded(k):
    """(base tape of seed k in draw order, verdict code, digest)."""
    o = vu.oracle()
    with o.recording(1, vu.CAP) as (count, rec):
        code, _, dig, _ = o.run_batch(cfg_of(k), 0, 1)
    assert count[0] <= vu.CAP
    base = rec[0, : int(count[0])].copy()
    base.setflags(write=False)
    return base, int(code[0]), int(dig[0])


def replay(k, tape, trace_cap=0):
    """Seed k driven by `tape`: (code, time, digest, misses[, trace])."""
    o = vu.oracle()
    with o.replaying(tape, 1) as miss:
        if trace_cap:
            r, tr = o.run_cluster(cfg_of(k), 0, trace_cap=trace_cap)
            return r["code"], r["time_us"], r["digest"], int(miss[0]), tr
        code, t, dig, _ = o.run_batch(cfg_of(k), 0, 1)
    return int(code[0]), int(t[0]), int(dig[0]), int(miss[0])


@functools.lru_cache(maxsize=None)
def _variant(k, applied_bytes):
    base = recorded(k)[0]
    idx, edits, _ = shrink.edit_list(base, KINDS)
    applied = np.frombuffer(applied_bytes, bool)
    return replay(k, shrink.apply_edits(base, idx, edits, applied))


def variant(k, applied):
    """(code, time, digest, misses) of seed k with the drop edits of `applied` applied; each
    distinct variant is replayed once per session."""
    return _variant(k, np.ascontiguousarray(applied, bool).tobytes())


def evaluator(k, counts=None):
    """shrink_passes' evaluate_masks for seed k over the oracle: one replay per candidate, each
    distinct candidate replayed once per session (`counts`: a list that gets each call's
    candidates)."""
    def evaluate_masks(applied):
        if counts is not None:
            counts.append(len(applied))
        return np.array([variant(k, a)[0] for a in applied])
    return evaluate_masks


@functools.lru_cache(maxsize=None)
def oracle_passes(k):
    """shrink_passes of seed k alone, every candidate replayed by the oracle."""
    base, code, _ = recorded(k)
    return shrink.shrink_passes(evaluator(k), base, KINDS, code)


def assert_one_minimal(k, p):
    """variants_util.assert_one_minimal's check at seed k: the minimal run fails with the
    recorded verdict, and putting any one kept fault's edit back gives another verdict."""
    base, code, _ = recorded(k)
    assert replay(k, shrink.apply_edits(base, p.idx, p.edits, p.applied))[0] == code
    for j in p.kept:
        a = p.applied.copy()
        a[j] = True
        assert replay(k, shrink.apply_edits(base, p.idx, p.edits, a))[0] != code, (k, j)
