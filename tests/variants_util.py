"""Shared by test_shrink.py, test_shrink_many.py, test_gpu_variants.py and
test_gpu_variant_groups.py: the fixtures' configs, the oracle's recording of one seed and its
replay of one edited tape, and ddmin over that replay. Seed k of a fixture (cluster k of the
README seed's batch; k = 0 where none is given) is run with cluster_base = k, so it is the
oracle's row 0: recorded with cluster 0, replayed (mro_set_decisions mode 1, one row) from a tape
whose records say cluster 0. Results are computed once per session."""
import functools

import numpy as np

from madraft_amd import _abi, shrink

CAP = 1 << 15
F = _abi
FIXTURES = {  # name -> (test, cfg keywords): cluster 0 of the README seed fails in each
    "figure_8": ("figure_8_unreliable_2c",
                 dict(flags=F.MR_F_BUG_VOTE_STALE | F.MR_F_SAFETY, iters=100)),
    "many_election": ("many_election_2a",
                      dict(flags=F.MR_F_SAFETY | F.MR_F_BUG_VOTE_TWICE | F.MR_F_UNRELIABLE)),
    "unreliable_3a": ("unreliable_3a", dict(flags=F.MR_F_BUG_NO_DEDUP)),
}
# the many-seed fixture: failing clusters of figure_8's first 20 — many drops and many rounds, a
# failure that is no drop's doing (one round), few drops
NAME = "figure_8"
KINDS = ("drop",)
SEEDS = (0, 3, 13, 15, 19)
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        from tests import oracle_lib
        _oracle = oracle_lib.Oracle()
    return _oracle


def cfg_of(name, k=0, **kw):
    test, ckw = FIXTURES[name]
    return oracle().cfg(test, **ckw, cluster_base=int(k), **kw)


@functools.lru_cache(maxsize=None)
def plain(name, k=0):
    """(code, time, digest) of seed k's own run."""
    code, t, dig, _ = oracle().run_batch(cfg_of(name, k), 0, 1)
    return int(code[0]), int(t[0]), int(dig[0])


@functools.lru_cache(maxsize=None)
def recorded(name, k=0):
    """(base tape of seed k in draw order, verdict code, digest) by the oracle."""
    o = oracle()
    with o.recording(1, CAP) as (count, rec):
        code, _, dig, _ = o.run_batch(cfg_of(name, k), 0, 1)
    assert count[0] <= CAP
    base = rec[0, : int(count[0])].copy()
    base.setflags(write=False)
    return base, int(code[0]), int(dig[0])


def replay(name, tape, k=0, trace_cap=0):
    """The oracle's run of seed k driven by `tape`: (code, time, digest, misses[, trace])."""
    o = oracle()
    cfg = cfg_of(name, k)
    with o.replaying(tape, 1) as miss:
        if trace_cap:
            r, tr = o.run_cluster(cfg, 0, trace_cap=trace_cap)
            return r["code"], r["time_us"], r["digest"], int(miss[0]), tr
        code, t, dig, _ = o.run_batch(cfg, 0, 1)
    return int(code[0]), int(t[0]), int(dig[0]), int(miss[0])


@functools.lru_cache(maxsize=None)
def _variant(name, kinds, k, applied_bytes):
    base = recorded(name, k)[0]
    idx, edits, _ = shrink.edit_list(base, kinds)
    applied = np.frombuffer(applied_bytes, bool)
    return replay(name, shrink.apply_edits(base, idx, edits, applied), k)


def variant(name, kinds, applied, k=0):
    """(code, time, digest, misses) of seed k with the edits of `applied` (columns of
    edit_list(base, kinds)) applied; each distinct variant is replayed once per session."""
    return _variant(name, tuple(kinds), int(k), np.ascontiguousarray(applied, bool).tobytes())


def evaluator(name, kinds, k=0, counts=None):
    """shrink_passes' evaluate_masks for seed k over the oracle: one replay per candidate, each
    distinct candidate replayed once per session (`counts`: a list that gets each call's
    candidates)."""
    def evaluate_masks(applied):
        if counts is not None:
            counts.append(len(applied))
        return np.array([variant(name, kinds, a, k)[0] for a in applied])
    return evaluate_masks


@functools.lru_cache(maxsize=None)
def oracle_passes(name, kinds, k=0):
    """shrink_passes of seed k alone, every candidate replayed by the oracle."""
    base, code, _ = recorded(name, k)
    return shrink.shrink_passes(evaluator(name, kinds, k), base, kinds, code)


def assert_one_minimal(name, p, k=0):
    """The oracle confirms: the minimal run fails with the recorded verdict, and putting any
    one kept fault's edit back gives another verdict (an empty kept set: nothing to remove)."""
    base, code, _ = recorded(name, k)
    assert replay(name, shrink.apply_edits(base, p.idx, p.edits, p.applied), k)[0] == code
    for j in p.kept:
        a = p.applied.copy()
        a[j] = True
        assert replay(name, shrink.apply_edits(base, p.idx, p.edits, a), k)[0] != code, (k, j)
