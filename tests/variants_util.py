"""Shared by test_shrink.py and test_gpu_variants.py: the fixtures' configs, the oracle's
recording of cluster 0 and its replay of one edited tape, and ddmin over that replay. A
variant is checked by the oracle's keyed replay (mro_set_decisions mode 1, one row) of the
edited tape, with cluster_base 0 so that row 0 runs the seed. Results are computed once per
session."""
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
_oracle = None


def oracle():
    global _oracle
    if _oracle is None:
        from tests import oracle_lib
        _oracle = oracle_lib.Oracle()
    return _oracle


def cfg_of(name, **kw):
    test, ckw = FIXTURES[name]
    return oracle().cfg(test, **ckw, **kw)


@functools.lru_cache(maxsize=None)
def recorded(name):
    """(base tape of cluster 0 in draw order, verdict code, digest) by the oracle."""
    o = oracle()
    with o.recording(1, CAP) as (count, rec):
        code, _, dig, _ = o.run_batch(cfg_of(name), 0, 1)
    assert count[0] <= CAP
    base = rec[0, : int(count[0])].copy()
    base.setflags(write=False)
    return base, int(code[0]), int(dig[0])


def replay(name, tape, trace_cap=0):
    """The oracle's run of cluster 0 driven by `tape`: (code, time, digest, misses[, trace])."""
    o = oracle()
    cfg = cfg_of(name)
    with o.replaying(tape, 1) as miss:
        if trace_cap:
            r, tr = o.run_cluster(cfg, 0, trace_cap=trace_cap)
            return r["code"], r["time_us"], r["digest"], int(miss[0]), tr
        code, t, dig, _ = o.run_batch(cfg, 0, 1)
    return int(code[0]), int(t[0]), int(dig[0]), int(miss[0])


def evaluator(name, kinds):
    """shrink_passes' evaluate_masks over the oracle: one replay per candidate."""
    base = recorded(name)[0]
    idx, edits, _ = shrink.edit_list(base, kinds)

    def evaluate_masks(applied):
        return np.array([replay(name, shrink.apply_edits(base, idx, edits, a))[0]
                         for a in applied])
    return evaluate_masks


@functools.lru_cache(maxsize=None)
def oracle_passes(name, kinds):
    """shrink_passes with every candidate replayed by the oracle."""
    base, code, _ = recorded(name)
    return shrink.shrink_passes(evaluator(name, kinds), base, kinds, code)


def assert_one_minimal(name, p):
    """The oracle confirms: the minimal run fails with the recorded verdict, and putting any
    one kept fault's edit back gives another verdict (an empty kept set: nothing to remove)."""
    base, code, _ = recorded(name)
    assert replay(name, shrink.apply_edits(base, p.idx, p.edits, p.applied))[0] == code
    for j in p.kept:
        a = p.applied.copy()
        a[j] = True
        assert replay(name, shrink.apply_edits(base, p.idx, p.edits, a))[0] != code, j
