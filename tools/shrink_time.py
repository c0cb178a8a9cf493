"""Wall time of the figure_8 fixture's shrink: `gpu` = shrink_seed on the GPU; `cpu` = ddmin
over the oracle evaluator with each round's candidates spread over the host cores (this mode
never loads the HIP library). `gpu-many` / `cpu-many`: the same for every failing seed among the
fixture's first 64 — a loop of shrink_seed against one shrink_seeds, and ddmin over the oracle
with one seed per host process."""
import json
import multiprocessing as mp
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from madraft_amd import _abi, shrink  # noqa: E402
from tests import variants_util as vu  # noqa: E402

NAME, KINDS = "figure_8", ("drop",)


def _code(tape):
    return vu.replay(NAME, tape)[0]


def gpu():
    test, ckw = vu.FIXTURES[NAME]
    ts = []
    for _ in range(3):
        t0 = time.perf_counter()
        r = shrink.shrink_seed(test, _abi.README_SEED, kinds=KINDS, **ckw)
        ts.append(round(time.perf_counter() - t0, 3))
    print(json.dumps({"mode": "gpu", "fixture": NAME, "faults": r.faults, "kept": int(r.kept.size),
                      "rounds": r.rounds, "candidates": r.candidates, "shrink_seed_s": ts}))


def cpu():
    base, code, _ = vu.recorded(NAME)
    idx, edits, _ = shrink.edit_list(base, KINDS)
    out = {}
    for procs in (1, 16):
        with mp.get_context("fork").Pool(procs) as pool:
            def ev(applied):
                return np.array(pool.map(_code, [shrink.apply_edits(base, idx, edits, a) for a in applied]))
            t0 = time.perf_counter()
            p = shrink.shrink_passes(ev, base, KINDS, code)
            out[procs] = round(time.perf_counter() - t0, 3)
    print(json.dumps({"mode": "cpu", "fixture": NAME, "faults": p.faults, "kept": int(p.kept.size),
                      "rounds": p.rounds, "candidates": p.candidates, "oracle_s_by_procs": out}))


N_SEEDS = 64  # the many-seed workload: every failing seed among the fixture's first N_SEEDS


def gpu_many():
    """(a) a loop of shrink_seed, (b) shrink_seeds, over the failing seeds of the first N_SEEDS."""
    from madraft_amd import sim
    test, ckw = vu.FIXTURES[NAME]
    with sim.Batch(test, N_SEEDS, **ckw) as b:
        b.run()
        failing = [_abi.README_SEED + int(k) for k in np.nonzero(b.verdicts()[0])[0]]
    loop_s, many_s = [], []
    for _ in range(2):
        t0 = time.perf_counter()
        one = [shrink.shrink_seed(test, s, kinds=KINDS, **ckw) for s in failing]
        loop_s.append(round(time.perf_counter() - t0, 3))
        t0 = time.perf_counter()
        res, launches = shrink.shrink_seeds(test, failing, kinds=KINDS, **ckw)
        many_s.append(round(time.perf_counter() - t0, 3))
    assert all(np.array_equal(a.kept, r.kept) and a.rounds == r.rounds for a, r in zip(one, res))
    print(json.dumps({"mode": "gpu-many", "fixture": NAME, "seeds": len(failing),
                      "faults": [r.faults for r in res], "kept": [int(r.kept.size) for r in res],
                      "candidates": sum(r.candidates for r in res),
                      "loop_launches": sum(r.rounds for r in one), "shrink_seed_loop_s": loop_s,
                      "many_launches": launches, "shrink_seeds_s": many_s}))


def _shrink_alone(k):
    base, code, _ = vu.recorded(NAME, k)
    idx, edits, _ = shrink.edit_list(base, KINDS)

    def ev(applied):  # (no memo: every candidate is replayed, as a user's run would)
        return np.array([vu.replay(NAME, shrink.apply_edits(base, idx, edits, a), k)[0] for a in applied])
    p = shrink.shrink_passes(ev, base, KINDS, code)
    return p.faults, int(p.kept.size), p.rounds, p.candidates


def cpu_many():
    """(c) ddmin over the oracle for the same seeds, one seed per worker, on 1 and 16 processes
    (recording included; this mode never loads the HIP library)."""
    code = vu.oracle().run_batch(vu.cfg_of(NAME), 0, N_SEEDS)[0]
    failing = [int(k) for k in np.nonzero(code)[0]]
    out = {}
    for procs in (1, 16):
        with mp.get_context("fork").Pool(procs) as pool:
            t0 = time.perf_counter()
            res = pool.map(_shrink_alone, failing, chunksize=1)
            out[procs] = round(time.perf_counter() - t0, 3)
    print(json.dumps({"mode": "cpu-many", "fixture": NAME, "seeds": len(failing),
                      "faults": [r[0] for r in res], "kept": [r[1] for r in res],
                      "rounds": [r[2] for r in res], "candidates": sum(r[3] for r in res),
                      "oracle_s_by_procs": out}))


if __name__ == "__main__":
    {"gpu": gpu, "cpu": cpu, "gpu-many": gpu_many, "cpu-many": cpu_many}[sys.argv[1]]()
