"""Wall time of the figure_8 fixture's shrink: `gpu` = shrink_seed on the GPU; `cpu` = ddmin
over the oracle evaluator with each round's candidates spread over the host cores (this mode
never loads the HIP library)."""
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


if __name__ == "__main__":
    {"gpu": gpu, "cpu": cpu}[sys.argv[1]]()
