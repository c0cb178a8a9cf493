"""GPU: variant batches (mr_batch_set_variants, docs/SEMANTICS.md §12.1) — every cluster a
variant of one seed: a shared base tape, edits, one mask row per cluster, misses drawn from
cluster 0's seed. Every variant must equal the oracle's keyed replay of its edited tape, bit
for bit, and the GPU shrinker must walk the same ddmin path as ddmin over the oracle."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from madraft_amd import _abi, shrink
from tests import variants_util as vu

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TRACE_CAP = 1 << 16


def _masks(n_clusters, n_edits, seed=5):
    """[n_clusters, n_edits] bool: none applied, all applied, the first, middle and last edit
    alone, then fixed-seed random rows."""
    m = np.random.default_rng(seed).random((n_clusters, n_edits)) < 0.5
    m[0] = False
    m[1] = True
    for r, j in zip((2, 3, 4), (0, n_edits // 2, n_edits - 1)):
        if r < n_clusters and n_edits:
            m[r] = False
            m[r, j] = True
    return m


@functools.lru_cache(maxsize=None)
def _reference(name, n_clusters):
    """(base, idx, edits, masks, oracle (code, time, digest, misses) per variant) with every
    recorded drop as an edit; the masks of a smaller batch are a prefix of a larger one's."""
    base = vu.recorded(name)[0]
    idx, edits = shrink.find_edits(base, "drop")
    masks = _masks(65 if name == "figure_8" else n_clusters, idx.size)[:n_clusters]
    want = [vu.replay(name, shrink.apply_edits(base, idx, edits, m)) for m in masks]
    return base, idx, edits, masks, want


def _batch(hip, name, clusters, **kw):
    test, ckw = vu.FIXTURES[name]
    return hip.Batch(test, clusters, **ckw, **kw)


def _results(b):
    code, t, dig = b.verdicts()
    return [(int(code[k]), int(t[k]), int(dig[k]), b.decisions(k)[0]) for k in range(b.clusters)]


@pytest.mark.parametrize("name,clusters,n_edits", [
    ("figure_8", 64, 87), ("figure_8", 65, 87),  # three mask words, the last partial; a partial wave
    ("many_election", 8, 3),                     # 7 servers, 50 decisions
    ("unreliable_3a", 32, None),                 # clerk entities 8 + k, the service state
])
def test_every_variant_equals_the_oracles_replay_of_its_tape(hip, name, clusters, n_edits):
    base, idx, edits, masks, want = _reference(name, clusters if name != "figure_8" else 65)
    masks, want = masks[:clusters], want[:clusters]
    assert n_edits is None or idx.size == n_edits
    if name == "unreliable_3a":
        assert (base["entity"][base["stream"] == _abi.MR_DS_NET] >= 8).any()
    with _batch(hip, name, clusters, trace_clusters=2, trace_cap=TRACE_CAP) as b:
        b.set_variants(base[np.random.default_rng(1).permutation(base.size)], edits[::-1],
                       masks[:, ::-1])  # any order
        assert b.kernel == "step_kernel_tape"
        assert b.run()["remaining"] == 0
        got = _results(b)
        tr = [b.trace(k) for k in range(2)]
    for k in range(clusters):
        assert got[k] == want[k], (k, got[k], want[k])
    assert len({w[2] for w in want}) > 1  # the variants are different runs
    for k in range(2):  # per-node state after every event, record for record
        otr = vu.replay(name, shrink.apply_edits(base, idx, edits, masks[k]), trace_cap=TRACE_CAP)[4]
        assert np.array_equal(tr[k], otr), k


def test_variants_without_edits_are_the_seed_run(hip):
    base, code, dig = vu.recorded("figure_8")
    with _batch(hip, "figure_8", 8) as b:
        b.set_variants(base)
        b.run()
        assert _results(b) == [_results(b)[0]] * 8
        assert all(r[0] == code and r[2] == dig and r[3] == 0 for r in _results(b))


def test_a_miss_draws_from_cluster_0s_seed_in_every_variant(hip):
    """A third of the base tape removed: those draws miss and take the Philox draw of cluster
    0's seed, which is what was recorded — so all 64 variants are the plain run of that seed."""
    base, code, dig = vu.recorded("figure_8")
    with _batch(hip, "figure_8", 1) as b:
        assert b.kernel != "step_kernel_tape"
        b.run()
        plain = b.verdicts()
    assert int(plain[0][0]) == code and int(plain[2][0]) == dig
    with _batch(hip, "figure_8", 64) as b:
        b.set_variants(base[np.arange(base.size) % 3 != 0], shrink.find_edits(base[1::3], "drop")[1])
        b.run()
        got = _results(b)
    assert all(g[0] == code and g[2] == dig and g[1] == int(plain[1][0]) for g in got)
    assert all(g[3] > 0 for g in got)


def test_mask_update_equals_fresh_variants_and_n0_is_philox_again(hip):
    base, idx, edits, masks, want = _reference("figure_8", 65)
    masks, want = masks[:64], want[:64]
    seed = _abi.README_SEED
    with _batch(hip, "figure_8", 64) as b:
        b.run()
        philox = b.verdicts()
        b.set_variants(base, edits)  # no cluster applies any edit
        b.reset(seed)
        b.run()
        assert all(r == want[0] for r in _results(b))
        b.set_variant_masks(masks[::-1])
        b.reset(seed)
        b.run()
        assert _results(b) == want[::-1]
        b.set_variant_masks(masks)
        b.reset(seed)  # the tables survive a reset
        b.run()
        assert _results(b) == want
        b.set_variant_masks(None)
        b.reset(seed)
        b.run()
        assert all(r == want[0] for r in _results(b))
        b.set_variants(None)
        assert b.kernel != "step_kernel_tape"
        b.reset(seed)
        b.run()
        again = b.verdicts()
        assert all(np.array_equal(x, y) for x, y in zip(philox, again))
        assert len(set(again[2].tolist())) > 1  # every cluster its own seed again


def test_rejected_variants_leave_the_previous_tables_working(hip):
    base, idx, edits, masks, want = _reference("figure_8", 65)
    masks, want = masks[:8], want[:8]
    seed = _abi.README_SEED
    dup = np.concatenate([base, base[5:6]])
    absent = edits[:3].copy()
    absent["seq"][1] = 0xFFFFFF0
    bad_stream = base.copy()
    bad_stream["stream"][7] = 4
    bad_edit_stream = edits[:3].copy()
    bad_edit_stream["stream"][2] = 0
    with _batch(hip, "figure_8", 8) as b:
        with pytest.raises(hip.SimError, match="without variants"):
            b.set_variant_masks(None)
        b.set_variants(base, edits, masks)
        for args, msg in [((dup, edits, masks), "duplicate decision key"),
                          ((base, np.concatenate([edits, edits[:1]]), None), "duplicate edit key"),
                          ((base, absent, None), "not in the base tape"),
                          ((bad_stream, edits, masks), "bad decision stream"),
                          ((base, bad_edit_stream, None), "bad decision stream")]:
            with pytest.raises(hip.SimError, match=msg):
                b.set_variants(*args)
        with pytest.raises(hip.SimError, match="masks"):
            b.set_variant_masks(masks[:, :5])
        assert b.kernel == "step_kernel_tape"
        b.reset(seed)
        b.run()
        assert _results(b) == want
        b.set_variants(None)  # n == 0 drops variants only: plain decisions stay in place
        b.set_decisions(base)
        b.set_variants(None)
        assert b.kernel == "step_kernel_tape"
        with pytest.raises(hip.SimError, match="without variants"):
            b.set_variant_masks(None)
    test, ckw = vu.FIXTURES["figure_8"]
    ckw = dict(ckw, flags=ckw["flags"] | _abi.MR_F_RECORD)
    with hip.Batch(test, 2, tape_cap=vu.CAP, **ckw) as b:
        with pytest.raises(hip.SimError, match="MR_F_RECORD"):
            b.set_variants(base, edits)
        b.run()  # still records
        n, rec = b.decisions(0, vu.CAP)
        assert n == base.size and np.array_equal(rec, base)


@pytest.mark.parametrize("name,kinds", [("figure_8", ("drop",)),
                                        ("many_election", ("drop", "delay"))])
def test_shrink_seed_walks_the_oracles_ddmin(hip, name, kinds):
    test, ckw = vu.FIXTURES[name]
    base, code, _ = vu.recorded(name)
    p = vu.oracle_passes(name, kinds)
    r = shrink.shrink_seed(test, _abi.README_SEED, kinds=kinds, **ckw)
    assert r.code == code and r.kind == p.kind and r.faults == p.faults
    assert (r.rounds, r.candidates) == (p.rounds, p.candidates)
    assert np.array_equal(r.kept, base[p.idx[p.kept]])
    assert np.array_equal(r.tape, shrink.apply_edits(base, p.idx, p.edits, p.applied))
    otr = vu.replay(name, r.tape, trace_cap=TRACE_CAP)[4]
    assert np.array_equal(r.trace, otr)


def test_shrink_seed_is_shrink_seeds_of_one_seed(hip):
    test, ckw = vu.FIXTURES["many_election"]
    kinds = ("drop", "delay")
    base = vu.recorded("many_election")[0]
    assert base.size == 50 and shrink.find_edits(base, "drop")[0].size == 3
    one = shrink.shrink_seed(test, _abi.README_SEED, kinds=kinds, **ckw)
    res, launches = shrink.shrink_seeds(test, [_abi.README_SEED], kinds=kinds, **ckw)
    assert len(res) == 1 and isinstance(res[0], shrink.ShrunkSeed)
    for field, x, y in zip(shrink.ShrunkSeed._fields, one, res[0]):
        assert np.array_equal(x, y) if isinstance(x, np.ndarray) else x == y, field
    assert launches == one.rounds  # one launch per ddmin round


def test_shrink_seed_raises_for_a_seed_it_does_not_shrink(hip):
    test, ckw = vu.FIXTURES["figure_8"]
    seed = _abi.README_SEED
    n = vu.recorded("figure_8")[0].size
    assert vu.plain("figure_8", 1)[0] == 0 and n > 64  # by the oracle: seed + 1 passes
    with pytest.raises(hip.SimError, match=f"^seed {seed + 1} passes {test}: nothing to shrink$"):
        shrink.shrink_seed(test, seed + 1, **ckw)
    with pytest.raises(hip.SimError,
                       match=f"^tape_cap 64 too small: the seed draws {n} decisions$"):
        shrink.shrink_seed(test, seed, tape_cap=64, **ckw)


def test_cli_shrink_output_replays_to_the_same_verdict(hip, tmp_path):
    p = vu.oracle_passes("figure_8", ("drop",))
    base = vu.recorded("figure_8")[0]
    args = [sys.executable, "-m", "madraft_amd", "figure_8_unreliable_2c", "--iters", "100",
            "--bug", "vote_stale", "--safety", "--seed", str(_abi.README_SEED)]
    tape = tmp_path / "tape.jsonl"
    out = subprocess.run(args + ["--shrink", "--shrink-tape", str(tape)], cwd=ROOT,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    j = json.loads(out.stdout.splitlines()[-1])
    assert (j["code"], j["verdict"], j["kind"]) == (43, _abi.FAIL_NAMES[43], "drop")
    assert (j["faults_before"], j["faults_after"]) == (87, p.kept.size)
    assert (j["rounds"], j["candidates"]) == (p.rounds, p.candidates)
    kept = base[p.idx[p.kept]]
    assert [(e["host"], e["index"], e["dropped"]) for e in j["kept"]] == \
        [(int(r["entity"]), int(r["seq"]), True) for r in kept]
    log = tmp_path / "kept.jsonl"
    log.write_text("".join(json.dumps(e) + "\n" for e in j["kept"]))
    for path in (log, tape):  # the kept drops alone; the minimal run's whole tape
        rep = subprocess.run(args + ["--replay", str(path)], cwd=ROOT, capture_output=True,
                             text=True)
        assert rep.returncode == 1, rep.stderr  # a failing verdict
        r = json.loads(rep.stdout.splitlines()[-1])
        assert r["code"] == 43
    assert r["events"] == j["events"]  # the tape replays the minimal run itself
