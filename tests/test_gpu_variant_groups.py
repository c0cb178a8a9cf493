"""GPU: variant batches of groups (mr_batch_set_variant_groups, docs/SEMANTICS.md §12.2) — each
group one seed with its own base tape and edits, each cluster a variant of its group's seed.
Every variant must equal the oracle's keyed replay of its edited tape at its group's seed, bit
for bit, and shrink_seeds must walk, for every seed, the ddmin path of the oracle shrinking that
seed alone, in as many launches as the longest walk has rounds."""
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
SEEDS = (0, 3, 15, 19)  # the groups: 87, 62, 7 and 2 drops = 3, 2, 1 and 1 mask words per row
LAYOUTS = {
    # runs of 70 / 40 / 14 / 4 clusters: the group boundaries fall inside waves
    "contiguous": np.repeat(np.arange(4), (70, 40, 14, 4)).astype(np.uint32),
    # every wave holds all four groups
    "interleaved": (np.arange(128) % 4).astype(np.uint32),
}
SEED = _abi.README_SEED


@functools.lru_cache(maxsize=None)
def _group(k):
    """(base, idx, edits) of seed k with every recorded drop as an edit."""
    base = vu.recorded(vu.NAME, k)[0]
    idx, edits = shrink.find_edits(base, "drop")
    return base, idx, edits


@functools.lru_cache(maxsize=None)
def _rows(g):
    """[70, edits of group g] bool, the mask rows of group g's clusters by rank in the group: a
    fixed-seed random row, all applied, the first, middle and last edit alone, none applied,
    then fixed-seed random rows. A group with fewer clusters takes a prefix."""
    n = _group(SEEDS[g])[1].size
    m = np.random.default_rng(5 + g).random((70, n)) < 0.5
    m[1] = True
    for r, j in zip((2, 3, 4), (0, n // 2, n - 1)):
        m[r] = False
        m[r, j] = True
    m[5] = False
    m.setflags(write=False)
    return m


def _applied(group_of):
    """Per cluster: the mask row over its own group's edits."""
    rank = np.zeros(4, int)
    out = []
    for g in group_of:
        out.append(_rows(g)[rank[g]])
        rank[g] += 1
    return out


def _masks(group_of, applied, reverse=False):
    """[clusters, 87] bool from the per-cluster rows (`reverse`: the groups' edits are passed in
    reverse order); the columns past a group's edits are set in odd clusters: nothing reads them."""
    width = max(_group(k)[1].size for k in SEEDS)
    m = np.zeros((len(group_of), width), bool)
    for c, a in enumerate(applied):
        m[c, : a.size] = a[::-1] if reverse else a
        m[c, a.size:] = c & 1
    return m


def _groups(shuffle=False):
    """set_variant_groups' list: (seed_cluster, base, edits) per group (`shuffle`: base in a
    fixed-seed random order, edits reversed)."""
    out = []
    for g, k in enumerate(SEEDS):
        base, _, edits = _group(k)
        if shuffle:
            base, edits = base[np.random.default_rng(g).permutation(base.size)], edits[::-1]
        out.append((k, base, edits))
    return out


def _want(group_of, applied):
    return [vu.variant(vu.NAME, vu.KINDS, a, SEEDS[g]) for g, a in zip(group_of, applied)]


def _batch(hip, clusters, **kw):
    test, ckw = vu.FIXTURES[vu.NAME]
    return hip.Batch(test, clusters, **ckw, **kw)


def _results(b):
    code, t, dig = b.verdicts()
    return [(int(code[k]), int(t[k]), int(dig[k]), b.decisions(k)[0]) for k in range(b.clusters)]


def test_the_groups_share_keys_with_different_words():
    """What makes a lookup in another group's slice visible: most keys of a tape are in the other
    tapes too, with other words."""
    for a in range(4):
        for b in range(a + 1, 4):
            x, y = _group(SEEDS[a])[0], _group(SEEDS[b])[0]
            key = lambda d: {(int(r["stream"]), int(r["entity"]), int(r["seq"])):
                             (int(r["w0"]), int(r["w1"])) for r in d}
            kx, ky = key(x), key(y)
            differ = sum(1 for k in kx if k in ky and kx[k] != ky[k])
            assert differ > min(x.size, y.size) // 2, (a, b, differ)
    assert [(_group(k)[1].size + 31) // 32 for k in SEEDS] == [3, 2, 1, 1]
    assert max(_group(k)[1].size for k in SEEDS) % 32 != 0  # the widest row's last word is partial


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_every_variant_equals_the_oracles_replay_at_its_groups_seed(hip, layout):
    group_of = LAYOUTS[layout]
    applied = _applied(group_of)
    want = _want(group_of, applied)
    traced = 4 if layout == "interleaved" else 0
    kw = dict(trace_clusters=traced, trace_cap=TRACE_CAP) if traced else {}
    with _batch(hip, 128, **kw) as b:
        b.set_variant_groups(_groups(shuffle=True), group_of, _masks(group_of, applied, reverse=True))
        assert b.kernel == "step_kernel_tape"
        assert b.run()["remaining"] == 0
        got = _results(b)
        tr = [b.trace(k) for k in range(traced)]
    for c in range(128):
        assert got[c] == want[c], (c, int(group_of[c]), got[c], want[c])
    assert len({w[2] for w in want}) > 64  # the variants are different runs
    for c in range(traced):  # per-node state after every event, record for record
        k = SEEDS[group_of[c]]
        base, idx, edits = _group(k)
        otr = vu.replay(vu.NAME, shrink.apply_edits(base, idx, edits, applied[c]), k,
                        trace_cap=TRACE_CAP)[4]
        assert np.array_equal(tr[c], otr), c


def test_a_miss_draws_from_the_groups_own_seed(hip):
    """A third of every base tape removed: those draws miss and take the Philox draw of the
    group's seed, which is what was recorded — so every variant of group g is seed g's plain run."""
    groups = []
    for k in SEEDS:
        base = _group(k)[0]
        groups.append((k, base[np.arange(base.size) % 3 != 0], shrink.find_edits(base[1::3], "drop")[1]))
    group_of = LAYOUTS["interleaved"][:64]
    with _batch(hip, 64) as b:
        b.set_variant_groups(groups, group_of)
        b.run()
        got = _results(b)
    for c, r in enumerate(got):
        assert r[:3] == vu.plain(vu.NAME, SEEDS[group_of[c]]), c
        assert r[3] > 0, c
    assert len({vu.plain(vu.NAME, k)[2] for k in SEEDS}) == 4


def test_one_group_equals_set_variants(hip):
    base, _, edits = _group(0)
    masks = np.random.default_rng(9).random((65, edits.size)) < 0.5
    masks[0], masks[1] = False, True
    with _batch(hip, 65) as b:
        b.set_variants(base, edits, masks)
        b.run()
        one = _results(b)
    with _batch(hip, 65) as b:
        b.set_variant_groups([(0, base, edits)], np.zeros(65, np.uint32), masks)
        b.run()
        assert _results(b) == one
    assert len({r[2] for r in one}) > 32


def test_table_life_cycle(hip):
    group_of = LAYOUTS["interleaved"][:32]
    applied = _applied(group_of)
    none = [np.zeros_like(a) for a in applied]
    want, want_none = _want(group_of, applied), _want(group_of, none)
    with _batch(hip, 32) as b:
        assert b.kernel != "step_kernel_tape"
        b.run()
        philox = b.verdicts()
        b.set_variant_groups(_groups(), group_of)  # no cluster applies any edit
        b.reset(SEED)
        b.run()
        assert _results(b) == want_none
        b.set_variant_masks(_masks(group_of, applied))
        b.reset(SEED)
        b.run()
        assert _results(b) == want
        b.reset(SEED)  # the tables survive a reset
        b.run()
        assert _results(b) == want
        b.set_variant_masks(None)
        b.reset(SEED)
        b.run()
        assert _results(b) == want_none
        b.set_variant_groups(_groups(), group_of, _masks(group_of, applied))  # fresh, with masks
        b.reset(SEED)
        b.run()
        assert _results(b) == want
        b.set_variant_groups([], group_of)  # n_groups = 0: Philox again, every cluster its own seed
        assert b.kernel != "step_kernel_tape"
        b.reset(SEED)
        b.run()
        again = b.verdicts()
        assert all(np.array_equal(x, y) for x, y in zip(philox, again))
        assert len(set(again[2].tolist())) > 4
        with pytest.raises(hip.SimError, match="without variants"):
            b.set_variant_masks(None)
        b.set_variant_groups(_groups(), group_of)
        assert b.kernel == "step_kernel_tape"
        b.set_variants(None)  # drops a grouped table too
        assert b.kernel != "step_kernel_tape"
        b.set_variants(_group(0)[0])
        b.set_variant_groups([], group_of)  # ... and n_groups = 0 a one-group table
        assert b.kernel != "step_kernel_tape"
        b.set_decisions(_group(0)[0])
        b.set_variant_groups([], group_of)  # set_decisions tables are not a variant call's to drop
        assert b.kernel == "step_kernel_tape"


def _raw(hip, b, g, base, edits, group_of, n=None, n_edits=None):
    """mr_batch_set_variant_groups with the arrays as given (ranges that the Python wrapper
    cannot produce)."""
    g = np.ascontiguousarray(g, _abi.VARIANT_GROUP_DTYPE)
    base = np.ascontiguousarray(base, _abi.DECISION_DTYPE)
    edits = np.ascontiguousarray(edits, _abi.DECISION_DTYPE)
    of = np.ascontiguousarray(group_of, np.uint32)
    hip._check(hip.lib().mr_batch_set_variant_groups(
        b._b, g.ctypes.data, g.size, base.ctypes.data, base.size if n is None else n,
        edits.ctypes.data, edits.size if n_edits is None else n_edits, of.ctypes.data, None))


def test_rejected_groups_leave_the_previous_tables_working(hip):
    group_of = LAYOUTS["interleaved"][:16]
    applied = _applied(group_of)
    want = _want(group_of, applied)
    good = _groups()
    (k0, base0, edits0), (k1, base1, edits1) = good[0], good[1]

    def with_group0(base=base0, edits=edits0):
        return [(k0, base, edits)] + good[1:]

    def keys(d):
        return {(int(r["stream"]), int(r["entity"]), int(r["seq"])) for r in d}

    # a key of group 1's base that group 0's base lacks, as an edit of group 0
    only1 = sorted(keys(base1) - keys(base0))
    assert only1
    foreign = edits0[:3].copy()
    foreign["stream"][1], foreign["entity"][1], foreign["seq"][1] = only1[0]
    absent = edits0[:3].copy()
    absent["seq"][1] = 0xFFFFFF0
    bad_stream = base0.copy()
    bad_stream["stream"][7] = 4
    bad_edit_stream = edits0[:3].copy()
    bad_edit_stream["stream"][2] = 0
    allbase = np.concatenate([base0, base1])
    alledits = np.concatenate([edits0, edits1])
    two = [(0, 0, base0.size, 0, edits0.size), (3, base0.size, base1.size, edits0.size, edits1.size)]
    of2 = group_of % 2

    def two_with(g, field, value):
        t = np.array(two, _abi.VARIANT_GROUP_DTYPE)
        t[field][g] = value
        return t

    with _batch(hip, 16) as b:
        with pytest.raises(hip.SimError, match="without variants"):
            b.set_variant_masks(None)
        b.set_variant_groups(good, group_of, _masks(group_of, applied))
        for groups, msg in [
                (with_group0(base=np.concatenate([base0, base0[5:6]])), "duplicate decision key"),
                (with_group0(edits=np.concatenate([edits0, edits0[:1]])), "duplicate edit key"),
                (with_group0(edits=foreign), "not in the base tape"),  # only in group 1's base
                (with_group0(edits=absent), "not in the base tape"),
                (with_group0(base=bad_stream), "bad decision stream"),
                (with_group0(edits=bad_edit_stream), "bad decision stream")]:
            with pytest.raises(hip.SimError, match=msg):
                b.set_variant_groups(groups, group_of)
        _raw(hip, b, two, allbase, alledits, of2)  # the raw form itself is accepted ...
        b.set_variant_groups(good, group_of, _masks(group_of, applied))  # ... and replaced again
        for t, of, msg in [
                (two_with(1, "n_base", base1.size + 1), of2, "overruns n"),
                (two_with(1, "base_off", allbase.size), of2, "overruns n"),
                (two_with(1, "n_edits", edits1.size + 1), of2, "overruns n_edits"),
                (two_with(0, "edit_off", alledits.size + 1), of2, "overruns n_edits"),
                (two_with(0, "n_base", 0), of2, "n_base >= 1"),
                (np.array(two, _abi.VARIANT_GROUP_DTYPE), np.where(np.arange(16) == 9, 2, of2),
                 "no such group")]:
            with pytest.raises(hip.SimError, match=msg):
                _raw(hip, b, t, allbase, alledits, of)
        with pytest.raises(hip.SimError, match="2\\^32 - 1"):  # checked before a record is read
            _raw(hip, b, two, allbase, alledits, of2, n=1 << 32)
        with pytest.raises(hip.SimError, match="2\\^32 - 1"):
            _raw(hip, b, two, allbase, alledits, of2, n_edits=1 << 32)
        with pytest.raises(hip.SimError, match="group_of"):
            b.set_variant_groups(good, group_of[:5])
        with pytest.raises(hip.SimError, match="masks"):
            b.set_variant_masks(_masks(group_of, applied)[:, :5])
        assert b.kernel == "step_kernel_tape"
        b.reset(SEED)
        b.run()
        assert _results(b) == want
    test, ckw = vu.FIXTURES[vu.NAME]
    ckw = dict(ckw, flags=ckw["flags"] | _abi.MR_F_RECORD)
    with hip.Batch(test, 2, tape_cap=vu.CAP, **ckw) as b:
        with pytest.raises(hip.SimError, match="MR_F_RECORD"):
            b.set_variant_groups(good, np.zeros(2, np.uint32))
        b.run()  # still records
        n, rec = b.decisions(0, vu.CAP)
        assert n == base0.size and np.array_equal(rec, base0)


def test_shrink_seeds_walks_the_oracles_ddmin_for_every_seed(hip):
    test, ckw = vu.FIXTURES[vu.NAME]
    seeds = [SEED + k for k in vu.SEEDS]
    res, launches = shrink.shrink_seeds(test, seeds, kinds=vu.KINDS, **ckw)
    alone = [vu.oracle_passes(vu.NAME, vu.KINDS, k) for k in vu.SEEDS]
    for k, r, p in zip(vu.SEEDS, res, alone):
        base, code, _ = vu.recorded(vu.NAME, k)
        assert r.code == code and r.kind == p.kind and r.faults == p.faults, k
        assert (r.rounds, r.candidates) == (p.rounds, p.candidates), k
        assert np.array_equal(r.kept, base[p.idx[p.kept]]), k
        tape = shrink.apply_edits(base, p.idx, p.edits, p.applied)
        assert np.array_equal(r.tape, tape), k
        assert np.array_equal(r.trace, vu.replay(vu.NAME, tape, k, trace_cap=TRACE_CAP)[4]), k
    assert launches == max(p.rounds for p in alone)
    assert launches < sum(p.rounds for p in alone)  # one seed at a time: a launch per round each


def test_shrink_seeds_reports_seeds_it_does_not_shrink(hip):
    test, ckw = vu.FIXTURES[vu.NAME]
    assert vu.plain(vu.NAME, 1)[0] == 0 and vu.recorded(vu.NAME, 0)[0].size > 64
    res, launches = shrink.shrink_seeds(test, [SEED, SEED + 1], kinds=vu.KINDS, tape_cap=64, **ckw)
    assert res == ["tape_cap", "passes"] and launches == 0


def test_cli_shrink_failures_prints_what_shrink_prints_per_seed(hip, tmp_path):
    args = [sys.executable, "-m", "madraft_amd", "figure_8_unreliable_2c", "--iters", "100",
            "--bug", "vote_stale", "--safety"]
    out = subprocess.run(args + ["--clusters", "16", "--shrink-failures", "3"], cwd=ROOT,
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    lines = [json.loads(s) for s in out.stdout.splitlines()]
    assert len(lines) == 4
    assert [j["seed"] - SEED for j in lines[:3]] == [0, 3, 4]
    summary = lines[3]
    assert (summary["seeds"], summary["shrunk"]) == (16, 3)
    assert summary["launches"] == max(j["rounds"] for j in lines[:3])
    assert summary["kept_sizes"] == sorted({j["faults_after"] for j in lines[:3]})
    # the same seeds one at a time, then each kept list replayed: processes side by side
    single = [subprocess.Popen(args + ["--seed", str(j["seed"]), "--shrink"], cwd=ROOT,
                               stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
              for j in lines[:3]]
    for j, p in zip(lines[:3], single):
        so, se = p.communicate()
        assert p.returncode == 0, se
        assert json.loads(so.splitlines()[-1]) == j  # (the line carries no timing: every field)
    replays = []
    for j in lines[:3]:
        log = tmp_path / f"kept{j['seed']}.jsonl"
        log.write_text("".join(json.dumps(e) + "\n" for e in j["kept"]))
        replays.append(subprocess.Popen(args + ["--seed", str(j["seed"]), "--replay", str(log)],
                                        cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                                        text=True))
    for p in replays:
        so, se = p.communicate()
        assert p.returncode == 1, se  # a failing verdict
        assert json.loads(so.splitlines()[-1])["code"] == 43
