"""GPU: seed lists (mr_batch_set_seeds, docs/SEMANTICS.md §12.3) and the packed tape read-back
(mr_batch_get_decisions_packed). Position c of a batch with a list runs the seed the list names:
its verdict, tape, replay and trace must equal the oracle's run of that seed (seed k of a fixture
is the oracle's row 0 at cluster_base = k, tests/variants_util.py), bit for bit."""
import functools

import numpy as np
import pytest

from madraft_amd import _abi, shrink
from tests import variants_util as vu

pytestmark = pytest.mark.gpu
SEED = _abi.README_SEED
TRACE_CAP = 1 << 16
# 130 positions, two full waves and two lanes: a fixed-seed permutation of range(200) cut to 126, a
# duplicate pair, and two offsets far outside the batch
OFFSETS = [int(o) for o in np.random.default_rng(7).permutation(200)[:126]] + \
    [3, 3, 70000, (1 << 32) - 1]
SHIFT = 7  # the second base: reset(SEED + SHIFT) moves every position's seed by 7
# the record / replay batches: positions = the figure_8 fixture's failing seeds, one of them twice
POS = (19, 0, 3, 3, 15, 13)
SMALL_CAP, SMALL_EVENTS = 64, 40  # tape_cap 64 with 40 events per cluster: 55 .. 70 draws (below)


def _batch(hip, name, clusters, **kw):
    test, ckw = vu.FIXTURES[name]
    ckw = dict(ckw)
    flags = ckw.pop("flags", 0) | kw.pop("flags", 0)
    return hip.Batch(test, clusters, flags=flags, **ckw, **kw)


def _verdicts(b):
    code, t, dig = b.verdicts()
    return [(int(code[k]), int(t[k]), int(dig[k])) for k in range(b.clusters)]


def _run(b):
    assert b.run()["remaining"] == 0
    return _verdicts(b)


def _positional(tape, pos):
    d = np.array(tape, _abi.DECISION_DTYPE)
    d["cluster"] = pos
    return d


@pytest.mark.parametrize("name", ["figure_8", "unreliable_3a"])  # the pool family, the service family
def test_every_position_equals_the_oracles_run_of_its_seed(hip, name):
    assert len(OFFSETS) == 130 and len(set(OFFSETS)) == 129
    want = [vu.plain(name, k) for k in OFFSETS]
    want_shifted = [vu.plain(name, k + SHIFT) for k in OFFSETS]
    assert len({w[2] for w in want}) > 100  # the seeds are different runs
    with _batch(hip, name, 130) as b:
        fresh_kernel = b.kernel
        assert fresh_kernel != "step_kernel_tape"
        b.set_seeds([SEED + k for k in OFFSETS])
        assert b.kernel == "step_kernel_tape"
        got = _run(b)
        for c in range(130):
            assert got[c] == want[c], (c, OFFSETS[c], got[c], want[c])
        cnt = b.counters()  # counters speak of positions: the first failing position, not its seed
        bad = [c for c in range(130) if want[c][0] != 0]
        assert cnt["failed"] == len(bad) and cnt["first_fail_cluster"] == bad[0]
        b.reset(SEED + SHIFT)  # the same list, moved to another base
        assert b.kernel == "step_kernel_tape"
        got = _run(b)
        for c in range(130):
            assert got[c] == want_shifted[c], (c, OFFSETS[c] + SHIFT, got[c], want_shifted[c])
        # a set_decisions round trip keeps the list
        b.set_decisions(_positional(vu.recorded(name, OFFSETS[0])[0][:5], 0))
        b.set_decisions(None)
        assert b.kernel == "step_kernel_tape"
        b.reset(SEED)
        assert _run(b) == want
        # the list dropped: the kernel and the verdicts of a batch that never had one
        b.set_seeds(None)
        assert b.kernel == fresh_kernel
        b.reset(SEED)
        dropped = _run(b)
    with _batch(hip, name, 130) as b:
        assert b.kernel == fresh_kernel
        assert _run(b) == dropped
    assert dropped[:5] == [vu.plain(name, k) for k in range(5)]
    assert dropped != want


def test_a_list_composes_with_lanes_stream_and_submit(hip):
    want = [vu.plain("figure_8", k) for k in OFFSETS]
    seeds = [SEED + k for k in OFFSETS]
    for kw in (dict(lanes=48), dict(lanes=48, stream=True), dict(lanes_per_wave=16)):
        with _batch(hip, "figure_8", 130, **kw) as b:
            b.set_seeds(seeds)
            assert _run(b) == want, kw
    with _batch(hip, "figure_8", 130) as b:
        b.set_seeds(seeds)
        b.submit(SEED)  # the list survives the submitted reset
        st, cnt = b.finish()
        assert st["remaining"] == 0 and cnt["done"] == 130
        assert _verdicts(b) == want


@functools.lru_cache(maxsize=None)
def _small(k):
    """(draws, the first SMALL_CAP records) of seed k stopped after SMALL_EVENTS events, by the
    oracle."""
    o = vu.oracle()
    with o.recording(1, 4096) as (count, rec):
        o.run_batch(vu.cfg_of("figure_8", k, max_events=SMALL_EVENTS), 0, 1)
    return int(count[0]), rec[0, : min(int(count[0]), SMALL_CAP)].copy()


def test_recording_a_list_gives_each_seeds_tape(hip):
    seeds = [SEED + k for k in POS]
    with _batch(hip, "figure_8", len(POS), flags=_abi.MR_F_RECORD, tape_cap=vu.CAP) as b:
        assert b.kernel == "step_kernel_tape"
        b.set_seeds(seeds)
        _run(b)
        drawn, off, rec = b.decisions_all()
        assert off[0] == 0 and off[-1] == rec.size
        for c, k in enumerate(POS):
            base = vu.recorded("figure_8", k)[0]
            mine = rec[int(off[c]): int(off[c + 1])]
            assert int(drawn[c]) == base.size == mine.size, (c, k)
            assert np.array_equal(mine, _positional(base, c)), (c, k)
            n, one = b.decisions(c, vu.CAP)  # the per-cluster call gives the same
            assert n == base.size and np.array_equal(one, mine), (c, k)
        d2, o2, r2 = b.decisions_all(first=2, count=3)  # a slice: first > 0, not the whole batch
        assert np.array_equal(d2, drawn[2:5]) and np.array_equal(o2, off[2:6] - off[2])
        assert np.array_equal(r2, rec[int(off[2]): int(off[5])])
        d0, o0, r0 = b.decisions_all(first=len(POS), count=0)
        assert d0.size == 0 and o0.tolist() == [0] and r0.size == 0
        with pytest.raises(hip.SimError, match="out of range"):
            b.decisions_all(first=4, count=3)


def test_packed_tapes_at_a_small_tape_cap(hip):
    """tape_cap 64: clusters that drew more keep exactly 64 records and report what they drew, the
    short ones beside them keep all of theirs, and the offsets say which is which."""
    counts = [_small(k)[0] for k in POS]
    assert max(counts) > SMALL_CAP > min(counts) and SMALL_CAP in counts, counts
    kept = [min(n, SMALL_CAP) for n in counts]
    with _batch(hip, "figure_8", len(POS), flags=_abi.MR_F_RECORD, tape_cap=SMALL_CAP,
                max_events=SMALL_EVENTS) as b:
        b.set_seeds([SEED + k for k in POS])
        _run(b)
        drawn, off, rec = b.decisions_all()
        assert drawn.tolist() == counts
        assert off.tolist() == np.concatenate([[0], np.cumsum(kept)]).tolist()
        for c, k in enumerate(POS):
            mine = rec[int(off[c]): int(off[c + 1])]
            n, one = b.decisions(c, SMALL_CAP)
            assert n == counts[c] and np.array_equal(one, mine), (c, k)
            assert np.array_equal(mine, _positional(_small(k)[1], c)), (c, k)
        d2, o2, r2 = b.decisions_all(first=1, count=4)
        assert d2.tolist() == counts[1:5] and o2.tolist() == (off[1:6] - off[1]).tolist()
        assert np.array_equal(r2, rec[int(off[1]): int(off[5])])
        # an out too small: an error, and no record of it written
        total = int(off[-1])
        out = np.zeros(total, _abi.DECISION_DTYPE)
        out["seq"] = 0xABCDEF01
        sentinel = out.copy()
        d3, o3 = np.zeros(len(POS), np.uint64), np.zeros(len(POS) + 1, np.uint64)
        rc = hip.lib().mr_batch_get_decisions_packed(b._b, 0, len(POS), d3.ctypes.data,
                                                     o3.ctypes.data, out.ctypes.data, total - 1)
        assert rc != 0 and "are kept" in hip.lib().mr_last_error().decode()
        assert np.array_equal(out, sentinel)
        assert d3.tolist() == counts and o3.tolist() == off.tolist()  # (the sizes are still told)
        rc = hip.lib().mr_batch_get_decisions_packed(b._b, 0, len(POS), None, o3.ctypes.data,
                                                     out.ctypes.data, total)  # drawn is optional
        assert rc == 0 and np.array_equal(out, rec)


def _one(hip, b, k, cap):
    """mr_batch_get_decisions of position k into a marked buffer of cap + 2 records (cap None: a
    NULL out): (n, the buffer's records that were written)."""
    n = _abi.C.c_size_t()
    if cap is None:
        assert hip.lib().mr_batch_get_decisions(b._b, k, None, 0, _abi.C.byref(n)) == 0
        return int(n.value), np.zeros(0, _abi.DECISION_DTYPE)
    out = np.zeros(cap + 2, _abi.DECISION_DTYPE)
    out["seq"], out["cluster"] = 0xABCDEF01, 0xFFFFFFFF
    assert hip.lib().mr_batch_get_decisions(b._b, k, out.ctypes.data, cap, _abi.C.byref(n)) == 0
    written = np.nonzero(out["cluster"] != 0xFFFFFFFF)[0]
    assert written.tolist() == list(range(written.size))  # a prefix, and nothing past it
    return int(n.value), out[: written.size]


def test_one_position_read_back_is_the_packed_ones_row(hip):
    """mr_batch_get_decisions is the packed read-back of one position: at a tape_cap below, at and
    above what the three positions drew (56, 70, 64 against 64), for a NULL out and caps around
    tape_cap, n is all the position drew and the records are decisions_all()'s row cut to the
    cap. With decisions set n is the misses, and no record comes back."""
    pos = POS[:3]
    counts = [_small(k)[0] for k in pos]
    assert counts[0] < SMALL_CAP < counts[1] and counts[2] == SMALL_CAP, counts
    with _batch(hip, "figure_8", 3, flags=_abi.MR_F_RECORD, tape_cap=SMALL_CAP,
                max_events=SMALL_EVENTS) as b:
        b.set_seeds([SEED + k for k in pos])
        _run(b)
        drawn, off, rec = b.decisions_all()
        assert drawn.tolist() == counts
        for c in range(3):
            row = rec[int(off[c]): int(off[c + 1])]
            assert row.size == min(counts[c], SMALL_CAP)
            for cap in (None, 1, SMALL_CAP - 1, SMALL_CAP, SMALL_CAP + 3):
                n, got = _one(hip, b, c, cap)
                assert n == counts[c], (c, cap)
                assert np.array_equal(got, row[: min(cap or 0, SMALL_CAP)]), (c, cap)
    tapes = [_halved(k, c) for c, k in enumerate(pos)]
    with _batch(hip, "figure_8", 3) as b:
        b.set_seeds([SEED + k for k in pos])
        b.set_decisions(np.concatenate(tapes))
        _run(b)
        misses = b.decisions_all()[0]
        assert all(int(m) > 0 for m in misses)
        for c in range(3):
            for cap in (None, 1, SMALL_CAP + 3):
                n, got = _one(hip, b, c, cap)
                assert n == int(misses[c]) and got.size == 0, (c, cap)


def _halved(k, pos):
    """Seed k's recorded tape with every second record removed, for position pos."""
    return _positional(vu.recorded("figure_8", k)[0][::2], pos)


def test_replay_misses_draw_from_the_positions_seed(hip):
    tapes = [_halved(k, c) for c, k in enumerate(POS)]
    want = [vu.replay("figure_8", _positional(t, 0), k) for t, k in zip(tapes, POS)]
    assert all(w[3] > 0 for w in want)
    with _batch(hip, "figure_8", len(POS)) as b:
        b.set_seeds([SEED + k for k in POS])
        b.set_decisions(np.concatenate(tapes))
        got = _run(b)
        misses = b.decisions_all()
        assert misses[1].tolist() == [0] * (len(POS) + 1) and misses[2].size == 0
        for c, k in enumerate(POS):
            assert got[c] + (int(misses[0][c]),) == want[c], (c, k)
            assert b.decisions(c)[0] == want[c][3]
    # every miss drew what the seed's own run drew there: the halved tape replays to the plain run
    assert [w[:3] for w in want] == [vu.plain("figure_8", k) for k in POS]


def test_replay_many_equals_replay_per_seed(hip):
    test, ckw = vu.FIXTURES["figure_8"]
    tapes = [_halved(k, 0) for k in POS]
    tapes[1] = tapes[1][:0]  # an empty tape: every draw a miss
    tapes[4] = vu.recorded("figure_8", POS[4])[0]  # a whole one: no miss
    seeds = [SEED + k for k in POS]
    many = hip.replay_many(test, tapes, seeds, trace_cap=TRACE_CAP, **ckw)
    assert len(many) == len(POS)
    for c, k in enumerate(POS):
        one = hip.replay(test, tapes[c], trace_cap=TRACE_CAP, seed=seeds[c], **ckw)
        assert many[c][1:] == one[1:], (c, k)
        assert np.array_equal(many[c][0], one[0]), (c, k)
        assert many[c][1:3] == vu.plain("figure_8", k)[:2]
    assert many[4][3] == 0 and many[1][3] == vu.recorded("figure_8", POS[1])[0].size
    otr = vu.replay("figure_8", tapes[0], POS[0], trace_cap=TRACE_CAP)[4]
    assert np.array_equal(many[0][0], otr)
    assert hip.replay_many(test, [], [], **ckw) == []


N_MIX = 70  # one full wave and six lanes


@functools.lru_cache(maxsize=None)
def _mix_recorded():
    """The oracle's recording of seeds 0 .. N_MIX - 1 stopped after SMALL_EVENTS events: their
    tapes in draw order and their plain verdicts."""
    o = vu.oracle()
    with o.recording(N_MIX, 4096) as (count, rec):
        code, t, dig, _ = o.run_batch(vu.cfg_of("figure_8", 0, max_events=SMALL_EVENTS), 0, N_MIX)
    assert 2 <= int(count.min()) and int(count.max()) <= 4096
    tapes = [rec[k, : int(count[k])].copy() for k in range(N_MIX)]
    return tapes, [(int(code[k]), int(t[k]), int(dig[k])) for k in range(N_MIX)]


def _mix_cut(tape, c):
    """What position c is given of `tape`, by c % 4: all of it, nothing, every second record, its
    first record only. (The last position, 69, is an empty one: the table's last row is empty.)"""
    return (tape, tape[:0], tape[::2], tape[:1])[c % 4]


def _mix_load(cut):
    """The positions' tapes, each naming its position, concatenated in a shuffled order."""
    order = np.random.default_rng(11).permutation(N_MIX)
    return np.concatenate([_positional(cut[c], c) for c in order])


def _mix_check(b, want, whole_of):
    """The batch's run equals `want` [(code, time, digest, misses)] at every position; a whole tape
    misses nothing, an empty one misses every draw of its seed's recorded run and ends as it did."""
    tapes, plain = _mix_recorded()
    got = _run(b)
    drawn, off, rec = b.decisions_all()
    assert off.tolist() == [0] * (N_MIX + 1) and rec.size == 0
    for c in range(N_MIX):
        assert got[c] + (int(drawn[c]),) == want[c], (c, got[c], int(drawn[c]), want[c])
        assert b.decisions(c)[0] == want[c][3], c
        k = whole_of(c)
        if c % 4 == 0:
            assert int(drawn[c]) == 0 and got[c] == plain[k], (c, k)
        if c % 4 == 1:
            assert int(drawn[c]) == tapes[k].size and got[c] == plain[k], (c, k)


def test_empty_and_short_rows_beside_long_ones_in_one_wave(hip):
    """One lookup serves every slice length a wave can hold at once: 70 positions (a full wave and
    a partial one) whose tapes are whole (47 .. 118 records), empty, halved or one record long, the
    last row empty, loaded by one set_decisions call in a shuffled order. The oracle's replay
    expresses an empty row (every draw of that row misses), so every expected value is its own.
    Then the same shapes under a permuted seed list: position c replays a cut of the tape of the
    seed the list names, and its misses draw from that seed."""
    tapes, plain = _mix_recorded()
    o = vu.oracle()
    cut = [_mix_cut(tapes[c], c) for c in range(N_MIX)]
    assert cut[N_MIX - 1].size == 0 and cut[0].size == tapes[0].size and cut[3].size == 1
    with o.replaying(np.concatenate([_positional(cut[c], c) for c in range(N_MIX)]), N_MIX) as miss:
        code, t, dig, _ = o.run_batch(vu.cfg_of("figure_8", 0, max_events=SMALL_EVENTS), 0, N_MIX)
        want = [(int(code[c]), int(t[c]), int(dig[c]), int(miss[c])) for c in range(N_MIX)]
    perm = [int(k) for k in np.random.default_rng(13).permutation(N_MIX)]
    assert perm != sorted(perm)
    cut2 = [_mix_cut(tapes[k], c) for c, k in enumerate(perm)]
    want2 = []
    for c, k in enumerate(perm):  # seed k alone, as the oracle's row 0 (tests/variants_util.py)
        with o.replaying(_positional(cut2[c], 0), 1) as miss:
            code, t, dig, _ = o.run_batch(vu.cfg_of("figure_8", k, max_events=SMALL_EVENTS), 0, 1)
            want2.append((int(code[0]), int(t[0]), int(dig[0]), int(miss[0])))
    with _batch(hip, "figure_8", N_MIX, max_events=SMALL_EVENTS) as b:
        b.set_decisions(_mix_load(cut))
        assert b.kernel == "step_kernel_tape"
        _mix_check(b, want, lambda c: c)
        b.reset(SEED)
        b.set_seeds([SEED + k for k in perm])
        b.set_decisions(_mix_load(cut2))
        _mix_check(b, want2, lambda c: perm[c])


def test_rejected_calls_leave_the_batch_as_it_was(hip):
    base = vu.recorded("figure_8", 0)[0]
    idx, edits = shrink.find_edits(base, "drop")
    masks = np.zeros((4, edits.size), bool)
    masks[1], masks[2, ::2] = True, True
    want_variants = [vu.variant("figure_8", ("drop",), m, 0) for m in masks]
    with _batch(hip, "figure_8", 4) as b:  # a list on a variant batch
        b.set_variants(base, edits, masks)
        with pytest.raises(hip.SimError, match="variants"):
            b.set_seeds([SEED + 3, SEED, SEED + 19, SEED + 3])
        got = _run(b)
        assert [g + (b.decisions(c)[0],) for c, g in enumerate(got)] == want_variants
        b.set_seeds(None)  # nothing to drop: no error, the variants stay
        assert b.kernel == "step_kernel_tape"
    seeds = [SEED + k for k in POS[:4]]
    want = [vu.plain("figure_8", k) for k in POS[:4]]
    with _batch(hip, "figure_8", 4) as b:  # variants on a listed batch
        b.set_seeds(seeds)
        with pytest.raises(hip.SimError, match="seed list"):
            b.set_variants(base, edits, masks)
        with pytest.raises(hip.SimError, match="seed list"):
            b.set_variant_groups([(0, base, edits)], np.zeros(4, np.uint32), masks)
        b.set_variants(None)  # dropping variants that are not there is no error
        with pytest.raises(hip.SimError, match="2\\^32"):  # a seed below the base
            b.set_seeds([SEED - 1] + seeds[1:])
        with pytest.raises(hip.SimError, match="shape"):
            b.set_seeds(seeds[:3])
        assert b.kernel == "step_kernel_tape"
        assert _run(b) == want
    L = hip.lib()  # a NULL batch
    off = np.zeros(2, np.uint64)
    assert L.mr_batch_set_seeds(None, None) != 0 and "null batch" in L.mr_last_error().decode()
    assert L.mr_batch_get_decisions_packed(None, 0, 1, None, off.ctypes.data, None, 0) != 0
    assert "null" in L.mr_last_error().decode()


def test_run_seeds_reports_each_failure_with_its_own_seed(hip, capsys):
    test, ckw = vu.FIXTURES["figure_8"]
    seeds = [SEED + k for k in (1, 19, 2, 3)]
    code, t, dig, cnt = hip.run_seeds(test, seeds, **ckw)
    want = [vu.plain("figure_8", k) for k in (1, 19, 2, 3)]
    assert [(int(c), int(x), int(d)) for c, x, d in zip(code, t, dig)] == want
    assert cnt["clusters"] == 4 and cnt["failed"] == 2 and cnt["first_fail_cluster"] == 1
    out = capsys.readouterr().out
    assert [ln for ln in out.splitlines() if ln.startswith("MADSIM_TEST_SEED=")] == \
        [f"MADSIM_TEST_SEED={SEED + 19}", f"MADSIM_TEST_SEED={SEED + 3}"]
