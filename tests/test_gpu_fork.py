"""mr_batch_fork on the GPU (docs/SEMANTICS.md §12.5): every forked position equals, bit for bit,
the oracle's run of the position's seed with the source's recorded prefix P set as keyed decisions.

P comes from a recording batch of the source seeds run to the same k events; k is a third of the
sources' median event count as the oracle counts it. Every case asserts that the sources were
still running at the fork, that at least half of the forked positions end with another digest
than their source (a fork that copied nothing of the future would not), and that the sources
themselves still equal their plain oracle runs."""
import contextlib
import copy

import numpy as np
import pytest

from madraft_amd import _abi
from tests.oracle_lib import COUNTER_KEYS

F = _abi
N = 200          # not a multiple of 64 or 256: tail waves and workgroups
TAPE_CAP = 1 << 15
SKIP = _abi.FORK_SKIP

# Every batch forked into below: case -> (scenario, the destination's MR_F_TRACE / MR_F_SAFETY /
# MR_F_RECORD flags, its traced clusters, environment). The GPU tests are parametrised from this
# table and assert that the batch they fork into has exactly these flags, and
# tests/test_fork_host.py checks from the same table that between them the cases hold every row of
# the device-array table that is cluster state.
FORK_CASES = {
    "tape_in_place": ("figure_8_unreliable_2c", ("MR_F_TRACE", "MR_F_SAFETY", "MR_F_RECORD"), 8, {}),
    "pool_figure_8_crash": ("figure_8_unreliable_crash", (), 0, {}),
    "pool_snapshot_7": ("snapshot_install_unreliable_crash_2d", (), 0, {}),
    "pool_snapshot_7_keys_in_hbm": ("snapshot_install_unreliable_crash_2d", (), 0, {"MR_KEY_ROWS": "4"}),
    "pool_kv_3b": ("snapshot_unreliable_recover_3b", (), 0, {}),
    "pool_ctrl_4a": ("basic_4a", (), 0, {}),
    "step_churn": ("unreliable_churn_2c", (), 0, {}),
    "traced_figure_8_crash": ("figure_8_unreliable_crash", ("MR_F_TRACE",), 4, {}),
    "traced_kv_3b": ("snapshot_unreliable_recover_3b", ("MR_F_TRACE",), 4, {}),
}
FORK_SCENARIOS = [(scn, " | ".join(flags) or "0", traced) for scn, flags, traced, _ in FORK_CASES.values()]
SHAPE_FLAGS = F.MR_F_TRACE | F.MR_F_SAFETY | F.MR_F_RECORD


def cases(prefix):
    return [k for k in FORK_CASES if k.startswith(prefix)]


def is_case(batch, case):
    """The batch forked into is the one the table lists for the case."""
    scn, flags, traced, _ = FORK_CASES[case]
    want = 0
    for f in flags:
        want |= getattr(F, f)
    cfg = batch.cfg
    return (int(cfg.scenario) == _abi.SCENARIO_ID[scn] and int(cfg.flags) & SHAPE_FLAGS == want and
            (int(cfg.trace_clusters) if want & F.MR_F_TRACE else 0) == traced and
            int(cfg.n_clusters) == N)


KW = {  # lowered loop counts
    "figure_8_unreliable_2c": dict(iters=150),
    "figure_8_unreliable_crash": dict(iters=150),
    "snapshot_install_unreliable_crash_2d": dict(nodes=7, iters=6),
    "snapshot_unreliable_recover_3b": {},
    "basic_4a": {},
    "unreliable_churn_2c": {},
}


def plain(oracle, cfg, n):
    """The oracle's plain runs of positions 0..n-1 of cfg: (code, t, dig, sums, events[n])."""
    cfg = copy.copy(cfg)
    code, t, dig, sums = oracle.run_batch(cfg, 0, n)
    ev = np.array([oracle.run_cluster(cfg, c)[0]["events"] for c in range(n)])
    return code, t, dig, sums, ev


def fork_point(events):
    return int(np.median(events)) // 3


def record_prefix(hip, test, n, k, **kw):
    """P of seeds 0..n-1 after exactly k events each: the tape of a one-cluster recording batch
    per seed. (A step or tape kernel's launch of k gives a cluster at most k events: a wave runs
    one event class per iteration and the other lanes wait. A wave of one cluster never waits, as
    a pool kernel's cluster never does, so both stand after exactly k.)"""
    flags = kw.pop("flags", 0) | F.MR_F_RECORD
    tapes = []
    for i in range(n):
        with hip.Batch(test, 1, flags=flags, tape_cap=TAPE_CAP, cluster_base=i, **kw) as r:
            st = r.run(max_events=k)
            assert st["remaining"] == 1 and st["events"] == k
            drawn, rec = r.decisions(0, TAPE_CAP)
        assert 0 < drawn <= TAPE_CAP
        tapes.append(np.array(rec))
    return tapes


def record_prefix_batch(hip, test, n, k, **kw):
    """The tapes of one recording batch of n clusters after a launch of k: each cluster's P where
    it stands then (at most k events; the same batch shape stands at the same points again)."""
    flags = kw.pop("flags", 0) | F.MR_F_RECORD
    with hip.Batch(test, n, flags=flags, tape_cap=TAPE_CAP, **kw) as r:
        assert r.run(max_events=k)["remaining"] == n
        drawn, off, rec = r.decisions_all()
    assert (drawn <= TAPE_CAP).all() and (drawn > 0).all()
    return [np.array(rec[int(off[i]):int(off[i + 1])]) for i in range(n)]


def with_prefix(tapes, src_of):
    rows = []
    for c, s in enumerate(src_of):
        d = tapes[int(s)].copy()
        d["cluster"] = c
        rows.append(d)
    return np.concatenate(rows)


def oracle_futures(oracle, cfg, tapes, src_of):
    """The Equivalence's right-hand side for every position: (code, t, dig, sums)."""
    with oracle.replaying(with_prefix(tapes, src_of), len(src_of)):
        return oracle.run_batch(copy.copy(cfg), 0, len(src_of))


def check_per_cluster_counters(cnt, want, n):
    code, t, _, sums = want
    assert cnt["done"] == n and cnt["passed"] == int((code == 0).sum())
    assert cnt["failed"] == n - cnt["passed"] and cnt["virt_time_us"] == int(t.astype(np.uint64).sum())
    for k in ("events", "msgs_sent", "kv_ops", "kv_checked", "kv_lin_checked", "leaders_elected",
              "max_index"):
        assert cnt[k] == sums[k], k
    fails = np.nonzero(code)[0]
    assert cnt["first_fail_cluster"] == (int(fails[0]) if fails.size else 2 ** 64 - 1)


def assert_futures_differ(got_dig, src_dig_of_position, forked):
    differ = int((got_dig[forked] != src_dig_of_position[forked]).sum())
    assert 2 * differ >= int(forked.sum()), (differ, int(forked.sum()))


# ---- case 1 (and 5): the tape kernel, in place, four sources

T1 = FORK_CASES["tape_in_place"][0]
SRC1 = (np.arange(N) // 50 * 50).astype(np.uint32)


@pytest.fixture(scope="module")
def case1(hip, oracle):
    """Shared by the tape cases: the sources' fork point, their prefixes and the oracle's futures."""
    kw = dict(KW[T1], flags=F.MR_F_SAFETY)
    cfg = hip.make_cfg(T1, N, **kw)
    pcode, pt, pdig, psums, ev = plain(oracle, cfg, N)
    k = fork_point(ev[::50])
    assert (ev[::50] > k).all()
    tapes = record_prefix_batch(hip, T1, N, k, **dict(kw))
    want = oracle_futures(oracle, cfg, tapes, SRC1)
    return dict(kw=kw, cfg=cfg, k=k, tapes=tapes, want=want, plain=(pcode, pt, pdig))


@pytest.mark.gpu
def test_tape_kernel_in_place(hip, oracle, case1):
    kw, k, want = case1["kw"], case1["k"], case1["want"]
    flags = kw["flags"] | F.MR_F_RECORD
    with hip.Batch(T1, N, **dict(kw, flags=flags), tape_cap=TAPE_CAP, trace_clusters=8,
                   trace_cap=2048) as b:
        assert b.kernel == "step_kernel_tape" and is_case(b, "tape_in_place")
        assert b.run(max_events=k)["remaining"] == N
        _, off, rec = b.decisions_all()  # P is what these sources have drawn, where they stand
        for s in range(0, N, 50):
            assert np.array_equal(rec[int(off[s]):int(off[s + 1])], case1["tapes"][s]), s
        b.fork(SRC1)
        assert b.run()["remaining"] == 0
        code, t, dig = b.verdicts()
        cnt = b.counters()
        drawn, off, rec = b.decisions_all()
        traces = [b.trace(c) for c in range(8)]
    for name, g, w in zip(("code", "time", "digest"), (code, t, dig), want[:3]):
        assert np.array_equal(g, w), name
    pcode, pt, pdig = case1["plain"]
    forked = SRC1 != np.arange(N)
    assert_futures_differ(dig, pdig[SRC1], forked)
    for s in range(0, N, 50):  # the sources: their plain runs
        assert (code[s], t[s], dig[s]) == (pcode[s], pt[s], pdig[s])
    # the whole history is kept per cluster on this kernel: every counter is the oracle's sum
    for key in COUNTER_KEYS:
        assert cnt[key] == want[3][key], key
    check_per_cluster_counters(cnt, want, N)
    # a forked position's final tape is its whole history: replayed from scratch, the same run
    assert (drawn <= TAPE_CAP).all()
    pick = [1, 7, 49, 51, 149, 199]
    tapes = [rec[int(off[c]):int(off[c + 1])] for c in pick]
    for c, tp in zip(pick, tapes):  # it starts with the source's prefix
        p = case1["tapes"][int(SRC1[c])]
        assert all(np.array_equal(tp[f][: p.size], p[f]) for f in p.dtype.names[1:]), c
    seeds = [int(case1["cfg"].seed_base) + c for c in pick]
    res = hip.replay_many(T1, tapes, seeds, trace_cap=2048, **kw)
    for c, (tr, rc, rt, misses) in zip(pick, res):
        assert (rc, rt, misses) == (int(code[c]), int(t[c]), 0), c
        if c < 8:
            assert np.array_equal(tr, traces[c]), c


@pytest.mark.gpu
@pytest.mark.parametrize("stream", [False, True], ids=["chunked", "streaming"])
def test_chunked_and_streaming_destination(hip, case1, stream):
    """lanes = 64 of 200 clusters: the destination is forked in the middle of its own run (its
    first chunk advanced, the streaming one with lanes' clusters held) and starts over."""
    kw, k, want = case1["kw"], case1["k"], case1["want"]
    flags = kw["flags"] | F.MR_F_RECORD
    with hip.Batch(T1, N, **dict(kw, flags=flags), tape_cap=TAPE_CAP) as src, \
            hip.Batch(T1, N, **dict(kw, flags=flags), tape_cap=TAPE_CAP, lanes=64,
                      stream=stream) as dst:
        assert src.run(max_events=k)["remaining"] == N
        assert dst.run(max_events=k // 2)["remaining"] == N
        dst.fork(SRC1, src)
        st = dst.run()
        assert st["remaining"] == 0 and st["launches"] >= (1 if stream else 4)
        got, cnt = dst.verdicts(), dst.counters()
    for g, w in zip(got, want[:3]):
        assert np.array_equal(g, w)
    for key in COUNTER_KEYS:
        assert cnt[key] == want[3][key], key


# ---- cases 2, 3, 4: a 4-cluster source forked into 200 positions of another batch

def across(hip, oracle, monkeypatch, case, kernel, kv_applies=False, single=False, caps=(4096, 4096)):
    """`single`: the four sources are one-cluster batches (a step kernel's wave of four would not
    stand after exactly k events each), forked in by four calls. `caps`: the trace_cap of a traced
    source and of the destination."""
    test, _, traced, env = FORK_CASES[case]
    for key, v in env.items():
        monkeypatch.setenv(key, v)
    kw = dict(KW[test])
    skw = dict(trace_clusters=traced, trace_cap=caps[0]) if traced else {}
    tkw = dict(trace_clusters=traced, trace_cap=caps[1]) if traced else {}
    src_of = ((np.arange(N) + 1) % 4).astype(np.uint32)  # no position runs its source's seed
    cfg = hip.make_cfg(test, N, **kw, **tkw)
    pcode, pt, pdig, _, ev = plain(oracle, hip.make_cfg(test, 4, **kw), 4)
    k = fork_point(ev)
    assert (ev > k).all()
    tapes = record_prefix(hip, test, 4, k, **dict(kw))
    want = oracle_futures(oracle, cfg, tapes, src_of)
    with contextlib.ExitStack() as stack:
        dst = stack.enter_context(hip.Batch(test, N, **kw, **tkw))
        assert is_case(dst, case)
        if single:
            for i in range(4):
                src = stack.enter_context(hip.Batch(test, 1, cluster_base=i, **kw))
                st = src.run(max_events=k)
                assert src.kernel == kernel and st["remaining"] == 1 and st["events"] == k
                dst.fork(np.where(src_of == i, 0, SKIP).astype(np.uint32), src)
            src = stack.enter_context(hip.Batch(test, 4, **kw))  # (run whole below)
        else:
            src = stack.enter_context(hip.Batch(test, 4, **kw, **skw))
            st = src.run(max_events=k)
            assert src.kernel == kernel and st["remaining"] == 4 and st["events"] == 4 * k
            dst.fork(src_of, src)
        assert dst.kernel == kernel
        assert dst.run()["remaining"] == 0
        code, t, dig = dst.verdicts()
        cnt = dst.counters()
        for name, g, w in zip(("code", "time", "digest"), (code, t, dig), want[:3]):
            assert np.array_equal(g, w), name
        check_per_cluster_counters(cnt, want, N)
        assert_futures_differ(dig, pdig[src_of], np.ones(N, bool))
        if traced:
            cap = caps[1]
            with oracle.replaying(with_prefix(tapes, src_of), N):
                for c in range(traced):
                    _, otr, odg = oracle.run_cluster_dig(copy.copy(cfg), c, cap)
                    assert otr.size < min(caps)  # (no trace overflowed: every record compared)
                    assert np.array_equal(dst.trace(c), otr), c
                    assert np.array_equal(dst.trace_digests(c), odg), c
                    if kv_applies:
                        _, _, oap = oracle.run_cluster_kv(copy.copy(cfg), c, cap)
                        assert oap.size and np.array_equal(dst.trace_applies(c), oap), c
        assert src.run()["remaining"] == 0  # the sources go on as if never read
        for g, w in zip(src.verdicts(), (pcode, pt, pdig)):
            assert np.array_equal(g, w)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases("pool_"))
def test_pool_kernels_across_batches(hip, oracle, monkeypatch, case):
    across(hip, oracle, monkeypatch, case, "pool_kernel")


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases("step_"))
def test_step_kernel_with_spawned_threads(hip, oracle, monkeypatch, case):
    across(hip, oracle, monkeypatch, case, "step_kernel", single=True)


@pytest.mark.gpu
@pytest.mark.parametrize("case", cases("traced_"))
def test_traces_come_along(hip, oracle, monkeypatch, case):
    """The two trace_caps differ: figure_8's destination rows are shorter than the source's (they
    take its head), the KV case's are longer (zero above the source's, as a reset leaves them)."""
    kv = case == "traced_kv_3b"
    across(hip, oracle, monkeypatch, case, "pool_kernel", kv_applies=kv,
           caps=(16384, 32768) if kv else (8192, 4096))


# ---- case 6: finished clusters, and forks that copy nothing

T6 = "figure_8_unreliable_2c"


@pytest.fixture(scope="module")
def case6(hip, oracle):
    kw = dict(KW[T6])
    cfg = hip.make_cfg(T6, N, **kw)
    pcode, pt, pdig, psums, ev = plain(oracle, hip.make_cfg(T6, 4, **kw), 4)
    k = fork_point(ev)
    assert (ev > k).all()
    tapes = record_prefix(hip, T6, 4, k, **dict(kw))
    src_of = ((np.arange(N) + 1) % 4).astype(np.uint32)
    return dict(kw=kw, cfg=cfg, k=k, tapes=tapes, src_of=src_of, plain4=(pcode, pt, pdig),
                want=oracle_futures(oracle, cfg, tapes, src_of))


@pytest.mark.gpu
def test_finished_destination_runs_again(hip, case6):
    kw, k = case6["kw"], case6["k"]
    with hip.Batch(T6, 4, **kw) as src, hip.Batch(T6, N, **kw) as dst:
        assert dst.run()["remaining"] == 0
        assert src.run(max_events=k)["remaining"] == 4
        with pytest.raises(hip.SimError, match="not a fork"):
            dst.fork_ms()
        dst.fork(case6["src_of"], src)
        assert dst.fork_ms() > 0
        assert dst.counters()["done"] == 0
        assert dst.run()["remaining"] == 0
        with pytest.raises(hip.SimError, match="not a fork"):
            dst.fork_ms()
        for g, w in zip(dst.verdicts(), case6["want"][:3]):
            assert np.array_equal(g, w)


@pytest.mark.gpu
def test_streaming_pool_destination(hip, case6):
    """A pool batch whose slots refill from the rest of the batch (D.stream with the pool family),
    forked in the middle of its run with clusters held for a resume: the launch loop starts over.
    A pool batch larger than the resident pools streams by itself on this same path (its L is the
    device's capacity instead of `lanes`), too large a batch for a quick test."""
    kw, k = case6["kw"], case6["k"]
    with hip.Batch(T6, 4, **kw) as src, hip.Batch(T6, N, **kw, lanes=64, stream=True) as dst:
        assert dst.kernel == "pool_kernel"
        assert dst.run(max_events=k // 2)["remaining"] == N
        assert src.run(max_events=k)["remaining"] == 4
        dst.fork(case6["src_of"], src)
        assert dst.run()["remaining"] == 0
        for g, w in zip(dst.verdicts(), case6["want"][:3]):
            assert np.array_equal(g, w)


@pytest.mark.gpu
def test_finished_source_gives_its_verdict(hip, case6):
    kw = case6["kw"]
    src_of = np.full(N, SKIP, np.uint32)
    src_of[5:150] = 2
    with hip.Batch(T6, 4, **kw) as src, hip.Batch(T6, N, **kw) as dst:
        assert src.run()["remaining"] == 0
        assert dst.run(max_events=case6["k"])["remaining"] == N
        dst.fork(src_of, src)
        assert dst.counters()["done"] == 145
        assert dst.run()["remaining"] == 0
        code, t, dig = dst.verdicts()
        pcode, pt, pdig = case6["plain4"]
        assert (code[5:150] == pcode[2]).all() and (t[5:150] == pt[2]).all()
        assert (dig[5:150] == pdig[2]).all()
    with hip.Batch(T6, N, **kw) as ref:  # the positions left alone: their own runs
        ref.run()
        rcode, rt, rdig = ref.verdicts()
    keep = src_of == SKIP
    assert np.array_equal(code[keep], rcode[keep]) and np.array_equal(dig[keep], rdig[keep])


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["identity", "none"])
def test_forks_that_copy_nothing_change_nothing(hip, case6, which):
    kw = dict(case6["kw"], flags=F.MR_F_RECORD)
    src_of = np.arange(N, dtype=np.uint32) if which == "identity" else np.full(N, SKIP, np.uint32)

    def state(b):
        return b.verdicts(), b.counters(), b.decisions_all()

    def same(a, b):
        return all(np.array_equal(x, y) for x, y in zip(a[0], b[0])) and a[1] == b[1] and \
            all(np.array_equal(x, y) for x, y in zip(a[2], b[2]))

    with hip.Batch(T6, N, **kw, tape_cap=TAPE_CAP) as b, hip.Batch(T6, N, **kw, tape_cap=TAPE_CAP) as ref:
        assert b.run(max_events=case6["k"])["remaining"] == N
        before = state(b)
        b.fork(src_of)
        assert same(before, state(b))
        b.run()
        ref.run()
        assert same(state(ref), state(b))


# ---- case 7: errors leave the batches as they were

@pytest.mark.gpu
def test_errors_leave_the_batch_as_it_was(hip, oracle, case6):
    kw, k = case6["kw"], case6["k"]
    none = np.full(N, SKIP, np.uint32)

    def bad(dst, src_of, src, message):
        with pytest.raises(hip.SimError, match=message):
            dst.fork(src_of, src)

    def at(c, s):
        a = none.copy()
        a[c] = s
        return a

    with hip.Batch(T6, N, **kw, trace_clusters=2) as dst, hip.Batch(T6, 4, **kw) as pool_src, \
            hip.Batch(T6, 4, **kw, flags=F.MR_F_RECORD, tape_cap=TAPE_CAP) as tape_src, \
            hip.Batch(T6, N, **kw, flags=F.MR_F_RECORD, tape_cap=TAPE_CAP) as rec_dst, \
            hip.Batch(T6, 4, **kw, log_cap=2 * int(dst.cfg.log_cap)) as big_src, \
            hip.Batch(T6, 4, **kw, trace_clusters=4, trace_cap=16) as short_src:
        assert dst.kernel == pool_src.kernel == "pool_kernel"
        assert dst.run(max_events=k)["remaining"] == N
        for b in (pool_src, tape_src, big_src, short_src):
            assert b.run(max_events=k)["remaining"] == 4
        assert rec_dst.run(max_events=k)["remaining"] == N
        bad(dst, at(9, 4), pool_src, "the source has 4 clusters")
        chained = none.copy()
        chained[1], chained[2] = 2, 3
        bad(dst, chained, None, "itself overwritten")
        pool_src.submit(int(pool_src.cfg.seed_base))
        bad(dst, at(9, 1), pool_src, "submitted step")
        pool_src.finish()
        bad(dst, at(9, 1), tape_src, "source ran on step_kernel / step_kernel_tape, destination "
                                     "continues on pool_kernel")
        bad(dst, at(1, 1), pool_src, "not traced")
        bad(dst, at(1, 1), short_src, "trace records past its trace_cap 16")
        bad(rec_dst, at(9, 1), pool_src, "recording destination")
        bad(dst, at(9, 1), big_src, "differ in log_cap")
        assert dst.run()["remaining"] == 0 and rec_dst.run()["remaining"] == 0
        got, rgot = dst.verdicts(), rec_dst.verdicts()
    ocode, ot, odig = oracle.run_batch(copy.copy(case6["cfg"]), 0, N)[:3]
    for g, r, w in zip(got, rgot, (ocode, ot, odig)):
        assert np.array_equal(g, w) and np.array_equal(r, w)


# ---- case 8: sim.run_futures

@pytest.mark.gpu
def test_run_futures_and_replay(hip, oracle):
    kw = dict(KW[T6])
    seed = _abi.README_SEED + 3
    ev = oracle.run_cluster(hip.make_cfg(T6, 1, seed, **kw), 0)[0]["events"]
    k = ev // 3
    r = hip.run_futures(T6, seed, k, 256, **kw)
    assert r["kernel"] == "pool_kernel" and r["counters"]["done"] == 256
    want = oracle_futures(oracle, hip.make_cfg(T6, 256, seed, **kw), [r["prefix"]], np.zeros(256, int))
    for g, w in zip((r["codes"], r["times_us"], r["digests"]), want[:3]):
        assert np.array_equal(g, w)
    assert np.unique(r["digests"]).size > 128
    failing = np.nonzero(r["codes"])[0]
    for c in list(failing[:1]) + [1, 255, 100][: 3 - min(1, failing.size)]:
        _, code, tm, _ = hip.replay(T6, r["prefix"], seed=seed, cluster_base=int(c), **kw)
        assert (code, tm) == (int(r["codes"][c]), int(r["times_us"][c])), c
    with pytest.raises(hip.SimError, match="ended within"):
        hip.run_futures(T6, seed, 10 * ev, 4, **kw)


# ---- parameter groups on the destination

@pytest.mark.gpu
def test_fork_into_parameter_groups(hip, oracle, case6):
    """Positions in the source's own settings (an all-inheriting group) equal the oracle; the other
    group has no from-scratch equivalent (its prefix ran under the source's settings): two
    identical runs agree."""
    kw, k, tapes = case6["kw"], case6["k"], case6["tapes"]
    group_of = (np.arange(N) % 2).astype(np.uint32)
    src_of = case6["src_of"]
    runs = []
    for _ in range(2):
        with hip.Batch(T6, N, **kw) as dst:
            dst.set_param_groups([{}, {"hb_us": 2 * int(dst.cfg.hb_us)}], group_of)
            for i in range(4):  # one-cluster tape sources: each stands after exactly k events
                with hip.Batch(T6, 1, cluster_base=i, **kw, flags=F.MR_F_RECORD,
                               tape_cap=TAPE_CAP) as src:
                    assert src.run(max_events=k)["events"] == k
                    dst.fork(np.where(src_of == i, 0, SKIP).astype(np.uint32), src)
            assert dst.kernel == "step_kernel_tape"
            assert dst.run()["remaining"] == 0
            runs.append(dst.verdicts())
    for a, b in zip(*runs):
        assert np.array_equal(a, b)
    own = group_of == 0
    for g, w in zip(runs[0], case6["want"][:3]):
        assert np.array_equal(g[own], w[own])
    assert (runs[0][2][~own] != case6["want"][2][~own]).any()


@pytest.mark.gpu
def test_command_line_fork_at(hip, capsys, tmp_path):
    """`--fork-at EVENTS --futures N`: the summary line, and the prefix written as a replay log
    that `--replay` with a future's seed plays to that future's verdict."""
    import json

    from madraft_amd import __main__ as cli
    log = str(tmp_path / "prefix.jsonl")
    args = [T6, "--iters", "150", "--seed", str(_abi.README_SEED + 3)]
    with pytest.raises(SystemExit) as e:
        cli.main(args + ["--fork-at", "300", "--futures", "64", "--fork-tape", log])
    lines = [json.loads(x) for x in capsys.readouterr().out.splitlines() if x.startswith("{")]
    head = lines[0]
    assert head["futures"] == 64 and head["passed"] + head["failed"] == 64
    assert head["kernel"] == "pool_kernel" and head["prefix_decisions"] > 0
    assert len(lines) == 1 + head["failed"] and e.value.code == (1 if head["failed"] else 0)
    r = hip.run_futures(T6, _abi.README_SEED + 3, 300, 64, iters=150)
    with pytest.raises(SystemExit):
        cli.main([T6, "--iters", "150", "--seed", str(_abi.README_SEED + 3 + 5), "--replay", log])
    out = json.loads(capsys.readouterr().out.splitlines()[-1])
    assert (out["code"], out["time_us"]) == (int(r["codes"][5]), int(r["times_us"][5]))
