"""The pool kernel's queue entry carries next_event's decision (madraft_amd/csrc/mr_qentry.h,
DESIGN.md §6.15): the claiming wave runs the event its publisher decided and does not decide again.

Bar: bit-exact. The pool kernel and the per-lane step kernel (MR_POOL=0), which decides every
event itself, agree on every verdict code, verdict time, trace digest and counter on batches
whose queues wrap many times; a batch reused for other seeds gives the first seeds' results again
and its apply checker still catches a buggy Raft where the oracle does; and every field of an
entry comes back from the packing as it went in, at both pool sizes.
"""
import os
import subprocess
import tempfile

import numpy as np
import pytest

from madraft_amd import _abi
from tests.oracle_lib import COUNTER_KEYS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = _abi.README_SEED


def agree(hip, monkeypatch, test, clusters, **kw):
    def run():
        with hip.Batch(test, clusters, **kw) as b:
            st = b.run()
            assert st["remaining"] == 0
            return b.kernel, b.verdicts(), b.counters()
    kp, vp, cp = run()
    monkeypatch.setenv("MR_POOL", "0")
    if "lanes" in kw:
        kw = dict(kw, lanes=0)
    ks, vs, cs = run()
    assert (kp, ks) == ("pool_kernel", "step_kernel")
    for name, a, c in zip(("code", "time", "digest"), vp, vs):
        bad = np.nonzero(a != c)[0]
        assert bad.size == 0, f"{test}: {name} differs in {bad.size} clusters, first {bad[0]}"
    for k in COUNTER_KEYS:
        assert cp[k] == cs[k], (test, k, cp[k], cs[k])
    assert cp["done"] == clusters
    return cp


# 1 024 clusters: two workgroups of the Raft pool (four of the service pool), each queue's 512
# (256) positions reused for every lap of the ~6 K - 20 K events a cluster runs, so the lap tags
# and the entries' decision bits are written and read at every position many times
@pytest.mark.gpu
@pytest.mark.parametrize("test,kw,env", [
    ("figure_8_unreliable_2c", {}, {}),                        # the headline: three kinds
    ("figure_8_unreliable_crash", {}, {}),                     # the fine kinds: all six queues
    ("snapshot_install_unreliable_2d", dict(nodes=7), {"MR_KEY_ROWS": "4"}),  # 7 servers: node 0..6
    ("unreliable_3a", {}, {}),                                 # the service pool: clerk hosts, tcli
    ("persist_partition_unreliable_linearizable_3a", {}, {}),  # and the continuation kind
])
def test_pool_entry_decision_equals_step_kernel(hip, monkeypatch, test, kw, env):
    """The event a claimed entry names is the event the step kernel's own next_event chooses."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    cnt = agree(hip, monkeypatch, test, 1024, **kw)
    if env:
        assert cnt["max_inflight"] > int(env["MR_KEY_ROWS"])  # keys in HBM were used


@pytest.mark.gpu
def test_pool_entry_of_a_streamed_cluster(hip, monkeypatch):
    """One workgroup's 512 slots stream 4 096 clusters: a slot's next cluster is published with an
    entry made from the state cluster_claim loaded, not from an event's result."""
    agree(hip, monkeypatch, "figure_8_unreliable_2c", 4096, lanes=512, iters=40)


def three_steps(hip, test, clusters, **kw):
    """One batch stepped (submit / finish) on the first seeds, on the next ones, and on the first
    again: each step's verdicts and counters, and the batch's config at the last step."""
    out = []
    with hip.Batch(test, clusters, **kw) as b:
        for base in (SEED, SEED + clusters, SEED):
            b.submit(base)
            st, cnt = b.finish()
            assert st["remaining"] == 0
            out.append((b.verdicts(), cnt))
        cfg = b.cfg
    return out, cfg


@pytest.mark.gpu
@pytest.mark.parametrize("test", ["figure_8_unreliable_2c", "snapshot_install_unreliable_crash_2d"])
def test_reused_batch_repeats_its_first_step(hip, test):
    """Nothing of a step leaks into the next one of the same batch: in particular no apply-checker
    record of the seeds in between (the second body's restarts replay the applier from a snapshot
    over records an earlier step wrote)."""
    (s1, s2, s3), _ = three_steps(hip, test, 512)
    for a, c in zip(s1[0], s3[0]):
        assert np.array_equal(a, c)
    for k in COUNTER_KEYS:
        assert s1[1][k] == s3[1][k], k
    assert not np.array_equal(s1[0][2], s2[0][2])  # the step in between ran other seeds


@pytest.mark.gpu
def test_reused_batch_apply_checker_still_catches(hip, oracle):
    """A buggy Raft (no prevLogIndex check) on a reused batch: APPLY_MISMATCH is caught for the same
    clusters, at the same time and with the same trace digest as the oracle's fresh run."""
    n = 256
    (_, _, s3), cfg = three_steps(hip, "figure_8_unreliable_2c", n, flags=_abi.MR_F_BUG_NO_PREV_CHECK)
    assert not cfg.flags & _abi.MR_F_BUG_NO_APPLY_CHECK and cfg.seed_base == SEED
    (code, t, dig), cnt = s3
    ocode, ot, odig, osum = oracle.run_batch(cfg, 0, n)
    assert np.array_equal(code, ocode) and np.array_equal(t, ot) and np.array_equal(dig, odig)
    for k in COUNTER_KEYS:
        assert cnt[k] == osum[k], k
    # (the oracle's count on these seeds: 256 when test_apply_checker_failures_bit_exact was written)
    assert int((ocode == 8).sum()) >= 200  # MR_FAIL_APPLY_MISMATCH


ENTRY_SRC = r"""
#include <cstdio>
#include "%s"
template <uint32_t FAM>
static long walk() {
  using Q = mr::QEntry<FAM>;
  static_assert(Q::round_trips(), "the header's own check");
  // laps: every 16-bit tag at the ends of the other fields, and these with every other field
  const uint32_t laps[] = {0u, 1u, 2u, 0x7FFFu, 0x8000u, 0xFFFEu, 0xFFFFu, 0x10000u, 0x12345u};
  long n = 0, bad = 0;
  auto one = [&](uint32_t lap, uint32_t slot, uint32_t cls, uint32_t node, bool tcli) {
    const uint32_t pos = (lap << Q::SLOT_B) | ((slot * 7u + 3u) & (Q::SLOT_N - 1u));  // any position of the lap
    const uint32_t e = Q::pack(pos, slot, mr::QDec{cls, node, tcli});
    const mr::QDec d = Q::dec(e);
    n++;
    if (Q::tag(e) != Q::tag_of(pos) || Q::tag(e) != (lap << 16) || Q::slot(e) != slot || d.cls != cls ||
        d.node != node || d.tcli != tcli)
      bad++;
  };
  for (uint32_t cls = 0; cls < Q::CLS_N; cls++)
    for (uint32_t node = 0; node < Q::NODE_N; node++)
      for (uint32_t tcli = 0; tcli <= Q::TCLI_B; tcli++)
        for (uint32_t slot = 0; slot < Q::SLOT_N; slot++) {
          for (uint32_t lap : laps) one(lap, slot, cls, node, tcli != 0u);
          if ((cls == 0u || cls == Q::CLS_N - 1u) && (node == 0u || node == Q::NODE_N - 1u))
            for (uint32_t lap = 0; lap < 0x10000u; lap += (slot == 0u || slot == Q::SLOT_N - 1u) ? 1u : 257u)
              one(lap, slot, cls, node, tcli != 0u);
        }
  std::printf("%%u %%u %%u %%u %%u %%ld %%ld\n", FAM, Q::SLOT_N, Q::CLS_N, Q::NODE_N, Q::TCLI_B, n, bad);
  return bad;
}
int main() { return (walk<1>() | walk<2>()) ? 1 : 0; }
"""


def test_queue_entry_round_trips():
    """mr_qentry.h on the host: every (class, node, spawned-thread bit, slot) with laps at both ends
    and around the 16-bit wrap, and every lap at the ends of the other fields, unpacks to what was
    packed, for the Raft pool (512 slots, nodes 0..7) and the service pool (256 slots, nodes
    0..31: servers and the clerk hosts 8 + k). An overlap of two fields also fails the header's
    static_assert, so the product does not build."""
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "q.cpp"), os.path.join(d, "q")
        with open(src, "w") as f:
            f.write(ENTRY_SRC % os.path.join(ROOT, "madraft_amd", "csrc", "mr_qentry.h"))
        subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-o", exe, src], check=True)
        out = subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split("\n")
    rows = [list(map(int, l.split())) for l in out if l]
    assert [r[:5] for r in rows] == [[1, 512, 4, 8, 0], [2, 256, 4, 32, 1]]
    assert all(r[5] > 100000 and r[6] == 0 for r in rows)
