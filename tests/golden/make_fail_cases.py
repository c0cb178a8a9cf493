"""Regenerate tests/golden/fail_cases.json: configurations under which the CPU oracle ends clusters
with the tester's failing verdicts (the rows of MR_FAIL_TABLE that are reference panic sites), each
on a real Raft that is misconfigured (timers, AppendEntries size, server count) or deliberately
buggy (MR_F_BUG_*), never the null node. A case holds the scenario, the cluster count, cluster_base,
the sim.make_cfg keywords, the oracle's verdict histogram and `expect`, the codes it is there to
reach.

tests/test_gpu_fail_sites.py holds the HIP path to every case bit for bit (verdict, time, digest,
traces, counters); tests/test_fail_sites.py checks the oracle against the file and that every
verdict code is accounted for. Checked here before the file is written:
  - every code of REQUIRED ends at least MIN_HITS clusters of one case that expects it (the thin
    codes of THIN: at least THIN_HITS);
  - a case has 128..512 clusters and at most MAX_WORK events in all (the oracle's count);
  - max_events = 200000, and no cluster ends SIM_EVENT_LIMIT unless the case expects it;
  - one of the first four clusters (the ones compared record by record) ends with an expected code.
Run:
    python tests/golden/make_fail_cases.py
"""
import collections
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

from madraft_amd import _abi, sim  # noqa: E402
from tests.oracle_lib import Oracle  # noqa: E402

REQUIRED = [2, 3, 4, 7, 17, 19, 20, 21, 24, 25, 26, 30, 31, 40, 46, 47, 48]
THIN = [35, 41]  # a few clusters in a thousand
MIN_HITS, THIN_HITS = 8, 2
MAX_WORK = 2500000
MAX_EVENTS = 200000

TWICE, STALE = _abi.MR_F_BUG_VOTE_TWICE, _abi.MR_F_BUG_VOTE_STALE
NO_PREV, NO_CHECK = _abi.MR_F_BUG_NO_PREV_CHECK, _abi.MR_F_BUG_NO_APPLY_CHECK
UNREL = _abi.MR_F_UNRELIABLE
FAST = dict(elect_lo_us=20000, elect_hi_us=40000)  # election timeouts below the heartbeat period

# (name, test, clusters, cluster_base, make_cfg keywords, expect)
CASES = [
    # tester.rs check_one_leader / check_terms / check_no_leader
    ("many_election_2a+vote_twice", "many_election_2a", 256, 0, dict(flags=TWICE), [2]),
    ("fail_no_agree_2b+vote_twice", "fail_no_agree_2b", 256, 6, dict(flags=TWICE), [2]),
    ("snapshot_install_unreliable_2d+vote_twice", "snapshot_install_unreliable_2d", 256, 0,
     dict(flags=TWICE), [2]),
    ("initial_election_2a+elect_20ms", "initial_election_2a", 256, 0, FAST, [3]),
    ("reelection_2a@7", "reelection_2a", 128, 0, dict(nodes=7), [4]),
    ("count_2b+elect_fixed", "count_2b", 128, 0, dict(elect_lo_us=150000, elect_hi_us=150001), [1]),
    # tester.rs end(): 120 s of virtual time
    ("snapshot_rpc_3b+hb_250ms", "snapshot_rpc_3b", 256, 0, dict(hb_us=250000), [7]),
    # raft/tests.rs 2B bodies
    ("fail_no_agree_2b@7", "fail_no_agree_2b", 128, 0, dict(nodes=7), [17]),
    ("concurrent_starts_2b+elect_20ms", "concurrent_starts_2b", 128, 0, FAST, [19]),
    ("concurrent_starts_2b+hb_250ms", "concurrent_starts_2b", 128, 0, dict(hb_us=250000), [19]),
    ("count_2b+hb_250ms", "count_2b", 128, 0, dict(hb_us=250000), [20]),
    ("count_2b+elect_20ms", "count_2b", 128, 0, FAST, [21]),
    ("count_2b+ae_1", "count_2b", 256, 0, dict(ae_max=1), [24]),
    ("count_2b+hb_20ms+ae_2", "count_2b", 256, 0, dict(hb_us=20000, ae_max=2), [21, 25]),
    # raft/tests.rs internal_churn
    ("unreliable_churn_2c+vote_stale", "unreliable_churn_2c", 256, 0,
     dict(flags=STALE | NO_CHECK), [26]),
    # shard_ctrler tester.rs check() and tests.rs
    ("multi_4a+vote_twice", "multi_4a", 512, 8, dict(flags=TWICE | NO_CHECK), [30]),
    ("basic_4a+all_bugs+elect_40ms", "basic_4a", 384, 7,
     dict(flags=TWICE | STALE | NO_PREV | NO_CHECK | UNREL, elect_lo_us=40000, elect_hi_us=80000),
     [30, 31, 34, 35, 36]),
    ("multi_4a+elect_20ms", "multi_4a", 128, 0, FAST, [40]),
    ("multi_4a+vote_stale+unreliable", "multi_4a", 512, 17,
     dict(flags=STALE | NO_CHECK | UNREL), [41]),
    # kvraft tests.rs one_partition_3a, tester.rs Clerk::check
    ("one_partition_3a+stale_read", "one_partition_3a", 256, 0,
     dict(flags=_abi.MR_F_BUG_STALE_READ), [46]),
    ("one_partition_3a+hb_250ms", "one_partition_3a", 256, 0, dict(hb_us=250000), [47]),
    ("snapshot_rpc_3b+vote_stale", "snapshot_rpc_3b", 128, 0, dict(flags=STALE | NO_CHECK), [48]),
]


def measure(o, name, test, clusters, base, kw, expect):
    kw = dict(kw, max_events=MAX_EVENTS)
    cfg = sim.make_cfg(test, clusters, cluster_base=base, **kw)
    code, _, _, s = o.run_batch(cfg, 0, clusters)
    hist = collections.Counter(code.tolist())
    assert 128 <= clusters <= 512 and s["events"] <= MAX_WORK, (name, clusters, s["events"])
    assert _abi.MR_RUNNING not in hist, name
    assert 61 in expect or 61 not in hist, (name, "SIM_EVENT_LIMIT", hist[61])
    assert set(code[:4].tolist()) & set(expect), (name, "no traced cluster fails as expected")
    assert all(hist[c] for c in expect), (name, hist)
    return {"name": name, "test": test, "clusters": clusters, "cluster_base": base, "kw": kw,
            "events_per_seed": s["events"] // clusters,
            "hist": {str(k): v for k, v in sorted(hist.items())}, "expect": expect}


def main():
    o = Oracle()
    cases = [measure(o, *c) for c in CASES]
    assert len({c["name"] for c in cases}) == len(cases)
    best = collections.Counter()  # code -> the most clusters one case that expects it ends with it
    for c in cases:
        for code in c["expect"]:
            best[code] = max(best[code], c["hist"][str(code)])
    for code in REQUIRED:
        assert best[code] >= MIN_HITS, (code, best[code])
    for code in THIN:
        assert best[code] >= THIN_HITS, (code, best[code])
    out = {"note": "oracle verdict histograms (code -> clusters) over seeds [cluster_base, "
                   "cluster_base + clusters) of sim.make_cfg(test, clusters, cluster_base="
                   "cluster_base, **kw); expect = the failing codes the case is there to reach; "
                   "tests/golden/make_fail_cases.py",
           "cases": cases}
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "fail_cases.json")
    json.dump(out, open(path, "w"), indent=1)
    print(path, len(cases), "cases; most clusters per expected code:", dict(sorted(best.items())))


if __name__ == "__main__":
    main()
