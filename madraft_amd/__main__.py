"""CLI: `python -m madraft_amd <test> [--clusters N] [--seed S]` — the batched
analogue of `MADSIM_TEST_SEED=S MADSIM_TEST_NUM=N cargo test <test>`;
`--replay log.jsonl` plays one cluster driven by an event-level decision log
(madraft_amd/trace.py) and prints its verdict; `--seed S --shrink` shrinks a failing seed to a
1-minimal set of dropped (or delayed) messages (madraft_amd/shrink.py);
`--clusters N --shrink-failures [K]` runs the N seeds and shrinks the first K failing ones in one
variant batch of groups, one launch per ddmin round for all of them; `--seeds LIST` (or `@file`)
runs exactly those seeds in one batch (docs/SEMANTICS.md §12.3), and with `--shrink` shrinks them;
`--sweep FIELD=V1,V2,...` (repeatable) runs every combination of the settings over the same seeds
in one batch of parameter groups (§12.4) and prints one JSON line per setting;
`--seed S --fork-at EVENTS --futures N` runs seed S for EVENTS events, forks that state into N
positions (§12.5) and prints the futures' verdict histogram and, per failing future, the
`sim.replay` call that reproduces it."""
import argparse
import json
import time

from . import _abi, shrink, sim, trace


# test bodies that switch the net back to reliable part-way (tests.rs:680 unreliable_agree_2c
# before join_all and the final one(); tests.rs:832 internal_churn before the final one()):
# their sends have no single mode, so a log of them must carry it per line (or be a raw log)
MIXED_MODE = {"unreliable_agree_2c", "unreliable_churn_2c"}


def net_mode(test, unreliable_flag):
    """The network mode a replayed log's sends were drawn under when a line does not say:
    `--unreliable` (MR_F_UNRELIABLE from the tester's start: every send unreliable), else the
    test body's own single mode — the tests named *unreliable* that stay unreliable to the end
    (figure_8_unreliable_2c tests.rs:692, snap_common's unreliable 2D tests :864) send every
    message unreliably, the others reliably. For the tests that switch modes (MIXED_MODE) there
    is no single answer: None, so trace.decisions_from_events rejects a send line without its
    own "unreliable" field instead of decoding it under the wrong latency range and loss draw."""
    if unreliable_flag:
        return True
    if test in MIXED_MODE:
        return None
    return "unreliable" in test


def parse_seeds(arg):
    """`--seeds`: "S1,S2,..." or "@file" with one seed per line (blank lines and # comments
    skipped); decimal or 0x... numbers, in the order given, duplicates kept."""
    if arg.startswith("@"):
        with open(arg[1:]) as f:
            words = [line.split("#", 1)[0].strip() for line in f]
    else:
        words = [w.strip() for w in arg.split(",")]
    seeds = [int(w, 0) for w in words if w]
    if not seeds:
        raise ValueError(f"--seeds {arg!r}: no seeds")
    return seeds


SWEEP_FIELDS = ("hb_us", "ae_max", "iters", "elect_us", "bug")


def parse_sweep(specs):
    """`--sweep` arguments as run_sweep's grid, in the order given: "hb_us=25000,50000" (likewise
    ae_max, iters), "elect_us=150000:300000,50000:60000" (lo:hi pairs), "bug=none,vote_stale"."""
    grid = {}
    for spec in specs:
        field, eq, vals = spec.partition("=")
        words = [w.strip() for w in vals.split(",") if w.strip()]
        if not eq or field not in SWEEP_FIELDS or not words:
            raise ValueError(f"--sweep {spec!r}: want FIELD=V1,V2,... with FIELD one of "
                             f"{', '.join(SWEEP_FIELDS)}")
        if field in grid:
            raise ValueError(f"--sweep {spec!r}: {field} is swept twice")
        if field == "bug":
            bad = [w for w in words if w not in _abi.BUG_FLAGS]
            if bad:
                raise ValueError(f"--sweep {spec!r}: unknown bug {bad[0]!r}")
            grid[field] = words
        elif field == "elect_us":
            pairs = [tuple(int(v, 0) for v in w.split(":")) for w in words]
            if any(len(p) != 2 or p[1] <= p[0] for p in pairs):
                raise ValueError(f"--sweep {spec!r}: want lo:hi pairs with lo < hi")
            grid[field] = pairs
        else:
            grid[field] = [int(w, 0) for w in words]
    return grid


def sweep_line(r):
    """One setting of a sweep as the command line reports it."""
    cnt = r["counters"]
    failing = (r["codes"] != _abi.MR_PASS).nonzero()[0]
    return {"params": r["params"], "passed": cnt["passed"], "failed": cnt["failed"],
            "fail_hist": cnt["fail_hist"],  # (the non-zero verdict counts by name, PASS among them)
            "first_fail_seed": r["seeds"][int(failing[0])] if failing.size else None}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("test")
    ap.add_argument("--clusters", type=int, default=None, help="seeds (MADSIM_TEST_NUM)")
    ap.add_argument("--seed", type=int, default=None, help="first seed (MADSIM_TEST_SEED)")
    ap.add_argument("--seeds", type=parse_seeds, default=None, metavar="LIST",
                    help="run exactly these seeds in one batch: S1,S2,... or @file (one per line); "
                         "with --shrink, shrink them")
    ap.add_argument("--nodes", type=int, default=None)
    ap.add_argument("--iters", type=int, default=0)
    ap.add_argument("--unreliable", action="store_true")
    ap.add_argument("--null", action="store_true", help="skeleton node (never campaigns)")
    ap.add_argument("--safety", action="store_true",
                    help="per-event Raft invariant checks (docs/SEMANTICS.md §11)")
    ap.add_argument("--bug", choices=["vote_twice", "vote_stale", "no_prev_check"],
                    help="run a known-buggy Raft variant")
    ap.add_argument("--replay", metavar="LOG", help="JSON-lines decision log (trace.py) to replay")
    ap.add_argument("--shrink", action="store_true",
                    help="shrink the failing --seed to the faults that cause it (shrink.py)")
    ap.add_argument("--shrink-kinds", default="drop", metavar="KINDS",
                    help="fault kinds to shrink, comma-separated: drop, delay (default drop)")
    ap.add_argument("--shrink-tape", metavar="LOG",
                    help="with --shrink: write the minimal run's whole tape as a --replay log")
    ap.add_argument("--shrink-failures", type=int, nargs="?", const=16, default=None, metavar="K",
                    help="run the --clusters seeds from --seed and shrink the first K failing "
                         "ones together (default 16; 0 = all), one JSON line per seed in --shrink's "
                         "format and a summary line")
    ap.add_argument("--sweep", action="append", default=[], metavar="FIELD=V1,V2,...",
                    help="sweep a setting over the same seeds in one batch (repeatable: every "
                         "combination): hb_us, ae_max, iters, elect_us=lo:hi,..., bug=none,NAME,...")
    ap.add_argument("--fork-at", type=int, default=None, metavar="EVENTS",
                    help="with --futures: run --seed for EVENTS events, then fork that state")
    ap.add_argument("--futures", type=int, default=None, metavar="N",
                    help="with --fork-at: the positions the state is forked into, each continuing "
                         "from its own seed (--seed + position)")
    ap.add_argument("--fork-tape", metavar="LOG",
                    help="with --fork-at: write the prefix's tape as a raw --replay log")
    a = ap.parse_args(argv)
    if (a.fork_at is None) != (a.futures is None):
        ap.error("--fork-at and --futures go together")
    if a.fork_at is not None and (a.replay or a.shrink or a.shrink_failures is not None or a.sweep
                                  or a.seeds):
        ap.error("--fork-at does not go with --replay, --shrink, --shrink-failures, --sweep or --seeds")
    grid = None
    if a.sweep:
        if a.replay or a.shrink or a.shrink_failures is not None:
            ap.error("--sweep does not go with --replay, --shrink or --shrink-failures: shrink a "
                     "failing (seed, setting) by passing that setting batch-wide")
        try:
            grid = parse_sweep(a.sweep)
        except ValueError as e:
            ap.error(str(e))
    flags = 0
    if a.bug:
        flags |= {"vote_twice": _abi.MR_F_BUG_VOTE_TWICE, "vote_stale": _abi.MR_F_BUG_VOTE_STALE,
                  "no_prev_check": _abi.MR_F_BUG_NO_PREV_CHECK}[a.bug]
    if a.replay:
        dec = trace.load_jsonl(a.replay, unreliable=net_mode(a.test, a.unreliable))
        tr, code, tm, misses = sim.replay(a.test, dec, seed=a.seed or _abi.README_SEED,
                                          nodes=a.nodes, iters=a.iters, unreliable=a.unreliable,
                                          null_raft=a.null, safety=a.safety, flags=flags)
        print(json.dumps({"code": code, "verdict": _abi.FAIL_NAMES.get(code, str(code)),
                          "time_us": tm, "events": int(tr.size), "misses": misses}))
        raise SystemExit(0 if code == _abi.MR_PASS else 1)
    cfg_kw = dict(nodes=a.nodes, iters=a.iters, unreliable=a.unreliable, null_raft=a.null,
                  safety=a.safety, flags=flags)

    def shrunk_line(seed, r):
        # the kept decisions as --replay lines: decoded where the test's sends have one network
        # mode, else as raw draw words
        mode = net_mode(a.test, a.unreliable)
        kept = trace.events_from_decisions(r.kept, unreliable=bool(mode), raw=mode is None)
        return json.dumps({"code": r.code, "verdict": _abi.FAIL_NAMES.get(r.code, str(r.code)),
                           "seed": seed, "kind": r.kind, "faults_before": r.faults,
                           "faults_after": int(r.kept.size), "rounds": r.rounds,
                           "candidates": r.candidates, "events": int(r.trace.size), "kept": kept})

    if a.shrink or a.shrink_failures is not None:
        # --shrink: the seed itself; else the N seeds' verdicts and the first K failing ones.
        # Either way the chosen seeds are shrunk together (shrink_seeds)
        seed = _abi.README_SEED if a.seed is None else a.seed
        chosen = [seed]
        if a.shrink and a.seeds:  # (shrink_seeds wants its first seed to be the smallest)
            chosen = sorted(a.seeds)
        elif not a.shrink:
            with sim.Batch(a.test, a.clusters or 1, seed, **cfg_kw) as b:
                b.run()
                code = b.verdicts()[0]
            failing = [seed + int(k) for k in (code != _abi.MR_PASS).nonzero()[0]]
            chosen = failing[: a.shrink_failures] if a.shrink_failures else failing
        res = shrink.shrink_seeds(a.test, chosen, kinds=tuple(a.shrink_kinds.split(",")), **cfg_kw)
        done = [r for r in res.results if not isinstance(r, str)]
        if a.seeds and a.shrink:  # one line per seed, in the order given
            by_seed = dict(zip(chosen, res.results))
            for s in a.seeds:
                r = by_seed[s]
                print(json.dumps({"seed": s, "skipped": r}) if isinstance(r, str) else shrunk_line(s, r))
            raise SystemExit(0)
        if a.shrink and not done:
            raise sim.SimError(res.results[0].error)
        if a.shrink and a.shrink_tape:
            trace.dump_jsonl(a.shrink_tape, done[0].tape, raw=True)
        for s, r in zip(chosen, res.results):
            print(json.dumps({"seed": s, "skipped": r}) if isinstance(r, str) else shrunk_line(s, r))
        if not a.shrink:
            print(json.dumps({"seeds": int(code.size), "failing": len(failing), "shrunk": len(done),
                              "launches": res.launches,
                              "kept_sizes": sorted({int(r.kept.size) for r in done})}))
        raise SystemExit(0)
    if a.fork_at is not None:
        seed = _abi.README_SEED if a.seed is None else a.seed
        r = sim.run_futures(a.test, seed, a.fork_at, a.futures, **cfg_kw)
        if a.fork_tape:
            trace.dump_jsonl(a.fork_tape, r["prefix"], raw=True)
        cnt = r["counters"]
        print(json.dumps({"seed": seed, "fork_at": a.fork_at, "futures": a.futures,
                          "prefix_decisions": int(r["prefix"].size), "kernel": r["kernel"],
                          "passed": cnt["passed"], "failed": cnt["failed"],
                          "fail_hist": cnt["fail_hist"]}))
        extra = "".join(f", {k}={v!r}" for k, v in cfg_kw.items() if v)
        for c in (r["codes"] != _abi.MR_PASS).nonzero()[0]:
            print(json.dumps({"position": int(c), "code": int(r["codes"][c]),
                              "verdict": _abi.FAIL_NAMES.get(int(r["codes"][c]), str(r["codes"][c])),
                              "time_us": int(r["times_us"][c]),
                              "replay": f"sim.replay({a.test!r}, prefix, seed={seed}, "
                                        f"cluster_base={int(c)}{extra})"}))
        raise SystemExit(1 if cnt["failed"] else 0)
    if grid:
        seeds = a.seeds or [(_abi.README_SEED if a.seed is None else a.seed) + k
                            for k in range(a.clusters or 1)]
        res = sim.run_sweep(a.test, grid, seeds=seeds, **cfg_kw)
        for r in res:
            print(json.dumps(sweep_line(r)))
        raise SystemExit(1 if any(r["counters"]["failed"] for r in res) else 0)
    t0 = time.time()
    if a.seeds:
        code, _, _, cnt = sim.run_seeds(a.test, a.seeds, **cfg_kw)
    else:
        code, _, _, cnt = sim.run_test(a.test, a.seed, a.clusters, nodes=a.nodes, iters=a.iters,
                                       unreliable=a.unreliable, null_raft=a.null, safety=a.safety,
                                       flags=flags)
    cnt["wall_s"] = time.time() - t0
    print(json.dumps(cnt))
    raise SystemExit(0 if cnt["failed"] == 0 else 1)


if __name__ == "__main__":
    main()
