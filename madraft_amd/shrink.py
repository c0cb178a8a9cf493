"""Shrink a failing seed to the faults that cause it (docs/SEMANTICS.md §12.1).

A recorded run is a set of keyed decisions. Some of them are faults: a dropped message, a
long latency. An edit takes one fault away (the message is delivered, the latency is 1 ms);
a candidate is the set of faults it keeps, every other fault edited away. `shrink` is delta
debugging (ddmin, Zeller & Hildebrandt 2002) over such sets with every round's candidates
evaluated at once. ddmin is a resumable walk; `shrink_many` drives one walk per failing seed in
lockstep, and `shrink_seeds` evaluates a joint round as one run of a variant batch of groups on
the GPU (`Batch.set_variant_groups`, §12.2): per seed one base tape and one mask row per
candidate. `shrink_seed` is its one-seed case.
"""
import collections

import numpy as np

from . import _abi
from ._abi import DECISION_DTYPE, LOSS_Q32, MR_DS_NET

KINDS = ("drop", "delay")

Shrunk = collections.namedtuple("Shrunk", "kept rounds candidates")
ShrunkSeed = collections.namedtuple(
    "ShrunkSeed", "kept kind code trace tape faults rounds candidates")


def max_candidates(n_faults):
    """The most candidates one `evaluate` call of shrink(.., n_faults, ..) submits."""
    return max(2, 2 * n_faults)


def shrink(evaluate, n_faults, target):
    """A 1-minimal subset of the faults 0..n_faults-1 that still fails.

    `evaluate(keep)` takes a bool array [candidates, n_faults] (row = the faults a candidate
    keeps) and returns one verdict code per row; a candidate fails when its code == target.
    The result is a function of those verdicts alone, by this policy:

    1. The first call submits the empty set and the full set, in that order. If the empty set
       fails the result is empty; if the full set does not fail, ValueError.
    2. Then ddmin on the current set (at first all faults, ascending) at granularity g (at first
       2): the set is cut into g contiguous chunks whose sizes differ by at most one, the larger
       first. One call submits the g chunks and then, where g > 2, the g complements (the set
       without chunk 0, without chunk 1, ...). The first failing candidate in that order
       becomes the current set: after a chunk g = 2, after a complement g = max(g - 1, 2).
       If none fails, g doubles (at most the set's size); if g was the set's size already, the
       round was the single-removal check — no chunk of one fault and no set with one fault
       removed fails — and the set is 1-minimal: done. A set of one fault is 1-minimal by
       step 1.

    Returns Shrunk(kept: ascending indices, rounds: evaluate calls, candidates: rows submitted).
    """
    return drive(shrink_walk(n_faults, target), evaluate)


def drive(walk, evaluate):
    """Run one resumable walk (shrink_walk, passes_walk) to its end: every array it yields goes
    to `evaluate`, whose verdict codes it receives; the walk's return value."""
    rows, done = _advance(walk)
    while rows is not None:
        rows, done = _advance(walk, evaluate(rows))
    return done


def _advance(walk, codes=None):
    """One step of a resumable walk: started (codes None) or sent its last round's verdict codes,
    it gives (its next round's rows, None), or at its end (None, its return value)."""
    try:
        return walk.send(codes), None
    except StopIteration as stop:
        return None, stop.value


def shrink_walk(n_faults, target):
    """shrink() as a resumable walk: a generator that yields each round's keep array
    [candidates, n_faults], is sent that round's verdict codes, and returns the Shrunk. The
    policy is shrink()'s; who runs the candidates, and what else runs beside them, is the
    driver's business (drive: one walk; shrink_many: one per seed, in lockstep)."""
    n = int(n_faults)

    def rows(sets):
        keep = np.zeros((len(sets), n), bool)
        for r, s in enumerate(sets):
            keep[r, s] = True
        return keep

    def failing(sets, codes):
        codes = np.asarray(codes)
        assert codes.shape == (len(sets),), codes.shape
        return codes == target

    cur = np.arange(n)
    rounds, cands = 1, 2
    sets = [cur[:0], cur]
    empty_fails, full_fails = failing(sets, (yield rows(sets)))
    if empty_fails:
        return Shrunk(cur[:0], rounds, cands)
    if not full_fails:
        raise ValueError("the run with every fault kept does not fail with the target verdict")
    g = 2
    while cur.size >= 2:
        chunks = np.array_split(cur, g)
        sets = list(chunks)
        if g > 2:
            sets += [np.concatenate(chunks[:i] + chunks[i + 1:]) for i in range(g)]
        rounds += 1
        cands += len(sets)
        hit = np.nonzero(failing(sets, (yield rows(sets))))[0]
        if hit.size:
            cur = sets[hit[0]]
            g = 2 if hit[0] < len(chunks) else max(g - 1, 2)
        elif g < cur.size:
            g = min(2 * g, cur.size)
        else:
            break
    return Shrunk(cur, rounds, cands)


def find_edits(base, kind):
    """(indices into `base`, edits) of one kind: `drop` — a NET record with w0 < LOSS_Q32,
    edited to w0 = 0xFFFFFFFF (delivered, latency kept); `delay` — a NET record that is no
    drop with w1 >= 2^31 (the upper half of the latency range), edited to w1 = 0 (1 ms)."""
    base = np.asarray(base, DECISION_DTYPE)
    net = base["stream"] == MR_DS_NET
    drop = net & (base["w0"] < LOSS_Q32)
    if kind == "drop":
        idx = np.nonzero(drop)[0]
        edits = base[idx].copy()
        edits["w0"] = 0xFFFFFFFF
    elif kind == "delay":
        idx = np.nonzero(net & ~drop & (base["w1"] >= 1 << 31))[0]
        edits = base[idx].copy()
        edits["w1"] = 0
    else:
        raise ValueError(f"unknown edit kind {kind!r} (one of {KINDS})")
    return idx, edits


def apply_edits(base, idx, edits, applied):
    """`base` with edits[j] in place of base[idx[j]] wherever applied[j]: the tape one variant
    replays, for mr_replay or the oracle."""
    out = np.array(base, DECISION_DTYPE)
    applied = np.asarray(applied, bool)
    out[idx[applied]] = edits[applied]
    return out


Passes = collections.namedtuple("Passes", "kind kept applied faults rounds candidates idx edits")


def edit_list(base, kinds):
    """(idx, edits, kind per edit) of every kind in `kinds`, drops before delays: the edits of
    one variant batch. The kinds' records are disjoint, so no key is edited twice."""
    parts = [(k, *find_edits(base, k)) for k in KINDS if k in kinds]
    if not parts or set(kinds) - set(KINDS):
        raise ValueError(f"edit kinds {kinds!r}: some of {KINDS}")
    return (np.concatenate([p[1] for p in parts]), np.concatenate([p[2] for p in parts]),
            np.concatenate([np.full(p[1].size, p[0]) for p in parts]))


def shrink_passes(evaluate_masks, base, kinds, target):
    """The passes of a seed's shrinking over `evaluate_masks(applied[candidates, n_edits]) ->
    codes` (column j = edit j of edit_list(base, kinds)), whatever runs the candidates — a
    variant batch, the oracle. Drops first, with no delay edited; if the empty drop set still
    fails (loss is not the cause) and `kinds` names delays, delays with every drop delivered.

    Returns Passes: the kind that was shrunk last, kept (positions in the edit list of the
    faults that stay), applied (the minimal run's edits), that kind's faults before, evaluate
    calls and candidates over all passes, and the edit list's idx and edits."""
    return drive(passes_walk(base, kinds, target), evaluate_masks)


def passes_walk(base, kinds, target):
    """shrink_passes() as a resumable walk: yields each round's applied array [candidates,
    n_edits], is sent its verdict codes, returns the Passes."""
    idx, edits, kind_of = edit_list(base, kinds)
    fixed = np.zeros(idx.size, bool)  # edits applied in every candidate of the pass
    rounds = cands = 0
    order = [k for k in KINDS if k in kinds]
    for kind in order:
        mine = np.nonzero(kind_of == kind)[0]
        walk = shrink_walk(mine.size, target)
        keep, res = _advance(walk)
        while keep is not None:
            applied = np.tile(fixed, (keep.shape[0], 1))
            applied[:, mine] = ~keep
            keep, res = _advance(walk, (yield applied))
        rounds += res.rounds
        cands += res.candidates
        fixed[mine] = True  # (a kind that is not the cause stays edited away in the next pass)
        if res.kept.size or kind == order[-1]:
            applied = fixed.copy()
            applied[mine[res.kept]] = False
            return Passes(kind, mine[res.kept], applied, mine.size, rounds, cands, idx, edits)


def shrink_many(evaluate_groups, bases, kinds, targets):
    """shrink_passes for several seeds at once: one walk per seed (bases[g], targets[g]), driven
    in lockstep. Each round the live walks' candidates go to one call of
    `evaluate_groups({g: applied[candidates, n_edits of g]}) -> {g: codes}`; a walk that has
    finished is given nothing more. Every walk sees only its own verdicts, so the Passes of seed
    g is what shrink_passes returns for it alone, and the number of evaluate_groups calls is the
    largest rounds among them.

    Returns (list of Passes, evaluate_groups calls)."""
    walks = [passes_walk(b, kinds, t) for b, t in zip(bases, targets)]
    out = [None] * len(walks)
    # (every walk has a first round: the empty and the full set)
    rows = {g: _advance(w)[0] for g, w in enumerate(walks)}
    calls = 0
    while rows:
        codes = evaluate_groups(rows)
        calls += 1
        nxt = {}
        for g in rows:
            nxt[g], out[g] = _advance(walks[g], np.asarray(codes[g]))
        rows = {g: r for g, r in nxt.items() if r is not None}
    return out, calls


def n_variants(base, kinds):
    """Clusters of the variant batch that serves every round of shrink_passes(.., base, kinds)."""
    return max(max_candidates(find_edits(base, k)[0].size) for k in KINDS if k in kinds)


def shrink_seed(test, seed, kinds=("drop",), tape_cap=1 << 16, **cfg_kw):
    """Shrink the failing run of `test` at `seed` (make_cfg's keywords: iters, flags, ...) to a
    1-minimal set of faults of `kinds` on the GPU: shrink_seeds' one-seed case — one record run,
    one variant batch of n_variants(base, kinds) clusters, one launch per ddmin round, one
    replay of the minimal tape. A seed that passes, or draws more than tape_cap decisions, is a
    SimError.

    Returns ShrunkSeed: kept (the base records of the faults that stay, DECISION_DTYPE), their
    kind, the verdict code, the minimal run's trace (mr_replay of its tape), that tape, the
    faults of that kind before, evaluate rounds and candidates run."""
    from . import sim
    r = shrink_seeds(test, [seed], kinds, tape_cap, **cfg_kw).results[0]
    if isinstance(r, str):
        raise sim.SimError(r.error)
    return r


SeedsShrunk = collections.namedtuple("SeedsShrunk", "results launches")


class NotShrunk(str):
    """Why shrink_seeds left a seed alone, "passes" or "tape_cap": a str, with `error`, what
    shrink_seed says of that seed."""

    def __new__(cls, why, error):
        self = super().__new__(cls, why)
        self.error = error
        return self


def _chunks(n, size):
    """range(n) cut into consecutive runs of at most `size` (at least 1) items."""
    size = max(1, int(size))
    return [range(i, min(n, i + size)) for i in range(0, n, size)]


def shrink_seeds(test, seeds, kinds=("drop",), tape_cap=1 << 16, record_bytes=1 << 32, **cfg_kw):
    """Shrink the failing runs of `test` at every seed of `seeds` at once (docs/SEMANTICS.md
    §12.2, §12.3; make_cfg's keywords: iters, flags, ...), each to a 1-minimal set of faults of
    `kinds`, in three batches whatever the number of seeds: every seed is recorded in one
    MR_F_RECORD batch over the seed list (Batch.set_seeds) and read back at once
    (Batch.decisions_all); then one variant batch holds a group per failing seed — group g owns a
    contiguous run of n_variants(its base, kinds) clusters — and every round of shrink_many is one
    set_variant_masks + reset + run of it: the launches are the longest seed's rounds, not their
    sum. The clusters a group's round does not use, and all of a finished group's, repeat its
    candidate 0 and their verdicts are ignored. Every minimal tape is replayed in one batch
    (sim.replay_many) and must give its seed's verdict. Memory stays bounded: a record batch holds
    at most record_bytes // (tape_cap * 16) seeds and a replay batch record_bytes // (trace_cap *
    32) (trace_cap: cfg_kw's, default 2^16), so more seeds than that take several of each.

    Returns SeedsShrunk(results, launches): results[i] is the ShrunkSeed of seeds[i], or, for a
    seed that is not shrunk, the string (NotShrunk) "passes" or "tape_cap" (it drew more than
    tape_cap decisions); launches = runs of the variant batch."""
    from . import sim
    seeds = [int(s) for s in seeds]
    flags = int(cfg_kw.pop("flags", 0))
    base_c = int(cfg_kw.pop("cluster_base", 0))
    results = [None] * len(seeds)
    if not seeds:
        return SeedsShrunk(results, 0)
    seed_base = seeds[0] - base_c  # the variant batch's; group g's seed_cluster = its seed - seeds[0]
    if min(seeds) < seeds[0] or max(seeds) - seeds[0] >= 1 << 32:
        raise sim.SimError("shrink_seeds: seeds[0] must be the smallest, the others within 2^32 of it")
    trace_cap = int(cfg_kw.pop("trace_cap", None) or 1 << 16)
    live, bases, targets = [], [], []
    for chunk in _chunks(len(seeds), int(record_bytes) // (int(tape_cap) * 16)):
        with sim.Batch(test, len(chunk), seed_base, cluster_base=base_c,
                       flags=flags | _abi.MR_F_RECORD, tape_cap=tape_cap, **cfg_kw) as b:
            b.set_seeds([seeds[i] for i in chunk])
            b.run()
            codes = b.verdicts()[0]
            drawn, off, rec = b.decisions_all()
        for k, i in enumerate(chunk):
            code, n = int(codes[k]), int(drawn[k])
            if code == _abi.MR_PASS or n > tape_cap:
                results[i] = NotShrunk(
                    "passes" if code == _abi.MR_PASS else "tape_cap",
                    f"tape_cap {tape_cap} too small: the seed draws {n} decisions" if n > tape_cap
                    else f"seed {seeds[i]} passes {test}: nothing to shrink")
                continue
            base = rec[int(off[k]): int(off[k + 1])].copy()
            base["cluster"] = 0  # (a tape names no position: what a 1-cluster recording gives)
            live.append(i)
            bases.append(base)
            targets.append(code)
    if not live:
        return SeedsShrunk(results, 0)
    lists = [edit_list(bs, kinds) for bs in bases]
    width = [n_variants(bs, kinds) for bs in bases]
    first = np.cumsum([0] + width)  # group g's clusters: first[g] .. first[g + 1]
    clusters, n_edits = int(first[-1]), max(ls[1].size for ls in lists)
    launches = 0
    with sim.Batch(test, clusters, seed_base, cluster_base=base_c, flags=flags, **cfg_kw) as b:
        b.set_variant_groups([(seeds[i] - seeds[0], bs, ls[1])
                              for i, bs, ls in zip(live, bases, lists)],
                             np.repeat(np.arange(len(live)), width))
        masks = np.zeros((clusters, n_edits), bool)

        def evaluate_groups(rows):
            nonlocal launches
            for g in range(len(live)):
                m = masks[first[g]: first[g + 1]]
                if g in rows:
                    applied = rows[g]
                    m[: applied.shape[0], : applied.shape[1]] = applied
                    m[applied.shape[0]:] = m[0]
                else:  # finished: candidate 0 of its last round in every row
                    m[1:] = m[0]
            b.set_variant_masks(masks)
            b.reset(seed_base)
            st = b.run()
            assert st["remaining"] == 0, st
            launches += 1
            code = b.verdicts()[0]
            return {g: code[first[g]: first[g] + applied.shape[0]] for g, applied in rows.items()}

        passes, _ = shrink_many(evaluate_groups, bases, kinds, targets)
    tapes = [apply_edits(bs, p.idx, p.edits, p.applied) for bs, p in zip(bases, passes)]
    for chunk in _chunks(len(live), int(record_bytes) // (trace_cap * 32)):
        played = sim.replay_many(test, [tapes[g] for g in chunk], [seeds[live[g]] for g in chunk],
                                 trace_cap=trace_cap, cluster_base=base_c, flags=flags, **cfg_kw)
        for g, (tr, code, _, _) in zip(chunk, played):
            i, bs, target, p = live[g], bases[g], targets[g], passes[g]
            if code != target:
                raise sim.SimError(f"seed {seeds[i]}: the minimal tape replays to verdict {code}, "
                                   f"not {target}")
            results[i] = ShrunkSeed(bs[p.idx[p.kept]], p.kind, target, tr, tapes[g], p.faults,
                                    p.rounds, p.candidates)
    return SeedsShrunk(results, launches)
