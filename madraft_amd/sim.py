"""Host API of the MI355X batched Raft simulator (binds libmadraft_hip.so).

Mirrors the reference's test-harness interface for the hot path: a test is
named as in src/raft/tests.rs, seeds are chosen like MADSIM_TEST_SEED /
MADSIM_TEST_NUM (README.md:44-66), and a failing seed is reported with the
tester's panic message (src/raft/tester.rs) and "MADSIM_TEST_SEED=<seed>".
One `Batch` = many independent seeds of one test, run in lockstep on one GPU.

There is no CPU fallback: if the HIP library is missing this module raises.
"""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import DECISION_DTYPE, EVENT_DTYPE, FAIL_NAMES, MrCfg, MrCounters, MrRunStats

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MADRAFT_HIP_LIB") or os.path.join(_HERE, "lib", "libmadraft_hip.so")
_lib = None


def lib():
    """Load libmadraft_hip.so (built in-tree by __graft_entry__.build())."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"HIP library {LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; "
            "g.build()'` (there is no CPU fallback)")
    L = C.CDLL(LIB_PATH)
    L.mr_last_error.restype = C.c_char_p
    L.mr_fail_message.restype = C.c_char_p
    L.mr_fail_message.argtypes = [C.c_uint32]
    L.mr_scenario_name.restype = C.c_char_p
    L.mr_scenario_name.argtypes = [C.c_uint32]
    L.mr_scenario_from_name.restype = C.c_uint32
    L.mr_scenario_from_name.argtypes = [C.c_char_p]
    L.mr_cfg_init.argtypes = [C.POINTER(MrCfg), C.c_uint32]
    L.mr_batch_create.argtypes = [C.POINTER(MrCfg), C.POINTER(C.c_void_p)]
    L.mr_batch_reset.argtypes = [C.c_void_p, C.c_uint64]
    L.mr_batch_run.argtypes = [C.c_void_p, C.c_uint64, C.POINTER(MrRunStats)]
    L.mr_batch_submit.argtypes = [C.c_void_p, C.c_uint64]
    L.mr_batch_finish.argtypes = [C.c_void_p, C.POINTER(MrRunStats), C.POINTER(MrCounters)]
    L.mr_batch_verdicts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mr_batch_counters.argtypes = [C.c_void_p, C.POINTER(MrCounters)]
    L.mr_trace_get.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                               C.POINTER(C.c_size_t)]
    L.mr_trace_digests.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]
    L.mr_trace_applies.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                   C.POINTER(C.c_size_t)]
    L.mr_batch_kernel.argtypes = [C.c_void_p]
    L.mr_batch_kernel.restype = C.c_char_p
    L.mr_batch_set_decisions.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t]
    L.mr_batch_get_decisions.argtypes = [C.c_void_p, C.c_uint32, C.c_void_p, C.c_size_t,
                                         C.POINTER(C.c_size_t)]
    L.mr_batch_set_variants.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_size_t, C.c_void_p]
    L.mr_batch_set_variant_masks.argtypes = [C.c_void_p, C.c_void_p]
    L.mr_batch_set_variant_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_size_t, C.c_void_p, C.c_size_t, C.c_void_p,
                                              C.c_void_p]
    L.mr_batch_set_seeds.argtypes = [C.c_void_p, C.c_void_p]
    L.mr_batch_set_param_groups.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.mr_batch_group_counters.argtypes = [C.c_void_p, C.c_uint32, C.POINTER(MrCounters)]
    L.mr_batch_get_decisions_packed.argtypes = [C.c_void_p, C.c_uint32, C.c_uint32, C.c_void_p,
                                                C.c_void_p, C.c_void_p, C.c_size_t]
    L.mr_batch_fork.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    L.mr_batch_fork_ms.argtypes = [C.c_void_p, C.POINTER(C.c_float)]
    L.mr_decision_word.argtypes = [C.c_uint32, C.c_uint32, C.c_uint32]
    L.mr_decision_word.restype = C.c_uint32
    L.mr_replay.argtypes = [C.POINTER(MrCfg), C.c_void_p, C.c_size_t, C.c_void_p, C.c_size_t,
                            C.POINTER(C.c_size_t), C.POINTER(C.c_uint16), C.POINTER(C.c_uint32),
                            C.POINTER(C.c_uint64)]
    L.mr_batch_destroy.argtypes = [C.c_void_p]
    L.mr_batch_destroy.restype = None
    _lib = L
    return L


def lib_sha16(path=None):
    """First 16 hex digits of the SHA-256 of the product library file (the build a
    measurement was taken with: bench.py's JSON line and profiles/pmc_*.json carry it)."""
    import hashlib
    h = hashlib.sha256()
    with open(path or LIB_PATH, "rb") as f:
        for blk in iter(lambda: f.read(1 << 20), b""):
            h.update(blk)
    return h.hexdigest()[:16]


class SimError(RuntimeError):
    pass


def _check(rc):
    if rc != 0:
        raise SimError(lib().mr_last_error().decode())


def fail_message(code):
    return lib().mr_fail_message(int(code)).decode()


def make_cfg(test, clusters=1, seed=_abi.README_SEED, *, nodes=None, iters=0, unreliable=False,
             null_raft=False, trace_clusters=0, trace_cap=None, cluster_base=0, device=0,
             safety=False, stream=False, **overrides):
    """mr_cfg for `test` with the reference's defaults (mr_cfg_init) plus overrides."""
    scn = _abi.SCENARIO_ID.get(test)
    if scn is None:
        raise SimError(f"unknown test {test!r}")
    cfg = MrCfg()
    _check(lib().mr_cfg_init(C.byref(cfg), scn))
    cfg.n_clusters = int(clusters)
    cfg.seed_base = int(seed)
    cfg.cluster_base = int(cluster_base)
    cfg.iters = int(iters)
    cfg.device = int(device)
    if nodes:
        cfg.n_nodes = int(nodes)
        if nodes > 5 and "msg_slots" not in overrides:
            cfg.msg_slots = 64  # 7-node elections peak at ~30 in flight
    if unreliable:
        cfg.flags |= _abi.MR_F_UNRELIABLE
    if null_raft:
        cfg.flags |= _abi.MR_F_NULL_RAFT
    if safety:
        cfg.flags |= _abi.MR_F_SAFETY
    if stream:
        cfg.flags |= _abi.MR_F_STREAM
    if trace_clusters:
        cfg.flags |= _abi.MR_F_TRACE
        cfg.trace_clusters = int(trace_clusters)
        if trace_cap:
            cfg.trace_cap = int(trace_cap)
    cfg.flags |= int(overrides.pop("flags", 0))  # extra MR_F_* bits (SAFETY, BUG_*)
    for k, v in overrides.items():
        setattr(cfg, k, int(v))
    return cfg


def _ptr(a):
    """The address of array `a` for a C call; NULL for None or an empty array."""
    return a.ctypes.data if a is not None and a.size else None


def _records(d):
    """(array, its _ptr) of keyed decisions for a C call: `d` (records or None) as one flat
    contiguous DECISION_DTYPE array."""
    a = np.ascontiguousarray(d if d is not None else [], dtype=DECISION_DTYPE).ravel()
    return a, _ptr(a)


def seed_offsets(seeds, seed_base, cluster_base=0):
    """The seed list of mr_batch_set_seeds for the absolute `seeds`: uint32 offsets from seed_base +
    cluster_base (docs/SEMANTICS.md §12.3). A seed below that base, or 2^32 or more above it, is a
    SimError."""
    base = int(seed_base) + int(cluster_base)
    off = [int(s) - base for s in seeds]
    for s, o in zip(seeds, off):
        if not 0 <= o < 1 << 32:
            raise SimError(f"seed {int(s)} is not within [0, 2^32) of the base {base} "
                           f"(seed_base {int(seed_base)} + cluster_base {int(cluster_base)})")
    return np.array(off, np.uint32)


def param_group_records(groups):
    """PARAM_GROUP_DTYPE records of a list of dicts with mr_param_group's field names (None: none)."""
    names = set(_abi.PARAM_GROUP_DTYPE.names) - {"reserved"}
    g = np.zeros(len(groups or []), _abi.PARAM_GROUP_DTYPE)
    for i, d in enumerate(groups or []):
        if set(d) - names:
            raise SimError(f"parameter group {i}: unknown field(s) {sorted(set(d) - names)}")
        for k, v in d.items():
            g[i][k] = int(v)
    return g


class Batch:
    """`clusters` seeds of one reference test, resident on one GPU."""

    def __init__(self, test=None, clusters=1, seed=_abi.README_SEED, *, cfg=None, **kw):
        self.cfg = cfg if cfg is not None else make_cfg(test, clusters, seed, **kw)
        self._b = C.c_void_p()
        self._n_edits = 0  # edits of the variants set (set_variants)
        _check(lib().mr_batch_create(C.byref(self.cfg), C.byref(self._b)))

    @property
    def clusters(self):
        return int(self.cfg.n_clusters)

    def close(self):
        if self._b:
            lib().mr_batch_destroy(self._b)
            self._b = C.c_void_p()

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    def reset(self, seed_base):
        self.cfg.seed_base = int(seed_base)
        _check(lib().mr_batch_reset(self._b, int(seed_base)))

    def run(self, max_events=0):
        st = MrRunStats()
        _check(lib().mr_batch_run(self._b, int(max_events), C.byref(st)))
        return {n: getattr(st, n) for n, _ in MrRunStats._fields_}

    def submit(self, seed_base):
        """reset(seed_base) + run()'s first launch, enqueued without waiting (mr_batch_submit);
        finish() completes it. Another batch's step can be submitted in between."""
        self.cfg.seed_base = int(seed_base)
        _check(lib().mr_batch_submit(self._b, int(seed_base)))

    def finish(self):
        """(run stats, counters) of the submitted step (mr_batch_finish)."""
        st, c = MrRunStats(), MrCounters()
        _check(lib().mr_batch_finish(self._b, C.byref(st), C.byref(c)))
        return {n: getattr(st, n) for n, _ in MrRunStats._fields_}, c.to_dict()

    def verdicts(self):
        n = self.clusters
        code = np.empty(n, np.uint16)
        t = np.empty(n, np.uint32)
        dig = np.empty(n, np.uint64)
        _check(lib().mr_batch_verdicts(self._b, code.ctypes.data, t.ctypes.data,
                                       dig.ctypes.data))
        return code, t, dig

    def counters(self):
        c = MrCounters()
        _check(lib().mr_batch_counters(self._b, C.byref(c)))
        return c.to_dict()

    def set_seeds(self, seeds):
        """Position c runs the absolute seed seeds[c] (mr_batch_set_seeds; any order, duplicates
        allowed, each within 2^32 above seed_base + cluster_base); None = seed c again. The list
        stays through reset() (the same offsets from the new base) and set_decisions()."""
        off = None
        if seeds is not None:
            off = seed_offsets(seeds, self.cfg.seed_base, self.cfg.cluster_base)
            if off.shape != (self.clusters,):
                raise SimError(f"seeds: shape {off.shape}, not ({self.clusters},)")
        _check(lib().mr_batch_set_seeds(self._b, off.ctypes.data if off is not None else None))

    def set_param_groups(self, groups, group_of=None):
        """Position c runs under the settings of groups[group_of[c]] (mr_batch_set_param_groups;
        docs/SEMANTICS.md §12.4): `groups` is a list of dicts with mr_param_group's field names
        (flags, hb_us, elect_lo_us, elect_hi_us, ae_max, iters; a missing or zero number = the
        batch's, `flags` = the group's SWEEPABLE_FLAGS bits, which replace the batch's). None or
        empty = the batch's cfg everywhere again. The groups stay through reset(), set_seeds() and
        every set_decisions() / set_variants*()."""
        g = param_group_records(groups)
        of = None
        if g.size:
            of = np.ascontiguousarray(group_of, dtype=np.uint32)
            if of.shape != (self.clusters,):
                raise SimError(f"group_of: shape {of.shape}, not ({self.clusters},)")
        _check(lib().mr_batch_set_param_groups(self._b, _ptr(g), g.size, _ptr(of)))

    def group_counters(self, g):
        """counters() restricted to the positions of parameter group g (mr_batch_group_counters)."""
        c = MrCounters()
        _check(lib().mr_batch_group_counters(self._b, int(g), C.byref(c)))
        return c.to_dict()

    def _set_tables(self, rc, n_edits=0):
        """After a call that replaces or drops the decision tables: `n_edits` = the mask columns
        of the variants now set (0: none; any earlier variants went with the tables)."""
        _check(rc)
        self._n_edits = int(n_edits)

    def set_decisions(self, d):
        """Drive the clusters by keyed decisions (DECISION_DTYPE records, any order;
        SEMANTICS §12); None = Philox again. Call before run()."""
        a, pa = _records(d)
        self._set_tables(lib().mr_batch_set_decisions(self._b, pa, a.size))

    def _mask_words(self, masks, n_edits):
        """[clusters, ceil(n_edits / 32)] uint32 mask rows from a bool array [clusters, n_edits]
        (True = the cluster applies the edit) or from rows already packed; None stays None."""
        if masks is None:
            return None
        m = np.asarray(masks)
        w = (n_edits + 31) // 32
        if m.dtype == np.bool_:
            if m.shape != (self.clusters, n_edits):
                raise SimError(f"masks: shape {m.shape}, not ({self.clusters}, {n_edits})")
            bits = np.zeros((self.clusters, w * 32), np.uint8)
            bits[:, :n_edits] = m
            m = np.packbits(bits, axis=1, bitorder="little").view("<u4")
        m = np.ascontiguousarray(m, dtype=np.uint32)
        if m.shape != (self.clusters, w):
            raise SimError(f"masks: shape {m.shape}, not ({self.clusters}, {w})")
        return m

    def set_variants(self, base, edits=None, masks=None):
        """Make every cluster a variant of cluster 0's seed (mr_batch_set_variants; SEMANTICS
        §12.1): `base` decisions shared by all, `edits` that replace the words of base records,
        `masks` [clusters, len(edits)] bool (or packed uint32 rows) saying which cluster applies
        which edit (None: none). base None or empty = Philox again."""
        a, pa = _records(base)
        e, pe = _records(edits if a.size else None)
        m = self._mask_words(masks if a.size else None, e.size)
        self._set_tables(lib().mr_batch_set_variants(self._b, pa, a.size, pe, e.size, _ptr(m)),
                         e.size)

    def set_variant_groups(self, groups, group_of, masks=None):
        """Make cluster c a variant of group group_of[c]'s seed (mr_batch_set_variant_groups;
        SEMANTICS §12.2). `groups` is a list of (seed_cluster, base, edits): the group's runs are
        runs of the seed seed_base + cluster_base + seed_cluster, replay its `base` decisions and
        apply `edits` (None: none) of it; `masks` [clusters, max_edits] bool, or packed uint32
        rows, column j = edit j of the cluster's own group (max_edits = the widest group's edits;
        None: no cluster applies any). No groups = Philox again."""
        groups = [(int(s), _records(b)[0], _records(e)[0]) for s, b, e in groups or []]
        g = np.zeros(len(groups), _abi.VARIANT_GROUP_DTYPE)
        g["seed_cluster"] = [s for s, _, _ in groups]
        g["n_base"] = [b.size for _, b, _ in groups]
        g["n_edits"] = [e.size for _, _, e in groups]
        g["base_off"] = np.cumsum(g["n_base"], dtype=np.uint64) - g["n_base"]
        g["edit_off"] = np.cumsum(g["n_edits"], dtype=np.uint64) - g["n_edits"]
        a, pa = _records(np.concatenate([b for _, b, _ in groups]) if groups else None)
        e, pe = _records(np.concatenate([e for _, _, e in groups]) if groups else None)
        widest = int(g["n_edits"].max(initial=0))
        of = m = None
        if groups:
            of = np.ascontiguousarray(group_of, dtype=np.uint32)
            if of.shape != (self.clusters,):
                raise SimError(f"group_of: shape {of.shape}, not ({self.clusters},)")
            m = self._mask_words(masks, widest)
        self._set_tables(lib().mr_batch_set_variant_groups(
            self._b, _ptr(g), g.size, pa, a.size, pe, e.size, _ptr(of), _ptr(m)), widest)

    def set_variant_masks(self, masks):
        """New masks for the variants set (mr_batch_set_variant_masks), [clusters, edits] bool or
        packed rows (a grouped batch: edits = the widest group's); then reset() and run()."""
        m = self._mask_words(masks, self._n_edits)
        _check(lib().mr_batch_set_variant_masks(self._b, _ptr(m)))

    def decisions(self, k, cap=1 << 20):
        """(n, records): with MR_F_RECORD cluster k's decisions in draw order (n drawn);
        with decisions set, n = its draws that found no record."""
        out = np.empty(cap, DECISION_DTYPE)
        n = C.c_size_t()
        _check(lib().mr_batch_get_decisions(self._b, int(k), out.ctypes.data, cap, C.byref(n)))
        return int(n.value), out[: min(n.value, cap)]

    def decisions_all(self, first=0, count=None):
        """(drawn, off, records) of clusters [first, first + count) in one read-back
        (mr_batch_get_decisions_packed): drawn[i] = decisions cluster first + i drew (with decisions
        set: its misses), records[off[i]: off[i + 1]] = those MR_F_RECORD kept, min(drawn, tape_cap)
        of them in draw order, cluster = the batch position."""
        count = self.clusters - int(first) if count is None else int(count)
        drawn = np.zeros(count, np.uint64)
        off = np.zeros(count + 1, np.uint64)
        f = lib().mr_batch_get_decisions_packed
        _check(f(self._b, int(first), count, _ptr(drawn), off.ctypes.data, None, 0))
        rec = np.empty(int(off[-1]), DECISION_DTYPE)
        if rec.size:
            _check(f(self._b, int(first), count, _ptr(drawn), off.ctypes.data, rec.ctypes.data,
                     rec.size))
        return drawn, off, rec

    def fork(self, src_of, src=None):
        """Position c becomes a copy of position src_of[c] of batch `src` (None: this batch) as that
        cluster stands now; _abi.FORK_SKIP leaves c as it is (mr_batch_fork; docs/SEMANTICS.md
        §12.5). Its later draws follow c's own rule here, so its whole run equals the run of c's
        seed with the source's decisions so far set as keyed decisions."""
        of = np.ascontiguousarray(src_of, dtype=np.uint32)
        if of.shape != (self.clusters,):
            raise SimError(f"src_of: shape {of.shape}, not ({self.clusters},)")
        _check(lib().mr_batch_fork(self._b, (src or self)._b, of.ctypes.data))

    def fork_ms(self):
        """Device time of this batch's last fork (mr_batch_fork_ms), before its next launch."""
        ms = C.c_float()
        _check(lib().mr_batch_fork_ms(self._b, C.byref(ms)))
        return float(ms.value)

    def trace(self, k, cap=None):
        cap = cap or int(self.cfg.trace_cap)
        out = np.empty(cap, EVENT_DTYPE)
        n = C.c_size_t()
        _check(lib().mr_trace_get(self._b, int(k), out.ctypes.data, cap, C.byref(n)))
        return out[: n.value]

    def trace_digests(self, k, cap=None):
        """mr_trace_digests: per record of trace(k), its node's apply digest (ABI 4)."""
        cap = cap or int(self.cfg.trace_cap)
        out = np.empty(cap, np.uint64)
        n = C.c_size_t()
        _check(lib().mr_trace_digests(self._b, int(k), out.ctypes.data, cap, C.byref(n)))
        return out[: n.value]

    def trace_applies(self, k, cap=None):
        """mr_trace_applies: [n, 2] (command, key hash after it) per log index (ABI 4)."""
        cap = cap or int(self.cfg.trace_cap)
        out = np.zeros((cap, 2), np.uint64)
        n = C.c_size_t()
        _check(lib().mr_trace_applies(self._b, int(k), out.ctypes.data, cap, C.byref(n)))
        return out[: n.value]

    @property
    def kernel(self):
        """mr_batch_kernel: "pool_kernel", "step_kernel" or "step_kernel_tape" (decisions,
        variants, a seed list or recording)."""
        return lib().mr_batch_kernel(self._b).decode()


def replay(test, decisions, trace_cap=1 << 16, cluster_base=0, **kw):
    """mr_replay: one cluster of `test` driven by keyed decisions (DECISION_DTYPE records,
    any order): (per-event trace, verdict code, verdict time, draws without a record)."""
    cfg = make_cfg(test, 1, cluster_base=cluster_base, **kw)
    d, pd = _records(decisions)
    out = np.empty(trace_cap, EVENT_DTYPE)
    n, code, tm, ms = C.c_size_t(), C.c_uint16(), C.c_uint32(), C.c_uint64()
    _check(lib().mr_replay(C.byref(cfg), pd, d.size,
                           out.ctypes.data, trace_cap, C.byref(n), C.byref(code), C.byref(tm),
                           C.byref(ms)))
    return out[: n.value], int(code.value), int(tm.value), int(ms.value)


# a key no draw has (mr_replay's): a cluster with this one record replays an empty tape, every draw
# a counted miss
_NO_DRAW = (_abi.MR_DS_TESTER, 0xFFFF, 0xFFFFFFFF, 0, 0)


def replay_many(test, tapes, seeds, trace_cap=1 << 16, **kw):
    """replay() of tapes[i] at the absolute seed seeds[i], for every i in one batch: position i
    runs seeds[i] (set_seeds) driven by tapes[i] (one set_decisions, cluster = position) and keeps
    a trace. A list of (trace, code, time_us, misses), element i what
    replay(test, tapes[i], seed=seeds[i] - cluster_base, ...) returns."""
    seeds = [int(s) for s in seeds]
    if len(tapes) != len(seeds):
        raise SimError(f"replay_many: {len(tapes)} tapes for {len(seeds)} seeds")
    if not seeds:
        return []
    kw = dict(kw)
    kw.pop("seed", None)
    base_c = int(kw.pop("cluster_base", 0))
    flags = int(kw.pop("flags", 0)) & ~_abi.MR_F_RECORD
    rows = []
    for i, t in enumerate(tapes):
        d = np.array(_records(t)[0])
        if not d.size:
            d = np.zeros(1, DECISION_DTYPE)
            d[0] = (0,) + _NO_DRAW
        d["cluster"] = i
        rows.append(d)
    with Batch(test, len(seeds), min(seeds) - base_c, cluster_base=base_c, flags=flags,
               trace_clusters=len(seeds), trace_cap=trace_cap, **kw) as b:
        b.set_seeds(seeds)
        b.set_decisions(np.concatenate(rows))
        b.run()
        code, tm, _ = b.verdicts()
        misses = b.decisions_all()[0]
        return [(b.trace(i, trace_cap), int(code[i]), int(tm[i]), int(misses[i]))
                for i in range(len(seeds))]


def _print_failures(test, code, t, seed_of):
    """The first failures like the #[madsim::test] harness (README.md:44-48); seed_of(k) = the seed
    position k ran."""
    for k in np.nonzero(code != _abi.MR_PASS)[0][:3]:
        print(f"---- {test} ----\npanicked at '{fail_message(code[k])}' "
              f"({FAIL_NAMES.get(int(code[k]), code[k])}, t={t[k] * 1e-6:.3f}s)\n"
              f"MADSIM_TEST_SEED={seed_of(int(k))}")


def run_seeds(test, seeds, **kw):
    """run_test for a list of absolute seeds: one batch of len(seeds) clusters with seed_base =
    min(seeds) - cluster_base, position i running seeds[i] (set_seeds). Returns (codes, times_us,
    digests, counters) by position; failures are printed with their own MADSIM_TEST_SEED."""
    seeds = [int(s) for s in seeds]
    if not seeds:
        raise SimError("run_seeds: no seeds")
    base_c = int(kw.pop("cluster_base", 0))
    with Batch(test, len(seeds), min(seeds) - base_c, cluster_base=base_c, **kw) as b:
        b.set_seeds(seeds)
        b.run()
        code, t, dig = b.verdicts()
        cnt = b.counters()
    _print_failures(test, code, t, lambda k: seeds[k])
    return code, t, dig, cnt


def run_futures(test, seed, at_events, futures, **kw):
    """`futures` different continuations of one run of `seed`, from its state after `at_events`
    events (docs/SEMANTICS.md §12.5). The seed is recorded up to there in a one-cluster MR_F_RECORD
    batch, which gives the prefix tape P (a SimError if the seed already ended); a one-cluster
    source of the futures' kernel family is brought to the same point (the recording batch itself
    when the futures run a tape kernel); the source is forked into every position of a batch of
    `futures` clusters, which runs to the end. Future c draws from the seed `seed` + cluster_base +
    c after the prefix, and `replay(test, P, seed=seed, cluster_base=cluster_base + c, ...)`
    reproduces it from scratch. Returns a dict: prefix (P), codes, times_us, digests, counters (a
    prefix run on the pool kernel is counted in its source: mr_batch_fork) and kernel."""
    seed, at_events, futures = int(seed), int(at_events), int(futures)
    if at_events < 1 or futures < 1:
        raise SimError("run_futures: at_events and futures must be >= 1")
    kw = dict(kw)
    base_c = int(kw.pop("cluster_base", 0))
    flags = int(kw.pop("flags", 0)) & ~_abi.MR_F_RECORD
    # (what sizes or schedules the futures' batch alone)
    fut_kw = {k: kw.pop(k) for k in ("trace_clusters", "trace_cap", "lanes", "stream") if k in kw}
    with Batch(test, 1, seed, cluster_base=base_c, flags=flags | _abi.MR_F_RECORD,
               tape_cap=max(1 << 16, 64 * at_events), **kw) as rec, \
            Batch(test, futures, seed, cluster_base=base_c, flags=flags, **fut_kw, **kw) as fut:
        if rec.run(max_events=at_events)["remaining"] == 0:
            raise SimError(f"run_futures: seed {seed + base_c} ended within {at_events} events")
        n, prefix = rec.decisions(0)
        if n > prefix.size:
            raise SimError(f"run_futures: the prefix drew {n} decisions, the tape keeps {prefix.size}")
        prefix = np.array(prefix)
        of = np.zeros(futures, np.uint32)
        if fut.kernel == "pool_kernel":  # a source whose message keys are the pool's
            with Batch(test, 1, seed, cluster_base=base_c, flags=flags, **kw) as src:
                if src.kernel != fut.kernel:
                    raise SimError("run_futures: no one-cluster source on " + fut.kernel)
                src.run(max_events=at_events)
                fut.fork(of, src)
        else:
            fut.fork(of, rec)
        fut.run()
        code, t, dig = fut.verdicts()
        return {"prefix": prefix, "codes": code, "times_us": t, "digests": dig,
                "counters": fut.counters(), "kernel": fut.kernel}


def sweep_groups(grid):
    """The parameter groups of a sweep: the cartesian product of `grid`'s value lists, in the order
    given (the last field varies fastest). `grid` maps hb_us, ae_max or iters to numbers, elect_us
    to (lo, hi) pairs, bug to the names in _abi.BUG_FLAGS, unreliable / null_raft to booleans.
    Returns (params, groups): per setting the dict of what the grid set, and its mr_param_group
    fields for Batch.set_param_groups."""
    params, groups = [{}], [{"flags": 0}]
    for field, values in grid.items():
        values = list(values)
        if not values:
            raise SimError(f"sweep: no values for {field!r}")
        np_, ng = [], []
        for p, g in zip(params, groups):
            for v in values:
                g2 = dict(g)
                if field in ("hb_us", "ae_max", "iters"):
                    v = int(v)
                    g2[field] = v
                elif field == "elect_us":
                    v = (int(v[0]), int(v[1]))
                    g2["elect_lo_us"], g2["elect_hi_us"] = v
                elif field == "bug":
                    if v not in _abi.BUG_FLAGS:
                        raise SimError(f"sweep: unknown bug {v!r}")
                    g2["flags"] |= _abi.BUG_FLAGS[v]
                elif field in ("unreliable", "null_raft"):
                    v = bool(v)
                    bit = _abi.MR_F_UNRELIABLE if field == "unreliable" else _abi.MR_F_NULL_RAFT
                    g2["flags"] |= bit if v else 0
                else:
                    raise SimError(f"sweep: unknown field {field!r}")
                np_.append({**p, field: v})
                ng.append(g2)
        params, groups = np_, ng
    return params, groups


def sweep_positions(n_groups, seeds):
    """(group_of, seed_of) of a sweep batch in group-minor order: position p is group p % G at seed
    seeds[p // G], so every wave mixes the groups and every group runs the same seeds."""
    p = np.arange(n_groups * len(seeds))
    return (p % n_groups).astype(np.uint32), [int(seeds[i]) for i in p // n_groups]


def run_sweep(test, grid, seeds=None, num=None, **kw):
    """Every setting of `grid` (sweep_groups) over the same seeds in one batch of parameter groups
    (docs/SEMANTICS.md §12.4). Seeds: the list `seeds`, else `num` seeds from kw's `seed` (default:
    the README's). The batch-wide sweepable flags in kw (unreliable, null_raft, bug bits in flags) are
    the default of every group that does not set them. Returns one dict per setting: params, group
    (the mr_param_group fields), seeds, codes, times_us, digests, counters (group_counters)."""
    kw = dict(kw)
    first = int(kw.pop("seed", _abi.README_SEED))
    seeds = [int(s) for s in seeds] if seeds is not None else [first + k for k in range(int(num or 1))]
    if not seeds:
        raise SimError("run_sweep: no seeds")
    params, groups = sweep_groups(grid)
    base_c = int(kw.pop("cluster_base", 0))
    with Batch(test, len(groups) * len(seeds), min(seeds) - base_c, cluster_base=base_c, **kw) as b:
        inherit = int(b.cfg.flags) & _abi.SWEEPABLE_FLAGS
        for g in groups:  # a group's flags replace the batch's: what the grid left alone stays
            if "bug" not in grid:
                g["flags"] |= inherit & ~(_abi.MR_F_UNRELIABLE | _abi.MR_F_NULL_RAFT)
            if "unreliable" not in grid:
                g["flags"] |= inherit & _abi.MR_F_UNRELIABLE
            if "null_raft" not in grid:
                g["flags"] |= inherit & _abi.MR_F_NULL_RAFT
        G = len(groups)
        group_of, seed_of = sweep_positions(G, seeds)
        b.set_seeds(seed_of)
        b.set_param_groups(groups, group_of)
        b.run()
        code, t, dig = b.verdicts()
        return [{"params": params[g], "group": groups[g], "seeds": seeds, "codes": code[g::G],
                 "times_us": t[g::G], "digests": dig[g::G], "counters": b.group_counters(g)}
                for g in range(G)]


def run_test(test, seed=None, num=None, **kw):
    """`MADSIM_TEST_SEED=seed MADSIM_TEST_NUM=num cargo test <test>` on the GPU.

    Returns (codes, times_us, digests, counters); failures are also printed
    like the #[madsim::test] harness (README.md:44-48).
    """
    seed = int(os.environ.get("MADSIM_TEST_SEED", _abi.README_SEED)) if seed is None else seed
    num = int(os.environ.get("MADSIM_TEST_NUM", 1)) if num is None else num
    with Batch(test, num, seed, **kw) as b:
        b.run()
        code, t, dig = b.verdicts()
        cnt = b.counters()
    _print_failures(test, code, t, lambda k: seed + int(b.cfg.cluster_base) + k)
    return code, t, dig, cnt
