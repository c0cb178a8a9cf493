"""mr_batch_fork without a device (docs/SEMANTICS.md §12.5): the owner column of mr_dev.h's array
table, as a host program evaluates it, and the entry point's declaration."""
import json
import os
import re
import shutil
import subprocess
import tempfile

import pytest

from madraft_amd import _abi
from tests.test_abi import LAYOUT_CONFIGS
from tests.test_gpu_fork import FORK_SCENARIOS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "madraft_sim.h")
DEV = os.path.join(ROOT, "madraft_amd", "csrc", "mr_dev.h")

# whose state every row is (docs/SEMANTICS.md §12.5)
OWNERS = {
    "MINOR": ["cs32", "cs64", "tmr", "mkey"],
    "MAJOR": ["nd32", "ms32", "log", "pay", "stor", "kt32", "kwk", "kv32", "lin32", "kvs32", "kring",
              "cfg32", "op32", "cval", "cidx", "led", "tfr"],
    "TRACED": ["trace", "tdig", "tapp", "adig"],
    "SHARED": ["remaining", "prof", "guard", "pcnt"],
}

OWN_SRC = """
#include <cstdio>
#include "{dev}"
#define MR_ROW_(m, elements, present, reset) #m,
static const char* const names[] = {{MR_DEV_ARRAYS(MR_ROW_)}};
static const char* const kinds[] = {{"MINOR", "MAJOR", "TRACED", "SHARED"}};
static_assert(mr::k_dev_own[mr::A_cs32] == mr::OWN_MINOR && mr::k_dev_own[mr::A_tfr] == mr::OWN_MAJOR, "");
static void one(uint32_t scn, uint32_t flags, uint32_t traced, uint32_t clusters) {{
  mr_cfg c;
  mr_cfg_defaults(&c, scn);
  c.n_clusters = clusters; c.flags = flags; c.trace_clusters = traced;
  const mr::DevLayout L = mr::dev_layout(c);
  for (uint32_t a = 0; a < mr::A__N; a++)
    std::printf("%s %s %zu %zu %lld ", names[a], kinds[mr::k_dev_own[a]], L.per[a], L.bytes[a],
                L.bytes[a] ? (long long)L.off[a] : -1ll);
  std::printf("total %zu reset", L.off[mr::A__N]);
  for (int k = 0; k < (int)mr::A__N; k++)
    for (uint32_t a = 0; a < mr::A__N; a++)
      if (mr::k_dev_reset[a] == k && L.bytes[a]) std::printf(" %s %zu", names[a], L.bytes[a]);
  std::printf("\\n");
}}
int main() {{
{calls}
  return 0;
}}"""


def run_host(body, extra=()):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    inc = os.path.join(os.path.dirname(os.path.dirname(os.path.realpath(hipcc))), "include")
    with tempfile.TemporaryDirectory() as d:
        src, exe = os.path.join(d, "f.cpp"), os.path.join(d, "f")
        open(src, "w").write(body)
        p = subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-D__HIP_PLATFORM_AMD__",
                            *extra, "-I", inc, "-o", exe, src], capture_output=True, text=True)
        if p.returncode:
            return None, p.stderr
        return subprocess.run([exe], capture_output=True, text=True, check=True).stdout, ""


def rows_of(configs, clusters):
    """Per config: ({row: (kind, per-owner bytes, bytes, offset)}, total, reset list)."""
    calls = "\n".join(f"  one({_abi.SCENARIO_ID[t]}, {flags}, {traced}, {clusters});"
                      for t, flags, traced in configs)
    out, err = run_host(OWN_SRC.format(dev=DEV, calls=calls))
    assert out is not None, err
    res = []
    for line in out.splitlines():
        w = line.split()
        t, r = w.index("total"), w.index("reset")
        rows = {w[i]: (w[i + 1], int(w[i + 2]), int(w[i + 3]), int(w[i + 4])) for i in range(0, t, 5)}
        res.append((rows, int(w[t + 1]), [[m, int(b)] for m, b in zip(w[r + 1::2], w[r + 2::2])]))
    assert len(res) == len(configs)
    return res


@pytest.fixture(scope="module")
def golden_rows():
    return rows_of(LAYOUT_CONFIGS, 64)


def test_every_row_says_whose_state_it_is(golden_rows):
    rows = golden_rows[0][0]
    assert {k: [m for m in rows if rows[m][0] == k] for k in OWNERS} == OWNERS


def test_bytes_are_per_owner_times_owners(golden_rows):
    """Every cluster row is per-cluster bytes x C, every traced row x the traced clusters, in the
    golden file's six batches of 64 clusters; cluster-major slabs are whole 16-B quads."""
    for (test, _, traced), (rows, _, _) in zip(LAYOUT_CONFIGS, golden_rows):
        for m, (kind, per, nbytes, off) in rows.items():
            owners = {"MINOR": 64, "MAJOR": 64, "TRACED": traced, "SHARED": 1}[kind]
            assert nbytes == per * owners, (test, m)
            assert (off == -1) == (nbytes == 0), (test, m)
            if kind in ("MAJOR", "TRACED"):
                assert per % 16 == 0, (test, m)


def test_layout_and_reset_still_match_the_golden_file(golden_rows):
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "dev_layout.json")))
    for (test, _, _), (rows, total, reset) in zip(LAYOUT_CONFIGS, golden_rows):
        want = golden[test]
        assert [(m, r[3]) for m, r in rows.items()] == list(want["offsets"].items()), test
        assert total == want["total"] and reset == want["reset"], test


def test_gpu_cases_reach_every_cluster_owned_row():
    """The scenarios tests/test_gpu_fork.py forks hold, between them, every row that is cluster
    state: none goes unexercised. 200 clusters, as there."""
    seen = set()
    for rows, _, _ in rows_of(FORK_SCENARIOS, 200):
        seen |= {m for m, (kind, per, nbytes, _) in rows.items() if nbytes and kind != "SHARED"}
    assert seen == set(OWNERS["MINOR"] + OWNERS["MAJOR"] + OWNERS["TRACED"])


def test_a_row_without_an_owner_does_not_compile():
    """A row typed as before the column, with its element count over C, is rejected by the
    compiler: C is no name where the owners are tabulated."""
    body = '#include "%s"\nint main() { return 0; }\n' % DEV
    ok, err = run_host(body)
    assert ok is not None, err
    text = open(DEV).read()
    assert "X(tfr, MR_MAJOR(TF_Q), true, KERNEL)" in text
    with tempfile.TemporaryDirectory() as d:
        bad = os.path.join(d, "mr_dev.h")
        text = text.replace("X(tfr, MR_MAJOR(TF_Q), true, KERNEL)", "X(tfr, TF_Q * C, true, KERNEL)")
        text = text.replace('"../../include/madraft_sim.h"', '"%s"' % HEADER)
        open(bad, "w").write(text)
        ok, err = run_host('#include "%s"\nint main() { return 0; }\n' % bad)
    assert ok is None and re.search(r"[‘'`]C[’'`] was not declared in this scope", err), err


def test_declared_and_exported():
    text = open(HEADER).read()
    assert re.search(r"^int mr_batch_fork\(mr_batch\* dst, mr_batch\* src[^;]*const uint32_t\* src_of",
                     text, re.M)
    assert "mr_batch_fork" in _abi.EXPORTS and _abi.FORK_SKIP == 0xFFFFFFFF
    assert _abi.MR_ABI_VERSION == 7
