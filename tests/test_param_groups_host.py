"""CPU: the parameter-group additions to the C ABI (include/madraft_sim.h, within ABI 7) and their
Python mirrors, run_sweep's grid expansion and position order, and the command line's --sweep."""
import os
import re
import subprocess
import tempfile

import numpy as np
import pytest

from madraft_amd import __main__ as cli
from madraft_amd import _abi, sim

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "madraft_sim.h")


def test_header_declares_the_struct_and_both_calls():
    txt = open(HEADER).read()
    assert re.search(r"typedef struct mr_param_group \{.*?\} mr_param_group;", txt, re.S)
    assert re.search(r"int mr_batch_set_param_groups\(mr_batch\* b, const mr_param_group\* g, "
                     r"size_t n_groups,\s*const uint32_t\* group_of", txt)
    assert re.search(r"int mr_batch_group_counters\(mr_batch\* b, uint32_t group, mr_counters\* out\);", txt)
    assert "an addition within ABI 7" in txt
    assert {"mr_batch_set_param_groups", "mr_batch_group_counters"} <= set(_abi.EXPORTS)


def test_abi_version_is_still_7():
    assert _abi.MR_ABI_VERSION == 7
    assert re.search(r"^#define MR_ABI_VERSION 7u$", open(HEADER).read(), re.M)


def test_struct_and_mask_as_the_c_compiler_sees_them():
    names = [n for n in _abi.PARAM_GROUP_DTYPE.names]
    offs = ", ".join(f"offsetof(mr_param_group, {n})" for n in names)
    src = f"""
#include <stdio.h>
#include <stddef.h>
#include "{HEADER}"
int main(void) {{
  size_t v[] = {{sizeof(mr_param_group), MR_F_SWEEPABLE, {offs}}};
  for (size_t i = 0; i < sizeof v / sizeof *v; i++) printf("%zu ", v[i]);
  return 0;
}}"""
    with tempfile.TemporaryDirectory() as d:
        c = os.path.join(d, "t.c")
        open(c, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-o", exe, c], check=True)
        got = list(map(int, subprocess.run([exe], capture_output=True, text=True,
                                           check=True).stdout.split()))
    assert got[0] == 32 == _abi.PARAM_GROUP_DTYPE.itemsize
    assert got[1] == _abi.SWEEPABLE_FLAGS
    assert got[2:] == [_abi.PARAM_GROUP_DTYPE.fields[n][1] for n in names]
    batch_wide = _abi.MR_F_SAFETY | _abi.MR_F_TRACE | _abi.MR_F_RECORD | _abi.MR_F_STREAM
    assert not _abi.SWEEPABLE_FLAGS & batch_wide
    assert _abi.SWEEPABLE_FLAGS | batch_wide == 0xFFF  # every flag is one or the other


def test_param_group_records():
    g = sim.param_group_records([{}, {"hb_us": 7, "flags": _abi.MR_F_BUG_NO_DEDUP},
                                 {"elect_lo_us": 1, "elect_hi_us": 2, "ae_max": 3, "iters": 4}])
    assert g.dtype == _abi.PARAM_GROUP_DTYPE and g.shape == (3,)
    assert not np.frombuffer(g[0].tobytes(), np.uint32).any()
    assert (g[1]["hb_us"], g[1]["flags"]) == (7, 0x100)
    assert np.frombuffer(g[2].tobytes(), np.uint32).tolist() == [0, 0, 1, 2, 3, 4, 0, 0]
    assert sim.param_group_records(None).size == 0
    with pytest.raises(sim.SimError, match="unknown field"):
        sim.param_group_records([{"hb": 1}])
    with pytest.raises(sim.SimError, match="unknown field"):
        sim.param_group_records([{"reserved": 1}])


def test_sweep_groups_is_the_cartesian_product_in_the_order_given():
    params, groups = sim.sweep_groups({"hb_us": [25000, 50000],
                                       "elect_us": [(150000, 300000), (50000, 60000)],
                                       "bug": ["none", "vote_stale"]})
    assert len(params) == len(groups) == 8
    assert params[0] == {"hb_us": 25000, "elect_us": (150000, 300000), "bug": "none"}
    assert params[1] == {"hb_us": 25000, "elect_us": (150000, 300000), "bug": "vote_stale"}
    assert params[2] == {"hb_us": 25000, "elect_us": (50000, 60000), "bug": "none"}
    assert params[4]["hb_us"] == 50000 and list(params[0]) == ["hb_us", "elect_us", "bug"]
    assert groups[3] == {"flags": _abi.MR_F_BUG_VOTE_STALE, "hb_us": 25000, "elect_lo_us": 50000,
                         "elect_hi_us": 60000}
    assert groups[0]["flags"] == 0
    assert sim.param_group_records(groups).size == 8  # every field is the struct's
    params, groups = sim.sweep_groups({"unreliable": [False, True], "iters": [5], "ae_max": [1, 2]})
    assert [g["flags"] for g in groups] == [0, 0, _abi.MR_F_UNRELIABLE, _abi.MR_F_UNRELIABLE]
    assert [g["ae_max"] for g in groups] == [1, 2, 1, 2] and all(g["iters"] == 5 for g in groups)
    assert sim.sweep_groups({}) == ([{}], [{"flags": 0}])  # no field: the one inherit group
    for bad in ({"hb": [1]}, {"bug": ["no_such"]}, {"hb_us": []}):
        with pytest.raises(sim.SimError):
            sim.sweep_groups(bad)


def test_sweep_positions_are_group_minor():
    group_of, seed_of = sim.sweep_positions(3, [10, 20, 30, 40])
    assert group_of.dtype == np.uint32
    assert group_of.tolist() == [0, 1, 2] * 4
    assert seed_of == [10, 10, 10, 20, 20, 20, 30, 30, 30, 40, 40, 40]
    for p in range(12):
        assert group_of[p] == p % 3 and seed_of[p] == [10, 20, 30, 40][p // 3]
    g8, _ = sim.sweep_positions(8, list(range(9)))
    assert set(g8[:64].tolist()) == set(range(8))  # a wave mixes every group


def test_sweep_arguments():
    grid = cli.parse_sweep(["hb_us=25000,50000,100000", "elect_us=150000:300000,50000:60000",
                            "bug=none,vote_stale"])
    assert grid == {"hb_us": [25000, 50000, 100000],
                    "elect_us": [(150000, 300000), (50000, 60000)], "bug": ["none", "vote_stale"]}
    assert list(grid) == ["hb_us", "elect_us", "bug"]
    assert cli.parse_sweep(["iters=0x10", "ae_max=1"]) == {"iters": [16], "ae_max": [1]}
    for bad in (["hb_us"], ["hb_us="], ["nodes=3,5"], ["bug=sometimes"], ["elect_us=5"],
                ["elect_us=9:3"], ["hb_us=1", "hb_us=2"], ["hb_us=fast"]):
        with pytest.raises(ValueError):
            cli.parse_sweep(bad)


@pytest.mark.parametrize("extra", [["--replay", "log.jsonl"], ["--shrink"], ["--shrink-failures"],
                                   ["--shrink-failures", "4"]])
def test_sweep_with_replay_or_shrink_is_a_usage_error(extra, capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["count_2b", "--sweep", "hb_us=10000,50000", *extra])
    assert e.value.code == 2
    assert "--sweep does not go with" in capsys.readouterr().err


def test_a_bad_sweep_is_a_usage_error(capsys):
    with pytest.raises(SystemExit) as e:
        cli.main(["count_2b", "--sweep", "nodes=3,5"])
    assert e.value.code == 2
    assert "FIELD=V1,V2" in capsys.readouterr().err
