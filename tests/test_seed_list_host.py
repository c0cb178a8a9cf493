"""CPU: the host side of seed lists (ABI 7, docs/SEMANTICS.md §12.3) — the offsets a list of
absolute seeds becomes, the CLI's --seeds parser, and the header's two new calls."""
import re

import numpy as np
import pytest

from madraft_amd import __main__ as cli
from madraft_amd import _abi, sim

BASE = _abi.README_SEED


def test_seed_offsets_round_trip():
    seeds = [BASE + 19, BASE, BASE + 3, BASE + 3, BASE + 70000, BASE + (1 << 32) - 1]
    off = sim.seed_offsets(seeds, BASE)
    assert off.dtype == np.uint32 and off.tolist() == [19, 0, 3, 3, 70000, (1 << 32) - 1]
    assert [BASE + int(o) for o in off] == seeds
    # cluster_base is part of the base: the same seeds from seed_base - 5 with cluster_base 5
    assert np.array_equal(sim.seed_offsets(seeds, BASE - 5, 5), off)
    assert sim.seed_offsets([], BASE).shape == (0,)
    big = (1 << 64) - 1  # 64-bit seeds: no detour through a signed or a floating type
    assert sim.seed_offsets([big, big - 7], big - 7).tolist() == [7, 0]


def test_seed_offsets_rejects_seeds_outside_the_base_window():
    with pytest.raises(sim.SimError, match=str(BASE - 1)):
        sim.seed_offsets([BASE, BASE - 1], BASE)
    with pytest.raises(sim.SimError, match=str(BASE + 4)):
        sim.seed_offsets([BASE + 4], BASE, cluster_base=5)
    with pytest.raises(sim.SimError, match=str(BASE + (1 << 32))):
        sim.seed_offsets([BASE, BASE + (1 << 32)], BASE)
    assert sim.seed_offsets([BASE + (1 << 32)], BASE, cluster_base=1).tolist() == [(1 << 32) - 1]


def test_cli_seeds_parser_reads_a_list_and_a_file(tmp_path):
    assert cli.parse_seeds("5,3, 3,0x10") == [5, 3, 3, 16]
    assert cli.parse_seeds(str(BASE + 19)) == [BASE + 19]
    f = tmp_path / "failing.txt"
    f.write_text(f"{BASE + 19}\n\n# found by the nightly run\n{BASE}  # the README seed\n{BASE + 3}\n")
    assert cli.parse_seeds("@" + str(f)) == [BASE + 19, BASE, BASE + 3]
    with pytest.raises(ValueError):
        cli.parse_seeds("")
    with pytest.raises(ValueError):
        cli.parse_seeds("1,x")
    (tmp_path / "none.txt").write_text("\n# nothing\n")
    with pytest.raises(ValueError):
        cli.parse_seeds("@" + str(tmp_path / "none.txt"))


def test_abi_version_and_the_two_calls_are_in_the_header():
    txt = open(_abi.HEADER).read()
    assert int(re.search(r"#define MR_ABI_VERSION (\d+)u", txt).group(1)) == _abi.MR_ABI_VERSION == 7
    assert re.search(r"^int mr_batch_set_seeds\(mr_batch\* b, const uint32_t\* seed_cluster", txt, re.M)
    assert re.search(r"^int mr_batch_get_decisions_packed\(mr_batch\* b, uint32_t first, uint32_t count, "
                     r"uint64_t\* drawn,\s+uint64_t\* off, mr_decision\* out, size_t cap\);", txt, re.M)
    assert {"mr_batch_set_seeds", "mr_batch_get_decisions_packed"} <= set(_abi.EXPORTS)
