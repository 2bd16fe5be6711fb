"""CPU proof that the inputs of tests/test_gpu_walk_pack.py show what they
are meant to show (recipe in tests/walk_pack_cases.py): shared links that
are congested and carry jobs of different ul + dl, so the last-job-wins
rule decides the value of a cell; a congested shared destination; nothing
near the congestion switch; and the stated number of truncated walks."""
import pytest

from tests import stage_oracle as so
from tests import walk_pack_cases as wp


@pytest.mark.parametrize("name", wp.SETS)
def test_shared_links_make_last_job_wins_visible(name):
    c = wp.conditions(name)
    shared = c["shared"]
    print(f"set {name}: {len(shared)} links shared by two or more jobs, "
          f"smallest relative gap to mu - lam = 0: {c['gap']:.3f}")
    assert len(shared) >= wp.MIN_SHARED[name]
    assert all(s["congested"] for s in shared)
    assert all(s["distinct"] for s in shared)
    assert all(c["dst_congested"])
    # no used link or server near the switch: no cell is left out of the
    # comparison
    assert c["gap"] >= so.BAND


@pytest.mark.parametrize("name", wp.SETS)
def test_truncated_walk_counts(name):
    assert wp.front(name)["overflow"] == 0
    fr = wp.front(name, wp.CAP)
    assert fr["H"] == wp.CAP
    assert fr["overflow"] == wp.TRUNCATED[name]


def test_set_c_is_padded_and_ragged():
    eng = so.engine("C")
    assert eng.N == 25 and eng.k_N_arr.tolist() == [20, 25]
    assert eng.k_E_arr.tolist() == [36, 46]
