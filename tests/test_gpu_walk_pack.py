"""GPU (MI355X) test of walk_eval's last-job-wins cells: the pack scratch has
one cell per link and per node, unit_mtx / written are zero-filled by the
kernel and written where a pack is non-zero, and the truncated walks are
counted by the kernel (per graph and into the optional device total).

Inputs and fp64 oracle: tests/walk_pack_cases.py (conditioning proven in
tests/test_walk_pack_inputs.py)."""
import pytest
import torch

from tests import stage_oracle as so
from tests import walk_pack_cases as wp
from tests.test_gpu_stages import _check, _ext, _f32, _gpu_engine, needs_gpu

pytestmark = pytest.mark.gpu


def _dirty(eg, H):
    """Allocate, fill and free tensors of the sizes walk_eval allocates
    (NaN for floats, 0x7f bytes for the rest), so that the caching allocator
    hands the launcher those dirty blocks for its torch::empty outputs.
    Best effort: nothing guarantees the allocator reuses them."""
    B, N, E, J = eg.B, eg.N, eg.E, eg.Jmax
    dev = eg.device
    blocks = [torch.full((B, N, N), float("nan"), device=dev),
              torch.full((B, J), float("nan"), device=dev)]
    for shape, dt in (((B, N, N), torch.uint8), ((B, E + N), torch.int64),
                      ((B,), torch.int32), ((B, J, H), torch.int32),
                      ((B, J), torch.int32)):
        t = torch.empty(shape, dtype=dt, device=dev)
        t.view(torch.uint8).fill_(0x7f)
        blocks.append(t)
    torch.cuda.synchronize()
    del blocks


def _walk(eg, fr, total=None):
    jg = so.jobs_to(fr["jobs"], "cuda", torch.float32)
    _dirty(eg, fr["H"])
    out = _ext().walk_eval(
        _f32(fr["sp"]), jg.sources, fr["dst"].cuda().contiguous(), jg.mask,
        jg.rates.contiguous(), jg.ul.contiguous(), jg.dl.contiguous(),
        eg.k_adj_indptr, eg.k_adj_idx, eg.k_adj_link, eg.k_conf_indptr,
        eg.k_conf_base, eg.k_conf_cols, eg.link_rates.contiguous(),
        eg.proc_bws.contiguous(), eg.k_edges, eg.T_arr.contiguous(),
        eg.k_E_arr, eg.k_N_arr, fr["H"], eg.fp_iters, total)
    torch.cuda.synchronize()
    return out


@needs_gpu
@pytest.mark.parametrize("name", wp.SETS)
def test_walk_eval_last_job_wins_vs_fp64(name):
    """Jobs with different ul + dl share congested links and one congested
    destination (26 shared links on set A, 11 on C): route_links, nhop and
    written (including the pad rows and columns of set C) are exact,
    unit_mtx and delay_emp within stage_oracle.tolerance of the oracle's
    fp32-reference error (CPU: delay_emp 2.1e-7 / 1.4e-7, unit_mtx 1.6e-7 /
    1.3e-7 on A / C -> tolerances 1.0e-6..1.6e-6).  The outputs are handed
    to the kernel in dirty blocks where the allocator plays along (best
    effort: the allocator is not obliged to reuse the freed blocks)."""
    c = wp.case(name)
    fr = c["front"]
    eg = _gpu_engine(name)
    assert min(eg.walk_cap, 64) == fr["H"]
    rl, nhop, de, um, wr, ovf = _walk(eg, fr)
    assert torch.equal(rl.cpu().to(torch.int64), fr["route_links"])
    assert torch.equal(nhop.cpu().to(torch.int64), fr["nhop"])
    assert torch.equal(wr.cpu(), c["want"][2])
    assert int(ovf.sum()) == 0 and ovf.shape == (eg.B,)
    assert bool(torch.isnan(de.cpu()[~fr["jobs"].mask]).all())
    if name == "C":
        n0 = int(eg.k_N_arr[0])
        assert n0 < eg.N
        assert not bool(wr[0, n0:].any()) and not bool(wr[0, :, n0:].any())
        assert bool((um[0, n0:] == 0).all() and (um[0, :, n0:] == 0).all())
    errs = so._eval_errs((de, um, wr), c["want"])
    _check("walk_eval pack", name, "walk_cap None", errs, c)


@needs_gpu
@pytest.mark.parametrize("name", wp.SETS)
def test_walk_eval_counts_truncated_walks(name):
    """walk_cap = 3: the per-graph counts sum to the oracle's 7 (A) and 5
    (C), and the device total handed in grows by exactly that on each of
    two calls; the truncated routes and everything evaluated on them still
    agree with the oracle."""
    c = wp.case(name, wp.CAP)
    fr = c["front"]
    assert fr["overflow"] == wp.TRUNCATED[name]
    eg = _gpu_engine(name, 0.0, wp.CAP)
    total = torch.full((), 1000, dtype=torch.int64, device="cuda")
    for call in (1, 2):
        rl, nhop, de, um, wr, ovf = _walk(eg, fr, total)
        assert int(ovf.sum()) == wp.TRUNCATED[name]
        assert int(total) == 1000 + call * wp.TRUNCATED[name]
    assert torch.equal(rl.cpu().to(torch.int64), fr["route_links"])
    assert torch.equal(nhop.cpu().to(torch.int64), fr["nhop"])
    errs = so._eval_errs((de, um, wr), c["want"])
    _check("walk_eval pack", name, f"walk_cap {wp.CAP}", errs, c)
