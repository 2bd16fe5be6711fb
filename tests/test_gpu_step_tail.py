"""GPU (MI355X) tests of the launches folded away around the episode kernels:
``decide`` on the strided diagonal of the delay matrix, ``critic`` looking
the destinations' compute slots up itself, the critic's loss summed by
``mse_finish``, and the kernels that zero their own outputs
(``actor_head_bwd``'s dλ tail, the K<=2 ChebConv backward's dW / db).

The "dirty block" trick — allocate a tensor of the output's size, fill it
with NaN, free it, launch — makes the caching allocator hand the launcher's
``torch::empty`` a dirty block.  It is best effort: nothing obliges the
allocator to reuse the block."""
import functools

import pytest
import torch

from tests import stage_oracle as so
from tests.test_gpu_stages import (_critic_kernel, _ext, _f32, _gpu_engine,
                                   needs_gpu)

pytestmark = pytest.mark.gpu

SETS = ("A", "C")


def _dirty(*shapes):
    blocks = [torch.full(s, float("nan"), device="cuda") for s in shapes]
    torch.cuda.synchronize()
    del blocks


def _bits(x):
    return x.contiguous().view(torch.int32)


def _ulps(a, b):
    """Largest distance in fp32 units in the last place (finite, same-sign
    values)."""
    a, b = _bits(a).to(torch.int64), _bits(b).to(torch.int64)
    return int((a - b).abs().max())


@needs_gpu
@pytest.mark.parametrize("name", SETS)
def test_decide_reads_the_diagonal_view(name):
    """decide on torch.diagonal(dm) (strides N², N + 1) against decide on
    its contiguous copy: dst and islocal equal.  The off-diagonal cells hold
    NaN, so a read through the wrong stride would show."""
    fr, eg = so.front(name), _gpu_engine(name)
    B, N = eg.B, eg.N
    dm = torch.full((B, N, N), float("nan"), device="cuda")
    torch.diagonal(dm, dim1=1, dim2=2).copy_(_f32(fr["uds"]))
    view = torch.diagonal(dm, dim1=1, dim2=2)
    assert view.stride() == (N * N, N + 1) and not view.is_contiguous()
    jg = so.jobs_to(fr["jobs"], "cuda", torch.float32)

    def run(uds):
        out = _ext().decide(_f32(fr["sp"]), eg.sp_hop.contiguous(), uds,
                            eg.k_servers, jg.sources, jg.mask,
                            jg.ul.contiguous(), jg.dl.contiguous(), None,
                            None, 0)
        torch.cuda.synchronize()
        return out

    dst_v, loc_v = run(view)
    dst_c, loc_c = run(view.contiguous())
    assert torch.equal(dst_v, dst_c) and torch.equal(loc_v, loc_c)
    assert torch.equal(dst_v.cpu()[fr["jobs"].mask],
                       fr["dst"][fr["jobs"].mask])


def _critic_lookup(eg, fr):
    jobs = so.jobs_to(fr["jobs"], "cuda", torch.float32)
    ge, loss = _ext().critic(
        fr["route_links"].to(torch.int32).cuda().contiguous(),
        fr["nhop"].to(torch.int32).cuda().contiguous(),
        fr["dst"].cuda().contiguous(), jobs.mask,
        jobs.rates.contiguous(), jobs.ul.contiguous(), jobs.dl.contiguous(),
        eg.k_conf_indptr, eg.k_conf_base, eg.k_conf_cols,
        eg.link_rates.contiguous(), eg.bw_comp.contiguous(), eg.k_E_arr,
        eg.T_arr.contiguous(), eg.Ee, eg.fp_iters, eg.delay_clamp,
        eg.node_vedge)
    torch.cuda.synchronize()
    return loss, ge


@needs_gpu
@pytest.mark.parametrize("name", SETS)
def test_critic_looks_the_destination_slot_up(name):
    """critic handed the destination nodes and node_vedge against critic
    handed the gathered vedge_dst: grad_edge and the per-graph loss
    bit-equal.  The distance between two launches of the gathered form is
    printed next to it."""
    fr, eg = so.front(name), _gpu_engine(name)
    loss_g, ge_g = _critic_kernel(eg, fr)
    loss_g2, ge_g2 = _critic_kernel(eg, fr)
    loss_l, ge_l = _critic_lookup(eg, fr)
    print(f"critic set {name}: gathered vs gathered again: grad_edge "
          f"{int((_bits(ge_g) != _bits(ge_g2)).sum())} cells differ, loss "
          f"{int((_bits(loss_g) != _bits(loss_g2)).sum())}; lookup vs "
          f"gathered: grad_edge {int((_bits(ge_l) != _bits(ge_g)).sum())} "
          f"cells differ, loss {int((_bits(loss_l) != _bits(loss_g)).sum())}")
    assert torch.equal(_bits(loss_l), _bits(loss_g))
    assert torch.equal(_bits(ge_l), _bits(ge_g))


@functools.lru_cache(maxsize=None)
def _fused_inputs(name):
    """What actor_head_bwd_fused takes on a set: the front's λ through
    actor_head_fwd, walk_eval's unit_mtx / written, the critic's grad_edge
    and per-graph loss."""
    fr, eg = so.front(name), _gpu_engine(name)
    ext = _ext()
    tables = (eg.k_conf_indptr, eg.k_conf_base, eg.k_conf_cols,
              eg.link_rates.contiguous(), eg.bw_comp.contiguous(),
              eg.k_edges, eg.node_vedge, eg.T_arr.contiguous(), eg.k_E_arr)
    lam = _f32(so.lam_input(name, 0.0)[0])
    dm, hist = ext.actor_head_fwd(lam, *tables, eg.N, eg.fp_iters, 0.0)
    jobs = so.jobs_to(fr["jobs"], "cuda", torch.float32)
    _, _, _, um, wr = eg._episode_eval(jobs, fr["dst"].cuda(),
                                       _f32(fr["sp"]))
    eg.overflow_total.zero_()
    loss, ge = _critic_kernel(eg, fr)
    return dict(eg=eg, tables=tables, lam=lam, dm=dm, hist=hist, um=um,
                wr=wr, ge=ge, loss=loss)


def _fused(c, loss=None):
    eg = c["eg"]
    out = _ext().actor_head_bwd_fused(
        c["ge"].contiguous(), c["dm"], c["um"], c["wr"], c["lam"], c["hist"],
        *c["tables"], eg.fp_iters, 0.0, loss)
    torch.cuda.synchronize()
    return out


@needs_gpu
@pytest.mark.parametrize("name", SETS)
def test_loss_fn_summed_by_mse_finish(name):
    """loss_fn from mse_finish's 256-wide tree against torch's loss.sum():
    within 4 fp32 ulps; dλ and loss_mse do not change with the extra
    argument."""
    c = _fused_inputs(name)
    dlam0, mse0 = _fused(c)
    dlam1, mse1, loss_fn = _fused(c, c["loss"])
    want = c["loss"].sum()
    d = _ulps(loss_fn.reshape(1), want.reshape(1))
    print(f"loss_fn set {name}: fused {float(loss_fn)!r}, torch "
          f"{float(want)!r}, {d} ulps apart")
    assert loss_fn.shape == () and d <= 4
    assert torch.equal(_bits(dlam0), _bits(dlam1))
    assert torch.equal(_bits(mse0.reshape(1)), _bits(mse1.reshape(1)))


@needs_gpu
def test_actor_head_bwd_zeroes_its_own_tail():
    """Set C (a graph with fewer computing nodes and fewer links than the
    batch maximum): dλ after a zero-filled block was freed equals dλ after a
    NaN-filled one, and every slot that is no real link or compute slot —
    [E + C_b, Ee) included — is zero."""
    c = _fused_inputs("C")
    eg = c["eg"]
    shape = tuple(c["lam"].shape)
    z = torch.zeros(shape, device="cuda")
    torch.cuda.synchronize()
    del z
    clean = _fused(c)[0]
    _dirty(shape)
    dirty = _fused(c)[0]
    assert torch.equal(_bits(clean), _bits(dirty))
    real = so.real_slots(so.engine("C"))
    assert not bool(real[:, eg.E:].all())           # a short compute tail
    assert bool((dirty.cpu()[~real] == 0).all())
    assert bool(torch.isfinite(dirty).all())


@needs_gpu
@pytest.mark.parametrize("case", [20, "ragged"])
@pytest.mark.parametrize("full", [False, True])
def test_cheb_bwd_zeroes_its_own_dw_db(case, full):
    """cheb_bwd_edge on the inputs of tests/test_gpu_cheb_edge_layers.py, on
    the edge-layer and on the full-width path, before and after the dirty
    block trick.  dW is ordered (two addends per cell onto zero commute):
    bit-equal.  db's column sums are float atomics whose order varies from
    run to run, so db is compared as that file compares it: worst max-abs
    error over max-abs against the fp64 oracle at most 4× the clean run's
    (floored at 2^-23) and under 5e-3.  On the edge-layer path the cells
    outside the real shapes, which nothing but the zero fill writes, are
    exact zeros."""
    from multihop_offload_amd.ops import dispatch
    from tests.test_gpu import _cheb_family_case
    from tests.test_gpu_cheb_edge_layers import FLOOR, L, _ragged_case, _worst

    ext = _ext()
    eng, x, dlam, W, bias, dmax, want = (
        _ragged_case() if case == "ragged" else _cheb_family_case(case, 2))
    W, bias = W.clone(), bias.clone()
    W[0, :, 4:, :] = 0.0
    W[L - 1, :, :, 1:] = 0.0
    bias[L - 1, 1:] = 0.0
    csr = (eng.k_ext_indptr, eng.k_ext_base, eng.k_ext_cols)
    nnz = eng.k_ext_max_nnz
    try:
        dispatch.cheb_force_full_width(full)
        lam, acts, t1s, edge = ext.cheb_fwd_edge(x, W, bias, *csr, nnz, 1)
        assert edge == (not full)
        torch.cuda.synchronize()
        dW0, db0 = ext.cheb_bwd_edge(dlam, x, lam, acts, t1s, W, *csr, nnz,
                                     edge)
        torch.cuda.synchronize()
        shapes = (tuple(dW0.shape), tuple(db0.shape))
        dW0, db0 = dW0.clone(), db0.clone()
        _dirty(*shapes)
        dW1, db1 = ext.cheb_bwd_edge(dlam, x, lam, acts, t1s, W, *csr, nnz,
                                     edge)
        torch.cuda.synchronize()
    finally:
        dispatch.cheb_force_full_width(False)
    assert bool(torch.isfinite(dW1).all() and torch.isfinite(db1).all())
    assert torch.equal(_bits(dW0), _bits(dW1))
    e0 = _worst(db0, want["db"])
    e1 = _worst(db1, want["db"])
    print(f"case={case} full={full} db: worst max-abs err / max-abs: clean "
          f"{e0:.3e}, dirty {e1:.3e}; "
          f"{int((_bits(db0) != _bits(db1)).sum())} cells differ in bits")
    assert e1 <= 4.0 * max(e0, FLOOR) and e1 < 5e-3, (e0, e1)
    if not full:
        assert not bool(dW1[:, 0, :, 4:, :].any())
        assert not bool(dW1[:, L - 1, :, :, 1:].any())
        assert not bool(db1[:, L - 1, 1:].any())
