"""The ChebConv kernels at the top of their shape ranges, called directly and
compared with the fp64 oracle of tests/large_shape_cases.py (its inputs are
checked on the CPU by tests/test_large_shape_inputs.py):

* the row-tiled family (chebconv_large.hip) for K = 1 and 2 at three, three
  exact and seven 64-row tiles, the last the first shape production routes
  to it, and with the top gradient confined to one tile so that a row tile
  lost or counted twice in the dW / db atomics is a 100% error;
* the LDS-resident families (chebconv.hip) at the largest shapes they
  accept, where the backward no longer stages the support CSR in LDS;
* every LDS-resident kernel with the CSR read from global memory, against
  its own staged run;
* the generic-K kernels at K = 4, 5 and 6, where the backward's reverse
  recurrence runs more than once (forward, saved terms and gradients).

Padded batches: graph 1 has an empty band of rows across a tile boundary and
an empty tail; every comparison covers those rows.

Tolerances.  Forward: per element, the bound of
``test_cheb_kernel_families_agree``.  Gradients: per (graph, layer) max-abs
error / oracle max-abs, at most 8× the same figure of the recurrence run in
fp32 torch on the CPU (never above 5e-3); each test prints the fp32
reference's figure, the tolerance and the kernel's figure, and
docs/KERNELS.md tabulates them.
"""
import pytest
import torch

from tests import large_shape_cases as lc

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")

L = lc.L


def _ext():
    from multihop_offload_amd.ops import dispatch
    return dispatch.require_hip()


def _plan(Ee, K, nnz):
    from multihop_offload_amd.ops import dispatch
    return dispatch.cheb_lds_plan(Ee, K, nnz)


def _dev(case):
    """x, dlam, W, bias, (indptr, base, cols) on the GPU."""
    d = {k: case[k].cuda() for k in ("x", "dlam", "W", "bias", "indptr",
                                     "base", "cols")}
    return d["x"], d["dlam"], d["W"], d["bias"], (d["indptr"], d["base"],
                                                  d["cols"])


def _check_forward(tag, case, lam, acts, slots):
    """lam and the activation slots ``slots`` against the oracle, every row
    of every graph; then the empty rows of a padded batch on their own."""
    want = case["want"]
    pairs = [("lam", lam.double().cpu(), want["lam"])]
    pairs.append(("acts", acts.double().cpu()[:, slots],
                  want["acts"][:, slots]))
    for name, g, w in pairs:
        err = (g - w).abs()
        bound = lc.fwd_bound(case, w)
        print(f"{tag} {name}: max abs err {float(err.max()):.3e}, smallest "
              f"bound {float(bound.min()):.3e}")
        assert bool(torch.isfinite(g).all()), (tag, name)
        assert bool((err <= bound).all()), (tag, name)
    if case["padded"]:
        empty = lc.empty_rows(case["Ee"], 1, True)
        w = want["acts"][1][:, empty][slots]
        g = acts.double().cpu()[1][:, empty][slots]
        # the hidden activations there are act(bias) rows, not zeros
        assert bool((want["acts"][1, 1:L][:, empty] != 0).any(2).all())
        assert bool(((g - w).abs() <= lc.fwd_bound(case, w)).all()), tag
        assert bool(((lam.double().cpu()[1, empty] - want["lam"][1, empty])
                     .abs() <= lc.fwd_bound(case, want["lam"][1, empty]))
                    .all()), tag


def _check_grads(tag, case, dW, db):
    for name, g in (("dW", dW), ("db", db)):
        errs = lc.grad_errors(g, case["want"][name])
        worst = float(errs.max())
        print(f"{tag} {name}: fp32-reference err {case['ref_err'][name]:.3e}"
              f" tolerance {case['tol'][name]:.3e} kernel err {worst:.3e}")
        assert bool(torch.isfinite(g).all()), (tag, name)
        assert worst <= case["tol"][name], (tag, name, errs)


def _run_large(case):
    ext = _ext()
    x, dlam, W, bias, csr = _dev(case)
    lam, acts = ext.cheb_large_fwd(x, W, bias, *csr)
    dW, db = ext.cheb_large_bwd(dlam, acts, W, *csr)
    torch.cuda.synchronize()
    return lam, acts, dW, db


def _run_lds(case, nnz, family):
    """One forward + backward of an LDS-resident family with the launch
    sized for ``nnz`` support entries.  Returns lam, acts, the saved
    Chebyshev terms, dW, db and the activation slots the family writes."""
    ext = _ext()
    x, dlam, W, bias, csr = _dev(case)
    slots = slice(0, L + 1)
    if family == "cheb":
        lam, acts, tk = ext.cheb_fwd(x, W, bias, *csr, nnz)
        dW, db = ext.cheb_bwd(dlam, acts, tk, W, *csr, nnz)
    elif family == "cheb_edge":
        lam, acts, tk, edge = ext.cheb_fwd_edge(x, W, bias, *csr, nnz, 1)
        assert edge
        dW, db = ext.cheb_bwd_edge(dlam, x, lam, acts, tk, W, *csr, nnz,
                                   edge)
        slots = slice(1, L)          # slots 0 and L are not written
    else:
        lam, acts, tk = ext.cheb_kn_fwd(x, W, bias, *csr, nnz)
        dW, db = ext.cheb_kn_bwd(dlam, acts, tk, W, *csr, nnz)
    torch.cuda.synchronize()
    return lam, acts, tk, dW, db, slots


def _families(K):
    return ("cheb", "cheb_edge") if K <= 2 else ("cheb_kn",)


@needs_gpu
def test_cheb_lds_plan_is_the_closed_form():
    """Host only, nothing is launched: the launchers' plan, through
    ``dispatch.cheb_lds_plan``, against the closed form stated in the test
    helpers, with and without room for the CSR; and ``cheb_fits_lds`` is the
    ``fits`` of the two plans it routes on."""
    ext = _ext()
    for K in range(1, 7):
        for Ee in list(range(1, 420)) + [599, 600]:
            for nnz in (0, 6 * Ee, lc.INFLATED_NNZ):
                assert _plan(Ee, K, nnz) == lc.lds_plans(Ee, K, nnz), \
                    (Ee, K, nnz)
            assert ext.cheb_fits_lds(Ee, K) == lc.fits_lds(Ee, K)


@needs_gpu
@pytest.mark.parametrize("Ee,K", lc.ROW_TILED)
def test_row_tiled_family(Ee, K):
    """cheb_large_fwd / cheb_large_bwd on padded batches of three graphs."""
    ext = _ext()
    if Ee == 385:
        assert ext.cheb_fits_lds(384, 2) and not ext.cheb_fits_lds(385, 2)
    case = lc.cheb_case(Ee, K)
    lam, acts, dW, db = _run_large(case)
    tag = f"cheb_large Ee={Ee} K={K}"
    _check_forward(tag, case, lam, acts, slice(0, L + 1))
    _check_grads(tag, case, dW, db)


@needs_gpu
@pytest.mark.parametrize("Ee,K,tile", lc.ONE_TILE)
def test_row_tiled_one_tile_support(Ee, K, tile):
    """dlam lives on the rows of one 64-row tile only (the first, or the
    five rows of the last), two unpadded graphs: the gradients of the top
    layer come from that tile alone, and the errors are normalised by this
    case's own oracle, so a tile dropped from or added twice to the dW / db
    atomics cannot hide among fifty others."""
    case = lc.cheb_case(Ee, K, False, tile)
    lam, acts, dW, db = _run_large(case)
    tag = f"cheb_large Ee={Ee} K={K} {tile} tile"
    _check_forward(tag, case, lam, acts, slice(0, L + 1))
    _check_grads(tag, case, dW, db)


@needs_gpu
@pytest.mark.parametrize("Ee,K", lc.LDS_TOP)
def test_lds_resident_families_at_their_largest_shapes(Ee, K):
    """The largest Ee each LDS-resident family accepts (and Ee = 377, whose
    rows_pad is the same 384 with seven padded rows): 24 or more MFMA row
    tiles over 8 waves.  The backward has no room left for the support CSR
    and reads it from global memory; at K = 2 the forward still stages it."""
    ext = _ext()
    case = lc.cheb_case(Ee, K)
    nnz = case["max_nnz"]
    assert ext.cheb_fits_lds(Ee, K)
    if Ee != 377:
        assert not ext.cheb_fits_lds(Ee + 1, K)
    plan = _plan(Ee, K, nnz)
    fwd, bwd = ("kn_fwd", "kn_bwd") if K > 2 else ("fwd", "bwd")
    assert plan[fwd]["fits"] and plan[bwd]["fits"]
    assert plan[bwd]["stage_csr"] == 0
    if K == 2:
        assert plan[fwd]["stage_csr"] == 1
    for family in _families(K):
        lam, acts, _, dW, db, slots = _run_lds(case, nnz, family)
        tag = f"{family} Ee={Ee} K={K}"
        _check_forward(tag, case, lam, acts, slots)
        _check_grads(tag, case, dW, db)


@needs_gpu
@pytest.mark.parametrize("Ee,K,padded", lc.GENERIC_K)
def test_generic_k_beyond_three(Ee, K, padded):
    """cheb_kn_fwd / cheb_kn_bwd at K = 4, 5 and 6, called directly.  From
    K = 4 on the backward's reverse recurrence runs more than once, so the
    swap of its two buffers and the weight slot of each step matter, and an
    even and an odd K end on opposite buffers; the K = 3 tests cannot see
    either.  lam, every activation slot, the K - 1 saved Chebyshev terms of
    every layer, dW and db against the fp64 oracle; the padded cases have
    three row tiles and the empty band, (368, 4) and (352, 5) are the
    largest shapes ``cheb_fits_lds`` accepts and run their backward with
    the support CSR in global memory, the others stage it."""
    ext = _ext()
    case = lc.cheb_case(Ee, K, padded)
    nnz = case["max_nnz"]
    top = (Ee, K) in lc.GENERIC_K_TOP
    if top:
        assert ext.cheb_fits_lds(Ee, K) and not ext.cheb_fits_lds(Ee + 1, K)
    plan = _plan(Ee, K, nnz)
    assert plan["kn_fwd"]["fits"] and plan["kn_bwd"]["fits"]
    assert plan["kn_bwd"]["stage_csr"] == (0 if top else 1)
    lam, acts, tks, dW, db, slots = _run_lds(case, nnz, "cheb_kn")
    tag = f"cheb_kn Ee={Ee} K={K}"
    _check_forward(tag, case, lam, acts, slots)
    want = case["want"]["tks"]
    assert tuple(tks.shape) == (case["B"], L, K - 1, Ee, lc.F)
    err = (tks.double().cpu() - want).abs()
    bound = lc.fwd_bound(case, want)
    print(f"{tag} tks: largest err / bound {float((err / bound).max()):.3f} "
          f"(fp32 reference {case['tks_err32']:.3f}), largest term "
          f"{float(want.abs().max()):.3e}")
    assert bool(torch.isfinite(tks).all()), tag
    assert bool((err <= bound).all()), tag
    _check_grads(tag, case, dW, db)


@needs_gpu
@pytest.mark.parametrize("Ee,K", lc.UNSTAGED)
def test_unstaged_csr_equals_staged(Ee, K):
    """Every LDS-resident kernel with the support CSR read from global
    memory (a launch sized for a max_nnz that cannot fit; the kernels touch
    only the true indptr[Ee] entries) against its own staged run: the
    forward outputs bit for bit, dW / db against the oracle within the
    gradient tolerance on both runs (their atomics are unordered)."""
    case = lc.cheb_case(Ee, K, False)
    nnz = case["max_nnz"]
    assert lc.INFLATED_NNZ >= nnz
    staged, unstaged = _plan(Ee, K, nnz), _plan(Ee, K, lc.INFLATED_NNZ)
    for name in staged:
        assert staged[name]["stage_csr"] == 1 and staged[name]["fits"]
        assert unstaged[name]["stage_csr"] == 0 and unstaged[name]["fits"]
        assert unstaged[name]["lds_bytes"] < staged[name]["lds_bytes"]
    for family in _families(K):
        a = _run_lds(case, nnz, family)
        b = _run_lds(case, lc.INFLATED_NNZ, family)
        slots = a[5]
        tag = f"{family} Ee={Ee} K={K}"
        assert torch.equal(a[0].view(torch.int32), b[0].view(torch.int32))
        assert torch.equal(a[1][:, slots].view(torch.int32),
                           b[1][:, slots].view(torch.int32)), tag
        if K > 1:
            ta, tb = a[2], b[2]
            if family == "cheb_edge":
                # slot 0 holds T1_0 as (Ee,4) at its head, the rest is unset
                head = lambda t: t[:, 0].reshape(t.shape[0], -1)[:, :Ee * 4]
                assert torch.equal(head(ta).view(torch.int32),
                                   head(tb).view(torch.int32)), tag
                ta, tb = ta[:, 1:], tb[:, 1:]
            assert torch.equal(ta.view(torch.int32), tb.view(torch.int32))
        for run, mode in ((a, "staged"), (b, "unstaged")):
            _check_forward(f"{tag} {mode}", case, run[0], run[1], slots)
            _check_grads(f"{tag} {mode}", case, run[3], run[4])
