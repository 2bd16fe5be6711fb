"""GPU tests of the edge-layer path of the K<=2 LDS-resident ChebConv
kernels (first layer 4 wide, last layer 1 wide; ops/hip/chebconv.hip)
against the full-width path of the same build, reached through
``dispatch.cheb_force_full_width``, and against an fp64 oracle.

Inputs follow the recipe of ``_cheb_family_case`` in tests/test_gpu.py with
the weights zero-padded to the real shapes (4→32, 32→32, 32→1).  Its oracle
holds for them unchanged: the loss reads column 0 of the last layer only, so
the columns and rows zeroed here carry neither value nor gradient there.
n=20: Ee=55 (rows_pad 64, 9 padded rows); n=30: Ee=85 (rows_pad 96: 12 GEMM
tiles over 8 waves, 12 row k-steps per wgrad half); "ragged": a 20-node case
padded to 25 next to a 25-node case, as stage set C of tests/stage_oracle.py.
Each case runs its launches once; the tests share them.
"""
import functools

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")

L, F = 5, 32
FLOOR = 2.0 ** -23      # fp32 epsilon: below it an error ratio means nothing
CASES = (20, 30, "ragged")


def _ragged_cases():
    from tests.test_engine import _case
    return [_case(seed=3, n=20).pad_to(25), _case(seed=9, n=25)]


def _ragged_case():
    """The recipe of ``_cheb_family_case`` (K=2) on the ragged engine."""
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack

    K = 2
    eng = EpisodeEngine(_ragged_cases(),
                        ChebConvStack(K=2, dtype=torch.float32, seed=0),
                        device="cuda", dtype=torch.float32)
    B, Ee = eng.B, eng.Ee
    ipt = eng.k_ext_indptr.cpu().numpy()
    base = eng.k_ext_base.cpu().numpy()
    cols = eng.k_ext_cols.cpu().numpy()
    A = torch.zeros(B, Ee, Ee, dtype=torch.float64)
    for b in range(B):
        for r in range(Ee):
            for a in range(ipt[b, r], ipt[b, r + 1]):
                A[b, r, cols[base[b] + a]] += 1.0
    assert torch.equal(A, A.transpose(1, 2))
    # the shorter graph leaves rows without neighbours at the end
    assert int(A[0].sum(1).ne(0).sum()) < int(A[1].sum(1).ne(0).sum())
    dmax = float(A.sum(dim=2).max())
    ev = torch.linalg.eigvalsh(A)
    tk = [torch.ones_like(ev), ev]
    gen = torch.Generator()
    gen.manual_seed(4242)
    x = torch.randn(B, Ee, 4, generator=gen)
    dlam = torch.randn(B, Ee, generator=gen)
    W = torch.randn(L, K, F, F, generator=gen)
    for k in range(K):
        W[:, k] *= 2.0 / (K * F ** 0.5 * float(tk[k].abs().max()))
    bias = 0.1 * torch.randn(L, F, generator=gen)

    Wd = W.double().unsqueeze(0).repeat(B, 1, 1, 1, 1).requires_grad_()
    bd = bias.double().unsqueeze(0).repeat(B, 1, 1).requires_grad_()
    h = torch.zeros(B, Ee, F, dtype=torch.float64)
    h[:, :, :4] = x.double()
    for l in range(L):
        out = h @ Wd[:, l, 0] + (A @ h) @ Wd[:, l, 1] + bd[:, l].unsqueeze(1)
        h = (torch.relu(out) if l == L - 1
             else torch.nn.functional.leaky_relu(out, 0.2))
        assert 0.1 < float(h.detach().abs().max()) < 10.0
    lam = h[:, :, 0]
    (lam * dlam.double()).sum().backward()
    want = dict(lam=lam.detach(), dW=Wd.grad, db=bd.grad)
    return eng, x.cuda(), dlam.cuda(), W.cuda(), bias.cuda(), dmax, want


@functools.lru_cache(maxsize=None)
def _runs(case):
    """One full-width and two edge-layer forward+backward launches on the
    case's inputs, with the fp64 oracle."""
    from multihop_offload_amd.ops import dispatch
    from tests.test_gpu import _cheb_family_case

    ext = dispatch.require_hip()
    eng, x, dlam, W, bias, dmax, want = (
        _ragged_case() if case == "ragged" else _cheb_family_case(case, 2))
    if case != "ragged":
        assert eng.Ee == {20: 55, 30: 85}[case]
    W, bias = W.clone(), bias.clone()
    W[0, :, 4:, :] = 0.0
    W[L - 1, :, :, 1:] = 0.0
    bias[L - 1, 1:] = 0.0
    csr = (eng.k_ext_indptr, eng.k_ext_base, eng.k_ext_cols)
    nnz = eng.k_ext_max_nnz

    def launch():
        lam, acts, t1s, edge = ext.cheb_fwd_edge(x, W, bias, *csr, nnz, 1)
        dW, db = ext.cheb_bwd_edge(dlam, x, lam, acts, t1s, W, *csr, nnz,
                                   edge)
        return dict(lam=lam, acts=acts, t1s=t1s, edge=edge, dW=dW, db=db)

    try:
        dispatch.cheb_force_full_width(True)
        full = launch()
    finally:
        dispatch.cheb_force_full_width(False)
    edge = launch()
    again = launch()
    torch.cuda.synchronize()
    assert not full["edge"] and edge["edge"] and again["edge"]
    return dict(eng=eng, want=want, full=full, edge=edge, again=again)


def _worst(g, w):
    """Worst max-abs error over max-abs of the oracle, per graph and
    layer — the metric of test_cheb_kernel_families_agree."""
    g = g.double().cpu()
    assert g.shape == w.shape
    worst = 0.0
    for b in range(g.shape[0]):
        for l in range(g.shape[1]):
            denom = float(w[b, l].abs().max())
            assert denom > 0
            worst = max(worst,
                        float((g[b, l] - w[b, l]).abs().max()) / denom)
    return worst


@needs_gpu
@pytest.mark.parametrize("case", CASES)
def test_forward_bit_equal(case):
    """lam, the hidden activations and their T1 are bit-equal on both
    paths, so nothing downstream of the actor can move; T1_0 is saved
    4 wide at the head of its slot."""
    r = _runs(case)
    full, edge = r["full"], r["edge"]
    B, Ee = full["lam"].shape
    assert torch.equal(edge["lam"], full["lam"])
    assert torch.equal(edge["acts"][:, 1:L], full["acts"][:, 1:L])
    assert torch.equal(edge["t1s"][:, 1:], full["t1s"][:, 1:])
    t1_0 = edge["t1s"][:, 0].reshape(B, -1)[:, :Ee * 4].reshape(B, Ee, 4)
    assert torch.equal(t1_0, full["t1s"][:, 0, :, :4])


@needs_gpu
@pytest.mark.parametrize("case", CASES)
def test_backward_error_against_full_width(case):
    """dW and db against the fp64 oracle: the edge-layer path has at most 4×
    the error of the full-width path on the same inputs (floored at 2^-23)
    and stays below the family test's 5e-3."""
    r = _runs(case)
    for name in ("dW", "db"):
        e_full = _worst(r["full"][name], r["want"][name])
        e_edge = _worst(r["edge"][name], r["want"][name])
        print(f"case={case} {name}: worst max-abs err / max-abs: "
              f"full-width {e_full:.3e}, edge-layer {e_edge:.3e}")
        assert e_edge <= 4.0 * max(e_full, FLOOR), (name, e_edge, e_full)
        assert e_edge < 5e-3, (name, e_edge)


@needs_gpu
@pytest.mark.parametrize("case", CASES)
def test_exact_zeros_outside_real_shapes(case):
    dW, db = _runs(case)["edge"]["dW"], _runs(case)["edge"]["db"]
    assert not bool(dW[:, 0, :, 4:, :].any())
    assert not bool(dW[:, L - 1, :, :, 1:].any())
    assert not bool(db[:, L - 1, 1:].any())
    # the live cells next to them are populated, in every graph
    assert bool(dW[:, 0, :, :4, :].flatten(1).ne(0).any(1).all())
    assert bool(dW[:, L - 1, :, :, 0].flatten(1).ne(0).any(1).all())
    assert bool(db[:, L - 1, 0].ne(0).all())


@needs_gpu
@pytest.mark.parametrize("case", CASES)
def test_dw_deterministic(case):
    r = _runs(case)
    assert torch.equal(r["edge"]["dW"], r["again"]["dW"])
    assert torch.equal(r["edge"]["lam"], r["again"]["lam"])


@needs_gpu
def test_engine_level_switch():
    """ChebStackFn through an EpisodeEngine on the ragged batch with the
    switch on and off: lam bit-equal (padded link slots included), parameter
    gradients of a fixed linear loss within the bound of the backward test
    against an fp64 model with the same parameters."""
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.graphs import JobInstance
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.ops import dispatch
    from tests.test_engine import _wake

    cases = _ragged_cases()
    rng = np.random.RandomState(0)
    inst = [JobInstance.sample(g.mobile_nodes, 0.15, rng) for g in cases]
    model = ChebConvStack(K=2, dtype=torch.float32, seed=11)
    _wake(model)
    eng = EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)
    assert eng.use_hip
    jobs = eng.pack_jobs(inst)
    gen = torch.Generator()
    gen.manual_seed(7)
    g = torch.randn(eng.B, eng.Ee, generator=gen)

    def run(full):
        try:
            dispatch.cheb_force_full_width(full)
            for p in model.parameters():
                p.grad = None
            lam = eng._lam_hip(jobs)
            (lam * g.cuda()).sum().backward()
            torch.cuda.synchronize()
        finally:
            dispatch.cheb_force_full_width(False)
        return lam.detach().cpu(), [p.grad.double().cpu()
                                    for p in model.parameters()]

    lam_f, g_f = run(True)
    lam_e, g_e = run(False)
    assert torch.equal(lam_e, lam_f)
    E_arr = eng.k_E_arr.cpu()
    assert int(E_arr.min()) < eng.E          # the batch has padded links
    for b in range(eng.B):
        assert torch.equal(lam_e[b, int(E_arr[b]):eng.E],
                           lam_f[b, int(E_arr[b]):eng.E])

    m64 = ChebConvStack(K=2, dtype=torch.float64, seed=11)
    with torch.no_grad():
        for p64, p in zip(m64.parameters(), model.parameters()):
            p64.copy_(p.double().cpu())
    eng64 = EpisodeEngine(cases, m64, device="cpu", dtype=torch.float64)
    x = eng._features(jobs).double().cpu()
    lam64 = m64(x.reshape(eng.B * eng.Ee, 4), eng64.support).reshape(
        eng.B, eng.Ee)
    (lam64 * g.double()).sum().backward()
    for i, p64 in enumerate(m64.parameters()):
        denom = float(p64.grad.abs().max())
        assert denom > 0
        e_full = float((g_f[i] - p64.grad).abs().max()) / denom
        e_edge = float((g_e[i] - p64.grad).abs().max()) / denom
        print(f"param {i} {tuple(p64.shape)}: full-width {e_full:.3e}, "
              f"edge-layer {e_edge:.3e}")
        assert e_edge <= 4.0 * max(e_full, FLOOR), (i, e_edge, e_full)
        assert e_edge < 5e-3, (i, e_edge)
