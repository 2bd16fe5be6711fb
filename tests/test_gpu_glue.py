"""GPU (MI355X) tests of the native per-step glue: the HIP kernels that
replace the torch operations between the episode kernels (fused actor
cotangent, masked Floyd–Warshall load, ChebConv parameter pack / gradient
reduce, feature build, episode summary, job sampling after the draws).

The torch glue (``native_glue=False``, and the fp64 CPU engine) is the
oracle.  Integer and boolean outputs, inf/nan positions and padded slots are
exact; floating outputs that differ only in summation order follow the
convention of docs/KERNELS.md "Stage tests": 8× the error of the fp32 torch
path against the fp64 CPU oracle, measured here and printed."""
import functools

import pytest
import torch

from tests import stage_oracle as so

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")

ACTOR = [(n, c) for n in so.SETS for c in so.ACTOR_CAPS[n]]


def _ext():
    from multihop_offload_amd.ops import dispatch
    return dispatch.require_hip()


def _model(K=2, dtype=torch.float32):
    """The conditioned model of test_engine_gpu_matches_cpu: small weights,
    output bias 0.5 (traffic predictions well inside the queueing model)."""
    from multihop_offload_amd.models.chebconv import ChebConvStack
    model = ChebConvStack(K=K, dtype=torch.float32, seed=3)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.01)
        model.layers[-1].bias.fill_(0.5)
    return model.to(dtype)


def _engine(name, native, cap=0.0, device="cuda", dtype=torch.float32,
            model=None):
    from multihop_offload_amd.engine import EpisodeEngine
    eg = EpisodeEngine(list(so.cases(name)), model or _model(dtype=dtype),
                       device=device, dtype=dtype, delay_clamp=cap,
                       native_glue=native)
    if device == "cuda":
        assert eg.use_hip and eg.native_glue == native
    return eg


def _f32(x):
    return x.to(torch.float32).cuda().contiguous()


def _jobs(name, device="cuda", dtype=torch.float32):
    return so.jobs_to(so.front(name)["jobs"], device, dtype)


def _report(what, err, ref, tol):
    print(f"{what}: kernel error {err:.3e}, fp32-reference error "
          f"{ref:.3e}, tolerance {tol:.3e}")


def _vec_err(got, want):
    """max-abs error over max-abs of the oracle (sums that cancel)."""
    return so.grad_err(got.reshape(1, -1), want.reshape(1, -1))


# ------------------------------------------------------------ actor backward
def _mse(dm, um, written):
    mask = written & torch.isfinite(dm)
    diff = torch.where(mask, dm - um, torch.zeros_like(dm))
    return (diff ** 2).sum() / mask.sum().clamp(min=1).to(dm.dtype)


@needs_gpu
@pytest.mark.parametrize("name,cap", ACTOR)
def test_actor_backward_fused_matches_dense_route(name, cap):
    """actor_head_bwd_fused against actor_head_bwd(grad_dist_matrix(...)):
    dλ bit-equal (same operation order), loss_mse by the convention.  The
    unwritten cells of unit_mtx and the cells of dm outside links and
    diagonal hold NaN in the fused call: nothing may read them.  Set D runs
    the kernel in global-scratch mode."""
    ext = _ext()
    eg = so.engine(name, cap, "float32", "cuda")
    tables = eg._actor_head_tables()
    lam = _f32(so.lam_input(name, cap)[0])
    dm, hist = ext.actor_head_fwd(lam, *tables, eg.N, eg.fp_iters, cap)
    _, um64, written = so.eval_case(name)["want"]
    assert bool(written.any())
    gen = torch.Generator().manual_seed(5)
    ge = _f32(torch.randn(eg.B, eg.Ee, generator=gen))

    cells = torch.zeros(eg.B * eg.N * eg.N, dtype=torch.bool)
    cells[so.dm_cells(so.engine(name, cap))] = True
    cells = cells.reshape(eg.B, eg.N, eg.N).cuda()
    wr = written.cuda()
    assert bool((wr & cells).sum() == wr.sum()), "written outside the cells"
    dm_clean = torch.where(cells, dm, torch.zeros_like(dm))
    um_clean = torch.where(wr, _f32(um64), torch.zeros_like(dm))
    nan = torch.full_like(dm, float("nan"))
    dm_nan = torch.where(cells, dm, nan)
    um_nan = torch.where(wr, um_clean, nan)

    grad_dist, mse_torch = eg.grad_dist_matrix(ge, dm_clean, um_clean, wr)
    dense = ext.actor_head_bwd(grad_dist.contiguous(), lam, hist, *tables,
                               eg.fp_iters, cap)
    fused, mse = ext.actor_head_bwd_fused(ge, dm_nan, um_nan, wr, lam, hist,
                                          *tables, eg.fp_iters, cap)
    torch.cuda.synchronize()
    assert torch.equal(fused, dense)

    dm_c, um_c, wr_c = dm_clean.cpu(), um_clean.cpu(), written
    want = _mse(dm_c.double(), um_c.double(), wr_c)
    ref = so.rel_err(_mse(dm_c, um_c, wr_c), want)
    tol = so.tolerance(ref)
    err = so.rel_err(mse, want)
    _report(f"actor_head_bwd_fused set {name} clamp {cap} loss_mse", err,
            ref, tol)
    assert err <= tol
    assert so.rel_err(mse_torch, want) <= tol


# --------------------------------------------------------------------- APSP
@needs_gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_floyd_warshall_dm_matches_prepared_input(name):
    """floyd_warshall_dm(dm, adj, n_arr) bit-equal to floyd_warshall on the
    torch-prepared matrix, with NaN in every non-adjacent cell of dm; on C
    (n_arr 20/25 in N = 25, N % 4 != 0) the pad rows and columns are +inf
    with a zero diagonal."""
    ext = _ext()
    eg = so.engine(name, 0.0, "float32", "cuda")
    lam = _f32(so.lam_input(name, 0.0)[0])
    dm, _ = ext.actor_head_fwd(lam, *eg._actor_head_tables(), eg.N,
                               eg.fp_iters, 0.0)
    n_arr = eg.k_N_arr if eg._padded else None
    assert (n_arr is not None) == (name == "C")
    inf = torch.full_like(dm, float("inf"))
    w = torch.where(eg._eye, torch.zeros_like(dm),
                    torch.where(eg.adj, dm, inf))
    want = ext.floyd_warshall(w, n_arr)
    got = ext.floyd_warshall_dm(
        torch.where(eg.adj, dm, torch.full_like(dm, float("nan"))), eg.adj,
        n_arr)
    torch.cuda.synchronize()
    assert torch.equal(got, want)
    assert bool(torch.isfinite(got[:, 0, 1:]).any())
    if name == "C":
        n = int(eg.k_N_arr[0])
        assert n == 20 and eg.N == 25
        pad = got[0].clone()
        pad[:n, :n] = float("inf")
        pad[:n, :n].fill_diagonal_(0.0)
        eye = torch.eye(eg.N, dtype=torch.bool, device="cuda")
        assert bool((pad[eye] == 0).all())
        assert bool(torch.isposinf(pad[~eye]).all())


# -------------------------------------------------------------- pack/reduce
@needs_gpu
@pytest.mark.parametrize("K", [2, 3])
def test_cheb_pack_params_bit_equal(K):
    from multihop_offload_amd.ops.functions import pack_cheb_params
    model = _model(K).cuda()
    params = []
    for layer in model.layers:
        params += [layer.weight, layer.bias]
    with torch.no_grad():
        Wp, bp = _ext().cheb_pack_params(params)
        Wt, bt = pack_cheb_params(params)
    assert Wp.shape == Wt.shape and bp.shape == bt.shape
    assert torch.equal(Wp, Wt) and torch.equal(bp, bt)


@functools.lru_cache(maxsize=None)
def _reduce_case():
    """Random per-graph partials (B = 8) for the K=2 model's shapes, flat
    offsets with 3-cell gaps, the fp64 sums and the tolerance."""
    shapes = [tuple(p.shape) for p in _model().parameters()]
    L = len(shapes) // 2
    gen = torch.Generator().manual_seed(11)
    dW = torch.randn(8, L, 2, 32, 32, generator=gen)
    db = torch.randn(8, L, 32, generator=gen)
    start = torch.randn(20000, generator=gen)
    offsets, off = [], 3
    for s in shapes:
        offsets.append(off)
        off += int(torch.Size(s).numel()) + 3
    assert off <= start.numel()

    def sums(dt):
        W, b = dW.to(dt).sum(0), db.to(dt).sum(0)
        out = []
        for i, s in enumerate(shapes):
            out.append(W[i // 2, :s[0], :s[1], :s[2]].reshape(-1)
                       if len(s) == 3 else b[i // 2, :s[0]])
        return out

    want, sum32 = sums(torch.float64), sums(torch.float32)
    ref = max(_vec_err(g, w) for g, w in zip(sum32, want))
    return dict(shapes=shapes, dW=dW, db=db, start=start, offsets=offsets,
                want=want, sum32=sum32, ref=ref, tol=so.tolerance(ref))


@needs_gpu
@pytest.mark.parametrize("accumulate", [False, True])
def test_cheb_reduce_grads(accumulate):
    """Sums over B against dW.double().sum(0) slices; the accumulate mode
    starts from a non-zero buffer (proves +=); cells between the segments
    keep what they held."""
    c = _reduce_case()
    flat = c["start"].cuda().clone()
    _ext().cheb_reduce_grads(c["dW"].cuda(), c["db"].cuda(),
                             [list(s) for s in c["shapes"]], flat,
                             c["offsets"], accumulate)
    flat = flat.cpu()
    touched = torch.zeros_like(flat, dtype=torch.bool)
    worst = ref = 0.0
    for off, want, s32 in zip(c["offsets"], c["want"], c["sum32"]):
        k = want.numel()
        touched[off:off + k] = True
        if accumulate:       # oracle and fp32 reference of start + sum
            before = c["start"][off:off + k]
            want, s32 = before.double() + want, before + s32
        worst = max(worst, _vec_err(flat[off:off + k], want))
        ref = max(ref, _vec_err(s32, want))
    tol = so.tolerance(ref)
    _report(f"cheb_reduce_grads accumulate={accumulate}", worst, ref, tol)
    assert worst <= tol
    assert torch.equal(flat[~touched], c["start"][~touched])


@needs_gpu
def test_fused_adam_route_matches_plain_gradients():
    """Set A, same weights and jobs: with FusedAdam attached the ChebConv
    backward adds into flat_g directly (no autograd gradients); with plain
    parameters it returns ordinary gradients.  flat_g equals the
    concatenated p.grad within the reduce tolerance."""
    from multihop_offload_amd.ops.functions import FusedAdam
    eg_f = _engine("A", True)
    eg_p = _engine("A", True)
    opt = FusedAdam(eg_f.model, lr=1e-4)
    opt.zero_grad()
    fired = {"fused": 0, "plain": 0}    # autograd gradients handed over

    def count(key):
        def hook(grad):     # also called with None where there is none
            fired[key] += grad is not None
        return hook

    for key, eg in (("fused", eg_f), ("plain", eg_p)):
        for p in eg.model.parameters():
            p.register_hook(count(key))
    jobs = _jobs("A")
    eg_f.gnn_episode(jobs, train=True)
    eg_p.gnn_episode(jobs, train=True)
    torch.cuda.synchronize()
    n_params = len(list(eg_p.model.parameters()))
    assert fired == {"fused": 0, "plain": n_params}, fired
    tol = _reduce_case()["tol"]
    off = 0
    for p in eg_p.model.parameters():
        k = p.numel()
        got, want = opt.flat_g[off:off + k], p.grad.reshape(-1)
        assert float(want.abs().max()) > 0
        err = _vec_err(got, want)
        _report(f"FusedAdam route param at {off}", err,
                _reduce_case()["ref"], tol)
        assert err <= tol
        off += k
    assert off == opt.flat_g.numel()


# ------------------------------------------------------------------ features
@needs_gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
def test_cheb_features_equal_torch(name):
    jobs = _jobs(name)
    got = _engine(name, True)._features(jobs)
    want = _engine(name, False)._features(jobs)
    assert got.is_contiguous() and got.shape == want.shape
    assert bool((want[..., 2] != 0).any())
    assert torch.equal(got, want)


# ------------------------------------------------------------------- summary
@needs_gpu
def test_episode_summary():
    """Counts exact, tau by the convention, on delays on both sides of T
    with nan padding; the nan padding stays in the returned delay_emp."""
    eg_n, eg_t = _engine("A", True), _engine("A", False)
    jobs = _jobs("A")
    gen = torch.Generator().manual_seed(2)
    d = torch.rand(eg_n.B, eg_n.Jmax, generator=gen) * 2000.0
    mask = jobs.mask.cpu()
    T = eg_n.T_arr.cpu()
    assert bool(((d > T[:, None]) & mask).any())
    assert bool(((d < T[:, None]) & mask).any()) and bool((~mask).any())
    d = torch.where(mask, d, torch.full_like(d, float("nan")))
    res = eg_n._result(jobs, d.cuda())
    res_t = eg_t._result(jobs, d.cuda())
    assert res.num_jobs.dtype == torch.int64
    assert res.congest.dtype == torch.int64 and res.tau.dtype == torch.float32
    assert torch.equal(res.num_jobs, res_t.num_jobs)
    assert torch.equal(res.congest, res_t.congest)
    assert torch.equal(res.num_jobs.cpu(), mask.sum(1))
    assert torch.equal(torch.isnan(res.delay_emp).cpu(), ~mask)

    def tau(dt):
        de = torch.where(mask, d, torch.zeros_like(d)).to(dt)
        return de.sum(1) / mask.sum(1).to(dt)

    want = tau(torch.float64)
    ref = so.rel_err(tau(torch.float32), want)
    tol = so.tolerance(ref)
    err = so.rel_err(res.tau, want)
    _report("episode_summary tau", err, ref, tol)
    assert err <= tol


# -------------------------------------------------------------- job sampling
@needs_gpu
@pytest.mark.parametrize("name", ["A", "B", "C"])
@pytest.mark.parametrize("load", [0.15, 0.6])
def test_jobs_from_draws_equal_torch(name, load):
    eg_n, eg_t = _engine(name, True), _engine(name, False)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    B, N, J = eg_n.B, eg_n.N, eg_n.Jmax
    scores = torch.rand(B, N, device="cuda", generator=gen)
    r_nj = torch.rand(B, device="cuda", generator=gen)
    r_rates = torch.rand(B, J, device="cuda", generator=gen)
    got = eg_n._jobs_from_draws(scores, r_nj, r_rates, load)
    want = eg_t._jobs_from_draws(scores, r_nj, r_rates, load)
    assert bool(want.mask.any()) and bool((want.rates > 0).any())
    for f in ("sources", "mask", "rates", "ul", "dl"):
        g, w = getattr(got, f), getattr(want, f)
        assert g.dtype == w.dtype and torch.equal(g, w), f


# ------------------------------------------------------------- whole episode
def _episode(eg, jobs):
    for p in eg.model.parameters():
        p.grad = None
    res = eg.gnn_episode(jobs, train=True)
    grads = [p.grad.detach().reshape(-1).cpu().double()
             for p in eg.model.parameters()]
    return res, grads


def _episode_errs(got, want):
    """One figure per output and one per parameter gradient (``grad0`` …:
    each against its own max-abs, never pooled — the output bias's gradient
    is orders of magnitude above the others)."""
    (res, grads), (wres, wgrads) = got, want
    errs = dict(
        tau=so.rel_err(res.tau, wres.tau),
        delay_emp=so.rel_err(res.delay_emp, wres.delay_emp),
        loss_fn=so.rel_err(res.loss_fn.reshape(1), wres.loss_fn.reshape(1)),
        loss_mse=so.rel_err(res.loss_mse.reshape(1),
                            wres.loss_mse.reshape(1)))
    assert len(grads) == len(wgrads)
    for i, (g, w) in enumerate(zip(grads, wgrads)):
        errs[f"grad{i}"] = _vec_err(g, w)
    return errs


@functools.lru_cache(maxsize=None)
def _episode_case(name):
    """fp64 CPU episode (the oracle), the fp32 CPU episode's error against
    it, and the tolerances."""
    j64 = _jobs(name, "cpu", torch.float64)
    want = _episode(_engine(name, False, device="cpu", dtype=torch.float64),
                    j64)
    j32 = _jobs(name, "cpu", torch.float32)
    got32 = _episode(_engine(name, False, device="cpu"), j32)
    assert torch.equal(got32[0].congest, want[0].congest)
    ref = _episode_errs(got32, want)
    return dict(want=want, ref=ref,
                tol={k: so.tolerance(v) for k, v in ref.items()})


@needs_gpu
@pytest.mark.parametrize("name", ["A", "C"])
def test_whole_episode_native_glue_matches_torch_glue(name):
    """Two GPU engines, native_glue on and off, same weights and jobs,
    train=True: integers and the nan pattern equal each other exactly;
    tau, delay_emp, both losses and every parameter gradient (each on its
    own) of both within the convention's tolerance of the fp64 CPU
    episode."""
    case = _episode_case(name)
    jobs = _jobs(name)
    nat = _episode(_engine(name, True), jobs)
    tor = _episode(_engine(name, False), jobs)
    torch.cuda.synchronize()
    for f in ("num_jobs", "congest"):
        assert torch.equal(getattr(nat[0], f), getattr(tor[0], f)), f
        assert torch.equal(getattr(nat[0], f).cpu(),
                           getattr(case["want"][0], f)), f
    assert torch.equal(torch.isnan(nat[0].delay_emp),
                       torch.isnan(tor[0].delay_emp))
    for label, got in (("native", nat), ("torch", tor)):
        errs = _episode_errs(got, case["want"])
        for k, e in errs.items():
            _report(f"episode set {name} {label} glue {k}", e,
                    case["ref"][k], case["tol"][k])
        for k, e in errs.items():
            assert e <= case["tol"][k], (name, label, k, e, case["tol"][k])
