"""GPU (MI355X) stage tests: each fused episode-stage HIP kernel on its own,
fed the same fp32 stage inputs as the engine's fp64 CPU torch path (the
oracle; recipes, metrics and tolerances in tests/stage_oracle.py, input
conditioning proven in tests/test_stage_inputs.py).

Tolerances are 8× the error of the same torch path run in fp32 on the CPU
against the fp64 oracle, per output and per set; integer and boolean
outputs, zeros in padded slots and inf/NaN positions are exact.  Measured
figures (fp32-reference error, adopted tolerance, kernel error on an
MI355X) are tabulated in docs/KERNELS.md, "Stage tests"."""
import types

import numpy as np
import pytest
import torch

from tests import stage_oracle as so

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")

ACTOR = [(n, c) for n in so.SETS for c in so.ACTOR_CAPS[n]]
CRITIC = [(n, c) for n in so.SETS for c in so.CRITIC_CAPS]


def _ext():
    from multihop_offload_amd.ops import dispatch
    return dispatch.require_hip()


def _gpu_engine(name, cap=0.0, walk_cap=None, fp_iters=10):
    eg = so.engine(name, cap, "float32", "cuda", walk_cap, fp_iters)
    assert eg.use_hip
    return eg


def _f32(x):
    return x.to(torch.float32).cuda().contiguous()


def _check(stage, name, what, errs, case):
    """Print every figure, then assert each against its tolerance."""
    for k, e in errs.items():
        print(f"{stage} set {name} {what} {k}: kernel error {e:.3e}, "
              f"fp32-reference error {case['ref'][k]:.3e}, tolerance "
              f"{case['tol'][k]:.3e}")
    for k, e in errs.items():
        assert e <= case["tol"][k], (stage, name, what, k, e, case["tol"][k])


def _actor_kernels(eg, lam, G):
    ext = _ext()
    tables = (eg.k_conf_indptr, eg.k_conf_base, eg.k_conf_cols,
              eg.link_rates.contiguous(), eg.bw_comp.contiguous(), eg.k_edges,
              eg.node_vedge, eg.T_arr.contiguous(), eg.k_E_arr)
    lam_g = _f32(lam)
    dm, hist = ext.actor_head_fwd(lam_g, *tables, eg.N, eg.fp_iters,
                                  eg.delay_clamp)
    dlam = ext.actor_head_bwd(_f32(G), lam_g, hist, *tables, eg.fp_iters,
                              eg.delay_clamp)
    torch.cuda.synchronize()
    return dm, hist, dlam


def _plan(eng):
    """The launchers' own plan at an engine's (or any) shape."""
    return _ext().queue_lds_plan(eng.N, eng.E, eng.Ee, eng.fp_iters)


@needs_gpu
def test_set_d_runs_all_three_queueing_kernels_in_large_mode():
    """Asked of the launchers (ext.queue_lds_plan) and stated independently
    (so.lds_plan: critic 5·Ee + 14·E, actor_head_fwd 13·E, actor_head_bwd
    16·E floats against 160 KiB = 40960): set D (E=3220, Ee=3649) is over
    all three and at E >= 1500 launches 1024 threads, while walk_eval's
    3·E + N still fits LDS; sets A-C are under all three."""
    eg = _gpu_engine("D")
    plan, want = _plan(eg), so.lds_modes(eg)
    assert all(want.values())
    assert {k: plan[k]["large"] for k in want} == want
    assert eg.E >= 1500
    assert all(p["threads"] == 1024 for p in plan.values())
    walk = plan["walk_eval"]
    assert walk["fits"] and not walk["large"] and so.lds_fits(eg)["walk_eval"]
    assert eg.hip_walk_ok and eg.hip_critic_ok and eg.hip_actor_ok
    for name in "ABC":
        e = _gpu_engine(name)
        assert not any(so.lds_modes(e).values())
        assert not any(p["large"] for p in _plan(e).values())


def _shape(N, E, Ee, fp_iters):
    return types.SimpleNamespace(N=N, E=E, Ee=Ee, fp_iters=fp_iters)


def _last_small(kernel, fp_iters):
    """Largest E (Ee = E + 8, N = 430) at which so.lds_plan keeps ``kernel``
    LDS-resident."""
    E = 1
    while not so.lds_plan(_shape(430, E + 1, E + 9, fp_iters))[kernel]["large"]:
        E += 1
    return E


def test_queue_lds_plan_matches_the_stated_formulas():
    """ext.queue_lds_plan (host only, nothing is launched) against
    so.lds_plan, which states the formulas on its own: lds_bytes, large,
    threads and fits of all four kernels on sets A-D and on both sides of
    every switch point, at fp_iters 10 and 3.  At 10 the switches are
    E = 3150/3151 (actor_head_fwd, 13·E), 2560/2561 (actor_head_bwd, 16·E)
    and 2153/2154 with Ee = E + 8 (critic, 5·Ee + 14·E); the large-mode
    limits of the actor head are 5·E at E = 8192/8193 and 2·E at
    20480/20481, walk_eval's 3·E + N at N = 430 is E = 13510/13511, and the
    thread count changes at E = 1499/1500 and, for walk_eval, N = 499/500."""
    try:
        ext = _ext()
    except RuntimeError:
        pytest.skip("HIP extension not built")
    assert _last_small("actor_head_fwd", 10) == 3150
    assert _last_small("actor_head_bwd", 10) == 2560
    assert _last_small("critic", 10) == 2153
    shapes = []
    for it in (10, so.FEW_ITERS):
        for name in so.SETS:
            e = so.engine(name)
            shapes.append(_shape(e.N, e.E, e.Ee, it))
        for kernel in ("actor_head_fwd", "actor_head_bwd", "critic"):
            E = _last_small(kernel, it)
            shapes += [_shape(430, E, E + 8, it), _shape(430, E + 1, E + 9, it)]
        for E in (8192, 8193, 20480, 20481, 13510, 13511, 1499, 1500):
            shapes.append(_shape(430, E, E + 8, it))
        for N in (499, 500):
            shapes.append(_shape(N, 1499, 1507, it))
    seen = {k: set() for k in ("large", "fits", "threads")}
    for sh in shapes:
        got = ext.queue_lds_plan(sh.N, sh.E, sh.Ee, sh.fp_iters)
        want = so.lds_plan(sh)
        assert got == want, (vars(sh), got, want)
        for kernel, p in want.items():
            for k in seen:
                seen[k].add((kernel, p[k]))
    # the cases reach both values of every field for every kernel that has two
    kernels = ("critic", "actor_head_fwd", "actor_head_bwd", "walk_eval")
    for kernel in kernels:
        assert {(kernel, 256), (kernel, 1024)} <= seen["threads"]
        assert {(kernel, True), (kernel, False)} <= seen["fits"]
        assert ((kernel, True) in seen["large"]) == (kernel != "walk_eval")


@needs_gpu
@pytest.mark.parametrize("name,cap", ACTOR)
def test_actor_head_fwd_vs_fp64(name, cap):
    """actor_head_fwd alone on a λ that congests 55-60 % of the links (and,
    with the clamp on, clamps 7-37 %): dm on every real link cell in both
    directions and on the diagonal (exactly inf at relays), every row of
    mu_hist over real links; elementwise relative error.
    CPU fp32-reference errors: dm 2.5e-7..1.7e-6, mu_hist 1.7e-7..3.2e-7
    -> tolerances 2.0e-6..1.4e-5 and 1.3e-6..2.6e-6.  Kernel errors on an
    MI355X: dm 2.5e-7..1.7e-6, mu_hist 1.7e-7..3.2e-7 (per set and clamp
    in docs/KERNELS.md)."""
    c = so.actor_case(name, cap)
    eg = _gpu_engine(name, cap)
    dm, hist, dlam = _actor_kernels(eg, c["lam"], c["G"])
    errs = so._actor_errs(so.engine(name, cap), (dm, hist, dlam), c["want"])
    errs.pop("dlam")
    _check("actor_head_fwd", name, f"cap {cap}", errs, c)


@needs_gpu
@pytest.mark.parametrize("name,cap", ACTOR)
def test_actor_head_bwd_vs_fp64(name, cap):
    """actor_head_bwd alone: standard-normal, non-symmetric cotangent G
    against autograd of (where(isfinite(dm), dm, 0)·G).sum() through the
    fp64 torch actor head; the whole (B, Ee) result, exact zeros in padded
    link slots and unused compute slots; per-graph max-abs error over
    per-graph max-abs.  CPU fp32-reference errors 9.3e-8..2.9e-6 ->
    tolerances 9.5e-7..2.3e-5.  Kernel errors on an MI355X 1.5e-7..2.9e-6
    (per set and clamp in docs/KERNELS.md)."""
    c = so.actor_case(name, cap)
    eg = _gpu_engine(name, cap)
    got = _actor_kernels(eg, c["lam"], c["G"])
    errs = so._actor_errs(so.engine(name, cap), got, c["want"])
    _check("actor_head_bwd", name, f"cap {cap}", {"dlam": errs["dlam"]}, c)


def _critic_kernel(eg, fr):
    jobs = so.jobs_to(fr["jobs"], "cuda", torch.float32)
    dst = fr["dst"].cuda()
    ge, loss = _ext().critic(
        fr["route_links"].to(torch.int32).cuda().contiguous(),
        fr["nhop"].to(torch.int32).cuda().contiguous(),
        eg.node_vedge.gather(1, dst).contiguous(), jobs.mask,
        jobs.rates.contiguous(), jobs.ul.contiguous(), jobs.dl.contiguous(),
        eg.k_conf_indptr, eg.k_conf_base, eg.k_conf_cols,
        eg.link_rates.contiguous(), eg.bw_comp.contiguous(), eg.k_E_arr,
        eg.T_arr.contiguous(), eg.Ee, eg.fp_iters, eg.delay_clamp)
    torch.cuda.synchronize()
    assert loss.shape == (eg.B,) and ge.shape == (eg.B, eg.Ee)
    return loss, ge


@needs_gpu
@pytest.mark.parametrize("name,cap", CRITIC)
def test_critic_vs_fp64(name, cap):
    """ext.critic alone on the oracle's integer routes (local nhop=0 jobs,
    offloaded jobs and masked-out jobs; both sides of max(x, 1); congested,
    free and — with the cap — clamped slots on the routes): per-graph loss
    (elementwise relative) and grad_edge (B, Ee) (per-graph max-abs over
    max-abs) against engine.critic_backward in fp64.  CPU fp32-reference
    errors: loss 9.2e-9..1.2e-7, grad_edge 4.3e-8..2.1e-7 -> tolerances
    9.5e-7 and 9.5e-7..1.6e-6.  Kernel errors on an MI355X (they vary a
    little from run to run with the order of the atomics): loss up to
    1.2e-7, grad_edge up to 2.1e-7 (docs/KERNELS.md)."""
    c = so.critic_case(name, cap)
    loss, ge = _critic_kernel(_gpu_engine(name, cap), c["front"])
    errs = so._critic_errs(so.engine(name), (loss, ge), c["want"])
    _check("critic", name, f"cap {cap}", errs, c)


@needs_gpu
@pytest.mark.parametrize("cap", so.CRITIC_CAPS)
def test_queueing_kernels_at_three_iterations_vs_fp64(cap):
    """actor_head_fwd, actor_head_bwd and critic on set A at fp_iters = 3
    (every other test runs 10): the stride of the mu history and every LDS
    carve offset depend on it.  Same recipes, metrics and fp64 oracle as the
    tests above, with the inputs repaired and the fp32-reference errors
    measured on 3-iteration engines (conditioning proven in
    tests/test_stage_inputs.py).  CPU fp32-reference errors: dm
    3.1e-7..1.5e-6, mu_hist 1.7e-7, dlam 1.9e-7..3.2e-6, loss
    8.8e-8..1.2e-7, grad_edge 1.5e-7 -> tolerances 9.5e-7..2.6e-5.  Kernel
    errors on an MI355X: dm, mu_hist and dlam at clamp 0 equal to the
    reference errors, dlam 1.4e-7 at clamp 0.5, loss 1.2e-7, grad_edge
    6.7e-8 (per output and clamp in docs/KERNELS.md)."""
    it = so.FEW_ITERS
    a = so.actor_case("A", cap, it)
    eg = _gpu_engine("A", cap, fp_iters=it)
    assert eg.fp_iters == it
    got = _actor_kernels(eg, a["lam"], a["G"])
    assert got[1].shape == (eg.B, it + 1, eg.E)
    errs = so._actor_errs(so.engine("A", cap, fp_iters=it), got, a["want"])
    _check("actor_head", "A", f"cap {cap} fp_iters {it}", errs, a)
    c = so.critic_case("A", cap, it)
    loss, ge = _critic_kernel(eg, c["front"])
    errs = so._critic_errs(so.engine("A"), (loss, ge), c["want"])
    _check("critic", "A", f"cap {cap} fp_iters {it}", errs, c)


def _decide(eg, jobs, sp, uds):
    jg = so.jobs_to(jobs, "cuda", torch.float32)
    dst, islocal = _ext().decide(
        _f32(sp), eg.sp_hop.contiguous(), _f32(uds), eg.k_servers,
        jg.sources, jg.mask, jg.ul.contiguous(), jg.dl.contiguous(),
        None, None, 0)
    torch.cuda.synchronize()
    return dst.cpu(), islocal.cpu()


@needs_gpu
@pytest.mark.parametrize("name", so.SETS + ("S",))
def test_decide_greedy_vs_fp64(name):
    """decide (greedy) on the oracle's fp32-rounded APSP and uds: dst and
    islocal equal engine.offload_decide's, except for jobs whose oracle
    best and runner-up costs differ by less than 1e-5 relative (at most 5 %
    of the unmasked jobs; 0 on these inputs).  Masked jobs come back as
    dst = src, islocal = True; set S carries a padded (-1) server slot;
    every set has relay rows with uds = inf."""
    fr = so.front(name)
    e64 = so.engine(name)
    eg = _gpu_engine(name)
    jobs = fr["jobs"]
    dst, islocal = _decide(eg, jobs, fr["sp"], fr["uds"])
    m = jobs.mask
    near = (so.decide_margin(so.decide_costs(e64, jobs, fr["sp"], fr["uds"]))
            < 1e-5) & m
    print(f"decide set {name}: {int(near.sum())} of {int(m.sum())} unmasked "
          f"jobs excluded as near-ties; {int((dst != fr['dst']).sum())} "
          "destinations differ")
    assert float(near.sum()) <= 0.05 * float(m.sum())
    assert torch.equal(dst[~near], fr["dst"][~near])
    assert torch.equal(islocal[~near], (fr["dst"] == jobs.sources)[~near])
    assert torch.equal(dst[~m], jobs.sources[~m]) and bool(islocal[~m].all())


@needs_gpu
def test_decide_exact_tie_takes_first_server():
    """One job of set A made exactly equidistant (bit-identical costs in
    fp32 and fp64) from its two cheapest servers: torch's argmin and the
    kernel's strict `<` both keep the first server slot."""
    t = so.tie_case()
    dst, islocal = _decide(_gpu_engine("A"), t["jobs"], t["sp"], t["uds"])
    b, j = t["b"], t["j"]
    assert int(dst[b, j]) == int(t["dst"][b, j])
    assert int(dst[b, j]) == int(so.engine("A").servers[b, t["s0"]])
    assert not bool(islocal[b, j])


@needs_gpu
@pytest.mark.parametrize("name,walk_cap", [(n, None) for n in so.SETS]
                         + [("A", 2)])
def test_walk_eval_vs_fp64(name, walk_cap):
    """walk_eval alone on the oracle's fp32-rounded APSP and the oracle's
    dst: route_links, nhop, written and the overflow total exactly equal
    engine.route_walk / evaluate's (both sides take a first-minimum argmin
    over identical fp32 values); delay_emp (NaN exactly where masked) and
    unit_mtx (exact zeros where unwritten) elementwise relative.  With
    walk_cap=2 on set A the walks that fall short are counted and the
    truncated routes still agree exactly.  CPU fp32-reference errors:
    delay_emp 1.8e-7..1.4e-6, unit_mtx 2.6e-7..1.4e-6 -> tolerances
    1.4e-6..1.1e-5 and 2.1e-6..1.1e-5.  Kernel errors on an MI355X:
    delay_emp 1.8e-7..1.4e-6, unit_mtx 2.7e-7..1.4e-6 (docs/KERNELS.md)."""
    c = so.eval_case(name, walk_cap)
    fr = c["front"]
    eg = _gpu_engine(name, 0.0, walk_cap)
    assert eg.hip_walk_ok and min(eg.walk_cap, 64) == fr["H"]
    jobs = so.jobs_to(fr["jobs"], "cuda", torch.float32)
    eg.overflow_total.zero_()
    rl, nhop, de, um, wr = eg._episode_eval(jobs, fr["dst"].cuda(),
                                            _f32(fr["sp"]))
    torch.cuda.synchronize()
    assert rl.shape == fr["route_links"].shape
    assert torch.equal(rl.cpu().to(torch.int64), fr["route_links"])
    assert torch.equal(nhop.cpu().to(torch.int64), fr["nhop"])
    assert int(eg.overflow_total) == fr["overflow"]
    assert (fr["overflow"] > 0) == (walk_cap is not None)
    eg.overflow_total.zero_()
    assert bool(torch.isnan(de.cpu()[~fr["jobs"].mask]).all())
    errs = so._eval_errs((de, um, wr), c["want"])
    _check("walk_eval", name, f"walk_cap {walk_cap}", errs, c)


def _adam_ref(p, g, m, v, t, scale, lr, b1, b2, eps):
    """fp64 reference of the documented FusedAdam pipeline on one tensor:
    scale -> clipnorm 1.0 -> Adam(eps) -> max_norm 1.0; a tensor whose
    gradient norm is not finite keeps p, m, v (max_norm still applies).
    The hyper-parameters arrive rounded to fp32, as the kernel gets them."""
    g = g * scale
    nrm = g.norm()
    if bool(torch.isfinite(nrm)):
        g = g / nrm if float(nrm) > 1.0 else g
        m = b1 * m + (1 - b1) * g
        v = b2 * v + (1 - b2) * g * g
        p = p - lr * (m / (1 - b1 ** t)) / (torch.sqrt(v / (1 - b2 ** t))
                                            + eps)
    if p.dim() == 3:
        n = torch.sqrt((p * p).sum(0, keepdim=True))
        p = torch.where(n > 1.0, p / n, p)
    else:
        n = p.norm()
        p = p / n if float(n) > 1.0 else p
    return p, m, v


@needs_gpu
def test_fused_adam_skips_non_finite_gradients():
    """Step 1 is finite (so m, v are non-zero).  Before step 2 one weight
    tensor is scaled so that some of its K-axis norms exceed 1, then a NaN
    goes into that tensor's gradient and an inf into one bias tensor's:
    after the step those tensors' m and v are bit-identical to before, the
    bias tensor's p too, and the weight tensor's p is bit-identical except
    where max_norm — which still applies — rescaled a column; every other
    tensor follows the fp64 pipeline, the step counter advances by one per
    step, and the all-finite step 3 updates every tensor.
    Tolerances (fp32 arithmetic on |p| <= 1.3 with an update of about lr =
    1e-3 per step): p within 1e-6 absolute (a few ulp of p plus 1e-4 of
    the update); m and v within 1e-5 relative plus 1e-6 of the tensor's
    largest entry for elements that cancel (the fp32-rounded betas are
    shared with the reference, leaving only product rounding)."""
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.ops.functions import FusedAdam

    def f32(x):
        return float(np.float32(x))

    lr, b1, b2, eps, scale = f32(1e-3), f32(0.9), f32(0.999), f32(1e-7), 0.5
    model = ChebConvStack(K=2, dtype=torch.float32, seed=7).cuda()
    params = list(model.parameters())
    w_bad, b_bad = 2, 5               # layer-1 weight, layer-2 bias
    with torch.no_grad():
        params[b_bad].fill_(0.1)      # norm 0.57: untouched by max_norm
    opt = FusedAdam(model, lr=1e-3)
    gen = torch.Generator().manual_seed(0)
    ref = [(p.detach().cpu().double(), torch.zeros_like(p.cpu()).double(),
            torch.zeros_like(p.cpu()).double()) for p in params]

    def views(buf):
        out, off = [], 0
        for p in params:
            out.append(buf[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return out

    def close(got, want, what):
        got = got.detach().cpu().double()
        bound = 1e-5 * want.abs() + 1e-6 * want.abs().max()
        assert bool(((got - want).abs() <= bound).all()), what

    for t, poisoned in ((1, False), (2, True), (3, False)):
        grads = [torch.randn(p.shape, generator=gen)
                 * (10.0 if i % 3 else 0.01) for i, p in enumerate(params)]
        if poisoned:
            with torch.no_grad():
                params[w_bad].mul_(4.0)        # exact in fp32 and fp64
            pw, mw, vw = ref[w_bad]
            ref[w_bad] = (pw * 4.0, mw, vw)
            grads[w_bad][1, 3, 5] = float("nan")
            grads[b_bad][7] = float("inf")
        before = [(p.detach().clone(), m.clone(), v.clone())
                  for p, m, v in zip(params, views(opt.m), views(opt.v))]
        opt.zero_grad()
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        opt.step(scale=scale)
        torch.cuda.synchronize()
        assert int(opt.step_dev) == t
        ref = [_adam_ref(p, g.double(), m, v, t, scale, lr, b1, b2, eps)
               for (p, m, v), g in zip(ref, grads)]
        for i, (p, m, v) in enumerate(zip(params, views(opt.m),
                                          views(opt.v))):
            p0, m0, v0 = before[i]
            if poisoned and i in (w_bad, b_bad):
                assert bool((m0 != 0).any()) and bool((v0 != 0).any())
                assert torch.equal(m, m0) and torch.equal(v, v0), i
                if i == b_bad:
                    assert torch.equal(p.detach(), p0)
                else:
                    n = torch.sqrt((p0.double() ** 2).sum(0))
                    assert bool((n > 1.01).any()) and bool((n < 0.99).any())
                    keep = (n < 0.99).expand_as(p0)
                    assert torch.equal(p.detach()[keep], p0[keep])
                    clip = (n > 1.01).expand_as(p0)
                    assert bool((p.detach()[clip] != p0[clip]).any())
            else:
                assert not torch.equal(p.detach(), p0), (t, i)
            assert bool(torch.isfinite(p).all())
            assert float((p.detach().cpu().double() - ref[i][0]).abs().max()) \
                <= 1e-6, (t, i)
            close(m, ref[i][1], (t, i, "m"))
            close(v, ref[i][2], (t, i, "v"))


@needs_gpu
@pytest.mark.parametrize("N", [200, 201])
def test_fw_at_the_lds_switch_point(N):
    """The LDS kernel holds N·ceil4(N) floats in 160 KiB: 200·200·4 =
    160000 fits, 201·204·4 = 164016 does not (tiled kernels).  Both sides
    of the switch against the fp64 reference, tolerances of the existing
    FW tests.  At N = 200 also n_arr = [200, 193] passed directly: the
    second graph's rows/columns >= 193 are inf with a zero diagonal (as
    engine.apsp pads them) and the result equals the run without n_arr."""
    from multihop_offload_amd.ops import dispatch, torch_ref
    from tests.test_gpu import _rand_w
    assert (200 * 200 * 4 <= 160 * 1024) and (201 * 204 * 4 > 160 * 1024)
    w = _rand_w(2, N)
    want = torch_ref.floyd_warshall(w.double())
    got = dispatch.floyd_warshall(w.cuda()).cpu()
    tol = 1e-5 if N <= 200 else 1e-4
    assert torch.allclose(got.double(), want, rtol=tol, atol=tol)
    if N == 200:
        wp = w.clone()
        wp[1, 193:, :] = float("inf")
        wp[1, :, 193:] = float("inf")
        idx = torch.arange(N)
        wp[1, idx, idx] = 0.0
        want_p = torch_ref.floyd_warshall(wp.double())
        n_arr = torch.tensor([200, 193], dtype=torch.int32, device="cuda")
        got_n = dispatch.floyd_warshall(wp.cuda(), n_arr).cpu()
        got_p = dispatch.floyd_warshall(wp.cuda()).cpu()
        assert torch.equal(got_n, got_p)
        assert torch.allclose(got_n.double(), want_p, rtol=tol, atol=tol)
        assert bool(torch.isinf(got_n[1, 193:, :193]).all())
