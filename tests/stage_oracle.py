"""Stage-level harness: case sets, input recipes, fp64 oracle wrappers and
error metrics for the per-kernel tests (tests/test_stage_inputs.py on the
CPU, tests/test_gpu_stages.py on the GPU).

The oracle of every stage is the engine's own torch path on
``device="cpu", dtype=torch.float64`` (pinned to the reference agent by
tests/test_engine.py).  Every input is rounded to fp32 first and the oracle
is fed the upcast of that fp32 tensor, so a kernel and the oracle always see
the same numbers.  The same torch path run in fp32 on the CPU gives the
"fp32-reference error" each tolerance is derived from (``tolerance``).

Nothing here needs a GPU.
"""
import functools

import numpy as np
import torch

from multihop_offload_amd.engine import EpisodeEngine, JobBatch
from multihop_offload_amd.graphs import CaseGraph, JobInstance
from multihop_offload_amd.models.chebconv import ChebConvStack
from multihop_offload_amd.queueing import delay_with_fallback, fixed_point_mu

SETS = ("A", "B", "C", "D")
# delay_clamp values per set for the actor-head tests: 0 everywhere and a
# cap of 0.5 on A-C.  On D the band repair does not converge at 0.5 (nor at
# 0.1) within REPAIR_ROUNDS; at 1.0 it does in 7 rounds and leaves 55 % of
# the links congested, 20 % clamped and 25 % on the plain 1/(mu-lam) branch.
CAP = 0.5
ACTOR_CAPS = {"A": (0.0, CAP), "B": (0.0, CAP), "C": (0.0, CAP),
              "D": (0.0, 1.0)}
BAND = 0.03           # every discontinuous decision stays this far from
REPAIR_ROUNDS = 50    # its boundary (relative)
LDS_FLOATS = 160 * 1024 // 4
TOL_FACTOR = 8.0
TOL_CEILING = 1e-3
FP32_EPS = 2.0 ** -23


# --------------------------------------------------------------- case sets
def _large_er(n=430):
    """One ER graph built like test_large_mode_queueing_kernels_match_cpu."""
    rng = np.random.RandomState(0)
    g = CaseGraph(n, t_max=1000, seed=11, gtype="er")
    g.links_init(50.0, rng=rng)
    g.add_relay(0)
    for s in range(2, 10):
        g.add_server(s, 300.0)
    for v in range(10, n):
        if g.roles[v] == 0:
            g.set_mobile_bw(v, 10.0)
    return g


@functools.lru_cache(maxsize=None)
def cases(name):
    from tests.test_engine import _case, _er_case
    from tests.test_gpu import _cases
    if name == "A":
        return tuple(_cases(20, 8))
    if name == "B":
        return (_er_case(2), _er_case(5), _er_case(7))
    if name == "C":
        return (_case(seed=3, n=20).pad_to(25), _case(seed=9, n=25))
    if name == "D":
        return (_large_er(430),)
    if name == "S":
        # decide only: ragged server counts (3 and 2) -> a padded -1 slot
        g = CaseGraph(20, t_max=1000, seed=9, gtype="ba")
        g.links_init(50.0, rng=np.random.RandomState(9))
        g.add_relay(0)
        for s in (2, 3):
            g.add_server(s, 300.0)
        for v in range(4, 20):
            g.set_mobile_bw(v, 10.0)
        return (_cases(20, 1)[0], g)
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def engine(name, cap=0.0, dtype="float64", device="cpu", walk_cap=None,
           fp_iters=10):
    """An EpisodeEngine over a case set (cached; the model is unused — every
    stage is fed its inputs directly)."""
    dt = getattr(torch, dtype)
    model = ChebConvStack(K=2, dtype=dt, seed=0)
    return EpisodeEngine(list(cases(name)), model, device=device, dtype=dt,
                         delay_clamp=cap, walk_cap=walk_cap,
                         fp_iters=fp_iters)


def single_engine(name, b, cap, dtype, fp_iters=10):
    dt = getattr(torch, dtype)
    return EpisodeEngine([cases(name)[b]], ChebConvStack(K=2, dtype=dt,
                                                         seed=0),
                         device="cpu", dtype=dt, delay_clamp=cap,
                         fp_iters=fp_iters)


def lds_plan(eng):
    """The tests' own statement of what the four queueing kernels launch
    with at ``eng``'s shape (anything with N, E, Ee, fp_iters), written from
    the documented formulas and never read off the extension: LDS floats in
    LDS-resident mode and, where the kernel has one, in global-scratch
    ("large") mode, taken when the first is over 160 KiB; 1024 threads from
    E >= 1500 (walk_eval also from N >= 500), else 256."""
    E, Ee, N, it = eng.E, eng.Ee, eng.N, eng.fp_iters
    floats = dict(
        critic=(5 * Ee + (it + 4) * E, 2 * Ee + 3 * E),
        actor_head_fwd=((it + 3) * E, 2 * E),
        actor_head_bwd=((it + 6) * E, 5 * E),
        walk_eval=(3 * E + N, None),
    )
    plan = {}
    for kernel, (small, large) in floats.items():
        is_large = large is not None and small > LDS_FLOATS
        n = large if is_large else small
        wide = E >= 1500 or (kernel == "walk_eval" and N >= 500)
        plan[kernel] = dict(lds_bytes=4 * n, large=is_large,
                            threads=1024 if wide else 256,
                            fits=n <= LDS_FLOATS)
    return plan


def lds_modes(eng):
    """Which of the three queueing kernels run in global-scratch ("large")
    mode."""
    return {k: v["large"] for k, v in lds_plan(eng).items()
            if k != "walk_eval"}


def lds_fits(eng):
    """Which of the four kernels can launch at all: the large-mode limits
    2·Ee + 3·E (critic), 2·E and 5·E (actor head), and walk_eval's
    3·E + N, against 160 KiB."""
    return {k: v["fits"] for k, v in lds_plan(eng).items()}


def real_slots(eng):
    """(B, Ee) bool: real links and real compute slots (the rest is batch
    padding the kernels must leave inert)."""
    comp = torch.zeros(eng.B, eng.Cmax, dtype=torch.bool)
    comp[eng._comp_b, eng._comp_r] = True
    return torch.cat([eng.link_mask, comp], dim=1)


def as32(x):
    """Round to fp32 and return the fp64 upcast (what the oracle is fed)."""
    return x.to(torch.float32).to(torch.float64)


# ------------------------------------------------- fixed point, with history
def mu_history(eng, lam_link):
    """mu_t for t = 0..fp_iters, (B, fp_iters+1, E): the loop of
    queueing.fixed_point_mu with every iterate kept (the last one is asserted
    equal to fixed_point_mu in tests/test_stage_inputs.py)."""
    lam = lam_link.reshape(-1)
    rates = eng.link_rates.reshape(-1)
    mu = rates / (eng.cf_degs.reshape(-1) + 1.0)
    hist = [mu]
    for _ in range(eng.fp_iters):
        busy = torch.clamp(lam / mu, 0.0, 1.0)
        mu = rates / (1.0 + eng.conf.spmv(busy))
        hist.append(mu)
    return torch.stack(hist, 0).reshape(-1, eng.B, eng.E).transpose(0, 1)


def band_marks(eng, lam, cap):
    """(B, Ee) bool: slots whose λ sits within BAND of a branch boundary of
    the queueing model — the clamp of any fixed-point iteration, the
    congestion switch, or (cap > 0) the delay clamp."""
    E = eng.E
    lam_l, lam_n = lam[:, :E], lam[:, E:]
    hist = mu_history(eng, lam_l)                      # (B, it+1, E)
    mark_l = ((lam_l[:, None, :] / hist[:, :-1] - 1.0).abs() < BAND).any(1)
    mu = hist[:, -1]
    mark_l |= (mu - lam_l).abs() / mu < BAND
    bw = eng.bw_comp
    mark_n = (bw - lam_n).abs() / bw < BAND
    if cap > 0:
        mark_l |= (1.0 / ((mu - lam_l) * cap) - 1.0).abs() < BAND
        mark_n |= (1.0 / ((bw - lam_n) * cap) - 1.0).abs() < BAND
    return torch.cat([mark_l, mark_n], dim=1) & real_slots(eng)


def regime(eng, lam, cap):
    """(congested, capped) bool (B, Ee) of the final delay branch."""
    E = eng.E
    mu = torch.cat([mu_history(eng, lam[:, :E])[:, -1], eng.bw_comp], dim=1)
    congested = lam > mu
    capped = torch.zeros_like(congested)
    if cap > 0:
        capped = ~congested & (1.0 / (mu - lam).clamp(min=1e-300) > cap)
    return congested, capped


# ----------------------------------------------------- λ recipe (tests 1-2)
@functools.lru_cache(maxsize=None)
def lam_input(name, cap, seed=0, fp_iters=10):
    """λ_ext (B, Ee), fp64 holding fp32 values: λ_link = μ0·3·u,
    λ_node = bw·1.5·u with u seeded uniform, then repaired away from every
    branch boundary (marked slots ×0.8 per round).  Returns (λ, rounds)."""
    eng = engine(name, cap, fp_iters=fp_iters)
    gen = torch.Generator().manual_seed(seed)
    u = torch.rand(eng.B, eng.Ee, generator=gen, dtype=torch.float64)
    mu0 = eng.link_rates / (eng.cf_degs + 1.0)
    lam = as32(torch.cat([mu0 * 3.0 * u[:, :eng.E],
                          eng.bw_comp * 1.5 * u[:, eng.E:]], dim=1))
    for rounds in range(REPAIR_ROUNDS + 1):
        mark = band_marks(eng, lam, cap)
        if not bool(mark.any()):
            break
        lam = as32(torch.where(mark, lam * 0.8, lam))
    return lam, rounds


def cotangent(eng, seed=1):
    """Standard-normal, deliberately non-symmetric (B, N, N) cotangent."""
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(eng.B, eng.N, eng.N, generator=gen,
                       dtype=torch.float32).to(torch.float64)


def actor_oracle(eng, lam, G):
    """dm, mu_hist and dλ of the torch actor head (the calls of
    engine.actor_forward after the model) in ``eng``'s dtype."""
    dt = eng.dtype
    lam = lam.to(dt).clone().requires_grad_(True)
    B, E = eng.B, eng.E
    lam_link = lam[:, :E].reshape(-1)
    mu = fixed_point_mu(lam_link, eng.link_rates.reshape(-1),
                        eng.cf_degs.reshape(-1), eng.conf, eng.fp_iters)
    link_delay = delay_with_fallback(lam_link, mu, eng.T_link, 101.0,
                                     eng.delay_clamp).reshape(B, E)
    node_delay = delay_with_fallback(lam[:, E:], eng.bw_comp,
                                     eng.T_arr[:, None], 100.0,
                                     eng.delay_clamp)
    dm = eng._delay_matrix(link_delay, node_delay)
    fin = torch.isfinite(dm)
    loss = (torch.where(fin, dm, torch.zeros_like(dm)) * G.to(dt)).sum()
    (dlam,) = torch.autograd.grad(loss, lam)
    with torch.no_grad():
        hist = mu_history(eng, lam[:, :E].detach())
    return dm.detach(), hist, dlam


def dm_cells(eng):
    """Flat (B·N·N) indices of the cells actor_head_fwd documents as
    written: real links in both directions and the whole diagonal."""
    N = eng.N
    diag = (eng._bidx[:, None] * (N * N)
            + torch.arange(N)[None, :] * (N + 1)).reshape(-1)
    return torch.cat([eng._lk_lin01.cpu(), eng._lk_lin10.cpu(), diag.cpu()])


# ------------------------------------------------------------ error metrics
def rel_err(got, want):
    """Max elementwise relative error over finite oracle entries; non-finite
    entries (inf / NaN) must sit at exactly the same places."""
    got = got.detach().cpu().to(torch.float64)
    want = want.detach().cpu().to(torch.float64)
    assert got.shape == want.shape, (got.shape, want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), "NaN positions"
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf), "inf positions"
    assert torch.equal(got[inf], want[inf]), "inf signs"
    fin = torch.isfinite(want)
    if not bool(fin.any()):
        return 0.0
    g, w = got[fin], want[fin]
    zero = w == 0
    assert torch.equal(g[zero], w[zero]), "exact zeros"
    return float(((g - w).abs()[~zero] / w.abs()[~zero]).max()) \
        if bool((~zero).any()) else 0.0


def grad_err(got, want):
    """Per-graph max-abs error over per-graph max-abs of the oracle, worst
    graph (for gradients, which cancel)."""
    got = got.detach().cpu().to(torch.float64).reshape(got.shape[0], -1)
    want = want.detach().cpu().to(torch.float64).reshape(want.shape[0], -1)
    assert got.shape == want.shape
    denom = want.abs().amax(1)
    assert bool((denom > 0).all())
    return float(((got - want).abs().amax(1) / denom).max())


def tolerance(ref_err):
    """Adopted tolerance from the fp32-reference error: 8× (the kernel's
    reduction order and atomics differ from torch's, and the measurement is
    one seed).  A reference error under one fp32 epsilon is that seed's luck
    — every output is rounded to fp32 at least once — so it is floored
    there.  Above TOL_CEILING the inputs are ill-conditioned: widen the
    band, not the tolerance."""
    tol = TOL_FACTOR * max(ref_err, FP32_EPS)
    assert tol <= TOL_CEILING, (ref_err, tol)
    return tol


# ------------------------------------------- jobs, decision, routes (3-5)
# (load, seed) of the JobInstance.sample draw per set; see front() for the
# band repair of the rates
JOB_RECIPE = {"A": (0.6, 0), "B": (0.6, 0), "C": (0.6, 1), "D": (0.6, 0),
              "S": (0.6, 0)}
CRITIC_CAPS = (0.0, CAP)


def sample_jobs(name, load, seed):
    """JobInstance.sample per case, packed, rates rounded to fp32."""
    eng = engine(name)
    insts = [JobInstance.sample(c.mobile_nodes, load,
                                np.random.RandomState(seed + i))
             for i, c in enumerate(cases(name))]
    jb = eng.pack_jobs(insts)
    jb.rates = as32(jb.rates)
    return jb


def jobs_to(jb, device, dtype):
    return JobBatch(sources=jb.sources.to(device), mask=jb.mask.to(device),
                    rates=jb.rates.to(device, dtype),
                    ul=jb.ul.to(device, dtype), dl=jb.dl.to(device, dtype))


def decide_costs(eng, jobs, sp, uds):
    """(B, J, S+1) cost vector of engine.offload_decide ([servers, local];
    padded server slots inf) — recomputed here for the runner-up margin; its
    argmin is asserted equal to offload_decide's dst on the CPU."""
    B, J, S = eng.B, eng.Jmax, eng.S
    bJ = eng._bidx[:, None]
    src = jobs.sources
    local = uds.gather(1, src) * jobs.ul
    srv = eng.servers_safe[:, None, :].expand(B, J, S)
    sp_s = sp[bJ, src].gather(2, srv)
    hop_s = eng.sp_hop[bJ, src].gather(2, srv)
    uds_s = uds.gather(1, srv.reshape(B, -1)).reshape(B, J, S)
    c = (torch.maximum(sp_s * jobs.ul[..., None], hop_s)
         + torch.maximum(sp_s * jobs.dl[..., None], hop_s)
         + torch.maximum(uds_s * jobs.ul[..., None], torch.ones_like(uds_s)))
    c = torch.where(eng.server_mask[:, None, :], c,
                    torch.full_like(c, float("inf")))
    return torch.cat([c, local[..., None]], dim=2)


def decide_margin(costs):
    """Relative gap between the best and the runner-up cost, (B, J)."""
    two = costs.topk(2, dim=2, largest=False).values
    best, second = two[..., 0], two[..., 1]
    gap = (second - best) / best.abs()
    return torch.where(torch.isfinite(second), gap,
                       torch.full_like(gap, float("inf")))


def pad_routes(route_links, H):
    """Oracle route_walk stops at the longest walk; the kernel's table is
    (B, J, H) — pad with -1."""
    B, J, h = route_links.shape
    assert h <= H
    out = torch.full((B, J, H), -1, dtype=torch.int64)
    out[:, :, :h] = route_links
    return out


@functools.lru_cache(maxsize=None)
def front(name, walk_cap=None, fp_iters=10):
    """Everything upstream of stages 3-5 from the fp64 oracle: delay matrix
    from the λ recipe (cap 0), APSP rounded to fp32, jobs, the oracle's
    decision and its integer routes.  Neither depends on the job rates, so
    the rates of jobs that put a slot inside a band (job_marks) are scaled
    by 0.8 per round until none is left."""
    eng = engine(name, 0.0, walk_cap=walk_cap, fp_iters=fp_iters)
    lam, _ = lam_input(name, 0.0, fp_iters=fp_iters)
    dm, _, _ = actor_oracle(eng, lam, torch.zeros(eng.B, eng.N, eng.N,
                                                  dtype=torch.float64))
    with torch.no_grad():
        sp = as32(eng.apsp(dm))
        uds = as32(torch.diagonal(dm, dim1=1, dim2=2))
        load, seed = JOB_RECIPE[name]
        jobs = sample_jobs(name, load, seed)
        dst, _ = eng.offload_decide(jobs, sp, uds)
        eng.overflow_total.zero_()
        rl, nhop = eng.route_walk(jobs, dst, sp)
        overflow = int(eng.overflow_total)
        eng.overflow_total.zero_()
    H = min(eng.walk_cap, 64)
    fr = dict(sp=sp, uds=uds, jobs=jobs, dst=dst, route_links=pad_routes(
        rl, H), nhop=nhop, overflow=overflow, H=H)
    for rounds in range(REPAIR_ROUNDS + 1):
        bad = job_marks(name, fr, fp_iters=fp_iters)
        if not bool(bad.any()):
            break
        jobs.rates = as32(torch.where(bad, jobs.rates * 0.8, jobs.rates))
    fr["rounds"] = rounds
    return fr


def eval_oracle(eng, fr):
    """delay_emp, unit_mtx, written (+ λ, μ, server load) of
    engine.evaluate in ``eng``'s dtype on the front's integer routes."""
    jobs = jobs_to(fr["jobs"], "cpu", eng.dtype)
    with torch.no_grad():
        return eng.evaluate(jobs, fr["dst"], fr["route_links"], fr["nhop"])


# the history stride and every carve offset of the three queueing kernels
# depend on fp_iters; the one numeric case away from the default of 10
FEW_ITERS = 3


def critic_oracle(name, cap, dtype, fr, fp_iters=10):
    """Per-graph loss (B,) and grad_edge (B, Ee) of engine.critic_backward
    in ``dtype``.  The engine returns only the summed loss: per-graph losses
    come from single-case engines where B > 1."""
    eng = engine(name, cap, dtype, fp_iters=fp_iters)
    jobs = jobs_to(fr["jobs"], "cpu", eng.dtype)
    rl, nhop, dst = fr["route_links"], fr["nhop"], fr["dst"]
    grad_edge, loss_sum = eng.critic_backward(jobs, dst, rl, nhop)
    if eng.B == 1:
        return loss_sum.reshape(1), grad_edge
    losses = []
    for b in range(eng.B):
        e1 = single_engine(name, b, cap, dtype, fp_iters)
        J1 = e1.Jmax
        assert not bool(jobs.mask[b, J1:].any())
        jb1 = JobBatch(sources=jobs.sources[b:b + 1, :J1],
                       mask=jobs.mask[b:b + 1, :J1],
                       rates=jobs.rates[b:b + 1, :J1],
                       ul=jobs.ul[b:b + 1, :J1], dl=jobs.dl[b:b + 1, :J1])
        assert int(rl[b].max()) < e1.E
        _, l1 = e1.critic_backward(jb1, dst[b:b + 1, :J1], rl[b:b + 1, :J1],
                                   nhop[b:b + 1, :J1])
        losses.append(l1)
    losses = torch.stack(losses)
    assert torch.allclose(losses.sum(), loss_sum, rtol=1e-5)
    return losses, grad_edge


def critic_lambda(eng, fr):
    """λ_ext (B, Ee) the job loads put on links and compute slots in the
    critic (rate·ul along each route and on the destination's slot)."""
    jobs = fr["jobs"]
    rl, dst = fr["route_links"], fr["dst"]
    load = torch.where(jobs.mask, jobs.rates * jobs.ul,
                       torch.zeros_like(jobs.rates))
    lam = torch.zeros(eng.B, eng.Ee, dtype=torch.float64)
    H = rl.shape[2]
    lam.scatter_add_(1, rl.clamp(min=0).reshape(eng.B, -1),
                     torch.where(rl >= 0, load[..., None].expand(-1, -1, H),
                                 torch.zeros(1, dtype=torch.float64)
                                 ).reshape(eng.B, -1))
    lam.scatter_add_(1, eng.node_vedge.gather(1, dst), load)
    return lam




def route_entries(eng, fr):
    """(seq, valid) (B, J, H+1): each job's route as extended-slot ids — its
    links in order, then its destination's compute slot."""
    rl, dst = fr["route_links"], fr["dst"]
    seq = torch.cat([rl.clamp(min=0),
                     eng.node_vedge.gather(1, dst)[..., None]], dim=2)
    valid = torch.cat([rl >= 0, fr["jobs"].mask[..., None]], dim=2)
    return seq, valid


def critic_units(eng, fr, cap):
    """(λ, unit) (B, Ee) of the critic's queueing model at ``cap``."""
    E = eng.E
    lam = critic_lambda(eng, fr)
    mu = mu_history(eng, lam[:, :E])[:, -1]
    unit = torch.cat([
        delay_with_fallback(lam[:, :E], mu, eng.T_arr[:, None], 101.0, cap),
        delay_with_fallback(lam[:, E:], eng.bw_comp, eng.T_arr[:, None],
                            100.0, cap)], dim=1)
    return lam, unit


def job_marks(name, fr, caps=CRITIC_CAPS, fp_iters=10):
    """(B, J) bool: jobs whose route touches a slot inside a band — for the
    critic (every cap) the three bands of band_marks on the λ the loads
    produce, plus |data·unit − 1| < BAND on a route entry; for walk_eval the
    congestion switch of the empirical evaluator on its own loads
    ((ul+dl)·rate on links, ul·rate on the destination)."""
    eng = engine(name, fp_iters=fp_iters)
    jobs, dst = fr["jobs"], fr["dst"]
    B, E = eng.B, eng.E
    seq, valid = route_entries(eng, fr)
    slot_bad = torch.zeros(B, eng.Ee, dtype=torch.bool)
    entry_bad = torch.zeros_like(valid)
    for cap in caps:
        lam, unit = critic_units(eng, fr, cap)
        slot_bad |= band_marks(eng, lam, cap)
        x = (jobs.ul + jobs.dl)[..., None] * unit.gather(
            1, seq.reshape(B, -1)).reshape(seq.shape)
        entry_bad |= (x - 1.0).abs() < BAND
    _, _, _, lam_e, mu_e, sload = eval_oracle(eng, fr)
    slot_bad[:, :E] |= (mu_e - lam_e).abs() / mu_e < BAND
    bw = eng.proc_bws
    node_bad = (bw - sload).abs() / bw.clamp(min=1e-300) < BAND
    entry_bad[..., -1] |= node_bad.gather(1, dst)
    entry_bad |= slot_bad.gather(1, seq.reshape(B, -1)).reshape(seq.shape)
    return (entry_bad & valid).any(2)


def check_front(name, fr, caps=CRITIC_CAPS, fp_iters=10):
    """Conditions the fp64 oracle alone must meet for stages 3-5; returns
    the list of violated ones (empty = usable)."""
    eng = engine(name, fp_iters=fp_iters)
    jobs, nhop = fr["jobs"], fr["nhop"]
    m = jobs.mask
    bad = []
    if bool(job_marks(name, fr, caps, fp_iters).any()):
        bad.append("a job inside a band")
    if not bool((~m).any()):
        bad.append("no masked-out job")
    if not bool((m & (nhop == 0)).any()):
        bad.append("no local job")
    if not bool((m & (nhop > 0)).any()):
        bad.append("no offloaded job")
    seq, valid = route_entries(eng, fr)
    used = torch.zeros(eng.B, eng.Ee, dtype=torch.bool)
    used.scatter_(1, seq.reshape(eng.B, -1), valid.reshape(eng.B, -1))
    for cap in caps:
        lam, unit = critic_units(eng, fr, cap)
        x = (jobs.ul + jobs.dl)[..., None] * unit.gather(
            1, seq.reshape(eng.B, -1)).reshape(seq.shape)
        if not bool(((x > 1) & valid).any()) \
                or not bool(((x < 1) & valid).any()):
            bad.append(f"cap {cap}: one side of max(x, 1) missing")
        cong, capped = regime(eng, lam, cap)
        if not bool((cong & used).any()) or not bool((~cong & used).any()):
            bad.append(f"cap {cap}: critic not both congested and free")
        if cap > 0 and not bool((capped & used).any()):
            bad.append(f"cap {cap}: no capped slot on a route")
    costs = decide_costs(eng, jobs, fr["sp"], fr["uds"])
    near = (decide_margin(costs) < 1e-5) & m
    if float(near.sum()) > 0.05 * float(m.sum()):
        bad.append("more than 5 % near-tied decisions")
    return bad


# ------------------------------------- per-stage cases: oracle + tolerances
def _actor_errs(eng, got, want):
    """Errors of (dm, mu_hist, dλ) against the fp64 oracle's; exact inf
    positions and exact zeros in padded slots are asserted on the way."""
    dm, hist, dlam = got
    wdm, whist, wdlam = want
    cells = dm_cells(eng)
    lk = eng.link_mask[:, None, :].expand_as(whist)
    pad = ~real_slots(eng)
    assert bool((dlam.detach().cpu()[pad] == 0).all()), "padded dλ not zero"
    return dict(
        dm=rel_err(dm.detach().cpu().reshape(-1)[cells],
                   wdm.reshape(-1)[cells]),
        mu_hist=rel_err(hist.detach().cpu()[lk], whist[lk]),
        dlam=grad_err(dlam, wdlam))


@functools.lru_cache(maxsize=None)
def actor_case(name, cap, fp_iters=10):
    """Inputs, fp64 oracle, fp32-reference errors and adopted tolerances of
    the actor-head tests."""
    e64 = engine(name, cap, fp_iters=fp_iters)
    e32 = engine(name, cap, "float32", fp_iters=fp_iters)
    lam, _ = lam_input(name, cap, fp_iters=fp_iters)
    G = cotangent(e64)
    want = actor_oracle(e64, lam, G)
    ref = _actor_errs(e64, actor_oracle(e32, lam, G), want)
    return dict(lam=lam, G=G, want=want, ref=ref,
                tol={k: tolerance(v) for k, v in ref.items()})


def _critic_errs(eng, got, want):
    loss, ge = got
    wloss, wge = want
    pad = ~real_slots(eng)
    assert bool((ge.detach().cpu()[pad] == 0).all()), "padded grad_edge"
    return dict(loss=rel_err(loss, wloss), grad_edge=grad_err(ge, wge))


@functools.lru_cache(maxsize=None)
def critic_case(name, cap, fp_iters=10):
    fr = front(name, fp_iters=fp_iters)
    want = critic_oracle(name, cap, "float64", fr, fp_iters)
    ref = _critic_errs(engine(name),
                       critic_oracle(name, cap, "float32", fr, fp_iters),
                       want)
    return dict(front=fr, want=want, ref=ref,
                tol={k: tolerance(v) for k, v in ref.items()})


def _eval_errs(got, want):
    de, um, wr = got
    wde, wum, wwr = want
    assert torch.equal(wr.cpu(), wwr), "written"
    return dict(delay_emp=rel_err(de, wde), unit_mtx=rel_err(um, wum))


@functools.lru_cache(maxsize=None)
def eval_case(name, walk_cap=None):
    fr = front(name, walk_cap)
    want = eval_oracle(engine(name), fr)[:3]
    ref = _eval_errs(eval_oracle(engine(name, 0.0, "float32"), fr)[:3], want)
    return dict(front=fr, want=want, ref=ref,
                tol={k: tolerance(v) for k, v in ref.items()})


@functools.lru_cache(maxsize=None)
def tie_case():
    """Set A's decide inputs with one job made exactly equidistant from two
    servers that are also its cheapest: both sp entries and both uds entries
    are copies of one fp32 value and the hop counts agree, so the two costs
    are bit-identical in fp32 and in fp64 and only the first-minimum rule
    separates them."""
    eng, fr = engine("A"), front("A")
    jobs = fr["jobs"]
    for b in range(eng.B):
        for j in range(eng.Jmax):
            if not bool(jobs.mask[b, j]):
                continue
            src = int(jobs.sources[b, j])
            hop = eng.sp_hop[b, src, eng.servers[b]]
            for s0 in range(eng.S):
                for s1 in range(s0 + 1, eng.S):
                    if float(hop[s0]) != float(hop[s1]):
                        continue
                    sp, uds = fr["sp"].clone(), fr["uds"].clone()
                    n0 = int(eng.servers[b, s0])
                    n1 = int(eng.servers[b, s1])
                    v = as32(torch.tensor(0.03, dtype=torch.float64))
                    sp[b, src, n0] = sp[b, src, n1] = v
                    sp[b, n0, src] = sp[b, n1, src] = v
                    uds[b, n0] = uds[b, n1] = 2.0 ** -10
                    c = decide_costs(eng, jobs, sp, uds)[b, j]
                    others = [k for k in range(eng.S + 1)
                              if k not in (s0, s1)]
                    if float(c[s0]) == float(c[s1]) \
                            and float(c[s0]) < float(c[others].min()):
                        with torch.no_grad():
                            dst, _ = eng.offload_decide(jobs, sp, uds)
                        return dict(jobs=jobs, sp=sp, uds=uds, dst=dst, b=b,
                                    j=j, s0=s0, s1=s1)
    raise AssertionError("no job with two servers at equal hop distance")
