"""GPU (MI355X) tests of the LDS-staged conflict CSR of the contention fixed
point (ops/hip/queue_model.h): the four queueing kernels with the CSR staged
per workgroup against the same kernels forced onto the global-memory CSR, bit
for bit, and the forward recurrence against a numpy float32 replay in CSR
order.  Case sets and input recipes are those of tests/stage_oracle.py.

Nothing here has a tolerance: a staged row is summed in the same order, into
one accumulator from +0, as a row read from global memory, so every output
must be identical."""
import contextlib

import numpy as np
import pytest
import torch

from tests import stage_oracle as so
from tests.test_gpu_stages import _ext, _f32, _gpu_engine, needs_gpu

pytestmark = pytest.mark.gpu

KERNELS = ("critic", "actor_head_fwd", "actor_head_bwd", "walk_eval")


@contextlib.contextmanager
def csr_mode(force_global=False, budget=-1):
    """Launch with the conflict CSR forced to global memory, or staged under
    ``budget`` bytes per workgroup (-1: the built-in default); the default
    is restored afterwards."""
    from multihop_offload_amd.ops import dispatch
    ext = _ext()
    dispatch.queue_csr_force_global(force_global)
    ext.queue_csr_set_budget(budget)
    try:
        yield
    finally:
        dispatch.queue_csr_force_global(False)
        ext.queue_csr_set_budget(-1)


def _csr_bytes(eg):
    """LDS bytes the staged CSR of each graph of an engine takes."""
    ext = _ext()
    Eb = eg.k_E_arr.cpu().tolist()
    cip = eg.k_conf_indptr.cpu()
    return [ext.queue_csr_bytes(e, int(cip[b, e])) for b, e in enumerate(Eb)]


def _staged(eg, fp_iters=None):
    """Per kernel, which graphs of the engine the next launch would stage:
    the launch's budget (ext.queue_csr_stage) against each graph's bytes."""
    it = eg.fp_iters if fp_iters is None else fp_iters
    stage = _ext().queue_csr_stage(eg.N, eg.E, eg.Ee, it)
    need = _csr_bytes(eg)
    return {k: [0 <= n <= stage[k]["budget_bytes"] for n in need]
            for k in KERNELS}


def _bits(x):
    """Float tensors compare by bit pattern (NaN positions and signs of zero
    included), everything else by value."""
    return x.view(torch.int32) if x.dtype == torch.float32 else x


def _same(a, b):
    return a.shape == b.shape and torch.equal(_bits(a), _bits(b))


def _tables(eg, conf=None):
    cip, base, cols = conf or (eg.k_conf_indptr, eg.k_conf_base,
                               eg.k_conf_cols)
    return (cip, base, cols, eg.link_rates.contiguous(),
            eg.bw_comp.contiguous(), eg.k_edges, eg.node_vedge,
            eg.T_arr.contiguous(), eg.k_E_arr)


def _dm_cells(eg):
    """Flat indices of the cells actor_head_fwd writes: both directions of
    every real link and the whole diagonal (the rest of dm is left
    uninitialised)."""
    B, N, E = eg.B, eg.N, eg.E
    real = (torch.arange(E, device="cuda")[None, :] < eg.k_E_arr[:, None])
    u, v = eg.k_edges[..., 0].long(), eg.k_edges[..., 1].long()
    base = torch.arange(B, device="cuda")[:, None] * (N * N)
    diag = (base + torch.arange(N, device="cuda")[None, :] * (N + 1))
    return torch.cat([(base + u * N + v)[real], (base + v * N + u)[real],
                      diag.reshape(-1)])


def _real_hist(eg, hist):
    """mu_hist over real links (the slots past E_b of a ragged batch are
    never written: whatever the LDS held)."""
    real = torch.arange(eg.E, device="cuda")[None, :] < eg.k_E_arr[:, None]
    return hist[real[:, None, :].expand_as(hist)]


def _run_all(eg, lam, G, jobs, sp, dst, rl, nhop, H, conf=None):
    """Every output of the five launches (actor_head_fwd, walk_eval, critic,
    actor_head_bwd, actor_head_bwd_fused) on one set of inputs.  ``rl`` /
    ``nhop`` None: the critic runs on walk_eval's own routes."""
    ext = _ext()
    tb = _tables(eg, conf)
    it, cap = eg.fp_iters, eg.delay_clamp
    out = {}
    dm, hist = ext.actor_head_fwd(lam, *tb, eg.N, it, cap)
    out["fwd.dm"] = dm.reshape(-1)[_dm_cells(eg)]
    out["fwd.mu_hist"] = _real_hist(eg, hist)
    w = ext.walk_eval(
        sp, jobs.sources, dst, jobs.mask, jobs.rates.contiguous(),
        jobs.ul.contiguous(), jobs.dl.contiguous(), eg.k_adj_indptr,
        eg.k_adj_idx, eg.k_adj_link, tb[0], tb[1], tb[2], tb[3],
        eg.proc_bws.contiguous(), eg.k_edges, eg.T_arr.contiguous(),
        eg.k_E_arr, eg.k_N_arr, H, it)
    for k, x in zip(("route_links", "nhop", "delay_emp", "unit_mtx",
                     "written", "overflow"), w):
        out["walk." + k] = x
    if rl is None:
        rl, nhop = w[0], w[1]
    ge, loss = ext.critic(
        rl, nhop, eg.node_vedge.gather(1, dst).contiguous(), jobs.mask,
        jobs.rates.contiguous(), jobs.ul.contiguous(), jobs.dl.contiguous(),
        tb[0], tb[1], tb[2], tb[3], tb[4], eg.k_E_arr, eg.T_arr.contiguous(),
        eg.Ee, it, cap)
    out["critic.grad_edge"], out["critic.loss"] = ge, loss
    out["bwd.dlam"] = ext.actor_head_bwd(G, lam, hist, *tb, it, cap)
    dl, mse = ext.actor_head_bwd_fused(ge, dm, w[3], w[4], lam, hist, *tb,
                                       it, cap)
    out["bwd_fused.dlam"], out["bwd_fused.loss_mse"] = dl, mse.reshape(1)
    torch.cuda.synchronize()
    return out


def _one_wave_of_jobs(jobs):
    """The kernels add job loads and route gradients into LDS cells with
    float atomics, one job per thread: with jobs in more than one wave the
    order of those adds — and the last bits of the critic's grad_edge and
    walk_eval's units — changes from launch to launch of the same kernel,
    whatever the CSR mode.  Masking out the jobs past the first 64 slots
    keeps every such add inside wave 0, whose order is fixed, so that
    bit-equality tests what it is meant to."""
    mask = jobs.mask.clone()
    mask[:, 64:] = False
    jobs.mask = mask
    return jobs


def _set_inputs(name, fp_iters=10):
    """λ and cotangent of the actor-head recipe, jobs / APSP / decision /
    routes of the oracle's front (job slots 0..63), on the GPU."""
    eg = _gpu_engine(name, fp_iters=fp_iters)
    lam, _ = so.lam_input(name, 0.0, fp_iters=fp_iters)
    fr = so.front(name, fp_iters=fp_iters)
    return eg, dict(
        lam=_f32(lam), G=_f32(so.cotangent(so.engine(name))),
        jobs=_one_wave_of_jobs(so.jobs_to(fr["jobs"], "cuda", torch.float32)),
        sp=_f32(fr["sp"]), dst=fr["dst"].cuda().contiguous(),
        rl=fr["route_links"].to(torch.int32).cuda().contiguous(),
        nhop=fr["nhop"].to(torch.int32).cuda().contiguous(), H=fr["H"])


def _compare(what, got, want):
    bad = [k for k in want if not _same(got[k], want[k])]
    for k in want:
        print(f"{what} {k}: {'identical' if k not in bad else 'DIFFERS'}")
    assert not bad, (what, bad)


@needs_gpu
@pytest.mark.parametrize("name,fp_iters", [("A", 10), ("A", so.FEW_ITERS),
                                           ("B", 10), ("C", 10)])
def test_staged_csr_equals_global_csr(name, fp_iters):
    """Sets A (E=36, conflict rows of 2 to 20 columns: under one chunk of 8
    up to three, rows starting anywhere inside a chunk) at fp_iters 10 and
    3, B (ragged E_arr 160/158/182, padded link slots, rows of 17 to 36) and
    C (pad nodes): every graph is staged under the default budget (asserted
    from queue_csr_stage and queue_csr_bytes), and every output of the five
    launches is bit-identical to the launch forced onto the global CSR."""
    eg, x = _set_inputs(name, fp_iters)
    staged = _staged(eg)
    assert all(all(v) for v in staged.values()), staged
    got = _run_all(eg, **x)
    with csr_mode(force_global=True):
        assert not any(any(v) for v in _staged(eg).values())
        want = _run_all(eg, **x)
    _compare(f"set {name} fp_iters {fp_iters}", got, want)


@needs_gpu
def test_one_launch_holds_both_modes():
    """Set B with the budget put between the staged sizes of its graphs
    (9424, 9120 and 11952 bytes -> 10688): graphs 0 and 1 stage, graph 2
    reads global memory in the same launch; all outputs equal the
    all-global launch."""
    eg, x = _set_inputs("B")
    need = _csr_bytes(eg)
    budget = (sorted(need)[-2] + sorted(need)[-1]) // 2
    with csr_mode(force_global=True):
        want = _run_all(eg, **x)
    with csr_mode(budget=budget):
        staged = _staged(eg)
        for k in KERNELS:
            assert sorted(staged[k]) == [False, True, True], (k, need, budget)
        got = _run_all(eg, **x)
    _compare(f"set B budget {budget}", got, want)


@needs_gpu
def test_several_rows_per_thread_still_staged():
    """One 150-node BA graph twice in a batch: E = 296 links on 256 threads,
    so threads own two rows and the row bounds and rates come from LDS, not
    registers; staged under the default budget.  Jobs at load 0.6 (slots
    0..63, see _one_wave_of_jobs); the routes are walk_eval's own."""
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from tests.test_gpu import _cases
    eg = EpisodeEngine(_cases(150, 2), ChebConvStack(K=2, dtype=torch.float32, seed=0),
                       device="cuda", dtype=torch.float32)
    assert eg.E > 256 and _ext().queue_lds_plan(
        eg.N, eg.E, eg.Ee, eg.fp_iters)["critic"]["threads"] == 256
    assert all(all(v) for v in _staged(eg).values())
    gen = torch.Generator(device="cuda").manual_seed(0)
    jobs = _one_wave_of_jobs(eg.sample_jobs(0.6, gen))
    assert int(jobs.mask.sum()) > 32
    u = torch.rand(eg.B, eg.Ee, device="cuda", generator=gen)
    mu0 = eg.link_rates / (eg.cf_degs + 1.0)
    lam = torch.cat([mu0 * 3.0 * u[:, :eg.E], eg.bw_comp * 1.5 * u[:, eg.E:]],
                    dim=1).contiguous()
    G = torch.randn(eg.B, eg.N, eg.N, device="cuda", generator=gen)
    dm, _ = _ext().actor_head_fwd(lam, *_tables(eg), eg.N, eg.fp_iters, 0.0)
    sp = eg.apsp(dm)
    dst, _ = eg.offload_decide(jobs, sp, torch.diagonal(dm, dim1=1, dim2=2))
    x = dict(lam=lam, G=G, jobs=jobs, sp=sp.contiguous(),
             dst=dst.contiguous(), rl=None, nhop=None,
             H=min(eg.walk_cap, 64))
    got = _run_all(eg, **x)
    assert int(got["walk.overflow"].sum()) == 0
    assert int(got["walk.nhop"].max()) > 0
    with csr_mode(force_global=True):
        want = _run_all(eg, **x)
    _compare("BA-150", got, want)


@needs_gpu
def test_set_d_takes_the_global_path():
    """Set D (E=3220, 97070 conflict entries, 219920 staged bytes) is over
    any budget a launch can carry: with the default setting every kernel
    reads the CSR from global memory (from queue_csr_stage / queue_csr_bytes)
    whether or not its launch has a staging area, and the outputs equal the
    forced-global ones."""
    eg, x = _set_inputs("D")
    stage = _ext().queue_csr_stage(eg.N, eg.E, eg.Ee, eg.fp_iters)
    (need,) = _csr_bytes(eg)
    for k in KERNELS:
        assert need > stage[k]["budget_bytes"], (k, need, stage[k])
    assert not any(any(v) for v in _staged(eg).values())
    got = _run_all(eg, **x)
    with csr_mode(force_global=True):
        want = _run_all(eg, **x)
    _compare("set D", got, want)


def test_csr_stage_leaves_the_plan_alone():
    """Host only.  queue_lds_plan is what it was (pinned by
    tests/test_gpu_stages.py); the staging area is reported next to it:
    the set budget where plan bytes + budget stay within 160 KiB less the
    kernels' static words, else 0, and 0 when forced global.  Staged bytes
    are 16-byte-rounded (E+1) ints + E floats + nnz 16-bit columns; more
    than 65535 links cannot be staged."""
    try:
        ext = _ext()
    except RuntimeError:
        pytest.skip("HIP extension not built")
    a16 = lambda n: (n + 15) // 16 * 16                     # noqa: E731
    for E, nnz in ((36, 322), (196, 3238), (1, 0), (65535, 7)):
        assert ext.queue_csr_bytes(E, nnz) == (a16(4 * (E + 1)) + a16(4 * E)
                                               + a16(2 * nnz))
    assert ext.queue_csr_bytes(65536, 7) == -1
    assert ext.queue_csr_bytes(196, 3238) <= 16384
    limit = 160 * 1024
    for N, E, Ee, it in ((20, 36, 55, 10), (100, 196, 300, 10),
                         (430, 3220, 3649, 10), (430, 3150, 3158, 10),
                         (430, 13000, 13008, 10)):
        plan = ext.queue_lds_plan(N, E, Ee, it)
        for budget in (-1, 8192, 65536):
            with csr_mode(budget=budget):
                stage = ext.queue_csr_stage(N, E, Ee, it)
                assert ext.queue_lds_plan(N, E, Ee, it) == plan
            b = 16384 if budget < 0 else budget
            for k in KERNELS:
                fits = a16(plan[k]["lds_bytes"]) + b + 64 <= limit
                assert stage[k] == {"budget_bytes": b if fits else 0}, (
                    N, E, k, budget, stage[k], plan[k])
        with csr_mode(force_global=True):
            stage = ext.queue_csr_stage(N, E, Ee, it)
            assert all(stage[k]["budget_bytes"] == 0 for k in KERNELS)
    seen = [ext.queue_csr_stage(430, E, E + 8, 10)["actor_head_fwd"]
            ["budget_bytes"] for E in (3150, 13000)]
    # 13·3150 floats sit 40 bytes under the limit: no room for an area;
    # at 13000 links the history is in global scratch and the area fits
    assert seen == [0, 16384]


# ----------------------------------------------------------- ordering oracle
def _replay_mu_hist(cip, cols, base, E_arr, rates, lam, iters):
    """numpy float32 replay of fixed_point_fwd, graph by graph: mu_0 =
    rates / (deg + 1); busy = clamp(lam / mu, 0, 1); mu = rates / (1 + sum of
    busy over the row in CSR order, one accumulator from +0).  The sum runs
    column position by column position over all rows at once; rows that have
    ended add +0, which changes nothing."""
    B, E = rates.shape
    f = np.float32
    out = np.zeros((B, iters + 1, E), dtype=f)
    for b in range(B):
        Eb = int(E_arr[b])
        rp = cip[b, :Eb + 1].astype(np.int64)
        cc = cols[int(base[b]):int(base[b]) + int(rp[Eb])].astype(np.int64)
        deg = (rp[1:] - rp[:-1])
        r, lm = rates[b, :Eb].astype(f), lam[b, :Eb].astype(f)
        mu = r / (deg.astype(f) + f(1.0))
        out[b, 0, :Eb] = mu
        for t in range(1, iters + 1):
            q = lm / mu
            busy = np.where(q < 0, f(0), np.where(q > 1, f(1), q)).astype(f)
            acc = np.zeros(Eb, dtype=f)
            for k in range(int(deg.max()) if Eb else 0):
                on = k < deg
                idx = np.where(on, rp[:-1] + k, 0)
                acc = (acc + np.where(on, busy[cc[idx]] if len(cc) else f(0),
                                      f(0))).astype(f)
            mu = (r / (f(1.0) + acc)).astype(f)
            out[b, t, :Eb] = mu
    return out


def _hist_vs_replay(eg, lam, conf=None):
    tb = _tables(eg, conf)
    _, hist = _ext().actor_head_fwd(lam, *tb, eg.N, eg.fp_iters, 0.0)
    torch.cuda.synchronize()
    want = _replay_mu_hist(
        tb[0].cpu().numpy(), tb[2].cpu().numpy(), tb[1].cpu().numpy(),
        eg.k_E_arr.cpu().numpy(), tb[3].cpu().numpy(), lam.cpu().numpy(),
        eg.fp_iters)
    real = (np.arange(eg.E)[None, :] < eg.k_E_arr.cpu().numpy()[:, None])
    real = np.broadcast_to(real[:, None, :], want.shape)
    got = hist.cpu().numpy()
    diff = int((got.view(np.int32)[real] != want.view(np.int32)[real]).sum())
    return hist, diff, int(real.sum())


@needs_gpu
@pytest.mark.parametrize("name", ["A", "B"])
def test_mu_hist_is_the_csr_order_recurrence(name):
    """mu_hist of actor_head_fwd over the real links of sets A and B equals
    the numpy float32 replay bit for bit, staged and forced global.  The
    forward has no a*b+c for the compiler to contract, and fp32 division
    and addition are correctly rounded on both sides.  (The kernels before
    the staged CSR met the same replay: 0 differing values on A and B.)"""
    eg = _gpu_engine(name)
    lam = _f32(so.lam_input(name, 0.0)[0])
    for what, mode in (("staged", {}), ("global", {"force_global": True})):
        with csr_mode(**mode):
            _, diff, n = _hist_vs_replay(eg, lam)
        print(f"set {name} {what}: {diff} of {n} mu_hist values differ from "
              "the float32 replay")
        assert diff == 0, (name, what, diff, n)


def _without_link0_conflicts(eg):
    """Set A's conflict CSR with every conflict of link 0 of every graph
    taken out: row 0 becomes empty (degree 0) and the rows that named it
    lose a column, so row starts move inside their chunks."""
    cip = eg.k_conf_indptr.cpu().numpy()
    cols = eg.k_conf_cols.cpu().numpy()
    base = eg.k_conf_base.cpu().numpy()
    Eb = eg.k_E_arr.cpu().numpy()
    new_cip, new_cols, new_base = np.zeros_like(cip), [], []
    for b in range(eg.B):
        new_base.append(sum(len(c) for c in new_cols))
        n = 0
        for e in range(cip.shape[1] - 1):
            row = cols[base[b] + cip[b, e]:base[b] + cip[b, e + 1]]
            row = row[row != 0] if e != 0 and e < Eb[b] else row[:0]
            new_cols.append(row)
            n += len(row)
            new_cip[b, e + 1] = n
    to = lambda a, dt: torch.as_tensor(a, dtype=dt).cuda()   # noqa: E731
    return (to(new_cip, torch.int32), to(np.asarray(new_base), torch.int64),
            to(np.concatenate(new_cols), torch.int32))


@needs_gpu
def test_empty_conflict_row():
    """Set A has no link without conflicts, so one is made (link 0 of every
    graph): mu_hist equals the replay bit for bit in both modes (the empty
    row keeps mu = rate), and the actor head's dm, mu_hist and dλ are
    identical staged and global."""
    eg = _gpu_engine("A")
    conf = _without_link0_conflicts(eg)
    assert bool((conf[0][:, 1] == 0).all()) and int(conf[0].max()) > 0
    lam = _f32(so.lam_input("A", 0.0)[0])
    G = _f32(so.cotangent(so.engine("A")))
    outs = {}
    for what, mode in (("staged", {}), ("global", {"force_global": True})):
        with csr_mode(**mode):
            hist, diff, n = _hist_vs_replay(eg, lam, conf)
            tb = _tables(eg, conf)
            dm, _ = _ext().actor_head_fwd(lam, *tb, eg.N, eg.fp_iters, 0.0)
            dlam = _ext().actor_head_bwd(G, lam, hist, *tb, eg.fp_iters, 0.0)
            torch.cuda.synchronize()
        print(f"empty row, {what}: {diff} of {n} mu_hist values differ")
        assert diff == 0
        assert torch.equal(hist[:, :, 0],
                           eg.link_rates[:, None, 0].expand(-1, hist.shape[1]))
        outs[what] = {"dm": dm.reshape(-1)[_dm_cells(eg)], "mu_hist": _real_hist(eg, hist),
                      "dlam": dlam}
    _compare("empty row", outs["staged"], outs["global"])
