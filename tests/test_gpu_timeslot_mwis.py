"""GPU (MI355X) tests of the packet simulator's scheduled MAC
(``timeslot_sim_mwis`` / ``timeslot_sim_mwis_stats`` in ops/hip/timeslot.hip,
``EpisodeEngine.simulate(mac="mwis")``).

As in test_gpu_timeslot.py the oracle is ``simulate_routes`` on fp64 copies
of the arrays after rounding through ``np.float32``, on the routes the GPU
episode produced, and every comparison is integer equality: the weights are
one fp64 multiply of the same two operands on both sides, so every
comparison of the schedule agrees and nothing needs a tolerance."""
import functools
import json
import os

import numpy as np
import pytest
import torch

from multihop_offload_amd.sim.timeslot import STAT_KEYS, simulate_routes
from tests import timeslot_cases as tc
from tests import timeslot_mwis_cases as mc

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATE = 8


def _engine(cases):
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
    eng = EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)
    assert eng.use_hip
    return eng


def _np(x):
    return x.detach().cpu().numpy()


@functools.lru_cache(maxsize=None)
def run(name):
    cases, jobs_list = tc.g2_batch() if name == "g2" else tc.g1_batch()
    eng = _engine(cases)
    jobs = eng.pack_jobs(jobs_list)
    res = (eng.local_episode(jobs) if name == "g4"
           else eng.baseline_episode(jobs))
    arr = tc.batch_arrivals(jobs_list, eng.Jmax)
    sim = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                       trace=True, mac="mwis")
    routes = (_np(res.dst), _np(res.route_links), _np(res.nhop))
    ref = mc.oracle_batch(cases, jobs_list, *routes, arr)
    return cases, jobs_list, eng, jobs, res, arr, sim, routes, ref


def _check_equal(name):
    cases, jobs_list, eng, jobs, res, arr, sim, routes, ref = run(name)
    ds, ct, tr, sched, rounds, logs = ref
    print(name, "completed", ct.sum(1).tolist(), "rounds_max", rounds)
    assert sim.sched_slots.dtype == torch.int32 and sim.sched_slots.is_cuda
    assert sim.sched_slots.shape == (eng.B, eng.E)
    assert np.array_equal(_np(sim.delay_sum), ds)
    assert np.array_equal(_np(sim.count), ct)
    assert np.array_equal(_np(sim.trace), tr)
    assert np.array_equal(_np(sim.sched_slots), sched)
    mask = _np(jobs.mask)
    assert not _np(sim.delay_sum)[~mask].any()
    assert not _np(sim.count)[~mask].any()
    for b, g in enumerate(cases):
        assert not _np(sim.sched_slots)[b, g.num_links:].any()
    return cases, ds, ct, rounds, logs, routes, jobs_list, arr


@needs_gpu
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_g1_g2_equal_the_oracle(name):
    """G1 (three 20-node cases, masked job slots) and G2 (a 40-node case and
    a 20-node case padded to 40: ragged E and J): delay_sum, count, trace
    and sched_slots equal the oracle; the batch is busy, scheduled
    differently from the fluid sharing, and needs three rounds somewhere."""
    cases, ds, ct, rounds, logs, routes, jobs_list, arr = _check_equal(name)
    if name == "g2":
        assert len({g.num_links for g in cases}) > 1, "E is ragged"
        assert len({j.num_jobs for j in jobs_list}) > 1, "J is ragged"
    share = tc.oracle_batch(cases, jobs_list, *routes, arr)
    mc.check_preconditions(cases, ct, ds, share[0], rounds, logs)


@needs_gpu
def test_g4_local_episode_node_leg_only():
    """G4: nhop = 0 everywhere: no link is ever busy, nothing is scheduled,
    and the node leg alone gives the fluid-sharing run's figures."""
    cases, ds, ct, rounds, logs, routes, jobs_list, arr = _check_equal("g4")
    assert not routes[2].any()
    assert ct.sum() > 100 and rounds == [0, 0, 0]
    sim = run("g4")[6]
    assert not sim.sched_slots.any()
    share = tc.oracle_batch(cases, jobs_list, *routes, arr)
    assert np.array_equal(ds, share[0])


@needs_gpu
def test_g3_tie_break():
    """G3: every contested slot is a tie between the two uplinks; the kernel
    gives the oracle's pair (the lower link id first), not the swapped
    one."""
    from multihop_offload_amd.engine import EpisodeResult
    g, jobs, arr, rl, nhop, dst = tc.g3_case()
    eng = _engine([g])
    jb = eng.pack_jobs([jobs])
    z = torch.zeros(1, device="cuda")
    res = EpisodeResult(
        tau=z, congest=z, num_jobs=z, delay_emp=z,
        dst=torch.as_tensor(dst[None], device="cuda"),
        route_links=torch.as_tensor(rl[None].astype(np.int32),
                                    device="cuda"),
        nhop=torch.as_tensor(nhop[None].astype(np.int32), device="cuda"))
    sim = eng.simulate(jb, res, torch.as_tensor(arr[None]), trace=True,
                       mac="mwis")
    ds, ct, tr, sc = simulate_routes(tc.rounded(g), tc.f32(jobs.ul),
                                     tc.f32(jobs.dl), dst, rl, nhop, arr,
                                     trace=True, mac="mwis")
    got = _np(sim.delay_sum)[0]
    print("oracle delay sums", ds.tolist(), "kernel", got.tolist())
    assert ds[0] > ds[1]
    assert got.tolist() == ds.tolist()
    assert got.tolist() != ds[::-1].tolist()
    assert _np(sim.count)[0].tolist() == ct.tolist()
    assert np.array_equal(_np(sim.trace)[0, :, 2], tr["pkts_in_network"])
    assert np.array_equal(_np(sim.sched_slots)[0], sc["sched_slots"])


@needs_gpu
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_stats_with_mwis(name):
    """stats=True, mac="mwis": every STAT_KEYS tensor and sched_slots equal
    the oracle; the plain sums are those of the statistics-free launch."""
    cases, jobs_list, eng, jobs, res, arr, sim, routes, ref = run(name)
    st_sim = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                          trace=True, stats=True, late_after=LATE,
                          mac="mwis")
    assert torch.equal(st_sim.delay_sum, sim.delay_sum)
    assert torch.equal(st_sim.count, sim.count)
    assert torch.equal(st_sim.trace, sim.trace)
    assert torch.equal(st_sim.sched_slots, sim.sched_slots)
    E = eng.E
    for b, (g, jb) in enumerate(zip(cases, jobs_list)):
        k, Eb = jb.num_jobs, g.num_links
        out = mc.oracle_case(g, jb, routes[0][b], routes[1][b], routes[2][b],
                             arr[b], stats=True, late_after=LATE)
        want, sc = out[-2], out[-1]
        for key in STAT_KEYS:
            got = _np(getattr(st_sim.stats, key))[b]
            if key in STAT_KEYS[:5]:
                assert np.array_equal(got[:k], want[key]), (key, b)
                assert not got[k:].any(), (key, b)
            else:
                assert np.array_equal(got[:Eb], want[key][:Eb]), (key, b)
                assert not got[Eb:E].any(), (key, b)
                n = g.num_nodes
                assert np.array_equal(got[E:E + n], want[key][Eb:]), (key, b)
        assert np.array_equal(_np(st_sim.sched_slots)[b, :Eb],
                              sc["sched_slots"])
        assert (sc["sched_slots"] <= want["busy_slots"][:Eb]).all()
    share = _np(st_sim.sched_share())
    busy = _np(st_sim.stats.busy_slots)[:, :E] > 0
    assert np.isnan(share[~busy]).all() and (share[busy] <= 1).all()


@needs_gpu
def test_default_is_unchanged():
    """simulate() without mac is the fluid-sharing oracle, as before, and
    carries no schedule."""
    cases, jobs_list, eng, jobs, res, arr, sim, routes, ref = run("g1")
    plain = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                         trace=True)
    ds, ct, tr = tc.oracle_batch(cases, jobs_list, *routes, arr)
    assert np.array_equal(_np(plain.delay_sum), ds)
    assert np.array_equal(_np(plain.count), ct)
    assert np.array_equal(_np(plain.trace), tr)
    assert plain.sched_slots is None
    explicit = eng.simulate(jobs, res, torch.as_tensor(arr),
                            warmup=tc.WARMUP, trace=True, mac="share")
    assert torch.equal(explicit.delay_sum, plain.delay_sum)
    assert explicit.sched_slots is None
    with pytest.raises(ValueError):
        eng.simulate(jobs, res, torch.as_tensor(arr), mac="tdma")


@needs_gpu
def test_launches_are_repeatable():
    cases, jobs_list, eng, jobs, res, arr, sim, routes, ref = run("g1")
    again = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                         trace=True, mac="mwis")
    assert torch.equal(again.delay_sum, sim.delay_sum)
    assert torch.equal(again.count, sim.count)
    assert torch.equal(again.trace, sim.trace)
    assert torch.equal(again.sched_slots, sim.sched_slots)


@needs_gpu
@pytest.mark.parametrize("stats", [False, True])
def test_staged_and_global_columns_agree(stats):
    """The conflict columns read from their 16-bit LDS copy (the default
    where they fit the staging area) and from global memory give the same
    integers; G2's 40-node case has the longest rows of the test cases."""
    from multihop_offload_amd.ops import dispatch
    cases, jobs_list, eng, jobs, res, arr, sim, routes, ref = run("g2")
    kw = dict(warmup=tc.WARMUP, trace=True, stats=stats, mac="mwis")
    dispatch.queue_csr_force_global(True)
    try:
        glob = eng.simulate(jobs, res, torch.as_tensor(arr), **kw)
    finally:
        dispatch.queue_csr_force_global(False)
    staged = eng.simulate(jobs, res, torch.as_tensor(arr), **kw)
    for a, b in ((glob, staged), (glob, sim)):
        assert torch.equal(a.delay_sum, b.delay_sum)
        assert torch.equal(a.count, b.count)
        assert torch.equal(a.trace, b.trace)
        assert torch.equal(a.sched_slots, b.sched_slots)
    if stats:
        assert torch.equal(glob.stats.nb_sum, staged.stats.nb_sum)
        assert torch.equal(glob.stats.busy_slots, staged.stats.busy_slots)


@needs_gpu
def test_lds_plan_binding():
    """The plans' bytes are the formulas of docs/KERNELS.md."""
    from multihop_offload_amd.ops import dispatch
    eng = run("g1")[2]
    N, E, J = eng.N, eng.E, eng.Jmax
    R = E + N
    W = 6 * R + (R + 31) // 32 + E + 5 * J + 4              # timeslot_sim
    S = W + 3 * R + (W + 3 * R) % 2 + 2 * R + 2 * E         # ..._stats
    M = W + R + 3 * E
    MS = S + 3 * E
    for stats, words in ((False, M + M % 2 + 2 * E),
                         (True, MS + MS % 2 + 2 * E)):
        plan = dispatch.timeslot_mwis_lds_plan(N, E, J, stats)
        assert set(plan) == {"lds_bytes", "large", "threads", "fits"}
        assert plan["lds_bytes"] == 4 * words, (stats, plan)
        assert plan["fits"] and not plan["large"] and plan["threads"] == 256
        assert not dispatch.timeslot_mwis_lds_plan(9000, 20000, 100,
                                                   stats)["fits"]
    assert dispatch.timeslot_lds_plan(N, E, J)["lds_bytes"] == 4 * W
    assert dispatch.timeslot_stats_lds_plan(N, E, J)["lds_bytes"] == 4 * S


@needs_gpu
def test_evaluate_sim_mac_cli_cuda(tmp_path):
    from multihop_offload_amd.harness import evaluate as ev
    out = str(tmp_path / "m.json")
    ev.main(["--training_set", "BAT1000",
             "--model_root", os.path.join(ROOT, "artifacts", "model"),
             "--sizes", "20", "--cases-per-size", "2", "--instances", "1",
             "--workers", "0", "--device", "cuda", "--simulate", "200",
             "--sim-mac", "mwis", "--sim-stats", "--out", out])
    doc = json.load(open(out))
    assert doc["sim_mac"] == "mwis" and doc["config"]["sim_mac"] == "mwis"
    for m in ("baseline", "local", "GNN"):
        for part in (doc["summary"][m], doc["per_size"]["20"][m]):
            assert {"tau", "sim_tau", "sim_backlog_ratio", "sim_tasks",
                    "sim_p99", "sim_sched_share"} <= set(part)
            assert part["sim_tasks"] > 0 and part["sim_tau"] >= 1.0
    # local sends nothing over a link: 0 / 0 busy slots, reported as nan
    assert np.isnan(doc["summary"]["local"]["sim_sched_share"])
    for m in ("baseline", "GNN"):
        assert 0.0 < doc["summary"][m]["sim_sched_share"] <= 1.0
