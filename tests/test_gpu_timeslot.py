"""GPU (MI355X) tests of the batched per-timeslot packet simulator
(ops/hip/timeslot.hip, EpisodeEngine.simulate).

The oracle is ``sim.timeslot.simulate_routes`` on fp64 copies of the arrays
after rounding through ``np.float32`` — exactly what the kernel widens — on
the routes the GPU episode produced.  Every comparison is integer equality
on delay_sum, count and trace: the fp64 operation sequences are identical,
so there is no tolerance.  ``ops.timeslot_sim`` raises when a graph's error
word is set, so every test here also checks that none is."""
import dataclasses
import functools
import json
import os

import numpy as np
import pytest
import torch

from tests import timeslot_cases as tc

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _engine(cases):
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.01)
        model.layers[-1].bias.fill_(0.5)
    eng = EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)
    assert eng.use_hip
    return eng


def _np(x):
    return x.detach().cpu().numpy()


@dataclasses.dataclass
class Batch:
    cases: list
    jobs_list: list
    eng: object
    jobs: object
    res: object
    arr: np.ndarray
    sim: object
    ds: np.ndarray
    ct: np.ndarray
    tr: np.ndarray


def _run(cases, jobs_list, episode="baseline"):
    eng = _engine(cases)
    jobs = eng.pack_jobs(jobs_list)
    res = (eng.baseline_episode(jobs) if episode == "baseline"
           else eng.local_episode(jobs))
    arr = tc.batch_arrivals(jobs_list, eng.Jmax)
    sim = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                       trace=True)
    ds, ct, tr = tc.oracle_batch(cases, jobs_list, _np(res.dst),
                                 _np(res.route_links), _np(res.nhop), arr)
    return Batch(cases, jobs_list, eng, jobs, res, arr, sim, ds, ct, tr)


@functools.lru_cache(maxsize=None)
def g1():
    return _run(*tc.g1_batch())


@functools.lru_cache(maxsize=None)
def g2():
    return _run(*tc.g2_batch())


def _check_equal(bt):
    sim = bt.sim
    assert sim.delay_sum.dtype == torch.int64
    assert sim.count.dtype == torch.int32 and sim.trace.dtype == torch.int32
    print("tasks completed per case:", bt.ct.sum(1).tolist(),
          "delay sums:", bt.ds.sum(1).tolist())
    assert np.array_equal(_np(sim.delay_sum), bt.ds)
    assert np.array_equal(_np(sim.count), bt.ct)
    assert np.array_equal(_np(sim.trace), bt.tr)
    mask = _np(bt.jobs.mask)
    assert not _np(sim.delay_sum)[~mask].any()
    assert not _np(sim.count)[~mask].any()
    back = np.where(mask[:, None, :], bt.arr, 0)[:, tc.WARMUP:].sum(1) - bt.ct
    assert np.array_equal(_np(sim.backlog), back) and (back >= 0).all()
    mean = _np(sim.mean_delay)
    assert np.isnan(mean[bt.ct == 0]).all()
    assert np.array_equal(mean[bt.ct > 0],
                          (bt.ds / np.maximum(bt.ct, 1))[bt.ct > 0])


@needs_gpu
def test_g1_three_ragged_cases_with_trace():
    """G1: three 20-node cases (seeds 7/8/9, loads 0.15/0.6/0.3): masked
    job slots, multi-pop slots, same-target hand-overs and deep queues;
    delay_sum, count and trace equal the oracle exactly.  (Two-link
    attachment gives every 20-node case 36 links and the job recipe gives
    each 8 jobs, so the ragged E and J are G2's.)"""
    bt = g1()
    assert not bool(bt.jobs.mask.all()), "masked slots present"
    assert int(_np(bt.res.nhop).max()) >= 2
    assert bt.ct.sum(1).min() > 100
    _check_equal(bt)


@needs_gpu
def test_g2_forty_nodes_and_padded_case():
    """G2: a 40-node case at load 0.3 and a 20-node case padded to 40 —
    ragged E (76 and 36 links) and ragged J."""
    bt = g2()
    assert len(set(bt.eng.E_list)) > 1, "E is ragged"
    assert len({j.num_jobs for j in bt.jobs_list}) > 1, "J is ragged"
    assert bt.eng.N == 40 and _np(bt.eng.k_N_arr).tolist() == [40, 20]
    assert bt.ct.sum(1).min() > 100
    _check_equal(bt)


def _g3_sim():
    from multihop_offload_amd.engine import EpisodeResult
    g, jobs, arr, rl, nhop, dst = tc.g3_case()
    eng = _engine([g])
    assert eng.Jmax == 2
    jb = eng.pack_jobs([jobs])
    z = torch.zeros(1, device="cuda")
    res = EpisodeResult(
        tau=z, congest=z, num_jobs=z, delay_emp=z,
        dst=torch.as_tensor(dst[None], device="cuda"),
        route_links=torch.as_tensor(rl[None].astype(np.int32),
                                    device="cuda"),
        nhop=torch.as_tensor(nhop[None].astype(np.int32), device="cuda"))
    sim = eng.simulate(jb, res, torch.as_tensor(arr[None]), trace=True)
    return g, jobs, arr, rl, nhop, dst, sim


@needs_gpu
def test_g3_hand_over_order():
    """G3: two jobs whose tasks reach the one-task-per-slot server in the
    same slots.  The oracle hands over in link order, which gives the two
    jobs different delay sums; the kernel must give the same pair, not the
    swapped one.  (Checked once by hand: with the oracle's ``finished`` list
    reversed before the hand-over, this case yields the swapped pair.)"""
    g, jobs, arr, rl, nhop, dst, sim = _g3_sim()
    from multihop_offload_amd.sim.timeslot import simulate_routes
    ds, ct, tr = simulate_routes(tc.rounded(g), tc.f32(jobs.ul),
                                 tc.f32(jobs.dl), dst, rl, nhop, arr,
                                 trace=True)
    assert ds[0] != ds[1]
    got = _np(sim.delay_sum)[0]
    print("oracle delay sums", ds.tolist(), "kernel", got.tolist())
    assert got.tolist() == ds.tolist()
    assert got.tolist() != ds[::-1].tolist()
    assert _np(sim.count)[0].tolist() == ct.tolist()
    assert np.array_equal(_np(sim.trace)[0, :, 2], tr["pkts_in_network"])


@needs_gpu
def test_g4_local_episode_node_leg_only():
    """G4: a local_episode result has nhop = 0 everywhere — the node leg
    alone."""
    cases, jobs_list = tc.g1_batch()
    bt = _run(cases, jobs_list, episode="local")
    assert not _np(bt.res.nhop).any()
    assert bt.ct.sum() > 100
    _check_equal(bt)


@needs_gpu
def test_g4_idle_job_warmup_and_trace_flag():
    """G4: a job whose arrivals are all zero reads sum 0, count 0, mean nan;
    warmup >= T gives all zeros; trace=False returns the sums of
    trace=True."""
    bt = g1()
    arr = bt.arr.copy()
    arr[:, :, 1] = 0
    a = torch.as_tensor(arr)
    s1 = bt.eng.simulate(bt.jobs, bt.res, a, warmup=tc.WARMUP, trace=True)
    assert not _np(s1.delay_sum)[:, 1].any() and not _np(s1.count)[:, 1].any()
    assert np.isnan(_np(s1.mean_delay)[:, 1]).all()
    ds, ct, tr = tc.oracle_batch(bt.cases, bt.jobs_list, _np(bt.res.dst),
                                 _np(bt.res.route_links), _np(bt.res.nhop),
                                 arr)
    assert np.array_equal(_np(s1.delay_sum), ds)
    assert np.array_equal(_np(s1.count), ct)
    assert np.array_equal(_np(s1.trace), tr)

    s0 = bt.eng.simulate(bt.jobs, bt.res, a, warmup=tc.WARMUP, trace=False)
    assert s0.trace is None
    assert torch.equal(s0.delay_sum, s1.delay_sum)
    assert torch.equal(s0.count, s1.count)

    for w in (tc.T_SIM, tc.T_SIM + 7):
        sw = bt.eng.simulate(bt.jobs, bt.res, a, warmup=w, trace=True)
        assert not sw.delay_sum.any() and not sw.count.any()
        assert not sw.backlog.any()
        assert torch.equal(sw.trace, s1.trace)     # the trace has no warmup


@needs_gpu
def test_g5_launches_are_repeatable():
    """G5: two launches on the same inputs are bitwise identical."""
    bt = g1()
    a = torch.as_tensor(bt.arr)
    again = bt.eng.simulate(bt.jobs, bt.res, a, warmup=tc.WARMUP, trace=True)
    assert torch.equal(again.delay_sum, bt.sim.delay_sum)
    assert torch.equal(again.count, bt.sim.count)
    assert torch.equal(again.trace, bt.sim.trace)


@needs_gpu
def test_lds_plan_binding_and_arrival_range():
    """The plan is exposed through its own binding, with the formula of
    docs/KERNELS.md; counts above 255 are refused on the host."""
    from multihop_offload_amd.ops import dispatch
    bt = g1()
    eng = bt.eng
    plan = dispatch.timeslot_lds_plan(eng.N, eng.E, eng.Jmax)
    assert set(plan) == {"lds_bytes", "large", "threads", "fits"}
    R = eng.E + eng.N
    assert plan["lds_bytes"] == 4 * (6 * R + (R + 31) // 32 + eng.E
                                     + 5 * eng.Jmax + 4)
    assert plan["fits"] and not plan["large"] and plan["threads"] == 256
    assert not dispatch.timeslot_lds_plan(9000, 20000, 100)["fits"]
    bad = torch.as_tensor(bt.arr).clone()
    bad[0, 0, 0] = 256
    with pytest.raises(ValueError):
        eng.simulate(bt.jobs, bt.res, bad)


@needs_gpu
def test_g6_full_gpu_path():
    """G6: draw_arrivals on the GPU, gnn_episode(train=False), simulate:
    counts never exceed arrivals and the backlog is non-negative."""
    bt = g1()
    eng = bt.eng
    gen = torch.Generator(device="cuda")
    gen.manual_seed(5)
    jobs = eng.sample_jobs(0.3, gen)
    arr = eng.draw_arrivals(jobs, 300, gen)
    assert arr.dtype == torch.uint8 and arr.shape == (3, 300, eng.Jmax)
    assert not arr.permute(0, 2, 1)[~jobs.mask].any()
    assert int(arr.sum()) > 100
    res = eng.gnn_episode(jobs, train=False)
    assert res.route_links is not None and res.nhop is not None
    sim = eng.simulate(jobs, res, arr, warmup=20)
    total = arr.sum(1, dtype=torch.int64)
    assert bool((sim.count.to(torch.int64) <= total).all())
    assert bool((sim.backlog >= 0).all())
    assert int(sim.count.sum()) > 50
    eng.check_overflow()


@needs_gpu
def test_g6_evaluate_simulate_cli_cuda(tmp_path):
    """G6: harness.evaluate --simulate on the GPU reports the sim_* fields
    next to the analytic ones."""
    from multihop_offload_amd.harness import evaluate as ev
    common = ["--training_set", "BAT1000",
              "--model_root", os.path.join(ROOT, "artifacts", "model"),
              "--sizes", "20", "--cases-per-size", "2", "--instances", "1",
              "--workers", "0", "--device", "cuda"]
    out1 = str(tmp_path / "b.json")
    ev.main(common + ["--simulate", "200", "--out", out1])
    b = json.load(open(out1))
    for m in ("baseline", "local", "GNN"):
        for part in (b["summary"][m], b["per_size"]["20"][m]):
            assert {"tau", "congest_ratio", "latency_ratio"} <= set(part)
            assert {"sim_tau", "sim_backlog_ratio", "sim_tasks"} <= set(part)
            assert part["sim_tasks"] > 0 and part["sim_tau"] >= 1.0
