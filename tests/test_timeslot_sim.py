"""CPU tests of the batched timeslot simulator's host side: pre-drawn
arrivals, ``simulate_routes``, the CPU engine path, the stand-alone host run
of the kernel's per-slot phases, and ``harness.evaluate --simulate``."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from multihop_offload_amd import AdhocCloudEnv
from multihop_offload_amd.env import apsp
from multihop_offload_amd.sim.timeslot import (draw_arrivals, dump_case,
                                               simulate, simulate_routes)
from tests import timeslot_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _baseline_flows(g, jobs):
    env = AdhocCloudEnv(g)
    env.set_jobs(jobs)
    _, dlist, dproc = env.dmtx_baseline()
    sp = apsp(g, dlist)
    np.fill_diagonal(sp, np.where(dproc > 0, dproc, g.T))
    env.offloading(sp, g.sp_hop)
    return env


def _routes_of(env, jobs):
    routes = [env.route_links(f) for f in env.flows]
    H = max(1, max(len(r) for r in routes))
    rl = -np.ones((jobs.num_jobs, H), dtype=np.int64)
    for j, r in enumerate(routes):
        rl[j, :len(r)] = r
    nhop = np.array([len(r) for r in routes], dtype=np.int64)
    dst = np.array([f.dst for f in env.flows], dtype=np.int64)
    return rl, nhop, dst


def _same_means(a, b):
    """bitwise, nan-aware"""
    return np.array_equal(np.asarray(a).view(np.int64),
                          np.asarray(b).view(np.int64)) or (
        np.array_equal(np.isnan(a), np.isnan(b))
        and np.array_equal(np.asarray(a)[~np.isnan(a)],
                           np.asarray(b)[~np.isnan(b)]))


@pytest.mark.parametrize("seed,warmup", [(1, 0), (5, 50)])
def test_predrawn_arrivals_match_seeded_run(small_case, jobs_for, seed,
                                            warmup):
    """C1: simulate(arrivals=draw_arrivals(seed)) is simulate(seed)."""
    g, jobs = small_case, jobs_for
    env = _baseline_flows(g, jobs)
    T = tc.T_SIM
    m0, c0, t0 = simulate(g, jobs, env.flows, T=T, seed=seed, warmup=warmup,
                          trace=True)
    arr = draw_arrivals(jobs, T, seed)
    assert arr.shape == (T, jobs.num_jobs)
    m1, c1, t1 = simulate(g, jobs, env.flows, T=T, seed=seed + 100,
                          warmup=warmup, trace=True, arrivals=arr)
    assert _same_means(m0, m1)
    assert np.array_equal(c0, c1)
    for k in ("arrivals", "departures", "pkts_in_network"):
        assert np.array_equal(t0[k], t1[k]), k
    assert np.array_equal(t0["arrivals"], arr.sum(1))
    assert c0.sum() > 50                      # the case is not idle


def test_simulate_routes_matches_simulate(small_case, jobs_for):
    """C2: explicit routes from env.route_links give the same integers."""
    g, jobs = small_case, jobs_for
    env = _baseline_flows(g, jobs)
    rl, nhop, dst = _routes_of(env, jobs)
    assert nhop.max() >= 1
    arr = draw_arrivals(jobs, tc.T_SIM, 3)
    mean, cnt, tr = simulate(g, jobs, env.flows, T=tc.T_SIM, warmup=50,
                             trace=True, arrivals=arr)
    ds, ct, tr2 = simulate_routes(g, jobs.ul, jobs.dl, dst, rl, nhop, arr,
                                  warmup=50, trace=True)
    assert ds.dtype == np.int64 and ct.dtype == np.int64
    assert np.array_equal(ct, cnt)
    with np.errstate(invalid="ignore"):
        assert _same_means(np.where(ct > 0, ds / np.maximum(ct, 1), np.nan),
                           mean)
    for k in tr:
        assert np.array_equal(tr[k], tr2[k]), k
    # without the trace: the same two arrays
    ds3, ct3 = simulate_routes(g, jobs.ul, jobs.dl, dst, rl, nhop, arr,
                               warmup=50)
    assert np.array_equal(ds3, ds) and np.array_equal(ct3, ct)


def _cpu_engine(cases):
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    model = ChebConvStack(K=2, dtype=torch.float64, seed=3)
    return EpisodeEngine(cases, model, device="cpu", dtype=torch.float64)


def test_cpu_engine_simulate_matches_per_case():
    """C2: engine.simulate on a B=3 batch is simulate_routes per case on the
    cases' own fp64 arrays; every episode kind carries its routes."""
    cases, jobs_list = tc.g1_batch()
    eng = _cpu_engine(cases)
    jobs = eng.pack_jobs(jobs_list)
    arr = tc.batch_arrivals(jobs_list, eng.Jmax)
    res = eng.baseline_episode(jobs)
    assert res.dst is not None and res.route_links is not None \
        and res.nhop is not None
    sim = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                       trace=True)
    assert sim.delay_sum.dtype == torch.int64
    for b, (g, jb) in enumerate(zip(cases, jobs_list)):
        k = jb.num_jobs
        ds, ct, tr = simulate_routes(
            g, jb.ul, jb.dl, res.dst[b, :k].numpy(),
            res.route_links[b, :k].numpy(), res.nhop[b, :k].numpy(),
            arr[b][:, :k], warmup=tc.WARMUP, trace=True)
        assert np.array_equal(sim.delay_sum[b, :k].numpy(), ds)
        assert np.array_equal(sim.count[b, :k].numpy(), ct)
        assert not sim.delay_sum[b, k:].any() and not sim.count[b, k:].any()
        assert np.array_equal(sim.trace[b, :, 2].numpy(),
                              tr["pkts_in_network"])
        back = arr[b, tc.WARMUP:, :k].sum(0) - ct
        assert np.array_equal(sim.backlog[b, :k].numpy(), back)
        assert (back >= 0).all()
    assert torch.isnan(sim.mean_delay[sim.count == 0]).all()
    for ep in (eng.local_episode(jobs), eng.gnn_episode(jobs, train=False)):
        assert ep.dst.shape == (3, eng.Jmax) and ep.nhop.shape == ep.dst.shape
        assert ep.route_links.shape[:2] == ep.dst.shape


def test_cpu_engine_b1_equals_simulate(small_case, jobs_for):
    """C2: the B=1 CPU engine equals sim.timeslot.simulate on the flows the
    oracle environment derives for the same baseline decisions."""
    g, jobs = small_case, jobs_for
    env = _baseline_flows(g, jobs)
    arr = draw_arrivals(jobs, tc.T_SIM, 3)
    mean, cnt = simulate(g, jobs, env.flows, T=tc.T_SIM, warmup=50,
                         arrivals=arr)
    eng = _cpu_engine([g])
    jb = eng.pack_jobs([jobs])
    k = jobs.num_jobs
    full = np.zeros((1, tc.T_SIM, eng.Jmax), dtype=np.int64)
    full[0, :, :k] = arr
    res = eng.baseline_episode(jb)
    assert np.array_equal(res.dst[0, :k].numpy(),
                          [f.dst for f in env.flows])
    sim = eng.simulate(jb, res, torch.as_tensor(full), warmup=50)
    assert np.array_equal(sim.count[0, :k].numpy(), cnt)
    assert _same_means(sim.mean_delay[0, :k].numpy(), mean)


def test_order_sensitive_case_oracle():
    """G3's expectation, on the CPU: the two jobs get different delay sums,
    and the pair is the one link-ascending hand-over gives (job 1 rides
    link 0 and is served first)."""
    g, jobs, arr, rl, nhop, dst = tc.g3_case()
    assert rl[1, 0] < rl[0, 0]
    ds, ct = simulate_routes(tc.rounded(g), jobs.ul, jobs.dl, dst, rl, nhop,
                             arr)
    assert ct.tolist() == [6, 6]
    assert ds[1] < ds[0], ds


# ---- C3: the kernel's phases as a stand-alone host program ----------------
def _compile_host(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++")
                if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    out = str(tmp_path_factory.mktemp("tshost") / "timeslot_host")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I",
            os.path.join(ROOT, "multihop_offload_amd", "ops", "hip"),
            os.path.join(ROOT, "tests", "host", "timeslot_host.cpp"),
            "-o", out]
    san = subprocess.run(base + ["-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=all"],
                         capture_output=True, text=True)
    if san.returncode == 0:
        return out, "address,undefined"
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    return out, "none"


@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    return _compile_host(tmp_path_factory)


@pytest.fixture(scope="module")
def g1_cpu():
    """G1's cases with baseline routes from the fp64 CPU engine."""
    cases, jobs_list = tc.g1_batch()
    eng = _cpu_engine(cases)
    res = eng.baseline_episode(eng.pack_jobs(jobs_list))
    arr = tc.batch_arrivals(jobs_list, eng.Jmax)
    ds, ct, tr = tc.oracle_batch(cases, jobs_list, res.dst.numpy(),
                                 res.route_links.numpy(), res.nhop.numpy(),
                                 arr)
    return cases, jobs_list, res, arr, ds, ct, tr


@pytest.mark.parametrize("b", [0, 1, 2])
@pytest.mark.parametrize("nt", [7, 64])
def test_host_program_matches_simulate_routes(tmp_path, host_prog, g1_cpu,
                                              b, nt):
    """C3: the phases, run thread by thread on the host (under ASan/UBSan
    where they link), equal simulate_routes exactly on the G1 dumps —
    delay sums, counts and the trace."""
    prog, san = host_prog
    print(f"host program built with sanitizers: {san}")
    cases, jobs_list, res, arr, ds, ct, tr = g1_cpu
    g, jb = cases[b], jobs_list[b]
    k = jb.num_jobs
    path = str(tmp_path / "case.bin")
    dump_case(path, g, jb.ul, jb.dl, res.dst[b, :k].numpy(),
              res.route_links[b, :k].numpy(), res.nhop[b, :k].numpy(),
              arr[b][:, :k], warmup=tc.WARMUP)
    run = subprocess.run([prog, path, str(nt), "trace"],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-400:] + run.stderr[-2000:]
    lines = run.stdout.split("\n")
    assert lines[0] == "error 0"
    got = np.array([[int(x) for x in ln.split()[1:]]
                    for ln in lines if ln.startswith("job ")])
    assert np.array_equal(got[:, 0], np.arange(k))
    assert np.array_equal(got[:, 1], ds[b, :k])
    assert np.array_equal(got[:, 2], ct[b, :k])
    gtr = np.array([[int(x) for x in ln.split()[2:]]
                    for ln in lines if ln.startswith("trace ")])
    assert np.array_equal(gtr, tr[b])
    assert ct[b].sum() > 100


# ---- C4: the evaluator CLI -------------------------------------------------
def test_evaluate_simulate_cli_cpu(tmp_path):
    """C4: --simulate adds the three sim_* fields per method, in the
    aggregate and per size, and leaves the analytic fields as they are (the
    committed checkpoint, so that both runs evaluate the same model)."""
    from multihop_offload_amd.harness import evaluate as ev
    common = ["--training_set", "BAT1000",
              "--model_root", os.path.join(ROOT, "artifacts", "model"),
              "--sizes", "20", "--cases-per-size", "2", "--instances", "1",
              "--workers", "0", "--device", "cpu"]
    out0, out1 = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    ev.main(common + ["--out", out0])
    ev.main(common + ["--simulate", "200", "--out", out1])
    a, b = json.load(open(out0)), json.load(open(out1))
    for m in ("baseline", "local", "GNN"):
        for part_a, part_b in ((a["summary"][m], b["summary"][m]),
                               (a["per_size"]["20"][m],
                                b["per_size"]["20"][m])):
            assert not any(k.startswith("sim_") for k in part_a)
            for k, v in part_a.items():
                assert part_b[k] == v, (m, k)
            assert set(part_b) - set(part_a) == {
                "sim_tau", "sim_backlog_ratio", "sim_tasks"}
            assert part_b["sim_tasks"] > 0
            assert part_b["sim_tau"] >= 1.0
            assert 0.0 <= part_b["sim_backlog_ratio"] <= 1.0
