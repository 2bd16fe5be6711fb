"""CPU tests of the packet simulator's statistics mode: the oracle
(``simulate_routes(stats=True)``), the bin function, ``SimStats``, the
stand-alone host run of the kernel's phases with ``Stats = true``, the CPU
engine and ``harness.evaluate --sim-stats``.

Everything is integers, so every comparison is equality; the one bound is
the histogram percentile's, which its bins make an upper bound that is exact
below 16 slots and at most one bin (12.5 %) over above."""
import functools
import json
import math
import os
import shutil
import subprocess
from collections import deque

import numpy as np
import pytest
import torch

from multihop_offload_amd.sim.timeslot import (STAT_KEYS, delay_bin,
                                               delay_bin_upper, dump_case,
                                               num_delay_bins,
                                               simulate_routes)
from tests import timeslot_cases as tc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LATE = 8            # the default horizon (1000) cannot be exceeded in 400 slots
QS = (0.5, 0.95, 0.99)


def _cpu_engine(cases):
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    model = ChebConvStack(K=2, dtype=torch.float64, seed=3)
    return EpisodeEngine(cases, model, device="cpu", dtype=torch.float64)


@functools.lru_cache(maxsize=None)
def batch(name):
    """A test batch on the fp64 CPU engine's baseline routes: the engine's
    statistics run and the per-case oracle outputs, computed once."""
    cases, jobs_list = tc.g1_batch() if name == "g1" else tc.g2_batch()
    eng = _cpu_engine(cases)
    jobs = eng.pack_jobs(jobs_list)
    res = eng.baseline_episode(jobs)
    arr = tc.batch_arrivals(jobs_list, eng.Jmax)
    per_case = []
    for b, (g, jb) in enumerate(zip(cases, jobs_list)):
        k = jb.num_jobs
        args = (g, jb.ul, jb.dl, res.dst[b, :k].numpy(),
                res.route_links[b, :k].numpy(), res.nhop[b, :k].numpy(),
                arr[b][:, :k])
        per_case.append((args, simulate_routes(
            *args, warmup=tc.WARMUP, trace=True, stats=True,
            late_after=LATE)))
    sim = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                       trace=True, stats=True, late_after=LATE)
    return cases, jobs_list, eng, jobs, res, arr, per_case, sim


def raw_sojourns(g, ul, dl, dst, route_links, nhop, arrivals, warmup):
    """A second, trace-free loop, written independently of the oracle's: one
    deque of [job, t0, stage, remaining] per resource.  Returns the (job,
    sojourn) pairs of the counted tasks, in completion order."""
    T, J = arrivals.shape
    E, N = int(g.num_links), int(g.num_nodes)
    cip, cols = np.asarray(g.conf_indptr), np.asarray(g.conf_indices)
    rate = [float(x) for x in np.asarray(g.link_rates)[:E]] \
        + [float(x) for x in np.asarray(g.proc_bws)[:N]]
    legs = []
    for j in range(J):
        ls = [int(x) for x in route_links[j, :int(nhop[j])]]
        legs.append([(l, float(ul[j])) for l in ls]
                    + [(E + int(dst[j]), float(ul[j]))]
                    + [(l, float(dl[j])) for l in ls[::-1]])
    fifo = [deque() for _ in range(E + N)]
    done = []
    for t in range(T):
        for j in range(J):
            for _ in range(int(arrivals[t, j])):
                fifo[legs[j][0][0]].append([j, t, 0, legs[j][0][1]])
        busy = [1 if fifo[l] else 0 for l in range(E)]
        moved = []
        for r in range(E + N):
            if not fifo[r]:
                continue
            cap = rate[r]
            if r < E:
                cap = cap / (1.0 + sum(busy[o]
                                       for o in cols[cip[r]:cip[r + 1]]))
            while cap > 0 and fifo[r]:
                task = fifo[r][0]
                served = min(cap, task[3])
                task[3] -= served
                cap -= served
                if task[3] > 1e-12:
                    break
                moved.append(fifo[r].popleft())
        for task in moved:
            task[2] += 1
            if task[2] < len(legs[task[0]]):
                r, task[3] = legs[task[0]][task[2]]
                fifo[r].append(task)
            elif task[1] >= warmup:
                done.append((task[0], t + 1 - task[1]))
    return np.array(done, dtype=np.int64).reshape(-1, 2)


def order_statistic(d, q):
    """numpy on the raw sojourns: the smallest value whose cumulative share
    reaches q (the ``inverted_cdf`` quantile)."""
    d = np.sort(np.asarray(d))
    return float(d[max(1, math.ceil(q * len(d))) - 1])


# ---- 1. oracle self-checks --------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_oracle_self_checks(name):
    cases, jobs_list, eng, jobs, res, arr, per_case, sim = batch(name)
    T, W = tc.T_SIM, tc.WARMUP
    for b, (args, out) in enumerate(per_case):
        g, k = cases[b], jobs_list[b].num_jobs
        E, N = g.num_links, g.num_nodes
        ds, ct, tr, st = out
        # stats=False returns what it returns now
        plain = simulate_routes(*args, warmup=W, trace=True)
        assert len(plain) == 3
        assert np.array_equal(plain[0], ds) and np.array_equal(plain[1], ct)
        for key in tr:
            assert np.array_equal(plain[2][key], tr[key]), key
        assert len(simulate_routes(*args, warmup=W)) == 2
        three = simulate_routes(*args, warmup=W, stats=True, late_after=LATE)
        assert len(three) == 3 and set(three[2]) == set(STAT_KEYS)
        for key in STAT_KEYS:
            assert np.array_equal(three[2][key], st[key]), key
        # shapes and dtypes of the contract
        assert st["delay_hist"].shape == (k, num_delay_bins(T))
        assert num_delay_bins(T) == 53
        for key in STAT_KEYS:
            want = np.int64 if key in ("stuck_age", "qlen_sum", "nb_sum") \
                else np.int32
            assert st[key].dtype == want, key
            if key not in ("delay_hist",) and st[key].ndim == 1:
                assert len(st[key]) in (k, E + N)
        # identities
        assert np.array_equal(st["delay_hist"].sum(1), ct)
        arrived = arr[b][W:, :k].sum(0)
        assert np.array_equal(st["stuck"], arrived - ct)
        assert (st["late"] <= ct).all() and (st["late"] >= 0).all()
        assert (st["delay_max"][ct == 0] == 0).all()
        assert (st["stuck_age"] >= st["stuck"]).all()       # T - t0 >= 1
        assert (st["stuck_age"] <= st["stuck"].astype(np.int64)
                * (T - W)).all()
        assert np.array_equal(st["qlen_max"] >= 1, st["busy_slots"] >= 1)
        assert (st["busy_slots"] <= T - W).all()
        assert (st["qlen_sum"] >= st["busy_slots"]).all()
        assert (st["qlen_sum"] <= st["qlen_max"].astype(np.int64)
                * st["busy_slots"]).all()
        assert not st["nb_sum"][E:].any()
        deg = np.diff(np.asarray(g.conf_indptr)[:E + 1])
        assert (st["nb_sum"][:E] <= deg * st["busy_slots"][:E]).all()
        # against the second loop
        raw = raw_sojourns(*args, warmup=W)
        assert len(raw) == ct.sum()
        for j in range(k):
            d = raw[raw[:, 0] == j, 1]
            assert st["delay_max"][j] == (d.max() if len(d) else 0)
            assert st["late"][j] == (d > LATE).sum()
            assert ds[j] == d.sum()
            want = np.bincount([delay_bin(x) for x in d],
                               minlength=num_delay_bins(T))
            assert np.array_equal(st["delay_hist"][j], want)
    if name == "g1":
        # the inputs do exercise the statistics (figures of the issue)
        st0 = per_case[0][1][3]
        assert per_case[0][1][1].sum() == 131 and st0["stuck"].sum() == 3
        assert per_case[1][1][3]["stuck"].sum() == 343
        assert per_case[2][1][3]["stuck"].sum() == 125
        assert max(p[1][3]["delay_max"].max() for p in per_case) > 300
        assert st0["late"].max() > 0
        assert all((p[1][3]["delay_hist"][:, 16:] > 0).sum() > 0
                   for p in per_case[1:])
    else:
        ct0 = per_case[0][1][1]
        assert (ct0 == 0).sum() == 2, "two jobs of G2 graph 0 never complete"
        assert sorted(per_case[0][1][3]["stuck"][ct0 == 0]) == [43, 44]


@pytest.mark.parametrize("name", ["g1", "g2"])
def test_percentile_bounds_on_raw_sojourns(name):
    """SimStats.percentile against numpy on the raw sojourns of the second
    loop: true <= got <= true * 1.125 + 1, per job, per graph and over the
    batch; nan exactly where nothing was counted."""
    cases, jobs_list, eng, jobs, res, arr, per_case, sim = batch(name)
    st = sim.stats
    raws = [raw_sojourns(*args, warmup=tc.WARMUP) for args, _ in per_case]
    checked = 0
    for q in QS:
        per_job = st.percentile(q, per="job").numpy()
        per_graph = st.percentile(q, per="graph").numpy()
        assert per_job.shape == (eng.B, eng.Jmax)
        assert per_graph.shape == (eng.B,)
        for b, raw in enumerate(raws):
            true = order_statistic(raw[:, 1], q)
            print(name, "graph", b, "q", q, "true", true, "got", per_graph[b])
            assert true <= per_graph[b] <= true * 1.125 + 1
            for j in range(eng.Jmax):
                d = raw[raw[:, 0] == j, 1]
                if len(d) == 0:
                    assert np.isnan(per_job[b, j])
                    continue
                true = order_statistic(d, q)
                assert true <= per_job[b, j] <= true * 1.125 + 1, (b, j, q)
                if true < 16:
                    assert per_job[b, j] == true
                checked += 1
        true = order_statistic(np.concatenate([r[:, 1] for r in raws]), q)
        got = float(st.percentile(q, per="all"))
        assert true <= got <= true * 1.125 + 1
    assert checked > 30
    if name == "g2":
        assert np.isnan(st.percentile(0.5, per="job").numpy()).sum() >= 2
    with pytest.raises(ValueError):
        st.percentile(0.5, per="slot")


# ---- 2. the bin function ----------------------------------------------------
def test_bin_function():
    bins = [delay_bin(d) for d in range(5001)]
    assert bins[:17] == list(range(17))
    assert all(b1 - b0 in (0, 1) for b0, b1 in zip(bins, bins[1:]))
    for d, k in enumerate(bins):
        assert delay_bin_upper(k) >= d
        lo = delay_bin_upper(k - 1) + 1 if k else 0
        assert lo <= d
        if k >= 16:                       # at most 12.5 % wide
            assert (delay_bin_upper(k) + 1 - lo) * 8 <= lo
    for k in range(bins[-1] + 1):
        assert delay_bin(delay_bin_upper(k)) == k
    assert delay_bin(400) == 52 and num_delay_bins(400) == 53


# ---- 3. the kernel's phases with Stats = true, as a host program -----------
@pytest.fixture(scope="module")
def stats_host_prog(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++")
                if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    out = str(tmp_path_factory.mktemp("tsstats") / "timeslot_stats_host")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I",
            os.path.join(ROOT, "multihop_offload_amd", "ops", "hip"),
            os.path.join(ROOT, "tests", "host", "timeslot_stats_host.cpp"),
            "-o", out]
    san = subprocess.run(base + ["-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=all"],
                         capture_output=True, text=True)
    if san.returncode == 0:
        return out, "address,undefined"
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    return out, "none"


@pytest.mark.parametrize("b", [0, 1, 2])
@pytest.mark.parametrize("nt,pad", [(7, 3), (64, 0)])
def test_host_program_statistics_match_oracle(tmp_path, stats_host_prog, b,
                                              nt, pad):
    """The phases with Stats = true, run thread by thread on the host (under
    ASan/UBSan where they link), give every statistic of the oracle on the
    G1 dumps; with pad > 0 the node columns start past the graph's own link
    count, as in a ragged batch, and the columns between stay zero."""
    prog, san = stats_host_prog
    print(f"host program built with sanitizers: {san}")
    cases, jobs_list, eng, jobs, res, arr, per_case, sim = batch("g1")
    g, jb = cases[b], jobs_list[b]
    k, E, N = jb.num_jobs, g.num_links, g.num_nodes
    path = str(tmp_path / "case.bin")
    dump_case(path, g, jb.ul, jb.dl, res.dst[b, :k].numpy(),
              res.route_links[b, :k].numpy(), res.nhop[b, :k].numpy(),
              arr[b][:, :k], warmup=tc.WARMUP)
    # the dump rounds the rates through fp32; so does this oracle run
    ds, ct, st = simulate_routes(
        tc.rounded(g), tc.f32(jb.ul), tc.f32(jb.dl), *per_case[b][0][3:],
        warmup=tc.WARMUP, stats=True, late_after=LATE)
    run = subprocess.run([prog, path, str(nt), str(LATE), str(pad)],
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-400:] + run.stderr[-2000:]
    lines = run.stdout.split("\n")
    assert lines[0] == "error 0"
    assert lines[1] == f"nbins {num_delay_bins(tc.T_SIM)}"
    rows = lambda tag: np.array(                            # noqa: E731
        [[int(x) for x in ln.split()[1:]] for ln in lines
         if ln.startswith(tag + " ")], dtype=np.int64)
    job, hist, rs = rows("job"), rows("hist"), rows("res")
    assert np.array_equal(job[:, 0], np.arange(k))
    for col, want in enumerate((ds, ct, st["delay_max"], st["late"],
                                st["stuck"], st["stuck_age"]), start=1):
        assert np.array_equal(job[:, col], want), col
    assert np.array_equal(hist[:, 1:], st["delay_hist"])
    assert np.array_equal(rs[:, 0], np.arange(E + pad + N))
    for col, key in enumerate(("qlen_sum", "qlen_max", "busy_slots",
                               "nb_sum"), start=1):
        assert np.array_equal(rs[:E, col], st[key][:E]), key
        assert not rs[E:E + pad, col].any(), key
        assert np.array_equal(rs[E + pad:, col], st[key][E:]), key
    assert ct.sum() > 100 and st["qlen_max"].max() > 1


# ---- 4. the CPU engine -------------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_cpu_engine_statistics_match_per_case_oracle(name):
    cases, jobs_list, eng, jobs, res, arr, per_case, sim = batch(name)
    st = sim.stats
    assert st is not None and st.T_sim == tc.T_SIM and st.warmup == tc.WARMUP
    assert st.late_after.tolist() == [LATE] * eng.B
    E, N, NB = eng.E, eng.N, num_delay_bins(tc.T_SIM)
    for key in STAT_KEYS:
        t = getattr(st, key)
        want = torch.int64 if key in ("stuck_age", "qlen_sum", "nb_sum") \
            else torch.int32
        assert t.dtype == want, key
        shape = (eng.B, eng.Jmax, NB) if key == "delay_hist" else \
            (eng.B, eng.Jmax) if key in STAT_KEYS[:5] else (eng.B, E + N)
        assert tuple(t.shape) == shape, key
    for b, (args, out) in enumerate(per_case):
        g, k = cases[b], jobs_list[b].num_jobs
        Eb, n = g.num_links, g.num_nodes
        one = out[3]
        for key in STAT_KEYS[:5]:
            got = getattr(st, key)[b].numpy()
            assert np.array_equal(got[:k], one[key]), key
            assert not got[k:].any(), key                   # masked slots
        for key in STAT_KEYS[5:]:
            got = getattr(st, key)[b].numpy()
            assert np.array_equal(got[:Eb], one[key][:Eb]), key
            assert not got[Eb:E].any(), key                 # padded links
            assert np.array_equal(got[E:E + n], one[key][Eb:]), key
            assert not got[E + n:].any(), key
    # stuck == backlog is an identity
    assert torch.equal(st.stuck.to(torch.int64), sim.backlog)
    # stats=False: no statistics, the other fields as before
    plain = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                         trace=True)
    assert plain.stats is None
    assert torch.equal(plain.delay_sum, sim.delay_sum)
    assert torch.equal(plain.count, sim.count)
    assert torch.equal(plain.backlog, sim.backlog)
    assert torch.equal(plain.trace, sim.trace)
    assert torch.equal(plain.mean_delay.isnan(), sim.mean_delay.isnan())
    assert torch.equal(plain.mean_delay.nan_to_num(), sim.mean_delay.nan_to_num())
    # the default horizon is floor(T) of each graph: nothing is late here
    dflt = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                        stats=True)
    assert dflt.stats.late_after.tolist() == [int(c.T) for c in cases]
    assert not dflt.stats.late.any()
    assert torch.equal(dflt.stats.delay_hist, st.delay_hist)


def test_simstats_helpers():
    """The derived figures, from their definitions."""
    cases, jobs_list, eng, jobs, res, arr, per_case, sim = batch("g2")
    st = sim.stats
    S = tc.T_SIM - tc.WARMUP
    assert torch.equal(st.utilization(), st.busy_slots.double() / S)
    assert torch.equal(st.mean_qlen(), st.qlen_sum.double() / S)
    assert float(st.utilization().max()) <= 1.0
    mc = st.mean_contention()
    assert tuple(mc.shape) == (eng.B, eng.E)
    bs = st.busy_slots[:, :eng.E]
    assert torch.equal(mc.isnan(), bs == 0)
    assert torch.equal(mc[bs > 0],
                       st.nb_sum[:, :eng.E][bs > 0].double() / bs[bs > 0])
    ct, lt = sim.count.to(torch.int64), st.late.to(torch.int64)
    lr = st.late_ratio(per="job")
    assert torch.equal(lr.isnan(), ct == 0)
    assert torch.equal(lr[ct > 0], lt[ct > 0].double() / ct[ct > 0])
    assert torch.equal(st.late_ratio(), lt.sum(1).double() / ct.sum(1))
    assert float(st.late_ratio(per="all")) == int(lt.sum()) / int(ct.sum())
    cm = st.censored_mean_delay(per="job")
    den = ct + st.stuck
    assert torch.equal(cm.isnan(), den == 0)
    assert torch.equal(cm[den > 0], (sim.delay_sum + st.stuck_age)[den > 0]
                       .double() / den[den > 0])
    # jobs that never complete have no mean delay but a censored one
    dead = (ct == 0) & (st.stuck > 0)
    assert int(dead.sum()) >= 2
    assert sim.mean_delay[dead].isnan().all() and cm[dead].isfinite().all()
    whole = float(st.censored_mean_delay(per="all"))
    assert whole == int((sim.delay_sum + st.stuck_age).sum()) / int(den.sum())


def test_dispatch_cpu_branch_fills_the_same_dict():
    """ops.dispatch.timeslot_sim on CPU tensors: a 3-tuple by default, with
    stats=True a 4-tuple whose dict equals the engine's statistics."""
    from multihop_offload_amd.ops import dispatch
    cases, jobs_list, eng, jobs, res, arr, per_case, sim = batch("g2")
    args = (torch.as_tensor(arr), res.route_links, res.nhop, res.dst,
            jobs.mask, jobs.ul, jobs.dl, eng.link_rates, eng.proc_bws,
            eng.k_conf_indptr, eng.k_conf_base, eng.k_conf_cols,
            eng.k_E_arr, eng.k_N_arr)
    out3 = dispatch.timeslot_sim(*args, warmup=tc.WARMUP)
    assert len(out3) == 3 and out3[2] is None
    out4 = dispatch.timeslot_sim(*args, warmup=tc.WARMUP, stats=True,
                                 late_after=LATE)
    assert len(out4) == 4 and set(out4[3]) == set(STAT_KEYS)
    assert torch.equal(out4[0], out3[0]) and torch.equal(out4[1], out3[1])
    assert torch.equal(out4[0], sim.delay_sum)
    for key in STAT_KEYS:
        assert torch.equal(out4[3][key], getattr(sim.stats, key)), key


# ---- 5. the evaluator CLI ----------------------------------------------------
def test_evaluate_sim_stats_cli_cpu(tmp_path):
    """--sim-stats adds exactly seven keys on top of --simulate's three, and
    leaves the analytic fields alone; it needs --simulate."""
    from multihop_offload_amd.harness import evaluate as ev
    common = ["--training_set", "BAT1000",
              "--model_root", os.path.join(ROOT, "artifacts", "model"),
              "--sizes", "20", "--cases-per-size", "2", "--instances", "1",
              "--workers", "0", "--device", "cpu"]
    out0, out1 = str(tmp_path / "a.json"), str(tmp_path / "b.json")
    ev.main(common + ["--out", out0])
    ev.main(common + ["--simulate", "200", "--sim-stats", "--out", out1])
    a, b = json.load(open(out0)), json.load(open(out1))
    new = {"sim_p50", "sim_p95", "sim_p99", "sim_late_ratio",
           "sim_tau_censored", "sim_link_util_max", "sim_node_util_max"}
    for m in ("baseline", "local", "GNN"):
        for part_a, part_b in ((a["summary"][m], b["summary"][m]),
                               (a["per_size"]["20"][m],
                                b["per_size"]["20"][m])):
            for k, v in part_a.items():
                assert part_b[k] == v, (m, k)
            assert set(part_b) - set(part_a) == new | {
                "sim_tau", "sim_backlog_ratio", "sim_tasks"}
            assert 1.0 <= part_b["sim_p50"] <= part_b["sim_p95"] \
                <= part_b["sim_p99"] <= 200
            assert math.isfinite(part_b["sim_tau_censored"])
            assert part_b["sim_tau_censored"] >= 1.0
            assert part_b["sim_late_ratio"] == 0.0      # horizon 1000 > 200
            assert 0.0 < part_b["sim_node_util_max"] <= 1.0
            assert 0.0 <= part_b["sim_link_util_max"] <= 1.0
    assert b["summary"]["baseline"]["sim_link_util_max"] > 0.0
    with pytest.raises(SystemExit):
        ev.main(common + ["--sim-stats", "--out", out1])
