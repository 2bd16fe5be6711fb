"""GPU (MI355X) tests of the packet simulator's statistics mode
(``timeslot_sim_stats`` in ops/hip/timeslot.hip,
``EpisodeEngine.simulate(stats=True)``).

As in test_gpu_timeslot.py the oracle is ``simulate_routes`` on fp64 copies
of the arrays after rounding through ``np.float32``, on the routes the GPU
episode produced, and every comparison is integer equality: the statistics
are counts, sums and maxima of integers the two sides already agree on."""
import functools

import numpy as np
import pytest
import torch

from multihop_offload_amd.sim.timeslot import (STAT_KEYS, num_delay_bins,
                                               simulate_routes)
from tests import timeslot_cases as tc

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")
LATE = 8            # the default horizon (1000) cannot be exceeded in 400 slots
PER_JOB, PER_RES = STAT_KEYS[:5], STAT_KEYS[5:]
I64 = ("stuck_age", "qlen_sum", "nb_sum")


def _engine(cases):
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
    eng = EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)
    assert eng.use_hip
    return eng


def _np(x):
    return x.detach().cpu().numpy()


def _oracle(cases, jobs_list, res, arr, warmup):
    """Per-case statistics of the oracle on the fp32-rounded arrays."""
    out = []
    dst, rl, nhop = _np(res.dst), _np(res.route_links), _np(res.nhop)
    for b, (g, jb) in enumerate(zip(cases, jobs_list)):
        k = jb.num_jobs
        out.append(simulate_routes(
            tc.rounded(g), tc.f32(jb.ul), tc.f32(jb.dl), dst[b][:k],
            rl[b][:k], nhop[b][:k], arr[b][:, :k], warmup=warmup, trace=True,
            stats=True, late_after=LATE))
    return out


@functools.lru_cache(maxsize=None)
def run(name):
    cases, jobs_list = tc.g2_batch() if name == "g2" else tc.g1_batch()
    eng = _engine(cases)
    jobs = eng.pack_jobs(jobs_list)
    res = (eng.local_episode(jobs) if name == "g1_local"
           else eng.baseline_episode(jobs))
    arr = tc.batch_arrivals(jobs_list, eng.Jmax)
    a = torch.as_tensor(arr)
    sim = eng.simulate(jobs, res, a, warmup=tc.WARMUP, trace=True,
                       stats=True, late_after=LATE)
    plain = eng.simulate(jobs, res, a, warmup=tc.WARMUP, trace=True)
    ref = _oracle(cases, jobs_list, res, arr, tc.WARMUP)
    return cases, jobs_list, eng, jobs, res, arr, sim, plain, ref


def _check_equal(name):
    cases, jobs_list, eng, jobs, res, arr, sim, plain, ref = run(name)
    st = sim.stats
    E, N, NB = eng.E, eng.N, num_delay_bins(tc.T_SIM)
    assert NB == 53
    for key in STAT_KEYS:
        t = getattr(st, key)
        assert t.is_cuda
        assert t.dtype == (torch.int64 if key in I64 else torch.int32), key
        shape = (eng.B, eng.Jmax, NB) if key == "delay_hist" else \
            (eng.B, eng.Jmax) if key in PER_JOB else (eng.B, E + N)
        assert tuple(t.shape) == shape, key
    for b, (g, jb) in enumerate(zip(cases, jobs_list)):
        k, Eb = jb.num_jobs, g.num_links
        n = int(_np(eng.k_N_arr)[b])
        ds, ct, tr, one = ref[b]
        assert np.array_equal(_np(sim.delay_sum)[b, :k], ds)
        assert np.array_equal(_np(sim.count)[b, :k], ct)
        assert np.array_equal(_np(sim.trace)[b, :, 2], tr["pkts_in_network"])
        for key in PER_JOB:
            got = _np(getattr(st, key))[b]
            assert np.array_equal(got[:k], one[key]), (key, b)
            assert not got[k:].any(), (key, b)              # masked slots
        for key in PER_RES:
            got = _np(getattr(st, key))[b]
            assert np.array_equal(got[:Eb], one[key][:Eb]), (key, b)
            assert not got[Eb:E].any(), (key, b)            # padded links
            assert np.array_equal(got[E:E + g.num_nodes], one[key][Eb:]), \
                (key, b)
            assert not got[E + n:].any(), (key, b)          # padded nodes
        print(name, "graph", b, "counted", int(ct.sum()), "stuck",
              int(one["stuck"].sum()), "delay_max", int(one["delay_max"].max()),
              "qlen_max", int(one["qlen_max"].max()))
    assert torch.equal(st.stuck.to(torch.int64), sim.backlog)
    # the statistics launch computes what the plain launch computes
    assert plain.stats is None
    assert torch.equal(plain.delay_sum, sim.delay_sum)
    assert torch.equal(plain.count, sim.count)
    assert torch.equal(plain.trace, sim.trace)
    return cases, jobs_list, eng, sim, ref


@needs_gpu
def test_g1_statistics_equal_oracle():
    """G1: three 20-node cases at loads 0.15/0.6/0.3 — light queues next to
    deep ones (hundreds of stuck tasks, sojourns past 300 slots, dozens of
    histogram bins above 16), masked job slots."""
    cases, jobs_list, eng, sim, ref = _check_equal("g1")
    assert max(int(r[3]["delay_max"].max()) for r in ref) > 100
    assert max(int(r[3]["qlen_max"].max()) for r in ref) > 20
    assert all(int(r[3]["stuck"].sum()) > 0 for r in ref)
    assert sum(int((r[3]["delay_hist"][:, 16:] > 0).sum()) for r in ref) > 50
    assert any(int(r[3]["late"].max()) > 0 for r in ref)
    assert any(int(r[3]["nb_sum"].max()) > 0 for r in ref)


@needs_gpu
def test_g2_statistics_ragged_and_padded():
    """G2: a 40-node case and a 20-node case padded to 40 — ragged E and J,
    so the node columns start past the small graph's own link count, and
    padded links and nodes must read zero; graph 0 has jobs that never
    complete (count 0, stuck > 0)."""
    cases, jobs_list, eng, sim, ref = _check_equal("g2")
    assert len(set(eng.E_list)) > 1 and _np(eng.k_N_arr).tolist() == [40, 20]
    ct0, st0 = ref[0][1], ref[0][3]
    assert ((ct0 == 0) & (st0["stuck"] > 0)).sum() >= 1
    pj = sim.stats.percentile(0.99, per="job")
    assert torch.equal(pj.isnan(), sim.count == 0)
    cm = sim.stats.censored_mean_delay(per="job")
    dead = (sim.count == 0) & (sim.stats.stuck > 0)
    assert cm[dead].isfinite().all()
    assert float(sim.stats.utilization().max()) <= 1.0


@needs_gpu
def test_g3_statistics_hand_over_order():
    """G3: the star whose two jobs reach the one-task-per-slot server in the
    same slots: the per-job delay_max follows the hand-over order, and the
    server node's qlen_max / busy_slots follow its queue exactly."""
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
                       stats=True, late_after=LATE)
    ds, ct, one = simulate_routes(tc.rounded(g), tc.f32(jobs.ul),
                                  tc.f32(jobs.dl), dst, rl, nhop, arr,
                                  stats=True, late_after=LATE)
    E = g.num_links
    assert one["delay_max"][0] != one["delay_max"][1]
    assert one["qlen_max"][E + 0] >= 2 and one["busy_slots"][E + 0] >= 6
    print("oracle delay_max", one["delay_max"].tolist(), "server qlen_max",
          int(one["qlen_max"][E]), "busy_slots", int(one["busy_slots"][E]))
    assert _np(sim.delay_sum)[0].tolist() == ds.tolist()
    for key in STAT_KEYS:
        got = _np(getattr(sim.stats, key))[0]
        assert np.array_equal(got, one[key]), key
    assert _np(sim.stats.delay_max)[0].tolist() \
        != one["delay_max"][::-1].tolist()


@needs_gpu
def test_local_episode_only_nodes_are_busy():
    """A local episode has zero-hop routes: no link ever holds a task, so
    every link column and all of nb_sum is zero, and the node columns equal
    the oracle."""
    cases, jobs_list, eng, sim, ref = _check_equal("g1_local")
    st = sim.stats
    assert not _np(run("g1_local")[4].nhop).any()
    E = eng.E
    assert not st.nb_sum.any()
    for key in PER_RES:
        assert not getattr(st, key)[:, :E].any(), key
    assert int(st.busy_slots[:, E:].sum()) > 100
    assert st.mean_contention().isnan().all()


@needs_gpu
def test_stats_lds_plan_and_oversized_shape():
    """The base plan's binding still gives the base formula; the statistics
    plan is the documented one, at least as large; a shape whose base plan
    fits and whose statistics plan does not is refused by the statistics
    entry point alone."""
    from multihop_offload_amd.ops import dispatch
    eng = run("g1")[2]

    def words(N, E, J):
        R = E + N
        return 6 * R + (R + 31) // 32 + E + 5 * J + 4

    def stats_bytes(N, E, J):
        R, w = E + N, words(N, E, J) + 3 * (E + N)
        return 4 * (w + w % 2 + 2 * R + 2 * E)

    for N, E, J in ((eng.N, eng.E, eng.Jmax), (40, 76, 13), (21, 36, 8),
                    (4, 3, 2)):
        base = dispatch.timeslot_lds_plan(N, E, J)
        plan = dispatch.timeslot_stats_lds_plan(N, E, J)
        assert set(plan) == {"lds_bytes", "large", "threads", "fits"}
        assert base["lds_bytes"] == 4 * words(N, E, J)
        assert plan["lds_bytes"] == stats_bytes(N, E, J)
        assert plan["lds_bytes"] >= base["lds_bytes"]
        assert plan["fits"] and not plan["large"]
        assert plan["threads"] == base["threads"] == 256
    assert not dispatch.timeslot_stats_lds_plan(9000, 20000, 100)["fits"]

    N, E, J, T = 1000, 3000, 1, 2
    assert dispatch.timeslot_lds_plan(N, E, J)["fits"]
    assert not dispatch.timeslot_stats_lds_plan(N, E, J)["fits"]
    dev = "cuda"
    i32 = dict(dtype=torch.int32, device=dev)
    args = (torch.zeros(1, T, J, dtype=torch.uint8, device=dev),
            torch.full((1, J, 1), -1, **i32), torch.zeros(1, J, **i32),
            torch.zeros(1, J, dtype=torch.int64, device=dev),
            torch.zeros(1, J, dtype=torch.bool, device=dev),
            torch.ones(1, J, device=dev), torch.ones(1, J, device=dev),
            torch.ones(1, E, device=dev), torch.ones(1, N, device=dev),
            torch.zeros(1, E + 1, **i32),
            torch.zeros(1, dtype=torch.int64, device=dev),
            torch.zeros(1, **i32), torch.zeros(1, **i32),       # no links
            torch.ones(1, **i32))                               # one node
    ds, ct, _ = dispatch.timeslot_sim(*args)
    assert not ds.any() and not ct.any()
    with pytest.raises(RuntimeError, match="too large"):
        dispatch.timeslot_sim(*args, stats=True, late_after=LATE)
    torch.cuda.synchronize()


@needs_gpu
def test_evaluate_sim_stats_cli_cuda(tmp_path):
    """harness.evaluate --simulate --sim-stats on the GPU: the seven
    statistics fields next to the three of --simulate, per method, in the
    summary and per size."""
    import json
    import os

    from multihop_offload_amd.harness import evaluate as ev
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    out = str(tmp_path / "b.json")
    ev.main(["--training_set", "BAT1000",
             "--model_root", os.path.join(root, "artifacts", "model"),
             "--sizes", "20", "--cases-per-size", "2", "--instances", "1",
             "--workers", "0", "--device", "cuda", "--simulate", "200",
             "--sim-stats", "--out", out])
    b = json.load(open(out))
    for m in ("baseline", "local", "GNN"):
        for part in (b["summary"][m], b["per_size"]["20"][m]):
            assert {"sim_tau", "sim_backlog_ratio", "sim_tasks"} <= set(part)
            assert 1.0 <= part["sim_p50"] <= part["sim_p95"] \
                <= part["sim_p99"] <= 200
            assert part["sim_tau_censored"] >= 1.0
            assert part["sim_late_ratio"] == 0.0        # horizon 1000 > 200
            assert 0.0 < part["sim_node_util_max"] <= 1.0
            assert 0.0 <= part["sim_link_util_max"] <= 1.0
