#!/usr/bin/env python3
"""Per-stage kernel micro-benchmark (GPU): times each fused kernel of the
episode step in isolation with hip events, at the flagship config
(N=110 BA, B=1024) and the large-graph config (N=1000 ER, B=64).

Run on an MI355X:  python profiles/bench_kernels.py [--config flagship|er1000]
Output: one JSON line per (config, stage) with mean µs over the timed reps.

``--config timeslot`` times the per-timeslot packet simulator instead
(B=256, N=100, load 0.15, T=1000): the bare kernel launch, the whole
``EpisodeEngine.simulate`` call, and the Python ``simulate_routes`` on a few
of the same instances on this host's CPU (whose outputs must equal the
kernel's), with the ratio per batch.  ``--config timeslot_stats`` is the
same configuration through the statistics entry point (``timeslot_sim_stats``,
``simulate(stats=True)``).  ``--config timeslot_mwis`` and
``--config timeslot_mwis_stats`` are the same batch through the scheduled-MAC
entry points (``timeslot_sim_mwis``, ``timeslot_sim_mwis_stats``,
``simulate(mac="mwis")``), with the rounds per slot the oracle's schedules
took on the instances timed in Python.

``--config fixedpoint`` times the three kernels that are little else than
the contention fixed point (actor_head_fwd, actor_head_bwd, critic) on the
benchmark's own batch (BA-100, seed 100, B=256 and B=1024) at fp_iters 1
and 10 — the slope is the cost of one iteration — with the conflict CSR
staged in LDS at each ``--budgets`` value and forced to global memory.  On a
build without the staging switch it times the kernels as they are.

``--config apsp`` times the Floyd–Warshall launch of the step (``eng.apsp``)
on the same batch and on the mixed 20–110 engine, register-resident kernel
against the in-place LDS kernel (``fw_force_inplace``).

``--config cheb`` times the K<=2 ChebConv kernels (cheb_fwd, cheb_bwd) on the
same batch at B=256 and B=1024, on the edge-layer path and forced onto the
full-width path (``cheb_force_full_width``), with the model's 5-layer weight
stack and with a 3-layer one (first, one middle, last layer — the kernels
take L from ``W``): (t5 - t3) / 2 is one middle layer, the rest of t5 the two
edge layers and the launch.  On a build without the switch it times the
kernels as they are.

``--config adam`` times the fused Adam launch alone on the benchmark's model
(one workgroup per tensor against ``adam_force_single_block``), and
``--config walk`` the walk_eval launch and ``eng._episode_eval`` around it,
both at B=256 and B=1024.
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def timeit(fn, reps=50, warmup=10):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(reps):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) * 1000.0 / reps   # µs


def bench_config(name, nodes, batch, gtype, distinct, reps):
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.harness.train_batched import build_training_cases

    cases = build_training_cases(nodes, batch, distinct, 1000, 7,
                                 gtype=gtype, workers=8)
    model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.01)
        model.layers[-1].bias.fill_(0.5)
    eng = EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    jobs = eng.sample_jobs(0.15, gen)

    out = {}
    # full step pieces
    with torch.enable_grad():
        dm, *_ = eng.actor_forward(jobs)
    sp = eng.apsp(dm)
    uds = torch.diagonal(dm.detach(), dim1=1, dim2=2)
    dst, _ = eng.offload_decide(jobs, sp, uds)
    rl, nhop, delay_emp, unit_mtx, written = eng._episode_eval(jobs, dst, sp)

    from multihop_offload_amd.ops.functions import ChebStackFn
    params = []
    for layer in eng.model.layers:
        params += [layer.weight, layer.bias]
    arr = torch.zeros(eng.B, eng.N, dtype=eng.dtype, device=eng.device)
    arr = arr.scatter_add(1, jobs.sources, jobs.rates * jobs.ul)
    f_job = torch.zeros(eng.B, eng.Ee, dtype=eng.dtype, device=eng.device)
    vidx = torch.where(eng.comp_mask, eng.node_vedge,
                       torch.zeros_like(eng.node_vedge))
    f_job = f_job.scatter_add(
        1, vidx, torch.where(eng.comp_mask, arr, torch.zeros_like(arr)))
    x = torch.stack([eng.f_self_loop, eng.f_rate, f_job,
                     eng.f_as_server], dim=-1).contiguous()

    from multihop_offload_amd.ops import dispatch
    ext = dispatch.require_hip()
    from multihop_offload_amd.ops.functions import (cheb_lds_fits,
                                                    pack_cheb_params)
    Wp, bp = pack_cheb_params(params)
    small = cheb_lds_fits(eng.Ee, 2)
    if small:
        out["cheb_fwd"] = timeit(lambda: ext.cheb_fwd(
            x, Wp, bp, eng.k_ext_indptr, eng.k_ext_base, eng.k_ext_cols,
            eng.k_ext_max_nnz), reps)
        lam, acts, t1s = ext.cheb_fwd(x, Wp, bp, eng.k_ext_indptr,
                                      eng.k_ext_base, eng.k_ext_cols,
                                      eng.k_ext_max_nnz)
        dlam = torch.randn_like(lam)
        out["cheb_bwd"] = timeit(lambda: ext.cheb_bwd(
            dlam, acts, t1s, Wp, eng.k_ext_indptr, eng.k_ext_base,
            eng.k_ext_cols, eng.k_ext_max_nnz), reps)
    else:
        out["cheb_large_fwd"] = timeit(lambda: ext.cheb_large_fwd(
            x, Wp, bp, eng.k_ext_indptr, eng.k_ext_base, eng.k_ext_cols),
            reps)
        lam, acts = ext.cheb_large_fwd(x, Wp, bp, eng.k_ext_indptr,
                                       eng.k_ext_base, eng.k_ext_cols)
        dlam = torch.randn_like(lam)
        out["cheb_large_bwd"] = timeit(lambda: ext.cheb_large_bwd(
            dlam, acts, Wp, eng.k_ext_indptr, eng.k_ext_base,
            eng.k_ext_cols), reps)

    lam_ext = lam.detach()
    out["actor_head_fwd"] = timeit(lambda: ext.actor_head_fwd(
        lam_ext, eng.k_conf_indptr, eng.k_conf_base, eng.k_conf_cols,
        eng.link_rates.contiguous(), eng.bw_comp.contiguous(), eng.k_edges,
        eng.node_vedge, eng.T_arr.contiguous(), eng.k_E_arr, eng.N,
        eng.fp_iters, 0.0), reps)
    dmk, mu_hist = ext.actor_head_fwd(
        lam_ext, eng.k_conf_indptr, eng.k_conf_base, eng.k_conf_cols,
        eng.link_rates.contiguous(), eng.bw_comp.contiguous(), eng.k_edges,
        eng.node_vedge, eng.T_arr.contiguous(), eng.k_E_arr, eng.N,
        eng.fp_iters, 0.0)
    gd = torch.randn_like(dmk)
    out["actor_head_bwd"] = timeit(lambda: ext.actor_head_bwd(
        gd, lam_ext, mu_hist, eng.k_conf_indptr, eng.k_conf_base,
        eng.k_conf_cols, eng.link_rates.contiguous(),
        eng.bw_comp.contiguous(), eng.k_edges, eng.node_vedge,
        eng.T_arr.contiguous(), eng.k_E_arr, eng.fp_iters, 0.0), reps)

    out["fw_apsp"] = timeit(lambda: eng.apsp(dm.detach()), reps)
    out["decide"] = timeit(lambda: eng.offload_decide(jobs, sp, uds), reps)
    out["walk_eval"] = timeit(lambda: eng._episode_eval(jobs, dst, sp), reps)
    vedge_dst = eng.node_vedge.gather(1, dst)
    out["critic"] = timeit(lambda: ext.critic(
        rl.contiguous(), nhop.contiguous(), vedge_dst.contiguous(),
        jobs.mask, jobs.rates.contiguous(), jobs.ul.contiguous(),
        jobs.dl.contiguous(), eng.k_conf_indptr, eng.k_conf_base,
        eng.k_conf_cols, eng.link_rates.contiguous(),
        eng.bw_comp.contiguous(), eng.k_E_arr, eng.T_arr.contiguous(),
        eng.Ee, eng.fp_iters, 0.0), reps)

    def full_step():
        jb = eng.sample_jobs(0.15, gen)
        r = eng.gnn_episode(jb, train=True)
        return r

    out["full_train_step"] = timeit(full_step, max(reps // 5, 5))
    for k, v in out.items():
        print(json.dumps({"config": name, "stage": k, "us": round(v, 1),
                          "B": eng.B, "N": eng.N, "E": eng.E,
                          "Ee": eng.Ee}), flush=True)
    return out


def bench_timeslot(nodes=100, batch=256, load=0.15, T_sim=1000, reps=50,
                   py_instances=4, stats=False, mac="share"):
    import time
    from types import SimpleNamespace

    import numpy as np

    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.harness.train_batched import build_training_cases
    from multihop_offload_amd.ops import dispatch
    from multihop_offload_amd.sim import timeslot as ts
    from multihop_offload_amd.sim.timeslot import (num_delay_bins,
                                                   simulate_routes)

    mwis = mac == "mwis"
    cases = build_training_cases(nodes, batch, 16, 1000, 7, gtype="ba",
                                 workers=8)
    model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
    eng = EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    jobs = eng.sample_jobs(load, gen)
    res = eng.baseline_episode(jobs)
    arr = eng.draw_arrivals(jobs, T_sim, gen)
    sim = eng.simulate(jobs, res, arr, stats=stats, mac=mac)
    tasks = int(arr.sum())

    # the bare launch: the wrapper's prefix sums and error read left out
    ext = dispatch.require_hip()
    slot_off = torch.zeros(eng.B, T_sim + 1, dtype=torch.int32,
                           device="cuda")
    slot_off[:, 1:] = arr.sum(2, dtype=torch.int64).cumsum(1)
    pool = int(slot_off[:, -1].max())
    args = (arr, slot_off, res.route_links.contiguous(),
            res.nhop.contiguous(), res.dst.contiguous(), jobs.mask,
            jobs.ul.contiguous(), jobs.dl.contiguous(), eng.k_conf_indptr,
            eng.k_conf_base, eng.k_conf_cols, eng.link_rates.contiguous(),
            eng.proc_bws.contiguous(), eng.T_arr.contiguous(), eng.k_E_arr,
            eng.k_N_arr, 0, pool, False)
    launch = ext.timeslot_sim_mwis if mwis else ext.timeslot_sim
    if stats:
        args += (torch.floor(eng.T_arr).to(torch.int32),
                 num_delay_bins(T_sim))
        launch = ext.timeslot_sim_mwis_stats if mwis \
            else ext.timeslot_sim_stats
    out = launch(*args)
    assert not bool(out[2].any())
    assert torch.equal(out[0], sim.delay_sum)
    if stats:
        assert torch.equal(out[6], sim.stats.delay_hist)
        assert torch.equal(out[9], sim.stats.qlen_sum)
    if mwis:
        assert torch.equal(out[-1], sim.sched_slots)
    kernel_us = timeit(lambda: launch(*args), reps)
    call_us = timeit(lambda: eng.simulate(jobs, res, arr, stats=stats,
                                          mac=mac), reps)
    # every schedule the oracle computes below: rounds per slot
    real_schedule, rounds = ts.mwis_schedule, []

    def counting_schedule(cip, cols, w):
        on, r = real_schedule(cip, cols, w)
        rounds.append(r)
        return on, r
    ts.mwis_schedule = counting_schedule

    # the Python simulator on the first instances, same host, same inputs
    f64 = lambda x: x.cpu().numpy().astype(np.float64)   # noqa: E731
    t_py = 0.0
    for b in range(py_instances):
        g = cases[b]
        k = int(jobs.mask[b].sum())
        view = SimpleNamespace(
            num_links=g.num_links, num_nodes=g.num_nodes,
            conf_indptr=g.conf_indptr, conf_indices=g.conf_indices,
            link_rates=f64(eng.link_rates[b, :g.num_links]),
            proc_bws=f64(eng.proc_bws[b]))
        a = (view, f64(jobs.ul[b, :k]), f64(jobs.dl[b, :k]),
             res.dst[b, :k].cpu().numpy(),
             res.route_links[b, :k].cpu().numpy(),
             res.nhop[b, :k].cpu().numpy(), arr[b][:, :k].cpu().numpy())
        t0 = time.perf_counter()
        ds, ct, *st = simulate_routes(*a, stats=stats,
                                      late_after=int(eng.T_arr[b]), mac=mac)
        t_py += time.perf_counter() - t0
        if mwis:
            sc = st.pop()
            assert np.array_equal(
                sc["sched_slots"],
                sim.sched_slots[b, :g.num_links].cpu().numpy())
            assert sc["rounds_max"] == max(rounds[-T_sim:])
        if stats:
            E = g.num_links
            assert np.array_equal(st[0]["delay_hist"],
                                  sim.stats.delay_hist[b, :k].cpu().numpy())
            assert np.array_equal(st[0]["stuck_age"],
                                  sim.stats.stuck_age[b, :k].cpu().numpy())
            for key in ("qlen_sum", "qlen_max", "busy_slots", "nb_sum"):
                got = getattr(sim.stats, key)[b].cpu().numpy()
                assert np.array_equal(st[0][key][:E], got[:E]), key
                assert np.array_equal(st[0][key][E:], got[eng.E:]), key
        assert np.array_equal(ds, sim.delay_sum[b, :k].cpu().numpy())
        assert np.array_equal(ct, sim.count[b, :k].cpu().numpy())
    ts.mwis_schedule = real_schedule
    py_s = t_py / py_instances
    if mwis:
        plan = dispatch.timeslot_mwis_lds_plan(eng.N, eng.E, eng.Jmax, stats)
        extra = {"rounds_mean_per_slot": round(float(np.mean(rounds)), 3),
                 "rounds_max": int(max(rounds)),
                 "rounds_instances": py_instances}
    else:
        plan = (dispatch.timeslot_stats_lds_plan if stats
                else dispatch.timeslot_lds_plan)(eng.N, eng.E, eng.Jmax)
        extra = {}
    print(json.dumps({
        "config": f"timeslot_b{batch}_n{nodes}",
        "stage": "timeslot_sim" + ("_mwis" if mwis else "")
        + ("_stats" if stats else ""),
        "B": eng.B, "N": eng.N, "E": eng.E, "J": eng.Jmax, "T": T_sim,
        "load": load, "tasks": tasks, "pool": pool,
        "lds_bytes": plan["lds_bytes"], "threads": plan["threads"],
        "kernel_us": round(kernel_us, 1), "simulate_call_us": round(call_us, 1),
        "python_s_per_instance": round(py_s, 4),
        "python_instances_timed": py_instances,
        "python_s_per_batch": round(py_s * eng.B, 2),
        "ratio_python_over_kernel": round(py_s * eng.B / (kernel_us * 1e-6)),
        "ratio_python_over_call": round(py_s * eng.B / (call_us * 1e-6)),
        "outputs_equal_python": True, **extra}), flush=True)


def bench_fixedpoint(batches=(256, 1024), budgets=(-1,), reps=200):
    import numpy as np

    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.harness.train_batched import build_training_cases
    from multihop_offload_amd.ops import dispatch

    ext = dispatch.require_hip()
    has_switch = hasattr(ext, "queue_csr_force_global")
    modes = [("as_built", None)]
    if has_switch:
        modes = [(f"staged_{b}" if b >= 0 else "staged_default", b)
                 for b in budgets] + [("global", None)]
    for batch in batches:
        # bench.py's cases: 100 nodes, 16 distinct BA graphs, T=1000, seed 100
        cases = build_training_cases(100, batch, 16, 1000, 100, gtype="ba",
                                     workers=8)
        nnz = [int(g.conf_indptr[g.num_links]) for g in cases]
        deg = np.concatenate([np.diff(g.conf_indptr[:g.num_links + 1])
                              for g in cases])
        print(json.dumps({
            "config": "fixedpoint", "B": batch, "conf_nnz_min": min(nnz),
            "conf_nnz_max": max(nnz), "E_max": max(g.num_links for g in cases),
            "row_degree_mean": round(float(deg.mean()), 2),
            "row_degree_max": int(deg.max()),
            "stage_bytes_max": (max(ext.queue_csr_bytes(g.num_links, n)
                                    for g, n in zip(cases, nnz))
                                if has_switch else None)}), flush=True)
        for iters in (1, 10):
            model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
            eng = EpisodeEngine(cases, model, device="cuda",
                                dtype=torch.float32, fp_iters=iters)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(0)
            jobs = eng.sample_jobs(0.15, gen)
            with torch.no_grad():
                dm, *_ = eng.actor_forward(jobs)
                sp = eng.apsp(dm)
                uds = torch.diagonal(dm, dim1=1, dim2=2)
                dst, _ = eng.offload_decide(jobs, sp, uds)
                rl, nhop, *_ = eng._episode_eval(jobs, dst, sp)
            tables = (eng.k_conf_indptr, eng.k_conf_base, eng.k_conf_cols,
                      eng.link_rates.contiguous(), eng.bw_comp.contiguous(),
                      eng.k_edges, eng.node_vedge, eng.T_arr.contiguous(),
                      eng.k_E_arr)
            lam = (torch.rand(eng.B, eng.Ee, device="cuda", generator=gen)
                   * 5.0).contiguous()
            vedge_dst = eng.node_vedge.gather(1, dst).contiguous()
            fwd = lambda: ext.actor_head_fwd(     # noqa: E731
                lam, *tables, eng.N, iters, 0.0)
            dmk, hist = fwd()
            gd = torch.randn_like(dmk)
            bwd = lambda: ext.actor_head_bwd(     # noqa: E731
                gd, lam, hist, *tables, iters, 0.0)
            crit = lambda: ext.critic(            # noqa: E731
                rl.contiguous(), nhop.contiguous(), vedge_dst, jobs.mask,
                jobs.rates.contiguous(), jobs.ul.contiguous(),
                jobs.dl.contiguous(), eng.k_conf_indptr, eng.k_conf_base,
                eng.k_conf_cols, eng.link_rates.contiguous(),
                eng.bw_comp.contiguous(), eng.k_E_arr,
                eng.T_arr.contiguous(), eng.Ee, iters, 0.0)
            walk = lambda: eng._episode_eval(jobs, dst, sp)   # noqa: E731
            for mode, budget in modes:
                if has_switch:
                    ext.queue_csr_force_global(mode == "global")
                    ext.queue_csr_set_budget(-1 if budget is None else budget)
                row = {"config": "fixedpoint", "B": batch, "fp_iters": iters,
                       "mode": mode}
                if has_switch:
                    row["budget_bytes"] = ext.queue_csr_stage(
                        eng.N, eng.E, eng.Ee, iters)["critic"]["budget_bytes"]
                for name, fn in (("actor_head_fwd", fwd),
                                 ("actor_head_bwd", bwd), ("critic", crit),
                                 ("walk_eval", walk)):
                    row[name + "_us"] = round(timeit(fn, reps, 20), 1)
                print(json.dumps(row), flush=True)
            if has_switch:
                ext.queue_csr_force_global(False)
                ext.queue_csr_set_budget(-1)


def bench_apsp(batches=(256, 1024), reps=200):
    """``eng.apsp`` (one floyd_warshall_dm launch plus its output
    allocation) on the benchmark's batch and on the mixed 20–110 engine
    (10 sizes padded to 110, ``n_arr``), with the register-resident kernel
    and forced onto the in-place LDS kernel.  On a build without the switch
    it times the kernel as it is."""
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.harness.train_batched import build_training_cases
    from multihop_offload_amd.ops import dispatch

    ext = dispatch.require_hip()
    has_switch = hasattr(ext, "fw_force_inplace")
    modes = ["registers", "inplace"] if has_switch else ["as_built"]

    def batch_cases(kind, batch):
        if kind == "bench":
            return build_training_cases(100, batch, 16, 1000, 100,
                                        gtype="ba", workers=8)
        sizes = list(range(20, 111, 10))
        cases = []
        for n in sizes:
            cases += [c.pad_to(110) for c in build_training_cases(
                n, max(batch // len(sizes), 8), 16, 1000, 100 + 17 * n,
                gtype="ba", workers=8)]
        return cases

    for kind in ("bench", "mixed_20_110"):
        for batch in batches:
            model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
            eng = EpisodeEngine(batch_cases(kind, batch), model,
                                device="cuda", dtype=torch.float32)
            gen = torch.Generator(device="cuda")
            gen.manual_seed(0)
            jobs = eng.sample_jobs(0.15, gen)
            with torch.no_grad():
                dm, *_ = eng.actor_forward(jobs)
            dm = dm.detach()
            row = {"config": "apsp", "batch": kind, "B": eng.B, "N": eng.N,
                   "padded": bool(eng._padded)}
            outs = []
            for mode in modes:
                if has_switch:
                    ext.fw_force_inplace(mode == "inplace")
                    row["rows_per_thread"] = max(
                        row.get("rows_per_thread", 0),
                        ext.fw_register_rows(eng.N))
                outs.append(eng.apsp(dm))
                row[mode + "_us"] = round(
                    timeit(lambda: eng.apsp(dm), reps, 20), 1)
            if has_switch:
                ext.fw_force_inplace(False)
                row["bit_equal"] = bool(torch.equal(
                    outs[0].view(torch.int32), outs[1].view(torch.int32)))
            print(json.dumps(row), flush=True)


def bench_cheb(batches=(256, 1024), reps=200):
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.harness.train_batched import build_training_cases
    from multihop_offload_amd.ops import dispatch
    from multihop_offload_amd.ops.functions import pack_cheb_params

    ext = dispatch.require_hip()
    has_switch = hasattr(ext, "cheb_force_full_width")
    modes = ["edge", "full"] if has_switch else ["as_built"]
    for batch in batches:
        cases = build_training_cases(100, batch, 16, 1000, 100, gtype="ba",
                                     workers=8)
        model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
        with torch.no_grad():
            for p in model.parameters():
                p.mul_(0.01)
            model.layers[-1].bias.fill_(0.5)
        eng = EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)
        jobs = eng.sample_jobs(0.15, gen)
        x = eng._features(jobs).contiguous()
        csr = (eng.k_ext_indptr, eng.k_ext_base, eng.k_ext_cols,
               eng.k_ext_max_nnz)
        layers = list(eng.model.layers)
        for nl in (3, 5):
            params = []
            for layer in layers[:nl - 1] + layers[-1:]:
                params += [layer.weight, layer.bias]
            Wp, bp = pack_cheb_params(params)
            row = {"config": "cheb", "B": eng.B, "Ee": eng.Ee, "L": nl}
            for mode in modes:
                if has_switch:
                    ext.cheb_force_full_width(mode == "full")
                    fwd = lambda: ext.cheb_fwd_edge(      # noqa: E731
                        x, Wp, bp, *csr, 1)
                    lam, acts, t1s, edge = fwd()
                    assert edge == (mode == "edge")
                    dlam = torch.randn_like(lam)
                    bwd = lambda: ext.cheb_bwd_edge(      # noqa: E731
                        dlam, x, lam, acts, t1s, Wp, *csr, edge)
                else:
                    fwd = lambda: ext.cheb_fwd(x, Wp, bp, *csr)  # noqa: E731
                    lam, acts, t1s = fwd()
                    dlam = torch.randn_like(lam)
                    bwd = lambda: ext.cheb_bwd(           # noqa: E731
                        dlam, acts, t1s, Wp, *csr)
                row[f"cheb_fwd_{mode}_us"] = round(timeit(fwd, reps, 20), 1)
                row[f"cheb_bwd_{mode}_us"] = round(timeit(bwd, reps, 20), 1)
            if has_switch:
                ext.cheb_force_full_width(False)
            print(json.dumps(row), flush=True)


def _bench_engine(batch):
    """The benchmark's own batch (BA-100, seed 100) and model."""
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.harness.train_batched import build_training_cases

    cases = build_training_cases(100, batch, 16, 1000, 100, gtype="ba",
                                 workers=8)
    model = ChebConvStack(K=2, dtype=torch.float32, seed=100)
    return EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)


def bench_adam(batches=(256, 1024), reps=200):
    """``FusedAdam.step`` alone (one fused_adam launch) on the benchmark's
    model, with the gradients one training episode of the benchmark's batch
    leaves in ``flat_g``: the one-workgroup-per-tensor kernel against the
    single-block one (``adam_force_single_block``).  The kernel sees the
    batch only through the gradient values.  On a build without the switch it
    times the kernel as it is."""
    from multihop_offload_amd.ops import dispatch
    from multihop_offload_amd.ops.functions import FusedAdam

    ext = dispatch.require_hip()
    has_switch = hasattr(ext, "adam_force_single_block")
    modes = ["blocks", "single"] if has_switch else ["as_built"]
    for batch in batches:
        eng = _bench_engine(batch)
        opt = FusedAdam(eng.model, lr=1e-4)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)
        opt.zero_grad()
        eng.gnn_episode(eng.sample_jobs(0.15, gen), explore=0.0, gen=gen,
                        train=True)
        row = {"config": "adam", "B": eng.B, "n_seg": int(opt.seg.shape[0]),
               "n_param": int(opt.flat_p.numel())}
        for mode in modes:
            if has_switch:
                ext.adam_force_single_block(mode == "single")
            # scale 1: the gradient keeps its magnitude over the launches
            row[mode + "_us"] = round(
                timeit(lambda: opt.step(scale=1.0), reps, 20), 1)
        if has_switch:
            ext.adam_force_single_block(False)
        print(json.dumps(row), flush=True)


def bench_walk(batches=(256, 1024), reps=200):
    """``eng._episode_eval`` (one walk_eval launch, its output allocations
    and the overflow bookkeeping around it) and the bare ``ext.walk_eval``
    call on the benchmark's batch, after the step's own forward, APSP and
    decision."""
    from multihop_offload_amd.ops import dispatch

    ext = dispatch.require_hip()
    for batch in batches:
        eng = _bench_engine(batch)
        gen = torch.Generator(device="cuda")
        gen.manual_seed(0)
        jobs = eng.sample_jobs(0.15, gen)
        with torch.no_grad():
            dm, *_ = eng.actor_forward(jobs)
        dm = dm.detach()
        sp = eng.apsp(dm)
        uds = torch.diagonal(dm, dim1=1, dim2=2)
        dst, _ = eng.offload_decide(jobs, sp, uds)
        args = (sp.contiguous(), jobs.sources, dst.contiguous(), jobs.mask,
                jobs.rates.contiguous(), jobs.ul.contiguous(),
                jobs.dl.contiguous(), eng.k_adj_indptr, eng.k_adj_idx,
                eng.k_adj_link, eng.k_conf_indptr, eng.k_conf_base,
                eng.k_conf_cols, eng.link_rates.contiguous(),
                eng.proc_bws.contiguous(), eng.k_edges,
                eng.T_arr.contiguous(), eng.k_E_arr, eng.k_N_arr,
                min(eng.walk_cap, 64), eng.fp_iters)
        row = {"config": "walk", "B": eng.B, "N": eng.N, "E": eng.E,
               "J": eng.Jmax}
        row["walk_eval_us"] = round(
            timeit(lambda: ext.walk_eval(*args), reps, 20), 1)
        row["episode_eval_us"] = round(
            timeit(lambda: eng._episode_eval(jobs, dst, sp), reps, 20), 1)
        print(json.dumps(row), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="both",
                    choices=["flagship", "er1000", "both", "timeslot",
                             "timeslot_stats", "timeslot_mwis",
                             "timeslot_mwis_stats", "fixedpoint", "apsp",
                             "cheb", "adam", "walk"])
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--budgets", type=str, default="-1",
                    help="fixedpoint: staging budgets in bytes, comma-"
                         "separated (-1 = the built-in default)")
    args = ap.parse_args()
    if args.config == "fixedpoint":
        bench_fixedpoint(budgets=tuple(int(b) for b in
                                       args.budgets.split(",")),
                         reps=max(args.reps, 100))
    if args.config == "apsp":
        bench_apsp(reps=max(args.reps, 200))
    if args.config == "cheb":
        bench_cheb(reps=max(args.reps, 200))
    if args.config == "adam":
        bench_adam(reps=max(args.reps, 200))
    if args.config == "walk":
        bench_walk(reps=max(args.reps, 200))
    if args.config == "timeslot":
        bench_timeslot(reps=args.reps)
    if args.config == "timeslot_stats":
        bench_timeslot(reps=args.reps, stats=True)
    if args.config == "timeslot_mwis":
        bench_timeslot(reps=args.reps, mac="mwis")
    if args.config == "timeslot_mwis_stats":
        bench_timeslot(reps=args.reps, stats=True, mac="mwis")
    if args.config in ("flagship", "both"):
        bench_config("flagship_b1024_n110", 110, 1024, "ba", 16, args.reps)
    if args.config in ("er1000", "both"):
        bench_config("er1000_b64", 1000, 64, "er", 1, max(args.reps // 5, 5))
