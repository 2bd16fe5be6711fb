"""Batched evaluator: reproduce the reference's headline table
(BASELINE.md / SURVEY.md §6) — mean task latency τ and task congestion
ratio for baseline / local / GNN over 20–110-node BA cases at a given load.

Uses the device-resident engine per node-size bucket (each bucket is a
same-N batch); GNN runs forward-only with the loaded checkpoint.

Run:  python -m multihop_offload_amd.harness.evaluate \
          --training_set BAT1000 --instances 10 --cases-per-size 20
"""

from __future__ import annotations

import argparse
import json
import os

import torch

from ..engine import EpisodeEngine, hist_percentile
from ..models.chebconv import ChebConvStack
from ..utils.checkpoint import latest_checkpoint, load, model_dir
from .train_batched import build_training_cases


def evaluate(model, sizes, cases_per_size, instances, T, load, seed,
             device, dtype, workers: int = 8, lam_margin: float = 0.0,
             refine: int = 0, simulate: int = 0, sim_warmup: int = 0,
             sim_stats: bool = False, sim_mac: str = "share"):
    """Returns per-method aggregate {tau, congest_jobs, num_jobs} summed /
    averaged over all (size, case, instance).  ``simulate`` > 0 also replays
    every episode's routes in the per-timeslot packet simulator for that
    many slots (one arrival draw per job instance, shared by the methods,
    from a generator of its own so the analytic fields do not move) and
    adds ``sim_tau`` (task-weighted mean simulated sojourn of the tasks
    that arrived after ``sim_warmup`` and completed), ``sim_backlog_ratio``
    (the share of those arrivals still in the network at the end) and
    ``sim_tasks`` (completed tasks).  ``sim_stats`` runs the simulator in
    its statistics mode and adds, over the same tasks: ``sim_p50`` /
    ``sim_p95`` / ``sim_p99`` (histogram upper bounds on the sojourn
    percentiles, all histograms merged), ``sim_late_ratio`` (share of the
    completed tasks later than the graph's horizon T, the packet-level
    counterpart of ``congest_ratio``), ``sim_tau_censored`` (mean sojourn
    with every task still in the network counted at its age so far: a lower
    bound that does not drop them) and ``sim_link_util_max`` /
    ``sim_node_util_max`` (the busiest link's and node's share of busy
    slots).  ``sim_mac="mwis"`` computes every ``sim_*`` field under the
    scheduled MAC of ``EpisodeEngine.simulate(mac="mwis")`` and, with
    ``sim_stats``, adds ``sim_sched_share``: the scheduled slots of all
    links over their busy slots."""
    mwis = sim_mac == "mwis"

    def fresh():
        return {"tau_sum": 0.0, "tau_n": 0, "congest": 0, "jobs": 0,
                "ratio_sum": 0.0, "ratio_n": 0, "sim_delay": 0,
                "sim_tasks": 0, "sim_backlog": 0, "sim_arrived": 0,
                "sim_hist": None, "sim_dmax": 0, "sim_late": 0,
                "sim_stuck_age": 0, "sim_link_util": 0.0,
                "sim_node_util": 0.0, "sim_sched": 0, "sim_busy": 0}

    def fields(d, jobs_too=False):
        out = {"tau": d["tau_sum"] / max(d["tau_n"], 1),
               "congest_ratio": d["congest"] / max(d["jobs"], 1),
               "latency_ratio": d["ratio_sum"] / max(d["ratio_n"], 1)}
        if jobs_too:
            out["jobs"] = d["jobs"]
        if simulate:
            out["sim_tau"] = (d["sim_delay"] / d["sim_tasks"]
                              if d["sim_tasks"] else float("nan"))
            out["sim_backlog_ratio"] = (d["sim_backlog"]
                                        / max(d["sim_arrived"], 1))
            out["sim_tasks"] = d["sim_tasks"]
        if simulate and sim_stats:
            for name, q in (("sim_p50", 0.5), ("sim_p95", 0.95),
                            ("sim_p99", 0.99)):
                out[name] = float(hist_percentile(
                    d["sim_hist"], torch.tensor(d["sim_dmax"]), q))
            out["sim_late_ratio"] = (d["sim_late"] / d["sim_tasks"]
                                     if d["sim_tasks"] else float("nan"))
            seen = d["sim_tasks"] + d["sim_backlog"]
            out["sim_tau_censored"] = (
                (d["sim_delay"] + d["sim_stuck_age"]) / seen
                if seen else float("nan"))
            out["sim_link_util_max"] = d["sim_link_util"]
            out["sim_node_util_max"] = d["sim_node_util"]
            if mwis:
                out["sim_sched_share"] = (d["sim_sched"] / d["sim_busy"]
                                          if d["sim_busy"] else float("nan"))
        return out

    agg = {m: fresh() for m in ("baseline", "local", "GNN")}
    per_size = {}
    for n in sizes:
        cases = build_training_cases(n, cases_per_size, cases_per_size, T,
                                     seed + n, workers=workers)
        engine = EpisodeEngine(cases, model, device=device, dtype=dtype,
                               lam_margin=lam_margin)
        gen = torch.Generator(device=device)
        gen.manual_seed(seed + n)
        sim_gen = torch.Generator(device=device)
        sim_gen.manual_seed(seed + n + 7919)
        ps = {m: fresh() for m in ("baseline", "local", "GNN")}
        for _ in range(instances):
            jobs = engine.sample_jobs(load, gen)
            results = {
                "baseline": engine.baseline_episode(jobs),
                "local": engine.local_episode(jobs),
                "GNN": engine.gnn_episode(jobs, train=False,
                                          refine=refine),
            }
            arrivals = (engine.draw_arrivals(jobs, simulate, sim_gen)
                        if simulate else None)
            bl = results["baseline"].delay_emp
            for m, res in results.items():
                # per-task latency ratio vs baseline (notebook cell 16)
                r = res.delay_emp / bl
                ok = torch.isfinite(r)
                sim = (engine.simulate(jobs, res, arrivals,
                                       warmup=sim_warmup, stats=sim_stats,
                                       mac=sim_mac)
                       if simulate else None)
                for d in (agg[m], ps[m]):
                    d["tau_sum"] += float(torch.nansum(res.tau))
                    d["tau_n"] += int(torch.isfinite(res.tau).sum())
                    d["congest"] += int(res.congest.sum())
                    d["jobs"] += int(res.num_jobs.sum())
                    d["ratio_sum"] += float(r[ok].sum())
                    d["ratio_n"] += int(ok.sum())
                    if sim is not None:
                        d["sim_delay"] += int(sim.delay_sum.sum())
                        d["sim_tasks"] += int(sim.count.sum())
                        d["sim_backlog"] += int(sim.backlog.sum())
                        d["sim_arrived"] += int(sim.backlog.sum()
                                                + sim.count.sum())
                    if sim is not None and sim.stats is not None:
                        st = sim.stats
                        hist = st.delay_hist.sum((0, 1),
                                                 dtype=torch.int64).cpu()
                        d["sim_hist"] = hist if d["sim_hist"] is None \
                            else d["sim_hist"] + hist
                        d["sim_dmax"] = max(d["sim_dmax"],
                                            int(st.delay_max.max()))
                        d["sim_late"] += int(st.late.sum())
                        d["sim_stuck_age"] += int(st.stuck_age.sum())
                        util = st.utilization()
                        E = st.num_links
                        d["sim_link_util"] = max(
                            d["sim_link_util"],
                            float(util[:, :E].max()) if E else 0.0)
                        d["sim_node_util"] = max(d["sim_node_util"],
                                                 float(util[:, E:].max()))
                        if mwis:
                            d["sim_sched"] += int(sim.sched_slots.sum())
                            d["sim_busy"] += int(st.busy_slots[:, :E].sum())
        engine.check_overflow()       # strict: truncated walks void an eval
        per_size[n] = {m: fields(d) for m, d in ps.items()}
    summary = {m: fields(d, jobs_too=True) for m, d in agg.items()}
    return summary, per_size


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--training_set", type=str, default="BAT1000")
    ap.add_argument("--model_root", type=str, default="model")
    ap.add_argument("--sizes", type=str, default="20,30,40,50,60,70,80,90,100,110")
    ap.add_argument("--cases-per-size", type=int, default=20)
    ap.add_argument("--instances", type=int, default=10)
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--load", type=float, default=0.15)
    ap.add_argument("--K", type=int, default=2)
    ap.add_argument("--seed", type=int, default=500)
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--lam_margin", type=float, default=0.0,
                    help="inference-time conservatism: inflate predicted "
                         "traffic by (1+margin) at decision time "
                         "(congestion-tail control; 0 = reference)")
    ap.add_argument("--refine", type=int, default=0,
                    help="congestion-aware refinement passes: jobs whose "
                         "analytic delay exceeds T fall back to local and "
                         "the assignment is re-evaluated (NOT reference "
                         "semantics; reported results must say so)")
    ap.add_argument("--simulate", type=int, default=0, metavar="T_SIM",
                    help="also replay every episode in the per-timeslot "
                         "packet simulator for T_SIM slots and report "
                         "sim_tau / sim_backlog_ratio / sim_tasks next to "
                         "the analytic fields (0 = off)")
    ap.add_argument("--sim-warmup", type=int, default=0,
                    help="slots whose arrivals the simulated figures skip")
    ap.add_argument("--sim-stats", action="store_true",
                    help="with --simulate: also report sim_p50 / sim_p95 / "
                         "sim_p99, sim_late_ratio, sim_tau_censored, "
                         "sim_link_util_max and sim_node_util_max")
    ap.add_argument("--sim-mac", choices=("share", "mwis"), default="share",
                    help="with --simulate: the MAC model of the replay. "
                         "share: every busy link transmits at rate / (1 + "
                         "busy conflicting links); mwis: a queue-weighted "
                         "greedy independent set of the conflict graph "
                         "transmits at full rate each slot (recorded as "
                         "sim_mac; with --sim-stats also sim_sched_share)")
    ap.add_argument("--out", type=str, default="out/eval_summary.json")
    args = ap.parse_args(argv)
    if args.sim_stats and not args.simulate:
        ap.error("--sim-stats requires --simulate T_SIM")
    if args.sim_mac != "share" and not args.simulate:
        ap.error("--sim-mac requires --simulate T_SIM")

    device = args.device or ("cuda" if torch.cuda.is_available() else "cpu")
    dtype = torch.float32 if device.startswith("cuda") else torch.float64
    model = ChebConvStack(K=args.K, dtype=dtype)
    ckpt = latest_checkpoint(model_dir(args.model_root, args.training_set))
    if ckpt:
        load(model, ckpt)
        print(f"loaded {ckpt}")
    else:
        print("WARNING: no checkpoint found — evaluating random init")

    sizes = [int(s) for s in args.sizes.split(",")]
    summary, per_size = evaluate(model, sizes, args.cases_per_size,
                                 args.instances, args.T, args.load,
                                 args.seed, device, dtype, args.workers,
                                 lam_margin=args.lam_margin,
                                 refine=args.refine,
                                 simulate=args.simulate,
                                 sim_warmup=args.sim_warmup,
                                 sim_stats=args.sim_stats,
                                 sim_mac=args.sim_mac)
    os.makedirs(os.path.dirname(args.out) or ".", exist_ok=True)
    # the default MAC leaves the file's key set as it was before --sim-mac
    config = vars(args)
    doc = {"summary": summary, "per_size": per_size, "config": config}
    if args.sim_mac == "share":
        config = {k: v for k, v in config.items() if k != "sim_mac"}
        doc["config"] = config
    else:
        doc["sim_mac"] = args.sim_mac
    with open(args.out, "w") as f:
        json.dump(doc, f, indent=1)
    print(json.dumps(summary, indent=1))
    return summary


if __name__ == "__main__":
    main()
