#!/usr/bin/env python3
"""Flagship benchmark: batched GNN-offloading training steps on MI355X.

Measures the BASELINE.json headline ("episodes/sec, 100-node BA load=0.15"):
one step = one full training iteration over a device-resident batch of
(graph, jobs) episodes — job sampling, ChebConv forward, contention fixed
point, batched min-plus APSP (HIP), offloading decisions + greedy routing,
analytic queueing evaluation, critic + semi-analytic backward, DP gradient
all-reduce (RCCL over xGMI for --gpus > 1) and the Adam step with Keras
max_norm constraints.

Launch (driver contract):
  python bench.py --gpus N --steps K --warmup W
  # N>1: python -m torch.distributed.run --nnodes=1 --nproc-per-node N \
  #        --master-addr 127.0.0.1 bench.py --gpus N ...
  # --dump-outputs DIR  write the last timed step's outputs as DIR/*.npy
  # --full              everything beyond the headline figure (nothing yet)

Reference speed anchor: GNN train step ≈ 0.25 s/instance
(unknown hardware) ⇒ 4 episodes/sec.
"""

import argparse
import json
import os
import sys
import time

import torch


def build_cases(n_nodes, batch, distinct, T, seed, gtype="ba", workers=None):
    """Synthetic cases of the named config: topologies with the datagen
    role/bandwidth distributions; the batch replicates `distinct`
    topologies with independent link-rate draws (data=synthetic)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from multihop_offload_amd.harness.train_batched import \
        build_training_cases
    if workers is None:
        # avoid oversubscribing the host CPU when several DP ranks build
        # their cases concurrently
        world = int(os.environ.get("WORLD_SIZE", "1"))
        workers = max(2, 16 // max(world, 1))
    return build_training_cases(n_nodes, batch, distinct, T, seed,
                                gtype=gtype, workers=workers)


def dump_outputs(path, results, model):
    """Write what the last timed step handed back as ``path/<name>.npy``:
    the per-engine EpisodeResult fields and the model parameters after the
    optimizer update (one flat vector, in ``model.parameters()`` order).
    Floating arrays keep their dtype (fp32 on GPU, fp64 on CPU), counts are
    stored as float64.  ``delay_emp`` is nan-padded past each graph's job
    count; the padding is written as 0 so the files compare with plain
    ``allclose`` (``num_jobs`` gives the valid prefix of every row)."""
    import numpy as np

    def host(t):
        a = t.detach().cpu().numpy()
        return a if a.dtype in (np.float32, np.float64) \
            else a.astype(np.float64)

    os.makedirs(path, exist_ok=True)
    arrays = {}
    for i, res in enumerate(results):
        tag = "" if len(results) == 1 else f"_engine{i}"
        valid = torch.arange(res.delay_emp.shape[1],
                             device=res.delay_emp.device)[None, :] \
            < res.num_jobs[:, None]
        arrays["tau" + tag] = host(res.tau)
        arrays["congest" + tag] = host(res.congest)
        arrays["num_jobs" + tag] = host(res.num_jobs)
        arrays["delay_emp" + tag] = host(torch.where(
            valid, res.delay_emp, torch.zeros_like(res.delay_emp)))
        arrays["loss_fn" + tag] = host(res.loss_fn).reshape(1)
        arrays["loss_mse" + tag] = host(res.loss_mse).reshape(1)
    arrays["params"] = host(torch.cat(
        [p.detach().reshape(-1) for p in model.parameters()]))
    total = sum(a.nbytes for a in arrays.values())
    assert total <= 64 * 2 ** 20, f"dump too large: {total} bytes"
    for name, a in arrays.items():
        np.save(os.path.join(path, name + ".npy"), a)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=None,
                    help="timed steps (default: 200 on GPU — long enough "
                         "for SMI utilisation sampling to corroborate the "
                         "timed region — 10 on CPU)")
    ap.add_argument("--warmup", type=int, default=None)
    ap.add_argument("--batch", type=int, default=256,
                    help="episodes per GPU per step (weak scaling)")
    ap.add_argument("--global_batch", type=int, default=0,
                    help="TOTAL episodes per step split across ranks "
                         "(strong scaling; overrides --batch).  BASELINE "
                         "config 3 is `--gpus 8 --global_batch 256 "
                         "--nodes 110`: a batch of 256 110-node graphs "
                         "sharded over 8 GPUs")
    ap.add_argument("--nodes", type=int, default=100)
    ap.add_argument("--distinct", type=int, default=16)
    ap.add_argument("--gtype", type=str, default="ba",
                    help="graph family (BASELINE config 4: --gtype er "
                         "--nodes 1000 --distinct 1)")
    ap.add_argument("--sizes", type=str, default=None,
                    help="BASELINE config 5: comma-separated node counts "
                         "in ONE padded engine (per-graph T drawn from "
                         "{700,800,950,1000}; inert-node padding with "
                         "per-graph kernel bounds — measured 3.75x faster "
                         "than per-size engine buckets)")
    ap.add_argument("--size_buckets", action="store_true",
                    help="config 5 via one engine per size (the slower "
                         "round-1 layout, kept for comparison)")
    ap.add_argument("--T", type=int, default=1000)
    ap.add_argument("--load", type=float, default=0.15)
    ap.add_argument("--K", type=int, default=2)
    ap.add_argument("--seed", type=int, default=100)
    ap.add_argument("--device", type=str, default=None)
    ap.add_argument("--capture", action="store_true",
                    help="capture the whole training step in a hipGraph "
                         "and replay it (single-GPU)")
    ap.add_argument("--dump-outputs", type=str, default=None, metavar="DIR",
                    help="after the timed steps, write what the last timed "
                         "step computed (episode results + updated "
                         "parameters) as DIR/<name>.npy; inputs are seeded, "
                         "so two builds can be compared output for output")
    ap.add_argument("--full", action="store_true",
                    help="also run the measurements and checks beyond the "
                         "headline figure (none at present: a plain run "
                         "already does only set-up, warm-up and the timed "
                         "steps)")
    args = ap.parse_args()

    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.parallel import dp

    rank, world = dp.init_from_env()
    if args.global_batch:
        assert args.global_batch % world == 0, \
            "--global_batch must divide evenly across ranks"
        args.batch = args.global_batch // world
    use_cuda = torch.cuda.is_available()
    device = args.device or ("cuda" if use_cuda else "cpu")
    if args.steps is None:
        args.steps = 200 if device.startswith("cuda") else 10
    if args.warmup is None:
        args.warmup = 20 if device.startswith("cuda") else 3
    dtype = torch.float32 if device.startswith("cuda") else torch.float64
    import torch.distributed as dist
    distributed = dist.is_available() and dist.is_initialized()
    capture = args.capture and use_cuda and not distributed

    from multihop_offload_amd.ops import dispatch as mho_dispatch
    use_fused = use_cuda and mho_dispatch.hip_available() \
        and dtype == torch.float32
    model = ChebConvStack(K=args.K, dtype=dtype, seed=args.seed)
    if args.sizes:
        sizes = [int(s) for s in args.sizes.split(",")]
        t_choices = [700, 800, 950, 1000]
        if args.size_buckets:
            engines = []
            for i, n in enumerate(sizes):
                cases = build_cases(n, max(args.batch // len(sizes), 8),
                                    min(args.distinct, 8),
                                    t_choices[i % len(t_choices)],
                                    args.seed + rank + 31 * n, args.gtype)
                engines.append(EpisodeEngine(cases, model, device=device,
                                             dtype=dtype))
        else:
            n_max = max(sizes)
            cases = []
            for i, n in enumerate(sizes):
                cases += [c.pad_to(n_max) for c in build_cases(
                    n, max(args.batch // len(sizes), 8),
                    min(args.distinct, 8),
                    t_choices[i % len(t_choices)],
                    args.seed + rank + 31 * n, args.gtype)]
            engines = [EpisodeEngine(cases, model, device=device,
                                     dtype=dtype)]
        episodes_per_step = sum(e.B for e in engines)
    else:
        cases = build_cases(args.nodes, args.batch, args.distinct, args.T,
                            args.seed + rank, args.gtype)
        engines = [EpisodeEngine(cases, model, device=device, dtype=dtype)]
        episodes_per_step = args.batch
    engine = engines[0]
    if use_fused:
        from multihop_offload_amd.ops.functions import FusedAdam
        optimizer = FusedAdam(engine.model, lr=1e-4)
        reducer = None
    else:
        optimizer = torch.optim.Adam(engine.model.parameters(), lr=1e-4,
                                     eps=1e-7, capturable=capture,
                                     foreach=True)
        reducer = dp.FlatAllreduce(engine.model.parameters())
    dp.broadcast_params(engine.model)
    if args.capture and use_cuda:
        gen = None                     # default generator is graph-safe
        torch.manual_seed(args.seed * 1009 + rank)
    else:
        gen = torch.Generator(device=device)
        gen.manual_seed(args.seed * 1009 + rank)

    def step():
        if use_fused:
            optimizer.zero_grad()
        else:
            for p in model.parameters():
                p.grad = None
        res = []                       # one EpisodeResult per engine
        for eng in engines:
            jobs = eng.sample_jobs(args.load, gen)
            res.append(eng.gnn_episode(jobs, explore=0.0, gen=gen,
                                       train=True))
        if use_fused:
            # one fused kernel: grad mean-scale, per-tensor clipnorm, Adam,
            # max_norm constraints; flat_g is the single RCCL payload
            if distributed:
                dist.all_reduce(optimizer.flat_g)
            optimizer.step(scale=1.0 / (episodes_per_step * world))
            return res
        # torch fallback path (CPU / no HIP)
        with torch.no_grad():
            for p in model.parameters():
                if p.grad is not None:
                    p.grad /= episodes_per_step
        reducer(average=True)
        with torch.no_grad():
            for p in model.parameters():
                if p.grad is not None:
                    n = p.grad.norm().clamp(min=1e-12)
                    p.grad *= torch.clamp(n, max=1.0) / n
        optimizer.step()
        model.apply_constraints()
        return res

    for _ in range(args.warmup):
        step()

    if capture:
        # hipGraph capture: the step must be sync-free and use the default
        # (graph-safe) RNG; replays advance RNG state per torch's graph pool
        torch.cuda.synchronize()
        hip_graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(hip_graph):
            captured = step()
        step = lambda: hip_graph.replay() or captured  # noqa: E731

    if distributed:
        dist.barrier()
    if use_cuda:
        torch.cuda.synchronize()
    t0 = time.perf_counter()
    last = None
    for _ in range(args.steps):
        last = step()
    if use_cuda:
        torch.cuda.synchronize()
    elapsed = time.perf_counter() - t0
    if distributed:
        e = torch.tensor([elapsed])
        if use_cuda:
            e = e.cuda()
        dist.all_reduce(e, op=dist.ReduceOp.MAX)
        elapsed = float(e.item())
        dist.barrier()

    n_gpus = world if distributed else 1
    episodes = episodes_per_step * n_gpus * args.steps
    value = episodes / elapsed
    ms_per_step = elapsed / args.steps * 1000.0
    if rank == 0:
        out = {
            "metric": "episodes/sec",
            "value": value,
            "unit": "episodes/s",
            "n_gpus": n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "strong" if args.global_batch else "weak",
            "vs_baseline": value / 4.0,
            "dtype": "fp32" if dtype == torch.float32 else "fp64",
            "data": "synthetic",
            "config": {
                "model": f"ChebConv-K{args.K}-5L-h32",
                "graph": (f"mixed[{args.sizes}]-{args.gtype}" if args.sizes
                          else f"{args.gtype}{args.nodes}" +
                          ("-m2" if args.gtype == "ba" else "")),
                "global_batch": episodes_per_step * n_gpus,
                "load": args.load,
                "T": args.T,
                "parallelism": f"dp{n_gpus}",
                "tau_gnn": float(torch.nanmean(last[-1].tau)),
                "congest_jobs": int(last[-1].congest.sum()),
            },
        }
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, last, model)
        print(json.dumps(out))
    if distributed:
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
