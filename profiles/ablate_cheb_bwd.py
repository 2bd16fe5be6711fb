#!/usr/bin/env python3
"""Stage ablation of cheb_bwd (timing only — masked outputs are wrong):
times the kernel with cumulative stage masks and differences them.
bit0 act-mask+db, bit1 load_rows+wgrads, bit2 dx gemm, bit3 spmv.  On a
build with the edge-layer path it ablates both that path and the full-width
one (``cheb_force_full_width``), one JSON line each.

Run on MI355X:  python profiles/ablate_cheb_bwd.py [--bench --batch 256]
(``--bench``: the benchmark's graphs, BA-100 seed 100, instead of BA-110)
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
    return s.elapsed_time(e) * 1000.0 / reps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=1024)
    ap.add_argument("--bench", action="store_true")
    ap.add_argument("--reps", type=int, default=50)
    args = ap.parse_args()

    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.harness.train_batched import \
        build_training_cases
    from multihop_offload_amd.ops import dispatch
    from multihop_offload_amd.ops.functions import pack_cheb_params

    nodes, seed = (100, 100) if args.bench else (110, 7)
    cases = build_training_cases(nodes, args.batch, 16, 1000, seed,
                                 workers=8)
    model = ChebConvStack(K=2, dtype=torch.float32, seed=3)
    with torch.no_grad():
        for p in model.parameters():
            p.mul_(0.01)
        model.layers[-1].bias.fill_(0.5)
    eng = EpisodeEngine(cases, model, device="cuda", dtype=torch.float32)
    ext = dispatch.require_hip()
    gen = torch.Generator(device="cuda")
    gen.manual_seed(0)
    jobs = eng.sample_jobs(0.15, gen)
    params = []
    for layer in eng.model.layers:
        params += [layer.weight, layer.bias]
    x = torch.randn(eng.B, eng.Ee, 4, device="cuda")
    Wp, bp = pack_cheb_params(params)
    csr = (eng.k_ext_indptr, eng.k_ext_base, eng.k_ext_cols,
           eng.k_ext_max_nnz)
    has_switch = hasattr(ext, "cheb_force_full_width")
    for path in (("edge", "full") if has_switch else ("as_built",)):
        if has_switch:
            ext.cheb_force_full_width(path == "full")
            lam, acts, t1s, edge = ext.cheb_fwd_edge(x, Wp, bp, *csr, 1)
            ext.cheb_force_full_width(False)
            assert edge == (path == "edge")
        else:
            lam, acts, t1s = ext.cheb_fwd(x, Wp, bp, *csr)
        dlam = torch.randn_like(lam)

        def run(mask):
            if has_switch:
                return timeit(lambda: ext.cheb_bwd_edge_ablate(
                    dlam, x, lam, acts, t1s, Wp, *csr, edge, mask),
                    args.reps)
            return timeit(lambda: ext.cheb_bwd_ablate(
                dlam, acts, t1s, Wp, *csr, mask), args.reps)

        t = {m: run(m) for m in (0, 1, 3, 7, 15)}
        out = {
            "path": path, "B": eng.B, "Ee": eng.Ee,
            "skeleton(us)": round(t[0], 1),
            "act_mask_db(us)": round(t[1] - t[0], 1),
            "load_acts_wgrads(us)": round(t[3] - t[1], 1),
            "dx_gemm(us)": round(t[7] - t[3], 1),
            "spmv(us)": round(t[15] - t[7], 1),
            "full(us)": round(t[15], 1),
        }
        print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
