"""Inputs that make walk_eval's last-job-wins rule visible (CPU only; used by
tests/test_walk_pack_inputs.py and tests/test_gpu_walk_pack.py).

With the sampler's constant ul / dl, two jobs on one congested link always
carry the same fallback unit, so it cannot be seen which of them was written
last.  Here the jobs of ``stage_oracle.front(name)`` get

    ul = 100 · (1 + 0.5 · (j mod 3)),   dl = 1 + (j mod 2)      (j: job slot)

their rates × 4 (rounded to fp32), and every real job is sent to its graph's
first server, so the routes converge on shared, congested links and on one
congested destination, with different ul + dl per job.  Routes come from the
CPU engine's ``route_walk`` on the front's fp32-rounded APSP, the expected
outputs from ``stage_oracle.eval_oracle``.
"""
import functools

import torch

from tests import stage_oracle as so

SETS = ("A", "C")
# truncated walks with walk_cap = 3 (asserted in test_walk_pack_inputs.py)
TRUNCATED = {"A": 7, "C": 5}
# lower bounds on the number of links shared by two or more jobs
MIN_SHARED = {"A": 20, "C": 10}
CAP = 3


@functools.lru_cache(maxsize=None)
def front(name, walk_cap=None):
    """The front dict of ``stage_oracle`` (sp, jobs, dst, route_links, nhop,
    overflow, H) under this module's recipe."""
    base = so.front(name)
    eng = so.engine(name, 0.0, walk_cap=walk_cap)
    jb = base["jobs"]
    j = torch.arange(jb.mask.shape[1])[None, :].expand_as(jb.mask)
    f64 = torch.float64
    jobs = so.JobBatch(
        sources=jb.sources.clone(), mask=jb.mask.clone(),
        rates=so.as32(jb.rates * 4.0),
        ul=(100.0 * (1.0 + 0.5 * (j % 3).to(f64))).contiguous(),
        dl=(1.0 + (j % 2).to(f64)).contiguous())
    first = eng.servers[:, :1].to(torch.int64).expand_as(jb.sources)
    dst = torch.where(jb.mask, first, jb.sources)
    with torch.no_grad():
        eng.overflow_total.zero_()
        rl, nhop = eng.route_walk(jobs, dst, base["sp"])
        overflow = int(eng.overflow_total)
        eng.overflow_total.zero_()
    H = min(eng.walk_cap, 64)
    return dict(sp=base["sp"], jobs=jobs, dst=dst,
                route_links=so.pad_routes(rl, H), nhop=nhop,
                overflow=overflow, H=H)


@functools.lru_cache(maxsize=None)
def case(name, walk_cap=None):
    """Front, fp64 oracle outputs (delay_emp, unit_mtx, written), the
    fp32-reference errors and the tolerances ``stage_oracle.tolerance``
    derives from them — the rule of test_walk_eval_vs_fp64."""
    fr = front(name, walk_cap)
    want = so.eval_oracle(so.engine(name), fr)[:3]
    ref = so._eval_errs(
        so.eval_oracle(so.engine(name, 0.0, "float32"), fr)[:3], want)
    return dict(front=fr, want=want, ref=ref,
                tol={k: so.tolerance(v) for k, v in ref.items()})


def conditions(name):
    """What the fp64 oracle alone shows about ``front(name)``: per shared
    link (two or more jobs) whether it is congested and carries different
    ul + dl; whether each graph's shared destination is congested; the
    smallest relative distance of a used link or server from the
    mu - lam = 0 boundary."""
    eng, fr = so.engine(name), front(name)
    jobs, rl, dst = fr["jobs"], fr["route_links"], fr["dst"]
    _, _, _, lam, mu, sload = so.eval_oracle(eng, fr)
    tot = jobs.ul + jobs.dl
    shared, gap = [], float("inf")
    for b in range(eng.B):
        on = {}
        for jj in torch.nonzero(jobs.mask[b]).flatten().tolist():
            for l in rl[b, jj][rl[b, jj] >= 0].tolist():
                on.setdefault(l, []).append(float(tot[b, jj]))
        for l, ts in on.items():
            gap = min(gap, abs(float(mu[b, l] - lam[b, l]))
                      / float(mu[b, l]))
            if len(ts) >= 2:
                shared.append(dict(b=b, link=l, jobs=len(ts),
                                   congested=bool(lam[b, l] > mu[b, l]),
                                   distinct=len(set(ts)) >= 2))
    dsts = []
    for b in range(eng.B):
        d = int(eng.servers[b, 0])
        assert bool((dst[b][jobs.mask[b]] == d).all())
        bw = float(eng.proc_bws[b, d])
        gap = min(gap, abs(bw - float(sload[b, d])) / bw)
        dsts.append(bool(sload[b, d] > bw))
    return dict(shared=shared, dst_congested=dsts, gap=gap)
