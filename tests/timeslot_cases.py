"""Shared inputs and oracle of the timeslot-simulator tests (CPU and GPU).

The oracle of every device comparison is ``sim.timeslot.simulate_routes`` on
fp64 copies of the arrays after rounding through ``np.float32`` — exactly the
values the kernel widens — and every comparison is integer equality.
"""
from types import SimpleNamespace

import numpy as np

from multihop_offload_amd import CaseGraph, JobInstance
from multihop_offload_amd.sim.timeslot import draw_arrivals, simulate_routes

T_SIM, WARMUP, ARR_SEED = 400, 50, 3
G1_SEEDS, G1_LOADS = (7, 8, 9), (0.15, 0.6, 0.3)


def make_case(seed, n=20):
    """The ``small_case`` recipe of conftest.py at another graph seed/size."""
    rng = np.random.RandomState(42)
    g = CaseGraph(n, t_max=1000, seed=seed, gtype="ba")
    g.links_init(50.0, rng=rng)
    g.add_relay(0)
    g.add_relay(1)
    for s in (2, 3, 4):
        g.add_server(s, 300.0)
    for v in range(5, n):
        g.set_mobile_bw(v, 10.0)
    return g


def jobs_at(g, load):
    return JobInstance.sample(g.mobile_nodes, load, np.random.RandomState(1))


def g1_batch():
    """Three 20-node cases at three loads (152, 550 and 291 tasks)."""
    cases = [make_case(s) for s in G1_SEEDS]
    jobs = [jobs_at(g, ld) for g, ld in zip(cases, G1_LOADS)]
    return cases, jobs


def g2_batch():
    """One 40-node case and one 20-node case padded to 40."""
    big = make_case(11, 40)
    small = make_case(7)
    cases = [big, small.pad_to(40)]
    jobs = [jobs_at(big, 0.3), jobs_at(small, 0.3)]
    return cases, jobs


def g3_case():
    """Order-sensitive hand-built case: a star, server 0 with leaves 1..3.
    Jobs sit on mobiles 2 and 1 (job order opposite to link order); the
    server's bandwidth equals ul, so it finishes one task per slot, and the
    link rates are equal and large enough that both uplinks deliver in the
    slot of arrival.  The task that the hand-over puts first is served a
    slot earlier."""
    adj = np.zeros((4, 4), dtype=np.int8)
    adj[0, 1:] = adj[1:, 0] = 1
    g = CaseGraph(4, t_max=1000, seed=0, gtype="ba", adj=adj)
    g.link_rates = np.full(g.num_links, 400.0)
    g.add_server(0, 100.0)
    for v in (1, 2, 3):
        g.set_mobile_bw(v, 1.0)
    jobs = JobInstance(sources=np.array([2, 1], dtype=np.int64),
                       rates=np.array([0.1, 0.1]),
                       ul=np.array([100.0, 100.0]),
                       dl=np.array([1.0, 1.0]))
    arrivals = np.zeros((40, 2), dtype=np.int64)
    arrivals[[0, 1, 7, 20, 21, 22]] = 1          # both jobs, same slots
    lm = np.asarray(g.link_matrix)
    route_links = np.array([[lm[2, 0]], [lm[1, 0]]], dtype=np.int64)
    nhop = np.array([1, 1], dtype=np.int64)
    dst = np.array([0, 0], dtype=np.int64)
    return g, jobs, arrivals, route_links, nhop, dst


def rounded(g):
    """The case as the kernel sees it: rates through fp32, widened again."""
    return SimpleNamespace(
        num_links=g.num_links, num_nodes=g.num_nodes,
        conf_indptr=g.conf_indptr, conf_indices=g.conf_indices,
        link_rates=np.asarray(g.link_rates).astype(np.float32)
        .astype(np.float64),
        proc_bws=np.asarray(g.proc_bws).astype(np.float32)
        .astype(np.float64))


def f32(a):
    return np.asarray(a).astype(np.float32).astype(np.float64)


def batch_arrivals(jobs_list, Jmax, T=T_SIM, seed=ARR_SEED):
    """(B,T,Jmax) int64, each case's own ``draw_arrivals`` stream, padded."""
    out = np.zeros((len(jobs_list), T, Jmax), dtype=np.int64)
    for b, jobs in enumerate(jobs_list):
        out[b, :, :jobs.num_jobs] = draw_arrivals(jobs, T, seed)
    return out


def oracle_batch(cases, jobs_list, dst, route_links, nhop, arrivals,
                 warmup=WARMUP, trace=True):
    """Per-case ``simulate_routes`` on the fp32-rounded arrays, packed like
    the device outputs: delay_sum (B,J) int64, count (B,J) int64, trace
    (B,T,3) int64; masked slots 0."""
    B, T, J = arrivals.shape
    ds = np.zeros((B, J), dtype=np.int64)
    ct = np.zeros((B, J), dtype=np.int64)
    tr = np.zeros((B, T, 3), dtype=np.int64)
    for b, (g, jobs) in enumerate(zip(cases, jobs_list)):
        k = jobs.num_jobs
        out = simulate_routes(rounded(g), f32(jobs.ul), f32(jobs.dl),
                              np.asarray(dst[b][:k]),
                              np.asarray(route_links[b][:k]),
                              np.asarray(nhop[b][:k]), arrivals[b][:, :k],
                              warmup=warmup, trace=trace)
        ds[b, :k], ct[b, :k] = out[0], out[1]
        if trace:
            for c, name in enumerate(("arrivals", "departures",
                                      "pkts_in_network")):
                tr[b, :, c] = out[2][name]
    return ds, ct, tr
