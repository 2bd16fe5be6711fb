"""Shared oracle loop of the scheduled-MAC simulator tests (CPU and GPU):
``tests.timeslot_cases.oracle_batch`` with ``mac="mwis"``, which also packs
the scheduled-slot counts and records every slot's schedule."""
import numpy as np

from multihop_offload_amd.sim import timeslot as ts
from tests import timeslot_cases as tc


def independent(g, on):
    """No two scheduled links of ``on`` conflict."""
    cip, cols = np.asarray(g.conf_indptr), np.asarray(g.conf_indices)
    return not any(on[cols[cip[l]:cip[l + 1]]].any()
                   for l in np.nonzero(on)[0])


def recorded(fn, *args, **kwargs):
    """``fn(*args, **kwargs)`` with every ``mwis_schedule`` call it makes
    recorded: returns ``(result, [(weights, on, rounds), ...])``."""
    real, log = ts.mwis_schedule, []

    def spy(cip, cols, w):
        on, r = real(cip, cols, w)
        log.append((np.array(w), on.copy(), r))
        return on, r
    ts.mwis_schedule = spy
    try:
        return fn(*args, **kwargs), log
    finally:
        ts.mwis_schedule = real


def oracle_case(g, jobs, dst, route_links, nhop, arrivals, warmup=tc.WARMUP,
                stats=False, late_after=None, mac="mwis"):
    """One case on the fp32-rounded arrays, as the kernel sees them."""
    k = jobs.num_jobs
    return ts.simulate_routes(
        tc.rounded(g), tc.f32(jobs.ul), tc.f32(jobs.dl), np.asarray(dst[:k]),
        np.asarray(route_links[:k]), np.asarray(nhop[:k]), arrivals[:, :k],
        warmup=warmup, trace=True, stats=stats, late_after=late_after,
        mac=mac)


def oracle_batch(cases, jobs_list, dst, route_links, nhop, arrivals,
                 warmup=tc.WARMUP):
    """Per-case ``simulate_routes(mac="mwis")`` packed like the device
    outputs: delay_sum, count (B,J), trace (B,T,3), sched_slots (B,E) with E
    the largest link count, all int64 and zero where padded; then the
    per-case ``rounds_max`` and the per-case schedule logs."""
    B, T, J = arrivals.shape
    E = max(g.num_links for g in cases)
    ds = np.zeros((B, J), dtype=np.int64)
    ct = np.zeros((B, J), dtype=np.int64)
    tr = np.zeros((B, T, 3), dtype=np.int64)
    sched = np.zeros((B, E), dtype=np.int64)
    rounds, logs = [], []
    for b, (g, jobs) in enumerate(zip(cases, jobs_list)):
        k = jobs.num_jobs
        out, log = recorded(oracle_case, g, jobs, dst[b], route_links[b],
                            nhop[b], arrivals[b], warmup=warmup)
        ds[b, :k], ct[b, :k] = out[0], out[1]
        for c, name in enumerate(("arrivals", "departures",
                                  "pkts_in_network")):
            tr[b, :, c] = out[2][name]
        sched[b, :g.num_links] = out[-1]["sched_slots"]
        rounds.append(out[-1]["rounds_max"])
        logs.append(log)
    return ds, ct, tr, sched, rounds, logs


def check_preconditions(cases, ct, ds, ds_share, rounds, logs):
    """What makes a batch worth comparing on: every case completes more than
    100 tasks and differs from the fluid-sharing run, some slot needs at
    least three rounds, and every recorded schedule is collision-free."""
    for b, g in enumerate(cases):
        assert ct[b].sum() > 100, (b, ct[b].sum())
        assert not np.array_equal(ds[b], ds_share[b]), b
        assert len(logs[b]) == tc.T_SIM
        for w, on, r in logs[b]:
            assert independent(g, on)
            assert not on[w <= 0].any()
    assert max(rounds) >= 3, rounds
