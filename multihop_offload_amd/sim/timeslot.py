"""Per-timeslot queueing simulator — validation oracle for the analytic
evaluator.

The reference's product path is the analytic M/M/1 + contention fixed-point
evaluator (``offloading_v3.py:455-550``); its repo carries vestiges of an
older per-timeslot packet simulator.  This module is a
compact discrete-time simulator used ONLY as a statistical cross-check of
the analytic evaluator in tests:

  * tasks arrive per job as Poisson(rate) per slot;
  * each task carries ``ul`` units to its destination hop-by-hop, is
    processed at the server (``ul`` units at the node bandwidth), and
    returns ``dl`` units hop-by-hop;
  * each link serves its FIFO with capacity ``rate_l / (1 + #busy
    conflicting links)`` units per slot (the same contention-sharing model
    the fixed point solves in steady state); servers serve at ``proc_bw``.

Under stable load the simulated mean task sojourn should track the analytic
per-job delays within a small factor (M/D/1-vs-M/M/1-style gap).
"""

from __future__ import annotations

from typing import List

import numpy as np

from ..env import AdhocCloudEnv, Flow
from ..graphs import CaseGraph, JobInstance


class _Task:
    __slots__ = ("job", "stage", "remaining", "t0", "done_at")

    def __init__(self, job: int, t0: int):
        self.job = job
        self.stage = 0           # index into the task's leg sequence
        self.remaining = 0.0
        self.t0 = t0
        self.done_at = -1


def draw_arrivals(jobs: JobInstance, T: int, seed: int) -> np.ndarray:
    """The (T, J) per-slot arrival counts ``simulate(seed=seed)`` draws
    inline: one ``RandomState(seed)`` stream, slot-major, job-minor."""
    rng = np.random.RandomState(seed)
    rates = np.asarray(jobs.rates, dtype=np.float64)
    return rng.poisson(rates, size=(int(T), len(rates)))


def delay_bin(d: int) -> int:
    """Histogram bin of a sojourn ``d >= 0``: exact below 16, then eight
    sub-bins per octave, so a bin is at most 12.5 % wide
    (``tsim::delay_bin`` in ops/hip/timeslot_phases.h is the same
    function)."""
    d = int(d)
    if d < 16:
        return d
    e = d.bit_length() - 1                      # floor(log2 d)
    return 16 + 8 * (e - 4) + ((d >> (e - 3)) & 7)


def delay_bin_upper(k: int) -> int:
    """The largest sojourn that falls into bin ``k``."""
    k = int(k)
    if k < 16:
        return k
    e, s = 4 + (k - 16) // 8, (k - 16) % 8
    return ((8 + s + 1) << (e - 3)) - 1


def num_delay_bins(T: int) -> int:
    """Bins of a ``T``-slot run: a sojourn cannot exceed ``T``."""
    return delay_bin(T) + 1


STAT_KEYS = ("delay_max", "late", "delay_hist", "stuck", "stuck_age",
             "qlen_sum", "qlen_max", "busy_slots", "nb_sum")

MAC_MODES = ("share", "mwis")


def mwis_schedule(conf_indptr, conf_indices, weights):
    """Distributed greedy maximum-weight independent set of the conflict
    graph (``utils.mwis.local_greedy_search`` on CSR rows) — the schedule of
    one slot under ``mac="mwis"``.

    The candidates are the links with ``weights[l] > 0``.  In each round a
    remaining candidate ``l`` wins when ``(w[l], -l) > (w[m], -m)`` for
    every remaining candidate ``m`` of its conflict row: a strictly larger
    weight, or an equal weight and the lower id.  All winners of a round are
    scheduled; they and their neighbours leave the candidate set.  The rows
    are symmetric without a self entry, so two adjacent links never win
    together and every round has a winner.  Returns ``(on bool (E,),
    rounds)``; ``rounds`` is 0 when there was no candidate."""
    w = np.asarray(weights, dtype=np.float64)
    E = len(w)
    cip = np.asarray(conf_indptr)
    cols = np.asarray(conf_indices)
    cand = w > 0
    on = np.zeros(E, dtype=bool)
    rounds = 0
    while cand.any():
        rounds += 1
        winners = []
        for l in np.nonzero(cand)[0]:
            for m in cols[cip[l]:cip[l + 1]]:
                if cand[m] and not (w[l] > w[m] or (w[l] == w[m] and l < m)):
                    break
            else:
                winners.append(int(l))
        assert winners, "conflict rows are not symmetric"
        for l in winners:
            on[l] = True
            cand[l] = False
            cand[cols[cip[l]:cip[l + 1]]] = False
    return on, rounds


def simulate_routes(g, ul, dl, dst, route_links, nhop, arrivals,
                    warmup: int = 0, trace: bool = False,
                    stats: bool = False, late_after=None,
                    mac: str = "share"):
    """The simulator loop over explicit routes — the contract of the batched
    HIP kernel (ops/hip/timeslot.hip), which reproduces it integer for
    integer.

    ``g`` supplies ``num_links``, ``num_nodes``, ``conf_indptr``,
    ``conf_indices``, ``link_rates`` and ``proc_bws``; ``route_links`` is
    (J, H) with job j's links in its first ``nhop[j]`` columns; ``arrivals``
    is (T, J) integer counts.  Returns ``(delay_sum int64 (J,), count int64
    (J,))`` over the tasks that arrived at ``t0 >= warmup`` and completed,
    plus the trace dict with ``trace=True``.

    ``stats=True`` appends a dict of integer arrays (``STAT_KEYS``).  Per
    job, over the counted tasks with sojourn ``d``: ``delay_max`` int32,
    ``late`` int32 (``d > late_after``, an int, default ``T``: never),
    ``delay_hist`` int32 (J, ``num_delay_bins(T)``) over ``delay_bin(d)``;
    after the last slot, over the tasks with ``t0 >= warmup`` still in the
    network: ``stuck`` int32 and ``stuck_age`` int64, the sum of ``T - t0``.
    Per resource (E + N,), link l at l and node v at E + v, over the slots
    ``t >= warmup`` sampled after the slot's arrivals and before service:
    ``qlen_sum`` int64, ``qlen_max`` int32, ``busy_slots`` int32 (FIFO not
    empty) and, links only, ``nb_sum`` int64: the busy conflicting links
    summed over the link's own busy slots.

    ``mac="mwis"`` replaces the fluid sharing by a collision-free schedule:
    after the slot's arrivals, ``w[l] = len(link_q[l]) * link_rates[l]`` (one
    fp64 multiply), ``on, r = mwis_schedule(conf_indptr, conf_indices, w)``,
    and only the links with ``on[l]`` serve, at the full ``link_rates[l]``.
    Nodes, the hand-over order, the trace, the warmup and every statistic
    keep their definitions (``busy_slots``: FIFO not empty; ``nb_sum``: busy
    conflicting links).  The returned tuple then ends with one more element,
    ``{"sched_slots": int32 (E,), "rounds_max": int}``: the slots ``t >=
    warmup`` in which each link was scheduled, and the largest number of
    rounds any slot's schedule took."""
    if mac not in MAC_MODES:
        raise ValueError(f"mac: one of {MAC_MODES}, not {mac!r}")
    mwis = mac == "mwis"
    arrivals = np.asarray(arrivals)
    T, J = arrivals.shape
    E, N = int(g.num_links), int(g.num_nodes)
    route_links = np.asarray(route_links).reshape(J, -1)
    conf_indptr = np.asarray(g.conf_indptr)
    conf_indices = np.asarray(g.conf_indices)
    link_rates = np.asarray(g.link_rates)
    proc_bws = np.asarray(g.proc_bws)

    # per-job leg sequence: [("link", l, ul)...] , ("node", dst, ul),
    # [("link", l, dl)... reversed]
    legs = []
    for j in range(J):
        links = route_links[j, :int(nhop[j])]
        seq = [("link", int(l), float(ul[j])) for l in links]
        seq.append(("node", int(dst[j]), float(ul[j])))
        seq += [("link", int(l), float(dl[j])) for l in links[::-1]]
        legs.append(seq)

    link_q: List[List[_Task]] = [[] for _ in range(E)]
    node_q: List[List[_Task]] = [[] for _ in range(N)]
    delay_sum = np.zeros(J, dtype=np.int64)
    count = np.zeros(J, dtype=np.int64)
    tr_arr = np.zeros(T, dtype=np.int64)
    tr_dep = np.zeros(T, dtype=np.int64)
    tr_net = np.zeros(T, dtype=np.int64)
    in_network = 0
    rows = np.repeat(np.arange(E), np.diff(conf_indptr[:E + 1]))
    if stats:
        late_after = T if late_after is None else int(late_after)
        delay_max = np.zeros(J, dtype=np.int32)
        late = np.zeros(J, dtype=np.int32)
        delay_hist = np.zeros((J, num_delay_bins(T)), dtype=np.int32)
        qlen_sum = np.zeros(E + N, dtype=np.int64)
        qlen_max = np.zeros(E + N, dtype=np.int32)
        busy_slots = np.zeros(E + N, dtype=np.int32)
        nb_sum = np.zeros(E + N, dtype=np.int64)
    if mwis:
        sched_slots = np.zeros(E, dtype=np.int32)
        rounds_max = 0

    def enqueue(task: _Task, t: int):
        while task.stage < len(legs[task.job]):
            kind, idx, units = legs[task.job][task.stage]
            task.remaining = units
            (link_q[idx] if kind == "link" else node_q[idx]).append(task)
            return
        task.done_at = t
        if task.t0 >= warmup:
            delay_sum[task.job] += t - task.t0
            count[task.job] += 1
            if stats:
                d = t - task.t0
                delay_max[task.job] = max(delay_max[task.job], d)
                late[task.job] += d > late_after
                delay_hist[task.job, delay_bin(d)] += 1

    for t in range(T):
        # arrivals
        for j in range(J):
            for _ in range(int(arrivals[t, j])):
                task = _Task(j, t)
                tr_arr[t] += 1
                in_network += 1
                enqueue(task, t)
                if task.done_at >= 0:           # zero-length leg sequence
                    in_network -= 1
                    tr_dep[t] += 1
        # link service with contention sharing
        busy = np.array([1 if q else 0 for q in link_q], dtype=np.int64)
        nb_busy = np.zeros(E)
        np.add.at(nb_busy, rows, busy[conf_indices])
        if stats and t >= warmup:
            for r, q in enumerate(link_q + node_q):
                if q:
                    qlen_sum[r] += len(q)
                    qlen_max[r] = max(qlen_max[r], len(q))
                    busy_slots[r] += 1
                    if r < E:
                        nb_sum[r] += int(nb_busy[r])
        if mwis:
            w = np.array([np.float64(len(q)) * np.float64(link_rates[l])
                          for l, q in enumerate(link_q)], dtype=np.float64)
            on, r = mwis_schedule(conf_indptr, conf_indices, w)
            rounds_max = max(rounds_max, r)
            if t >= warmup:
                sched_slots += on
        finished = []
        for l in range(E):
            if not link_q[l]:
                continue
            if mwis:
                if not on[l]:
                    continue
                cap = link_rates[l]
            else:
                cap = link_rates[l] / (1.0 + nb_busy[l])
            while cap > 0 and link_q[l]:
                head = link_q[l][0]
                served = min(cap, head.remaining)
                head.remaining -= served
                cap -= served
                if head.remaining <= 1e-12:
                    link_q[l].pop(0)
                    head.stage += 1
                    finished.append(head)
                else:
                    break
        for n in range(N):
            if not node_q[n]:
                continue
            cap = proc_bws[n]
            while cap > 0 and node_q[n]:
                head = node_q[n][0]
                served = min(cap, head.remaining)
                head.remaining -= served
                cap -= served
                if head.remaining <= 1e-12:
                    node_q[n].pop(0)
                    head.stage += 1
                    finished.append(head)
                else:
                    break
        for task in finished:
            enqueue(task, t + 1)
            if task.done_at >= 0:
                in_network -= 1
                tr_dep[min(t + 1, T - 1)] += 1
        tr_net[t] = in_network

    out = (delay_sum, count)
    if trace:
        out += ({"arrivals": tr_arr, "departures": tr_dep,
                 "pkts_in_network": tr_net},)
    if stats:
        stuck = np.zeros(J, dtype=np.int32)
        stuck_age = np.zeros(J, dtype=np.int64)
        for q in link_q + node_q:
            for task in q:
                if task.t0 >= warmup:
                    stuck[task.job] += 1
                    stuck_age[task.job] += T - task.t0
        out += ({"delay_max": delay_max, "late": late,
                 "delay_hist": delay_hist, "stuck": stuck,
                 "stuck_age": stuck_age, "qlen_sum": qlen_sum,
                 "qlen_max": qlen_max, "busy_slots": busy_slots,
                 "nb_sum": nb_sum},)
    if mwis:
        out += ({"sched_slots": sched_slots, "rounds_max": int(rounds_max)},)
    return out


def simulate(g: CaseGraph, jobs: JobInstance, flows: List[Flow],
             T: int = 2000, seed: int = 0, warmup: int = 0,
             trace: bool = False, arrivals=None, mac: str = "share"):
    """Returns (mean_delay_per_job (J,), completed_counts (J,)); with
    ``trace=True`` also a dict of per-slot totals (arrivals, sink
    departures, packets in network — the reference ``plot_metrics``
    series, offloading_v3.py:588-607).  ``arrivals`` ((T, J) counts)
    replaces the seeded Poisson draws; ``draw_arrivals(jobs, T, seed)`` is
    the stream ``seed`` alone would give.  ``mac`` is passed through to
    ``simulate_routes``; the schedule dict of ``mac="mwis"`` is dropped."""
    J = jobs.num_jobs
    if arrivals is None:
        arrivals = draw_arrivals(jobs, T, seed)
    arrivals = np.asarray(arrivals)
    assert arrivals.shape == (T, J), (arrivals.shape, (T, J))

    env = AdhocCloudEnv(g)
    routes = [env.route_links(f) if f.src != f.dst else np.empty(0, int)
              for f in flows]
    nhop = np.array([len(r) for r in routes], dtype=np.int64)
    route_links = -np.ones((J, max(int(nhop.max()) if J else 0, 1)),
                           dtype=np.int64)
    for j, r in enumerate(routes):
        route_links[j, :len(r)] = r
    dst = np.array([f.dst for f in flows], dtype=np.int64)

    out = simulate_routes(g, jobs.ul, jobs.dl, dst, route_links, nhop,
                          arrivals, warmup=warmup, trace=trace, mac=mac)
    delay_sum, count = out[0], out[1]
    with np.errstate(invalid="ignore", divide="ignore"):
        mean_delay = np.where(count > 0, delay_sum / np.maximum(count, 1),
                              np.nan)
    if trace:
        return mean_delay, count, out[2]
    return mean_delay, count


def dump_case(path, g, ul, dl, dst, route_links, nhop, arrivals,
              warmup: int = 0, mac: int = 0):
    """Flat binary dump of one ``simulate_routes`` case for the stand-alone
    host program (tests/host/timeslot_host.cpp): nine int32 header words
    ``E N J H T warmup P nconf mac`` (``mac`` 0: share, 1: mwis, read by
    tests/host/timeslot_mwis_host.cpp), then conf_indptr (E+1) int32,
    conf_indices int32, link_rates (E) fp32, proc_bws (N) fp32, arrivals
    (T,J) uint8, slot_off (T+1) int32, route_links (J,H) int32, nhop (J)
    int32, dst (J) int64, ul (J) fp32, dl (J) fp32.  The rates are rounded
    to fp32, as the kernel holds them."""
    arrivals = np.asarray(arrivals)
    T, J = arrivals.shape
    assert arrivals.min(initial=0) >= 0 and arrivals.max(initial=0) <= 255
    E, N = int(g.num_links), int(g.num_nodes)
    rl = np.asarray(route_links, dtype=np.int32).reshape(J, -1)
    if rl.shape[1] == 0:
        rl = -np.ones((J, 1), dtype=np.int32)
    slot_off = np.zeros(T + 1, dtype=np.int32)
    slot_off[1:] = np.cumsum(arrivals.sum(axis=1))
    cip = np.asarray(g.conf_indptr, dtype=np.int32)[:E + 1]
    cols = np.asarray(g.conf_indices, dtype=np.int32)[:cip[-1]]
    head = np.array([E, N, J, rl.shape[1], T, warmup, max(int(slot_off[-1]), 1),
                     len(cols), int(mac)], dtype=np.int32)
    with open(path, "wb") as f:
        for a in (head, cip, cols,
                  np.asarray(g.link_rates, dtype=np.float32)[:E],
                  np.asarray(g.proc_bws, dtype=np.float32)[:N],
                  arrivals.astype(np.uint8), slot_off, rl,
                  np.asarray(nhop, dtype=np.int32),
                  np.asarray(dst, dtype=np.int64),
                  np.asarray(ul, dtype=np.float32),
                  np.asarray(dl, dtype=np.float32)):
            f.write(np.ascontiguousarray(a).tobytes())
