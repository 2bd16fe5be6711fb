"""Device dispatch for the compute kernels.

CPU tensors → pure-torch reference implementations (``torch_ref``).
GPU tensors → the gfx950 HIP extension (``ops/hip``), which is REQUIRED on
GPU: a missing extension raises instead of silently falling back to eager
torch, so GPU runs always exercise the native kernels.
"""

from __future__ import annotations

import os

import torch

from . import torch_ref

_HIP_EXT = None
_HIP_TRIED = False


def _load_hip():
    global _HIP_EXT, _HIP_TRIED
    if _HIP_TRIED:
        return _HIP_EXT
    _HIP_TRIED = True
    try:
        from . import hip_loader
        _HIP_EXT = hip_loader.load()
    except Exception:
        _HIP_EXT = None
    return _HIP_EXT


def hip_available() -> bool:
    return _load_hip() is not None


def require_hip():
    ext = _load_hip()
    if ext is None:
        raise RuntimeError(
            "multihop_offload_amd HIP extension not built — run "
            "`python setup.py build_ext --inplace` (gfx950). GPU execution "
            "without the native kernels is disabled by design.")
    return ext


_require_hip = require_hip


def floyd_warshall(w: torch.Tensor, n_arr=None) -> torch.Tensor:
    """Batched min-plus APSP.  ``n_arr`` (optional (B,) int32): per-graph
    effective node count for inert-padded batches — the kernel relaxes
    only the leading n×n submatrix (pad rows are +inf already)."""
    if w.is_cuda and os.environ.get("MHO_FORCE_TORCH") != "1":
        ext = _require_hip()
        return ext.floyd_warshall(w.contiguous(), n_arr)
    return torch_ref.floyd_warshall(w)


def fw_force_inplace(on: bool) -> None:
    """Make every later Floyd–Warshall launch take the in-place LDS kernel
    instead of the register-resident one that serves fp32 up to N = 128
    (``False`` restores the choice by shape).  A host-side switch for
    before/after timings and the register-vs-in-place tests; the results are
    bit-equal either way."""
    _require_hip().fw_force_inplace(bool(on))


def queue_csr_force_global(on: bool) -> None:
    """Make every later launch of the queueing kernels (critic, actor head,
    walk_eval) and of the scheduled-MAC simulator (``timeslot_sim(mac=
    "mwis")``) read the conflict CSR from global memory instead of staging
    it in LDS (``False`` restores the per-workgroup decision).  A host-side
    switch for before/after timings and the staged-vs-global tests; the
    results are bit-equal either way."""
    _require_hip().queue_csr_force_global(bool(on))


def cheb_force_full_width(on: bool) -> None:
    """Make every later forward of the K<=2 LDS-resident ChebConv kernels
    (``ChebStackFn``, ``cheb_fwd_edge``) take the full-width path, which
    pads the first and the last layer to 32 columns, instead of the
    edge-layer path that serves a real output width of 1 (``False`` restores
    the choice by width).  A host-side switch for before/after timings, the
    edge-layer tests and bisecting; the backward follows its forward.
    ``lam`` is bit-equal either way, the gradients agree to rounding."""
    _require_hip().cheb_force_full_width(bool(on))


def adam_force_single_block(on: bool) -> None:
    """Make every later ``fused_adam`` launch take the single-workgroup
    kernel instead of the one-workgroup-per-tensor kernel (``False``
    restores it).  A host-side switch for before/after timings and the
    blocks-vs-single-block tests; the results are bit-equal either way."""
    _require_hip().adam_force_single_block(bool(on))


def cheb_lds_plan(Ee: int, K: int, max_nnz: int) -> dict:
    """LDS plans of the LDS-resident ChebConv launchers for graphs of Ee
    extended links, order K and at most ``max_nnz`` support entries: for each
    of ``fwd``, ``bwd`` (the K<=2 kernels, plain and edge) and ``kn_fwd``,
    ``kn_bwd`` (generic K) a dict of ``rows_pad``, ``lds_bytes``,
    ``stage_csr`` (1: the support CSR is copied into LDS, 0: read from
    global memory) and ``fits`` — the launcher's own plan, nothing is
    launched."""
    plan = _require_hip().cheb_lds_plan(int(Ee), int(K), int(max_nnz))
    return {k: dict(v) for k, v in plan.items()}


# the statistics of timeslot_sim(stats=True), in the extension's order
STAT_KEYS = ("delay_max", "late", "delay_hist", "stuck", "stuck_age",
             "qlen_sum", "qlen_max", "busy_slots", "nb_sum")
_STAT_I64 = ("stuck_age", "qlen_sum", "nb_sum")
_STAT_PER_JOB = STAT_KEYS[:5]


def empty_stats(B: int, J: int, R: int, NB: int) -> dict:
    """Zeroed CPU statistics tensors of a (B, J) batch with R = E + N
    resource columns and NB histogram bins, in the kernel's dtypes."""
    out = {}
    for k in STAT_KEYS:
        shape = (B, J, NB) if k == "delay_hist" else \
            (B, J) if k in _STAT_PER_JOB else (B, R)
        out[k] = torch.zeros(shape, dtype=torch.int64 if k in _STAT_I64
                             else torch.int32)
    return out


def fill_stats(st: dict, b: int, one: dict, idx, Eb: int, E: int) -> None:
    """Place one ``simulate_routes(stats=True)`` dict into row b: its jobs
    at the job slots ``idx``, its Eb links at columns [0, Eb) and its nodes
    from column E on."""
    for k in STAT_KEYS:
        v = torch.as_tensor(one[k])
        if k in _STAT_PER_JOB:
            st[k][b, idx] = v
        else:
            st[k][b, :Eb] = v[:Eb]
            st[k][b, E:E + len(v) - Eb] = v[Eb:]


def timeslot_lds_plan(N: int, E: int, J: int) -> dict:
    """LDS plan of the timeslot simulator kernel for a batch of N nodes, at
    most E links and J job slots: ``lds_bytes``, ``threads``, ``large``,
    ``fits`` — the launcher's own plan."""
    return dict(_require_hip().timeslot_lds_plan(int(N), int(E), int(J)))


def timeslot_stats_lds_plan(N: int, E: int, J: int) -> dict:
    """LDS plan of the simulator's statistics launch
    (``timeslot_sim(stats=True)``): the base plan's regions, then the live
    queue lengths and the per-resource accumulators."""
    return dict(_require_hip().timeslot_stats_lds_plan(int(N), int(E),
                                                       int(J)))


def timeslot_mwis_lds_plan(N: int, E: int, J: int,
                           stats: bool = False) -> dict:
    """LDS plan of the simulator's scheduled-MAC launch
    (``timeslot_sim(mac="mwis")``, with ``stats`` its statistics
    counterpart): the regions of the plan it extends, then the schedule's
    state, verdict and count words and the fp64 weights."""
    return dict(_require_hip().timeslot_mwis_lds_plan(int(N), int(E), int(J),
                                                      bool(stats)))


MAC_MODES = ("share", "mwis")


def timeslot_sim(arrivals, route_links, nhop, dst, mask, ul, dl, link_rates,
                 proc_bws, conf_indptr, conf_base, conf_cols, E_arr, n_arr,
                 T_arr=None, warmup: int = 0, trace: bool = False,
                 stats: bool = False, late_after=None, mac: str = "share"):
    """Batched per-timeslot packet simulation of ``sim.timeslot``.

    ``arrivals`` (B,T,J) integer counts (at most 255 each; masked job slots
    are ignored), routes as the episode kernels return them
    (``route_links`` (B,J,H) padded -1, ``nhop``, ``dst``), the job payloads
    and the engine's batch tables.  Returns ``(delay_sum int64 (B,J), count
    int32 (B,J), trace int32 (B,T,3) or None)`` with the trace columns
    (arrivals, departures, tasks in network).  GPU tensors run the HIP
    kernel (required — no eager fallback); CPU tensors loop over
    ``simulate_routes``.

    ``stats=True`` returns a 4-tuple whose last element is a dict of the
    integer statistics of ``sim.timeslot.simulate_routes(stats=True)``
    (``STAT_KEYS``): the per-job ones (B,J) (``delay_hist`` (B,J,NB)), the
    per-resource ones (B,E+N) with link l at column l and node v at column
    E + v, E the batch-maximum link count; masked job slots and padded
    links and nodes are zero.  ``late_after`` is an int32 (B,) tensor or an
    int (default ``T``: no sojourn is late).

    ``mac="mwis"`` runs the scheduled MAC of ``simulate_routes(mac="mwis")``
    (a queue-weighted greedy independent set of the conflict graph serves
    each slot at full rate) and appends ``sched_slots`` int32 (B,E) to the
    returned tuple, zero on padded links.  Any other value but ``"share"``
    raises ``ValueError``."""
    if mac not in MAC_MODES:
        raise ValueError(f"timeslot_sim: mac must be one of {MAC_MODES}, "
                         f"not {mac!r}")
    mwis = mac == "mwis"
    B, T, J = arrivals.shape
    if arrivals.numel() and (int(arrivals.max()) > 255
                             or int(arrivals.min()) < 0):
        raise ValueError("timeslot_sim: arrival counts must lie in [0, 255]")
    mask = mask.to(torch.bool)
    arr = torch.where(mask[:, None, :], arrivals,
                      torch.zeros_like(arrivals)).to(torch.uint8).contiguous()
    if route_links.shape[2] == 0:
        route_links = route_links.new_full((B, J, 1), -1)
    warmup = int(warmup)
    if warmup < 0:
        raise ValueError("timeslot_sim: warmup must be non-negative")

    if stats:
        if late_after is None:
            late_after = T
        if not torch.is_tensor(late_after):
            late_after = torch.full((B,), int(late_after), dtype=torch.int32)
        late_after = late_after.to(device=arr.device, dtype=torch.int32) \
            .reshape(B).contiguous()

    if arr.is_cuda:
        ext = _require_hip()
        slot_off = torch.zeros(B, T + 1, dtype=torch.int32, device=arr.device)
        slot_off[:, 1:] = arr.sum(2, dtype=torch.int64).cumsum(1)
        pool = int(slot_off[:, -1].max()) if B else 0
        if T_arr is None:
            T_arr = torch.zeros(B, dtype=torch.float32, device=arr.device)
        args = (
            arr, slot_off, route_links.to(torch.int32).contiguous(),
            nhop.to(torch.int32).contiguous(),
            dst.to(torch.int64).contiguous(), mask.contiguous(),
            ul.to(torch.float32).contiguous(),
            dl.to(torch.float32).contiguous(), conf_indptr, conf_base,
            conf_cols, link_rates.to(torch.float32).contiguous(),
            proc_bws.to(torch.float32).contiguous(),
            T_arr.to(torch.float32).contiguous(), E_arr, n_arr, warmup,
            pool, bool(trace))
        if stats:
            from ..sim.timeslot import num_delay_bins
            fn = ext.timeslot_sim_mwis_stats if mwis \
                else ext.timeslot_sim_stats
            out = fn(*args, late_after, num_delay_bins(T))
        else:
            out = (ext.timeslot_sim_mwis if mwis else ext.timeslot_sim)(*args)
        delay_sum, count, error, tr = out[:4]
        if bool(error.any()):
            bad = torch.nonzero(error).flatten().tolist()
            raise RuntimeError(
                "timeslot_sim: guard rail tripped (input out of range, pool "
                f"or loop bound) in graphs {bad[:8]}, bits "
                f"{error[bad[:8]].tolist()}")
        ret = (delay_sum, count, (tr if trace else None))
        if stats:
            ret += (dict(zip(STAT_KEYS, out[4:4 + len(STAT_KEYS)])),)
        if mwis:
            ret += (out[-1],)
        return ret

    from types import SimpleNamespace

    import numpy as np

    from ..sim.timeslot import num_delay_bins, simulate_routes
    delay_sum = torch.zeros(B, J, dtype=torch.int64)
    count = torch.zeros(B, J, dtype=torch.int32)
    tr = torch.zeros(B, T, 3, dtype=torch.int32) if trace else None
    cip = conf_indptr.numpy()
    cols = conf_cols.numpy()
    N = proc_bws.shape[1]
    E = link_rates.shape[1]
    st = empty_stats(B, J, E + N, num_delay_bins(T)) if stats else None
    sched = torch.zeros(B, E, dtype=torch.int32) if mwis else None
    for b in range(B):
        Eb = int(E_arr[b])
        lo = int(conf_base[b])
        g = SimpleNamespace(
            num_links=Eb, num_nodes=N, conf_indptr=cip[b, :Eb + 1],
            conf_indices=cols[lo:lo + int(cip[b, Eb])],
            link_rates=link_rates[b, :Eb].numpy().astype(np.float64),
            proc_bws=proc_bws[b].numpy().astype(np.float64))
        idx = torch.nonzero(mask[b]).flatten()
        out = simulate_routes(
            g, ul[b, idx].numpy().astype(np.float64),
            dl[b, idx].numpy().astype(np.float64), dst[b, idx].numpy(),
            route_links[b, idx].numpy(), nhop[b, idx].numpy(),
            arr[b][:, idx].numpy(), warmup=warmup, trace=trace,
            stats=stats, late_after=int(late_after[b]) if stats else None,
            mac=mac)
        if mwis:
            sched[b, :Eb] = torch.as_tensor(out[-1]["sched_slots"])
            out = out[:-1]
        if stats:
            fill_stats(st, b, out[-1], idx, Eb, E)
        delay_sum[b, idx] = torch.as_tensor(out[0])
        count[b, idx] = torch.as_tensor(out[1]).to(torch.int32)
        if trace:
            for k, name in enumerate(("arrivals", "departures",
                                      "pkts_in_network")):
                tr[b, :, k] = torch.as_tensor(out[2][name]).to(torch.int32)
    ret = (delay_sum, count, tr)
    if stats:
        ret += (st,)
    if mwis:
        ret += (sched,)
    return ret
