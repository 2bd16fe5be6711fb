"""Batched device-resident episode engine.

The reference processes one graph × one job instance at a time, with Python
loops over jobs/links and CPU Dijkstra between two TF segments
(SURVEY.md §3.1).  This engine runs **B (graph, jobs) instances as one tensor
program** — features → ChebConv → contention fixed point → delay matrices →
batched min-plus APSP → decision/greedy-routing walk → analytic evaluation →
critic → semi-analytic backward — with zero host round-trips inside a step.
On MI355X the hot stages dispatch to HIP kernels (ops/); the same code runs
on CPU (fp64) where it is tested for exact agreement with the oracle
``AdhocCloudEnv``/``ACOAgent`` path.

Batching layout:
  * per-graph dense tensors are stacked: (B, N, N) / (B, E) / (B, Ē);
    all graphs in a batch share N; link counts MAY differ (ragged E — E is
    the batch max, per-graph counts in E_arr, virtual extended edges
    renumbered to start at E); conflict structure is flat block-diagonal
    CSR over B·E (resp. B·Ē); horizons T may differ per graph;
  * job instances are padded to Jmax with a validity mask; padded jobs have
    zero rate and are excluded from routes, losses and metrics;
  * the per-instance actor gradient sets of the reference's replay memory
    (gnn_offloading_agent.py:156-169) become one fused VJP: instances are
    independent blocks, so the batched cotangent yields the SUM of the
    per-instance gradients in a single backward pass.
"""

from __future__ import annotations

import dataclasses
from typing import Optional, Sequence

import numpy as np
import torch

from .graphs import CaseGraph
from .models.chebconv import ChebConvStack
from .queueing import ConflictCSR, delay_with_fallback, fixed_point_mu
from .ops import dispatch as ops


@dataclasses.dataclass
class JobBatch:
    """Padded per-graph job instances on device (the batched analog of
    ``JobInstance``); padded slots are masked out of every reduction."""
    sources: torch.Tensor   # (B, J) int64, padded with a valid mobile node
    mask: torch.Tensor      # (B, J) bool — real jobs
    rates: torch.Tensor     # (B, J)
    ul: torch.Tensor        # (B, J)
    dl: torch.Tensor        # (B, J)

    @property
    def num_real(self):
        return self.mask.sum()


@dataclasses.dataclass
class EpisodeResult:
    """Per-graph episode outcome (training losses populated when
    ``train=True``)."""
    tau: torch.Tensor            # (B,) mean per-job empirical delay
    congest: torch.Tensor        # (B,) number of congested jobs
    num_jobs: torch.Tensor       # (B,)
    delay_emp: torch.Tensor      # (B, J) per-job empirical delay (nan-padded)
    loss_fn: Optional[torch.Tensor] = None      # 0-dim, on device
    loss_mse: Optional[torch.Tensor] = None
    # the episode's decisions and routes (what ``simulate`` replays)
    dst: Optional[torch.Tensor] = None          # (B, J) computing node
    route_links: Optional[torch.Tensor] = None  # (B, J, H) link ids, -1 pad
    nhop: Optional[torch.Tensor] = None         # (B, J)


def hist_percentile(hist: torch.Tensor, dmax: torch.Tensor,
                    q: float) -> torch.Tensor:
    """Upper bound on the q-quantile of the sojourns behind a delay
    histogram (``sim.timeslot.delay_bin`` bins along the last dimension):
    the upper edge of the first bin whose cumulative count reaches
    ``max(1, ceil(q * total))``, capped at the largest sojourn ``dmax``;
    nan where the histogram is empty.  Exact below 16 slots, at most 12.5 %
    over above."""
    from .sim.timeslot import delay_bin_upper
    hist = hist.to(torch.int64)
    total = hist.sum(-1)
    need = torch.ceil(q * total.to(torch.float64)).to(torch.int64) \
        .clamp(min=1)
    k = (hist.cumsum(-1) >= need[..., None]).to(torch.int8).argmax(-1)
    edges = torch.tensor([delay_bin_upper(i) for i in range(hist.shape[-1])],
                         dtype=torch.int64, device=hist.device)
    got = torch.minimum(edges[k], dmax.to(torch.int64)).to(torch.float64)
    return torch.where(total > 0, got, torch.full_like(got, float("nan")))


@dataclasses.dataclass
class SimStats:
    """Integer statistics of one ``EpisodeEngine.simulate(stats=True)`` run
    (definitions: ``sim.timeslot.simulate_routes``).  Per-resource tensors
    are (B, E + N): link l at column l, node v at column E + v."""
    delay_max: torch.Tensor      # (B, J) int32
    late: torch.Tensor           # (B, J) int32, sojourn > late_after
    delay_hist: torch.Tensor     # (B, J, NB) int32
    stuck: torch.Tensor          # (B, J) int32, == SimResult.backlog
    stuck_age: torch.Tensor      # (B, J) int64
    qlen_sum: torch.Tensor       # (B, E + N) int64
    qlen_max: torch.Tensor       # (B, E + N) int32
    busy_slots: torch.Tensor     # (B, E + N) int32
    nb_sum: torch.Tensor         # (B, E + N) int64, zero on nodes
    delay_sum: torch.Tensor      # (B, J) int64, as in SimResult
    count: torch.Tensor          # (B, J) int32, as in SimResult
    late_after: torch.Tensor     # (B,) int32
    num_links: int               # E, the column of node 0
    T_sim: int
    warmup: int

    def _scope(self, x: torch.Tensor, per: str, how: str = "sum"):
        """Reduce a (B, J, ...) per-job tensor over the scope ``per``."""
        if per == "job":
            return x
        if per not in ("graph", "all"):
            raise ValueError("per: 'graph', 'job' or 'all'")
        dims = (1,) if per == "graph" else (0, 1)
        return x.amax(dims) if how == "max" else x.sum(dims)

    @staticmethod
    def _ratio(num, den):
        num, den = num.to(torch.float64), den.to(torch.float64)
        return torch.where(den > 0, num / den.clamp(min=1),
                           torch.full_like(den, float("nan")))

    def percentile(self, q: float, per: str = "graph") -> torch.Tensor:
        """Upper bound on the q-quantile (q in [0, 1]) of the counted
        sojourns, histograms merged over the scope (``hist_percentile``)."""
        return hist_percentile(
            self._scope(self.delay_hist.to(torch.int64), per),
            self._scope(self.delay_max, per, "max"), q)

    def late_ratio(self, per: str = "graph") -> torch.Tensor:
        """Share of the counted tasks later than ``late_after``."""
        return self._ratio(self._scope(self.late.to(torch.int64), per),
                           self._scope(self.count.to(torch.int64), per))

    def censored_mean_delay(self, per: str = "graph") -> torch.Tensor:
        """``(delay_sum + stuck_age) / (count + stuck)``: a lower bound on
        the mean sojourn that does not drop the tasks still in the
        network."""
        return self._ratio(
            self._scope(self.delay_sum + self.stuck_age, per),
            self._scope((self.count + self.stuck).to(torch.int64), per))

    def utilization(self) -> torch.Tensor:
        """(B, E + N) share of the sampled slots with a non-empty FIFO."""
        return self.busy_slots.to(torch.float64) \
            / max(self.T_sim - self.warmup, 1)

    def mean_qlen(self) -> torch.Tensor:
        """(B, E + N) mean FIFO length over the sampled slots."""
        return self.qlen_sum.to(torch.float64) \
            / max(self.T_sim - self.warmup, 1)

    def mean_contention(self) -> torch.Tensor:
        """(B, E) mean number of busy conflicting links a link saw in its
        own busy slots — the simulated ``sum busy`` of the fixed point's
        ``rate / (1 + sum busy)``; nan where the link was never busy."""
        E = self.num_links
        return self._ratio(self.nb_sum[:, :E], self.busy_slots[:, :E])


@dataclasses.dataclass
class SimResult:
    """Per-job outcome of the per-timeslot packet simulation of an episode's
    routes (``EpisodeEngine.simulate``)."""
    delay_sum: torch.Tensor      # (B, J) int64, slots over completed tasks
    count: torch.Tensor          # (B, J) completed tasks with t0 >= warmup
    mean_delay: torch.Tensor     # (B, J) delay_sum / count, nan where 0
    backlog: torch.Tensor        # (B, J) arrived after warmup, not completed
    trace: Optional[torch.Tensor] = None   # (B, T, 3) arrivals, departures,
    #                                        tasks in network per slot
    stats: Optional[SimStats] = None       # with simulate(stats=True)
    sched_slots: Optional[torch.Tensor] = None   # (B, E) int32 slots t >=
    #                  warmup a link was scheduled in, with simulate(mac="mwis")

    def sched_share(self) -> torch.Tensor:
        """(B, E) float64 share of a link's busy slots in which it was
        scheduled (``mac="mwis"`` with ``stats=True``); nan where the link
        was never busy."""
        if self.sched_slots is None or self.stats is None:
            raise ValueError("sched_share: needs simulate(stats=True, "
                             "mac='mwis')")
        E = self.sched_slots.shape[1]
        return SimStats._ratio(self.sched_slots,
                               self.stats.busy_slots[:, :E])


class EpisodeEngine:
    """Device-resident batched episode engine — the MI355X product path.

    Holds a batch of (same-N, ragged-E, per-graph-T) cases as flat
    block-diagonal CSRs plus the index tables every step needs, and runs
    full GNN/baseline/local episodes in a handful of fused HIP kernel
    launches (torch fp64 composition on CPU, proven equal to the numpy
    oracle in tests/test_engine.py).  Reference analogs:
    ``offloading_v3.AdhocCloud`` decisions/evaluation +
    ``gnn_offloading_agent.ACOAgent`` forward/backward, batched.
    Mixed sizes: one engine per size, or ``CaseGraph.pad_to``.
    """

    def __init__(self, cases: Sequence[CaseGraph], model: ChebConvStack,
                 device: str = "cpu", dtype: torch.dtype = torch.float32,
                 fp_iters: int = 10, walk_cap: Optional[int] = None,
                 delay_clamp: float = 0.0, lam_margin: float = 0.0,
                 native_glue: bool = True):
        assert len(cases) > 0
        N = cases[0].num_nodes
        T = cases[0].T
        assert all(c.num_nodes == N for c in cases), "batch shares N"
        # link counts are RAGGED (e.g. distinct ER topologies): E = max,
        # per-graph E_b in E_arr; padded link slots [E_b, E) are isolated
        # (rate 1, no conflicts, excluded from every edge-indexed scatter).
        # Extended-edge ids are renumbered so the virtual (self-loop) edges
        # of every graph start at E: id < E_b keeps, virtual -> E + rank.
        E = max(c.num_links for c in cases)
        self.cases = list(cases)
        self.B, self.N, self.E, self.T = len(cases), N, E, T
        self.E_list = [c.num_links for c in cases]
        self.device = torch.device(device)
        self.dtype = dtype
        self.fp_iters = fp_iters
        # pole mitigation for training: clamp the 1/(mu-lam) delay branch
        # at this value (0 = off, reference semantics) — see queueing.py
        self.delay_clamp = float(delay_clamp)
        # inference-time conservatism: the decision stage sees predicted
        # traffic inflated by (1+lam_margin) — a calibratable knob that
        # biases marginal offloads toward local compute (congestion-tail
        # control without retraining); 0 = reference behavior
        self.lam_margin = float(lam_margin)
        self.model = model.to(self.device)
        self.walk_cap = walk_cap or N

        Cmax = max(len(c.ext.comp_nodes) for c in cases)
        Ee = E + Cmax
        self.Ee = Ee
        B = self.B

        def t(a, dt=None):
            return torch.as_tensor(np.asarray(a), dtype=dt or dtype,
                                   device=self.device)

        def ti(a):
            return torch.as_tensor(np.asarray(a), dtype=torch.int64,
                                   device=self.device)

        def pad_rows(arrs, width, fill, dt=np.float64):
            out = np.full((B, width), fill, dtype=dt)
            for b, a in enumerate(arrs):
                out[b, :len(a)] = a
            return out

        edges_np = np.zeros((B, E, 2), dtype=np.int64)
        for b, c in enumerate(cases):
            edges_np[b, :c.num_links] = c.edges
        self.edges = ti(edges_np)                              # (B,E,2) pad 0
        self.link_rates = t(pad_rows([c.link_rates for c in cases], E, 1.0))
        self.cf_degs = t(pad_rows([c.cf_degs for c in cases], E, 0.0))
        self.proc_bws = t([c.proc_bws for c in cases])         # (B,N)
        self.roles = ti([c.roles for c in cases])
        self.adj = torch.as_tensor(
            np.stack([c.adj for c in cases]) != 0, device=self.device)
        self.link_matrix = ti([c.link_matrix for c in cases])  # (B,N,N)
        # virtual-edge ids under the ragged renumbering: E + rank
        nv = -np.ones((B, N), dtype=np.int64)
        for b, c in enumerate(cases):
            v = c.ext.node_vedge
            nv[b] = np.where(v >= 0, v - c.num_links + E, -1)
        self.node_vedge = ti(nv)                               # (B,N)
        self.comp_mask = self.roles < 2                        # (B,N)
        self.sp_hop = t([c.sp_hop for c in cases])             # (B,N,N)
        # valid-link selection tables (static): flat (B*E) indices of real
        # links and their (B*N*N) scatter positions
        lm = np.zeros((B, E), dtype=bool)
        for b, c in enumerate(cases):
            lm[b, :c.num_links] = True
        self.link_mask = torch.as_tensor(lm, device=self.device)
        sel_b, sel_e = np.nonzero(lm)
        self._lk_sel = ti(sel_b * E + sel_e)
        e0v = edges_np[sel_b, sel_e, 0]
        e1v = edges_np[sel_b, sel_e, 1]
        self._lk_lin01 = ti(sel_b * (N * N) + e0v * N + e1v)
        self._lk_lin10 = ti(sel_b * (N * N) + e1v * N + e0v)

        # servers, padded
        S = max(len(c.servers) for c in cases)
        srv = -np.ones((B, S), dtype=np.int64)
        for b, c in enumerate(cases):
            srv[b, :len(c.servers)] = c.servers
        self.S = S
        self.servers = ti(srv)
        self.server_mask = self.servers >= 0
        self.servers_safe = self.servers.clamp(min=0)

        # mobiles
        mob_counts = [len(c.mobile_nodes) for c in cases]
        assert min(mob_counts) >= 1, \
            "every case needs at least one mobile node (job sources)"
        self.Jmax = max(mob_counts) - 1 if max(mob_counts) > 1 else 1
        self.mobile_mask = self.roles == 0

        # flat block-diagonal conflict CSR over B·E (original line graph);
        # padded link rows are absent (no conflicts)
        rows, cols = [], []
        for b, c in enumerate(cases):
            r = np.repeat(np.arange(c.num_links),
                          np.diff(c.conf_indptr)) + b * E
            rows.append(r)
            cols.append(c.conf_indices + b * E)
        self.conf = ConflictCSR.__new__(ConflictCSR)
        self.conf.row = ti(np.concatenate(rows))
        self.conf.col = ti(np.concatenate(cols))
        self.conf.n = B * E

        # flat block-diagonal extended line-graph CSR over B·Ē (GNN
        # support), ids remapped (virtual edges at E + rank)
        def remap(ids, Eb):
            ids = np.asarray(ids)
            return np.where(ids < Eb, ids, ids - Eb + E)

        rows, cols = [], []
        for b, c in enumerate(cases):
            ext = c.ext
            Eb = c.num_links
            ne = ext.num_edges_ext
            r = remap(np.repeat(np.arange(ne), np.diff(ext.ext_indptr)),
                      Eb) + b * Ee
            rows.append(r)
            cols.append(remap(ext.ext_indices, Eb) + b * Ee)
        self.support = ConflictCSR.__new__(ConflictCSR)
        self.support.row = ti(np.concatenate(rows))
        self.support.col = ti(np.concatenate(cols))
        self.support.n = B * Ee

        # static feature columns (B,Ē) under the renumbering: real links at
        # [0,Eb), padded link slots isolated, virtual edges at [E, E+Cb)
        def feat(attr, link_fill, tail_fill):
            out = np.full((B, Ee), tail_fill, dtype=np.float64)
            for b, c in enumerate(cases):
                v = getattr(c.ext, attr)
                Eb = c.num_links
                out[b, :Eb] = v[:Eb]
                out[b, Eb:E] = link_fill
                out[b, E:E + len(v) - Eb] = v[Eb:]
            return t(out)

        for c in cases:
            c.ext.refresh_rates()
        self.f_self_loop = feat("edge_self_loop", 0.0, 1.0)
        self.f_as_server = feat("edge_as_server", 0.0, 0.0)
        self.f_rate = feat("edge_rate_ext", 1.0, 1.0)
        # proc bws of computing nodes in extended-edge order (B, Ē-E),
        # padded with 1.0 (kept finite; padded slots never reach a scatter)
        self.Cmax = Cmax
        bw = np.ones((B, self.Cmax), dtype=np.float64)
        for b, c in enumerate(cases):
            bw[b, :len(c.ext.comp_nodes)] = c.proc_bws[c.ext.comp_nodes]
        self.bw_comp = t(bw)

        # computing-node index tables: for every (graph b, computing node n):
        # its node id, its rank in the graph's extended-edge tail
        cb, cn, cr = [], [], []
        for b, c in enumerate(cases):
            for rank, n in enumerate(c.ext.comp_nodes):
                cb.append(b)
                cn.append(int(n))
                cr.append(rank)
        self._comp_b = ti(cb)
        self._comp_n = ti(cn)
        self._comp_r = ti(cr)

        self._bidx = torch.arange(B, device=self.device)
        self._eye = torch.eye(N, dtype=torch.bool,
                              device=self.device)[None, :, :]
        # device-side exploration scalar + stateless-RNG state for the
        # in-kernel ε-greedy/softmax sampling (capture-safe: a hipGraph
        # replay reads the CURRENT explore value and a counter this engine
        # bumps with a device op each decision)
        self._explore_buf = torch.zeros((), dtype=torch.float32,
                                        device=self.device)
        self._rng_state = torch.tensor([12345, 0], dtype=torch.int64,
                                       device=self.device)
        # truncated-walk counter, accumulated on device (sync-free inner
        # loop); callers poll check_overflow() at log points — a greedy
        # walk that fails to reach its destination within walk_cap hops
        # would otherwise silently underestimate loads/delays
        self.overflow_total = torch.zeros((), dtype=torch.int64,
                                          device=self.device)
        # per-graph horizon T (BASELINE config 5: ragged batches may mix T)
        self.T_arr = t([float(c.T) for c in cases])            # (B,)
        self.T_link = self.T_arr.repeat_interleave(E)          # (B*E,)

        # ---- kernel tables (int32 CSR forms for the fused HIP kernels) ----
        def t32(a):
            return torch.as_tensor(np.asarray(a, dtype=np.int32),
                                   device=self.device)

        self.k_adj_indptr = t32([c.adj_indptr for c in cases])     # (B,N+1)

        def pad_i32(arrs, width):
            out = np.zeros((B, width), dtype=np.int32)
            for b, a in enumerate(arrs):
                out[b, :len(a)] = a
            return t32(out)

        self.k_adj_idx = pad_i32([c.adj_indices for c in cases], 2 * E)
        self.k_adj_link = pad_i32([c.adj_link_ids for c in cases], 2 * E)
        # conflict indptr padded by repeating the last value (rows E_b..E
        # are empty)
        cip = np.zeros((B, E + 1), dtype=np.int32)
        for b, c in enumerate(cases):
            Eb = c.num_links
            cip[b, :Eb + 1] = c.conf_indptr
            cip[b, Eb + 1:] = c.conf_indptr[-1]
        self.k_conf_indptr = t32(cip)
        self.k_E_arr = t32([c.num_links for c in cases])           # (B,)
        # per-graph effective node counts (pad_to batches carry inert pad
        # nodes; kernels skip them — O(n³) APSP instead of O(Nmax³))
        self.k_N_arr = t32([getattr(c, "real_n", c.num_nodes)
                            for c in cases])
        self._padded = any(getattr(c, "real_n", c.num_nodes) != N
                           for c in cases)
        cc, base = [], [0]
        for c in cases:
            cc.append(np.asarray(c.conf_indices, dtype=np.int32))
            base.append(base[-1] + len(c.conf_indices))
        self.k_conf_cols = t32(np.concatenate(cc))
        self.k_conf_base = torch.as_tensor(np.asarray(base[:-1]),
                                           dtype=torch.int64,
                                           device=self.device)
        self.k_edges = t32(edges_np)                               # (B,E,2)
        self.k_servers = t32(srv)                                  # (B,S)
        # extended line-graph CSR (ChebConv support) under the
        # renumbering: rows [E_b, E) empty, virtual rows at E + rank
        ipt = np.zeros((B, Ee + 1), dtype=np.int32)
        cc, base = [], [0]
        for b, c in enumerate(cases):
            ext = c.ext
            Eb = c.num_links
            src_ipt = ext.ext_indptr
            counts = np.zeros(Ee, dtype=np.int64)
            counts[:Eb] = np.diff(src_ipt)[:Eb]
            nv = ext.num_edges_ext - Eb
            counts[E:E + nv] = np.diff(src_ipt)[Eb:]
            ipt[b, 1:] = np.cumsum(counts)
            # column ids in row order (rows reordered the same way)
            colsrc = np.asarray(ext.ext_indices)
            link_cols = colsrc[:src_ipt[Eb]]
            virt_cols = colsrc[src_ipt[Eb]:]
            allc = np.concatenate([link_cols, virt_cols])
            allc = np.where(allc < Eb, allc, allc - Eb + E)
            cc.append(allc.astype(np.int32))
            base.append(base[-1] + len(allc))
        self.k_ext_indptr = t32(ipt)
        self.k_ext_max_nnz = int(max(int(c.ext.ext_indptr[-1])
                                     for c in cases))
        self.k_ext_cols = t32(np.concatenate(cc))
        self.k_ext_base = torch.as_tensor(np.asarray(base[:-1]),
                                          dtype=torch.int64,
                                          device=self.device)
        import os
        self.use_hip = (self.device.type == "cuda"
                        and os.environ.get("MHO_FORCE_TORCH") != "1")
        # per-kernel LDS fit, asked of the launchers' own plans (a stage
        # whose kernel does not fit even in its global-scratch mode falls
        # back to the torch tensor path; the rest stay on the fused
        # kernels).  Every use is behind `use_hip and`.
        self.hip_walk_ok = self.hip_critic_ok = self.hip_actor_ok = False
        if self.use_hip:
            assert dtype == torch.float32, "HIP kernels are fp32"
            from .ops import dispatch
            plan = dispatch.require_hip().queue_lds_plan(N, E, Ee, fp_iters)
            self.hip_walk_ok = plan["walk_eval"]["fits"]
            self.hip_critic_ok = plan["critic"]["fits"]
            self.hip_actor_ok = (plan["actor_head_fwd"]["fits"]
                                 and plan["actor_head_bwd"]["fits"])
        # the per-step glue between the episode kernels (features, parameter
        # pack / gradient reduce, APSP prep, actor cotangent, summary, job
        # sampling after the draws) as HIP kernels; False keeps the torch
        # glue around the same episode kernels (the oracle of the glue tests)
        self.native_glue = bool(native_glue) and self.use_hip

    def set_rng_seed(self, seed: int):
        """Seed the in-kernel stateless sampler (per-DP-rank seeds keep the
        ε-greedy draws independent across ranks)."""
        self._rng_state[0] = int(seed)
        self._rng_state[1] = 0

    # ------------------------------------------------------------------ jobs
    def sample_jobs(self, arrival_scale: float,
                    gen: Optional[torch.Generator] = None) -> JobBatch:
        """Device-side analog of ``JobInstance.sample``: per graph, J ~
        U{int(0.3·M), M-1} jobs on a random subset of mobiles, rates
        U(0.1,0.5)·scale, ul=100, dl=1."""
        B, N, J = self.B, self.N, self.Jmax
        dev = self.device
        scores_raw = torch.rand(B, N, device=dev, generator=gen)
        r_nj = torch.rand(B, device=dev, generator=gen)
        r_rates = torch.rand(B, J, device=dev, generator=gen)
        return self._jobs_from_draws(scores_raw, r_nj, r_rates,
                                     arrival_scale)

    def _jobs_from_draws(self, scores_raw: torch.Tensor, r_nj: torch.Tensor,
                         r_rates: torch.Tensor,
                         arrival_scale: float) -> JobBatch:
        """Everything of ``sample_jobs`` after the three uniform draws: one
        HIP launch on the native path, the torch composition otherwise (the
        two agree exactly; equal scores among mobiles — a 2^-24 event per
        pair — are ordered by node id in the kernel)."""
        J = self.Jmax
        dev = self.device
        if self.native_glue:
            sources, mask, rates, ul, dl = ops.require_hip().jobs_from_draws(
                scores_raw, r_nj, r_rates, self.mobile_mask,
                float(arrival_scale))
            return JobBatch(sources=sources, mask=mask, rates=rates, ul=ul,
                            dl=dl)
        scores = torch.where(self.mobile_mask, scores_raw,
                             torch.full_like(scores_raw, 2.0))
        order = torch.argsort(scores, dim=1)                 # mobiles first
        sources = order[:, :J]                               # (B,J)
        M = self.mobile_mask.sum(1)                          # (B,)
        lo = (0.3 * M).to(torch.int64)
        span = (M - lo).clamp(min=1)
        nj = lo + (r_nj * span.to(self.dtype)).to(torch.int64)
        nj = nj.clamp(min=1)
        mask = torch.arange(J, device=dev)[None, :] < nj[:, None]
        # clamp padded sources to a valid mobile (first sampled) for safety
        sources = torch.where(mask, sources, sources[:, :1])
        rates = (r_rates * 0.4 + 0.1) * arrival_scale
        z = torch.zeros(self.B, J, device=dev, dtype=self.dtype)
        return JobBatch(
            sources=sources,
            mask=mask,
            rates=torch.where(mask, rates.to(self.dtype), z),
            ul=torch.where(mask, torch.full_like(z, 100.0), z),
            dl=torch.where(mask, torch.full_like(z, 1.0), z),
        )

    def pack_jobs(self, instances) -> JobBatch:
        """Pack a list of per-case :class:`JobInstance` (length B, each with
        ``num_jobs <= Jmax``) into a padded device JobBatch — the bridge
        from the host-side samplers/harnesses into the engine."""
        B, J = self.B, self.Jmax
        assert len(instances) == B
        src = np.zeros((B, J), dtype=np.int64)
        mask = np.zeros((B, J), dtype=bool)
        rates = np.zeros((B, J))
        ul = np.zeros((B, J))
        dl = np.zeros((B, J))
        for b, jobs in enumerate(instances):
            k = jobs.num_jobs
            assert k <= J, (k, J)
            src[b, :k] = jobs.sources
            # pad with a node that has a virtual self-loop edge: a relay
            # (node 0 can be one) has none and would index -1 downstream
            src[b, k:] = (jobs.sources[0] if k
                          else self.cases[b].ext.comp_nodes[0])
            mask[b, :k] = True
            rates[b, :k] = jobs.rates
            ul[b, :k] = jobs.ul
            dl[b, :k] = jobs.dl
        dev, dt = self.device, self.dtype
        return JobBatch(
            sources=torch.as_tensor(src, device=dev),
            mask=torch.as_tensor(mask, device=dev),
            rates=torch.as_tensor(rates, dtype=dt, device=dev),
            ul=torch.as_tensor(ul, dtype=dt, device=dev),
            dl=torch.as_tensor(dl, dtype=dt, device=dev),
        )

    # ------------------------------------------------------- actor forward
    def _features(self, jobs: JobBatch) -> torch.Tensor:
        """x (B,Ē,4) = [self-loop, rate, job load, as-server]: the job load
        Σ rate·ul lands on the virtual edge of each job's source."""
        if self.native_glue:
            return ops.require_hip().cheb_features(
                jobs.sources, jobs.rates.contiguous(), jobs.ul.contiguous(),
                jobs.mask, self.node_vedge, self.comp_mask, self.f_self_loop,
                self.f_rate, self.f_as_server)
        B, Ee, N = self.B, self.Ee, self.N
        arr = torch.zeros(B, N, dtype=self.dtype, device=self.device)
        arr = arr.scatter_add(1, jobs.sources, jobs.rates * jobs.ul)
        f_job = torch.zeros(B, Ee, dtype=self.dtype, device=self.device)
        vidx = torch.where(self.comp_mask, self.node_vedge,
                           torch.zeros_like(self.node_vedge))
        f_job = f_job.scatter_add(
            1, vidx, torch.where(self.comp_mask, arr, torch.zeros_like(arr)))
        return torch.stack([self.f_self_loop, self.f_rate, f_job,
                            self.f_as_server], dim=-1)

    def _actor_head_tables(self):
        """The batch tables the actor-head kernels take after λ (forward)
        or after (cotangent, λ, mu_hist) (backward)."""
        return (self.k_conf_indptr, self.k_conf_base, self.k_conf_cols,
                self.link_rates.contiguous(), self.bw_comp.contiguous(),
                self.k_edges, self.node_vedge, self.T_arr.contiguous(),
                self.k_E_arr)

    def _lam_hip(self, jobs: JobBatch) -> torch.Tensor:
        """features → ChebConv → λ (B,Ē) on the HIP path (autograd graph
        kept)."""
        B, Ee = self.B, self.Ee
        x = self._features(jobs)                                  # (B,Ē,4)
        from .ops.functions import ChebStackFn, cheb_compat
        if cheb_compat(self.model):
            params = []
            for layer in self.model.layers:
                params += [layer.weight, layer.bias]
            lam = ChebStackFn.apply(x.contiguous(), self, *params)
        else:
            # no silent eager fallback on GPU: unsupported model
            # shapes refuse loudly unless explicitly overridden
            import os as _os
            if _os.environ.get("MHO_ALLOW_TORCH_GPU") != "1":
                raise RuntimeError(
                    "model shape unsupported by the fused ChebConv "
                    "kernels (feature width > 32 or dropout > 0); "
                    "refusing eager torch on GPU — set "
                    "MHO_ALLOW_TORCH_GPU=1 to override")
            return self.model(x.reshape(B * Ee, 4),
                              self.support).reshape(B, Ee)
        if self.lam_margin:
            lam = lam * (1.0 + self.lam_margin)
        return lam

    def _actor_forward_native(self, jobs: JobBatch):
        """``actor_forward`` of the native-glue episode: the head runs
        outside autograd, because its backward takes the cotangent as
        (grad_edge, unit_mtx, written) and never as a dense (B,N,N) tensor.
        Returns (dm without a graph, saved) with ``saved`` what
        ``_actor_backward_native`` needs."""
        lam = self._lam_hip(jobs)
        lam_c = lam.detach().contiguous()
        dm, mu_hist = ops.require_hip().actor_head_fwd(
            lam_c, *self._actor_head_tables(), self.N, self.fp_iters,
            self.delay_clamp)
        return dm, (lam, lam_c, mu_hist)

    def _actor_backward_native(self, saved, grad_edge, dm, unit_mtx,
                               written, critic_loss=None):
        """Actor backward of the native-glue episode: the head's VJP with
        the cotangent assembled in the kernel (``grad_dist_matrix`` fused
        into ``actor_head_bwd``), then autograd through the ChebConv stack.
        Returns loss_mse, and with ``critic_loss`` (the critic's per-graph
        loss) ``(loss_mse, loss_fn)``: its sum, taken in the kernel that
        finishes loss_mse."""
        lam, lam_c, mu_hist = saved
        out = ops.require_hip().actor_head_bwd_fused(
            grad_edge.contiguous(), dm, unit_mtx, written, lam_c, mu_hist,
            *self._actor_head_tables(), self.fp_iters, self.delay_clamp,
            critic_loss)
        lam.backward(out[0])
        return out[1] if critic_loss is None else (out[1], out[2])

    def actor_forward(self, jobs: JobBatch):
        """features → ChebConv → λ → fixed point → delays → (B,N,N) delay
        matrix (autograd graph kept).  Reference gnn_offloading_agent.py:
        211-276, batched."""
        B, E, Ee, N = self.B, self.E, self.Ee, self.N
        if self.use_hip and self.hip_actor_ok:
            from .ops.functions import ActorHeadFn
            dm = ActorHeadFn.apply(self._lam_hip(jobs), self)
            return dm, None, None

        x = self._features(jobs)                                  # (B,Ē,4)
        lam = self.model(x.reshape(B * Ee, 4), self.support).reshape(B, Ee)
        if self.lam_margin:
            lam = lam * (1.0 + self.lam_margin)

        lam_link = lam[:, :E].reshape(-1)
        mu = fixed_point_mu(lam_link, self.link_rates.reshape(-1),
                            self.cf_degs.reshape(-1), self.conf,
                            self.fp_iters)
        link_delay = delay_with_fallback(lam_link, mu, self.T_link, 101.0,
                                         self.delay_clamp).reshape(B, E)
        node_delay = delay_with_fallback(lam[:, E:], self.bw_comp,
                                         self.T_arr[:, None], 100.0,
                                         self.delay_clamp)

        dm = self._delay_matrix(link_delay, node_delay)
        return dm, link_delay, node_delay

    def _delay_matrix(self, link_delay, node_delay):
        B, N, E = self.B, self.N, self.E
        flat = torch.zeros(B * N * N, dtype=self.dtype, device=self.device)
        ld_valid = link_delay.reshape(-1)[self._lk_sel]
        flat = flat.index_put((self._lk_lin01,), ld_valid)
        flat = flat.index_put((self._lk_lin10,), ld_valid)
        # diagonal: node delays at computing nodes, +inf at relays
        diag_idx = (self._bidx[:, None] * (N * N)
                    + torch.arange(N, device=self.device)[None, :] * (N + 1))
        inf = torch.full((B, N), float("inf"), dtype=self.dtype,
                         device=self.device)
        flat = flat.index_put((diag_idx.reshape(-1),), inf.reshape(-1))
        lin = (self._comp_b * (N * N) + self._comp_n * (N + 1))
        flat = flat.index_put((lin,), node_delay[self._comp_b, self._comp_r])
        return flat.reshape(B, N, N)

    # --------------------------------------------------------------- APSP
    def apsp(self, dm: torch.Tensor) -> torch.Tensor:
        """Batched all-pairs shortest paths over the delay-weighted graphs.
        Input: (B,N,N) delay matrix (off-diagonal link delays; diagonal
        ignored).  Non-edges → +inf, diagonal → 0, then min-plus
        Floyd–Warshall (detached — the reference's Dijkstra is outside the
        tape too, gnn_offloading_agent.py:304-306)."""
        B, N = self.B, self.N
        with torch.no_grad():
            if self.native_glue:
                # mask and diagonal applied in the kernel's LDS load
                return ops.require_hip().floyd_warshall_dm(
                    dm.detach(), self.adj,
                    self.k_N_arr if self._padded else None)
            w = torch.where(self.adj, dm.detach(),
                            torch.full_like(dm, float("inf")))
            w = torch.where(self._eye, torch.zeros_like(w), w)
            return ops.floyd_warshall(
                w, self.k_N_arr if self._padded else None)

    # ----------------------------------------------- decision + routing walk
    def offload_decide(self, jobs: JobBatch, sp: torch.Tensor,
                       uds: torch.Tensor, explore: float = 0.0,
                       gen: Optional[torch.Generator] = None,
                       prob: bool = False):
        """Greedy server selection (offloading_v3.py:388-439), batched.
        ``sp``: (B,N,N) shortest-path delays with ZERO diagonal;
        ``uds``: (B,N) per-node unit processing delays (inf at relays)."""
        B, J, S = self.B, self.Jmax, self.S
        if S == 0:
            # no servers anywhere in the batch: every job computes locally
            # (the reference's cost vector degenerates to [local])
            local = uds.gather(1, jobs.sources) * jobs.ul
            return jobs.sources.clone(), local
        if self.use_hip:
            from .ops import dispatch
            ext = dispatch.require_hip()
            # ε-greedy + softmax sampling run INSIDE the kernel: explore is
            # read from a device scalar (pass a 0-dim tensor for hipGraph
            # capture — the replay sees the current value) and randomness
            # comes from the stateless counter RNG, bumped here with a
            # device op (capture-safe, advances per replay)
            expl_t = None
            if torch.is_tensor(explore):
                expl_t = explore.to(self.device, torch.float32)
            elif explore > 0:
                self._explore_buf.fill_(float(explore))
                expl_t = self._explore_buf
            rng_t = None
            if expl_t is not None or prob:
                self._rng_state[1] += 1
                rng_t = self._rng_state
            # uds goes in by its strides (the diagonal view of dm: no copy)
            dst, islocal = ext.decide(
                sp.contiguous(), self.sp_hop.contiguous(), uds,
                self.k_servers, jobs.sources, jobs.mask,
                jobs.ul.contiguous(), jobs.dl.contiguous(),
                expl_t, rng_t, 1 if prob else 0)
            return dst, None

        bJ = self._bidx[:, None]
        src = jobs.sources                                    # (B,J)
        local = uds.gather(1, src) * jobs.ul                  # (B,J)

        sp_src = sp[bJ, src]                                  # (B,J,N)
        hop_src = self.sp_hop[bJ, src]                        # (B,J,N)
        srv = self.servers_safe[:, None, :].expand(B, J, S)
        ul_d = torch.maximum(sp_src.gather(2, srv) * jobs.ul[..., None],
                             hop_src.gather(2, srv))
        # undirected graphs: sp/hop are symmetric, so dl leg reuses the rows
        dl_d = torch.maximum(sp_src.gather(2, srv) * jobs.dl[..., None],
                             hop_src.gather(2, srv))
        uds_srv = uds.gather(1, srv.reshape(B, -1)).reshape(B, J, S)
        pr_d = torch.maximum(uds_srv * jobs.ul[..., None],
                             torch.ones_like(uds_srv))
        server_costs = ul_d + dl_d + pr_d                     # (B,J,S)
        server_costs = torch.where(
            self.server_mask[:, None, :], server_costs,
            torch.full_like(server_costs, float("inf")))
        costs = torch.cat([server_costs, local[..., None]], dim=2)  # (B,J,S+1)

        if prob:
            # the maximum runs over the finite costs only, as in the kernel:
            # a padded server slot or an unreachable server (inf) would
            # otherwise clamp to 1e30 and leave every real choice at weight 0
            fin = torch.isfinite(costs)
            logits = torch.where(fin, costs.clamp(max=1e30),
                                 torch.full_like(costs, float("-inf")))
            logits = logits - logits.amax(dim=2, keepdim=True)
            p = torch.exp(logits)
            p = torch.where(fin, p, torch.zeros_like(p))
            choice = torch.multinomial(
                p.reshape(B * J, S + 1), 1, generator=gen).reshape(B, J)
        else:
            choice = costs.argmin(dim=2)                      # (B,J)
        if explore > 0:
            nS = self.server_mask.sum(1, keepdim=True)        # (B,1)
            r = torch.rand(B, J, device=self.device, generator=gen)
            rc = (torch.rand(B, J, device=self.device, generator=gen)
                  * (nS + 1).to(self.dtype)).to(torch.int64)
            # uniform over [0..S_b]; index S_b means "local" → map to slot S
            rc = torch.where(rc >= nS, torch.full_like(rc, S), rc)
            choice = torch.where(r < explore, rc, choice)

        is_local = choice >= torch.minimum(
            self.server_mask.sum(1, keepdim=True),
            torch.full_like(choice, S))
        # map server slots through the server table
        dst = torch.where(
            is_local, src,
            self.servers_safe.gather(1, choice.clamp(max=S - 1)))
        dst = torch.where(jobs.mask, dst, src)
        est = torch.where(
            is_local, local,
            server_costs.gather(2, choice.clamp(max=S - 1)[..., None])[..., 0])
        return dst, est

    def route_walk(self, jobs: JobBatch, dst: torch.Tensor, sp: torch.Tensor):
        """Greedy next-hop walk (offloading_v3.py:441-453), lockstep over all
        jobs: next = argmin over neighbors of sp[nb, dst] (first-min =
        ascending node id, like np.argmin).  Returns (route_links (B,J,H)
        int64 padded -1, nhop (B,J))."""
        B, J, N = self.B, self.Jmax, self.N
        bJ = self._bidx[:, None]
        node = jobs.sources.clone()
        links, hops = [], torch.zeros(B, J, dtype=torch.int64,
                                      device=self.device)
        sp_to_dst = sp.gather(
            2, dst[:, None, :].expand(B, N, J))               # (B,N,J)
        for _ in range(self.walk_cap):
            active = (node != dst) & jobs.mask
            if not bool(active.any()):
                break
            adj_row = self.adj[bJ, node]                      # (B,J,N)
            cand = torch.where(adj_row, sp_to_dst.transpose(1, 2),
                               torch.full_like(sp_to_dst.transpose(1, 2),
                                               float("inf")))
            nxt = cand.argmin(dim=2)                          # (B,J)
            link = self.link_matrix[bJ, node, nxt]            # (B,J)
            links.append(torch.where(active, link,
                                     torch.full_like(link, -1)))
            node = torch.where(active, nxt, node)
            hops += active.to(torch.int64)
        if links:
            route_links = torch.stack(links, dim=2)           # (B,J,H)
        else:
            route_links = torch.full((B, J, 0), -1, dtype=torch.int64,
                                     device=self.device)
        # jobs still short of their destination after walk_cap hops were
        # truncated — count them (device-side; see check_overflow)
        self.overflow_total += ((node != dst) & jobs.mask).sum()
        return route_links, hops

    # --------------------------------------------------------- evaluation
    def _episode_eval(self, jobs: JobBatch, dst: torch.Tensor,
                      sp: torch.Tensor):
        """Walk + evaluate: fused HIP kernel on GPU, torch path on CPU.
        Returns (route_links, nhop, delay_emp, unit_mtx, written)."""
        if self.use_hip and self.hip_walk_ok:
            from .ops import dispatch
            ext = dispatch.require_hip()
            H = min(self.walk_cap, 64)
            rl, nhop, delay_emp, unit_mtx, written, overflow = ext.walk_eval(
                sp.contiguous(), jobs.sources, dst.contiguous(), jobs.mask,
                jobs.rates.contiguous(), jobs.ul.contiguous(),
                jobs.dl.contiguous(), self.k_adj_indptr, self.k_adj_idx,
                self.k_adj_link, self.k_conf_indptr, self.k_conf_base,
                self.k_conf_cols, self.link_rates.contiguous(),
                self.proc_bws.contiguous(), self.k_edges,
                self.T_arr.contiguous(), self.k_E_arr, self.k_N_arr, H,
                self.fp_iters, self.overflow_total)
            # the kernel adds its truncated walks to overflow_total itself
            self._last_overflow = overflow
            return rl, nhop, delay_emp, unit_mtx, written
        rl, nhop = self.route_walk(jobs, dst, sp)
        delay_emp, unit_mtx, written, *_ = self.evaluate(jobs, dst, rl, nhop)
        return rl, nhop, delay_emp, unit_mtx, written

    def check_overflow(self, strict: bool = True) -> int:
        """Truncated-walk detection: number of greedy walks that failed to
        reach their destination since the last call (synchronises; call at
        log points, not inside the hot loop).  ``strict`` raises on any —
        the evaluation harnesses use that; trainers log the count instead
        (a transiently pathological delay matrix under exploration should
        not kill a long run)."""
        n = int(self.overflow_total)
        if n:
            self.overflow_total.zero_()
            if strict:
                raise RuntimeError(
                    f"{n} greedy routing walk(s) failed to reach their "
                    f"destination within walk_cap={self.walk_cap} hops — "
                    "loads/delays for those jobs are truncated "
                    "(pathological delay matrix or walk_cap too small "
                    "for this topology)")
        return n

    def evaluate(self, jobs: JobBatch, dst: torch.Tensor,
                 route_links: torch.Tensor, nhop: torch.Tensor):
        """Analytic queueing evaluation (offloading_v3.py:455-550), batched.
        Returns (delay_emp (B,J), unit_mtx (B,N,N), unit_mask, link_lambda,
        link_mu, server_load)."""
        B, E, N, J = self.B, self.E, self.N, self.Jmax
        H = route_links.shape[2]
        valid = route_links >= 0                              # (B,J,H)
        safe = route_links.clamp(min=0)

        ulr = jobs.ul * jobs.rates
        dlr = jobs.dl * jobs.rates
        load = (ulr + dlr)[..., None].expand(B, J, H)
        flat_idx = (self._bidx[:, None, None] * E + safe).reshape(-1)
        link_lambda = torch.zeros(B * E, dtype=self.dtype, device=self.device)
        link_lambda = link_lambda.scatter_add(
            0, flat_idx, torch.where(valid, load,
                                     torch.zeros_like(load)).reshape(-1))
        server_load = torch.zeros(B, N, dtype=self.dtype, device=self.device)
        server_load = server_load.scatter_add(
            1, dst, torch.where(jobs.mask, ulr, torch.zeros_like(ulr)))

        with torch.no_grad():
            mu = fixed_point_mu(link_lambda, self.link_rates.reshape(-1),
                                self.cf_degs.reshape(-1), self.conf,
                                self.fp_iters)
        lam_r = link_lambda.reshape(B, E)
        mu_r = mu.reshape(B, E)

        # per-(job,hop) unit link delays with the per-job congestion fallback
        lam_h = lam_r.gather(1, safe.reshape(B, -1)).reshape(B, J, H)
        mu_h = mu_r.gather(1, safe.reshape(B, -1)).reshape(B, J, H)
        tot = (jobs.ul + jobs.dl)[..., None]
        gap = mu_h - lam_h
        unit = torch.where(gap > 0, 1.0 / torch.where(gap > 0, gap,
                                                      torch.ones_like(gap)),
                           self.T_arr[:, None, None] * lam_h / (tot * mu_h))
        nh = nhop.to(self.dtype)[..., None]
        hop_delay = (torch.maximum(jobs.ul[..., None] * unit, nh)
                     + torch.maximum(jobs.dl[..., None] * unit, nh))
        link_part = torch.where(valid, hop_delay,
                                torch.zeros_like(hop_delay)).sum(dim=2)

        bw_dst = self.proc_bws.gather(1, dst)
        sl_dst = server_load.gather(1, dst)
        sgap = bw_dst - sl_dst
        sunit = torch.where(
            sgap > 0, 1.0 / torch.where(sgap > 0, sgap, torch.ones_like(sgap)),
            self.T_arr[:, None] * sl_dst / (jobs.ul * bw_dst))
        server_part = torch.maximum(jobs.ul * sunit, torch.ones_like(sunit))
        delay_emp = torch.where(jobs.mask, link_part + server_part,
                                torch.full_like(link_part, float("nan")))

        # empirical unit-delay matrix + mask (for the MSE anchor)
        unit_mtx = torch.zeros(B * N * N, dtype=self.dtype, device=self.device)
        written = torch.zeros(B * N * N, dtype=torch.bool, device=self.device)
        e0 = self.edges[..., 0].gather(1, safe.reshape(B, -1)).reshape(B, J, H)
        e1 = self.edges[..., 1].gather(1, safe.reshape(B, -1)).reshape(B, J, H)
        base = (self._bidx[:, None, None] * (N * N))
        lin01 = (base + e0 * N + e1).reshape(-1)
        lin10 = (base + e1 * N + e0).reshape(-1)
        vmask = valid.reshape(-1)
        unit_mtx = unit_mtx.index_put((lin01[vmask],),
                                      unit.reshape(-1)[vmask])
        unit_mtx = unit_mtx.index_put((lin10[vmask],),
                                      unit.reshape(-1)[vmask])
        written = written.index_put((lin01[vmask],),
                                    torch.ones_like(lin01[vmask],
                                                    dtype=torch.bool))
        written = written.index_put((lin10[vmask],),
                                    torch.ones_like(lin10[vmask],
                                                    dtype=torch.bool))
        lin_d = (self._bidx[:, None] * (N * N) + dst * (N + 1)).reshape(-1)
        jm = jobs.mask.reshape(-1)
        unit_mtx = unit_mtx.index_put((lin_d[jm],), sunit.reshape(-1)[jm])
        written = written.index_put((lin_d[jm],),
                                    torch.ones_like(lin_d[jm],
                                                    dtype=torch.bool))
        return (delay_emp, unit_mtx.reshape(B, N, N),
                written.reshape(B, N, N), lam_r, mu_r, server_load)

    # ------------------------------------------------------------- critic
    def critic_backward(self, jobs: JobBatch, dst: torch.Tensor,
                        route_links: torch.Tensor,
                        nhop: Optional[torch.Tensor] = None,
                        per_graph: bool = False):
        """Critic loss over the routes tensor + grad wrt routes
        (gnn_offloading_agent.py:333-374) and the closed-form route-bias
        cotangent accumulation (:384-416), batched.  Returns
        (grad_edge (B,Ē), loss_fn scalar); with ``per_graph`` (HIP path
        only) the loss stays (B,), for the caller to sum in a later
        kernel."""
        B, E, Ee, J = self.B, self.E, self.Ee, self.Jmax
        if self.use_hip and self.hip_critic_ok:
            from .ops import dispatch
            ext = dispatch.require_hip()
            # the kernel looks the destinations' compute slots up itself
            grad_edge, loss = ext.critic(
                route_links.contiguous(), nhop.contiguous(),
                dst.contiguous(), jobs.mask,
                jobs.rates.contiguous(), jobs.ul.contiguous(),
                jobs.dl.contiguous(), self.k_conf_indptr, self.k_conf_base,
                self.k_conf_cols, self.link_rates.contiguous(),
                self.bw_comp.contiguous(), self.k_E_arr,
                self.T_arr.contiguous(), Ee,
                self.fp_iters, self.delay_clamp, self.node_vedge)
            return grad_edge, (loss if per_graph else loss.sum())
        vedge_dst = self.node_vedge.gather(1, dst)            # (B,J)
        H = route_links.shape[2]
        valid = route_links >= 0
        safe = route_links.clamp(min=0)

        # routes (B,Ē,J) — link hops + destination self-loop edge
        routes = torch.zeros(B, Ee, J, dtype=self.dtype, device=self.device)
        jidx = torch.arange(J, device=self.device)[None, :, None] \
            .expand(B, J, H)
        routes = routes.index_put(
            (self._bidx[:, None, None].expand(B, J, H)[valid],
             safe[valid], jidx[valid]), torch.ones(1, dtype=self.dtype,
                                                   device=self.device)[0]
            .expand(int(valid.sum())))
        jm = jobs.mask
        routes = routes.index_put(
            (self._bidx[:, None].expand(B, J)[jm], vedge_dst[jm],
             torch.arange(J, device=self.device)[None, :].expand(B, J)[jm]),
            torch.ones(int(jm.sum()), dtype=self.dtype, device=self.device))
        routes.requires_grad_(True)

        jobs_load = (jobs.rates * jobs.ul)[..., None]          # (B,J,1)
        jobs_data = (jobs.ul + jobs.dl)[:, None, :]            # (B,1,J)
        link_load = torch.bmm(routes, jobs_load)[..., 0]       # (B,Ē)
        lam_link = link_load[:, :E].reshape(-1)
        mu = fixed_point_mu(lam_link, self.link_rates.reshape(-1),
                            self.cf_degs.reshape(-1), self.conf,
                            self.fp_iters)
        link_d = delay_with_fallback(lam_link, mu, self.T_link, 101.0,
                                     self.delay_clamp).reshape(B, E)
        node_d = delay_with_fallback(link_load[:, E:], self.bw_comp,
                                     self.T_arr[:, None], 100.0,
                                     self.delay_clamp)
        unit_edge = torch.cat([link_d, node_d], dim=1)         # (B,Ē)
        delay_job_edge = torch.maximum(
            jobs_data * unit_edge[..., None] * routes, routes)
        loss_fn = delay_job_edge.sum()
        (grad_routes,) = torch.autograd.grad(loss_fn, routes,
                                             retain_graph=False)  # (B,Ē,J)

        # route-bias VJP: forward prefix sums of -grad_routes along each route
        # (links in order, then the destination self-loop edge)
        seq = torch.cat([safe, vedge_dst[..., None]], dim=2)   # (B,J,H+1)
        seq_valid = torch.cat([valid, jm[..., None]], dim=2)
        g_seq = grad_routes.gather(
            1, seq.transpose(1, 2)).transpose(1, 2)            # (B,J,H+1)? no:
        # grad_routes is (B,Ē,J): gather along Ē with index (B,H+1,J) where
        # index[b,h,j] = seq[b,j,h]
        g_seq = grad_routes.gather(1, seq.permute(0, 2, 1))    # (B,H+1,J)
        g_seq = g_seq.permute(0, 2, 1)                         # (B,J,H+1)
        g_seq = torch.where(seq_valid, g_seq, torch.zeros_like(g_seq))
        pref = -torch.cumsum(g_seq, dim=2)
        grad_edge = torch.zeros(B * Ee, dtype=self.dtype, device=self.device)
        flat_seq = (self._bidx[:, None, None] * Ee + seq).reshape(-1)
        grad_edge = grad_edge.scatter_add(
            0, flat_seq, torch.where(seq_valid, pref,
                                     torch.zeros_like(pref)).reshape(-1))
        return grad_edge.reshape(B, Ee), loss_fn.detach()

    def grad_dist_matrix(self, grad_edge: torch.Tensor, dm: torch.Tensor,
                         unit_mtx: torch.Tensor, written: torch.Tensor):
        """Assemble the N×N actor cotangent: route-bias scatter
        (gnn_offloading_agent.py:410-416) + 0.001·MSE anchor (:440-444)."""
        B, N, E = self.B, self.N, self.E
        flat = torch.zeros(B * N * N, dtype=self.dtype, device=self.device)
        ge_valid = grad_edge[:, :E].reshape(-1)[self._lk_sel]
        flat = flat.index_put((self._lk_lin01,), ge_valid)
        flat = flat.index_put((self._lk_lin10,), ge_valid)
        lin = (self._comp_b * (N * N) + self._comp_n * (N + 1))
        flat = flat.index_put(
            (lin,), grad_edge[self._comp_b, E + self._comp_r])
        grad_dist = flat.reshape(B, N, N)

        diff = dm.detach() - unit_mtx
        anchor_mask = written & torch.isfinite(dm.detach())
        anchor = torch.where(anchor_mask, 0.001 * diff,
                             torch.zeros_like(diff))
        n_valid = anchor_mask.sum().clamp(min=1)
        loss_mse = ((torch.where(anchor_mask, diff, torch.zeros_like(diff))
                     ** 2).sum() / n_valid.to(diff.dtype))
        return grad_dist + anchor, loss_mse

    # ------------------------------------------------------------ episodes
    def gnn_episode(self, jobs: JobBatch, explore: float = 0.0,
                    gen: Optional[torch.Generator] = None,
                    train: bool = True, prob: bool = False,
                    per_sample: bool = False,
                    refine: int = 0) -> EpisodeResult:
        """One full GNN episode over the batch.  With ``train=True`` the
        summed per-instance actor gradients are left in ``model.param.grad``
        (caller applies the optimizer / DP all-reduce).  With
        ``per_sample=True`` the result additionally carries
        ``per_sample_grads``: one gradient set per instance (the reference's
        replay-memory unit, gnn_offloading_agent.py:141-169), extracted from
        the per-graph dW/db partials of the fused ChebConv backward."""
        ctx = torch.enable_grad() if train else torch.no_grad()
        native_bwd = self.native_glue and self.hip_actor_ok
        with ctx:
            if native_bwd:
                dm, actor_saved = self._actor_forward_native(jobs)
            else:
                dm, link_delay, node_delay = self.actor_forward(jobs)
        sp = self.apsp(dm)
        uds = torch.diagonal(dm.detach(), dim1=1, dim2=2)     # (B,N)
        dst, est = self.offload_decide(jobs, sp, uds, explore, gen, prob)
        route_links, nhop, delay_emp, unit_mtx, written = \
            self._episode_eval(jobs, dst, sp)
        # congestion-aware refinement (inference-time, opt-in): jobs whose
        # analytic delay exceeds the horizon fall back to local compute and
        # the assignment is re-evaluated.  Sound because job sources are
        # distinct mobiles — a fallback only sheds load from links/servers
        # (remaining delays can only improve) and adds load to the job's
        # OWN processor (exactly the `local` method's delay).  Not part of
        # the reference semantics; records produced with it say so.
        for _ in range(int(refine) if not train else 0):
            over = jobs.mask & (delay_emp > self.T_arr[:, None])
            if not bool(over.any()):
                break
            dst = torch.where(over, jobs.sources, dst)
            route_links, nhop, delay_emp, unit_mtx, written = \
                self._episode_eval(jobs, dst, sp)

        loss_fn = loss_mse = None
        self.last_per_sample_grads = None
        if train:
            # native path: the critic's loss stays per graph and is summed
            # by the kernel that finishes loss_mse
            fuse_sum = native_bwd and self.use_hip and self.hip_critic_ok
            grad_edge, loss_fn = self.critic_backward(
                jobs, dst, route_links, nhop, per_graph=fuse_sum)
            self.per_sample_request = per_sample
            if fuse_sum:
                loss_mse, loss_fn = self._actor_backward_native(
                    actor_saved, grad_edge, dm, unit_mtx, written, loss_fn)
            elif native_bwd:
                loss_mse = self._actor_backward_native(
                    actor_saved, grad_edge, dm, unit_mtx, written)
            else:
                grad_dist, loss_mse = self.grad_dist_matrix(
                    grad_edge, dm, unit_mtx, written)
            if per_sample and not self.use_hip:
                # CPU/torch fallback: instances are independent blocks, so
                # a masked cotangent per graph yields its gradient set
                params = list(self.model.parameters())
                out = []
                for b in range(self.B):
                    gd = torch.zeros_like(grad_dist)
                    gd[b] = grad_dist[b]
                    gs = torch.autograd.grad(dm, params, grad_outputs=gd,
                                             retain_graph=True,
                                             allow_unused=True)
                    out.append([torch.zeros_like(p) if g is None
                                else g.detach()
                                for p, g in zip(params, gs)])
                self.last_per_sample_grads = out
                dm.backward(grad_dist)
            else:
                if not native_bwd:
                    dm.backward(grad_dist)
                if per_sample:
                    self.last_per_sample_grads = \
                        self._collect_per_sample_grads()
            self.per_sample_request = False

        return self._result(jobs, delay_emp, loss_fn, loss_mse,
                            routes=(dst, route_links, nhop))

    def _result(self, jobs: JobBatch, delay_emp: torch.Tensor,
                loss_fn=None, loss_mse=None, routes=None) -> EpisodeResult:
        """Per-graph summary of an episode: mean delay over the real jobs,
        congested-job and job counts (one HIP launch on the native path)."""
        if self.native_glue:
            tau, congest, nj = ops.require_hip().episode_summary(
                delay_emp.contiguous(), jobs.mask, self.T_arr)
        else:
            nj = jobs.mask.sum(1)
            de = torch.where(jobs.mask, delay_emp,
                             torch.zeros_like(delay_emp))
            tau = de.sum(1) / nj.to(self.dtype)
            congest = ((delay_emp > self.T_arr[:, None]) & jobs.mask).sum(1)
        dst, route_links, nhop = routes or (None, None, None)
        return EpisodeResult(tau=tau, congest=congest, num_jobs=nj,
                             delay_emp=delay_emp, loss_fn=loss_fn,
                             loss_mse=loss_mse, dst=dst,
                             route_links=route_links, nhop=nhop)

    # ----------------------------------------------- packet-level simulation
    def draw_arrivals(self, jobs: JobBatch, T_sim: int,
                      gen: Optional[torch.Generator] = None) -> torch.Tensor:
        """Per-slot Poisson arrival counts (B, T_sim, J) uint8 for
        ``simulate``, drawn on the engine's device; masked job slots are
        zero.  Raises if a count does not fit uint8."""
        lam = torch.where(jobs.mask, jobs.rates,
                          torch.zeros_like(jobs.rates))
        lam = lam[:, None, :].expand(self.B, int(T_sim), lam.shape[1])
        arr = torch.poisson(lam.contiguous(), generator=gen)
        if arr.numel() and float(arr.max()) > 255:
            raise ValueError("draw_arrivals: a slot count exceeds 255 "
                             "(uint8) — job rates too high for the "
                             "simulator's arrival format")
        return arr.to(torch.uint8)

    def simulate(self, jobs: JobBatch, result: EpisodeResult,
                 arrivals: torch.Tensor, warmup: int = 0,
                 trace: bool = False, stats: bool = False,
                 late_after=None, mac: str = "share") -> SimResult:
        """Replay an episode's decisions packet by packet: the per-timeslot
        simulator of ``sim.timeslot`` over ``result``'s routes, all B graphs
        in one HIP launch on the GPU.  ``arrivals`` is (B, T, J) counts
        (``draw_arrivals``).  On the CPU engine each case runs
        ``simulate_routes`` on its own fp64 arrays, so B=1 equals
        ``sim.timeslot.simulate``.  ``stats=True`` also fills
        ``SimResult.stats`` (``SimStats``): delay maxima, tails and
        histograms, the age of the backlog and per-resource queue
        statistics; ``late_after`` (an int or a (B,) tensor) is the sojourn
        above which a task counts as late, by default ``floor(T)`` of each
        graph, the analytic congestion horizon.  ``mac="mwis"`` replaces
        the fluid sharing of a link's rate by a collision-free schedule (a
        queue-weighted greedy independent set of the conflict graph per
        slot, ``sim.timeslot.mwis_schedule``) and fills
        ``SimResult.sched_slots``."""
        if mac not in ops.MAC_MODES:
            raise ValueError(f"simulate: mac must be one of {ops.MAC_MODES}, "
                             f"not {mac!r}")
        mwis = mac == "mwis"
        sched = None
        if result.dst is None or result.route_links is None \
                or result.nhop is None:
            raise ValueError("simulate: the EpisodeResult carries no routes")
        B, J = self.B, self.Jmax
        arrivals = torch.as_tensor(arrivals, device=self.device)
        assert arrivals.shape[0] == B and arrivals.shape[2] == J, \
            (tuple(arrivals.shape), (B, J))
        T_sim = arrivals.shape[1]
        warmup = int(warmup)
        st = None
        if stats:
            if late_after is None:
                late_after = torch.floor(self.T_arr)
            if not torch.is_tensor(late_after):
                late_after = torch.full((B,), int(late_after))
            late_after = late_after.to(device=self.device,
                                       dtype=torch.int32).reshape(B)
        if self.use_hip:
            out = ops.timeslot_sim(
                arrivals, result.route_links, result.nhop, result.dst,
                jobs.mask, jobs.ul, jobs.dl, self.link_rates, self.proc_bws,
                self.k_conf_indptr, self.k_conf_base, self.k_conf_cols,
                self.k_E_arr, self.k_N_arr, self.T_arr, warmup=warmup,
                trace=trace, stats=stats, late_after=late_after, mac=mac)
            delay_sum, count, tr = out[:3]
            st = out[3] if stats else None
            sched = out[-1] if mwis else None
        else:
            from .sim.timeslot import num_delay_bins, simulate_routes
            if arrivals.numel() and (int(arrivals.max()) > 255
                                     or int(arrivals.min()) < 0):
                raise ValueError("simulate: arrival counts must lie in "
                                 "[0, 255]")
            delay_sum = torch.zeros(B, J, dtype=torch.int64)
            count = torch.zeros(B, J, dtype=torch.int32)
            tr = torch.zeros(B, T_sim, 3, dtype=torch.int32) if trace \
                else None
            arr_np = arrivals.cpu().numpy()
            if stats:
                st = ops.empty_stats(B, J, self.E + self.N,
                                     num_delay_bins(T_sim))
            if mwis:
                sched = torch.zeros(B, self.E, dtype=torch.int32)
            for b, g in enumerate(self.cases):
                k = int(jobs.mask[b].sum())
                assert bool(jobs.mask[b, :k].all()), "mask is a prefix"
                out = simulate_routes(
                    g, jobs.ul[b, :k].cpu().numpy().astype(np.float64),
                    jobs.dl[b, :k].cpu().numpy().astype(np.float64),
                    result.dst[b, :k].cpu().numpy(),
                    result.route_links[b, :k].cpu().numpy(),
                    result.nhop[b, :k].cpu().numpy(), arr_np[b][:, :k],
                    warmup=warmup, trace=trace, stats=stats,
                    late_after=int(late_after[b]) if stats else None,
                    mac=mac)
                if mwis:
                    sched[b, :g.num_links] = torch.as_tensor(
                        out[-1]["sched_slots"])
                    out = out[:-1]
                if stats:
                    ops.fill_stats(st, b, out[-1], slice(0, k),
                                   g.num_links, self.E)
                delay_sum[b, :k] = torch.as_tensor(out[0])
                count[b, :k] = torch.as_tensor(out[1]).to(torch.int32)
                if trace:
                    for c, name in enumerate(("arrivals", "departures",
                                              "pkts_in_network")):
                        tr[b, :, c] = torch.as_tensor(
                            out[2][name]).to(torch.int32)
            delay_sum = delay_sum.to(self.device)
            count = count.to(self.device)
            tr = tr.to(self.device) if trace else None
            if stats:
                st = {k: v.to(self.device) for k, v in st.items()}
            if mwis:
                sched = sched.to(self.device)
        cnt = count.to(torch.float64)
        mean = torch.where(count > 0,
                           delay_sum.to(torch.float64) / cnt.clamp(min=1),
                           torch.full_like(cnt, float("nan")))
        arrived = torch.where(jobs.mask[:, None, :], arrivals,
                              torch.zeros_like(arrivals))[:, warmup:] \
            .sum(1, dtype=torch.int64)
        if stats:
            st = SimStats(**st, delay_sum=delay_sum, count=count,
                          late_after=late_after, num_links=self.E,
                          T_sim=int(T_sim), warmup=warmup)
        return SimResult(delay_sum=delay_sum, count=count, mean_delay=mean,
                         backlog=arrived - count.to(torch.int64), trace=tr,
                         stats=st, sched_slots=sched)

    def _collect_per_sample_grads(self):
        """Slice the per-graph dW/db partials stashed by ChebStackFn's
        backward into one gradient set per instance (the reference's
        replay-memory unit)."""
        raw = getattr(self, "_per_sample_raw", None)
        if raw is None:
            raise RuntimeError(
                "per-sample gradients need the fused ChebConv GPU path")
        dW, db = raw
        self._per_sample_raw = None
        params = list(self.model.parameters())
        L = len(params) // 2
        out = []
        for b in range(self.B):
            gset = []
            for l in range(L):
                kw, fi, fo = params[2 * l].shape
                gset.append(dW[b, l, :kw, :fi, :fo])
                gset.append(db[b, l, :params[2 * l + 1].shape[0]])
            out.append(gset)
        return out

    def baseline_episode(self, jobs: JobBatch) -> EpisodeResult:
        """Greedy baseline (AdHoc_train.py:126-142), batched."""
        B, N = self.B, self.N
        with torch.no_grad():
            # 1/rate stays +inf at rate==0, exactly like the reference's
            # dead `delay if delay > 0 else T` guard (AdHoc_train.py:132)
            dlist = 1.0 / self.link_rates                      # (B,E)
            dm = self._delay_matrix(
                dlist, torch.zeros_like(self.bw_comp))
            sp = self.apsp(dm)
            dproc = 1.0 / self.proc_bws
            uds = torch.where((self.proc_bws > 0),
                              dproc, torch.full_like(dproc, float("inf")))
            dst, est = self.offload_decide(jobs, sp, uds)
            rl, nhop, delay_emp, _, _ = self._episode_eval(jobs, dst, sp)
            return self._result(jobs, delay_emp, routes=(dst, rl, nhop))

    def local_episode(self, jobs: JobBatch) -> EpisodeResult:
        """Local computing (offloading_v3.py:363-386), batched."""
        B, J = self.B, self.Jmax
        with torch.no_grad():
            dst = jobs.sources
            if self.use_hip:
                # the fused kernel handles src==dst routes (0 hops) directly
                sp0 = torch.zeros(B, self.N, self.N, dtype=self.dtype,
                                  device=self.device)
                route_links, nhop, delay_emp, _, _ = self._episode_eval(
                    jobs, dst, sp0)
            else:
                route_links = torch.full((B, J, 0), -1, dtype=torch.int64,
                                         device=self.device)
                nhop = torch.zeros(B, J, dtype=torch.int64,
                                   device=self.device)
                delay_emp, *_ = self.evaluate(jobs, dst, route_links, nhop)
            return self._result(jobs, delay_emp,
                                routes=(dst, route_links, nhop))
