"""Inputs, host twin and fp64 reference for the exact per-job tests of the
sampling modes of ``decide_kernel`` (tests/test_gpu_decide_sampling.py on the
GPU; tests/test_decide_sampling_inputs.py proves the inputs on the CPU).

The kernel's RNG is stateless: every job's uniforms are a function of
(seed, counter, b·J + j) alone (the stream contract, docs/KERNELS.md).  The
twin below recomputes them in Python integers and numpy fp32, the reference
takes the costs of ``stage_oracle.decide_costs`` in fp64, an fp64 softmax and
the inverse CDF at the twin's uniform.  A job whose draw lies within DELTA of
a CDF boundary is *near*: there the kernel's fp32 CDF may round to the other
side, and the GPU tests leave it out (at most NEAR_CAP of the jobs).

The inputs go straight into ``ext.decide``: three synthetic graphs of twelve
nodes, 300 job slots (the launch has 256 threads and strides over J), five
server slots with 3, 5 and 1 valid servers.  Nothing here needs a GPU.
"""
import functools
import math
import types

import numpy as np
import torch

from multihop_offload_amd.engine import JobBatch
from tests import stage_oracle as so

B, N, J, S = 3, 12, 300, 5
THREADS = 256                        # decide's launch
SERVERS = ((1, 2, 3, -1, -1), (1, 2, 3, 4, 5), (1, -1, -1, -1, -1))
RELAYS = (10, 11)                    # uds = inf
# (seed, counter) pairs of the GPU tests: a negative seed (the kernel reads
# the int64 as unsigned) and a counter past 2^32
SEEDS = (31337, -7)
COUNTERS = (1, 2, 7, 2 ** 33 + 1)
EPS = (0.3, 1.0)
KS_COUNTERS = tuple(range(1, 9))
NEAR_CAP = 0.005
# smallest share of the unmasked jobs whose choice changes with the counter
# or the seed (prob mode); the CPU test holds the reference to it
CHANGE_SHARE = 0.4

# edge jobs: (graph, reserved source node, job slots).  The sources are
# reserved, so no ordinary job shares their doctored sp rows.
INF_EDGE = (1, 9, tuple(range(3, 300, 13)))   # sp to server slot 2 is +inf
INF_SLOT = 2
CLAMP = (0, 9, (5, 290))                      # one finite cost above 1e30
CLAMP_SLOT = 1
UNREACHABLE = (2, 9, (11, 270))               # the only server at sp = +inf
TIE = (1, 8, (20, 260))                       # slots 0 and 1 bit-identical
EDGES = dict(inf=INF_EDGE, clamp=CLAMP, unreachable=UNREACHABLE, tie=TIE)

M64 = (1 << 64) - 1
EXPLORE_OFFSET = 0x517CC1B727220A95


# ------------------------------------------------------------ stream twin
def mix64(z):
    """The splitmix64 finaliser on a Python integer, wrapping at 64 bits."""
    z = (z + 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def u01(h):
    """Top 24 bits as a float32 in [0, 1)."""
    return np.float32(h >> 40) * np.float32(2.0 ** -24)


def stream_key(seed, counter):
    return mix64((seed & M64) ^ mix64(counter & M64))


@functools.lru_cache(maxsize=None)
def streams(seed, counter, nb=B, nj=J):
    """The three uniforms of every job, (nb, nj) float32 each: the ``prob``
    draw, the explore-or-not draw and the exploration pick."""
    key = stream_key(seed, counter)
    u = np.zeros((3, nb, nj), dtype=np.float32)
    for b in range(nb):
        for j in range(nj):
            bj = b * nj + j
            u[0, b, j] = u01(mix64(key ^ bj))
            h1 = mix64(key ^ ((EXPLORE_OFFSET + bj) & M64))
            u[1, b, j] = u01(h1)
            u[2, b, j] = u01(mix64(h1))
    return u[0], u[1], u[2]


def explore_twin(seed, counter, eps, n_valid):
    """(explores (nb, nj) bool, pick (nb, nj) int64): a job explores iff its
    second uniform is under float32(eps); its pick is a valid server slot or
    ``S`` for local (``rc >= nS``), from the third uniform in fp32."""
    nb = len(n_valid)
    _, u_eps, u_pick = streams(seed, counter, nb, J)
    explores = u_eps < np.float32(eps)
    ns1 = (np.asarray(n_valid, dtype=np.int64) + 1).astype(np.float32)
    rc = (u_pick * ns1[:, None]).astype(np.float32).astype(np.int64)
    pick = np.where(rc >= np.asarray(n_valid)[:, None], S, rc)
    return torch.from_numpy(explores), torch.from_numpy(pick)


# ------------------------------------------------------------------ inputs
def _mobile(b, ordinary=True):
    taken = set(s for s in SERVERS[b] if s >= 0) | set(RELAYS)
    if ordinary:
        taken |= {8, 9}
    return [v for v in range(N) if v not in taken]


@functools.lru_cache(maxsize=None)
def inputs():
    """The crafted ``ext.decide`` inputs, every float rounded to fp32 and
    kept as fp64 (``so.as32``), and the masks of the edge jobs."""
    rng = np.random.RandomState(20240)
    sp = rng.uniform(1.0, 1.3, size=(B, N, N))
    sp = np.triu(sp, 1)
    sp = sp + sp.transpose(0, 2, 1)
    hop = np.ones((B, N, N)) - np.eye(N)
    uds = rng.uniform(3.0, 4.5, size=(B, N))
    src = np.zeros((B, J), dtype=np.int64)
    for b in range(B):
        srv = [s for s in SERVERS[b] if s >= 0]
        uds[b, srv] = rng.uniform(1.0, 1.5, size=len(srv))
        uds[b, list(RELAYS)] = np.inf
        pool = _mobile(b)
        src[b] = np.asarray(pool)[rng.randint(0, len(pool), size=J)]
    ul = rng.uniform(0.9, 1.1, size=(B, J))
    dl = rng.uniform(0.9, 1.1, size=(B, J))
    mask = rng.uniform(size=(B, J)) >= 0.1

    kind = {}
    for name, (b, node, slots) in EDGES.items():
        m = np.zeros((B, J), dtype=bool)
        m[b, list(slots)] = True
        src[m] = node
        mask |= m
        kind[name] = torch.from_numpy(m)
    b, node, _ = INF_EDGE
    sv = SERVERS[b][INF_SLOT]
    sp[b, node, sv] = sp[b, sv, node] = np.inf
    b, node, _ = CLAMP
    sv = SERVERS[b][CLAMP_SLOT]
    sp[b, node, sv] = sp[b, sv, node] = 1e31
    b, node, _ = UNREACHABLE
    sv = SERVERS[b][0]
    sp[b, node, sv] = sp[b, sv, node] = np.inf
    b, node, _ = TIE
    s0, s1 = SERVERS[b][0], SERVERS[b][1]
    sp[b, node, s1] = sp[b, s1, node] = sp[b, node, s0]
    uds[b, s1] = uds[b, s0]

    t = lambda a: so.as32(torch.from_numpy(a))
    mask = torch.from_numpy(mask)
    jobs = JobBatch(sources=torch.from_numpy(src), mask=mask,
                    rates=torch.ones(B, J, dtype=torch.float64),
                    ul=t(ul), dl=t(dl))
    servers = torch.tensor(SERVERS, dtype=torch.int32)
    edge = torch.zeros(B, J, dtype=torch.bool)
    for m in kind.values():
        edge |= m
    return dict(sp=t(sp), hop=t(hop), uds=t(uds), servers=servers, jobs=jobs,
                kind=kind, ordinary=mask & ~edge,
                n_valid=(servers >= 0).sum(1).tolist())


def view(servers, hop, dtype=torch.float64):
    """What ``so.decide_costs`` reads off an engine, for a server table
    (B, S) padded -1 and a hop matrix."""
    nb, ns = servers.shape
    return types.SimpleNamespace(
        B=nb, Jmax=None, S=ns, _bidx=torch.arange(nb),
        servers_safe=servers.clamp(min=0).to(torch.int64),
        server_mask=servers >= 0, sp_hop=hop.to(dtype))


def costs(vw, jobs, sp, uds, dtype=torch.float64):
    """(B, J, S+1) costs [server slots in order, local] in ``dtype``."""
    vw = types.SimpleNamespace(**vars(vw))
    vw.Jmax = jobs.sources.shape[1]
    vw.sp_hop = vw.sp_hop.to(dtype)
    jb = JobBatch(sources=jobs.sources, mask=jobs.mask, rates=jobs.rates,
                  ul=jobs.ul.to(dtype), dl=jobs.dl.to(dtype))
    return so.decide_costs(vw, jb, sp.to(dtype), uds.to(dtype))


# --------------------------------------------------------------- reference
def softmax_cdf(c):
    """(w, cdf, psum) of the kernel's weights exp(min(c, 1e30) - cmax), 0
    for a non-finite cost, cmax over the finite clamped costs; in c's
    dtype."""
    fin = torch.isfinite(c)
    cl = c.clamp(max=1e30)
    cmax = torch.where(fin, cl, torch.full_like(c, -math.inf)) \
        .amax(-1, keepdim=True)
    w = torch.where(fin, torch.exp(cl - cmax), torch.zeros_like(c))
    cdf = w.cumsum(-1)
    return w, cdf, cdf[..., -1]


def greedy_choice(c):
    """First minimum of the cost vector (slot index, ``S`` = local)."""
    return torch.from_numpy(np.argmin(c.numpy(), axis=-1))


def prob_choice(c, u, delta):
    """(choice, near): the inverse CDF of the fp64 softmax at r = u·psum —
    the first slot with r < cdf, local when none — and the jobs whose r lies
    within delta·psum of a boundary."""
    _, cdf, psum = softmax_cdf(c)
    r = torch.as_tensor(u).to(torch.float64) * psum
    choice = (r[..., None] >= cdf).sum(-1).clamp(max=c.shape[-1] - 1)
    near = ((r[..., None] - cdf).abs() < delta * psum[..., None]).any(-1)
    return choice, near


def outputs(choice, servers, jobs):
    """(dst, islocal) of a slot choice; masked jobs stay at their source."""
    ns = servers.shape[1]
    local = (choice >= ns) | ~jobs.mask
    srv = servers.to(torch.int64)[:, None, :].expand(-1, choice.shape[1], -1)
    dst = srv.gather(2, choice.clamp(max=ns - 1)[..., None])[..., 0]
    return torch.where(local, jobs.sources, dst), local


@functools.lru_cache(maxsize=None)
def case_costs():
    inp = inputs()
    vw = view(inp["servers"], inp["hop"])
    return costs(vw, inp["jobs"], inp["sp"], inp["uds"])


@functools.lru_cache(maxsize=None)
def cdf_deviation():
    """Worst |cdf32 - cdf64| / psum over the unmasked jobs: the same costs
    and softmax run in fp32 torch on the CPU."""
    inp = inputs()
    vw = view(inp["servers"], inp["hop"])
    c32 = costs(vw, inp["jobs"], inp["sp"], inp["uds"], torch.float32)
    _, cdf32, _ = softmax_cdf(c32)
    _, cdf64, psum = softmax_cdf(case_costs())
    dev = (cdf32.double() - cdf64).abs() / psum[..., None]
    return float(dev[inp["jobs"].mask].max())


def delta():
    """Half-width of the near band, as a share of psum: 8× the fp32
    reference's CDF deviation, floored at one step of the uniform."""
    return so.TOL_FACTOR * max(cdf_deviation(), 2.0 ** -24)


@functools.lru_cache(maxsize=None)
def expected(seed, counter, prob, eps):
    """The reference decision of one launch: dict(dst, islocal, choice,
    near, explores).  ``prob`` picks the base choice (inverse CDF or greedy),
    ``eps`` (None or 0: no exploration) overrides it where the twin
    explores.  ``near`` is set only where the ``prob`` choice is used."""
    inp = inputs()
    jobs = inp["jobs"]
    c = case_costs()
    if prob:
        u, _, _ = streams(seed, counter)
        choice, near = prob_choice(c, torch.from_numpy(u), delta())
    else:
        choice = greedy_choice(c)
        near = torch.zeros(B, J, dtype=torch.bool)
    explores = torch.zeros(B, J, dtype=torch.bool)
    if eps:
        explores, pick = explore_twin(seed, counter, eps, inp["n_valid"])
        choice = torch.where(explores, pick, choice)
    explores = explores & jobs.mask
    near = near & jobs.mask & ~explores
    dst, islocal = outputs(choice, inp["servers"], jobs)
    return dict(dst=dst, islocal=islocal, choice=choice, near=near,
                explores=explores)


def ks_distance(x):
    """Kolmogorov–Smirnov distance of a sample from U(0, 1)."""
    x = np.sort(np.asarray(x, dtype=np.float64).ravel())
    n = len(x)
    i = np.arange(1, n + 1)
    return float(max((i / n - x).max(), (x - (i - 1) / n).max()))
