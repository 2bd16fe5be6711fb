"""GPU (MI355X): the sampling modes of ``decide_kernel`` (episode.hip),
exactly and per job.  The kernel's RNG is stateless, so the host twin of
tests/decide_sampling_cases.py gives every job's uniforms; the fp64 reference
there gives the exact softmax CDF, and the kernel's choice must be the
inverse CDF at that uniform (``prob``), or the twin's exploration pick
(ε-greedy).  Only jobs whose draw lies within delta·psum of a CDF boundary
are left out of a ``prob`` comparison — at most 0.5 % of the unmasked jobs,
proven on the CPU by tests/test_decide_sampling_inputs.py; every exploration
and greedy comparison is exact with no exclusion.  The stream contract is in
docs/KERNELS.md."""
import itertools

import pytest
import torch

from tests import decide_sampling_cases as dc
from tests import stage_oracle as so

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")

PAIRS = list(itertools.product(dc.SEEDS, dc.COUNTERS))


def _ext():
    from multihop_offload_amd.ops import dispatch
    return dispatch.require_hip()


def _f32(x):
    return x.to(torch.float32).cuda().contiguous()


def _args():
    inp = dc.inputs()
    jobs = inp["jobs"]
    return (_f32(inp["sp"]), _f32(inp["hop"]), _f32(inp["uds"]),
            inp["servers"].cuda(), jobs.sources.cuda(), jobs.mask.cuda(),
            _f32(jobs.ul), _f32(jobs.dl))


def _launch(args, seed=None, counter=None, prob=False, eps=None):
    """One ``ext.decide`` launch; eps=None passes no explore tensor."""
    rng = None if seed is None else torch.tensor(
        [seed, counter], dtype=torch.int64, device="cuda")
    expl = None if eps is None else torch.tensor(
        float(eps), dtype=torch.float32, device="cuda")
    dst, islocal = _ext().decide(*args, expl, rng, 1 if prob else 0)
    torch.cuda.synchronize()
    return dst.cpu(), islocal.cpu()


def _check_invariants(dst, islocal):
    """What holds for every launch: masked jobs stay home, no pad or -1 is
    ever a destination, islocal is dst == src."""
    inp = dc.inputs()
    jobs = inp["jobs"]
    m = jobs.mask
    assert torch.equal(dst[~m], jobs.sources[~m]) and bool(islocal[~m].all())
    assert bool((dst >= 0).all()) and bool((dst < dc.N).all())
    for b in range(dc.B):
        ok = set(s for s in dc.SERVERS[b] if s >= 0)
        assert set(dst[b][~islocal[b]].tolist()) <= ok, b
    assert torch.equal(islocal, dst == jobs.sources)


def _compare(tag, got, want, keep):
    dst, islocal = got
    diff = (dst != want["dst"]) | (islocal != want["islocal"])
    print(f"{tag}: {int(want['near'].sum())} near jobs left out, "
          f"{int((diff & keep).sum())} of {int(keep.sum())} compared jobs "
          f"differ ({int(diff.sum())} with the near ones)")
    assert torch.equal(dst[keep], want["dst"][keep]), tag
    assert torch.equal(islocal[keep], want["islocal"][keep]), tag


@needs_gpu
def test_prob_mode_is_the_inverse_cdf_at_the_twins_uniform():
    """``prob`` with no explore tensor, 2 seeds × 4 counters: dst and
    islocal equal the fp64 reference on every job that is not near."""
    inp = dc.inputs()
    kind, m = inp["kind"], inp["jobs"].mask
    n = int(m.sum())
    args = _args()
    for seed, counter in PAIRS:
        want = dc.expected(seed, counter, True, None)
        got = _launch(args, seed, counter, prob=True)
        assert int(want["near"].sum()) <= dc.NEAR_CAP * n
        _compare(f"prob seed {seed} counter {counter}", got, want,
                 ~want["near"])
        dst, islocal = got
        _check_invariants(dst, islocal)
        b = dc.INF_EDGE[0]
        assert not bool((dst[kind["inf"]]
                         == dc.SERVERS[b][dc.INF_SLOT]).any())
        b = dc.CLAMP[0]
        assert bool((dst[kind["clamp"]]
                     == dc.SERVERS[b][dc.CLAMP_SLOT]).all())
        assert bool(islocal[kind["unreachable"]].all())


@needs_gpu
@pytest.mark.parametrize("eps", dc.EPS)
def test_epsilon_greedy_is_the_twin_exactly(eps):
    """``prob = 0`` with an explore tensor: which jobs explore, their slot
    and local at rc >= nS — the whole output equals the twin's, no
    exclusions (the greedy margin is 4e-4 or more on these inputs)."""
    inp = dc.inputs()
    m = inp["jobs"].mask
    args = _args()
    greedy = _launch(args)
    inf_hits = 0
    for seed, counter in PAIRS:
        want = dc.expected(seed, counter, False, eps)
        dst, islocal = _launch(args, seed, counter, eps=eps)
        tag = f"eps {eps} seed {seed} counter {counter}"
        assert torch.equal(dst, want["dst"]), tag
        assert torch.equal(islocal, want["islocal"]), tag
        _check_invariants(dst, islocal)
        # jobs that do not explore keep the greedy choice
        keep = ~want["explores"]
        assert torch.equal(dst[keep], greedy[0][keep]), tag
        if eps == 1.0:
            assert torch.equal(want["explores"], m)
        b = dc.INF_EDGE[0]
        inf_hits += int((dst[inp["kind"]["inf"]]
                         == dc.SERVERS[b][dc.INF_SLOT]).sum())
    print(f"eps {eps}: the +inf server returned {inf_hits} times")
    assert inf_hits > 0


@needs_gpu
def test_prob_with_exploration():
    """``prob = 1`` and eps = 0.3: the exploring jobs (exactly the twin's
    set) follow the exploration twin, the others the ``prob`` reference
    minus its near jobs."""
    m = dc.inputs()["jobs"].mask
    args = _args()
    for seed, counter in PAIRS:
        want = dc.expected(seed, counter, True, 0.3)
        plain = dc.expected(seed, counter, True, None)
        got = _launch(args, seed, counter, prob=True, eps=0.3)
        tag = f"prob + eps 0.3 seed {seed} counter {counter}"
        assert int(want["near"].sum()) <= dc.NEAR_CAP * int(m.sum())
        ex = want["explores"]
        assert torch.equal(ex, dc.expected(seed, counter, False, 0.3)
                           ["explores"])
        assert not bool((want["near"] & ex).any())
        _compare(tag, got, want, ~want["near"])
        _check_invariants(*got)
        # the two sets: exploring jobs equal the exploration twin exactly,
        # the rest equal the prob-only reference
        assert torch.equal(got[0][ex], want["dst"][ex]), tag
        rest = ~ex & ~plain["near"]
        assert torch.equal(got[0][rest], plain["dst"][rest]), tag
        # the exploration moved some job off its prob choice
        assert bool((want["dst"][ex] != plain["dst"][ex]).any())


@needs_gpu
def test_explore_zero_is_the_greedy_launch():
    """An explore tensor holding 0.0 (``prob = 0``) is bit-equal to the
    launch with no explore tensor and no rng."""
    args = _args()
    greedy = _launch(args)
    want = dc.expected(dc.SEEDS[0], dc.COUNTERS[0], False, None)
    assert torch.equal(greedy[0], want["dst"])
    assert torch.equal(greedy[1], want["islocal"])
    for seed, counter in PAIRS[:2]:
        got = _launch(args, seed, counter, eps=0.0)
        assert torch.equal(got[0], greedy[0])
        assert torch.equal(got[1], greedy[1])


@needs_gpu
def test_determinism_and_advance():
    """Two launches on one (seed, counter) are bit-equal; counter + 1, and
    another seed, change at least CHANGE_SHARE of the unmasked choices (the
    reference's own share less the near jobs of either launch)."""
    m = dc.inputs()["jobs"].mask
    n = int(m.sum())
    args = _args()
    seed, counter = dc.SEEDS[0], dc.COUNTERS[0]
    for prob, eps in ((True, None), (False, 0.3), (True, 0.3)):
        a = _launch(args, seed, counter, prob, eps)
        b = _launch(args, seed, counter, prob, eps)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    base = _launch(args, seed, counter, prob=True)
    wbase = dc.expected(seed, counter, True, None)
    for other in ((seed, counter + 1), (dc.SEEDS[1], counter)):
        got = _launch(args, *other, prob=True)
        want = dc.expected(*other, True, None)
        changed = int(((got[0] != base[0]) & m).sum())
        ref = int(((want["dst"] != wbase["dst"]) & m).sum())
        slack = int(want["near"].sum()) + int(wbase["near"].sum())
        print(f"{other}: {changed} of {n} unmasked destinations change, "
              f"reference {ref}")
        assert changed >= ref - slack
        assert changed >= dc.CHANGE_SHARE * n


@needs_gpu
def test_graph_replay_draws_fresh_randomness_and_reads_explore():
    """One ``eng.offload_decide(..., explore=<0-dim device tensor>,
    prob=True)`` on stage-oracle set A, captured in a linear torch.cuda.graph
    and replayed: every replay equals an eager ``ext.decide`` on the same
    inputs with the rng tensor [seed, c0 + i] and the same explore value,
    the engine's counter has advanced by the number of replays, and a replay
    after the explore tensor was set to 0 equals the prob-only launch at its
    counter."""
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack

    ext = _ext()
    fr = so.front("A")
    eng = EpisodeEngine(list(so.cases("A")),
                        ChebConvStack(K=2, dtype=torch.float32, seed=0),
                        device="cuda", dtype=torch.float32)
    assert eng.use_hip
    seed = 4242
    eng.set_rng_seed(seed)
    jobs = so.jobs_to(fr["jobs"], "cuda", torch.float32)
    sp, uds = _f32(fr["sp"]), _f32(fr["uds"])
    explore = torch.tensor(0.3, dtype=torch.float32, device="cuda")

    def eager(counter, eps):
        rng = torch.tensor([seed, counter], dtype=torch.int64, device="cuda")
        expl = None if eps is None else torch.tensor(
            eps, dtype=torch.float32, device="cuda")
        dst, _ = ext.decide(sp, eng.sp_hop.contiguous(), uds, eng.k_servers,
                            jobs.sources, jobs.mask, jobs.ul.contiguous(),
                            jobs.dl.contiguous(), expl, rng, 1)
        return dst

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        eng.offload_decide(jobs, sp, uds, explore=explore, prob=True)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    c0 = int(eng._rng_state[1])
    assert c0 == 1 and int(eng._rng_state[0]) == seed

    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        dst, _ = eng.offload_decide(jobs, sp, uds, explore=explore,
                                    prob=True)
    torch.cuda.synchronize()
    assert int(eng._rng_state[1]) == c0        # capture launches nothing
    clones = []
    for _ in range(3):
        graph.replay()
        torch.cuda.synchronize()
        clones.append(dst.clone())
    assert int(eng._rng_state[1]) == c0 + 3
    for i, got in enumerate(clones, 1):
        assert torch.equal(got, eager(c0 + i, 0.3)), i
    assert not torch.equal(clones[0], clones[1])
    assert not torch.equal(clones[1], clones[2])

    explore.zero_()
    graph.replay()
    torch.cuda.synchronize()
    got = dst.clone()
    assert int(eng._rng_state[1]) == c0 + 4
    assert torch.equal(got, eager(c0 + 4, None))
    assert torch.equal(got, eager(c0 + 4, 0.0))
    assert not torch.equal(got, eager(c0 + 4, 0.3))
    explore.fill_(0.3)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(dst, eager(c0 + 5, 0.3))
