"""The inputs, the stream twin and the fp64 reference of the exact
``decide`` sampling tests (tests/test_gpu_decide_sampling.py), checked on the
CPU alone: the choices compete, few draws lie near a CDF boundary, no greedy
decision is a near-tie, the twin's streams are uniform and uncorrelated, and
the reference's greedy choice is ``engine.offload_decide``'s.  A bad seed
fails here, as an input problem, and never looks like a kernel failure."""
import itertools

import numpy as np
import pytest
import torch

from tests import decide_sampling_cases as dc
from tests import stage_oracle as so

PAIRS = list(itertools.product(dc.SEEDS, dc.COUNTERS))


def test_mix64_is_the_published_splitmix64():
    # the first two outputs of splitmix64 seeded with 0
    assert dc.mix64(0) == 0xE220A8397B1DCDAF
    assert dc.mix64(0x9E3779B97F4A7C15) == 0x6E789E6AA1B965F4
    assert dc.u01(dc.M64) == np.float32(1.0 - 2.0 ** -24)
    assert dc.u01((1 << 40) - 1) == np.float32(0.0)
    # a negative seed is read as its 64-bit pattern
    assert dc.stream_key(-7, 1) == dc.stream_key((1 << 64) - 7, 1)
    assert dc.stream_key(-7, 1) != dc.stream_key(7, 1)


def test_shapes_and_edge_jobs():
    inp = dc.inputs()
    jobs, kind = inp["jobs"], inp["kind"]
    m = jobs.mask
    assert (dc.B, dc.N, dc.J, dc.S) == (3, 12, 300, 5) and dc.J > dc.THREADS
    assert inp["n_valid"] == [3, 5, 1]
    srv = inp["servers"]
    # valid slots first, pads at the tail
    assert bool(((srv >= 0).int().diff(dim=1) <= 0).all())
    for name in ("sp", "hop", "uds"):
        assert torch.equal(inp[name], so.as32(inp[name])), name
    sp, uds = inp["sp"], inp["uds"]
    assert torch.equal(sp, sp.transpose(1, 2))
    assert not bool(torch.diagonal(sp, dim1=1, dim2=2).any())
    assert bool(torch.isinf(uds[:, list(dc.RELAYS)]).all())
    masked = float((~m).double().mean())
    print(f"masked job slots {masked:.3f}, {int((~m)[:, dc.THREADS:].sum())} "
          f"of them past thread {dc.THREADS - 1}")
    assert 0.05 < masked < 0.15 and bool((~m)[:, dc.THREADS:].any(1).all())
    # ordinary sources are mobile nodes whose sp rows are untouched
    for b in range(dc.B):
        pool = set(dc._mobile(b))
        assert set(jobs.sources[b][inp["ordinary"][b]].tolist()) <= pool
        fin = sp[b][sorted(pool)]
        assert bool(((fin >= 1.0) & (fin <= 1.3) | (fin == 0)).all())
    for name, (b, node, slots) in dc.EDGES.items():
        k = kind[name]
        assert int(k.sum()) == len(slots) and bool(m[k].all())
        assert bool((jobs.sources[k] == node).all())
        assert min(slots) < dc.THREADS <= max(slots)

    c = dc.case_costs()
    w, cdf, psum = dc.softmax_cdf(c)
    greedy = dc.greedy_choice(c)
    # +inf sp: weight 0, never greedy, every other choice alive
    k = kind["inf"]
    assert bool(torch.isinf(c[k][:, dc.INF_SLOT]).all())
    assert bool((w[k][:, dc.INF_SLOT] == 0).all())
    assert int((w[k] > 0).sum(1).min()) == dc.S
    assert not bool((greedy[k] == dc.INF_SLOT).any())
    # the clamp: one finite cost above 1e30 takes all the mass
    k = kind["clamp"]
    big = c[k][:, dc.CLAMP_SLOT]
    assert bool(torch.isfinite(big).all()) and bool((big > 1e30).all())
    assert bool(torch.isfinite(big.float()).all())
    onehot = torch.zeros(dc.S + 1, dtype=torch.float64)
    onehot[dc.CLAMP_SLOT] = 1.0
    assert torch.equal(w[k], onehot.expand(int(k.sum()), -1))
    assert not bool((greedy[k] == dc.CLAMP_SLOT).any())
    # the only server unreachable: local, greedy and prob
    k = kind["unreachable"]
    assert bool(torch.isinf(c[k][:, :dc.S]).all())
    assert bool((greedy[k] == dc.S).all())
    assert bool((cdf[k][:, :dc.S] == 0).all()) and bool((psum[k] == 1).all())
    # two bit-identical server costs, in fp64 and in fp32, both alive
    k = kind["tie"]
    inp32 = dc.costs(dc.view(srv, inp["hop"]), jobs, sp, uds, torch.float32)
    for cc in (c, inp32):
        assert torch.equal(cc[k][:, 0], cc[k][:, 1])
    assert bool((w[k][:, 0] > 0.05 * psum[k]).all())
    assert bool((cdf[k][:, 1] == 2 * cdf[k][:, 0]).all())


def test_choices_compete():
    """(a) every ordinary job with three choices or more has three of them
    at probability 0.05 or more."""
    inp = dc.inputs()
    w, _, psum = dc.softmax_cdf(dc.case_costs())
    p = w / psum[..., None]
    alive = (p >= 0.05).sum(-1)
    many = torch.tensor(inp["n_valid"])[:, None].expand(-1, dc.J) + 1 >= 3
    sel = inp["ordinary"] & many
    print(f"{int(sel.sum())} ordinary jobs with 3+ choices, fewest choices "
          f"at p >= 0.05: {int(alive[sel].min())}")
    assert int(sel.sum()) > 400 and int(alive[sel].min()) >= 3
    # graph 2 (one server): both choices alive
    two = inp["ordinary"] & ~many
    assert int(alive[two].min()) == 2


def test_near_boundary_jobs_are_rare():
    """(b) delta = 8 × the fp32 reference's CDF deviation (floored at
    2^-24); at most 0.5 % of the unmasked jobs draw within delta·psum of a
    CDF boundary, at every (seed, counter) the GPU tests use."""
    dev, delta = dc.cdf_deviation(), dc.delta()
    n = int(dc.inputs()["jobs"].mask.sum())
    print(f"fp32-reference CDF deviation {dev:.3e} of psum, delta "
          f"{delta:.3e}")
    assert delta == so.TOL_FACTOR * max(dev, 2.0 ** -24)
    assert dev < 1e-5                      # the softmax is well conditioned
    for seed, counter in PAIRS:
        for eps in (None, 0.3):
            near = dc.expected(seed, counter, True, eps)["near"]
            print(f"seed {seed} counter {counter} eps {eps}: "
                  f"{int(near.sum())} of {n} unmasked jobs near")
            assert int(near.sum()) <= dc.NEAR_CAP * n


def test_no_greedy_near_tie():
    """(c) no unmasked ordinary job has a best / runner-up gap under 1e-5
    relative; an edge job has either that or an exact tie, which the
    first-minimum rule settles identically in every precision."""
    inp = dc.inputs()
    gap = so.decide_margin(dc.case_costs())
    m = inp["jobs"].mask
    print(f"smallest greedy gap {float(gap[inp['ordinary']].min()):.3e}")
    assert float(gap[inp["ordinary"]].min()) >= 1e-5
    edge = m & ~inp["ordinary"]
    assert bool(((gap[edge] >= 1e-5) | (gap[edge] == 0)).all())


def test_streams_are_uniform_and_uncorrelated():
    """(d) the twin's three streams over 8 counters of seed 31337: KS
    distance from U(0,1) under the 0.1 % critical value 1.95/sqrt(n), and
    the prob uniform uncorrelated (|r| < 4/sqrt(n)) with either exploration
    uniform of the same job."""
    seed = dc.SEEDS[0]
    u = np.stack([np.stack(dc.streams(seed, c)) for c in dc.KS_COUNTERS], 1)
    u = u.reshape(3, -1).astype(np.float64)
    n = u.shape[1]
    assert n == 8 * dc.B * dc.J
    for name, x in zip(("prob", "explore", "pick"), u):
        d = dc.ks_distance(x)
        print(f"{name}: KS distance {d:.4f}, critical {1.95 / n ** 0.5:.4f}")
        assert d < 1.95 / n ** 0.5
        assert x.min() >= 0.0 and x.max() < 1.0
    for k in (1, 2):
        r = float(np.corrcoef(u[0], u[k])[0, 1])
        print(f"correlation of prob with stream {k}: {r:+.4f}")
        assert abs(r) < 4.0 / n ** 0.5
    # the streams differ from each other, between counters and seeds
    a, b2 = dc.streams(seed, 1), dc.streams(seed, 2)
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(a[0], b2[0])
    assert not np.array_equal(a[0], dc.streams(dc.SEEDS[1], 1)[0])


def test_exploration_twin_reaches_what_the_gpu_tests_assert():
    inp = dc.inputs()
    m = inp["jobs"].mask
    for seed, counter in PAIRS:
        for eps in dc.EPS:
            e = dc.expected(seed, counter, False, eps)
            share = float(e["explores"].sum()) / float(m.sum())
            assert abs(share - eps) < 0.06
            if eps == 1.0:
                assert torch.equal(e["explores"], m)
            # a pad is never picked, local is
            ch = e["choice"][e["explores"]]
            nv = torch.tensor(inp["n_valid"])[:, None].expand(-1, dc.J)
            assert bool(((ch < nv[e["explores"]]) | (ch == dc.S)).all())
            assert bool((ch == dc.S).any())
            assert bool((e["dst"] >= 0).all())
    # the +inf server is reached by exploration at every eps
    k = inp["kind"]["inf"]
    for eps in dc.EPS:
        hits = sum(int((dc.expected(s, c, False, eps)["choice"][k]
                        == dc.INF_SLOT).sum()) for s, c in PAIRS)
        print(f"eps {eps}: exploration picks the +inf server {hits} times")
        assert hits > 0


def test_choices_change_with_counter_and_seed():
    m = dc.inputs()["jobs"].mask
    n = float(m.sum())
    seed, counter = dc.SEEDS[0], dc.COUNTERS[0]
    base = dc.expected(seed, counter, True, None)["choice"]
    for other in ((seed, counter + 1), (dc.SEEDS[1], counter)):
        ch = dc.expected(*other, True, None)["choice"]
        share = float(((ch != base) & m).sum()) / n
        print(f"{other}: {share:.3f} of the unmasked choices change")
        assert share >= dc.CHANGE_SHARE + 0.05


def test_torch_prob_path_takes_cmax_over_finite_costs():
    """The engine's torch ``prob`` path on set S (graph 1 has a padded
    server slot, cost inf): the maximum runs over the finite costs, as in
    the kernel, so the draw is valid and never returns the pad (it raised
    "invalid multinomial distribution" while inf clamped to 1e30 set the
    maximum).  The same torch code on the crafted inputs follows the
    reference softmax and treats the edge jobs as the kernel must."""
    from multihop_offload_amd.engine import EpisodeEngine

    eng, fr = so.engine("S"), so.front("S")
    jobs = fr["jobs"]
    assert bool((eng.k_servers[1] < 0).any())
    gen = torch.Generator().manual_seed(3)
    with torch.no_grad():
        dst, _ = eng.offload_decide(jobs, fr["sp"], fr["uds"], prob=True,
                                    gen=gen)
    assert bool((dst >= 0).all())
    assert torch.equal(dst[~jobs.mask], jobs.sources[~jobs.mask])

    # the crafted inputs (competing costs, pads, inf, the clamp) through the
    # same torch code: per (graph, slot) the number of jobs choosing it over
    # 20 draws against the reference softmax, within 4.5 sigma
    inp = dc.inputs()
    jobs, srv, kind = inp["jobs"], inp["servers"], inp["kind"]
    vw = dc.view(srv, inp["hop"])
    vw.Jmax, vw.use_hip = dc.J, False
    vw.device, vw.dtype = torch.device("cpu"), torch.float64
    w, _, psum = dc.softmax_cdf(dc.case_costs())
    p = torch.where(jobs.mask[..., None], w / psum[..., None],
                    torch.zeros_like(w))
    n = 20
    counts = torch.zeros(dc.B, dc.S + 1, dtype=torch.float64)
    for _ in range(n):
        dst, _ = EpisodeEngine.offload_decide(vw, jobs, inp["sp"], inp["uds"],
                                              prob=True, gen=gen)
        local = dst == jobs.sources
        slot = (dst[..., None] == srv.to(torch.int64)[:, None, :]).int() \
            .argmax(-1)
        slot = torch.where(local, torch.full_like(slot, dc.S), slot)
        assert bool((local | (dst[..., None] == srv[:, None, :]).any(-1))
                    .all())
        b = dc.CLAMP[0]
        assert bool((dst[kind["clamp"]]
                     == dc.SERVERS[b][dc.CLAMP_SLOT]).all())
        b = dc.INF_EDGE[0]
        assert not bool((dst[kind["inf"]]
                         == dc.SERVERS[b][dc.INF_SLOT]).any())
        assert bool(local[kind["unreachable"]].all())
        hit = torch.nn.functional.one_hot(slot, dc.S + 1).double()
        counts += (hit * jobs.mask[..., None]).sum(1)
    want = n * p.sum(1)
    sigma = (n * (p * (1 - p)).sum(1)).sqrt()
    print("counts", counts.tolist(), "expected", want.tolist())
    assert bool(((counts - want).abs() <= 4.5 * sigma + 1e-9).all())
    assert bool((counts[want == 0] == 0).all())


@pytest.mark.parametrize("name", ("A", "S"))
def test_reference_greedy_is_offload_decide(name):
    """(e) on an engine-built set the reference's costs, first-minimum
    choice and output mapping give ``engine.offload_decide``'s dst."""
    eng, fr = so.engine(name), so.front(name)
    jobs = fr["jobs"]
    vw = dc.view(eng.k_servers.cpu(), eng.sp_hop)
    c = dc.costs(vw, jobs, fr["sp"], fr["uds"])
    assert torch.equal(c, so.decide_costs(eng, jobs, fr["sp"], fr["uds"]))
    dst, islocal = dc.outputs(dc.greedy_choice(c), eng.k_servers.cpu(), jobs)
    with torch.no_grad():
        want, _ = eng.offload_decide(jobs, fr["sp"], fr["uds"])
    assert torch.equal(dst, want)
    assert torch.equal(islocal[jobs.mask], (want == jobs.sources)[jobs.mask])
