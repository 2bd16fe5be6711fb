"""The inputs of the per-kernel stage tests (tests/test_gpu_stages.py),
checked on the fp64 CPU oracle alone: every recipe of tests/stage_oracle.py
reaches the code path it is meant for and keeps every discontinuous
decision away from its boundary, and the fp32-reference errors the
tolerances are derived from stay under the conditioning ceiling.  A bad
seed fails here, as an input problem, and never looks like a kernel
failure."""
import pytest
import torch

from multihop_offload_amd.queueing import fixed_point_mu
from tests import stage_oracle as so

ACTOR = [(n, c) for n in so.SETS for c in so.ACTOR_CAPS[n]]
CRITIC = [(n, c) for n in so.SETS for c in so.CRITIC_CAPS]


def test_shapes_reach_the_documented_paths():
    want = dict(A=(20, 36, 55, 3, 15), B=(24, 182, None, 3, None),
                C=(25, 46, None, 3, None), D=(430, 3220, 3649, 8, None))
    for name, (N, E, Ee, S, J) in want.items():
        eng = so.engine(name)
        assert (eng.N, eng.E, eng.S) == (N, E, S)
        assert Ee is None or eng.Ee == Ee
        assert J is None or eng.Jmax == J
        large = so.lds_modes(eng)
        # A-C: all three queueing kernels LDS-resident at 256 threads;
        # D: all three on global scratch at 1024 threads, walk_eval in LDS
        assert all(large.values()) == (name == "D")
        assert any(large.values()) == (name == "D")
        assert (eng.E >= 1500) == (name == "D")
        assert all(so.lds_fits(eng).values())
    assert so.engine("B").E_list == [160, 158, 182]          # ragged E
    assert so.engine("C").E_list == [36, 46]
    assert so.engine("C").k_N_arr.tolist() == [20, 25]       # inert pad nodes
    assert so.engine("C")._padded
    assert so.engine("S").k_servers.tolist()[1][-1] == -1    # padded server


@pytest.mark.parametrize("name,cap", ACTOR)
def test_lambda_recipe_is_conditioned(name, cap):
    eng = so.engine(name, cap)
    lam, rounds = so.lam_input(name, cap)
    print(f"set {name} cap {cap}: repaired in {rounds} rounds")
    assert rounds <= so.REPAIR_ROUNDS
    assert not bool(so.band_marks(eng, lam, cap).any())
    assert torch.equal(lam, so.as32(lam)) and bool((lam > 0).all())
    # the history helper is the fixed point of the package
    hist = so.mu_history(eng, lam[:, :eng.E])
    mu = fixed_point_mu(lam[:, :eng.E].reshape(-1),
                        eng.link_rates.reshape(-1), eng.cf_degs.reshape(-1),
                        eng.conf, eng.fp_iters)
    assert torch.equal(hist[:, -1].reshape(-1), mu)
    cong, capped = so.regime(eng, lam, cap)
    lk = eng.link_mask
    n = float(lk.sum())
    f_cong = float((cong[:, :eng.E] & lk).sum()) / n
    f_cap = float((capped[:, :eng.E] & lk).sum()) / n
    print(f"congested {f_cong:.3f} capped {f_cap:.3f}")
    assert f_cong >= 0.2 and 1.0 - f_cong >= 0.2
    if cap > 0:
        assert f_cap >= 0.05
    # compute slots see both branches too
    real_n = so.real_slots(eng)[:, eng.E:]
    assert bool((cong[:, eng.E:] & real_n).any())
    assert bool((~cong[:, eng.E:] & real_n).any())
    # the clamp of the fixed point is active on some iteration
    ratio = lam[:, None, :eng.E] / hist[:, :-1]
    assert bool(((ratio > 1) & lk[:, None, :]).any())


@pytest.mark.parametrize("name", so.SETS + ("S",))
def test_front_is_conditioned(name):
    eng = so.engine(name)
    fr = so.front(name)
    print(f"set {name}: job rates repaired in {fr['rounds']} rounds")
    assert fr["rounds"] <= so.REPAIR_ROUNDS
    # S feeds decide only: the critic's cap conditions do not apply
    caps = () if name == "S" else so.CRITIC_CAPS
    assert so.check_front(name, fr, caps) == []
    assert fr["overflow"] == 0
    jobs = fr["jobs"]
    assert torch.equal(jobs.rates, so.as32(jobs.rates))
    # the margin helper recomputes offload_decide's own cost vector
    costs = so.decide_costs(eng, jobs, fr["sp"], fr["uds"])
    choice = costs.argmin(2)
    nS = eng.server_mask.sum(1, keepdim=True)
    dst = torch.where((choice >= nS) | ~jobs.mask, jobs.sources,
                      eng.servers_safe.gather(1, choice.clamp(max=eng.S - 1)))
    assert torch.equal(dst, fr["dst"])
    # relay rows carry uds = inf
    assert bool(torch.isinf(fr["uds"][eng.roles == 2]).all())
    assert bool((eng.roles == 2).any())


def test_truncated_walk_front():
    fr = so.front("A", 2)
    assert fr["H"] == 2 and fr["route_links"].shape[2] == 2
    assert fr["overflow"] > 0
    assert int(fr["nhop"].max()) == 2
    assert not bool(so.job_marks("A", fr).any())


def test_tie_case_is_an_exact_first_minimum():
    eng = so.engine("A")
    t = so.tie_case()
    costs = so.decide_costs(eng, t["jobs"], t["sp"], t["uds"])
    b, j, s0, s1 = t["b"], t["j"], t["s0"], t["s1"]
    assert s0 < s1
    assert float(costs[b, j, s0]) == float(costs[b, j, s1])
    assert float(costs[b, j, s0]) == float(costs[b, j].min())
    assert int(t["dst"][b, j]) == int(eng.servers[b, s0])
    # identical fp32 inputs -> the tie is exact in fp32 as well
    c32 = so.decide_costs(so.engine("A", 0.0, "float32"),
                          so.jobs_to(t["jobs"], "cpu", torch.float32),
                          t["sp"].float(), t["uds"].float())
    assert float(c32[b, j, s0]) == float(c32[b, j, s1]) == float(
        c32[b, j].min())


@pytest.mark.parametrize("name,cap", ACTOR)
def test_actor_head_reference_errors(name, cap):
    c = so.actor_case(name, cap)
    for k in c["ref"]:
        print(f"actor set {name} cap {cap} {k}: fp32-reference error "
              f"{c['ref'][k]:.3e} -> tolerance {c['tol'][k]:.3e}")
        assert c["tol"][k] <= so.TOL_CEILING


@pytest.mark.parametrize("name,cap", CRITIC)
def test_critic_reference_errors(name, cap):
    c = so.critic_case(name, cap)
    for k in c["ref"]:
        print(f"critic set {name} cap {cap} {k}: fp32-reference error "
              f"{c['ref'][k]:.3e} -> tolerance {c['tol'][k]:.3e}")
        assert c["tol"][k] <= so.TOL_CEILING


@pytest.mark.parametrize("name,walk_cap", [(n, None) for n in so.SETS]
                         + [("A", 2)])
def test_walk_eval_reference_errors(name, walk_cap):
    c = so.eval_case(name, walk_cap)
    for k in c["ref"]:
        print(f"walk_eval set {name} walk_cap {walk_cap} {k}: fp32-reference "
              f"error {c['ref'][k]:.3e} -> tolerance {c['tol'][k]:.3e}")
        assert c["tol"][k] <= so.TOL_CEILING


@pytest.mark.parametrize("cap", so.CRITIC_CAPS)
def test_three_iteration_inputs_are_conditioned(cap):
    """Set A at fp_iters = 3 (the one numeric case away from 10): λ and the
    job rates are repaired on 3-iteration engines, reach both delay
    branches, and the tolerances stay under the ceiling."""
    it = so.FEW_ITERS
    eng = so.engine("A", cap, fp_iters=it)
    assert eng.fp_iters == it
    lam, rounds = so.lam_input("A", cap, fp_iters=it)
    assert rounds <= so.REPAIR_ROUNDS
    assert not bool(so.band_marks(eng, lam, cap).any())
    assert so.mu_history(eng, lam[:, :eng.E]).shape[1] == it + 1
    cong, _ = so.regime(eng, lam, cap)
    lk = eng.link_mask
    assert bool((cong[:, :eng.E] & lk).any())
    assert bool((~cong[:, :eng.E] & lk).any())
    fr = so.front("A", fp_iters=it)
    assert fr["rounds"] <= so.REPAIR_ROUNDS
    assert so.check_front("A", fr, so.CRITIC_CAPS, it) == []
    for what, c in (("actor", so.actor_case("A", cap, it)),
                    ("critic", so.critic_case("A", cap, it))):
        for k in c["ref"]:
            print(f"{what} set A cap {cap} fp_iters {it} {k}: fp32-reference "
                  f"error {c['ref'][k]:.3e} -> tolerance {c['tol'][k]:.3e}")
            assert c["tol"][k] <= so.TOL_CEILING
