"""CPU tests of the packet simulator's scheduled MAC (``mac="mwis"``): the
schedule itself, the oracle loop, the CPU engine path, the stand-alone host
run of the kernel's phases with ``Mwis = true`` and the evaluator CLI.  Every
comparison is integer equality."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

from multihop_offload_amd.sim import timeslot as ts
from multihop_offload_amd.sim.timeslot import (dump_case, mwis_schedule,
                                               simulate_routes)
from multihop_offload_amd.utils.mwis import local_greedy_search
from tests import timeslot_cases as tc
from tests import timeslot_mwis_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _cpu_engine(cases):
    from multihop_offload_amd.engine import EpisodeEngine
    from multihop_offload_amd.models.chebconv import ChebConvStack
    model = ChebConvStack(K=2, dtype=torch.float64, seed=3)
    return EpisodeEngine(cases, model, device="cpu", dtype=torch.float64)


# ---- 1: the schedule against the dense reference rebuild -------------------
@pytest.mark.parametrize("seed", range(50))
def test_schedule_matches_local_greedy_search(seed):
    rng = np.random.RandomState(seed)
    n = rng.randint(8, 41)
    adj = np.triu(rng.rand(n, n) < rng.uniform(0.05, 0.5), 1)
    adj = adj | adj.T
    w = rng.randint(0, 4, size=n).astype(np.float64)   # ties and zeros
    cip = np.concatenate([[0], np.cumsum(adj.sum(1))])
    cols = np.concatenate([np.nonzero(r)[0] for r in adj]).astype(np.int64)
    on, rounds = mwis_schedule(cip, cols, w)
    assert on.dtype == bool and on.shape == (n,)
    want = {v for v in local_greedy_search(adj, w)[0] if w[v] > 0}
    assert set(np.nonzero(on)[0].tolist()) == want
    assert not (adj[on][:, on]).any()                   # independent
    for v in np.nonzero((w > 0) & ~on)[0]:              # maximal
        assert (adj[v] & on).any(), v
    assert rounds == 0 if not (w > 0).any() else rounds >= 1
    assert mwis_schedule(cip, cols, np.zeros(n))[1] == 0


# ---- 2: oracle sanity on G1 and G2 -----------------------------------------
@pytest.fixture(scope="module")
def batches():
    """G1 and G2 with baseline routes from the fp64 CPU engine: the mwis
    oracle on the fp32-rounded arrays, and the share oracle beside it."""
    out = {}
    for name, (cases, jobs_list) in (("g1", tc.g1_batch()),
                                     ("g2", tc.g2_batch())):
        eng = _cpu_engine(cases)
        jobs = eng.pack_jobs(jobs_list)
        res = eng.baseline_episode(jobs)
        arr = tc.batch_arrivals(jobs_list, eng.Jmax)
        routes = (res.dst.numpy(), res.route_links.numpy(), res.nhop.numpy())
        ref = mc.oracle_batch(cases, jobs_list, *routes, arr)
        share = tc.oracle_batch(cases, jobs_list, *routes, arr)
        out[name] = (cases, jobs_list, eng, jobs, res, arr, ref, share)
    return out


def test_oracle_sanity(batches):
    rounds_all = []
    for name in ("g1", "g2"):
        cases, jobs_list, eng, jobs, res, arr, ref, share = batches[name]
        ds, ct, tr, sched, rounds, logs = ref
        print(name, "completed", ct.sum(1).tolist(), "rounds_max", rounds)
        rounds_all += rounds
        for b, (g, jb) in enumerate(zip(cases, jobs_list)):
            k = jb.num_jobs
            assert ct[b].sum() > 100
            assert not np.array_equal(ds[b], share[0][b])
            out = mc.oracle_case(g, jb, res.dst[b].numpy(),
                                 res.route_links[b].numpy(),
                                 res.nhop[b].numpy(), arr[b], stats=True)
            st, sc = out[-2], out[-1]
            assert np.array_equal(out[0], ds[b, :k])    # stats change nothing
            assert sc["sched_slots"].dtype == np.int32
            assert np.array_equal(sc["sched_slots"], sched[b, :g.num_links])
            assert (sc["sched_slots"]
                    <= st["busy_slots"][:g.num_links]).all()
            assert sc["sched_slots"].sum() > 0
            assert sc["rounds_max"] == rounds[b] == max(r for _, _, r
                                                        in logs[b])
            for w, on, r in logs[b]:
                assert mc.independent(g, on)
    assert max(rounds_all) >= 3, rounds_all


# ---- 3: the tie-break on G3 ------------------------------------------------
def _reversed_tie(cip, cols, w):
    """``mwis_schedule`` with ties going to the HIGHER id: the real one on
    the graph with the ids mirrored."""
    E = len(w)
    rows = [sorted(E - 1 - int(m) for m in cols[cip[E - 1 - n]:cip[E - n]])
            for n in range(E)]
    cip2 = np.concatenate([[0], np.cumsum([len(r) for r in rows])])
    cols2 = np.array([m for r in rows for m in r], dtype=np.int64)
    on, r = _REAL(cip2, cols2, np.asarray(w)[::-1])
    return on[::-1].copy(), r


_REAL = mwis_schedule


def g3_oracle(**kw):
    g, jobs, arr, rl, nhop, dst = tc.g3_case()
    return simulate_routes(tc.rounded(g), jobs.ul, jobs.dl, dst, rl, nhop,
                           arr, mac="mwis", **kw)


def test_tie_break_g3(monkeypatch):
    g, jobs, arr, rl, nhop, dst = tc.g3_case()
    assert rl[1, 0] < rl[0, 0]                  # job 1 rides the lower id
    cip, cols = np.asarray(g.conf_indptr), np.asarray(g.conf_indices)
    assert rl[0, 0] in cols[cip[rl[1, 0]]:cip[rl[1, 0] + 1]]   # they conflict
    ds, ct, sc = g3_oracle()
    assert ct.tolist() == [6, 6]
    assert ds[0] > ds[1], ds
    monkeypatch.setattr(ts, "mwis_schedule", _reversed_tie)
    ds2, ct2, _ = g3_oracle()
    assert ct2.tolist() == [6, 6]
    assert ds2.tolist() == ds.tolist()[::-1]    # the case discriminates


# ---- 4: the defaults are where they were -----------------------------------
def test_share_is_the_default(tmp_path, batches):
    cases, jobs_list, eng, jobs, res, arr, ref, share = batches["g1"]
    g, jb = cases[0], jobs_list[0]
    k = jb.num_jobs
    args = (g, jb.ul, jb.dl, res.dst[0, :k].numpy(),
            res.route_links[0, :k].numpy(), res.nhop[0, :k].numpy(),
            arr[0][:, :k])
    a = simulate_routes(*args, warmup=tc.WARMUP, trace=True, stats=True)
    b = simulate_routes(*args, warmup=tc.WARMUP, trace=True, stats=True,
                        mac="share")
    assert len(a) == len(b) == 4
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    for d0, d1 in ((a[2], b[2]), (a[3], b[3])):
        assert d0.keys() == d1.keys()
        for key in d0:
            assert np.array_equal(d0[key], d1[key]), key
    assert tuple(a[3]) == ts.STAT_KEYS
    with pytest.raises(ValueError):
        simulate_routes(*args, mac="tdma")
    p0, p1, p2 = (str(tmp_path / n) for n in ("a.bin", "b.bin", "c.bin"))
    dump_case(p0, *args, warmup=tc.WARMUP)
    dump_case(p1, *args, warmup=tc.WARMUP, mac=0)
    dump_case(p2, *args, warmup=tc.WARMUP, mac=1)
    raw0, raw1, raw2 = (open(p, "rb").read() for p in (p0, p1, p2))
    assert raw0 == raw1
    assert np.frombuffer(raw0[:36], dtype=np.int32)[8] == 0
    assert np.frombuffer(raw2[:36], dtype=np.int32)[8] == 1
    assert raw0[:32] == raw2[:32] and raw0[36:] == raw2[36:]


# ---- 5: the CPU engine -----------------------------------------------------
@pytest.mark.parametrize("name", ["g1", "g2"])
def test_cpu_engine_simulate_mwis(batches, name):
    """engine.simulate(mac="mwis") is the oracle per case on the cases' own
    fp64 arrays; G2's padded links and nodes read zero."""
    cases, jobs_list, eng, jobs, res, arr, ref, share = batches[name]
    sim = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP,
                       trace=True, stats=True, mac="mwis")
    assert sim.sched_slots.dtype == torch.int32
    assert sim.sched_slots.shape == (eng.B, eng.E)
    for b, (g, jb) in enumerate(zip(cases, jobs_list)):
        k, Eb = jb.num_jobs, g.num_links
        out = simulate_routes(
            g, jb.ul, jb.dl, res.dst[b, :k].numpy(),
            res.route_links[b, :k].numpy(), res.nhop[b, :k].numpy(),
            arr[b][:, :k], warmup=tc.WARMUP, trace=True, stats=True,
            late_after=int(g.T), mac="mwis")
        assert np.array_equal(sim.delay_sum[b, :k].numpy(), out[0])
        assert np.array_equal(sim.count[b, :k].numpy(), out[1])
        assert np.array_equal(sim.trace[b, :, 2].numpy(),
                              out[2]["pkts_in_network"])
        assert np.array_equal(sim.sched_slots[b, :Eb].numpy(),
                              out[4]["sched_slots"])
        assert not sim.sched_slots[b, Eb:].any()
        assert np.array_equal(sim.stats.busy_slots[b, :Eb].numpy(),
                              out[3]["busy_slots"][:Eb])
    if name == "g2":
        assert cases[1].num_links < eng.E       # there are padded links
    share_ = sim.sched_share()
    assert share_.dtype == torch.float64 and share_.shape == (eng.B, eng.E)
    busy = sim.stats.busy_slots[:, :eng.E] > 0
    assert torch.isnan(share_[~busy]).all()
    assert ((share_[busy] > 0) | (sim.sched_slots[busy] == 0)).all()
    assert (share_[busy] <= 1).all()
    plain = eng.simulate(jobs, res, torch.as_tensor(arr), warmup=tc.WARMUP)
    assert plain.sched_slots is None
    with pytest.raises(ValueError):
        plain.sched_share()
    with pytest.raises(ValueError):
        eng.simulate(jobs, res, torch.as_tensor(arr), mac="tdma")


# ---- 6: the kernel's phases as a stand-alone host program ------------------
@pytest.fixture(scope="module")
def host_prog(tmp_path_factory):
    cxx = next((c for c in ("c++", "g++", "clang++")
                if shutil.which(c)), None)
    if cxx is None:
        pytest.skip("no host C++ compiler found")
    out = str(tmp_path_factory.mktemp("tsmwis") / "timeslot_mwis_host")
    base = [cxx, "-std=c++17", "-O1", "-g", "-I",
            os.path.join(ROOT, "multihop_offload_amd", "ops", "hip"),
            os.path.join(ROOT, "tests", "host", "timeslot_mwis_host.cpp"),
            "-o", out]
    san = subprocess.run(base + ["-fsanitize=address,undefined",
                                 "-fno-sanitize-recover=all"],
                         capture_output=True, text=True)
    if san.returncode == 0:
        return out, "address,undefined"
    plain = subprocess.run(base, capture_output=True, text=True)
    assert plain.returncode == 0, plain.stderr
    return out, "none"


def _run_host(prog, path, nt, stage=False):
    run = subprocess.run([prog, path, str(nt)] + ["stage"] * stage,
                         capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-400:] + run.stderr[-2000:]
    lines = run.stdout.split("\n")
    assert lines[0] == "error 0"

    def rows(tag, skip):
        return np.array([[int(x) for x in ln.split()[skip:]]
                         for ln in lines if ln.startswith(tag + " ")])
    return (rows("job", 1), rows("trace", 2), rows("sched", 1),
            int(lines[1].split()[1]))


@pytest.mark.parametrize("b", [0, 1, 2])
@pytest.mark.parametrize("nt,stage", [(7, False), (64, False), (64, True)])
def test_host_program_matches_oracle(tmp_path, host_prog, batches, b, nt,
                                     stage):
    """The Mwis phases, thread by thread on the host (under ASan/UBSan where
    they link), with the schedule's words dirty at the start: delay sums,
    counts, trace and sched_slots equal the oracle on the G1 dumps, with the
    conflict columns read in place and from their 16-bit staged copy."""
    prog, san = host_prog
    print(f"host program built with sanitizers: {san}")
    cases, jobs_list, eng, jobs, res, arr, ref, share = batches["g1"]
    ds, ct, tr, sched, rounds, logs = ref
    g, jb = cases[b], jobs_list[b]
    k = jb.num_jobs
    path = str(tmp_path / "case.bin")
    dump_case(path, g, jb.ul, jb.dl, res.dst[b, :k].numpy(),
              res.route_links[b, :k].numpy(), res.nhop[b, :k].numpy(),
              arr[b][:, :k], warmup=tc.WARMUP, mac=1)
    job, gtr, gsc, iters = _run_host(prog, path, nt, stage)
    assert np.array_equal(job[:, 0], np.arange(k))
    assert np.array_equal(job[:, 1], ds[b, :k])
    assert np.array_equal(job[:, 2], ct[b, :k])
    assert np.array_equal(gtr, tr[b])
    assert np.array_equal(gsc[:, 0], np.arange(g.num_links))
    assert np.array_equal(gsc[:, 1], sched[b, :g.num_links])
    # the round loop may run one closing round that finds no candidate
    assert rounds[b] <= iters <= rounds[b] + 1


def test_host_program_g3_and_share_mode(tmp_path, host_prog):
    """G3 on the host twin gives the oracle's pair, not the swapped one; a
    dump with mode word 0 runs the plain phases."""
    prog, san = host_prog
    g, jobs, arr, rl, nhop, dst = tc.g3_case()
    ds, ct, tr, sc = g3_oracle(trace=True)
    path = str(tmp_path / "g3.bin")
    dump_case(path, g, jobs.ul, jobs.dl, dst, rl, nhop, arr, mac=1)
    job, gtr, gsc, _ = _run_host(prog, path, 5)
    assert job[:, 1].tolist() == ds.tolist() and ds[0] > ds[1]
    assert job[:, 2].tolist() == ct.tolist()
    assert np.array_equal(gtr[:, 2], tr["pkts_in_network"])
    assert np.array_equal(gsc[:, 1], sc["sched_slots"])
    ds0, ct0 = simulate_routes(tc.rounded(g), jobs.ul, jobs.dl, dst, rl,
                               nhop, arr)
    dump_case(path, g, jobs.ul, jobs.dl, dst, rl, nhop, arr)
    job0, _, gsc0, _ = _run_host(prog, path, 5)
    assert job0[:, 1].tolist() == ds0.tolist()
    assert gsc0.size == 0


# ---- 7: the evaluator CLI --------------------------------------------------
def test_evaluate_sim_mac_cli_cpu(tmp_path):
    from multihop_offload_amd.harness import evaluate as ev
    common = ["--training_set", "BAT1000",
              "--model_root", os.path.join(ROOT, "artifacts", "model"),
              "--sizes", "20", "--cases-per-size", "2", "--instances", "1",
              "--workers", "0", "--device", "cpu", "--simulate", "200"]
    paths = [str(tmp_path / n) for n in ("a.json", "b.json", "c.json")]
    ev.main(common + ["--sim-stats", "--out", paths[0]])
    ev.main(common + ["--sim-mac", "mwis", "--out", paths[1]])
    ev.main(common + ["--sim-mac", "mwis", "--sim-stats", "--out", paths[2]])
    a, b, c = (json.load(open(p)) for p in paths)
    assert set(a) == {"summary", "per_size", "config"}  # today's key set
    assert "sim_mac" not in a["config"]
    assert set(a["config"]) == set(c["config"]) - {"sim_mac"}
    assert b["sim_mac"] == c["sim_mac"] == c["config"]["sim_mac"] == "mwis"
    for m in ("baseline", "local", "GNN"):
        for pa, pb, pc in ((a["summary"][m], b["summary"][m],
                            c["summary"][m]),
                           (a["per_size"]["20"][m], b["per_size"]["20"][m],
                            c["per_size"]["20"][m])):
            assert "sim_sched_share" not in pa and "sim_sched_share" not in pb
            assert set(pc) - set(pa) == {"sim_sched_share"}
            assert set(pb) < set(pa)
            for k, v in pa.items():
                if not k.startswith("sim_"):
                    assert pb[k] == v and pc[k] == v, (m, k)
            assert pc["sim_tasks"] > 0 and pc["sim_tasks"] == pb["sim_tasks"]
            assert pc["sim_tau"] == pb["sim_tau"] >= 1.0
    # the local method sends nothing over a link: 0 scheduled slots over 0
    # busy slots has no value, and the field says so
    assert np.isnan(c["summary"]["local"]["sim_sched_share"])
    assert c["summary"]["local"]["sim_link_util_max"] == 0.0
    for m in ("baseline", "GNN"):
        assert 0.0 < c["summary"][m]["sim_sched_share"] <= 1.0
        assert c["summary"][m]["sim_tau"] != a["summary"][m]["sim_tau"]
    with pytest.raises(SystemExit):
        ev.main(common[:-2] + ["--sim-mac", "mwis"])
