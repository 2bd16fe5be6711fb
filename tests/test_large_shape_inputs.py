"""The inputs of the top-of-range kernel tests
(tests/test_gpu_cheb_top_shapes.py, tests/test_gpu_fw_tiled.py), checked on
the fp64 CPU oracle alone: every recipe of tests/large_shape_cases.py reaches
the shape class it is meant for and can see the mistakes that class can make.
These are conditions on the inputs, not measurements of a kernel; a bad seed
fails here and never looks like a kernel failure."""
import numpy as np
import pytest
import torch
from scipy.sparse.csgraph import dijkstra

from tests import large_shape_cases as lc

CHEB = ([(Ee, K, True, None) for Ee, K in lc.ROW_TILED + lc.LDS_TOP]
        + [(Ee, K, False, None) for Ee, K in lc.UNSTAGED]
        + [(Ee, K, False, tile) for Ee, K, tile in lc.ONE_TILE]
        + [(Ee, K, padded, None) for Ee, K, padded in lc.GENERIC_K])


# ---------------------------------------------------------- Floyd–Warshall
FW = sorted({(N, None) for _, N in lc.FW_EXACT}
            | {(N, n_list) for _, N, n_list in lc.FW_PADDED + lc.FW_MASKED},
            key=str)


@pytest.mark.parametrize("N,n_list", FW)
def test_fw_integer_inputs(N, n_list):
    w, adj, want = lc.fw_oracle(N, 0, n_list)
    B = w.shape[0]
    eye = torch.eye(N, dtype=torch.bool)
    assert w.dtype == torch.float64 and want.dtype == torch.float64
    assert bool((w[:, eye] == 0).all()) and not bool(adj[:, eye].any())
    assert bool(torch.isinf(w[~adj & ~eye]).all())
    for b in range(B):
        # the oracle is Dijkstra's, exactly (non-edges as absent entries)
        dense = np.where(adj[b].numpy(), w[b].numpy(), 0.0)
        ref = dijkstra(dense, directed=True)
        assert np.array_equal(want[b].numpy(), ref)
        assert not torch.equal(w[b], w[b].T)
        n = N if n_list is None else n_list[b]
        real = torch.zeros(N, N, dtype=torch.bool)
        real[:n, :n] = True
        off = real & ~eye
        fin = torch.isfinite(want[b])
        # pad nodes are isolated
        assert not bool(fin[~real & ~eye].any())
        unreachable = float((~fin[off]).double().mean())
        improved = float((want[b] < w[b])[off & fin].double().mean())
        print(f"N={N} n={n} graph {b}: unreachable {unreachable:.3f}, "
              f"improved through a pivot {improved:.3f}, "
              f"largest distance {float(want[b][fin].max()):.0f}")
        assert 0.2 <= unreachable <= 0.7
        assert improved >= 0.5
        d = want[b][fin]
        assert bool((d == d.round()).all()) and float(d.max()) < 2 ** 24
    # distinct graphs: blockIdx.z picks the wrong one visibly
    assert not torch.equal(want[0], want[1])
    assert not torch.equal(want[1], want[2])


@pytest.mark.parametrize("dtype,N", lc.FW_REAL)
def test_fw_real_inputs(dtype, N):
    w, adj, want = lc.fw_oracle(N, 1, None, False)
    fin = adj
    assert bool((w[fin] >= 0.01).all()) and bool((w[fin] <= 2.0).all())
    assert torch.equal(w[fin], w[fin].float().double())     # fp32 holds them
    assert not bool((w[fin] == w[fin].round()).all())
    assert not torch.equal(w[0], w[0].T)
    inf = torch.isinf(want)
    assert 0.2 <= float(inf.double().mean()) <= 0.7


def test_fw_shapes_reach_the_tiled_kernels():
    lim = lc.LDS_LIMIT
    # fp32: the LDS kernel holds N rows of N rounded up to 4 floats
    assert 200 * 200 * 4 <= lim < 201 * 204 * 4
    assert 144 * 144 * 8 > lim >= 143 * 143 * 8
    assert [(N + 63) // 64 for _, N in lc.FW_EXACT[:3]] == [4, 5, 5]
    assert [N % 64 for _, N in lc.FW_EXACT[:3]] == [9, 1, 0]
    assert [N % 32 for _, N in lc.FW_EXACT[3:]] == [16, 1, 0]
    assert all(N * N * 8 > lim for _, N in lc.FW_EXACT[3:])
    for dtype, N, n_list in lc.FW_PADDED:
        assert N * N * (4 if dtype == "float32" else 8) > lim
        assert min(n_list) < N == max(n_list)
    # the masked entry's fp64 fallback onto the LDS kernel
    assert [(d, N) for d, N, _ in lc.FW_MASKED] == [
        ("float32", 201), ("float64", 144), ("float64", 100)]
    assert 100 * 100 * 8 <= lim


# ---------------------------------------------------------------- ChebConv
@pytest.mark.parametrize("Ee,K,padded,tile", CHEB)
def test_cheb_inputs_are_conditioned(Ee, K, padded, tile):
    c = lc.cheb_case(Ee, K, padded, tile)
    A, want, B = c["A"], c["want"], c["B"]
    print(f"Ee={Ee} K={K} padded={padded} tile={tile}: seed {c['seed']} "
          f"(+{c['seed'] - 1000 * Ee - K}), fp32-reference forward error "
          f"{c['fwd_err32']:.2e}, nearest pre-activation to its kink "
          f"{c['kink']:.2e}, fp32-reference dW / db error "
          f"{c['ref_err']['dW']:.2e} / {c['ref_err']['db']:.2e}")
    assert B == (3 if padded else 2)
    assert torch.equal(A, A.transpose(1, 2))
    assert bool(((A == 0) | (A == 1)).all())
    assert not bool(torch.diagonal(A, dim1=1, dim2=2).any())
    # the CSR is the adjacency
    dense = torch.zeros_like(A)
    ipt, cols = c["indptr"].numpy(), c["cols"].numpy()
    for b in range(B):
        for r in range(Ee):
            lo, hi = c["base"][b] + ipt[b, r], c["base"][b] + ipt[b, r + 1]
            dense[b, r, cols[lo:hi]] += 1.0
    assert torch.equal(dense, A)
    assert c["max_nnz"] == int(A.sum((1, 2)).max())
    assert 4.5 < float(A.sum(2)[0].mean()) < 6.5
    # weights carry the real shapes only; the kernels get what the oracle got
    assert c["W"].dtype == torch.float32 and c["bias"].dtype == torch.float32
    assert not bool(c["W"][0, :, lc.FIN:].any())
    assert not bool(c["W"][-1, :, :, 1:].any())
    assert not bool(c["bias"][-1, 1:].any())

    amax = want["acts"][:, 1:].abs().amax(dim=(0, 2, 3))
    assert bool(((amax > 0.1) & (amax < 10.0)).all()), amax
    share = (want["lam"] > 0).double().mean(1)
    assert bool(((share >= 0.3) & (share <= 0.7)).all()), share
    for k in ("dW", "db"):
        assert bool((want[k].abs().reshape(B, lc.L, -1).amax(2) > 0).all())
    cond = lc.db_condition(want)
    print(f"largest db condition {float(cond.max()):.2f}")
    assert float(cond.max()) <= lc.DB_COND
    assert c["kink"] > lc.KINK >= 4.0 * c["fwd_err32"]
    for k in ("dW", "db"):
        assert c["tol"][k] == min(8.0 * max(c["ref_err"][k], 2.0 ** -24),
                                  5e-3)
        assert c["ref_err"][k] < 1e-4       # the recipe is well conditioned
    if K > 1:
        # the oracle's saved terms are the recurrence on its own activations
        tks, h = want["tks"], want["acts"][:, :lc.L]
        assert tuple(tks.shape) == (B, lc.L, K - 1, Ee, lc.F)
        terms = [h, A[:, None] @ h]
        for k in range(2, K):
            terms.append(2.0 * (A[:, None] @ terms[-1]) - terms[-2])
        assert torch.allclose(tks, torch.stack(terms[1:], 2), rtol=0,
                              atol=1e-12 * float(tks.abs().max()))
        print(f"largest term {float(tks.abs().max()):.3e}, fp32-reference "
              f"error of the terms {c['tks_err32']:.3f} of the forward bound")
        assert c["tks_err32"] < 1.0

    if padded:
        empty = lc.empty_rows(Ee, 1, True)
        band = empty[:-lc.TAIL]
        assert list(empty[-lc.TAIL:]) == list(range(Ee - lc.TAIL, Ee))
        # the band lies within the rows before the tail, across a tile edge
        assert band[-1] + 1 < Ee - lc.TAIL
        assert band[0] // 64 + 1 == band[-1] // 64 and band[0] % 64 != 0
        assert not bool(A[1, empty].any()) and not bool(c["x"][1, empty].any())
        assert len(lc.empty_rows(Ee, 0, True)) == 0
        assert bool((A[0].sum(1) > 0).sum() > (A[1].sum(1) > 0).sum())
        # an empty row's first activation is act(bias); deeper ones follow
        # from it through W_0 alone and are the same in every empty row
        act = torch.nn.functional.leaky_relu(c["bias"][0].double(), 0.2)
        assert torch.equal(want["acts"][1, 1, empty],
                           act.expand(len(empty), -1))
        assert torch.allclose(want["acts"][1, :, empty],
                              want["acts"][1, :, empty[:1]].expand(
                                  -1, len(empty), -1), rtol=1e-12, atol=0)
    if tile is not None:
        rows = lc._tile_rows(Ee, tile)
        assert len(rows) == (64 if tile == "first" else 5)
        live = torch.zeros(Ee, dtype=torch.bool)
        live[rows] = True
        assert not bool(c["dlam"][:, ~live].any())
        assert bool(((want["lam"] > 0) & (c["dlam"] != 0))[:, live]
                    .any(1).all())


def test_cheb_shapes_reach_the_documented_paths():
    # the switch points between the LDS-resident and the row-tiled kernels
    for K, top in ((2, 384), (1, 400), (3, 368)):
        assert lc.fits_lds(top, K) and not lc.fits_lds(top + 1, K)
    for Ee, K in lc.LDS_TOP:
        assert lc.fits_lds(Ee, K)
    assert [Ee for Ee, K in lc.LDS_TOP if not lc.fits_lds(Ee + 1, K)] == \
        [384, 400, 368]
    assert not lc.fits_lds(385, 2)
    # row tiles: one-row last tile, exact tiles, the first production shape
    assert [((Ee + 63) // 64, Ee % 64) for Ee in (129, 192, 385)] == \
        [(3, 1), (3, 0), (7, 1)]
    assert [((Ee + 63) // 64, Ee % 64) for Ee in (133, 389)] == \
        [(3, 5), (7, 5)]
    # 24 or more MFMA row tiles over 8 waves at the top shapes
    assert all(lc.lds_plan(Ee, K, 3, False, 0)["rows_pad"] // 16 >= 23
               for Ee, K in lc.LDS_TOP)
    assert lc.lds_plan(377, 2, 3, False, 0)["rows_pad"] == 384
    # K=2, Ee=384: 3584 bytes are left in the backward, 44544 in the forward
    bwd = lc.lds_plan(384, 2, 3, False, 0)
    assert lc.LDS_LIMIT - bwd["lds_bytes"] + 4 * 385 == 3584
    nnz = lc.cheb_case(384, 2)["max_nnz"]
    plans = lc.lds_plans(384, 2, nnz)
    assert 4 * (385 + nnz) > 3584
    assert plans["bwd"]["stage_csr"] == 0 and plans["fwd"]["stage_csr"] == 1
    assert plans["bwd"]["fits"] and plans["fwd"]["fits"]
    # every top shape runs its backward unstaged at its own max_nnz
    for Ee, K in lc.LDS_TOP:
        p = lc.lds_plans(Ee, K, lc.cheb_case(Ee, K)["max_nnz"])
        assert p["kn_bwd" if K > 2 else "bwd"]["stage_csr"] == 0, (Ee, K)
    # generic K past 3: the reverse recurrence of the backward runs K - 2
    # times, twice or more and on both parities; the two top shapes are the
    # largest of their K and alone run the backward unstaged
    assert sorted({K for _, K, _ in lc.GENERIC_K}) == [4, 5, 6]
    assert all(K - 2 >= 2 for _, K, _ in lc.GENERIC_K)
    for K, top in ((4, 368), (5, 352)):
        assert lc.fits_lds(top, K) and not lc.fits_lds(top + 1, K)
        assert (top, K) in lc.GENERIC_K_TOP
    assert {(Ee, K) for Ee, K, _ in lc.GENERIC_K} >= set(lc.GENERIC_K_TOP)
    for Ee, K, padded in lc.GENERIC_K:
        assert lc.fits_lds(Ee, K)
        p = lc.lds_plans(Ee, K, lc.cheb_case(Ee, K, padded)["max_nnz"])
        assert p["kn_fwd"]["fits"] and p["kn_bwd"]["fits"]
        assert p["kn_bwd"]["stage_csr"] == \
            (0 if (Ee, K) in lc.GENERIC_K_TOP else 1), (Ee, K)
    assert [(Ee + 63) // 64 for Ee, _, padded in lc.GENERIC_K if padded] == \
        [3, 3, 6]
    # the small shape stages everything at its own max_nnz and nothing at
    # the inflated one the unstaged test passes
    for Ee, K in lc.UNSTAGED:
        nnz = lc.cheb_case(Ee, K, False)["max_nnz"]
        assert all(p["stage_csr"] == 1 and p["fits"]
                   for p in lc.lds_plans(Ee, K, nnz).values())
        assert all(p["stage_csr"] == 0 and p["fits"]
                   for p in lc.lds_plans(Ee, K, lc.INFLATED_NNZ).values())
        assert lc.INFLATED_NNZ > nnz
