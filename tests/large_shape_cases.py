"""Inputs and fp64 oracles for the kernel tests at the top of the shape
ranges (tests/test_gpu_cheb_top_shapes.py, tests/test_gpu_fw_tiled.py).
CPU only; tests/test_large_shape_inputs.py checks every recipe here on the
oracle alone, so a badly conditioned seed fails there, as an input problem.

ChebConv.  The kernels read the support only as a CSR (indptr (B,Ee+1) int32,
base (B) int64, cols int32, max_nnz), so the adjacencies are built directly:
symmetric 0/1, mean degree about 6, any Ee, no 400-node engine.  In a padded
batch graph 1 has an empty band of rows across a 64-row tile boundary and an
empty tail of 30 rows, the layout engine.py gives ragged batches.  The oracle
is the dense fp64 recurrence and autograd of ``_cheb_family_case``
(tests/test_gpu.py) with its weight scale from the spectrum of A, the weights
zero-padded to the real shapes (4→32, 32→32, 32→1) as the edge-layer tests
do, and two conditioning steps: every layer's weights are rescaled so its
pre-activation max-abs lies in [0.5, 3], and the last layer's bias[0] is
shifted by the fp64 median of column 0's pre-activation over the rows that
have neighbours, so that about half of lam is positive.  dlam is N(1, 1), so
that the last layer's db is not a cancelling sum.  The builder walks
seeds until the conditions the CPU tests assert hold with margin, among them
that no pre-activation lies within 2^-17 of the kink of its activation, four
times the fp32 reference's forward error or more: a mask bit flipped by
rounding is not a kernel error.

Floyd–Warshall.  Directed graphs of out-degree 3 with integer weights 1..15,
the nodes randomly permuted into two components (70% / 30%), one sink reached
from the first; diagonal 0, non-edges +inf, optionally only the first n_real
nodes connected.  Every path sum is a small integer, exact in fp32 and fp64:
the kernels must reproduce the fp64 oracle bit for bit.
"""
import functools

import numpy as np
import torch

from multihop_offload_amd.ops import torch_ref

L, F, FIN = 5, 32, 4
LDS_LIMIT = 160 * 1024
TAIL = 30               # empty rows at the end of graph 1 of a padded batch
# Nearest a pre-activation may come to zero: 128 fp32 roundings of an O(1)
# value.  The fp32 reference's forward error is a quarter of it at the most
# (asserted by the CPU tests), so rounding flips no activation mask.
KINK = 2.0 ** -17
# Largest db_condition a case may have.  The last layer's db is one sum over
# the rows with lam > 0; with a zero-mean dlam it cancels to a few percent of
# its addends and the figure shows the summation order (sequential chunks and
# unordered atomics in the kernels, pairwise in the fp32 reference: up to 9x
# apart on an MI355X), not the kernel.  dlam is therefore drawn with mean 1.
DB_COND = 8.0
SEED_TRIES = 100


# ---------------------------------------------------------------- LDS plan
def lds_plan(Ee, K, nbuf, with_bias, max_nnz):
    """The closed form of the LDS-resident launchers' plan, stated
    independently: nbuf row buffers of rows_pad×33 floats, K 32×32 weight
    matrices, 32 bias floats where the kernel stages them, and the support
    CSR (Ee+1 row pointers, max_nnz columns) when that still fits."""
    rows_pad = (Ee + 15) // 16 * 16
    nbytes = 4 * (nbuf * rows_pad * 33 + K * 1024 + (32 if with_bias else 0))
    csr = 4 * (Ee + 1 + max_nnz)
    stage = nbytes + csr <= LDS_LIMIT
    return dict(rows_pad=rows_pad, lds_bytes=nbytes + (csr if stage else 0),
                stage_csr=int(stage), fits=nbytes <= LDS_LIMIT)


def lds_plans(Ee, K, max_nnz):
    """What ``dispatch.cheb_lds_plan`` must return."""
    return dict(fwd=lds_plan(Ee, K, 2, True, max_nnz),
                bwd=lds_plan(Ee, K, 3, False, max_nnz),
                kn_fwd=lds_plan(Ee, K, 3, True, max_nnz),
                kn_bwd=lds_plan(Ee, K, 3, False, max_nnz))


def fits_lds(Ee, K):
    """The routing decision of ``cheb_fits_lds``."""
    nbuf = 3 if K > 2 else 2
    return (lds_plan(Ee, K, nbuf, True, 0)["fits"]
            and lds_plan(Ee, K, 3, False, 0)["fits"])


# ------------------------------------------------------------ support CSR
def empty_rows(Ee, b, padded):
    """Rows of graph b without neighbours and with zero features."""
    if not padded or b != 1:
        return np.zeros(0, dtype=np.int64)
    # rows 120..139 where Ee has room for them, else rows 60..67: with the
    # tail no more than 30% of the rows, so lam > 0 on 30..70% of all rows
    # stays reachable with one bias for the batch
    band = np.arange(120, 140) if Ee >= 192 else np.arange(60, 68)
    assert band[-1] + 8 < Ee - TAIL
    return np.concatenate([band, np.arange(Ee - TAIL, Ee)])


def support(Ee, B, seed, padded):
    """Dense symmetric 0/1 adjacencies (B,Ee,Ee) fp64 and their CSR."""
    rng = np.random.RandomState(seed)
    A = np.zeros((B, Ee, Ee))
    for b in range(B):
        real = np.setdiff1d(np.arange(Ee), empty_rows(Ee, b, padded))
        m = 3 * len(real)                    # mean degree about 6
        i = real[rng.randint(0, len(real), size=m)]
        j = real[rng.randint(0, len(real), size=m)]
        keep = i != j
        A[b, i[keep], j[keep]] = 1.0
        A[b, j[keep], i[keep]] = 1.0
    indptr = np.zeros((B, Ee + 1), dtype=np.int32)
    base = np.zeros(B, dtype=np.int64)
    cols = []
    for b in range(B):
        base[b] = sum(len(c) for c in cols)
        r, c = np.nonzero(A[b])
        indptr[b, 1:] = np.cumsum(np.bincount(r, minlength=Ee))
        cols.append(c.astype(np.int32))
    max_nnz = int(indptr[:, -1].max())
    return (torch.from_numpy(A), torch.from_numpy(indptr),
            torch.from_numpy(base), torch.from_numpy(np.concatenate(cols)),
            max_nnz)


# ------------------------------------------------------------------ oracle
def cheb_stack(A, x, W, bias, dlam, dtype):
    """The Chebyshev recurrence of models/chebconv.py, dense per graph, in
    ``dtype``; dW (B,L,K,32,32) and db (B,L,32) per graph from autograd of
    sum(lam·dlam).  Returns lam, the (B,L+1,Ee,32) activations, the
    (B,L,K-1,Ee,32) Chebyshev terms T_1..T_{K-1} of every layer's input
    (None at K = 1), the (B,L,Ee,32) pre-activations and their gradients
    delta, dW, db."""
    B, Ee = x.shape[:2]
    K = W.shape[1]
    A = A.to(dtype)
    Wd = W.to(dtype).unsqueeze(0).repeat(B, 1, 1, 1, 1).requires_grad_()
    bd = bias.to(dtype).unsqueeze(0).repeat(B, 1, 1).requires_grad_()
    h = torch.zeros(B, Ee, F, dtype=dtype)
    h[:, :, :FIN] = x.to(dtype)
    acts, pres, tks = [h], [], []
    for l in range(L):
        out = h @ Wd[:, l, 0]
        if K > 1:
            t_prev, t_cur = h, A @ h
            terms = [t_cur]
            out = out + t_cur @ Wd[:, l, 1]
            for k in range(2, K):
                t_prev, t_cur = t_cur, 2.0 * (A @ t_cur) - t_prev
                terms.append(t_cur)
                out = out + t_cur @ Wd[:, l, k]
            tks.append(torch.stack(terms, 1).detach())
        out = out + bd[:, l].unsqueeze(1)
        out.retain_grad()
        pres.append(out)
        h = (torch.relu(out) if l == L - 1
             else torch.nn.functional.leaky_relu(out, 0.2))
        acts.append(h)
    lam = h[:, :, 0]
    (lam * dlam.to(dtype)).sum().backward()
    return dict(lam=lam.detach(), acts=torch.stack(acts, 1).detach(),
                tks=torch.stack(tks, 1) if K > 1 else None,
                pres=torch.stack(pres, 1).detach(),
                delta=torch.stack([p.grad for p in pres], 1),
                dW=Wd.grad, db=bd.grad)


def db_condition(want):
    """Per (graph, layer), for the entry of db that its error figure is
    normalised by: sum_r |delta[r][j]| / |sum_r delta[r][j]|.  Rounding puts
    about 2^-24 of the numerator into the sum whatever the order, so this is
    how many roundings the figure can show."""
    db = want["db"]
    j = db.abs().argmax(2, keepdim=True)
    num = want["delta"].abs().sum(2).gather(2, j)[..., 0]
    return num / db.abs().amax(2)


def grad_errors(got, want):
    """Per (graph, layer): max-abs error / oracle max-abs, as a (B,L) fp64
    tensor — the figure of the stage tests."""
    got = got.double().cpu()
    assert got.shape == want.shape
    B, Lw = want.shape[:2]
    err = (got - want).abs().reshape(B, Lw, -1).amax(2)
    den = want.abs().reshape(B, Lw, -1).amax(2)
    assert bool((den > 0).all())
    return err / den


def _conditioned_weights(A, x, K, gen):
    """W (L,K,32,32) and bias (L,32) in fp32: the family case's draw and
    spectral scale, zero-padded to the real shapes, then conditioned layer
    by layer on the fp64 forward."""
    B, Ee = x.shape[:2]
    ev = torch.linalg.eigvalsh(A)
    tk = [torch.ones_like(ev), ev]
    for k in range(2, K):
        tk.append(2.0 * ev * tk[-1] - tk[-2])
    W = torch.randn(L, K, F, F, generator=gen).double()
    for k in range(K):
        W[:, k] *= 2.0 / (K * F ** 0.5 * float(tk[k].abs().max()))
    bias = (0.1 * torch.randn(L, F, generator=gen)).double()
    W[0, :, FIN:, :] = 0.0
    W[L - 1, :, :, 1:] = 0.0
    bias[L - 1, 1:] = 0.0
    has_nb = A.sum(2) > 0                                   # (B,Ee)
    h = torch.zeros(B, Ee, F, dtype=torch.float64)
    h[:, :, :FIN] = x.double()
    for l in range(L):
        def pre():
            out = h @ W[l, 0]
            if K > 1:
                t_prev, t_cur = h, A @ h
                out = out + t_cur @ W[l, 1]
                for k in range(2, K):
                    t_prev, t_cur = t_cur, 2.0 * (A @ t_cur) - t_prev
                    out = out + t_cur @ W[l, k]
            return out
        amax = float(pre().abs().max())
        W[l] *= min(max(amax, 0.5), 3.0) / amax
        W[l] = W[l].float().double()                        # what fp32 holds
        out = pre()
        if l == L - 1:
            # midway between the two central values: on none of them
            v = (out[:, :, 0] + bias[l, 0])[has_nb].sort().values
            bias[l, 0] -= 0.5 * float(v[len(v) // 2 - 1] + v[len(v) // 2])
            bias[l] = bias[l].float().double()
        out = out + bias[l]
        h = (torch.relu(out) if l == L - 1
             else torch.nn.functional.leaky_relu(out, 0.2))
    return W.float(), bias.float()


def _tile_rows(Ee, tile):
    """Rows of the first or the last 64-row tile."""
    if tile == "first":
        return np.arange(0, min(64, Ee))
    return np.arange((Ee - 1) // 64 * 64, Ee)


def _try_cheb_case(Ee, K, padded, tile, seed):
    B = 3 if padded else 2
    A, indptr, base, cols, max_nnz = support(Ee, B, seed, padded)
    gen = torch.Generator()
    gen.manual_seed(seed)
    x = torch.randn(B, Ee, FIN, generator=gen)
    dlam = 1.0 + torch.randn(B, Ee, generator=gen)
    for b in range(B):
        x[b, empty_rows(Ee, b, padded)] = 0.0
    if tile is not None:
        keep = torch.zeros(Ee, dtype=torch.bool)
        keep[_tile_rows(Ee, tile)] = True
        dlam = dlam * keep
    W, bias = _conditioned_weights(A, x, K, gen)
    want = cheb_stack(A, x, W, bias, dlam, torch.float64)
    ref32 = cheb_stack(A, x, W, bias, dlam, torch.float32)

    # conditions, each with margin to what the CPU tests assert
    amax = want["acts"][:, 1:].abs().amax(dim=(0, 2, 3))
    if not bool(((amax > 0.15) & (amax < 8.0)).all()):
        return None
    share = (want["lam"] > 0).double().mean(1)
    if not bool(((share > 0.33) & (share < 0.67)).all()):
        return None
    if tile is not None:
        alive = want["lam"][:, _tile_rows(Ee, tile)] > 0
        if not bool(alive.any(1).all()):
            return None
    for k in ("dW", "db"):
        if not bool((want[k].abs().reshape(B, L, -1).amax(2) > 0).all()):
            return None
    if float(db_condition(want).max()) >= 0.75 * DB_COND:
        return None
    # no pre-activation within KINK of the kink of its activation (exact
    # zeros are the zero-padded columns: the same zero in every precision)
    fwd_err32 = float((ref32["pres"].double() - want["pres"]).abs().max())
    pres = want["pres"].abs()
    kink = float(pres[pres > 0].min())
    if kink <= KINK:
        return None
    ref_err = {k: float(grad_errors(ref32[k], want[k]).max())
               for k in ("dW", "db")}
    tol = {k: min(8.0 * max(v, 2.0 ** -24), 5e-3) for k, v in ref_err.items()}
    case = dict(Ee=Ee, K=K, B=B, padded=padded, tile=tile, seed=seed, A=A,
                indptr=indptr, base=base, cols=cols, max_nnz=max_nnz, x=x,
                dlam=dlam, W=W, bias=bias, want=want,
                dmax=float(A.sum(2).max()), fwd_err32=fwd_err32, kink=kink,
                ref_err=ref_err, tol=tol, tks_err32=None)
    if K > 1:
        # the fp32 reference's Chebyshev terms, as a share of the forward
        # bound (the terms grow like the spectrum of A to the power k)
        err = (ref32["tks"].double() - want["tks"]).abs()
        case["tks_err32"] = float((err / fwd_bound(case, want["tks"])).max())
    return case


@functools.lru_cache(maxsize=None)
def cheb_case(Ee, K, padded=True, tile=None):
    """The conditioned case of this shape: the first seed from
    1000·Ee + K on that meets every condition.  ``tile`` ("first"/"last")
    keeps dlam on the rows of that 64-row tile only.  Gradient tolerances:
    ``tol[name]`` is 8× the fp32 reference's own error ``ref_err[name]``
    (worst (graph, layer); floored at one fp32 rounding), at most 5e-3."""
    seed0 = 1000 * Ee + K
    for seed in range(seed0, seed0 + SEED_TRIES):
        case = _try_cheb_case(Ee, K, padded, tile, seed)
        if case is not None:
            return case
    raise AssertionError(f"no conditioned seed for Ee={Ee} K={K} "
                         f"padded={padded} tile={tile}")


def fwd_bound(case, want):
    """Per-element forward bound of test_cheb_kernel_families_agree."""
    amax = float(case["want"]["acts"].abs().max())
    atol = 5 * (case["K"] * 32 + case["dmax"]) * 2.0 ** -24 * amax
    return atol + 1e-3 * want.abs()


ROW_TILED = [(Ee, K) for Ee in (129, 192, 385) for K in (1, 2)]
LDS_TOP = [(377, 2), (384, 2), (400, 1), (368, 3)]
UNSTAGED = [(85, 2), (85, 3)]          # B=2, unpadded
# generic-K kernels past K = 3 (Ee, K, padded): the backward's reverse
# recurrence runs K - 2 times, so an even and an odd K end on opposite
# buffers; three row tiles with the empty band; the largest Ee the
# LDS-resident family accepts at K = 4 and K = 5
GENERIC_K = [(85, 4, False), (85, 5, False), (129, 4, True), (129, 5, True),
             (368, 4, True), (352, 5, False), (61, 6, False)]
GENERIC_K_TOP = [(368, 4), (352, 5)]
# a max_nnz whose CSR alone exceeds the LDS: every plan reads the CSR from
# global memory.  The kernels copy or read only the true indptr[Ee] entries.
INFLATED_NNZ = 1 << 16
ONE_TILE = [(Ee, K, tile) for Ee in (133, 389) for K in (1, 2)
            for tile in ("first", "last")]


# ---------------------------------------------------------- Floyd–Warshall
def fw_case(N, seed=0, n_list=None, integer=True, B=3):
    """(w, adj): w (B,N,N) fp64 prepared weights (0 diagonal, +inf
    non-edges), adj the boolean link mask.  Graph b connects its first
    n_list[b] nodes only (default all N).  Non-integer weights are
    uniform(0.01, 2) rounded to fp32."""
    rng = np.random.RandomState(100000 + 1000 * N + seed)
    w = np.full((B, N, N), np.inf)
    for b in range(B):
        n = N if n_list is None else n_list[b]
        perm = rng.permutation(n)
        na = int(round(0.7 * n))
        comp_a, comp_b = perm[:na], perm[na:]
        sink = comp_a[-1]
        for comp in (comp_a, comp_b):
            for u in comp:
                if u == sink:
                    continue
                others = comp[comp != u]
                for v in rng.choice(others, size=3, replace=False):
                    w[b, u, v] = (rng.randint(1, 16) if integer else
                                  np.float32(rng.uniform(0.01, 2.0)))
    adj = np.isfinite(w)
    idx = np.arange(N)
    w[:, idx, idx] = 0.0
    return torch.from_numpy(w), torch.from_numpy(adj)


@functools.lru_cache(maxsize=None)
def fw_oracle(N, seed=0, n_list=None, integer=True):
    """The case and its fp64 shortest distances (torch_ref)."""
    w, adj = fw_case(N, seed, n_list, integer)
    return w, adj, torch_ref.floyd_warshall(w)


FW_EXACT = [("float32", 201), ("float32", 257), ("float32", 320),
            ("float64", 144), ("float64", 161), ("float64", 192)]
FW_PADDED = [("float32", 320, (320, 280, 320)),
             ("float64", 192, (192, 150, 192))]
FW_MASKED = [("float32", 201, (201, 150, 201)),
             ("float64", 144, (144, 100, 144)),
             ("float64", 100, (100, 70, 100))]
FW_REAL = [("float32", 201), ("float64", 144)]
