"""The tiled Floyd–Warshall kernels (fw64_phase1-3 for fp32 N > 200,
fw_phase1-3<double> for fp64 N > 143; ops/hip/fw.hip) against the fp64 oracle
on the inputs of tests/large_shape_cases.py: directed (asymmetric, so a
swapped row / column strip in phase 2 shows), two components and a sink (so
+inf cells, inf + inf and the +inf padding of partial tiles reach the output)
and integer weights, whose path sums are exact in both formats.  The integer
cases therefore assert equality, +inf positions included, with no tolerance.
tests/test_large_shape_inputs.py checks the inputs on the CPU."""
import pytest
import torch

from tests import large_shape_cases as lc

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")


def _ext():
    from multihop_offload_amd.ops import dispatch
    return dispatch.require_hip()


def _bits(x):
    return x.view(torch.int32 if x.dtype == torch.float32 else torch.int64)


def _tiled(dtype, N):
    """Does (B,N,N) of this dtype take the tiled kernels?"""
    if dtype == torch.float32:
        return N * ((N + 3) // 4 * 4) * 4 > lc.LDS_LIMIT
    return N * N * 8 > lc.LDS_LIMIT


def _n_arr(n_list):
    return torch.tensor(n_list, dtype=torch.int32, device="cuda")


@needs_gpu
@pytest.mark.parametrize("dtype,N", lc.FW_EXACT)
def test_tiled_kernels_equal_the_oracle_exactly(dtype, N):
    """Three distinct graphs per launch (blockIdx.z).  fp32: N = 201 is the
    first tiled N (4 tiles of 64, the last 9 wide), 257 leaves a tile 1 wide,
    320 is exact; fp64: N = 144 is the first over the LDS limit, 161 leaves a
    32-tile 1 wide, 192 is exact."""
    dtype = getattr(torch, dtype)
    assert _tiled(dtype, N)
    if N == 144:
        assert 144 * 144 * 8 > 160 * 1024 >= 143 * 143 * 8
    if N == 201:
        assert not _tiled(dtype, 200)
    w, _, want = lc.fw_oracle(N)
    wd = w.to(dtype).cuda()
    keep = wd.clone()
    got = _ext().floyd_warshall(wd, None)
    torch.cuda.synchronize()
    assert torch.equal(wd, keep)                 # the input is cloned
    assert got.dtype == dtype
    assert torch.equal(got.double().cpu(), want)


@needs_gpu
@pytest.mark.parametrize("dtype,N,n_list", lc.FW_PADDED)
def test_padded_graph_on_the_tiled_path(dtype, N, n_list):
    """One graph of the batch connects only its first n_real nodes.  With
    and without ``n_arr`` the result is the same bits and the oracle; pad
    cells are +inf off the diagonal and 0 on it."""
    dtype = getattr(torch, dtype)
    assert _tiled(dtype, N)
    w, _, want = lc.fw_oracle(N, 0, n_list)
    wd = w.to(dtype).cuda()
    ext = _ext()
    plain = ext.floyd_warshall(wd, None)
    with_n = ext.floyd_warshall(wd, _n_arr(n_list))
    torch.cuda.synchronize()
    assert torch.equal(_bits(plain), _bits(with_n))
    assert torch.equal(with_n.double().cpu(), want)
    eye = torch.eye(N, dtype=torch.bool, device="cuda")
    for b, n in enumerate(n_list):
        pad = torch.ones(N, N, dtype=torch.bool, device="cuda")
        pad[:n, :n] = False
        assert bool((with_n[b][pad & eye] == 0).all())
        off = with_n[b][pad & ~eye]
        assert bool((torch.isinf(off) & (off > 0)).all())
    assert int((~torch.isinf(with_n[1])).sum()) < \
        int((~torch.isinf(with_n[0])).sum())


@needs_gpu
@pytest.mark.parametrize("dtype,N,n_list", lc.FW_MASKED)
def test_masked_entry_falls_back_to_the_prepared_matrix(dtype, N, n_list):
    """floyd_warshall_dm on shapes its LDS kernel does not serve: fp32
    N = 201 and fp64 N = 144 prepare the matrix with torch and take the
    tiled kernels, fp64 N = 100 the in-place LDS kernel.  The raw matrix is
    NaN wherever ``adj`` is false; the result has no NaN, is bit-equal to
    the unmasked entry on the prepared matrix and equals the oracle."""
    dtype = getattr(torch, dtype)
    assert _tiled(dtype, N) == (N != 100)
    w, adj, want = lc.fw_oracle(N, 0, n_list)
    prepared = w.to(dtype).cuda()
    adj = adj.cuda()
    raw = torch.where(adj, prepared, torch.full_like(prepared, float("nan")))
    assert bool(torch.isnan(raw).any())
    ext = _ext()
    n_arr = _n_arr(n_list)
    got = ext.floyd_warshall_dm(raw, adj, n_arr)
    ref = ext.floyd_warshall(prepared, n_arr)
    torch.cuda.synchronize()
    assert got.dtype == dtype
    assert not bool(torch.isnan(got).any())
    assert torch.equal(_bits(got), _bits(ref))
    assert torch.equal(got.double().cpu(), want)


@needs_gpu
@pytest.mark.parametrize("dtype,N", lc.FW_REAL)
def test_non_integer_weights_within_the_rounding_bound(dtype, N):
    """Asymmetric uniform(0.01, 2) weights on the same structure.  A
    distance is a sum of at most N−1 positive terms, each addition rounds
    once and the minimum is monotone, so the relative error is below
    N·2⁻²⁴ (fp32) or N·2⁻⁵³ (fp64); +inf positions match exactly."""
    dtype = getattr(torch, dtype)
    assert _tiled(dtype, N)
    w, _, want = lc.fw_oracle(N, 1, None, False)
    got = _ext().floyd_warshall(w.to(dtype).cuda(), None).double().cpu()
    inf = torch.isinf(want)
    assert torch.equal(torch.isinf(got), inf)
    assert not bool(torch.isnan(got).any())
    rtol = N * (2.0 ** -24 if dtype == torch.float32 else 2.0 ** -53)
    err = ((got - want).abs() / want.clamp(min=1e-300))[~inf]
    print(f"{dtype} N={N}: max rel err {float(err.max()):.3e}, "
          f"bound {rtol:.3e}")
    assert bool(((got - want).abs()[~inf] <= rtol * want[~inf]).all())
