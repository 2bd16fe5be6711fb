"""The register-resident Floyd–Warshall kernel (fp32, N <= 128) against the
in-place LDS kernel it replaces on those shapes: the two run the same
fminf(cur, dik + dkj) per pivot in the same order, so every output is compared
bit for bit (``dispatch.fw_force_inplace`` selects the old kernel)."""
import contextlib

import pytest
import torch

pytestmark = pytest.mark.gpu

needs_gpu = pytest.mark.skipif(not torch.cuda.is_available(),
                               reason="no GPU")

B = 3
COVERED = [1, 2, 5, 17, 33, 100, 110, 128]
FIRST_UNCOVERED = 129


def _ext():
    from multihop_offload_amd.ops import dispatch
    return dispatch.require_hip()


@contextlib.contextmanager
def inplace():
    from multihop_offload_amd.ops import dispatch
    dispatch.fw_force_inplace(True)
    try:
        yield
    finally:
        dispatch.fw_force_inplace(False)


def _weights(N, n_list=None, seed=0):
    """(B,N,N) fp32 on the GPU: positive random weights, about half the
    off-diagonal cells +inf, 0 on the diagonal; with ``n_list`` the rows and
    columns from n_b on are pads (+inf, 0 on the diagonal); node N-1 has no
    outgoing link, so some pairs stay unreachable.  Returns the
    prepared matrix, the raw matrix with NaN wherever ``adj`` is false (what
    the masked entry is given), ``adj`` and ``n_arr``."""
    g = torch.Generator().manual_seed(1000 * N + seed)
    w = torch.rand(B, N, N, generator=g) * 9.0 + 0.5
    adj = torch.rand(B, N, N, generator=g) < 0.5
    idx = torch.arange(N)
    adj[:, idx, idx] = False
    if N >= 3:
        adj[:, N - 1, :] = False             # a sink: nothing reachable from it
    n_arr = None
    if n_list is not None:
        for b, n in enumerate(n_list):
            adj[b, n:, :] = False
            adj[b, :, n:] = False
        n_arr = torch.tensor(n_list, dtype=torch.int32, device="cuda")
    prepared = torch.where(adj, w, torch.full_like(w, float("inf")))
    prepared[:, idx, idx] = 0.0
    raw = torch.where(adj, w, torch.full_like(w, float("nan")))
    return prepared.cuda(), raw.cuda(), adj.cuda(), n_arr


def _both(N, n_list=None):
    """{unmasked, masked} outputs of the kernel chosen by shape and of the
    forced in-place kernel."""
    ext = _ext()
    w, raw, adj, n_arr = _weights(N, n_list)
    w_before = w.clone()

    def run():
        return {"unmasked": ext.floyd_warshall(w, n_arr),
                "masked": ext.floyd_warshall_dm(raw, adj, n_arr)}
    got = run()
    with inplace():
        assert ext.fw_register_rows(N) == 0
        want = run()
    torch.cuda.synchronize()
    assert torch.equal(w, w_before)          # the input is cloned, not used
    return got, want, n_arr


def _bits(x):
    return x.view(torch.int32)


@needs_gpu
@pytest.mark.parametrize("N", COVERED + [FIRST_UNCOVERED])
def test_register_kernel_equals_inplace_kernel(N):
    ext = _ext()
    covered = ext.fw_register_rows(N) > 0
    assert covered == (N in COVERED)         # 129 takes the old kernel
    got, want, _ = _both(N)
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    assert torch.equal(_bits(got["masked"]), _bits(got["unmasked"]))
    if N >= 3:
        # some pairs stay unreachable (the sink's row), some were reached
        # through a pivot (finite where the input had +inf)
        inf = torch.isinf(got["masked"])
        assert bool(inf[:, N - 1, :N - 1].all())
        w = _weights(N)[0]
        assert bool((torch.isinf(w) & ~inf).any())


@needs_gpu
@pytest.mark.parametrize("N,n_list", [(33, [1, 2, 33]),
                                      (110, [20, 77, 110])])
def test_ragged_n_arr(N, n_list):
    assert _ext().fw_register_rows(N) > 0
    got, want, n_arr = _both(N, n_list)
    for k in want:
        assert torch.equal(_bits(got[k]), _bits(want[k])), k
    m = got["masked"]
    for b, n in enumerate(n_list):
        pad = torch.ones(N, N, dtype=torch.bool, device="cuda")
        pad[:n, :n] = False
        eye = torch.eye(N, dtype=torch.bool, device="cuda")
        assert bool((m[b][pad & eye] == 0).all())
        assert bool(torch.isinf(m[b][pad & ~eye]).all())
        assert bool((m[b][pad & ~eye] > 0).all())


@needs_gpu
def test_register_kernel_vs_fp64_reference():
    """Tolerance of tests/test_gpu.py::test_fw_lds_kernel_vs_ref."""
    from multihop_offload_amd.ops import dispatch, torch_ref
    from tests.test_gpu import _rand_w
    w = _rand_w(8, 100)
    assert _ext().fw_register_rows(100) > 0
    want = torch_ref.floyd_warshall(w.double())
    got = dispatch.floyd_warshall(w.cuda()).cpu()
    assert torch.allclose(got.double(), want, rtol=1e-5, atol=1e-5)


@needs_gpu
def test_fp64_keeps_the_inplace_kernel():
    """fp64 input is served by fw_lds_kernel<double> whatever the switch
    says: same bits with the register kernel on and off, on both entries."""
    ext = _ext()
    w, raw, adj, _ = _weights(100)
    w64, raw64 = w.double(), raw.double()
    got = (ext.floyd_warshall(w64, None),
           ext.floyd_warshall_dm(raw64, adj, None))
    with inplace():
        want = (ext.floyd_warshall(w64, None),
                ext.floyd_warshall_dm(raw64, adj, None))
    torch.cuda.synchronize()
    for g, x in zip(got, want):
        assert g.dtype == torch.float64
        assert torch.equal(g.view(torch.int64), x.view(torch.int64))
    # and it is the fp64 result, not a rounded fp32 one
    from multihop_offload_amd.ops import torch_ref
    ref = torch_ref.floyd_warshall(w64.cpu())
    assert torch.allclose(got[0].cpu(), ref, rtol=1e-12, atol=1e-12)


@needs_gpu
@pytest.mark.parametrize("N", [17, 100])
def test_nan_cells_propagate_as_in_the_inplace_kernel(N):
    """The register kernel takes its minimum with a bare v_min_f32 on cells
    canonicalised at load; NaN weights (quiet, as torch writes them) must
    come out exactly as through fminf in the in-place kernel."""
    ext = _ext()
    w = _weights(N)[0]
    g = torch.Generator().manual_seed(N)
    nan = (torch.rand(B, N, N, generator=g) < 0.05).cuda()
    nan &= ~torch.eye(N, dtype=torch.bool, device="cuda")
    w = torch.where(nan, torch.full_like(w, float("nan")), w)
    got = ext.floyd_warshall(w, None)
    with inplace():
        want = ext.floyd_warshall(w, None)
    torch.cuda.synchronize()
    assert torch.equal(_bits(got), _bits(want))
