"""GPU (MI355X) tests of the one-workgroup-per-tensor fused Adam against the
single-workgroup kernel (``dispatch.adam_force_single_block``), bit for bit,
and of its step counter under hipGraph replay."""
import pytest
import torch

from tests.test_gpu_stages import needs_gpu

pytestmark = pytest.mark.gpu

W_BAD, B_BAD = 2, 5


def _model(which):
    from multihop_offload_amd.models.chebconv import ChebConvStack
    if which == "K2":
        m = ChebConvStack(K=2, dtype=torch.float32, seed=7)       # 10 tensors
    else:
        m = ChebConvStack(num_layer=9, K=3, dtype=torch.float32, seed=7)
    return m.cuda()


def _three_steps(which, constraints, single):
    """The three steps of test_fused_adam_three_steps_vs_fp32_replay (step 2:
    a NaN in a weight gradient, an inf in a bias gradient, that weight
    scaled past max_norm first).  Returns p, m, v, flat_g, step_dev after
    every step."""
    from multihop_offload_amd.ops import dispatch
    from multihop_offload_amd.ops.functions import FusedAdam

    model = _model(which)
    params = list(model.parameters())
    with torch.no_grad():
        params[B_BAD].fill_(0.1)
    opt = FusedAdam(model, lr=1e-3, constraints=constraints)
    gen = torch.Generator().manual_seed(0)
    out = []
    dispatch.adam_force_single_block(single)
    try:
        for t in (1, 2, 3):
            grads = [torch.randn(p.shape, generator=gen)
                     * (10.0 if i % 3 else 0.01)
                     for i, p in enumerate(params)]
            if t == 2:
                with torch.no_grad():
                    params[W_BAD].mul_(4.0)
                grads[W_BAD][1, 3, 5] = float("nan")
                grads[B_BAD][7] = float("inf")
            opt.zero_grad()
            for p, g in zip(params, grads):
                p.grad.copy_(g)
            opt.step(scale=0.5)
            torch.cuda.synchronize()
            assert int(opt._ticket) == 0
            out.append(tuple(x.clone() for x in (
                opt.flat_p, opt.m, opt.v, opt.flat_g, opt.step_dev)))
    finally:
        dispatch.adam_force_single_block(False)
    return out, len(params)


@needs_gpu
@pytest.mark.parametrize("constraints", [True, False])
@pytest.mark.parametrize("which,n_tensors", [("K2", 10), ("K3x9", 18)])
def test_adam_blocks_equal_single_block_bit_for_bit(which, n_tensors,
                                                    constraints):
    """p, m, v, the scaled gradient and step_dev after each of three steps,
    one workgroup per tensor against the single workgroup, as raw bits (NaN
    and inf in flat_g included), with and without the constraints, on the
    benchmark's model (10 tensors) and on a 9-layer K=3 stack (18 tensors:
    more than the single-block kernel's group of 16, and the K=3 pair
    path).  Both kernels compile the same adam_value; no tolerance is
    used."""
    new, n = _three_steps(which, constraints, single=False)
    old, _ = _three_steps(which, constraints, single=True)
    assert n == n_tensors
    for t, (a, b) in enumerate(zip(new, old), start=1):
        assert int(a[4]) == t and int(b[4]) == t
        for x, y, what in zip(a, b, ("p", "m", "v", "flat_g", "step_dev")):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), \
                (which, constraints, t, what)
        assert bool(torch.isfinite(a[0]).all())
    # step 2 really carried the non-finite gradients
    assert not bool(torch.isfinite(new[1][3]).all())


@needs_gpu
def test_adam_blocks_step_counter_survives_graph_replay():
    """One opt.step(scale=1.0) captured in a torch.cuda.graph and replayed
    three times: step_dev is 3, the ticket reads 0, and p / m / v equal
    three eager steps of a twin optimizer bit for bit (the gradient buffer
    is left alone: scale 1 rewrites it with itself)."""
    from multihop_offload_amd.ops.functions import FusedAdam

    gen = torch.Generator().manual_seed(1)
    opts = []
    for _ in range(2):
        model = _model("K2")
        opts.append((FusedAdam(model, lr=1e-3), list(model.parameters())))
    grads = [torch.randn(p.shape, generator=gen) * (3.0 if i % 2 else 0.05)
             for i, p in enumerate(opts[0][1])]
    for opt, params in opts:
        for p, g in zip(params, grads):
            p.grad.copy_(g)
    (cap, _), (twin, _) = opts
    assert torch.equal(cap.flat_p, twin.flat_p)

    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        cap.step(scale=1.0)
    torch.cuda.synchronize()
    assert int(cap.step_dev) == 0          # capture launches nothing
    for _ in range(3):
        graph.replay()
    for _ in range(3):
        twin.step(scale=1.0)
    torch.cuda.synchronize()
    assert int(cap.step_dev) == 3 and int(twin.step_dev) == 3
    assert int(cap._ticket) == 0 and int(twin._ticket) == 0
    for what in ("flat_p", "m", "v", "flat_g"):
        x, y = getattr(cap, what), getattr(twin, what)
        assert torch.equal(x.view(torch.int32), y.view(torch.int32)), what
