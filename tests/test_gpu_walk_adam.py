"""GPU (MI355X) tests of walk_eval's neighbour scan (first minimum in
ascending CSR order on an exact tie) and of the fused Adam that takes all
its norms from one tree."""
import numpy as np
import pytest
import torch

from tests import stage_oracle as so
from tests.test_gpu_stages import _ext, _f32, _gpu_engine, needs_gpu

pytestmark = pytest.mark.gpu

@needs_gpu
def test_walk_exact_tie_takes_the_lower_neighbour():
    """Set A, graph 0: node 3 has 12 neighbours (ascending ids).  One job is
    made to start there, and the neighbours at CSR positions 2 and 9 get one
    bit-equal distance to the job's destination, half of every other
    neighbour's: the first hop takes the link to the lower id, and
    route_links, nhop and the overflow count equal engine.route_walk's on
    the same inputs."""
    e64, eg, fr = so.engine("A"), _gpu_engine("A"), so.front("A")
    case = so.cases("A")[0]
    deg = np.diff(case.adj_indptr)
    h = int(deg.argmax())
    lo, hi = int(case.adj_indptr[h]), int(case.adj_indptr[h + 1])
    nbrs = [int(x) for x in case.adj_indices[lo:hi]]
    assert len(nbrs) > 9 and nbrs == sorted(nbrs)
    n1, n2 = nbrs[2], nbrs[9]
    d = next(n for n in range(e64.N) if n != h and n not in nbrs)
    j0 = int(torch.nonzero(fr["jobs"].mask[0])[0])
    jobs = so.jobs_to(fr["jobs"], "cpu", torch.float64)
    jobs.sources = jobs.sources.clone()
    jobs.sources[0, j0] = h
    dst = fr["dst"].clone()
    dst[0, j0] = d
    sp = fr["sp"].clone()
    v = so.as32(0.5 * sp[0, nbrs, d].min())
    assert float(v) > 0
    sp[0, n1, d] = sp[0, n2, d] = v
    e64.overflow_total.zero_()
    with torch.no_grad():
        rl, nhop = e64.route_walk(jobs, dst, sp)
    overflow = int(e64.overflow_total)
    e64.overflow_total.zero_()
    want_rl = so.pad_routes(rl, fr["H"])
    assert int(want_rl[0, j0, 0]) == int(case.adj_link_ids[lo + 2])

    jg = so.jobs_to(jobs, "cuda", torch.float32)
    out = _ext().walk_eval(
        _f32(sp), jg.sources, dst.cuda().contiguous(), jg.mask,
        jg.rates.contiguous(), jg.ul.contiguous(), jg.dl.contiguous(),
        eg.k_adj_indptr, eg.k_adj_idx, eg.k_adj_link, eg.k_conf_indptr,
        eg.k_conf_base, eg.k_conf_cols, eg.link_rates.contiguous(),
        eg.proc_bws.contiguous(), eg.k_edges, eg.T_arr.contiguous(),
        eg.k_E_arr, eg.k_N_arr, fr["H"], eg.fp_iters)
    torch.cuda.synchronize()
    assert torch.equal(out[0].cpu().to(torch.int64), want_rl)
    assert torch.equal(out[1].cpu().to(torch.int64), nhop)
    assert int(out[5].sum()) == overflow


# ------------------------------------------------------------------- Adam
def _tree_sum(x, nt=256):
    """fp32 sum of a vector the way the kernel takes a norm: thread t adds
    its elements t, t+nt, ... in order, then red[t] += red[t+w] for
    w = nt/2 .. 1."""
    n = x.numel()
    pad = torch.zeros((n + nt - 1) // nt * nt, dtype=torch.float32)
    pad[:n] = x
    red = torch.zeros(nt, dtype=torch.float32)
    for row in pad.view(-1, nt):
        red = red + row
    w = nt // 2
    while w:
        red = red[:w] + red[w:2 * w]
        w //= 2
    return red[0]


def _adam_replay(p, g, m, v, t, scale, lr, b1, b2, eps, constraints):
    """Plain torch fp32 replay of one tensor through the fused pipeline, with
    the kernel's partial-sum order for the two whole-tensor norms.  Returns
    (p, m, v, scaled g)."""
    f32 = torch.float32
    g = (g * torch.tensor(scale, dtype=f32))
    nrm = torch.sqrt(_tree_sum((g * g).reshape(-1)))
    if bool(torch.isfinite(nrm)):
        f = 1.0 / nrm if float(nrm) > 1.0 else torch.tensor(1.0, dtype=f32)
        gv = g * f
        gv = torch.where(torch.isfinite(gv), gv, torch.zeros_like(gv))
        m = b1 * m + (1.0 - b1) * gv
        v = b2 * v + (1.0 - b2) * gv * gv
        bc1 = torch.tensor(1.0 / (1.0 - np.float32(b1) ** np.float32(t)),
                           dtype=f32)
        bc2 = torch.tensor(1.0 / (1.0 - np.float32(b2) ** np.float32(t)),
                           dtype=f32)
        p = p - lr * (m * bc1) / (torch.sqrt(v * bc2) + eps)
    if constraints:
        if p.dim() == 3:
            sq = torch.zeros_like(p[0])
            for k in range(p.shape[0]):
                sq = sq + p[k] * p[k]
            n = torch.sqrt(sq)
            p = torch.where(n > 1.0, p * (1.0 / n), p)
        else:
            n = torch.sqrt(_tree_sum((p * p).reshape(-1)))
            p = p * (1.0 / n) if float(n) > 1.0 else p
    return p, m, v, g


@needs_gpu
@pytest.mark.parametrize("constraints", [True, False])
def test_fused_adam_three_steps_vs_fp32_replay(constraints):
    """p, m, v, the scaled gradient and step_dev over three steps (the
    inputs of test_fused_adam_skips_non_finite_gradients: step 2 carries a
    NaN in a weight tensor's gradient and an inf in a bias tensor's, and
    that weight tensor is scaled past max_norm first) against a torch fp32
    replay that takes the two whole-tensor norms in the kernel's order
    (strided partials, then the tree), with and without the constraints.

    Not exact: the compiler contracts a*b+c in the moment updates and the
    sums of squares, which torch does not, so the comparison uses the
    tolerances tests/test_gpu_stages.py derives for this kernel — p within
    1e-6 absolute, m and v within 1e-5 relative plus 1e-6 of the tensor's
    largest entry.  What must be exact is: the skipped tensors keep m and v
    (and p, up to the max_norm rescale of columns whose norm exceeds 1) bit
    for bit, the scaled gradient equals g*scale bit for bit, and the step
    counter advances by one."""
    from multihop_offload_amd.models.chebconv import ChebConvStack
    from multihop_offload_amd.ops.functions import FusedAdam

    f32 = lambda x: float(np.float32(x))                   # noqa: E731
    lr, b1, b2, eps, scale = f32(1e-3), f32(0.9), f32(0.999), f32(1e-7), 0.5
    model = ChebConvStack(K=2, dtype=torch.float32, seed=7).cuda()
    params = list(model.parameters())
    w_bad, b_bad = 2, 5
    with torch.no_grad():
        params[b_bad].fill_(0.1)
    opt = FusedAdam(model, lr=1e-3, constraints=constraints)
    gen = torch.Generator().manual_seed(0)
    ref = [(p.detach().cpu().clone(), torch.zeros_like(p.cpu()),
            torch.zeros_like(p.cpu())) for p in params]

    def views(buf):
        out, off = [], 0
        for p in params:
            out.append(buf[off:off + p.numel()].view(p.shape))
            off += p.numel()
        return out

    for t in (1, 2, 3):
        grads = [torch.randn(p.shape, generator=gen)
                 * (10.0 if i % 3 else 0.01) for i, p in enumerate(params)]
        if t == 2:
            with torch.no_grad():
                params[w_bad].mul_(4.0)
            ref[w_bad] = (ref[w_bad][0] * 4.0,) + ref[w_bad][1:]
            grads[w_bad][1, 3, 5] = float("nan")
            grads[b_bad][7] = float("inf")
        before = [(p.detach().clone(), m.clone(), v.clone())
                  for p, m, v in zip(params, views(opt.m), views(opt.v))]
        opt.zero_grad()
        for p, g in zip(params, grads):
            p.grad.copy_(g)
        opt.step(scale=scale)
        torch.cuda.synchronize()
        assert int(opt.step_dev) == t
        new = [_adam_replay(p, g, m, v, t, scale, lr, b1, b2, eps,
                            constraints) for (p, m, v), g in zip(ref, grads)]
        ref = [r[:3] for r in new]
        for i, (p, m, v, g) in enumerate(zip(params, views(opt.m),
                                             views(opt.v),
                                             views(opt.flat_g))):
            assert torch.allclose(g.cpu(), new[i][3], rtol=0, atol=0,
                                  equal_nan=True), (t, i, "g")
            p0, m0, v0 = before[i]
            if t == 2 and i in (w_bad, b_bad):
                assert torch.equal(m, m0) and torch.equal(v, v0), (t, i)
                if i == b_bad or not constraints:
                    assert torch.equal(p.detach(), p0), (t, i)
            else:
                assert not torch.equal(p.detach(), p0), (t, i)
            assert bool(torch.isfinite(p).all())
            err_p = float((p.detach().cpu().double()
                           - ref[i][0].double()).abs().max())
            print(f"constraints {constraints} step {t} tensor {i}: "
                  f"max |p - replay| {err_p:.2e}")
            assert err_p <= 1e-6, (t, i, err_p)
            for got, want, what in ((m, ref[i][1], "m"), (v, ref[i][2], "v")):
                got, want = got.detach().cpu().double(), want.double()
                bound = 1e-5 * want.abs() + 1e-6 * want.abs().max()
                assert bool(((got - want).abs() <= bound).all()), (t, i, what)
