// Fused optimizer step for gfx950 — SURVEY.md §2.4 K14.
//
// One launch (one workgroup per parameter tensor; the actor has ten small
// ones) performs the reference's whole update pipeline (gnn_offloading_agent.py:114-121,
// 156-169 + Keras constraint semantics):
//   grad scale (1/batch) → per-tensor clipnorm(1.0) → Adam (eps 1e-7,
//   bias-corrected) → max_norm(1.0) constraints (kernel: per-(fi,fo) norm
//   over the Chebyshev axis; bias: whole-vector norm).
//
// Parameters live in ONE flat buffer (the model's tensors are views), which
// is also the RCCL all-reduce payload — the same flat-buffer layout the DP
// design uses.
//
// Two kernels compute the same thing bit for bit:
//   fused_adam_blocks_kernel  block r owns tensor r, so tensors do not wait
//       for each other, and within a phase a thread issues all its loads
//       before its first store (EPT elements in registers at a time): the
//       launch is a few global round trips long instead of one per loop
//       iteration.  The step counter is advanced by the block that draws
//       the last ticket.  Taken when the caller passes a ticket tensor.
//   fused_adam_kernel  the single workgroup that walks the tensors in
//       groups of SEG_GROUP; taken without a ticket tensor and under
//       adam_force_single_block(true) (before/after timings, the oracle of
//       tests/test_gpu_adam_blocks.py).

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

namespace {

constexpr int NT = 256;          // threads of a workgroup
constexpr int SEG_GROUP = 16;    // tensors whose norms share one tree
constexpr int EPT = 8;           // blocks kernel: elements a thread holds
constexpr int PPT = 4;           // ... and (fi, fo) pairs, K of each

// Sum each of the first `rows` rows of per-thread partials into column 0:
// the one-row tree (red[tid] += red[tid + w], w = nt/2 .. 1) applied to
// every row between the same barriers, so a row's sum is bit for bit what
// a tree of its own gives.  Opens and ends on a barrier.
__device__ __forceinline__ void tree_rows(float (*red)[NT], int rows,
                                          int tid, int nt) {
    __syncthreads();
    for (int w = nt >> 1; w > 0; w >>= 1) {
        if (tid < w)
            for (int r = 0; r < rows; ++r) red[r][tid] += red[r][tid + w];
        __syncthreads();
    }
}

// Adam on one element's values with its tensor's clip factor f (f >= 0).
// Returns the parameter after the step; the new moments go to *mn, *vn.
__device__ __forceinline__ float adam_value(
    float pj, float gj, float mj, float vj, float f, float lr, float beta1,
    float beta2, float eps, float bc1, float bc2, float* mn_out,
    float* vn_out) {
    float gv = gj * f;
    gv = isfinite(gv) ? gv : 0.f;   // isolated inf/NaN lanes
    const float mn = beta1 * mj + (1.f - beta1) * gv;
    const float vn = beta2 * vj + (1.f - beta2) * gv * gv;
    *mn_out = mn;
    *vn_out = vn;
    return pj - lr * (mn * bc1) / (sqrtf(vn * bc2) + eps);
}

// Adam on element j with its tensor's clip factor f (f < 0: the tensor is
// skipped).  Returns the element's parameter after the step.
__device__ __forceinline__ float adam_element(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ m, float* __restrict__ v, int j, float f, float lr,
    float beta1, float beta2, float eps, float bc1, float bc2) {
    if (f < 0.f) return p[j];
    float mn, vn;
    const float pj = adam_value(p[j], g[j], m[j], v[j], f, lr, beta1, beta2,
                                eps, bc1, bc2, &mn, &vn);
    m[j] = mn;
    v[j] = vn;
    p[j] = pj;
    return pj;
}

// segment descriptor: [offset, size, K, fi, fo]; bias rows have K == 0
//
// Up to SEG_GROUP tensors go through each phase together: the clip norms of
// all of them come from one tree, then every element is updated once, then
// (constraints) the bias norms come from a second tree.  A thread's strided
// partial sums and the tree are those of a one-tensor-at-a-time pass, so
// every norm — and with it every result — is bit for bit the same.
__global__ void fused_adam_kernel(
    float* __restrict__ p, float* __restrict__ g,
    float* __restrict__ m, float* __restrict__ v,
    const int* __restrict__ seg, int n_seg,
    float scale, float lr, float beta1, float beta2, float eps,
    int* __restrict__ step_dev, int do_constraints) {
    __shared__ float red[SEG_GROUP][NT];
    __shared__ float factor[SEG_GROUP];
    __shared__ float bc_s[2];
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    if (tid == 0) {
        // the step counter lives on device so hipGraph replays advance it
        const float t = (float)(atomicAdd(step_dev, 1) + 1);
        bc_s[0] = 1.0f / (1.0f - powf(beta1, t));
        bc_s[1] = 1.0f / (1.0f - powf(beta2, t));
    }

    for (int s0 = 0; s0 < n_seg; s0 += SEG_GROUP) {
        const int ns = n_seg - s0 < SEG_GROUP ? n_seg - s0 : SEG_GROUP;
        const int* sg = seg + s0 * 5;

        // ---- grad scale + per-tensor clipnorm(1.0) -----------------------
        for (int r = 0; r < ns; ++r) {
            const int off = sg[r * 5], size = sg[r * 5 + 1];
            float acc = 0.f;
            for (int i = tid; i < size; i += nt) {
                const float gv = g[off + i] * scale;
                g[off + i] = gv;
                acc += gv * gv;
            }
            red[r][tid] = acc;
        }
        tree_rows(red, ns, tid, nt);
        if (tid < ns) {
            const float nrm = sqrtf(red[tid][0]);
            // non-finite gradient norm (inf/NaN from the 1/(mu-lam) pole
            // in fp32): SKIP this tensor's update entirely — one poisoned
            // step would otherwise write NaN into p/m/v and freeze the
            // policy permanently (observed at seed-dependent rates)
            factor[tid] = isfinite(nrm) ? (nrm > 1.0f ? 1.0f / nrm : 1.0f)
                                        : -1.0f;
        }
        __syncthreads();
        const float bc1 = bc_s[0], bc2 = bc_s[1];

        // ---- Adam; Keras max_norm(1.0) of the kernels on the way ---------
        // kernels — a thread takes (fi, fo) pairs and walks the K axis, so
        // the pair's norm never leaves it; biases (and everything when the
        // constraints are off) — strided elements, the partial sums of the
        // whole-vector norm into `red`
        for (int r = 0; r < ns; ++r) {
            const int off = sg[r * 5], size = sg[r * 5 + 1];
            const int K = sg[r * 5 + 2];
            const float f = factor[r];
            if (K > 0 && do_constraints) {
                const int pairs = sg[r * 5 + 3] * sg[r * 5 + 4];
                for (int i = tid; i < pairs; i += nt) {
                    float sq = 0.f;
                    for (int k = 0; k < K; ++k) {
                        const float w = adam_element(
                            p, g, m, v, off + k * pairs + i, f, lr, beta1,
                            beta2, eps, bc1, bc2);
                        sq += w * w;
                    }
                    const float nrm = sqrtf(sq);
                    if (nrm > 1.0f) {
                        const float c = 1.0f / nrm;
                        for (int k = 0; k < K; ++k) p[off + k * pairs + i] *= c;
                    }
                }
                red[r][tid] = 0.f;
            } else {
                float acc = 0.f;
                for (int i = tid; i < size; i += nt) {
                    const float w = adam_element(p, g, m, v, off + i, f, lr,
                                                 beta1, beta2, eps, bc1, bc2);
                    acc += w * w;
                }
                red[r][tid] = acc;
            }
        }
        if (!do_constraints) {
            __syncthreads();               // `red` and `factor` are reused
            continue;
        }
        // ---- max_norm(1.0) of the biases: whole-vector norm --------------
        tree_rows(red, ns, tid, nt);
        for (int r = 0; r < ns; ++r) {
            if (sg[r * 5 + 2] > 0) continue;
            const int off = sg[r * 5], size = sg[r * 5 + 1];
            const float nrm = sqrtf(red[r][0]);
            if (nrm > 1.0f) {
                const float c = 1.0f / nrm;
                // a thread rescales the elements it wrote itself
                for (int i = tid; i < size; i += nt) p[off + i] *= c;
            }
        }
        __syncthreads();                   // `red` and `factor` are reused
    }
}

// One-row tree over red[0 .. NT): tree_rows with rows == 1.
__device__ __forceinline__ void tree_one(float* red, int tid) {
    __syncthreads();
    for (int w = NT >> 1; w > 0; w >>= 1) {
        if (tid < w) red[tid] += red[tid + w];
        __syncthreads();
    }
}

// Adam + max_norm of a kernel tensor with a compile-time Chebyshev order:
// a thread takes PPT (fi, fo) pairs at a time, loads the K elements of
// each from all four arrays, then computes and stores.  The rescale of a
// pair whose norm exceeds 1 happens in registers (the single-block kernel
// stores, reloads and stores again: the same product).  The sums of squares
// here and in the kernel below are written as the fused multiply-adds the
// single-block kernel's `acc += x * x` loops compile to, one element after
// the other: unrolled, `0 + a·a + b·b` would leave the compiler the choice of
// which product to fuse, and the norms would differ in the last bit.
template <int KC>
__device__ __forceinline__ void adam_pairs(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ m, float* __restrict__ v, int off, int pairs,
    float f, float lr, float beta1, float beta2, float eps, float bc1,
    float bc2, int tid) {
    for (int base = 0; base < pairs; base += PPT * NT) {
        float pv[PPT][KC], gv[PPT][KC], mv[PPT][KC], vv[PPT][KC];
#pragma unroll
        for (int u = 0; u < PPT; ++u) {
            const int i = base + u * NT + tid;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const int j = off + k * pairs + i;
                const bool in = i < pairs;
                pv[u][k] = in ? p[j] : 0.f;
                gv[u][k] = in && f >= 0.f ? g[j] : 0.f;
                mv[u][k] = in && f >= 0.f ? m[j] : 0.f;
                vv[u][k] = in && f >= 0.f ? v[j] : 0.f;
            }
        }
#pragma unroll
        for (int u = 0; u < PPT; ++u) {
            const int i = base + u * NT + tid;
            if (i >= pairs) continue;
            float sq = 0.f;
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                if (f >= 0.f) {
                    const int j = off + k * pairs + i;
                    float mn, vn;
                    pv[u][k] = adam_value(pv[u][k], gv[u][k], mv[u][k],
                                          vv[u][k], f, lr, beta1, beta2, eps,
                                          bc1, bc2, &mn, &vn);
                    m[j] = mn;
                    v[j] = vn;
                }
                sq = __fmaf_rn(pv[u][k], pv[u][k], sq);
            }
            const float nrm = sqrtf(sq);
            const float c = 1.0f / nrm;
            if (f >= 0.f || nrm > 1.0f) {
#pragma unroll
                for (int k = 0; k < KC; ++k)
                    p[off + k * pairs + i] =
                        nrm > 1.0f ? pv[u][k] * c : pv[u][k];
            }
        }
    }
}

// One workgroup per tensor (grid.x = n_seg); see the file header.  The
// arithmetic is fused_adam_kernel's: a thread's strided partial (elements
// tid, tid + NT, ... in order), the NT-wide tree, the clip factor,
// adam_value, the per-pair max_norm inside the thread, the bias-norm tree.
//
// Step counter: thread 0 of every block reads t = *step_dev + 1 at its top
// and takes a ticket when its block is done; the block that draws
// n_seg - 1 stores step_dev = t and resets the ticket, so no block can read
// the counter after it was written, and a hipGraph replay advances it.
__global__ void __launch_bounds__(NT) fused_adam_blocks_kernel(
    float* __restrict__ p, float* __restrict__ g,
    float* __restrict__ m, float* __restrict__ v,
    const int* __restrict__ seg, int n_seg,
    float scale, float lr, float beta1, float beta2, float eps,
    int* step_dev, int* ticket, int do_constraints) {
    __shared__ float red[NT];        // clip norm
    __shared__ float red2[NT];       // bias norm
    __shared__ float bc_s[2];
    __shared__ int t_s;
    const int tid = threadIdx.x;
    const int r = blockIdx.x;
    const int off = seg[r * 5], size = seg[r * 5 + 1], K = seg[r * 5 + 2];
    const int pairs = seg[r * 5 + 3] * seg[r * 5 + 4];
    if (tid == 0) {
        const int ti = __hip_atomic_load(step_dev, __ATOMIC_RELAXED,
                                         __HIP_MEMORY_SCOPE_AGENT) + 1;
        const float t = (float)ti;
        t_s = ti;
        bc_s[0] = 1.0f / (1.0f - powf(beta1, t));
        bc_s[1] = 1.0f / (1.0f - powf(beta2, t));
    }

    // ---- grad scale + clipnorm(1.0) --------------------------------------
    float acc = 0.f;
    for (int base = 0; base < size; base += EPT * NT) {
        float gv[EPT];
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            const int i = base + u * NT + tid;
            gv[u] = i < size ? g[off + i] : 0.f;
        }
#pragma unroll
        for (int u = 0; u < EPT; ++u) {
            const int i = base + u * NT + tid;
            if (i < size) {
                const float x = gv[u] * scale;
                g[off + i] = x;
                acc = __fmaf_rn(x, x, acc);
            }
        }
    }
    red[tid] = acc;
    tree_one(red, tid);              // also orders the stores to g
    const float nrm = sqrtf(red[0]);
    // non-finite gradient norm: skip the tensor (see fused_adam_kernel)
    const float f = isfinite(nrm) ? (nrm > 1.0f ? 1.0f / nrm : 1.0f) : -1.0f;
    const float bc1 = bc_s[0], bc2 = bc_s[1];

    // ---- Adam; max_norm(1.0) ---------------------------------------------
    if (K > 0 && do_constraints) {
        if (K == 1) {
            adam_pairs<1>(p, g, m, v, off, pairs, f, lr, beta1, beta2, eps,
                          bc1, bc2, tid);
        } else if (K == 2) {
            adam_pairs<2>(p, g, m, v, off, pairs, f, lr, beta1, beta2, eps,
                          bc1, bc2, tid);
        } else if (K == 3) {
            adam_pairs<3>(p, g, m, v, off, pairs, f, lr, beta1, beta2, eps,
                          bc1, bc2, tid);
        } else {
            // any other order: one element at a time
            for (int i = tid; i < pairs; i += NT) {
                float sq = 0.f;
                for (int k = 0; k < K; ++k) {
                    const float w = adam_element(
                        p, g, m, v, off + k * pairs + i, f, lr, beta1, beta2,
                        eps, bc1, bc2);
                    sq += w * w;
                }
                const float pn = sqrtf(sq);
                if (pn > 1.0f) {
                    const float c = 1.0f / pn;
                    for (int k = 0; k < K; ++k) p[off + k * pairs + i] *= c;
                }
            }
        }
    } else {
        float acc2 = 0.f;
        for (int base = 0; base < size; base += EPT * NT) {
            float pv[EPT], gv[EPT], mv[EPT], vv[EPT];
#pragma unroll
            for (int u = 0; u < EPT; ++u) {
                const int i = base + u * NT + tid;
                const bool in = i < size;
                pv[u] = in ? p[off + i] : 0.f;
                gv[u] = in && f >= 0.f ? g[off + i] : 0.f;
                mv[u] = in && f >= 0.f ? m[off + i] : 0.f;
                vv[u] = in && f >= 0.f ? v[off + i] : 0.f;
            }
#pragma unroll
            for (int u = 0; u < EPT; ++u) {
                const int i = base + u * NT + tid;
                if (i >= size) continue;
                if (f >= 0.f) {
                    float mn, vn;
                    pv[u] = adam_value(pv[u], gv[u], mv[u], vv[u], f, lr,
                                       beta1, beta2, eps, bc1, bc2, &mn, &vn);
                    m[off + i] = mn;
                    v[off + i] = vn;
                    p[off + i] = pv[u];
                }
                acc2 = __fmaf_rn(pv[u], pv[u], acc2);
            }
        }
        if (do_constraints) {
            // ---- max_norm(1.0) of a bias: whole-vector norm --------------
            red2[tid] = acc2;
            tree_one(red2, tid);
            const float bn = sqrtf(red2[0]);
            if (bn > 1.0f) {
                const float c = 1.0f / bn;
                // a thread rescales the elements it wrote itself
                for (int i = tid; i < size; i += NT) p[off + i] *= c;
            }
        }
    }

    // t_s was written before the first tree's barriers
    if (tid == 0) {
        const int tk = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL,
                                              __HIP_MEMORY_SCOPE_AGENT);
        if (tk == n_seg - 1) {
            __hip_atomic_store(step_dev, t_s, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
            __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        }
    }
}

bool adam_single_forced = false;

}  // namespace

// adam_force_single_block(true): every later fused_adam launch takes the
// single-workgroup kernel, with or without a ticket tensor.
void adam_force_single_block(bool on) { adam_single_forced = on; }

void fused_adam_hip(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                    torch::Tensor v, torch::Tensor seg, torch::Tensor step,
                    double scale, double lr, double beta1, double beta2,
                    double eps, bool constraints,
                    c10::optional<torch::Tensor> ticket) {
    const int n_seg = seg.size(0);
    auto stream = at::cuda::getCurrentCUDAStream();
    if (ticket.has_value() && !adam_single_forced && n_seg > 0) {
        TORCH_CHECK(ticket->scalar_type() == torch::kInt32
                    && ticket->numel() == 1, "fused_adam: ticket is one int32");
        hipLaunchKernelGGL(fused_adam_blocks_kernel, dim3(n_seg), dim3(NT),
                           0, stream.stream(),
                           p.data_ptr<float>(), g.data_ptr<float>(),
                           m.data_ptr<float>(), v.data_ptr<float>(),
                           seg.data_ptr<int>(), n_seg,
                           (float)scale, (float)lr, (float)beta1,
                           (float)beta2, (float)eps, step.data_ptr<int>(),
                           ticket->data_ptr<int>(), constraints ? 1 : 0);
        return;
    }
    hipLaunchKernelGGL(fused_adam_kernel, dim3(1), dim3(NT), 0,
                       stream.stream(),
                       p.data_ptr<float>(), g.data_ptr<float>(),
                       m.data_ptr<float>(), v.data_ptr<float>(),
                       seg.data_ptr<int>(), n_seg,
                       (float)scale, (float)lr, (float)beta1, (float)beta2,
                       (float)eps, step.data_ptr<int>(),
                       constraints ? 1 : 0);
}
