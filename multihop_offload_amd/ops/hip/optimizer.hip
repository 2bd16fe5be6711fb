// Fused optimizer step for gfx950 — SURVEY.md §2.4 K14.
//
// One launch (a single workgroup; the actor has ~3.4k parameters) performs
// the reference's whole update pipeline (gnn_offloading_agent.py:114-121,
// 156-169 + Keras constraint semantics):
//   grad scale (1/batch) → per-tensor clipnorm(1.0) → Adam (eps 1e-7,
//   bias-corrected) → max_norm(1.0) constraints (kernel: per-(fi,fo) norm
//   over the Chebyshev axis; bias: whole-vector norm).
//
// Parameters live in ONE flat buffer (the model's tensors are views), which
// is also the RCCL all-reduce payload — the same flat-buffer layout the DP
// design uses.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

namespace {

constexpr int NT = 256;          // threads of the one workgroup
constexpr int SEG_GROUP = 16;    // tensors whose norms share one tree

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

// Adam on element j with its tensor's clip factor f (f < 0: the tensor is
// skipped).  Returns the element's parameter after the step.
__device__ __forceinline__ float adam_element(
    float* __restrict__ p, const float* __restrict__ g,
    float* __restrict__ m, float* __restrict__ v, int j, float f, float lr,
    float beta1, float beta2, float eps, float bc1, float bc2) {
    if (f < 0.f) return p[j];
    float gv = g[j] * f;
    gv = isfinite(gv) ? gv : 0.f;   // isolated inf/NaN lanes
    const float mn = beta1 * m[j] + (1.f - beta1) * gv;
    const float vn = beta2 * v[j] + (1.f - beta2) * gv * gv;
    m[j] = mn;
    v[j] = vn;
    float pj = p[j];
    pj -= lr * (mn * bc1) / (sqrtf(vn * bc2) + eps);
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

}  // namespace

void fused_adam_hip(torch::Tensor p, torch::Tensor g, torch::Tensor m,
                    torch::Tensor v, torch::Tensor seg, torch::Tensor step,
                    double scale, double lr, double beta1, double beta2,
                    double eps, bool constraints) {
    const int n_seg = seg.size(0);
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(fused_adam_kernel, dim3(1), dim3(NT), 0,
                       stream.stream(),
                       p.data_ptr<float>(), g.data_ptr<float>(),
                       m.data_ptr<float>(), v.data_ptr<float>(),
                       seg.data_ptr<int>(), n_seg,
                       (float)scale, (float)lr, (float)beta1, (float)beta2,
                       (float)eps, step.data_ptr<int>(),
                       constraints ? 1 : 0);
}
