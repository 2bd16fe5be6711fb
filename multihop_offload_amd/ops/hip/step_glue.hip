// Per-step glue of the training episode for gfx950: the small tensor
// programs between the episode kernels (parameter pack, gradient reduce,
// feature build, job sampling after the draws, episode summary), each as ONE
// launch instead of a chain of elementwise/scatter/copy launches.  Every
// kernel here is capture-safe: no host reads, no synchronisation, outputs
// allocated through torch.
//
// Where a result is compared exactly with the torch composition it replaces,
// the arithmetic keeps torch's roundings: `#pragma clang fp contract(off)`
// stops the compiler from fusing a multiply and an add that torch rounds
// separately.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "gfx950.h"

namespace {

constexpr int PAD = 32;          // padded feature width of the cheb kernels
constexpr int MAX_LAYERS = 8;
constexpr int MAX_PARAMS = 2 * MAX_LAYERS;

inline hipStream_t cur_stream() {
    return at::cuda::getCurrentCUDAStream().stream();
}

// ---------------------------------------------------------------------------
// cheb_pack_params: per-layer (weight (K,fi,fo), bias (fo)) → zero-padded
// (L,K,32,32) / (L,32).
// ---------------------------------------------------------------------------
struct PackArgs {
    const float* w[MAX_LAYERS];
    const float* b[MAX_LAYERS];
    int kw[MAX_LAYERS], fi[MAX_LAYERS], fo[MAX_LAYERS], nb[MAX_LAYERS];
    int L, K;
};

__global__ void cheb_pack_kernel(const PackArgs a, float* __restrict__ Wp,
                                 float* __restrict__ bp) {
    const int nW = a.L * a.K * PAD * PAD;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < nW) {
        const int o = i % PAD, r = (i / PAD) % PAD;
        const int k = (i / (PAD * PAD)) % a.K, l = i / (PAD * PAD * a.K);
        const bool in = k < a.kw[l] && r < a.fi[l] && o < a.fo[l];
        Wp[i] = in ? a.w[l][((size_t)k * a.fi[l] + r) * a.fo[l] + o] : 0.f;
    } else if (i < nW + a.L * PAD) {
        const int q = i - nW, l = q / PAD, o = q % PAD;
        bp[q] = o < a.nb[l] ? a.b[l][o] : 0.f;
    }
}

// ---------------------------------------------------------------------------
// cheb_reduce_grads: per-graph partials dW (B,L,K,32,32) / db (B,L,32) →
// compact per-parameter gradients summed over B, written (or added) at each
// parameter's offset of one flat buffer.  A block owns 32 consecutive flat
// cells × 32 slices of B; the slices meet in LDS in a fixed order, so the
// sum is deterministic.
// ---------------------------------------------------------------------------
constexpr int REDUCE_SLICES = 32;

struct ReduceArgs {
    int start[MAX_PARAMS + 1];   // first compact cell of parameter p
    int offset[MAX_PARAMS];      // its offset in the flat buffer
    int fi[MAX_PARAMS], fo[MAX_PARAMS];   // weight shape; fi = 0: a bias
    int P, K, L;
};

__global__ void cheb_reduce_kernel(const float* __restrict__ dW,
                                   const float* __restrict__ db,
                                   const ReduceArgs a, int B,
                                   float* __restrict__ flat, int accumulate) {
    __shared__ float part[REDUCE_SLICES][32];
    const int lane = threadIdx.x & 31, slice = threadIdx.x >> 5;
    const int cell = blockIdx.x * 32 + lane;
    const int total = a.start[a.P];
    const float* src = nullptr;
    size_t stride = 0;
    int dst = -1;
    if (cell < total) {
        int p = 0;
        while (cell >= a.start[p + 1]) ++p;
        const int local = cell - a.start[p], l = p >> 1;
        dst = a.offset[p] + local;
        if (a.fi[p]) {
            const int o = local % a.fo[p], r = (local / a.fo[p]) % a.fi[p];
            const int k = local / (a.fo[p] * a.fi[p]);
            src = dW + (((size_t)l * a.K + k) * PAD + r) * PAD + o;
            stride = (size_t)a.L * a.K * PAD * PAD;
        } else {
            src = db + (size_t)l * PAD + local;
            stride = (size_t)a.L * PAD;
        }
    }
    float acc = 0.f;
    if (src) {
#pragma unroll 8
        for (int b = slice; b < B; b += REDUCE_SLICES)
            acc += src[(size_t)b * stride];
    }
    part[slice][lane] = acc;
    __syncthreads();
    if (slice == 0 && dst >= 0) {
        float s = part[0][lane];
#pragma unroll
        for (int q = 1; q < REDUCE_SLICES; ++q) s += part[q][lane];
        flat[dst] = accumulate ? flat[dst] + s : s;
    }
}

// ---------------------------------------------------------------------------
// cheb_features: x (B,Ee,4) = [self_loop, rate, job load, as_server]; the job
// column is Σ rate·ul of the jobs whose source owns that compute slot.
// grid.x = B, LDS: Ee floats.
// ---------------------------------------------------------------------------
__global__ void cheb_features_kernel(
    const long* __restrict__ sources,      // (B,J)
    const float* __restrict__ rates,       // (B,J)
    const float* __restrict__ ul,          // (B,J)
    const bool* __restrict__ mask,         // (B,J)
    const long* __restrict__ node_vedge,   // (B,N)
    const bool* __restrict__ comp_mask,    // (B,N)
    const float* __restrict__ f_self_loop, // (B,Ee)
    const float* __restrict__ f_rate,      // (B,Ee)
    const float* __restrict__ f_as_server, // (B,Ee)
    float4* __restrict__ x,                // (B,Ee) of 4
    int N, int J, int Ee) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* fjob = reinterpret_cast<float*>(smem_raw);
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    for (int e = tid; e < Ee; e += nt) fjob[e] = 0.f;
    __syncthreads();
    for (int j = tid; j < J; j += nt) {
        const size_t bj = (size_t)b * J + j;
        if (!mask[bj]) continue;           // padded jobs carry zero rate
        const long n = sources[bj];
        if (n < 0 || n >= N || !comp_mask[(size_t)b * N + n]) continue;
        const long ve = node_vedge[(size_t)b * N + n];
        if (ve >= 0 && ve < Ee) atomicAdd(&fjob[ve], rates[bj] * ul[bj]);
    }
    __syncthreads();
    for (int e = tid; e < Ee; e += nt) {
        const size_t be = (size_t)b * Ee + e;
        x[be] = make_float4(f_self_loop[be], f_rate[be], fjob[e],
                            f_as_server[be]);
    }
}

// ---------------------------------------------------------------------------
// episode_summary: per graph tau = Σ delay / jobs, congested-job count, job
// count.  grid.x = B, one wave per graph.
// ---------------------------------------------------------------------------
__global__ void episode_summary_kernel(
    const float* __restrict__ delay_emp,   // (B,J) nan where padded
    const bool* __restrict__ mask,         // (B,J)
    const float* __restrict__ T_arr,       // (B)
    float* __restrict__ tau, long* __restrict__ congest,
    long* __restrict__ num_jobs, int J) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const float T = T_arr[b];
    float sum = 0.f;
    int nj = 0, nc = 0;
    for (int j = lane; j < J; j += 64) {
        const size_t bj = (size_t)b * J + j;
        if (!mask[bj]) continue;
        const float d = delay_emp[bj];
        sum += d;
        nj += 1;
        nc += d > T ? 1 : 0;
    }
    for (int w = 32; w > 0; w >>= 1) {
        sum += __shfl_down(sum, w, 64);
        nj += __shfl_down(nj, w, 64);
        nc += __shfl_down(nc, w, 64);
    }
    if (lane == 0) {
        tau[b] = sum / (float)nj;          // no jobs: nan, like 0/0 in torch
        congest[b] = nc;
        num_jobs[b] = nj;
    }
}

// ---------------------------------------------------------------------------
// jobs_from_draws: everything of EpisodeEngine.sample_jobs after the three
// uniform draws.  Per graph: rank the mobiles by score (non-mobiles score
// 2.0 and rank behind them; equal scores rank by node id, as a stable sort
// does), J ~ lo + trunc(r·span), sources = the J lowest-ranked mobiles,
// rates = (r·0.4 + 0.1)·scale with each operation rounded to fp32 on its
// own.  grid.x = B; LDS (all dynamic): N floats + J + 1 ints.
// ---------------------------------------------------------------------------
__global__ void jobs_from_draws_kernel(
    const float* __restrict__ scores_raw,  // (B,N)
    const float* __restrict__ r_nj,        // (B)
    const float* __restrict__ r_rates,     // (B,J)
    const bool* __restrict__ mobile,       // (B,N)
    float scale, int N, int J,
    long* __restrict__ sources, bool* __restrict__ mask,
    float* __restrict__ rates, float* __restrict__ ul,
    float* __restrict__ dl) {
#pragma clang fp contract(off)
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* score = reinterpret_cast<float*>(smem_raw);
    int* order = reinterpret_cast<int*>(score + N);
    int& s_M = order[J];                   // mobile count of this graph
    const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
    if (tid == 0) s_M = 0;
    __syncthreads();
    int m_loc = 0;
    for (int n = tid; n < N; n += nt) {
        const bool mob = mobile[(size_t)b * N + n];
        score[n] = mob ? scores_raw[(size_t)b * N + n] : 2.0f;
        m_loc += mob ? 1 : 0;
    }
    if (m_loc) atomicAdd(&s_M, m_loc);
    __syncthreads();
    for (int n = tid; n < N; n += nt) {
        const float s = score[n];
        int rank = 0;
        for (int m = 0; m < N; ++m) {
            const float t = score[m];
            rank += (t < s || (t == s && m < n)) ? 1 : 0;
        }
        if (rank < J) order[rank] = n;
    }
    __syncthreads();
    const int M = s_M;
    const long lo = (long)(0.3f * (float)M);
    const long span = M - lo > 1 ? M - lo : 1;
    long nj = lo + (long)(r_nj[b] * (float)span);
    if (nj < 1) nj = 1;
    for (int j = tid; j < J; j += nt) {
        const size_t bj = (size_t)b * J + j;
        const bool real = j < nj;
        sources[bj] = order[real ? j : 0];
        mask[bj] = real;
        const float r = (r_rates[bj] * 0.4f + 0.1f) * scale;
        rates[bj] = real ? r : 0.f;
        ul[bj] = real ? 100.f : 0.f;
        dl[bj] = real ? 1.f : 0.f;
    }
}

void check_f32(const torch::Tensor& t, const char* name) {
    TORCH_CHECK(t.is_cuda() && t.scalar_type() == torch::kFloat
                && t.is_contiguous(), name, ": contiguous fp32 CUDA tensor "
                "expected");
}

}  // namespace

std::vector<torch::Tensor> cheb_pack_params_hip(
    std::vector<torch::Tensor> params) {
    TORCH_CHECK(!params.empty() && params.size() % 2 == 0
                && params.size() <= MAX_PARAMS, "expected up to ",
                MAX_LAYERS, " (weight, bias) pairs");
    PackArgs a;
    a.L = params.size() / 2;
    a.K = params[0].size(0);
    for (int l = 0; l < a.L; ++l) {
        const auto& w = params[2 * l];
        const auto& b = params[2 * l + 1];
        check_f32(w, "weight");
        check_f32(b, "bias");
        TORCH_CHECK(w.dim() == 3 && b.dim() == 1 && w.size(0) <= a.K
                    && w.size(1) <= PAD && w.size(2) <= PAD
                    && b.size(0) <= PAD, "parameter shape beyond the padded "
                    "(K,32,32)/(32) layout");
        a.w[l] = w.data_ptr<float>();
        a.b[l] = b.data_ptr<float>();
        a.kw[l] = w.size(0);
        a.fi[l] = w.size(1);
        a.fo[l] = w.size(2);
        a.nb[l] = b.size(0);
    }
    auto opts = params[0].options().requires_grad(false);
    auto Wp = torch::empty({a.L, a.K, PAD, PAD}, opts);
    auto bp = torch::empty({a.L, PAD}, opts);
    const int n = a.L * a.K * PAD * PAD + a.L * PAD;
    hipLaunchKernelGGL(cheb_pack_kernel, dim3((n + 255) / 256), dim3(256), 0,
                       cur_stream(), a, Wp.data_ptr<float>(),
                       bp.data_ptr<float>());
    return {Wp, bp};
}

void cheb_reduce_grads_hip(torch::Tensor dW, torch::Tensor db,
                           std::vector<std::vector<int64_t>> shapes,
                           torch::Tensor flat_out,
                           std::vector<int64_t> offsets, bool accumulate) {
    check_f32(dW, "dW");
    check_f32(db, "db");
    check_f32(flat_out, "flat_out");
    TORCH_CHECK(dW.dim() == 5 && dW.size(3) == PAD && dW.size(4) == PAD
                && db.dim() == 3 && db.size(2) == PAD
                && db.size(0) == dW.size(0) && db.size(1) == dW.size(1),
                "expected dW (B,L,K,32,32) and db (B,L,32)");
    ReduceArgs a;
    a.P = shapes.size();
    a.L = dW.size(1);
    a.K = dW.size(2);
    TORCH_CHECK(a.P == 2 * a.L && a.P <= MAX_PARAMS
                && offsets.size() == shapes.size(),
                "one (weight, bias) shape pair and offset per layer");
    a.start[0] = 0;
    for (int p = 0; p < a.P; ++p) {
        const auto& s = shapes[p];
        int64_t numel;
        if (p % 2 == 0) {
            TORCH_CHECK(s.size() == 3 && s[0] >= 1 && s[0] <= a.K
                        && s[1] >= 1 && s[1] <= PAD && s[2] >= 1
                        && s[2] <= PAD, "weight shape beyond (K,32,32)");
            a.fi[p] = s[1];
            a.fo[p] = s[2];
            numel = s[0] * s[1] * s[2];
        } else {
            TORCH_CHECK(s.size() == 1 && s[0] >= 1 && s[0] <= PAD,
                        "bias shape beyond (32)");
            a.fi[p] = 0;
            a.fo[p] = s[0];
            numel = s[0];
        }
        TORCH_CHECK(offsets[p] >= 0
                    && offsets[p] + numel <= flat_out.numel(),
                    "segment outside the flat buffer");
        a.offset[p] = offsets[p];
        a.start[p + 1] = a.start[p] + numel;
    }
    const int total = a.start[a.P];
    hipLaunchKernelGGL(cheb_reduce_kernel, dim3((total + 31) / 32),
                       dim3(32 * REDUCE_SLICES), 0, cur_stream(),
                       dW.data_ptr<float>(),
                       db.data_ptr<float>(), a, (int)dW.size(0),
                       flat_out.data_ptr<float>(), accumulate ? 1 : 0);
}

torch::Tensor cheb_features_hip(
    torch::Tensor sources, torch::Tensor rates, torch::Tensor ul,
    torch::Tensor mask, torch::Tensor node_vedge, torch::Tensor comp_mask,
    torch::Tensor f_self_loop, torch::Tensor f_rate,
    torch::Tensor f_as_server) {
    check_f32(rates, "rates");
    check_f32(ul, "ul");
    check_f32(f_self_loop, "f_self_loop");
    check_f32(f_rate, "f_rate");
    check_f32(f_as_server, "f_as_server");
    const int B = sources.size(0), J = sources.size(1);
    const int N = node_vedge.size(1), Ee = f_rate.size(1);
    TORCH_CHECK(sources.scalar_type() == torch::kLong
                && node_vedge.scalar_type() == torch::kLong
                && mask.scalar_type() == torch::kBool
                && comp_mask.scalar_type() == torch::kBool
                && sources.is_contiguous() && mask.is_contiguous()
                && node_vedge.is_contiguous() && comp_mask.is_contiguous(),
                "index/mask dtype or layout");
    TORCH_CHECK(rates.sizes() == sources.sizes()
                && ul.sizes() == sources.sizes()
                && mask.sizes() == sources.sizes()
                && comp_mask.sizes() == node_vedge.sizes()
                && node_vedge.size(0) == B && f_rate.size(0) == B
                && f_self_loop.sizes() == f_rate.sizes()
                && f_as_server.sizes() == f_rate.sizes(), "shape mismatch");
    const size_t lds = sizeof(float) * Ee;
    TORCH_CHECK(lds <= LDS_LIMIT, "Ee too large for the feature kernel");
    auto x = torch::empty({B, Ee, 4}, f_rate.options());
    hipLaunchKernelGGL(cheb_features_kernel, dim3(B), dim3(256), lds,
                       cur_stream(), sources.data_ptr<long>(),
                       rates.data_ptr<float>(), ul.data_ptr<float>(),
                       mask.data_ptr<bool>(), node_vedge.data_ptr<long>(),
                       comp_mask.data_ptr<bool>(),
                       f_self_loop.data_ptr<float>(),
                       f_rate.data_ptr<float>(),
                       f_as_server.data_ptr<float>(),
                       reinterpret_cast<float4*>(x.data_ptr<float>()),
                       N, J, Ee);
    return x;
}

std::vector<torch::Tensor> episode_summary_hip(torch::Tensor delay_emp,
                                               torch::Tensor mask,
                                               torch::Tensor T_arr) {
    check_f32(delay_emp, "delay_emp");
    check_f32(T_arr, "T_arr");
    TORCH_CHECK(mask.scalar_type() == torch::kBool && mask.is_contiguous()
                && mask.sizes() == delay_emp.sizes()
                && delay_emp.dim() == 2
                && T_arr.numel() == delay_emp.size(0), "shape mismatch");
    const int B = delay_emp.size(0), J = delay_emp.size(1);
    auto tau = torch::empty({B}, delay_emp.options());
    auto congest = torch::empty({B}, delay_emp.options().dtype(torch::kLong));
    auto num_jobs = torch::empty_like(congest);
    hipLaunchKernelGGL(episode_summary_kernel, dim3(B), dim3(64), 0,
                       cur_stream(), delay_emp.data_ptr<float>(),
                       mask.data_ptr<bool>(), T_arr.data_ptr<float>(),
                       tau.data_ptr<float>(), congest.data_ptr<long>(),
                       num_jobs.data_ptr<long>(), J);
    return {tau, congest, num_jobs};
}

std::vector<torch::Tensor> jobs_from_draws_hip(
    torch::Tensor scores_raw, torch::Tensor r_nj, torch::Tensor r_rates,
    torch::Tensor mobile_mask, double arrival_scale) {
    check_f32(scores_raw, "scores_raw");
    check_f32(r_nj, "r_nj");
    check_f32(r_rates, "r_rates");
    const int B = scores_raw.size(0), N = scores_raw.size(1);
    const int J = r_rates.size(1);
    TORCH_CHECK(mobile_mask.scalar_type() == torch::kBool
                && mobile_mask.is_contiguous()
                && mobile_mask.sizes() == scores_raw.sizes()
                && r_nj.numel() == B && r_rates.size(0) == B && J >= 1
                && J <= N, "shape mismatch");
    const size_t lds = sizeof(float) * N + sizeof(int) * (J + 1);
    TORCH_CHECK(lds <= LDS_LIMIT, "N too large for the job-sampling kernel");
    auto fo = scores_raw.options();
    auto sources = torch::empty({B, J}, fo.dtype(torch::kLong));
    auto mask = torch::empty({B, J}, fo.dtype(torch::kBool));
    auto rates = torch::empty({B, J}, fo);
    auto ul = torch::empty({B, J}, fo);
    auto dl = torch::empty({B, J}, fo);
    hipLaunchKernelGGL(jobs_from_draws_kernel, dim3(B), dim3(256), lds,
                       cur_stream(), scores_raw.data_ptr<float>(),
                       r_nj.data_ptr<float>(), r_rates.data_ptr<float>(),
                       mobile_mask.data_ptr<bool>(), (float)arrival_scale, N,
                       J, sources.data_ptr<long>(), mask.data_ptr<bool>(),
                       rates.data_ptr<float>(), ul.data_ptr<float>(),
                       dl.data_ptr<float>());
    return {sources, mask, rates, ul, dl};
}
