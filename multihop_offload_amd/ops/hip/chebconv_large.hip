// Row-tiled ChebConv for graphs whose activations exceed the LDS budget
// (e.g. 1000-node ER: Ē ≈ 8.5k rows) — BASELINE config 4.
//
// Layout: activations live in the (B, L+1, Ē, 32) acts tensor (global, L2-
// resident at these sizes); each block owns a 64-row tile of one graph and
// stages its X tile + the SpMV result tile in LDS (~42 KB → 3 blocks/CU).
// The dense products run on the same mfma_f32_16x16x4 tiles as the
// LDS-resident kernel (cheb_tiles.h).  One launch per layer forward; two
// per layer backward (the dX SpMV needs the full U = δ·W1ᵀ materialized
// first).

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "cheb_tiles.h"

namespace {

using namespace cheb;

constexpr int RT = 64;         // rows per tile

// dst_tile(LDS, RT×STRIDE) = rows [r0, r0+RT) of (A · src_global)
DEV_INLINE void spmv_tile(const float* __restrict__ src, float* __restrict__
                          dst, const int* __restrict__ indptr,
                          const int* __restrict__ cols, int r0, int Ee,
                          int tid, int nt) {
    for (int task = tid; task < RT * (F / 4); task += nt) {
        const int rr = task >> 3;
        const int c0 = (task & 7) * 4;
        const int r = r0 + rr;
        float4 acc = {0.f, 0.f, 0.f, 0.f};
        if (r < Ee) acc = csr_gather4(src, indptr, cols, r, c0);
        float* d = dst + rr * STRIDE + c0;
        d[0] = acc.x; d[1] = acc.y; d[2] = acc.z; d[3] = acc.w;
    }
}

// ---- forward, one layer: acts[l+1] = act(X·W0 + (A·X)·W1 + b) -----------
__global__ void cheb_large_fwd_layer(
    const float* __restrict__ x_l,       // (B,Ee,32) = acts[l]
    float* __restrict__ x_next,          // (B,Ee,32) = acts[l+1]
    const float* __restrict__ W,         // (K,32,32) this layer (padded)
    const float* __restrict__ bias,      // (32)
    const int* __restrict__ ext_indptr,  // (B,Ee+1)
    const long* __restrict__ ext_base,
    const int* __restrict__ ext_cols,
    long x_stride,                       // per-graph elements in x_l/x_next
    int Ee, int K, int last) {
    __shared__ __attribute__((aligned(16))) float Xt[RT * STRIDE];
    __shared__ __attribute__((aligned(16))) float Tt[RT * STRIDE];
    __shared__ __attribute__((aligned(16))) float Yt[RT * STRIDE];
    __shared__ float Wl[2 * F * F];
    __shared__ float bl[F];

    const int b = blockIdx.y;
    const int r0 = blockIdx.x * RT;
    const int tid = threadIdx.x, nt = blockDim.x;
    const float* xb = x_l + (size_t)b * x_stride;
    const int* ipt = ext_indptr + (size_t)b * (Ee + 1);
    const int* cls = ext_cols + ext_base[b];

    for (int i = tid; i < K * F * F; i += nt) Wl[i] = W[i];
    for (int i = tid; i < F; i += nt) bl[i] = bias[i];
    for (int i = tid; i < RT * STRIDE; i += nt) Yt[i] = 0.f;
    load_rows(Xt, xb, r0, RT, Ee, tid, nt);
    if (K > 1) spmv_tile(xb, Tt, ipt, cls, r0, Ee, tid, nt);
    __syncthreads();
    gemm_rows(Xt, Yt, Wl, false, RT, tid);
    if (K > 1) gemm_rows(Tt, Yt, Wl + F * F, false, RT, tid);
    __syncthreads();
    store_rows(Yt, x_next + (size_t)b * x_stride, r0, RT, Ee, tid, nt,
               [&](float4 y, int c0) {
                   return float4{act(y.x + bl[c0], last),
                                 act(y.y + bl[c0 + 1], last),
                                 act(y.z + bl[c0 + 2], last),
                                 act(y.w + bl[c0 + 3], last)};
               });
}

// ---- backward stage A (per layer): δpre = δ⊙act'(acts[l+1]);
// db/dW partials; U = δpre·W1ᵀ; delta ← δpre·W0ᵀ --------------------------
__global__ void cheb_large_bwd_a(
    float* __restrict__ delta,           // (B,Ee,32) in: δ, out: δpre·W0ᵀ
    float* __restrict__ U,               // (B,Ee,32) out: δpre·W1ᵀ
    const float* __restrict__ x_l,       // acts[l]
    const float* __restrict__ x_next,    // acts[l+1] (post-act mask)
    const float* __restrict__ W,         // (K,32,32)
    float* __restrict__ dW,              // (B,K,32,32) partials (prezeroed)
    float* __restrict__ db,              // (B,32) partials (prezeroed)
    const int* __restrict__ ext_indptr,
    const long* __restrict__ ext_base,
    const int* __restrict__ ext_cols,
    long x_stride, long dw_stride, long db_stride,
    int Ee, int K, int last, int want_dx) {
    __shared__ __attribute__((aligned(16))) float Dt[RT * STRIDE];
    __shared__ __attribute__((aligned(16))) float Xt[RT * STRIDE];
    __shared__ __attribute__((aligned(16))) float Ot[RT * STRIDE];
    __shared__ float Wl[2 * F * F];

    const int b = blockIdx.y;
    const int r0 = blockIdx.x * RT;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int* ipt = ext_indptr + (size_t)b * (Ee + 1);
    const int* cls = ext_cols + ext_base[b];
    float* del = delta + (size_t)b * Ee * F;
    const float* xa = x_next + (size_t)b * x_stride;
    const float* xl = x_l + (size_t)b * x_stride;

    for (int i = tid; i < K * F * F; i += nt) Wl[i] = W[i];
    // δpre tile (mask applied on load)
    const float slope = last ? 0.f : 0.2f;
    load_rows(Dt, del, r0, RT, Ee, tid, nt, [&](float4 d, size_t off) {
        const float4 a = *reinterpret_cast<const float4*>(xa + off);
        d.x *= dact(a.x, slope);
        d.y *= dact(a.y, slope);
        d.z *= dact(a.z, slope);
        d.w *= dact(a.w, slope);
        return d;
    });
    load_rows(Xt, xl, r0, RT, Ee, tid, nt);
    __syncthreads();

    // db partials (column sums of the tile; rows past Ee are zero)
    db_colsum(Dt, RT, db + (size_t)b * db_stride, tid, nt);
    wgrad_rows<1>(Xt, Dt, dW + (size_t)b * dw_stride, RT, tid);
    if (K > 1) {
        __syncthreads();
        spmv_tile(xl, Ot, ipt, cls, r0, Ee, tid, nt);   // T1 tile
        __syncthreads();
        wgrad_rows<1>(Ot, Dt, dW + (size_t)b * dw_stride + F * F, RT, tid);
    }
    if (!want_dx) return;
    __syncthreads();

    // U = δpre·W1ᵀ ; newdelta = δpre·W0ᵀ
    if (K > 1) {
        for (int i = tid; i < RT * STRIDE; i += nt) Ot[i] = 0.f;
        __syncthreads();
        gemm_rows(Dt, Ot, Wl + F * F, true, RT, tid);
        __syncthreads();
        store_rows(Ot, U + (size_t)b * Ee * F, r0, RT, Ee, tid, nt);
    }
    for (int i = tid; i < RT * STRIDE; i += nt) Xt[i] = 0.f;  // reuse as acc
    __syncthreads();
    gemm_rows(Dt, Xt, Wl, true, RT, tid);
    __syncthreads();
    store_rows(Xt, del, r0, RT, Ee, tid, nt);
}

// ---- backward stage B (per layer): delta += A·U --------------------------
__global__ void cheb_large_bwd_b(
    float* __restrict__ delta, const float* __restrict__ U,
    const int* __restrict__ ext_indptr, const long* __restrict__ ext_base,
    const int* __restrict__ ext_cols, int Ee) {
    const int b = blockIdx.y;
    const int r0 = blockIdx.x * RT;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int* ipt = ext_indptr + (size_t)b * (Ee + 1);
    const int* cls = ext_cols + ext_base[b];
    const float* ub = U + (size_t)b * Ee * F;
    float* del = delta + (size_t)b * Ee * F;
    for (int task = tid; task < RT * (F / 4); task += nt) {
        const int rr = task >> 3;
        const int c0 = (task & 7) * 4;
        const int r = r0 + rr;
        if (r >= Ee) continue;
        const float4 acc = csr_gather4(ub, ipt, cls, r, c0);
        float* d = del + (size_t)r * F + c0;
        d[0] += acc.x; d[1] += acc.y; d[2] += acc.z; d[3] += acc.w;
    }
}

}  // namespace

std::vector<torch::Tensor> cheb_large_fwd_hip(
    torch::Tensor x, torch::Tensor W, torch::Tensor bias,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols) {
    const int B = x.size(0), Ee = x.size(1);
    const int L = W.size(0), K = W.size(1);
    TORCH_CHECK(K <= 2, "cheb_large supports K<=2");
    auto acts = torch::zeros({B, L + 1, (long)Ee, F}, x.options());
    // acts[0][:, :4] = x (rest stays zero)
    acts.select(1, 0).narrow(2, 0, 4).copy_(x);
    auto stream = at::cuda::getCurrentCUDAStream();
    const int tiles = (Ee + RT - 1) / RT;
    for (int l = 0; l < L; ++l) {
        hipLaunchKernelGGL(cheb_large_fwd_layer, dim3(tiles, B), dim3(256),
                           0, stream.stream(),
                           acts.select(1, l).data_ptr<float>(),
                           acts.select(1, l + 1).data_ptr<float>(),
                           W.select(0, l).data_ptr<float>(),
                           bias.select(0, l).data_ptr<float>(),
                           ext_indptr.data_ptr<int>(),
                           ext_base.data_ptr<long>(),
                           ext_cols.data_ptr<int>(),
                           (long)(L + 1) * Ee * F, Ee, K,
                           l == L - 1 ? 1 : 0);
    }
    auto lam = acts.select(1, L).select(2, 0).contiguous();   // (B,Ee)
    return {lam, acts};
}

std::vector<torch::Tensor> cheb_large_bwd_hip(
    torch::Tensor dlam, torch::Tensor acts, torch::Tensor W,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols) {
    const int B = dlam.size(0), Ee = dlam.size(1);
    const int L = W.size(0), K = W.size(1);
    auto dW = torch::zeros({B, L, K, F, F}, dlam.options());
    auto db = torch::zeros({B, L, F}, dlam.options());
    auto delta = torch::zeros({B, (long)Ee, F}, dlam.options());
    delta.select(2, 0).copy_(dlam);
    auto U = torch::zeros_like(delta);
    auto stream = at::cuda::getCurrentCUDAStream();
    const int tiles = (Ee + RT - 1) / RT;
    for (int l = L - 1; l >= 0; --l) {
        const int want_dx = l > 0 ? 1 : 0;
        hipLaunchKernelGGL(cheb_large_bwd_a, dim3(tiles, B), dim3(256), 0,
                           stream.stream(),
                           delta.data_ptr<float>(), U.data_ptr<float>(),
                           acts.select(1, l).data_ptr<float>(),
                           acts.select(1, l + 1).data_ptr<float>(),
                           W.select(0, l).data_ptr<float>(),
                           dW.select(1, l).data_ptr<float>(),
                           db.select(1, l).data_ptr<float>(),
                           ext_indptr.data_ptr<int>(),
                           ext_base.data_ptr<long>(),
                           ext_cols.data_ptr<int>(),
                           (long)(L + 1) * Ee * F,
                           (long)L * K * F * F, (long)L * F,
                           Ee, K, l == L - 1 ? 1 : 0, want_dx);
        if (want_dx && K > 1) {
            hipLaunchKernelGGL(cheb_large_bwd_b, dim3(tiles, B), dim3(256),
                               0, stream.stream(),
                               delta.data_ptr<float>(), U.data_ptr<float>(),
                               ext_indptr.data_ptr<int>(),
                               ext_base.data_ptr<long>(),
                               ext_cols.data_ptr<int>(), Ee);
        }
    }
    return {dW, db};
}
