// Fused queueing-model kernels for gfx950: the differentiable contention
// fixed point + congestion-fallback delays, forward AND hand-derived
// reverse-mode, one workgroup per graph with LDS-staged state.
//
// critic_kernel  — the whole critic of the reference
//   (gnn_offloading_agent.py:333-374 loss/grad-wrt-routes + :384-416
//   route-bias VJP) in ONE kernel: route loads → 10-iteration fixed point
//   (history in LDS) → unit delays → loss → closed-form reverse through the
//   unrolled iterations → per-route prefix scan → grad_edge.
// actor_head_fwd/bwd — the actor delay head (:229-274): λ → fixed point →
//   link/node delays → N×N delay matrix, and its VJP (grad_dist → δλ).
//
// The fixed point, the delay units and each kernel's LDS plan (regions,
// launch size, LDS-resident or global-scratch "large" mode) are in
// queue_model.h.
//
// Gradient conventions match torch autograd exactly (tests):
//   clamp passes gradient at the boundaries inclusive;
//   torch.maximum splits the gradient 0.5/0.5 at exact ties.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "queue_model.h"

namespace {

using namespace qm;

// ---------------------------------------------------------------------------
// critic: loss + grad_edge in one pass.
// ---------------------------------------------------------------------------
__global__ void critic_kernel(
    const int* __restrict__ route_links,   // (B,J,H) -1 pad
    const int* __restrict__ nhop,          // (B,J)
    const long* __restrict__ vedge_dst,    // (B,J) slots | nodes (node_vedge)
    const long* __restrict__ node_vedge,   // (B,N) | nullptr
    const bool* __restrict__ mask,         // (B,J)
    const float* __restrict__ rate,        // (B,J)
    const float* __restrict__ ul,          // (B,J)
    const float* __restrict__ dl,          // (B,J)
    const Tables t,                        // bw = bw_comp (B,C)
    float* __restrict__ grad_edge,         // (B,Ee) out (large: prezeroed)
    float* __restrict__ loss_out,          // (B,) out
    float* __restrict__ g_hist,            // (B,(iters+1),E) scratch | null
    float* __restrict__ g_dunit,           // (B,Ee) scratch (prezeroed)
    float* __restrict__ g_dlam,            // (B,Ee) scratch (prezeroed)
    const CriticPlan p,
    float cap,                             // delay clamp (0 = off)
    int stage_budget,                      // CSR staging bytes (0 = none)
    int E, int C, int Ee, int J, int H, int iters, int N) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    const int b = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    // the compute slot of job bj's destination: handed in, or looked up
    // from the destination node
    const long* nvb = node_vedge ? node_vedge + (size_t)b * N : nullptr;
    auto dst_slot = [&](size_t bj) {
        const long d = vedge_dst[bj];
        return (int)(nvb ? nvb[d] : d);
    };
    // large graphs (e.g. 1000-node ER): reverse-pass accumulators and the mu
    // history live in global scratch (same-CU coherence through
    // __syncthreads suffices — one workgroup per graph)
    float* lam_e = lds + p.lam_e;
    float* unit = lds + p.unit;
    float* dunit = region(lds, p.dunit, g_dunit + (size_t)b * Ee);
    float* dlam = region(lds, p.dlam, g_dlam + (size_t)b * Ee);
    float* dgre = region(lds, p.dgre, grad_edge + (size_t)b * Ee);
    float* hist = region(lds, p.hist, g_hist + (size_t)b * (iters + 1) * E);
    float* s1 = lds + p.s1;
    float* s2 = lds + p.s2;
    float* s3 = lds + p.s3;
    __shared__ float loss_acc;
    const Graph g = graph_view(t, b);
    const Csr csr = stage_csr(g.cip, g.rates, g.ccols, g.Eb,
                              smem_raw + stage_align(p.lds_bytes),
                              stage_budget, tid, nt);

    for (int e = tid; e < Ee; e += nt) {
        lam_e[e] = 0.f;
        if (!p.large) { dunit[e] = 0.f; dlam[e] = 0.f; dgre[e] = 0.f; }
        // (large mode: the global scratch arrives prezeroed)
    }
    if (tid == 0) loss_acc = 0.f;
    __syncthreads();

    // ---- route loads: lam_ext = routes @ (rate*ul) -----------------------
    for (int j = tid; j < J; j += nt) {
        const size_t bj = (size_t)b * J + j;
        if (!mask[bj]) continue;
        const float load = rate[bj] * ul[bj];
        const int nh = nhop[bj];
        for (int h = 0; h < nh; ++h) {
            const int l = route_links[bj * H + h];
            if (l < 0) break;
            atomicAdd(&lam_e[l], load);
        }
        atomicAdd(&lam_e[dst_slot(bj)], load);
    }
    __syncthreads();

    // ---- fixed point + unit delays ---------------------------------------
    fixed_point_fwd(csr, lam_e, hist, s1, g.Eb, E, iters, tid, nt);
    const float* mu_last = hist + (size_t)iters * E;
    for (int e = tid; e < g.Eb; e += nt)
        unit[e] = unit_fwd(lam_e[e], mu_last[e], g.T, 101.0f, cap);
    for (int k = tid; k < C; k += nt)
        unit[E + k] = unit_fwd(lam_e[E + k], g.bw[k], g.T, 100.0f, cap);
    __syncthreads();

    // ---- loss + dL/dunit over route entries ------------------------------
    float lloc = 0.f;
    for (int j = tid; j < J; j += nt) {
        const size_t bj = (size_t)b * J + j;
        if (!mask[bj]) continue;
        const float data = ul[bj] + dl[bj];
        const int nh = nhop[bj];
        for (int h = 0; h <= nh; ++h) {
            const int e = (h < nh) ? route_links[bj * H + h]
                                   : dst_slot(bj);
            if (e < 0) break;
            const float x = data * unit[e];
            lloc += x > 1.f ? x : 1.f;
            // d max(x*r, r)/d unit at r=1, torch tie 0.5/0.5
            const float wx = x > 1.f ? 1.f : (x < 1.f ? 0.f : 0.5f);
            atomicAdd(&dunit[e], data * wx);
        }
    }
    atomicAdd(&loss_acc, lloc);
    __syncthreads();

    // ---- reverse: dunit → (dlam over links via fixed point, direct nodes)
    for (int e = tid; e < g.Eb; e += nt) {
        float dl_, dm_;
        unit_bwd(lam_e[e], mu_last[e], g.T, 101.0f, cap, dunit[e], &dl_,
                 &dm_);
        dlam[e] += dl_;
        s2[e] = dm_;                               // dmu into the reverse
    }
    for (int k = tid; k < C; k += nt) {
        float dl_, dm_;
        unit_bwd(lam_e[E + k], g.bw[k], g.T, 100.0f, cap, dunit[E + k], &dl_,
                 &dm_);
        dlam[E + k] += dl_;                        // bw is constant
    }
    __syncthreads();
    fixed_point_bwd(csr, lam_e, hist, s2 /*dmu*/, s1 /*dnb*/, s3 /*dbusy*/,
                    dlam, g.Eb, E, iters, tid, nt);
    __syncthreads();

    // ---- grad_routes prefix scan → grad_edge -----------------------------
    for (int j = tid; j < J; j += nt) {
        const size_t bj = (size_t)b * J + j;
        if (!mask[bj]) continue;
        const float data = ul[bj] + dl[bj];
        const float load = rate[bj] * ul[bj];
        const int nh = nhop[bj];
        float run = 0.f;
        for (int h = 0; h <= nh; ++h) {
            const int e = (h < nh) ? route_links[bj * H + h]
                                   : dst_slot(bj);
            if (e < 0) break;
            const float x = data * unit[e];
            const float wx = x > 1.f ? 1.f : (x < 1.f ? 0.f : 0.5f);
            const float direct = data * unit[e] * wx + (1.f - wx);
            const float gr = direct + dlam[e] * load;
            run += gr;
            atomicAdd(&dgre[e], -run);
        }
    }
    __syncthreads();
    if (!p.large) {
        float* geb = grad_edge + (size_t)b * Ee;
        for (int e = tid; e < Ee; e += nt) geb[e] = dgre[e];
    }
    if (tid == 0) loss_out[b] = loss_acc;
}

// ---------------------------------------------------------------------------
// actor head forward: λ_ext → delays → (B,N,N) delay matrix; saves mu
// history + λ for backward.
// ---------------------------------------------------------------------------
__global__ void actor_head_fwd_kernel(
    const float* __restrict__ lam_ext,     // (B,Ee)
    const Tables t,                        // bw = bw_comp (B,C)
    const int* __restrict__ edges,         // (B,E,2)
    const long* __restrict__ node_vedge,   // (B,N)
    float* __restrict__ dm,                // (B,N,N) out (prezeroed)
    float* __restrict__ mu_hist_out,       // (B,(iters+1),E) out
    const ActorFwdPlan p, float cap, int stage_budget, int N, int E, int C,
    int Ee, int iters) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    const int b = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    float* ho = mu_hist_out + (size_t)b * (iters + 1) * E;
    float* lam = lds + p.lam;
    float* hist = region(lds, p.hist, ho);
    float* busy = lds + p.busy;
    const Graph g = graph_view(t, b);
    const float* le = lam_ext + (size_t)b * Ee;
    const int* edg = edges + (size_t)b * E * 2;
    const long* nv = node_vedge + (size_t)b * N;
    float* dmb = dm + (size_t)b * N * N;

    for (int e = tid; e < g.Eb; e += nt) lam[e] = le[e];
    const Csr csr = stage_csr(g.cip, g.rates, g.ccols, g.Eb,
                              smem_raw + stage_align(p.lds_bytes),
                              stage_budget, tid, nt);
    __syncthreads();
    fixed_point_fwd(csr, lam, hist, busy, g.Eb, E, iters, tid, nt);
    const float* mu_last = hist + (size_t)iters * E;
    for (int e = tid; e < g.Eb; e += nt) {
        const float d = unit_fwd(lam[e], mu_last[e], g.T, 101.0f, cap);
        const int u = edg[e * 2], v = edg[e * 2 + 1];
        dmb[(size_t)u * N + v] = d;
        dmb[(size_t)v * N + u] = d;
    }
    for (int n = tid; n < N; n += nt) {
        const long ve = nv[n];
        dmb[(size_t)n * N + n] =
            ve >= 0 ? unit_fwd(le[ve], g.bw[ve - E], g.T, 100.0f, cap)
                    : INFINITY;
    }
    if (!p.large) {
        for (size_t i = tid; i < (size_t)(iters + 1) * E; i += nt)
            ho[i] = hist[i];
    }
}

// ---- cotangent sources of the actor head backward ------------------------
// The backward needs the (B,N,N) cotangent only at the cells the forward
// wrote: both directions of every real link and the diagonal.  DenseCot
// reads them from a dense tensor; FusedCot assembles them on the fly from
// the critic's grad_edge and the 0.001·MSE anchor, and sums the anchor's
// squared error on the way (engine.grad_dist_matrix without its dozen
// (B,N,N) passes).
struct DenseCot {
    const float* grad_dist;                // (B,N,N)
    DEV_INLINE float cell(int b, int N, int r, int c, int /*edge*/,
                          float& /*sq*/, int& /*cnt*/) const {
        return grad_dist[((size_t)b * N + r) * N + c];
    }
    DEV_INLINE void finish(int, float, int, float*, float*) const {}
};

struct FusedCot {
    const float* grad_edge;                // (B,Ee)
    const float* dm;                       // (B,N,N) valid on link+diag cells
    const float* unit_mtx;                 // (B,N,N) meaningful where written
    const bool* written;                   // (B,N,N)
    float* mse_sq;                         // (B) Σ diff²
    int* mse_cnt;                          // (B) anchor cells
    int Ee;
    // grad_edge[edge] + anchor(r,c); edge < 0 (a node without a compute
    // slot) contributes the anchor alone.  unit_mtx is read only where
    // written is set, dm only on the cells this kernel visits (the actor
    // head leaves dm uninitialised elsewhere).
    DEV_INLINE float cell(int b, int N, int r, int c, int edge, float& sq,
                          int& cnt) const {
#pragma clang fp contract(off)
        const size_t i = ((size_t)b * N + r) * N + c;
        float a = 0.f;
        if (written[i]) {
            const float d = dm[i];
            if (isfinite(d)) {
                const float diff = d - unit_mtx[i];
                a = 0.001f * diff;
                sq += diff * diff;
                cnt += 1;
            }
        }
        const float ge = edge >= 0 ? grad_edge[(size_t)b * Ee + edge] : 0.f;
        return ge + a;
    }
    // one (Σ, count) pair per graph; called by every thread of the block.
    // The two accumulators are cells of the plan's own LDS that the kernel
    // has finished with (no static LDS on top of the plan's bytes).
    DEV_INLINE void finish(int b, float sq, int cnt, float* free1,
                           float* free2) const {
        float* s_sq = free1;
        int* s_cnt = reinterpret_cast<int*>(free2);
        if (threadIdx.x == 0) { *s_sq = 0.f; *s_cnt = 0; }
        __syncthreads();
        if (cnt) { atomicAdd(s_sq, sq); atomicAdd(s_cnt, cnt); }
        __syncthreads();
        if (threadIdx.x == 0) {
            mse_sq[b] = *s_sq;
            mse_cnt[b] = *s_cnt;
        }
    }
};

// loss_mse = Σ_b Σ diff² / max(Σ_b count, 1), one block; with `loss`
// (the critic's per-graph loss) also loss_fn = Σ_b loss[b] from the same
// strided partials and 256-wide tree
__global__ void mse_finish_kernel(const float* __restrict__ mse_sq,
                                  const int* __restrict__ mse_cnt,
                                  const float* __restrict__ loss, int B,
                                  float* __restrict__ out,
                                  float* __restrict__ loss_out) {
    __shared__ float s_sq[256];
    __shared__ float s_ls[256];
    __shared__ long long s_cnt[256];       // integer count, like torch's
    float sq = 0.f, ls = 0.f;
    long long cnt = 0;
    for (int b = threadIdx.x; b < B; b += 256) {
        sq += mse_sq[b];
        cnt += mse_cnt[b];
        if (loss) ls += loss[b];
    }
    s_sq[threadIdx.x] = sq;
    s_ls[threadIdx.x] = ls;
    s_cnt[threadIdx.x] = cnt;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (threadIdx.x < w) {
            s_sq[threadIdx.x] += s_sq[threadIdx.x + w];
            s_ls[threadIdx.x] += s_ls[threadIdx.x + w];
            s_cnt[threadIdx.x] += s_cnt[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        out[0] = s_sq[0] / (float)(s_cnt[0] > 1 ? s_cnt[0] : 1);
        if (loss) loss_out[0] = s_ls[0];
    }
}

// actor head backward: cotangent on dm (dense or fused, see above) → δλ_ext
// (B,Ee)
template <class Cot>
__global__ void actor_head_bwd_kernel(
    const Cot cot,
    const float* __restrict__ lam_ext,     // (B,Ee)
    const float* __restrict__ mu_hist,     // (B,(iters+1),E)
    const Tables t,                        // bw = bw_comp (B,C)
    const int* __restrict__ edges,
    const long* __restrict__ node_vedge,
    float* __restrict__ dlam_ext,          // (B,Ee) out
    const ActorBwdPlan p, float cap, int stage_budget, int N, int E, int C,
    int Ee, int iters) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    const int b = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const float* hg = mu_hist + (size_t)b * (iters + 1) * E;
    float* lam = lds + p.lam;
    const float* hist = region(lds, p.hist, hg);
    float* dmu = lds + p.dmu;
    float* dlam = lds + p.dlam;
    float* s1 = lds + p.s1;
    float* s2 = lds + p.s2;
    const Graph g = graph_view(t, b);
    const float* le = lam_ext + (size_t)b * Ee;
    const int* edg = edges + (size_t)b * E * 2;
    const long* nv = node_vedge + (size_t)b * N;
    float* out = dlam_ext + (size_t)b * Ee;
    float sq = 0.f;                        // FusedCot's anchor error
    int cnt = 0;

    // dlam_ext arrives torch::empty: the link part is written whole below,
    // the node part only at the slots that exist — zero [E, Ee) here, before
    // the first barrier (a graph with fewer computing nodes, a padded tail)
    for (int e = E + tid; e < Ee; e += nt) out[e] = 0.f;
    for (int e = tid; e < g.Eb; e += nt) lam[e] = le[e];
    if (!p.large) {
        float* h = lds + p.hist;
        for (size_t i = tid; i < (size_t)(iters + 1) * E; i += nt)
            h[i] = hg[i];
    }
    const Csr csr = stage_csr(g.cip, g.rates, g.ccols, g.Eb,
                              smem_raw + stage_align(p.lds_bytes),
                              stage_budget, tid, nt);
    __syncthreads();
    const float* mu_last = hist + (size_t)iters * E;

    // link part: cotangent = gd[u,v] + gd[v,u] (dm wrote both)
    for (int e = tid; e < g.Eb; e += nt) {
        const int u = edg[e * 2], v = edg[e * 2 + 1];
        const float dd = cot.cell(b, N, u, v, e, sq, cnt)
            + cot.cell(b, N, v, u, e, sq, cnt);
        float dl_, dm_;
        unit_bwd(lam[e], mu_last[e], g.T, 101.0f, cap, dd, &dl_, &dm_);
        dlam[e] = dl_;
        dmu[e] = dm_;
    }
    __syncthreads();
    fixed_point_bwd(csr, lam, hist, dmu, s1, s2, dlam, g.Eb, E, iters, tid,
                    nt);

    for (int e = tid; e < E; e += nt) out[e] = e < g.Eb ? dlam[e] : 0.f;
    // node part: diagonal cotangent, direct (no fixed point)
    for (int n = tid; n < N; n += nt) {
        const long ve = nv[n];
        // every diagonal cell is visited: the anchor error counts it even
        // where there is no compute slot to hand a gradient to
        const float dd = cot.cell(b, N, n, n, (int)ve, sq, cnt);
        if (ve >= 0) {
            float dl_, dm_;
            unit_bwd(le[ve], g.bw[ve - E], g.T, 100.0f, cap, dd, &dl_, &dm_);
            out[ve] = dl_;
        }
    }
    // s1 / s2 were last read inside fixed_point_bwd, behind its barrier
    cot.finish(b, sq, cnt, s1, s2);
}

}  // namespace

std::vector<torch::Tensor> critic_hip(
    torch::Tensor route_links, torch::Tensor nhop, torch::Tensor vedge_dst,
    torch::Tensor mask, torch::Tensor rate, torch::Tensor ul,
    torch::Tensor dl, torch::Tensor conf_indptr, torch::Tensor conf_base,
    torch::Tensor conf_cols, torch::Tensor rates, torch::Tensor bw_comp,
    torch::Tensor E_arr, torch::Tensor T_arr, long Ee, long iters,
    double cap, c10::optional<torch::Tensor> node_vedge) {
    const int B = route_links.size(0), J = route_links.size(1);
    const int H = route_links.size(2);
    const int E = rates.size(1), C = bw_comp.size(1);
    // with node_vedge (B,N), `vedge_dst` holds the destination NODES and the
    // kernel looks their compute slots up itself
    const long* nv = nullptr;
    int N = 0;
    if (node_vedge.has_value()) {
        TORCH_CHECK(node_vedge->scalar_type() == torch::kInt64
                    && node_vedge->dim() == 2 && node_vedge->size(0) == B
                    && node_vedge->is_contiguous()
                    && vedge_dst.is_contiguous(),
                    "critic: node_vedge is a contiguous (B,N) int64");
        nv = node_vedge->data_ptr<long>();
        N = node_vedge->size(1);
    }
    auto loss = torch::empty({B}, rates.options());
    const CriticPlan p = critic_plan(E, (int)Ee, (int)iters);
    TORCH_CHECK(p.fits, "graph too large even for the global-scratch critic");
    torch::Tensor g_hist, g_dunit, g_dlam;
    torch::Tensor grad_edge;
    if (p.large) {
        g_hist = torch::empty({B, iters + 1, (long)E}, rates.options());
        g_dunit = torch::zeros({B, (long)Ee}, rates.options());
        g_dlam = torch::zeros({B, (long)Ee}, rates.options());
        grad_edge = torch::zeros({B, (long)Ee}, rates.options());
    } else {
        g_hist = torch::empty({1}, rates.options());
        g_dunit = g_hist;
        g_dlam = g_hist;
        // small mode copies the full dgre LDS row out — no prezero needed
        grad_edge = torch::empty({B, (long)Ee}, rates.options());
    }
    auto stream = at::cuda::getCurrentCUDAStream();
    const int budget = stage_budget(p);
    hipLaunchKernelGGL(critic_kernel, dim3(B), dim3(p.threads),
                       launch_lds_bytes(p, budget), stream.stream(),
                       route_links.data_ptr<int>(), nhop.data_ptr<int>(),
                       vedge_dst.data_ptr<long>(), nv, mask.data_ptr<bool>(),
                       rate.data_ptr<float>(), ul.data_ptr<float>(),
                       dl.data_ptr<float>(),
                       tables(conf_indptr, conf_base, conf_cols, rates,
                              bw_comp, T_arr, E_arr),
                       grad_edge.data_ptr<float>(), loss.data_ptr<float>(),
                       g_hist.data_ptr<float>(), g_dunit.data_ptr<float>(),
                       g_dlam.data_ptr<float>(), p, (float)cap, budget,
                       E, C, (int)Ee, J, H, (int)iters, N);
    return {grad_edge, loss};
}

std::vector<torch::Tensor> actor_head_fwd_hip(
    torch::Tensor lam_ext, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw_comp, torch::Tensor edges, torch::Tensor node_vedge,
    torch::Tensor T_arr, torch::Tensor E_arr, long N, long iters,
    double cap) {
    const int B = lam_ext.size(0), Ee = lam_ext.size(1);
    const int E = rates.size(1), C = bw_comp.size(1);
    // every cell a consumer reads (real links both directions + the full
    // diagonal) is written by the kernel; non-edge cells are masked by
    // adj / `written` everywhere downstream — skip the fill launch
    auto dm = torch::empty({B, N, N}, lam_ext.options());
    auto mu_hist = torch::empty({B, iters + 1, (long)E}, lam_ext.options());
    const ActorFwdPlan p = actor_fwd_plan(E, (int)iters);
    TORCH_CHECK(p.fits, "graph too large for LDS actor head");
    auto stream = at::cuda::getCurrentCUDAStream();
    const int budget = stage_budget(p);
    hipLaunchKernelGGL(actor_head_fwd_kernel, dim3(B), dim3(p.threads),
                       launch_lds_bytes(p, budget), stream.stream(),
                       lam_ext.data_ptr<float>(),
                       tables(conf_indptr, conf_base, conf_cols, rates,
                              bw_comp, T_arr, E_arr),
                       edges.data_ptr<int>(), node_vedge.data_ptr<long>(),
                       dm.data_ptr<float>(), mu_hist.data_ptr<float>(),
                       p, (float)cap, budget, (int)N, E, C, Ee, (int)iters);
    return {dm, mu_hist};
}

namespace {

template <class Cot>
torch::Tensor actor_head_bwd_launch(
    const Cot& cot, int N, torch::Tensor lam_ext, torch::Tensor mu_hist,
    torch::Tensor conf_indptr, torch::Tensor conf_base,
    torch::Tensor conf_cols, torch::Tensor rates, torch::Tensor bw_comp,
    torch::Tensor edges, torch::Tensor node_vedge, torch::Tensor T_arr,
    torch::Tensor E_arr, long iters, double cap) {
    const int B = lam_ext.size(0), Ee = lam_ext.size(1);
    const int E = rates.size(1), C = bw_comp.size(1);
    auto dlam = torch::empty_like(lam_ext);    // the kernel writes all of it
    const ActorBwdPlan p = actor_bwd_plan(E, (int)iters);
    TORCH_CHECK(p.fits, "graph too large for LDS actor head bwd");
    auto stream = at::cuda::getCurrentCUDAStream();
    const int budget = stage_budget(p);
    hipLaunchKernelGGL(actor_head_bwd_kernel<Cot>, dim3(B), dim3(p.threads),
                       launch_lds_bytes(p, budget), stream.stream(), cot,
                       lam_ext.data_ptr<float>(), mu_hist.data_ptr<float>(),
                       tables(conf_indptr, conf_base, conf_cols, rates,
                              bw_comp, T_arr, E_arr),
                       edges.data_ptr<int>(), node_vedge.data_ptr<long>(),
                       dlam.data_ptr<float>(),
                       p, (float)cap, budget, N, E, C, Ee, (int)iters);
    return dlam;
}

}  // namespace

torch::Tensor actor_head_bwd_hip(
    torch::Tensor grad_dist, torch::Tensor lam_ext, torch::Tensor mu_hist,
    torch::Tensor conf_indptr, torch::Tensor conf_base,
    torch::Tensor conf_cols, torch::Tensor rates, torch::Tensor bw_comp,
    torch::Tensor edges, torch::Tensor node_vedge, torch::Tensor T_arr,
    torch::Tensor E_arr, long iters, double cap) {
    return actor_head_bwd_launch(
        DenseCot{grad_dist.data_ptr<float>()}, (int)grad_dist.size(1),
        lam_ext, mu_hist, conf_indptr, conf_base, conf_cols, rates, bw_comp,
        edges, node_vedge, T_arr, E_arr, iters, cap);
}

// Same backward with the cotangent assembled in the kernel:
//   link e=(u,v):  (ge[e] + a(u,v)) + (ge[e] + a(v,u))
//   node n, slot ve:  ge[ve] + a(n,n)
//   a(c) = written[c] && isfinite(dm[c]) ? 0.001·(dm[c] − unit_mtx[c]) : 0
// in the association order of `grad_dist + anchor` followed by the dense
// kernel's gd[u,v] + gd[v,u], so dλ is bit-equal to the dense route.
// walk_eval_kernel (episode.hip, stages 3/3b) sets `written` only at
// (u,v)/(v,u) of a routed real link and at (d,d) of a destination, i.e.
// inside the 2·E_b + N cells visited here, so the anchor mask is covered.
// Returns (dλ (B,Ee), loss_mse 0-dim), and with `critic_loss` (the critic's
// per-graph loss) a third 0-dim tensor, its sum.
std::vector<torch::Tensor> actor_head_bwd_fused_hip(
    torch::Tensor grad_edge, torch::Tensor dm, torch::Tensor unit_mtx,
    torch::Tensor written, torch::Tensor lam_ext, torch::Tensor mu_hist,
    torch::Tensor conf_indptr, torch::Tensor conf_base,
    torch::Tensor conf_cols, torch::Tensor rates, torch::Tensor bw_comp,
    torch::Tensor edges, torch::Tensor node_vedge, torch::Tensor T_arr,
    torch::Tensor E_arr, long iters, double cap,
    c10::optional<torch::Tensor> critic_loss) {
    const int B = lam_ext.size(0), Ee = lam_ext.size(1);
    const int N = dm.size(1);
    if (critic_loss.has_value())
        TORCH_CHECK(critic_loss->scalar_type() == torch::kFloat32
                    && critic_loss->numel() == B
                    && critic_loss->is_contiguous(),
                    "critic_loss is the critic's (B,) fp32 loss");
    TORCH_CHECK(grad_edge.is_contiguous() && dm.is_contiguous()
                && unit_mtx.is_contiguous() && written.is_contiguous()
                && lam_ext.is_contiguous(), "contiguous inputs expected");
    TORCH_CHECK(grad_edge.size(0) == B && grad_edge.size(1) == Ee
                && dm.size(0) == B && dm.size(2) == N
                && unit_mtx.sizes() == dm.sizes()
                && written.sizes() == dm.sizes(), "shape mismatch");
    auto mse_sq = torch::empty({B}, lam_ext.options());
    auto mse_cnt = torch::empty({B}, lam_ext.options().dtype(torch::kInt));
    auto dlam = actor_head_bwd_launch(
        FusedCot{grad_edge.data_ptr<float>(), dm.data_ptr<float>(),
                 unit_mtx.data_ptr<float>(), written.data_ptr<bool>(),
                 mse_sq.data_ptr<float>(), mse_cnt.data_ptr<int>(), Ee},
        N, lam_ext, mu_hist, conf_indptr, conf_base, conf_cols, rates,
        bw_comp, edges, node_vedge, T_arr, E_arr, iters, cap);
    auto loss_mse = torch::empty({}, lam_ext.options());
    auto loss_fn = torch::empty({}, lam_ext.options());
    hipLaunchKernelGGL(mse_finish_kernel, dim3(1), dim3(256), 0,
                       at::cuda::getCurrentCUDAStream().stream(),
                       mse_sq.data_ptr<float>(), mse_cnt.data_ptr<int>(),
                       critic_loss.has_value()
                           ? critic_loss->data_ptr<float>() : nullptr,
                       B, loss_mse.data_ptr<float>(),
                       loss_fn.data_ptr<float>());
    if (critic_loss.has_value()) return {dlam, loss_mse, loss_fn};
    return {dlam, loss_mse};
}

// Host-only: what each queueing kernel's launcher would launch with at this
// shape (nothing is launched).  The engine takes its per-stage fit flags
// from here and the tests ask it which mode a shape reaches.
py::dict queue_lds_plan(long N, long E, long Ee, long iters) {
    using namespace pybind11::literals;
    auto row = [](const Launch& l) {
        return py::dict("lds_bytes"_a = l.lds_bytes, "large"_a = l.large,
                        "threads"_a = l.threads, "fits"_a = l.fits);
    };
    return py::dict(
        "critic"_a = row(critic_plan((int)E, (int)Ee, (int)iters)),
        "actor_head_fwd"_a = row(actor_fwd_plan((int)E, (int)iters)),
        "actor_head_bwd"_a = row(actor_bwd_plan((int)E, (int)iters)),
        "walk_eval"_a = row(walk_plan((int)N, (int)E)));
}

// Host-only: the CSR staging area each launcher adds to its plan's bytes at
// this shape, with the current setting (0: the launch reads the conflict CSR
// from global memory).  Inside a launch a workgroup stages its graph's CSR
// when queue_csr_bytes(E_b, nnz_b) is within that budget and E_b fits 16
// bits.
py::dict queue_csr_stage(long N, long E, long Ee, long iters) {
    using namespace pybind11::literals;
    auto row = [](const Launch& l) {
        return py::dict("budget_bytes"_a = stage_budget(l));
    };
    return py::dict(
        "critic"_a = row(critic_plan((int)E, (int)Ee, (int)iters)),
        "actor_head_fwd"_a = row(actor_fwd_plan((int)E, (int)iters)),
        "actor_head_bwd"_a = row(actor_bwd_plan((int)E, (int)iters)),
        "walk_eval"_a = row(walk_plan((int)N, (int)E)));
}

long queue_csr_bytes(long Eb, long nnz) {
    return Eb <= STAGE_MAX_E ? (long)stage_bytes(Eb, nnz) : -1;
}

// force every later launch onto the global-memory CSR (before/after timings,
// staged-vs-global tests)
void queue_csr_force_global(bool on) { stage_force_global = on; }

// staging bytes per workgroup of later launches; negative restores the
// default.  Returns the previous setting.
long queue_csr_set_budget(long bytes) {
    const long prev = stage_budget_setting;
    stage_budget_setting = bytes < 0 ? STAGE_BUDGET_DEFAULT : (int)bytes;
    return prev;
}
