// Fused episode kernels for gfx950: one workgroup per graph, queueing state
// staged in LDS.  These replace the torch gather/scatter/index chains of the
// engine's decision, routing-walk and evaluation stages (profiled at ~35% of
// step GPU time plus the per-hop host sync of the walk loop).
//
// Reference semantics (clean-room): offloading_v3.py:388-550.
// Oracle: multihop_offload_amd/engine.py torch path (tests/test_gpu.py).
//
// ε-greedy exploration and the softmax ("prob") sampling mode run INSIDE
// decide_kernel with a counter-based stateless RNG (splitmix64 over
// (seed, step counter, b, j)): `explore` is read from a device scalar and
// the counter from a device tensor the engine bumps once per step, so the
// whole decision stage is a single launch and hipGraph capture replays
// with fresh randomness.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "queue_model.h"

namespace {

DEV_INLINE float fmax1(float a, float b) { return a > b ? a : b; }

// splitmix64 — stateless counter-based RNG (statistically strong per-call
// avalanche; each (seed, counter, b, j) tuple is an independent draw)
DEV_INLINE unsigned long long mix64(unsigned long long z) {
    z += 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

DEV_INLINE float u01(unsigned long long h) {
    // top 24 bits → [0,1) float
    return (float)(h >> 40) * (1.0f / 16777216.0f);
}

// cost of offloading a job to server node sv: uplink + downlink along the
// shortest path (floored at the hop count) + compute; sp_row/hop_row are
// the rows of the job's source, uds the graph's row with element stride us
DEV_INLINE float server_cost(const float* sp_row, const float* hop_row,
                             const float* uds, long us, int sv, float ulj,
                             float dlj) {
    const float spv = sp_row[sv];
    const float hpv = hop_row[sv];
    return fmax1(spv * ulj, hpv) + fmax1(spv * dlj, hpv)
           + fmax1(uds[sv * us] * ulj, 1.0f);
}

// unnormalised softmax weight of a cost; a non-finite cost weighs nothing
DEV_INLINE float softmax_w(float c, float cmax) {
    return isfinite(c) ? __expf((c < 1e30f ? c : 1e30f) - cmax) : 0.f;
}

// ---------------------------------------------------------------------------
// decide: per-job offloading costs + argmin choice (offloading_v3.py:401-422)
// + in-kernel ε-greedy / softmax sampling (:416-422).
// grid.x = B, threads loop jobs; each thread scans the S servers serially.
// ---------------------------------------------------------------------------
__global__ void decide_kernel(
    const float* __restrict__ sp,       // (B,N,N) diag=0
    const float* __restrict__ hop,      // (B,N,N)
    const float* __restrict__ uds,      // (B,N)   inf at relays, by its
    long uds_sb, long uds_sn,           //         strides (dm's diagonal)
    const int* __restrict__ servers,    // (B,S)   pad -1 (tail-contiguous)
    const long* __restrict__ src,       // (B,J)
    const bool* __restrict__ mask,      // (B,J)
    const float* __restrict__ ul,       // (B,J)
    const float* __restrict__ dl,       // (B,J)
    const float* __restrict__ explore,  // device scalar | nullptr
    const long* __restrict__ rng,       // (2,): seed, step counter | nullptr
    long* __restrict__ dst_out,         // (B,J)
    bool* __restrict__ islocal_out,     // (B,J)
    int prob, int N, int J, int S) {
    const int b = blockIdx.x;
    const float* spb = sp + (size_t)b * N * N;
    const float* hpb = hop + (size_t)b * N * N;
    const float* udsb = uds + (size_t)b * uds_sb;
    const int* srvb = servers + (size_t)b * S;
    const float eps = explore ? *explore : 0.0f;
    const unsigned long long key =
        rng ? mix64((unsigned long long)rng[0]
                    ^ mix64((unsigned long long)rng[1])) : 0ull;
    int nS = 0;
    for (int s = 0; s < S; ++s) nS += (srvb[s] >= 0);
    for (int j = threadIdx.x; j < J; j += blockDim.x) {
        const size_t bj = (size_t)b * J + j;
        const int s0 = (int)src[bj];
        if (!mask[bj]) { dst_out[bj] = s0; islocal_out[bj] = true; continue; }
        const float ulj = ul[bj], dlj = dl[bj];
        const float local = udsb[s0 * uds_sn] * ulj;
        const float* sp_row = spb + (size_t)s0 * N;
        const float* hop_row = hpb + (size_t)s0 * N;
        int best_s;
        if (prob) {
            // softmax over raw costs (the reference's prob mode quirk:
            // HIGH-cost servers get HIGH probability — util.py:113-116);
            // three passes that each recompute the cost instead of storing
            // S of them per thread: max, sum, then inverse-CDF walk with one
            // uniform
            float cmax = local < 1e30f ? local : 1e30f;
            for (int s = 0; s < S; ++s) {
                const int sv = srvb[s];
                if (sv < 0) continue;
                float c = server_cost(sp_row, hop_row, udsb, uds_sn, sv, ulj, dlj);
                if (isfinite(c)) { c = c < 1e30f ? c : 1e30f;
                                   cmax = c > cmax ? c : cmax; }
            }
            float psum = 0.f;
            for (int s = 0; s < S; ++s) {
                const int sv = srvb[s];
                if (sv < 0) continue;
                psum += softmax_w(
                    server_cost(sp_row, hop_row, udsb, uds_sn, sv, ulj, dlj), cmax);
            }
            psum += softmax_w(local, cmax);
            const float r = u01(mix64(key ^ (unsigned long long)bj)) * psum;
            float acc = 0.f;
            best_s = -1;                     // fallthrough: local
            for (int s = 0; s < S; ++s) {
                const int sv = srvb[s];
                if (sv < 0) continue;
                acc += softmax_w(
                    server_cost(sp_row, hop_row, udsb, uds_sn, sv, ulj, dlj), cmax);
                if (r < acc) { best_s = s; break; }
            }
        } else {
            // torch argmin tie-break = first index; the cost vector is
            // [server_0 .. server_{S-1}, local]: first-min among servers via
            // strict <, and local wins only if strictly below every server.
            float best = INFINITY;
            best_s = -1;
            for (int s = 0; s < S; ++s) {
                const int sv = srvb[s];
                if (sv < 0) continue;
                const float c =
                    server_cost(sp_row, hop_row, udsb, uds_sn, sv, ulj, dlj);
                if (c < best) { best = c; best_s = s; }
            }
            if (local < best) best_s = -1;      // -1 = local
        }
        if (eps > 0.f) {
            const unsigned long long h1 =
                mix64(key ^ (0x517CC1B727220A95ull + bj));
            if (u01(h1) < eps) {
                // uniform over the nS valid servers + local
                const int rc = (int)(u01(mix64(h1)) * (float)(nS + 1));
                best_s = rc >= nS ? -1 : rc;
            }
        }
        dst_out[bj] = best_s < 0 ? s0 : srvb[best_s];
        islocal_out[bj] = best_s < 0;
    }
}

// ---------------------------------------------------------------------------
// walk_eval: greedy next-hop walk + load accumulation + contention fixed
// point + per-job empirical delays (offloading_v3.py:441-550).
// grid.x = B; one workgroup per graph; LDS regions: qm::walk_plan.
//
// unit_mtx determinism: several jobs can traverse the same link (or share a
// destination) with DIFFERENT per-job fallback units when congested; the
// oracle's Python loop makes the LAST job's value win.  Stage 3 reproduces
// that deterministically under parallel execution by packing
// (job_index+1) << 32 | float_bits(unit) into a u64 scratch cell with
// atomicMax (units are finite non-negative, so the job index dominates),
// then unpacking after a barrier — block b owns slice b, so no cross-block
// coherence is needed.  Only a graph's links and its diagonal can be
// written, so the scratch has one cell per link and one per node (link l at
// l, node n at E + n), not one per matrix cell: stage 3 packs once per hop,
// stage 3b writes the (u,v), (v,u) and (n,n) cells of the non-zero packs
// into unit_mtx/written, which the workgroup zero-fills at its top with
// plain stores that nothing waits for.
//
// overflow[b] is counted in LDS and stored once; a non-zero count is also
// added to the optional device-side total, so the caller needs no reduction.
// ---------------------------------------------------------------------------
__global__ void walk_eval_kernel(
    const float* __restrict__ sp,        // (B,N,N)
    const long* __restrict__ src,        // (B,J)
    const long* __restrict__ dstv,       // (B,J)
    const bool* __restrict__ mask,       // (B,J)
    const float* __restrict__ rate,      // (B,J)
    const float* __restrict__ ul,        // (B,J)
    const float* __restrict__ dl,        // (B,J)
    const int* __restrict__ adj_indptr,  // (B,N+1)
    const int* __restrict__ adj_idx,     // (B,2E)
    const int* __restrict__ adj_link,    // (B,2E)
    const qm::Tables t,                  // bw = per-node bw (B,N)
    const int* __restrict__ edges,       // (B,E,2)
    int* __restrict__ route_links,       // (B,J,H) out, -1 pad
    int* __restrict__ nhop,              // (B,J) out
    float* __restrict__ delay_emp,       // (B,J) out (nan for padded jobs)
    float* __restrict__ unit_mtx,        // (B,N,N) out
    bool* __restrict__ written,          // (B,N,N) out
    unsigned long long* __restrict__ upack,  // (B,E+N) scratch
    int* __restrict__ overflow,          // (B) out
    unsigned long long* __restrict__ overflow_total,  // () += | nullptr
    const int* __restrict__ n_arr,       // (B) real node counts (padding)
    const qm::WalkPlan p, int stage_budget, int N, int E, int J, int H,
    int fp_iters) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* lds = reinterpret_cast<float*>(smem_raw);
    float* lam = lds + p.lam;
    float* mu = lds + p.mu;
    float* busy = lds + p.busy;
    float* sload = lds + p.sload;
    __shared__ int ovf_s;                // truncated walks of this graph

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    const float* spb = sp + (size_t)b * N * N;
    const int* aip = adj_indptr + (size_t)b * (N + 1);
    const int* aix = adj_idx + (size_t)b * 2 * E;
    const int* alk = adj_link + (size_t)b * 2 * E;
    const qm::Graph g = qm::graph_view(t, b);
    unsigned long long* upk = upack + (size_t)b * (E + N);
    float* um = unit_mtx + (size_t)b * N * N;
    bool* wm = written + (size_t)b * N * N;
    // per-graph effective sizes: padded link slots / inert pad nodes are
    // isolated and never touched by routes, so every E/N-length loop below
    // runs on the real extent only (ragged-E batches, pad_to mixed-N)
    const int Eb = g.Eb;
    const int nb_ = n_arr[b];
    // ends on a barrier when it stages; the one below covers the rest
    const qm::Csr csr = qm::stage_csr(
        g.cip, g.rates, g.ccols, Eb, smem_raw + qm::stage_align(p.lds_bytes),
        stage_budget, tid, nt);

    for (int e = tid; e < Eb; e += nt) lam[e] = 0.0f;
    for (int n = tid; n < nb_; n += nt) sload[n] = 0.0f;
    for (int i = tid; i < E + N; i += nt) upk[i] = 0ull;
    if (tid == 0) ovf_s = 0;
    // outputs arrive torch::empty: zero the whole slice (pad rows and
    // columns stay 0/false), stage 3b overwrites the written cells after
    // the barriers below.  16-byte stores when every slice is aligned.
    if (((N * N) & 15) == 0) {
        float4* um4 = reinterpret_cast<float4*>(um);
        uint4* wm4 = reinterpret_cast<uint4*>(wm);
        for (int i = tid; i < N * N / 4; i += nt)
            um4[i] = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int i = tid; i < N * N / 16; i += nt)
            wm4[i] = make_uint4(0u, 0u, 0u, 0u);
    } else {
        for (int i = tid; i < N * N; i += nt) { um[i] = 0.f; wm[i] = false; }
    }
    __syncthreads();

    // ---- stage 1: walk + load accumulation -------------------------------
    for (int j = tid; j < J; j += nt) {
        const size_t bj = (size_t)b * J + j;
        if (!mask[bj]) {
            nhop[bj] = 0;
            for (int h = 0; h < H; ++h)
                route_links[bj * H + h] = -1;
            continue;
        }
        const int d = (int)dstv[bj];
        int node = (int)src[bj];
        const float add = (ul[bj] + dl[bj]) * rate[bj];
        int h = 0;
        while (node != d && h < H) {
            const int lo = aip[node], hi = aip[node + 1];
            float bestv = INFINITY;
            int bestn = -1, bestl = -1;
            for (int a = lo; a < hi; ++a) {
                const int nb2 = aix[a];
                const float v = spb[(size_t)nb2 * N + d];
                if (v < bestv) { bestv = v; bestn = nb2; bestl = alk[a]; }
            }
            // precondition: a walked node has a neighbour with finite sp
            // to d (connected graphs).  If none has, stop instead of
            // indexing with -1; the walk is counted as truncated below.
            if (bestl < 0) break;
            route_links[((size_t)b * J + j) * H + h] = bestl;
            atomicAdd(&lam[bestl], add);
            node = bestn;
            ++h;
        }
        if (node != d) atomicAdd(&ovf_s, 1);
        nhop[bj] = h;
        for (int h2 = h; h2 < H; ++h2)       // outputs arrive torch::empty
            route_links[bj * H + h2] = -1;
        atomicAdd(&sload[d], ul[bj] * rate[bj]);
    }
    __syncthreads();

    // ---- stage 2: contention fixed point (offloading_v3.py:500-506) ------
    // only the last iterate is needed: row stride 0 keeps no history
    qm::fixed_point_fwd(csr, lam, mu, busy, Eb, 0, fp_iters, tid, nt);

    // ---- stage 3: per-job empirical delays (offloading_v3.py:522-549) ----
    const int* edg = edges + (size_t)b * E * 2;
    for (int j = tid; j < J; j += nt) {
        const size_t bj = (size_t)b * J + j;
        if (!mask[bj]) { delay_emp[bj] = NAN; continue; }
        const float ulj = ul[bj], dlj = dl[bj];
        const float tot = ulj + dlj;
        const float nh = (float)nhop[bj];
        const unsigned long long jtag = ((unsigned long long)(j + 1)) << 32;
        float acc = 0.0f;
        for (int h = 0; h < nhop[bj]; ++h) {
            const int l = route_links[((size_t)b * J + j) * H + h];
            if (l < 0) break;
            const float unit = qm::emp_unit(lam[l], mu[l], g.T, tot);
            atomicMax(&upk[l], jtag | (unsigned long long)
                                   __float_as_uint(unit));
            acc += fmax1(ulj * unit, nh) + fmax1(dlj * unit, nh);
        }
        const int d = (int)dstv[bj];
        const float sunit = qm::emp_unit(sload[d], g.bw[d], g.T, ulj);
        atomicMax(&upk[E + d],
                  jtag | (unsigned long long)__float_as_uint(sunit));
        acc += fmax1(ulj * sunit, 1.0f);
        delay_emp[bj] = acc;
    }
    __syncthreads();
    // ---- stage 3b: unpack last-job-wins units into unit_mtx/written ------
    for (int e = tid; e < Eb; e += nt) {
        const unsigned long long pk = upk[e];
        if (!pk) continue;
        const float unit = __uint_as_float((unsigned int)(pk & 0xffffffffull));
        const int u = edg[e * 2], v = edg[e * 2 + 1];
        um[(size_t)u * N + v] = unit;
        um[(size_t)v * N + u] = unit;
        wm[(size_t)u * N + v] = true;
        wm[(size_t)v * N + u] = true;
    }
    for (int n = tid; n < nb_; n += nt) {
        const unsigned long long pk = upk[E + n];
        if (!pk) continue;
        um[(size_t)n * N + n] =
            __uint_as_float((unsigned int)(pk & 0xffffffffull));
        wm[(size_t)n * N + n] = true;
    }
    if (tid == 0) {
        const int cnt = ovf_s;
        overflow[b] = cnt;
        if (cnt && overflow_total)
            atomicAdd(overflow_total, (unsigned long long)cnt);
    }
}

}  // namespace

std::vector<torch::Tensor> decide_hip(
    torch::Tensor sp, torch::Tensor hop, torch::Tensor uds,
    torch::Tensor servers, torch::Tensor src, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl,
    c10::optional<torch::Tensor> explore, c10::optional<torch::Tensor> rng,
    long prob) {
    const int B = sp.size(0), N = sp.size(1);
    const int J = src.size(1), S = servers.size(1);
    // uds is read through its strides: the diagonal view of the delay
    // matrix (strides N², N + 1) needs no copy
    TORCH_CHECK(uds.dim() == 2 && uds.size(0) == B && uds.size(1) == N
                && uds.scalar_type() == torch::kFloat32,
                "decide: uds is (B,N) fp32");
    auto dst = torch::empty({B, J}, src.options());
    auto islocal = torch::empty({B, J}, mask.options());
    const float* ep = explore.has_value()
        ? explore->data_ptr<float>() : nullptr;
    const long* rp = rng.has_value() ? rng->data_ptr<long>() : nullptr;
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(decide_kernel, dim3(B), dim3(256), 0, stream.stream(),
                       sp.data_ptr<float>(), hop.data_ptr<float>(),
                       uds.data_ptr<float>(), (long)uds.stride(0),
                       (long)uds.stride(1),
                       servers.data_ptr<int>(), src.data_ptr<long>(),
                       mask.data_ptr<bool>(), ul.data_ptr<float>(),
                       dl.data_ptr<float>(), ep, rp,
                       dst.data_ptr<long>(),
                       islocal.data_ptr<bool>(), (int)prob, N, J, S);
    return {dst, islocal};
}

std::vector<torch::Tensor> walk_eval_hip(
    torch::Tensor sp, torch::Tensor src, torch::Tensor dst,
    torch::Tensor mask, torch::Tensor rate, torch::Tensor ul,
    torch::Tensor dl, torch::Tensor adj_indptr, torch::Tensor adj_idx,
    torch::Tensor adj_link, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor edges, torch::Tensor T_arr,
    torch::Tensor E_arr, torch::Tensor n_arr, long H,
    long fp_iters, c10::optional<torch::Tensor> overflow_total) {
    const int B = sp.size(0), N = sp.size(1);
    const int J = src.size(1), E = rates.size(1);
    unsigned long long* ovf_total = nullptr;
    if (overflow_total.has_value()) {
        TORCH_CHECK(overflow_total->scalar_type() == torch::kInt64
                    && overflow_total->numel() == 1
                    && overflow_total->is_cuda(),
                    "walk_eval: overflow_total is one int64 on the device");
        ovf_total = reinterpret_cast<unsigned long long*>(
            overflow_total->data_ptr<long>());
    }
    auto opts_i = adj_indptr.options();
    auto opts_f = sp.options();
    // all outputs fully initialized in-kernel (no fill launches)
    auto route_links = torch::empty({B, J, H}, opts_i.dtype(torch::kInt32));
    auto nhop = torch::empty({B, J}, opts_i.dtype(torch::kInt32));
    auto delay_emp = torch::empty({B, J}, opts_f);
    auto unit_mtx = torch::empty({B, N, N}, opts_f);
    auto written = torch::empty({B, N, N}, opts_f.dtype(torch::kBool));
    // u64 scratch for deterministic last-job-wins unit writes, one cell per
    // link and per node (the kernel zeroes its own slice — empty, not zeros)
    auto upack = torch::empty({B, E + N}, opts_f.dtype(torch::kInt64));
    auto overflow = torch::empty({B}, opts_i.dtype(torch::kInt32));
    const qm::WalkPlan p = qm::walk_plan(N, E);
    TORCH_CHECK(p.fits, "graph too large for LDS walk_eval");
    auto stream = at::cuda::getCurrentCUDAStream();
    const int budget = qm::stage_budget(p);
    hipLaunchKernelGGL(walk_eval_kernel, dim3(B), dim3(p.threads),
                       qm::launch_lds_bytes(p, budget), stream.stream(),
                       sp.data_ptr<float>(), src.data_ptr<long>(),
                       dst.data_ptr<long>(), mask.data_ptr<bool>(),
                       rate.data_ptr<float>(), ul.data_ptr<float>(),
                       dl.data_ptr<float>(),
                       adj_indptr.data_ptr<int>(), adj_idx.data_ptr<int>(),
                       adj_link.data_ptr<int>(),
                       qm::tables(conf_indptr, conf_base, conf_cols, rates,
                                  bw, T_arr, E_arr),
                       edges.data_ptr<int>(),
                       route_links.data_ptr<int>(), nhop.data_ptr<int>(),
                       delay_emp.data_ptr<float>(),
                       unit_mtx.data_ptr<float>(), written.data_ptr<bool>(),
                       reinterpret_cast<unsigned long long*>(
                           upack.data_ptr<long>()),
                       overflow.data_ptr<int>(), ovf_total,
                       n_arr.data_ptr<int>(), p,
                       budget, N, E, J, (int)H, (int)fp_iters);
    return {route_links, nhop, delay_emp, unit_mtx, written, overflow};
}
