// Batched all-pairs shortest paths (min-plus Floyd–Warshall) for gfx950.
//
// Design (MI355X-first): one workgroup per graph.  fp32 up to N = 128 keeps
// the matrix in registers with only the pivot row and column in LDS
// (fw_reg_kernel); above that, and for fp64, the whole N×N distance matrix
// is resident in LDS (160 KiB/CU ⇒ N ≤ 200 at fp32, fw_lds_kernel).  The k-loop runs
// entirely on-chip with one barrier per k; a batch of B graphs fills the
// 256 CUs with B workgroups.  In-place updates are safe: row k and column k
// cannot improve through k itself (d[k][k] = 0), so no thread writes the
// cells another thread reads within an iteration.
//
// Replaces the reference's per-graph networkx Dijkstra
// (util.py:101-110, called twice per method per instance) — the dominant
// CPU hot spot of the reference pipeline.
//
// For N > 200 the host falls back to the tiled global-memory path
// (fw_tiled below): standard 3-phase blocked FW, batched over graphs.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include <type_traits>

#include "gfx950.h"

namespace {

// n_arr: optional per-graph EFFECTIVE node count (inert-padded batches,
// CaseGraph.pad_to): the kernel relaxes only the leading n×n submatrix
// (staged at compact stride n in LDS) — pad nodes are isolated, so their
// +inf rows in global memory are already final.  O(n³) instead of O(N³)
// per graph: a 20-node case padded to 120 does 216× less work.
//
// MASKED: `src` is the actor head's delay matrix as it stands (garbage
// outside link cells) and `adj` the adjacency mask; the load applies
// i==j ? 0 : (adj ? src : +inf) itself and the result goes to `d`, a fresh
// uninitialised output, pad cells included (+inf, 0 on the diagonal) —
// what the unmasked kernel computes in place from a prepared clone, bit for
// bit, without the five (B,N,N) passes that prepare it.  Unmasked: src == d.
template <typename T, bool MASKED>
__global__ void fw_lds_kernel(const T* src, const bool* __restrict__ adj,
                              T* d, int N, const int* __restrict__ n_arr) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    T* s = reinterpret_cast<T*>(smem_raw);
    T* D = d + (size_t)blockIdx.x * N * N;
    const T* S = src + (size_t)blockIdx.x * N * N;
    const bool* A = MASKED ? adj + (size_t)blockIdx.x * N * N : nullptr;
    const int n = n_arr ? n_arr[blockIdx.x] : N;
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    // LDS row stride padded to a float4 multiple with +inf columns: the
    // vectorized relax path then covers EVERY n (min-plus is inert on inf
    // pads), instead of degrading to the scalar path when n % 4 != 0
    const int ns = (sizeof(T) == 4) ? ((n + 3) & ~3) : n;
    for (int c = tid; c < n * ns; c += nt) {
        const int r = c / ns, j = c % ns;
        T v = (T)INFINITY;
        if (j < n) {
            const size_t g = (size_t)r * N + j;
            if (!MASKED) v = S[g];
            else if (r == j) v = (T)0;
            else if (A[g]) v = S[g];
        }
        s[c] = v;
    }
    __syncthreads();
    // thread layout: each of 32 lanes per half-wave owns a 4-column group,
    // rows strided across the remaining threads — d[k][j..j+3] loads once
    // per k, d[i][k] broadcasts.
    const int i0 = tid >> 5;
    const int istep = nt >> 5;
    if (sizeof(T) == 4) {
        for (int k = 0; k < n; ++k) {
            for (int j = (tid & 31) * 4; j < n; j += 128) {
                float4 dkj = *reinterpret_cast<const float4*>(
                    reinterpret_cast<const float*>(s) + k * ns + j);
                for (int i = i0; i < n; i += istep) {
                    const float dik =
                        reinterpret_cast<const float*>(s)[i * ns + k];
                    float* row = reinterpret_cast<float*>(s) + i * ns + j;
                    float4 cur = *reinterpret_cast<float4*>(row);
                    cur.x = fminf(cur.x, dik + dkj.x);
                    cur.y = fminf(cur.y, dik + dkj.y);
                    cur.z = fminf(cur.z, dik + dkj.z);
                    cur.w = fminf(cur.w, dik + dkj.w);
                    *reinterpret_cast<float4*>(row) = cur;
                }
            }
            __syncthreads();
        }
    } else {
        for (int k = 0; k < n; ++k) {
            for (int j = tid & 31; j < n; j += 32) {
                const T dkj = s[k * ns + j];
                for (int i = i0; i < n; i += istep) {
                    const T alt = s[i * ns + k] + dkj;
                    if (alt < s[i * ns + j]) s[i * ns + j] = alt;
                }
            }
            __syncthreads();
        }
    }
    if (MASKED) {
        for (int c = tid; c < N * N; c += nt) {
            const int r = c / N, j = c % N;
            D[c] = (r < n && j < n) ? s[r * ns + j]
                                    : (r == j ? (T)0 : (T)INFINITY);
        }
    } else {
        for (int c = tid; c < n * n; c += nt)
            D[(size_t)(c / n) * N + (c % n)] = s[(c / n) * ns + (c % n)];
    }
}

// ---- register-resident path, fp32, N ≤ FWR_MAX_N --------------------------
// Only row k and column k of the matrix are read by threads other than a
// cell's owner, so the cells live in registers: thread (tr, tc) of a
// ceil(n/RT) × ceil(n/4) grid owns the RT×4 block at (tr·RT, tc·4), and LDS
// holds just the pivot row and pivot column, double-buffered.  Iteration k
// reads buffer k&1 (one float4 of row k, RT broadcast values of column k)
// and relaxes the block, and the owners of row k+1 and column k+1 write
// them to the other buffer: one barrier per pivot.  Row k+1 and column k+1
// have then seen pivots 0…k, which is what fw_lds_kernel reads in place,
// and the arithmetic per cell is the same fminf(cur, dik + dkj) in the same
// order (fw_min below), so the result is bit-identical.  Load/store
// conventions, MASKED and n_arr are those of fw_lds_kernel.  RT is chosen
// by N so that the thread grid fits 512 lanes and nearly fills them
// (N=100: 5×4 blocks, 500 lanes).
constexpr int FWR_THREADS = 512;
constexpr int FWR_MAX_N = 128;
constexpr int FWR_COL_SLOTS = 256;

// rows per thread for an N×N matrix; 0: not covered
constexpr int fw_reg_rows(int N) {
    return N <= 64 ? 2 : N <= 88 ? 4 : N <= 100 ? 5 : N <= 119 ? 7
         : N <= FWR_MAX_N ? 8 : 0;
}
constexpr bool fw_reg_fits(int N) {
    const int rt = fw_reg_rows(N);
    return ((N + 3) / 4) * ((N + rt - 1) / rt) <= FWR_THREADS;
}
// the thread grid grows with n, so the largest N of each bucket decides
static_assert(fw_reg_fits(64) && fw_reg_fits(88) && fw_reg_fits(100)
              && fw_reg_fits(119) && fw_reg_fits(128),
              "fw_reg_kernel: thread grid exceeds the workgroup");

// fminf of two canonical values: the v_min_f32 that fminf compiles to,
// without the v_max_f32 x, x the compiler puts in front of it for every
// operand it cannot prove canonical (here: every cell, each pivot — a third
// of the loop's vector instructions).  The sums pair up in v_pk_add_f32.
typedef float float2_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ float fw_min(float a, float b) {
    float r;
    asm("v_min_f32 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
    return r;
}

template <int RT, bool MASKED>
__global__ __launch_bounds__(FWR_THREADS)
void fw_reg_kernel(const float* src, const bool* __restrict__ adj, float* d,
                   int N, const int* __restrict__ n_arr) {
    // column-buffer slots per row group: a float4 multiple, so the RT
    // values of a thread's rows read as one or two ds_read_b128
    constexpr int CS = RT <= 4 ? 4 : 8;
    static_assert((FWR_MAX_N + RT - 1) / RT * CS <= FWR_COL_SLOTS, "colb");
    __shared__ __attribute__((aligned(16))) float rowb[2][FWR_MAX_N];
    __shared__ __attribute__((aligned(16))) float colb[2][FWR_COL_SLOTS];
    float* D = d + (size_t)blockIdx.x * N * N;
    const float* S = src + (size_t)blockIdx.x * N * N;
    const bool* A = MASKED ? adj + (size_t)blockIdx.x * N * N : nullptr;
    const int n = n_arr ? min(max(n_arr[blockIdx.x], 0), N) : N;
    const int tid = threadIdx.x;
    const int TC = max((n + 3) >> 2, 1);
    const int tr = tid / TC, tc = tid - tr * TC;
    const int r0 = tr * RT, c0 = tc * 4;
    const bool active = r0 < n;

    // cells are canonicalised once here (a signalling NaN is quieted, as
    // fminf does on every call); every later value is the result of an add
    // or a min and canonical already
    float c[RT][4];
#pragma unroll
    for (int q = 0; q < RT; ++q)
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            const int r = r0 + q, j = c0 + p;
            float v = INFINITY;
            if (active && r < n && j < n) {
                const size_t g = (size_t)r * N + j;
                if (!MASKED) v = S[g];
                else if (r == j) v = 0.f;
                else if (A[g]) v = S[g];
            }
            c[q][p] = __builtin_canonicalizef(v);
        }

    // Pivot k = kb + P, kb a multiple of L = lcm(RT, 4): which of a thread's
    // rows is row k+1 (QN) and which of its columns is column k+1 (PN) are
    // then compile-time, so publishing them indexes no register dynamically.
    // The owners of row k+1 relax and publish it before the block (those
    // four cells are relaxed again with the block: same operands, same
    // bits), and the half of the block that holds column k+1 goes first, so
    // both LDS writes are under way while the rest is relaxed.
    constexpr int L = RT % 4 == 0 ? RT : RT % 2 == 0 ? 2 * RT : 4 * RT;
    auto relax_half = [&](auto hc, const float4& rk, const float* ck) {
        constexpr int H = decltype(hc)::value;
        const float2_t r2 = H == 0 ? float2_t{rk.x, rk.y}
                                   : float2_t{rk.z, rk.w};
#pragma unroll
        for (int q = 0; q < RT; ++q) {
            const float2_t dik = {ck[q], ck[q]};
            const float2_t alt = dik + r2;
            c[q][2 * H] = fw_min(c[q][2 * H], alt.x);
            c[q][2 * H + 1] = fw_min(c[q][2 * H + 1], alt.y);
        }
    };
    auto pivot = [&](int kb, int rgb, int cgb, auto pc) {
        constexpr int P = decltype(pc)::value;
        constexpr int buf = P & 1;                  // k & 1: kb is even
        constexpr int QN = (P + 1) % RT, PN = (P + 1) % 4;
        const bool more = kb + P + 1 < n;           // block-uniform
        if (active) {
            const float4 rk =
                *reinterpret_cast<const float4*>(&rowb[buf][c0]);
            float ck[CS];
#pragma unroll
            for (int q = 0; q < CS; q += 4) {
                const float4 t = *reinterpret_cast<const float4*>(
                    &colb[buf][tr * CS + q]);
                ck[q] = t.x; ck[q + 1] = t.y;
                ck[q + 2] = t.z; ck[q + 3] = t.w;
            }
            if (more && tr == rgb + (P + 1) / RT) {
                const float4 v = {fw_min(c[QN][0], ck[QN] + rk.x),
                                  fw_min(c[QN][1], ck[QN] + rk.y),
                                  fw_min(c[QN][2], ck[QN] + rk.z),
                                  fw_min(c[QN][3], ck[QN] + rk.w)};
                *reinterpret_cast<float4*>(&rowb[buf ^ 1][c0]) = v;
            }
            relax_half(std::integral_constant<int, PN / 2>{}, rk, ck);
            if (more && tc == cgb + (P + 1) / 4) {
#pragma unroll
                for (int q = 0; q < RT; ++q)
                    colb[buf ^ 1][tr * CS + q] = c[q][PN];
            }
            relax_half(std::integral_constant<int, 1 - PN / 2>{}, rk, ck);
        }
        __syncthreads();
    };
    // pivots kb + P … kb + L − 1, stopping at n
    auto pivots = [&](auto self, int kb, int rgb, int cgb, auto pc) -> void {
        constexpr int P = decltype(pc)::value;
        pivot(kb, rgb, cgb, pc);
        if constexpr (P + 1 < L) {
            if (kb + P + 1 < n)
                self(self, kb, rgb, cgb, std::integral_constant<int, P + 1>{});
        }
    };

    if (active && n > 0) {                          // row 0 and column 0
        if (tr == 0)
            *reinterpret_cast<float4*>(&rowb[0][c0]) =
                float4{c[0][0], c[0][1], c[0][2], c[0][3]};
        if (tc == 0) {
#pragma unroll
            for (int q = 0; q < RT; ++q) colb[0][tr * CS + q] = c[q][0];
        }
    }
    __syncthreads();
    for (int kb = 0, rgb = 0, cgb = 0; kb < n;      // n is block-uniform
         kb += L, rgb += L / RT, cgb += L / 4)
        pivots(pivots, kb, rgb, cgb, std::integral_constant<int, 0>{});

    if (active) {
#pragma unroll
        for (int q = 0; q < RT; ++q)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                const int r = r0 + q, j = c0 + p;
                if (r < n && j < n) D[(size_t)r * N + j] = c[q][p];
            }
    }
    if (MASKED && n < N) {
        for (int e = tid; e < N * N; e += FWR_THREADS) {
            const int r = e / N, j = e % N;
            if (r >= n || j >= n) D[e] = r == j ? 0.f : INFINITY;
        }
    }
}

// fw_force_inplace(true): every later launch takes fw_lds_kernel (before/
// after timings, register-vs-in-place tests); a captured graph keeps what
// its launches were given at capture.
bool fw_inplace_forced = false;

// Launch fw_reg_kernel if it covers N and is not switched off.
template <bool MASKED>
bool fw_reg_launch(const float* src, const bool* adj, float* d, int B, int N,
                   const int* n_arr, hipStream_t stream) {
    if (fw_inplace_forced || B == 0 || N == 0) return false;
#define FW_REG_CASE(RT)                                                     \
    case RT:                                                                \
        hipLaunchKernelGGL((fw_reg_kernel<RT, MASKED>), dim3(B),            \
                           dim3(FWR_THREADS), 0, stream, src, adj, d, N,    \
                           n_arr);                                          \
        return true;
    switch (fw_reg_rows(N)) {
        FW_REG_CASE(2) FW_REG_CASE(4) FW_REG_CASE(5) FW_REG_CASE(7)
        FW_REG_CASE(8)
        default: return false;
    }
#undef FW_REG_CASE
}

// ---- tiled (global-memory) path for large N -------------------------------
// Classic 3-phase blocked FW with TILE=32. Grid z = graph.
constexpr int TILE = 32;

template <typename T>
__device__ inline void fw_tile_body(T* __restrict__ c, const T* __restrict__ a,
                                    const T* __restrict__ b) {
    // c = min(c, a (+) b) over the k dimension of the tile, in LDS
    const int tx = threadIdx.x, ty = threadIdx.y;
    T v = c[ty * TILE + tx];
#pragma unroll
    for (int k = 0; k < TILE; ++k) {
        const T alt = a[ty * TILE + k] + b[k * TILE + tx];
        v = alt < v ? alt : v;
    }
    c[ty * TILE + tx] = v;
}

template <typename T>
__global__ void fw_phase1(T* __restrict__ d, int N, int nb, int kb) {
    __shared__ T tile[TILE * TILE];
    T* D = d + (size_t)blockIdx.z * N * N;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int r = kb * TILE + ty, c = kb * TILE + tx;
    tile[ty * TILE + tx] = (r < N && c < N) ? D[r * N + c]
                                            : (T)INFINITY;
    __syncthreads();
    for (int k = 0; k < TILE; ++k) {
        const T alt = tile[ty * TILE + k] + tile[k * TILE + tx];
        if (alt < tile[ty * TILE + tx]) tile[ty * TILE + tx] = alt;
        __syncthreads();
    }
    if (r < N && c < N) D[r * N + c] = tile[ty * TILE + tx];
}

template <typename T>
__global__ void fw_phase2(T* __restrict__ d, int N, int nb, int kb) {
    // blockIdx.x: which tile along the strip; blockIdx.y: 0=row strip, 1=col
    __shared__ T piv[TILE * TILE];
    __shared__ T cur[TILE * TILE];
    T* D = d + (size_t)blockIdx.z * N * N;
    int jb = blockIdx.x;
    if (jb >= kb) jb += 1;                  // skip the pivot tile
    if (jb >= nb) return;
    const int tx = threadIdx.x, ty = threadIdx.y;
    const int pr = kb * TILE + ty, pc = kb * TILE + tx;
    piv[ty * TILE + tx] = (pr < N && pc < N) ? D[pr * N + pc] : (T)INFINITY;
    int r, c;
    if (blockIdx.y == 0) { r = kb * TILE + ty; c = jb * TILE + tx; }
    else                 { r = jb * TILE + ty; c = kb * TILE + tx; }
    cur[ty * TILE + tx] = (r < N && c < N) ? D[r * N + c] : (T)INFINITY;
    __syncthreads();
    if (blockIdx.y == 0) {
        for (int k = 0; k < TILE; ++k) {
            const T alt = piv[ty * TILE + k] + cur[k * TILE + tx];
            if (alt < cur[ty * TILE + tx]) cur[ty * TILE + tx] = alt;
            __syncthreads();
        }
    } else {
        for (int k = 0; k < TILE; ++k) {
            const T alt = cur[ty * TILE + k] + piv[k * TILE + tx];
            if (alt < cur[ty * TILE + tx]) cur[ty * TILE + tx] = alt;
            __syncthreads();
        }
    }
    if (r < N && c < N) D[r * N + c] = cur[ty * TILE + tx];
}

template <typename T>
__global__ void fw_phase3(T* __restrict__ d, int N, int nb, int kb) {
    __shared__ T rowt[TILE * TILE];   // tile (ib, kb)
    __shared__ T colt[TILE * TILE];   // tile (kb, jb)
    T* D = d + (size_t)blockIdx.z * N * N;
    int ib = blockIdx.y, jb = blockIdx.x;
    if (ib >= kb) ib += 1;
    if (jb >= kb) jb += 1;
    if (ib >= nb || jb >= nb) return;
    const int tx = threadIdx.x, ty = threadIdx.y;
    int r = ib * TILE + ty, c = kb * TILE + tx;
    rowt[ty * TILE + tx] = (r < N && c < N) ? D[r * N + c] : (T)INFINITY;
    r = kb * TILE + ty; c = jb * TILE + tx;
    colt[ty * TILE + tx] = (r < N && c < N) ? D[r * N + c] : (T)INFINITY;
    __syncthreads();
    r = ib * TILE + ty; c = jb * TILE + tx;
    if (r < N && c < N) {
        T v = D[r * N + c];
#pragma unroll
        for (int k = 0; k < TILE; ++k) {
            const T alt = rowt[ty * TILE + k] + colt[k * TILE + tx];
            v = alt < v ? alt : v;
        }
        D[r * N + c] = v;
    }
}

// ---- TILE=64 fp32 specialization for large N (ER-1000 class) -------------
// Halves the memory-side traffic of the TILE=32 path (4·N³/TILE bytes per
// full FW) and gives each 256-thread block 8× the work per tile triple.
constexpr int T64 = 64;

__global__ void fw64_phase1(float* __restrict__ d, int N, int nb, int kb) {
    __shared__ __attribute__((aligned(16))) float tile[T64 * T64];
    float* D = d + (size_t)blockIdx.z * N * N;
    const int tid = threadIdx.x;                     // 256 threads
    for (int c = tid; c < T64 * T64; c += 256) {
        const int r = kb * T64 + c / T64, cc = kb * T64 + c % T64;
        tile[c] = (r < N && cc < N) ? D[(size_t)r * N + cc] : INFINITY;
    }
    __syncthreads();
    // each thread owns 16 cells (row group of 4 × col group of 4)
    const int ty = tid >> 4, tx = tid & 15;          // 16×16 thread grid
    for (int k = 0; k < T64; ++k) {
        float kj[4], ik[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            kj[q] = tile[k * T64 + tx * 4 + q];
            ik[q] = tile[(ty * 4 + q) * T64 + k];
        }
        __syncthreads();
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                float* cell = tile + (ty * 4 + q) * T64 + tx * 4 + p;
                const float alt = ik[q] + kj[p];
                if (alt < *cell) *cell = alt;
            }
        __syncthreads();
    }
    for (int c = tid; c < T64 * T64; c += 256) {
        const int r = kb * T64 + c / T64, cc = kb * T64 + c % T64;
        if (r < N && cc < N) D[(size_t)r * N + cc] = tile[c];
    }
}

__global__ void fw64_phase2(float* __restrict__ d, int N, int nb, int kb) {
    __shared__ __attribute__((aligned(16))) float piv[T64 * T64];
    __shared__ __attribute__((aligned(16))) float cur[T64 * T64];
    float* D = d + (size_t)blockIdx.z * N * N;
    int jb = blockIdx.x;
    if (jb >= kb) jb += 1;
    if (jb >= nb) return;
    const int tid = threadIdx.x;
    const bool row_strip = blockIdx.y == 0;
    for (int c = tid; c < T64 * T64; c += 256) {
        const int pr = kb * T64 + c / T64, pc = kb * T64 + c % T64;
        piv[c] = (pr < N && pc < N) ? D[(size_t)pr * N + pc] : INFINITY;
        int r, cc;
        if (row_strip) { r = kb * T64 + c / T64; cc = jb * T64 + c % T64; }
        else           { r = jb * T64 + c / T64; cc = kb * T64 + c % T64; }
        cur[c] = (r < N && cc < N) ? D[(size_t)r * N + cc] : INFINITY;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    if (row_strip) {
        for (int k = 0; k < T64; ++k) {
            float ik[4], kj[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ik[q] = piv[(ty * 4 + q) * T64 + k];
                kj[q] = cur[k * T64 + tx * 4 + q];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    float* cell = cur + (ty * 4 + q) * T64 + tx * 4 + p;
                    const float alt = ik[q] + kj[p];
                    if (alt < *cell) *cell = alt;
                }
            __syncthreads();
        }
    } else {
        for (int k = 0; k < T64; ++k) {
            float ik[4], kj[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                ik[q] = cur[(ty * 4 + q) * T64 + k];
                kj[q] = piv[k * T64 + tx * 4 + q];
            }
            __syncthreads();
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int p = 0; p < 4; ++p) {
                    float* cell = cur + (ty * 4 + q) * T64 + tx * 4 + p;
                    const float alt = ik[q] + kj[p];
                    if (alt < *cell) *cell = alt;
                }
            __syncthreads();
        }
    }
    for (int c = tid; c < T64 * T64; c += 256) {
        int r, cc;
        if (row_strip) { r = kb * T64 + c / T64; cc = jb * T64 + c % T64; }
        else           { r = jb * T64 + c / T64; cc = kb * T64 + c % T64; }
        if (r < N && cc < N) D[(size_t)r * N + cc] = cur[c];
    }
}

// phase 3: 256 threads, 4×4 registers per thread over a 64×64 output tile;
// independent min-add chains, no barriers inside the k-loop.
__global__ void fw64_phase3(float* __restrict__ d, int N, int nb, int kb) {
    __shared__ __attribute__((aligned(16))) float rowt[T64 * T64];
    __shared__ __attribute__((aligned(16))) float colt[T64 * T64];
    float* D = d + (size_t)blockIdx.z * N * N;
    int ib = blockIdx.y, jb = blockIdx.x;
    if (ib >= kb) ib += 1;
    if (jb >= kb) jb += 1;
    if (ib >= nb || jb >= nb) return;
    const int tid = threadIdx.x;
    for (int c = tid; c < T64 * T64; c += 256) {
        int r = ib * T64 + c / T64, cc = kb * T64 + c % T64;
        rowt[c] = (r < N && cc < N) ? D[(size_t)r * N + cc] : INFINITY;
        r = kb * T64 + c / T64;
        cc = jb * T64 + c % T64;
        colt[c] = (r < N && cc < N) ? D[(size_t)r * N + cc] : INFINITY;
    }
    __syncthreads();
    const int ty = tid >> 4, tx = tid & 15;
    const int r0 = ib * T64 + ty * 4;
    const int c0 = jb * T64 + tx * 4;
    float4 v[4];
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        v[q] = {INFINITY, INFINITY, INFINITY, INFINITY};
        if (r0 + q < N)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (c0 + p < N)
                    (&v[q].x)[p] = D[(size_t)(r0 + q) * N + c0 + p];
    }
#pragma unroll 2
    for (int k = 0; k < T64; ++k) {
        const float4 ckj =
            *reinterpret_cast<const float4*>(colt + k * T64 + tx * 4);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const float dik = rowt[(ty * 4 + q) * T64 + k];
            v[q].x = fminf(v[q].x, dik + ckj.x);
            v[q].y = fminf(v[q].y, dik + ckj.y);
            v[q].z = fminf(v[q].z, dik + ckj.z);
            v[q].w = fminf(v[q].w, dik + ckj.w);
        }
    }
#pragma unroll
    for (int q = 0; q < 4; ++q)
        if (r0 + q < N)
#pragma unroll
            for (int p = 0; p < 4; ++p)
                if (c0 + p < N)
                    D[(size_t)(r0 + q) * N + c0 + p] = (&v[q].x)[p];
}

}  // namespace

torch::Tensor floyd_warshall_hip(torch::Tensor w,
                                 c10::optional<torch::Tensor> n_arr) {
    TORCH_CHECK(w.is_cuda() && w.dim() == 3 && w.size(1) == w.size(2),
                "expected (B,N,N) CUDA tensor");
    auto d = w.contiguous().clone();
    const int B = d.size(0), N = d.size(1);
    auto stream = at::cuda::getCurrentCUDAStream();
    const int* np_ = n_arr.has_value() ? n_arr->data_ptr<int>() : nullptr;

    AT_DISPATCH_FLOATING_TYPES(d.scalar_type(), "fw", [&] {
        const int Ns = sizeof(scalar_t) == 4 ? ((N + 3) & ~3) : N;
        const size_t lds = (size_t)N * Ns * sizeof(scalar_t);
        bool in_registers = false;
        if constexpr (std::is_same_v<scalar_t, float>)
            in_registers = fw_reg_launch<false>(
                d.data_ptr<float>(), nullptr, d.data_ptr<float>(), B, N, np_,
                stream.stream());
        if (in_registers) {
        } else if (lds <= LDS_LIMIT) {
            hipLaunchKernelGGL((fw_lds_kernel<scalar_t, false>), dim3(B),
                               dim3(512), lds, stream.stream(),
                               d.data_ptr<scalar_t>(), nullptr,
                               d.data_ptr<scalar_t>(), N, np_);
        } else if constexpr (std::is_same_v<scalar_t, float>) {
            // fp32 large-N: TILE=64 (half the fabric traffic of TILE=32,
            // 8x the work per block; ER-1000 class)
            const int nb = (N + T64 - 1) / T64;
            for (int kb = 0; kb < nb; ++kb) {
                hipLaunchKernelGGL(fw64_phase1, dim3(1, 1, B), dim3(256), 0,
                                   stream.stream(), d.data_ptr<float>(),
                                   N, nb, kb);
                if (nb > 1) {
                    hipLaunchKernelGGL(fw64_phase2, dim3(nb - 1, 2, B),
                                       dim3(256), 0, stream.stream(),
                                       d.data_ptr<float>(), N, nb, kb);
                    hipLaunchKernelGGL(fw64_phase3,
                                       dim3(nb - 1, nb - 1, B), dim3(256),
                                       0, stream.stream(),
                                       d.data_ptr<float>(), N, nb, kb);
                }
            }
        } else {
            const int nb = (N + TILE - 1) / TILE;
            dim3 thr(TILE, TILE);
            for (int kb = 0; kb < nb; ++kb) {
                hipLaunchKernelGGL(fw_phase1<scalar_t>, dim3(1, 1, B), thr, 0,
                                   stream.stream(), d.data_ptr<scalar_t>(),
                                   N, nb, kb);
                if (nb > 1) {
                    hipLaunchKernelGGL(fw_phase2<scalar_t>,
                                       dim3(nb - 1, 2, B), thr, 0,
                                       stream.stream(),
                                       d.data_ptr<scalar_t>(), N, nb, kb);
                    hipLaunchKernelGGL(fw_phase3<scalar_t>,
                                       dim3(nb - 1, nb - 1, B), thr, 0,
                                       stream.stream(),
                                       d.data_ptr<scalar_t>(), N, nb,
                                       kb);
                }
            }
        }
    });
    return d;
}

// APSP straight from the actor head's delay matrix: non-edges → +inf,
// diagonal → 0 in the LDS load (see fw_lds_kernel<MASKED>).  Shapes too
// large for the LDS kernel prepare the matrix with torch and take the tiled
// path.
torch::Tensor floyd_warshall_dm_hip(torch::Tensor dm, torch::Tensor adj,
                                    c10::optional<torch::Tensor> n_arr) {
    TORCH_CHECK(dm.is_cuda() && dm.dim() == 3 && dm.size(1) == dm.size(2),
                "expected (B,N,N) CUDA tensor");
    TORCH_CHECK(adj.scalar_type() == torch::kBool
                && adj.sizes() == dm.sizes(), "adj: (B,N,N) bool expected");
    const int B = dm.size(0), N = dm.size(1);
    const size_t lds = (size_t)N * ((N + 3) & ~3) * sizeof(float);
    if (dm.scalar_type() != torch::kFloat || lds > LDS_LIMIT) {
        auto w = torch::where(adj, dm, torch::full_like(dm, INFINITY));
        auto eye = torch::eye(N, adj.options()).unsqueeze(0);
        return floyd_warshall_hip(
            torch::where(eye, torch::zeros_like(w), w), n_arr);
    }
    dm = dm.contiguous();
    adj = adj.contiguous();
    auto out = torch::empty_like(dm);
    const int* np_ = n_arr.has_value() ? n_arr->data_ptr<int>() : nullptr;
    auto stream = at::cuda::getCurrentCUDAStream().stream();
    if (!fw_reg_launch<true>(dm.data_ptr<float>(), adj.data_ptr<bool>(),
                             out.data_ptr<float>(), B, N, np_, stream))
        hipLaunchKernelGGL((fw_lds_kernel<float, true>), dim3(B), dim3(512),
                           lds, stream, dm.data_ptr<float>(),
                           adj.data_ptr<bool>(), out.data_ptr<float>(), N,
                           np_);
    return out;
}

void fw_force_inplace(bool on) { fw_inplace_forced = on; }

// rows per thread of the register kernel that serves fp32 (B,N,N) input;
// 0: N is outside its range (or it is switched off) and fw_lds_kernel or
// the tiled path runs
long fw_register_rows(long N) {
    return fw_inplace_forced || N < 1 || N > FWR_MAX_N ? 0
                                                        : fw_reg_rows((int)N);
}
