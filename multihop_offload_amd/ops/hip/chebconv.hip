// Fused ChebConv actor stack for gfx950 — the flagship kernel.
//
// Forward: all `L` ChebConv layers (Chebyshev order K ≤ 2: out =
// X·W0 + (A·X)·W1 + b, hidden leaky_relu(0.2), output relu) of the whole
// batch in ONE launch: one workgroup per graph, the activation matrices
// LDS-resident (row stride 33 f32 against bank conflicts), the extended
// line-graph adjacency (the "support"/Laplacian of the reference,
// gnn_offloading_agent.py:218,226) streamed from its CSR through L2, and
// the dense X·W products computed on MFMA tiles
// (`__builtin_amdgcn_mfma_f32_16x16x4f32`, 16×16 C-tiles, K=4 steps).
//
// Backward: the exact reverse (one launch): activation masks from the saved
// per-layer activations, per-graph dW/db partials (summed over the batch by
// torch), dX propagated through W0ᵀ and the symmetric SpMV.
//
// Feature dims are padded to 32 in the weight and gradient layouts
// (layer-0 input 4→32, output 1→32 with zero-padded weights; padding is
// exact — zero rows/cols contribute 0).
//
// Edge layers.  When the caller states a real output width of 1
// (cheb_fwd_edge / cheb_bwd_edge, L >= 2) the K<=2 kernels do the first and
// the last layer at their real width instead of working on the zeros:
//   forward, layer 0: a 4-column SpMV and one MFMA k-step per Chebyshev
//     term (the skipped terms are exact zeros, the k order is kept, so the
//     sums are bitwise those of the full-width path); T1_0 is saved 4 wide
//     at the head of t1s slot 0; no acts[0] store.
//   forward, last layer: only the c0 = 0 tile; lam goes from the MFMA
//     registers to memory; no acts[L] store.
//   backward, last layer: ReLU mask from lam; db of one column; both terms'
//     weight gradients in one pass over the two live tiles each (term ×
//     tile × row half = 8 waves, still two atomic addends per cell);
//     dX = d⊗w0 + (A·d)⊗w1 with a one-column gather — no MFMA product, no
//     32-column SpMV.
//   backward, layer 0: X_0 from x and T1_0 4 wide; weight gradients as in
//     the last layer, over the i0 = 0 tiles.
// dW / db cells outside the real shapes are never written again and stay
// the zeros the backward kernel stores at its top.  Any other width, the old entry points
// and cheb_force_full_width(true) run the full-width path.

#include <hip/hip_runtime.h>
#include <torch/extension.h>
#include <ATen/cuda/CUDAContext.h>

#include "cheb_tiles.h"

namespace {

using namespace cheb;

// row buffers (rows_pad×STRIDE each) in dynamic LDS; the launchers and
// cheb_fits_lds size the launch from these
constexpr int FWD_NBUF = 2;      // cheb_fwd_kernel: Xb | Tb
constexpr int BWD_NBUF = 3;      // cheb_bwd_kernel: Ab | Db | Tb
constexpr int KN_NBUF = 3;       // cheb_kn_*: Xb | Tb | Yb, Db | Pb | Qb

// 4 output tiles × 2 row-range halves keeps all 8 waves busy
constexpr int WGRAD_SPLIT = 2;

// ---- fused layer tile: Xb <- act(X·W0 + T·W1 + b) -----------------------
// In place: the two column halves of a row tile read the same A operands,
// all 32 columns of the tile's rows, so one wave owns both halves (as in
// gemm_layer_first): it has read every operand before it writes, and no
// other wave reads those rows.  With the halves on two waves and no barrier
// between the tiles of a wave, the wave that finished its half first wrote
// activated values into columns its neighbour was still reading (seen at
// K = 1 from 19 row tiles on: wrong and run-to-run different lam).  Each
// half keeps its k order, so the sums are bitwise what they were.
DEV_INLINE void gemm_layer_fused(float* __restrict__ Xb,
                                 const float* __restrict__ Tb,
                                 const float* __restrict__ Wl,
                                 const float* __restrict__ bl,
                                 int K, bool last, int rows_pad, int tid) {
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int nw = blockDim.x >> 6;
    const int r_in = lane & 15;
    const int k_in = lane >> 4;
    for (int mt = wid; mt < rows_pad / 16; mt += nw) {
        f32x4 acc[2] = {{0.f, 0.f, 0.f, 0.f}, {0.f, 0.f, 0.f, 0.f}};
#pragma unroll
        for (int kk = 0; kk < F / 4; ++kk) {
            const int k = kk * 4 + k_in;
            const float a = Xb[(mt * 16 + r_in) * STRIDE + k];
#pragma unroll
            for (int h = 0; h < 2; ++h)
                acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    a, Wl[k * F + h * 16 + r_in], acc[h], 0, 0, 0);
        }
        if (K > 1) {
#pragma unroll
            for (int kk = 0; kk < F / 4; ++kk) {
                const int k = kk * 4 + k_in;
                const float a = Tb[(mt * 16 + r_in) * STRIDE + k];
#pragma unroll
                for (int h = 0; h < 2; ++h)
                    acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                        a, Wl[F * F + k * F + h * 16 + r_in], acc[h], 0, 0,
                        0);
            }
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int col = h * 16 + (lane & 15);
            const float bv = bl[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + (lane >> 4) * 4 + r;
                Xb[row * STRIDE + col] = act(acc[h][r] + bv, last);
            }
        }
    }
}

// ---- fused backward tile: Tb <- D·W1ᵀ, Ab <- D·W0ᵀ (registers) ----------
DEV_INLINE void gemm_dx_fused(const float* __restrict__ Db,
                              float* __restrict__ Ab,
                              float* __restrict__ Tb,
                              const float* __restrict__ Wl, int K,
                              int rows_pad, int tid) {
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int nw = blockDim.x >> 6;
    const int mtiles = rows_pad / 16;
    const int r_in = lane & 15;
    const int k_in = lane >> 4;
    for (int t = wid; t < mtiles * 2; t += nw) {
        const int mt = t >> 1;
        const int c0 = (t & 1) * 16;
        f32x4 acc0 = {0.f, 0.f, 0.f, 0.f};
        f32x4 acc1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < F / 4; ++kk) {
            const int k = kk * 4 + k_in;
            const float d = Db[(mt * 16 + r_in) * STRIDE + k];
            acc0 = __builtin_amdgcn_mfma_f32_16x16x4f32(
                d, Wl[(c0 + r_in) * F + k], acc0, 0, 0, 0);
            if (K > 1)
                acc1 = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    d, Wl[F * F + (c0 + r_in) * F + k], acc1, 0, 0, 0);
        }
        const int col = c0 + (lane & 15);
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = mt * 16 + (lane >> 4) * 4 + r;
            Ab[row * STRIDE + col] = acc0[r];
            if (K > 1) Tb[row * STRIDE + col] = acc1[r];
        }
    }
}

// ---- SpMV over the support: dst[r][:] (+)= sum_nb src[nb][:] -------------
// modes: 0: dst = A·src; 1: dst += A·src; 2 (Chebyshev in place):
// dst = 2*(A·src) - dst; 3 (reverse recurrence): dst += 2*(A·src)
DEV_INLINE void spmv(const float* __restrict__ src, float* __restrict__ dst,
                     const int* __restrict__ indptr,
                     const int* __restrict__ cols, int Ee, int rows_pad,
                     int tid, int nt, int mode) {
    // thread handles (row, 8-col group)
    for (int task = tid; task < rows_pad * (F / 8); task += nt) {
        const int r = task / (F / 8);
        const int c0 = (task % (F / 8)) * 8;
        float acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        if (r < Ee) {
            // 4-way unrolled neighbor loop: 4 independent row pointers keep
            // 32 LDS reads in flight per iteration instead of 8 (the serial
            // version is latency-bound on the ds_read chain)
            int a = indptr[r];
            const int end = indptr[r + 1];
            float acc1[8] = {0, 0, 0, 0, 0, 0, 0, 0};
            for (; a + 3 < end; a += 4) {
                const float* s0 = src + cols[a] * STRIDE + c0;
                const float* s1 = src + cols[a + 1] * STRIDE + c0;
                const float* s2 = src + cols[a + 2] * STRIDE + c0;
                const float* s3 = src + cols[a + 3] * STRIDE + c0;
#pragma unroll
                for (int c = 0; c < 8; ++c) {
                    acc[c] += s0[c] + s1[c];
                    acc1[c] += s2[c] + s3[c];
                }
            }
            for (; a < end; ++a) {
                const float* s = src + cols[a] * STRIDE + c0;
#pragma unroll
                for (int c = 0; c < 8; ++c) acc[c] += s[c];
            }
#pragma unroll
            for (int c = 0; c < 8; ++c) acc[c] += acc1[c];
        }
        float* d = dst + r * STRIDE + c0;
        if (mode == 0) {
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] = acc[c];
        } else if (mode == 1) {
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] += acc[c];
        } else if (mode == 2) {
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] = 2.f * acc[c] - d[c];
        } else {
#pragma unroll
            for (int c = 0; c < 8; ++c) d[c] += 2.f * acc[c];
        }
    }
}

// ---- small LDS-tile helpers for the generic-K path -----------------------
DEV_INLINE void zero_rows(float* __restrict__ buf, int rows_pad, int tid,
                          int nt) {
    for (int t = tid; t < rows_pad * F; t += nt)
        buf[(t / F) * STRIDE + (t % F)] = 0.f;
}

DEV_INLINE void negate_rows(float* __restrict__ buf, int rows_pad, int tid,
                            int nt) {
    for (int t = tid; t < rows_pad * F; t += nt) {
        float* p = buf + (t / F) * STRIDE + (t % F);
        *p = -*p;
    }
}

DEV_INLINE void add_rows(float* __restrict__ dst,
                         const float* __restrict__ src, int rows_pad,
                         int tid, int nt) {
    for (int t = tid; t < rows_pad * F; t += nt)
        dst[(t / F) * STRIDE + (t % F)] += src[(t / F) * STRIDE + (t % F)];
}

// dst = act(src + bias): leaky_relu(0.2) hidden, relu on the last layer
DEV_INLINE void bias_act_rows(const float* __restrict__ src,
                              float* __restrict__ dst,
                              const float* __restrict__ bl, bool last,
                              int rows_pad, int tid, int nt) {
    for (int t = tid; t < rows_pad * F; t += nt) {
        const int r = t / F, c = t % F;
        dst[r * STRIDE + c] = act(src[r * STRIDE + c] + bl[c], last);
    }
}

// ---- kernel prologue, shared by the K<=2 and the generic-K kernels -------
// Point ipt/cls at graph b's support CSR.  With stage_csr the CSR is copied
// into LDS at `lds` first: it is read by every SpMV of every layer, and
// latency-bound global gathers otherwise dominate.  The caller's first
// barrier covers the copy.
DEV_INLINE void graph_csr(const int* __restrict__ ext_indptr,
                          const long* __restrict__ ext_base,
                          const int* __restrict__ ext_cols, int b, int Ee,
                          int stage_csr, int* __restrict__ lds, int tid,
                          int nt, const int*& ipt, const int*& cls) {
    ipt = ext_indptr + (size_t)b * (Ee + 1);
    cls = ext_cols + ext_base[b];
    if (stage_csr) {
        int* l_ipt = lds;
        int* l_cols = l_ipt + (Ee + 1);
        for (int i = tid; i < Ee + 1; i += nt) l_ipt[i] = ipt[i];
        const int nnz = ipt[Ee];
        for (int i = tid; i < nnz; i += nt) l_cols[i] = cls[i];
        ipt = l_ipt;
        cls = l_cols;
    }
}

// Xb <- features of one graph: 4 real cols as one float4, the rest (and the
// padded rows) zero
DEV_INLINE void load_features(float* __restrict__ Xb,
                              const float* __restrict__ xb, int Ee,
                              int rows_pad, int tid, int nt) {
    for (int r = tid; r < rows_pad; r += nt) {
        float* row = Xb + r * STRIDE;
        for (int c = 0; c < F; ++c) row[c] = 0.f;
        if (r < Ee) {
            const float4 v =
                *reinterpret_cast<const float4*>(xb + (size_t)r * 4);
            row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
        }
    }
}

// Db <- top delta of one graph: only column 0 carries dλ
DEV_INLINE void load_top_delta(float* __restrict__ Db,
                               const float* __restrict__ dlamb, int Ee,
                               int rows_pad, int tid, int nt) {
    for (int r = tid; r < rows_pad; r += nt) {
        float* row = Db + r * STRIDE;
        for (int c = 0; c < F; ++c) row[c] = 0.f;
        if (r < Ee) row[0] = dlamb[r];
    }
}

// ---- edge layers at their real width (header comment) --------------------
constexpr int FIN = 4;           // real input width of layer 0

// buf[:, 0:cols] <- a dense (Ee, 4) matrix in columns 0..3, zeros in the
// other columns and in the padded rows.  cols = 4 feeds the forward (which
// reads 4 columns), cols = 16 one wgrad tile.
DEV_INLINE void load_rows4(float* __restrict__ buf,
                           const float* __restrict__ g4, int cols, int Ee,
                           int rows_pad, int tid, int nt) {
    for (int r = tid; r < rows_pad; r += nt) {
        float* row = buf + r * STRIDE;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (r < Ee) v = *reinterpret_cast<const float4*>(g4 + (size_t)r * 4);
        row[0] = v.x; row[1] = v.y; row[2] = v.z; row[3] = v.w;
        for (int c = FIN; c < cols; ++c) row[c] = 0.f;
    }
}

// dst[r][0:4] = (A·src)[r][0:4]: the neighbour loop of spmv (pairs, two
// accumulators), so the sums are bitwise its columns 0..3
DEV_INLINE void spmv4(const float* __restrict__ src, float* __restrict__ dst,
                      const int* __restrict__ indptr,
                      const int* __restrict__ cols, int Ee, int rows_pad,
                      int tid, int nt) {
    for (int r = tid; r < rows_pad; r += nt) {
        float acc[FIN] = {0, 0, 0, 0};
        if (r < Ee) {
            int a = indptr[r];
            const int end = indptr[r + 1];
            float acc1[FIN] = {0, 0, 0, 0};
            for (; a + 3 < end; a += 4) {
                const float* s0 = src + cols[a] * STRIDE;
                const float* s1 = src + cols[a + 1] * STRIDE;
                const float* s2 = src + cols[a + 2] * STRIDE;
                const float* s3 = src + cols[a + 3] * STRIDE;
#pragma unroll
                for (int c = 0; c < FIN; ++c) {
                    acc[c] += s0[c] + s1[c];
                    acc1[c] += s2[c] + s3[c];
                }
            }
            for (; a < end; ++a) {
                const float* s = src + cols[a] * STRIDE;
#pragma unroll
                for (int c = 0; c < FIN; ++c) acc[c] += s[c];
            }
#pragma unroll
            for (int c = 0; c < FIN; ++c) acc[c] += acc1[c];
        }
#pragma unroll
        for (int c = 0; c < FIN; ++c) dst[r * STRIDE + c] = acc[c];
    }
}

// Layer 0: Xb <- act(X[:, 0:4]·W0[0:4] + T[:, 0:4]·W1[0:4] + b), the kk = 0
// steps of gemm_layer_fused in its order.  One wave owns both column halves
// of a row tile: it has read its A operands before it writes, and no other
// wave reads those rows.
DEV_INLINE void gemm_layer_first(float* __restrict__ Xb,
                                 const float* __restrict__ Tb,
                                 const float* __restrict__ Wl,
                                 const float* __restrict__ bl, int K,
                                 int rows_pad, int tid) {
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int nw = blockDim.x >> 6;
    const int r_in = lane & 15;
    const int k_in = lane >> 4;
    for (int mt = wid; mt < rows_pad / 16; mt += nw) {
        const float ax = Xb[(mt * 16 + r_in) * STRIDE + k_in];
        const float at = K > 1 ? Tb[(mt * 16 + r_in) * STRIDE + k_in] : 0.f;
        f32x4 acc[2];
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
            acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                ax, Wl[k_in * F + h * 16 + r_in], zero, 0, 0, 0);
            if (K > 1)
                acc[h] = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    at, Wl[F * F + k_in * F + h * 16 + r_in], acc[h], 0, 0,
                    0);
        }
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int col = h * 16 + (lane & 15);
            const float bv = bl[col];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + (lane >> 4) * 4 + r;
                Xb[row * STRIDE + col] = act(acc[h][r] + bv, false);
            }
        }
    }
}

// Last layer of real width 1: the c0 = 0 tile of gemm_layer_fused, column 0
// of it written straight to lam
DEV_INLINE void gemm_layer_last(const float* __restrict__ Xb,
                                const float* __restrict__ Tb,
                                const float* __restrict__ Wl,
                                const float* __restrict__ bl,
                                float* __restrict__ lam, int K, int Ee,
                                int rows_pad, int tid) {
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int nw = blockDim.x >> 6;
    const int r_in = lane & 15;
    const int k_in = lane >> 4;
    for (int mt = wid; mt < rows_pad / 16; mt += nw) {
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < F / 4; ++kk) {
            const int k = kk * 4 + k_in;
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                Xb[(mt * 16 + r_in) * STRIDE + k], Wl[k * F + r_in], acc, 0,
                0, 0);
        }
        if (K > 1) {
#pragma unroll
            for (int kk = 0; kk < F / 4; ++kk) {
                const int k = kk * 4 + k_in;
                acc = __builtin_amdgcn_mfma_f32_16x16x4f32(
                    Tb[(mt * 16 + r_in) * STRIDE + k],
                    Wl[F * F + k * F + r_in], acc, 0, 0, 0);
            }
        }
        if ((lane & 15) == 0) {
            const float bv = bl[0];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = mt * 16 + (lane >> 4) * 4 + r;
                if (row < Ee) lam[row] = act(acc[r] + bv, true);
            }
        }
    }
}

// Db[:, 0:16] <- top delta with the ReLU mask of the last layer: column 0
// is dλ where lam > 0 (lam == nullptr: unmasked), the rest of the one live
// wgrad tile zero
DEV_INLINE void load_top_delta_edge(float* __restrict__ Db,
                                    const float* __restrict__ dlamb,
                                    const float* __restrict__ lamb, int Ee,
                                    int rows_pad, int tid, int nt) {
    for (int r = tid; r < rows_pad; r += nt) {
        float* row = Db + r * STRIDE;
        float d = 0.f;
        if (r < Ee) d = dlamb[r] * (lamb ? dact(lamb[r], 0.f) : 1.f);
        row[0] = d;
        for (int c = 1; c < 16; ++c) row[c] = 0.f;
    }
}

// db[0] = sum_r D[r][0]: one wave, one plain store (db was zeroed and the
// cell has this one writer)
DEV_INLINE void db_col0(const float* __restrict__ D, int rows,
                        float* __restrict__ db_out, int tid) {
    if (tid >= 64) return;
    float acc = 0.f;
    for (int r = tid; r < rows; r += 64) acc += D[r * STRIDE];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (tid == 0) db_out[0] = acc;
}

// Weight gradients of an edge layer, both Chebyshev terms in one pass.
// Only the i0 = 0 tiles (layer 0, `first`) or the j0 = 0 tiles (last layer)
// are live: term × live tile × row half is one task per wave, and each cell
// still gets two atomic addends onto zero, which commute — dW stays
// run-to-run deterministic.  Cells outside the real shape are not written.
DEV_INLINE void wgrad_edge(const float* __restrict__ Xs,
                           const float* __restrict__ Ts,
                           const float* __restrict__ delta,
                           float* __restrict__ dw_out,  // global [K][32][32]
                           int K, bool first, int rows, int tid) {
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int nw = blockDim.x >> 6;
    const int n = rows / (4 * WGRAD_SPLIT);
    for (int t = wid; t < 2 * WGRAD_SPLIT * K; t += nw) {
        const int k = t / (2 * WGRAD_SPLIT);
        const int o = ((t / WGRAD_SPLIT) & 1) * 16;
        const int part = t % WGRAD_SPLIT;
        const int i0 = first ? 0 : o, j0 = first ? o : 0;
        const f32x4 acc = wgrad_tile(k ? Ts : Xs, delta, i0, j0, part * n,
                                     part * n + n, lane);
        if (first ? (lane >> 4) == 0 : (lane & 15) == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                atomicAdd(&dw_out[(size_t)k * F * F +
                                  (i0 + (lane >> 4) * 4 + r) * F + j0 +
                                  (lane & 15)], acc[r]);
        }
    }
}

// Last layer's dX = d⊗w0 + (A·d)⊗w1 into Ab, d = Db[:, 0]; wv = w0 | w1,
// column 0 of W_0 and W_1.  parts (timing ablation): bit0 the d⊗w0 term,
// bit1 the gather.
DEV_INLINE void dx_rank1(const float* __restrict__ Db, float* __restrict__ Ab,
                         const float* __restrict__ wv,
                         const int* __restrict__ indptr,
                         const int* __restrict__ cols, int Ee, int rows_pad,
                         int K, int parts, int tid, int nt) {
    for (int r = tid; r < rows_pad; r += nt) {
        const float dv = (parts & 1) ? Db[r * STRIDE] : 0.f;
        float ad = 0.f;
        if ((parts & 2) && K > 1 && r < Ee) {
            int a = indptr[r];
            const int end = indptr[r + 1];
            float ad1 = 0.f;
            for (; a + 3 < end; a += 4) {
                ad += Db[cols[a] * STRIDE] + Db[cols[a + 1] * STRIDE];
                ad1 += Db[cols[a + 2] * STRIDE] + Db[cols[a + 3] * STRIDE];
            }
            for (; a < end; ++a) ad += Db[cols[a] * STRIDE];
            ad += ad1;
        }
        float* o = Ab + r * STRIDE;
#pragma unroll
        for (int c = 0; c < F; ++c)
            o[c] = dv * wv[c] + (K > 1 ? ad * wv[F + c] : 0.f);
    }
}

// ---------------------------------------------------------------------------
// forward: x (B,Ee,4) → lam (B,Ee); saves per-layer activations
// LDS: Xb | Tb (rows_pad*STRIDE each) | Wl (K*32*32) | bias (32) | CSR
// EDGE: first and last layer at their real width (needs L >= 2): acts
// slots 0 and L are not written, t1s slot 0 holds T1_0 as (Ee,4)
// ---------------------------------------------------------------------------
template <bool EDGE>
__global__ void cheb_fwd_kernel(
    const float* __restrict__ x_in,      // (B,Ee,4)
    const float* __restrict__ W,         // (L,K,32,32) padded
    const float* __restrict__ bias,      // (L,32) padded
    const int* __restrict__ ext_indptr,  // (B,Ee+1)
    const long* __restrict__ ext_base,   // (B)
    const int* __restrict__ ext_cols,    // flat local
    float* __restrict__ acts,            // (B,L+1,Ee,32) out
    float* __restrict__ t1s,             // (B,L,Ee,32) out: A·X per layer
    float* __restrict__ lam,             // (B,Ee) out
    int Ee, int L, int K, int rows_pad, int stage_csr) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* Xb = reinterpret_cast<float*>(smem_raw);
    float* Tb = Xb + (size_t)rows_pad * STRIDE;
    float* Wl = Tb + (size_t)rows_pad * STRIDE;   // K*32*32
    float* bl = Wl + (size_t)K * F * F;           // 32

    const int b = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int *ipt, *cls;
    graph_csr(ext_indptr, ext_base, ext_cols, b, Ee, stage_csr,
              reinterpret_cast<int*>(bl + F), tid, nt, ipt, cls);
    float* actsb = acts + (size_t)b * (L + 1) * Ee * F;

    if (EDGE) {
        // ---- layer 0 at its real width: 4 columns in, rows 0..3 of W_k
        load_rows4(Xb, x_in + (size_t)b * Ee * 4, FIN, Ee, rows_pad, tid,
                   nt);
        for (int i = tid; i < K * FIN * F; i += nt)
            Wl[(i / (FIN * F)) * F * F + i % (FIN * F)] =
                W[(size_t)(i / (FIN * F)) * F * F + i % (FIN * F)];
        for (int i = tid; i < F; i += nt) bl[i] = bias[i];
        __syncthreads();
        if (K > 1) {
            spmv4(Xb, Tb, ipt, cls, Ee, rows_pad, tid, nt);
            __syncthreads();
            // T1_0, 4 wide, at the head of its t1s slot
            float4* t1b =
                reinterpret_cast<float4*>(t1s + (size_t)b * L * Ee * F);
            for (int r = tid; r < Ee; r += nt) {
                const float* s = Tb + r * STRIDE;
                t1b[r] = make_float4(s[0], s[1], s[2], s[3]);
            }
        }
        gemm_layer_first(Xb, Tb, Wl, bl, K, rows_pad, tid);
        __syncthreads();
        store_rows(Xb, actsb + (size_t)Ee * F, 0, Ee, Ee, tid, nt);
        __syncthreads();
    } else {
        load_features(Xb, x_in + (size_t)b * Ee * 4, Ee, rows_pad, tid, nt);
        __syncthreads();
        store_rows(Xb, actsb, 0, Ee, Ee, tid, nt);
    }

    // the full-width layers: all of them, or all but the two edge layers
    for (int l = EDGE ? 1 : 0; l < (EDGE ? L - 1 : L); ++l) {
        // stage weights + bias
        for (int i = tid; i < K * F * F; i += nt)
            Wl[i] = W[((size_t)l * K) * F * F + i];
        for (int i = tid; i < F; i += nt) bl[i] = bias[l * F + i];
        __syncthreads();
        if (K > 1) {
            spmv(Xb, Tb, ipt, cls, Ee, rows_pad, tid, nt, 0); // T1 = A·X
            __syncthreads();
            // save T1 for the backward weight-gradient pass
            store_rows(Tb, t1s + ((size_t)b * L + l) * Ee * F, 0, Ee,
                       Ee, tid, nt);
        }
        // in-register tile product + activation, written back into Xb
        gemm_layer_fused(Xb, Tb, Wl, bl, K, l == L - 1, rows_pad, tid);
        __syncthreads();
        store_rows(Xb, actsb + (size_t)(l + 1) * Ee * F, 0, Ee, Ee,
                   tid, nt);
        __syncthreads();
    }

    if (EDGE) {
        // ---- last layer at its real width: one output column
        const int l = L - 1;
        for (int i = tid; i < K * F * F; i += nt)
            Wl[i] = W[((size_t)l * K) * F * F + i];
        if (tid == 0) bl[0] = bias[l * F];
        __syncthreads();
        if (K > 1) {
            spmv(Xb, Tb, ipt, cls, Ee, rows_pad, tid, nt, 0);
            __syncthreads();
            store_rows(Tb, t1s + ((size_t)b * L + l) * Ee * F, 0, Ee, Ee,
                       tid, nt);
        }
        gemm_layer_last(Xb, Tb, Wl, bl, lam + (size_t)b * Ee, K, Ee,
                        rows_pad, tid);
    } else {
        for (int r = tid; r < Ee; r += nt) lam[(size_t)b * Ee + r] =
            Xb[r * STRIDE];
    }
}

// ---------------------------------------------------------------------------
// backward: dlam (B,Ee) + saved acts → per-graph dW (B,L,K,32,32),
// db (B,L,32); dX not needed at layer 0.
// LDS: Ab | Db | Tb | Wl | scratch
// ---------------------------------------------------------------------------
// stage_mask (timing ablation only — outputs are wrong unless 0xF):
// bit0 act-mask+db, bit1 load_rows+wgrads, bit2 dx gemm, bit3 spmv
// EDGE: the backward of the EDGE forward (x_in, lam and its acts / t1s), on
// the LDS plan of the full-width one.  On the last layer bit2 is the d⊗w0
// term and bit3 the one-column gather of dx_rank1.
template <bool EDGE>
__global__ void cheb_bwd_kernel(
    const float* __restrict__ dlam,      // (B,Ee)
    const float* __restrict__ x_in,      // (B,Ee,4)   (EDGE only)
    const float* __restrict__ lam,       // (B,Ee)     (EDGE only)
    const float* __restrict__ acts,      // (B,L+1,Ee,32)
    const float* __restrict__ t1s,       // (B,L,Ee,32): A·X from forward
    const float* __restrict__ W,         // (L,K,32,32)
    const int* __restrict__ ext_indptr,
    const long* __restrict__ ext_base,
    const int* __restrict__ ext_cols,
    float* __restrict__ dW,              // (B,L,K,32,32) out
    float* __restrict__ db,              // (B,L,32) out
    int Ee, int L, int K, int rows_pad, int stage_csr, int stage_mask) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* Ab = reinterpret_cast<float*>(smem_raw);   // X_l, later dX
    float* Db = Ab + (size_t)rows_pad * STRIDE;       // current delta
    float* Tb = Db + (size_t)rows_pad * STRIDE;
    float* Wl = Tb + (size_t)rows_pad * STRIDE;   // K*F*F

    const int b = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    float* dWb = dW + (size_t)b * L * K * F * F;
    float* dbb = db + (size_t)b * L * F;
    // dW / db arrive torch::empty: the workgroup zeroes its own slice (the
    // atomic adds and the cells outside an edge layer's real shape need it)
    // with stores nothing waits for; the first add is behind a barrier.
    // Both slices are whole float4s (F = 32).
    {
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        float4* w4 = reinterpret_cast<float4*>(dWb);
        for (int i = tid; i < L * K * F * F / 4; i += nt) w4[i] = z;
        float4* b4 = reinterpret_cast<float4*>(dbb);
        for (int i = tid; i < L * F / 4; i += nt) b4[i] = z;
    }
    const int *ipt, *cls;
    graph_csr(ext_indptr, ext_base, ext_cols, b, Ee, stage_csr,
              reinterpret_cast<int*>(Wl + (size_t)K * F * F), tid, nt, ipt,
              cls);
    const float* actsb = acts + (size_t)b * (L + 1) * Ee * F;

    if (EDGE) {
        // ---- last layer: the delta has one live column
        const int l = L - 1;
        load_top_delta_edge(Db, dlam + (size_t)b * Ee,
                            (stage_mask & 1) ? lam + (size_t)b * Ee : nullptr,
                            Ee, rows_pad, tid, nt);
        if (stage_mask & 2) {
            load_rows(Ab, actsb + (size_t)l * Ee * F, 0, rows_pad, Ee, tid,
                      nt);
            if (K > 1)
                load_rows(Tb, t1s + ((size_t)b * L + l) * Ee * F, 0,
                          rows_pad, Ee, tid, nt);
        }
        // w0 | w1: column 0 of W_0 and W_1
        for (int i = tid; i < K * F; i += nt)
            Wl[i] = W[(((size_t)l * K + i / F) * F + i % F) * F];
        __syncthreads();
        if (stage_mask & 1) db_col0(Db, Ee, dbb + l * F, tid);
        if (stage_mask & 2)
            wgrad_edge(Ab, Tb, Db, dWb + ((size_t)l * K) * F * F, K, false,
                       rows_pad, tid);
        __syncthreads();
        if (stage_mask & 12)
            dx_rank1(Db, Ab, Wl, ipt, cls, Ee, rows_pad, K,
                     (stage_mask >> 2) & 3, tid, nt);
        __syncthreads();
        float* tmp = Ab;
        Ab = Db;
        Db = tmp;
    } else {
        load_top_delta(Db, dlam + (size_t)b * Ee, Ee, rows_pad, tid, nt);
        __syncthreads();
    }

    // the full-width layers: all of them, or all but the two edge layers
    for (int l = EDGE ? L - 2 : L - 1; l >= (EDGE ? 1 : 0); --l) {
        const bool last = (l == L - 1);
        // activation mask from stored post-act X_{l+1} (coalesced float4)
        if (stage_mask & 1)
            mask_rows(Db, actsb + (size_t)(l + 1) * Ee * F, Ee,
                      last ? 0.f : 0.2f, tid, nt);
        // load X_l  (feeding the wgrad MFMA tiles straight from global
        // was MEASURED 2x slower — dependent-accumulator stalls on the
        // ~400-cycle loads; and folding db into the mask sweep above was
        // measured +13% — atomic flush every column-group change.
        // profiles/r02_notes.md: measure, don't guess.)
        if (stage_mask & 2) {
            if (EDGE)
                load_rows(Ab, actsb + (size_t)l * Ee * F, 0, rows_pad, Ee, tid,
                      nt);
            else
                load_rows(Ab, actsb + (size_t)l * Ee * F, 0, rows_pad, Ee,
                          tid, nt);
        }
        for (int i = tid; i < K * F * F; i += nt)
            Wl[i] = W[((size_t)l * K) * F * F + i];
        __syncthreads();

        if (stage_mask & 1) db_colsum(Db, Ee, dbb + l * F, tid, nt);
        if (stage_mask & 2) {
            if (K > 1)
                // issue the T1 staging loads BEFORE wgrad0: disjoint sets
                // (reads t1s/global, writes Tb rows vs wgrad0's Ab/Db
                // reads + dW atomics), so no barrier between them — the
                // global-load latency hides under the wgrad0 MFMA work
                load_rows(Tb, t1s + ((size_t)b * L + l) * Ee * F, 0,
                          rows_pad, Ee, tid, nt);         // T1 from forward
            wgrad_rows<WGRAD_SPLIT>(Ab, Db, dWb + ((size_t)l * K) * F * F,
                                    rows_pad, tid);
            if (K > 1) {
                __syncthreads();
                wgrad_rows<WGRAD_SPLIT>(Tb, Db,
                                        dWb + ((size_t)l * K + 1) * F * F,
                                        rows_pad, tid);
            }
        }
        if (l == 0) break;                       // features are leaves
        __syncthreads();
        // U = Db·W1ᵀ (into Tb) and dX = Db·W0ᵀ (into Ab), fused per tile
        if (stage_mask & 4)
            gemm_dx_fused(Db, Ab, Tb, Wl, K, rows_pad, tid);
        __syncthreads();
        if ((stage_mask & 8) && K > 1) {
            spmv(Tb, Ab, ipt, cls, Ee, rows_pad, tid, nt, 1); // dX += A·U
            __syncthreads();
        }
        // swap: Ab (dX) becomes the delta of the layer below
        float* tmp = Ab;
        Ab = Db;
        Db = tmp;
        if (!EDGE) __syncthreads();
    }

    if (EDGE) {
        // ---- layer 0: X_0 = x and T1_0, 4 wide; db, the i0 = 0 tiles of dW
        if (stage_mask & 1)
            mask_rows(Db, actsb + (size_t)Ee * F, Ee, 0.2f, tid, nt);
        if (stage_mask & 2) {
            load_rows4(Ab, x_in + (size_t)b * Ee * 4, 16, Ee, rows_pad, tid,
                       nt);
            if (K > 1)
                load_rows4(Tb, t1s + (size_t)b * L * Ee * F, 16, Ee,
                           rows_pad, tid, nt);
        }
        __syncthreads();
        if (stage_mask & 1) db_colsum(Db, Ee, dbb, tid, nt);
        if (stage_mask & 2)
            wgrad_edge(Ab, Tb, Db, dWb, K, true, rows_pad, tid);
    }
}

// ---------------------------------------------------------------------------
// Generic-K (K >= 2, covers K > 2) fused ChebConv stack.  Three LDS row
// buffers carry the Chebyshev recurrence T_k = 2·A·T_{k-1} − T_{k-2}
// (T_0 = X, T_1 = A·X; models/chebconv.py:54-63): Xb holds T_{k-2} and is
// consumed in place, Tb holds T_{k-1}, Yb accumulates Σ_k T_k·W_k.  The
// per-layer T_k (k >= 1) land in `tks` for the backward's weight
// gradients; the backward reverses the recurrence with the adjoint
// ĝ_{k-1} += 2·A·ĝ_k, ĝ_{k-2} −= ĝ_k (A symmetric), dX = ĝ_0 + A·ĝ_1.
// The K<=2 kernels above stay the tuned flagship path.
// ---------------------------------------------------------------------------
__global__ void cheb_kn_fwd_kernel(
    const float* __restrict__ x_in,      // (B,Ee,4)
    const float* __restrict__ W,         // (L,K,32,32) padded
    const float* __restrict__ bias,      // (L,32)
    const int* __restrict__ ext_indptr,  // (B,Ee+1)
    const long* __restrict__ ext_base,   // (B)
    const int* __restrict__ ext_cols,
    float* __restrict__ acts,            // (B,L+1,Ee,32) out
    float* __restrict__ tks,             // (B,L,K-1,Ee,32) out
    float* __restrict__ lam,             // (B,Ee) out
    int B, int Ee, int L, int K, int rows_pad, int stage_csr) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* Xb = reinterpret_cast<float*>(smem_raw);
    float* Tb = Xb + (size_t)rows_pad * STRIDE;
    float* Yb = Tb + (size_t)rows_pad * STRIDE;
    float* Wl = Yb + (size_t)rows_pad * STRIDE;   // K*32*32
    float* bl = Wl + (size_t)K * F * F;           // 32

    const int b = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int *ipt, *cls;
    graph_csr(ext_indptr, ext_base, ext_cols, b, Ee, stage_csr,
              reinterpret_cast<int*>(bl + F), tid, nt, ipt, cls);
    float* actsb = acts + (size_t)b * (L + 1) * Ee * F;
    float* tksb = tks + (size_t)b * L * (K - 1) * Ee * F;

    load_features(Xb, x_in + (size_t)b * Ee * 4, Ee, rows_pad, tid, nt);
    __syncthreads();
    store_rows(Xb, actsb, 0, Ee, Ee, tid, nt);

    for (int l = 0; l < L; ++l) {
        for (int i = tid; i < K * F * F; i += nt)
            Wl[i] = W[((size_t)l * K) * F * F + i];
        for (int i = tid; i < F; i += nt) bl[i] = bias[l * F + i];
        zero_rows(Yb, rows_pad, tid, nt);
        __syncthreads();
        gemm_rows(Xb, Yb, Wl, false, rows_pad, tid);          // T0·W0
        spmv(Xb, Tb, ipt, cls, Ee, rows_pad, tid, nt, 0);     // T1 = A·X
        __syncthreads();
        store_rows(Tb, tksb + (size_t)l * (K - 1) * Ee * F, 0, Ee, Ee,
                   tid, nt);
        gemm_rows(Tb, Yb, Wl + F * F, false, rows_pad, tid);  // T1·W1
        float* prev = Xb;                                     // T_{k-2}
        float* cur = Tb;                                      // T_{k-1}
        for (int k = 2; k < K; ++k) {
            __syncthreads();
            spmv(cur, prev, ipt, cls, Ee, rows_pad, tid, nt, 2);
            __syncthreads();
            float* t = prev; prev = cur; cur = t;             // cur = T_k
            store_rows(cur, tksb + ((size_t)l * (K - 1) + k - 1) * Ee * F,
                       0, Ee, Ee, tid, nt);
            gemm_rows(cur, Yb, Wl + (size_t)k * F * F, false, rows_pad,
                      tid);
        }
        __syncthreads();
        bias_act_rows(Yb, Xb, bl, l == L - 1, rows_pad, tid, nt);
        __syncthreads();
        store_rows(Xb, actsb + (size_t)(l + 1) * Ee * F, 0, Ee, Ee,
                   tid, nt);
        __syncthreads();
    }
    for (int r = tid; r < Ee; r += nt) lam[(size_t)b * Ee + r] =
        Xb[r * STRIDE];
}

__global__ void cheb_kn_bwd_kernel(
    const float* __restrict__ dlam,      // (B,Ee)
    const float* __restrict__ acts,      // (B,L+1,Ee,32)
    const float* __restrict__ tks,       // (B,L,K-1,Ee,32)
    const float* __restrict__ W,         // (L,K,32,32)
    const int* __restrict__ ext_indptr,
    const long* __restrict__ ext_base,
    const int* __restrict__ ext_cols,
    float* __restrict__ dW,              // (B,L,K,32,32) out (prezeroed)
    float* __restrict__ db,              // (B,L,32) out (prezeroed)
    int B, int Ee, int L, int K, int rows_pad, int stage_csr) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    float* Db = reinterpret_cast<float*>(smem_raw);   // delta
    float* Pb = Db + (size_t)rows_pad * STRIDE;
    float* Qb = Pb + (size_t)rows_pad * STRIDE;
    float* Wl = Qb + (size_t)rows_pad * STRIDE;       // K*F*F

    const int b = blockIdx.x;
    const int tid = threadIdx.x, nt = blockDim.x;
    const int *ipt, *cls;
    graph_csr(ext_indptr, ext_base, ext_cols, b, Ee, stage_csr,
              reinterpret_cast<int*>(Wl + (size_t)K * F * F), tid, nt, ipt,
              cls);
    const float* actsb = acts + (size_t)b * (L + 1) * Ee * F;
    const float* tksb = tks + (size_t)b * L * (K - 1) * Ee * F;
    float* dWb = dW + (size_t)b * L * K * F * F;
    float* dbb = db + (size_t)b * L * F;

    load_top_delta(Db, dlam + (size_t)b * Ee, Ee, rows_pad, tid, nt);
    __syncthreads();

    for (int l = L - 1; l >= 0; --l) {
        const bool last = (l == L - 1);
        mask_rows(Db, actsb + (size_t)(l + 1) * Ee * F, Ee,
                  last ? 0.f : 0.2f, tid, nt);
        for (int i = tid; i < K * F * F; i += nt)
            Wl[i] = W[((size_t)l * K) * F * F + i];
        __syncthreads();
        db_colsum(Db, Ee, dbb + l * F, tid, nt);
        // weight gradients: dW_k = T_kᵀ·Db, T_k streamed through Pb
        load_rows(Pb, actsb + (size_t)l * Ee * F, 0, rows_pad, Ee, tid, nt);
        __syncthreads();
        wgrad_rows<WGRAD_SPLIT>(Pb, Db, dWb + ((size_t)l * K) * F * F,
                                rows_pad, tid);
        for (int k = 1; k < K; ++k) {
            __syncthreads();
            load_rows(Pb, tksb + ((size_t)l * (K - 1) + k - 1) * Ee * F, 0,
                      rows_pad, Ee, tid, nt);
            __syncthreads();
            wgrad_rows<WGRAD_SPLIT>(Pb, Db,
                                    dWb + ((size_t)l * K + k) * F * F,
                                    rows_pad, tid);
        }
        if (l == 0) break;
        __syncthreads();
        // dX via the reverse recurrence (buffers: Pb=ĝ_cur, Qb=ĝ_prev)
        zero_rows(Pb, rows_pad, tid, nt);
        zero_rows(Qb, rows_pad, tid, nt);
        __syncthreads();
        if (K == 1) {
            gemm_rows(Db, Pb, Wl, true, rows_pad, tid);        // ĝ_0
            __syncthreads();
            // dX = ĝ_0 → copy into Db
            for (int t = tid; t < rows_pad * F; t += nt)
                Db[(t / F) * STRIDE + (t % F)] =
                    Pb[(t / F) * STRIDE + (t % F)];
        } else {
            gemm_rows(Db, Pb, Wl + (size_t)(K - 1) * F * F, true, rows_pad,
                     tid);                                    // ĝ_{K-1}
            gemm_rows(Db, Qb, Wl + (size_t)(K - 2) * F * F, true, rows_pad,
                     tid);                                    // ĝ_{K-2} base
            float* cur = Pb;
            float* prv = Qb;
            for (int k = K - 1; k >= 2; --k) {
                __syncthreads();
                spmv(cur, prv, ipt, cls, Ee, rows_pad, tid, nt, 3);
                __syncthreads();
                negate_rows(cur, rows_pad, tid, nt);          // −ĝ_k
                __syncthreads();
                gemm_rows(Db, cur, Wl + (size_t)(k - 2) * F * F, true,
                         rows_pad, tid);                      // + base_{k-2}
                float* t = cur; cur = prv; prv = t;           // cur=ĝ_{k-1}
            }
            __syncthreads();
            // dX = ĝ_0 + A·ĝ_1  (cur=ĝ_1, prv=ĝ_0)
            spmv(cur, Db, ipt, cls, Ee, rows_pad, tid, nt, 0);
            __syncthreads();
            add_rows(Db, prv, rows_pad, tid, nt);
        }
        __syncthreads();
    }
}

}  // namespace

// Does a graph of Ee extended links run on the LDS-resident kernels of this
// K, forward and backward?  The Python side routes on this.
bool cheb_fits_lds(long Ee, long K) {
    const bool kn = K > 2;
    return cheb_lds_plan(Ee, K, kn ? KN_NBUF : FWD_NBUF, true, 0).fits &&
           cheb_lds_plan(Ee, K, kn ? KN_NBUF : BWD_NBUF, false, 0).fits;
}

// Host-only: the plan each LDS-resident launcher computes at this shape
// (nothing is launched).  fwd/bwd are the K<=2 kernels (plain and edge share
// a plan), kn_* the generic-K ones; the tests ask it whether a launch stages
// the support CSR in LDS or reads it from global memory.
py::dict cheb_lds_plan_py(long Ee, long K, long max_nnz) {
    using namespace pybind11::literals;
    auto row = [&](int nbuf, bool with_bias) {
        const LdsPlan p = cheb_lds_plan((int)Ee, (int)K, nbuf, with_bias,
                                        max_nnz);
        return py::dict("rows_pad"_a = p.rows_pad,
                        "lds_bytes"_a = (long)p.lds_bytes,
                        "stage_csr"_a = p.stage_csr, "fits"_a = p.fits);
    };
    return py::dict("fwd"_a = row(FWD_NBUF, true),
                    "bwd"_a = row(BWD_NBUF, false),
                    "kn_fwd"_a = row(KN_NBUF, true),
                    "kn_bwd"_a = row(KN_NBUF, false));
}

// cheb_force_full_width(true): every later cheb_fwd_edge launch takes the
// full-width path whatever the stated width (before/after timings, tests,
// bisecting); false restores the choice by width.  Read when the forward is
// launched; the backward follows the flag its forward returned.
static bool cheb_full_forced = false;
void cheb_force_full_width(bool on) { cheb_full_forced = on; }

static std::vector<torch::Tensor> cheb_fwd_launch(
    torch::Tensor x, torch::Tensor W, torch::Tensor bias,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz, bool edge) {
    const int B = x.size(0), Ee = x.size(1);
    const int L = W.size(0), K = W.size(1);
    TORCH_CHECK(K <= 2, "fused ChebConv kernel supports K<=2");
    TORCH_CHECK(x.dim() == 3 && x.size(2) == FIN && x.is_contiguous(),
                "x must be a contiguous (B,Ee,4)");
    const LdsPlan plan = cheb_lds_plan(Ee, K, FWD_NBUF, true, max_nnz);
    TORCH_CHECK(plan.fits, "graph too large for fused ChebConv");
    auto acts = torch::empty({B, L + 1, Ee, F}, x.options());
    auto t1s = torch::empty({B, L, Ee, F}, x.options());
    auto lam = torch::empty({B, Ee}, x.options());
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(edge ? cheb_fwd_kernel<true> : cheb_fwd_kernel<false>,
                       dim3(B), dim3(512), plan.lds_bytes, stream.stream(),
                       x.data_ptr<float>(), W.data_ptr<float>(),
                       bias.data_ptr<float>(), ext_indptr.data_ptr<int>(),
                       ext_base.data_ptr<long>(), ext_cols.data_ptr<int>(),
                       acts.data_ptr<float>(), t1s.data_ptr<float>(),
                       lam.data_ptr<float>(),
                       Ee, L, K, plan.rows_pad, plan.stage_csr);
    return {lam, acts, t1s};
}

std::vector<torch::Tensor> cheb_fwd_hip(
    torch::Tensor x, torch::Tensor W, torch::Tensor bias,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz) {
    return cheb_fwd_launch(x, W, bias, ext_indptr, ext_base, ext_cols,
                           max_nnz, false);
}

// The forward for weights whose real output width the caller states
// (W, bias zero-padded outside the real shapes).  Width 1 and L >= 2 take
// the edge-layer path, anything else the full-width one.  Returns (lam,
// acts, t1s, edge); with edge set, acts slots 0 and L and the tail of t1s
// slot 0 are unwritten and only cheb_bwd_edge(..., edge) reads the rest.
std::tuple<torch::Tensor, torch::Tensor, torch::Tensor, bool>
cheb_fwd_edge_hip(torch::Tensor x, torch::Tensor W, torch::Tensor bias,
                  torch::Tensor ext_indptr, torch::Tensor ext_base,
                  torch::Tensor ext_cols, long max_nnz, long out_width) {
    const bool edge = !cheb_full_forced && out_width == 1 && W.size(0) >= 2;
    auto out = cheb_fwd_launch(x, W, bias, ext_indptr, ext_base, ext_cols,
                               max_nnz, edge);
    return {out[0], out[1], out[2], edge};
}

std::vector<torch::Tensor> cheb_kn_fwd_hip(
    torch::Tensor x, torch::Tensor W, torch::Tensor bias,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz) {
    const int B = x.size(0), Ee = x.size(1);
    const int L = W.size(0), K = W.size(1);
    TORCH_CHECK(K >= 2, "generic-K ChebConv kernel expects K>=2");
    const LdsPlan plan = cheb_lds_plan(Ee, K, KN_NBUF, true, max_nnz);
    TORCH_CHECK(plan.fits,
                "graph too large for generic-K fused ChebConv (LDS)");
    auto acts = torch::empty({B, L + 1, Ee, F}, x.options());
    auto tks = torch::empty({B, L, K - 1, Ee, F}, x.options());
    auto lam = torch::empty({B, Ee}, x.options());
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(cheb_kn_fwd_kernel, dim3(B), dim3(512),
                       plan.lds_bytes, stream.stream(),
                       x.data_ptr<float>(), W.data_ptr<float>(),
                       bias.data_ptr<float>(), ext_indptr.data_ptr<int>(),
                       ext_base.data_ptr<long>(), ext_cols.data_ptr<int>(),
                       acts.data_ptr<float>(), tks.data_ptr<float>(),
                       lam.data_ptr<float>(),
                       B, Ee, L, K, plan.rows_pad, plan.stage_csr);
    return {lam, acts, tks};
}

std::vector<torch::Tensor> cheb_kn_bwd_hip(
    torch::Tensor dlam, torch::Tensor acts, torch::Tensor tks,
    torch::Tensor W, torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz) {
    const int B = dlam.size(0), Ee = dlam.size(1);
    const int L = W.size(0), K = W.size(1);
    const LdsPlan plan = cheb_lds_plan(Ee, K, KN_NBUF, false, max_nnz);
    TORCH_CHECK(plan.fits,
                "graph too large for generic-K fused ChebConv bwd (LDS)");
    auto dW = torch::zeros({B, L, K, F, F}, dlam.options());
    auto db = torch::zeros({B, L, F}, dlam.options());
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(cheb_kn_bwd_kernel, dim3(B), dim3(512),
                       plan.lds_bytes, stream.stream(),
                       dlam.data_ptr<float>(), acts.data_ptr<float>(),
                       tks.data_ptr<float>(), W.data_ptr<float>(),
                       ext_indptr.data_ptr<int>(), ext_base.data_ptr<long>(),
                       ext_cols.data_ptr<int>(),
                       dW.data_ptr<float>(), db.data_ptr<float>(),
                       B, Ee, L, K, plan.rows_pad, plan.stage_csr);
    return {dW, db};
}

// edge: the forward's flag; x and lam are read only when it is set
std::vector<torch::Tensor> cheb_bwd_edge_hip_mask(
    torch::Tensor dlam, torch::Tensor x, torch::Tensor lam,
    torch::Tensor acts, torch::Tensor t1s, torch::Tensor W,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz, bool edge, long stage_mask) {
    const int B = dlam.size(0), Ee = dlam.size(1);
    const int L = W.size(0), K = W.size(1);
    TORCH_CHECK(K <= 2, "fused ChebConv kernel supports K<=2");
    TORCH_CHECK(dlam.is_contiguous() && acts.size(0) == B &&
                acts.size(1) == L + 1 && acts.size(2) == Ee &&
                t1s.size(0) == B && t1s.size(1) == L && t1s.size(2) == Ee,
                "cheb_bwd: dlam / acts / t1s shapes disagree");
    if (edge)
        TORCH_CHECK(L >= 2 && x.dim() == 3 && x.size(0) == B &&
                    x.size(1) == Ee && x.size(2) == FIN &&
                    x.is_contiguous() && lam.dim() == 2 &&
                    lam.size(0) == B && lam.size(1) == Ee &&
                    lam.is_contiguous(),
                    "cheb_bwd_edge: x (B,Ee,4) and lam (B,Ee) of the "
                    "forward expected");
    const LdsPlan plan = cheb_lds_plan(Ee, K, BWD_NBUF, false, max_nnz);
    TORCH_CHECK(plan.fits, "graph too large for fused ChebConv bwd");
    // each workgroup zeroes its own slice: no fill launches
    auto dW = torch::empty({B, L, K, F, F}, dlam.options());
    auto db = torch::empty({B, L, F}, dlam.options());
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(edge ? cheb_bwd_kernel<true> : cheb_bwd_kernel<false>,
                       dim3(B), dim3(512), plan.lds_bytes, stream.stream(),
                       dlam.data_ptr<float>(),
                       edge ? x.data_ptr<float>() : nullptr,
                       edge ? lam.data_ptr<float>() : nullptr,
                       acts.data_ptr<float>(), t1s.data_ptr<float>(),
                       W.data_ptr<float>(), ext_indptr.data_ptr<int>(),
                       ext_base.data_ptr<long>(), ext_cols.data_ptr<int>(),
                       dW.data_ptr<float>(), db.data_ptr<float>(),
                       Ee, L, K, plan.rows_pad, plan.stage_csr,
                       (int)stage_mask);
    return {dW, db};
}

std::vector<torch::Tensor> cheb_bwd_edge_hip(
    torch::Tensor dlam, torch::Tensor x, torch::Tensor lam,
    torch::Tensor acts, torch::Tensor t1s, torch::Tensor W,
    torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz, bool edge) {
    return cheb_bwd_edge_hip_mask(dlam, x, lam, acts, t1s, W, ext_indptr,
                                  ext_base, ext_cols, max_nnz, edge, 0xF);
}

std::vector<torch::Tensor> cheb_bwd_hip_mask(
    torch::Tensor dlam, torch::Tensor acts, torch::Tensor t1s,
    torch::Tensor W, torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz, long stage_mask) {
    return cheb_bwd_edge_hip_mask(dlam, torch::Tensor(), torch::Tensor(),
                                  acts, t1s, W, ext_indptr, ext_base,
                                  ext_cols, max_nnz, false, stage_mask);
}

std::vector<torch::Tensor> cheb_bwd_hip(
    torch::Tensor dlam, torch::Tensor acts, torch::Tensor t1s,
    torch::Tensor W, torch::Tensor ext_indptr, torch::Tensor ext_base,
    torch::Tensor ext_cols, long max_nnz) {
    return cheb_bwd_hip_mask(dlam, acts, t1s, W, ext_indptr, ext_base,
                             ext_cols, max_nnz, 0xF);
}
