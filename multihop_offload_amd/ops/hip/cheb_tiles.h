// Tile primitives shared by the three ChebConv kernel families:
// the K<=2 flagship kernels and the generic-K kernels (chebconv.hip, whole
// graph LDS-resident) and the row-tiled large-graph kernels
// (chebconv_large.hip).  One definition of the LDS row layout, the MFMA
// operand layouts and the LDS budget, so a layout experiment is a one-place
// change.
//
// Everything device-side is force-inlined: callers pass compile-time
// constants (the row-tile height, the wgrad split) where they have them and
// the loops fold to the same constant trip counts as hand-written copies.

#pragma once

#include <hip/hip_runtime.h>

#include "gfx950.h"

namespace cheb {

constexpr int F = 32;          // padded feature width
constexpr int STRIDE = 33;     // LDS row stride (f32) — breaks bank conflicts
typedef float f32x4 __attribute__((ext_vector_type(4)));

// leaky_relu(0.2) on hidden layers, relu on the last
DEV_INLINE float act(float y, bool last) {
    return last ? (y > 0.f ? y : 0.f) : (y > 0.f ? y : 0.2f * y);
}

// act'(·) read off the stored post-activation x; slope is 0.2 on hidden
// layers and 0 on the last
DEV_INLINE float dact(float x, float slope) { return x > 0.f ? 1.f : slope; }

// ---- dense tile product: dst += src · W  (or · Wᵀ), MFMA 16×16×4 ---------
// src, dst: LDS [rows][STRIDE], rows a multiple of 16; W: LDS [32][32]
// row-major [in][out].  Wave w owns tiles w, w+nw, ... of (rows/16 × 2).
DEV_INLINE void gemm_rows(const float* __restrict__ src,
                          float* __restrict__ dst,
                          const float* __restrict__ W, bool transposeW,
                          int rows, int tid) {
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int nw = blockDim.x >> 6;
    const int mtiles = rows / 16;
    const int r_in = lane & 15;          // A-operand row within tile
    const int k_in = lane >> 4;          // A/B k index (0..3)
    for (int t = wid; t < mtiles * 2; t += nw) {
        const int mt = t >> 1;
        const int c0 = (t & 1) * 16;
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int kk = 0; kk < F / 4; ++kk) {
            const int k = kk * 4 + k_in;
            const float a = src[(mt * 16 + r_in) * STRIDE + k];
            const float b = transposeW ? W[(c0 + r_in) * F + k]
                                       : W[k * F + c0 + r_in];
            acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
        }
        // C layout: col = lane&15, row = (lane>>4)*4 + reg
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = mt * 16 + (lane >> 4) * 4 + r;
            dst[row * STRIDE + c0 + (lane & 15)] += acc[r];
        }
    }
}

// ---- weight-gradient tile: dW[i][j] += sum_r src[r][i] * delta[r][j] -----
// MFMA over the row (K) dimension.  wgrad_tile: one wave's 16×16 tile at
// (i0, j0) over the row k-steps [kk0, kk1) (4 rows each), C layout as in
// gemm_rows.
DEV_INLINE f32x4 wgrad_tile(const float* __restrict__ src,
                            const float* __restrict__ delta, int i0, int j0,
                            int kk0, int kk1, int lane) {
    const int k_in = lane >> 4;
    const int c_in = lane & 15;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int kk = kk0; kk < kk1; ++kk) {
        const int r = kk * 4 + k_in;
        const float a = src[r * STRIDE + i0 + c_in];
        const float b = delta[r * STRIDE + j0 + c_in];
        acc = __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, acc, 0, 0, 0);
    }
    return acc;
}

// 2×2 output tiles of 16×16, each over SPLIT equal row ranges (rows a
// multiple of 4*SPLIT); one (tile, range) per wave.  The ranges and the row
// tiles of a graph combine through global fp32 atomics (dW is zero by
// then: the K<=2 backward zeroes its own slice, the other launchers fill
// it).
template <int SPLIT>
DEV_INLINE void wgrad_rows(const float* __restrict__ src,
                           const float* __restrict__ delta,
                           float* __restrict__ dw_out,  // global [32][32]
                           int rows, int tid) {
    const int lane = tid & 63;
    const int wid = tid >> 6;
    const int nw = blockDim.x >> 6;
    for (int t = wid; t < 4 * SPLIT; t += nw) {
        const int tile = t / SPLIT, part = t % SPLIT;
        const int i0 = (tile >> 1) * 16, j0 = (tile & 1) * 16;
        const int kk0 = part * (rows / (4 * SPLIT));
        const int kk1 = kk0 + rows / (4 * SPLIT);
        const f32x4 acc = wgrad_tile(src, delta, i0, j0, kk0, kk1, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r)
            atomicAdd(&dw_out[(i0 + (lane >> 4) * 4 + r) * F + j0
                              + (lane & 15)], acc[r]);
    }
}

// ---- row tile <-> global copies (coalesced, float4 on global) ------------
// The LDS tile holds `rows` rows that map to global rows [r0, r0+rows) of a
// dense (Ee, F) matrix.  LDS rows have stride 33 (misaligned for vector LDS
// ops); global rows are dense F=32 floats, 16B-aligned.  The task split
// (row, 4-col group) puts consecutive lanes on consecutive 16B segments.
// Loads zero-fill rows at or past Ee; stores clamp the row count to Ee, so
// a caller whose tile starts at row 0 passes rows = Ee and the clamp folds
// away.  `f` maps the float4 on its way through: f(value, global element
// offset) on loads, f(value, first column) on stores.
template <class Fn>
DEV_INLINE void load_rows(float* __restrict__ lds,
                          const float* __restrict__ gmem, int r0, int rows,
                          int Ee, int tid, int nt, Fn f) {
    for (int t = tid; t < rows * (F / 4); t += nt) {
        const int rr = t >> 3;
        const int c = (t & 7) * 4;
        float4 v = {0.f, 0.f, 0.f, 0.f};
        if (r0 + rr < Ee) {
            const size_t off = (size_t)(r0 + rr) * F + c;
            v = f(*reinterpret_cast<const float4*>(gmem + off), off);
        }
        float* d = lds + rr * STRIDE + c;
        d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
    }
}

DEV_INLINE void load_rows(float* __restrict__ lds,
                          const float* __restrict__ gmem, int r0, int rows,
                          int Ee, int tid, int nt) {
    load_rows(lds, gmem, r0, rows, Ee, tid, nt,
              [](float4 v, size_t) { return v; });
}

template <class Fn>
DEV_INLINE void store_rows(const float* __restrict__ lds,
                           float* __restrict__ gmem, int r0, int rows,
                           int Ee, int tid, int nt, Fn f) {
    const int n = min(rows, Ee - r0);
    for (int t = tid; t < n * (F / 4); t += nt) {
        const int rr = t >> 3;
        const int c = (t & 7) * 4;
        const float* s = lds + rr * STRIDE + c;
        const float4 v = {s[0], s[1], s[2], s[3]};
        *reinterpret_cast<float4*>(gmem + (size_t)(r0 + rr) * F + c) =
            f(v, c);
    }
}

DEV_INLINE void store_rows(const float* __restrict__ lds,
                           float* __restrict__ gmem, int r0, int rows,
                           int Ee, int tid, int nt) {
    store_rows(lds, gmem, r0, rows, Ee, tid, nt,
               [](float4 v, int) { return v; });
}

// ---- D ⊙= act'(X_{l+1}) in place on an LDS-resident delta ----------------
// xact: the stored post-activation rows (Ee, F) in global memory.
DEV_INLINE void mask_rows(float* __restrict__ D,
                          const float* __restrict__ xact, int Ee,
                          float slope, int tid, int nt) {
    for (int t = tid; t < Ee * (F / 4); t += nt) {
        const int r = t >> 3;
        const int c = (t & 7) * 4;
        const float4 v =
            *reinterpret_cast<const float4*>(xact + (size_t)r * F + c);
        float* d = D + r * STRIDE + c;
        d[0] *= dact(v.x, slope);
        d[1] *= dact(v.y, slope);
        d[2] *= dact(v.z, slope);
        d[3] *= dact(v.w, slope);
    }
}

// ---- db[j] += sum_r D[r][j] over `rows` LDS rows -------------------------
// (column, row-chunk) threads, one atomic per thread; db is zero by then, like dW.
// The chunk order of the atomics is not fixed, so db is reproducible only
// to the last bits.
DEV_INLINE void db_colsum(const float* __restrict__ D, int rows,
                          float* __restrict__ db_out, int tid, int nt) {
    const int nchunk = nt / F;
    const int j = tid % F, ch = tid / F;
    float acc = 0.f;
    for (int r = ch; r < rows; r += nchunk) acc += D[r * STRIDE + j];
    atomicAdd(&db_out[j], acc);
}

// ---- (A·src)[r][c0..c0+3] for a dense global src (Ee, F) -----------------
DEV_INLINE float4 csr_gather4(const float* __restrict__ src,
                              const int* __restrict__ indptr,
                              const int* __restrict__ cols, int r, int c0) {
    float4 acc = {0.f, 0.f, 0.f, 0.f};
    for (int a = indptr[r]; a < indptr[r + 1]; ++a) {
        const float4 v = *reinterpret_cast<const float4*>(
            src + (size_t)cols[a] * F + c0);
        acc.x += v.x; acc.y += v.y; acc.z += v.z; acc.w += v.w;
    }
    return acc;
}

// ---- host: LDS budget of the LDS-resident kernels ------------------------
// `nbuf` row buffers of rows_pad×STRIDE, K weight matrices, optionally the
// bias row, and — when it still fits — the graph's CSR (Ee+1 row pointers +
// max_nnz columns) so the SpMVs read it from LDS.
struct LdsPlan {
    int rows_pad;        // Ee rounded up to the 16-row MFMA tile
    size_t lds_bytes;    // dynamic LDS to launch with (CSR included if staged)
    int stage_csr;
    bool fits;           // false: the graph needs the row-tiled kernels
};

inline LdsPlan cheb_lds_plan(int Ee, int K, int nbuf, bool with_bias,
                             long max_nnz) {
    LdsPlan p;
    p.rows_pad = (Ee + 15) & ~15;
    p.lds_bytes = sizeof(float) * ((size_t)nbuf * p.rows_pad * STRIDE +
                                   (size_t)K * F * F + (with_bias ? F : 0));
    p.fits = p.lds_bytes <= LDS_LIMIT;
    const size_t csr_bytes = sizeof(int) * ((size_t)Ee + 1 + max_nnz);
    p.stage_csr = (p.lds_bytes + csr_bytes <= LDS_LIMIT) ? 1 : 0;
    if (p.stage_csr) p.lds_bytes += csr_bytes;
    return p;
}

}  // namespace cheb
