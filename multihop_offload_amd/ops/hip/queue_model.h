// The queueing model shared by the critic, the actor head (queueing.hip) and
// walk_eval (episode.hip): the contention fixed point and its reverse, the
// delay units, the per-graph view over the batch tables, and ONE host-side
// LDS plan per kernel — the launcher sizes the launch from it and the kernel
// carves its pointers from the same offsets, so the two cannot disagree.

#pragma once

#include <hip/hip_runtime.h>
#include <torch/extension.h>

#include "gfx950.h"

namespace qm {

// ---- the batch tables every kernel here reads, and one graph's view ------
struct Tables {
    const int* conf_indptr;   // (B,E+1) into conf_cols[conf_base]
    const long* conf_base;    // (B+1)
    const int* conf_cols;     // flat, local link ids
    const float* rates;       // (B,E)
    const float* bw;          // (B,bw_stride) compute bandwidths
    const float* T_arr;       // (B)
    const int* E_arr;         // (B) real link counts (ragged-E batches)
    int E, bw_stride;
};

inline Tables tables(const torch::Tensor& conf_indptr,
                     const torch::Tensor& conf_base,
                     const torch::Tensor& conf_cols,
                     const torch::Tensor& rates, const torch::Tensor& bw,
                     const torch::Tensor& T_arr,
                     const torch::Tensor& E_arr) {
    return {conf_indptr.data_ptr<int>(), conf_base.data_ptr<long>(),
            conf_cols.data_ptr<int>(), rates.data_ptr<float>(),
            bw.data_ptr<float>(), T_arr.data_ptr<float>(),
            E_arr.data_ptr<int>(), (int)rates.size(1), (int)bw.size(1)};
}

struct Graph {
    const int* cip;       // conflict CSR row pointers
    const int* ccols;     // conflict CSR columns
    const float* rates;
    const float* bw;
    float T;
    int Eb;               // real link count: every E-length loop runs to Eb
};

DEV_INLINE Graph graph_view(const Tables& t, int b) {
    return {t.conf_indptr + (size_t)b * (t.E + 1),
            t.conf_cols + t.conf_base[b], t.rates + (size_t)b * t.E,
            t.bw + (size_t)b * t.bw_stride, t.T_arr[b], t.E_arr[b]};
}

// ---- the conflict CSR of one graph, staged in LDS or read in place --------
// A graph's conflict CSR is constant, and the fixed point walks all of it
// once per iteration.  A workgroup whose CSR fits the launch's staging
// budget copies it into LDS once (row pointers, link rates, 16-bit columns)
// and iterates from there; any other workgroup reads it from global memory.
// Both views hand a row out in chunks of CHUNK columns so the gathers of a
// chunk are in flight together; row_sum adds them in CSR order into one
// accumulator, so the two views give bit-equal sums.
constexpr int CHUNK = 8;          // columns per chunk: one 128-bit LDS read
constexpr int STAGE_ALIGN = 16;   // bytes; every staged array starts on it
constexpr int STAGE_MAX_E = 65535;   // columns are staged as 16-bit

__host__ DEV_INLINE size_t stage_align(size_t bytes) {
    return (bytes + STAGE_ALIGN - 1) / STAGE_ALIGN * STAGE_ALIGN;
}
// LDS bytes of a staged CSR of Eb rows and nnz columns: (Eb+1) row
// pointers, Eb rates, nnz 16-bit columns zero-padded to a whole chunk
__host__ DEV_INLINE size_t stage_bytes(long Eb, long nnz) {
    return stage_align(sizeof(int) * (size_t)(Eb + 1))
        + stage_align(sizeof(float) * (size_t)Eb)
        + stage_align(sizeof(unsigned short) * (size_t)nnz);
}

struct GlobalCsr {
    const int* cip;
    const float* rt;
    const int* ccols;
    DEV_INLINE int row(int e) const { return cip[e]; }
    DEV_INLINE float rate(int e) const { return rt[e]; }
    DEV_INLINE int chunk_begin(int lo) const { return lo; }
    // columns c..c+CHUNK-1 of a row ending at hi (c < hi); slots past the
    // row repeat column c
    DEV_INLINE void cols(int c, int hi, int (&col)[CHUNK]) const {
#pragma unroll
        for (int k = 0; k < CHUNK; ++k)
            col[k] = ccols[c + k < hi ? c + k : c];
    }
};

struct StagedCsr {
    const int* rp;                 // LDS
    const float* rt;               // LDS
    const unsigned short* c16;     // LDS, STAGE_ALIGN-aligned, zero-padded
    DEV_INLINE int row(int e) const { return rp[e]; }
    DEV_INLINE float rate(int e) const { return rt[e]; }
    // chunks are aligned in the column array, not in the row: the slots of
    // the first chunk before `lo` belong to the previous row
    DEV_INLINE int chunk_begin(int lo) const { return lo & ~(CHUNK - 1); }
    DEV_INLINE void cols(int c, int /*hi*/, int (&col)[CHUNK]) const {
        const uint4 w = *reinterpret_cast<const uint4*>(c16 + c);
        const unsigned wd[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
        for (int k = 0; k < CHUNK; ++k)
            col[k] = (int)((wd[k >> 1] >> ((k & 1) * 16)) & 0xffffu);
    }
};

// What a kernel knows about its graph's CSR after stage_csr.
struct Csr {
    bool staged;       // block-uniform
    GlobalCsr g;
    StagedCsr s;
};

// Decide and stage.  `stage` is the launch's staging area (after the plan's
// bytes, STAGE_ALIGN-aligned), `budget` its size in bytes (0: none).  Every
// thread of the block calls this; it ends on a barrier when it staged.
DEV_INLINE Csr stage_csr(const int* cip, const float* rates,
                         const int* ccols, int Eb, char* stage, int budget,
                         int tid, int nt) {
    Csr c;
    c.g = {cip, rates, ccols};
    const int nnz = cip[Eb];
    c.staged = budget > 0 && Eb <= STAGE_MAX_E
        && stage_bytes(Eb, nnz) <= (size_t)budget;
    int* rp = reinterpret_cast<int*>(stage);
    float* rt = reinterpret_cast<float*>(
        stage + stage_align(sizeof(int) * (size_t)(Eb + 1)));
    unsigned short* c16 = reinterpret_cast<unsigned short*>(
        reinterpret_cast<char*>(rt) + stage_align(sizeof(float) * (size_t)Eb));
    c.s = {rp, rt, c16};
    if (c.staged) {
        for (int i = tid; i <= Eb; i += nt) rp[i] = cip[i];
        for (int i = tid; i < Eb; i += nt) rt[i] = rates[i];
        const int padded = (nnz + CHUNK - 1) & ~(CHUNK - 1);
#pragma unroll 4
        for (int i = tid; i < padded; i += nt)
            c16[i] = i < nnz ? (unsigned short)ccols[i] : (unsigned short)0;
        __syncthreads();
    }
    return c;
}

// Sum of x[col] over the row [lo, hi) in CSR order, one accumulator from +0.
// The gathers of a chunk are issued together, then added in order.
// Padded: slots outside the row add +0.0f — exact when x >= +0 (busy).
// Otherwise the add is predicated (dnb is signed).
template <bool Padded, class View>
DEV_INLINE float row_sum(const View& cs, const float* x, int lo, int hi) {
    float s = 0.0f;
    for (int c = cs.chunk_begin(lo); c < hi; c += CHUNK) {
        int col[CHUNK];
        cs.cols(c, hi, col);
        float v[CHUNK];
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) v[k] = x[col[k]];
#pragma unroll
        for (int k = 0; k < CHUNK; ++k) {
            const bool in = c + k >= lo && c + k < hi;
            if (Padded) s += in ? v[k] : 0.0f;
            else if (in) s += v[k];
        }
    }
    return s;
}

// forward fixed point storing mu_t for t=0..iters into `hist` ((iters+1)*E)
// Eb: real (per-graph) link count the loops run over; Estride: row stride
// of the mu history (the BATCH-max E — ragged-E / padded batches).
// Estride = 0 keeps no history: every round reads and overwrites row 0
// (read, barrier, write — walk_eval).
template <class View>
DEV_INLINE void fixed_point_fwd_on(const View& cs, const float* lam,
                                   float* hist, float* busy, int Eb,
                                   int Estride, int iters, int tid, int nt) {
    if (Eb <= nt) {
        // at most one row per thread: bounds, rate and lam in registers
        const bool on = tid < Eb;
        int lo = 0, hi = 0;
        float rate = 0.f, lam_e = 0.f;
        if (on) {
            lo = cs.row(tid);
            hi = cs.row(tid + 1);
            rate = cs.rate(tid);
            lam_e = lam[tid];
            hist[tid] = rate / ((float)(hi - lo) + 1.0f);
        }
        __syncthreads();
        for (int t = 1; t <= iters; ++t) {
            const float* mu_prev = hist + (size_t)(t - 1) * Estride;
            float* mu_cur = hist + (size_t)t * Estride;
            if (on) {
                const float r = lam_e / mu_prev[tid];
                busy[tid] = r < 0.f ? 0.f : (r > 1.f ? 1.f : r);
            }
            __syncthreads();
            if (on)
                mu_cur[tid] = rate / (1.0f + row_sum<true>(cs, busy, lo, hi));
            __syncthreads();
        }
        return;
    }
    for (int e = tid; e < Eb; e += nt) {
        const float deg = (float)(cs.row(e + 1) - cs.row(e));
        hist[e] = cs.rate(e) / (deg + 1.0f);
    }
    __syncthreads();
    for (int t = 1; t <= iters; ++t) {
        const float* mu_prev = hist + (size_t)(t - 1) * Estride;
        float* mu_cur = hist + (size_t)t * Estride;
        for (int e = tid; e < Eb; e += nt) {
            const float r = lam[e] / mu_prev[e];
            busy[e] = r < 0.f ? 0.f : (r > 1.f ? 1.f : r);
        }
        __syncthreads();
        for (int e = tid; e < Eb; e += nt) {
            const float nbv =
                row_sum<true>(cs, busy, cs.row(e), cs.row(e + 1));
            mu_cur[e] = cs.rate(e) / (1.0f + nbv);
        }
        __syncthreads();
    }
}

// The two views are two instantiations behind a block-uniform branch, so
// the staged one compiles to LDS reads (a pointer picked at run time
// between LDS and global would make every read a flat one).
DEV_INLINE void fixed_point_fwd(const Csr& c, const float* lam, float* hist,
                                float* busy, int Eb, int Estride, int iters,
                                int tid, int nt) {
    if (c.staged)
        fixed_point_fwd_on(c.s, lam, hist, busy, Eb, Estride, iters, tid, nt);
    else
        fixed_point_fwd_on(c.g, lam, hist, busy, Eb, Estride, iters, tid, nt);
}

// reverse through the unrolled fixed point: consumes dmu (cotangent on
// mu_iters), accumulates into dlam.  Scratch: dnb[E], dbusy[E] (dbusy only
// when a thread owns several rows).  Ends on a barrier behind the last read
// of the scratch.
template <class View>
DEV_INLINE void fixed_point_bwd_on(const View& cs, const float* lam,
                                   const float* hist, float* dmu, float* dnb,
                                   float* dbusy, float* dlam, int Eb,
                                   int Estride, int iters, int tid, int nt) {
    if (Eb <= nt) {
        // at most one row per thread: the row's dmu, dlam and dbusy never
        // leave the thread, only dnb is exchanged
        const bool on = tid < Eb;
        int lo = 0, hi = 0;
        float rate = 1.f, lam_e = 0.f, dmu_e = 0.f, dlam_e = 0.f;
        if (on) {
            lo = cs.row(tid);
            hi = cs.row(tid + 1);
            rate = cs.rate(tid);
            lam_e = lam[tid];
            dmu_e = dmu[tid];
            dlam_e = dlam[tid];
        }
        for (int t = iters; t >= 1; --t) {
            const float* mu_prev = hist + (size_t)(t - 1) * Estride;
            const float* mu_cur = hist + (size_t)t * Estride;
            float mp = 1.f;
            if (on) {
                const float mc = mu_cur[tid];
                mp = mu_prev[tid];
                dnb[tid] = -mc * mc / rate * dmu_e;
            }
            __syncthreads();
            if (on) {
                const float acc = row_sum<false>(cs, dnb, lo, hi);
                const float ratio = lam_e / mp;
                const float pass = (ratio <= 1.0f) ? 1.0f : 0.0f;
                const float g = pass * acc;
                dlam_e += g / mp;
                dmu_e = -g * lam_e / (mp * mp);
            }
            __syncthreads();
        }
        if (on) {
            dmu[tid] = dmu_e;
            dlam[tid] = dlam_e;
        }
        return;
    }
    for (int t = iters; t >= 1; --t) {
        const float* mu_prev = hist + (size_t)(t - 1) * Estride;
        const float* mu_cur = hist + (size_t)t * Estride;
        for (int e = tid; e < Eb; e += nt) {
            // mu_t = rates/(1+nb) => d nb = -mu_t^2/rates * d mu_t
            dnb[e] = -mu_cur[e] * mu_cur[e] / cs.rate(e) * dmu[e];
        }
        __syncthreads();
        for (int e = tid; e < Eb; e += nt) {
            // busy feeds the nb of every conflicting link (A symmetric)
            dbusy[e] = row_sum<false>(cs, dnb, cs.row(e), cs.row(e + 1));
        }
        __syncthreads();
        for (int e = tid; e < Eb; e += nt) {
            const float ratio = lam[e] / mu_prev[e];
            const float pass = (ratio <= 1.0f) ? 1.0f : 0.0f;  // ratio>=0
            const float g = pass * dbusy[e];
            dlam[e] += g / mu_prev[e];
            dmu[e] = -g * lam[e] / (mu_prev[e] * mu_prev[e]);
        }
        __syncthreads();
    }
}

DEV_INLINE void fixed_point_bwd(const Csr& c, const float* lam,
                                const float* hist, float* dmu, float* dnb,
                                float* dbusy, float* dlam, int Eb,
                                int Estride, int iters, int tid, int nt) {
    if (c.staged)
        fixed_point_bwd_on(c.s, lam, hist, dmu, dnb, dbusy, dlam, Eb, Estride,
                           iters, tid, nt);
    else
        fixed_point_bwd_on(c.g, lam, hist, dmu, dnb, dbusy, dlam, Eb, Estride,
                           iters, tid, nt);
}

// unit = 1/(mu-lam), overwritten by T*lam/(denom*mu) where lam-mu > 0.
// cap > 0 clamps the 1/(mu-lam) branch (torch.clamp semantics: value
// capped, gradient zero where inv > cap) — pole mitigation for training.
DEV_INLINE float unit_fwd(float lam, float mu, float T, float denom,
                          float cap) {
    if ((lam - mu) > 0.f) return T * lam / (denom * mu);
    const float inv = 1.0f / (mu - lam);
    return (cap > 0.f && inv > cap) ? cap : inv;
}
// cotangents: given dunit, produce (dlam, dmu) contributions
DEV_INLINE void unit_bwd(float lam, float mu, float T, float denom,
                         float cap, float dunit, float* dlam, float* dmu) {
    if ((lam - mu) > 0.f) {
        *dlam = dunit * T / (denom * mu);
        *dmu = -dunit * T * lam / (denom * mu * mu);
    } else {
        const float inv = 1.0f / (mu - lam);
        if (cap > 0.f && inv > cap) { *dlam = 0.f; *dmu = 0.f; return; }
        *dlam = dunit * inv * inv;
        *dmu = -dunit * inv * inv;
    }
}

// walk_eval's empirical unit of a link (lam, mu) or a server (load, bw).
// Deliberately not unit_fwd: the evaluator tests mu - lam > 0 where unit_fwd
// tests lam - mu > 0 (an exact tie and a NaN take the other branch), its
// fallback denominator is per job (ul + dl on links, ul on the server), and
// it is never clamped.
DEV_INLINE float emp_unit(float lam, float mu, float T, float denom) {
    const float gap = mu - lam;
    return gap > 0.f ? 1.0f / gap : T * lam / (denom * mu);
}

// ---- host: one LDS plan per kernel ---------------------------------------
// A plan lists the kernel's regions once, in carve order, as float offsets
// into dynamic LDS.  `spill` regions move to global scratch (offset GLOBAL)
// when the all-LDS layout is over the limit; the byte total is whatever the
// list adds up to in the mode chosen.
constexpr int GLOBAL = -1;

struct Launch {
    size_t lds_bytes;   // dynamic LDS to launch with
    int threads;
    bool large;         // some region lives in global scratch
    bool fits;          // false: too large even so — do not launch
};

struct Carve {
    bool large;
    size_t floats = 0;
    bool spilled = false;
    int lds(size_t n) {
        const size_t off = floats;
        floats += n;
        return (int)off;
    }
    int spill(size_t n) {
        if (!large) return lds(n);
        spilled = true;
        return GLOBAL;
    }
};

template <class Plan, class Layout>
inline Plan make_plan(int threads, Layout layout) {
    Plan p;
    for (bool large : {false, true}) {
        Carve c{large};
        layout(p, c);
        p.lds_bytes = sizeof(float) * c.floats;
        p.large = c.spilled;
        p.fits = p.lds_bytes <= LDS_LIMIT;
        if (p.fits) break;
    }
    p.threads = threads;
    return p;
}

// large graphs ship few workgroups (one per graph): widen them so the
// E-length loops (and walk_eval's N*N unpack) keep more lanes busy per CU
inline int launch_threads(int E, int N = 0) {
    return (E >= 1500 || N >= 500) ? 1024 : 256;
}

// ---- host: the CSR staging area of a launch ------------------------------
// Not part of the plan: the launcher appends it to the plan's bytes when the
// two still fit, and hands its size to the kernel, where each workgroup
// decides for its own graph (stage_csr).  The default holds the conflict CSR
// of every graph of the 100-node BA training cases (largest: 196 rows, 3238
// columns, 8064 bytes) twice over; measured against 8 and 32 KiB in
// profiles/fixed_point_lds.md.
constexpr int STAGE_BUDGET_DEFAULT = 16 * 1024;
constexpr size_t STATIC_LDS_RESERVE = 64;   // the kernels' few static words

// Plain host variables read by the launchers (set from Python through
// queue_csr_force_global / queue_csr_set_budget); a captured graph keeps
// whatever its launches were given at capture.
inline bool stage_force_global = false;
inline int stage_budget_setting = STAGE_BUDGET_DEFAULT;

inline size_t stage_offset(const Launch& l) {
    return stage_align(l.lds_bytes);
}
// bytes of staging area the launcher adds to this plan's launch (0: none)
inline int stage_budget(const Launch& l) {
    if (stage_force_global || stage_budget_setting <= 0) return 0;
    const size_t total = stage_offset(l) + (size_t)stage_budget_setting
        + STATIC_LDS_RESERVE;
    return total <= LDS_LIMIT ? stage_budget_setting : 0;
}
inline size_t launch_lds_bytes(const Launch& l, int budget) {
    return budget > 0 ? stage_offset(l) + (size_t)budget : l.lds_bytes;
}

// kernel side: base pointer of a region, wherever the plan put it
template <class T>
DEV_INLINE T* region(float* lds, int off, T* global) {
    return off == GLOBAL ? global : lds + off;
}

struct CriticPlan : Launch {
    int lam_e, unit, dunit, dlam, dgre, hist, s1, s2, s3;
};
inline CriticPlan critic_plan(int E, int Ee, int iters) {
    return make_plan<CriticPlan>(
        launch_threads(E), [=](CriticPlan& p, Carve& c) {
            p.lam_e = c.lds(Ee);
            p.unit = c.lds(Ee);
            p.dunit = c.spill(Ee);
            p.dlam = c.spill(Ee);
            p.dgre = c.spill(Ee);      // large: grad_edge accumulates directly
            p.hist = c.spill((size_t)(iters + 1) * E);
            p.s1 = c.lds(E);
            p.s2 = c.lds(E);
            p.s3 = c.lds(E);
        });
}

struct ActorFwdPlan : Launch { int lam, hist, busy; };
inline ActorFwdPlan actor_fwd_plan(int E, int iters) {
    return make_plan<ActorFwdPlan>(
        launch_threads(E), [=](ActorFwdPlan& p, Carve& c) {
            p.lam = c.lds(E);
            p.hist = c.spill((size_t)(iters + 1) * E);   // large: mu_hist_out
            p.busy = c.lds(E);
        });
}

struct ActorBwdPlan : Launch { int lam, hist, dmu, dlam, s1, s2; };
inline ActorBwdPlan actor_bwd_plan(int E, int iters) {
    return make_plan<ActorBwdPlan>(
        launch_threads(E), [=](ActorBwdPlan& p, Carve& c) {
            p.lam = c.lds(E);
            p.hist = c.spill((size_t)(iters + 1) * E);   // large: mu_hist
            p.dmu = c.lds(E);
            p.dlam = c.lds(E);
            p.s1 = c.lds(E);
            p.s2 = c.lds(E);
        });
}

struct WalkPlan : Launch { int lam, mu, busy, sload; };
inline WalkPlan walk_plan(int N, int E) {
    return make_plan<WalkPlan>(
        launch_threads(E, N), [=](WalkPlan& p, Carve& c) {
            p.lam = c.lds(E);
            p.mu = c.lds(E);
            p.busy = c.lds(E);
            p.sload = c.lds(N);
        });
}

// timeslot_sim (timeslot.hip): 32-bit words, all in LDS — queue heads and
// tails, the finished chains (head, first target, length) and the
// per-resource job chains over the R = E + N resources, one bit per
// resource, the busy flags, five per-job rows and four scalars.  The task
// pool is global.  4 * (6 R + ceil(R / 32) + E + 5 J + 4) bytes.
struct TimeslotPlan : Launch {
    int head, tail, fhead, ftgt0, fcnt, jfirst, fmask, busy, arr, jres,
        jnext, jnh, jdst, misc;
};
inline void timeslot_regions(TimeslotPlan& p, Carve& c, int N, int E,
                             int J) {
    const size_t R = (size_t)E + N;
    p.head = c.lds(R);
    p.tail = c.lds(R);
    p.fhead = c.lds(R);
    p.ftgt0 = c.lds(R);
    p.fcnt = c.lds(R);
    p.jfirst = c.lds(R);
    p.fmask = c.lds((R + 31) / 32);
    p.busy = c.lds(E);
    p.arr = c.lds(J);
    p.jres = c.lds(J);
    p.jnext = c.lds(J);
    p.jnh = c.lds(J);
    p.jdst = c.lds(J);
    p.misc = c.lds(4);
}
inline TimeslotPlan timeslot_plan(int N, int E, int J) {
    return make_plan<TimeslotPlan>(
        launch_threads(E, N), [=](TimeslotPlan& p, Carve& c) {
            timeslot_regions(p, c, N, E, J);
        });
}

// The statistics launch of timeslot_sim: the base regions in the same order,
// then the live queue length, the sampled maximum and the busy-slot count
// (one word per resource), one pad word where the count so far is odd, and
// the two 64-bit sums (queue length per resource, nb per link).  With W the
// base plan's words: 4 * (W + 3 R + (W + 3 R) % 2 + 2 R + 2 E) bytes.
struct TimeslotStatsPlan : TimeslotPlan {
    int qlen, qmax, bslots, qsum, nbsum;
};
inline void timeslot_stats_regions(TimeslotStatsPlan& p, Carve& c, int N,
                                   int E, int J) {
    const size_t R = (size_t)E + N;
    timeslot_regions(p, c, N, E, J);
    p.qlen = c.lds(R);
    p.qmax = c.lds(R);
    p.bslots = c.lds(R);
    c.lds(c.floats & 1);                    // the 64-bit rows start even
    p.qsum = c.lds(2 * R);
    p.nbsum = c.lds(2 * (size_t)E);
}
inline TimeslotStatsPlan timeslot_stats_plan(int N, int E, int J) {
    return make_plan<TimeslotStatsPlan>(
        launch_threads(E, N), [=](TimeslotStatsPlan& p, Carve& c) {
            timeslot_stats_regions(p, c, N, E, J);
        });
}

// The scheduled-MAC launches (timeslot_sim_mwis, timeslot_sim_mwis_stats):
// the regions of the plan above them in the same order, then the schedule's
// own: the live queue length per resource where the plan has none yet, the
// schedule state, the round's verdict and the scheduled-slot count (one word
// per link), one pad word where the count so far is odd, and the 64-bit
// weights.  With W the base plan's words and S the statistics plan's:
//   4 * (W + R + 3 E + (W + R + 3 E) % 2 + 2 E) bytes, and
//   4 * (S + 3 E + (S + 3 E) % 2 + 2 E) bytes with the statistics.
struct MwisRegions { int sstate, swin, sslots, swt; };
inline void timeslot_mwis_regions(MwisRegions& m, Carve& c, int E) {
    m.sstate = c.lds(E);
    m.swin = c.lds(E);
    m.sslots = c.lds(E);
    c.lds(c.floats & 1);                    // the 64-bit row starts even
    m.swt = c.lds(2 * (size_t)E);
}
struct TimeslotMwisPlan : TimeslotPlan {
    int qlen;
    MwisRegions mw;
};
inline TimeslotMwisPlan timeslot_mwis_plan(int N, int E, int J) {
    return make_plan<TimeslotMwisPlan>(
        launch_threads(E, N), [=](TimeslotMwisPlan& p, Carve& c) {
            timeslot_regions(p, c, N, E, J);
            p.qlen = c.lds((size_t)E + N);
            timeslot_mwis_regions(p.mw, c, E);
        });
}
struct TimeslotMwisStatsPlan : TimeslotStatsPlan {
    MwisRegions mw;
};
inline TimeslotMwisStatsPlan timeslot_mwis_stats_plan(int N, int E, int J) {
    return make_plan<TimeslotMwisStatsPlan>(
        launch_threads(E, N), [=](TimeslotMwisStatsPlan& p, Carve& c) {
            timeslot_stats_regions(p, c, N, E, J);
            timeslot_mwis_regions(p.mw, c, E);
        });
}

}  // namespace qm
