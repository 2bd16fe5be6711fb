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

// forward fixed point storing mu_t for t=0..iters into `hist` ((iters+1)*E)
// Eb: real (per-graph) link count the loops run over; Estride: row stride
// of the mu history (the BATCH-max E — ragged-E / padded batches).
// Estride = 0 keeps no history: every round reads and overwrites row 0
// (read, barrier, write — walk_eval).
DEV_INLINE void fixed_point_fwd(const float* lam, const float* rates,
                                const int* cip, const int* ccols,
                                float* hist, float* busy, int Eb,
                                int Estride, int iters, int tid, int nt) {
    for (int e = tid; e < Eb; e += nt) {
        const float deg = (float)(cip[e + 1] - cip[e]);
        hist[e] = rates[e] / (deg + 1.0f);
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
            float nbv = 0.0f;
            for (int a = cip[e]; a < cip[e + 1]; ++a) nbv += busy[ccols[a]];
            mu_cur[e] = rates[e] / (1.0f + nbv);
        }
        __syncthreads();
    }
}

// reverse through the unrolled fixed point: consumes dmu (cotangent on
// mu_iters), accumulates into dlam.  Scratch: dnb[E], dbusy[E].
DEV_INLINE void fixed_point_bwd(const float* lam, const float* rates,
                                const int* cip, const int* ccols,
                                const float* hist, float* dmu, float* dnb,
                                float* dbusy, float* dlam, int Eb,
                                int Estride, int iters, int tid, int nt) {
    for (int t = iters; t >= 1; --t) {
        const float* mu_prev = hist + (size_t)(t - 1) * Estride;
        const float* mu_cur = hist + (size_t)t * Estride;
        for (int e = tid; e < Eb; e += nt) {
            // mu_t = rates/(1+nb) => d nb = -mu_t^2/rates * d mu_t
            dnb[e] = -mu_cur[e] * mu_cur[e] / rates[e] * dmu[e];
        }
        __syncthreads();
        for (int e = tid; e < Eb; e += nt) {
            // busy feeds the nb of every conflicting link (A symmetric)
            float acc = 0.0f;
            for (int a = cip[e]; a < cip[e + 1]; ++a) acc += dnb[ccols[a]];
            dbusy[e] = acc;
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
inline TimeslotPlan timeslot_plan(int N, int E, int J) {
    return make_plan<TimeslotPlan>(
        launch_threads(E, N), [=](TimeslotPlan& p, Carve& c) {
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
        });
}

}  // namespace qm
