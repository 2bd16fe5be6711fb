// Per-slot phases of the per-timeslot packet simulator (timeslot.hip), written
// against one graph's state so that the same text runs as a workgroup on the
// GPU and as plain C++ on the host (tests/host/timeslot_host.cpp calls every
// phase for tid = 0..nt-1, one phase after the other).
//
// The contract is sim/timeslot.py::simulate_routes, integer for integer.
// Resources are the Eb real links, then the N nodes; each owns a FIFO of
// tasks threaded through `next` in the task pool.  Nothing here contains a
// barrier: the caller separates the phases.  Order never depends on timing —
// every queue is appended to by exactly one thread per phase (its owner,
// r % nt == tid), and that thread walks its sources in the oracle's order.
//
//   init_jobs   | init_queues | then per slot t:
//   arrive(t)   : owner of r appends slot t's new tasks bound for r (j
//                 ascending), then snapshots busy[r]
//   serve(t)    : owner of r drains its FIFO against the slot's capacity and
//                 chains what it popped through `fnext` (pop order)
//   handover(t) : owner of r walks the source resources that finished
//                 something (a bit set, ascending) and appends the finished
//                 tasks whose next leg is r; thread 0 writes the
//                 trace row; slot t+1's arrival counts are staged
//
// Statistics mode: every phase is a template on `Stats`, false by default, so
// the plain names are the statistics-free simulator, unchanged.  With Stats
// the owner of r also keeps qlen[r], samples it after the arrivals of every
// slot t >= warmup (qsum / qmax / bslots, and nbsum in serve), the owner of a
// job's last leg adds the sojourn to the job's max / late / histogram, and
// two phases follow the last slot: tally_backlog and store_resource_stats.
// All of it is integers, each word with one writer or an integer sum.
//
// Scheduled MAC: a second template parameter `Mwis`, false by default, swaps
// the link capacity rate / (1 + nb) for the slot's schedule
// (sim/timeslot.py::mwis_schedule): the owner of r keeps qlen[r] (as with
// Stats), and between arrive and serve the caller runs
//   sched_init        : weight qlen * rate (one fp64 multiply) and the
//                       candidate flag of every link
//   then per round, while sched_init / sched_round_commit report a candidate:
//   sched_round_pick  : the owner of a candidate scans its conflict row and
//                       writes its own verdict (won / lost)
//   sched_round_commit: a winner marks itself scheduled and its neighbours
//                       out — the one shared write, every writer storing the
//                       same value
// serve<Stats, true> gives a scheduled link its full rate and any other link
// nothing, and counts the scheduled slots t >= warmup; store_sched_slots
// follows the last slot.  These phases read the conflict columns through
// conf_col: the 16-bit copy that stage_cols made at init, where the caller
// had room for one, and ccols in place otherwise.
//
// Guard rails: every index read from memory is range-checked before use and
// every loop has a bound derived from the pool capacity P; a violation sets
// st.misc[ERR] and the caller stops stepping that graph.

#pragma once

#include <cstdint>

#ifndef DEV_INLINE
#define DEV_INLINE inline
#endif

#if defined(__HIP_DEVICE_COMPILE__)
#define TSIM_COUNT_ADD(p, v) atomicAdd((p), (v))   // integer count only
#define TSIM_COUNT_ADD64(p, v) \
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)(v))
#define TSIM_SET_BITS(p, v) atomicOr((p), (v))     // a set: no order in it
#else
#define TSIM_COUNT_ADD(p, v) (*(p) += (v))
#define TSIM_COUNT_ADD64(p, v) (*(p) += (v))
#define TSIM_SET_BITS(p, v) (*(p) |= (v))
#endif

namespace tsim {

enum { ERR = 0, DEP = 1, INNET = 2, MISC_WORDS = 4 };
enum {  // error bits
    E_INPUT = 1,    // route / nhop / dst out of range
    E_POOL = 2,     // task index or pool offset out of range
    E_BOUND = 4,    // a loop ran past its iteration bound
    E_TARGET = 8    // a task's next resource out of range
};

struct Case {                       // one graph, read-only
    int Eb, n, N, J, H, T, warmup, P;
    const int* cip;                 // (Eb+1) conflict CSR row pointers
    const int* ccols;               // conflict CSR columns
    const float* rates;             // (Eb) link rates
    const float* bw;                // (N) node bandwidths
    const unsigned char* arrivals;  // (T,J)
    const int* slot_off;            // (T+1) exclusive prefix of slot totals
    const int* route_links;         // (J,H), -1 padded
    const int* nhop;                // (J)
    const int64_t* dst;             // (J)
    const bool* mask;               // (J)
    const float* ul;                // (J)
    const float* dl;                // (J)
    // statistics mode only
    int late_after = 0;             // sojourns above it count as late
    int nbins = 0;                  // delay_bin(T) + 1 histogram bins
    int node_col = 0;               // output column of node 0 (batch max E)
    // scheduled MAC only: ccols as 16-bit words (LDS on the GPU, filled by
    // stage_cols), or null: read ccols in place
    const unsigned short* ccols16 = nullptr;
};

struct State {                      // one graph, mutable
    // task pool (global memory), P entries each
    int* job;
    int* stage;
    int* t0;
    int* next;                      // FIFO link
    int* fnext;                     // finished-this-slot chain (pop order)
    int* tgt;                       // next leg's resource
    double* rem;
    // per-resource / per-job words (LDS on the GPU)
    int* head;                      // (R)
    int* tail;                      // (R)
    int* fhead;                     // (R)
    int* ftgt0;                     // (R) next resource of fhead[r]
    int* fcnt;                      // (R) length of r's finished chain
    unsigned* fmask;                // (ceil(R/32)) bit r: fhead[r] non-empty
    int* busy;                      // (Eb)
    int* arr;                       // (J) staged arrival counts of the slot
    int* jres;                      // (J) first leg's resource; -1 masked, -2 bad
    int* jfirst;                    // (R) first job whose first leg is r
    int* jnext;                     // (J) next job with the same first leg
    int* jnh;                       // (J) validated nhop (0 where masked)
    int* jdst;                      // (J) validated dst
    int* misc;                      // (MISC_WORDS)
    // outputs
    long long* delay_sum;           // (J)
    int* count;                     // (J)
    int* trace;                     // (T,3) or null
    // statistics mode only: live length and accumulators (LDS on the GPU),
    // indexed by resource id
    int* qlen = nullptr;            // (R) tasks in r's FIFO
    long long* qsum = nullptr;      // (R) sum of qlen over the sampled slots
    int* qmax = nullptr;            // (R) largest sampled qlen
    int* bslots = nullptr;          // (R) sampled slots with qlen > 0
    long long* nbsum = nullptr;     // (Eb) sum of nb over sampled busy slots
    // statistics outputs, zeroed by the caller
    int* delay_max = nullptr;       // (J)
    int* late = nullptr;            // (J)
    int* delay_hist = nullptr;      // (J, nbins)
    int* stuck = nullptr;           // (J)
    long long* stuck_age = nullptr; // (J)
    long long* qlen_sum = nullptr;  // (node_col + N), as the three below
    int* qlen_max = nullptr;
    int* busy_slots = nullptr;
    long long* nb_sum = nullptr;
    // scheduled MAC only (LDS on the GPU); qlen above is live here too
    double* swt = nullptr;          // (Eb) the slot's weights
    int* sstate = nullptr;          // (Eb) S_OUT / S_CAND / S_ON
    int* swin = nullptr;            // (Eb) the round's verdict, W_*
    int* sslots = nullptr;          // (Eb) scheduled slots t >= warmup
    int* sched_slots = nullptr;     // output, zeroed by the caller
};

enum { S_OUT = 0, S_CAND = 1, S_ON = 2 };       // a link in the slot's schedule
enum { W_NONE = 0, W_WON = 1, W_LOST = 2 };     // a candidate's round

DEV_INLINE int num_res(const Case& c) { return c.Eb + c.N; }

// conflict column a of the graph: the scheduled MAC walks the rows several
// times a slot and reads the staged copy where there is one
template <bool Mwis>
DEV_INLINE int conf_col(const Case& c, int a) {
    if constexpr (Mwis)
        if (c.ccols16) return (int)c.ccols16[a];
    return c.ccols[a];
}
DEV_INLINE int mask_words(int R) { return (R + 31) / 32; }

// Histogram bin of a sojourn d >= 0: exact below 16, then eight sub-bins per
// octave (sim/timeslot.py::delay_bin is the same function).
DEV_INLINE int delay_bin(int d) {
    if (d < 16) return d < 0 ? 0 : d;
    int e = 4;
    while ((d >> (e + 1)) != 0) ++e;            // e = floor(log2 d)
    return 16 + 8 * (e - 4) + ((d >> (e - 3)) & 7);
}

// resource of leg `stage` of job j; -1 once the task has no legs left
DEV_INLINE int leg_res(const Case& c, const State& st, int j, int stage) {
    const int nh = st.jnh[j];
    if (stage < nh) return c.route_links[(size_t)j * c.H + stage];
    if (stage == nh) return c.Eb + st.jdst[j];
    if (stage <= 2 * nh) return c.route_links[(size_t)j * c.H + 2 * nh - stage];
    return -1;
}

DEV_INLINE double leg_units(const Case& c, const State& st, int j,
                            int stage) {
    return stage <= st.jnh[j] ? (double)c.ul[j] : (double)c.dl[j];
}

DEV_INLINE void stage_arrivals(const Case& c, State& st, int t, int tid,
                               int nt) {
    for (int j = tid; j < c.J; j += nt)
        st.arr[j] = st.jres[j] >= 0
            ? (int)c.arrivals[(size_t)t * c.J + j] : 0;
}

DEV_INLINE void append(State& st, int r, int q) {
    st.next[q] = -1;
    const int tl = st.tail[r];
    if (tl >= 0) st.next[tl] = q; else st.head[r] = q;
    st.tail[r] = q;
}

// ---- init, part 1: validate the jobs, first-leg table, zero the outputs --
DEV_INLINE void init_jobs(const Case& c, State& st, int tid, int nt) {
    if (tid == 0) {
        int bad = 0;
        if (c.Eb < 0 || c.n < 0 || c.n > c.N || c.P < 0 ||
            c.slot_off[0] != 0 || c.slot_off[c.T] > c.P)
            bad = E_INPUT;
        st.misc[ERR] = bad;
        st.misc[DEP] = 0;
        st.misc[INNET] = 0;
    }
    for (int j = tid; j < c.J; j += nt) {
        st.delay_sum[j] = 0;
        st.count[j] = 0;
        int res = -1;
        st.jnh[j] = 0;
        st.jdst[j] = 0;
        if (c.mask[j]) {
            const int nh = c.nhop[j];
            const long long d = c.dst[j];
            bool ok = nh >= 0 && nh <= c.H && d >= 0 && d < c.n;
            for (int h = 0; ok && h < nh; ++h) {
                const int l = c.route_links[(size_t)j * c.H + h];
                ok = l >= 0 && l < c.Eb;
            }
            if (ok) {
                st.jnh[j] = nh;
                st.jdst[j] = (int)d;
            }
            res = ok ? leg_res(c, st, j, 0) : -2;  // -2: reported in part 2
        }
        st.jres[j] = res;
    }
}

// ---- init, part 2: empty queues, per-resource job chains, slot 0 staged --
template <bool Stats = false, bool Mwis = false>
DEV_INLINE void init_queues(const Case& c, State& st, int tid, int nt) {
    const int R = num_res(c);
    for (int r = tid; r < R; r += nt) {
        st.head[r] = st.tail[r] = st.fhead[r] = st.ftgt0[r] = -1;
        st.fcnt[r] = 0;
        if (r < c.Eb) st.busy[r] = 0;
        if constexpr (Stats) {
            st.qlen[r] = st.qmax[r] = st.bslots[r] = 0;
            st.qsum[r] = 0;
            if (r < c.Eb) st.nbsum[r] = 0;
        }
        if constexpr (Mwis) {
            st.qlen[r] = 0;
            if (r < c.Eb) {
                st.swt[r] = 0.0;
                st.sstate[r] = S_OUT;
                st.swin[r] = W_NONE;
                st.sslots[r] = 0;
            }
        }
        int first = -1;
        for (int j = c.J - 1; j >= 0; --j)
            if (st.jres[j] == r) { st.jnext[j] = first; first = j; }
        st.jfirst[r] = first;
    }
    for (int j = tid; j < c.J; j += nt)
        if (st.jres[j] == -2) st.misc[ERR] = E_INPUT;
    if (c.T > 0) stage_arrivals(c, st, 0, tid, nt);
}

// ---- scheduled MAC, init: the conflict columns staged as 16-bit words ------
// `c16` holds cip[Eb] words and is what c.ccols16 points to; the caller has
// checked Eb <= 65535.  A column that the narrowing would alias onto a valid
// link is reported here, since the range checks of the phases can no longer
// see it.  Runs with init_queues (after init_jobs has written misc[ERR]).
DEV_INLINE void stage_cols(const Case& c, State& st, unsigned short* c16,
                           int tid, int nt) {
    const int nnz = c.cip[c.Eb];
    for (int a = tid; a < nnz; a += nt) {
        const int o = c.ccols[a];
        if (o < 0 || o >= c.Eb) st.misc[ERR] = E_INPUT;
        c16[a] = (unsigned short)o;
    }
}

// ---- arrivals of slot t, then the busy snapshot ---------------------------
template <bool Stats = false, bool Mwis = false>
DEV_INLINE void arrive(const Case& c, State& st, int t, int tid, int nt) {
    const int R = num_res(c);
    for (int w = tid; w < mask_words(R); w += nt) st.fmask[w] = 0u;
    for (int r = tid; r < R; r += nt) {
        int it = 0;
        [[maybe_unused]] int added = 0;
        for (int j = st.jfirst[r]; j >= 0; j = st.jnext[j]) {
            if (j >= c.J || ++it > c.J) { st.misc[ERR] = E_BOUND; break; }
            const int k = st.arr[j];
            if (k <= 0) continue;
            int off = c.slot_off[t];
            for (int i = 0; i < j; ++i) off += st.arr[i];
            if (off < 0 || off + k > c.P) { st.misc[ERR] = E_POOL; break; }
            const double units = leg_units(c, st, j, 0);
            for (int i = 0; i < k; ++i) {
                const int q = off + i;
                st.job[q] = j;
                st.stage[q] = 0;
                st.t0[q] = t;
                st.rem[q] = units;
                append(st, r, q);
            }
            if constexpr (Stats || Mwis) added += k;
        }
        if (r < c.Eb) st.busy[r] = st.head[r] >= 0;
        if constexpr (Stats || Mwis) {
            [[maybe_unused]] const int len = st.qlen[r] + added;
            if (added) st.qlen[r] = len;
            if constexpr (Stats) {      // the sample: arrivals in, none served
                if (t >= c.warmup && len > 0) {
                    st.qsum[r] += len;
                    if (len > st.qmax[r]) st.qmax[r] = len;
                    st.bslots[r] += 1;
                }
            }
        }
    }
}

// ---- scheduled MAC: the slot's weights and candidates ----------------------
// After arrive: qlen is the FIFO length the oracle weighs, and every word
// here belongs to the thread that wrote it there.  Returns whether this
// thread owns a candidate: the first round's go-ahead.
DEV_INLINE bool sched_init(const Case& c, State& st, int tid, int nt) {
    bool any = false;
    for (int l = tid; l < c.Eb; l += nt) {
        const double w = (double)st.qlen[l] * (double)c.rates[l];
        st.swt[l] = w;
        st.sstate[l] = w > 0.0 ? S_CAND : S_OUT;
        st.swin[l] = W_NONE;
        any = any || w > 0.0;
    }
    return any;
}

// One round, part 1: a candidate wins when (w, -id) beats every candidate of
// its conflict row.  Only swin[l] is written, by l's owner.
DEV_INLINE void sched_round_pick(const Case& c, State& st, int tid, int nt) {
    for (int l = tid; l < c.Eb; l += nt) {
        int verdict = W_NONE;
        if (st.sstate[l] == S_CAND) {
            const double w = st.swt[l];
            verdict = W_WON;
            for (int a = c.cip[l]; a < c.cip[l + 1]; ++a) {
                const int o = conf_col<true>(c, a);
                if (o < 0 || o >= c.Eb) { st.misc[ERR] = E_INPUT; break; }
                if (st.sstate[o] != S_CAND) continue;
                const double wo = st.swt[o];
                if (!(w > wo || (w == wo && l < o))) {
                    verdict = W_LOST;
                    break;
                }
            }
        }
        st.swin[l] = verdict;
    }
}

// One round, part 2: winners join the schedule and put their neighbours out.
// Two winners may both store S_OUT to a shared neighbour; a neighbour that
// won itself (possible only with asymmetric rows) keeps its own S_ON.
// Returns whether a candidate of this thread lost the round: the caller goes
// on while any thread says so.  That is read off the verdicts alone, so a
// loser that a winner has just put out still asks for one more round, which
// then finds no candidate.
DEV_INLINE bool sched_round_commit(const Case& c, State& st, int tid,
                                   int nt) {
    bool left = false;
    for (int l = tid; l < c.Eb; l += nt) {
        const int verdict = st.swin[l];
        left = left || verdict == W_LOST;
        if (verdict != W_WON) continue;
        st.sstate[l] = S_ON;
        for (int a = c.cip[l]; a < c.cip[l + 1]; ++a) {
            const int o = conf_col<true>(c, a);
            if (o < 0 || o >= c.Eb) { st.misc[ERR] = E_INPUT; break; }
            if (st.swin[o] != W_WON) st.sstate[o] = S_OUT;
        }
    }
    return left;
}

// ---- service: every resource drains its own FIFO --------------------------
template <bool Stats = false, bool Mwis = false>
DEV_INLINE void serve(const Case& c, State& st, int t, int tid, int nt) {
    const int R = num_res(c);
    for (int r = tid; r < R; r += nt) {
        int fh = -1, ft = -1, ftg = -1, nf = 0;
        [[maybe_unused]] int popped = 0;
        int q = st.head[r];
        if (q >= 0) {
            double cap;
            if (r < c.Eb) {
                int nb = 0;
                if constexpr (Stats || !Mwis) {
                    for (int a = c.cip[r]; a < c.cip[r + 1]; ++a) {
                        const int o = conf_col<Mwis>(c, a);
                        if (o < 0 || o >= c.Eb) {
                            st.misc[ERR] = E_INPUT;
                            break;
                        }
                        nb += st.busy[o];
                    }
                }
                if constexpr (Stats)
                    if (t >= c.warmup) st.nbsum[r] += nb;
                if constexpr (Mwis) {       // the schedule: all or nothing
                    const bool on = st.sstate[r] == S_ON;
                    if (on && t >= c.warmup) st.sslots[r] += 1;
                    cap = on ? (double)c.rates[r] : 0.0;
                } else {
                    cap = (double)c.rates[r] / (1.0 + (double)nb);
                }
            } else {
                cap = (double)c.bw[r - c.Eb];
            }
            int it = 0;
            while (cap > 0.0 && q >= 0) {
                if (q >= c.P) { st.misc[ERR] = E_POOL; break; }
                if (++it > c.P) { st.misc[ERR] = E_BOUND; break; }
                double rem = st.rem[q];
                const double served = rem < cap ? rem : cap;
                rem -= served;
                cap -= served;
                if (!(rem <= 1e-12)) { st.rem[q] = rem; break; }
                const int nq = st.next[q];
                const int j = st.job[q];
                if (j < 0 || j >= c.J) { st.misc[ERR] = E_POOL; break; }
                const int stage = st.stage[q] + 1;
                st.stage[q] = stage;
                if constexpr (Stats || Mwis) ++popped;
                const int nr = leg_res(c, st, j, stage);
                if (nr < 0) {                       // no legs left
                    const int t0 = st.t0[q];
                    if (t0 >= c.warmup) {
                        st.delay_sum[j] += (long long)(t + 1 - t0);
                        st.count[j] += 1;
                        if constexpr (Stats) {
                            const int d = t + 1 - t0;
                            const int k = delay_bin(d);
                            if (d < 0 || k >= c.nbins) {
                                st.misc[ERR] = E_POOL;
                                break;
                            }
                            if (d > st.delay_max[j]) st.delay_max[j] = d;
                            if (d > c.late_after) st.late[j] += 1;
                            st.delay_hist[(size_t)j * c.nbins + k] += 1;
                        }
                    }
                    TSIM_COUNT_ADD(&st.misc[DEP], 1);
                } else if (nr >= R) {
                    st.misc[ERR] = E_TARGET;
                    break;
                } else {
                    st.tgt[q] = nr;
                    st.rem[q] = leg_units(c, st, j, stage);
                    st.fnext[q] = -1;
                    if (ft >= 0) st.fnext[ft] = q; else { fh = q; ftg = nr; }
                    ft = q;
                    ++nf;
                }
                q = nq;
            }
            st.head[r] = q;
            if (q < 0) st.tail[r] = -1;
            if constexpr (Stats || Mwis)
                if (popped) st.qlen[r] -= popped;
        }
        st.fhead[r] = fh;
        st.ftgt0[r] = ftg;
        st.fcnt[r] = nf;
        if (fh >= 0) TSIM_SET_BITS(&st.fmask[r >> 5], 1u << (r & 31));
    }
}

// ---- hand-over: finished tasks join their next queue, oracle order --------
template <bool Stats = false, bool Mwis = false>
DEV_INLINE void handover(const Case& c, State& st, int t, int tid, int nt) {
    const int R = num_res(c);
    for (int r = tid; r < R; r += nt) {
        int it = 0;
        [[maybe_unused]] int added = 0;
        bool stop = false;
        // sources with something to hand over, ascending: the set bits
        for (int w = 0; w < mask_words(R) && !stop; ++w) {
            for (unsigned m = st.fmask[w]; m && !stop; m &= m - 1) {
                const int s = w * 32 + __builtin_ctz(m);
                if (s >= R) { st.misc[ERR] = E_BOUND; stop = true; break; }
                // the chain's first task and its target are in LDS (most
                // chains hold one task); the rest follow through the pool
                const int n = st.fcnt[s];
                int q = st.fhead[s], tg = st.ftgt0[s];
                for (int i = 0; i < n; ++i) {
                    if (q < 0 || q >= c.P) {
                        st.misc[ERR] = E_POOL; stop = true; break;
                    }
                    if (++it > c.P) {
                        st.misc[ERR] = E_BOUND; stop = true; break;
                    }
                    if (tg == r) {
                        append(st, r, q);
                        if constexpr (Stats || Mwis) ++added;
                    }
                    if (i + 1 < n) {
                        q = st.fnext[q];
                        if (q < 0 || q >= c.P) {
                            st.misc[ERR] = E_POOL; stop = true; break;
                        }
                        tg = st.tgt[q];
                    }
                }
            }
        }
        if constexpr (Stats || Mwis)
            if (added) st.qlen[r] += added;
    }
    if (tid == 0) {
        const int arrived = c.slot_off[t + 1] - c.slot_off[t];
        const int dep = st.misc[DEP];
        st.misc[DEP] = 0;
        st.misc[INNET] += arrived - dep;
        if (st.trace) {
            const int td = t + 1 < c.T ? t + 1 : c.T - 1;
            st.trace[(size_t)t * 3 + 0] = arrived;
            st.trace[(size_t)td * 3 + 1] += dep;
            st.trace[(size_t)t * 3 + 2] = st.misc[INNET];
        }
    }
    if (t + 1 < c.T) stage_arrivals(c, st, t + 1, tid, nt);
}

// ---- statistics, after the last slot: the tasks still in the network ------
// Threads stride over the pool; a task is unfinished iff it has a leg left.
// Integer sums commute, so the adds may land in any order.
DEV_INLINE void tally_backlog(const Case& c, State& st, int tid, int nt) {
    const int used = c.slot_off[c.T];
    if (used < 0 || used > c.P) {
        if (tid == 0) st.misc[ERR] = E_POOL;
        return;
    }
    for (int q = tid; q < used; q += nt) {
        const int j = st.job[q];
        const int stage = st.stage[q];
        const int t0 = st.t0[q];
        if (j < 0 || j >= c.J || stage < 0 || t0 < 0 || t0 >= c.T) {
            st.misc[ERR] = E_POOL;
            break;
        }
        if (t0 < c.warmup || leg_res(c, st, j, stage) < 0) continue;
        TSIM_COUNT_ADD(&st.stuck[j], 1);
        TSIM_COUNT_ADD64(&st.stuck_age[j], (long long)(c.T - t0));
    }
}

// ---- statistics: the per-resource accumulators leave for their columns ----
// Link l goes to column l, node v to column node_col + v: the outputs are
// laid out by the batch's largest link count, not by this graph's Eb.
DEV_INLINE void store_resource_stats(const Case& c, State& st, int tid,
                                     int nt) {
    const int R = num_res(c);
    for (int r = tid; r < R; r += nt) {
        const int col = r < c.Eb ? r : c.node_col + (r - c.Eb);
        st.qlen_sum[col] = st.qsum[r];
        st.qlen_max[col] = st.qmax[r];
        st.busy_slots[col] = st.bslots[r];
        if (r < c.Eb) st.nb_sum[col] = st.nbsum[r];
    }
}

// ---- scheduled MAC: the scheduled-slot counts leave for their columns ------
DEV_INLINE void store_sched_slots(const Case& c, State& st, int tid, int nt) {
    for (int l = tid; l < c.Eb; l += nt) st.sched_slots[l] = st.sslots[l];
}

}  // namespace tsim
