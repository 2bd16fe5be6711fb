// timeslot_sim: the per-timeslot packet simulator of sim/timeslot.py, batched.
// grid.x = B, one workgroup per graph; queue heads/tails, busy flags and the
// per-job rows live in LDS (qm::timeslot_plan), the task pool in global
// memory.  The per-slot phases are tsim:: functions (timeslot_phases.h, also
// compiled as plain C++ by tests/host/timeslot_host.cpp); this file only
// carves the state, separates the phases with barriers and launches.
//
// Exactness: remaining work, capacity and the 1e-12 test are fp64 in the
// oracle's operation order (IEEE divide and subtract; this build has no
// fast-math, and the phases contain no a*b+c for the compiler to contract),
// so delay_sum / count / trace equal simulate_routes integer for integer on
// the fp32-rounded inputs.
//
// Statistics mode (timeslot_sim_stats) is the same kernel text instantiated
// with Stats = true: its own LDS plan (qm::timeslot_stats_plan) adds the live
// queue lengths and the per-resource accumulators, the per-job delay figures
// go to global memory beside delay_sum / count, and two more phases run after
// the last slot.  Stats = false compiles to the statistics-free kernel.
//
// Scheduled MAC (timeslot_sim_mwis, timeslot_sim_mwis_stats) is the same text
// again with Mwis = true: between the arrivals and the service of a slot the
// workgroup runs the rounds of sim/timeslot.py::mwis_schedule over the
// conflict rows (two barriers a round), and a scheduled link serves at its
// full rate.  The weights are one fp64 multiply of an exactly converted queue
// length and the widened fp32 rate, so every comparison agrees with the
// oracle bit for bit.  Its plans (qm::timeslot_mwis_plan and its statistics
// counterpart) append the schedule's words, and the launcher adds the staging
// area of queue_model.h behind them where it fits (queue_csr_force_global and
// queue_csr_set_budget apply); Mwis = false compiles to the two kernels
// above, unchanged.
//
// A graph whose guard rails trip (tsim::ERR) stops stepping; error[b] carries
// the bits and the Python wrapper raises.

#include <ATen/cuda/CUDAContext.h>

#include "queue_model.h"
#include "timeslot_phases.h"

namespace {

struct StatArgs {                   // the statistics outputs, all prezeroed
    const int* late_after;          // (B)
    int* delay_max;                 // (B,J)
    int* late;                      // (B,J)
    int* delay_hist;                // (B,J,nbins)
    int* stuck;                     // (B,J)
    long long* stuck_age;           // (B,J)
    long long* qlen_sum;            // (B,E+N), as the three below
    int* qlen_max;
    int* busy_slots;
    long long* nb_sum;
    int nbins;
};
struct MwisArgs {
    int* sched_slots;               // (B,E) prezeroed
    int stage_budget;               // bytes of LDS after the plan's, or 0
};
template <bool Stats, bool Mwis = false>
using plan_t = std::conditional_t<
    Mwis,
    std::conditional_t<Stats, qm::TimeslotMwisStatsPlan,
                       qm::TimeslotMwisPlan>,
    std::conditional_t<Stats, qm::TimeslotStatsPlan, qm::TimeslotPlan>>;

// the one argument of type T among the mode arguments of a launch
template <class T, class First, class... Rest>
__device__ __forceinline__ const T& mode_arg(const First& first,
                                             const Rest&... rest) {
    if constexpr (std::is_same_v<T, First>) return first;
    else return mode_arg<T>(rest...);
}

// ModeArg is the StatArgs of a statistics launch, then the MwisArgs of a
// scheduled one, and nothing at all otherwise, so that the plain kernel
// keeps its argument list.
template <bool Stats, bool Mwis, class... ModeArg>
__global__ void timeslot_kernel(
    const unsigned char* __restrict__ arrivals,   // (B,T,J)
    const int* __restrict__ slot_off,             // (B,T+1)
    const int* __restrict__ route_links,          // (B,J,H)
    const int* __restrict__ nhop,                 // (B,J)
    const long* __restrict__ dst,                 // (B,J)
    const bool* __restrict__ mask,                // (B,J)
    const float* __restrict__ ul,                 // (B,J)
    const float* __restrict__ dl,                 // (B,J)
    const qm::Tables tb,                          // bw = per-node bw (B,N)
    const int* __restrict__ n_arr,                // (B) real node counts
    int* __restrict__ pool_i,                     // (B,6,P)
    double* __restrict__ pool_rem,                // (B,P)
    long long* __restrict__ delay_sum,            // (B,J) out
    int* __restrict__ count,                      // (B,J) out
    int* __restrict__ error,                      // (B) out
    int* __restrict__ trace,                      // (B,T,3) prezeroed, or null
    const plan_t<Stats, Mwis> p, int N, int J, int H, int T, int warmup,
    int P, const ModeArg... mode_args) {
    extern __shared__ __attribute__((aligned(16))) char smem_raw[];
    int* w = reinterpret_cast<int*>(smem_raw);

    const int b = blockIdx.x;
    const int tid = threadIdx.x;
    const int nt = blockDim.x;
    const qm::Graph g = qm::graph_view(tb, b);

    tsim::Case c;
    c.Eb = g.Eb; c.n = n_arr[b]; c.N = N; c.J = J; c.H = H; c.T = T;
    c.warmup = warmup; c.P = P;
    c.cip = g.cip; c.ccols = g.ccols; c.rates = g.rates; c.bw = g.bw;
    c.arrivals = arrivals + (size_t)b * T * J;
    c.slot_off = slot_off + (size_t)b * (T + 1);
    c.route_links = route_links + (size_t)b * J * H;
    c.nhop = nhop + (size_t)b * J;
    c.dst = reinterpret_cast<const int64_t*>(dst) + (size_t)b * J;
    c.mask = mask + (size_t)b * J;
    c.ul = ul + (size_t)b * J;
    c.dl = dl + (size_t)b * J;

    tsim::State st;
    int* pi = pool_i + (size_t)b * 6 * P;
    st.job = pi;            st.stage = pi + (size_t)P;
    st.t0 = pi + 2 * (size_t)P;   st.next = pi + 3 * (size_t)P;
    st.fnext = pi + 4 * (size_t)P; st.tgt = pi + 5 * (size_t)P;
    st.rem = pool_rem + (size_t)b * P;
    st.head = w + p.head;   st.tail = w + p.tail;
    st.fhead = w + p.fhead; st.jfirst = w + p.jfirst;
    st.fmask = reinterpret_cast<unsigned*>(w + p.fmask);
    st.ftgt0 = w + p.ftgt0; st.fcnt = w + p.fcnt;
    st.jnh = w + p.jnh;     st.jdst = w + p.jdst;
    st.busy = w + p.busy;   st.arr = w + p.arr;
    st.jres = w + p.jres;   st.jnext = w + p.jnext;
    st.misc = w + p.misc;
    st.delay_sum = delay_sum + (size_t)b * J;
    st.count = count + (size_t)b * J;
    st.trace = trace ? trace + (size_t)b * T * 3 : nullptr;
    if constexpr (Stats) {
        const StatArgs& sa = mode_arg<StatArgs>(mode_args...);
        const size_t RS = (size_t)tb.E + N;     // per-resource output stride
        c.late_after = sa.late_after[b];
        c.nbins = sa.nbins;
        c.node_col = tb.E;
        st.qlen = w + p.qlen;   st.qmax = w + p.qmax;
        st.bslots = w + p.bslots;
        st.qsum = reinterpret_cast<long long*>(w + p.qsum);
        st.nbsum = reinterpret_cast<long long*>(w + p.nbsum);
        st.delay_max = sa.delay_max + (size_t)b * J;
        st.late = sa.late + (size_t)b * J;
        st.delay_hist = sa.delay_hist + (size_t)b * J * sa.nbins;
        st.stuck = sa.stuck + (size_t)b * J;
        st.stuck_age = sa.stuck_age + (size_t)b * J;
        st.qlen_sum = sa.qlen_sum + b * RS;
        st.qlen_max = sa.qlen_max + b * RS;
        st.busy_slots = sa.busy_slots + b * RS;
        st.nb_sum = sa.nb_sum + b * RS;
    }
    if constexpr (Mwis) {
        const MwisArgs& ma = mode_arg<MwisArgs>(mode_args...);
        st.qlen = w + p.qlen;
        st.sstate = w + p.mw.sstate;
        st.swin = w + p.mw.swin;
        st.sslots = w + p.mw.sslots;
        st.swt = reinterpret_cast<double*>(w + p.mw.swt);
        st.sched_slots = ma.sched_slots + (size_t)b * tb.E;
    }
    // The schedule walks the conflict rows up to two times a round: a graph
    // whose columns fit the launch's staging area (after the plan's bytes,
    // as for the fixed point's stage_csr) reads them from LDS as 16-bit
    // words, any other graph from global memory.  Block-uniform.
    unsigned short* c16 = nullptr;
    if constexpr (Mwis) {
        const MwisArgs& ma = mode_arg<MwisArgs>(mode_args...);
        if (c.Eb >= 0 && c.Eb <= tb.E && c.Eb <= qm::STAGE_MAX_E) {
            const int nnz = c.cip[c.Eb];
            if (ma.stage_budget > 0 && nnz >= 0 &&
                sizeof(unsigned short) * (size_t)nnz
                    <= (size_t)ma.stage_budget)
                c16 = reinterpret_cast<unsigned short*>(
                    smem_raw + qm::stage_align(p.lds_bytes));
        }
        c.ccols16 = c16;
    }

    // the ragged link count must fit the carve before anything indexes by it
    const bool sized = c.Eb >= 0 && c.Eb <= tb.E;
    if (!sized) {
        if (tid == 0) error[b] = tsim::E_INPUT;
        for (int j = tid; j < J; j += nt) {
            st.delay_sum[j] = 0;
            st.count[j] = 0;
        }
        return;
    }
    tsim::init_jobs(c, st, tid, nt);
    __syncthreads();
    tsim::init_queues<Stats, Mwis>(c, st, tid, nt);
    if constexpr (Mwis)
        if (c16) tsim::stage_cols(c, st, c16, tid, nt);
    // The error word is only ever read through the barrier itself: a thread
    // that sets it reads its own store on arrival, so every thread gets the
    // same answer and the workgroup leaves the loop together.
    int err = __syncthreads_or(st.misc[tsim::ERR]);
    for (int t = 0; t < T && !err; ++t) {
        tsim::arrive<Stats, Mwis>(c, st, t, tid, nt);
        if constexpr (Mwis) {
            // sched_init reads only what this thread's arrive wrote; the
            // barrier that publishes the arrivals carries its answer.  Like
            // err, `left` is the barrier's own result, so the workgroup
            // leaves the round loop together.
            int left = __syncthreads_or(tsim::sched_init(c, st, tid, nt));
            for (int round = 0; left; ++round) {
                if (round >= c.Eb) {            // cannot happen: see KERNELS.md
                    if (tid == 0) st.misc[tsim::ERR] = tsim::E_BOUND;
                    break;
                }
                tsim::sched_round_pick(c, st, tid, nt);
                __syncthreads();
                left = __syncthreads_or(
                    tsim::sched_round_commit(c, st, tid, nt));
            }
        } else {
            __syncthreads();
        }
        tsim::serve<Stats, Mwis>(c, st, t, tid, nt);
        __syncthreads();
        tsim::handover<Stats, Mwis>(c, st, t, tid, nt);
        err = __syncthreads_or(st.misc[tsim::ERR]);
    }
    if constexpr (Mwis) {
        if (!err) tsim::store_sched_slots(c, st, tid, nt);
    }
    if constexpr (Stats) {
        if (!err) {
            tsim::tally_backlog(c, st, tid, nt);
            tsim::store_resource_stats(c, st, tid, nt);
            __syncthreads();
        }
    }
    if (tid == 0) error[b] = st.misc[tsim::ERR];
}

// Every entry point: checks, allocations and the launch of one instantiation.
// Stats appends the nine statistic tensors to the four of the plain launch,
// Mwis appends sched_slots after them.
template <bool Stats, bool Mwis = false>
std::vector<torch::Tensor> timeslot_launch(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace,
    torch::Tensor late_after, long nbins) {
    const int B = arrivals.size(0), T = arrivals.size(1);
    const int J = arrivals.size(2);
    const int N = bw.size(1), E = rates.size(1), H = route_links.size(2);
    TORCH_CHECK(arrivals.is_cuda() && arrivals.is_contiguous() &&
                arrivals.scalar_type() == torch::kUInt8,
                "arrivals: contiguous uint8 (B,T,J) on the GPU");
    TORCH_CHECK(slot_off.scalar_type() == torch::kInt32 &&
                slot_off.is_contiguous() && slot_off.size(0) == B &&
                slot_off.size(1) == T + 1, "slot_off: int32 (B,T+1)");
    TORCH_CHECK(route_links.scalar_type() == torch::kInt32 &&
                route_links.is_contiguous() && route_links.size(0) == B &&
                route_links.size(1) == J && H >= 1,
                "route_links: int32 (B,J,H>=1)");
    TORCH_CHECK(nhop.scalar_type() == torch::kInt32 && nhop.is_contiguous() &&
                nhop.numel() == (int64_t)B * J, "nhop: int32 (B,J)");
    TORCH_CHECK(dst.scalar_type() == torch::kInt64 && dst.is_contiguous() &&
                dst.numel() == (int64_t)B * J, "dst: int64 (B,J)");
    TORCH_CHECK(mask.scalar_type() == torch::kBool && mask.is_contiguous() &&
                mask.numel() == (int64_t)B * J, "mask: bool (B,J)");
    TORCH_CHECK(ul.scalar_type() == torch::kFloat32 && ul.is_contiguous() &&
                dl.scalar_type() == torch::kFloat32 && dl.is_contiguous() &&
                ul.numel() == (int64_t)B * J && dl.numel() == (int64_t)B * J,
                "ul, dl: fp32 (B,J)");
    TORCH_CHECK(rates.is_contiguous() && bw.is_contiguous() &&
                rates.size(0) == B && bw.size(0) == B &&
                conf_indptr.size(0) == B && conf_indptr.size(1) == E + 1 &&
                E_arr.numel() == B && n_arr.numel() == B &&
                conf_base.numel() >= B, "batch tables disagree on B or E");
    TORCH_CHECK(pool >= 0 && warmup >= 0, "pool, warmup: non-negative");
    plan_t<Stats, Mwis> p;
    if constexpr (Stats) {
        TORCH_CHECK(late_after.is_cuda() && late_after.is_contiguous() &&
                    late_after.scalar_type() == torch::kInt32 &&
                    late_after.numel() == B, "late_after: int32 (B)");
        TORCH_CHECK(nbins >= 1 && nbins <= T + 1,
                    "nbins: sim.timeslot.num_delay_bins(T)");
    }
    if constexpr (Stats && Mwis) {
        p = qm::timeslot_mwis_stats_plan(N, E, J);
        TORCH_CHECK(p.fits, "graph too large for LDS timeslot_sim_mwis_stats");
    } else if constexpr (Mwis) {
        p = qm::timeslot_mwis_plan(N, E, J);
        TORCH_CHECK(p.fits, "graph too large for LDS timeslot_sim_mwis");
    } else if constexpr (Stats) {
        p = qm::timeslot_stats_plan(N, E, J);
        TORCH_CHECK(p.fits, "graph too large for LDS timeslot_sim_stats");
    } else {
        p = qm::timeslot_plan(N, E, J);
        TORCH_CHECK(p.fits, "graph too large for LDS timeslot_sim");
    }

    auto opts_i = nhop.options();
    const long P = pool > 0 ? pool : 1;
    auto pool_i = torch::empty({B, 6, P}, opts_i);
    auto pool_rem = torch::empty({B, P}, ul.options().dtype(torch::kFloat64));
    auto delay_sum = torch::empty({B, J}, opts_i.dtype(torch::kInt64));
    auto count = torch::empty({B, J}, opts_i);
    auto error = torch::zeros({B}, opts_i);
    torch::Tensor trace;
    if (want_trace) trace = torch::zeros({B, T, 3}, opts_i);
    StatArgs sa{};
    std::vector<torch::Tensor> stat_out;
    if constexpr (Stats) {
        auto opts_l = opts_i.dtype(torch::kInt64);
        auto delay_max = torch::zeros({B, J}, opts_i);
        auto late = torch::zeros({B, J}, opts_i);
        auto delay_hist = torch::zeros({B, J, nbins}, opts_i);
        auto stuck = torch::zeros({B, J}, opts_i);
        auto stuck_age = torch::zeros({B, J}, opts_l);
        auto qlen_sum = torch::zeros({B, E + N}, opts_l);
        auto qlen_max = torch::zeros({B, E + N}, opts_i);
        auto busy_slots = torch::zeros({B, E + N}, opts_i);
        auto nb_sum = torch::zeros({B, E + N}, opts_l);
        sa.late_after = late_after.data_ptr<int>();
        sa.delay_max = delay_max.data_ptr<int>();
        sa.late = late.data_ptr<int>();
        sa.delay_hist = delay_hist.data_ptr<int>();
        sa.stuck = stuck.data_ptr<int>();
        sa.stuck_age =
            reinterpret_cast<long long*>(stuck_age.data_ptr<long>());
        sa.qlen_sum = reinterpret_cast<long long*>(qlen_sum.data_ptr<long>());
        sa.qlen_max = qlen_max.data_ptr<int>();
        sa.busy_slots = busy_slots.data_ptr<int>();
        sa.nb_sum = reinterpret_cast<long long*>(nb_sum.data_ptr<long>());
        sa.nbins = (int)nbins;
        stat_out = {delay_max, late, delay_hist, stuck, stuck_age,
                    qlen_sum, qlen_max, busy_slots, nb_sum};
    }
    MwisArgs ma{};
    torch::Tensor sched_slots;
    if constexpr (Mwis) {
        sched_slots = torch::zeros({B, E}, opts_i);
        ma.sched_slots = sched_slots.data_ptr<int>();
        ma.stage_budget = qm::stage_budget(p);
    }
    const size_t lds_bytes = qm::launch_lds_bytes(p, ma.stage_budget);
    auto stream = at::cuda::getCurrentCUDAStream();
    auto launch = [&](auto kernel, auto... mode_args) {
        hipLaunchKernelGGL(
            kernel, dim3(B), dim3(p.threads), lds_bytes, stream.stream(),
            arrivals.data_ptr<uint8_t>(), slot_off.data_ptr<int>(),
            route_links.data_ptr<int>(), nhop.data_ptr<int>(),
            dst.data_ptr<long>(), mask.data_ptr<bool>(),
            ul.data_ptr<float>(), dl.data_ptr<float>(),
            qm::tables(conf_indptr, conf_base, conf_cols, rates, bw, T_arr,
                       E_arr),
            n_arr.data_ptr<int>(), pool_i.data_ptr<int>(),
            pool_rem.data_ptr<double>(),
            reinterpret_cast<long long*>(delay_sum.data_ptr<long>()),
            count.data_ptr<int>(), error.data_ptr<int>(),
            want_trace ? trace.data_ptr<int>() : nullptr, p, N, J, H, T,
            (int)warmup, (int)P, mode_args...);
    };
    if constexpr (Stats && Mwis)
        launch(timeslot_kernel<true, true, StatArgs, MwisArgs>, sa, ma);
    else if constexpr (Mwis)
        launch(timeslot_kernel<false, true, MwisArgs>, ma);
    else if constexpr (Stats)
        launch(timeslot_kernel<true, false, StatArgs>, sa);
    else
        launch(timeslot_kernel<false, false>);
    if (!want_trace) trace = torch::empty({0}, opts_i);
    std::vector<torch::Tensor> out = {delay_sum, count, error, trace};
    out.insert(out.end(), stat_out.begin(), stat_out.end());
    if constexpr (Mwis) out.push_back(sched_slots);
    return out;
}

}  // namespace

std::vector<torch::Tensor> timeslot_sim_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace) {
    return timeslot_launch<false>(
        arrivals, slot_off, route_links, nhop, dst, mask, ul, dl, conf_indptr,
        conf_base, conf_cols, rates, bw, T_arr, E_arr, n_arr, warmup, pool,
        want_trace, torch::Tensor(), 0);
}

// timeslot_sim plus the statistics of sim/timeslot.py (stats=True): returns
// delay_sum, count, error, trace, then delay_max, late, delay_hist, stuck,
// stuck_age (per job) and qlen_sum, qlen_max, busy_slots, nb_sum (B, E+N).
// `nbins` is sim.timeslot.num_delay_bins(T); a sojourn whose bin is not below
// it trips the pool guard rail instead of being stored.
std::vector<torch::Tensor> timeslot_sim_stats_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace,
    torch::Tensor late_after, long nbins) {
    return timeslot_launch<true>(
        arrivals, slot_off, route_links, nhop, dst, mask, ul, dl, conf_indptr,
        conf_base, conf_cols, rates, bw, T_arr, E_arr, n_arr, warmup, pool,
        want_trace, late_after, nbins);
}

// The scheduled MAC of sim/timeslot.py (mac="mwis"): what timeslot_sim
// returns, then sched_slots int32 (B,E), zero on padded links.
std::vector<torch::Tensor> timeslot_sim_mwis_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace) {
    return timeslot_launch<false, true>(
        arrivals, slot_off, route_links, nhop, dst, mask, ul, dl, conf_indptr,
        conf_base, conf_cols, rates, bw, T_arr, E_arr, n_arr, warmup, pool,
        want_trace, torch::Tensor(), 0);
}

// ... with the statistics: what timeslot_sim_stats returns, then sched_slots.
std::vector<torch::Tensor> timeslot_sim_mwis_stats_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace,
    torch::Tensor late_after, long nbins) {
    return timeslot_launch<true, true>(
        arrivals, slot_off, route_links, nhop, dst, mask, ul, dl, conf_indptr,
        conf_base, conf_cols, rates, bw, T_arr, E_arr, n_arr, warmup, pool,
        want_trace, late_after, nbins);
}

py::dict timeslot_lds_plan(long N, long E, long J) {
    using namespace pybind11::literals;
    const qm::TimeslotPlan p = qm::timeslot_plan((int)N, (int)E, (int)J);
    return py::dict("lds_bytes"_a = p.lds_bytes, "large"_a = p.large,
                    "threads"_a = p.threads, "fits"_a = p.fits);
}

py::dict timeslot_stats_lds_plan(long N, long E, long J) {
    using namespace pybind11::literals;
    const qm::TimeslotStatsPlan p =
        qm::timeslot_stats_plan((int)N, (int)E, (int)J);
    return py::dict("lds_bytes"_a = p.lds_bytes, "large"_a = p.large,
                    "threads"_a = p.threads, "fits"_a = p.fits);
}

py::dict timeslot_mwis_lds_plan(long N, long E, long J, bool stats) {
    using namespace pybind11::literals;
    const qm::Launch p = stats
        ? static_cast<qm::Launch>(
              qm::timeslot_mwis_stats_plan((int)N, (int)E, (int)J))
        : static_cast<qm::Launch>(
              qm::timeslot_mwis_plan((int)N, (int)E, (int)J));
    return py::dict("lds_bytes"_a = p.lds_bytes, "large"_a = p.large,
                    "threads"_a = p.threads, "fits"_a = p.fits);
}
