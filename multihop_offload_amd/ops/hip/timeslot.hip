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
// A graph whose guard rails trip (tsim::ERR) stops stepping; error[b] carries
// the bits and the Python wrapper raises.

#include <ATen/cuda/CUDAContext.h>

#include "queue_model.h"
#include "timeslot_phases.h"

namespace {

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
    const qm::TimeslotPlan p, int N, int J, int H, int T, int warmup,
    int P) {
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
    tsim::init_queues(c, st, tid, nt);
    // The error word is only ever read through the barrier itself: a thread
    // that sets it reads its own store on arrival, so every thread gets the
    // same answer and the workgroup leaves the loop together.
    int err = __syncthreads_or(st.misc[tsim::ERR]);
    for (int t = 0; t < T && !err; ++t) {
        tsim::arrive(c, st, t, tid, nt);
        __syncthreads();
        tsim::serve(c, st, t, tid, nt);
        __syncthreads();
        tsim::handover(c, st, t, tid, nt);
        err = __syncthreads_or(st.misc[tsim::ERR]);
    }
    if (tid == 0) error[b] = st.misc[tsim::ERR];
}

}  // namespace

std::vector<torch::Tensor> timeslot_sim_hip(
    torch::Tensor arrivals, torch::Tensor slot_off, torch::Tensor route_links,
    torch::Tensor nhop, torch::Tensor dst, torch::Tensor mask,
    torch::Tensor ul, torch::Tensor dl, torch::Tensor conf_indptr,
    torch::Tensor conf_base, torch::Tensor conf_cols, torch::Tensor rates,
    torch::Tensor bw, torch::Tensor T_arr, torch::Tensor E_arr,
    torch::Tensor n_arr, long warmup, long pool, bool want_trace) {
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
    const qm::TimeslotPlan p = qm::timeslot_plan(N, E, J);
    TORCH_CHECK(p.fits, "graph too large for LDS timeslot_sim");

    auto opts_i = nhop.options();
    const long P = pool > 0 ? pool : 1;
    auto pool_i = torch::empty({B, 6, P}, opts_i);
    auto pool_rem = torch::empty({B, P}, ul.options().dtype(torch::kFloat64));
    auto delay_sum = torch::empty({B, J}, opts_i.dtype(torch::kInt64));
    auto count = torch::empty({B, J}, opts_i);
    auto error = torch::zeros({B}, opts_i);
    torch::Tensor trace;
    if (want_trace) trace = torch::zeros({B, T, 3}, opts_i);
    auto stream = at::cuda::getCurrentCUDAStream();
    hipLaunchKernelGGL(
        timeslot_kernel, dim3(B), dim3(p.threads), p.lds_bytes,
        stream.stream(), arrivals.data_ptr<uint8_t>(),
        slot_off.data_ptr<int>(), route_links.data_ptr<int>(),
        nhop.data_ptr<int>(), dst.data_ptr<long>(), mask.data_ptr<bool>(),
        ul.data_ptr<float>(), dl.data_ptr<float>(),
        qm::tables(conf_indptr, conf_base, conf_cols, rates, bw, T_arr,
                   E_arr),
        n_arr.data_ptr<int>(), pool_i.data_ptr<int>(),
        pool_rem.data_ptr<double>(),
        reinterpret_cast<long long*>(delay_sum.data_ptr<long>()),
        count.data_ptr<int>(), error.data_ptr<int>(),
        want_trace ? trace.data_ptr<int>() : nullptr, p, N, J, H, T,
        (int)warmup, (int)P);
    if (!want_trace) trace = torch::empty({0}, opts_i);
    return {delay_sum, count, error, trace};
}

py::dict timeslot_lds_plan(long N, long E, long J) {
    using namespace pybind11::literals;
    const qm::TimeslotPlan p = qm::timeslot_plan((int)N, (int)E, (int)J);
    return py::dict("lds_bytes"_a = p.lds_bytes, "large"_a = p.large,
                    "threads"_a = p.threads, "fits"_a = p.fits);
}
