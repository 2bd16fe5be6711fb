// Stand-alone host run of the timeslot simulator's per-slot phases
// (multihop_offload_amd/ops/hip/timeslot_phases.h) on one dumped case
// (sim.timeslot.dump_case).  It plays a workgroup of `nt` threads in
// sequence: every phase is called for tid = 0..nt-1 before the next phase
// starts, which is what the kernel's barriers guarantee.  Prints
//   error <bits>
//   job <j> <delay_sum> <count>      (one line per job)
//   trace <t> <arrivals> <departures> <in_network>   (with a third argument)
// Built by tests/test_timeslot_sim.py, under the sanitizers where they link.
//
//   c++ -std=c++17 -I multihop_offload_amd/ops/hip timeslot_host.cpp -o th
//   ./th case.bin [nt] [trace]

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "timeslot_phases.h"

namespace {

template <class T>
bool read_vec(std::FILE* f, std::vector<T>& v, size_t n) {
    v.resize(n);
    return n == 0 || std::fread(v.data(), sizeof(T), n, f) == n;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s case.bin [nt] [trace]\n", argv[0]);
        return 2;
    }
    const int nt = argc > 2 ? std::atoi(argv[2]) : 64;
    const bool want_trace = argc > 3;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || nt < 1) {
        std::fprintf(stderr, "cannot open %s (or nt < 1)\n", argv[1]);
        return 2;
    }
    int h[9];
    if (std::fread(h, sizeof(int), 9, f) != 9) return 2;
    const int E = h[0], N = h[1], J = h[2], H = h[3], T = h[4];
    const int warmup = h[5], P = h[6], nconf = h[7];
    if (E < 0 || N < 0 || J < 0 || H < 1 || T < 0 || P < 1 || nconf < 0) {
        std::fprintf(stderr, "bad header\n");
        return 2;
    }
    std::vector<int> cip, ccols, slot_off, rl, nhop;
    std::vector<float> rates, bw, ul, dl;
    std::vector<unsigned char> arrivals;
    std::vector<int64_t> dst;
    const bool ok =
        read_vec(f, cip, (size_t)E + 1) && read_vec(f, ccols, (size_t)nconf) &&
        read_vec(f, rates, (size_t)E) && read_vec(f, bw, (size_t)N) &&
        read_vec(f, arrivals, (size_t)T * J) &&
        read_vec(f, slot_off, (size_t)T + 1) &&
        read_vec(f, rl, (size_t)J * H) && read_vec(f, nhop, (size_t)J) &&
        read_vec(f, dst, (size_t)J) && read_vec(f, ul, (size_t)J) &&
        read_vec(f, dl, (size_t)J);
    std::fclose(f);
    if (!ok || cip[E] != nconf) {
        std::fprintf(stderr, "short or inconsistent dump\n");
        return 2;
    }
    // a dump holds real jobs only; std::vector<bool> has no data()
    bool* mask = new bool[J > 0 ? J : 1];
    for (int j = 0; j < J; ++j) mask[j] = true;

    tsim::Case c;
    c.Eb = E; c.n = N; c.N = N; c.J = J; c.H = H; c.T = T;
    c.warmup = warmup; c.P = P;
    c.cip = cip.data(); c.ccols = ccols.data();
    c.rates = rates.data(); c.bw = bw.data();
    c.arrivals = arrivals.data(); c.slot_off = slot_off.data();
    c.route_links = rl.data(); c.nhop = nhop.data(); c.dst = dst.data();
    c.mask = mask; c.ul = ul.data(); c.dl = dl.data();

    const size_t R = (size_t)E + N;
    std::vector<int> job(P), stage(P), t0(P), next(P), fnext(P), tgt(P);
    std::vector<double> rem(P);
    std::vector<int> head(R), tail(R), fhead(R), jfirst(R), busy(E);
    std::vector<int> arr(J), jres(J), jnext(J), misc(tsim::MISC_WORDS);
    std::vector<int> ftgt0(R), fcnt(R), jnh(J), jdst(J);
    std::vector<unsigned> fmask(tsim::mask_words((int)R));
    std::vector<long long> delay_sum(J);
    std::vector<int> count(J), trace(want_trace ? (size_t)T * 3 : 0, 0);

    tsim::State st;
    st.job = job.data(); st.stage = stage.data(); st.t0 = t0.data();
    st.next = next.data(); st.fnext = fnext.data(); st.tgt = tgt.data();
    st.rem = rem.data();
    st.head = head.data(); st.tail = tail.data(); st.fhead = fhead.data();
    st.fmask = fmask.data(); st.ftgt0 = ftgt0.data(); st.fcnt = fcnt.data();
    st.jnh = jnh.data(); st.jdst = jdst.data();
    st.jfirst = jfirst.data(); st.busy = busy.data(); st.arr = arr.data();
    st.jres = jres.data(); st.jnext = jnext.data(); st.misc = misc.data();
    st.delay_sum = delay_sum.data(); st.count = count.data();
    st.trace = want_trace ? trace.data() : nullptr;

    for (int tid = 0; tid < nt; ++tid) tsim::init_jobs(c, st, tid, nt);
    for (int tid = 0; tid < nt; ++tid) tsim::init_queues(c, st, tid, nt);
    for (int t = 0; t < T && !st.misc[tsim::ERR]; ++t) {
        for (int tid = 0; tid < nt; ++tid) tsim::arrive(c, st, t, tid, nt);
        for (int tid = 0; tid < nt; ++tid) tsim::serve(c, st, t, tid, nt);
        for (int tid = 0; tid < nt; ++tid) tsim::handover(c, st, t, tid, nt);
    }

    std::printf("error %d\n", st.misc[tsim::ERR]);
    for (int j = 0; j < J; ++j)
        std::printf("job %d %lld %d\n", j, delay_sum[j], count[j]);
    if (want_trace)
        for (int t = 0; t < T; ++t)
            std::printf("trace %d %d %d %d\n", t, trace[(size_t)t * 3],
                        trace[(size_t)t * 3 + 1], trace[(size_t)t * 3 + 2]);
    delete[] mask;
    return st.misc[tsim::ERR] ? 1 : 0;
}
