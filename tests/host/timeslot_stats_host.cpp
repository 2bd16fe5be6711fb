// Stand-alone host run of the timeslot simulator's statistics mode: the
// phases of multihop_offload_amd/ops/hip/timeslot_phases.h with Stats = true
// on one dumped case (sim.timeslot.dump_case), a workgroup of `nt` threads
// played in sequence, phase by phase, as in timeslot_host.cpp.  The
// per-resource outputs are laid out as the kernel lays them out for a batch
// whose largest link count is E + `pad`: link l in column l, node v in column
// E + pad + v, the columns between left zero.  Prints
//   error <bits>
//   nbins <NB>
//   job <j> <delay_sum> <count> <delay_max> <late> <stuck> <stuck_age>
//   hist <j> <NB counts>
//   res <column> <qlen_sum> <qlen_max> <busy_slots> <nb_sum>
// Built by tests/test_timeslot_stats.py, under the sanitizers where they link.
//
//   c++ -std=c++17 -I multihop_offload_amd/ops/hip timeslot_stats_host.cpp
//   ./a.out case.bin nt late_after [pad]

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
    if (argc < 4) {
        std::fprintf(stderr, "usage: %s case.bin nt late_after [pad]\n",
                     argv[0]);
        return 2;
    }
    const int nt = std::atoi(argv[2]);
    const int late_after = std::atoi(argv[3]);
    const int pad = argc > 4 ? std::atoi(argv[4]) : 0;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || nt < 1 || pad < 0) {
        std::fprintf(stderr, "cannot open %s (or nt < 1, pad < 0)\n",
                     argv[1]);
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

    const int NB = tsim::delay_bin(T) + 1;
    tsim::Case c;
    c.Eb = E; c.n = N; c.N = N; c.J = J; c.H = H; c.T = T;
    c.warmup = warmup; c.P = P;
    c.cip = cip.data(); c.ccols = ccols.data();
    c.rates = rates.data(); c.bw = bw.data();
    c.arrivals = arrivals.data(); c.slot_off = slot_off.data();
    c.route_links = rl.data(); c.nhop = nhop.data(); c.dst = dst.data();
    c.mask = mask; c.ul = ul.data(); c.dl = dl.data();
    c.late_after = late_after; c.nbins = NB; c.node_col = E + pad;

    const size_t R = (size_t)E + N, C = R + pad;
    std::vector<int> job(P), stage(P), t0(P), next(P), fnext(P), tgt(P);
    std::vector<double> rem(P);
    std::vector<int> head(R), tail(R), fhead(R), jfirst(R), busy(E);
    std::vector<int> arr(J), jres(J), jnext(J), misc(tsim::MISC_WORDS);
    std::vector<int> ftgt0(R), fcnt(R), jnh(J), jdst(J);
    std::vector<unsigned> fmask(tsim::mask_words((int)R));
    std::vector<long long> delay_sum(J);
    std::vector<int> count(J);
    // the accumulators start dirty: init_queues has to clear them
    std::vector<int> qlen(R, -7), qmax(R, -7), bslots(R, -7);
    std::vector<long long> qsum(R, -7), nbsum(E, -7);
    std::vector<int> delay_max(J, 0), late(J, 0), stuck(J, 0);
    std::vector<int> hist((size_t)J * NB, 0);
    std::vector<long long> stuck_age(J, 0), qlen_sum(C, 0), nb_sum(C, 0);
    std::vector<int> qlen_max(C, 0), busy_slots(C, 0);

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
    st.trace = nullptr;
    st.qlen = qlen.data(); st.qsum = qsum.data(); st.qmax = qmax.data();
    st.bslots = bslots.data(); st.nbsum = nbsum.data();
    st.delay_max = delay_max.data(); st.late = late.data();
    st.delay_hist = hist.data(); st.stuck = stuck.data();
    st.stuck_age = stuck_age.data(); st.qlen_sum = qlen_sum.data();
    st.qlen_max = qlen_max.data(); st.busy_slots = busy_slots.data();
    st.nb_sum = nb_sum.data();

    for (int tid = 0; tid < nt; ++tid) tsim::init_jobs(c, st, tid, nt);
    for (int tid = 0; tid < nt; ++tid)
        tsim::init_queues<true>(c, st, tid, nt);
    for (int t = 0; t < T && !st.misc[tsim::ERR]; ++t) {
        for (int tid = 0; tid < nt; ++tid)
            tsim::arrive<true>(c, st, t, tid, nt);
        for (int tid = 0; tid < nt; ++tid)
            tsim::serve<true>(c, st, t, tid, nt);
        for (int tid = 0; tid < nt; ++tid)
            tsim::handover<true>(c, st, t, tid, nt);
    }
    if (!st.misc[tsim::ERR]) {
        for (int tid = 0; tid < nt; ++tid) {
            tsim::tally_backlog(c, st, tid, nt);
            tsim::store_resource_stats(c, st, tid, nt);
        }
    }

    std::printf("error %d\n", st.misc[tsim::ERR]);
    std::printf("nbins %d\n", NB);
    for (int j = 0; j < J; ++j)
        std::printf("job %d %lld %d %d %d %d %lld\n", j, delay_sum[j],
                    count[j], delay_max[j], late[j], stuck[j], stuck_age[j]);
    for (int j = 0; j < J; ++j) {
        std::printf("hist %d", j);
        for (int k = 0; k < NB; ++k)
            std::printf(" %d", hist[(size_t)j * NB + k]);
        std::printf("\n");
    }
    for (size_t r = 0; r < C; ++r)
        std::printf("res %zu %lld %d %d %lld\n", r, qlen_sum[r], qlen_max[r],
                    busy_slots[r], nb_sum[r]);
    delete[] mask;
    return st.misc[tsim::ERR] ? 1 : 0;
}
