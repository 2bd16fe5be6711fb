// Stand-alone host run of the timeslot simulator's scheduled MAC: the phases
// of multihop_offload_amd/ops/hip/timeslot_phases.h with Mwis = true on one
// dumped case (sim.timeslot.dump_case), a workgroup of `nt` threads played in
// sequence, phase by phase, as in timeslot_host.cpp.  The mode is the dump's
// ninth header word: 1 runs the scheduled MAC, 0 the plain phases (and prints
// no sched lines).  With a third argument the conflict columns are first
// staged as 16-bit words (tsim::stage_cols), as the kernel does where they
// fit its staging area.  The round loop is the kernel's: sched_init's and
// sched_round_commit's answers are or-ed over the threads, as the barrier
// does.  Prints
//   error <bits>
//   rounds_max <most iterations of the round loop in one slot>
//   job <j> <delay_sum> <count>
//   trace <t> <arrivals> <departures> <in_network>
//   sched <l> <sched_slots>
// Built by tests/test_timeslot_mwis.py, under the sanitizers where they link.
//
//   c++ -std=c++17 -I multihop_offload_amd/ops/hip timeslot_mwis_host.cpp
//   ./a.out case.bin nt [stage]

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

// the slot loop of timeslot_kernel<false, Mwis>, barriers replaced by
// finishing every thread's call; returns the most round-loop iterations
template <bool Mwis>
int run(const tsim::Case& c, tsim::State& st, int nt, unsigned short* c16) {
    int rounds_max = 0;
    for (int tid = 0; tid < nt; ++tid) tsim::init_jobs(c, st, tid, nt);
    for (int tid = 0; tid < nt; ++tid) {
        tsim::init_queues<false, Mwis>(c, st, tid, nt);
        if (c16) tsim::stage_cols(c, st, c16, tid, nt);
    }
    for (int t = 0; t < c.T && !st.misc[tsim::ERR]; ++t) {
        bool left = false;
        for (int tid = 0; tid < nt; ++tid) {
            tsim::arrive<false, Mwis>(c, st, t, tid, nt);
            if constexpr (Mwis) left |= tsim::sched_init(c, st, tid, nt);
        }
        if constexpr (Mwis) {
            int round = 0;
            for (; left; ++round) {
                if (round >= c.Eb) {
                    st.misc[tsim::ERR] = tsim::E_BOUND;
                    break;
                }
                for (int tid = 0; tid < nt; ++tid)
                    tsim::sched_round_pick(c, st, tid, nt);
                left = false;
                for (int tid = 0; tid < nt; ++tid)
                    left |= tsim::sched_round_commit(c, st, tid, nt);
            }
            if (round > rounds_max) rounds_max = round;
        }
        for (int tid = 0; tid < nt; ++tid)
            tsim::serve<false, Mwis>(c, st, t, tid, nt);
        for (int tid = 0; tid < nt; ++tid)
            tsim::handover<false, Mwis>(c, st, t, tid, nt);
    }
    if constexpr (Mwis) {
        if (!st.misc[tsim::ERR])
            for (int tid = 0; tid < nt; ++tid)
                tsim::store_sched_slots(c, st, tid, nt);
    }
    return rounds_max;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s case.bin nt [stage]\n", argv[0]);
        return 2;
    }
    const int nt = std::atoi(argv[2]);
    const bool want_stage = argc > 3;
    std::FILE* f = std::fopen(argv[1], "rb");
    if (!f || nt < 1) {
        std::fprintf(stderr, "cannot open %s (or nt < 1)\n", argv[1]);
        return 2;
    }
    int h[9];
    if (std::fread(h, sizeof(int), 9, f) != 9) return 2;
    const int E = h[0], N = h[1], J = h[2], H = h[3], T = h[4];
    const int warmup = h[5], P = h[6], nconf = h[7], mode = h[8];
    if (E < 0 || N < 0 || J < 0 || H < 1 || T < 0 || P < 1 || nconf < 0 ||
        mode < 0 || mode > 1) {
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
    std::vector<unsigned short> cols16(
        want_stage && mode && E <= 65535 ? nconf : 0, 0xffffu);
    unsigned short* c16 = cols16.empty() ? nullptr : cols16.data();
    c.ccols16 = c16;

    const size_t R = (size_t)E + N;
    std::vector<int> job(P), stage(P), t0(P), next(P), fnext(P), tgt(P);
    std::vector<double> rem(P);
    std::vector<int> head(R), tail(R), fhead(R), jfirst(R), busy(E);
    std::vector<int> arr(J), jres(J), jnext(J), misc(tsim::MISC_WORDS);
    std::vector<int> ftgt0(R), fcnt(R), jnh(J), jdst(J);
    std::vector<unsigned> fmask(tsim::mask_words((int)R));
    std::vector<long long> delay_sum(J);
    std::vector<int> count(J), trace((size_t)T * 3, 0);
    // the schedule's words start dirty: init_queues has to clear them
    std::vector<int> qlen(R, -7), sstate(E, 7), swin(E, 7), sslots(E, -7);
    std::vector<double> swt(E, -7.0);
    std::vector<int> sched_slots(E, 0);

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
    st.trace = trace.data();
    st.qlen = qlen.data(); st.swt = swt.data(); st.sstate = sstate.data();
    st.swin = swin.data(); st.sslots = sslots.data();
    st.sched_slots = sched_slots.data();

    const int rounds_max = mode ? run<true>(c, st, nt, c16)
                                : run<false>(c, st, nt, nullptr);

    std::printf("error %d\n", st.misc[tsim::ERR]);
    std::printf("rounds_max %d\n", rounds_max);
    for (int j = 0; j < J; ++j)
        std::printf("job %d %lld %d\n", j, delay_sum[j], count[j]);
    for (int t = 0; t < T; ++t)
        std::printf("trace %d %d %d %d\n", t, trace[(size_t)t * 3],
                    trace[(size_t)t * 3 + 1], trace[(size_t)t * 3 + 2]);
    if (mode)
        for (int l = 0; l < E; ++l)
            std::printf("sched %d %d\n", l, sched_slots[l]);
    delete[] mask;
    return st.misc[tsim::ERR] ? 1 : 0;
}
