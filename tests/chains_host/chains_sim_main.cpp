// chains_sim_main.cpp -- the chain scheduler of the batched online separator (se_snmf_nat_amd/csrc/snmf_online_batch_chains.h)
// as a stand-alone host program: ochains_run drives a SIMULATED batch that keeps the process / restart contract of
// snmf_online_batch_* (hop queue, flush frames, output counts, capacities) and marks every output sample with the chain and
// file it belongs to.  400 seeded random corpora (slots, hop, delay, chains of 0 to 3 files, empty files, NULL outputs, the
// tightest capacities the entry allows, chunk_hops from 0 to INT32_MAX) are checked sample by sample.  No device, no library:
// tests/test_online_chains_native_api.py builds it with the address and undefined-behaviour sanitizers and runs it.
#include <cassert>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <random>
#include "snmf_online_batch_chains.h"

int fail(int code, const char* fmt, ...) { va_list ap; va_start(ap, fmt); vfprintf(stderr, fmt, ap); va_end(ap); fputc('\n', stderr); return code; }

struct Sim {
    int S, hop, delay; size_t nB, r, nA;
    std::vector<int64_t> pend, l; std::vector<char> fin; std::vector<double> tag;  // tag: first value of the stream's dictionary
    std::vector<double> h0tag;
    int calls = 0, restarts = 0; int64_t fed_slots = 0, busy_slots = 0;
    int restart(int n, const int32_t* slots, const double* Bd, const double* Bmd, const float* H0, const float* Ad) {
        ++restarts;
        for (int i = 0; i < n; ++i) {
            int s = slots[i]; assert(s >= 0 && s < S);
            assert(fin[s] || (l[s] == 0 && pend[s] == 0));
            pend[s] = 0; l[s] = 0; fin[s] = 0;
            if (Bd) { tag[s] = Bd[i * nB]; assert(H0); h0tag[s] = H0[i * r]; if (nA) { assert(Ad); volatile float v = Ad[i * nA + nA - 1]; (void)v; } volatile double w = Bd[i * nB + nB - 1]; (void)w; }
            else { assert(!H0 && !Ad); tag[s] += 1000; }  // carry marks the dictionary
            (void)Bmd;
        }
        return 0;
    }
    int process(const float* const* pcm, const int64_t* n, const int32_t* flush, float* const* xt, int16_t* const* x16, const int64_t* cap, int64_t* n_out) {
        ++calls;
        for (int s = 0; s < S; ++s) {
            n_out[s] = 0;
            if (fin[s]) { assert(n[s] == 0 && !flush[s]); continue; }
            if (n[s] == 0 && !flush[s]) continue;
            double sum = 0; for (int64_t j = 0; j < n[s]; ++j) sum += pcm[s][j];
            int64_t tot = pend[s] + n[s], nfr = tot / hop, tail = flush[s] ? delay + 1 : 0;
            int64_t out = std::max<int64_t>(0, l[s] + nfr + tail - delay) - std::max<int64_t>(0, l[s] - delay);
            assert(out * hop <= cap[s]);
            for (int64_t j = 0; j < out * hop; ++j) { xt[s][j] = (float)tag[s]; x16[s][j] = (int16_t)(int)h0tag[s]; }
            n_out[s] = out * hop; l[s] += nfr + tail; pend[s] = tot % hop;
            if (flush[s]) { fin[s] = 1; pend[s] = 0; }
            (void)sum;
        }
        return 0;
    }
    int basis(int k, double* dst) { for (size_t i = 0; i < nB; ++i) dst[i] = tag[k]; return 0; }
};

// 0 (the default), a few hops, or far more than any file holds: the scratch must follow the data, not the argument
static int32_t chunk_hops(std::mt19937& g) {
    switch (g() % 4) {
    case 0: return 0;
    case 1: return g() % 2 ? 2147483647 : 1000000;
    default: return 1 + (int32_t)(g() % 40);
    }
}

int main() {
    std::mt19937 g(1);
    for (int trial = 0; trial < 400; ++trial) {
        OChainsGeom ge; ge.S = 1 + g() % 9; ge.hop = 1 + g() % 20; ge.delay = g() % 4; ge.nB = 3; ge.r = 2; ge.nA = g() % 2 ? 4 : 0; ge.step0 = 1 + g() % 50;
        int nc = g() % 12; std::vector<int32_t> nfiles(nc); size_t nf = 0;
        for (auto& v : nfiles) { v = g() % 4; nf += v; }
        std::vector<std::vector<float>> pcm(nf); std::vector<const float*> pp(nf); std::vector<int64_t> ns(nf), cap(nf), nout(nf, -5);
        std::vector<std::vector<float>> xf(nf); std::vector<std::vector<int16_t>> x16(nf); std::vector<std::vector<double>> B(nf);
        std::vector<float*> pf(nf); std::vector<int16_t*> p16(nf); std::vector<double*> pB(nf);
        for (size_t i = 0; i < nf; ++i) {
            ns[i] = g() % 5 == 0 ? 0 : g() % (60 * ge.hop); pcm[i].assign(ns[i], 1.f); pp[i] = ns[i] ? pcm[i].data() : nullptr;
            cap[i] = (ns[i] / ge.hop + ge.delay + 1) * ge.hop;  // the tightest allowed
            xf[i].assign(cap[i], -1.f); x16[i].assign(cap[i], -1); B[i].assign(ge.nB, -1);
            pf[i] = g() % 7 ? xf[i].data() : nullptr; p16[i] = g() % 7 ? x16[i].data() : nullptr; pB[i] = g() % 7 ? B[i].data() : nullptr;
        }
        std::vector<double> Bd(ge.nB * nc); std::vector<float> H0(ge.r * nc), Ad(ge.nA * nc + 1);
        for (int c = 0; c < nc; ++c) { Bd[c * ge.nB] = c; H0[c * ge.r] = (float)c; }
        OChainsArgs<float> a{nc, nfiles.data(), pp.data(), ns.data(), Bd.data(), nullptr, H0.data(), ge.nA ? Ad.data() : nullptr, chunk_hops(g),
                             p16.data(), pf.data(), cap.data(), nout.data(), pB.data()};
        int64_t total = 0;
        int rc = ochains_check_args(ge, a, &total); assert(rc == 0 && total == (int64_t)nf);
        Sim sim{ge.S, ge.hop, ge.delay, ge.nB, ge.r, ge.nA};
        sim.pend.assign(ge.S, 0); sim.l.assign(ge.S, 0); sim.fin.assign(ge.S, 0); sim.tag.assign(ge.S, -7); sim.h0tag.assign(ge.S, -7);
        if (nf) { rc = ochains_run(ge, a, sim); assert(rc == 0); }
        size_t i = 0;
        for (int c = 0; c < nc; ++c)
            for (int j = 0; j < nfiles[c]; ++j, ++i) {
                int64_t want = (ns[i] / ge.hop + 1) * ge.hop;
                assert(nout[i] == want);
                for (int64_t k = 0; k < cap[i]; ++k) {
                    if (pf[i]) assert(xf[i][k] == (k < want ? (float)(c + 1000 * j) : -1.f));
                    if (p16[i]) assert(x16[i][k] == (k < want ? c : -1));
                }
                if (pB[i]) assert(B[i][0] == c + 1000 * j && B[i][2] == c + 1000 * j);
            }
        for (int s = 0; s < ge.S; ++s) assert(sim.fin[s] || (sim.l[s] == 0 && sim.pend[s] == 0));
    }
    puts("chains driver: 400 simulated corpora ok");
    return 0;
}
