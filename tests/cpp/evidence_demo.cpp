// tests/cpp/evidence_demo.cpp — cortex::Handle::log_evidence on the scalar SSM chain of test/inference_engine_tests.jl:436-453 (T = 50):
// one chain-scan sweep, then log p(y) from the stored messages.  Data y_t = t / 2 + ((7 t) mod 5), q = r = 1.
//   g++ -std=c++17 -Iinclude tests/cpp/evidence_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        const int T = 50;
        cortex::Handle h(cortex::make_config(0, 1, CX_SCHED_CHAIN_SCAN));
        // ids as BipartiteFactorGraphs hands them out: x 1..T, y T+1..2T, likelihood 2T+1..3T, transition 3T+1..4T-1
        std::vector<int64_t> ev, ef, fid, ys, liks;
        std::vector<int32_t> kind;
        std::vector<double> par, y;
        for (int i = 0; i < T; i++) { ev.push_back(T + 1 + i); ef.push_back(2 * T + 1 + i); ev.push_back(1 + i); ef.push_back(2 * T + 1 + i); }
        for (int i = 0; i < T - 1; i++) { ev.push_back(1 + i); ef.push_back(3 * T + 1 + i); ev.push_back(2 + i); ef.push_back(3 * T + 1 + i); }
        for (int f = 0; f < 2 * T - 1; f++) { fid.push_back(2 * T + 1 + f); kind.push_back(CX_FACTOR_GAUSS_ADDITIVE); par.insert(par.end(), {1.0, 0.0, 0.0, 0.0}); }
        h.graph_create(ev, ef, fid, kind, par);
        for (int i = 0; i < T; i++) { const int t = i + 1; ys.push_back(T + 1 + i); liks.push_back(2 * T + 1 + i); y.push_back(0.5 * t + (7 * t) % 5); }
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
        const auto before = h.log_evidence();      // nothing computed yet: undefined
        h.sweep(1);
        const auto after = h.log_evidence();
        std::printf("before %.17g %lld %lld %lld %lld\n", before.first, (long long)before.second[0], (long long)before.second[1],
                    (long long)before.second[2], (long long)before.second[3]);
        std::printf("evidence %.17g %lld %lld %lld %lld\n", after.first, (long long)after.second[0], (long long)after.second[1],
                    (long long)after.second[2], (long long)after.second[3]);
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
