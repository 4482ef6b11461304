// tests/cpp/sample_demo.cpp — cortex::Handle::sample_posterior on the scalar SSM chain of learn_demo.cpp (T = 50, y_t = t / 2 +
// ((7 t) mod 5), q = r = 1): one chain-scan sweep, then 4 device draws of the states (seed 5) and one draw with zero noise (the
// posterior mean).
//   g++ -std=c++17 -Iinclude tests/cpp/sample_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        const int T = 50;
        cortex::Handle h(cortex::make_config(0, 1, CX_SCHED_CHAIN_SCAN));
        // ids: x 1..T, y T+1..2T, likelihood 2T+1..3T, transition 3T+1..4T-1
        std::vector<int64_t> ev, ef, fid, ys, liks, xs;
        std::vector<int32_t> kind;
        std::vector<double> par, y;
        for (int i = 0; i < T; i++) { ev.push_back(T + 1 + i); ef.push_back(2 * T + 1 + i); ev.push_back(1 + i); ef.push_back(2 * T + 1 + i); }
        for (int i = 0; i < T - 1; i++) { ev.push_back(1 + i); ef.push_back(3 * T + 1 + i); ev.push_back(2 + i); ef.push_back(3 * T + 1 + i); }
        for (int f = 0; f < 2 * T - 1; f++) { fid.push_back(2 * T + 1 + f); kind.push_back(CX_FACTOR_GAUSS_ADDITIVE); par.insert(par.end(), {1.0, 0.0, 0.0, 0.0}); }
        h.graph_create(ev, ef, fid, kind, par);
        for (int i = 0; i < T; i++) {
            const int t = i + 1;
            ys.push_back(T + 1 + i); liks.push_back(2 * T + 1 + i); y.push_back(0.5 * t + (7 * t) % 5); xs.push_back(1 + i);
        }
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
        h.sweep(1);
        const auto draws = h.sample_posterior(4, 5, xs);                 // 4 x T x 1
        const std::vector<double> zero(2 * T, 0.0);                      // 1 x n_variables x 1
        const auto mean = h.sample_posterior(1, 0, xs, &zero);
        std::printf("draws");
        for (double v : draws.first) std::printf(" %.17g", v);
        std::printf("\nmean");
        for (double v : mean.first) std::printf(" %.17g", v);
        std::printf("\ncounts %lld %lld %lld %lld\n", (long long)draws.second[0], (long long)draws.second[1], (long long)draws.second[2],
                    (long long)draws.second[3]);
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
