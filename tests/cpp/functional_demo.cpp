// tests/cpp/functional_demo.cpp — cortex::Handle::linear_moments on the scalar SSM chain of sample_demo.cpp (T = 50, y_t = t / 2 +
// ((7 t) mod 5), q = r = 1): one chain-scan sweep, then the mean and covariance of three functionals: x_1 - x_50, the mean of
// x_11 .. x_30, and x_25 + 2 y_25 (a weight on an observed variable).
//   g++ -std=c++17 -Iinclude tests/cpp/functional_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        const int T = 50;
        cortex::Handle h(cortex::make_config(0, 1, CX_SCHED_CHAIN_SCAN));
        std::vector<int64_t> ev, ef, fid, ys, liks;
        std::vector<int32_t> kind;
        std::vector<double> par, y;
        for (int i = 0; i < T; i++) { ev.push_back(T + 1 + i); ef.push_back(2 * T + 1 + i); ev.push_back(1 + i); ef.push_back(2 * T + 1 + i); }
        for (int i = 0; i < T - 1; i++) { ev.push_back(1 + i); ef.push_back(3 * T + 1 + i); ev.push_back(2 + i); ef.push_back(3 * T + 1 + i); }
        for (int f = 0; f < 2 * T - 1; f++) { fid.push_back(2 * T + 1 + f); kind.push_back(CX_FACTOR_GAUSS_ADDITIVE); par.insert(par.end(), {1.0, 0.0, 0.0, 0.0}); }
        h.graph_create(ev, ef, fid, kind, par);
        for (int i = 0; i < T; i++) {
            const int t = i + 1;
            ys.push_back(T + 1 + i); liks.push_back(2 * T + 1 + i); y.push_back(0.5 * t + (7 * t) % 5);
        }
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
        h.sweep(1);
        std::vector<int64_t> off{0, 2}, ids{1, T};
        std::vector<double> w{1.0, -1.0};
        for (int t = 11; t <= 30; t++) { ids.push_back(t); w.push_back(1.0 / 20); }
        off.push_back((int64_t)ids.size());
        ids.push_back(25); w.push_back(1.0); ids.push_back(T + 25); w.push_back(2.0);
        off.push_back((int64_t)ids.size());
        const auto r = h.linear_moments(off, ids, w);
        const auto m = h.linear_moments(off, ids, w, false);
        std::printf("mean");
        for (double v : r.mean) std::printf(" %.17g", v);
        std::printf("\nmean_only");
        for (double v : m.mean) std::printf(" %.17g", v);
        std::printf("\ncov");
        for (double v : r.cov) std::printf(" %.17g", v);
        std::printf("\ncounts %lld %lld %lld %lld %zu\n", (long long)r.counts[0], (long long)r.counts[1], (long long)r.counts[2], (long long)r.counts[3],
                    m.cov.size());
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
