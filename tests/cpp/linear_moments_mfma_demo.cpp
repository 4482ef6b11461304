// tests/cpp/linear_moments_mfma_demo.cpp — cortex::Handle::linear_moments_mfma on the d = 16 linear-Gaussian chain of sample_mfma_demo.cpp
// (T = 12): one chain-scan sweep, then the exact mean and covariance of four functionals on the matrix cores — the mean of the states
// 3 .. 8 (every component), component 0 of x_2, component 0 of x_11 (with the one before: a lag-9 autocovariance), and the contrast
// 1'(x_1 - x_12) with a weight on the datum y_5 as well.
//   g++ -std=c++17 -Iinclude -Itests/cpp tests/cpp/linear_moments_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"
#include "demo_chain.hpp"

int main() {
    try {
        const int T = 12, d = 16;
        cortex::Handle h(cortex::make_config(0, d, CX_SCHED_CHAIN_SCAN));
        demo::chain(h, T, d);      // tests/cpp/demo_chain.hpp: the two parameter sets, the graph, the data
        h.sweep(1);
        // the functionals, CSR
        std::vector<int64_t> off{0}, ids;
        std::vector<double> w;
        auto entry = [&](int64_t id, double all, double first) {
            ids.push_back(id);
            for (int k = 0; k < d; k++) w.push_back(k == 0 ? first : all);
        };
        for (int t = 3; t <= 8; t++) entry(t, 1.0 / (6 * d), 1.0 / (6 * d));
        off.push_back((int64_t)ids.size());
        entry(2, 0.0, 1.0);
        off.push_back((int64_t)ids.size());
        entry(11, 0.0, 1.0);
        off.push_back((int64_t)ids.size());
        entry(1, 1.0, 1.0); entry(12, -1.0, -1.0); entry(T + 5, 2.0, 2.0);
        off.push_back((int64_t)ids.size());
        const auto r = h.linear_moments_mfma(off, ids, w);
        const auto m = h.linear_moments_mfma(off, ids, w, false);
        std::printf("counts %lld %lld %lld %lld\n", (long long)r.counts[0], (long long)r.counts[1], (long long)r.counts[2], (long long)r.counts[3]);
        std::printf("sizes %zu %zu %zu %zu\n", r.mean.size(), r.cov.size(), m.mean.size(), m.cov.size());
        std::printf("mean");
        for (double v : r.mean) std::printf(" %.17g", v);
        std::printf("\ncov");
        for (double v : r.cov) std::printf(" %.17g", v);
        std::printf("\nmeans_only");
        for (double v : m.mean) std::printf(" %.17g", v);
        std::printf("\n");
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
