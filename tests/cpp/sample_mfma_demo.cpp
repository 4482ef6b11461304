// tests/cpp/sample_mfma_demo.cpp — cortex::Handle::sample_posterior_mfma on a d = 16 linear-Gaussian chain (T = 12): one chain-scan
// sweep, then the posterior mean of the states (the draw under zero noise) and three joint draws under seed 7, on the matrix cores.
// x_{t+1} = A x_t + N(0, I / 2), y_t = x_t + N(0, I); A[i][i] = 0.9, A[i][(i + 1) mod d] = 0.05; y_t[k] = t / 4 + ((3 t + k) mod 7) - 3.
//   g++ -std=c++17 -Iinclude -Itests/cpp tests/cpp/sample_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"
#include "demo_chain.hpp"

int main() {
    try {
        const int T = 12, d = 16;
        cortex::Handle h(cortex::make_config(0, d, CX_SCHED_CHAIN_SCAN));
        const std::vector<int64_t> xs = demo::chain(h, T, d).xs;      // tests/cpp/demo_chain.hpp: the two parameter sets, the graph, the data
        h.sweep(1);
        const std::vector<double> zero((size_t)2 * T * d, 0.0);
        const auto mean = h.sample_posterior_mfma(1, 0, xs, &zero);      // ε = 0: the posterior mean
        const auto draws = h.sample_posterior_mfma(3, 7, xs);
        const auto all = h.sample_posterior_mfma(1, 7, {});              // every variable: the data rows too
        std::printf("counts %lld %lld %lld %lld\n", (long long)mean.second[0], (long long)mean.second[1], (long long)mean.second[2], (long long)mean.second[3]);
        std::printf("sizes %zu %zu %zu\n", mean.first.size(), draws.first.size(), all.first.size());
        std::printf("mean");
        for (double v : mean.first) std::printf(" %.17g", v);
        std::printf("\ndraws");
        for (double v : draws.first) std::printf(" %.17g", v);
        std::printf("\nall");
        for (double v : all.first) std::printf(" %.17g", v);
        std::printf("\n");
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
