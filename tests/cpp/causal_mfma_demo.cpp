// tests/cpp/causal_mfma_demo.cpp — cortex::Handle::causal_marginals_mfma on a d = 16 linear-Gaussian chain (T = 12): one chain-scan
// sweep, then the Kalman predicted and filtered states and the fixed-lag smoother (lag 2) of every state on the matrix cores.
// x_{t+1} = A x_t + N(0, I / 2), y_t = x_t + N(0, I); A[i][i] = 0.9, A[i][(i + 1) mod d] = 0.05; y_t[k] = t / 4 + ((3 t + k) mod 7) - 3.
//   g++ -std=c++17 -Iinclude -Itests/cpp tests/cpp/causal_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
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
        const auto before = h.causal_marginals_mfma(CX_CAUSAL_FILTERED, 0, xs);      // nothing computed yet: every row undefined
        h.sweep(1);
        const auto all = h.causal_marginals_mfma(CX_CAUSAL_FILTERED);                // every variable: the data rows too
        const auto pre = h.causal_marginals_mfma(CX_CAUSAL_PREDICTED, 0, xs);
        const auto flt = h.causal_marginals_mfma(CX_CAUSAL_FILTERED, 0, xs);
        const auto lag = h.causal_marginals_mfma(CX_CAUSAL_FILTERED, 2, xs);
        auto head = [](const char *name, const cortex::Handle::CausalMarginals &r) {
            std::printf("%s %lld %lld %lld %lld\n", name, (long long)r.counts[0], (long long)r.counts[1], (long long)r.counts[2], (long long)r.counts[3]);
        };
        head("before", before); head("all", all); head("predicted", pre); head("filtered", flt); head("lag2", lag);
        const size_t no = (size_t)d + (size_t)d * d;
        for (int t = 0; t < T; t++) {      // per state and estimate: mean[0], mean[d - 1], cov[0][0], cov[1][0], cov[d - 1][d - 1]
            const cortex::Handle::CausalMarginals *rs[3] = {&pre, &flt, &lag};
            std::printf("row %d", t);
            for (const auto *r : rs) {
                const double *o = &r->rows[(size_t)t * no];
                std::printf(" %.17g %.17g %.17g %.17g %.17g", o[0], o[d - 1], o[d], o[d + d], o[d + (size_t)d * d - 1]);
            }
            std::printf("\n");
        }
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
