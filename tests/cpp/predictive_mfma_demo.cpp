// tests/cpp/predictive_mfma_demo.cpp — cortex::Handle::predictive_mfma on a d = 16 linear-Gaussian chain (T = 12): one chain-scan
// sweep, then the one-step-ahead predictive of every datum (CX_PREDICT_CAUSAL: the Kalman innovations) on the matrix cores.  x_{t+1} = A x_t + N(0, I / 2), y_t = x_t + N(0, I);
// A[i][i] = 0.9, A[i][(i + 1) mod d] = 0.05; y_t[k] = t / 4 + ((3 t + k) mod 7) - 3.
//   g++ -std=c++17 -Iinclude -Itests/cpp tests/cpp/predictive_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
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
        const auto before = h.predictive_mfma(CX_PREDICT_CAUSAL);      // nothing computed yet: every row undefined
        h.sweep(1);
        const auto after = h.predictive_mfma(CX_PREDICT_CAUSAL);
        const auto total_only = h.predictive_mfma(CX_PREDICT_CAUSAL, {}, false);
        std::printf("before %.17g %lld %lld %lld %lld\n", before.total, (long long)before.counts[0], (long long)before.counts[1],
                    (long long)before.counts[2], (long long)before.counts[3]);
        std::printf("causal %.17g %lld %lld %lld %lld\n", after.total, (long long)after.counts[0], (long long)after.counts[1],
                    (long long)after.counts[2], (long long)after.counts[3]);
        std::printf("total_only %.17g %zu\n", total_only.total, total_only.rows.size());
        const size_t no = (size_t)d + (size_t)d * d + 2;
        for (size_t r = 0; r < after.ids.size(); r++) {      // per row: factor id, log density, squared residual, y^[0], S[0][0], S[1][0]
            const double *o = &after.rows[r * no];
            std::printf("row %lld %.17g %.17g %.17g %.17g %.17g\n", (long long)after.ids[r], o[d + d * d], o[d + d * d + 1], o[0], o[d], o[d + d]);
        }
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
