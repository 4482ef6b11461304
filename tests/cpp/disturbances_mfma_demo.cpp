// tests/cpp/disturbances_mfma_demo.cpp — cortex::Handle::factor_disturbances_mfma on the d = 16 linear-Gaussian chain of
// learn_mfma_demo.cpp (T = 12): one chain-scan sweep, then the smoothed disturbance of every factor, and the scores of the last
// transition alone.  x_{t+1} = A x_t + N(0, I / 2), y_t = x_t + N(0, I); A[i][i] = 0.9, A[i][(i + 1) mod d] = 0.05;
// y_t[k] = t / 4 + ((3 t + k) mod 7) - 3.
//   g++ -std=c++17 -Iinclude -Itests/cpp tests/cpp/disturbances_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"
#include "demo_chain.hpp"

static void row(const char *name, const std::vector<double> &v) {
    std::printf("%s", name);
    for (double x : v) std::printf(" %.17g", x);
    std::printf("\n");
}

int main() {
    try {
        const int T = 12, d = 16;
        cortex::Handle h(cortex::make_config(0, d, CX_SCHED_CHAIN_SCAN));
        demo::chain(h, T, d);      // tests/cpp/demo_chain.hpp: the two parameter sets, the graph, the data
        const auto before = h.factor_disturbances_mfma({}, false);      // nothing computed yet: undefined
        h.sweep(1);
        const auto after = h.factor_disturbances_mfma();
        const auto one = h.factor_disturbances_mfma({4 * T - 1}, false);
        std::printf("before %lld %lld %lld %lld\n", (long long)before.counts[0], (long long)before.counts[1], (long long)before.counts[2],
                    (long long)before.counts[3]);
        std::printf("counts %lld %lld %lld %lld\n", (long long)after.counts[0], (long long)after.counts[1], (long long)after.counts[2],
                    (long long)after.counts[3]);
        std::printf("ids");
        for (int64_t f : after.ids) std::printf(" %lld", (long long)f);
        std::printf("\n");
        row("rows", after.rows);
        row("scores", after.scores);
        row("total", {after.total});
        row("one", one.scores);
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
