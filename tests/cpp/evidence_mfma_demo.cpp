// tests/cpp/evidence_mfma_demo.cpp — cortex::Handle::log_evidence_mfma on a d = 16 linear-Gaussian chain (T = 12): one chain-scan
// sweep, then log p(y) from the stored messages on the matrix cores.  x_{t+1} = A x_t + N(0, I / 2), y_t = x_t + N(0, I);
// A[i][i] = 0.9, A[i][(i + 1) mod d] = 0.05; y_t[k] = t / 4 + ((3 t + k) mod 7) - 3.
//   g++ -std=c++17 -Iinclude -Itests/cpp tests/cpp/evidence_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
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
        const auto before = h.log_evidence_mfma();      // nothing computed yet: undefined
        h.sweep(1);
        const auto after = h.log_evidence_mfma();
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
