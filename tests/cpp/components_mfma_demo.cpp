// tests/cpp/components_mfma_demo.cpp — cortex::Handle::log_evidence_components_mfma on two d = 16 linear-Gaussian chains in ONE handle
// (T = 5 and T = 9; the second chain's ids follow the first's: + 19), the model and data rule of evidence_mfma_demo.cpp per chain:
// x_{t+1} = A x_t + N(0, I / 2), y_t = x_t + N(0, I); A[i][i] = 0.9, A[i][(i + 1) mod d] = 0.05; y_t[k] = t / 4 + ((3 t + k) mod 7) - 3.
// One chain-scan sweep, then the log-evidence of each chain.
//   g++ -std=c++17 -Iinclude tests/cpp/components_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Prints "components <C>", "value <k> <log-evidence> <counts x 4>" per component and "counts <counts x 4>" (the whole graph's).
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        const int d = 16;
        cortex::Handle h(cortex::make_config(0, d, CX_SCHED_CHAIN_SCAN));
        std::vector<double> A((size_t)d * d, 0.0), Q((size_t)d * d, 0.0), I((size_t)d * d, 0.0);
        for (int i = 0; i < d; i++) { A[(size_t)i * d + i] = 0.9; A[(size_t)i * d + (i + 1) % d] = 0.05; Q[(size_t)i * d + i] = 0.5; I[(size_t)i * d + i] = 1.0; }
        h.set_factor_matrices(0, A, Q);      // set 0: the transitions
        h.set_factor_matrices(1, I, I);      // set 1: the likelihoods
        std::vector<int64_t> ev, ef, fid, ys, liks;
        std::vector<int32_t> kind, role;
        std::vector<double> par, y;
        int64_t off = 0;
        for (const int T : {5, 9}) {
            for (int i = 0; i < T; i++) {
                ev.push_back(off + T + 1 + i); ef.push_back(off + 2 * T + 1 + i); role.push_back(CX_ROLE_OUT);
                ev.push_back(off + 1 + i); ef.push_back(off + 2 * T + 1 + i); role.push_back(CX_ROLE_IN);
            }
            for (int i = 0; i < T - 1; i++) {
                ev.push_back(off + 1 + i); ef.push_back(off + 3 * T + 1 + i); role.push_back(CX_ROLE_IN);
                ev.push_back(off + 2 + i); ef.push_back(off + 3 * T + 1 + i); role.push_back(CX_ROLE_OUT);
            }
            for (int f = 0; f < 2 * T - 1; f++) {
                fid.push_back(off + 2 * T + 1 + f); kind.push_back(CX_FACTOR_GAUSS_LINEAR);
                par.insert(par.end(), {f < T ? 1.0 : 0.0, 0.0, 0.0, 0.0});      // params[0]: the parameter set
            }
            for (int i = 0; i < T; i++) {
                const int t = i + 1;
                ys.push_back(off + T + 1 + i); liks.push_back(off + 2 * T + 1 + i);
                for (int k = 0; k < d; k++) y.push_back(0.25 * t + (3 * t + k) % 7 - 3.0);
            }
            off += 4 * T - 1;
        }
        h.graph_create(ev, ef, fid, kind, par, role);
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
        h.sweep(1);
        std::printf("components %lld\n", (long long)h.components().second);
        const auto r = h.log_evidence_components_mfma();
        for (size_t k = 0; k < r.values.size(); k++)
            std::printf("value %zu %.17g %lld %lld %lld %lld\n", k, r.values[k], (long long)r.comp_counts[k][0], (long long)r.comp_counts[k][1],
                        (long long)r.comp_counts[k][2], (long long)r.comp_counts[k][3]);
        std::printf("counts %lld %lld %lld %lld\n", (long long)r.counts[0], (long long)r.counts[1], (long long)r.counts[2], (long long)r.counts[3]);
        // the sum against the one total
        const auto total = h.log_evidence_mfma();
        if (r.values.size() != 2 || !(std::fabs(r.values[0] + r.values[1] - total.first) <= 1e-12 * (std::fabs(r.values[0]) + std::fabs(r.values[1]))) ||
            r.counts != total.second) {
            std::fprintf(stderr, "the total differs\n");
            return 1;
        }
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
