// tests/cpp/linear_moments_mfma_demo.cpp — cortex::Handle::linear_moments_mfma on the d = 16 linear-Gaussian chain of sample_mfma_demo.cpp
// (T = 12): one chain-scan sweep, then the exact mean and covariance of four functionals on the matrix cores — the mean of the states
// 3 .. 8 (every component), component 0 of x_2, component 0 of x_11 (with the one before: a lag-9 autocovariance), and the contrast
// 1'(x_1 - x_12) with a weight on the datum y_5 as well.
//   g++ -std=c++17 -Iinclude tests/cpp/linear_moments_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        const int T = 12, d = 16;
        cortex::Handle h(cortex::make_config(0, d, CX_SCHED_CHAIN_SCAN));
        std::vector<double> A((size_t)d * d, 0.0), Q((size_t)d * d, 0.0), I((size_t)d * d, 0.0);
        for (int i = 0; i < d; i++) { A[(size_t)i * d + i] = 0.9; A[(size_t)i * d + (i + 1) % d] = 0.05; Q[(size_t)i * d + i] = 0.5; I[(size_t)i * d + i] = 1.0; }
        h.set_factor_matrices(0, A, Q);      // set 0: the transitions
        h.set_factor_matrices(1, I, I);      // set 1: the likelihoods
        // ids: x 1..T, y T+1..2T, likelihood 2T+1..3T (OUT y, IN x), transition 3T+1..4T-1 (IN x_t, OUT x_{t+1})
        std::vector<int64_t> ev, ef, fid, ys, liks;
        std::vector<int32_t> kind, role;
        std::vector<double> par, y;
        for (int i = 0; i < T; i++) {
            ev.push_back(T + 1 + i); ef.push_back(2 * T + 1 + i); role.push_back(CX_ROLE_OUT);
            ev.push_back(1 + i); ef.push_back(2 * T + 1 + i); role.push_back(CX_ROLE_IN);
        }
        for (int i = 0; i < T - 1; i++) {
            ev.push_back(1 + i); ef.push_back(3 * T + 1 + i); role.push_back(CX_ROLE_IN);
            ev.push_back(2 + i); ef.push_back(3 * T + 1 + i); role.push_back(CX_ROLE_OUT);
        }
        for (int f = 0; f < 2 * T - 1; f++) {
            fid.push_back(2 * T + 1 + f); kind.push_back(CX_FACTOR_GAUSS_LINEAR);
            par.insert(par.end(), {f < T ? 1.0 : 0.0, 0.0, 0.0, 0.0});      // params[0]: the parameter set
        }
        h.graph_create(ev, ef, fid, kind, par, role);
        for (int i = 0; i < T; i++) {
            const int t = i + 1;
            ys.push_back(T + 1 + i); liks.push_back(2 * T + 1 + i);
            for (int k = 0; k < d; k++) y.push_back(0.25 * t + (3 * t + k) % 7 - 3.0);
        }
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
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
