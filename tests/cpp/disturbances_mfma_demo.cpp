// tests/cpp/disturbances_mfma_demo.cpp — cortex::Handle::factor_disturbances_mfma on the d = 16 linear-Gaussian chain of
// learn_mfma_demo.cpp (T = 12): one chain-scan sweep, then the smoothed disturbance of every factor, and the scores of the last
// transition alone.  x_{t+1} = A x_t + N(0, I / 2), y_t = x_t + N(0, I); A[i][i] = 0.9, A[i][(i + 1) mod d] = 0.05;
// y_t[k] = t / 4 + ((3 t + k) mod 7) - 3.
//   g++ -std=c++17 -Iinclude tests/cpp/disturbances_mfma_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

static void row(const char *name, const std::vector<double> &v) {
    std::printf("%s", name);
    for (double x : v) std::printf(" %.17g", x);
    std::printf("\n");
}

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
