// tests/cpp/offsets_demo.cpp — cortex::Handle::set_factor_offsets on a d = 2 state-space chain with a control input and an observation
// mean (T = 12):  x_{t+1} = A x_t + B u_t + N(0, Q),  y_t = H x_t + c + N(0, R),  u_t = (sin 0.7 t, 1), data y_t = (t / 2 + ((7 t) mod 5),
// 1 - t / 4).  One chain-scan sweep, then the marginal of every state.
//   g++ -std=c++17 -Iinclude tests/cpp/offsets_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Prints "marginal <variable id> <mean x 2> <covariance x 4>" per state.
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        const int T = 12, d = 2;
        cortex::Handle h(cortex::make_config(0, d, CX_SCHED_CHAIN_SCAN));
        h.set_factor_matrices(0, {0.9, 0.2, -0.1, 0.8}, {0.3, 0.05, 0.05, 0.2});      // (A, Q)
        h.set_factor_matrices(1, {1.0, 0.5, 0.0, 1.0}, {0.5, 0.1, 0.1, 0.4});         // (H, R)
        std::vector<int64_t> ev, ef, fid, ys, liks, trs, xs;
        std::vector<int32_t> kind, role;
        std::vector<double> par, y, c, bu;
        // states 1 .. T, data T + 1 .. 2 T, likelihoods 2 T + 1 .. 3 T (y out, x in), transitions 3 T + 1 .. 4 T - 1 (x_t in, x_t+1 out)
        for (int i = 0; i < T; i++) {
            ev.push_back(T + 1 + i); ef.push_back(2 * T + 1 + i); role.push_back(CX_ROLE_OUT);
            ev.push_back(1 + i); ef.push_back(2 * T + 1 + i); role.push_back(CX_ROLE_IN);
            fid.push_back(2 * T + 1 + i); kind.push_back(CX_FACTOR_GAUSS_LINEAR); par.insert(par.end(), {1.0, 0.0, 0.0, 0.0});
        }
        for (int i = 0; i < T - 1; i++) {
            ev.push_back(1 + i); ef.push_back(3 * T + 1 + i); role.push_back(CX_ROLE_IN);
            ev.push_back(2 + i); ef.push_back(3 * T + 1 + i); role.push_back(CX_ROLE_OUT);
            fid.push_back(3 * T + 1 + i); kind.push_back(CX_FACTOR_GAUSS_LINEAR); par.insert(par.end(), {0.0, 0.0, 0.0, 0.0});
        }
        h.graph_create(ev, ef, fid, kind, par, role);
        for (int i = 0; i < T; i++) {
            const int t = i + 1;
            xs.push_back(1 + i); ys.push_back(T + 1 + i); liks.push_back(2 * T + 1 + i);
            y.push_back(0.5 * t + (7 * t) % 5); y.push_back(1.0 - 0.25 * t);
            c.push_back(0.3); c.push_back(-0.2);                                      // the observation mean
        }
        for (int i = 0; i < T - 1; i++) {                                             // B u_t, B = diag(0.1, 0.2)
            trs.push_back(3 * T + 1 + i);
            bu.push_back(0.1 * std::sin(0.7 * (i + 1))); bu.push_back(0.2);
        }
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
        h.set_factor_offsets(liks, c);
        h.set_factor_offsets(trs, bu);
        h.sweep(1);
        const std::vector<double> m = h.get_marginals(xs);
        for (int i = 0; i < T; i++) {
            std::printf("marginal %lld", (long long)xs[i]);
            for (int k = 0; k < d + d * d; k++) std::printf(" %.17g", m[(size_t)i * (d + d * d) + k]);
            std::printf("\n");
        }
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
