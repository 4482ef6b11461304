// tests/cpp/demo_chain.hpp — the model of the *_mfma_demo.cpp programs, built once: a linear-Gaussian chain of T steps at dim d,
// x_{t+1} = A x_t + N(0, I / 2), y_t = x_t + N(0, I); A[i][i] = 0.9, A[i][(i + 1) mod d] = 0.05; y_t[k] = t / 4 + ((3 t + k) mod 7) - 3.
// tests/gpu_support.py: demo_chain is the same model in numpy.
#pragma once
#include <cstdint>
#include <vector>

#include "cortex_hip.hpp"

namespace demo {

struct ChainIds { std::vector<int64_t> xs, ys, liks; };      // the states, the data and the likelihoods, in time order

// sets the two parameter sets of `h`, creates the graph and sets the data; no sweep.
// ids: x 1..T, y T+1..2T, likelihood 2T+1..3T (OUT y, IN x), transition 3T+1..4T-1 (IN x_t, OUT x_{t+1})
inline ChainIds chain(cortex::Handle &h, int T, int d) {
    std::vector<double> A((size_t)d * d, 0.0), Q((size_t)d * d, 0.0), I((size_t)d * d, 0.0);
    for (int i = 0; i < d; i++) { A[(size_t)i * d + i] = 0.9; A[(size_t)i * d + (i + 1) % d] = 0.05; Q[(size_t)i * d + i] = 0.5; I[(size_t)i * d + i] = 1.0; }
    h.set_factor_matrices(0, A, Q);      // set 0: the transitions
    h.set_factor_matrices(1, I, I);      // set 1: the likelihoods
    std::vector<int64_t> ev, ef, fid;
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
    ChainIds ids;
    for (int i = 0; i < T; i++) {
        const int t = i + 1;
        ids.xs.push_back(1 + i); ids.ys.push_back(T + 1 + i); ids.liks.push_back(2 * T + 1 + i);
        for (int k = 0; k < d; k++) y.push_back(0.25 * t + (3 * t + k) % 7 - 3.0);
    }
    h.set_messages(ids.ys, ids.liks, CX_TO_FACTOR, CX_FORM_POINT, y);
    return ids;
}

}  // namespace demo
