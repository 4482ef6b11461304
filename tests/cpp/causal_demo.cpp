// tests/cpp/causal_demo.cpp — cortex::Handle::causal_marginals on the scalar SSM chain of evidence_demo.cpp (T = 50, q = r = 1, data
// y_t = t / 2 + ((7 t) mod 5)): one chain-scan sweep, then the predicted, the filtered and the lag-5 rows of every state.
//   g++ -std=c++17 -Iinclude tests/cpp/causal_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Prints "<name> <variable id> <mean> <variance>" per row and "<name>_counts <counts x 4>".
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        const int T = 50;
        cortex::Handle h(cortex::make_config(0, 1, CX_SCHED_CHAIN_SCAN));
        std::vector<int64_t> ev, ef, fid, ys, liks, xs;
        std::vector<int32_t> kind;
        std::vector<double> par, y;
        for (int i = 0; i < T; i++) { ev.push_back(T + 1 + i); ef.push_back(2 * T + 1 + i); ev.push_back(1 + i); ef.push_back(2 * T + 1 + i); }
        for (int i = 0; i < T - 1; i++) { ev.push_back(1 + i); ef.push_back(3 * T + 1 + i); ev.push_back(2 + i); ef.push_back(3 * T + 1 + i); }
        for (int f = 0; f < 2 * T - 1; f++) { fid.push_back(2 * T + 1 + f); kind.push_back(CX_FACTOR_GAUSS_ADDITIVE); par.insert(par.end(), {1.0, 0.0, 0.0, 0.0}); }
        h.graph_create(ev, ef, fid, kind, par);
        for (int i = 0; i < T; i++) { const int t = i + 1; ys.push_back(T + 1 + i); liks.push_back(2 * T + 1 + i); y.push_back(0.5 * t + (7 * t) % 5); xs.push_back(1 + i); }
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
        h.sweep(1);
        const char *names[3] = {"predicted", "filtered", "lag5"};
        const int32_t modes[3] = {CX_CAUSAL_PREDICTED, CX_CAUSAL_FILTERED, CX_CAUSAL_FILTERED}, lags[3] = {0, 0, 5};
        for (int k = 0; k < 3; k++) {
            const auto r = h.causal_marginals(modes[k], lags[k], xs);
            for (int i = 0; i < T; i++) std::printf("%s %lld %.17g %.17g\n", names[k], (long long)xs[i], r.rows[2 * i], r.rows[2 * i + 1]);
            std::printf("%s_counts %lld %lld %lld %lld\n", names[k], (long long)r.counts[0], (long long)r.counts[1], (long long)r.counts[2], (long long)r.counts[3]);
        }
        const auto all = h.causal_marginals(CX_CAUSAL_FILTERED);      // every variable: the states, then the data
        if (all.rows.size() != (size_t)(4 * T) || all.counts[0] != 2 * T || all.rows[2 * T] != y[0] || all.rows[2 * T + 1] != 0.0) { std::fprintf(stderr, "the call for every variable differs\n"); return 1; }
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
