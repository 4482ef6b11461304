// tests/cpp/predictive_demo.cpp — cortex::Handle::predictive on the scalar SSM chain of evidence_demo.cpp (T = 50, q = r = 1, data
// y_t = t / 2 + ((7 t) mod 5)): one chain-scan sweep, then the leave-one-out and the causal rows of every likelihood factor.
//   g++ -std=c++17 -Iinclude tests/cpp/predictive_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Prints "<mode> <factor id> <mean> <variance> <log density> <squared residual>" per row and "<mode>_total <total> <counts x 4>".
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        const int T = 50;
        cortex::Handle h(cortex::make_config(0, 1, CX_SCHED_CHAIN_SCAN));
        std::vector<int64_t> ev, ef, fid, ys, liks;
        std::vector<int32_t> kind;
        std::vector<double> par, y;
        for (int i = 0; i < T; i++) { ev.push_back(T + 1 + i); ef.push_back(2 * T + 1 + i); ev.push_back(1 + i); ef.push_back(2 * T + 1 + i); }
        for (int i = 0; i < T - 1; i++) { ev.push_back(1 + i); ef.push_back(3 * T + 1 + i); ev.push_back(2 + i); ef.push_back(3 * T + 1 + i); }
        for (int f = 0; f < 2 * T - 1; f++) { fid.push_back(2 * T + 1 + f); kind.push_back(CX_FACTOR_GAUSS_ADDITIVE); par.insert(par.end(), {1.0, 0.0, 0.0, 0.0}); }
        h.graph_create(ev, ef, fid, kind, par);
        for (int i = 0; i < T; i++) { const int t = i + 1; ys.push_back(T + 1 + i); liks.push_back(2 * T + 1 + i); y.push_back(0.5 * t + (7 * t) % 5); }
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
        h.sweep(1);
        const char *names[2] = {"loo", "causal"};
        for (int mode = 0; mode < 2; mode++) {
            const auto r = h.predictive(mode);
            for (size_t i = 0; i < r.ids.size(); i++)
                std::printf("%s %lld %.17g %.17g %.17g %.17g\n", names[mode], (long long)r.ids[i], r.rows[4 * i], r.rows[4 * i + 1], r.rows[4 * i + 2], r.rows[4 * i + 3]);
            const auto t = h.predictive(mode, {}, false);
            if (t.total != r.total || t.counts != r.counts) { std::fprintf(stderr, "total-only call differs\n"); return 1; }
            std::printf("%s_total %.17g %lld %lld %lld %lld\n", names[mode], r.total, (long long)r.counts[0], (long long)r.counts[1], (long long)r.counts[2],
                        (long long)r.counts[3]);
        }
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
