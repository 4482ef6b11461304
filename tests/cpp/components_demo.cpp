// tests/cpp/components_demo.cpp — cortex::Handle::components and log_evidence_components on two scalar SSM chains in ONE handle (T = 5 and
// T = 9, q = r = 1, data y_t = t / 2 + ((7 t) mod 5); the second chain's ids follow the first's: + 19): one tree sweep, then the component
// of every variable and the log-evidence of each chain.
//   g++ -std=c++17 -Iinclude tests/cpp/components_demo.cpp -o demo -L cortex.jl_amd -lcortex_hip -Wl,-rpath,$PWD/cortex.jl_amd
// Prints "components <C>", "labels <label per variable, ascending id>", "value <k> <log-evidence> <counts x 4>" per component and
// "counts <counts x 4>" (the whole graph's).
// Exit code 77: no GPU (the library has no CPU fallback).
#include <cmath>
#include <cstdio>
#include <vector>

#include "cortex_hip.hpp"

int main() {
    try {
        cortex::Handle h(cortex::make_config(0, 1, CX_SCHED_TREE));
        std::vector<int64_t> ev, ef, fid, ys, liks;
        std::vector<int32_t> kind;
        std::vector<double> par, y;
        int64_t off = 0;
        for (const int T : {5, 9}) {
            for (int i = 0; i < T; i++) { ev.push_back(off + T + 1 + i); ef.push_back(off + 2 * T + 1 + i); ev.push_back(off + 1 + i); ef.push_back(off + 2 * T + 1 + i); }
            for (int i = 0; i < T - 1; i++) { ev.push_back(off + 1 + i); ef.push_back(off + 3 * T + 1 + i); ev.push_back(off + 2 + i); ef.push_back(off + 3 * T + 1 + i); }
            for (int f = 0; f < 2 * T - 1; f++) { fid.push_back(off + 2 * T + 1 + f); kind.push_back(CX_FACTOR_GAUSS_ADDITIVE); par.insert(par.end(), {1.0, 0.0, 0.0, 0.0}); }
            for (int i = 0; i < T; i++) { const int t = i + 1; ys.push_back(off + T + 1 + i); liks.push_back(off + 2 * T + 1 + i); y.push_back(0.5 * t + (7 * t) % 5); }
            off += 4 * T - 1;
        }
        h.graph_create(ev, ef, fid, kind, par);
        h.set_messages(ys, liks, CX_TO_FACTOR, CX_FORM_POINT, y);
        h.sweep(1);
        const auto lab = h.components();
        std::printf("components %lld\nlabels", (long long)lab.second);
        for (const int64_t l : lab.first) std::printf(" %lld", (long long)l);
        std::printf("\n");
        const auto r = h.log_evidence_components();
        for (size_t k = 0; k < r.values.size(); k++)
            std::printf("value %zu %.17g %lld %lld %lld %lld\n", k, r.values[k], (long long)r.comp_counts[k][0], (long long)r.comp_counts[k][1],
                        (long long)r.comp_counts[k][2], (long long)r.comp_counts[k][3]);
        std::printf("counts %lld %lld %lld %lld\n", (long long)r.counts[0], (long long)r.counts[1], (long long)r.counts[2], (long long)r.counts[3]);
        // the named variables, and the sum against the one total
        const auto two = h.components({1, 20});
        const auto total = h.log_evidence();
        if (two.first.size() != 2 || two.first[0] != 0 || two.first[1] != 1 || r.values.size() != 2 ||
            !(std::fabs(r.values[0] + r.values[1] - total.first) <= 1e-12 * (std::fabs(r.values[0]) + std::fabs(r.values[1]))) || r.counts != total.second) {
            std::fprintf(stderr, "the named call or the total differs\n");
            return 1;
        }
        return 0;
    } catch (const cortex::Error &e) {
        std::fprintf(stderr, "%s\n", e.what());
        return e.code == CX_ERR_NO_DEVICE ? 77 : 1;
    }
}
