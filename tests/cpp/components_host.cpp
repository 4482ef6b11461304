// tests/cpp/components_host.cpp — the host labelling and term sort of cx_components.h on their own, for the address / undefined-behaviour
// sanitizers on the CPU (no HIP, no GPU):
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-omit-frame-pointer -Icortex.jl_amd/csrc tests/cpp/components_host.cpp -o components_host
// Checks, on random forests of factors of 1 .. 5 variables with random variable numbering: every connection joins equal labels, labels
// are numbered by least variable, the count equals a flood fill's, the sorted terms are a permutation ordered by (label, term), every
// component starts at its alignment and never crosses an aligned block it fits in, and the positions between hold no term.  Also the
// corner cases: no connection at all, a factor without a connection.  Exit code 0: all held.
#include <cstdio>
#include <cstdlib>
#include <random>

#include "cx_components.h"

static int failures = 0;
#define CHECK(cond) do { if (!(cond)) { std::fprintf(stderr, "line %d: %s\n", __LINE__, #cond); failures++; } } while (0)

static void one(std::mt19937_64 &rng, int nv, int nf, int kmax) {
    std::vector<int32_t> ev, ef;
    for (int f = 0; f < nf; f++) {
        const int k = 1 + (int)(rng() % (unsigned)kmax);
        for (int j = 0; j < k; j++) { ev.push_back((int32_t)(rng() % (unsigned)nv)); ef.push_back(f); }
    }
    std::vector<int32_t> vl, fl;
    const int64_t C = cx::comp::label(nv, nf, (int64_t)ev.size(), ev.data(), ef.data(), vl, fl);
    CHECK((int)vl.size() == nv && (int)fl.size() == nf);
    for (size_t e = 0; e < ev.size(); e++) CHECK(vl[(size_t)ev[e]] == fl[(size_t)ef[e]]);
    // numbered by least variable: the first occurrence of the labels ascends, and a flood fill finds as many sets
    int32_t next = 0;
    for (int v = 0; v < nv; v++) {
        CHECK(vl[(size_t)v] >= 0 && vl[(size_t)v] <= next);
        if (vl[(size_t)v] == next) next++;
    }
    CHECK(next == C);
    std::vector<int32_t> seen((size_t)nv, -1);
    int64_t sets = 0;
    for (int s = 0; s < nv; s++) {
        if (seen[(size_t)s] >= 0) continue;
        seen[(size_t)s] = (int32_t)sets;
        bool grew = true;
        while (grew) {      // (quadratic: the graphs are small)
            grew = false;
            for (int f = 0; f < nf; f++) {
                bool touched = false;
                for (size_t e = 0; e < ev.size(); e++) touched = touched || (ef[e] == f && seen[(size_t)ev[e]] == sets);
                if (!touched) continue;
                for (size_t e = 0; e < ev.size(); e++)
                    if (ef[e] == f && seen[(size_t)ev[e]] < 0) { seen[(size_t)ev[e]] = (int32_t)sets; grew = true; }
            }
        }
        sets++;
    }
    CHECK(sets == C);
    for (int v = 0; v < nv; v++) CHECK(seen[(size_t)v] == vl[(size_t)v]);
    // the terms: the variables, then one per factor that has a connection
    std::vector<int32_t> term(vl), perm, key;
    std::vector<int64_t> beg, end;
    for (int f = 0; f < nf; f++) if (fl[(size_t)f] >= 0) term.push_back(fl[(size_t)f]);
    const int64_t tile = 8, quad = 4;      // (small, so that components of more than a tile occur)
    const int64_t npos = cx::comp::sort_terms(C, term, tile, quad, perm, key, beg, end);
    CHECK((int64_t)perm.size() == npos && (int64_t)key.size() == npos && (int64_t)beg.size() == C && (int64_t)end.size() == C);
    CHECK(npos % quad == 0 && npos < 3 * (int64_t)term.size() + quad);
    std::vector<char> hit(term.size(), 0);
    size_t placed = 0;
    for (int64_t k = 0; k < C; k++) {
        const int64_t b = beg[(size_t)k], e = end[(size_t)k], len = e - b;
        CHECK(len >= 1 && b >= (k ? end[(size_t)k - 1] : 0) && e <= npos);
        int64_t p2 = 1;
        while (p2 < len && p2 < tile) p2 <<= 1;
        CHECK(b % p2 == 0);
        if (len <= tile) CHECK(b / p2 == (e - 1) / p2);      // inside one aligned block
        for (int64_t p = b; p < e; p++) {
            CHECK(key[(size_t)p] == k && perm[(size_t)p] >= 0 && (size_t)perm[(size_t)p] < term.size() && !hit[(size_t)perm[(size_t)p]]);
            hit[(size_t)perm[(size_t)p]] = 1;
            CHECK(term[(size_t)perm[(size_t)p]] == k);
            if (p > b) CHECK(perm[(size_t)p - 1] < perm[(size_t)p]);      // the term index is the secondary key
            placed++;
        }
    }
    CHECK(placed == term.size());
    size_t holes = 0;
    for (int64_t p = 0; p < npos; p++) if (key[(size_t)p] < 0) { CHECK(perm[(size_t)p] == -1 && key[(size_t)p] == -1); holes++; }
    CHECK(holes + placed == (size_t)npos);
}

int main() {
    std::mt19937_64 rng(20240607);
    for (int rep = 0; rep < 200; rep++) one(rng, 1 + (int)(rng() % 60), (int)(rng() % 40), 1 + (int)(rng() % 5));
    one(rng, 5, 0, 1);                                  // no factor, no connection: five components
    {
        std::vector<int32_t> vl, fl;
        const int32_t ev[] = {0, 1}, ef[] = {1, 1};     // factor 0 has no connection
        CHECK(cx::comp::label(3, 2, 2, ev, ef, vl, fl) == 2);
        CHECK(fl[0] == -1 && fl[1] == 0 && vl[0] == 0 && vl[1] == 0 && vl[2] == 1);
    }
    if (failures) { std::fprintf(stderr, "%d checks failed\n", failures); return 1; }
    std::printf("components_host: ok\n");
    return 0;
}
