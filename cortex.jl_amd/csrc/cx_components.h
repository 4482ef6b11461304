// cx_components.h — the connected components of the bipartite graph as cx_graph_create received it (cx_graph_components,
// cx_log_evidence_components), and the evidence terms sorted by component.  Host logic only: no HIP, builds with g++
// (cx_hostlogic.cpp: cxh_flat_components).
//
// Two variables are in one component when a path of connections joins them; observed variables and opaque factors are nodes like any
// other, so the labels depend on the graph alone.  Components are numbered 0 .. C-1 by their least variable index (variable indices
// ascend with the ids); a factor has the label of its variables.
#pragma once
#include <algorithm>
#include <cstdint>
#include <numeric>
#include <vector>

namespace cx {
namespace comp {

// union-find over the nv variables and the nf factors (node nv + f): path halving, union by smaller root index — the root of a set is
// its least node, which is a variable whenever the set holds one
struct Sets {
    std::vector<int32_t> parent;
    explicit Sets(int64_t n) : parent((size_t)n) { std::iota(parent.begin(), parent.end(), 0); }
    int32_t find(int32_t x) {
        while (parent[(size_t)x] != x) {
            parent[(size_t)x] = parent[(size_t)parent[(size_t)x]];
            x = parent[(size_t)x];
        }
        return x;
    }
    void unite(int32_t a, int32_t b) {
        a = find(a); b = find(b);
        if (a == b) return;
        if (a < b) parent[(size_t)b] = a; else parent[(size_t)a] = b;
    }
};

// edge e joins variable index edge_var[e] and factor index edge_fac[e].  var_label [nv], fac_label [nf] (-1: a factor without a
// connection); returns C
inline int64_t label(int64_t nv, int64_t nf, int64_t ne, const int32_t *edge_var, const int32_t *edge_fac, std::vector<int32_t> &var_label,
                     std::vector<int32_t> &fac_label) {
    Sets s(nv + nf);
    for (int64_t e = 0; e < ne; e++) s.unite(edge_var[e], (int32_t)(nv + edge_fac[e]));
    var_label.assign((size_t)nv, -1);
    fac_label.assign((size_t)nf, -1);
    int32_t C = 0;
    for (int64_t v = 0; v < nv; v++) {
        const int32_t r = s.find((int32_t)v);      // (r <= v: the least node of the set, labelled before v when r < v)
        var_label[(size_t)v] = r == v ? C++ : var_label[(size_t)r];
    }
    for (int64_t f = 0; f < nf; f++) {
        const int32_t r = s.find((int32_t)(nv + f));
        if (r < nv) fac_label[(size_t)f] = var_label[(size_t)r];
    }
    return C;
}

// The evidence terms (index v for variable v, nv + pair row, nv + n_pair + k-ary row) sorted by (component, term index) into positions:
// component k holds the positions beg[k] .. end[k] - 1, perm[p] is the term at position p and key[p] its component.  A counting sort:
// stable, so the term index is the secondary key.  term_label [nt]: the component of every term.
// Every component starts at a multiple of min(tile, the power of two that holds its terms): one of up to `tile` terms never crosses
// the border of an aligned block of that size, a longer one starts a tile.  Whatever sums the positions in a pattern that is fixed
// relative to such blocks (four per thread, 64 threads per wave, `tile` per workgroup) therefore adds a component's terms in an order
// that depends on that component alone — not on which others share the graph.  The positions between the components (and up to a
// multiple of `quad` at the end) hold perm = key = -1; there are fewer than 3 nt + quad positions (the gap before a component is
// shorter than twice its length).  `tile` is a power of two.
inline int64_t sort_terms(int64_t C, const std::vector<int32_t> &term_label, int64_t tile, int64_t quad, std::vector<int32_t> &perm,
                          std::vector<int32_t> &key, std::vector<int64_t> &beg, std::vector<int64_t> &end) {
    const size_t nt = term_label.size();
    std::vector<int64_t> len((size_t)C, 0);
    for (size_t t = 0; t < nt; t++) len[(size_t)term_label[t]]++;
    beg.assign((size_t)C, 0);
    end.assign((size_t)C, 0);
    int64_t at = 0;
    for (int64_t k = 0; k < C; k++) {
        int64_t p = 1;
        while (p < len[(size_t)k] && p < tile) p <<= 1;
        at = (at + p - 1) / p * p;
        beg[(size_t)k] = at;
        at += len[(size_t)k];
        end[(size_t)k] = at;
    }
    const int64_t npos = (at + quad - 1) / quad * quad;
    perm.assign((size_t)npos, -1);
    key.assign((size_t)npos, -1);
    std::vector<int64_t> next(beg);
    for (size_t t = 0; t < nt; t++) {
        const int32_t k = term_label[t];
        const int64_t p = next[(size_t)k]++;
        perm[(size_t)p] = (int32_t)t;
        key[(size_t)p] = k;
    }
    return npos;
}

}  // namespace comp
}  // namespace cx
