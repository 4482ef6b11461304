// cortex_hip.hpp — C++17 host classes over the C ABI of cortex_hip.h (header-only; nothing here is part of the ABI).
//
// SURVEY.md §8b asks for "a Julia subtype (shim) and an equivalent C++ host class, both owning a cx_handle*".  The Julia
// shim is julia/CortexHIP.jl; this is the C++ side:
//
//   cortex::Handle        RAII owner of a cx_handle; every method is one ABI call, a non-zero status becomes cortex::Error
//                         carrying cx_last_error() (the analogue of the shim's `error(unsafe_string(cx_last_error(h)))`).
//                         Exceptions exist only on THIS side of the boundary — none crosses the C ABI.
//   cortex::HipProcessor  the plugin of src/inference_engine.jl:331-509 in the two forms a host scheduler drives:
//                           process(kind, variable, factor)  = `process!` overridden to ENQUEUE (precedent: the
//                                                              InferenceRequestScanner, inference_engine.jl:528-537);
//                           flush()                          = one cx_update_batch for everything enqueued, in order;
//                           update_marginals(ids, sweeps)    = `update_marginals!` specialised on the processor type:
//                                                              cx_sweep + cx_get_marginals.
//   cortex::VmpProcessor  the variational families (weak dependencies): set_marginal / update_marginals / marginals.
//
// tests/cpp/host_class_demo.cpp drives both against the reference's SSM test graphs; tests/test_gpu_cpp_host.py checks
// its output against the exact smoother and the array form of the variational updates.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <utility>
#include <array>
#include <vector>

#include "cortex_hip.h"

namespace cortex {

struct Error : std::runtime_error {
    int32_t code;
    Error(int32_t c, const std::string &msg) : std::runtime_error("cortex_hip status " + std::to_string(c) + ": " + msg), code(c) {}
};

inline cx_config make_config(int32_t device = 0, int32_t dim = 1, int32_t schedule = CX_SCHED_FUSED, int32_t family = CX_FAMILY_GAUSSIAN,
                             bool marginals_in_sweep = true, bool materialize_messages_to_factor = false) {
    cx_config c{};
    c.struct_size = (int32_t)sizeof(cx_config);
    c.device = device; c.dim = dim; c.schedule = schedule; c.family = family;
    c.compute_marginals_in_sweep = marginals_in_sweep ? 1 : 0;
    c.materialize_messages_to_factor = materialize_messages_to_factor ? 1 : 0;
    return c;
}

class Handle {
  public:
    explicit Handle(const cx_config &cfg) : dim_(cfg.dim) {
        const int32_t rc = cx_create(&cfg, &h_);
        if (rc != CX_OK) throw Error(rc, cx_last_error(nullptr));
    }
    ~Handle() { if (h_) (void)cx_destroy(h_); }
    Handle(const Handle &) = delete;
    Handle &operator=(const Handle &) = delete;
    Handle(Handle &&o) noexcept : h_(o.h_), dim_(o.dim_) { o.h_ = nullptr; }
    Handle &operator=(Handle &&o) noexcept { if (this != &o) { if (h_) (void)cx_destroy(h_); h_ = o.h_; dim_ = o.dim_; o.h_ = nullptr; } return *this; }

    cx_handle *get() const { return h_; }
    int32_t dim() const { return dim_; }

    // graph ingestion: the flattened BipartiteFactorGraph (model_engine.jl:329-391)
    void graph_create(const std::vector<int64_t> &edge_var, const std::vector<int64_t> &edge_fac, const std::vector<int64_t> &factor_ids,
                      const std::vector<int32_t> &factor_kind, const std::vector<double> &factor_params /* CX_NPARAM per factor, or empty */,
                      const std::vector<int32_t> &edge_role = {}) {
        if (edge_var.size() != edge_fac.size() || factor_ids.size() != factor_kind.size() ||
            (!edge_role.empty() && edge_role.size() != edge_var.size()) ||
            (!factor_params.empty() && factor_params.size() != factor_ids.size() * CX_NPARAM))
            throw Error(CX_ERR_INVALID_ARGUMENT, "graph_create: array lengths disagree");
        std::vector<double> zeros;
        const double *params = factor_params.data();
        if (factor_params.empty()) { zeros.assign(factor_ids.size() * CX_NPARAM, 0.0); params = zeros.data(); }
        check(cx_graph_create(h_, (int64_t)edge_var.size(), edge_var.data(), edge_fac.data(), edge_role.empty() ? nullptr : edge_role.data(),
                              (int64_t)factor_ids.size(), factor_ids.data(), factor_kind.data(), params));
    }
    void set_factor_matrices(int64_t parameter_set, const std::vector<double> &A, const std::vector<double> &Q) {
        check(cx_set_factor_matrices(h_, parameter_set, A.data(), Q.data()));
    }
    // dim 2 - 4: the named two-variable CX_FACTOR_GAUSS_LINEAR factors become x_out = A x_in + b + N(0, Q); offsets: dim doubles per factor
    // (cx_set_factor_offsets; factors not named keep theirs, initially 0)
    void set_factor_offsets(const std::vector<int64_t> &factor_ids, const std::vector<double> &offsets) {
        need(offsets.size(), factor_ids.size() * (size_t)dim_, "set_factor_offsets offsets");
        check(cx_set_factor_offsets(h_, (int64_t)factor_ids.size(), factor_ids.empty() ? nullptr : factor_ids.data(), offsets.empty() ? nullptr : offsets.data()));
    }
    // dim 5 - 64: the same through the matrix-core kernels (cx_set_factor_offsets_mfma); offsets: the user's dim doubles per factor
    void set_factor_offsets_mfma(const std::vector<int64_t> &factor_ids, const std::vector<double> &offsets) {
        need(offsets.size(), factor_ids.size() * (size_t)dim_, "set_factor_offsets_mfma offsets");
        check(cx_set_factor_offsets_mfma(h_, (int64_t)factor_ids.size(), factor_ids.empty() ? nullptr : factor_ids.data(), offsets.empty() ? nullptr : offsets.data()));
    }
    cx_stats stats() const { cx_stats s{}; check(cx_graph_stats(h_, &s)); return s; }
    // CX_SCHED_TREE: { depth, stages, items, k-ary entries, components, messages up, messages down, marginals } of the last sweep's plan
    std::array<int64_t, 8> tree_plan_stats() const { std::array<int64_t, 8> o{}; check(cx_tree_plan_stats(h_, o.data())); return o; }
    std::array<int64_t, 4> tree_heavy_path_stats() const { std::array<int64_t, 4> o{}; check(cx_tree_heavy_path_stats(h_, o.data())); return o; }

    // data injection / read-back: the user's set_value! on message signals (signal.jl:232-253)
    void set_messages(const std::vector<int64_t> &variable_ids, const std::vector<int64_t> &factor_ids, int32_t direction, int32_t form,
                      const std::vector<double> &payload) {
        need(payload.size(), variable_ids.size() * (size_t)cx_payload_doubles(dim_, form), "set_messages payload");
        check(cx_set_messages(h_, (int64_t)variable_ids.size(), variable_ids.data(), factor_ids.data(), direction, form, payload.data()));
    }
    std::vector<double> get_messages(const std::vector<int64_t> &variable_ids, const std::vector<int64_t> &factor_ids, int32_t direction,
                                     int32_t form = CX_FORM_MOMENT) const {
        std::vector<double> out(variable_ids.size() * (size_t)cx_payload_doubles(dim_, CX_FORM_MOMENT));
        check(cx_get_messages(h_, (int64_t)variable_ids.size(), variable_ids.data(), factor_ids.data(), direction, form, out.data()));
        return out;
    }
    void seed_messages(int32_t direction, double mean, double variance) { check(cx_seed_messages(h_, direction, mean, variance)); }
    std::vector<double> get_marginals(const std::vector<int64_t> &variable_ids) const {
        std::vector<double> out(variable_ids.size() * (size_t)cx_payload_doubles(dim_, CX_FORM_MOMENT));
        check(cx_get_marginals(h_, (int64_t)variable_ids.size(), variable_ids.data(), out.data()));
        return out;
    }

    // compute
    void update_batch(const std::vector<cx_item> &items) { check(cx_update_batch(h_, items.data(), (int64_t)items.size())); }
    void update_batch_async(const std::vector<cx_item> &items) { check(cx_update_batch_async(h_, items.data(), (int64_t)items.size())); }
    void sweep(int32_t n = 1) { check(cx_sweep(h_, n)); }
    // CX_SCHED_REFERENCE: ONE update_marginals!(engine, variable_ids) — the named variables in the caller's order, only what is pending for them
    void sweep_for(const std::vector<int64_t> &variable_ids) { check(cx_sweep_for(h_, (int64_t)variable_ids.size(), variable_ids.data())); }
    std::array<int64_t, 4> chain_scan_stats() const { std::array<int64_t, 4> o{}; check(cx_chain_scan_stats(h_, o.data())); return o; }      // state, one-launch scans so far, 0, 0
    std::array<int64_t, 8> ref_plan_stats() const { std::array<int64_t, 8> o{}; check(cx_ref_plan_stats(h_, o.data())); return o; }      // stages, launches, executions, messages, passes, plans, hits, misses
    std::vector<cx_item> ref_trace() const {       // the executions of the last reference-order call, in the reference's order
        int64_t n = 0;
        check(cx_ref_trace(h_, 0, nullptr, &n));
        std::vector<cx_item> out((size_t)n);
        if (n) check(cx_ref_trace(h_, n, out.data(), &n));
        return out;
    }
    // a user resolver's wiring: one triple per add_dependency!(signal, dependency; flags) (CX_WIRE_*), right after graph_create
    void graph_wire(const std::vector<cx_item> &signals, const std::vector<cx_item> &dependencies, const std::vector<int32_t> &flags) {
        need(dependencies.size(), signals.size(), "graph_wire dependencies"); need(flags.size(), signals.size(), "graph_wire flags");
        check(cx_graph_wire(h_, (int64_t)signals.size(), signals.data(), dependencies.data(), flags.data()));
    }
    void set_damping(double lambda) { check(cx_set_damping(h_, lambda)); }      // fused / flooding sweeps: new = (1 - lambda) rule + lambda old
    double residual() { double r = 0; check(cx_residual(h_, &r)); return r; }
    std::array<int64_t, 4> message_health() { std::array<int64_t, 4> o{}; check(cx_message_health(h_, o.data())); return o; }      // defined, undefined, negative precision, non-finite
    // log p(data) from the stored messages (exact on forests at a fixed point, the Bethe estimate elsewhere); counts: factor terms, variable
    // terms, terms with an undefined input, terms whose belief is not positive definite (the value is NaN when either of the last two is > 0)
    std::pair<double, std::array<int64_t, 4>> log_evidence() {
        double v = 0; std::array<int64_t, 4> o{};
        check(cx_log_evidence(h_, &v, o.data()));
        return {v, o};
    }
    // the same at the matrix-core dims, 5 .. 64 (cx_log_evidence_mfma): one wave per term on the f64 matrix cores
    std::pair<double, std::array<int64_t, 4>> log_evidence_mfma() {
        double v = 0; std::array<int64_t, 4> o{};
        check(cx_log_evidence_mfma(h_, &v, o.data()));
        return {v, o};
    }
    // the connected component of every named variable (empty: every variable in ascending id) and the number of components; components
    // are numbered by their least variable id (cx_graph_components)
    std::pair<std::vector<int64_t>, int64_t> components(const std::vector<int64_t> &variable_ids = {}) {
        const int64_t n = variable_ids.empty() ? stats().n_variables : (int64_t)variable_ids.size();
        std::vector<int64_t> out((size_t)n + 1);      // (+ 1: never a NULL array)
        int64_t c = 0;
        check(cx_graph_components(h_, (int64_t)variable_ids.size(), variable_ids.empty() ? nullptr : variable_ids.data(), out.data(), &c));
        out.resize((size_t)n);
        return {out, c};
    }
    // log p(data) per connected component from the stored messages (cx_log_evidence_components): values [C] (NaN: that component has an
    // undefined input or a belief that is not positive definite, the others keep theirs), comp_counts [C][4] and counts (the whole graph's)
    // as log_evidence's counts
    struct EvidenceComponents { std::vector<double> values; std::vector<std::array<int64_t, 4>> comp_counts; std::array<int64_t, 4> counts{}; };
    EvidenceComponents evidence_components(int32_t (*call)(cx_handle *, int64_t, double *, int64_t *, int64_t *, int64_t *)) {
        EvidenceComponents r;
        int64_t c = 0;
        check(cx_graph_components(h_, 0, nullptr, nullptr, &c));
        r.values.resize((size_t)c + 1);
        r.comp_counts.resize((size_t)c + 1);
        check(call(h_, c, r.values.data(), r.comp_counts[0].data(), &c, r.counts.data()));
        r.values.resize((size_t)c);
        r.comp_counts.resize((size_t)c);
        return r;
    }
    EvidenceComponents log_evidence_components() { return evidence_components(cx_log_evidence_components); }
    // the same at the matrix-core dims, 5 .. 64 (cx_log_evidence_components_mfma): the terms, counts and NaN rule of log_evidence_mfma
    EvidenceComponents log_evidence_components_mfma() { return evidence_components(cx_log_evidence_components_mfma); }
    // the joint posterior of two-variable Gaussian factors from the stored messages: per factor 2d means then the 2d x 2d covariance
    // (row-major), (out, in) (NaN rows: an undefined input or a belief that is not positive definite)
    std::vector<double> factor_beliefs(const std::vector<int64_t> &factor_ids) {
        std::vector<double> out(factor_ids.size() * (size_t)(2 * dim_ + 4 * dim_ * dim_));
        check(cx_factor_beliefs(h_, (int64_t)factor_ids.size(), factor_ids.data(), out.data()));
        return out;
    }
    // EM statistics in residual coordinates, summed per group: n_groups rows of 1 + 2d + 3d^2 doubles (n | Σ E[r] | Σ E[x_in] | S_rr | S_rx |
    // S_xx); empty factor_ids and groups: one group per parameter set (dim 2 - 4).  counts: factors, non-empty groups, undefined, not pd
    std::pair<std::vector<double>, std::array<int64_t, 4>> factor_statistics(const std::vector<int64_t> &factor_ids, const std::vector<int64_t> &groups,
                                                                             int64_t n_groups) {
        need(groups.size(), factor_ids.size(), "factor_statistics groups");
        std::vector<double> out((size_t)n_groups * (size_t)(1 + 2 * dim_ + 3 * dim_ * dim_));
        std::array<int64_t, 4> o{};
        const bool by_set = factor_ids.empty();
        check(cx_factor_statistics(h_, (int64_t)factor_ids.size(), by_set ? nullptr : factor_ids.data(), by_set ? nullptr : groups.data(), n_groups,
                                   out.data(), o.data()));
        return {out, o};
    }
    // the two above at the matrix-core dims, 5 .. 64 (cx_factor_beliefs_mfma, cx_factor_statistics_mfma): the same layouts with d the dim
    // the handle was created with; one wave per factor on the f64 matrix cores
    std::vector<double> factor_beliefs_mfma(const std::vector<int64_t> &factor_ids) {
        std::vector<double> out(factor_ids.size() * (size_t)(2 * dim_ + 4 * dim_ * dim_) + 1);      // (+ 1: never a NULL array)
        check(cx_factor_beliefs_mfma(h_, (int64_t)factor_ids.size(), factor_ids.data(), out.data()));
        out.pop_back();
        return out;
    }
    std::pair<std::vector<double>, std::array<int64_t, 4>> factor_statistics_mfma(const std::vector<int64_t> &factor_ids, const std::vector<int64_t> &groups,
                                                                                  int64_t n_groups) {
        need(groups.size(), factor_ids.size(), "factor_statistics_mfma groups");
        std::vector<double> out((size_t)n_groups * (size_t)(1 + 2 * dim_ + 3 * dim_ * dim_));
        std::array<int64_t, 4> o{};
        const bool by_set = factor_ids.empty();
        check(cx_factor_statistics_mfma(h_, (int64_t)factor_ids.size(), by_set ? nullptr : factor_ids.data(), by_set ? nullptr : groups.data(), n_groups,
                                        out.data(), o.data()));
        return {out, o};
    }
    // the smoothed disturbance of every two-variable x_out = A x_in + b + w factor at the matrix-core dims (cx_factor_disturbances_mfma): per
    // row E[w | data] (d) then Cov(w | data) (d x d, row-major), per score row t = E[w'Q⁻¹w | data] and q = E[w]'Q⁻¹E[w]; factor_ids empty:
    // every such factor in ascending id (`ids` names them).  counts: rows, finite, with an undefined input, not positive definite (NaN rows);
    // total: Σ t of the finite rows.  rows == false: scores, total and counts only
    struct Disturbances { std::vector<int64_t> ids; std::vector<double> rows, scores; double total = 0; std::array<int64_t, 4> counts{}; };
    Disturbances factor_disturbances_mfma(const std::vector<int64_t> &factor_ids = {}, bool rows = true) {
        Disturbances r;
        r.ids = factor_ids;
        if (factor_ids.empty()) {
            int64_t n = 0;
            check(cx_factor_disturbance_rows_mfma(h_, 0, nullptr, &n));
            r.ids.resize((size_t)n);
            if (n) check(cx_factor_disturbance_rows_mfma(h_, n, r.ids.data(), &n));
        }
        if (rows) r.rows.resize(r.ids.size() * (size_t)(dim_ + dim_ * dim_));
        r.scores.resize(r.ids.size() * 2);
        check(cx_factor_disturbances_mfma(h_, (int64_t)factor_ids.size(), factor_ids.empty() ? nullptr : factor_ids.data(),
                                          rows && !r.rows.empty() ? r.rows.data() : nullptr, r.scores.empty() ? nullptr : r.scores.data(), &r.total,
                                          r.counts.data()));
        return r;
    }
    // the predictive score of every datum that a Gaussian rule factor generates, from the stored messages (cx_predictive): per row ŷ (d), S
    // (d x d, row-major), log density, squared standardised residual; factor_ids empty: every row in ascending factor id (`ids` names them).
    // mode CX_PREDICT_LOO: given all other data; CX_PREDICT_CAUSAL: given the data of the inputs' ancestors (a chain: the Kalman innovations,
    // total = log_evidence).  counts: rows, scored, with an undefined input, improper; total: Σ log density of the scored rows.
    // rows == false: total and counts only
    struct Predictive { std::vector<int64_t> ids; std::vector<double> rows; double total = 0; std::array<int64_t, 4> counts{}; };
    Predictive predictive(int32_t mode, const std::vector<int64_t> &factor_ids = {}, bool rows = true) {
        Predictive r;
        r.ids = factor_ids;
        const int64_t *ids = factor_ids.empty() ? nullptr : factor_ids.data();
        if (rows && factor_ids.empty()) {
            int64_t n = 0;
            check(cx_predictive_rows(h_, 0, nullptr, &n));
            r.ids.resize((size_t)n);
            if (n) check(cx_predictive_rows(h_, n, r.ids.data(), &n));
        }
        if (rows) r.rows.resize(r.ids.size() * (size_t)(dim_ + dim_ * dim_ + 2));
        check(cx_predictive(h_, mode, (int64_t)factor_ids.size(), ids, rows && !r.rows.empty() ? r.rows.data() : nullptr, &r.total, r.counts.data()));
        return r;
    }
    // the same at the matrix-core dims, 5 .. 64 (cx_predictive_mfma): one wave per row on the f64 matrix cores; a row is a two-variable
    // CX_FACTOR_GAUSS_LINEAR factor whose OUT end alone is observed, its d + d² + 2 doubles in the caller's dim
    Predictive predictive_mfma(int32_t mode, const std::vector<int64_t> &factor_ids = {}, bool rows = true) {
        Predictive r;
        r.ids = factor_ids;
        const int64_t *ids = factor_ids.empty() ? nullptr : factor_ids.data();
        if (rows && factor_ids.empty()) {
            int64_t n = 0;
            check(cx_predictive_rows_mfma(h_, 0, nullptr, &n));
            r.ids.resize((size_t)n);
            if (n) check(cx_predictive_rows_mfma(h_, n, r.ids.data(), &n));
        }
        if (rows) r.rows.resize(r.ids.size() * (size_t)(dim_ + dim_ * dim_ + 2));
        check(cx_predictive_mfma(h_, mode, (int64_t)factor_ids.size(), ids, rows && !r.rows.empty() ? r.rows.data() : nullptr, &r.total, r.counts.data()));
        return r;
    }
    // the causal estimates of the states beside the smoothed marginals, from the stored messages (cx_causal_marginals): per row the mean (d)
    // then the covariance (d x d, row-major); variable_ids empty: every variable in ascending id.  mode CX_CAUSAL_PREDICTED: p(x_t | y_<t);
    // CX_CAUSAL_FILTERED: p(x_t | y_<=t), with lag L > 0 the fixed-lag smoother p(x_t | y_<=t+L).  counts: rows, finite, with an undefined
    // input, improper (NaN rows)
    struct CausalMarginals { std::vector<double> rows; std::array<int64_t, 4> counts{}; };
    CausalMarginals causal_marginals(int32_t mode, int32_t lag = 0, const std::vector<int64_t> &variable_ids = {}) {
        const int64_t n = variable_ids.empty() ? stats().n_variables : (int64_t)variable_ids.size();
        CausalMarginals r;
        r.rows.resize((size_t)n * (size_t)(dim_ + dim_ * dim_) + 1);      // (+ 1: never a NULL out)
        check(cx_causal_marginals(h_, mode, lag, (int64_t)variable_ids.size(), variable_ids.empty() ? nullptr : variable_ids.data(), r.rows.data(),
                                  r.counts.data()));
        r.rows.resize((size_t)n * (size_t)(dim_ + dim_ * dim_));
        return r;
    }
    // the same at the matrix-core dims, 5 .. 64 (cx_causal_marginals_mfma): one wave per row on the f64 matrix cores, rows of d + d² doubles
    // in the caller's dim; a lag L adds L launches over every transition with two free ends and, on its first use, the β workspace
    CausalMarginals causal_marginals_mfma(int32_t mode, int32_t lag = 0, const std::vector<int64_t> &variable_ids = {}) {
        const int64_t n = variable_ids.empty() ? stats().n_variables : (int64_t)variable_ids.size();
        CausalMarginals r;
        r.rows.resize((size_t)n * (size_t)(dim_ + dim_ * dim_) + 1);      // (+ 1: never a NULL out)
        check(cx_causal_marginals_mfma(h_, mode, lag, (int64_t)variable_ids.size(), variable_ids.empty() ? nullptr : variable_ids.data(), r.rows.data(),
                                       r.counts.data()));
        r.rows.resize((size_t)n * (size_t)(dim_ + dim_ * dim_));
        return r;
    }
    // joint posterior draws on a forest (the simulation smoother): n_samples x n x dim doubles for variable_ids (empty: every variable in
    // ascending id); noise (optional): the standard normals, n_samples x n_variables x dim in ascending id order, in place of the device's
    // Philox4x32-10 draws.  counts: free variables, components, components with an undefined input, components not positive definite
    std::pair<std::vector<double>, std::array<int64_t, 4>> sample_posterior(int64_t n_samples, uint64_t seed, const std::vector<int64_t> &variable_ids,
                                                                            const std::vector<double> *noise = nullptr) {
        const int64_t nv = stats().n_variables, n = variable_ids.empty() ? nv : (int64_t)variable_ids.size();
        if (noise) need(noise->size(), (size_t)(n_samples * nv * dim_), "sample_posterior noise");
        std::vector<double> out((size_t)((n_samples > 0 ? n_samples : 0) * n * dim_));
        std::array<int64_t, 4> o{};
        check(cx_sample_posterior(h_, n_samples, seed, noise ? noise->data() : nullptr, n, variable_ids.empty() ? nullptr : variable_ids.data(),
                                  out.data(), o.data()));
        return {out, o};
    }
    // the same at the matrix-core dims, 5 .. 64 (cx_sample_posterior_mfma): the links of the forest on the f64 matrix cores, the samples in
    // panels of 16 through a blocked scan; dim is the caller's, the padding of an embedded dim never shows
    std::pair<std::vector<double>, std::array<int64_t, 4>> sample_posterior_mfma(int64_t n_samples, uint64_t seed, const std::vector<int64_t> &variable_ids,
                                                                                 const std::vector<double> *noise = nullptr) {
        const int64_t nv = stats().n_variables, n = variable_ids.empty() ? nv : (int64_t)variable_ids.size();
        if (noise) need(noise->size(), (size_t)(n_samples * nv * dim_), "sample_posterior_mfma noise");
        std::vector<double> out((size_t)((n_samples > 0 ? n_samples : 0) * n * dim_) + 1);      // (+ 1: never a NULL out)
        std::array<int64_t, 4> o{};
        check(cx_sample_posterior_mfma(h_, n_samples, seed, noise ? noise->data() : nullptr, n, variable_ids.empty() ? nullptr : variable_ids.data(),
                                       out.data(), o.data()));
        out.resize(out.size() - 1);
        return {out, o};
    }
    // exact mean (K) and covariance (K x K, row-major; want_cov == false: empty) of K linear functionals of the joint posterior of a forest
    // (cx_linear_moments), in CSR form: functional k has the entries offsets[k] .. offsets[k + 1] - 1 of variable_ids and weights (dim per
    // entry).  counts: components, failed components, functionals made NaN, non-observed variables
    struct LinearMoments { std::vector<double> mean, cov; std::array<int64_t, 4> counts{}; };
    LinearMoments linear_moments(const std::vector<int64_t> &offsets, const std::vector<int64_t> &variable_ids, const std::vector<double> &weights,
                                 bool want_cov = true) {
        need(offsets.empty() ? 0 : 1, 1, "linear_moments offsets");
        const int64_t K = (int64_t)offsets.size() - 1;
        need(weights.size(), variable_ids.size() * (size_t)dim_, "linear_moments weights");
        LinearMoments r;
        r.mean.resize((size_t)K);
        if (want_cov) r.cov.resize((size_t)(K * K));
        check(cx_linear_moments(h_, K, offsets.data(), variable_ids.data(), weights.data(), r.mean.data(), want_cov && K ? r.cov.data() : nullptr,
                                r.counts.data()));
        return r;
    }
    // the same at the matrix-core dims (cx_linear_moments_mfma; a handle created with dim 5 .. 64): the moments of the distribution
    // sample_posterior_mfma draws from, exact
    LinearMoments linear_moments_mfma(const std::vector<int64_t> &offsets, const std::vector<int64_t> &variable_ids, const std::vector<double> &weights,
                                      bool want_cov = true) {
        need(offsets.empty() ? 0 : 1, 1, "linear_moments_mfma offsets");
        const int64_t K = (int64_t)offsets.size() - 1;
        need(weights.size(), variable_ids.size() * (size_t)dim_, "linear_moments_mfma weights");
        LinearMoments r;
        r.mean.resize((size_t)K);
        if (want_cov) r.cov.resize((size_t)(K * K));
        check(cx_linear_moments_mfma(h_, K, offsets.data(), variable_ids.data(), weights.data(), r.mean.data(), want_cov && K ? r.cov.data() : nullptr,
                                     r.counts.data()));
        return r;
    }
    std::pair<int32_t, double> sweep_until(double tol, int32_t max_sweeps, int32_t check_every = 10) {
        int32_t n = 0; double r = 0;
        check(cx_sweep_until(h_, tol, max_sweeps, check_every, &n, &r));
        return {n, r};
    }
    void sync() { check(cx_sync(h_)); }
    void set_stream(void *hip_stream) { check(cx_set_stream(h_, hip_stream)); }

    // variational families
    void set_marginals(const std::vector<int64_t> &variable_ids, int32_t form, const std::vector<double> &payload) {
        need(payload.size(), variable_ids.size() * (form == CX_FORM_POINT ? 1u : 2u), "set_marginals payload");
        check(cx_set_marginals(h_, (int64_t)variable_ids.size(), variable_ids.data(), form, payload.data()));
    }
    void update_marginals(const std::vector<int64_t> &variable_ids) { check(cx_update_marginals(h_, (int64_t)variable_ids.size(), variable_ids.data())); }
    void update_marginals_of_class(int64_t which /* CX_VMP_ALL_NORMAL | CX_VMP_ALL_PRECISION */) { check(cx_update_marginals(h_, which, nullptr)); }

    // checkpoint
    std::vector<unsigned char> export_state() {
        int64_t n = 0;
        check(cx_state_bytes(h_, &n));
        std::vector<unsigned char> blob((size_t)n);
        check(cx_state_export(h_, blob.data(), n));
        return blob;
    }
    void import_state(const std::vector<unsigned char> &blob) { check(cx_state_import(h_, blob.data(), (int64_t)blob.size())); }

    // partitions (one process per GPU): deep halo and per-sweep message halo
    void halo_configure_state(const std::vector<int64_t> &sv, const std::vector<int64_t> &sf, const std::vector<int64_t> &rv, const std::vector<int64_t> &rf) {
        check(cx_halo_configure_state(h_, (int64_t)sv.size(), sv.data(), sf.data(), (int64_t)rv.size(), rv.data(), rf.data()));
    }
    void halo_configure(const std::vector<int64_t> &sv, const std::vector<int64_t> &sf, const std::vector<int64_t> &rv, const std::vector<int64_t> &rf) {
        check(cx_halo_configure(h_, (int64_t)sv.size(), sv.data(), sf.data(), (int64_t)rv.size(), rv.data(), rf.data()));
    }
    void halo_peers(const std::vector<int32_t> &rank, const std::vector<int64_t> &send_off, const std::vector<int64_t> &send_count,
                    const std::vector<int64_t> &recv_off, const std::vector<int64_t> &recv_count) {
        check(cx_halo_peers(h_, (int32_t)rank.size(), rank.data(), send_off.data(), send_count.data(), recv_off.data(), recv_count.data()));
    }
    void comm_init(int32_t world, int32_t rank, const void *id128) { check(cx_comm_init(h_, world, rank, id128)); }
    void halo_state_exchange() { check(cx_halo_state_exchange(h_)); }
    void halo_exchange_sweep(int n_sweeps) { check(cx_halo_exchange_sweep(h_, n_sweeps)); }
    void halo_ipc_exchange() { check(cx_halo_ipc_exchange(h_)); }
    void halo_ipc_exchange_sweep(int n_sweeps) { check(cx_halo_ipc_exchange_sweep(h_, n_sweeps)); }
    void sweep_exchange(int32_t n = 1) { check(cx_sweep_exchange(h_, n)); }

  private:
    void check(int32_t rc) const { if (rc != CX_OK) throw Error(rc, cx_last_error(h_)); }
    static void need(size_t got, size_t want, const char *what) {
        if (got != want) throw Error(CX_ERR_INVALID_ARGUMENT, std::string(what) + ": " + std::to_string(got) + " doubles, expected " + std::to_string(want));
    }
    cx_handle *h_ = nullptr;
    int32_t dim_ = 1;
};

// The sum-product processor.  A host scheduler (the reference's update_marginals! loop, or any restatement of it) calls
// process() where the reference calls process!(processor, engine, variable_id, signal); signals that are mutually independent
// may be enqueued together and computed by one flush().
class HipProcessor {
  public:
    explicit HipProcessor(Handle &h) : h_(h) {}
    void process(int32_t kind /* CX_ITEM_* */, int64_t variable_id, int64_t factor_id = 0) {
        cx_item it{};
        it.kind = kind; it.variable_id = variable_id; it.factor_id = factor_id;
        queue_.push_back(it);
    }
    size_t pending() const { return queue_.size(); }
    void flush() {
        if (queue_.empty()) return;
        std::vector<cx_item> q;
        q.swap(queue_);          // the queue is empty again even if the batch fails
        h_.update_batch(q);
        launches_++;
    }
    // update_marginals!(engine, ids) as a whole-call override: n_sweeps passes of the device schedule, then the marginals
    std::vector<double> update_marginals(const std::vector<int64_t> &variable_ids, int32_t n_sweeps = 1) {
        flush();
        h_.sweep(n_sweeps);
        // the sweep writes the marginals of the messages it STARTED from; refresh the requested ones from what it produced
        for (int64_t v : variable_ids) process(CX_ITEM_INDIVIDUAL_MARGINAL, v);
        flush();
        return h_.get_marginals(variable_ids);
    }
    int64_t launches() const { return launches_; }

  private:
    Handle &h_;
    std::vector<cx_item> queue_;
    int64_t launches_ = 0;
};

// The variational families: the state is the set of marginals.
class VmpProcessor {
  public:
    explicit VmpProcessor(Handle &h) : h_(h) {}
    void observe(int64_t variable_id, double y) { h_.set_marginals({variable_id}, CX_FORM_POINT, {y}); }
    void set_normal(int64_t variable_id, double mean, double precision) { h_.set_marginals({variable_id}, CX_FORM_MEAN_PRECISION, {mean, precision}); }
    void set_gamma(int64_t variable_id, double shape, double scale) { h_.set_marginals({variable_id}, CX_FORM_GAMMA, {shape, scale}); }
    void update_marginals(const std::vector<int64_t> &variable_ids) { h_.update_marginals(variable_ids); }
    std::vector<double> marginals(const std::vector<int64_t> &variable_ids) const { return h_.get_marginals(variable_ids); }

  private:
    Handle &h_;
};

}  // namespace cortex
