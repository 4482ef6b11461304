// cx_derived.h — what a caller's change voids.  A handle caches state derived from other state (chains, tree plan, rule masks, work
// lists, constant messages, side sums, off-chain marginals, request lists, the parameter part of the evidence / learn caches); each
// piece has a flag or an epoch that says it is due.  The rule ("What a change voids"): an API entry that changes X calls
// changed(h, X) — here, and nowhere else, is written which flags X raises; whoever rebuilds Y clears Y's flag where it rebuilds.
// Pure host C++ over any struct H that carries the flags by cx_handle's names (cx_hostlogic.cpp instantiates it on a plain one).
#pragma once

#include "cx_const.h"

namespace cxh {

enum class Change : int32_t {
    StoredToVariable = 0,   // cx_set_messages wrote factor→variable messages (priors, cut messages)
    StoredToFactor,         // cx_set_messages wrote variable→factor messages: data, new data of an observed variable included
    NewlyObserved,          // ... and CX_FORM_POINT data reached a variable that was free (mark_observed): issued after StoredToFactor
    RuleMatrices,           // cx_set_factor_matrices (dim > 1)
    RuleCoefficients,       // cx_set_factor_coefficients (dim 1)
    RuleEdgeSets,           // cx_set_factor_edge_sets (dim 2..4)
    GhostSet,               // cx_halo_configure / cx_halo_configure_state changed which variables are stand-ins
    ChainBlock,             // ... and the handle became a time block of a partitioned chain (dim > 1, chain scan): issued after GhostSet
    Seeded,                 // cx_seed_messages overwrote every stored message of one direction
    BatchWrote,             // cx_update_batch computed and stored the messages / marginals its items name
    ForeignSweepRan,        // a reference-order call ran: messages changed behind the back of the other schedules' constants
    StateImported,          // cx_state_import: messages, marginals and the observed flags are another handle's
    GraphCreated,           // cx_graph_create flattened a graph into the handle
    RuleOffsets,            // cx_set_factor_offsets (dim 2..4), cx_set_factor_offsets_mfma (dim 5..64)
    kCount
};

template <class H>
void changed(H &h, Change c) {
    const bool scalar = h.cfg.dim == 1, mfma = cx::is_mfma_dim(h.cfg.dim);
    // the paired sweep (cx_sweep_pair.hip) relies on every variable being free, every stored message defined and the unary messages being
    // the same in both Jacobi buffers: whatever sets messages or data, or changes which variables are observed or stand-ins, makes
    // the check due again.  Rule parameters are read by the launch itself: they void nothing.
    switch (c) {
    case Change::RuleMatrices: case Change::RuleCoefficients: case Change::RuleEdgeSets: case Change::RuleOffsets: case Change::ChainBlock: case Change::kCount: break;
    default: h.pair_check_due = true; break;
    }
    // the slot classes and the transition list of cx_causal_marginals (cx_causal.hip) follow the graph and WHICH variables are observed;
    // messages and rule parameters are read by every call: they void nothing
    switch (c) {
    case Change::NewlyObserved: case Change::GhostSet: case Change::StateImported: case Change::GraphCreated: h.causal_plan_dirty = true; break;
    default: break;
    }
    switch (c) {
    case Change::StoredToVariable:
        // a stored message into a chain variable is part of its side sum; marginals of variables OFF the chains (observed ones,
        // stand-ins) depend on stored factor→variable messages only.  (dim 64, pot64_fresh: by the slot list, at the call site)
        h.chain_side_dirty = true; h.offchain_marg_dirty = true;
        break;
    case Change::StoredToFactor:
        // data injection changes the chains' leaf messages but no marginal of a variable off the chains (offchain_marg_dirty stays:
        // this runs once per iteration of the wired-VMP and plug-in loops, a variable phase per call otherwise); the constant
        // messages out of the observed senders are due again in both Jacobi buffers (dim 2..4) / by k_point64 (matrix cores)
        h.chain_side_dirty = true;
        if (!scalar && !mfma) h.observed_passes_due = 2;
        if (mfma) h.point64_dirty = true;
        break;
    case Change::NewlyObserved:
        // a newly observed variable leaves the chains and the forest; rule masks (dim 2..4) and work lists (matrix cores) depend on
        // WHICH variables are observed, not on their data; the cached "every free variable" request of the reference order
        // (cx_api_ref.hip: ref_sweep_all) follows vinfo_epoch at every dim — the dim > 1 paths used to leave it: a fix
        h.chains_dirty = true; h.tree_dirty = true; h.vinfo_epoch++;
        if (scalar) h.offchain_marg_dirty = true;      // the variable is now off the chains (read by the scalar chain scan alone: sweep_main)
        else if (mfma) h.work64_dirty = true;
        else h.spdir_dirty = true;
        break;
    case Change::RuleMatrices:
        // the messages out of observed variables, N(A y, Q), are cached in both Jacobi buffers / by k_point64; factors of more than two
        // variables read the raw (A, Q); the chains' leaf messages follow the tables.  The tree plan holds table INDICES: it stays.
        // (offchain_marg_dirty: read by the scalar chain scan alone, and dim 1 has no matrices)
        h.param_epoch++;
        h.observed_passes_due = 2; h.kary_dirty = true; h.point64_dirty = true; h.chain_side_dirty = true;
        if (mfma) h.pot64_fresh = false;
        break;
    case Change::RuleCoefficients:
        // the coefficient table is uploaded again; a factor of more than two variables beside a chain feeds its side sums and the
        // marginals of the variables off it.  The scalar plans read the coefficients on the device every sweep: no plan is voided.
        h.param_epoch++;
        h.kary_dirty = true; h.chain_side_dirty = true; h.offchain_marg_dirty = true;
        break;
    case Change::RuleEdgeSets:
        // the tree plan's items carry the parameter set of the sending edge as the plan found it.  chain_side_dirty stays: the dim 2..4
        // chain scan never computes a message out of a factor of more than two variables (it is a stored message there, and whoever
        // recomputes it — cx_update_batch — raises the flag)
        h.param_epoch++;
        h.kary_dirty = true; h.tree_dirty = true;
        break;
    case Change::GhostSet:
        // stand-ins are no chain positions and no tree nodes.  (The reference order is not partitioned: vinfo_epoch has no reader here.)
        h.chains_dirty = true; h.tree_dirty = true;
        break;
    case Change::ChainBlock:
        // the rule masks and work lists of a time block treat its stand-ins as constant senders
        h.spdir_dirty = true; h.work64_dirty = true;
        break;
    case Change::Seeded:
        h.chain_side_dirty = true; h.offchain_marg_dirty = true;
        if (mfma) h.pot64_fresh = false;
        break;
    case Change::BatchWrote:
        // as a set of both directions; the matrix-core items write ONE buffer: a sweep recomputes the constant messages into both
        h.chain_side_dirty = true; h.offchain_marg_dirty = true;
        if (mfma) { h.point64_dirty = true; h.pot64_fresh = false; }
        break;
    case Change::ForeignSweepRan:
        // (as after a batch: a sweep of another schedule recomputes its constants)
        if (mfma) { h.point64_dirty = true; h.pot64_fresh = false; }
        break;
    case Change::StateImported:
        // everything derived from the observed flags or from stored messages; the marginals themselves travel in the blob, with
        // their own "off-chain marginals are due" bit, which the importer restores after this call
        h.vinfo_epoch++;
        h.chains_dirty = true; h.tree_dirty = true; h.spdir_dirty = true; h.work64_dirty = true; h.point64_dirty = true;
        h.chain_side_dirty = true; h.offchain_marg_dirty = true;
        if (mfma) h.pot64_fresh = false;
        break;
    case Change::GraphCreated:
        h.kary_dirty = true;
        if (scalar) h.offchain_marg_dirty = true; else h.spdir_dirty = true;
        if (mfma) h.pot64_fresh = false;
        break;
    case Change::RuleOffsets:
        // what RuleMatrices voids and that reads eta: the messages out of observed variables, N(A y + b, Q), cached in both Jacobi buffers;
        // the chains' leaf messages and side sums.  Precisions, k-ary tables, the tree plan and the matrix cores' state do not see b.  (The
        // linear terms themselves are rewritten by the entry, and again by cx_set_factor_matrices: they follow (A, Q) too.)
        // The matrix-core dims cache the same messages by k_point64, and a time block's potentials would hold the links' terms.
        h.param_epoch++;
        h.observed_passes_due = 2; h.chain_side_dirty = true;
        if (mfma) { h.point64_dirty = true; h.pot64_fresh = false; }
        break;
    case Change::kCount: break;
    }
}

// CX_FORM_POINT data for the variables `vars`: they are observed from now on (their messages are data, never recomputed).  Returns
// whether any of them was free until now — the caller then uploads d_vinfo and calls changed(h, Change::NewlyObserved); new data for
// variables that were observed already leaves the structure (observed flags, rule masks, chains, tiles) as it is.
template <class H>
bool mark_observed(H &h, const int32_t *vars, int64_t n) {
    bool newly = false;
    for (int64_t i = 0; i < n; i++)
        if (!(h.vinfo[vars[i]] & cx::kClamped)) { h.vinfo[vars[i]] |= cx::kClamped; newly = true; }
    return newly;
}

}  // namespace cxh
