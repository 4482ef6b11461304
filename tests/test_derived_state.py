"""csrc/cx_derived.h on the CPU: what each change to a handle voids, per dimension class.

EXPECTED is the dependency graph written out: for every change and every dimension class (1, 2..4, matrix cores) the flags that move when
cxh::changed runs on a handle with nothing due.  It was transcribed from the assignments that stood at the top of the API entries before the
header existed (one line of provenance per change below); entries marked FIX are flags a sibling path had forgotten although the flag has a
reader in that configuration.  An edit of the switch has to edit this table too.

NEEDS is the other direction, and the guard for the next cache: for every derived item, the changes it depends on according to its reader
("What a change voids").  No change may leave clean an item that depends on it."""
import pytest

from tests import hostlogic as H

DIMS = {"scalar": 1, "small": 3, "mfma": 64}
ALL = tuple(DIMS)


def moved(*flags, only=ALL):
    return {c: set(flags) if c in only else set() for c in ALL}


def merge(*parts):
    return {c: set().union(*(p[c] for p in parts)) for c in ALL}


EXPECTED = {
    # cx_set_messages, CX_TO_VARIABLE: its first line raised both at every dim
    "StoredToVariable": moved("chain_side_dirty", "offchain_marg_dirty"),
    # cx_set_messages, CX_TO_FACTOR: the first line (chain_side_dirty); mv_set_messages (observed_passes_due); mv64_set_messages (point64_dirty)
    "StoredToFactor": merge(moved("chain_side_dirty"), moved("observed_passes_due", only=("small",)), moved("point64_dirty", only=("mfma",))),
    # the three clamp loops: scalar (vinfo_epoch, chains, tree, offchain), dim 2..4 (chains, tree, spdir), matrix cores (work64, chains, tree);
    # FIX: vinfo_epoch at dim > 1 — cx_api_ref.hip: ref_sweep_all caches "every free variable" under it at every dim
    "NewlyObserved": merge(moved("chains_dirty", "tree_dirty", "vinfo_epoch"), moved("offchain_marg_dirty", only=("scalar",)),
                           moved("spdir_dirty", only=("small",)), moved("work64_dirty", only=("mfma",))),
    # cx_set_factor_matrices + upload_ptab (pot64_fresh: read by the matrix-core chain scan alone, written false at every dim > 1 before)
    "RuleMatrices": merge(moved("param_epoch", "observed_passes_due", "kary_dirty", "point64_dirty", "chain_side_dirty"), moved("pot64_fresh", only=("mfma",))),
    # cx_set_factor_coefficients
    "RuleCoefficients": moved("param_epoch", "kary_dirty", "chain_side_dirty", "offchain_marg_dirty"),
    # cx_set_factor_edge_sets
    "RuleEdgeSets": moved("param_epoch", "kary_dirty", "tree_dirty"),
    # cx_halo_configure; FIX: cx_halo_configure_state when it takes stand-ins away (cx_api_sweep.hip: build_tree reads kGhost through the plan)
    "GhostSet": moved("chains_dirty", "tree_dirty"),
    # cx_halo_configure, the time-block branch
    "ChainBlock": moved("spdir_dirty", "work64_dirty"),
    # cx_seed_messages
    "Seeded": merge(moved("chain_side_dirty", "offchain_marg_dirty"), moved("pot64_fresh", only=("mfma",))),
    # update_batch's first line; mv_update_batch (pot64_fresh at its top, point64_dirty behind its matrix-core launches)
    "BatchWrote": merge(moved("chain_side_dirty", "offchain_marg_dirty"), moved("point64_dirty", "pot64_fresh", only=("mfma",))),
    # the end of ref_sweep
    "ForeignSweepRan": moved("point64_dirty", "pot64_fresh", only=("mfma",)),
    # cx_state_import: its first line, the vinfo section, its last lines
    "StateImported": merge(moved("vinfo_epoch", "chains_dirty", "tree_dirty", "spdir_dirty", "work64_dirty", "point64_dirty", "chain_side_dirty", "offchain_marg_dirty"),
                           moved("pot64_fresh", only=("mfma",))),
    # cx_graph_create: flatten (kary_dirty), the dim > 1 branch (spdir_dirty, upload_ptab's pot64_fresh), the scalar end (offchain_marg_dirty)
    "GraphCreated": merge(moved("kary_dirty"), moved("offchain_marg_dirty", only=("scalar",)), moved("spdir_dirty", only=("small", "mfma")),
                          moved("pot64_fresh", only=("mfma",))),
}


def test_the_table_names_every_change():
    assert set(EXPECTED) == set(H.CHANGES)
    with pytest.raises(ValueError):
        H.derived_apply(1, len(H.CHANGES))


@pytest.mark.parametrize("cls", ALL)
@pytest.mark.parametrize("change", H.CHANGES)
def test_each_change_moves_exactly_the_flags_of_the_table(change, cls):
    after = H.derived_apply(DIMS[cls], change)
    got = {f for f in H.DERIVED_FLAGS if after[f] != H.DERIVED_CLEAN[f]}
    assert got == EXPECTED[change][cls], f"{change} on a {cls} handle"
    # what "moved" means: a flag is raised, the passes due are 2, the block potentials no longer fresh, an epoch one further
    for f in got:
        assert after[f] == (2 if f == "observed_passes_due" else 0 if f == "pot64_fresh" else 1), f"{change}: {f}"


def test_a_change_only_ever_raises():
    """on a handle with everything due already, no change takes anything back (the clears belong to whoever rebuilds)"""
    due = {**{f: 1 for f in H.DERIVED_FLAGS}, "observed_passes_due": 2, "pot64_fresh": 0, "vinfo_epoch": 7, "param_epoch": 7}
    for change in H.CHANGES:
        for cls in ALL:
            after = H.derived_apply(DIMS[cls], change, due)
            for f in H.DERIVED_FLAGS:
                assert after[f] >= due[f] if f != "pot64_fresh" else after[f] == 0, f"{change} on a {cls} handle: {f}"


# derived item -> (its flag, the dimension classes in which it has a reader, the changes it depends on): DESIGN.md §2's table, by reader
NEEDS = {
    "chains (build_chains)": ("chains_dirty", ALL, ("NewlyObserved", "GhostSet", "StateImported")),
    "tree plan (build_tree)": ("tree_dirty", ALL, ("NewlyObserved", "GhostSet", "StateImported", "RuleEdgeSets")),
    "rule masks (mv_refresh_spdir)": ("spdir_dirty", ("small",), ("NewlyObserved", "ChainBlock", "StateImported", "GraphCreated")),
    "work lists (build_work64)": ("work64_dirty", ("mfma",), ("NewlyObserved", "ChainBlock", "StateImported")),
    "constant messages, matrix cores (k_point64)": ("point64_dirty", ("mfma",), ("StoredToFactor", "RuleMatrices", "BatchWrote", "ForeignSweepRan", "StateImported")),
    "constant messages, dim 2..4 (observed passes)": ("observed_passes_due", ("small",), ("StoredToFactor", "RuleMatrices")),
    "k-ary tables (kary_upload)": ("kary_dirty", ("scalar", "small"), ("RuleMatrices", "RuleCoefficients", "RuleEdgeSets", "GraphCreated")),
    "side sums (chain scan)": ("chain_side_dirty", ("scalar", "small"), ("StoredToVariable", "StoredToFactor", "RuleMatrices", "RuleCoefficients", "Seeded", "BatchWrote", "StateImported")),
    "off-chain marginals (sweep_main)": ("offchain_marg_dirty", ("scalar",), ("StoredToVariable", "NewlyObserved", "RuleCoefficients", "Seeded", "BatchWrote", "GraphCreated")),
    "block potentials (chain64_sweep)": ("pot64_fresh", ("mfma",), ("RuleMatrices", "Seeded", "BatchWrote", "ForeignSweepRan", "StateImported")),
    "every-free-variable request (ref_sweep_all)": ("vinfo_epoch", ALL, ("NewlyObserved", "StateImported")),
    "parameter part of the evidence and learn caches": ("param_epoch", ALL, ("RuleMatrices", "RuleCoefficients", "RuleEdgeSets")),
}
# entries that exist at some dims only: dim 1 has no rule matrices and no edge sets, dim > 1 no coefficients, the matrix cores no k-ary factors
NO_ENTRY = {"scalar": {"RuleMatrices", "RuleEdgeSets", "ChainBlock"}, "small": {"RuleCoefficients"}, "mfma": {"RuleCoefficients", "RuleEdgeSets"}}


def test_no_change_leaves_clean_what_depends_on_it():
    assert {flag for flag, _, _ in NEEDS.values()} <= set(H.DERIVED_FLAGS)
    for item, (flag, classes, changes) in NEEDS.items():
        assert set(changes) <= set(H.CHANGES), item
        for change in changes:
            for cls in classes:
                if change in NO_ENTRY[cls]:
                    continue
                after = H.derived_apply(DIMS[cls], change)
                assert after[flag] != H.DERIVED_CLEAN[flag], f"{item} depends on {change}, which leaves {flag} clean on a {cls} handle"
