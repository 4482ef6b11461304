"""Parameter learning for linear-Gaussian models on the device: the M-step of EM (Shumway–Stoffer) from the residual statistics of
DeviceGraph.factor_statistics (cx_factor_statistics), and an EM loop for dim 2..4 parameter sets.  numpy only.  DESIGN.md §4f.

The statistics are in residual coordinates r = x_out - A x_in - b of the CURRENT parameters, so the update is a correction:

    ΔA = S_rx S_xx⁻¹,   A' = A + ΔA,   Q' = (S_rr - ΔA S_rx') / n          (b learned too: regress r on [x_in, 1])

Nothing of the size of the raw second moments is cancelled: a Q-only update Q' = S_rr / n is a plain average of noise-sized terms.
"""
from __future__ import annotations

import warnings

import numpy as np

from . import _lib as L


def _sym_pd(Q, what="Q"):
    Q = 0.5 * (Q + Q.T)
    try:
        np.linalg.cholesky(Q)
    except np.linalg.LinAlgError:
        raise ValueError(f"m_step: the new {what} is not positive definite") from None
    return Q


def m_step(stats, A, b=None, learn=("A", "Q")):
    """New parameters of one group from its residual statistics.

    stats: one group's entries, {"n", "sum_r" [d], "sum_x" [d], "S_rr", "S_rx", "S_xx" [d, d]} (index the arrays of
    DeviceGraph.factor_statistics with the group, or pass them as they are when there is one group).  A, b: the parameters the
    statistics were taken under (b None: 0).  learn: any of "A", "b", "Q".  Returns {"A", "b", "Q"}: A and b as given where not
    learned; Q None where not learned (the caller keeps its own), else symmetrised and checked positive definite."""
    d = np.asarray(stats["S_rr"]).reshape(-1).size
    d = int(round(np.sqrt(d)))
    n = float(np.asarray(stats["n"]).reshape(-1)[0])
    if not n > 0:
        raise ValueError("m_step: the group has no factors")
    sr = np.asarray(stats["sum_r"], float).reshape(d)
    sx = np.asarray(stats["sum_x"], float).reshape(d)
    Srr = np.asarray(stats["S_rr"], float).reshape(d, d)
    Srx = np.asarray(stats["S_rx"], float).reshape(d, d)
    Sxx = np.asarray(stats["S_xx"], float).reshape(d, d)
    if not (np.isfinite(Srr).all() and np.isfinite(Srx).all() and np.isfinite(Sxx).all()):
        raise ValueError("m_step: the statistics are NaN (an undefined input or a belief that is not positive definite)")
    A = np.asarray(A, float).reshape(d, d)
    b = np.zeros(d) if b is None else np.asarray(b, float).reshape(d)
    learn = set(learn)
    if not learn <= {"A", "b", "Q"}:
        raise ValueError(f"m_step: unknown entries in learn: {sorted(learn - {'A', 'b', 'Q'})}")
    if "A" in learn and "b" in learn:
        # r ≈ [ΔA Δb] z, z = [x_in; 1]
        Srz = np.hstack([Srx, sr[:, None]])
        Szz = np.block([[Sxx, sx[:, None]], [sx[None, :], np.array([[n]])]])
        D = np.linalg.solve(Szz, Srz.T).T
        dA, db = D[:, :d], D[:, d]
        corr = D @ Srz.T
    elif "A" in learn:
        dA, db = np.linalg.solve(Sxx, Srx.T).T, np.zeros(d)
        corr = dA @ Srx.T
    elif "b" in learn:
        dA, db = np.zeros((d, d)), sr / n
        corr = np.outer(db, sr)
    else:
        dA, db, corr = np.zeros((d, d)), np.zeros(d), np.zeros((d, d))
    Q = _sym_pd((Srr - corr) / n) if "Q" in learn else None
    return {"A": A + dA, "b": b + db, "Q": Q}


def group(stats, g):
    """the entries of group g of DeviceGraph.factor_statistics' first result"""
    return {k: np.asarray(v)[g] for k, v in stats.items()}


def auxiliary_residuals(dist, Q):
    """The auxiliary residuals of the disturbance smoother (Durbin and Koopman) from DeviceGraph.factor_disturbances_mfma's rows:
    z = E[w | data] / sqrt(diag(Var(E[w | data]))), and Var(E[w | data]) = Q - Cov(w | data), so z = mean / sqrt(diag(Q - cov)), [n, d].
    Under the model every entry is standard normal: a large one on a likelihood factor marks an outlier, on a transition a structural
    break.  dist: the dict (with "mean" and "cov"); Q: [d, d], or [n, d, d] with the Q of every row.  z is NaN where
    diag(Q - cov) <= 64 d ε diag(Q): such a factor tells nothing about its disturbance (Cov(w | data) = Q: a forecast's transitions, the
    factor behind missing data) and the quotient would be rounding over rounding — the flat-pivot factor of the readers at these dims."""
    mean, cov = np.asarray(dist["mean"], float), np.asarray(dist["cov"], float)
    n, d = mean.shape
    Qd = np.broadcast_to(np.diagonal(np.asarray(Q, float), axis1=-2, axis2=-1), (n, d))
    v = Qd - np.diagonal(cov, axis1=1, axis2=2)
    ok = v > 64.0 * d * np.finfo(np.float64).eps * Qd
    return np.where(ok, mean / np.sqrt(np.where(ok, v, 1.0)), np.nan)


def em(dev, sets, n_iter, sweeps_per_iter=1, learn=("A", "Q"), offsets=None, by_component=False):
    """EM on the parameter sets of a dim 2..4 DeviceGraph: per iteration sweep(sweeps_per_iter) → log_evidence → factor_statistics
    (one group per parameter set) → m_step → set_factor_matrices.  On a handle of dim 5..64 the same loop runs on log_evidence_mfma and
    factor_statistics_mfma; offsets= and by_component=True raise ValueError there (multi_start_em is the way to run several starts in
    one handle at these dims: it uses log_evidence_components_mfma).

    sets: {set: (A, Q)}, the starting parameters (set on the handle here).  learn: a tuple for every set, or {set: tuple}.
    Returns (trace, params): trace[i] = log p(data) under the parameters of iteration i (n_iter + 1 values, the last under the final
    parameters) and params = {set: (A, Q)}.

    offsets: None, or {set: b}: every two-variable CX_FACTOR_GAUSS_LINEAR factor of that set starts at x_out = A x_in + b + N(0, Q)
    (DeviceGraph.set_factor_offsets; the factor → set map is what graph_create was given) and "b" may be learned for it: one b per set,
    applied after each M-step beside (A, Q).  Then returns (trace, params, offsets) with offsets = {set: b}.

    by_component=True: the trace is an array [n_iter + 1, C], row i = DeviceGraph.log_evidence_components under the parameters of
    iteration i, one column per connected component.  On a synth.replicas graph (replica k's sets are k * S + s) this is multi-start EM
    in one handle: the statistics are grouped by set, so every replica is updated from its own, and its column is its own trace.

    The log-evidence trace is non-decreasing only where the E-step is exact: a chain-scan or tree sweep, or one reference-order
    call, on a forest.  Fused / flooding sweeps give Bethe beliefs (exact on forests only once converged) and loops give Bethe
    statistics: the iteration is then a generalised EM without that guarantee."""
    if dev.dim < 2:
        raise ValueError("em: dim 2..4 (dim 1 has per-factor parameters: call factor_statistics with explicit groups and m_step)")
    mfma = dev.dim >= 5      # the matrix-core dims: log_evidence_mfma and factor_statistics_mfma
    if mfma and offsets is not None:
        raise ValueError("em: offsets= at dim 5..64: em_mfma takes them (set_factor_offsets is dim 2..4, set_factor_offsets_mfma dim 5..64)")
    if mfma and by_component:
        raise ValueError("em: by_component=True at dim 5..64: log_evidence_components does not exist at these dims (log_evidence_mfma gives the total)")
    params = {int(s): (np.array(A, float), np.array(Q, float)) for s, (A, Q) in sets.items()}
    for s, (A, Q) in params.items():
        dev.set_factor_matrices(s, A, Q)
    offs, facs = None, {}
    if offsets is not None:
        offs = {int(s): np.array(b, float).reshape(dev.dim) for s, b in offsets.items()}
        if not set(offs) <= set(params):
            raise ValueError("em: offsets names a set that sets does not")
        for s, b in offs.items():
            facs[s] = dev.linear_factors_of_set(s)
            dev.set_factor_offsets(facs[s], np.tile(b, (len(facs[s]), 1)))
    for s in params:
        ls = learn.get(s, ("A", "Q")) if isinstance(learn, dict) else learn
        if "b" in ls and offs is not None and s not in offs:
            raise ValueError(f'em: "b" is learned for the sets that offsets names (set {s} is not one)')
    if by_component:
        evidence = lambda: dev.log_evidence_components()[0]      # noqa: E731
    else:
        evidence = lambda: (dev.log_evidence_mfma() if mfma else dev.log_evidence())[0]      # noqa: E731
    trace = _em_loop(dev, params, offs, facs, n_iter, sweeps_per_iter, learn, evidence)
    if by_component:
        trace = np.array(trace, dtype=np.float64).reshape(n_iter + 1, -1)
    if offs is not None:
        return trace, params, offs
    return trace, params


def em_mfma(dev, sets, n_iter, sweeps_per_iter=1, learn=("A", "Q"), offsets=None):
    """em for a DeviceGraph of dim 5..64: the same iterations (_em_loop) on log_evidence_mfma and factor_statistics_mfma, with per-factor
    offsets through set_factor_offsets_mfma.  sets, learn, the trace and what makes it non-decreasing: as em.

    offsets: None, or {set: b} with em's meaning — every two-variable CX_FACTOR_GAUSS_LINEAR factor of that set starts at
    x_out = A x_in + b + N(0, Q), and "b" may be learned for it, one b per set.  Always returns (trace, params, offsets); offsets is
    {set: b}, empty when none was given."""
    if dev.dim < 5:
        raise ValueError("em_mfma: dim 5..64 (dim 2..4: em)")
    params = {int(s): (np.array(A, float), np.array(Q, float)) for s, (A, Q) in sets.items()}
    for s, (A, Q) in params.items():
        dev.set_factor_matrices(s, A, Q)
    offs = {int(s): np.array(b, float).reshape(-1) * np.ones(dev.dim) for s, b in (offsets or {}).items()}
    if not set(offs) <= set(params):
        raise ValueError("em_mfma: offsets names a set that sets does not")
    facs = {}
    for s, b in offs.items():
        facs[s] = dev.linear_factors_of_set(s)
        dev.set_factor_offsets_mfma(facs[s], np.tile(b, (len(facs[s]), 1)))
    for s in params:
        ls = learn.get(s, ("A", "Q")) if isinstance(learn, dict) else learn
        if "b" in ls and s not in offs:
            raise ValueError(f'em_mfma: "b" is learned for the sets that offsets names (set {s} is not one)')
    trace = _em_loop(dev, params, offs, facs, n_iter, sweeps_per_iter, learn, lambda: dev.log_evidence_mfma()[0])
    return trace, params, offs


def _em_loop(dev, params, offs, facs, n_iter, sweeps_per_iter, learn, evidence):
    """The iterations of em, em_mfma and multi_start_em on a handle that holds the starting parameters: sweep → evidence() (the trace's
    row) → factor_statistics (factor_statistics_mfma at dim 5..64), one group per parameter set → m_step → set_factor_matrices (and the
    offsets of the sets in offs, by the setter of the handle's dim).  params and offs are updated in place; returns the n_iter + 1 rows."""
    if dev.schedule not in (L.SCHED_CHAIN_SCAN, L.SCHED_TREE, L.SCHED_REFERENCE):
        warnings.warn("em: the log-evidence is guaranteed non-decreasing only under an exact E-step (chain scan, tree, reference order on "
                      "a forest)", RuntimeWarning, stacklevel=3)
    statistics = dev.factor_statistics_mfma if dev.dim >= 5 else dev.factor_statistics
    set_offsets = dev.set_factor_offsets_mfma if dev.dim >= 5 else dev.set_factor_offsets
    n_groups = max(params) + 1
    trace = []
    for it in range(n_iter + 1):
        dev.sweep(sweeps_per_iter)
        trace.append(evidence())
        if it == n_iter:
            break
        stats, _ = statistics(n_groups=n_groups)
        for s, (A, Q) in params.items():
            ls = learn.get(s, ("A", "Q")) if isinstance(learn, dict) else learn
            if not ls:
                continue
            new = m_step(group(stats, s), A, b=None if offs is None else offs.get(s), learn=ls)
            params[s] = (new["A"], Q if new["Q"] is None else new["Q"])
            dev.set_factor_matrices(s, *params[s])
            if offs is not None and s in offs:
                offs[s] = new["b"]
                set_offsets(facs[s], np.tile(offs[s], (len(facs[s]), 1)))
    return trace


def multi_start_em(model, starts, n_iter, learn=("A", "Q"), schedule=L.SCHED_CHAIN_SCAN, sweeps_per_iter=1):
    """EM on one dim 2..64 model from K starting points at once: K replicas of the model as one graph (synth.replicas) in a handle of
    its own, replica k under starts[k] = {set: (A, Q)} (a set a start does not name begins at model.psets), em's iterations with the
    log-evidence per connected component (log_evidence_components, log_evidence_components_mfma at dim 5..64) as the trace.  The
    statistics are grouped by parameter set and replica k's sets are k * S + s, so every start is updated from its own statistics:
    the K runs do not interact and each column is the trace that em gives from that start alone.
    learn: a tuple for every set, or {set: tuple} in the MODEL's set numbers (the same for every start).  schedule: an exact one for
    the model (SCHED_CHAIN_SCAN on chains, SCHED_TREE on forests).
    Returns (trace [n_iter + 1, K], params, best): params[k] = {set: (A, Q)} of start k in the model's set numbers, best = the argmax
    of the last row of the trace (a start whose component read an undefined input or a belief that is not positive definite has NaN
    there and is never the best)."""
    from . import synth
    from .device import DeviceGraph

    starts = [{int(s): AQ for s, AQ in st.items()} for st in starts]
    rep = synth.replicas(model, starts)
    S, K = rep.meta["S"], len(starts)
    if isinstance(learn, dict):
        learn = {k * S + int(s): tuple(learn.get(int(s), ("A", "Q"))) for k in range(K) for s in model.psets}
    dev = DeviceGraph(dim=model.dim, schedule=schedule)
    try:
        synth.load_into_device(rep, dev)
        components = dev.log_evidence_components_mfma if dev.dim >= 5 else dev.log_evidence_components
        if dev.components()[1] != K:
            raise ValueError("multi_start_em: the model is not one connected component (its replicas are not the components of the graph)")
        params = {int(s): (np.array(A, float), np.array(Q, float)) for s, (A, Q) in rep.psets.items()}
        for s, (A, Q) in params.items():
            dev.set_factor_matrices(s, A, Q)
        trace = _em_loop(dev, params, None, {}, n_iter, sweeps_per_iter, learn, lambda: components()[0])
    finally:
        dev.close()
    trace = np.array(trace, dtype=np.float64).reshape(n_iter + 1, K)
    last = np.where(np.isnan(trace[-1]), -np.inf, trace[-1])
    return trace, [{int(s): params[k * S + int(s)] for s in model.psets} for k in range(K)], int(np.argmax(last))


def profile(model, candidates, schedule=L.SCHED_TREE):
    """The log-likelihood of one dim 2..64 model under K candidate parameter sets from ONE handle and one exact sweep: K replicas of the
    model as one graph (synth.replicas), one component each.  candidates: a list of {set: (A, Q)}; a set a candidate does not name
    falls back to model.psets.  schedule: an exact one for the model (SCHED_TREE, or SCHED_CHAIN_SCAN on chains).
    Returns (loglik [K], comp_counts [K, 4]) of DeviceGraph.log_evidence_components: loglik[k] = log p(data | candidate k), NaN when
    that replica read an undefined message or a belief that is not positive definite (comp_counts[k, 2:]).  A model of dim 5..64 goes
    through log_evidence_components_mfma."""
    from . import synth
    from .device import DeviceGraph

    rep = synth.replicas(model, list(candidates))
    dev = DeviceGraph(dim=model.dim, schedule=schedule)
    try:
        synth.load_into_device(rep, dev)
        dev.sweep(1)
        values, comp_counts, _ = dev.log_evidence_components_mfma() if model.dim >= 5 else dev.log_evidence_components()
    finally:
        dev.close()
    if len(values) != len(rep.meta["replica_offset"]):
        raise ValueError("profile: the model is not one connected component (its replicas are not the components of the graph)")
    return values, comp_counts
