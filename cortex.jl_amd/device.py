"""DeviceGraph — thin Python owner of a `cx_handle` (include/cortex_hip.h).

This is plumbing over the C ABI, not an algorithm: every method is one ABI call.  It is what the
host-side processor (hip_processor.py) and bench.py drive."""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _lib as L


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


class DeviceGraph:
    def __init__(self, device: int = 0, dim: int = 1, schedule: int = L.SCHED_FUSED, marginals_in_sweep: bool = True,
                 materialize_messages_to_factor: bool = False, family: int = L.FAMILY_GAUSSIAN):
        self.lib = L.load()
        self._batch_raw = None
        cfg = L.Config(C.sizeof(L.Config), device, dim, schedule, int(marginals_in_sweep),      # True/1: every sweep; 2: on demand (chain scan, dim 2..4)
                       int(materialize_messages_to_factor), int(family), 0)
        h = C.c_void_p()
        rc = self.lib.cx_create(C.byref(cfg), C.byref(h))
        if rc != L.OK:
            raise L.CortexHipError(rc, self.lib.cx_last_error(None).decode())
        self.h = h
        self.dim = dim
        self.schedule = schedule

    # -- status handling ------------------------------------------------------------------------
    def _check(self, rc: int):
        if rc != L.OK:
            raise L.CortexHipError(rc, self.lib.cx_last_error(self.h).decode())

    def last_error(self) -> str:
        """cx_last_error: the text of the handle's last refused call (what CortexHipError carries; here for a raw self.lib call)"""
        return self.lib.cx_last_error(self.h).decode()

    def close(self):
        if getattr(self, "h", None):
            self.lib.cx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- graph ----------------------------------------------------------------------------------
    def graph_create(self, edge_var, edge_fac, factor_ids, factor_kind, factor_params, edge_role=None):
        edge_var, edge_fac, factor_ids = _i64(edge_var), _i64(edge_fac), _i64(factor_ids)
        factor_kind = np.ascontiguousarray(factor_kind, dtype=np.int32)
        fp = np.zeros((len(factor_ids), L.NPARAM), dtype=np.float64)
        factor_params = np.asarray(factor_params, dtype=np.float64)
        if factor_params.ndim == 1:
            fp[:, 0] = factor_params
        else:
            fp[:, : factor_params.shape[1]] = factor_params
        role = None
        if edge_role is not None:
            role_arr = np.ascontiguousarray(edge_role, dtype=np.int32)
            role = _p(role_arr, C.c_int32)
        self._check(self.lib.cx_graph_create(self.h, len(edge_var), _p(edge_var, C.c_int64), _p(edge_fac, C.c_int64),
                                             role, len(factor_ids), _p(factor_ids, C.c_int64),
                                             _p(factor_kind, C.c_int32), _p(fp, C.c_double)))
        # kept on the host for the callers that need the factor -> parameter set map (learn.em with offsets)
        self._factor_ids, self._factor_kind, self._factor_params = factor_ids.copy(), factor_kind.copy(), fp

    def set_factor_coefficients(self, variable_ids, factor_ids, a):
        """cx_set_factor_coefficients: a_i of the ROLE_IN edges of CX_FACTOR_GAUSS_LINEAR_N factors (default 1)"""
        v, f, a = _i64(np.atleast_1d(variable_ids)), _i64(np.atleast_1d(factor_ids)), _f64(np.atleast_1d(a))
        self._check(self.lib.cx_set_factor_coefficients(self.h, len(v), _p(v, C.c_int64), _p(f, C.c_int64), _p(a, C.c_double)))

    def set_factor_matrices(self, parameter_set: int, A, Q):
        A, Q = _f64(A), _f64(Q)
        if A.shape != (self.dim, self.dim) or Q.shape != (self.dim, self.dim):
            raise ValueError(f"A and Q must be {self.dim}x{self.dim}")
        self._check(self.lib.cx_set_factor_matrices(self.h, int(parameter_set), _p(A, C.c_double), _p(Q, C.c_double)))
        self._n_sets = max(getattr(self, "_n_sets", 0), int(parameter_set) + 1)      # (the default n_groups of factor_statistics)

    def set_factor_offsets(self, factor_ids, b):
        """cx_set_factor_offsets (dim 2..4): the named two-variable CX_FACTOR_GAUSS_LINEAR factors become x_out = A x_in + b + N(0, Q);
        b: [n, dim] (or [dim] for one factor).  Factors not named keep their offset (initially 0)."""
        f = _i64(np.atleast_1d(factor_ids))
        b = _f64(b).reshape(-1, self.dim) if len(f) else _f64(np.zeros((0, self.dim)))
        if len(b) != len(f):
            raise ValueError(f"b must be [{len(f)}, {self.dim}]")
        self._check(self.lib.cx_set_factor_offsets(self.h, len(f), _p(f, C.c_int64) if len(f) else None, _p(b, C.c_double) if len(f) else None))

    def set_factor_offsets_mfma(self, factor_ids, b):
        """cx_set_factor_offsets_mfma (dim 5..64): set_factor_offsets for a handle on the matrix-core kernels; b: [n, dim] in the handle's own
        (user's) dim.  log_evidence_mfma, log_evidence_components_mfma, factor_beliefs_mfma, factor_statistics_mfma and factor_disturbances_mfma take the offsets; the
        other derived calls of these dims refuse while an offset is non-zero."""
        f = _i64(np.atleast_1d(factor_ids))
        b = _f64(b).reshape(-1, self.dim) if len(f) else _f64(np.zeros((0, self.dim)))
        if len(b) != len(f):
            raise ValueError(f"b must be [{len(f)}, {self.dim}]")
        self._check(self.lib.cx_set_factor_offsets_mfma(self.h, len(f), _p(f, C.c_int64) if len(f) else None, _p(b, C.c_double) if len(f) else None))

    def linear_factors_of_set(self, parameter_set: int):
        """the ids of the two-variable CX_FACTOR_GAUSS_LINEAR factors that name `parameter_set` (dim > 1), from what graph_create was given"""
        lin = self._factor_kind == L.FACTOR_GAUSS_LINEAR
        return self._factor_ids[lin & (self._factor_params[:, 0] == int(parameter_set))]

    def set_factor_edge_sets(self, variable_ids, factor_ids, parameter_sets):
        """cx_set_factor_edge_sets: dim 2..4, the A_i of ROLE_IN edges of CX_FACTOR_GAUSS_LINEAR_N factors by parameter set"""
        v, f, s = _i64(np.atleast_1d(variable_ids)), _i64(np.atleast_1d(factor_ids)), _i64(np.atleast_1d(parameter_sets))
        self._check(self.lib.cx_set_factor_edge_sets(self.h, len(v), _p(v, C.c_int64), _p(f, C.c_int64), _p(s, C.c_int64)))

    def stats(self) -> dict:
        s = L.Stats()
        self._check(self.lib.cx_graph_stats(self.h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in L.Stats._fields_}

    def tree_plan_stats(self):
        """cx_tree_plan_stats: the stages of the tree schedule's last sweep (zeros before it and for other schedules)"""
        out = (C.c_int64 * 8)()
        self._check(self.lib.cx_tree_plan_stats(self.h, out))
        keys = ("depth", "stages", "items", "kary_entries", "components", "messages_up", "messages_down", "marginals")
        return dict(zip(keys, [int(x) for x in out]))

    def tree_heavy_path_stats(self):
        """cx_tree_heavy_path_stats: zeros unless the tree schedule's last sweep ran over heavy paths"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.cx_tree_heavy_path_stats(self.h, out))
        return dict(zip(("light_depths", "paths", "single_variables", "launches"), [int(x) for x in out]))

    def chain_plan_stats(self):
        """cx_chain_plan_stats: the composition / walk plan of the dim 64 chain-scan schedule (zeros for other handles)"""
        out = (C.c_int64 * 8)()
        self._check(self.lib.cx_chain_plan_stats(self.h, out))
        keys = ("links_per_block", "fan", "levels", "potentials", "compositions", "rules", "launches", "device_bytes")
        return dict(zip(keys, (int(x) for x in out)))

    def chain_scan_stats(self):
        """cx_chain_scan_stats: the scalar chain scan as one launch — state (1 ready, 0 not prepared, -1 off) and how many such launches ran"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.cx_chain_scan_stats(self.h, out))
        return {"state": int(out[0]), "launches": int(out[1]), "halo_batch_graph_launches": int(out[2])}

    def sweep_stats(self):
        """cx_sweep_stats: the partner-run table's entries and how many of them fall back to the per-lane index; sweeps that stored no marginals; launches that ran two sweeps at once
        (cx_sweep_pair.hip)"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.cx_sweep_stats(self.h, out))
        return {"partner_run_entries": int(out[0]), "partner_run_fallback": int(out[1]), "sweeps_without_marginals": int(out[2]),
                "paired_launches": int(out[3])}

    def sweep_deep_stats(self):
        """cx_sweep_deep_stats: launches that ran three / four sweeps at once (cx_sweep_deep.hip; every depth: sweep_deep_launches), the depth of the last call that ran multi-sweep
        launches and the rows per segment at that depth"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.cx_sweep_deep_stats(self.h, out))
        return {"depth3_launches": int(out[0]), "depth4_launches": int(out[1]), "depth": int(out[2]), "rows": int(out[3])}

    def sweep_deep_launches(self):
        """cx_sweep_deep_launches: [d] = launches that ran d sweeps at once, d = 2 .. 6; [0] = [1] = 0"""
        out = (C.c_int64 * 7)()
        self._check(self.lib.cx_sweep_deep_launches(self.h, out))
        return tuple(int(x) for x in out)

    def edge_index(self, variable_ids, factor_ids):
        v, f = _i64(np.atleast_1d(variable_ids)), _i64(np.atleast_1d(factor_ids))
        out = np.zeros(len(v), dtype=np.int64)
        self._check(self.lib.cx_edge_index(self.h, len(v), _p(v, C.c_int64), _p(f, C.c_int64), _p(out, C.c_int64)))
        return out

    # -- data -----------------------------------------------------------------------------------
    def set_messages(self, variable_ids, factor_ids, direction: int, form: int, payload):
        v, f = _i64(np.atleast_1d(variable_ids)), _i64(np.atleast_1d(factor_ids))
        p = _f64(payload)
        need = len(v) * self.lib.cx_payload_doubles(self.dim, form)
        if p.size != need:
            raise ValueError(f"payload has {p.size} doubles, expected {need}")
        self._check(self.lib.cx_set_messages(self.h, len(v), _p(v, C.c_int64), _p(f, C.c_int64), direction, form,
                                             _p(p, C.c_double)))

    def get_messages(self, variable_ids, factor_ids, direction: int, form: int = L.FORM_MOMENT):
        v, f = _i64(np.atleast_1d(variable_ids)), _i64(np.atleast_1d(factor_ids))
        out = np.zeros((len(v), self.lib.cx_payload_doubles(self.dim, L.FORM_MOMENT)), dtype=np.float64)
        self._check(self.lib.cx_get_messages(self.h, len(v), _p(v, C.c_int64), _p(f, C.c_int64), direction, form,
                                             _p(out, C.c_double)))
        return out

    def seed_messages(self, direction: int, mean: float, variance: float):
        self._check(self.lib.cx_seed_messages(self.h, direction, float(mean), float(variance)))

    def get_marginals(self, variable_ids):
        v = _i64(np.atleast_1d(variable_ids))
        out = np.zeros((len(v), self.lib.cx_payload_doubles(self.dim, L.FORM_MOMENT)), dtype=np.float64)
        self._check(self.lib.cx_get_marginals(self.h, len(v), _p(v, C.c_int64), _p(out, C.c_double)))
        return out

    # -- compute --------------------------------------------------------------------------------
    def update_batch(self, kinds, variable_ids, factor_ids):
        n = len(kinds)
        items = (L.Item * n)()
        for i in range(n):
            items[i].kind = int(kinds[i])
            items[i].variable_id = int(variable_ids[i])
            items[i].factor_id = int(factor_ids[i])
        self._check(self.lib.cx_update_batch(self.h, items, n))

    def update_batch_packed(self, records: bytes, n: int):
        """cx_update_batch_async (small batches return when their launch is queued) with the items already packed (`struct.pack("<iiqq", kind, 0, variable_id, factor_id)` each, concatenated):
        a scheduler that launches thousands of small batches packs every signal's record once"""
        if self._batch_raw is None:
            proto = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_char_p, C.c_int64)
            self._batch_raw = proto(("cx_update_batch_async", self.lib))
        rc = self._batch_raw(self.h, records, n)
        if rc != L.OK:
            self._check(rc)

    def get_products(self, variable_ids, range_lo, range_hi, form: int = L.FORM_MOMENT):
        """stored ProductOfMessages(variable, lo:hi) values, [n, 2] (dim > 1: [n, d + d * d], as messages)"""
        v = _i64(np.atleast_1d(variable_ids))
        lo = np.ascontiguousarray(np.atleast_1d(range_lo), dtype=np.int32)
        hi = np.ascontiguousarray(np.atleast_1d(range_hi), dtype=np.int32)
        out = np.zeros((len(v), self.lib.cx_payload_doubles(self.dim, L.FORM_MOMENT) if self.dim > 1 else 2), dtype=np.float64)
        self._check(self.lib.cx_get_products(self.h, len(v), _p(v, C.c_int64), _p(lo, C.c_int32), _p(hi, C.c_int32), form,
                                             _p(out, C.c_double)))
        return out

    def get_joint_marginals(self, factor_ids):
        """stored JointMarginal(factor) values: (mean [n, 2], covariance [n, 2, 2]), variables in ascending id order"""
        f = _i64(np.atleast_1d(factor_ids))
        out = np.zeros((len(f), 6), dtype=np.float64)
        self._check(self.lib.cx_get_joint_marginals(self.h, len(f), _p(f, C.c_int64), _p(out, C.c_double)))
        return out[:, :2], out[:, 2:].reshape(-1, 2, 2)

    def sweep(self, n: int = 1):
        self._check(self.lib.cx_sweep(self.h, int(n)))

    def set_damping(self, lam: float):
        """cx_set_damping: new = (1 - lam) rule + lam old for every factor→variable message of a fused / flooding sweep"""
        self._check(self.lib.cx_set_damping(self.h, float(lam)))

    def sweep_for(self, variable_ids):
        """cx_sweep_for: ONE update_marginals!(engine, variable_ids) under CX_SCHED_REFERENCE, the ids in the caller's order"""
        v = _i64(np.atleast_1d(variable_ids))
        self._check(self.lib.cx_sweep_for(self.h, len(v), _p(v, C.c_int64)))

    def graph_wire(self, signals, dependencies, flags):
        """cx_graph_wire: add_dependency!(signal, dependency; flags) triple by triple; a signal is (kind, variable_id, factor_id)"""
        item = np.dtype([("kind", "<i4"), ("reserved", "<i4"), ("variable_id", "<i8"), ("factor_id", "<i8")])      # cx_item
        assert item.itemsize == C.sizeof(L.Item)

        def items(rows):
            rows = np.asarray(rows, dtype=np.int64).reshape(-1, 3)
            out = np.zeros(max(len(rows), 1), dtype=item)
            out["kind"][:len(rows)] = rows[:, 0]; out["variable_id"][:len(rows)] = rows[:, 1]; out["factor_id"][:len(rows)] = rows[:, 2]
            return out

        sig, dep = items(signals), items(dependencies)
        fl = np.ascontiguousarray(flags, dtype=np.int32)
        n = len(fl)
        if len(np.asarray(signals).reshape(-1, 3)) != n or len(np.asarray(dependencies).reshape(-1, 3)) != n:
            raise ValueError("graph_wire: signals, dependencies and flags must have one row per triple")
        self._check(self.lib.cx_graph_wire(self.h, n, sig.ctypes.data_as(C.POINTER(L.Item)), dep.ctypes.data_as(C.POINTER(L.Item)), _p(fl, C.c_int32) if n else None))

    def cluster_stats(self) -> dict:
        """cx_cluster_stats: the XCD-resident cluster — state (1 ready, 0 not prepared, -1 off), workgroups per launch, calls that were
        finished on plain launches after a barrier of the cluster timed out, whether the last reference-order call ran on it"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.cx_cluster_stats(self.h, out))
        return {"state": int(out[0]), "workgroups": int(out[1]), "recovered_calls": int(out[2]), "last_reference_call": bool(out[3])}

    def ref_plan_stats(self) -> dict:
        out = (C.c_int64 * 8)()
        self._check(self.lib.cx_ref_plan_stats(self.h, out))
        keys = ("stages", "launches", "executions", "messages", "rounds", "plans", "hits", "misses")
        return dict(zip(keys, (int(x) for x in out)))

    def ref_trace(self):
        """cx_ref_trace: the executions of the last reference-order call as (kind, variable_id, factor_id, lo, hi) tuples"""
        n = C.c_int64()
        self._check(self.lib.cx_ref_trace(self.h, 0, None, C.byref(n)))
        items = (L.Item * max(1, n.value))()
        self._check(self.lib.cx_ref_trace(self.h, n.value, items, C.byref(n)))
        out = []
        for it in items[:n.value]:
            if it.kind == L.ITEM_PRODUCT_OF_MESSAGES:
                out.append((it.kind, int(it.variable_id), 0, int(it.factor_id) >> 32, int(it.factor_id) & 0xffffffff))
            else:
                out.append((it.kind, int(it.variable_id), int(it.factor_id), 0, 0))
        return out

    def sweep_begin(self):
        self._check(self.lib.cx_sweep_begin(self.h))

    def sweep_main(self):
        self._check(self.lib.cx_sweep_main(self.h))

    def sweep_end(self):
        self._check(self.lib.cx_sweep_end(self.h))

    def sync(self):
        self._check(self.lib.cx_sync(self.h))

    def set_stream(self, stream_ptr: Optional[int]):
        self._check(self.lib.cx_set_stream(self.h, C.c_void_p(stream_ptr or 0)))

    def residual(self) -> float:
        out = C.c_double()
        self._check(self.lib.cx_residual(self.h, C.byref(out)))
        return out.value

    def message_health(self):
        """cx_message_health: the stored factor→variable messages into non-observed variables, counted on the device by state"""
        out = (C.c_int64 * 4)()
        self._check(self.lib.cx_message_health(self.h, out))
        return dict(zip(("defined", "undefined", "negative_precision", "non_finite"), [int(x) for x in out]))

    def log_evidence(self):
        """cx_log_evidence: log p(data) from the stored factor→variable messages — exact on forests at a fixed point, the Bethe
        estimate elsewhere — and its term counts.  The value is NaN when a term read an undefined message or a belief that is not
        positive definite (counts "undefined" / "not_positive_definite")."""
        val = C.c_double()
        out = (C.c_int64 * 4)()
        self._check(self.lib.cx_log_evidence(self.h, C.byref(val), out))
        return float(val.value), dict(zip(("factor_terms", "variable_terms", "undefined", "not_positive_definite"), [int(x) for x in out]))

    def log_evidence_mfma(self):
        """cx_log_evidence_mfma: log_evidence at the matrix-core dims (a handle created with dim 5 .. 64) — (value, counts) with the
        keys of log_evidence.  One wave per term on the f64 matrix cores; a dim embedded in the next tile size gives the real model's
        value.  log_evidence itself keeps refusing these dims."""
        val = C.c_double()
        out = (C.c_int64 * 4)()
        self._check(self.lib.cx_log_evidence_mfma(self.h, C.byref(val), out))
        return float(val.value), dict(zip(("factor_terms", "variable_terms", "undefined", "not_positive_definite"), [int(x) for x in out]))

    def components(self, variable_ids=None):
        """cx_graph_components: (labels, n_components) — the connected component of every named variable (None: every variable in
        ascending id) of the graph as graph_create received it.  Observed variables and opaque factors are nodes like any other;
        components are numbered by their least variable id.  Host work only."""
        nc = C.c_int64()
        if variable_ids is None:
            ids, n = None, self.stats()["n_variables"]
        else:
            ids = _i64(np.atleast_1d(variable_ids))
            n = len(ids)
        out = np.zeros(n, dtype=np.int64)
        self._check(self.lib.cx_graph_components(self.h, 0 if ids is None else n, None if ids is None else _p(ids, C.c_int64),
                                                 _p(out, C.c_int64) if n else None, C.byref(nc)))
        return out, int(nc.value)

    def log_evidence_components(self, cap=None):
        """cx_log_evidence_components: log p(data) of every connected component from the stored messages.  Returns (values [C],
        comp_counts [C, 4], counts): values[k] sums the terms of log_evidence that belong to component k and is NaN when one of them
        read an undefined message or a belief that is not positive definite (the other components keep their values); comp_counts[k]
        = (factor terms, variable terms, undefined, not positive definite) of component k; counts is log_evidence's dict for the
        whole graph.  cap: return the first min(cap, C) components only."""
        return self._log_evidence_components(self.lib.cx_log_evidence_components, cap)

    def log_evidence_components_mfma(self, cap=None):
        """cx_log_evidence_components_mfma: log_evidence_components at the matrix-core dims (a handle created with dim 5 .. 64) — the
        same return value, with the terms, counts and NaN rule of log_evidence_mfma: the independent models of one handle told apart
        (K candidates of a likelihood profile, K starts of EM, a panel of series).  log_evidence_components itself keeps refusing
        these dims."""
        return self._log_evidence_components(self.lib.cx_log_evidence_components_mfma, cap)

    def _log_evidence_components(self, call, cap):
        nc = C.c_int64()
        if getattr(self, "_n_components", None) is None:      # (a handle has one graph for life: counted once, host work)
            self._check(self.lib.cx_graph_components(self.h, 0, None, None, C.byref(nc)))
            self._n_components = int(nc.value)
        n = self._n_components if cap is None else min(int(cap), self._n_components)
        val = np.zeros(n, dtype=np.float64)
        cc = np.zeros((n, 4), dtype=np.int64)
        out = (C.c_int64 * 4)()
        self._check(call(self.h, n, _p(val, C.c_double) if n else None, _p(cc, C.c_int64) if n else None, C.byref(nc), out))
        return val, cc, dict(zip(("factor_terms", "variable_terms", "undefined", "not_positive_definite"), [int(x) for x in out]))

    def factor_beliefs(self, factor_ids):
        """cx_factor_beliefs: the joint posterior of two-variable Gaussian factors from the stored messages, (means [n, 2d],
        covariances [n, 2d, 2d]) in the order (out, in) — ADDITIVE: the lower variable id first.  Observed entries are the datum with
        zero rows and columns; a factor with an undefined input (or a belief that is not positive definite) reads as NaN."""
        return self._factor_beliefs(self.lib.cx_factor_beliefs, factor_ids)

    def factor_beliefs_mfma(self, factor_ids):
        """cx_factor_beliefs_mfma: factor_beliefs at the matrix-core dims (a handle created with dim 5 .. 64), two-variable
        CX_FACTOR_GAUSS_LINEAR factors — the same shapes, order and NaN rule; d is the dim the handle was created with, whatever tile
        size it runs in.  factor_beliefs itself keeps refusing these dims."""
        return self._factor_beliefs(self.lib.cx_factor_beliefs_mfma, factor_ids)

    def _factor_beliefs(self, call, factor_ids):
        f = _i64(np.atleast_1d(factor_ids))
        n2 = 2 * self.dim
        out = np.zeros((len(f), n2 + n2 * n2), dtype=np.float64)
        self._check(call(self.h, len(f), _p(f, C.c_int64), _p(out, C.c_double)))
        return out[:, :n2].copy(), out[:, n2:].reshape(len(f), n2, n2).copy()

    def factor_statistics(self, factor_ids=None, groups=None, n_groups=None):
        """cx_factor_statistics: EM statistics in residual coordinates r = x_out - A x_in - b, summed per group.  factor_ids=None
        (dim 2..4): one group per parameter set (n_groups default: the sets given to set_factor_matrices).  Returns ({"n" [G],
        "sum_r" [G, d], "sum_x" [G, d], "S_rr", "S_rx", "S_xx" [G, d, d]}, counts) with counts "factors", "groups", "undefined",
        "not_positive_definite"; a group's arrays (n excepted) are NaN when one of its factors is undefined or not positive definite."""
        return self._factor_statistics(self.lib.cx_factor_statistics, factor_ids, groups, n_groups)

    def factor_statistics_mfma(self, factor_ids=None, groups=None, n_groups=None):
        """cx_factor_statistics_mfma: factor_statistics at the matrix-core dims (a handle created with dim 5 .. 64) — the same
        arguments, dict keys, shapes, counts and NaN rule, r = x_out - A x_in - b (b: set_factor_offsets_mfma, 0 unless set).  One wave per factor on the f64
        matrix cores; sums in a fixed order, bit-identical across calls.  factor_statistics itself keeps refusing these dims."""
        return self._factor_statistics(self.lib.cx_factor_statistics_mfma, factor_ids, groups, n_groups)

    def _factor_statistics(self, call, factor_ids, groups, n_groups):
        d = self.dim
        if factor_ids is None:
            if groups is not None:
                raise ValueError("groups need factor_ids")
            if n_groups is None:
                n_groups = getattr(self, "_n_sets", 0)
            f = g = None
            n = 0
        else:
            f, g = _i64(np.atleast_1d(factor_ids)), _i64(np.atleast_1d(groups))
            if len(f) != len(g):
                raise ValueError("factor_ids and groups differ in length")
            n = len(f)
            if n_groups is None:
                n_groups = int(g.max()) + 1 if n and g.max() >= 0 else 1
        ns = 1 + 2 * d + 3 * d * d
        out = np.zeros((max(int(n_groups), 0), ns), dtype=np.float64)
        cnt = (C.c_int64 * 4)()
        self._check(call(self.h, n, None if f is None else _p(f, C.c_int64), None if g is None else _p(g, C.c_int64),
                         int(n_groups), _p(out, C.c_double) if out.size else None, cnt))
        G = len(out)
        o = 1 + 2 * d
        stats = {"n": out[:, 0].copy(), "sum_r": out[:, 1:1 + d].copy(), "sum_x": out[:, 1 + d:o].copy(),
                 "S_rr": out[:, o:o + d * d].reshape(G, d, d).copy(), "S_rx": out[:, o + d * d:o + 2 * d * d].reshape(G, d, d).copy(),
                 "S_xx": out[:, o + 2 * d * d:].reshape(G, d, d).copy()}
        return stats, dict(zip(("factors", "groups", "undefined", "not_positive_definite"), [int(x) for x in cnt]))

    def factor_disturbance_rows_mfma(self):
        """cx_factor_disturbance_rows_mfma: the factor ids of the rows factor_disturbances_mfma(factor_ids=None) returns, ascending"""
        return self._predictive_rows(self.lib.cx_factor_disturbance_rows_mfma)

    def factor_disturbances_mfma(self, factor_ids=None, rows=True):
        """cx_factor_disturbances_mfma: the smoothed disturbance of every two-variable x_out = A x_in + b + w, w ~ N(0, Q), factor of a
        handle created with dim 5 .. 64 — PER FACTOR what factor_statistics_mfma sums per group (r = x_out - A x_in - b is w).
        factor_ids=None: every such factor in ascending id; otherwise the named ones in the caller's order.  Returns {"factor_ids",
        "mean" [n, d] = E[r | data], "cov" [n, d, d] = Cov(r | data), "expected_mahalanobis" [n] = E[r'Q⁻¹r | data], "mahalanobis" [n]
        = E[r]'Q⁻¹E[r], "total" (the sum of expected_mahalanobis over the finite rows: minus twice the quadratic part of the EM
        Q-function), "counts"}; a row with an undefined input or a failed factorisation is NaN (counts "undefined" /
        "not_positive_definite").  rows=False: no "mean" and "cov" (the scores, the total and the counts alone come to the host, and
        they are the bits of the call with rows).  learn.auxiliary_residuals standardises the means."""
        d = self.dim
        f = None if factor_ids is None else _i64(np.atleast_1d(factor_ids))
        pf = None if f is None else _p(f, C.c_int64)
        n = 0 if f is None else len(f)
        ids = self.factor_disturbance_rows_mfma() if f is None else f
        tot, cnt = C.c_double(), (C.c_int64 * 4)()
        sc = np.zeros((len(ids), 2), dtype=np.float64)
        out = np.zeros((len(ids), d + d * d), dtype=np.float64) if rows else None
        self._check(self.lib.cx_factor_disturbances_mfma(self.h, n, pf, _p(out, C.c_double) if rows and out.size else None,
                                                         _p(sc, C.c_double) if sc.size else None, C.byref(tot), cnt))
        assert cnt[0] == len(ids)
        res = {"factor_ids": ids, "expected_mahalanobis": sc[:, 0].copy(), "mahalanobis": sc[:, 1].copy(), "total": float(tot.value),
               "counts": dict(zip(("rows", "finite", "undefined", "not_positive_definite"), [int(x) for x in cnt]))}
        if rows:
            res["mean"] = out[:, :d].copy()
            res["cov"] = out[:, d:].reshape(len(ids), d, d).copy()
        return res

    def predictive_rows(self):
        """cx_predictive_rows: the factor ids of the rows predictive(factor_ids=None) scores, ascending"""
        return self._predictive_rows(self.lib.cx_predictive_rows)

    def predictive_rows_mfma(self):
        """cx_predictive_rows_mfma: the factor ids of the rows predictive_mfma(factor_ids=None) scores, ascending"""
        return self._predictive_rows(self.lib.cx_predictive_rows_mfma)

    def _predictive_rows(self, call):
        n = C.c_int64()
        self._check(call(self.h, 0, None, C.byref(n)))
        ids = np.zeros(n.value, dtype=np.int64)
        if n.value:
            self._check(call(self.h, n.value, _p(ids, C.c_int64), C.byref(n)))
        return ids

    def predictive(self, mode="loo", factor_ids=None, rows=True):
        """cx_predictive: the predictive distribution of every datum that a Gaussian rule factor generates (its OUT end the one observed
        variable), from the stored messages.  mode "loo": given all other data (the sum of log_density is the leave-one-out score);
        "causal": given the data of its inputs' ancestors only (on a chain: the Kalman innovations, the sum is log_evidence).
        factor_ids=None: every row in ascending factor id.  Returns {"factor_ids", "mean" [n, d], "cov" [n, d, d], "log_density" [n],
        "mahalanobis" [n], "total", "counts"}; a row with an undefined input or an improper predictive is NaN (counts "undefined" /
        "improper"), "total" sums the scored rows only.  rows=False: the total and the counts alone (the arrays are None)."""
        return self._predictive(self.lib.cx_predictive, self.lib.cx_predictive_rows, mode, factor_ids, rows)

    def predictive_mfma(self, mode="loo", factor_ids=None, rows=True):
        """cx_predictive_mfma: predictive at the matrix-core dims (a handle created with dim 5 .. 64) — the same arguments, dict keys,
        shapes, counts and NaN rule; d is the dim the handle was created with, whatever tile size it runs in.  A row is a two-variable
        CX_FACTOR_GAUSS_LINEAR factor whose OUT end alone is observed.  One wave per row on the f64 matrix cores; the total is
        bit-identical across calls and between rows=False and rows=True.  predictive itself keeps refusing these dims."""
        return self._predictive(self.lib.cx_predictive_mfma, self.lib.cx_predictive_rows_mfma, mode, factor_ids, rows)

    def _predictive(self, call, rows_call, mode, factor_ids, rows):
        m = {"loo": L.PREDICT_LOO, "causal": L.PREDICT_CAUSAL}.get(mode, mode)
        d = self.dim
        f = None if factor_ids is None else _i64(np.atleast_1d(factor_ids))
        pf = None if f is None else _p(f, C.c_int64)
        n = 0 if f is None else len(f)
        tot, cnt = C.c_double(), (C.c_int64 * 4)()
        keys = ("rows", "scored", "undefined", "improper")
        if not rows:
            self._check(call(self.h, int(m), n, pf, None, C.byref(tot), cnt))
            return {"factor_ids": f, "mean": None, "cov": None, "log_density": None, "mahalanobis": None, "total": float(tot.value),
                    "counts": dict(zip(keys, [int(x) for x in cnt]))}
        if f is None:
            f = self._predictive_rows(rows_call)
        out = np.zeros((len(f), d + d * d + 2), dtype=np.float64)
        self._check(call(self.h, int(m), n, pf, _p(out, C.c_double) if out.size else None, C.byref(tot), cnt))
        assert cnt[0] == len(out)
        return {"factor_ids": f, "mean": out[:, :d].copy(), "cov": out[:, d:d + d * d].reshape(len(f), d, d).copy(),
                "log_density": out[:, d + d * d].copy(), "mahalanobis": out[:, d + d * d + 1].copy(), "total": float(tot.value),
                "counts": dict(zip(keys, [int(x) for x in cnt]))}

    def causal_marginals(self, mode="filtered", lag=0, variable_ids=None):
        """cx_causal_marginals: the causal estimates of the states beside the smoothed marginals of get_marginals, from the stored
        messages.  mode "predicted": p(x_t | y_<t); "filtered": p(x_t | y_<=t); "filtered" with lag=L: the fixed-lag smoother
        p(x_t | y_<=t+L) (on a forest: the data of the descendants within L transitions).  variable_ids=None: every variable in
        ascending id.  Returns {"variable_ids", "mean" [n, d], "cov" [n, d, d], "counts"}; an observed variable's row is its datum and a
        zero covariance, a row with an undefined input or a precision that is not positive definite is NaN (counts "undefined" /
        "improper")."""
        return self._causal_marginals(self.lib.cx_causal_marginals, mode, lag, variable_ids)

    def causal_marginals_mfma(self, mode="filtered", lag=0, variable_ids=None):
        """cx_causal_marginals_mfma: causal_marginals at the matrix-core dims (a handle created with dim 5 .. 64) — the same arguments,
        dict keys, shapes, counts and NaN rule; d is the dim the handle was created with, whatever tile size it runs in.  One wave per
        row on the f64 matrix cores; a lag L adds L launches over every transition with two free ends and, on its first use, the β
        workspace (cortex_hip.h states its size).  A row is also improper when a pivot of its precision is at rounding level of the
        sum of all stored messages into the variable (the state behind a leading gap, predicted).  causal_marginals itself keeps
        refusing these dims."""
        return self._causal_marginals(self.lib.cx_causal_marginals_mfma, mode, lag, variable_ids)

    def _causal_marginals(self, call, mode, lag, variable_ids):
        m = {"predicted": L.CAUSAL_PREDICTED, "filtered": L.CAUSAL_FILTERED}.get(mode, mode)
        d = self.dim
        if variable_ids is None:
            ids, n = None, self.stats()["n_variables"]
        else:
            ids = _i64(np.atleast_1d(variable_ids))
            n = len(ids)
        out = np.zeros((n, d + d * d), dtype=np.float64)
        cnt = (C.c_int64 * 4)()
        self._check(call(self.h, int(m), int(lag), n if ids is not None else 0, None if ids is None else _p(ids, C.c_int64), _p(out, C.c_double), cnt))
        assert cnt[0] == n
        return {"variable_ids": ids, "mean": out[:, :d].copy(), "cov": out[:, d:].reshape(n, d, d).copy(),
                "counts": dict(zip(("rows", "finite", "undefined", "improper"), [int(x) for x in cnt]))}

    def sample_posterior(self, n_samples, seed=0, variable_ids=None, noise=None):
        """cx_sample_posterior: joint draws from p(x | data) on a forest (the simulation smoother), from the stored messages.
        Returns (samples [n_samples, n, d] for variable_ids — None: every variable in ascending id —, counts) with counts "free",
        "components", "undefined", "not_positive_definite".  noise: the standard normals [n_samples, n_variables, d] in ascending
        variable-id order (observed rows ignored) in place of the device's Philox4x32-10 draws; the result is then affine in noise."""
        return self._sample_posterior(self.lib.cx_sample_posterior, n_samples, seed, variable_ids, noise)

    def sample_posterior_mfma(self, n_samples, seed=0, variable_ids=None, noise=None):
        """cx_sample_posterior_mfma: sample_posterior at the matrix-core dims (a handle created with dim 5 .. 64) — the same arguments,
        shapes, counts and NaN rule; d is the dim the handle was created with, whatever tile size it runs in (the padding of an
        embedded dim gets no noise and never shows).  The links of the forest are computed once per call, one wave each on the f64
        matrix cores (cortex_hip.h states the size of their workspace); the samples run in panels of 16 through a blocked scan.  A
        component with no information at all (no observed neighbour, no opaque message) is NaN and counted "not_positive_definite".
        sample_posterior itself keeps refusing these dims."""
        return self._sample_posterior(self.lib.cx_sample_posterior_mfma, n_samples, seed, variable_ids, noise)

    def _sample_posterior(self, call, n_samples, seed, variable_ids, noise):
        d = self.dim
        S = int(n_samples)
        if variable_ids is None:
            ids, n = None, self.stats()["n_variables"]
        else:
            ids = _i64(np.atleast_1d(variable_ids))
            n = len(ids)
        eps = None
        if noise is not None:
            nv = self.stats()["n_variables"]
            eps = _f64(noise)
            if eps.shape != (S, nv, d):
                raise ValueError(f"noise must be [{S}, {nv}, {d}]")
        out = np.zeros((max(S, 0), n, d), dtype=np.float64)
        cnt = (C.c_int64 * 4)()
        self._check(call(self.h, S, C.c_uint64(int(seed) & (2 ** 64 - 1)), None if eps is None else _p(eps, C.c_double),
                         n if ids is not None else 0, None if ids is None else _p(ids, C.c_int64), _p(out, C.c_double) if S >= 1 else None, cnt))
        return out, dict(zip(("free", "components", "undefined", "not_positive_definite"), [int(x) for x in cnt]))

    def linear_moments(self, functionals, cov=True):
        """cx_linear_moments: the exact mean and covariance of linear functionals φ_k(x) = Σ_i w_{k,i}' x_i of the joint posterior of a
        forest, from the stored messages.  functionals: a list of (variable_ids, weights [n_k, d] — [n_k] at dim 1 —) pairs, or the CSR
        triple (offsets [K + 1], variable_ids [nnz], weights [nnz, d]).  Returns (mean [K], cov [K, K] or None, counts) with counts
        "components", "failed", "nan_functionals", "free"; a functional that touches a failed component is NaN (its row and column of
        cov too).  cov=False: the means only."""
        return self._linear_moments(self.lib.cx_linear_moments, functionals, cov)

    def linear_moments_mfma(self, functionals, cov=True):
        """cx_linear_moments_mfma: linear_moments at the matrix-core dims (a handle created with dim 5 .. 64) — the same arguments,
        shapes, counts and NaN rule; d is the dim the handle was created with, whatever tile size it runs in.  The distribution is the
        one sample_posterior_mfma draws from: mean = W x⁰ and cov = W B Bᵀ Wᵀ of its affine map x = x⁰ + B ε, exact, with no
        Monte-Carlo error and K² + K doubles to the host.  The call shares the sampler's plan and link workspace; functionals run in
        panels of 16 on the f64 matrix cores.  A component with no information at all is failed.  linear_moments itself keeps refusing
        these dims."""
        return self._linear_moments(self.lib.cx_linear_moments_mfma, functionals, cov)

    def _linear_moments(self, call, functionals, cov):
        d = self.dim
        if isinstance(functionals, tuple) and len(functionals) == 3 and not isinstance(functionals[0], tuple):
            off, ids, w = _i64(np.atleast_1d(functionals[0])), _i64(np.atleast_1d(functionals[1])), _f64(functionals[2])
        else:
            parts = [(_i64(np.atleast_1d(i)), _f64(x).reshape(-1, d)) for i, x in functionals]
            for i, x in parts:
                if len(i) != len(x):
                    raise ValueError("a functional needs one weight vector of length dim per variable id")
            off = _i64(np.concatenate([[0], np.cumsum([len(i) for i, _ in parts])]))
            ids = _i64(np.concatenate([i for i, _ in parts])) if parts else _i64(np.zeros(0))
            w = _f64(np.concatenate([x for _, x in parts])) if parts else _f64(np.zeros((0, d)))
        if len(off) < 1:
            raise ValueError("offsets needs at least one entry")
        K = len(off) - 1
        if w.size != len(ids) * d:
            raise ValueError(f"weights must be [{len(ids)}, {d}]")
        mean = np.zeros(K, dtype=np.float64)
        cv = np.zeros((K, K), dtype=np.float64) if cov else None
        cnt = (C.c_int64 * 4)()
        self._check(call(self.h, K, _p(off, C.c_int64), _p(ids, C.c_int64) if len(ids) else None, _p(w, C.c_double) if w.size else None,
                         _p(mean, C.c_double) if K else None, _p(cv, C.c_double) if cov and K else None, cnt))
        return mean, cv, dict(zip(("components", "failed", "nan_functionals", "free"), [int(x) for x in cnt]))

    def posterior_covariance(self, var_a, var_b):
        """the d x d cross-covariance Cov(x_a, x_b) of two variables under the joint posterior of a forest: 2d unit functionals of
        linear_moments (var_a == var_b: the marginal covariance)"""
        d = self.dim
        eye = np.eye(d)
        fs = [([var_a], eye[i:i + 1]) for i in range(d)] + [([var_b], eye[i:i + 1]) for i in range(d)]
        _, cv, _ = self.linear_moments(fs)
        return cv[:d, d:].copy()

    def contrast_variance(self, var_a, var_b):
        """Var(1'(x_a - x_b)) under the joint posterior of a forest (dim 1: the variance of x_a - x_b): one functional of linear_moments"""
        one = np.ones((1, self.dim))
        _, cv, _ = self.linear_moments([([var_a, var_b], np.concatenate([one, -one]))])
        return float(cv[0, 0])

    def posterior_covariance_mfma(self, var_a, var_b):
        """posterior_covariance at the matrix-core dims: 2d unit functionals of linear_moments_mfma"""
        d = self.dim
        eye = np.eye(d)
        fs = [([var_a], eye[i:i + 1]) for i in range(d)] + [([var_b], eye[i:i + 1]) for i in range(d)]
        _, cv, _ = self.linear_moments_mfma(fs)
        return cv[:d, d:].copy()

    def contrast_variance_mfma(self, var_a, var_b):
        """contrast_variance at the matrix-core dims: one functional of linear_moments_mfma"""
        one = np.ones((1, self.dim))
        _, cv, _ = self.linear_moments_mfma([([var_a, var_b], np.concatenate([one, -one]))])
        return float(cv[0, 0])

    # -- halo -----------------------------------------------------------------------------------
    def halo_configure(self, send_var, send_fac, recv_var, recv_fac):
        sv, sf, rv, rf = _i64(send_var), _i64(send_fac), _i64(recv_var), _i64(recv_fac)
        self._check(self.lib.cx_halo_configure(self.h, len(sv), _p(sv, C.c_int64), _p(sf, C.c_int64), len(rv),
                                               _p(rv, C.c_int64), _p(rf, C.c_int64)))

    def sweep_until(self, tol: float, max_sweeps: int, check_every: int = 10):
        """(sweeps run, last residual): cx_sweep_until"""
        n, r = C.c_int32(), C.c_double()
        self._check(self.lib.cx_sweep_until(self.h, float(tol), int(max_sweeps), int(check_every), C.byref(n), C.byref(r)))
        return n.value, r.value

    def halo_configure_state(self, send_var, send_fac, recv_var, recv_fac):
        """Deep halo: the lists name factor→variable messages of redundant variables (cx_halo_configure_state)."""
        sv, sf, rv, rf = _i64(send_var), _i64(send_fac), _i64(recv_var), _i64(recv_fac)
        self._check(self.lib.cx_halo_configure_state(self.h, len(sv), _p(sv, C.c_int64), _p(sf, C.c_int64), len(rv),
                                                     _p(rv, C.c_int64), _p(rf, C.c_int64)))

    def halo_set_layers(self, variable_ids, layers, depth: int):
        v = _i64(np.atleast_1d(variable_ids))
        lay = np.ascontiguousarray(np.atleast_1d(layers), dtype=np.int32)
        self._check(self.lib.cx_halo_set_layers(self.h, len(v), _p(v, C.c_int64), _p(lay, C.c_int32), int(depth)))

    def halo_state_pack(self):
        self._check(self.lib.cx_halo_state_pack(self.h))

    def halo_state_unpack(self):
        self._check(self.lib.cx_halo_state_unpack(self.h))

    def halo_state_exchange(self):
        self._check(self.lib.cx_halo_state_exchange(self.h))

    def halo_exchange_sweep(self, n: int):
        """the exchange and n sweeps, the exchange overlapped with the owned part of the first sweep"""
        self._check(self.lib.cx_halo_exchange_sweep(self.h, int(n)))

    @property
    def halo_doubles(self) -> int:
        """doubles per message in the halo buffers (the storage form)"""
        d = self.dim
        return 2 if d == 1 else (d + d * d if d == 64 else d + d * (d + 1) // 2)

    def chain_block_maps(self):
        """cx_chain_block_maps: (forward map [6], backward map [6], side of the first variable [2], side of the last [2],
        first variable id, last variable id, links)"""
        d = self.dim
        nd, ns = (6, 2) if d == 1 else (d * (d + 1) + d * d + 2 * d, d + d * (d + 1) // 2)     # dim > 1: P | B | C | h | c;  eta | Lambda packed
        f, b, sf, sl = np.zeros(nd), np.zeros(nd), np.zeros(ns), np.zeros(ns)
        v0, v1, nl = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self.lib.cx_chain_block_maps(self.h, _p(f, C.c_double), _p(b, C.c_double), _p(sf, C.c_double), _p(sl, C.c_double),
                                                 C.byref(v0), C.byref(v1), C.byref(nl)))
        return f, b, sf, sl, v0.value, v1.value, nl.value

    def halo_buffers(self):
        sp, rp, sb, rb = C.c_void_p(), C.c_void_p(), C.c_int64(), C.c_int64()
        self._check(self.lib.cx_halo_buffers(self.h, C.byref(sp), C.byref(sb), C.byref(rp), C.byref(rb)))
        return (sp.value or 0, sb.value), (rp.value or 0, rb.value)

    def halo_set_buffers(self, send_ptr: int, recv_ptr: int):
        self._check(self.lib.cx_halo_set_buffers(self.h, C.c_void_p(send_ptr or 0), C.c_void_p(recv_ptr or 0)))

    # -- RCCL exchange issued by the library -------------------------------------------------------
    def comm_unique_id(self) -> bytes:
        buf = C.create_string_buffer(128)
        rc = self.lib.cx_comm_unique_id(buf)
        if rc != L.OK:
            raise L.CortexHipError(rc, self.lib.cx_last_error(None).decode())
        return buf.raw

    def comm_init(self, world: int, rank: int, unique_id: bytes):
        assert len(unique_id) == 128
        self._check(self.lib.cx_comm_init(self.h, world, rank, C.c_char_p(unique_id)))

    # -- deep-halo exchange through IPC-mapped receive areas (cx_api_ipc.hip) -----------------------
    def halo_ipc_alloc(self):
        """-> (64-byte IPC handle, device address of the block, bytes of one receive area)"""
        buf = C.create_string_buffer(64)
        base, area = C.c_void_p(), C.c_int64()
        self._check(self.lib.cx_halo_ipc_alloc(self.h, buf, C.byref(base), C.byref(area)))
        return buf.raw, int(base.value), int(area.value)

    def halo_ipc_connect(self, peer_index: int, remote_entry: int, remote_recv_off: int, remote_area_bytes: int, handle: bytes = None,
                         same_process_base: int = None):
        assert (handle is None) != (same_process_base is None)
        self._check(self.lib.cx_halo_ipc_connect(self.h, int(peer_index), C.c_char_p(handle) if handle is not None else None,
                                                 C.c_void_p(same_process_base) if same_process_base is not None else None,
                                                 int(remote_entry), int(remote_recv_off), int(remote_area_bytes)))

    def halo_ipc_exchange(self):
        self._check(self.lib.cx_halo_ipc_exchange(self.h))

    def halo_ipc_exchange_sweep(self, n: int):
        """the exchange around the owned part of the first of n sweeps"""
        self._check(self.lib.cx_halo_ipc_exchange_sweep(self.h, int(n)))

    def halo_ipc_batch(self, n: int):
        """cx_halo_ipc_batch: n sweeps with the next exchange pushed inside the last one (bit-identical to exchange + sweep(n))"""
        self._check(self.lib.cx_halo_ipc_batch(self.h, int(n)))

    def halo_ipc_set_fused(self, on: bool):
        """cx_halo_ipc_set_fused: every neighbour pushes from another device -> one launch per exchange"""
        self._check(self.lib.cx_halo_ipc_set_fused(self.h, 1 if on else 0))

    def halo_ipc_push(self):
        self._check(self.lib.cx_halo_ipc_push(self.h))

    def halo_ipc_unpack(self):
        self._check(self.lib.cx_halo_ipc_unpack(self.h))

    def halo_ipc_status(self):
        """synchronises -> (timed_out, exchanges)"""
        t, n = C.c_int32(), C.c_int64()
        self._check(self.lib.cx_halo_ipc_status(self.h, C.byref(t), C.byref(n)))
        return bool(t.value), int(n.value)

    def halo_ipc_set_timeout(self, seconds: float):
        self._check(self.lib.cx_halo_ipc_set_timeout(self.h, float(seconds)))

    def halo_peers(self, peers):
        """peers: iterable of (rank, send_offset, send_count, recv_offset, recv_count), in messages."""
        peers = list(peers)
        r = np.ascontiguousarray([p[0] for p in peers], dtype=np.int32)
        cols = [np.ascontiguousarray([p[k] for p in peers], dtype=np.int64) for k in (1, 2, 3, 4)]
        self._check(self.lib.cx_halo_peers(self.h, len(peers), _p(r, C.c_int32), *[_p(c, C.c_int64) for c in cols]))

    def sweep_exchange(self, n: int = 1):
        self._check(self.lib.cx_sweep_exchange(self.h, int(n)))

    # -- variational families (cx_set_marginals / cx_update_marginals) ----------------------------
    def set_marginals(self, variable_ids, form: int, payload):
        v = _i64(np.atleast_1d(variable_ids))
        p = _f64(payload)
        need = len(v) * (1 if form == L.FORM_POINT else 2)
        if p.size != need:
            raise ValueError(f"payload has {p.size} doubles, expected {need}")
        self._check(self.lib.cx_set_marginals(self.h, len(v), _p(v, C.c_int64), form, _p(p, C.c_double)))

    def update_marginals(self, variable_ids):
        """One `update_marginals!(engine, ids)`; `variable_ids` may be L.VMP_ALL_NORMAL / L.VMP_ALL_PRECISION."""
        if isinstance(variable_ids, (int, np.integer)) and variable_ids < 0:
            self._check(self.lib.cx_update_marginals(self.h, int(variable_ids), None))
            return
        v = _i64(np.atleast_1d(variable_ids))
        self._check(self.lib.cx_update_marginals(self.h, len(v), _p(v, C.c_int64)))

    # -- checkpoint (cx_state_*) -----------------------------------------------------------------
    def export_state(self) -> np.ndarray:
        """The handle's mutable state (messages, marginals, observed flags, sweep counter) as a uint8 array."""
        n = C.c_int64()
        self._check(self.lib.cx_state_bytes(self.h, C.byref(n)))
        blob = np.empty(n.value, dtype=np.uint8)
        self._check(self.lib.cx_state_export(self.h, blob.ctypes.data_as(C.c_void_p), n.value))
        return blob

    def import_state(self, blob) -> None:
        blob = np.ascontiguousarray(blob, dtype=np.uint8)
        self._check(self.lib.cx_state_import(self.h, blob.ctypes.data_as(C.c_void_p), blob.size))

    def save_state(self, path: str) -> None:
        self.export_state().tofile(path)

    def load_state(self, path: str) -> None:
        self.import_state(np.fromfile(path, dtype=np.uint8))

    # -- measurement ----------------------------------------------------------------------------
    def profile_enable(self, on=True):
        """True/1: hipEvents around every launch; n > 1: around every n-th launch; False/0: off."""
        self._check(self.lib.cx_profile_enable(self.h, int(on)))

    def profile_read(self, kernel: int):
        ms, n = C.c_double(), C.c_int64()
        self._check(self.lib.cx_profile_read(self.h, kernel, C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def kernel_name(self, kernel: int) -> str:
        return self.lib.cx_kernel_name(kernel).decode()
