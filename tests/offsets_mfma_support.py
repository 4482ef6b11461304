"""Shared by the factor-offset tests of the matrix-core dims (cx_set_factor_offsets_mfma, dim 5..64): numpy statements of what the device
computes with offsets there, next to the model-level references of tests/offsets_support.py.

  linear_terms(A, Q, b)              (g_out, g_in, kappa) = (Q^-1 b, -A' Q^-1 b, b' Q^-1 b): what k_offset_terms64 keeps per slot
  term_table_log_z(gm, f2v)          the evidence from stored messages by the term table of k_evm_terms with offsets (uncentred, as the
                                     kernel evaluates it): variables, then kFacFree / kFacObs / kFacBoth with g and kappa
  OffsetsPlan64 / run_plan_offsets   the chain-64 plan built with Input.offsets (the links' h and c name rows of the "off" space) and its
                                     numpy execution: tests/test_chain64_plan.py's executor with that space added
  chain_offsets_inputs(model, b)     a model of tests/anisotropic.chain in the abstract slot space of tests/test_chain64_plan.py, its g
                                     rows and its side messages (the likelihoods with their own offsets)
"""
from __future__ import annotations

import numpy as np

from tests import hostlogic as H

LOG2PI = float(np.log(2.0 * np.pi))


def linear_terms(A, Q, b):
    Qi = np.linalg.inv(np.asarray(Q, float))
    b = np.asarray(b, float)
    return Qi @ b, -np.asarray(A, float).T @ Qi @ b, float(b @ Qi @ b)


def _half_quad_logdet(eta, lam):
    """1/2 eta' lam^-1 eta - 1/2 log det lam"""
    sign, ld = np.linalg.slogdet(lam)
    assert sign > 0
    return 0.5 * float(eta @ np.linalg.solve(lam, eta)) - 0.5 * float(ld)


def term_table_log_z(gm, f2v):
    """log Z = sum_a log z_a + sum_i (1 - d_i) log z_i of a GModel of two-variable factors x_out = A x_in + b + N(0, Q) (no opaque
    messages), every term as cx_evidence_mfma.hip states it with offsets: the potential of a factor is the zero-offset one times
    exp(g_out'x_out + g_in'x_in - kappa / 2)."""
    d, nv = gm.d, len(gm.var_ids)
    assert set(gm.groups) == {2} and len(gm.opq_var) == 0
    g = gm.groups[2]
    e, l = f2v[2]
    M_eta, M_lam, deg = np.zeros((nv, d)), np.zeros((nv, d, d)), np.zeros(nv, np.int64)
    for j in range(2):
        np.add.at(M_eta, g["vars"][:, j], e[:, j])
        np.add.at(M_lam, g["vars"][:, j], l[:, j])
        np.add.at(deg, g["vars"][:, j], 1)
    total = 0.0
    for v in range(nv):
        if gm.obs[v] or deg[v] == 1:
            continue
        total += (1 - deg[v]) * (_half_quad_logdet(M_eta[v], M_lam[v]) + 0.5 * d * LOG2PI)
    for fi in range(len(g["fid"])):
        vo, vi = g["vars"][fi]
        A, Q, b = -g["C"][fi][1], g["Q"][fi], g["b"][fi]
        Qi = np.linalg.inv(Q)
        ldq = float(np.linalg.slogdet(2 * np.pi * Q)[1])
        g_out, g_in, kappa = linear_terms(A, Q, b)
        P, B, C = Qi, A.T @ Qi, A.T @ Qi @ A          # the rule table towards IN: the sender's end, the cross term, the receiver's end
        oo, oi = bool(gm.obs[vo]), bool(gm.obs[vi])
        if oo and oi:                                  # kFacBoth
            yo, yi = gm.y[vo], gm.y[vi]
            q = yo @ P @ yo - 2.0 * yo @ (B.T @ yi) + yi @ C @ yi
            q += kappa - 2.0 * yo @ g_out - 2.0 * yi @ g_in
            total += -0.5 * ldq - 0.5 * q
        elif oo or oi:                                 # kFacObs: the table towards the free end
            if oo:
                y, vf, jf = gm.y[vo], vi, 1
                Pt, Bt, Ct, g_obs, g_free = P, B, C, g_out, g_in
            else:
                y, vf, jf = gm.y[vi], vo, 0
                Pt, Bt, Ct, g_obs, g_free = C, B.T, P, g_in, g_out
            S = M_lam[vf] - l[fi, jf] + Ct
            h = M_eta[vf] - e[fi, jf] + Bt @ y + g_free
            cst = -0.5 * ldq - 0.5 * y @ Pt @ y + 0.5 * d * LOG2PI + y @ g_obs - 0.5 * kappa
            total += cst + _half_quad_logdet(h, S)
        else:                                          # kFacFree: OUT goes first
            lo, eo = M_lam[vo] - l[fi, 0], M_eta[vo] - e[fi, 0]
            li, ei = M_lam[vi] - l[fi, 1], M_eta[vi] - e[fi, 1]
            M = lo + P
            w = eo + g_out
            cst = -0.5 * ldq + _half_quad_logdet(w, M) + d * LOG2PI - 0.5 * kappa
            S = li + C - B @ np.linalg.solve(M, B.T)
            h = ei + B @ np.linalg.solve(M, w) + g_in
            total += cst + _half_quad_logdet(h, S)
    return float(total)


# ---- the chain-64 plan with the offsets' space ------------------------------------------------------------------------------------------
SPACES = H.SPACES + ("aux", "off")


def split(handle):
    return SPACES[int(handle) >> 56], int(handle) & ((1 << 56) - 1)


class _OffsetsLib:
    """the host-logic library with cxh_plan64_create answered by cxh_plan64_create_offsets (the same arguments)"""

    def __init__(self, lib):
        self._lib = lib
        lib.cxh_plan64_create_offsets.restype = lib.cxh_plan64_create.restype
        lib.cxh_plan64_create_offsets.argtypes = lib.cxh_plan64_create.argtypes

    def __getattr__(self, name):
        return getattr(self._lib, "cxh_plan64_create_offsets" if name == "cxh_plan64_create" else name)


class OffsetsPlan64(H.Plan64):
    """tests.hostlogic.Plan64 built with Input.offsets"""

    def __init__(self, *args, **kw):
        real = H.lib
        H.lib = lambda: _OffsetsLib(real())
        try:
            super().__init__(*args, **kw)
        finally:
            H.lib = real


def run_plan_offsets(plan, mem, d):
    """the launches of the plan in order on the arenas of `mem` (name -> flat array: zero, f2v, ptab, btab, pot, ent, off); the arithmetic
    of tests/test_chain64_plan.py's executor — the compositions add the children's h and c, a step is
    eta_out = c + B M^-1 (eta_in + h) — with the handles resolved over the eight spaces"""
    dd = d * d

    def view(handle, n):
        sp, off = split(handle)
        a = mem["zero"] if sp == "zero" else mem[sp]
        assert (0 if sp == "zero" else off) + n <= a.size, (sp, off, n)
        return a[:n] if sp == "zero" else a[off:off + n]

    def mat(handle):
        return view(handle, dd).reshape(d, d)

    def msg(handle):
        v = view(handle, d + dd)
        return v[:d], v[d:].reshape(d, d)

    for jobs in plan.compose_launches:
        for out, first, n in jobs.tolist():
            ch = plan.children[first:first + n]
            P, B, C = (mat(ch[0][k]).copy() for k in (0, 1, 3))
            h, c = view(ch[0][4], d).copy(), view(ch[0][5], d).copy()
            for r in ch[1:]:
                P2, B2, C2 = (mat(r[k]) for k in (0, 1, 3))
                h2, c2 = view(r[4], d), view(r[5], d)
                se, sL = np.zeros(d), np.zeros((d, d))
                for s in r[6:9]:
                    e, Lm = msg(s)
                    se, sL = se + e, sL + Lm
                Mi = np.linalg.inv(C + sL + P2)
                gv = c + se + h2
                P, h = P - B.T @ Mi @ B, h + B.T @ Mi @ gv
                C, c = C2 - B2 @ Mi @ B2.T, c2 + B2 @ Mi @ gv
                B = B2 @ Mi @ B
            view(out, plan.pot)[:] = np.concatenate([P.ravel(), B.ravel(), B.T.ravel(), C.ravel(), h, c])
    for jobs in plan.walk_launches:
        for _, first, n in jobs.tolist():
            for st in plan.steps[first:first + n]:
                e_in, L_in = view(st[6], d).copy(), np.zeros((d, d))
                for s in st[0:3]:
                    e, Lm = msg(s)
                    e_in, L_in = e_in + e, L_in + Lm
                P, Bt, C = (mat(st[k]) for k in (3, 4, 5))
                Mi = np.linalg.inv(L_in + P)
                out = view(st[8], d + dd)
                out[:d] = view(st[7], d) + Bt.T @ Mi @ e_in
                out[d:] = (C - Bt.T @ Mi @ Bt).ravel()


def chain_offsets_inputs(model, b):
    """A chain of tests/anisotropic.chain (x_t = A x_{t-1} + b_t + w, y_t = H x_t + c_t + v, every y observed) in the slot space of
    tests/test_chain64_plan.py: slot p = the likelihood's message into position p, npos + l / npos + nlinks + l = the forward / backward
    message of link l.  Returns what OffsetsPlan64 and run_plan_offsets take, the g rows of the links' slots included."""
    from cortex.jl_amd import _lib as L

    d = model.dim
    (A, Q), (Hm, R) = model.psets[0], model.psets[1]
    Qi, Ri = np.linalg.inv(Q), np.linalg.inv(R)
    T = len(model.x_ids)
    pos = {int(x): t for t, x in enumerate(model.x_ids)}
    data = {int(v): np.asarray(y, float) for v, y in zip(model.data_var, np.asarray(model.data_y).reshape(len(model.data_var), d))}
    ends = {}
    for v, f, r in zip(model.edge_var.tolist(), model.edge_fac.tolist(), model.edge_role.tolist()):
        ends.setdefault(f, {})[r] = v
    sets = dict(zip(model.factor_ids.tolist(), np.asarray(model.factor_var).astype(int).tolist()))
    npos, nlinks = T, T - 1
    nslots = npos + 2 * nlinks
    f2v = np.full((nslots, d + d * d), np.nan)
    goff = np.zeros((nslots, d))
    for f, s in sets.items():
        vo, vi = ends[f][L.ROLE_OUT], ends[f][L.ROLE_IN]
        bf = np.asarray(b.get(f, np.zeros(d)), float)
        if s == 1:      # the likelihood y = H x + c + v, y observed: the message k_point64 writes into x, eta = g_in + H' R^-1 y
            t = pos[vi]
            f2v[t, :d] = -Hm.T @ Ri @ bf + Hm.T @ Ri @ data[vo]
            f2v[t, d:] = (Hm.T @ Ri @ Hm).ravel()
        else:           # the transition x_{t+1} = A x_t + b + w: link t; its slot at the OUT end is `to`, at the IN end `from`
            t = pos[vi]
            assert pos[vo] == t + 1
            g_out, g_in, _ = linear_terms(A, Q, bf)
            goff[npos + t] = g_out
            goff[npos + nlinks + t] = g_in
    ls = np.arange(nlinks, dtype=np.int32)
    side = np.full((npos, 3), -1, dtype=np.int32)
    side[:, 0] = np.arange(npos)
    fw = np.concatenate([(A.T @ Qi @ A).ravel(), (Qi @ A).ravel(), Qi.ravel()])
    bw = np.concatenate([Qi.ravel(), (A.T @ Qi).ravel(), (A.T @ Qi @ A).ravel()])
    return dict(d=d, npos=npos, nlinks=nlinks, nslots=nslots, link_pos=ls.copy(), frm=npos + nlinks + ls, to=npos + ls,
                tab_fwd=np.zeros(nlinks, np.int32), tab_bwd=np.ones(nlinks, np.int32), head_f=ls == 0, head_b=ls == nlinks - 1, side=side,
                ptab=np.concatenate([fw, bw]), btab=np.concatenate([(Qi @ A).T.ravel(), (A.T @ Qi).T.ravel()]), f2v=f2v, goff=goff)
