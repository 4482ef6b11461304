// cx_evidence_mfma_terms.h — the term of cx_log_evidence_mfma as one wave computes it, shared by its two entry points:
// k_evm_terms (cx_evidence_mfma.hip) and, for a handle with factor offsets, k_evm_terms_off (cx_evidence_mfma_off.hip).  Two translation
// units on purpose: with both kernels in one, hipcc's inliner saw more callers of the helpers it decides about itself and the plain
// 1 x 1 instance came out two registers larger than it was; apart, the plain kernels compile to what they were.
#pragma once
#include "cx_evidence_mfma_core.h"
#include "cx_mfma_reader.h"

namespace cx {
namespace evm {

using namespace w64;

// term record (8 int32): {kind, rule-table index, A offset, A count, B offset, B count, y0, y1}; A and B are runs of message slots in `srcs`
//   kVar      B = every slot of the variable, y0 = d_i            kOpaque  B = the slot of the opaque message
//   kFacFree  table 2 set + 1 (towards IN), A = the OUT variable's other slots, B = the IN variable's other slots, y0 / y1 = the factor's
//             OUT / IN slot (read with offsets only)
//   kFacObs   table towards the free end, B = the free variable's other slots, y0 = the observed end's slot (its datum: v2f), y1 = the
//             free end's slot (read with offsets only)
//   kFacBoth  table 2 set + 1, y0 = the OUT end's slot, y1 = the IN end's slot
// Factor offsets (cx_set_factor_offsets_mfma; OFF, entry points of their own): with r = x_out - A x_in - b the potential gains
// g_out'x_out + g_in'x_in - ½ κ, g by slot (goff: [nslots][KD], zero above the user's dim) and κ = b'Q⁻¹b at both slots of the factor (kap):
//   kFacFree  η_out += g_out before the first factorisation, h += g_in after the Gram pass, -½ κ
//   kFacObs   h = B y + g_free,  + y'g_obs - ½ κ                kFacBoth  r'Q⁻¹r += κ - 2 y_o'g_out - 2 y_i'g_in
constexpr int kVar = 0, kOpaque = 1, kFacFree = 2, kFacObs = 3, kFacBoth = 4;
constexpr int kTB = 256;      // terms per block of k_evm_part

// a slot's vector of goff in the column layout (lane (g, c): entry 16 j + c)
template <int NT>
__device__ __forceinline__ void load_g(const double *__restrict__ goff, const int slot, double (&gcv)[NT], const int c) {
#pragma unroll
    for (int j = 0; j < NT; j++) gcv[j] = goff[(int64_t)slot * (16 * NT) + 16 * j + c];
}

// one wave per term.  ptab: [table][P | B | C], btab: [table] B' (upload_ptab); ldq[set] = log det 2πQ of the real block; u: the user's dim
template <int NT, bool OFF>
__device__ __forceinline__ void evm_term(int nterm, const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab,
                                         const double *__restrict__ btab, const double *__restrict__ ldq, const double *__restrict__ f2v,
                                         const double *__restrict__ v2f, const double *__restrict__ goff, const double *__restrict__ kap, const int u,
                                         double *__restrict__ tval, uint8_t *__restrict__ tflag, double *S, double (*Vs)[16 * kLdT], double *ZS) {
    // (S, Vs, ZS: the entry point's own LDS)
    constexpr int KD = 16 * NT, KM = KD + KD * KD, NU = NT * (NT + 1) / 2;
    // Workgroups go to the eight XCDs in turn, each with an L2 of its own: XCD x takes the x-th eighth of the terms in index order, so
    // that terms next to each other in the list — the host sorts them by variable: they share most of their message records — run at
    // about the same time behind ONE L2
    const int per = (nterm + 7) >> 3, w = (blockIdx.x & 7) * per + (blockIdx.x >> 3);
    if (w >= nterm) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mo = g * KD + c;
    const int32_t *t = rec + 8 * (int64_t)w;
    const int kind = t[0], tab_i = t[1], a_off = t[2], a_n = t[3], b_off = t[4], b_n = t[5], y0 = t[6], y1 = t[7];
    const double *tab = ptab + (int64_t)(tab_i < 0 ? 0 : tab_i) * 3 * KD * KD;
    const double *bt = btab + (int64_t)(tab_i < 0 ? 0 : tab_i) * KD * KD;
    const double hl2pi = 0.5 * u * ev::kLog2Pi;

    if (kind == kFacBoth) {      // log N(y_o; A y_i, Q): r'Q⁻¹r = y_o'Q⁻¹y_o - 2 y_o'(Q⁻¹A y_i) + y_i'(A'Q⁻¹A) y_i from the table towards IN
        double orv[NT][4], ocv[NT], irv[NT][4], icv[NT], po[NT], bi[NT], ci[NT];
        load_y<NT>(v2f + (int64_t)y0 * KM, orv, ocv, g, c);
        load_y<NT>(v2f + (int64_t)y1 * KM, irv, icv, g, c);
        xty<NT>(tab, orv, po, mo);                       // Q⁻¹ y_o (P is symmetric)
        xty<NT>(tab + KD * KD, irv, bi, mo);             // B' y_i = Q⁻¹A y_i
        xty<NT>(tab + 2 * KD * KD, irv, ci, mo);         // C y_i
        double q = dot_cv<NT>(ocv, po, g, c, u) - 2.0 * dot_cv<NT>(ocv, bi, g, c, u) + dot_cv<NT>(icv, ci, g, c, u);
        if constexpr (OFF) {
            double go[NT], gi[NT];
            load_g<NT>(goff, y0, go, c);
            load_g<NT>(goff, y1, gi, c);
            q += kap[y0] - 2.0 * dot_cv<NT>(ocv, go, g, c, u) - 2.0 * dot_cv<NT>(icv, gi, g, c, u);
        }
        const bool undef = __builtin_isnan(q);
        if (lane == 0) { tval[w] = undef ? 0.0 : -0.5 * ldq[tab_i >> 1] - 0.5 * q; tflag[w] = undef ? ev::kTermUndef : 0; }
        return;
    }

    d4 Sm[NU];
    double hcv[NT], zrv[NT][4];
#pragma unroll
    for (int i = 0; i < NU; i++) Sm[i] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NT; j++) hcv[j] = 0.0;
    double cst = 0.0;      // what the term holds besides ½ h'S⁻¹h - ½ log det S of the last factorisation
    bool pd_a = true, undef_a = false;      // the first factorisation of a factor with two free ends: positive definite; its inputs undefined
    if (kind == kFacFree) {
        // the rule towards IN on m_{out→a} (rule64_body's passes), its message left in Sm / hcv
        d4 M[NU];
        double wcv[NT];
#pragma unroll
        for (int j = 0; j < NT; j++) wcv[j] = 0.0;
        load_upper<NT>(M, [&](int k) { return ((gcdp)tab)[mo + k]; });
        add_sources<NT>(M, wcv, f2v, srcs + a_off, a_n, mo, c);
        if constexpr (OFF) {
            double go[NT];
            load_g<NT>(goff, y0, go, c);
#pragma unroll
            for (int j = 0; j < NT; j++) wcv[j] += go[j];
        }
        undef_a = __builtin_isnan(bcast(M[0][0], 0)) || __builtin_isnan(bcast(wcv[0], 0));      // (whole messages are NaN together)
        double ld1, q1;
        factor_solve<NT>(M, wcv, zrv, S, Vs, g, c, u, ld1, q1, pd_a);
        cst = -0.5 * ldq[tab_i >> 1] + 0.5 * q1 - 0.5 * ld1 + 2.0 * hl2pi;
        park_z<NT>(ZS, zrv, g);
        // Yt = U^-T B', then Λ' = C - Yt'Yt (upper tiles), η' = Yt' z
        d4 Y[NT][NT];
        solve_block_cols<NT, false>(Y, M, Vs, [&](int k) { return ((gcdp)bt)[mo + k]; }, g, c);
        gram_pass<NT, -1>(Sm, Y, ZS, [&](int k) { return ((gcdp)tab)[2 * KD * KD + mo + k]; }, [&](int a, double v) { hcv[a] = v; }, g);
        if constexpr (OFF) {
            double gi[NT];
            load_g<NT>(goff, y1, gi, c);
#pragma unroll
            for (int j = 0; j < NT; j++) hcv[j] += gi[j];
            cst -= 0.5 * kap[y0];
        }
    } else if (kind == kFacObs) {      // (kVar, kOpaque: S and h start at zero)
        double yrv[NT][4], ycv[NT], py[NT];
        load_y<NT>(v2f + (int64_t)y0 * KM, yrv, ycv, g, c);
        xty<NT>(tab, yrv, py, mo);                       // P y
        xty<NT>(bt, yrv, hcv, mo);                       // B y
        cst = -0.5 * ldq[tab_i >> 1] - 0.5 * dot_cv<NT>(ycv, py, g, c, u) + hl2pi;
        if constexpr (OFF) {
            double gobs[NT], gfree[NT];
            load_g<NT>(goff, y0, gobs, c);
            load_g<NT>(goff, y1, gfree, c);
#pragma unroll
            for (int j = 0; j < NT; j++) hcv[j] += gfree[j];
            cst += dot_cv<NT>(ycv, gobs, g, c, u) - 0.5 * kap[y0];
        }
        load_upper<NT>(Sm, [&](int k) { return ((gcdp)tab)[2 * KD * KD + mo + k]; });
    }
    add_sources<NT>(Sm, hcv, f2v, srcs + b_off, b_n, mo, c);
    // Undefined: an INPUT is NaN (whole messages are NaN together; a NaN datum reaches hcv and cst).  A first factorisation that is not
    // positive definite also leaves NaN in Λ', η' and cst: that term is "not positive definite", so with two free ends the inputs of the
    // second stage are looked at themselves (Λ[0][0] and η[0] of every source record), not through Sm
    bool undef = undef_a;
    if (kind == kFacFree) undef = any_nan_record<NT>(undef, f2v, srcs + b_off, b_n);
    else undef = __builtin_isnan(bcast(Sm[0][0], 0)) || __builtin_isnan(bcast(hcv[0], 0)) || __builtin_isnan(cst);
    double ld, q;
    bool pd;
    factor_solve<NT>(Sm, hcv, zrv, S, Vs, g, c, u, ld, q, pd);
    if (lane != 0) return;
    double val;
    unsigned fl = 0;
    if (kind == kOpaque) {
        val = (!undef && pd) ? 0.5 * ld - 0.5 * q - hl2pi : 0.0;      // improper (a flat forecast end) or undefined: no constant
    } else {
        const bool npd = !undef && !(pd && pd_a);
        if (kind == kVar) { val = (double)(1 - y0) * (0.5 * q - 0.5 * ld + hl2pi); fl = ev::kTermVar; }
        else val = cst + 0.5 * q - 0.5 * ld;
        fl |= (undef ? ev::kTermUndef : 0u) | (npd ? ev::kTermNpd : 0u);
        if (undef || npd) val = 0.0;
    }
    tval[w] = val;
    tflag[w] = (uint8_t)fl;
}

// k_evm_terms_off for the handle's tile count (cx_evidence_mfma_off.hip): the arguments of k_evm_terms, g and κ from the handle
void launch_terms_off(cx_handle *h, int n, const int32_t *d_rec, const int32_t *d_srcs, const double *d_ldq, double *d_tval, uint8_t *d_tflag);

}  // namespace evm
}  // namespace cx
