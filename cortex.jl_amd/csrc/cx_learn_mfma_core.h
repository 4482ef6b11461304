// cx_learn_mfma_core.h — the wave's work on one two-variable factor at the matrix-core dims (lm_factors; the algebra is derived at the
// head of cx_learn_mfma.hip) and the host cache of its callers.  Two translation units hold its kernel entry points: cx_learn_mfma.hip
// (cx_factor_beliefs_mfma, cx_factor_statistics_mfma) and cx_disturb_mfma.hip (cx_factor_disturbances_mfma).  They are apart because the
// inliner's decisions, and with them an instance's registers, follow the number of callers in a unit (profiles/factor_offsets_mfma.md).
#pragma once
#include "cx_evidence_mfma_core.h"
#include "cx_mfma_reader.h"

namespace cx {
namespace lm {

using namespace w64;

// waves of one launch = wave workspaces: what the chip holds at once (1024 SIMDs; two waves on each at 1 x 1 and 2 x 2 tiles, one at 4 x 4)
constexpr int max_waves(int KD) { return KD == 64 ? 1024 : 2048; }
constexpr int kNMat = 6;             // KD x KD matrices of a wave workspace

__host__ __device__ constexpr int64_t ws_doubles(int KD) { return (int64_t)kNMat * KD * KD + 4 * KD; }

// What one pass stored, every lane of the wave may read after this.  The lanes of ONE wave exchange data through device memory here,
// with no atomic to synchronise on, so the memory model's fences alone promise nothing: what makes it work is stated explicitly.
// (i) the wave runs in lockstep and is alone in its workgroup; (ii) s_waitcnt vmcnt(0): every store of the pass has been acknowledged
// before the next pass issues a load — written out, as factor_solve writes its LDS waits, not left to how a fence happens to be
// lowered; (iii) a compute unit's vector L1 is write-through and coherent for the stores of its own waves (not in threadgroup-split
// mode, which HIP does not use), so no cache invalidate is needed.  The fences keep the COMPILER from moving accesses across.
__device__ __forceinline__ void ws_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// A matrix (or vector) behind a buffer descriptor (cx_mv64w_core.h: BufAcc): element = base + ONE per-lane part + a wave-uniform constant
// that sits in a scalar register or the instruction.  With plain pointers every tile row out of reach of the 13-bit immediate costs a
// 64-bit per-lane address, all of them hoisted out of the factor loop: the kernel spilled at every tile count.
struct Mat {
    BufAcc b;
    int off;
    __device__ __forceinline__ double ld(int lane_part, int cst) const { return b.ld(lane_part, off + cst); }
    __device__ __forceinline__ void st(int lane_part, int cst, double v) const { b.st(lane_part, off + cst, v); }
};

// dst = add + alpha X'Y (has_add or 0), all NT x NT tiles, operands read tile by tile; dst is none of the operands
template <int NT>
__device__ __forceinline__ void mm_tn(const Mat dst, const Mat X, const Mat Y, const bool has_add, const Mat add, const double alpha, const int mo) {
    constexpr int KD = 16 * NT;
#pragma unroll 1
    for (int a = 0; a < NT; a++) {      // one block row of the result per round trip to memory: NT accumulators, 2 NT + NT² operand tiles in flight
        d4 acc[NT];
#pragma unroll
        for (int b = 0; b < NT; b++) acc[b] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int j = 0; j < NT; j++) {
            d4 T;
#pragma unroll
            for (int r = 0; r < 4; r++) T[r] = X.ld(mo, (16 * j + 4 * r) * KD + 16 * a);
#pragma unroll
            for (int b = 0; b < NT; b++) {
                d4 Sx;
#pragma unroll
                for (int r = 0; r < 4; r++) Sx[r] = Y.ld(mo, tile_const_n<NT>(j, b, r));
                acc[b] = tts(T, Sx, acc[b]);
            }
        }
#pragma unroll
        for (int b = 0; b < NT; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int o = (16 * a + 4 * r) * KD + 16 * b;
                dst.st(mo, o, alpha * acc[b][r] + (has_add ? add.ld(mo, o) : 0.0));
            }
    }
}

// every element of a KD x KD matrix: dst = alpha src (has_src or 0)
template <int NT>
__device__ __forceinline__ void fill(const Mat dst, const bool has_src, const Mat src, const double alpha, const int lane) {
    constexpr int KD = 16 * NT;
#pragma unroll 1
    for (int k = 0; k < KD * KD; k += 4 * 64) {      // (KD² is a multiple of 256)
        double x[4];
#pragma unroll
        for (int i = 0; i < 4; i++) x[i] = has_src ? alpha * src.ld(lane, k + 64 * i) : 0.0;
#pragma unroll
        for (int i = 0; i < 4; i++) dst.st(lane, k + 64 * i, x[i]);
    }
}

// dst = U^-T X, one block column at a time (U: the off-diagonal tiles of M after factor_solve, V_k = U_kk⁻¹ in Vs); IDENT: X = I
template <int NT, bool IDENT>
__device__ __forceinline__ void solve_cols(const d4 (&M)[NT * (NT + 1) / 2], double (*Vs)[16 * kLdT], const Mat X, const Mat dst, const int g, const int c, const int mo) {
#pragma unroll
    for (int b = 0; b < NT; b++) {
        asm volatile("" ::: "memory");      // (one block column in flight at a time)
        d4 Y[NT];
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) Y[j][r] = IDENT ? ((j == b && g + 4 * r == c) ? 1.0 : 0.0) : X.ld(mo, tile_const_n<NT>(j, b, r));
        evm::solve_col<NT>(Y, M, Vs, IDENT ? b : 0, g, c);      // (U^-T is lower triangular: the tiles above the diagonal stay zero)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) dst.st(mo, tile_const_n<NT>(j, b, r), Y[j][r]);
    }
}

// out[a] (lane (g, c): entry 16 a + c) = (X'y)[16 a + c], y in the row layout
template <int NT>
__device__ __forceinline__ void xty_ws(const Mat X, const double (&yrv)[NT][4], double (&out)[NT], const int mo) {
#pragma unroll
    for (int a = 0; a < NT; a++) {
        double x[NT][4], p = 0.0;      // (the loads of a block column issued together, the products after them)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) x[j][r] = X.ld(mo, tile_const_n<NT>(j, a, r));
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) p += x[j][r] * yrv[j][r];
        out[a] = sum_groups(p);
    }
}

// factor record (8 int32), by factor index: {flags (-1: not covered; bit 0: OUT observed, bit 1: IN observed), parameter set, A offset,
// A count, B offset, B count, OUT slot, IN slot}; A / B: the OUT / IN variable's other message slots in `srcs` (a free end only)
// wbeg (null: wave w takes partial w): the partials of wave w; pbeg (null: partial p is item p): the items of partial p; items: factor indices
// ptab: [table][P | B | C], btab: [table] B' (upload_ptab); atab: [set][A | A']; u: the user's dim
//
// MODE: what becomes of a factor's moments.  kBeliefs: f = x_out, one factor per wave, its row of 2u + 4u² written out.  kStatistics:
// f = r, added to the partial's row.  kDisturbances: f = r again (stages 1 to 3 are the statistics'), written PER FACTOR: wave w of
// nwave walks the contiguous run [rw.row0 + w n / nwave, rw.row0 + (w + 1) n / nwave) of `items` (n = rw.n; wbeg, pbeg, acc_all and meta
// are not read) and leaves for row i
//   rw.scores[2 i] = t = s + q,  rw.scores[2 i + 1] = q   with s = Σ_ab (Q⁻¹)_ab Cov(r)_ab and q = E[r]'Q⁻¹E[r] over the real block, Q⁻¹ the P
//                                block of the rule table towards IN: E[r'Q⁻¹r | data] and the squared length of the mean
//   rw.rval[i] = t, rw.rflag[i] = mfr::kRowOk / kRowUndefined / kRowImproper (an unscored row: 0 and NaN scores)
//   out (or null) row i - rw.row0 = E[r] (u), Cov(r) (u², row-major, both triangles as the last product left them), NaN when unscored
// Every workspace matrix a row reads it has written itself and the sums s, q run over fixed lanes in a fixed order: a row's bits do
// not depend on the wave that took it nor on the rows before it.
enum Mode { kBeliefs = 0, kStatistics = 1, kDisturbances = 2 };
struct RowsOut {
    int row0 = 0, n = 0;
    double *rval = nullptr, *scores = nullptr;
    uint8_t *rflag = nullptr;
};

template <int NT, int MODE, bool OFF>
__device__ __forceinline__ void lm_factors(const int nwave, const int32_t *__restrict__ wbeg, const int32_t *__restrict__ pbeg, const int32_t *__restrict__ items,
                                           const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab,
                                           const double *__restrict__ btab, const double *__restrict__ atab, const double *__restrict__ f2v,
                                           const double *__restrict__ v2f, const double *__restrict__ goff, const double *__restrict__ boff, const int u,
                                           double *ws_all, double *acc_all, int32_t *__restrict__ meta, double *__restrict__ out, const RowsOut rw = RowsOut{}) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD, NU = NT * (NT + 1) / 2, DD = KD * KD;
    constexpr bool STATS = MODE != kBeliefs, SUMS = MODE == kStatistics, ROWS = MODE == kDisturbances;      // STATS: f = r
    __shared__ double S[16 * kLdT];
    __shared__ double Vs[NT][16 * kLdT];
    const int w = blockIdx.x;
    if (w >= nwave) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mo = g * KD + c;
    const int na = 2 * u + 3 * u * u, nb = 2 * u + 4 * u * u;
    const double nan = __builtin_nan("");
    const int p0 = (!ROWS && wbeg) ? wbeg[w] : w, p1 = (!ROWS && wbeg) ? wbeg[w + 1] : w + 1;
    for (int p = p0; p < p1; p++) {
        const gdp acc = (gdp)(acc_all + (int64_t)p * na);
        int n_undef = 0, n_npd = 0;
        if (SUMS)
            for (int i = lane; i < na; i += 64) acc[i] = 0.0;
        const int i0 = ROWS ? rw.row0 + (int)((int64_t)w * rw.n / nwave) : pbeg ? pbeg[p] : p;
        const int i1 = ROWS ? rw.row0 + (int)((int64_t)(w + 1) * rw.n / nwave) : pbeg ? pbeg[p + 1] : p + 1;
        for (int it = i0; it < i1; it++) {
            // Every address below is a wave-uniform base plus a constant: left alone, hipcc hoists them ALL out of this loop as 64-bit
            // per-lane addresses (several hundred registers, spilled).  The bases are made opaque once per factor instead.
            const double *ptab_ = ptab, *btab_ = btab, *atab_ = atab, *f2v_ = f2v, *v2f_ = v2f;
            double *ws_ = ws_all + (int64_t)w * ws_doubles(KD);
            asm volatile("" : "+s"(ptab_), "+s"(btab_), "+s"(atab_), "+s"(f2v_), "+s"(v2f_), "+s"(ws_));
            const double *goff_ = goff, *boff_ = boff;
            if constexpr (OFF) asm volatile("" : "+s"(goff_), "+s"(boff_));
            const gdp ws = (gdp)ws_;
            const gdp P0 = ws, P2 = ws + 2 * DD, P4 = ws + 4 * DD, vf = ws + kNMat * DD, vx = vf + KD;      // (the element-wise passes at the end)
            const BufAcc wsb = buf_of((gcdp)ws);
            const Mat W0{wsb, 0}, W1{wsb, DD}, W2{wsb, 2 * DD}, W3{wsb, 3 * DD}, W4{wsb, 4 * DD}, W5{wsb, 5 * DD};
            const int32_t *t = rec + 8 * (int64_t)items[it];
            const int fl = t[0], set = t[1], a_off = t[2], a_n = t[3], b_off = t[4], b_n = t[5], so = t[6], si = t[7];
            const bool oo = (fl & 1) != 0, oi = (fl & 2) != 0;
            const BufAcc tabb = buf_of((gcdp)(ptab_ + (int64_t)(2 * set + 1) * 3 * DD)), atb = buf_of((gcdp)(atab_ + (int64_t)set * 2 * DD));
            const Mat tabP{tabb, 0}, tabC{tabb, 2 * DD}, bt{buf_of((gcdp)(btab_ + (int64_t)(2 * set + 1) * DD)), 0}, Am{atb, 0}, At{atb, DD};
            double hcv[NT], m0cv[NT], mucv[NT], zrv[NT][4];
#pragma unroll
            for (int j = 0; j < NT; j++) hcv[j] = 0.0;
            bool undef = false, pd_a = true, pd = true;
            double ld, q;
            if (!oo) {
                // ---- 1. OUT is eliminated: W1 = W_M, W2 = Yt, W3 = M⁻¹, W5 = J' -------------------------------------------------------
                d4 M[NU];
                double wcv[NT];
#pragma unroll
                for (int j = 0; j < NT; j++) wcv[j] = 0.0;
                evm::load_upper<NT>(M, [&](int k) { return tabP.ld(mo, k); });
                evm::add_sources<NT>(M, wcv, f2v_, srcs + a_off, a_n, mo, c);
                if constexpr (OFF) {      // η_o + g_out
                    const gcdp go = (gcdp)(goff_ + (int64_t)so * KD);
#pragma unroll
                    for (int j = 0; j < NT; j++) wcv[j] += go[16 * j + c];
                }
                undef = __builtin_isnan(bcast(M[0][0], 0)) || __builtin_isnan(bcast(wcv[0], 0));      // (whole messages are NaN together)
                if (STATS) {      // Λ_o whole, for K = M⁻¹ Λ_o A
#pragma unroll 1
                    for (int e = 0; e < NT * NT; e++) {      // a tile per round trip
                        const int o = (e / NT * 16) * KD + 16 * (e % NT);
                        d4 x = d4{0.0, 0.0, 0.0, 0.0};
                        for (int s = 0; s < a_n; s++) {
                            const gcdp pr = (gcdp)(f2v_ + (int64_t)srcs[a_off + s] * KM);
#pragma unroll
                            for (int r = 0; r < 4; r++) x[r] += pr[KD + mo + o + 4 * r * KD];
                        }
#pragma unroll
                        for (int r = 0; r < 4; r++) W0.st(mo, o + 4 * r * KD, x[r]);
                    }
                }
                evm::factor_solve<NT>(M, wcv, zrv, S, Vs, g, c, u, ld, q, pd_a);
                solve_cols<NT, true>(M, Vs, W1, W1, g, c, mo);
                if (!oi) solve_cols<NT, false>(M, Vs, bt, W2, g, c, mo);
                ws_sync();
                mm_tn<NT>(W3, W1, W1, false, W1, 1.0, mo);
                xty_ws<NT>(W1, zrv, m0cv, mo);
                if (!oi) xty_ws<NT>(W2, zrv, hcv, mo);      // η' = Yt'z
                if (STATS) mm_tn<NT>(W4, W0, Am, false, W0, 1.0, mo);      // Λ_o A (Λ_o is symmetric)
                ws_sync();
                mm_tn<NT>(W5, STATS ? W4 : bt, W3, false, W3, STATS ? -1.0 : 1.0, mo);
            } else {
                double yrv[NT][4];
                evm::load_y<NT>(v2f_ + (int64_t)so * KM, yrv, m0cv, g, c);
                undef = __builtin_isnan(bcast(m0cv[0], 0));
                fill<NT>(W3, false, W3, 0.0, lane);
                fill<NT>(W5, STATS, At, -1.0, lane);      // J' = -A' (r = y - A x_in) or 0
                if (!oi) xty_ws<NT>(bt, yrv, hcv, mo);      // η' = B y
            }
            if (!oi) {
                // ---- 2. IN: W1 = W_S, W2 = Σ_ii -----------------------------------------------------------------------------------
                d4 Sm[NU];      // Λ' = C - Yt'Yt (Yt = 0 behind an observed OUT end), upper tiles
#pragma unroll
                for (int a = 0; a < NT; a++)
#pragma unroll
                    for (int b = a; b < NT; b++) {
                        asm volatile("" ::: "memory");      // (one tile in flight at a time)
                        d4 G = d4{0.0, 0.0, 0.0, 0.0};
                        if (!oo) {
#pragma unroll
                            for (int j = 0; j < NT; j++) {
                                d4 Ya, Yb;
#pragma unroll
                                for (int r = 0; r < 4; r++) { Ya[r] = W2.ld(mo, tile_const_n<NT>(j, a, r)); Yb[r] = W2.ld(mo, tile_const_n<NT>(j, b, r)); }
                                G = tts(Ya, Yb, G);
                            }
                        }
#pragma unroll
                        for (int r = 0; r < 4; r++) Sm[utn<NT>(a, b)][r] = tabC.ld(mo, tile_const_n<NT>(a, b, r)) - G[r];
                    }
                if (!oo) undef = evm::any_nan_record<NT>(undef, f2v_, srcs + b_off, b_n);      // (a first factorisation that failed left NaN in Λ', η')
                evm::add_sources<NT>(Sm, hcv, f2v_, srcs + b_off, b_n, mo, c);
                if constexpr (OFF) {      // η_i + η' + g_in
                    const gcdp gi = (gcdp)(goff_ + (int64_t)si * KD);
#pragma unroll
                    for (int j = 0; j < NT; j++) hcv[j] += gi[16 * j + c];
                }
                if (oo) undef = undef || __builtin_isnan(bcast(Sm[0][0], 0)) || __builtin_isnan(bcast(hcv[0], 0));
                evm::factor_solve<NT>(Sm, hcv, zrv, S, Vs, g, c, u, ld, q, pd);
                solve_cols<NT, true>(Sm, Vs, W1, W1, g, c, mo);
                ws_sync();
                mm_tn<NT>(W2, W1, W1, false, W1, 1.0, mo);
                xty_ws<NT>(W1, zrv, mucv, mo);
            } else {
                double yrv[NT][4];
                evm::load_y<NT>(v2f_ + (int64_t)si * KM, yrv, mucv, g, c);
                undef = undef || __builtin_isnan(bcast(mucv[0], 0));
                fill<NT>(W2, false, W2, 0.0, lane);
            }
            // ---- 3. W0 = N = Σ_ii J', W4 = Cov(f) = M⁻¹ + J N, vf = E[f], vx = μ_i ---------------------------------------------------
            double murv[NT][4], fcv[NT];
#pragma unroll
            for (int j = 0; j < NT; j++)
#pragma unroll
                for (int r = 0; r < 4; r++) murv[j][r] = cv_to_rv(mucv[j], g, r);
            ws_sync();
            mm_tn<NT>(W0, W2, W5, false, W2, 1.0, mo);
            xty_ws<NT>(W5, murv, fcv, mo);
            ws_sync();
            mm_tn<NT>(W4, W5, W0, true, W3, 1.0, mo);
            if (g == 0) {
#pragma unroll
                for (int j = 0; j < NT; j++) {
                    double f = m0cv[j] + fcv[j];
                    if constexpr (OFF && STATS) f -= ((gcdp)(boff_ + (int64_t)so * KD))[16 * j + c];      // r = x_out - A x_in - b
                    vf[16 * j + c] = f; vx[16 * j + c] = mucv[j];
                }
            }
            ws_sync();
            const bool npd = !undef && !(pd_a && pd);
            if (ROWS) {
                // s = Σ P .* Cov(r), q = vf'P vf over the real block: four elements per round trip and lane, the lanes added by wave_sum
                const bool bad = undef || npd;
                double ps = 0.0, pq = 0.0;
#pragma unroll 1
                for (int k0 = lane; k0 < u * u; k0 += 4 * 64) {
                    double pv[4], cv[4], fa[4], fb[4];
#pragma unroll
                    for (int k = 0; k < 4; k++) {
                        const int i = k0 + 64 * k, ii = i < u * u ? i : 0, a = ii / u, b = ii - a * u;
                        pv[k] = i < u * u ? tabP.ld(a * KD + b, 0) : 0.0;
                        cv[k] = P4[a * KD + b]; fa[k] = vf[a]; fb[k] = vf[b];
                    }
#pragma unroll
                    for (int k = 0; k < 4; k++) { ps += pv[k] * cv[k]; pq += pv[k] * (fa[k] * fb[k]); }
                }
                const double s = evm::wave_sum(ps), q2 = evm::wave_sum(pq), tt = s + q2;
                if (lane == 0) {
                    rw.rval[it] = bad ? 0.0 : tt;
                    rw.rflag[it] = (uint8_t)(undef ? mfr::kRowUndefined : npd ? mfr::kRowImproper : mfr::kRowOk);
                    rw.scores[2 * (int64_t)it] = bad ? nan : tt;
                    rw.scores[2 * (int64_t)it + 1] = bad ? nan : q2;
                }
                if (out) {
                    double *o = out + (int64_t)(it - rw.row0) * (u + u * u);
                    for (int i = lane; i < u; i += 64) o[i] = bad ? nan : vf[i];
                    for (int i = lane; i < u * u; i += 64) {
                        const int a = i / u, b = i - a * u;
                        o[u + i] = bad ? nan : P4[a * KD + b];
                    }
                }
            } else if (SUMS) {
                n_undef += undef ? 1 : 0;
                n_npd += npd ? 1 : 0;
                if (!undef && !npd) {
                    for (int i = lane; i < u; i += 64) { acc[i] += vf[i]; acc[u + i] += vx[i]; }
#pragma unroll 1
                    for (int i0 = lane; i0 < u * u; i0 += 4 * 64) {      // four elements per round trip, the loads before the stores
                        double rr[4], rx[4], xx[4];
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int i = i0 + 64 * k, ii = i < u * u ? i : 0, a = ii / u, b = ii - a * u;
                            rr[k] = acc[2 * u + ii] + (P4[a * KD + b] + vf[a] * vf[b]);
                            rx[k] = acc[2 * u + u * u + ii] + (P0[b * KD + a] + vf[a] * vx[b]);
                            xx[k] = acc[2 * u + 2 * u * u + ii] + (P2[a * KD + b] + vx[a] * vx[b]);
                        }
#pragma unroll
                        for (int k = 0; k < 4; k++) {
                            const int i = i0 + 64 * k;
                            if (i < u * u) { acc[2 * u + i] = rr[k]; acc[2 * u + u * u + i] = rx[k]; acc[2 * u + 2 * u * u + i] = xx[k]; }
                        }
                    }
                }
            } else {
                const bool bad = undef || npd;
                double *o = out + (int64_t)it * nb;
                for (int i = lane; i < 2 * u; i += 64) o[i] = bad ? nan : (i < u ? vf[i] : vx[i - u]);
                for (int i = lane; i < 4 * u * u; i += 64) {
                    const int a = i / (2 * u), b = i - a * 2 * u;
                    const double x = a < u ? (b < u ? P4[a * KD + b] : P0[(b - u) * KD + a]) : (b < u ? P0[(a - u) * KD + b] : P2[(a - u) * KD + (b - u)]);
                    o[2 * u + i] = bad ? nan : x;
                }
            }
        }
        if (SUMS && lane == 0) { meta[2 * p] = n_undef; meta[2 * p + 1] = n_npd; }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
// The factor records follow the graph and WHICH variables are observed (vinfo_epoch: cx_derived.h), the A table the rule parameters
// (param_epoch); the lists of a grouping depend on the graph, the observed flags and the caller's arrays alone (a factor's parameter set
// is fixed by the graph) and are kept until another grouping replaces them or the records are rebuilt: an EM loop uploads them once
struct Cache {
    bool built = false;
    uint64_t vinfo_epoch = 0;
    std::vector<int32_t> kind, set;      // by factor index: -1 not covered (kind -2: an opaque message), else the record's flags; its parameter set
    int64_t unsupported_fac = -1;
    DevBuf<int32_t> d_rec, d_srcs;
    mfr::ParamTable atab;
    DevBuf<double> d_ws;
    // the grouping
    mfr::RequestKey group_key;      // tag: n_groups; the ids and their groups
    int64_t n_items = 0, n_part = 0, n_wave = 0;
    std::vector<int64_t> group_n;             // factors of every group
    std::vector<int32_t> part_group, h_meta;
    std::vector<double> h_rows;
    DevBuf<int32_t> d_items, d_pbeg, d_wbeg, d_gbeg, d_meta;
    DevBuf<double> d_acc, d_rows;
    // beliefs
    DevBuf<int32_t> d_bitems;
    DevBuf<double> d_bout;
    // disturbances (cx_disturb_mfma.hip): the rows of the last request and the call's whole-call arrays
    mfr::RequestKey rows_key;      // tag: 0; the ids
    int64_t n_drows = 0;
    DevBuf<int32_t> d_ditems;
    DevBuf<double> d_drval, d_dscores, d_dout;
    DevBuf<uint8_t> d_drflag;
    DevBuf<ev::Part> d_dpart;
    mfr::Totals dtotals;
};

// cx_learn_mfma.hip: the refusals of a reader (cx_mfma_reader.h), the cache and its factor records; what a factor that is no row is told
int32_t prepare(cx_handle *h, const std::string &who, const char *small_dims, const char *bad_args, Cache *&out);
std::string no_pair(int64_t id);

}  // namespace lm
}  // namespace cx

