// cx_learn_mfma.hip — cx_factor_beliefs_mfma and cx_factor_statistics_mfma: the joint posterior of every two-variable
// x_out = A x_in + N(0, Q) factor and the EM statistics of cx_factor_statistics at the matrix-core dims (cx_create dim
// 5 .. 64, internal tiles of 16 / 32 / 64), from the stored factor→variable messages and the caller's data.  DESIGN.md §4n.
//
// ONE WAVE per factor, on the pieces of cx_log_evidence_mfma (cx_evidence_mfma_core.h): sums of message records, the blocked Cholesky
// with U in registers, block-column solves U^-T X.  What a factor needs besides is explicit inverses and a handful of KD x KD products;
// at 4 x 4 tiles they do not fit in registers beside U, so every intermediate matrix is PARKED in a workspace of the wave's own in device
// memory (six KD x KD matrices, row-major, plain vector loads and stores; a workgroup-scope fence between a pass that writes one and the
// pass that reads it — the wave is alone in its workgroup) and every product is X'Y read tile by tile from there: tts() contracts over
// tile rows, so the algebra below is arranged to need no other form.
//
// With (P, B, C) = (Q⁻¹, A'Q⁻¹, A'Q⁻¹A) the rule table towards IN, bt = B' = Q⁻¹A, and the leave-one-out messages m_{out→a} = (Λ_o, η_o),
// m_{in→a} = (Λ_i, η_i) summed directly from the other stored messages (opaque ones included):
//   1. OUT goes first:  M = Λ_o + P = U'U,  z = U^-T η_o,  W_M = U^-T (solve against the identity),  Yt = U^-T bt,
//                       M⁻¹ = W_M'W_M,  m0 = M⁻¹η_o = W_M'z,  Λ' = C - Yt'Yt,  η' = Yt'z          (x_out | x_in ~ N(m0 + G x_in, M⁻¹), G = M⁻¹bt)
//   2. IN:              S = Λ_i + Λ' = U_S'U_S,  W_S = U_S^-T,  Σ_ii = W_S'W_S,  μ_i = W_S'(U_S^-T (η_i + η'))
//   3. the pair (f, x_in) with f = m0 + J x_in + N(0, M⁻¹):   N = Σ_ii J' = Cov(x_in, f),   E[f] = m0 + J μ_i,   Cov(f) = M⁻¹ + J N
//        beliefs      f = x_out:           J' = B M⁻¹ = bt'M⁻¹
//        statistics   f = r = x_out - A x_in: J = G - A = -K with K = M⁻¹Λ_o A formed AS SUCH (J' = -(Λ_o A)'M⁻¹): a flat OUT leaf has
//                     Λ_o = 0, K = 0 and Cov(r) = M⁻¹ = Q to the rounding of one inverse; nothing of the size of A Σ_ii A' is cancelled
//   an observed OUT end (datum y):  m0 = y, M⁻¹ = 0, J = 0 (beliefs) or -A (statistics: r = y - A x_in), Λ' = C, η' = B y
//   an observed IN end (datum y):   μ_i = y, Σ_ii = 0; stage 1 as it is (E[x_out] = M⁻¹(η_o + bt y))
// Embedded dims: every matrix is block-diagonal (real block, identity block) and so is every product; rows and sums hold the real
// block only, d below is the user's.
// Factor offsets (cx_set_factor_offsets_mfma; OFF, entry points of their own): x_out = A x_in + b + N(0, Q) puts the linear terms g_out, g_in
//   (goff: by slot, [nslots][KD]) into the factor's potential — η_o + g_out enters stage 1, η_i + η' + g_in stage 2 (an observed OUT end:
//   η' = B y as before) — and the statistics' residual is r = x_out - A x_in - b: E[r] = m0 + J μ_i - b with the factor's own b (boff: by
//   slot, the same layout; it may differ within a group), Cov as it was.
// Undefined / not positive definite: cx_log_evidence_mfma's rules.  An input record (or datum) that is NaN: undefined; a failed pivot of
// either factorisation: not positive definite; with two free ends the inputs of the second stage are looked at themselves.
//
// k_lm_factors<NT, STATS>  a wave walks a contiguous run of PARTIALS (a partial: a contiguous run of factors of one group in the list
//                          sorted by group, then factor index) and adds each factor's 2d + 3d² moments, in order, to the partial's own
//                          row; beliefs: one factor per wave, its row written out
// k_lm_reduce              a group's partials added in index order
// No atomics; the cut into partials and waves depends on the grouping alone: two calls on one state are bit-identical (per handle).
// Sums are plain f64 in that fixed order (not compensated: a run is at most a few hundred noise-sized terms).
// Device workspace: at most W = max_waves(KD) wave workspaces of 6 KD² + 4 KD doubles (W = 1024 at KD = 64, 2048 below), and one row of
// 2d + 3d² doubles per partial, at most W + n_groups of them: it does not grow with the number of factors (KD = 64: 198,656 B + 99,328 B each,
// 305 MB plus n_groups rows at most; KD = 32: 154 MB; KD = 16: 39 MB).  cx_factor_beliefs_mfma goes through its list W factors at a time.
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
template <int NT, bool STATS, bool OFF>
__device__ __forceinline__ void lm_factors(const int nwave, const int32_t *__restrict__ wbeg, const int32_t *__restrict__ pbeg, const int32_t *__restrict__ items,
                                           const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab,
                                           const double *__restrict__ btab, const double *__restrict__ atab, const double *__restrict__ f2v,
                                           const double *__restrict__ v2f, const double *__restrict__ goff, const double *__restrict__ boff, const int u,
                                           double *ws_all, double *acc_all, int32_t *__restrict__ meta, double *__restrict__ out) {
    constexpr int KD = 16 * NT, KM = KD + KD * KD, NU = NT * (NT + 1) / 2, DD = KD * KD;
    __shared__ double S[16 * kLdT];
    __shared__ double Vs[NT][16 * kLdT];
    const int w = blockIdx.x;
    if (w >= nwave) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mo = g * KD + c;
    const int na = 2 * u + 3 * u * u, nb = 2 * u + 4 * u * u;
    const double nan = __builtin_nan("");
    const int p0 = wbeg ? wbeg[w] : w, p1 = wbeg ? wbeg[w + 1] : w + 1;
    for (int p = p0; p < p1; p++) {
        const gdp acc = (gdp)(acc_all + (int64_t)p * na);
        int n_undef = 0, n_npd = 0;
        if (STATS)
            for (int i = lane; i < na; i += 64) acc[i] = 0.0;
        const int i0 = pbeg ? pbeg[p] : p, i1 = pbeg ? pbeg[p + 1] : p + 1;
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
            if (STATS) {
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
        if (STATS && lane == 0) { meta[2 * p] = n_undef; meta[2 * p + 1] = n_npd; }
    }
}

template <int NT, bool STATS, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_lm_factors(const int nwave, const int32_t *__restrict__ wbeg, const int32_t *__restrict__ pbeg, const int32_t *__restrict__ items,
                  const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab, const double *__restrict__ btab,
                  const double *__restrict__ atab, const double *__restrict__ f2v, const double *__restrict__ v2f, const int u, double *ws_all,
                  double *acc_all, int32_t *__restrict__ meta, double *__restrict__ out) {
    lm_factors<NT, STATS, false>(nwave, wbeg, pbeg, items, rec, srcs, ptab, btab, atab, f2v, v2f, nullptr, nullptr, u, ws_all, acc_all, meta, out);
}
// the factors of a handle with factor offsets
template <int NT, bool STATS, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_lm_factors_off(const int nwave, const int32_t *__restrict__ wbeg, const int32_t *__restrict__ pbeg, const int32_t *__restrict__ items,
                      const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab, const double *__restrict__ btab,
                      const double *__restrict__ atab, const double *__restrict__ f2v, const double *__restrict__ v2f, const double *__restrict__ goff,
                      const double *__restrict__ boff, const int u, double *ws_all, double *acc_all, int32_t *__restrict__ meta, double *__restrict__ out) {
    lm_factors<NT, STATS, true>(nwave, wbeg, pbeg, items, rec, srcs, ptab, btab, atab, f2v, v2f, goff, boff, u, ws_all, acc_all, meta, out);
}

// row g of out = the rows gbeg[g] .. gbeg[g + 1] - 1 of acc, added in index order
__global__ __launch_bounds__(256) void k_lm_reduce(const int na, const int32_t *__restrict__ gbeg, const double *__restrict__ acc, double *__restrict__ out) {
    const int i = blockIdx.y * 256 + threadIdx.x, grp = blockIdx.x;
    if (i >= na) return;
    double s = 0.0;
    for (int p = gbeg[grp]; p < gbeg[grp + 1]; p++) s += acc[(int64_t)p * na + i];
    out[(int64_t)grp * na + i] = s;
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
};

static int32_t build(cx_handle *h, Cache &C, const std::string &who) {
    using namespace cxh;
    const int64_t nf = h->nf;
    mfr::Pairs P;
    mfr::pairs_of(h, P);
    std::vector<int32_t> rec((size_t)nf * 8, -1), srcs;
    C.kind.assign((size_t)nf, -1);
    C.set = P.set;
    C.unsupported_fac = P.unsupported_fac;
    for (int64_t f = 0; f < nf; f++) {
        if (h->fac_kind[f] == CX_FACTOR_OPAQUE) C.kind[f] = -2;
        if (P.so[f] < 0) continue;
        const bool oo = (h->vinfo[P.vo[f]] & kClamped) != 0, oi = (h->vinfo[P.vi[f]] & kClamped) != 0;
        const mfr::Run a = oo ? mfr::Run{} : mfr::other_slots(h, P.vo[f], P.so[f], srcs), b = oi ? mfr::Run{} : mfr::other_slots(h, P.vi[f], P.si[f], srcs);
        const int32_t r[8] = {(oo ? 1 : 0) | (oi ? 2 : 0), P.set[f], a.off, a.n, b.off, b.n, P.so[f], P.si[f]};
        std::copy(r, r + 8, &rec[(size_t)f * 8]);
        C.kind[f] = r[0];
    }
    CX_REQUIRE(h, nf < (int64_t)0x0fffffff && (int64_t)srcs.size() < (int64_t)0x7fffffff, CX_ERR_UNSUPPORTED, who + ": more than 2^28 factors");
    int32_t rc;
    if ((rc = dev_upload(h, &C.d_rec, rec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &C.d_srcs, srcs)) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the local host vectors die here)
    C.built = true;
    C.vinfo_epoch = h->vinfo_epoch;
    C.group_key.valid = false;
    return CX_OK;
}

// [set][A | A'] at the internal dim (blockdiag(A, I) for an embedded one: cx_set_factor_matrices)
static void fill_atab(const cx_handle *h, std::vector<double> &at) {
    const size_t d = (size_t)h->cfg.dim, dd = d * d, ns = std::max<size_t>(h->psets.size(), 1);
    at.assign(ns * 2 * dd, cxh::kNaN);
    for (size_t s = 0; s < h->psets.size(); s++) {
        if (h->psets[s].empty()) continue;
        const double *A = h->psets[s].data();
        for (size_t r = 0; r < d; r++)
            for (size_t c = 0; c < d; c++) { at[s * 2 * dd + r * d + c] = A[r * d + c]; at[s * 2 * dd + dd + c * d + r] = A[r * d + c]; }
    }
}

// the refusals of a reader (cx_mfma_reader.h), the cache and its factor records
static int32_t prepare(cx_handle *h, const std::string &who, const char *small_dims, const char *bad_args, Cache *&out) {
    using namespace cxh;
    int32_t rc;
    if ((rc = mfr::prepare(h, who, bad_args, {small_dims, "the variational and Beta-Bernoulli families have no Gaussian factor beliefs", "factors", true})) != CX_OK) return rc;
    if (h->learn_mfma && h->learn_mfma->vinfo_epoch != h->vinfo_epoch) h->learn_mfma.reset();      // other variables are observed
    if (!h->learn_mfma) h->learn_mfma.reset(new Cache());
    Cache &C = *h->learn_mfma;
    if (!C.built && (rc = build(h, C, who)) != CX_OK) { h->learn_mfma.reset(); return rc; }
    if ((rc = C.atab.refresh(h, [&](std::vector<double> &t) { fill_atab(h, t); })) != CX_OK) return rc;
    if ((rc = mv_ensure_chain_msgs(h)) != CX_OK) return rc;      // (every reader of d_mv_f2v calls this first)
    out = &C;
    return CX_OK;
}

static std::string no_pair(int64_t id) { return "factor " + std::to_string(id) + " is no two-variable CX_FACTOR_GAUSS_LINEAR factor"; }

// the group of every factor index (-1: not counted), checked by cx_factor_statistics' rules
static int32_t assign_groups(cx_handle *h, const Cache &C, const std::string &who, int64_t n, const int64_t *ids, const int64_t *groups, int64_t n_groups,
                             std::vector<int32_t> &grp) {
    using namespace cxh;
    const int64_t nf = h->nf;
    grp.assign((size_t)nf, -1);
    if (!ids) {
        if (C.unsupported_fac >= 0) return mfr::refuse_factor(h, who, C.unsupported_fac);
        for (int64_t f = 0; f < nf; f++) {
            if (C.kind[f] < 0) continue;
            if (C.set[f] >= n_groups)
                return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factor " + std::to_string(h->fac_ids[f]) + " uses parameter set " + std::to_string(C.set[f]) +
                            ": n_groups must exceed every set in use");
            grp[f] = C.set[f];
        }
        return CX_OK;
    }
    std::vector<int64_t> first((size_t)n_groups, -1);
    for (int64_t i = 0; i < n; i++) {
        const int64_t f = find_factor(h, ids[i]);
        if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(ids[i]));
        const int64_t g = groups[i];
        if (g < -1 || g >= n_groups) return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": group " + std::to_string(g) + " of factor " + std::to_string(ids[i]) + " is not in -1 .. n_groups - 1");
        if (g < 0) continue;
        if (C.kind[f] < 0) return fail(h, CX_ERR_UNSUPPORTED, who + ": " + no_pair(ids[i]));
        if (grp[f] >= 0) return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factor " + std::to_string(ids[i]) + " is listed twice");
        grp[f] = (int32_t)g;
        const int64_t q = first[(size_t)g];
        if (q < 0) { first[(size_t)g] = f; continue; }
        if (C.set[f] != C.set[q])
            return fail(h, CX_ERR_INVALID_ARGUMENT, who + ": factors " + std::to_string(h->fac_ids[q]) + " and " + std::to_string(ids[i]) + " are in group " +
                        std::to_string(g) + " but do not share their A (one parameter set per group)");
    }
    return CX_OK;
}

// items by group, then factor index; a group's run cut into partials of at most ceil(items / max_waves) factors; the partials dealt to
// at most max_waves waves in contiguous runs
static int32_t build_lists(cx_handle *h, Cache &C, const std::vector<int32_t> &grp, int64_t n_groups, int na) {
    using namespace cxh;
    std::vector<int64_t> cnt((size_t)n_groups + 1, 0);
    for (int32_t g : grp) if (g >= 0) cnt[(size_t)g + 1]++;
    C.group_n.assign(cnt.begin() + 1, cnt.end());
    for (int64_t g = 0; g < n_groups; g++) cnt[(size_t)g + 1] += cnt[(size_t)g];
    const int64_t n_items = cnt[(size_t)n_groups];
    std::vector<int32_t> items((size_t)n_items), pbeg, wbeg, gbeg;
    {
        std::vector<int64_t> at(cnt.begin(), cnt.end() - 1);
        for (size_t f = 0; f < grp.size(); f++) if (grp[f] >= 0) items[(size_t)at[(size_t)grp[f]]++] = (int32_t)f;
    }
    const int64_t mw = max_waves(h->cfg.dim), len = std::max<int64_t>(1, (n_items + mw - 1) / mw);
    C.part_group.clear();
    for (int64_t g = 0; g < n_groups; g++) {
        gbeg.push_back((int32_t)pbeg.size());
        for (int64_t a = cnt[(size_t)g]; a < cnt[(size_t)g + 1]; a += len) { pbeg.push_back((int32_t)a); C.part_group.push_back((int32_t)g); }
    }
    gbeg.push_back((int32_t)pbeg.size());
    const int64_t np = (int64_t)pbeg.size(), nw = std::min<int64_t>(np, mw);
    pbeg.push_back((int32_t)n_items);
    for (int64_t w = 0; w <= nw; w++) wbeg.push_back((int32_t)(nw ? w * np / nw : 0));
    int32_t rc;
    if ((rc = dev_upload(h, &C.d_items, items)) != CX_OK || (rc = dev_upload(h, &C.d_pbeg, pbeg)) != CX_OK || (rc = dev_upload(h, &C.d_wbeg, wbeg)) != CX_OK ||
        (rc = dev_upload(h, &C.d_gbeg, gbeg)) != CX_OK)
        return rc;
    if ((rc = C.d_meta.ensure(h, 2 * np)) != CX_OK || (rc = C.d_acc.ensure(h, np * na)) != CX_OK || (rc = C.d_rows.ensure(h, n_groups * na)) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
    C.h_meta.assign((size_t)(2 * np), 0);
    C.h_rows.assign((size_t)(n_groups * na), 0.0);
    C.n_items = n_items; C.n_part = np; C.n_wave = nw;
    return CX_OK;
}

template <bool STATS>
static void launch(cx_handle *h, Cache &C, int nwave, const int32_t *wbeg, const int32_t *pbeg, const int32_t *items, double *out) {
    const int u = mfr::user_dim(h);
    mfr::for_tiles(h->cfg.dim, [&](auto nt) {
        constexpr int NT = decltype(nt)::value, W = NT == 4 ? 1 : 2;      // (4 x 4 tiles at two waves per SIMD: 7 to 11 registers spilled, so one)
        if (h->has_offsets)      // cx_set_factor_offsets_mfma: the instances that read g and b
            hipLaunchKernelGGL((k_lm_factors_off<NT, STATS, W>), dim3((unsigned)nwave), dim3(64), 0, h->stream, nwave, wbeg, pbeg, items, C.d_rec, C.d_srcs, h->d_ptab,
                               h->d_ptab_bt, C.atab.d, h->d_mv_f2v, h->d_mv_v2f, (const double *)h->d_off_g, (const double *)h->d_off_b, u, C.d_ws, C.d_acc, C.d_meta, out);
        else
        hipLaunchKernelGGL((k_lm_factors<NT, STATS, W>), dim3((unsigned)nwave), dim3(64), 0, h->stream, nwave, wbeg, pbeg, items, C.d_rec, C.d_srcs, h->d_ptab,
                           h->d_ptab_bt, C.atab.d, h->d_mv_f2v, h->d_mv_v2f, u, C.d_ws, C.d_acc, C.d_meta, out);
    });
}

}  // namespace lm

template <> void Deleter<lm::Cache>::operator()(lm::Cache *C) const { delete C; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_factor_beliefs_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, double *out) {
    try {
        namespace lm = cx::lm;
        const std::string who = "cx_factor_beliefs_mfma";
        lm::Cache *Cp = nullptr;
        int32_t rc;
        const char *bad = n >= 0 && (n == 0 || (factor_ids && out)) ? nullptr : "null argument or negative count";
        if ((rc = lm::prepare(h, who, "cx_factor_beliefs", bad, Cp)) != CX_OK) return rc;
        if (n == 0) return CX_OK;
        lm::Cache &C = *Cp;
        std::vector<int32_t> items((size_t)n);
        for (int64_t i = 0; i < n; i++) {
            const int64_t f = find_factor(h, factor_ids[i]);
            if (f < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no factor " + std::to_string(factor_ids[i]));
            if (C.kind[(size_t)f] < 0) return fail(h, CX_ERR_UNSUPPORTED, who + ": " + lm::no_pair(factor_ids[i]));
            items[(size_t)i] = (int32_t)f;
        }
        const int d = h->cfg.dim, u = cx::mfr::user_dim(h);
        const int64_t nb = 2 * u + 4 * (int64_t)u * u, chunk = std::min<int64_t>(n, lm::max_waves(d));
        if ((rc = C.d_bitems.ensure(h, chunk)) != CX_OK || (rc = C.d_bout.ensure(h, chunk * nb)) != CX_OK || (rc = C.d_ws.ensure(h, chunk * lm::ws_doubles(d))) != CX_OK) return rc;
        for (int64_t at = 0; at < n; at += chunk) {
            const int64_t m = std::min(chunk, n - at);
            CX_HIP(h, hipMemcpyAsync(C.d_bitems, items.data() + at, (size_t)m * 4, hipMemcpyHostToDevice, h->stream));
            lm::launch<false>(h, C, (int)m, nullptr, nullptr, C.d_bitems, C.d_bout);
            CX_HIP(h, hipGetLastError());
            CX_HIP(h, hipMemcpyAsync(out + at * nb, C.d_bout, (size_t)(m * nb) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            CX_HIP(h, hipStreamSynchronize(h->stream));
        }
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_factor_beliefs_mfma: host allocation failed"); }
}

extern "C" int32_t cx_factor_statistics_mfma(cx_handle *h, int64_t n, const int64_t *factor_ids, const int64_t *groups, int64_t n_groups, double *out,
                                             int64_t *counts4) {
    try {
        namespace lm = cx::lm;
        const std::string who = "cx_factor_statistics_mfma";
        lm::Cache *Cp = nullptr;
        int32_t rc;
        const char *bad = !(out && counts4 && n_groups > 0) ? "null output or n_groups < 1"
                          : !(factor_ids ? (n >= 0 && (n == 0 || groups)) : !groups)
                              ? "factor_ids and groups go together (n >= 0), or both null for the parameter-set grouping"
                              : nullptr;
        if ((rc = lm::prepare(h, who, "cx_factor_statistics", bad, Cp)) != CX_OK) return rc;
        lm::Cache &C = *Cp;
        const int d = h->cfg.dim, u = cx::mfr::user_dim(h), na = 2 * u + 3 * u * u, ns = 1 + na;
        if (!C.group_key.matches(n_groups, n, factor_ids, groups)) {
            C.group_key.valid = false;
            std::vector<int32_t> grp;
            if ((rc = lm::assign_groups(h, C, who, n, factor_ids, groups, n_groups, grp)) != CX_OK) return rc;
            if ((rc = lm::build_lists(h, C, grp, n_groups, na)) != CX_OK) return rc;
            C.group_key.remember(n_groups, n, factor_ids, groups);
        }
        std::fill(out, out + n_groups * ns, 0.0);
        for (int k = 0; k < 4; k++) counts4[k] = 0;
        if (C.n_part == 0) return CX_OK;
        if ((rc = C.d_ws.ensure(h, C.n_wave * lm::ws_doubles(d))) != CX_OK) return rc;
        lm::launch<true>(h, C, (int)C.n_wave, C.d_wbeg, C.d_pbeg, C.d_items, nullptr);
        hipLaunchKernelGGL(lm::k_lm_reduce, dim3((unsigned)n_groups, (unsigned)((na + 255) / 256)), dim3(256), 0, h->stream, na, C.d_gbeg, C.d_acc, C.d_rows);
        CX_HIP(h, hipGetLastError());
        CX_HIP(h, hipMemcpyAsync(C.h_rows.data(), C.d_rows, (size_t)(n_groups * na) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipMemcpyAsync(C.h_meta.data(), C.d_meta, (size_t)(2 * C.n_part) * sizeof(int32_t), hipMemcpyDeviceToHost, h->stream));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        std::vector<int64_t> g_bad((size_t)n_groups, 0);
        for (int64_t p = 0; p < C.n_part; p++) {
            counts4[2] += C.h_meta[(size_t)(2 * p)];
            counts4[3] += C.h_meta[(size_t)(2 * p + 1)];
            g_bad[(size_t)C.part_group[(size_t)p]] += C.h_meta[(size_t)(2 * p)] + C.h_meta[(size_t)(2 * p + 1)];
        }
        for (int64_t g = 0; g < n_groups; g++) {
            if (C.group_n[(size_t)g] == 0) continue;
            counts4[0] += C.group_n[(size_t)g];
            counts4[1] += 1;
            double *o = out + g * ns;
            o[0] = (double)C.group_n[(size_t)g];
            for (int k = 0; k < na; k++) o[1 + k] = g_bad[(size_t)g] > 0 ? kNaN : C.h_rows[(size_t)(g * na + k)];
        }
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, "cx_factor_statistics_mfma: host allocation failed"); }
}
