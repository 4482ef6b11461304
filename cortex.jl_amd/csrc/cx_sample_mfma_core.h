// cx_sample_mfma_core.h — what cx_sample_posterior_mfma (cx_sample_mfma.hip) and cx_linear_moments_mfma
// (cx_functional_mfma.hip, §4s) share at the matrix-core dims (cx_create dim 5 .. 64, internal tiles of 16 / 32 / 64): the links of a
// Gaussian forest from the stored factor→variable messages and the data, the panels and their accessors, the forward blocked scan and
// the plan.  One plan per handle (cx_handle::sample_mfma), whichever entry builds it first.
//
//   q(x) = b_r(x_r) Π_a b_a(x_C | x_p)     per component, rooted where cx::treeplan::root_forest roots it
//
// Only two-variable rule factors and opaque messages exist at these dims.  For a link factor with child end C and parent end p, (P, B')
// is the rule table TOWARDS p, M = P + Σ (the child's other stored messages) = U'U, η_C the sum of their η:
//   x_C = M⁻¹(B' x_p + η_C) + U⁻¹ ε_C = G x_p + off + U⁻¹ ε_C,     the root: Λ_r = Σ all its stored messages = U'U, G = 0
// UNCENTRED (nothing centred exists at these dims; §4r says what that costs).  A link is stored as the scan reads it, in the tile layout
// of tts (T'S, a contraction over tile ROWS): G' = (U^-T B')' U^-T | U^-T | off, 2 KD² + KD doubles per position.
//
//   plan (host, cached)  the forest plan of cx_sample_core.h (sp::build_forest), the link records from mfr::checked_pairs, the
//                        components with no information at all (no observed neighbour, no opaque message), decided on the host
//   k_spm_cond           one wave per root and per link: table + sum of records, factor_solve, U^-T through the identity, then one
//                        block column of U^-T B' at a time against it (Y and U^-T are never both whole in registers)
//   k_sp_flag(_comp)     cx_sample_core.h's status pass, as it is
//   per light depth      the blocked scan of cx_sample_core.h over PANELS of 16 samples: a panel is NT tile registers, lane (g, c)
//                        register r = component g + 4 r of sample c; one step is NT² (+ triangular) tile products
//     k_spm_compose      level l: one wave per (tile item, panel) composes the offsets from zero, and one wave per (tile item, block
//                        column) the product of the tile's G: the same step on the block columns of the identity, no offset, no noise
//     k_spm_walk<TOP>    one wave per (path, panel) from the head's parent;  k_spm_walk: level l .. 1 from each item's carry
//   z                    laid out [position][sample][KD]: the sampler's gather reads runs of u doubles, the adjoint's u lies the same
// The standard normals: Philox4x32-10 with the counter and key of cx_sample_posterior, in registers; the padding components of an
// embedded dim and the unused columns of a last panel get exact zeros.  No atomics: two calls on one state are bit-identical.
#pragma once
#include <cstdlib>

#include "cx_evidence_mfma_core.h"
#include "cx_mfma_reader.h"
#include "cx_sample_core.h"

namespace cx {
namespace spm {

using namespace w64;
using evm::add_sources, evm::any_nan_record, evm::factor_solve, evm::load_upper, evm::pad_identity, evm::solve_col, evm::solve_identity_cols;

constexpr int kPanel = 16;      // samples per panel: the columns of a tile

template <int NT>
struct LR {
    static constexpr int KD = 16 * NT, GT = 0, UT = KD * KD, OFF = 2 * KD * KD, N = 2 * KD * KD + KD;      // a link: G' | U^-T | off
};

// ---- the links ------------------------------------------------------------------------------------------------------------------------
// item record (8 int32): {position, rule-table index towards the parent (-1: a root), sources offset, sources count, 0, 0, 0, 0};
// sources: the message slots summed into M (a root: all of its slots; a link: the child's slots but the link factor's), in ascending
// neighbour order.  st[q] = 0 ok, 1 an input record is NaN, 2 a pivot below u is not positive and finite.  A failed link is zeros.
template <int NT, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_spm_cond(int n, const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab, const double *__restrict__ btab,
                const double *__restrict__ f2v, const int u, double *__restrict__ link, uint8_t *__restrict__ st) {
    constexpr int KD = 16 * NT, NU = NT * (NT + 1) / 2;
    __shared__ double S[16 * kLdT];
    __shared__ double Vs[NT][16 * kLdT];
    __shared__ double ZS[KD];
    const int w = blockIdx.x;
    if (w >= n) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mo = g * KD + c;
    const int32_t *t = rec + 8 * (int64_t)w;
    const int q = t[0], tabi = t[1], s_off = t[2], s_n = t[3];
    const bool root = tabi < 0;
    gdp l = (gdp)(link + (int64_t)q * LR<NT>::N);

    d4 M[NU];
    double wcv[NT], zrv[NT][4];
#pragma unroll
    for (int i = 0; i < NU; i++) M[i] = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int j = 0; j < NT; j++) wcv[j] = 0.0;
    if (!root) {
        const gcdp P = (gcdp)(ptab + (int64_t)tabi * 3 * KD * KD);
        load_upper<NT>(M, [&](int k) { return P[mo + k]; });
    }
    add_sources<NT>(M, wcv, f2v, srcs + s_off, s_n, mo, c);
    if (root) pad_identity<NT>(M, g, c, u);      // (a sum of messages may be zero on the padding of an embedded dim; P is the identity there)
    const bool undef = any_nan_record<NT>(false, f2v, srcs + s_off, s_n);
    double ld, qd;
    bool pd;
    factor_solve<NT>(M, wcv, zrv, S, Vs, g, c, u, ld, qd, pd);
    const int status = undef ? 1 : pd ? 0 : 2;
    if (lane == 0) st[q] = (uint8_t)status;
    if (status) {
        for (int k = lane; k < LR<NT>::N; k += 64) l[k] = 0.0;
        return;
    }
    evm::park_z<NT>(ZS, zrv, g);
    // W = U^-T: the lower block triangle, W[b][j] = tile (j, b), j >= b.  Stored whole: the upper block triangle is zeros
    d4 W[NT][NT];
    solve_identity_cols<NT>(W, M, Vs, g, c);
#pragma unroll
    for (int b = 0; b < NT; b++)
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) l[LR<NT>::UT + mo + tile_const_n<NT>(j, b, r)] = j >= b ? W[b][j][r] : 0.0;
    // off = U⁻¹ (U^-T η) = W'z: entry 16 a + c
#pragma unroll
    for (int a = 0; a < NT; a++) {
        double p = 0.0;
#pragma unroll
        for (int j = a; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) p += W[a][j][r] * ZS[16 * j + g + 4 * r];
        p = sum_groups(p);
        if (g == 0) l[LR<NT>::OFF + 16 * a + c] = p;
    }
    // G' = Y'W, Y = U^-T B': one block column p of B' at a time (tile row p of G'), tile (p, q) = Σ_{j >= q} Y(j, p)' W(j, q)
    if (root) {
        for (int k = lane; k < KD * KD; k += 64) l[LR<NT>::GT + k] = 0.0;
        return;
    }
    const gcdp bt = (gcdp)(btab + (int64_t)tabi * KD * KD);
#pragma unroll
    for (int p = 0; p < NT; p++) {
        asm volatile("" ::: "memory");      // (one block column of B' in flight at a time)
        d4 Y[NT];
#pragma unroll
        for (int j = 0; j < NT; j++)
#pragma unroll
            for (int r = 0; r < 4; r++) Y[j][r] = bt[mo + tile_const_n<NT>(j, p, r)];
        solve_col<NT>(Y, M, Vs, 0, g, c);
#pragma unroll
        for (int qq = 0; qq < NT; qq++) {
            d4 A = d4{0.0, 0.0, 0.0, 0.0};
#pragma unroll
            for (int j = qq; j < NT; j++) A = tts(Y[j], W[qq][j], A);
#pragma unroll
            for (int r = 0; r < 4; r++) l[LR<NT>::GT + mo + tile_const_n<NT>(p, qq, r)] = A[r];
        }
    }
}

// ---- the noise of a panel ---------------------------------------------------------------------------------------------------------------
struct Gen {
    const double *noise;       // caller's ε of this chunk of samples, [samples of the chunk][nv][u]; null: Philox
    int64_t nv;
    uint64_t seed;
    int64_t s0;                // global index of the chunk's first sample
    int64_t n_valid;           // samples of the chunk that exist (the columns behind them get zero noise and are never stored)
    int u;                     // the user's dim: components u .. KD - 1 get zero noise
};

// E[b], lane (g, c) register r = ε[16 b + g + 4 r] of variable v in sample (panel * 16 + c) of the chunk.  Philox yields components
// (2 j, 2 j + 1) from one counter: the lanes g and g ^ 1 need both halves of the pairs at (16 b + 4 r + (g & ~1)) / 2, so the even
// lane group makes the pairs of r = 0, 1 and the odd one those of r = 2, 3, and they exchange: every normal is made once
template <int NT>
__device__ __forceinline__ void panel_noise(const Gen &gen, const int panel, const int32_t v, d4 (&E)[NT], const int g, const int c) {
    const int64_t sl = (int64_t)panel * kPanel + c;
    const bool live = sl < gen.n_valid;
    if (gen.noise) {
        const double *p = gen.noise + (sl * gen.nv + v) * gen.u;
#pragma unroll
        for (int b = 0; b < NT; b++)
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const int k = 16 * b + g + 4 * r;
                E[b][r] = (live && k < gen.u) ? p[k] : 0.0;
            }
        return;
    }
    const int odd = g & 1, g0 = g & ~1;
#pragma unroll
    for (int b = 0; b < NT; b++) {
        double mine[2], theirs[2];
#pragma unroll
        for (int i = 0; i < 2; i++) {
            const int r = 2 * odd + i, k = 16 * b + 4 * r + g0;      // the pair (k, k + 1), k even
            double n0 = 0.0, n1 = 0.0;
            if (k < gen.u) sp::normal_pair(gen.seed, (uint64_t)(gen.s0 + sl), (uint32_t)v, (uint32_t)(k >> 1), n0, n1);
            mine[i] = odd ? n1 : n0;
            theirs[i] = odd ? n0 : n1;
        }
        const double got0 = __shfl_xor(theirs[0], 16, 64), got1 = __shfl_xor(theirs[1], 16, 64);
        // the even lane made r = 0, 1 and got r = 2, 3; the odd lane the other way round
        const double e[4] = {odd ? got0 : mine[0], odd ? got1 : mine[1], odd ? mine[0] : got0, odd ? mine[1] : got1};
#pragma unroll
        for (int r = 0; r < 4; r++) E[b][r] = (live && 16 * b + g + 4 * r < gen.u) ? e[r] : 0.0;
    }
}

// ---- one step of one panel (or of one block column of a running product) ----------------------------------------------------------------
// Z <- G Z (+ add): GT = G' row-major, Z_new[a] = add[a] + Σ_b tts(G'[b][a], Z[b])
template <int NT>
__device__ __forceinline__ void apply_g(const gcdp GT, d4 (&Z)[NT], d4 (&N)[NT], const int mo) {
#pragma unroll
    for (int a = 0; a < NT; a++) {
#pragma unroll
        for (int b = 0; b < NT; b++) {
            d4 T;
#pragma unroll
            for (int r = 0; r < 4; r++) T[r] = GT[mo + tile_const_n<NT>(b, a, r)];
            N[a] = tts(T, Z[b], N[a]);
        }
    }
#pragma unroll
    for (int a = 0; a < NT; a++) Z[a] = N[a];
}
// the step of a position: Z <- G Z + off + U⁻¹ E; NOISE false: Z <- G Z (the running product)
template <int NT, bool NOISE>
__device__ __forceinline__ void link_step(const double *__restrict__ link, const int64_t q, const int32_t *__restrict__ pos_var, const Gen &gen, const int panel,
                                          d4 (&Z)[NT], const int g, const int c, const int mo) {
    const gcdp l = (gcdp)(link + q * LR<NT>::N);
    d4 N[NT];
    if constexpr (NOISE) {
        d4 E[NT];
        panel_noise<NT>(gen, panel, pos_var[q], E, g, c);
#pragma unroll
        for (int a = 0; a < NT; a++) {
#pragma unroll
            for (int r = 0; r < 4; r++) N[a][r] = l[LR<NT>::OFF + 16 * a + g + 4 * r];
#pragma unroll
            for (int b = a; b < NT; b++) {      // (U^-T is lower block triangular: tiles (b, a), b >= a)
                d4 T;
#pragma unroll
                for (int r = 0; r < 4; r++) T[r] = l[LR<NT>::UT + mo + tile_const_n<NT>(b, a, r)];
                N[a] = tts(T, E[b], N[a]);
            }
        }
    } else {
#pragma unroll
        for (int a = 0; a < NT; a++) N[a] = d4{0.0, 0.0, 0.0, 0.0};
    }
    apply_g<NT>(l + LR<NT>::GT, Z, N, mo);
}
// the step of an item of a level above the positions: Z <- Gc Z + oc
template <int NT, bool OFFSET>
__device__ __forceinline__ void item_step(const double *__restrict__ Gb, const double *__restrict__ ob, const int64_t i, const int np, const int panel, d4 (&Z)[NT],
                                          const int lane, const int mo) {
    constexpr int KD = 16 * NT;
    d4 N[NT];
#pragma unroll
    for (int a = 0; a < NT; a++) {
        if constexpr (OFFSET) {
            const gcdp o = (gcdp)(ob + ((i * np + panel) * NT + a) * 256);
#pragma unroll
            for (int r = 0; r < 4; r++) N[a][r] = o[4 * lane + r];
        } else N[a] = d4{0.0, 0.0, 0.0, 0.0};
    }
    apply_g<NT>((gcdp)(Gb + i * KD * KD), Z, N, mo);
}
// a panel in a level buffer ([item][panel][tile][lane][4]: 32 contiguous bytes per lane)
template <int NT>
__device__ __forceinline__ void put_panel(double *__restrict__ buf, const int64_t slot, const d4 (&Z)[NT], const int lane) {
    gdp o = (gdp)(buf + slot * NT * 256);
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[a * 256 + 4 * lane + r] = Z[a][r];
}
template <int NT>
__device__ __forceinline__ void get_panel(const double *__restrict__ buf, const int64_t slot, d4 (&Z)[NT], const int lane) {
    const gcdp o = (gcdp)(buf + slot * NT * 256);
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) Z[a][r] = o[a * 256 + 4 * lane + r];
}
// z of a position: [position][sample of the chunk][KD], so that the gather reads runs of u doubles
template <int NT>
__device__ __forceinline__ void put_z(double *__restrict__ Zb, const int64_t q, const int64_t S, const int panel, const d4 (&Z)[NT], const int g, const int c) {
    constexpr int KD = 16 * NT;
    gdp o = (gdp)(Zb + (q * S + (int64_t)panel * kPanel + c) * KD);
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) o[16 * a + g + 4 * r] = Z[a][r];
}
template <int NT>
__device__ __forceinline__ void get_z(const double *__restrict__ Zb, const int64_t q, const int64_t S, const int panel, d4 (&Z)[NT], const int g, const int c) {
    constexpr int KD = 16 * NT;
    const gcdp o = (gcdp)(Zb + (q * S + (int64_t)panel * kPanel + c) * KD);
#pragma unroll
    for (int a = 0; a < NT; a++)
#pragma unroll
        for (int r = 0; r < 4; r++) Z[a][r] = o[16 * a + g + 4 * r];
}

// ---- the blocked scan (cx_sample_core.h: k_sp_compose, k_sp_walk; the levels, ranges, tops and carries are the same) -------------------
// level buffers: Gc [item][KD²] holds the item's composed G TRANSPOSED (what apply_g reads), oc and carry [item][panel] panels.
// Wave x of item j: x < np the panel x, otherwise block column x - np of the product of the items' G
template <int NT, bool POS>
__global__ __launch_bounds__(64) void k_spm_compose(int64_t n, int np, const int2 *__restrict__ rng, const double *__restrict__ link,
                                                    const int32_t *__restrict__ pos_var, Gen gen, const double *__restrict__ Gb, const double *__restrict__ ob,
                                                    double *__restrict__ Gc, double *__restrict__ oc) {
    constexpr int KD = 16 * NT;
    const int64_t j = blockIdx.x / (np + NT);
    const int x = (int)(blockIdx.x - j * (np + NT));
    if (j >= n) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mo = g * KD + c;
    const int2 r = rng[j];
    d4 Z[NT];
    if (x >= np) {
        const int k = x - np;      // block column k of the identity
#pragma unroll
        for (int a = 0; a < NT; a++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) Z[a][rr] = (a == k && g + 4 * rr == c) ? 1.0 : 0.0;
        for (int32_t i = r.x; i < r.y; i++) {
            if constexpr (POS) link_step<NT, false>(link, i, pos_var, gen, 0, Z, g, c, mo);
            else item_step<NT, false>(Gb, ob, i, np, 0, Z, lane, mo);
        }
        // Z[a] = tile (a, k) of the product; Gc holds its transpose: element (16 k + c, 16 a + g + 4 r)
        gdp o = (gdp)(Gc + j * KD * KD);
#pragma unroll
        for (int a = 0; a < NT; a++)
#pragma unroll
            for (int rr = 0; rr < 4; rr++) o[(16 * k + c) * KD + 16 * a + g + 4 * rr] = Z[a][rr];
        return;
    }
#pragma unroll
    for (int a = 0; a < NT; a++) Z[a] = d4{0.0, 0.0, 0.0, 0.0};
    for (int32_t i = r.x; i < r.y; i++) {
        if constexpr (POS) link_step<NT, true>(link, i, pos_var, gen, x, Z, g, c, mo);
        else item_step<NT, true>(Gb, ob, i, np, x, Z, lane, mo);
    }
    put_panel<NT>(oc, j * np + x, Z, lane);
}

// TOP: item j is a path, top[j] = (range of its top-level items, the position of its head's parent (-1: a root), -), the carry in is the
// parent's z; otherwise the carry of item j of this level.  POS: the children are positions (z written to Zb), else items of the level
// below (their carries written to cb)
template <int NT, bool POS, bool TOP>
__global__ __launch_bounds__(64) void k_spm_walk(int64_t n, int np, int64_t S, const int4 *__restrict__ top, const int2 *__restrict__ rng,
                                                 const double *__restrict__ carry, const double *__restrict__ link, const int32_t *__restrict__ pos_var, Gen gen,
                                                 const double *__restrict__ Gb, const double *__restrict__ ob, double *__restrict__ cb, double *__restrict__ Zb) {
    constexpr int KD = 16 * NT;
    const int64_t j = blockIdx.x / np;
    const int x = (int)(blockIdx.x - j * np);
    if (j >= n) return;
    const int lane = threadIdx.x, g = lane >> 4, c = lane & 15, mo = g * KD + c;
    d4 Z[NT];
    int32_t b, e;
    if constexpr (TOP) {
        const int4 p = top[j];
        b = p.x; e = p.y;
        if (p.z >= 0) get_z<NT>(Zb, p.z, S, x, Z, g, c);
        else {
#pragma unroll
            for (int a = 0; a < NT; a++) Z[a] = d4{0.0, 0.0, 0.0, 0.0};
        }
    } else {
        const int2 r = rng[j];
        b = r.x; e = r.y;
        get_panel<NT>(carry, j * np + x, Z, lane);
    }
    for (int32_t i = b; i < e; i++) {
        if constexpr (POS) {
            link_step<NT, true>(link, i, pos_var, gen, x, Z, g, c, mo);
            put_z<NT>(Zb, i, S, x, Z, g, c);
        } else {
            put_panel<NT>(cb, (int64_t)i * np + x, Z, lane);
            item_step<NT, true>(Gb, ob, i, np, x, Z, lane, mo);
        }
    }
}

// ---- host -------------------------------------------------------------------------------------------------------------------------------
// The plan follows the graph and WHICH variables are observed (vinfo_epoch); rule tables, messages and data are read by every call
struct Plan : sp::ForestDev, sp::ForestDims {
    bool valid = false;
    int64_t nv = -1, ne = -1;
    uint64_t vinfo_epoch = 0;
    int64_t n_item = 0;                        // roots and links: one record each
    std::vector<uint8_t> h_cflag, h_cimp;      // per component: the status pass; no information at all (decided here, on the host)
    DevBuf<int32_t> d_rec, d_srcs, d_vid;
    DevBuf<uint8_t> d_cimp;
    // the scan run leaf-to-root (cx_functional_mfma.hip): per position the heads of the light paths that hang on it, in path order
    DevBuf<int32_t> d_att_off, d_att_head;
    // the link workspace: 2 KD² + KD doubles per position; it outlives a rebuild of the plan when its size allows
    DevBuf<double> d_link;
    // per call, grown on demand: z, the level buffers, the caller's noise, the output
    DevBuf<double> d_Z, d_noise, d_out;
    std::vector<DevBuf<double>> d_Gc, d_oc, d_carry;      // per level
    // cx_linear_moments_mfma, per call: the functionals (offsets, entries, weights), the noise coordinates g of every functional, the
    // status and mean of every functional, the block partials of the covariance, the covariance
    DevBuf<int64_t> d_foff;
    DevBuf<int32_t> d_fvar, d_ffun;
    DevBuf<double> d_fw, d_fg, d_fcov, d_fcpart;
    DevBuf<ev::Part> d_fpart;
};

// CX_SAMPLE_MFMA_TILE (2 .. 64, default 64), read when a plan is built: the items per tile of the blocked scan.  A small tile gives a
// short chain the tile levels that only a long one has otherwise: the tests' way to every level kernel, and the knob of an A/B
inline int tile_items() {
    const char *e = std::getenv("CX_SAMPLE_MFMA_TILE");
    const long v = e && *e ? std::strtol(e, nullptr, 10) : sp::kTile;
    return (int)std::min<long>(std::max<long>(v, 2), sp::kTile);
}
// name (CX_SAMPLE_MFMA_CHUNK, CX_FN_MFMA_CHUNK: a multiple of 16; 0 or unset: as many as the scratch bound allows), read by every call:
// samples or functionals per chunk.  The tests' way across a chunk boundary with few of them
inline int64_t chunk_override(const char *name) {
    const char *e = std::getenv(name);
    const long v = e && *e ? std::strtol(e, nullptr, 10) : 0;
    return v > 0 ? (int64_t)((v + kPanel - 1) / kPanel) * kPanel : 0;
}

inline int32_t build_plan(cx_handle *h, Plan &P, const std::string &who) {
    using namespace cxh;
    P.valid = false;
    mfr::Pairs pairs;
    int32_t rc;
    if ((rc = mfr::checked_pairs(h, who, pairs)) != CX_OK) return rc;
    sp::Forest F;
    if ((rc = sp::build_forest(h, P, F, who, tile_items())) != CX_OK) return rc;
    CX_REQUIRE(h, P.npos < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 free variables");
    // the records: the roots, then the links in the forest's order (parents before children).  The table towards the parent: the
    // child's sending slot's, spdir = 2 set + (1: the message goes forward, from the IN end's slot) — as cx_causal_mfma.hip names it
    std::vector<int32_t> rec, srcs;
    auto item = [&](int32_t q, int32_t tab, mfr::Run r) {
        const int32_t t[8] = {q, tab, r.off, r.n, 0, 0, 0, 0};
        rec.insert(rec.end(), t, t + 8);
    };
    for (int32_t v : F.order) {
        const int32_t f = F.vfac[v];
        if (f < 0) { item(F.var_pos[v], -1, mfr::other_slots(h, v, -1, srcs)); continue; }
        if (pairs.so[f] < 0) return fail(h, CX_ERR_STATE, who + ": factor " + std::to_string(h->fac_ids[f]) + " joins two free variables but is no rule factor");
        // cs: the child's slot on the link factor, the OUT end's or the IN end's; the rule towards the parent sends through it
        const int32_t cs = pairs.vo[f] == v ? pairs.so[f] : pairs.si[f];
        item(F.var_pos[v], h->spdir[(size_t)cs], mfr::other_slots(h, v, cs, srcs));
    }
    CX_REQUIRE(h, (int64_t)srcs.size() < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 inputs");
    P.n_item = (int64_t)rec.size() / 8;
    if (srcs.empty()) srcs.push_back(0);
    if (rec.empty()) rec.assign(8, 0);
    // a component with no information at all: no observed neighbour and no opaque message anywhere in it
    P.h_cimp.assign((size_t)P.n_comp, 2);
    for (int32_t v : F.order)
        for (int32_t e = h->var_off[v]; e < h->var_off[v + 1]; e++) {
            const int32_t f = pairs.efac[(size_t)e];
            const bool info = h->fac_kind[f] == CX_FACTOR_OPAQUE ||
                              (pairs.so[f] >= 0 && (h->vinfo[(size_t)(pairs.vo[f] == v ? pairs.vi[f] : pairs.vo[f])] & kClamped));
            if (info) P.h_cimp[(size_t)F.vcomp[v]] = 0;
        }
    // a datum's slot; -1: an observed variable on no connection
    for (int64_t v = 0; v < h->nv; v++) if (h->var_off[v + 1] == h->var_off[v]) F.dslot[(size_t)v] = -1;
    // the forest read from the other end: a position's light paths, in path order (from top, rngs and the depths alone)
    std::vector<int32_t> att_off((size_t)P.npos + 1, 0), att_head;
    for (const int4 &t : F.top) if (t.z >= 0) att_off[(size_t)t.z + 1]++;
    for (int64_t q = 0; q < P.npos; q++) att_off[q + 1] += att_off[q];
    att_head.assign((size_t)att_off[P.npos] + 1, 0);
    {
        std::vector<int32_t> at(att_off.begin(), att_off.end() - 1);
        for (const sp::Depth &dp : P.depths)
            for (int64_t k = 0; k < dp.n_paths; k++) {
                const int4 &t = F.top[(size_t)(dp.top_off + k)];
                if (t.z < 0) continue;
                // the path's first position: of its first tile at every level, down to the positions
                int32_t b = t.x;
                for (int l = dp.levels; l >= 1; l--) b = F.rngs[(size_t)(dp.rng_off[(size_t)l - 1] + b)].x;
                att_head[(size_t)at[t.z]++] = b;
            }
    }
    static_cast<sp::ForestDev &>(P) = sp::ForestDev();
    if ((rc = sp::upload_forest(h, P, P, F)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_att_off, att_off)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_att_head, att_head)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_rec, rec)) != CX_OK) return rc;
    if ((rc = dev_upload(h, &P.d_srcs, srcs)) != CX_OK) return rc;
    { std::vector<uint8_t> ci = P.h_cimp; if (ci.empty()) ci.push_back(0); if ((rc = dev_upload(h, &P.d_cimp, ci)) != CX_OK) return rc; CX_HIP(h, hipStreamSynchronize(h->stream)); }
    const int64_t kd = h->cfg.dim;
    if ((rc = P.d_link.ensure(h, std::max<int64_t>(P.npos, 1) * (2 * kd * kd + kd))) != CX_OK) return rc;
    const size_t levels = P.level_cap.size();
    P.d_Gc.clear(); P.d_oc.clear(); P.d_carry.clear();
    P.d_Gc.resize(levels); P.d_oc.resize(levels); P.d_carry.resize(levels);
    for (size_t l = 1; l < levels; l++)
        if ((rc = dev_alloc(h, &P.d_Gc[l], std::max<int64_t>(P.level_cap[l], 1) * kd * kd)) != CX_OK) return rc;
    CX_HIP(h, hipStreamSynchronize(h->stream));      // (the host vectors die here)
    P.h_cflag.assign((size_t)P.n_comp, 0);
    P.nv = h->nv; P.ne = h->ne;
    P.vinfo_epoch = h->vinfo_epoch;
    P.valid = true;
    return CX_OK;
}

inline unsigned blocks(int64_t n, int b) { return (unsigned)((n + b - 1) / b); }

template <int NT>
void launch_cond(cx_handle *h, Plan &P) {
    // waves per SIMD as the register counts allow; the launch bound makes hipcc keep to them without scratch
    constexpr int W = NT == 1 ? 4 : NT == 2 ? 3 : 2;
    if (P.n_item)
        hipLaunchKernelGGL((k_spm_cond<NT, W>), dim3((unsigned)P.n_item), dim3(64), 0, h->stream, (int)P.n_item, P.d_rec, P.d_srcs, h->d_ptab, h->d_ptab_bt,
                           h->d_mv_f2v, mfr::user_dim(h), P.d_link, P.d_st);
    if (P.n_comp) {
        hipLaunchKernelGGL(sp::k_sp_flag, dim3((unsigned)P.n_chunk), dim3(sp::kT), 0, h->stream, P.d_cbeg, P.d_cpos, P.d_st, P.d_cpart);
        hipLaunchKernelGGL(sp::k_sp_flag_comp, dim3(blocks(P.n_comp, sp::kT)), dim3(sp::kT), 0, h->stream, P.n_comp, P.d_ccb, P.d_cpart, P.d_cflag);
    }
}

// the scan of a chunk of S samples (np panels), as sp::launch_samples goes through the depths and levels
template <int NT>
void launch_samples(cx_handle *h, Plan &P, int64_t S, const Gen &g) {
    const int np = (int)(S / kPanel);
    for (const sp::Depth &dp : P.depths) {
        for (int l = 1; l <= dp.levels; l++) {
            const int64_t n = dp.n_items[(size_t)l - 1];
            const int2 *rng = P.d_rng + dp.rng_off[(size_t)l - 1];
            const unsigned grid = (unsigned)(n * (np + NT));
            if (l == 1)
                hipLaunchKernelGGL((k_spm_compose<NT, true>), dim3(grid), dim3(64), 0, h->stream, n, np, rng, P.d_link, P.d_pos_var, g, nullptr, nullptr, P.d_Gc[1],
                                   P.d_oc[1]);
            else
                hipLaunchKernelGGL((k_spm_compose<NT, false>), dim3(grid), dim3(64), 0, h->stream, n, np, rng, P.d_link, P.d_pos_var, g, P.d_Gc[(size_t)l - 1],
                                   P.d_oc[(size_t)l - 1], P.d_Gc[(size_t)l], P.d_oc[(size_t)l]);
        }
        const int4 *top = P.d_top + dp.top_off;
        const int L = dp.levels;
        const unsigned gtop = (unsigned)(dp.n_paths * np);
        if (L == 0)
            hipLaunchKernelGGL((k_spm_walk<NT, true, true>), dim3(gtop), dim3(64), 0, h->stream, dp.n_paths, np, S, top, nullptr, nullptr, P.d_link, P.d_pos_var, g,
                               nullptr, nullptr, nullptr, P.d_Z);
        else
            hipLaunchKernelGGL((k_spm_walk<NT, false, true>), dim3(gtop), dim3(64), 0, h->stream, dp.n_paths, np, S, top, nullptr, nullptr, P.d_link, P.d_pos_var, g,
                               P.d_Gc[(size_t)L], P.d_oc[(size_t)L], P.d_carry[(size_t)L], P.d_Z);
        for (int l = L; l >= 1; l--) {
            const int64_t n = dp.n_items[(size_t)l - 1];
            const int2 *rng = P.d_rng + dp.rng_off[(size_t)l - 1];
            const unsigned grid = (unsigned)(n * np);
            if (l == 1)
                hipLaunchKernelGGL((k_spm_walk<NT, true, false>), dim3(grid), dim3(64), 0, h->stream, n, np, S, nullptr, rng, P.d_carry[1], P.d_link, P.d_pos_var, g,
                                   nullptr, nullptr, nullptr, P.d_Z);
            else
                hipLaunchKernelGGL((k_spm_walk<NT, false, false>), dim3(grid), dim3(64), 0, h->stream, n, np, S, nullptr, rng, P.d_carry[(size_t)l], P.d_link,
                                   P.d_pos_var, g, P.d_Gc[(size_t)l - 1], P.d_oc[(size_t)l - 1], P.d_carry[(size_t)l - 1], P.d_Z);
        }
    }
}

// z and the level buffers for a chunk of S samples (or functionals)
inline int32_t ensure_chunk(cx_handle *h, Plan &P, int64_t S) {
    const int64_t kd = h->cfg.dim;
    int32_t rc;
    if ((rc = P.d_Z.ensure(h, std::max<int64_t>(P.npos, 1) * S * kd)) != CX_OK) return rc;
    for (size_t l = 1; l < P.level_cap.size(); l++)
        if ((rc = P.d_oc[l].ensure(h, std::max<int64_t>(P.level_cap[l], 1) * S * kd)) != CX_OK ||
            (rc = P.d_carry[l].ensure(h, std::max<int64_t>(P.level_cap[l], 1) * S * kd)) != CX_OK) return rc;
    return CX_OK;
}

// the handle's plan, rebuilt when the graph or the observed flags have changed
inline int32_t plan_of(cx_handle *h, const std::string &who, Plan *&Pp) {
    if (!h->sample_mfma) h->sample_mfma.reset(new Plan());
    Plan &P = *h->sample_mfma;
    if (!P.valid || P.nv != h->nv || P.ne != h->ne || P.vinfo_epoch != h->vinfo_epoch) {
        const int32_t rc = build_plan(h, P, who);
        if (rc != CX_OK) return rc;
    }
    Pp = &P;
    return CX_OK;
}

}  // namespace spm
}  // namespace cx
