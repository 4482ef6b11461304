// cx_sample.hip — cx_sample_posterior: joint draws of the non-observed variables of a Gaussian forest (dim 1 .. 4) from the stored
// factor→variable messages, on the device: forward filtering, backward sampling on any forest.  No counterpart in the reference
// (Cortex.jl computes no numbers); the derivation is DESIGN.md §4g.
//
//   q(x) = b_r(x_r) Π_a b_a(x_{C_a} | x_{p_a})       per component, rooted where cx::treeplan::root_forest roots it (at an end of a
//                                                     longest path), p_a the factor's variable nearest the root, C_a its other free ones
//
// In coordinates centred on every variable's belief mean c (x = c + z) a draw is the affine recursion, down the rooted forest,
//   z_C = G z_p + off + L⁻ᵀ ε_C,    J_CC = L L',  G = -J_CC⁻¹ J_Cp,  off = J_CC⁻¹ h_C
// (J, h: the factor belief's joint precision and right-hand side, centred, as cx_log_evidence forms them); the root: z_r = L_r⁻ᵀ ε_r
// with Λ_r = L_r L_r'.  z has the size of the posterior spread whatever the size of the data.
//
//   plan (host, cached)  every free variable gets a POSITION: the forest cut into heavy paths (every variable on exactly one path,
//                        leaves included), paths by light depth, positions in path order, the head's link first
//   k_sp_cond            one thread per root and per two-variable link factor: the link (G | off | L⁻ᵀ) of the child, in registers
//   k_sp_cond_kary       one thread per factor of 3 .. 7 variables with two or more free ones: the joint in LDS, the links of all its
//                        children (a child's noise also reads its later siblings' ε: the extra blocks of L⁻ᵀ)
//   k_sp_flag            one block per chunk of 8192 positions of one component, then one thread per component: the status of
//                        its links ORed (undefined input / not positive definite)
//   per light depth      a blocked scan of the affine maps along the paths, for every sample (S lanes per tile):
//     k_sp_compose       level l: one thread per (tile of 64 items of level l - 1, sample) composes the offsets from zero; one more
//                        thread per tile the matrix product (shared by all samples)
//     k_sp_walk<TOP>     one thread per (path, sample): from the head's parent (written by a smaller light depth) over the top tiles
//     k_sp_walk          level l .. 1: from each tile's carry over its items; level 1 writes z of every position
//   k_sp_gather          out[s][i] = c + z, the datum of observed variables, NaN in a failed component; nontemporal stores
// The standard normals come from Philox4x32-10 in registers, counter (pair of components, variable index, sample): a draw does not
// depend on the launch, the requested ids or the number of samples.  No atomics: two calls on one state are bit-identical.
#include "cx_sample_core.h"

namespace cx {

template <> void Deleter<sp::Plan>::operator()(sp::Plan *P) const { delete P; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_sample_posterior(cx_handle *h, int64_t n_samples, uint64_t seed, const double *noise, int64_t n, const int64_t *variable_ids,
                                       double *out, int64_t *counts4) {
    const std::string who = "cx_sample_posterior";
    try {
        cx::ev::Cache *Ep = nullptr;
        int32_t rc;
        const char *bad = n_samples >= 1 && out && counts4 && (!variable_ids || n >= 0)
                              ? nullptr : "n_samples < 1, a null output or counts4, or a negative count with variable ids";
        if ((rc = cx::ev::prepare(h, who, bad, Ep)) != CX_OK) return rc;
        CX_REQUIRE(h, !h->offsets_nonzero, CX_ERR_UNSUPPORTED, who + ": the handle has non-zero factor offsets (cx_set_factor_offsets), which this call does not implement");
        cx::ev::Cache &E = *Ep;
        cx::sp::Plan *Pp = nullptr;
        if ((rc = cx::sp::plan_of(h, E, who, Pp)) != CX_OK) return rc;
        cx::sp::Plan &P = *Pp;
        const int d = h->cfg.dim;
        const int64_t nv = h->nv, nout = variable_ids ? n : nv;
        std::vector<int32_t> vids;
        if (variable_ids) {
            vids.resize((size_t)n);
            for (int64_t i = 0; i < n; i++) {
                const int64_t v = find_var(h, variable_ids[i]);
                if (v < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no variable " + std::to_string(variable_ids[i]));
                vids[(size_t)i] = (int32_t)v;
            }
            if ((rc = P.d_vid.ensure(h, n)) != CX_OK) return rc;
            if (n) CX_HIP(h, hipMemcpyAsync(P.d_vid, vids.data(), (size_t)n * 4, hipMemcpyHostToDevice, h->stream));
        }
        // samples in chunks of at most ~2^27 doubles of scratch (z, the level buffers, the output, the caller's noise)
        int64_t per = P.npos + nout + (noise ? nv : 0);
        for (size_t l = 1; l < P.level_cap.size(); l++) per += 2 * P.level_cap[l];
        per = std::max<int64_t>(per * d, 1);
        const int64_t chunk = std::max<int64_t>(1, std::min<int64_t>(n_samples, ((int64_t)1 << 27) / per));
        CX_HIP(h, hipStreamSynchronize(h->stream));
        cx::ev::var_pass(h, E);
        for (int64_t s0 = 0; s0 < n_samples; s0 += chunk) {
            const int S = (int)std::min<int64_t>(chunk, n_samples - s0);
            if ((rc = cx::sp::ensure_chunk(h, P, S, nout, noise != nullptr)) != CX_OK) return rc;
            if (noise) CX_HIP(h, hipMemcpyAsync(P.d_noise, noise + s0 * nv * d, (size_t)(S * nv * d) * sizeof(double), hipMemcpyHostToDevice, h->stream));
            const cx::sp::Gen g{noise ? P.d_noise : nullptr, nv * d, seed, s0};
            const int32_t *dv = variable_ids ? P.d_vid : nullptr;
            if (nout || s0 == 0) {
                cx::ev::with_dim(d, [&](auto D) {
                    if (nout) cx::sp::launch_all<D()>(h, E, P, S, g, nout, dv, s0 == 0);
                    else cx::sp::launch_cond<D()>(h, E, P);
                });
                CX_HIP(h, hipGetLastError());
            }
            if (nout) CX_HIP(h, hipMemcpyAsync(out + s0 * nout * d, P.d_out, (size_t)(S * nout * d) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            CX_HIP(h, hipStreamSynchronize(h->stream));      // (the caller's noise chunk is read before the next one is copied)
        }
        if (P.n_comp) CX_HIP(h, hipMemcpy(P.h_cflag.data(), P.d_cflag, (size_t)P.n_comp, hipMemcpyDeviceToHost));
        int64_t und = 0, npd = 0;
        for (uint8_t c : P.h_cflag) { und += (c & 1) != 0; npd += (c & 1) == 0 && (c & 2) != 0; }
        counts4[0] = P.npos;
        counts4[1] = P.n_comp;
        counts4[2] = und;
        counts4[3] = npd;
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": host allocation failed"); }
}
