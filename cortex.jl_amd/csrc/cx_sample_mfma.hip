// cx_sample_mfma.hip — cx_sample_posterior_mfma: cx_sample_posterior at the matrix-core dims (cx_create dim 5 .. 64,
// internal tiles of 16 / 32 / 64): joint draws of the non-observed variables of a Gaussian forest from the stored factor→variable
// messages and the data.  The derivation is DESIGN.md §4r.  The links, the panels, the blocked scan and the plan are those of
// cx_sample_mfma_core.h, shared with cx_linear_moments_mfma (cx_functional_mfma.hip); here: the gather and the entry.
//
//   k_spm_gather         out[s][i][0 .. u) = x: z is laid out [position][sample][KD], so a row is one run of u doubles
#include "cx_sample_mfma_core.h"

namespace cx {
namespace spm {

// ---- out[s][i][0 .. u) = x (the datum of an observed variable, NaN in a failed or improper component): one thread per double ---------
__global__ __launch_bounds__(256) void k_spm_gather(int64_t n, int64_t n_valid, int64_t S, int u, int kd, const int32_t *__restrict__ vids,
                                                    const uint8_t *__restrict__ vinfo, const int32_t *__restrict__ dslot, const int32_t *__restrict__ var_pos,
                                                    const int32_t *__restrict__ comp, const uint8_t *__restrict__ cflag, const uint8_t *__restrict__ cimp,
                                                    const double *__restrict__ v2f, const double *__restrict__ Zb, double *__restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (t >= n_valid * n * u) return;
    const int64_t row = t / u, s = row / n, i = row - s * n;
    const int k = (int)(t - row * u);
    const int32_t v = vids ? vids[i] : (int32_t)i;
    double x;
    if (vinfo[v] & kClamped) x = dslot[v] >= 0 ? v2f[(int64_t)dslot[v] * ((int64_t)kd * (kd + 1)) + k] : __builtin_nan("");
    else {
        const int32_t q = var_pos[v], cc = comp[q];
        x = (cflag[cc] | cimp[cc]) ? __builtin_nan("") : Zb[((int64_t)q * S + s) * kd + k];
    }
    __builtin_nontemporal_store(x, out + t);
}

}  // namespace spm

template <> void Deleter<spm::Plan>::operator()(spm::Plan *P) const { delete P; }

}  // namespace cx

using namespace cxh;

extern "C" int32_t cx_sample_posterior_mfma(cx_handle *h, int64_t n_samples, uint64_t seed, const double *noise, int64_t n, const int64_t *variable_ids,
                                            double *out, int64_t *counts4) {
    const std::string who = "cx_sample_posterior_mfma";
    try {
        namespace spm = cx::spm;
        namespace mfr = cx::mfr;
        int32_t rc;
        const char *bad = n_samples >= 1 && out && counts4 && (!variable_ids || n >= 0)
                              ? nullptr : "n_samples < 1, a null output or counts4, or a negative count with variable ids";
        if ((rc = mfr::prepare(h, who, bad, {"cx_sample_posterior", "the variational and Beta-Bernoulli families have no Gaussian joint to draw from", "links"})) != CX_OK)
            return rc;
        if ((rc = mv_ensure_chain_msgs(h)) != CX_OK) return rc;      // (every reader of d_mv_f2v calls this first)
        spm::Plan *Pp = nullptr;
        if ((rc = spm::plan_of(h, who, Pp)) != CX_OK) return rc;
        spm::Plan &P = *Pp;
        const int kd = h->cfg.dim, u = mfr::user_dim(h);
        const int64_t nv = h->nv, nout = variable_ids ? n : nv;
        if (variable_ids) {
            std::vector<int32_t> vids((size_t)n);
            for (int64_t i = 0; i < n; i++) {
                const int64_t v = find_var(h, variable_ids[i]);
                if (v < 0) return fail(h, CX_ERR_NOT_FOUND, who + ": no variable " + std::to_string(variable_ids[i]));
                vids[(size_t)i] = (int32_t)v;
            }
            if ((rc = P.d_vid.ensure(h, n)) != CX_OK) return rc;
            if (n) CX_HIP(h, hipMemcpy(P.d_vid, vids.data(), (size_t)n * 4, hipMemcpyHostToDevice));
        }
        // samples in chunks of whole panels that keep the scratch (z, the level buffers, the output, the caller's noise) under ~2^27
        // doubles, cx_sample.hip's bound; one panel at the least
        int64_t per = P.npos * kd + nout * u + (noise ? nv * u : 0);
        for (size_t l = 1; l < P.level_cap.size(); l++) per += 2 * P.level_cap[l] * kd;
        per = std::max<int64_t>(per, 1);
        const int64_t padded = (n_samples + spm::kPanel - 1) / spm::kPanel * spm::kPanel;
        int64_t chunk = std::max<int64_t>(spm::kPanel, std::min<int64_t>(padded, ((int64_t)1 << 27) / per / spm::kPanel * spm::kPanel));
        if (const int64_t o = spm::chunk_override("CX_SAMPLE_MFMA_CHUNK")) chunk = std::min(o, padded);
        CX_REQUIRE(h, P.npos * (chunk / spm::kPanel) < (int64_t)0x7fffff00, CX_ERR_UNSUPPORTED, who + ": more than 2^31 (position, panel) pairs in a chunk");
        if ((rc = spm::ensure_chunk(h, P, chunk)) != CX_OK) return rc;
        if (noise && (rc = P.d_noise.ensure(h, chunk * nv * u)) != CX_OK) return rc;
        if ((rc = P.d_out.ensure(h, std::max<int64_t>(chunk * nout * u, 1))) != CX_OK) return rc;
        // the links, once per call
        mfr::for_tiles(kd, [&](auto nt) { spm::launch_cond<decltype(nt)::value>(h, P); });
        CX_HIP(h, hipGetLastError());
        const int32_t *dv = variable_ids ? P.d_vid.get() : nullptr;
        for (int64_t s0 = 0; nout && s0 < n_samples; s0 += chunk) {
            const int64_t valid = std::min<int64_t>(chunk, n_samples - s0);
            const int64_t S = (valid + spm::kPanel - 1) / spm::kPanel * spm::kPanel;
            if (noise) CX_HIP(h, hipMemcpyAsync(P.d_noise, noise + s0 * nv * u, (size_t)(valid * nv * u) * sizeof(double), hipMemcpyHostToDevice, h->stream));
            const spm::Gen g{noise ? P.d_noise.get() : nullptr, nv, seed, s0, valid, u};
            mfr::for_tiles(kd, [&](auto nt) { spm::launch_samples<decltype(nt)::value>(h, P, S, g); });
            hipLaunchKernelGGL(spm::k_spm_gather, dim3(spm::blocks(valid * nout * u, 256)), dim3(256), 0, h->stream, nout, valid, S, u, kd, dv, h->d_vinfo, P.d_dslot,
                               P.d_var_pos, P.d_comp, P.d_cflag, P.d_cimp, h->d_mv_v2f, P.d_Z, P.d_out);
            CX_HIP(h, hipGetLastError());
            CX_HIP(h, hipMemcpyAsync(out + s0 * nout * u, P.d_out, (size_t)(valid * nout * u) * sizeof(double), hipMemcpyDeviceToHost, h->stream));
            CX_HIP(h, hipStreamSynchronize(h->stream));      // (the caller's noise chunk is read before the next one is copied)
        }
        CX_HIP(h, hipStreamSynchronize(h->stream));
        if (P.n_comp) CX_HIP(h, hipMemcpy(P.h_cflag.data(), P.d_cflag, (size_t)P.n_comp, hipMemcpyDeviceToHost));
        int64_t und = 0, npd = 0;
        for (int64_t c = 0; c < P.n_comp; c++) {
            const bool imp = P.h_cimp[(size_t)c] != 0, ud = (P.h_cflag[(size_t)c] & 1) != 0;
            und += !imp && ud;
            npd += imp || (!ud && (P.h_cflag[(size_t)c] & 2) != 0);
        }
        counts4[0] = P.npos;
        counts4[1] = P.n_comp;
        counts4[2] = und;
        counts4[3] = npd;
        return CX_OK;
    } catch (const std::bad_alloc &) { return fail(h, CX_ERR_OUT_OF_MEMORY, who + ": host allocation failed"); }
}
