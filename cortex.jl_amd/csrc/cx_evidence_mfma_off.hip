// cx_evidence_mfma_off.hip — the terms of cx_log_evidence_mfma / cx_log_evidence_components_mfma for a handle with factor offsets
// (cx_set_factor_offsets_mfma): the entry points of evm_term<NT, true> (cx_evidence_mfma_terms.h, which says why they are a translation
// unit of their own) and their launch.
#include "cx_evidence_mfma_terms.h"

namespace cx {
namespace evm {

// g: [nslots][KD] by slot, kap: [nslots] (k_offset_terms64, cx_mv64.hip)
template <int NT, int WAVES_PER_SIMD>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(WAVES_PER_SIMD, WAVES_PER_SIMD)))
void k_evm_terms_off(int nterm, const int32_t *__restrict__ rec, const int32_t *__restrict__ srcs, const double *__restrict__ ptab,
                     const double *__restrict__ btab, const double *__restrict__ ldq, const double *__restrict__ f2v,
                     const double *__restrict__ v2f, const double *__restrict__ goff, const double *__restrict__ kap, const int u,
                     double *__restrict__ tval, uint8_t *__restrict__ tflag) {
    __shared__ double S[16 * kLdT];
    __shared__ double Vs[NT][16 * kLdT];
    __shared__ double ZS[16 * NT];
    evm_term<NT, true>(nterm, rec, srcs, ptab, btab, ldq, f2v, v2f, goff, kap, u, tval, tflag, S, Vs, ZS);
}

void launch_terms_off(cx_handle *h, int n, const int32_t *d_rec, const int32_t *d_srcs, const double *d_ldq, double *d_tval, uint8_t *d_tflag) {
    const int u = mfr::user_dim(h);
    const unsigned grid = 8u * (unsigned)((n + 7) / 8);      // (an eighth of the terms per XCD, as k_evm_terms)
    mfr::for_tiles(h->cfg.dim, [&](auto nt) {
        constexpr int NT = decltype(nt)::value, W = NT == 1 ? 4 : NT == 2 ? 3 : 2;      // (the plain instances' waves per SIMD)
        hipLaunchKernelGGL((k_evm_terms_off<NT, W>), dim3(grid), dim3(64), 0, h->stream, n, d_rec, d_srcs, h->d_ptab, h->d_ptab_bt, d_ldq, h->d_mv_f2v,
                           h->d_mv_v2f, (const double *)h->d_off_g, (const double *)h->d_off_kappa, u, d_tval, d_tflag);
    });
}

}  // namespace evm
}  // namespace cx
