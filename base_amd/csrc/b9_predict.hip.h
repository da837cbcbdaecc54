// b9_predict.hip.h -- k_predict_mags: the forward half of rows a4-a7, a9 without the chi^2 (b9_predict_mags).
// Part of the single translation unit b9_kernels.hip (included there, after b9_star.hip.h); gfx950 only.
#pragma once

// Predicted apparent magnitudes and stages of n stellar systems at ONE parameter row whose isochrone(s) k_derive_iso_rows
// has derived (hdr / iso_data: one per population).  One lane per system, a grid-stride loop over the systems; every
// workgroup first stages the derived isochrones' mass columns and magnitude rows in LDS (the MS/RGB lookup of every lane
// searches them), the WD branch reads its axes from L2 (wd_axes_global).  A system's magnitudes are
// formed by chi2_system's device functions and expressions -- star_mags of the primary, the flux combination with the
// secondary at q m1 when q > 0, then + (mod + (A_f / A_V - 1) A_V) -- except that a filter in which NEITHER component
// gives flux stays exactly B9_MAG_NOFLUX.  Nothing depends on the lane, the workgroup or the launch's other systems.
//   dynamic LDS: per population mass[mass_cap] | mags[mass_cap][NFP] -- the derived isochrone's block of iso_data as it is
//   (msrgb_mags' binary search reads no further than mass[n - 1])
template <int NFP>
__global__ __launch_bounds__(256) void k_predict_mags(DevPack pk, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data,
                                                      long long iso_stride, int mass_cap, int n_pops, const double *__restrict__ params,
                                                      long long n, const double *__restrict__ mass1, const double *__restrict__ mass_ratio,
                                                      const int *__restrict__ wd_type, const int *__restrict__ pop,
                                                      double *__restrict__ out_mags, int *__restrict__ out_stage)
{
    extern __shared__ double s_iso[];
    __shared__ IsoHdr s_hdr[2];
    __shared__ double s_par[B9_NPARAM];
    const int tid = threadIdx.x;
    const long long per_pop = (long long)mass_cap * (NFP + 1);
    if (tid < n_pops) s_hdr[tid] = hdr[tid];
    if (tid < B9_NPARAM) s_par[tid] = params[tid];
    for (int k = 0; k < n_pops; ++k) {
        const double *g = iso_data + (size_t)k * iso_stride;
        for (long long j = tid; j < per_pop; j += 256) s_iso[k * per_pop + j] = g[j];
    }
    __syncthreads();
    const double mod = s_par[B9_P_MOD], av = s_par[B9_P_ABS];
    const int nf = pk.nf;
    for (long long i = (long long)blockIdx.x * 256 + tid; i < n; i += (long long)gridDim.x * 256) {
        const int k = (n_pops > 1 && pop) ? pop[i] : 0;
        const IsoHdr h = s_hdr[k];
        double *row = out_mags + (size_t)i * nf;
        if (!h.valid) {                              // the row lies outside the grid for this population
#pragma unroll
            for (int f = 0; f < NFP; ++f) if (f < nf) row[f] = B9_MAG_NOFLUX;
            out_stage[i] = B9_STAGE_DNE;
            continue;
        }
        const IsoView<NFP> iso = iso_view_of<NFP>(h, s_iso + k * per_pop, s_iso + k * per_pop + mass_cap);
        const WdAxes ax = wd_axes_global(pk, h.i_feh, h.i_y);
        const double m1 = mass1[i], q = mass_ratio[i];
        const int wt = wd_type ? wd_type[i] : 0;
        double p1[NFP];
        bool dark[NFP];
        star_mags<NFP>(pk, ax, iso, s_par, m1, wt, p1);
#pragma unroll
        for (int f = 0; f < NFP; ++f) dark[f] = p1[f] == B9_MAG_NOFLUX;
        if (q > 0.0) {
            double p2[NFP];
            star_mags<NFP>(pk, ax, iso, s_par, q * m1, wt, p2);
#pragma unroll
            for (int f = 0; f < NFP; ++f) {
                dark[f] = dark[f] && p2[f] == B9_MAG_NOFLUX;
                p1[f] -= (2.5 / LN10) * log1pexp((-0.4 * LN10) * (p2[f] - p1[f]));
            }
        }
#pragma unroll
        for (int f = 0; f < NFP; ++f)
            if (f < nf) row[f] = dark[f] ? B9_MAG_NOFLUX : p1[f] + (mod + pk.abs_m1[f] * av);
        out_stage[i] = m1 <= h.agb_tip ? B9_STAGE_MSRG : (m1 <= pk.m_wd_up ? B9_STAGE_WD : B9_STAGE_NSBH);
    }
}
