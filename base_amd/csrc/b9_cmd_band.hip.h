// b9_cmd_band.hip.h -- b9_cmd_band (the cmdBand counterpart): the model locus a saved chain implies in the CMD, reduced over the rows
// line by line.  k_band_points (the MS/RGB points of every ratio locus) and k_band_wd_points (the WD points, gathered from
// k_wd_node_table_status' table) write a chunk of rows' value table; k_band_accumulate walks it row by row, one lane per line.
// Part of the single translation unit b9_kernels.hip (included there, after b9_wd_moments.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// A population has P = n_ratio n_eep + n_types n_wd_nodes points of C = 1 + nf + n_colour columns (the ZAMS mass, the apparent
// magnitudes, the colours); line (k P + p) C + c (include/base9_hip.h).  The value table of a chunk is [row][line], line-major:
// the accumulation's lanes over consecutive lines read 512 contiguous bytes per row.  A word that does not enter -- the point does
// not exist in the row, the magnitude is not finite or is B9_MAG_NOFLUX, a colour lacks one of its filters -- is a NaN.
// Nothing of a word depends on the spec's other points or columns, on the chunk or on the launch.  B9BandSpec: b9_launch.h.
// ------------------------------------------------------------------------------------------
using BandSpecDev = B9BandSpec;

#define B9_BAND_ABSENT (__builtin_nan(""))

// a point's columns from its mass and its apparent magnitudes x[f] (already B9_BAND_ABSENT where the filter does not enter).
// A colour's filters are run-time indices: the lane reads its own two words back from the table (a dynamic index into x would
// put the array in scratch); an absent filter's NaN makes the colour absent.
template <int NFP>
__device__ __forceinline__ void band_store_point(const BandSpecDev &sp, int nf, double *out, double mass, const double (&x)[NFP])
{
    out[0] = mass;
#pragma unroll
    for (int f = 0; f < NFP; ++f) if (f < nf) out[1 + f] = x[f];
    for (int c = 0; c < sp.n_colour; ++c) out[1 + nf + c] = out[1 + sp.colour[c][0]] - out[1 + sp.colour[c][1]];
}

// k_band_points: one lane per (row-population wp = blockIdx.y, locus s, EEP e).  The primary is the derived isochrone's point
// itself (b9_derive_isochrone's arrays), the secondary msrgb_mags at q m on the same isochrone, combined by k_predict_mags'
// expression under its `dark` rule; then + (mod + (A_f / A_V - 1) A_V).
template <int NFP>
__global__ __launch_bounds__(256) void k_band_points(DevPack pk, const IsoHdr *__restrict__ hdr, const double *__restrict__ iso_data, long long iso_stride,
                                                     int mass_cap, int n_pops, const double *__restrict__ params, BandSpecDev sp, double *__restrict__ values)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= sp.n_ratio * sp.n_eep) return;
    const int wp = blockIdx.y, w = wp / n_pops, k = wp - w * n_pops;
    const int s = i / sp.n_eep, ei = i - s * sp.n_eep;
    const IsoHdr h = hdr[wp];
    const int nf = pk.nf;
    double *out = values + (size_t)w * sp.n_lines + ((size_t)k * sp.P + (size_t)i) * sp.C;
    const long long idx = ((long long)sp.eep0 + ei) - h.first_eep;
    if (!h.valid || idx < 0 || idx >= h.n) {
        for (int c = 0; c < sp.C; ++c) out[c] = B9_BAND_ABSENT;
        return;
    }
    const double *par = params + (size_t)w * B9_NPARAM;
    const double mod = par[B9_P_MOD], av = par[B9_P_ABS];
    const double *g = iso_data + (size_t)wp * iso_stride;
    const IsoView<NFP> iso = iso_view_of<NFP>(h, g, g + mass_cap);
    const double m = iso.mass[idx], q = sp.ratio[s];
    double p1[NFP];
    bool dark[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) { p1[f] = iso.mags[(size_t)idx * NFP + f]; dark[f] = p1[f] == B9_MAG_NOFLUX; }
    if (q > 0.0) {
        double p2[NFP];
        msrgb_mags<NFP>(iso, q * m, p2);
#pragma unroll
        for (int f = 0; f < NFP; ++f) {
            dark[f] = dark[f] && p2[f] == B9_MAG_NOFLUX;
            p1[f] -= (2.5 / LN10) * log1pexp((-0.4 * LN10) * (p2[f] - p1[f]));
        }
    }
#pragma unroll
    for (int f = 0; f < NFP; ++f) {
        const double x = p1[f] + (mod + pk.abs_m1[f] * av);
        p1[f] = (dark[f] || !isfinite(x) || x == B9_MAG_NOFLUX) ? B9_BAND_ABSENT : x;
    }
    band_store_point<NFP>(sp, nf, out, m, p1);
}

// k_band_wd_points: one lane per (row-population wp = blockIdx.y, selected type t, node j): the node's row and status of the chunk's
// node table (k_wd_node_table_status; its magnitudes are apparent already), its mass tip + dM (double)j on the table's own grid.
template <int NFP>
__global__ __launch_bounds__(256) void k_band_wd_points(DevPack pk, const IsoHdr *__restrict__ hdr, int n_pops, const double *__restrict__ tab, int n_wp,
                                                        BandSpecDev sp, double *__restrict__ values)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    const int n_nodes = sp.n_wd_nodes;
    if (i >= sp.n_types * n_nodes) return;
    const int wp = blockIdx.y, w = wp / n_pops, k = wp - w * n_pops;
    const int t = i / n_nodes, j0 = i - t * n_nodes;                 // node j = j0 + 1
    const IsoHdr h = hdr[wp];
    const int nf = pk.nf;
    double *out = values + (size_t)w * sp.n_lines + ((size_t)k * sp.P + (size_t)sp.n_ratio * sp.n_eep + (size_t)i) * sp.C;
    const double dM = (pk.m_wd_up - h.agb_tip) / n_nodes;
    const WdTable<const double> T = wd_table_view(tab, NFP, n_wp, n_nodes);
    // (the table holds nothing for a population outside the grid or without steps: its words are read only behind this guard)
    bool exists = h.valid && dM > 0.0;
    if (exists) exists = T.der[(size_t)n_wp * n_nodes * B9_WDS_DER + (size_t)wp * n_nodes + j0] == 2.0;
    if (!exists) {
        for (int c = 0; c < sp.C; ++c) out[c] = B9_BAND_ABSENT;
        return;
    }
    const double *row = T.rows + (((size_t)wp * 2 + sp.type_id[t]) * n_nodes + (size_t)j0) * NFP;
    double x[NFP];
#pragma unroll
    for (int f = 0; f < NFP; ++f) {
        const double v = row[f];
        x[f] = (!isfinite(v) || v == B9_MAG_NOFLUX) ? B9_BAND_ABSENT : v;
    }
    band_store_point<NFP>(sp, nf, out, h.agb_tip + dM * (double)(j0 + 1), x);
}

// k_band_accumulate: one lane per line, the chunk's rows in ascending order: d = v - pivot, then N += 1, SUM += d, SUMSQ += d d,
// MIN = fmin, MAX = fmax, and + 1.0 to one bin word -- each one plain IEEE operation per row.  The state is carried whole in mom
// [line][B9_BAND_NMOM] and bins [line][n_bins + 3] (either may be null), so chunks and continued calls are invisible.
// The bin words live in LDS, [word][lane]: 33 words under a run-time index would otherwise go to scratch; so do the line's edges,
// which come in as [b][line] (a wave's loads coalesce).  A lane's LDS words are its own: no barrier is needed.
//   dynamic LDS: bins [n_bins + 3][64] | edges [n_bins + 1][64]   (bins null: none)
__global__ __launch_bounds__(64) void k_band_accumulate(const double *__restrict__ values, int n_rows, long long n_lines, const double *__restrict__ pivot,
                                                        double *__restrict__ mom, double *__restrict__ bins, const double *__restrict__ edges_t, int n_bins)
{
    extern __shared__ double s_band[];
    const int lane = threadIdx.x;
    const long long line = (long long)blockIdx.x * 64 + lane;
    if (line >= n_lines) return;
    double *const s_bin = s_band + lane, *const s_edge = s_band + (size_t)(n_bins + 3) * 64 + lane;
    const double piv = pivot[line];
    double n = 0.0, sum = 0.0, sumsq = 0.0, mn = 0.0, mx = 0.0;
    if (mom) {
        const double *m = mom + (size_t)line * B9_BAND_NMOM;
        n = m[B9_BAND_N]; sum = m[B9_BAND_SUM]; sumsq = m[B9_BAND_SUMSQ]; mn = m[B9_BAND_MIN]; mx = m[B9_BAND_MAX];
    }
    if (bins) {
        for (int w = 0; w < n_bins + 3; ++w) s_bin[w * 64] = bins[(size_t)line * (n_bins + 3) + w];
        for (int b = 0; b <= n_bins; ++b) s_edge[b * 64] = edges_t[(size_t)b * n_lines + line];
    }
    for (int r = 0; r < n_rows; ++r) {
        const double v = values[(size_t)r * n_lines + line];
        if (v != v) continue;
        const double d = v - piv;
        n += 1.0; sum += d; sumsq += d * d; mn = fmin(mn, v); mx = fmax(mx, v);
        if (bins) {
            int lo = 0, hi = n_bins + 1;                 // the number of edges <= v: 0 below, 1 + b in bin b, n_bins + 1 at or above
            while (lo < hi) {
                const int mid = (lo + hi) >> 1;
                if (s_edge[mid * 64] <= v) lo = mid + 1; else hi = mid;
            }
            s_bin[lo * 64] += 1.0;
            s_bin[(n_bins + 2) * 64] += 1.0;
        }
    }
    if (mom) {
        double *m = mom + (size_t)line * B9_BAND_NMOM;
        m[B9_BAND_N] = n; m[B9_BAND_SUM] = sum; m[B9_BAND_SUMSQ] = sumsq; m[B9_BAND_MIN] = mn; m[B9_BAND_MAX] = mx;
    }
    if (bins)
        for (int w = 0; w < n_bins + 3; ++w) bins[(size_t)line * (n_bins + 3) + w] = s_bin[w * 64];
}
