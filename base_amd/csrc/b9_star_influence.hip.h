// b9_star_influence.hip.h -- b9_star_influence (the starInfluence counterpart): k_infl_accumulate (the per-star leave-one-star-out
// state of the caller's per-row quantities, one LANE per star) and k_infl_groups (a row's sums of v over the stars of each group,
// one WAVE per row).  The values v come from b9_pointwise's kernels (k_star_lpd / k_star_lpd_wd, b9_pointwise.hip.h): the same
// scratch [row][star] and the same row_in; the tails are k_pw_tail's.
// Part of the single translation unit b9_kernels.hip (included there, after b9_pointwise.hip.h); gfx950 only.
#pragma once

// ------------------------------------------------------------------------------------------
// Star influence ("Star influence").  Stars are independent given the cluster parameters, so the posterior
// without star i is the chain reweighted by exp(-v_ri).  Per star the kernel carries the six head words -- (ROWS, NINF, RMAX,
// SNEG) by k_pw_accumulate's rule, the same instruction sequence and so the same bits; SNEG2 the sum of the squared weights;
// MEANV the Welford mean of v -- and per quantity q_j the four words WQ = sum w q, WQ2 = sum w q^2 (both in the scale of RMAX,
// rescaled with SNEG at a jump of the maximum), MQ the Welford mean of q over the star's finite rows and CVQ the co-moment of
// (v, q).  No random numbers, no atomics.
//
// k_infl_accumulate<QT>: grid (256-star chunk) x 256, one launch per tile of QT quantities, `tile` an argument.  A lane's row
// values are independent loads, all issued before the dependent chain, as in k_pw_accumulate.  q [n_rows][n_q] is the chunk's part of the caller's array: r and j
// are uniform over the wave, so its words are read as uniform loads and live in scalar registers.  Every tile recomputes the
// head from the words the call before left in acc; only the launch with store_head set -- the last of the chunk, ordered after
// the others by the stream -- writes it back, so no launch reads a head that a workgroup of the same launch may have advanced.
// A quantity's words never meet another quantity's, so its bits do not depend on QT, on n_q or on its place.  A tile's last quantities past n_q are worked on quantity n_q - 1 and not stored.
// State: 6 + 4 QT doubles on top of the B9_PW_MAX_ROWS row values: 54 at QT = 4 -- no instance carries scratch
// (profiles/influence_kernel_resources.txt).
// ------------------------------------------------------------------------------------------
template <int QT>
__global__ __launch_bounds__(256) void k_infl_accumulate(const double *__restrict__ scratch, const int *__restrict__ row_in, int n_rows, int n_stars,
                                                         const double *__restrict__ q, int n_q, int tile, int store_head, double *__restrict__ acc)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n_stars) return;
    const int j0 = tile * QT, n_acc = B9_INF_N(n_q);
    double v[B9_PW_MAX_ROWS];
#pragma unroll
    for (int r = 0; r < B9_PW_MAX_ROWS; ++r) v[r] = (r < n_rows && row_in[r]) ? scratch[(size_t)r * n_stars + i] : 0.0;
    double *__restrict__ const a = acc + (size_t)i * n_acc;
    double rows = a[B9_INF_ROWS], ninf = a[B9_INF_NINF], rmax = a[B9_INF_RMAX], sneg = a[B9_INF_SNEG], sneg2 = a[B9_INF_SNEG2], meanv = a[B9_INF_MEANV];
    int jq[QT];                                          // the tile's quantities (uniform)
    double wq[QT], wq2[QT], mq[QT], cvq[QT];
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        jq[t] = min(j0 + t, n_q - 1);
        wq[t] = a[B9_INF_WQ(jq[t])]; wq2[t] = a[B9_INF_WQ(jq[t]) + 1]; mq[t] = a[B9_INF_WQ(jq[t]) + 2]; cvq[t] = a[B9_INF_WQ(jq[t]) + 3];
    }
#pragma unroll
    for (int r = 0; r < B9_PW_MAX_ROWS; ++r) {
        if (r >= n_rows || !row_in[r]) continue;
        const double x = v[r], k = rows - ninf;          // k: the finite rows taken so far
        rows = rows + 1.0;
        if (x == NEG_INF) { ninf = ninf + 1.0; continue; }
        const double *__restrict__ const qr = q + (size_t)r * n_q;
        const double w = -x;
        if (k == 0.0) {
            rmax = w; sneg = 1.0; sneg2 = 1.0; meanv = x;
#pragma unroll
            for (int t = 0; t < QT; ++t) { const double y = qr[jq[t]]; wq[t] = y; wq2[t] = y * y; mq[t] = y; cvq[t] = 0.0; }
            continue;
        }
        if (w > rmax) {
            const double f = exp(rmax - w), ff = f * f;
            sneg = __builtin_fma(sneg, f, 1.0);
            sneg2 = __builtin_fma(sneg2, ff, 1.0);
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const double y = qr[jq[t]];
                wq[t] = __builtin_fma(wq[t], f, y);
                wq2[t] = __builtin_fma(wq2[t], f, y * y);
            }
            rmax = w;
        } else {
            const double e = exp(w - rmax);
            sneg = sneg + e;
            sneg2 = __builtin_fma(e, e, sneg2);
#pragma unroll
            for (int t = 0; t < QT; ++t) {
                const double y = qr[jq[t]];
                wq[t] = __builtin_fma(e, y, wq[t]);
                wq2[t] = __builtin_fma(e * y, y, wq2[t]);
            }
        }
        const double dv = x - meanv;
        meanv = meanv + dv / (k + 1.0);
#pragma unroll
        for (int t = 0; t < QT; ++t) {
            const double y = qr[jq[t]], dq = y - mq[t];
            mq[t] = mq[t] + dq / (k + 1.0);
            cvq[t] = __builtin_fma(dv, y - mq[t], cvq[t]);
        }
    }
    if (store_head) {
        a[B9_INF_ROWS] = rows; a[B9_INF_NINF] = ninf; a[B9_INF_RMAX] = rmax; a[B9_INF_SNEG] = sneg; a[B9_INF_SNEG2] = sneg2; a[B9_INF_MEANV] = meanv;
    }
#pragma unroll
    for (int t = 0; t < QT; ++t) {
        if (j0 + t >= n_q) continue;
        a[B9_INF_WQ(j0 + t)] = wq[t]; a[B9_INF_WQ(j0 + t) + 1] = wq2[t]; a[B9_INF_WQ(j0 + t) + 2] = mq[t]; a[B9_INF_WQ(j0 + t) + 3] = cvq[t];
    }
}

// ------------------------------------------------------------------------------------------
// k_infl_groups<NG>: one WAVE per row, k_pw_rows' frame: the wave reads the row's values and the stars' group ids coalesced, in
// k_pw_rows' batches of 64 B9_PW_ROWS_UNROLL stars.  Every lane forms its star as each group sees it -- v where the star's id is the
// group's, +0.0 elsewhere -- and every such word goes through a scalar register pair (v_readlane) into the group's accumulator, one
// plain add each in star order.  Adding +0.0 leaves a chain's bits alone (no chain is ever -0.0: each starts from +0.0).  The NG
// chains are independent, so they overlap where k_pw_rows' single chain waits for itself.  (Selecting per star on the scalar side --
// the value and the id both read across, a compare and two selects per group -- took 585 us a chunk of 32 rows at 20k stars and two
// groups against 221 us for this form; docs/LABNOTES.md section 39.)  -inf propagates; a row outside the grid gives -inf for every
// group.  out [n_rows][n_groups]; NG >= n_groups, the chains past n_groups take +0.0 only and are not stored.
// ------------------------------------------------------------------------------------------
template <int NG>
__global__ __launch_bounds__(64) void k_infl_groups(const double *__restrict__ scratch, const int *__restrict__ row_in, int n_stars,
                                                    const int *__restrict__ group, int n_groups, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const int r = blockIdx.x, lane = threadIdx.x;
    if (!row_in[r]) {
        if (lane < n_groups) out[(size_t)r * n_groups + lane] = NEG_INF;
        return;
    }
    const double *__restrict__ const x = scratch + (size_t)r * n_stars;
    double a[NG];
#pragma unroll
    for (int g = 0; g < NG; ++g) a[g] = 0.0;
    int s = 0;
    for (; s + 64 * B9_PW_ROWS_UNROLL <= n_stars; s += 64 * B9_PW_ROWS_UNROLL) {       // (k_pw_rows' batches: the loads of 512 stars in flight)
        double v[B9_PW_ROWS_UNROLL];
        int id[B9_PW_ROWS_UNROLL];
#pragma unroll
        for (int u = 0; u < B9_PW_ROWS_UNROLL; ++u) { v[u] = x[s + 64 * u + lane]; id[u] = group[s + 64 * u + lane]; }
#pragma unroll
        for (int u = 0; u < B9_PW_ROWS_UNROLL; ++u) {
            double m[NG];                                // the lane's star as every group sees it: the select is done once, in the lanes
#pragma unroll
            for (int g = 0; g < NG; ++g) m[g] = id[u] == g ? v[u] : 0.0;
#pragma unroll
            for (int l = 0; l < 64; ++l) {
#pragma unroll
                for (int g = 0; g < NG; ++g) a[g] = a[g] + pw_lane(m[g], l);
            }
        }
    }
    for (; s < n_stars; s += 64) {                       // the last, partial batch: 64 stars at a time, the very last ones counted
        const int n_last = min(64, n_stars - s);
        const double v = lane < n_last ? x[s + lane] : 0.0;
        const int id = lane < n_last ? group[s + lane] : -1;
        double m[NG];
#pragma unroll
        for (int g = 0; g < NG; ++g) m[g] = id == g ? v : 0.0;
        for (int l = 0; l < n_last; ++l) {
#pragma unroll
            for (int g = 0; g < NG; ++g) a[g] = a[g] + pw_lane(m[g], l);
        }
    }
    if (lane == 0) {
#pragma unroll
        for (int g = 0; g < NG; ++g)
            if (g < n_groups) out[(size_t)r * n_groups + g] = a[g];
    }
}
