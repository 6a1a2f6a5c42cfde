// Max-value entropy search from the predictive moments (spx.h SPX_ACQ_MES): log Phi, the per-level term
//     h(g) = g phi(g) / (2 Phi(g)) - log Phi(g)
// and its derivative h'(g) = -(r/2)(1 + g^2 + g r), r = phi / Phi.  Shared by mes_kernels.hip (k_mes_logsurv, k_mes_values) and
// the refinement objective (refine_kernels.hip: acq_terms<SPX_ACQ_DEV_MES>) -- one source, the same bits.  tests/mes_oracle.py
// restates every expression below operation for operation; nothing here may contract into an fma.
//
// The lower tail.  With t = 1 / a^2 and the asymptotic series S = 1 - t + 3 t^2 - 15 t^3 + ... of Phi(a) = phi(a) S / (-a):
//     Q(t) = a^2 (S - 1) = -1 + 3 t - 15 t^2 + ...            (summed directly, Horner, 14 terms: up to 27!! t^13)
//     log S = log1p(Q t)
//     log Phi(a) = -a^2/2 - log(-a) - log(2 pi)/2 + log S
//     h(a)  = Q / (2 S) + log(2 pi)/2 + log(-a) - log S          (the two halves -+a^2/2 never formed)
//     h'(a) = W(t) / (2 a S^2),   W = (1 + Q)/t + Q = 2 - 12 t + 90 t^2 - ...   (13 terms; h' -> 1/a)
// Switch-overs:
//   SPX_MES_ERFC_UNDERFLOW = -37.5: below it 0.5 erfc(-a / sqrt 2) leaves the normal range (4.7e-308 at -37.5) and log Phi takes
//     the series; above it log(0.5 erfc) keeps relative accuracy, so k_mes_logsurv never needs the series for a finite sum.
//   SPX_MES_SERIES_BELOW = -12: below it h and h' take the series.  At -12 the first term left out of S is 29!! / 12^30 =
//     2.6e-17 (4e-15 in Q); closer to zero the truncation grows quickly (6e-13 in Q at -10) and the series turns at k = g^2 / 2.
//     Above -12 the plain formula is used.  Its two terms of size g^2 / 2 cancel to about log(-g) + 0.42, and the larger one
//     carries the rounding of g / sqrt 2 through erfc (2 (g^2 / 2) u relative): g^4 u / 2 absolute, 1.1e-12 at -12, where the
//     series takes over, instead of 4e-11 at -30 and NaN / -inf below -37.5.  W has 13 terms: the first one left out is
//     28 * 27!! / 12^26 = 2.6e-13 of h' at -12 (2e-15 at -14, under an ulp from -16 on) -- a gradient weight, where the plain
//     formula's 1 + g^2 + g r cancels to 2 / g^2 and loses g^4 / 2 ulp.
// SPX_MES_HOST: the same text compiled for the host (tests/c/mes_client.cpp, built with -ffp-contract=off), so that the series
// coefficients, the switch-overs and the order of operations of THIS file are held to the 50-digit yardstick on a CPU at the
// bound of the last place; on the device only erfc, exp, log and log1p come from another library.
#pragma once
#ifdef SPX_MES_HOST
#include <cmath>
#define SPX_MES_FN static inline
#else
#include "common.h"
#define SPX_MES_FN __device__ __forceinline__
#endif

#define SPX_MES_ERFC_UNDERFLOW (-37.5)
#define SPX_MES_SERIES_BELOW (-12.0)
#define SPX_MES_HALF_LOG_2PI 0.91893853320467274178
#define SPX_MES_SQRT_2PI 2.50662827463100050242
#define SPX_MES_RSQRT2 0.70710678118654752440

// Q(t) = sum_{k=1..14} (-1)^k (2k-1)!! t^(k-1)
SPX_MES_FN double mes_tail_q(double t)
{
#pragma clang fp contract(off)
    double q = 213458046676875.0;
    q = q * t - 7905853580625.0;
    q = q * t + 316234143225.0;
    q = q * t - 13749310575.0;
    q = q * t + 654729075.0;
    q = q * t - 34459425.0;
    q = q * t + 2027025.0;
    q = q * t - 135135.0;
    q = q * t + 10395.0;
    q = q * t - 945.0;
    q = q * t + 105.0;
    q = q * t - 15.0;
    q = q * t + 3.0;
    q = q * t - 1.0;
    return q;
}

// W(t) = sum_{m=0..12} (-1)^m (2m+2) (2m+1)!! t^m
SPX_MES_FN double mes_tail_w(double t)
{
#pragma clang fp contract(off)
    double w = 205552193096250.0;
    w = w * t - 7589619437400.0;
    w = w * t + 302484832650.0;
    w = w * t - 13094581500.0;
    w = w * t + 620269650.0;
    w = w * t - 32432400.0;
    w = w * t + 1891890.0;
    w = w * t - 124740.0;
    w = w * t + 9450.0;
    w = w * t - 840.0;
    w = w * t + 90.0;
    w = w * t - 12.0;
    w = w * t + 2.0;
    return w;
}

// log Phi(a) with relative accuracy for every finite a
SPX_MES_FN double mes_log_ndtr(double a)
{
#pragma clang fp contract(off)
    if (a < SPX_MES_ERFC_UNDERFLOW) {
        const double t = 1.0 / (a * a);
        const double q = mes_tail_q(t);
        return ((-(a * a) / 2.0 - log(-a)) - SPX_MES_HALF_LOG_2PI) + log1p(q * t);
    }
    const double p = 0.5 * erfc(fabs(a) * SPX_MES_RSQRT2);
    return a >= 0.0 ? log1p(-p) : log(p);
}

// h(g), and with GRAD its derivative.  g >= 38.6: phi and 0.5 erfc are zero, h = 0 - log1p(-0) = +0.0, never negative
// (-log Phi >= 0 and g phi / 2 >= 0 for g >= 0).  NaN in, NaN out.
template <bool GRAD>
SPX_MES_FN void mes_h_terms(double g, double& h, double& hp)
{
#pragma clang fp contract(off)
    if (g < SPX_MES_SERIES_BELOW) {
        const double t = 1.0 / (g * g);
        const double q = mes_tail_q(t);
        const double e = q * t;
        const double s = 1.0 + e;
        h = ((q / (2.0 * s) + SPX_MES_HALF_LOG_2PI) + log(-g)) - log1p(e);
        if (GRAD) hp = mes_tail_w(t) / ((2.0 * g) * (s * s));
        return;
    }
    const double p = 0.5 * erfc(fabs(g) * SPX_MES_RSQRT2);
    const double cdf = g >= 0.0 ? 1.0 - p : p;
    const double lcdf = g >= 0.0 ? log1p(-p) : log(p);
    const double pdf = exp(-(g * g) / 2.0) / SPX_MES_SQRT_2PI;
    const double r = pdf / cdf;
    h = (g * r) / 2.0 - lcdf;
    if (GRAD) hp = -(r / 2.0) * ((1.0 + g * g) + g * r);
}

#ifndef SPX_MES_HOST
// ---- shared by the kernels of the plain pass (mes_kernels.hip) and of the pass over fantasies (mes_fant_kernels.hip) ----
SPX_MES_FN bool mes_valid(double mu, double v) { return isfinite(mu) && v > 0.0 && isfinite(v); }

// s += x, compensated
SPX_MES_FN void mes_add(double& s, double& comp, double x)
{
#pragma clang fp contract(off)
    const double t = s + x;
    if (fabs(s) >= fabs(x)) comp += (s - t) + x;
    else comp += (x - t) + s;
    s = t;
}

// One fit record by one workgroup of 256 threads, from its bracket and its partial sums part [nb][J]: G_j = the partial sums in
// block order, the quartiles of the minimum by linear interpolation of G on the probe grid, the reflected-Gumbel fit, K levels
// y*_k = min(a + b w_k, cap).  fit = {lo, hi, y25, y50, y75, a, b, cap}.  sg [J], sh_q [3], sh_ab [3]: LDS of the caller.
SPX_MES_FN void mes_fit_record(double lo, double hi, bool any_valid, const double* __restrict__ part, int nb, int J, int K,
                               double noise, double best, double* __restrict__ G, double* __restrict__ ystar,
                               double* __restrict__ fit, double* sg, double* sh_q, double* sh_ab)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x;
    for (int j = tid; j < J; j += 256) {
        double s = 0.0, comp = 0.0;
        for (int b = 0; b < nb; ++b) mes_add(s, comp, part[(size_t)b * J + j]);
        const double g = any_valid ? s + comp : __builtin_nan("");
        G[j] = g;
        sg[j] = g;
    }
    __syncthreads();
    const double step = (hi - lo) / (double)(J - 1);
    if (tid < 3) {
        // t_p = log(1 - p) for p = 0.25, 0.5, 0.75
        const double tp = tid == 0 ? -0.2876820724517809 : tid == 1 ? -0.6931471805599453 : -1.3862943611198906;
        int j = 0;
        while (j < J && !(sg[j] <= tp)) ++j;
        double yp = __builtin_nan("");
        if (j > 0 && j < J) {
            const double y0 = lo + (double)(j - 1) * step, y1 = lo + (double)j * step;
            const double g0 = sg[j - 1], g1 = sg[j];
            yp = y0 + (y1 - y0) * (g0 - tp) / (g0 - g1);
        }
        sh_q[tid] = yp;
    }
    __syncthreads();
    if (tid == 0) {
        const double bb = (sh_q[2] - sh_q[0]) / 1.5725335836855194;     // log(log 4) - log(log(4/3))
        const double aa = sh_q[1] - bb * -0.36651292058166435;          // log(log 2)
        const double c5 = 5.0 * sqrt(noise);
        const double cap = best - c5;
        sh_ab[0] = aa; sh_ab[1] = bb; sh_ab[2] = cap;
        fit[0] = lo; fit[1] = hi; fit[2] = sh_q[0]; fit[3] = sh_q[1]; fit[4] = sh_q[2]; fit[5] = aa; fit[6] = bb; fit[7] = cap;
    }
    __syncthreads();
    const double aa = sh_ab[0], bb = sh_ab[1], cap = sh_ab[2];
    for (int k = tid; k < K; k += 256) {
        const double u = ((double)k + 0.5) / (double)K;
        const double w = log(-log1p(-u));
        const double bw = bb * w;
        double y = aa + bw;
        y = (y < cap || y != y) ? y : cap;          // np.minimum: NaN on either side stays
        ystar[k] = y;
    }
}
#endif
