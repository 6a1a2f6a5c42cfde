// Device helper of the Thompson-sampling prior (spx.h: spx_thompson; ts_kernels.hip: k_ts_prior): cos(2 pi r) of a phase r
// given in TURNS and already reduced to [-1/2, 1/2], on W values in lock step -- the style of cov_device.h: every stage is a
// loop over W, no special-case selects, no table, no scratch.
//
//   t = 1/4 - |r|                  cos(2 pi r) = sin(2 pi t), |t| <= 1/4.  For |r| >= 1/8 the subtraction is exact (Sterbenz);
//                                  below, t in (1/8, 1/4] is rounded once: at most 2^-55 absolute, times the slope 2 pi cos(2 pi t)
//                                  <= 4.45 where the result is >= 0.707: at most 1.12 ulp of the result
//   s = t t                        one rounding; the polynomial's sensitivity to it, |s P'(s) / P(s)| = |x cot x - 1| / 2 with
//                                  x = 2 pi t, is at most 1/2 on |x| <= pi / 2: 0.25 ulp
//   P(s) = sum_k c_k s^k           c_k = (-1)^k (2 pi)^(2k+1) / (2k+1)!, k = 0 .. 10, each rounded to nearest from 60 digits;
//                                  Horner, one fma per coefficient.  The first term left out, c_11 s^11 <= 8.9e-5 / 16^11 =
//                                  5.0e-18 against P >= 4: 0.012 ulp.  The steps' roundings (half an ulp of an intermediate that
//                                  is at most 2 pi / 4 of the result, damped by s c_{k+1} / c_k <= 0.42 per step) and those of
//                                  the coefficients: at most 0.5 (1.58 / (1 - 0.42)) + 0.5 < 1.9 ulp
//   out = t P                      one rounding: 0.5 ulp
// A relative error of e 2^-53 is at most e ulp of the result, so the budget of this header is
//   SPX_TS_COS_ULPS = 4 ulp of the result (1.12 + 0.25 + 0.012 + 1.9 + 0.5 = 3.8),
// relative all the way down: the zeros of the cosine sit at r = +-1/4, where t = 0 is exact and the result is an odd
// polynomial in t, so a result near zero keeps its relative accuracy (denormal |t| does not occur: t is a multiple of 2^-55).
// tests/test_ts_host.py compiles this text for the host (SPX_TS_HOST, tests/c/ts_client.cpp, no contraction) and holds it to a
// 50-digit reference at that budget; README.md has the measured worst case.
// NaN r gives NaN (every operation propagates it); the caller forms r = u - rint(u), which is NaN for a NaN or infinite u and
// exactly 0 for |u| >= 2^52.
// FMA-unit instructions per value: 1 (t; |r| is an input modifier) + 1 (s) + 10 (Horner) + 1 (out) = 13 (the gfx950 listing of
// k_ts_prior agrees: ts_kernels.hip has the count of the whole loop and the bound that follows from it).
//
// sin2pi(r) = sin(2 pi r) of the same reduced phase, for the gradient of a path (spx.h: spx_thompson_grad_batch;
// ts_grad_kernels.hip), in the same style and with the same polynomial:
//   t = min(|r|, 1/2 - |r|)        sin(2 pi |r|) = sin(2 pi t), 0 <= t <= 1/4.  The minimum selects the difference for |r| >= 1/4
//                                  only, where it is exact (Sterbenz: 1/4 <= |r| <= 1/2): t carries NO rounding
//   s = t t,  P(s),  t P           as above;  out = copysign(t P, r): sin2pi(+-0) = +-0 and sin2pi(+-1/2) = +-0 (t = 0)
// The budget, in units of u = 2^-53 relative, each of which is at most one ulp of the result; every term below grows with t and
// is taken at t = 1/4 (s = 1/16, P = 4):
//   s rounded once (u), times the sensitivity 1/2                                                                    0.5
//   the term left out, c_11 s^11 / P                                                                                 0.012
//   Horner: the last fma rounds P itself (1); the one before it rounds p_1 with |p_1| s = c_0 - P = 2.283, the earlier
//   ones p_k with |p_k| s^k <= |c_k| s^k = 0.319, 0.019, 0.001 (k = 2, 3, 4 ...): 1 + 2.622 / 4                      1.655
//   the coefficients: c_0 is 2 pi rounded, off by 0.351 u, weight c_0 / P = 1.571 (0.552); the others by at most u each,
//   weights |c_k| s^k / P = 0.646, 0.080, 0.005, ... (0.731)                                                         1.283
//   out = t P, one rounding: half an ulp of the result                                                               0.5
//   SPX_TS_SIN_ULPS = 4 ulp of the result (3.95): no more than the cosine's, which pays 1.12 for its rounded t.
// Unlike the cosine's t, |r| can be arbitrarily small (r = u whenever |u| < 1/2).  Down to the smallest normal result the bound
// is relative as above (s may underflow to 0: then P = c_0 exactly and the budget only shrinks).  Where the result is
// sub-normal no relative bound holds: t P is rounded to the quantum 2^-1074 and the result is within ONE quantum of the true
// value (half for the rounding, the relative terms above are below a hundredth of a quantum there).
// tests/test_ts_grad_host.py holds this text, compiled for the host (tests/c/ts_grad_client.cpp), to a 50-digit reference at
// that budget; README.md has the measured worst case.  NaN r gives NaN.  FMA-unit instructions per value: 1 (1/2 - |r|) + 1
// (min) + 1 (s) + 10 + 1 (t P); the sign is a bit operation.
#pragma once
#ifdef SPX_TS_HOST
#include <cmath>
#define SPX_TS_FN static inline
#else
#include "common.h"
#define SPX_TS_FN __device__ __forceinline__
#endif

#define SPX_TS_COS_ULPS 4
#define SPX_TS_SIN_ULPS 4
#define SPX_TS_TWO_PI 6.283185307179586   // == 2 * np.pi

template <int W>
SPX_TS_FN void cos2pi(const double (&r)[W], double (&out)[W])
{
#pragma clang fp contract(off)
    double t[W], s[W], p[W];
#pragma unroll
    for (int w = 0; w < W; ++w) t[w] = 0.25 - __builtin_fabs(r[w]);
#pragma unroll
    for (int w = 0; w < W; ++w) s[w] = t[w] * t[w];
#pragma unroll
    for (int w = 0; w < W; ++w) p[w] = __builtin_fma(0x1.2877020d52cf0p-10, s[w], -0x1.8a404211f9547p-7);   // c_10, c_9
#define SPX_TS_STEP(C_)                                   \
    _Pragma("unroll") for (int w = 0; w < W; ++w) p[w] = __builtin_fma(p[w], s[w], C_)
    SPX_TS_STEP(0x1.aaec32af93359p-4);     // c_8  =  (2 pi)^17 / 17!
    SPX_TS_STEP(-0x1.6fadb9f155744p-1);    // c_7  = -(2 pi)^15 / 15!
    SPX_TS_STEP(0x1.e8f434d018d63p+1);     // c_6  =  (2 pi)^13 / 13!
    SPX_TS_STEP(-0x1.e3074fde8871fp+3);    // c_5  = -(2 pi)^11 / 11!
    SPX_TS_STEP(0x1.50783487ee782p+5);     // c_4  =  (2 pi)^9 / 9!
    SPX_TS_STEP(-0x1.32d2cce62bd86p+6);    // c_3  = -(2 pi)^7 / 7!
    SPX_TS_STEP(0x1.466bc6775aae2p+6);     // c_2  =  (2 pi)^5 / 5!
    SPX_TS_STEP(-0x1.4abbce625be53p+5);    // c_1  = -(2 pi)^3 / 3!
    SPX_TS_STEP(0x1.921fb54442d18p+2);     // c_0  =  2 pi
#pragma unroll
    for (int w = 0; w < W; ++w) out[w] = t[w] * p[w];
}

template <int W>
SPX_TS_FN void sin2pi(const double (&r)[W], double (&out)[W])
{
#pragma clang fp contract(off)
    double t[W], s[W], p[W];
#pragma unroll
    for (int w = 0; w < W; ++w) {
        const double a = __builtin_fabs(r[w]);
        t[w] = __builtin_fmin(a, 0.5 - a);
    }
#pragma unroll
    for (int w = 0; w < W; ++w) s[w] = t[w] * t[w];
#pragma unroll
    for (int w = 0; w < W; ++w) p[w] = __builtin_fma(0x1.2877020d52cf0p-10, s[w], -0x1.8a404211f9547p-7);   // c_10, c_9
    SPX_TS_STEP(0x1.aaec32af93359p-4);
    SPX_TS_STEP(-0x1.6fadb9f155744p-1);
    SPX_TS_STEP(0x1.e8f434d018d63p+1);
    SPX_TS_STEP(-0x1.e3074fde8871fp+3);
    SPX_TS_STEP(0x1.50783487ee782p+5);
    SPX_TS_STEP(-0x1.32d2cce62bd86p+6);
    SPX_TS_STEP(0x1.466bc6775aae2p+6);
    SPX_TS_STEP(-0x1.4abbce625be53p+5);
    SPX_TS_STEP(0x1.921fb54442d18p+2);
#pragma unroll
    for (int w = 0; w < W; ++w) out[w] = __builtin_copysign(t[w] * p[w], r[w]);
}
#undef SPX_TS_STEP
