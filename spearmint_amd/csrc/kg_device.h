// Knowledge gradient of one (draw, candidate) from its n = A + 1 lines (spx.h SPX_ACQ_KG): line i is mu_i + b_i Z with Z ~ N(0, 1),
// and
//     KG = min_i mu_i - E_Z[min_i (mu_i + b_i Z)] = sum_k (b_k - b_{k+1}) f(-|z_k|),     f(z) = phi(z) + z Phi(z),
// over the lines on the lower envelope in order of falling slope, z_k the breakpoint between the k-th and the next (Frazier,
// Powell & Dayanik 2009).  Every term is >= 0, so nothing cancels.  f(-|z|) is ei_dev(0, 1, -|z|): the EI formula of every pass
// at unit sigma, with its arithmetic and its tail.
//
// How the envelope is found: the sort-free all-pairs form, two sweeps over the lines, each line looked at on its own.
//   sweep 1  kg_on_envelope(i): with z_ij = (mu_j - mu_i) / (b_i - b_j) for b_j < b_i -- ONE expression for a pair, whichever of
//            the two asks, so both see the same bits -- line i is the minimum on [lo_i, hi_i], lo_i = max over the steeper
//            lines of z_ji, hi_i = min over the flatter ones of z_ij.  It is ON the envelope when lo_i < hi_i (strictly: a line that
//            only touches the envelope in a point is off) and no line of the SAME slope beats it.
//            Tie rule: among lines of equal slope the lowest intercept stays, and among equal lines (duplicates) the lowest index.
//   sweep 2  kg_term(i): the successor of an envelope line is the envelope line of the largest slope below its own (after sweep 1
//            no two envelope lines share a slope); its term is (b_i - b_next) f(-|z_i,next|), +0.0 for the last line and for every line
//            off the envelope.
// The value is the sum of the terms in the order of the lines (line 0 = the candidate, then the representer points as given),
// from +0.0: it depends on the lines and their order alone.  All slopes equal: no line has a flatter one, every term is +0.0 and
// so is the sum, exactly.  f is clamped at +0.0 from below (beyond |z| = 37.5 its two denormal halves may round to a negative
// sum, and at |z| = inf ei_dev is 0 x inf), so no term and no value is negative.  A rounding error in a breakpoint can put a line
// that touches the envelope within that error on or off it; the chain over the lines kept is complete either way, and the value
// moves by that rounding of the breakpoint, not by a term.
// Non-finite mu or slope among the lines: the caller's business (k_kg_value writes NaN); the functions here expect finite lines.
// Cost: n divisions per line in sweep 1, n comparisons per line in sweep 2, one f per envelope line.
// SPX_KG_HOST: the same text compiled for the host (tests/c/kg_client.cpp, built with -ffp-contract=off).
#pragma once
#ifdef SPX_KG_HOST
#include <cmath>
#define __device__
#define __forceinline__ inline
#define SPX_EHVI_HOST       // (ei_device.h: the host build brings what it needs of common.h itself)
#define SPX_ACQ_DEV_EI 0
#define SPX_ACQ_DEV_PI 1
#define SPX_ACQ_DEV_LCB 2
#endif
#include "ei_device.h"

#define SPX_KG_INF __builtin_inf()

// f(-|z|) >= +0.0
__device__ __forceinline__ double kg_f(double z)
{
#pragma clang fp contract(off)
    const double v = ei_dev(0.0, 1.0, -fabs(z));
    return v > 0.0 ? v : 0.0;
}

// Lines: intercept a0 for line 0 and a[j] for j >= 1 (a[0] is not read), slope b[j * bs].
__device__ __forceinline__ bool kg_on_envelope(double a0, const double* a, const double* b, int bs, int n, int i)
{
#pragma clang fp contract(off)
    const double ai = i ? a[i] : a0, bi = b[(size_t)i * bs];
    double lo = -SPX_KG_INF, hi = SPX_KG_INF;
    bool beaten = false;
    for (int j = 0; j < n; ++j) {
        const double aj = j ? a[j] : a0, bj = b[(size_t)j * bs];
        // ONE division per pair, whatever the order of the slopes: for b_j > b_i it is z_ji = (mu_i - mu_j) / (b_j - b_i) with both
        // signs turned, the same bits.  Lanes of a wave own different lines, so a division per branch would be issued twice.
        // (b_j == b_i: inf or NaN, used by neither select)
        const double z = (aj - ai) / (bi - bj);
        lo = (bj > bi && z > lo) ? z : lo;
        hi = (bj < bi && z < hi) ? z : hi;
        beaten = beaten || (bj == bi && (aj < ai || (aj == ai && j < i)));
    }
    return !beaten && lo < hi;
}

// on[j * os] != 0: line j is on the envelope (sweep 1); line i must be.
__device__ __forceinline__ double kg_term(double a0, const double* a, const double* b, int bs, const unsigned char* on, int os, int n, int i)
{
#pragma clang fp contract(off)
    const double ai = i ? a[i] : a0, bi = b[(size_t)i * bs];
    double an = 0.0, bn = -SPX_KG_INF;
    for (int j = 0; j < n; ++j) {
        const double bj = b[(size_t)j * bs];
        if (on[(size_t)j * os] && bj < bi && bj > bn) {
            bn = bj;
            an = j ? a[j] : a0;
        }
    }
    if (bn == -SPX_KG_INF) return 0.0;
    const double db = bi - bn;
    return db * kg_f((an - ai) / db);
}
