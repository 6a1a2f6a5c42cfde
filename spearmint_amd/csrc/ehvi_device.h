// Expected hypervolume improvement of one (draw, candidate) over two independent Gaussian predictions, both objectives
// minimised (spx.h SPX_ACQ_EHVI).  The front has n points a_1 < ... < a_n, b_1 > ... > b_n and a reference point (r1, r2);
// with a_0 = -inf, a_{n+1} = r1, b_0 = r2 it cuts the region that a new point can still dominate into n + 1 vertical strips,
// strip i between a_i and a_{i+1} and below b_i:
//     EHVI = sum_{i=0..n} [G1(a_{i+1}) - G1(a_i)] G2(b_i),   G_k(y) = E[(y - f_k)+] = ei_dev(m_k, v_k, best = y),   G1(a_0) := +0.0
// The caller hands the strips over as two arrays of n + 1 doubles, possibly tile by tile: edges[i] = a_{i+1} (the last one r1)
// and levels[i] = b_i (the first one r2).  Summed sequentially in i; G1 of an edge is evaluated once and carried into the next
// strip as its lower edge; every strip is evaluated (none is skipped: a strip whose term is zero adds its zero); nothing may
// contract into an fma.  The first strip ASSIGNS its product, so that n = 0 is G1(r1) G2(r2) to the bit, the sign of a zero
// included.  func_v < 0 in either GP: ei_dev is NaN and so is the sum.  tests/ehvi_oracle.py restates this operation for
// operation.
// SPX_EHVI_HOST: the same text compiled for the host (tests/c/ehvi_client.cpp, built with -ffp-contract=off); on the device only
// erf, erfc, exp and sqrt come from another library.
#pragma once
#ifdef SPX_EHVI_HOST
#include <cmath>
#define __device__
#define __forceinline__ inline
#define SPX_ACQ_DEV_EI 0
#define SPX_ACQ_DEV_PI 1
#define SPX_ACQ_DEV_LCB 2
#endif
#include "ei_device.h"

// strips [0, cnt) of a tile; first: the tile starts at strip 0 of the front.  g_lo: G1 of the lower edge (in: of the tile's
// first strip, out: of the strip behind its last); acc: the sum so far
__device__ __forceinline__ void ehvi_strips(double m1, double v1, double m2, double v2, const double* edges, const double* levels,
                                            int cnt, bool first, double& g_lo, double& acc)
{
#pragma clang fp contract(off)
    for (int i = 0; i < cnt; ++i) {
        const double g_hi = ei_dev(m1, v1, edges[i]);
        const double g2 = ei_dev(m2, v2, levels[i]);
        const double term = (g_hi - g_lo) * g2;
        acc = (first && i == 0) ? term : acc + term;
        g_lo = g_hi;
    }
}
