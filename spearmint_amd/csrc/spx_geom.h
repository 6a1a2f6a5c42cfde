// Geometry shared by host and device code: plain C++, no HIP (common.h and spx_plan.h include it).
#pragma once
#include <stdint.h>

#define SPX_NB 64        // Cholesky / inverse block size
#define SPX_BM 128       // predict GEMM: rows (observations) per workgroup tile
#define SPX_BN 128       // predict GEMM: candidates per workgroup tile
#define SPX_BK 16        // predict GEMM: contraction depth per LDS stage
#define SPX_PADN 128     // observations are padded to a multiple of this

// device hyper table row: [mean, noise, amp2, amp2*(1+1e-6)]
#define SPX_HT 4

static inline int64_t round_up(int64_t x, int64_t m) { return (x + m - 1) / m * m; }

static inline int padded_dim(int D)
{
    if (D <= 4) return 4;
    if (D <= 8) return 8;
    if (D <= 16) return 16;
    return (int)round_up(D, 32);
}
