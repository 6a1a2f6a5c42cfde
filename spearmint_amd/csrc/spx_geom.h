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

// Max-value entropy search: candidates per partial log-survival sum / per partial minimum of the plain pass (mes_kernels.hip)
// and of the pass over fantasies (mes_fant_kernels.hip), and the block counts their tables are sized by (plan_ei, spx_plan.h)
#define MES_CT 512        // candidates per partial sum of k_mes_logsurv
#define MES_BT 1024       // candidates per partial minimum of k_mes_bounds
#define MESF_CT 512       // candidates per partial sum of k_mes_fant_logsurv (MES_CT of the plain pass)
#define MESF_BT 1024      // candidates per partial minimum of k_mes_fant_bounds

static inline int mes_sum_blocks(int64_t M) { return (int)((M + MES_CT - 1) / MES_CT); }
static inline int mes_bound_blocks(int64_t M) { return (int)((M + MES_BT - 1) / MES_BT); }
static inline int mes_fant_sum_blocks(int64_t M) { return (int)((M + MESF_CT - 1) / MESF_CT); }
static inline int mes_fant_bound_blocks(int64_t M) { return (int)((M + MESF_BT - 1) / MESF_BT); }
