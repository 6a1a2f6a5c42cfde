// Expected hypervolume improvement (spx.h SPX_ACQ_EHVI): the stage behind an ordinary grid pass that kept its moments, and
// behind the second GP's pass over the same candidates.  One thread per (draw, candidate); the strips of the front are the
// same for every thread, so a workgroup stages them through LDS EHVI_TILE at a time and every thread walks the tile in order
// (ehvi_device.h: sequential in i, G1 of an edge evaluated once).  Pointwise in the candidate: no reduction, no atomics.
#include "ehvi_device.h"

#define EHVI_TILE 256     // strips per LDS tile (2 x 2 KiB)

__global__ __launch_bounds__(256) void k_ehvi(const double* __restrict__ m1, const double* __restrict__ v1,
                                              const double* __restrict__ m2, const double* __restrict__ v2,
                                              const double* __restrict__ edges, const double* __restrict__ levels, int nstrips,
                                              int64_t M, int64_t Mp, double* __restrict__ ei_draw)
{
#pragma clang fp contract(off)
    __shared__ double s_edge[EHVI_TILE], s_level[EHVI_TILE];
    const int tid = threadIdx.x;
    const int64_t c = (int64_t)blockIdx.x * 256 + tid;
    const bool live = c < M;                                              // (a thread past M stays for the barriers and reads candidate 0)
    const size_t at = (size_t)blockIdx.y * (size_t)Mp + (size_t)(live ? c : 0);
    const double a_m = m1[at], a_v = v1[at], b_m = m2[at], b_v = v2[at];
    double g_lo = 0.0, acc = 0.0;
    for (int t0 = 0; t0 < nstrips; t0 += EHVI_TILE) {
        const int cnt = min(EHVI_TILE, nstrips - t0);
        __syncthreads();                                                  // the last tile has been read by every wave
        if (tid < cnt) { s_edge[tid] = edges[t0 + tid]; s_level[tid] = levels[t0 + tid]; }
        __syncthreads();
        ehvi_strips(a_m, a_v, b_m, b_v, s_edge, s_level, cnt, t0 == 0, g_lo, acc);
    }
    if (live) ei_draw[at] = acc;
}

void launch_ehvi(hipStream_t s, const double* m1, const double* v1, const double* m2, const double* v2, const double* edges,
                 const double* levels, int nstrips, int64_t M, int64_t Mp, int H, double* ei_draw)
{
    hipLaunchKernelGGL(k_ehvi, dim3((unsigned)((M + 255) / 256), H), dim3(256), 0, s, m1, v1, m2, v2, edges, levels, nstrips, M, Mp,
                       ei_draw);
}
