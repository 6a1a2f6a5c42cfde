// The two device-side ends of spx_main_effects (spx_api.hip): the structured rows a grid pass scores, and the reduction of the
// pass's kept predictive means into the main-effect curves.  Everything between them is the ordinary EI pass.
//
// Rows (spx.h).  With nb = D T blocks of Q rows: row r = (j T + k) Q + q is base[q] with coordinate j replaced by levels[k];
// the last Q rows, r = nb Q + q, are base[q] itself.
//
// k_effects_rows   one thread per ELEMENT of the row-major candidate buffer, element-fastest: consecutive lanes store
//                  consecutive doubles, so every store instruction of a wave writes 512 contiguous bytes.  base (Q D doubles)
//                  and levels (T) are read through L2: the kernel is a pure write stream of rows x D x 8 bytes.  D = 1: every
//                  element is its row's only coordinate, the same index arithmetic.
// k_effects_mean   curves[d][b] = np.mean(func_m_d[b Q .. (b + 1) Q)): numpy's pairwise sum (np_sum.h, non-recursive) and one
//                  true division by Q.  The order of the additions is fixed by numpy, so one lane walks one block; lanes that
//                  did so straight from memory would sit Q x 8 bytes apart.  Instead a workgroup copies `G` whole blocks --
//                  one contiguous range of the draw's row -- into LDS with coalesced loads, at a row stride of Q | 1 doubles
//                  (odd: the lanes' walks start in different banks), and lane g < G walks block g there.  A block longer than
//                  the tile (Q > 6143) is walked from memory (LDS = false).  Workgroups behind the reduction's copy the draw's
//                  last Q means into base_mean.
#include "common.h"
#include "np_sum.h"
#include "spx_plan.h"

__global__ __launch_bounds__(SPX_EFFECTS_THREADS) void k_effects_rows(const double* __restrict__ base,
                                                                      const double* __restrict__ levels, int D, int T, int Q,
                                                                      int64_t r0, int64_t m, double* __restrict__ out)
{
    const int64_t total = m * D;                        // elements of this pass: rows [r0, r0 + m)
    const int64_t nb = (int64_t)D * T;                  // blocks with a substituted coordinate
    const int64_t stride = (int64_t)gridDim.x * SPX_EFFECTS_THREADS;
    for (int64_t e = (int64_t)blockIdx.x * SPX_EFFECTS_THREADS + threadIdx.x; e < total; e += stride) {
        const int64_t rl = e / D;
        const int c = (int)(e - rl * D);
        const int64_t r = r0 + rl;
        const int64_t b = r / Q;
        const int q = (int)(r - b * Q);
        double v = base[(size_t)q * D + c];
        if (b < nb) {
            const int j = (int)(b / T);
            if (c == j) v = levels[b - (int64_t)j * T];
        }
        out[e] = v;
    }
}

template <bool LDS>
__global__ __launch_bounds__(SPX_EFFECTS_THREADS) void k_effects_mean(const double* __restrict__ mean, int64_t mstride,
                                                                      int64_t nb, int Q, int G, int64_t ntiles,
                                                                      double* __restrict__ curves,
                                                                      double* __restrict__ base_mean)
{
    extern __shared__ double tile[];
    const int d = blockIdx.y;
    const double* row = mean + (size_t)d * mstride;
    if ((int64_t)blockIdx.x >= ntiles) {                // base_mean[d][q] = func_m_d(nb Q + q)
        const int64_t q = ((int64_t)blockIdx.x - ntiles) * SPX_EFFECTS_THREADS + threadIdx.x;
        if (base_mean && q < Q) base_mean[(size_t)d * Q + q] = row[nb * Q + q];
        return;
    }
    const int64_t b0 = (int64_t)blockIdx.x * G;
    const int gn = (int)((nb - b0 < G) ? (nb - b0) : G);     // blocks of this workgroup (uniform)
    const int g = threadIdx.x;
    const double* src;
    if (LDS) {
        const int ldq = Q | 1;
        const int en = gn * Q;                          // <= SPX_EFFECTS_LDS_BYTES / 8
        const double* from = row + b0 * Q;
        for (int e = threadIdx.x; e < en; e += SPX_EFFECTS_THREADS) {
            const int eg = e / Q;
            tile[eg * ldq + (e - eg * Q)] = from[e];
        }
        __syncthreads();
        src = tile + g * ldq;
    } else {
        src = row + (b0 + g) * Q;
    }
    // (0.0 + ...: np.add.reduce starts from the identity, as the mean over draws does in predict_kernels.hip)
    if (g < gn) curves[(size_t)d * nb + b0 + g] = (0.0 + np_pairwise(src, 1, Q)) / (double)Q;
}

void launch_effects_rows(hipStream_t s, const double* base, const double* levels, int D, int T, int Q, int64_t r0, int64_t m,
                         double* out)
{
    int64_t blocks = (m * D + SPX_EFFECTS_THREADS - 1) / SPX_EFFECTS_THREADS;
    if (blocks < 1) blocks = 1;
    if (blocks > (1 << 20)) blocks = 1 << 20;
    hipLaunchKernelGGL(k_effects_rows, dim3((unsigned)blocks), dim3(SPX_EFFECTS_THREADS), 0, s, base, levels, D, T, Q, r0, m, out);
}

void launch_effects_mean(hipStream_t s, const EffectsPlan& p, const double* mean, int64_t mstride, int Q, int H, double* curves,
                         double* base_mean)
{
    const unsigned gx = (unsigned)(p.mean_tiles + p.gather_tiles);
    for (int h0 = 0; h0 < H; h0 += 65535) {             // (grid.y)
        const int nh = H - h0 < 65535 ? H - h0 : 65535;
        const double* mh = mean + (size_t)h0 * mstride;
        double* ch = curves + (size_t)h0 * p.nblocks;
        double* bh = base_mean ? base_mean + (size_t)h0 * Q : nullptr;
        if (p.mean_lds)
            hipLaunchKernelGGL(k_effects_mean<true>, dim3(gx, nh), dim3(SPX_EFFECTS_THREADS), p.lds_bytes, s, mh, mstride,
                               p.nblocks, Q, p.wg_blocks, p.mean_tiles, ch, bh);
        else
            hipLaunchKernelGGL(k_effects_mean<false>, dim3(gx, nh), dim3(SPX_EFFECTS_THREADS), 0, s, mh, mstride, p.nblocks, Q,
                               p.wg_blocks, p.mean_tiles, ch, bh);
    }
}
