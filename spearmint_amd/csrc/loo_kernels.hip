// The device side of spx_loo (spx_api.hip): leave-one-out cross-validation of the resident factorisation without a refit
// (Rasmussen & Williams 5.4.2).  With c_j = (K^-1)_jj and alpha = K^-1 (y - mean):
//     loo_mean_j = y_j - alpha_j / c_j        loo_var_j = 1 / c_j
// K^-1 = W^T W with W = L^-1, so c_j = sum_k W[k][j]^2 = the squared norm of row j of WT ([model][Np][Np], row-major, row j
// holds W[k][j] for k >= j): a sum of non-negative terms, no cancellation.
//
// k_loo_diag   one wavefront per row j < N of one model, walked as k_alpha (chol_kernels.hip) walks it: lane l starts at the
//              64-aligned column (j & ~63) + l and strides by 64, entries left of the diagonal are masked (they are another
//              tile's business, not zeros to rely on).  Every load instruction of a wave reads 512 contiguous bytes.  Each lane
//              adds its squares in column order -- one fma per entry, four loads in flight, the chain itself in order -- and the
//              64 partial sums meet in the xor butterfly 32, 16, ... 1.  The order therefore depends on j and Np alone: not on
//              the grid, not on H, not on which draw of how many the row belongs to.  Pad columns (>= N) of a row j < N are
//              exact zeros in WT and are included.  8-byte loads: a row's live part starts at an arbitrary 64-aligned column and
//              the lane <-> column map above is the contract; the kernel is a pure read stream at 8+ waves per SIMD, which
//              hides the narrower load.
//              The three results: c, then 1 / c and y_j - alpha_j / c as IEEE operations in that order (__ddiv_rn, __dsub_rn:
//              nothing for the compiler to contract or reassociate).
#include "common.h"

__global__ __launch_bounds__(256) void k_loo_diag(const double* __restrict__ WT, const double* __restrict__ alpha,
                                                  const double* __restrict__ y, int N, int Np,
                                                  double* __restrict__ loo_mean, double* __restrict__ loo_var,
                                                  double* __restrict__ kinv_diag)
{
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int h = blockIdx.y;
    const int j = blockIdx.x * 4 + wave;
    if (j >= N) return;                                 // (wave-uniform: no shuffle below is left without its partners)
    const double* row = WT + ((size_t)h * Np + j) * Np;
    double acc = 0.0;
    int i = (j & ~63) + lane;
    for (; i + 192 < Np; i += 256) {                    // Np is a multiple of 64: the bound is the same for all lanes
        const double w0 = row[i], w1 = row[i + 64], w2 = row[i + 128], w3 = row[i + 192];
        const double v0 = i >= j ? w0 : 0.0;            // (only the first 64 columns can lie left of the diagonal)
        acc = fma(v0, v0, acc);
        acc = fma(w1, w1, acc);
        acc = fma(w2, w2, acc);
        acc = fma(w3, w3, acc);
    }
    for (; i < Np; i += 64) {
        const double v = i >= j ? row[i] : 0.0;
        acc = fma(v, v, acc);
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_xor(acc, off);
    if (lane == 0) {
        const size_t o = (size_t)h * N + j;
        kinv_diag[o] = acc;
        loo_var[o] = __ddiv_rn(1.0, acc);
        loo_mean[o] = __dsub_rn(y[j], __ddiv_rn(alpha[(size_t)h * Np + j], acc));
    }
}

// WT, alpha: the first of nh draws of ONE model; y [N]: that model's observed values; the outputs [nh][N]
void launch_loo_diag(hipStream_t s, const double* WT, const double* alpha, const double* y, int N, int Np, int nh,
                     double* loo_mean, double* loo_var, double* kinv_diag)
{
    for (int h0 = 0; h0 < nh; h0 += 65535) {            // (grid.y)
        const int n = nh - h0 < 65535 ? nh - h0 : 65535;
        hipLaunchKernelGGL(k_loo_diag, dim3((N + 3) / 4, n), dim3(256), 0, s, WT + (size_t)h0 * Np * Np, alpha + (size_t)h0 * Np, y,
                           N, Np, loo_mean + (size_t)h0 * N, loo_var + (size_t)h0 * N, kinv_diag + (size_t)h0 * N);
    }
}
