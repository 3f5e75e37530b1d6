// What the device-side updates of an exact GP share (gp_append.hip, gp_drop.hip, gp_refactor.hip; the
// slot mapping also serves gpmpc_set_gp's host loop): the MFMA tile pack of the mean rows, the 16 x 16
// Gram loop, Cholesky factor and triangular inverse, the RBF value of a raw row difference and the
// launch check.  sqp_kernel.hip (gp_tiles) reads the pack; it does not include this file.
#pragma once
#include "gpmpc_common.h"

namespace gpmpc {

typedef double f64x4 __attribute__((ext_vector_type(4)));

// Launches and leaves the calling launcher with the error, if any
#define GP_LAUNCH(kernel, grid, block, stream, ...)                        \
    do {                                                                   \
        hipLaunchKernelGGL(kernel, grid, block, 0, stream, __VA_ARGS__);   \
        const hipError_t e_ = hipGetLastError();                           \
        if (e_ != hipSuccess) return e_;                                   \
    } while (0)

// Tile pack.  Row i of the GP lies in tile t = i / 16, slot rr = i % 16.  tX[t][rr][4] is the row
// [inv_ell2 xc, c |xc|^2] (xc the input centred on GPDev::xbar, c = -inv_ell2 / 2).  tW[t] follows the
// MFMA C/D rows: register q of lane group grp holds row grp + 4q, so the row's entries
// {al, al xc} are tW[t][(4 grp + j) * 4 + q], j = 0 .. 3, with grp = rr % 4, q = rr / 4.
struct TileSlot {
    int t, rr, grp, q;
};
__host__ __device__ inline TileSlot tile_slot(int t, int rr) { return TileSlot{t, rr, rr % 4, rr / 4}; }
__host__ __device__ inline TileSlot tile_slot(int i) { return tile_slot(i / 16, i % 16); }
__host__ __device__ inline size_t tile_x_at(const TileSlot& s) { return (size_t)s.t * 64 + s.rr * 4; }
__host__ __device__ inline size_t tile_w_at(const TileSlot& s, int j) { return (size_t)s.t * 64 + (s.grp * 4 + j) * 4 + s.q; }

// xc = x - xbar in the GP's d dimensions, zero in the others (and everywhere for a row that is not live)
__device__ __forceinline__ void tile_centre(double (&xc)[3], double x0, double x1, double x2, const double (&xbar)[3],
                                            int d, bool live = true) {
    const double x[3] = {x0, x1, x2};
#pragma unroll
    for (int k = 0; k < 3; ++k) xc[k] = (k < d && live) ? x[k] - xbar[k] : 0.0;
}

// The row's tX entries (live = false: a row with xc = 0 whose last entry is +0, not c * 0)
__device__ __forceinline__ void tile_write_x(double* tX, const TileSlot& s, const double (&xc)[3], double inv_ell2,
                                             double c, bool live = true) {
    double sq = 0.0;
#pragma unroll
    for (int k = 0; k < 3; ++k) sq += xc[k] * xc[k];
    double* tx = tX + tile_x_at(s);
#pragma unroll
    for (int k = 0; k < 3; ++k) tx[k] = inv_ell2 * xc[k];
    tx[3] = live ? c * sq : 0.0;
}

// The row's tW entries (live = false: exact zeros)
__device__ __forceinline__ void tile_write_w(double* tW, const TileSlot& s, double al, const double (&xc)[3],
                                             bool live = true) {
    const double wv[4] = {al, al * xc[0], al * xc[1], al * xc[2]};
#pragma unroll
    for (int j = 0; j < 4; ++j) tW[tile_w_at(s, j)] = live ? wv[j] : 0.0;
}

// k(x, x') from the raw row difference (d0, d1, d2), c = -inv_ell2 / 2
__device__ __forceinline__ double rbf_raw(double c, double sf2, double d0, double d1, double d2) {
    return sf2 * exp_rbf(c * fma(d0, d0, fma(d1, d1, d2 * d2)));
}

// Gram matrix of 16 rows over 16 * tiles columns, one wave: `row` is lane (lc, kq)'s row lc at column
// 4 kq, of which it takes columns 16s + 4kq + j (both MFMA operands are one register, so the K order is
// free); a lane that is not live contributes a zero row.  Four accumulators added in a fixed order:
// entry r of the result is G[kq + 4r][lc].
__device__ __forceinline__ f64x4 gram16(const double* row, int tiles, bool live = true) {
    f64x4 g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < tiles; ++s, row += 16) {
        double4 w = *reinterpret_cast<const double4*>(row);
        if (!live) w = double4{0.0, 0.0, 0.0, 0.0};
        g[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.x, w.x, g[0], 0, 0, 0);
        g[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.y, w.y, g[1], 0, 0, 0);
        g[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.z, w.z, g[2], 0, 0, 0);
        g[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(w.w, w.w, g[3], 0, 0, 0);
    }
    f64x4 sum;
#pragma unroll
    for (int r = 0; r < 4; ++r) sum[r] = (g[0][r] + g[1][r]) + (g[2][r] + g[3][r]);
    return sum;
}

// Cholesky factor of the 16 x 16 matrix S in place (lower triangle), thread = row; every thread of the
// workgroup calls it, after a barrier that follows the last write to S.  Returns whether every pivot
// was finite and positive (the same value in every thread); a bad pivot is replaced by 1.  The pivot
// reaches the other threads through LDS (tmp: one double), or, in a workgroup of one wave (kOneWave,
// tmp unused), by __shfl: the same arithmetic with one barrier per column less.
template <bool kOneWave = false>
__device__ inline bool chol16(double (*S)[17], double* tmp, int tid) {
    bool ok = true;
    for (int j = 0; j < 16; ++j) {
        double s = 0.0;
        if (tid < 16 && tid >= j) {
            s = S[tid][j];
            for (int k = 0; k < j; ++k) s = fma(-S[tid][k], S[j][k], s);
            if (!kOneWave && tid == j) tmp[0] = s;
        }
        double piv;
        if (kOneWave) {
            piv = __shfl(s, j);
        } else {
            __syncthreads();
            piv = tmp[0];
        }
        const bool good = isfinite(piv) && piv > 0.0;
        ok = ok && good;
        const double ljj = good ? sqrt(piv) : 1.0;
        if (tid < 16 && tid >= j) S[tid][j] = (tid == j) ? ljj : s / ljj;
        __syncthreads();
    }
    return ok;
}

// Inverse of the lower-triangular 16 x 16 matrix S into Li (zero above the diagonal on entry),
// thread = column
__device__ inline void inv_lower16(double (*S)[17], double (*Li)[17], int tid) {
    if (tid < 16) {
        for (int i = tid; i < 16; ++i) {
            double s = (i == tid) ? 1.0 : 0.0;
            for (int k = tid; k < i; ++k) s = fma(-S[i][k], Li[k][tid], s);
            Li[i][tid] = s / S[i][i];
        }
    }
}

}  // namespace gpmpc
