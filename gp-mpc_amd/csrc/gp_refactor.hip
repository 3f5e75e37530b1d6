// Refactorising an exact GP on the device (gpmpc_gp_refactor): a from-scratch factorisation of
// Khat = k(X, X) + sn2 I from the handle's own rows, the caller's device targets y and the
// hyperparameters passed in.  The result is what gpmpc_set_gp would have uploaded:
//
//   Khat = L L^T,  M = L^-1 (stored transposed, GPDev::linvT: row j of linvT is column j of M)
//   w = M y,  alpha = M^T w = Khat^-1 y
//
// in 16 x 16 tiles over the padded size npad = 16 nt.  A (the GP's spare factor buffer, stride npad,
// row-major) holds the lower tiles of Khat, then of L; the inverses L_kk^-1 of the diagonal tiles'
// factors go to scratch (dinv) and A_kk itself is left alone, so no workgroup reads a tile another
// one is writing.  Panel k (k = 0 .. nt-1) is two launches:
//
//   gp_refactor_panel_kernel   every wave factors A_kk in registers (lane = row, columns exchanged
//                              by v_readlane) and inverts L_kk from LDS; workgroup 0 stores
//                              L_kk^-1; then one wave per row tile i > k: L_ik = A_ik L_kk^-T on
//                              v_mfma_f64_16x16x4_f64, in place.
//   gp_refactor_update_kernel  one wave per tile (i, j), four per workgroup, k <= i, j <= i:
//       j > k          A_ij -= L_ik L_jk^T                    the right-looking SYRK
//       j <= k         the same step of the forward substitution L B = I, also right-looking:
//                      X_kj = L_kk^-1 B_kj (B_kk = I);  i == k: row tile k of M, written to linvT;
//                      i > k: B_ij -= L_ik X_kj.  B_ij (i > j) lives transposed in A's otherwise
//                      unused upper tile (j, i); its first touch, at k = j, is a plain write.
//
// Before them gp_refactor_mask_kernel reads the inert mask off the old factor's diagonal (and writes
// the targets with the inert rows' entries zeroed) and gp_refactor_build_kernel generates Khat
// (exp_rbf on the raw row differences, as gp_append_w_kernel does; the diagonal is exactly
// sf2 + sn2) and zeroes linvT; after them gp_refactor_w_kernel forms w (16 threads per row, each over
// every 16th column in ascending order, their sums added in a fixed order through LDS) and
// gp_refactor_alpha_kernel alpha (one wave per row: every lane sums its columns in ascending order,
// then a fixed butterfly), rows[.][3], tX, tW and the status.  2 nt + 4 plain launches and one
// 4-byte memset on the caller's stream; no sum crosses waves except through memory in a fixed order,
// no floating-point atomics, no grid-wide barrier.  launch_gp_refactor is three pieces (begin, factor,
// solve) around the build; the hyperparameter fit (gp_fit.hip) queues the same pieces around a build of
// its own.
//
// Inert rows (rejected append blocks) and the padding rows past n have a zero on the old factor's
// diagonal.  They take part as identity rows of Khat (diagonal 1, off-diagonal 0), so their row and
// column of L and of M are exact zeros off the diagonal; their target is never read into a sum, and
// they end with a zero linvT row and column, zero weight and zero tX / tW.
//
// Guard.  The status is 1 when every live target is finite and every pivot finite and positive (a
// bad pivot is replaced by 1); otherwise 0 and the GP's contents are unspecified.  Every access stays
// in bounds whatever the values.
#include "gp_tile.h"
#include <algorithm>

namespace gpmpc {

constexpr int kRefWaves = 4;   // tiles per workgroup (one wave each)

// Lane l's value in every lane (l a compile-time constant after unrolling): two v_readlane_b32
__device__ __forceinline__ double lane_value(double v, int l) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), l),
                            __builtin_amdgcn_readlane(__double2loint(v), l));
}

// mask[i] = 1 for an inert or padding row (zero diagonal of the old factor), ym the targets with those
// rows' entries replaced by zero; a live target that is not finite clears the status (set to 1 on the
// stream before the launch)
__global__ __launch_bounds__(256) void gp_refactor_mask_kernel(GPRefactor a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.npad) return;
    const bool inert = i >= a.n || a.linvT[(size_t)i * a.npad + i] == 0.0;
    const double yi = inert ? 0.0 : a.y[i];
    a.mask[i] = inert ? 1 : 0;
    a.ym[i] = yi;
    if (!isfinite(yi)) *a.flag = 0;
}

// Lower tiles of Khat into A (diagonal tiles in full), zeros into linvT.  One workgroup per tile.
__global__ __launch_bounds__(256) void gp_refactor_build_kernel(GPRefactor a) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    const int i = 16 * ti + (threadIdx.x >> 4), j = 16 * tj + (threadIdx.x & 15);
    a.linvT[(size_t)i * a.npad + j] = 0.0;
    if (tj > ti) return;
    const double4* rows = reinterpret_cast<const double4*>(a.rows);
    const double4 xi = rows[i], xj = rows[j];
    const double d0 = xi.x - xj.x, d1 = xi.y - xj.y, d2 = xi.z - xj.z;
    const double c = -0.5 * a.inv_ell2;
    double v = rbf_raw(c, a.sf2, d0, d1, d2);
    if (i == j) v = a.sf2 + a.sn2;
    if (a.mask[i] || a.mask[j]) v = (i == j) ? 1.0 : 0.0;
    a.A[(size_t)i * a.npad + j] = v;
}

// L_kk = chol(A_kk) and its inverse, then L_ik = A_ik L_kk^-T for the workgroup's row tiles
__global__ __launch_bounds__(64 * kRefWaves) void gp_refactor_panel_kernel(GPRefactor a, int k) {
    __shared__ double S[16][17], Li[16][17];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int nt = a.npad / 16;
    // Every wave factors A_kk in registers, lane (any kq) = row lc: no barrier inside.  Right-looking by
    // columns, which applies to every entry the updates j = 0, 1, .. in that order; a bad pivot is
    // replaced by 1.  What the lanes compute above the diagonal is never used.
    double s[16];
    {
        const double4* row = reinterpret_cast<const double4*>(a.A + (size_t)(16 * k + lc) * a.npad + 16 * k);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const double4 v = row[q];
            s[4 * q] = v.x, s[4 * q + 1] = v.y, s[4 * q + 2] = v.z, s[4 * q + 3] = v.w;
        }
    }
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 16; ++j) {
        const double piv = lane_value(s[j], j);
        const bool good = isfinite(piv) && piv > 0.0;
        ok = ok && good;
        const double ljj = good ? sqrt(piv) : 1.0;
        s[j] = (lc == j) ? ljj : s[j] / ljj;
#pragma unroll
        for (int q = j + 1; q < 16; ++q) s[q] = fma(-s[j], lane_value(s[j], q), s[q]);
    }
    if (tid < 16) {
#pragma unroll
        for (int q = 0; q < 16; ++q) S[tid][q] = s[q];
    }
    __syncthreads();
    // L_kk^-1 by forward substitution, lane = column lc (the terms before the diagonal are exact zeros)
    double li[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        double t = (i == lc) ? 1.0 : 0.0;
#pragma unroll
        for (int q = 0; q < i; ++q) t = fma(-S[i][q], li[q], t);
        li[i] = t / S[i][i];
    }
    if (tid < 16) {
#pragma unroll
        for (int i = 0; i < 16; ++i) Li[i][tid] = li[i];
    }
    __syncthreads();
    if (blockIdx.x == 0) {
        a.dinv[(size_t)k * 256 + tid] = Li[tid >> 4][tid & 15];
        if (tid == 0 && !ok) *a.flag = 0;
    }
    const int i = k + 1 + blockIdx.x * kRefWaves + wave;
    if (i >= nt) return;   // wave-uniform
    // lane (lc, kq) takes K indices 4 kq + j: one double4 of its row of A_ik; B[q][c] = L_kk^-1[c][q]
    double* arow = a.A + (size_t)(16 * i) * a.npad + 16 * k;
    const double4 av = *reinterpret_cast<const double4*>(arow + (size_t)lc * a.npad + 4 * kq);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, Li[lc][4 * kq + 0], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, Li[lc][4 * kq + 1], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.z, Li[lc][4 * kq + 2], acc, 0, 0, 0);
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av.w, Li[lc][4 * kq + 3], acc, 0, 0, 0);
    // acc[r] = L_ik[kq + 4r][lc]
#pragma unroll
    for (int r = 0; r < 4; ++r) arow[(size_t)(kq + 4 * r) * a.npad + lc] = acc[r];
}

// Step k of the trailing update and of the forward substitution: tile (i, j), i = k + blockIdx.y
__global__ __launch_bounds__(64 * kRefWaves) void gp_refactor_update_kernel(GPRefactor a, int k) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int i = k + blockIdx.y, j = blockIdx.x * kRefWaves + wave;
    if (j > i) return;   // wave-uniform
    const size_t ld = a.npad;
    if (j > k) {   // A_ij -= L_ik L_jk^T
        const double4 av = *reinterpret_cast<const double4*>(a.A + (size_t)(16 * i + lc) * ld + 16 * k + 4 * kq);
        const double4 bv = *reinterpret_cast<const double4*>(a.A + (size_t)(16 * j + lc) * ld + 16 * k + 4 * kq);
        double* ct = a.A + (size_t)(16 * i + kq) * ld + 16 * j + lc;
        f64x4 acc;
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = ct[(size_t)(4 * r) * ld];
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.x, bv.x, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.y, bv.y, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.z, bv.z, acc, 0, 0, 0);
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-av.w, bv.w, acc, 0, 0, 0);
#pragma unroll
        for (int r = 0; r < 4; ++r) ct[(size_t)(4 * r) * ld] = acc[r];
        return;
    }
    // X_kj = L_kk^-1 B_kj; x[r] = X_kj[kq + 4r][lc].  B_kj[q][c] is A[16j + c][16k + q]
    const double* di = a.dinv + (size_t)k * 256;
    f64x4 x;
    if (j == k) {
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = di[(kq + 4 * r) * 16 + lc];
    } else {
        const double4 lv = *reinterpret_cast<const double4*>(di + lc * 16 + 4 * kq);
        const double4 bv = *reinterpret_cast<const double4*>(a.A + (size_t)(16 * j + lc) * ld + 16 * k + 4 * kq);
        x = f64x4{0.0, 0.0, 0.0, 0.0};
        x = __builtin_amdgcn_mfma_f64_16x16x4f64(lv.x, bv.x, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f64_16x16x4f64(lv.y, bv.y, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f64_16x16x4f64(lv.z, bv.z, x, 0, 0, 0);
        x = __builtin_amdgcn_mfma_f64_16x16x4f64(lv.w, bv.w, x, 0, 0, 0);
    }
    if (i == k) {   // M[16k + kq + 4r][16j + lc]: row 16j + lc of linvT; inert rows end as zeros
        const int col = 16 * j + lc;
        const bool mc = a.mask[col] != 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * k + kq + 4 * r;
            a.linvT[(size_t)col * ld + row] = (mc || a.mask[row] != 0) ? 0.0 : x[r];
        }
        return;
    }
    // B_ij -= L_ik X_kj: x[r] is the B operand of K-step r, the A operand L_ik[lc][kq + 4r]
    const double* lrow = a.A + (size_t)(16 * i + lc) * ld + 16 * k + kq;
    double* bt = a.A + (size_t)(16 * j + lc) * ld + 16 * i + kq;   // B_ij[kq + 4r][lc]
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    if (j < k) {
#pragma unroll
        for (int r = 0; r < 4; ++r) acc[r] = bt[4 * r];
    }
#pragma unroll
    for (int r = 0; r < 4; ++r) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(-lrow[4 * r], x[r], acc, 0, 0, 0);
#pragma unroll
    for (int r = 0; r < 4; ++r) bt[4 * r] = acc[r];
}

// w_i = sum_{j <= i} M[i][j] ym_j: 64 rows per workgroup, thread (c, q) sums the terms j = q, q + 16, ..
// of row 64 b + c in ascending order; the 16 partial sums are added in the order of q through LDS
__global__ __launch_bounds__(1024) void gp_refactor_w_kernel(GPRefactor a) {
    __shared__ double part[16][64];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + c;
    double s = 0.0;
    if (i < a.npad) {
        const double* col = a.linvT + i;
#pragma unroll 4
        for (int j = q; j <= i; j += 16) s = fma(col[(size_t)j * a.npad], a.ym[j], s);
    }
    part[q][c] = s;
    __syncthreads();
    if (q != 0 || i >= a.npad) return;
    double t = part[0][c];
#pragma unroll
    for (int p = 1; p < 16; ++p) t += part[p][c];
    a.w[i] = t;
}

// alpha_j = sum_{i >= j} M[i][j] w_i: one wave per row of linvT; rows[.][3], tX, tW, the status
__global__ __launch_bounds__(64 * kRefWaves) void gp_refactor_alpha_kernel(GPRefactor a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * kRefWaves + wave;
    if (blockIdx.x == 0 && threadIdx.x == 0 && a.ok) *a.ok = *a.flag;
    if (j >= a.npad) return;   // wave-uniform
    const double* row = a.linvT + (size_t)j * a.npad;
    double s = 0.0;
    for (int i = (j & ~63) + lane; i < a.npad; i += 64) s = fma(row[i], a.w[i], s);
    s += __shfl_xor(s, 32);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (lane != 0) return;
    const bool live = a.mask[j] == 0;
    const double4 rw = reinterpret_cast<const double4*>(a.rows)[j];
    const double al = live ? s : 0.0;
    a.rows[(size_t)j * 4 + 3] = al;
    const TileSlot slot = tile_slot(j);
    double xc[3];
    tile_centre(xc, rw.x, rw.y, rw.z, a.xbar, a.d, live);
    tile_write_x(a.tX, slot, xc, a.inv_ell2, -0.5 * a.inv_ell2, live);
    tile_write_w(a.tW, slot, al, xc);
}

static bool refactor_shape_ok(const GPRefactor& a) { return a.n >= 1 && a.npad % 16 == 0 && a.n <= a.npad; }

hipError_t launch_gp_refactor_begin(const GPRefactor& a, hipStream_t stream) {
    if (!refactor_shape_ok(a)) return hipErrorInvalidValue;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.flag), 1, 1, stream);   // the status starts at 1
    if (e != hipSuccess) return e;
    GP_LAUNCH(gp_refactor_mask_kernel, dim3((a.npad + 255) / 256), dim3(256), stream, a);
    return hipSuccess;
}

hipError_t launch_gp_refactor_factor(const GPRefactor& a, hipStream_t stream) {
    if (!refactor_shape_ok(a)) return hipErrorInvalidValue;
    const int nt = a.npad / 16, tb = (nt + kRefWaves - 1) / kRefWaves;
    for (int k = 0; k < nt; ++k) {
        const int below = nt - k - 1;
        GP_LAUNCH(gp_refactor_panel_kernel, dim3(std::max(1, (below + kRefWaves - 1) / kRefWaves)), dim3(64 * kRefWaves),
                  stream, a, k);
        GP_LAUNCH(gp_refactor_update_kernel, dim3(tb, nt - k), dim3(64 * kRefWaves), stream, a, k);
    }
    return hipSuccess;
}

hipError_t launch_gp_refactor_solve(const GPRefactor& a, hipStream_t stream) {
    if (!refactor_shape_ok(a)) return hipErrorInvalidValue;
    GP_LAUNCH(gp_refactor_w_kernel, dim3((a.npad + 63) / 64), dim3(1024), stream, a);
    GP_LAUNCH(gp_refactor_alpha_kernel, dim3((a.npad + kRefWaves - 1) / kRefWaves), dim3(64 * kRefWaves), stream, a);
    return hipSuccess;
}

hipError_t launch_gp_refactor(const GPRefactor& a, hipStream_t stream) {
    hipError_t e = launch_gp_refactor_begin(a, stream);
    if (e != hipSuccess) return e;
    const int nt = a.npad / 16;
    GP_LAUNCH(gp_refactor_build_kernel, dim3(nt, nt), dim3(256), stream, a);
    e = launch_gp_refactor_factor(a, stream);
    return e != hipSuccess ? e : launch_gp_refactor_solve(a, stream);
}

}  // namespace gpmpc
