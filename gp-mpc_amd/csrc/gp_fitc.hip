// Building the FITC inducing-point mean of an exact GP on the device (gpmpc_gp_fitc): the posterior weights of
// the M inducing rows S = X[idx] from the handle's own training rows X (n rows, npad = 16 nt padded), its
// current hyperparameters and the caller's device targets y, restating gpmpc/gpmpc.py:392-397 in the factored
// form (mpad = 16 mt the padded M; jitter an absolute value on the diagonal of K_ss):
//
//   K_ss + jitter I = L L^T,  V = L^-1 k(S, X)  (mpad x npad),  Gamma_i = sf2 + sn2 - |V[:, i]|^2,
//   B = I + V Gamma^-1 V^T = C C^T,  w = L^-T B^-1 V Gamma^-1 y
//
// so that the FITC mean at z is sum_j w_j k(z, S_j) with k carrying sf2: what gpmpc_set_gp(X = S, alpha = w)
// installs.  Launches (plain, on the caller's stream), after a 4-byte memset that sets the status to 1:
//
//   gp_fitc_gather_kernel   the inert mask of the training rows (zero on the factor's diagonal, or past n), the
//                           targets with the inert rows' entries zeroed, the inducing rows gathered and checked
//   gp_fitc_kss_kernel      lower tiles of K_ss + jitter I (exp_rbf on the raw row differences, the diagonal
//                           exactly sf2 + jitter); zeros into (L^-1)^T
//   launch_gp_refactor_factor on the M-sized view: L and (L^-1)^T, the pivots' status (gp_refactor.hip)
//   gp_fitc_v_kernel        V, one wave per 16 x 16 tile (I, J) on v_mfma_f64_16x16x4_f64: the k loop runs over
//                           the tiles 0 .. I of L^-1 in ascending order, k(S, X) generated on the fly (every lane
//                           four values per step, none twice in a wave); an inert column is exact zeros
//   gp_fitc_gamma_kernel    |V[:, i]|^2 per column (four interleaved sums over the rows in ascending order, added
//                           in a fixed order), Gamma^-1 (0 for an inert row) and Gamma^-1 y
//   gp_fitc_b_kernel        lower tiles of B, one wave per tile, four accumulators over the columns in ascending
//                           order added in a fixed order (gram16's loop with two operands); zeros into (C^-1)^T
//   launch_gp_refactor_factor again: C and (C^-1)^T
//   gp_fitc_row_kernel      u = V (Gamma^-1 y), one wave per row, a fixed butterfly
//   gp_fitc_lower_kernel    p = C^-1 u                 (gp_refactor_w_kernel's sums)
//   gp_fitc_upper_kernel    q = C^-T p, then w = L^-T q (gp_refactor_alpha_kernel's); the second one closes with
//                           rows[.][3] = w and the tile pack of the inducing rows, centred on the GP's xbar
//
// 4 mt + 9 launches.  Every sum has a fixed order, there are no floating-point atomics and no grid-wide barrier:
// the result depends on the inputs alone, bit for bit.  Everything is built in work space (V in the GP's spare
// factor buffer) and in staged rows and tiles the caller installs after it has read the status.
//
// Guard.  The status is 1 when every index names a live row, every live target is finite, every pivot of L and
// of C is finite and positive (a bad one is replaced by 1) and every live row's Gamma is finite and positive;
// otherwise 0, and the caller discards what was built.  A bad index reads row 0 instead.  Every access stays in
// bounds whatever the values.
#include "gp_tile.h"

namespace gpmpc {

constexpr int kFitcWaves = 4;   // tiles per workgroup (one wave each)

__global__ __launch_bounds__(256) void gp_fitc_gather_kernel(GPFitc a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i < a.npad) {
        const bool inert = i >= a.n || a.linvT[(size_t)i * a.npad + i] == 0.0;
        const double yi = inert ? 0.0 : a.y[i];
        a.lmask[i] = inert ? 1 : 0;
        a.t[i] = yi;
        if (!isfinite(yi)) *a.flag = 0;
    }
    if (i >= a.mpad) return;
    const bool pad = i >= a.M;
    int r = 0;
    if (!pad) {
        r = a.idx[i];
        bool bad = r < 0 || r >= a.n;
        if (!bad) bad = a.linvT[(size_t)r * a.npad + r] == 0.0;
        if (bad) {
            *a.flag = 0;
            r = 0;
        }
    }
    const double4 x = reinterpret_cast<const double4*>(a.rows)[r];
    reinterpret_cast<double4*>(a.srows)[i] = pad ? double4{0.0, 0.0, 0.0, 0.0} : double4{x.x, x.y, x.z, 0.0};
    a.sidx[i] = r;
    a.smask[i] = pad ? 1 : 0;
}

// Lower tiles of K_ss + jitter I into A (diagonal tiles in full; a padding row is an identity row), zeros into
// lt1.  One workgroup per tile.
__global__ __launch_bounds__(256) void gp_fitc_kss_kernel(GPFitc a) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    const int i = 16 * ti + (threadIdx.x >> 4), j = 16 * tj + (threadIdx.x & 15);
    a.lt1[(size_t)i * a.mpad + j] = 0.0;
    if (tj > ti) return;
    const double4* rows = reinterpret_cast<const double4*>(a.srows);
    const double4 xi = rows[i], xj = rows[j];
    double v = rbf_raw(-0.5 * a.inv_ell2, a.sf2, xi.x - xj.x, xi.y - xj.y, xi.z - xj.z);
    if (i == j) v = a.sf2 + a.jitter;
    if (a.smask[i] || a.smask[j]) v = (i == j) ? 1.0 : 0.0;
    a.A[(size_t)i * a.mpad + j] = v;
}

// V tile (I, J) = sum over kt <= I of L^-1 tile (I, kt) times k(S tile kt, X tile J).  Lane (lc, kq) holds
// training row 16 J + lc and generates k(S[16 kt + 4 kq + j], that row), j = 0 .. 3: the B operands of the step's
// four MFMAs; the A operands are L^-1[16 I + lc][16 kt + 4 kq + j] = lt1[(16 kt + 4 kq + j) mpad + 16 I + lc].
__global__ __launch_bounds__(64 * kFitcWaves) void gp_fitc_v_kernel(GPFitc a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int I = blockIdx.y, J = blockIdx.x * kFitcWaves + wave;
    if (J >= a.npad / 16) return;   // wave-uniform
    const size_t ldm = a.mpad;
    const int col = 16 * J + lc;
    const double4 x = reinterpret_cast<const double4*>(a.rows)[col];
    const bool live = a.lmask[col] == 0;
    const double c = -0.5 * a.inv_ell2;
    const double4* srows = reinterpret_cast<const double4*>(a.srows);
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int kt = 0; kt <= I; ++kt) {
        const int k0 = 16 * kt + 4 * kq;
        double e[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double4 s = srows[k0 + j];
            const double d0 = s.x - x.x, d1 = s.y - x.y, d2 = s.z - x.z;
            e[j] = c * fma(d0, d0, fma(d1, d1, d2 * d2));
        }
        exp_rbf_n<4>(e);
        const double* lt = a.lt1 + (size_t)k0 * ldm + 16 * I + lc;
#pragma unroll
        for (int j = 0; j < 4; ++j)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(lt[(size_t)j * ldm], live ? a.sf2 * e[j] : 0.0, acc, 0, 0, 0);
    }
    // acc[r] = V[16 I + kq + 4 r][16 J + lc]
#pragma unroll
    for (int r = 0; r < 4; ++r) a.V[(size_t)(16 * I + kq + 4 * r) * a.npad + col] = acc[r];
}

// Gamma_i = sf2 + sn2 - |V[:, i]|^2, thread = column: ginv = 1 / Gamma (0 for an inert row), t = ginv y
__global__ __launch_bounds__(256) void gp_fitc_gamma_kernel(GPFitc a) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= a.npad) return;
    const double* v = a.V + i;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int r = 0; r < a.mpad; r += 4) {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double x = v[(size_t)(r + k) * a.npad];
            s[k] = fma(x, x, s[k]);
        }
    }
    const double gam = (a.sf2 + a.sn2) - ((s[0] + s[1]) + (s[2] + s[3]));
    const bool live = a.lmask[i] == 0;
    const bool good = isfinite(gam) && gam > 0.0;
    if (live && !good) *a.flag = 0;
    const double gi = (live && good) ? 1.0 / gam : 0.0;
    a.ginv[i] = gi;
    a.t[i] = gi * a.t[i];
}

// B tile (I, J), J <= I: I + sum over the columns of V[16 I + r][.] ginv[.] V[16 J + c][.]; zeros into lt2
__global__ __launch_bounds__(64 * kFitcWaves) void gp_fitc_b_kernel(GPFitc a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int I = blockIdx.y, J = blockIdx.x * kFitcWaves + wave;
    if (J >= a.mpad / 16) return;   // wave-uniform
    const size_t ldm = a.mpad;
#pragma unroll
    for (int r = 0; r < 4; ++r) a.lt2[(size_t)(16 * I + kq + 4 * r) * ldm + 16 * J + lc] = 0.0;
    if (J > I) return;
    const double* ra = a.V + (size_t)(16 * I + lc) * a.npad + 4 * kq;
    const double* rb = a.V + (size_t)(16 * J + lc) * a.npad + 4 * kq;
    const double* gi = a.ginv + 4 * kq;
    f64x4 g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int s = 0; s < a.npad / 16; ++s) {
        const double4 av = *reinterpret_cast<const double4*>(ra + 16 * s);
        const double4 bv = *reinterpret_cast<const double4*>(rb + 16 * s);
        const double4 gv = *reinterpret_cast<const double4*>(gi + 16 * s);
        g[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x * gv.x, g[0], 0, 0, 0);
        g[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.y * gv.y, g[1], 0, 0, 0);
        g[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.z, bv.z * gv.z, g[2], 0, 0, 0);
        g[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.w, bv.w * gv.w, g[3], 0, 0, 0);
    }
    // entry r is B[16 I + kq + 4 r][16 J + lc]; a padding row is an identity row
    const int col = 16 * J + lc;
    const bool mc = a.smask[col] != 0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * I + kq + 4 * r;
        double v = (g[0][r] + g[1][r]) + (g[2][r] + g[3][r]);
        if (row == col) v += 1.0;
        if (mc || a.smask[row] != 0) v = (row == col) ? 1.0 : 0.0;
        a.A[(size_t)row * ldm + col] = v;
    }
}

// u_r = sum_i V[r][i] t_i: one wave per row, every lane its columns in ascending order, then a fixed butterfly
__global__ __launch_bounds__(64 * kFitcWaves) void gp_fitc_row_kernel(GPFitc a) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = blockIdx.x * kFitcWaves + wave;
    if (r >= a.mpad) return;   // wave-uniform
    const double* row = a.V + (size_t)r * a.npad;
    double s = 0.0;
    for (int i = lane; i < a.npad; i += 64) s = fma(row[i], a.t[i], s);
    s += __shfl_xor(s, 32);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (lane == 0) a.u[r] = s;
}

// out_i = sum_{j <= i} T[i][j] v_j for the lower-triangular T stored transposed (lt[j mpad + i]): 64 rows per
// workgroup, thread (c, q) sums the terms j = q, q + 16, .. in ascending order; the 16 sums are added in the
// order of q through LDS
__global__ __launch_bounds__(1024) void gp_fitc_lower_kernel(GPFitc a, const double* lt, const double* v, double* out) {
    __shared__ double part[16][64];
    const int c = threadIdx.x & 63, q = threadIdx.x >> 6;
    const int i = blockIdx.x * 64 + c;
    double s = 0.0;
    if (i < a.mpad) {
        const double* col = lt + i;
#pragma unroll 4
        for (int j = q; j <= i; j += 16) s = fma(col[(size_t)j * a.mpad], v[j], s);
    }
    part[q][c] = s;
    __syncthreads();
    if (q != 0 || i >= a.mpad) return;
    double t = part[0][c];
#pragma unroll
    for (int p = 1; p < 16; ++p) t += part[p][c];
    out[i] = t;
}

// out_j = sum_{i >= j} T[i][j] v_i: one wave per row of lt.  last: out_j is the weight of inducing row j, written
// to the staged rows and tile pack (a padding row: zeros)
__global__ __launch_bounds__(64 * kFitcWaves) void gp_fitc_upper_kernel(GPFitc a, const double* lt, const double* v,
                                                                        double* out, int last) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int j = blockIdx.x * kFitcWaves + wave;
    if (j >= a.mpad) return;   // wave-uniform
    const double* row = lt + (size_t)j * a.mpad;
    double s = 0.0;
    for (int i = (j & ~63) + lane; i < a.mpad; i += 64) s = fma(row[i], v[i], s);
    s += __shfl_xor(s, 32);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    if (lane != 0) return;
    out[j] = s;
    if (!last) return;
    const bool live = a.smask[j] == 0;
    const double4 rw = reinterpret_cast<const double4*>(a.srows)[j];
    const double w = live ? s : 0.0;
    a.srows[(size_t)j * 4 + 3] = w;
    const TileSlot slot = tile_slot(j);
    double xc[3];
    tile_centre(xc, rw.x, rw.y, rw.z, a.xbar, a.d, live);
    tile_write_x(a.stX, slot, xc, a.inv_ell2, -0.5 * a.inv_ell2, live);
    tile_write_w(a.stW, slot, w, xc);
}

hipError_t launch_gp_fitc(const GPFitc& a, hipStream_t stream) {
    if (a.M < 1 || a.M > a.n || a.n > a.npad || a.npad % 16 != 0 || a.mpad % 16 != 0 || a.M > a.mpad ||
        a.mpad - a.M >= 16 || a.mpad > a.npad)
        return hipErrorInvalidValue;
    hipError_t e = hipMemsetD32Async(reinterpret_cast<hipDeviceptr_t>(a.flag), 1, 1, stream);   // the status starts at 1
    if (e != hipSuccess) return e;
    const int nt = a.npad / 16, mt = a.mpad / 16;
    // the two factorisations: gp_refactor.hip's panels on an M-sized view (what they read of it: A, the factor
    // written, the diagonal tiles' inverses, the mask and the status)
    GPRefactor f{};
    f.A = a.A;
    f.linvT = a.lt1;
    f.npad = a.mpad;
    f.n = a.M;
    f.dinv = a.dinv;
    f.mask = a.smask;
    f.flag = a.flag;
    GP_LAUNCH(gp_fitc_gather_kernel, dim3((a.npad + 255) / 256), dim3(256), stream, a);
    GP_LAUNCH(gp_fitc_kss_kernel, dim3(mt, mt), dim3(256), stream, a);
    e = launch_gp_refactor_factor(f, stream);
    if (e != hipSuccess) return e;
    GP_LAUNCH(gp_fitc_v_kernel, dim3((nt + kFitcWaves - 1) / kFitcWaves, mt), dim3(64 * kFitcWaves), stream, a);
    GP_LAUNCH(gp_fitc_gamma_kernel, dim3((a.npad + 255) / 256), dim3(256), stream, a);
    GP_LAUNCH(gp_fitc_b_kernel, dim3((mt + kFitcWaves - 1) / kFitcWaves, mt), dim3(64 * kFitcWaves), stream, a);
    f.linvT = a.lt2;
    e = launch_gp_refactor_factor(f, stream);
    if (e != hipSuccess) return e;
    const dim3 waves((a.mpad + kFitcWaves - 1) / kFitcWaves);
    GP_LAUNCH(gp_fitc_row_kernel, waves, dim3(64 * kFitcWaves), stream, a);
    GP_LAUNCH(gp_fitc_lower_kernel, dim3((a.mpad + 63) / 64), dim3(1024), stream, a, (const double*)a.lt2,
              (const double*)a.u, a.p);
    GP_LAUNCH(gp_fitc_upper_kernel, waves, dim3(64 * kFitcWaves), stream, a, (const double*)a.lt2, (const double*)a.p,
              a.q, 0);
    GP_LAUNCH(gp_fitc_upper_kernel, waves, dim3(64 * kFitcWaves), stream, a, (const double*)a.lt1, (const double*)a.q,
              a.u, 1);
    return hipSuccess;
}

}  // namespace gpmpc
