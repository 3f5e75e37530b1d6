// Fitting an exact GP's hyperparameters on the device (gpmpc_gp_mll, gpmpc_gp_fit): the marginal log
// likelihood per live row and its gradient from what the handle holds, and Adam on it.
//
//   MLL / n = (-y^T alpha / 2 + sum_i log M_ii - n log(2 pi) / 2) / n        M = L^-1 (GPDev::linvT, transposed)
//   d(MLL / n) / d theta = tr((alpha alpha^T - Khat^-1) dKhat / d theta) / (2 n)
//   dKhat / d ell = sf2 E o D2 / ell^3,  dKhat / d sf2 = E,  dKhat / d sn2 = I    (E = exp(-D2 / 2 ell^2))
//
// n counts the live rows.  Khat^-1 = M^T M = linvT linvT^T is never stored:
//
//   gp_fit_grad_kernel     one wave per lower 16 x 16 tile (I, J), J <= I: the tile of Khat^-1 over the column
//                          tiles t >= I of linvT (the ones before are structural zeros of both row tiles) on
//                          v_mfma_f64_16x16x4_f64, then W = alpha_i alpha_j - Khat^-1_ij, E and D2 from the
//                          rows in the MFMA C/D layout and the tile's three sums {W E D2, W E, W on i = j}
//                          (an off-diagonal tile counts twice) after a fixed butterfly into its slot.
//   gp_fit_finish_kernel   one workgroup: the slots in tile order (thread q takes tiles q, q + 256, ..; the 256
//                          sums are added in the order of q), sum log M_ii, y^T alpha and the count of live rows;
//                          writes {MLL / n, d / d ell, d / d sf2, d / d sn2}.
//
// An inert or padding row has alpha = 0 and a zero row and column of linvT, so its W is an exact zero.
//
// The fit (the loop of gpmpc/gp.py fit_gp) keeps raw parameters, Adam's moments and step count, the last
// loss, the stop and fail flags and the constrained hyperparameters in a device block (kFit*).  One
// iteration: gp_fit_build_kernel (Khat at the block's hyperparameters; gp_refactor_build_kernel with
// device-resident values), gp_refactor.hip's panels, w and alpha, the two kernels above and
// gp_fit_adam_kernel (torch.optim.Adam's step through softplus' chain rule, the |last - loss| < 1e-3
// rule, the next hyperparameters).  After a stop or a failure the block no longer changes, so iterations
// queued past it repeat the last factorisation and leave the result alone.
//
// Plain stream-ordered launches; no sum crosses waves except through memory in a fixed order, no
// floating-point atomics, no grid-wide barrier.
#include "gp_tile.h"

namespace gpmpc {

constexpr int kFitWaves = 4;      // tiles per workgroup (one wave each)
constexpr int kFitThreads = 256;  // of the finishing workgroup

__device__ __forceinline__ double wave_sum(double s) {
    s += __shfl_xor(s, 32);
    s += __shfl_xor(s, 16);
    s += __shfl_xor(s, 8);
    s += __shfl_xor(s, 4);
    s += __shfl_xor(s, 2);
    s += __shfl_xor(s, 1);
    return s;
}

// softplus as torch computes it (threshold 20) and its derivative
__device__ __forceinline__ double softplus20(double x) { return x > 20.0 ? x : log1p(exp(x)); }
__device__ __forceinline__ double softplus20_grad(double x) {
    const double z = exp(x);
    return x > 20.0 ? 1.0 : z / (z + 1.0);
}

__global__ void gp_fit_set_hyp_kernel(double* state, double inv_ell2, double sf2, double sn2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    double* hyp = state + kFitHyp;
    hyp[0] = inv_ell2, hyp[1] = sf2, hyp[2] = sn2, hyp[3] = 1.0 / sqrt(inv_ell2);
}

__device__ __forceinline__ void fit_write_hyp(double* state) {
    const double ell = softplus20(state[kFitRaw]);
    double* hyp = state + kFitHyp;
    hyp[0] = 1.0 / (ell * ell);
    hyp[1] = softplus20(state[kFitRaw + 1]);
    hyp[2] = 1e-6 + softplus20(state[kFitRaw + 2]);
    hyp[3] = ell;
}

__global__ void gp_fit_init_kernel(double* state, double r0, double r1, double r2) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    for (int k = 0; k < kFitDoubles; ++k) state[k] = 0.0;
    state[kFitRaw] = r0, state[kFitRaw + 1] = r1, state[kFitRaw + 2] = r2;
    state[kFitLast] = INFINITY;
    fit_write_hyp(state);
}

// gp_refactor_build_kernel with the hyperparameters read from the fit-state block
__global__ __launch_bounds__(256) void gp_fit_build_kernel(GPRefactor a, const double* hyp) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    const int i = 16 * ti + (threadIdx.x >> 4), j = 16 * tj + (threadIdx.x & 15);
    a.linvT[(size_t)i * a.npad + j] = 0.0;
    if (tj > ti) return;
    const double inv_ell2 = hyp[0], sf2 = hyp[1], sn2 = hyp[2];
    const double4* rows = reinterpret_cast<const double4*>(a.rows);
    const double4 xi = rows[i], xj = rows[j];
    const double d0 = xi.x - xj.x, d1 = xi.y - xj.y, d2 = xi.z - xj.z;
    const double c = -0.5 * inv_ell2;
    double v = rbf_raw(c, sf2, d0, d1, d2);
    if (i == j) v = sf2 + sn2;
    if (a.mask[i] || a.mask[j]) v = (i == j) ? 1.0 : 0.0;
    a.A[(size_t)i * a.npad + j] = v;
}

// Tile (I, J) of Khat^-1 and its three sums: I = blockIdx.y, J = blockIdx.x * kFitWaves + wave
__global__ __launch_bounds__(64 * kFitWaves) void gp_fit_grad_kernel(GPFit f) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int lc = lane & 15, kq = lane >> 4;
    const int I = blockIdx.y, J = blockIdx.x * kFitWaves + wave;
    if (J > I) return;   // wave-uniform
    const int nt = f.npad / 16;
    const size_t ld = f.npad;
    // lane (lc, kq) takes columns 16t + 4kq + j of row lc of either row tile (both operands one register each,
    // so the K order is free); four accumulators added in a fixed order: kinv[r] = Khat^-1[16I + kq + 4r][16J + lc]
    const double* ar = f.linvT + (size_t)(16 * I + lc) * ld + 16 * I + 4 * kq;
    const double* br = f.linvT + (size_t)(16 * J + lc) * ld + 16 * I + 4 * kq;
    f64x4 g[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) g[j] = f64x4{0.0, 0.0, 0.0, 0.0};
    for (int t = I; t < nt; ++t, ar += 16, br += 16) {
        const double4 av = *reinterpret_cast<const double4*>(ar);
        const double4 bv = *reinterpret_cast<const double4*>(br);
        g[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.x, bv.x, g[0], 0, 0, 0);
        g[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.y, bv.y, g[1], 0, 0, 0);
        g[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.z, bv.z, g[2], 0, 0, 0);
        g[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(av.w, bv.w, g[3], 0, 0, 0);
    }
    const double c = -0.5 * f.state[kFitHyp];
    const double4* rows = reinterpret_cast<const double4*>(f.rows);
    const int j = 16 * J + lc;
    const double4 xj = rows[j];
    double s_ed = 0.0, s_e = 0.0, s_d = 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = 16 * I + kq + 4 * r;
        const double4 xi = rows[i];
        const double kinv = (g[0][r] + g[1][r]) + (g[2][r] + g[3][r]);
        const double w = fma(xi.w, xj.w, -kinv);
        const double d0 = xi.x - xj.x, d1 = xi.y - xj.y, d2 = xi.z - xj.z;
        const double q = fma(d0, d0, fma(d1, d1, d2 * d2));
        const double we = w * exp_rbf(c * q);
        s_e += we;
        s_ed = fma(we, q, s_ed);
        if (i == j) s_d += w;
    }
    s_ed = wave_sum(s_ed);
    s_e = wave_sum(s_e);
    s_d = wave_sum(s_d);
    if (lane != 0) return;
    const double twice = (I == J) ? 1.0 : 2.0;
    double* slot = f.part + ((size_t)I * (I + 1) / 2 + J) * 3;
    slot[0] = twice * s_ed, slot[1] = twice * s_e, slot[2] = s_d;
}

// The slots in tile order, log det and y^T alpha over the live rows; out[4]
__global__ __launch_bounds__(kFitThreads) void gp_fit_finish_kernel(GPFit f, double* out) {
    __shared__ double part[6][kFitThreads], tot[6];
    const int q = threadIdx.x;
    const int nt = f.npad / 16;
    const size_t tiles = (size_t)nt * (nt + 1) / 2;
    double s[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};   // W E D2, W E, W on the diagonal, log M_ii, y alpha, live rows
    for (size_t p = q; p < tiles; p += kFitThreads) {
        const double* slot = f.part + p * 3;
        s[0] += slot[0], s[1] += slot[1], s[2] += slot[2];
    }
    for (int i = q; i < f.n; i += kFitThreads) {
        const double m = f.linvT[(size_t)i * f.npad + i];
        if (m == 0.0) continue;   // inert
        s[3] += log(m);
        s[4] = fma(f.y[i], f.rows[(size_t)i * 4 + 3], s[4]);
        s[5] += 1.0;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k) part[k][q] = s[k];
    __syncthreads();
    if (q < 6) {
        double t = part[q][0];
        for (int p = 1; p < kFitThreads; ++p) t += part[q][p];
        tot[q] = t;
    }
    __syncthreads();
    if (q != 0) return;
    const double* hyp = f.state + kFitHyp;
    const double ell = hyp[3], sf2 = hyp[1];
    const double n = tot[5], h = 0.5 / n;
    out[0] = (-0.5 * tot[4] + tot[3] - 0.5 * n * 1.8378770664093453) / n;   // log(2 pi)
    out[1] = h * (sf2 / (ell * ell * ell)) * tot[0];
    out[2] = h * tot[1];
    out[3] = h * tot[2];
}

// One Adam step on the loss -MLL / n with respect to the raw parameters; hist row = the step taken
__global__ void gp_fit_adam_kernel(double* state, const int32_t* flag, double lr, double* hist) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    if (state[kFitStop] != 0.0 || state[kFitFail] != 0.0) return;
    const double* ev = state + kFitOut;
    const double loss = -ev[0];
    double g[3];
    bool fin = *flag != 0 && isfinite(loss);
    for (int k = 0; k < 3; ++k) {
        g[k] = -ev[1 + k] * softplus20_grad(state[kFitRaw + k]);
        fin = fin && isfinite(g[k]);
    }
    if (!fin) {
        state[kFitFail] = 1.0;
        return;
    }
    constexpr double b1 = 0.9, b2 = 0.999, eps = 1e-8;
    const double t = state[kFitStep] + 1.0;
    const double bc1 = 1.0 - pow(b1, t), bc2 = 1.0 - pow(b2, t);
    const double step = lr / bc1, bc2s = sqrt(bc2);
    for (int k = 0; k < 3; ++k) {
        const double m = state[kFitM + k] + (1.0 - b1) * (g[k] - state[kFitM + k]);
        const double v = b2 * state[kFitV + k] + (1.0 - b2) * g[k] * g[k];
        state[kFitM + k] = m;
        state[kFitV + k] = v;
        state[kFitRaw + k] -= step * (m / (sqrt(v) / bc2s + eps));
    }
    state[kFitStep] = t;
    if (hist) {
        double* hr = hist + ((size_t)t - 1) * 4;
        hr[0] = loss, hr[1] = state[kFitRaw], hr[2] = state[kFitRaw + 1], hr[3] = state[kFitRaw + 2];
    }
    if (fabs(state[kFitLast] - loss) < 1e-3) {
        state[kFitStop] = 1.0;
        return;   // (the factor of the final refactorisation is the host's: the block's hyperparameters stay)
    }
    state[kFitLast] = loss;
    fit_write_hyp(state);
}

hipError_t launch_gp_fit_set_hyp(double* state, double inv_ell2, double sf2, double sn2, hipStream_t stream) {
    GP_LAUNCH(gp_fit_set_hyp_kernel, dim3(1), dim3(64), stream, state, inv_ell2, sf2, sn2);
    return hipSuccess;
}

hipError_t launch_gp_fit_eval(const GPFit& f, double* out, hipStream_t stream) {
    if (f.n < 1 || f.npad % 16 != 0 || f.n > f.npad) return hipErrorInvalidValue;
    const int nt = f.npad / 16;
    GP_LAUNCH(gp_fit_grad_kernel, dim3((nt + kFitWaves - 1) / kFitWaves, nt), dim3(64 * kFitWaves), stream, f);
    GP_LAUNCH(gp_fit_finish_kernel, dim3(1), dim3(kFitThreads), stream, f, out);
    return hipSuccess;
}

hipError_t launch_gp_fit_init(double* state, const double* raw, hipStream_t stream) {
    GP_LAUNCH(gp_fit_init_kernel, dim3(1), dim3(64), stream, state, raw[0], raw[1], raw[2]);
    return hipSuccess;
}

hipError_t launch_gp_fit_iteration(const GPRefactor& a, const GPFit& f, double lr, double* hist_dev, hipStream_t stream) {
    if (a.npad != f.npad || a.npad % 16 != 0 || a.n < 1 || a.n > a.npad) return hipErrorInvalidValue;
    const int nt = a.npad / 16;
    GP_LAUNCH(gp_fit_build_kernel, dim3(nt, nt), dim3(256), stream, a, f.state + kFitHyp);
    hipError_t e = launch_gp_refactor_factor(a, stream);
    if (e == hipSuccess) e = launch_gp_refactor_solve(a, stream);
    if (e == hipSuccess) e = launch_gp_fit_eval(f, f.state + kFitOut, stream);
    if (e != hipSuccess) return e;
    GP_LAUNCH(gp_fit_adam_kernel, dim3(1), dim3(64), stream, f.state, a.flag, lr, hist_dev);
    return hipSuccess;
}

}  // namespace gpmpc
