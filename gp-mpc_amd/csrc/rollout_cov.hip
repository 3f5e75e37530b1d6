// State covariance along a finished rollout (gpmpc_rollout_lin, cov_dev): the tightening's recursion
// (gpmpc/gpmpc.py:425-498) with the learned model's own Jacobians along the trajectory in place of the prior's
// constant Ad, Bd:
//   S_0 = cov0 or zero
//   Phi_k = A_k + B_k K                      (K = the feedback gain; open loop: Phi_k = A_k)
//   S_{k+1} = Phi_k S_k Phi_k^T + Bd diag(q_k) Bd^T
//   q_k[j] = dt^2 sum_g W_{j,g}(x_k, u_k) (var_{g,k} + noise_g)     W = Model::var_weights, Bd = columns Model::unc
// The steps are sequential; the work is parallel over trajectories and matrix entries: NX^2 threads per trajectory,
// thread (i, j) owns entry (i, j), and a 256-thread block holds 256 / NX^2 trajectories (16, 7 and 1 for cartpole,
// quad2d and quad3d; the rest of the block idles).  Per step, with S_k, Phi_k and M in LDS:
//   1. Phi[i][j] = A[i][j] + sum_c B[i][c] K[c][j], c ascending; the threads of the uncertain diagonal entries form q
//   2. M[i][j] = sum_b S[i][b] Phi[j][b], b ascending                                   (M = S Phi^T)
//   3. i <= j only: S'[i][j] = sum_a Phi[i][a] M[a][j], a ascending, + q on the diagonal; stored to (i, j) and (j, i)
// so every S_k is symmetric bit for bit (one triangle is computed and mirrored), every sum has a fixed order, and a
// trajectory's bits depend on its own inputs alone.  The products are NX-term dot products on the VALU: at NX = 4, 6, 12
// a 16x16x4 MFMA tile would be 94, 86 and 44 % padding and the launch is bound by its T sequential steps.
#include "models.h"

namespace gpmpc {

template <int ID>
__global__ __launch_bounds__(256) void rollout_cov_kernel(RolloutCovArgs a) {
    using M = Model<ID>;
    constexpr int NX = M::NX, NU = M::NU, NGP = M::NGP, NUNC = M::NUNC, NN = NX * NX, TPB = 256 / NN;
    __shared__ double S[TPB * NN], Phi[TPB * NN], Mx[TPB * NN];
    const int slot = threadIdx.x / NN, e = threadIdx.x - slot * NN, i = e / NX, j = e - i * NX;
    const size_t p = (size_t)blockIdx.x * TPB + slot;
    const bool on = slot < TPB && p < (size_t)a.P;
    const size_t tr = on ? p : 0;
    double* Ss = S + (on ? slot : 0) * NN;
    double* Ps = Phi + (on ? slot : 0) * NN;
    double* Ms = Mx + (on ? slot : 0) * NN;
    const double* x = a.x + tr * (a.T + 1) * NX;
    const double* u = a.u + tr * a.T * NU;
    const double* A = a.A + tr * a.T * NN;
    const double* B = a.B + tr * a.T * NX * NU;
    const double* var = a.var + tr * a.T * NGP;
    double* cov = a.cov + tr * (a.T + 1) * NN;
    int unc = -1;   // this thread's entry is the diagonal entry of uncertain dimension unc
#pragma unroll
    for (int q = 0; q < NUNC; ++q)
        if (i == j && i == M::unc[q]) unc = q;
    double kcol[NU];   // column j of K
#pragma unroll
    for (int c = 0; c < NU; ++c) kcol[c] = a.closed ? a.K[c * NX + j] : 0.0;
    if (on) {
        const double s0 = a.cov0 ? a.cov0[tr * NN + e] : 0.0;
        Ss[e] = s0;
        cov[e] = s0;
    }
    const double dt2 = a.dt * a.dt;
    for (int k = 0; k < a.T; ++k) {
        double q = 0.0;
        if (on) {
            double phi = A[(size_t)k * NN + e];
            if (a.closed) {
#pragma unroll
                for (int c = 0; c < NU; ++c) phi = fma(B[(size_t)k * NX * NU + i * NU + c], kcol[c], phi);
            }
            Ps[e] = phi;
            if (unc >= 0) {
                double xk[NX], uk[NU], W[NUNC][NGP];
#pragma unroll
                for (int r = 0; r < NX; ++r) xk[r] = x[(size_t)k * NX + r];
#pragma unroll
                for (int c = 0; c < NU; ++c) uk[c] = u[(size_t)k * NU + c];
                M::var_weights(xk, uk, W);
                double acc = 0.0;
#pragma unroll
                for (int qq = 0; qq < NUNC; ++qq) {
                    if (qq != unc) continue;
#pragma unroll
                    for (int g = 0; g < NGP; ++g) acc = fma(W[qq][g], var[(size_t)k * NGP + g] + a.noise[g], acc);
                }
                q = acc * dt2;
            }
        }
        __syncthreads();   // Phi_k (and S_k) written
        if (on) {
            double m = 0.0;
#pragma unroll
            for (int bb = 0; bb < NX; ++bb) m = fma(Ss[i * NX + bb], Ps[j * NX + bb], m);
            Ms[e] = m;
        }
        __syncthreads();   // M written, S_k read
        if (on && i <= j) {
            double s = 0.0;
#pragma unroll
            for (int aa = 0; aa < NX; ++aa) s = fma(Ps[i * NX + aa], Ms[aa * NX + j], s);
            s += q;
            Ss[i * NX + j] = s;
            Ss[j * NX + i] = s;
            cov[(size_t)(k + 1) * NN + i * NX + j] = s;
            cov[(size_t)(k + 1) * NN + j * NX + i] = s;
        }
        __syncthreads();   // S_{k+1} written before the next step's reads, Phi_k read before it is replaced
    }
}

hipError_t launch_rollout_cov(int model, const RolloutCovArgs& a, hipStream_t stream) {
    auto blocks = [&](int nx) { const int tpb = 256 / (nx * nx); return dim3((unsigned)((a.P + tpb - 1) / tpb)); };
    switch (model) {
        case kQuad2D: hipLaunchKernelGGL(rollout_cov_kernel<kQuad2D>, blocks(6), dim3(256), 0, stream, a); break;
        case kQuad3D: hipLaunchKernelGGL(rollout_cov_kernel<kQuad3D>, blocks(12), dim3(256), 0, stream, a); break;
        case kCartpole: hipLaunchKernelGGL(rollout_cov_kernel<kCartpole>, blocks(4), dim3(256), 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace gpmpc
