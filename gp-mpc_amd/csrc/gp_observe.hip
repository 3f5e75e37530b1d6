// GP training rows from transitions on the device (gpmpc_preprocess, gpmpc_gp_informative, gpmpc_gp_observe): the
// device restatement of GPMPC.preprocess_data (gpmpc/gpmpc.py, the reference's gpmpc/gpmpc.py:113-151) and the
// counting rank of the points' variance scores.  One thread per output row; nothing here synchronises the host.
#include "gpmpc_common.h"
#include "models.h"

#include <cmath>

namespace gpmpc {

namespace {

constexpr int kObserveThreads = 64;

// Row r of the outputs from transition pick[r]: the GP inputs z[gp_src_g] of z = [x; u] in GP order, and per GP the
// target.  x_dot = (x_next - x) / dt_diff; the quadrotors' thrust target is the norm of x_dot's velocity components
// with gravity added to the z-component, minus the prior thrust map a u_0 + b; their rate targets and cartpole's two
// targets are x_dot_j - f_j(x, u) with f the prior (Model<ID>::f at zero GP means).
template <int ID>
__global__ void gp_observe_kernel(const GPObserve a) {
    using M = Model<ID>;
    constexpr int NX = M::NX, NU = M::NU, NGP = M::NGP;
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= a.m) return;
    const int src = a.pick != nullptr ? a.pick[r] : r;
    const bool live = src >= 0 && src < a.P;   // (an index outside the transitions reads nothing)
    const bool want_y = a.targets != nullptr || a.yg[0] != nullptr;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double z[NX + NU], y[NGP];
#pragma unroll
    for (int i = 0; i < NX + NU; ++i) z[i] = nan;
#pragma unroll
    for (int g = 0; g < NGP; ++g) y[g] = nan;
    if (live) {
#pragma unroll
        for (int i = 0; i < NX; ++i) z[i] = a.x[(size_t)src * NX + i];
#pragma unroll
        for (int i = 0; i < NU; ++i) z[NX + i] = a.u[(size_t)src * NU + i];
    }
    if (live && want_y) {
        double xd[NX], f[NX];
#pragma unroll
        for (int i = 0; i < NX; ++i) xd[i] = (a.xnext[(size_t)src * NX + i] - z[i]) / a.dt_diff;
        const double gm[kMaxGP] = {0.0, 0.0, 0.0, 0.0};
        M::f(a.params, z, z + NX, gm, f);
        if constexpr (ID == kQuad2D) {
            const double vz = xd[3] + a.gravity;
            y[0] = sqrt(xd[1] * xd[1] + vz * vz) - (a.params[0] * z[NX] + a.params[1]);
            y[1] = xd[5] - f[5];
        } else if constexpr (ID == kQuad3D) {
            const double vz = xd[5] + a.gravity;
            y[0] = sqrt(xd[1] * xd[1] + xd[3] * xd[3] + vz * vz) - (a.params[0] * z[NX] + a.params[1]);
            y[1] = xd[6] - f[6];
            y[2] = xd[7] - f[7];
        } else {
            y[0] = xd[1] - f[1];
            y[1] = xd[3] - f[3];
        }
    }
    int D = 0;
#pragma unroll
    for (int g = 0; g < NGP; ++g) D += M::gp_dim[g];
    int col = 0;
#pragma unroll
    for (int g = 0; g < NGP; ++g) {
        const int d = M::gp_dim[g];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (k < d) {
                const double v = z[M::gp_src[g][k]];
                if (a.inputs != nullptr) a.inputs[(size_t)r * D + col + k] = v;
                if (a.Xg[g] != nullptr) a.Xg[g][(size_t)r * d + k] = v;
            }
        }
        col += d;
        if (a.targets != nullptr) a.targets[(size_t)r * NGP + g] = y[g];
        if (a.yg[g] != nullptr) a.yg[g][r] = y[g];
    }
}

__global__ void gp_score_kernel(const GPRank a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.P) return;
    double s = a.var[i] / a.sf2[0];
    for (int g = 1; g < a.n_gp; ++g) {
        const double t = a.var[(size_t)g * a.ldv + i] / a.sf2[g];
        if (t > s || t != t) s = t;   // (a NaN stays: nothing compares above it)
    }
    bool finite = true;
    for (int k = 0; k < a.ldz; ++k) finite = finite && isfinite(a.Z[(size_t)i * a.ldz + k]);
    if (!finite) s = __longlong_as_double(0x7ff8000000000000ll);
    a.score[i] = s;
    if (a.score_out != nullptr) a.score_out[i] = s;
}

// rank_i = #{j : s_j beats s_i}, a permutation of 0 .. P-1, so every slot of pick below m is written exactly once
__global__ void gp_rank_kernel(const GPRank a) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= a.P) return;
    const double si = a.score[i];
    const bool fi = isfinite(si);
    int rank = 0;
    for (int j = 0; j < a.P; ++j) {
        const double sj = a.score[j];
        const bool fj = isfinite(sj);
        bool beats;
        if (fi != fj) beats = fj;
        else if (fi && sj != si) beats = sj > si;
        else beats = j < i;
        rank += beats ? 1 : 0;
    }
    if (rank < a.m) a.pick[rank] = i;
}

}  // namespace

hipError_t launch_gp_observe(const GPObserve& a, hipStream_t stream) {
    const dim3 grid((a.m + kObserveThreads - 1) / kObserveThreads), block(kObserveThreads);
    switch (a.model) {
        case kQuad2D: hipLaunchKernelGGL(gp_observe_kernel<kQuad2D>, grid, block, 0, stream, a); break;
        case kQuad3D: hipLaunchKernelGGL(gp_observe_kernel<kQuad3D>, grid, block, 0, stream, a); break;
        case kCartpole: hipLaunchKernelGGL(gp_observe_kernel<kCartpole>, grid, block, 0, stream, a); break;
        default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_gp_score_rank(const GPRank& a, hipStream_t stream) {
    const dim3 grid((a.P + kObserveThreads - 1) / kObserveThreads), block(kObserveThreads);
    hipLaunchKernelGGL(gp_score_kernel, grid, block, 0, stream, a);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(gp_rank_kernel, grid, block, 0, stream, a);
    return hipGetLastError();
}

}  // namespace gpmpc
