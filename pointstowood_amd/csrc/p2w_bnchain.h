// The device code that the chained-BatchNorm entry points (p2w_bnchain.hip) and the head (p2w_head.hip) share: the column constants,
// the one-stage arithmetic, the statistics kernel, the reduction over the work items and the workspace they use.  One private
// copy per translation unit; the bits of a result do not depend on which of the two asked for it.
#pragma once
#include "p2w_runsum.h"

namespace {

constexpr int BC_MAX = P2W_BN_CHAIN_MAX;
constexpr int BC_R = P2W_BN_CHAIN_ROWS;
constexpr int BC_KMAX = 5;                // sums per column of a backward stage with a depthwise convolution
constexpr int BC_RED_U = 16;              // items per thread and batch of the reduction: 8 x 16 = 128 items per batch
constexpr int BC_RED_BATCH = 8 * BC_RED_U;

// what every kernel is given by value: the stages' column vectors ([C] each; a == nullptr: no depthwise), the statistics
// ([L, C], written by the forward's reductions) and, in the backward, k1 = dbeta / M and k2 = dgamma / M per stage ([L, 2, C])
struct BcParams {
    const float* a[BC_MAX];
    const float* b[BC_MAX];
    const float* gamma[BC_MAX];
    const float* beta[BC_MAX];
    int relu[BC_MAX];
    const float* mean;
    const float* invstd;
    const float* kq;
};

template <int V> struct BcCol { float a[V], b[V], mu[V], is[V], gm[V], bt[V]; };        // forward constants of one stage
template <int V> struct BcGrad { float sc[V], k1[V], k2[V]; };                        // backward constants: sc = gamma invstd

template <int V> __device__ __forceinline__ void bc_load(const BcParams& P, int t, int C, int c, BcCol<V>& k) {
    if (P.a[t]) { gr_ld<V>(&P.a[t][c], k.a); gr_ld<V>(&P.b[t][c], k.b); }
    else {
#pragma unroll
        for (int u = 0; u < V; ++u) { k.a[u] = 1.f; k.b[u] = 0.f; }                     // (1 u + 0 = u exactly)
    }
    gr_ld<V>(&P.mean[(size_t)t * C + c], k.mu);
    gr_ld<V>(&P.invstd[(size_t)t * C + c], k.is);
    gr_ld<V>(&P.gamma[t][c], k.gm);
    gr_ld<V>(&P.beta[t][c], k.bt);
}
template <int V> __device__ __forceinline__ void bc_load_grad(const BcParams& P, int t, int C, int c, const BcCol<V>& k, BcGrad<V>& g) {
    gr_ld<V>(&P.kq[((size_t)t * 2 + 0) * C + c], g.k1);
    gr_ld<V>(&P.kq[((size_t)t * 2 + 1) * C + c], g.k2);
#pragma unroll
    for (int u = 0; u < V; ++u) g.sc[u] = k.gm[u] * k.is[u];
}

// one stage, fp32, every operation rounded on its own: v = a u + b, xhat = (v - mean) invstd, y = xhat gamma + beta,
// u = relu ? (y < 0 ? 0 : y) : y   (a NaN stays a NaN, as torch.relu leaves it)
template <int V> __device__ __forceinline__ void bc_stage(const BcCol<V>& k, bool relu, float (&x)[V], float (&xh)[V]) {
#pragma unroll
    for (int u = 0; u < V; ++u) {
        const float v = k.a[u] * x[u] + k.b[u];
        xh[u] = (v - k.mu[u]) * k.is[u];
        const float y = xh[u] * k.gm[u] + k.bt[u];
        x[u] = relu ? (y < 0.f ? 0.f : y) : y;
    }
}
// the gradient through one stage: gy = relu ? g [u_out > 0] : g, gv = ((gy - k1) - xhat k2) sc, g = a gv
template <int V>
__device__ __forceinline__ void bc_stage_bwd(const BcCol<V>& k, const BcGrad<V>& q, bool relu, const float (&xh)[V], const float (&uo)[V],
                                             float (&g)[V]) {
#pragma unroll
    for (int u = 0; u < V; ++u) {
        const float gy = relu ? (uo[u] > 0.f ? g[u] : 0.f) : g[u];
        g[u] = (((gy - q.k1[u]) - xh[u] * q.k2[u]) * q.sc[u]) * k.a[u];
    }
}

// the leading ReLU of p2w_relu_bn: u = z < 0 ? 0 : z (a NaN stays a NaN)
template <int V> __device__ __forceinline__ void bc_pre(float (&x)[V]) {
#pragma unroll
    for (int u = 0; u < V; ++u) x[u] = x[u] < 0.f ? 0.f : x[u];
}

#define BC_ITEM_PROLOGUE()                                                     \
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;           \
    const int item = (int)(gid / q);                                           \
    if (item >= items) return;                                                 \
    const int c = (int)(gid % q) * V;                                          \
    const int r0 = item * BC_R, r1 = min(M, r0 + BC_R)

// Forward, statistics of stage S + 1 (S = the stages in front of it, recomputed): s1 = sum u_S, s2 = sum u_S^2 per item and column.
// TZ = the element type of z (float, or gr_half widened as it is loaded)
template <int V, int S, bool PRE = false, class TZ = float>
__global__ __launch_bounds__(256) void bc_stats_kernel(BcParams P, const TZ* __restrict__ z, int ldz, int M, int C, int q, int items,
                                                       double* __restrict__ part) {
    BC_ITEM_PROLOGUE();
    BcCol<V> k[S > 0 ? S : 1];
#pragma unroll
    for (int t = 0; t < S; ++t) bc_load<V>(P, t, C, c, k[t]);
    double s1[V], s2[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { s1[u] = 0.0; s2[u] = 0.0; }
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        float x[V], xh[V];
        gr_ld<V>(&z[(size_t)r * ldz + c], x);
        if constexpr (PRE) bc_pre<V>(x);
#pragma unroll
        for (int t = 0; t < S; ++t) bc_stage<V>(k[t], P.relu[t] != 0, x, xh);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const double xd = (double)x[u];
            s1[u] = s1[u] + xd;
            s2[u] = s2[u] + xd * xd;
        }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
        part[((size_t)item * 2 + 0) * C + c + u] = s1[u];
        part[((size_t)item * 2 + 1) * C + c + u] = s2[u];
    }
}

// what the reduction does with a column's K totals
struct BcFinish {
    int stats;                       // 1: forward statistics, 0: backward sums
    const float* a; const float* b;  // the stage's depthwise vectors (nullptr: none)
    const float* gamma; const float* invstd;                     // backward, K = 5
    double momentum, eps;
    float* o0; float* o1;            // mean, invstd | dgamma, dbeta
    float* running_mean; float* running_var;
    float* kq;                       // [2, C]: dbeta / M, dgamma / M
    float* ddw_w; float* ddw_b;      // backward (nullptr: the caller wants none)
    float* dw; const double* gpart; float* dbias;                // backward, K = 3 (p2w_head.hip): see below
};

// The items in ascending order.  One block per CB = 32 / K columns; lane l of 32 = (sum kind l / CB, column l % CB), the block's 8
// lane groups load BC_RED_BATCH items at a time into LDS (the next batch is in flight while this one is added), the first 32
// threads add their chain's values in item order, and the first CB threads finish their column in fp64, rounding once:
//   statistics: mean_u = s0 / M, var_u = max(s1 / M - mean_u^2, 0); mean = a mean_u + b, var = a^2 var_u with a depthwise in front;
//               invstd = 1 / sqrt(var + eps); running_mean = (1 - m) running_mean + m mean, running_var likewise with var M / (M - 1)
//   backward:   dbeta = s0, dgamma = s1, k1 = s0 / M, k2 = s1 / M,
//               ddw_w = gamma invstd (s2 - (s0 / M) s3 - (s1 / M) s4)   (= sum gv u),   ddw_b = 0 (BatchNorm removes a bias in front of it)
//   K = 3 (the head's backward): dw = s2 besides, and block 0's second wave adds gpart[items] into dbias - lane l takes the items
//               l, l + 64, ... in ascending order, then the 64 lanes in a butterfly (xor 32, 16, .. 1), fp64, rounded once
template <int K>
__global__ __launch_bounds__(256) void bc_reduce_kernel(const double* __restrict__ part, int items, int C, int M, BcFinish F) {
    constexpr int CB = 32 / K;
    __shared__ double sm[BC_RED_BATCH][32];
    __shared__ double tot[32];
    const int l = threadIdx.x & 31, sub = threadIdx.x >> 5;
    const int kind = l / CB, col = blockIdx.x * CB + l % CB;
    const bool on = kind < K && col < C;
    double v[BC_RED_U], acc = 0.0;
#pragma unroll
    for (int u = 0; u < BC_RED_U; ++u) {
        const int it = u * 8 + sub;
        v[u] = (on && it < items) ? part[((size_t)it * K + kind) * C + col] : 0.0;
    }
    for (int base = 0; base < items; base += BC_RED_BATCH) {
#pragma unroll
        for (int u = 0; u < BC_RED_U; ++u) sm[u * 8 + sub][l] = v[u];
        __syncthreads();
        if (base + BC_RED_BATCH < items) {
#pragma unroll
            for (int u = 0; u < BC_RED_U; ++u) {
                const int it = base + BC_RED_BATCH + u * 8 + sub;
                v[u] = (on && it < items) ? part[((size_t)it * K + kind) * C + col] : 0.0;
            }
        }
        if (threadIdx.x < 32) {
            const int n = min(BC_RED_BATCH, items - base);
            for (int i = 0; i < n; ++i) acc = acc + sm[i][l];
        }
        __syncthreads();
    }
    if (threadIdx.x < 32) tot[l] = acc;
    __syncthreads();
    if constexpr (K == 3) {
        if (F.dbias && blockIdx.x == 0 && (threadIdx.x >> 6) == 1) {
            double sg = 0.0;
            for (int it = threadIdx.x & 63; it < items; it += 64) sg = sg + F.gpart[it];
#pragma unroll
            for (int off = 32; off >= 1; off >>= 1) sg = sg + __shfl_xor(sg, off, 64);
            if ((threadIdx.x & 63) == 0) F.dbias[0] = (float)sg;
        }
    }
    if (threadIdx.x >= CB || !on) return;
    const double s0 = tot[l], s1 = tot[CB + l], n = (double)M;
    if (F.stats) {
        double mu = s0 / n;
        double var = s1 / n - mu * mu;
        var = var > 0.0 ? var : 0.0;
        if (F.a) {
            const double a = (double)F.a[col];
            mu = a * mu + (double)F.b[col];
            var = (a * a) * var;
        }
        F.o0[col] = (float)mu;
        F.o1[col] = (float)(1.0 / sqrt(var + F.eps));
        F.running_mean[col] = (float)((1.0 - F.momentum) * (double)F.running_mean[col] + F.momentum * mu);
        F.running_var[col] = (float)((1.0 - F.momentum) * (double)F.running_var[col] + F.momentum * (var * n / (n - 1.0)));
    } else {
        F.o0[col] = (float)s1;       // dgamma
        F.o1[col] = (float)s0;       // dbeta
        F.kq[col] = (float)(s0 / n);
        F.kq[C + col] = (float)(s1 / n);
        if (F.ddw_w) {
            double w = 0.0;
            if constexpr (K == BC_KMAX) {
                const double s2 = tot[2 * CB + l], s3 = tot[3 * CB + l], s4 = tot[4 * CB + l];
                w = ((double)F.gamma[col] * (double)F.invstd[col]) * ((s2 - (s0 / n) * s3) - (s1 / n) * s4);
            }
            F.ddw_w[col] = (float)w;
        }
        if (F.ddw_b) F.ddw_b[col] = 0.f;
        if constexpr (K == 3) {
            if (F.dw) F.dw[col] = (float)tot[2 * CB + l];
        }
    }
}

struct BcWs { double* part; float* kq; int items; };
inline BcWs bc_carve(P2wArena& a, int M, int C, int L) {
    BcWs W;
    W.items = p2w_cdiv(M, BC_R);
    W.part = a.take<double>((size_t)W.items * BC_KMAX * C);
    W.kq = a.take<float>((size_t)L * 2 * C);
    return W;
}
inline bool bc_sizes_ok(long long M, long long C, long long L) {
    return M >= 2 && C >= 1 && L >= 1 && L <= BC_MAX && M < 0x7fffffffll && M * C <= (1ll << 38) && L * C < 0x7fffffffll;
}

#define BC_GRID(items, q) (unsigned)(((long long)(items) * (q) + 255) / 256), 256, 0, s

}  // namespace
