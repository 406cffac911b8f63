// The tail of the PointNetConv edge MLP for training (model.py:198-202, pointnet.py:122): ReLU, training-mode BatchNorm1d and the
// max over every target's edges, applied to the layer-2 pre-activation Z [E, C2] without forming relu(Z), BN(relu(Z)) or their
// gradients.  Per column BatchNorm is the affine map y -> (y - mean) invstd gamma + beta, non-decreasing for gamma >= 0 and
// non-increasing for gamma < 0, so the maximum of BN(y) over a target's rows is BN of the rows' maximum of y (minimum where
// gamma < 0).  The forward therefore needs, from one read of Z, the column sums of y = relu(z) and y^2 and one extremum with its
// row per (target, column); the backward is one more read of Z and one write of dZ, BatchNorm's gradient through the batch
// statistics being a closed form in the per-column sums dbeta and dgamma.
//
// Streaming kernels, bandwidth-bound: no LDS tiles, no MFMA.  A lane owns V adjacent columns: V = 4 (16-byte accesses) when C2 and
// the pitches are multiples of 4 and the pointers are 16-byte aligned, V = 1 (4-byte accesses) otherwise.  Every sum is taken per
// column by one lane in ascending row order, so the bits do not depend on V, on the grid or on the run: no floating-point atomics.
//   sums:  fp64 partials per work item of P2W_BN_GROUP consecutive targets (rows ascending), then the items in ascending order
//          (bnmax_reduce_kernel: the loads of 128 items are in flight together, one lane per column adds them in order).
// Z and dZ also come in float16 and bfloat16 (p2w_relu_bn_max_io / _bwd_io; TZ = gr_half or gr_bf16, p2w_runsum.h): the element is
// widened as it is loaded (exact) and dz rounded once as it is stored (gr_f2h / gr_f2b); V = 4 is then one 8-byte access on z / dz.
// Everything between the load and the store is the fp32 code, so ext, arg, the sums and out are the fp32 entry point's on the
// widened tensor bit for bit, and dz is its fp32 dz rounded once.
#include "p2w_runsum.h"

namespace {

constexpr int BN_G = P2W_BN_GROUP;
constexpr int RED_COLS = 16;           // columns per block of the reduction: 16 x (two sums) = 32 chains
constexpr int RED_U = 16;              // items per thread and batch: 8 x 16 = 128 items per batch
constexpr int RED_BATCH = 8 * RED_U;

__device__ __forceinline__ int bn_clamp(int v, int E) { return max(0, min(v, E)); }

// Forward, first launch: one lane per (item of BN_G consecutive targets, V columns).  The item's rows are consecutive; the lane walks
// them once in ascending order, adds y and y * y in fp64 (y * y is exact in fp64) and keeps the extremum of the current target with the
// lowest row that holds it (strict comparison on an ascending walk).  ptr is clamped to [0, E] and made non-decreasing, so no bad
// offset reaches an address.  A NaN in z counts as a non-positive value (y = 0).
template <int V, class TZ>
__global__ __launch_bounds__(256) void bnmax_part_kernel(const TZ* __restrict__ z, int ldz, const int* __restrict__ ptr,
                                                         const float* __restrict__ gamma, int M, int E, int C2, int q, int items,
                                                         float* __restrict__ ext, int* __restrict__ arg, double* __restrict__ part) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int item = (int)(gid / q);
    if (item >= items) return;
    const int c = (int)(gid % q) * V;
    const int t0 = item * BN_G, t1 = min(M, t0 + BN_G);
    float gm[V];
    gr_ld<V>(&gamma[c], gm);
    double s1[V], s2[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { s1[u] = 0.0; s2[u] = 0.0; }
    int r = bn_clamp(ptr[t0], E);
    for (int t = t0; t < t1; ++t) {
        const int e = max(r, bn_clamp(ptr[t + 1], E));
        float best[V]; int a[V];
#pragma unroll
        for (int u = 0; u < V; ++u) { best[u] = 0.f; a[u] = -1; }
#pragma unroll 8
        for (; r < e; ++r) {
            float v[V];
            gr_ld<V>(&z[(size_t)r * ldz + c], v);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float y = v[u] > 0.f ? v[u] : 0.f;
                const double yd = (double)y;
                s1[u] = s1[u] + yd;
                s2[u] = s2[u] + yd * yd;
                const bool better = gm[u] < 0.f ? y < best[u] : y > best[u];
                if (a[u] < 0 || better) { best[u] = y; a[u] = r; }
            }
        }
        gr_st<V>(&ext[(size_t)t * C2 + c], best);
        gr_st<V>(&arg[(size_t)t * C2 + c], a);
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
        part[((size_t)item * 2 + 0) * C2 + c + u] = s1[u];
        part[((size_t)item * 2 + 1) * C2 + c + u] = s2[u];
    }
}

// Backward, first launch: the same items over g, ext and arg [M, C2]: s1 = sum g, s2 = sum g xhat(ext) over the non-empty targets,
// xhat(ext) = (ext - mean) invstd in fp64 on the fp32 mean and invstd of the forward.
template <int V>
__global__ __launch_bounds__(256) void bnmax_bwd_part_kernel(const float* __restrict__ g, const float* __restrict__ ext,
                                                             const int* __restrict__ arg, const float* __restrict__ mean,
                                                             const float* __restrict__ invstd, int M, int C2, int q, int items,
                                                             double* __restrict__ part) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    const int item = (int)(gid / q);
    if (item >= items) return;
    const int c = (int)(gid % q) * V;
    const int t0 = item * BN_G, t1 = min(M, t0 + BN_G);
    float mu[V], is[V];
    gr_ld<V>(&mean[c], mu);
    gr_ld<V>(&invstd[c], is);
    double s1[V], s2[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { s1[u] = 0.0; s2[u] = 0.0; }
#pragma unroll 4
    for (int t = t0; t < t1; ++t) {
        float gv[V], ev[V]; int a[V];
        gr_ld<V>(&g[(size_t)t * C2 + c], gv);
        gr_ld<V>(&ext[(size_t)t * C2 + c], ev);
        gr_ld<V>(&arg[(size_t)t * C2 + c], a);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            if (a[u] >= 0) {
                const double gd = (double)gv[u];
                s1[u] = s1[u] + gd;
                s2[u] = s2[u] + gd * (((double)ev[u] - (double)mu[u]) * (double)is[u]);
            }
        }
    }
#pragma unroll
    for (int u = 0; u < V; ++u) {
        part[((size_t)item * 2 + 0) * C2 + c + u] = s1[u];
        part[((size_t)item * 2 + 1) * C2 + c + u] = s2[u];
    }
}

// Second launch of both directions: the items in ascending order.  One block per RED_COLS columns; lane l of 32 = (sum kind, column),
// the block's 8 lane groups load RED_BATCH items at a time into LDS (the next batch is in flight while this one is added), and the
// first 32 threads add their column's values in item order.  Then the block's first RED_COLS threads finish their column:
//   forward (stats = true):  mean = s1 / E, var = max(s2 / E - mean^2, 0), invstd = 1 / sqrt(var + eps), all in fp64, rounded once;
//                            running_mean = (1 - m) running_mean + m mean, running_var = (1 - m) running_var + m var E / (E - 1)
//   backward:                o0 = dgamma = s2, o1 = dbeta = s1, kq[0][c] = s1 / E, kq[1][c] = s2 / E (rounded once from fp64)
__global__ __launch_bounds__(256) void bnmax_reduce_kernel(const double* __restrict__ part, int items, int C2, int E, bool stats,
                                                           double momentum, double eps, float* __restrict__ o0, float* __restrict__ o1,
                                                           float* __restrict__ running_mean, float* __restrict__ running_var,
                                                           float* __restrict__ kq) {
    __shared__ double sm[RED_BATCH][32];
    __shared__ double tot[32];
    const int l = threadIdx.x & 31, sub = threadIdx.x >> 5;
    const int kind = l >> 4, col = blockIdx.x * RED_COLS + (l & 15);
    const bool on = col < C2;
    double v[RED_U], acc = 0.0;
#pragma unroll
    for (int u = 0; u < RED_U; ++u) {
        const int it = u * 8 + sub;
        v[u] = (on && it < items) ? part[((size_t)it * 2 + kind) * C2 + col] : 0.0;
    }
    for (int base = 0; base < items; base += RED_BATCH) {
#pragma unroll
        for (int u = 0; u < RED_U; ++u) sm[u * 8 + sub][l] = v[u];
        __syncthreads();
        if (base + RED_BATCH < items) {
#pragma unroll
            for (int u = 0; u < RED_U; ++u) {
                const int it = base + RED_BATCH + u * 8 + sub;
                v[u] = (on && it < items) ? part[((size_t)it * 2 + kind) * C2 + col] : 0.0;
            }
        }
        if (threadIdx.x < 32) {
            const int n = min(RED_BATCH, items - base);
            for (int i = 0; i < n; ++i) acc = acc + sm[i][l];
        }
        __syncthreads();
    }
    if (threadIdx.x < 32) tot[l] = acc;
    __syncthreads();
    if (threadIdx.x >= RED_COLS || !on) return;
    const double s1 = tot[l], s2 = tot[l + 16], n = (double)E;
    if (stats) {
        const double mu = s1 / n;
        double var = s2 / n - mu * mu;
        var = var > 0.0 ? var : 0.0;
        o0[col] = (float)mu;
        o1[col] = (float)(1.0 / sqrt(var + eps));
        running_mean[col] = (float)((1.0 - momentum) * (double)running_mean[col] + momentum * mu);
        running_var[col] = (float)((1.0 - momentum) * (double)running_var[col] + momentum * (var * n / (n - 1.0)));
    } else {
        o0[col] = (float)s2;       // dgamma
        o1[col] = (float)s1;       // dbeta
        kq[col] = (float)(s1 / n);
        kq[C2 + col] = (float)(s2 / n);
    }
}

// Forward, third launch: out = ((ext - mean) invstd) gamma + beta per (target, V columns), 0 for a target without rows.
template <int V>
__global__ __launch_bounds__(256) void bnmax_apply_kernel(const float* __restrict__ ext, const int* __restrict__ arg,
                                                          const float* __restrict__ mean, const float* __restrict__ invstd,
                                                          const float* __restrict__ gamma, const float* __restrict__ beta, int M, int C2,
                                                          int q, float* __restrict__ out) {
    const long long gid = (long long)blockIdx.x * 256 + threadIdx.x;
    if (gid >= (long long)M * q) return;
    const int t = (int)(gid / q), c = (int)(gid % q) * V;
    float ev[V], mu[V], is[V], gm[V], bt[V], o[V]; int a[V];
    gr_ld<V>(&ext[(size_t)t * C2 + c], ev);
    gr_ld<V>(&arg[(size_t)t * C2 + c], a);
    gr_ld<V>(&mean[c], mu); gr_ld<V>(&invstd[c], is); gr_ld<V>(&gamma[c], gm); gr_ld<V>(&beta[c], bt);
#pragma unroll
    for (int u = 0; u < V; ++u) o[u] = a[u] >= 0 ? ((ev[u] - mu[u]) * is[u]) * gm[u] + bt[u] : 0.f;
    gr_st<V>(&out[(size_t)t * C2 + c], o);
}

// Backward, third launch: one block per item of BN_G targets, whose rows are consecutive.  The item's offsets go to LDS; W lanes cover a
// row pass (W V columns), the block's 256 / W row lanes take rows rl, rl + 256 / W, ...; a row's target is found by bisection in LDS.
//   xhat = (y - mean) invstd,  dy = ((g[e == arg] - k1) - xhat k2) (gamma invstd),  dz = z > 0 ? dy : 0          (fp32, no fma)
// with k1 = dbeta / E and k2 = dgamma / E from the reduction.  Every element of the rows [ptr[0], ptr[M]) is written once.
template <int V, class TZ>
__global__ __launch_bounds__(256) void bnmax_dz_kernel(const float* __restrict__ g, const TZ* __restrict__ z, int ldz,
                                                       const int* __restrict__ ptr, const int* __restrict__ arg,
                                                       const float* __restrict__ mean, const float* __restrict__ invstd,
                                                       const float* __restrict__ gamma, const float* __restrict__ kq, int M, int E, int C2,
                                                       int W, TZ* __restrict__ dz, int lddz) {
    __shared__ int sp[BN_G + 1];
    const int t0 = blockIdx.x * BN_G, nt = min(BN_G, M - t0);
    if (threadIdx.x == 0) {
        int prev = bn_clamp(ptr[t0], E);
        sp[0] = prev;
        for (int i = 1; i <= nt; ++i) { prev = max(prev, bn_clamp(ptr[t0 + i], E)); sp[i] = prev; }
    }
    __syncthreads();
    const int r0 = sp[0], r1 = sp[nt];
    const int cl = threadIdx.x & (W - 1), rl = threadIdx.x / W, R = 256 / W;
    for (int c = cl * V; c < C2; c += W * V) {
        float mu[V], is[V], gm[V], k1[V], k2[V], sc[V];
        gr_ld<V>(&mean[c], mu); gr_ld<V>(&invstd[c], is); gr_ld<V>(&gamma[c], gm);
        gr_ld<V>(&kq[c], k1); gr_ld<V>(&kq[C2 + c], k2);
#pragma unroll
        for (int u = 0; u < V; ++u) sc[u] = gm[u] * is[u];
#pragma unroll 2
        for (int r = r0 + rl; r < r1; r += R) {
            int lo = 0, hi = nt;                                // the last target whose first row is <= r
            while (hi - lo > 1) {
                const int mid = (lo + hi) >> 1;
                if (sp[mid] <= r) lo = mid; else hi = mid;
            }
            const size_t trow = (size_t)(t0 + lo) * C2 + c;
            float zv[V], gv[V], o[V]; int a[V];
            gr_ld<V>(&z[(size_t)r * ldz + c], zv);
            gr_ld<V>(&arg[trow], a);
            gr_ld<V>(&g[trow], gv);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float y = zv[u] > 0.f ? zv[u] : 0.f;
                const float xhat = (y - mu[u]) * is[u];
                const float gi = a[u] == r ? gv[u] : 0.f;
                const float dy = ((gi - k1[u]) - xhat * k2[u]) * sc[u];
                o[u] = zv[u] > 0.f ? dy : 0.f;
            }
            gr_st<V>(&dz[(size_t)r * lddz + c], o);
        }
    }
}

struct BmWs { double* part; float* kq; int items; };
inline BmWs bm_carve(P2wArena& a, int M, int C2) {
    BmWs W;
    W.items = p2w_cdiv(M, BN_G);
    W.part = a.take<double>((size_t)W.items * 2 * C2);
    W.kq = a.take<float>((size_t)2 * C2);
    return W;
}
inline bool bm_sizes_ok(long long E, long long M, long long C2) {
    return E >= 2 && M >= 1 && C2 >= 1 && E < 0x7fffffffll && M < 0x7fffffffll && M * C2 <= (1ll << 38);     // (grids of M C2 / 4 / 256 blocks)
}

}  // namespace

extern "C" size_t p2w_relu_bn_max_ws_bytes(int32_t E, int32_t M, int32_t C2) {
    if (!bm_sizes_ok(E, M, C2)) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { bm_carve(a, M, C2); });
}

namespace {

template <class TZ>
int32_t bnmax_fwd_t(const TZ* z, int32_t ldz, const int32_t* ptr, const float* gamma, const float* beta, float* running_mean,
                    float* running_var, double momentum, double eps, int32_t E, int32_t M, int32_t C2, float* out, float* ext, int32_t* arg,
                    float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (!bm_sizes_ok(E, M, C2) || ldz < C2 || !(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return P2W_EINVAL;
    P2W_CHECK_PTR(z); P2W_CHECK_PTR(ptr); P2W_CHECK_PTR(gamma); P2W_CHECK_PTR(beta); P2W_CHECK_PTR(running_mean); P2W_CHECK_PTR(running_var);
    P2W_CHECK_PTR(out); P2W_CHECK_PTR(ext); P2W_CHECK_PTR(arg); P2W_CHECK_PTR(mean); P2W_CHECK_PTR(invstd); P2W_CHECK_PTR(ws);
    P2W_CHECK_ALIGN16(ws);
    P2wArena arena(ws);
    const BmWs L = bm_carve(arena, M, C2);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    const bool v4 = !(C2 & 3) && !(ldz & 3) && gr_alv(z) && gr_al16(gamma) && gr_al16(beta) && gr_al16(out) && gr_al16(ext) && gr_al16(arg) &&
                    gr_al16(mean) && gr_al16(invstd);
    hipStream_t s = p2w_s(stream);
    const int q = v4 ? C2 >> 2 : C2;
    const unsigned pb = (unsigned)(((long long)L.items * q + 255) / 256), ab = (unsigned)(((long long)M * q + 255) / 256);
    if (v4) bnmax_part_kernel<4, TZ><<<pb, 256, 0, s>>>(z, ldz, ptr, gamma, M, E, C2, q, L.items, ext, arg, L.part);
    else bnmax_part_kernel<1, TZ><<<pb, 256, 0, s>>>(z, ldz, ptr, gamma, M, E, C2, q, L.items, ext, arg, L.part);
    bnmax_reduce_kernel<<<p2w_cdiv(C2, RED_COLS), 256, 0, s>>>(L.part, L.items, C2, E, true, momentum, eps, mean, invstd, running_mean,
                                                               running_var, nullptr);
    if (v4) bnmax_apply_kernel<4><<<ab, 256, 0, s>>>(ext, arg, mean, invstd, gamma, beta, M, C2, q, out);
    else bnmax_apply_kernel<1><<<ab, 256, 0, s>>>(ext, arg, mean, invstd, gamma, beta, M, C2, q, out);
    return P2W_LAUNCH_STATUS();
}

template <class TZ>
int32_t bnmax_bwd_t(const float* g, const TZ* z, int32_t ldz, const int32_t* ptr, const int32_t* arg, const float* ext, const float* mean,
                    const float* invstd, const float* gamma, int32_t E, int32_t M, int32_t C2, TZ* dz, int32_t lddz, float* dgamma, float* dbeta,
                    void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (!bm_sizes_ok(E, M, C2) || ldz < C2 || lddz < C2) return P2W_EINVAL;
    P2W_CHECK_PTR(g); P2W_CHECK_PTR(z); P2W_CHECK_PTR(ptr); P2W_CHECK_PTR(arg); P2W_CHECK_PTR(ext); P2W_CHECK_PTR(mean); P2W_CHECK_PTR(invstd);
    P2W_CHECK_PTR(gamma); P2W_CHECK_PTR(dz); P2W_CHECK_PTR(dgamma); P2W_CHECK_PTR(dbeta); P2W_CHECK_PTR(ws);
    P2W_CHECK_ALIGN16(ws);
    P2wArena arena(ws);
    const BmWs L = bm_carve(arena, M, C2);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    const bool v4 = !(C2 & 3) && !(ldz & 3) && !(lddz & 3) && gr_al16(g) && gr_alv(z) && gr_al16(arg) && gr_al16(ext) && gr_al16(mean) &&
                    gr_al16(invstd) && gr_al16(gamma) && gr_alv(dz);
    hipStream_t s = p2w_s(stream);
    const int q = v4 ? C2 >> 2 : C2;
    const unsigned pb = (unsigned)(((long long)L.items * q + 255) / 256);
    if (v4) bnmax_bwd_part_kernel<4><<<pb, 256, 0, s>>>(g, ext, arg, mean, invstd, M, C2, q, L.items, L.part);
    else bnmax_bwd_part_kernel<1><<<pb, 256, 0, s>>>(g, ext, arg, mean, invstd, M, C2, q, L.items, L.part);
    bnmax_reduce_kernel<<<p2w_cdiv(C2, RED_COLS), 256, 0, s>>>(L.part, L.items, C2, E, false, 0.0, 0.0, dgamma, dbeta, nullptr, nullptr, L.kq);
    if (v4) bnmax_dz_kernel<4, TZ><<<L.items, 256, 0, s>>>(g, z, ldz, ptr, arg, mean, invstd, gamma, L.kq, M, E, C2, run_row_lanes<4>(C2), dz, lddz);
    else bnmax_dz_kernel<1, TZ><<<L.items, 256, 0, s>>>(g, z, ldz, ptr, arg, mean, invstd, gamma, L.kq, M, E, C2, run_row_lanes<1>(C2), dz, lddz);
    return P2W_LAUNCH_STATUS();
}

}  // namespace

// z by its dtype code (include/p2w.h: P2W_F32, P2W_F16, P2W_BF16); an unknown code is refused before anything else is looked at
extern "C" int32_t p2w_relu_bn_max_io(const void* z, int32_t tz, int32_t ldz, const int32_t* ptr, const float* gamma, const float* beta,
                                      float* running_mean, float* running_var, double momentum, double eps, int32_t E, int32_t M, int32_t C2,
                                      float* out, float* ext, int32_t* arg, float* mean, float* invstd, void* ws, size_t ws_bytes,
                                      p2w_stream_t stream) {
    if (tz == P2W_F32)
        return bnmax_fwd_t(static_cast<const float*>(z), ldz, ptr, gamma, beta, running_mean, running_var, momentum, eps, E, M, C2, out, ext,
                           arg, mean, invstd, ws, ws_bytes, stream);
    if (tz == P2W_F16)
        return bnmax_fwd_t(static_cast<const gr_half*>(z), ldz, ptr, gamma, beta, running_mean, running_var, momentum, eps, E, M, C2, out, ext,
                           arg, mean, invstd, ws, ws_bytes, stream);
    if (tz == P2W_BF16)
        return bnmax_fwd_t(static_cast<const gr_bf16*>(z), ldz, ptr, gamma, beta, running_mean, running_var, momentum, eps, E, M, C2, out, ext,
                           arg, mean, invstd, ws, ws_bytes, stream);
    return P2W_EUNSUPPORTED;
}

extern "C" int32_t p2w_relu_bn_max(const float* z, int32_t ldz, const int32_t* ptr, const float* gamma, const float* beta,
                                   float* running_mean, float* running_var, double momentum, double eps, int32_t E, int32_t M, int32_t C2,
                                   float* out, float* ext, int32_t* arg, float* mean, float* invstd, void* ws, size_t ws_bytes,
                                   p2w_stream_t stream) {
    return p2w_relu_bn_max_io(z, P2W_F32, ldz, ptr, gamma, beta, running_mean, running_var, momentum, eps, E, M, C2, out, ext, arg, mean, invstd,
                              ws, ws_bytes, stream);
}

extern "C" int32_t p2w_relu_bn_max_bwd_io(const float* g, const void* z, int32_t tz, int32_t ldz, const int32_t* ptr, const int32_t* arg,
                                          const float* ext, const float* mean, const float* invstd, const float* gamma, int32_t E, int32_t M,
                                          int32_t C2, void* dz, int32_t lddz, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                                          p2w_stream_t stream) {
    if (tz == P2W_F32)
        return bnmax_bwd_t(g, static_cast<const float*>(z), ldz, ptr, arg, ext, mean, invstd, gamma, E, M, C2, static_cast<float*>(dz), lddz,
                           dgamma, dbeta, ws, ws_bytes, stream);
    if (tz == P2W_F16)
        return bnmax_bwd_t(g, static_cast<const gr_half*>(z), ldz, ptr, arg, ext, mean, invstd, gamma, E, M, C2, static_cast<gr_half*>(dz), lddz,
                           dgamma, dbeta, ws, ws_bytes, stream);
    if (tz == P2W_BF16)
        return bnmax_bwd_t(g, static_cast<const gr_bf16*>(z), ldz, ptr, arg, ext, mean, invstd, gamma, E, M, C2, static_cast<gr_bf16*>(dz), lddz,
                           dgamma, dbeta, ws, ws_bytes, stream);
    return P2W_EUNSUPPORTED;
}

extern "C" int32_t p2w_relu_bn_max_bwd(const float* g, const float* z, int32_t ldz, const int32_t* ptr, const int32_t* arg, const float* ext,
                                       const float* mean, const float* invstd, const float* gamma, int32_t E, int32_t M, int32_t C2,
                                       float* dz, int32_t lddz, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    return p2w_relu_bn_max_bwd_io(g, z, P2W_F32, ldz, ptr, arg, ext, mean, invstd, gamma, E, M, C2, dz, lddz, dgamma, dbeta, ws, ws_bytes, stream);
}
