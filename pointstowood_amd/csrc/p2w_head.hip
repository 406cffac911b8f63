// The tail of the network's head for training with one class (model.py:241-243 behind conv1): training-mode BatchNorm1d of the
// pre-activation Z [M, C], ReLU and the 1 x C convolution, as one operator:
//     logit[r] = sum_c w[c] u[r, c] + bias,   u = relu(BN(z)).
// Neither u nor its gradient is ever stored.  The statistics are the one-stage chain's own (p2w_bnchain.h: bc_stats_kernel with no
// stage in front, bc_reduce_kernel), and u, xhat and dz come from bc_stage / bc_stage_bwd, so everything that p2w_bn_chain (L = 1,
// ReLU) also computes has its bits.
//
// Streaming kernels, bandwidth-bound: no LDS tiles, no MFMA, no floating-point atomics.
//   forward, third launch (hd_rowdot_kernel): one wave per HD_ROWS consecutive rows.  Lane l owns the columns 256 p + 4 l + e
//     (e = 0 .. 3) of pass p = 0 .. ceil(C / 256) - 1; its column constants of a pass stay in registers while it walks the rows.
//     THE SUMMATION ORDER of a row, a function of C alone: every lane starts at +0 and adds fl(w[c] u[r, c]) for its columns c < C in
//     ascending order (pass by pass, e = 0 .. 3; a lane without a column keeps +0); then the 64 lanes are added in a butterfly,
//     partner lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1 (fp32 addition commutes, so every lane holds the same bits); then + bias.
//     V = 4 loads a lane's four columns in one 16-byte access, V = 1 in four 4-byte accesses with a bound check each: the same
//     columns per lane, the same order, the same bits.
//   backward: the chain's scheme - a lane owns V adjacent columns and walks the P2W_BN_CHAIN_ROWS rows of its work item in ascending
//     order, fp64 partials per item, the items in ascending order.  The gradient of u is fl(g[r] w[c]), formed in registers from the
//     M floats of g.
//   TZ = the element type of z and dz (p2w_bn_relu_rowdot_io / _bwd_io): float, or gr_half widened on load and rounded to nearest even
//     on store (p2w_runsum.h: gr_ld, gr_f2h), or gr_bf16 likewise (gr_f2b; p2w_bn_relu_rowdot_bf16 / _bwd_bf16); the logits, their gradient and every sum are what they are for float.
#include "p2w_bnchain.h"

namespace {

constexpr int HD_ROWS = 16;      // rows per wave of the forward

template <int V, class TZ>
__global__ __launch_bounds__(256) void hd_rowdot_kernel(BcParams P, const float* __restrict__ w, const float* __restrict__ bias,
                                                        const TZ* __restrict__ z, int ldz, int M, int C, float* __restrict__ logit) {
    const int lane = threadIdx.x & 63;
    const long long first = ((long long)blockIdx.x * 4 + (threadIdx.x >> 6)) * HD_ROWS;
    if (first >= M) return;
    const int r0 = (int)first, nr = min(HD_ROWS, M - r0);
    float acc[HD_ROWS];
#pragma unroll
    for (int j = 0; j < HD_ROWS; ++j) acc[j] = 0.f;
    for (int c = lane * 4; c < C; c += 256) {
        BcCol<4> k;
        float wv[4];
        if constexpr (V == 4) {
            bc_load<4>(P, 0, C, c, k);
            gr_ld<4>(&w[c], wv);
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const bool in = c + e < C;
                k.a[e] = 1.f; k.b[e] = 0.f;
                k.mu[e] = in ? P.mean[c + e] : 0.f;
                k.is[e] = in ? P.invstd[c + e] : 0.f;
                k.gm[e] = in ? P.gamma[0][c + e] : 0.f;
                k.bt[e] = in ? P.beta[0][c + e] : 0.f;
                wv[e] = in ? w[c + e] : 0.f;
            }
        }
#pragma unroll
        for (int j = 0; j < HD_ROWS; ++j) {
            if (j < nr) {
                float x[4], xh[4];
                const TZ* row = &z[(size_t)(r0 + j) * ldz + c];
                if constexpr (V == 4) gr_ld<4>(row, x);
                else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) x[e] = c + e < C ? (float)row[e] : 0.f;
                }
                bc_stage<4>(k, true, x, xh);
#pragma unroll
                for (int e = 0; e < 4; ++e)
                    if (V == 4 || c + e < C) acc[j] = acc[j] + wv[e] * x[e];
            }
        }
    }
    const float b = bias[0];
    float mine = 0.f;
#pragma unroll
    for (int j = 0; j < HD_ROWS; ++j) {
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) acc[j] = acc[j] + __shfl_xor(acc[j], off, 64);
        if (lane == j) mine = acc[j];
    }
    if (lane < nr) logit[r0 + lane] = mine + b;
}

// Backward, the sums: per item and column s0 = sum gy, s1 = sum gy xhat, s2 = sum g u with gy = fl(g[r] w[c]) [u > 0] - fp64 terms on
// the fp32 values; the item's sum of g (fp64) from the lane of its column 0
template <int V, class TZ>
__global__ __launch_bounds__(256) void hd_bwd_sums_kernel(BcParams P, const float* __restrict__ w, const float* __restrict__ g,
                                                          const TZ* __restrict__ z, int ldz, int M, int C, int q, int items,
                                                          double* __restrict__ part, double* __restrict__ gpart) {
    BC_ITEM_PROLOGUE();
    BcCol<V> k;
    bc_load<V>(P, 0, C, c, k);
    float wv[V];
    gr_ld<V>(&w[c], wv);
    double s[3][V], sg = 0.0;
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int u = 0; u < V; ++u) s[j][u] = 0.0;
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        float x[V], xh[V];
        gr_ld<V>(&z[(size_t)r * ldz + c], x);
        const float gs = g[r];
        bc_stage<V>(k, true, x, xh);
        sg = sg + (double)gs;
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const float gw = gs * wv[u];
            const float gy = x[u] > 0.f ? gw : 0.f;
            const double gd = (double)gy;
            s[0][u] = s[0][u] + gd;
            s[1][u] = s[1][u] + gd * (double)xh[u];
            s[2][u] = s[2][u] + (double)gs * (double)x[u];
        }
    }
#pragma unroll
    for (int j = 0; j < 3; ++j)
#pragma unroll
        for (int u = 0; u < V; ++u) part[((size_t)item * 3 + j) * C + c + u] = s[j][u];
    if (c == 0) gpart[item] = sg;
}

// Backward, last launch: dz = the gradient fl(g[r] w[c]) through the ReLU and the BatchNorm (bc_stage_bwd)
template <int V, class TZ>
__global__ __launch_bounds__(256) void hd_dz_kernel(BcParams P, const float* __restrict__ w, const float* __restrict__ g,
                                                    const TZ* __restrict__ z, int ldz, int M, int C, int q, int items,
                                                    TZ* __restrict__ dz, int lddz) {
    BC_ITEM_PROLOGUE();
    BcCol<V> k;
    BcGrad<V> kg;
    bc_load<V>(P, 0, C, c, k);
    bc_load_grad<V>(P, 0, C, c, k, kg);
    float wv[V];
    gr_ld<V>(&w[c], wv);
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        float x[V], xh[V], gg[V];
        gr_ld<V>(&z[(size_t)r * ldz + c], x);
        const float gs = g[r];
        bc_stage<V>(k, true, x, xh);
#pragma unroll
        for (int u = 0; u < V; ++u) gg[u] = gs * wv[u];
        bc_stage_bwd<V>(k, kg, true, xh, x, gg);
        gr_st<V>(&dz[(size_t)r * lddz + c], gg);
    }
}

struct HdWs { BcWs bc; double* gpart; };
inline HdWs hd_carve(P2wArena& a, int M, int C) {
    HdWs W;
    W.bc = bc_carve(a, M, C, 1);
    W.gpart = a.take<double>((size_t)W.bc.items);
    return W;
}

inline BcParams hd_params(const float* gamma, const float* beta, const float* mean, const float* invstd, const float* kq) {
    BcParams P{};
    P.gamma[0] = gamma; P.beta[0] = beta; P.relu[0] = 1;
    P.mean = mean; P.invstd = invstd; P.kq = kq;
    return P;
}

template <int V, class TZ> void hd_forward(const BcParams& P, const float* w, const float* bias, const TZ* z, int ldz, int M, int C, float* running_mean,
                                 float* running_var, double momentum, double eps, float* logit, float* mean, float* invstd, const HdWs& W,
                                 hipStream_t s) {
    const int q = C / V, items = W.bc.items;
    bc_stats_kernel<V, 0, false, TZ><<<BC_GRID(items, q)>>>(P, z, ldz, M, C, q, items, W.bc.part);
    BcFinish F{};
    F.stats = 1; F.momentum = momentum; F.eps = eps; F.o0 = mean; F.o1 = invstd; F.running_mean = running_mean; F.running_var = running_var;
    bc_reduce_kernel<2><<<p2w_cdiv(C, 16), 256, 0, s>>>(W.bc.part, items, C, M, F);
    hd_rowdot_kernel<V, TZ><<<p2w_cdiv(p2w_cdiv(M, HD_ROWS), 4), 256, 0, s>>>(P, w, bias, z, ldz, M, C, logit);
}

template <int V, class TZ> void hd_backward(const BcParams& P, const float* w, const float* g, const TZ* z, int ldz, int M, int C, TZ* dz, int lddz,
                                  float* dgamma, float* dbeta, float* dw, float* dbias, const HdWs& W, hipStream_t s) {
    const int q = C / V, items = W.bc.items;
    hd_bwd_sums_kernel<V, TZ><<<BC_GRID(items, q)>>>(P, w, g, z, ldz, M, C, q, items, W.bc.part, W.gpart);
    BcFinish F{};
    F.o0 = dgamma; F.o1 = dbeta; F.kq = W.bc.kq; F.dw = dw; F.gpart = W.gpart; F.dbias = dbias;
    bc_reduce_kernel<3><<<p2w_cdiv(C, 32 / 3), 256, 0, s>>>(W.bc.part, items, C, M, F);
    hd_dz_kernel<V, TZ><<<BC_GRID(items, q)>>>(P, w, g, z, ldz, M, C, q, items, dz, lddz);
}

// the entry points' bodies on z's (and dz's) element type
template <class TZ>
int32_t hd_rowdot_t(const TZ* z, int32_t ldz, const float* gamma, const float* beta, const float* w, const float* bias, float* running_mean,
                    float* running_var, double momentum, double eps, int32_t M, int32_t C, float* logit, float* mean, float* invstd, void* ws,
                    size_t ws_bytes, p2w_stream_t stream) {
    if (!bc_sizes_ok(M, C, 1) || ldz < C) return P2W_EINVAL;
    if (!(eps >= 0.0) || !(momentum >= 0.0 && momentum <= 1.0)) return P2W_EINVAL;
    P2W_CHECK_PTR(z); P2W_CHECK_PTR(gamma); P2W_CHECK_PTR(beta); P2W_CHECK_PTR(w); P2W_CHECK_PTR(bias); P2W_CHECK_PTR(running_mean);
    P2W_CHECK_PTR(running_var); P2W_CHECK_PTR(logit); P2W_CHECK_PTR(mean); P2W_CHECK_PTR(invstd); P2W_CHECK_PTR(ws);
    const bool v4 = !(C & 3) && !(ldz & 3) && gr_alv(z) && gr_al16(gamma) && gr_al16(beta) && gr_al16(w) && gr_al16(mean) && gr_al16(invstd);
    P2W_CHECK_ALIGN16(ws);
    P2wArena arena(ws);
    const HdWs W = hd_carve(arena, M, C);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    const BcParams P = hd_params(gamma, beta, mean, invstd, nullptr);
    hipStream_t s = p2w_s(stream);
    if (v4) hd_forward<4, TZ>(P, w, bias, z, ldz, M, C, running_mean, running_var, momentum, eps, logit, mean, invstd, W, s);
    else hd_forward<1, TZ>(P, w, bias, z, ldz, M, C, running_mean, running_var, momentum, eps, logit, mean, invstd, W, s);
    return P2W_LAUNCH_STATUS();
}

template <class TZ>
int32_t hd_rowdot_bwd_t(const float* g, const TZ* z, int32_t ldz, const float* gamma, const float* beta, const float* w, const float* mean,
                        const float* invstd, int32_t M, int32_t C, TZ* dz, int32_t lddz, float* dgamma, float* dbeta, float* dw, float* dbias,
                        void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (!bc_sizes_ok(M, C, 1) || ldz < C || lddz < C) return P2W_EINVAL;
    P2W_CHECK_PTR(g); P2W_CHECK_PTR(z); P2W_CHECK_PTR(gamma); P2W_CHECK_PTR(beta); P2W_CHECK_PTR(w); P2W_CHECK_PTR(mean); P2W_CHECK_PTR(invstd);
    P2W_CHECK_PTR(dz); P2W_CHECK_PTR(dgamma); P2W_CHECK_PTR(dbeta); P2W_CHECK_PTR(dw); P2W_CHECK_PTR(dbias); P2W_CHECK_PTR(ws);
    bool v4 = !(C & 3) && !(ldz & 3) && !(lddz & 3) && gr_alv(z) && gr_al16(gamma) && gr_al16(beta) && gr_al16(w) && gr_al16(mean) &&
              gr_al16(invstd) && gr_alv(dz);
    P2W_CHECK_ALIGN16(ws);
    P2wArena arena(ws);
    const HdWs W = hd_carve(arena, M, C);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    v4 = v4 && gr_al16(W.bc.kq);
    const BcParams P = hd_params(gamma, beta, mean, invstd, W.bc.kq);
    hipStream_t s = p2w_s(stream);
    if (v4) hd_backward<4, TZ>(P, w, g, z, ldz, M, C, dz, lddz, dgamma, dbeta, dw, dbias, W, s);
    else hd_backward<1, TZ>(P, w, g, z, ldz, M, C, dz, lddz, dgamma, dbeta, dw, dbias, W, s);
    return P2W_LAUNCH_STATUS();
}

}  // namespace

extern "C" size_t p2w_bn_relu_rowdot_ws_size(int32_t M, int32_t C) {
    if (!bc_sizes_ok(M, C, 1)) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { hd_carve(a, M, C); });
}

extern "C" int32_t p2w_bn_relu_rowdot_io(const void* z, int32_t tz, int32_t ldz, const float* gamma, const float* beta, const float* w,
                                         const float* bias, float* running_mean, float* running_var, double momentum, double eps, int32_t M,
                                         int32_t C, float* logit, float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (tz == P2W_F32)
        return hd_rowdot_t(static_cast<const float*>(z), ldz, gamma, beta, w, bias, running_mean, running_var, momentum, eps, M, C, logit, mean,
                           invstd, ws, ws_bytes, stream);
    if (tz == P2W_F16)
        return hd_rowdot_t(static_cast<const gr_half*>(z), ldz, gamma, beta, w, bias, running_mean, running_var, momentum, eps, M, C, logit, mean,
                           invstd, ws, ws_bytes, stream);
    return P2W_EUNSUPPORTED;
}

extern "C" int32_t p2w_bn_relu_rowdot(const float* z, int32_t ldz, const float* gamma, const float* beta, const float* w, const float* bias,
                                      float* running_mean, float* running_var, double momentum, double eps, int32_t M, int32_t C,
                                      float* logit, float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    return p2w_bn_relu_rowdot_io(z, P2W_F32, ldz, gamma, beta, w, bias, running_mean, running_var, momentum, eps, M, C, logit, mean, invstd, ws,
                                 ws_bytes, stream);
}

extern "C" int32_t p2w_bn_relu_rowdot_bwd_io(const float* g, const void* z, int32_t tz, int32_t ldz, const float* gamma, const float* beta,
                                             const float* w, const float* mean, const float* invstd, int32_t M, int32_t C, void* dz,
                                             int32_t lddz, float* dgamma, float* dbeta, float* dw, float* dbias, void* ws, size_t ws_bytes,
                                             p2w_stream_t stream) {
    if (tz == P2W_F32)
        return hd_rowdot_bwd_t(g, static_cast<const float*>(z), ldz, gamma, beta, w, mean, invstd, M, C, static_cast<float*>(dz), lddz, dgamma,
                               dbeta, dw, dbias, ws, ws_bytes, stream);
    if (tz == P2W_F16)
        return hd_rowdot_bwd_t(g, static_cast<const gr_half*>(z), ldz, gamma, beta, w, mean, invstd, M, C, static_cast<gr_half*>(dz), lddz,
                               dgamma, dbeta, dw, dbias, ws, ws_bytes, stream);
    return P2W_EUNSUPPORTED;
}

extern "C" int32_t p2w_bn_relu_rowdot_bwd(const float* g, const float* z, int32_t ldz, const float* gamma, const float* beta, const float* w,
                                          const float* mean, const float* invstd, int32_t M, int32_t C, float* dz, int32_t lddz,
                                          float* dgamma, float* dbeta, float* dw, float* dbias, void* ws, size_t ws_bytes,
                                          p2w_stream_t stream) {
    return p2w_bn_relu_rowdot_bwd_io(g, z, P2W_F32, ldz, gamma, beta, w, mean, invstd, M, C, dz, lddz, dgamma, dbeta, dw, dbias, ws, ws_bytes,
                                     stream);
}

// ---- the bfloat16 instantiations (include/p2w.h: the dtype code 2 stays unknown to the two _io entry points above)
extern "C" int32_t p2w_bn_relu_rowdot_bf16(const void* z, int32_t ldz, const float* gamma, const float* beta, const float* w,
                                           const float* bias, float* running_mean, float* running_var, double momentum, double eps,
                                           int32_t M, int32_t C, float* logit, float* mean, float* invstd, void* ws, size_t ws_bytes,
                                           p2w_stream_t stream) {
    return hd_rowdot_t(static_cast<const gr_bf16*>(z), ldz, gamma, beta, w, bias, running_mean, running_var, momentum, eps, M, C, logit, mean,
                       invstd, ws, ws_bytes, stream);
}

extern "C" int32_t p2w_bn_relu_rowdot_bwd_bf16(const float* g, const void* z, int32_t ldz, const float* gamma, const float* beta,
                                               const float* w, const float* mean, const float* invstd, int32_t M, int32_t C, void* dz,
                                               int32_t lddz, float* dgamma, float* dbeta, float* dw, float* dbias, void* ws,
                                               size_t ws_bytes, p2w_stream_t stream) {
    return hd_rowdot_bwd_t(g, static_cast<const gr_bf16*>(z), ldz, gamma, beta, w, mean, invstd, M, C, static_cast<gr_bf16*>(dz), lddz, dgamma,
                           dbeta, dw, dbias, ws, ws_bytes, stream);
}
