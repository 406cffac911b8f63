// Everything between two GEMMs of the inverted residual block for training (model.py:46-85): a chain of up to P2W_BN_CHAIN_MAX
// stages over the pre-activation Z [M, C], each an optional depthwise convolution with kernel size 1 (v = a u + b per column), a
// training-mode BatchNorm1d and an optional ReLU, with an optional residual add and ReLU at the end.  Every stage is a map per
// column once its two statistics are known, so the whole chain is computed from Z alone: one read of Z per BatchNorm for its
// statistics (the earlier stages recomputed in fp32 on the way), one read and one write to apply the chain; the backward is one
// read of Z and G per BatchNorm for its two column sums, BatchNorm's gradient through the batch statistics being a closed form in
// them, and one pass that writes dZ.  Nothing of [M, C] size exists besides Z, the residual, the output and the gradients.
//
// Streaming kernels, bandwidth-bound: no LDS tiles, no MFMA.  A lane owns V adjacent columns (V = 4: 16-byte accesses when C, the
// pitches and the pointers allow, V = 1: 4-byte accesses, the same bits) and walks the P2W_BN_CHAIN_ROWS consecutive rows of its
// work item in ascending order; its column constants stay in registers.  Sums: fp64 partials per item, then the items in ascending
// order (bc_reduce_kernel: the scheme of p2w_bnmax.hip's reduction, for K sums per column) - no floating-point atomics, the bits
// depend on the inputs alone.  The forward recomputation inside the backward is the forward's own code on the forward's rounded
// mean and invstd, so every ReLU mask is the forward's.
//
// p2w_relu_bn (the tail of the feature-propagation MLP, model.py:198-202: Linear, ReLU, BatchNorm1d) is the one-stage chain on
// u = (z < 0 ? 0 : z): the same kernels with the compile-time switch PRE, which clamps z as it is loaded and masks dz with z > 0.
// PRE exists for one stage only; every other instantiation is PRE = false and compiles to the code it was.
//
// Element types (the p2w_*_io entry points): TZ for z and dz, TO for out and g - float, or gr_half (p2w_runsum.h) widened as it is
// loaded and rounded to nearest even by gr_f2h as it is stored.  Built: (float, float) - what the fp32 entry points run, the code it
// was -, (gr_half, gr_half) for a chain between two float16 GEMMs and (gr_half, float) for one whose result is not only a GEMM's
// input; (gr_bf16, gr_bf16) and (gr_bf16, float) are the same two for bfloat16 (gr_f2b).  The residual, dres, the saved out of a
// chain with a residual (a ReLU mask), the [C] vectors and the workspace stay fp32 / fp64; arithmetic, sums and their order do not
// depend on the element types, so a 16-bit route has the fp32 route's bits on the widened tensors, rounded once where it stores
// float16 / bfloat16.  V = 4 is an 8-byte access on a 16-bit tensor.
#include "p2w_bnchain.h"

namespace {

// Forward, last launch: out = u_L, or max(u_L + res, 0)
template <int V, int L, bool PRE = false, class TZ = float, class TO = float>
__global__ __launch_bounds__(256) void bc_apply_kernel(BcParams P, const TZ* __restrict__ z, int ldz, const float* __restrict__ res, int ldr,
                                                       int M, int C, int q, int items, TO* __restrict__ out, int ldo) {
    BC_ITEM_PROLOGUE();
    BcCol<V> k[L];
#pragma unroll
    for (int t = 0; t < L; ++t) bc_load<V>(P, t, C, c, k[t]);
#pragma unroll 4
    for (int r = r0; r < r1; ++r) {
        float x[V], xh[V];
        gr_ld<V>(&z[(size_t)r * ldz + c], x);
        if constexpr (PRE) bc_pre<V>(x);
#pragma unroll
        for (int t = 0; t < L; ++t) bc_stage<V>(k[t], P.relu[t] != 0, x, xh);
        if (res) {
            float rv[V];
            gr_ld<V>(&res[(size_t)r * ldr + c], rv);
#pragma unroll
            for (int u = 0; u < V; ++u) { const float s = x[u] + rv[u]; x[u] = s < 0.f ? 0.f : s; }
        }
        gr_st<V>(&out[(size_t)r * ldo + c], x);
    }
}

// the forward recomputed for the backward: xh[t] and uo[t] (the stage's output) of every stage, uin = the input of stage S (0-based)
template <int V, int L>
__device__ __forceinline__ void bc_replay(const BcParams& P, const BcCol<V> (&k)[L], int S, float (&x)[V], float (&xh)[L][V], float (&uo)[L][V],
                                          float (&uin)[V]) {
#pragma unroll
    for (int t = 0; t < L; ++t) {
        if (t == S) {
#pragma unroll
            for (int u = 0; u < V; ++u) uin[u] = x[u];
        }
        bc_stage<V>(k[t], P.relu[t] != 0, x, xh[t]);
#pragma unroll
        for (int u = 0; u < V; ++u) uo[t][u] = x[u];
    }
}

// Backward, the sums of stage S (0-based; the stages above it are finished: their k1, k2 are in P.kq): per item and column
//   s0 = sum gy, s1 = sum gy xhat_S, and with DW (the stage has a depthwise convolution, input u) s2 = sum gy u, s3 = sum u,
//   s4 = sum xhat_S u - fp64 terms on the fp32 values.  `outp` (the forward's output) is given when the chain had a residual.
template <int V, int L, int S, bool DW, bool PRE = false, class TZ = float, class TO = float>
__global__ __launch_bounds__(256) void bc_bwd_sums_kernel(BcParams P, const TO* __restrict__ g, int ldg, const TZ* __restrict__ z, int ldz,
                                                          const float* __restrict__ outp, int ldo, int M, int C, int q, int items,
                                                          double* __restrict__ part) {
    constexpr int K = DW ? BC_KMAX : 2;
    BC_ITEM_PROLOGUE();
    BcCol<V> k[L];
    BcGrad<V> kg[L];
#pragma unroll
    for (int t = 0; t < L; ++t) {
        bc_load<V>(P, t, C, c, k[t]);
        if (t > S) bc_load_grad<V>(P, t, C, c, k[t], kg[t]);
    }
    double s[K][V];
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int u = 0; u < V; ++u) s[j][u] = 0.0;
#pragma unroll 2
    for (int r = r0; r < r1; ++r) {
        float x[V], xh[L][V], uo[L][V], uin[V], gg[V];
        gr_ld<V>(&z[(size_t)r * ldz + c], x);
        gr_ld<V>(&g[(size_t)r * ldg + c], gg);
        if constexpr (PRE) bc_pre<V>(x);
        bc_replay<V, L>(P, k, S, x, xh, uo, uin);
        if (outp) {
            float ov[V];
            gr_ld<V>(&outp[(size_t)r * ldo + c], ov);
#pragma unroll
            for (int u = 0; u < V; ++u) gg[u] = ov[u] > 0.f ? gg[u] : 0.f;
        }
#pragma unroll
        for (int t = L - 1; t > S; --t) bc_stage_bwd<V>(k[t], kg[t], P.relu[t] != 0, xh[t], uo[t], gg);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            const float gy = P.relu[S] ? (uo[S][u] > 0.f ? gg[u] : 0.f) : gg[u];
            const double gd = (double)gy, xd = (double)xh[S][u];
            s[0][u] = s[0][u] + gd;
            s[1][u] = s[1][u] + gd * xd;
            if constexpr (DW) {
                const double ud = (double)uin[u];
                s[2][u] = s[2][u] + gd * ud;
                s[3][u] = s[3][u] + ud;
                s[4][u] = s[4][u] + xd * ud;
            }
        }
    }
#pragma unroll
    for (int j = 0; j < K; ++j)
#pragma unroll
        for (int u = 0; u < V; ++u) part[((size_t)item * K + j) * C + c + u] = s[j][u];
}

// Backward, last launch: dz = the gradient through every stage, dres = g [out > 0]
template <int V, int L, bool PRE = false, class TZ = float, class TO = float>
__global__ __launch_bounds__(256) void bc_dz_kernel(BcParams P, const TO* __restrict__ g, int ldg, const TZ* __restrict__ z, int ldz,
                                                    const float* __restrict__ outp, int ldo, int M, int C, int q, int items, TZ* __restrict__ dz,
                                                    int lddz, float* __restrict__ dres, int lddr) {
    BC_ITEM_PROLOGUE();
    BcCol<V> k[L];
    BcGrad<V> kg[L];
#pragma unroll
    for (int t = 0; t < L; ++t) { bc_load<V>(P, t, C, c, k[t]); bc_load_grad<V>(P, t, C, c, k[t], kg[t]); }
#pragma unroll 2
    for (int r = r0; r < r1; ++r) {
        float x[V], xh[L][V], uo[L][V], uin[V], gg[V];
        gr_ld<V>(&z[(size_t)r * ldz + c], x);
        gr_ld<V>(&g[(size_t)r * ldg + c], gg);
        [[maybe_unused]] float zin[V];
        if constexpr (PRE) {
#pragma unroll
            for (int u = 0; u < V; ++u) zin[u] = x[u];
            bc_pre<V>(x);
        }
        bc_replay<V, L>(P, k, -1, x, xh, uo, uin);
        if (outp) {
            float ov[V];
            gr_ld<V>(&outp[(size_t)r * ldo + c], ov);
#pragma unroll
            for (int u = 0; u < V; ++u) gg[u] = ov[u] > 0.f ? gg[u] : 0.f;
            if (dres) gr_st<V>(&dres[(size_t)r * lddr + c], gg);
        }
#pragma unroll
        for (int t = L - 1; t >= 0; --t) bc_stage_bwd<V>(k[t], kg[t], P.relu[t] != 0, xh[t], uo[t], gg);
        if constexpr (PRE) {
#pragma unroll
            for (int u = 0; u < V; ++u) gg[u] = zin[u] > 0.f ? gg[u] : 0.f;
        }
        gr_st<V>(&dz[(size_t)r * lddz + c], gg);
    }
}

// NULL and alignment of the stages' vectors; v4 is cleared where one of them is off 16 bytes
inline int32_t bc_stages_ok(const p2w_bn_stage* st, int L, bool forward, bool& v4) {
    for (int t = 0; t < L; ++t) {
        if ((st[t].dw_w == nullptr) != (st[t].dw_b == nullptr)) return P2W_EINVAL;
        P2W_CHECK_PTR(st[t].gamma); P2W_CHECK_PTR(st[t].beta);
        if (forward) {
            P2W_CHECK_PTR(st[t].running_mean); P2W_CHECK_PTR(st[t].running_var);
            if (!(st[t].eps >= 0.0) || !(st[t].momentum >= 0.0 && st[t].momentum <= 1.0)) return P2W_EINVAL;
        }
        v4 = v4 && gr_al16(st[t].gamma) && gr_al16(st[t].beta) && gr_al16(st[t].dw_w) && gr_al16(st[t].dw_b);
    }
    return P2W_OK;
}
inline BcParams bc_params(const p2w_bn_stage* st, int L, const float* mean, const float* invstd, const float* kq) {
    BcParams P{};
    for (int t = 0; t < L; ++t) {
        P.a[t] = st[t].dw_w; P.b[t] = st[t].dw_b; P.gamma[t] = st[t].gamma; P.beta[t] = st[t].beta; P.relu[t] = st[t].relu != 0;
    }
    P.mean = mean; P.invstd = invstd; P.kq = kq;
    return P;
}

template <int V, bool PRE, class TZ, class TO> void bc_forward(const BcParams& P, const p2w_bn_stage* st, int L, const TZ* z, int ldz, const float* res, int ldr, int M, int C,
                                 TO* out, int ldo, float* mean, float* invstd, const BcWs& W, hipStream_t s) {
    const int q = C / V;
    for (int t = 0; t < L; ++t) {
        if (t == 0) bc_stats_kernel<V, 0, PRE, TZ><<<BC_GRID(W.items, q)>>>(P, z, ldz, M, C, q, W.items, W.part);
        else if (t == 1) bc_stats_kernel<V, 1, false, TZ><<<BC_GRID(W.items, q)>>>(P, z, ldz, M, C, q, W.items, W.part);
        else bc_stats_kernel<V, 2, false, TZ><<<BC_GRID(W.items, q)>>>(P, z, ldz, M, C, q, W.items, W.part);
        BcFinish F{};
        F.stats = 1; F.a = st[t].dw_w; F.b = st[t].dw_b; F.momentum = st[t].momentum; F.eps = st[t].eps;
        F.o0 = mean + (size_t)t * C; F.o1 = invstd + (size_t)t * C; F.running_mean = st[t].running_mean; F.running_var = st[t].running_var;
        bc_reduce_kernel<2><<<p2w_cdiv(C, 16), 256, 0, s>>>(W.part, W.items, C, M, F);
    }
    if (L == 1) bc_apply_kernel<V, 1, PRE, TZ, TO><<<BC_GRID(W.items, q)>>>(P, z, ldz, res, ldr, M, C, q, W.items, out, ldo);
    else if (L == 2) bc_apply_kernel<V, 2, false, TZ, TO><<<BC_GRID(W.items, q)>>>(P, z, ldz, res, ldr, M, C, q, W.items, out, ldo);
    else bc_apply_kernel<V, 3, false, TZ, TO><<<BC_GRID(W.items, q)>>>(P, z, ldz, res, ldr, M, C, q, W.items, out, ldo);
}

template <int V, int L, int S, bool PRE, class TZ, class TO> void bc_bwd_stage(const BcParams& P, const p2w_bn_stage* st, const TO* g, int ldg, const TZ* z, int ldz,
                                                 const float* outp, int ldo, const float* invstd, int M, int C, float* dgamma, float* dbeta,
                                                 float* ddw_w, float* ddw_b, const BcWs& W, hipStream_t s) {
    const int q = C / V;
    const bool dw = st[S].dw_w != nullptr;
    if constexpr (PRE) bc_bwd_sums_kernel<V, L, S, false, true, TZ, TO><<<BC_GRID(W.items, q)>>>(P, g, ldg, z, ldz, outp, ldo, M, C, q, W.items, W.part);
    else if (dw) bc_bwd_sums_kernel<V, L, S, true, false, TZ, TO><<<BC_GRID(W.items, q)>>>(P, g, ldg, z, ldz, outp, ldo, M, C, q, W.items, W.part);
    else bc_bwd_sums_kernel<V, L, S, false, false, TZ, TO><<<BC_GRID(W.items, q)>>>(P, g, ldg, z, ldz, outp, ldo, M, C, q, W.items, W.part);
    BcFinish F{};
    F.a = st[S].dw_w; F.b = st[S].dw_b; F.gamma = st[S].gamma; F.invstd = invstd + (size_t)S * C;
    F.o0 = dgamma + (size_t)S * C; F.o1 = dbeta + (size_t)S * C; F.kq = W.kq + (size_t)S * 2 * C;
    F.ddw_w = ddw_w ? ddw_w + (size_t)S * C : nullptr; F.ddw_b = ddw_b ? ddw_b + (size_t)S * C : nullptr;
    if (dw) bc_reduce_kernel<BC_KMAX><<<p2w_cdiv(C, 32 / BC_KMAX), 256, 0, s>>>(W.part, W.items, C, M, F);
    else bc_reduce_kernel<2><<<p2w_cdiv(C, 16), 256, 0, s>>>(W.part, W.items, C, M, F);
}

template <int V, int L, bool PRE, class TZ, class TO> void bc_backward(const BcParams& P, const p2w_bn_stage* st, const TO* g, int ldg, const TZ* z, int ldz, const float* outp,
                                         int ldo, const float* invstd, int M, int C, TZ* dz, int lddz, float* dres, int lddr, float* dgamma,
                                         float* dbeta, float* ddw_w, float* ddw_b, const BcWs& W, hipStream_t s) {
    if constexpr (L >= 3) bc_bwd_stage<V, L, 2, false, TZ, TO>(P, st, g, ldg, z, ldz, outp, ldo, invstd, M, C, dgamma, dbeta, ddw_w, ddw_b, W, s);
    if constexpr (L >= 2) bc_bwd_stage<V, L, 1, false, TZ, TO>(P, st, g, ldg, z, ldz, outp, ldo, invstd, M, C, dgamma, dbeta, ddw_w, ddw_b, W, s);
    bc_bwd_stage<V, L, 0, PRE, TZ, TO>(P, st, g, ldg, z, ldz, outp, ldo, invstd, M, C, dgamma, dbeta, ddw_w, ddw_b, W, s);
    bc_dz_kernel<V, L, PRE, TZ, TO><<<BC_GRID(W.items, C / V)>>>(P, g, ldg, z, ldz, outp, ldo, M, C, C / V, W.items, dz, lddz, dres, lddr);
}

// the two entry points' bodies on one pair of element types (TZ: z and dz, TO: out and g); pre (p2w_relu_bn) is a chain of one stage
// without a depthwise convolution and without a residual
template <class TZ, class TO>
int32_t bc_chain_forward_t(bool pre, const TZ* z, int32_t ldz, const float* res, int32_t ldr, const p2w_bn_stage* stages, int32_t L, int32_t M,
                           int32_t C, TO* out, int32_t ldo, float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (!bc_sizes_ok(M, C, L) || ldz < C || ldo < C || (res && ldr < C)) return P2W_EINVAL;
    P2W_CHECK_PTR(z); P2W_CHECK_PTR(stages); P2W_CHECK_PTR(out); P2W_CHECK_PTR(mean); P2W_CHECK_PTR(invstd); P2W_CHECK_PTR(ws);
    bool v4 = !(C & 3) && !(ldz & 3) && !(ldo & 3) && (!res || !(ldr & 3)) && gr_alv(z) && gr_al16(res) && gr_alv(out) && gr_al16(mean) &&
              gr_al16(invstd);
    const int32_t bad = bc_stages_ok(stages, L, true, v4);
    if (bad != P2W_OK) return bad;
    P2W_CHECK_ALIGN16(ws);
    P2wArena arena(ws);
    const BcWs W = bc_carve(arena, M, C, L);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    const BcParams P = bc_params(stages, L, mean, invstd, nullptr);
    hipStream_t s = p2w_s(stream);
    if (pre) {
        if (v4) bc_forward<4, true, TZ, TO>(P, stages, 1, z, ldz, nullptr, 0, M, C, out, ldo, mean, invstd, W, s);
        else bc_forward<1, true, TZ, TO>(P, stages, 1, z, ldz, nullptr, 0, M, C, out, ldo, mean, invstd, W, s);
    } else {
        if (v4) bc_forward<4, false, TZ, TO>(P, stages, L, z, ldz, res, ldr, M, C, out, ldo, mean, invstd, W, s);
        else bc_forward<1, false, TZ, TO>(P, stages, L, z, ldz, res, ldr, M, C, out, ldo, mean, invstd, W, s);
    }
    return P2W_LAUNCH_STATUS();
}

template <class TZ, class TO>
int32_t bc_chain_backward_t(bool pre, const TO* g, int32_t ldg, const TZ* z, int32_t ldz, const float* out, int32_t ldo,
                            const p2w_bn_stage* stages, int32_t L, const float* mean, const float* invstd, int32_t M, int32_t C, TZ* dz,
                            int32_t lddz, float* dres, int32_t lddr, float* dgamma, float* dbeta, float* ddw_w, float* ddw_b, void* ws,
                            size_t ws_bytes, p2w_stream_t stream) {
    if (!bc_sizes_ok(M, C, L) || ldg < C || ldz < C || lddz < C || (out && ldo < C) || (dres && (lddr < C || !out))) return P2W_EINVAL;
    P2W_CHECK_PTR(g); P2W_CHECK_PTR(z); P2W_CHECK_PTR(stages); P2W_CHECK_PTR(mean); P2W_CHECK_PTR(invstd); P2W_CHECK_PTR(dz);
    P2W_CHECK_PTR(dgamma); P2W_CHECK_PTR(dbeta); P2W_CHECK_PTR(ws);
    bool v4 = !(C & 3) && !(ldg & 3) && !(ldz & 3) && !(lddz & 3) && (!out || !(ldo & 3)) && (!dres || !(lddr & 3)) && gr_alv(g) && gr_alv(z) &&
              gr_al16(out) && gr_al16(mean) && gr_al16(invstd) && gr_alv(dz) && gr_al16(dres);
    const int32_t bad = bc_stages_ok(stages, L, false, v4);
    if (bad != P2W_OK) return bad;
    for (int t = 0; t < L; ++t)
        if (stages[t].dw_w && (!ddw_w || !ddw_b)) return P2W_ENULL;
    P2W_CHECK_ALIGN16(ws);
    P2wArena arena(ws);
    const BcWs W = bc_carve(arena, M, C, L);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    v4 = v4 && gr_al16(W.kq);
    const BcParams P = bc_params(stages, L, mean, invstd, W.kq);
    hipStream_t s = p2w_s(stream);
#define BC_BWD(V, LL, PRE) bc_backward<V, LL, PRE, TZ, TO>(P, stages, g, ldg, z, ldz, out, ldo, invstd, M, C, dz, lddz, dres, lddr, dgamma, dbeta, ddw_w, ddw_b, W, s)
    if (pre) { if (v4) BC_BWD(4, 1, true); else BC_BWD(1, 1, true); }
    else if (v4) { if (L == 1) BC_BWD(4, 1, false); else if (L == 2) BC_BWD(4, 2, false); else BC_BWD(4, 3, false); }
    else { if (L == 1) BC_BWD(1, 1, false); else if (L == 2) BC_BWD(1, 2, false); else BC_BWD(1, 3, false); }
#undef BC_BWD
    return P2W_LAUNCH_STATUS();
}

// the dtype codes of the _io entry points: (z, out) = (f32, f32), (f16, f32), (f16, f16), (bf16, f32), (bf16, bf16); everything else
// (a float16 / bfloat16 mix among it) is refused first
int32_t bc_chain_forward(bool pre, const void* z, int32_t tz, int32_t ldz, const float* res, int32_t ldr, const p2w_bn_stage* stages, int32_t L,
                         int32_t M, int32_t C, void* out, int32_t to, int32_t ldo, float* mean, float* invstd, void* ws, size_t ws_bytes,
                         p2w_stream_t stream) {
#define BC_FWD(TZ, TO) bc_chain_forward_t<TZ, TO>(pre, static_cast<const TZ*>(z), ldz, res, ldr, stages, L, M, C, static_cast<TO*>(out), ldo, mean, invstd, ws, ws_bytes, stream)
    if (tz == P2W_F32 && to == P2W_F32) return BC_FWD(float, float);
    if (tz == P2W_F16 && to == P2W_F32) return BC_FWD(gr_half, float);
    if (tz == P2W_F16 && to == P2W_F16) return BC_FWD(gr_half, gr_half);
    if (tz == P2W_BF16 && to == P2W_F32) return BC_FWD(gr_bf16, float);
    if (tz == P2W_BF16 && to == P2W_BF16) return BC_FWD(gr_bf16, gr_bf16);
#undef BC_FWD
    return P2W_EUNSUPPORTED;
}

int32_t bc_chain_backward(bool pre, const void* g, int32_t to, int32_t ldg, const void* z, int32_t tz, int32_t ldz, const float* out, int32_t ldo,
                          const p2w_bn_stage* stages, int32_t L, const float* mean, const float* invstd, int32_t M, int32_t C, void* dz,
                          int32_t lddz, float* dres, int32_t lddr, float* dgamma, float* dbeta, float* ddw_w, float* ddw_b, void* ws,
                          size_t ws_bytes, p2w_stream_t stream) {
#define BC_BWD_T(TZ, TO) bc_chain_backward_t<TZ, TO>(pre, static_cast<const TO*>(g), ldg, static_cast<const TZ*>(z), ldz, out, ldo, stages, L, mean, invstd, M, C, \
                                                     static_cast<TZ*>(dz), lddz, dres, lddr, dgamma, dbeta, ddw_w, ddw_b, ws, ws_bytes, stream)
    if (tz == P2W_F32 && to == P2W_F32) return BC_BWD_T(float, float);
    if (tz == P2W_F16 && to == P2W_F32) return BC_BWD_T(gr_half, float);
    if (tz == P2W_F16 && to == P2W_F16) return BC_BWD_T(gr_half, gr_half);
    if (tz == P2W_BF16 && to == P2W_F32) return BC_BWD_T(gr_bf16, float);
    if (tz == P2W_BF16 && to == P2W_BF16) return BC_BWD_T(gr_bf16, gr_bf16);
#undef BC_BWD_T
    return P2W_EUNSUPPORTED;
}

}  // namespace

extern "C" size_t p2w_bn_chain_ws_size(int32_t M, int32_t C, int32_t L) {
    if (!bc_sizes_ok(M, C, L)) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { bc_carve(a, M, C, L); });
}

extern "C" int32_t p2w_bn_chain_io(const void* z, int32_t tz, int32_t ldz, const float* res, int32_t ldr, const p2w_bn_stage* stages, int32_t L,
                                   int32_t M, int32_t C, void* out, int32_t to, int32_t ldo, float* mean, float* invstd, void* ws,
                                   size_t ws_bytes, p2w_stream_t stream) {
    return bc_chain_forward(false, z, tz, ldz, res, ldr, stages, L, M, C, out, to, ldo, mean, invstd, ws, ws_bytes, stream);
}

extern "C" int32_t p2w_bn_chain(const float* z, int32_t ldz, const float* res, int32_t ldr, const p2w_bn_stage* stages, int32_t L, int32_t M,
                                int32_t C, float* out, int32_t ldo, float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    return p2w_bn_chain_io(z, P2W_F32, ldz, res, ldr, stages, L, M, C, out, P2W_F32, ldo, mean, invstd, ws, ws_bytes, stream);
}

extern "C" int32_t p2w_bn_chain_bwd_io(const void* g, int32_t to, int32_t ldg, const void* z, int32_t tz, int32_t ldz, const float* out,
                                       int32_t ldo, const p2w_bn_stage* stages, int32_t L, const float* mean, const float* invstd, int32_t M,
                                       int32_t C, void* dz, int32_t lddz, float* dres, int32_t lddr, float* dgamma, float* dbeta, float* ddw_w,
                                       float* ddw_b, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    return bc_chain_backward(false, g, to, ldg, z, tz, ldz, out, ldo, stages, L, mean, invstd, M, C, dz, lddz, dres, lddr, dgamma, dbeta, ddw_w,
                             ddw_b, ws, ws_bytes, stream);
}

extern "C" int32_t p2w_bn_chain_bwd(const float* g, int32_t ldg, const float* z, int32_t ldz, const float* out, int32_t ldo,
                                    const p2w_bn_stage* stages, int32_t L, const float* mean, const float* invstd, int32_t M, int32_t C, float* dz,
                                    int32_t lddz, float* dres, int32_t lddr, float* dgamma, float* dbeta, float* ddw_w, float* ddw_b, void* ws,
                                    size_t ws_bytes, p2w_stream_t stream) {
    return p2w_bn_chain_bwd_io(g, P2W_F32, ldg, z, P2W_F32, ldz, out, ldo, stages, L, mean, invstd, M, C, dz, lddz, dres, lddr, dgamma, dbeta,
                               ddw_w, ddw_b, ws, ws_bytes, stream);
}

// ---- ReLU in front of one training-mode BatchNorm1d: the one-stage chain on relu(z)
extern "C" size_t p2w_relu_bn_ws_size(int32_t M, int32_t C) { return p2w_bn_chain_ws_size(M, C, 1); }

extern "C" int32_t p2w_relu_bn_io(const void* z, int32_t tz, int32_t ldz, const float* gamma, const float* beta, float* running_mean,
                                  float* running_var, double momentum, double eps, int32_t M, int32_t C, void* out, int32_t to, int32_t ldo,
                                  float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    const p2w_bn_stage st = {nullptr, nullptr, gamma, beta, running_mean, running_var, momentum, eps, 0};
    return bc_chain_forward(true, z, tz, ldz, nullptr, 0, &st, 1, M, C, out, to, ldo, mean, invstd, ws, ws_bytes, stream);
}

extern "C" int32_t p2w_relu_bn(const float* z, int32_t ldz, const float* gamma, const float* beta, float* running_mean, float* running_var,
                               double momentum, double eps, int32_t M, int32_t C, float* out, int32_t ldo, float* mean, float* invstd, void* ws,
                               size_t ws_bytes, p2w_stream_t stream) {
    return p2w_relu_bn_io(z, P2W_F32, ldz, gamma, beta, running_mean, running_var, momentum, eps, M, C, out, P2W_F32, ldo, mean, invstd, ws,
                          ws_bytes, stream);
}

extern "C" int32_t p2w_relu_bn_bwd_io(const void* g, int32_t to, int32_t ldg, const void* z, int32_t tz, int32_t ldz, const float* gamma,
                                      const float* mean, const float* invstd, int32_t M, int32_t C, void* dz, int32_t lddz, float* dgamma,
                                      float* dbeta, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    // (the chain's kernels load beta beside gamma; without a ReLU behind the BatchNorm no gradient depends on it: gamma stands in)
    const p2w_bn_stage st = {nullptr, nullptr, gamma, gamma, nullptr, nullptr, 0.0, 0.0, 0};
    return bc_chain_backward(true, g, to, ldg, z, tz, ldz, nullptr, 0, &st, 1, mean, invstd, M, C, dz, lddz, nullptr, 0, dgamma, dbeta, nullptr,
                             nullptr, ws, ws_bytes, stream);
}

extern "C" int32_t p2w_relu_bn_bwd(const float* g, int32_t ldg, const float* z, int32_t ldz, const float* gamma, const float* mean,
                                   const float* invstd, int32_t M, int32_t C, float* dz, int32_t lddz, float* dgamma, float* dbeta, void* ws,
                                   size_t ws_bytes, p2w_stream_t stream) {
    return p2w_relu_bn_bwd_io(g, P2W_F32, ldg, z, P2W_F32, ldz, gamma, mean, invstd, M, C, dz, lddz, dgamma, dbeta, ws, ws_bytes, stream);
}
