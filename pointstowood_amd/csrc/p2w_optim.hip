// The optimiser step of the training loop behind backward(): unscale, the global gradient norm, the clip, AdamW and the loss-scale law
// of torch's GradScaler, decided and applied on the device (what pointstowood/src/trainer.py:196-204 composes from scaler.unscale_,
// clip_grad_norm_, scaler.step(AdamW) and scaler.update()).  include/p2w.h (p2w_clip_adamw) is the specification; in short:
//
//   norm      one workgroup per chunk of P2W_OPTIM_CHUNK consecutive elements of ONE tensor: every lane reads four groups of four
//             gradients (16 bytes at a time where the tensor's address allows, else 4), forms u = fl32(g * inv_scale) and adds the exact
//             fp64 squares to an fp64 register in ascending index; the 64 lanes of a wave are summed by the xor-shuffle tree of
//             p2w_loss.hip, the four waves are added in wave order and the chunk's sum goes to the workspace word of its global index.
//   finalise  one workgroup: thread t adds the chunk sums t, t + 256, ... in ascending order, the same tree and wave order give sumsq;
//             thread 0 decides found_inf, forms norm, coef, the new loss scale and the step's seven fp32 scalars and writes the record.
//   update    the same chunks: every workgroup reads the record, returns without a store on found_inf, and otherwise applies the
//             element law of the header, every operation individually rounded (this file is built without contraction, the square root
//             and the division are the correctly rounded ones).
//
// The tensor table reaches the kernels BY VALUE in the kernel arguments, one launch per group of at most P2W_OPTIM_GROUP tensors, so
// nothing is uploaded and the caller may rebuild the table at every step.  No memset, no atomics, no host synchronisation, no workgroup
// waits for another: every word the finalise pass reads was written by a norm launch, and the update launches are behind it in stream
// order.  Every order above depends on the table's element counts alone, so equal inputs give equal bits whatever the workspace held.
#include "p2w_common.h"
#include <math.h>

#pragma clang fp contract(off)

namespace {

constexpr int OP_THREADS = 256;
constexpr int OP_WAVES = OP_THREADS / P2W_WAVE;
constexpr int OP_GROUPS = P2W_OPTIM_CHUNK / (4 * OP_THREADS);     // groups of four elements per lane and chunk
static_assert(OP_GROUPS * 4 * OP_THREADS == P2W_OPTIM_CHUNK, "a chunk is a whole number of rounds of the workgroup");

// one launch's share of the table: the tensors (none empty), first[k] = the launch's first workgroup of tensor k (first[count] = the
// grid), chunk0 = the global index of the launch's first chunk
struct OpGroup {
    p2w_optim_tensor t[P2W_OPTIM_GROUP];
    uint32_t first[P2W_OPTIM_GROUP + 1];
    int32_t count;
    long long chunk0;
};

__device__ __forceinline__ double op_wave_sum(double v) {
#pragma unroll
    for (int off = P2W_WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// the tensor of workgroup b: the largest k with first[k] <= b (the same in every lane)
__device__ __forceinline__ int op_find(const OpGroup& G, uint32_t b) {
    int lo = 0, hi = G.count;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (G.first[mid] <= b) lo = mid; else hi = mid;
    }
    return lo;
}

__device__ __forceinline__ bool op_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// four consecutive elements from i, those at or beyond n as +0; 16 bytes at once where `wide` and all four exist
__device__ __forceinline__ float4 op_load4(const float* __restrict__ a, long long i, long long n, bool wide) {
    if (wide && i + 4 <= n) return *reinterpret_cast<const float4*>(a + i);
    float4 r = float4{0.0f, 0.0f, 0.0f, 0.0f};
    if (i < n) r.x = a[i];
    if (i + 1 < n) r.y = a[i + 1];
    if (i + 2 < n) r.z = a[i + 2];
    if (i + 3 < n) r.w = a[i + 3];
    return r;
}

__device__ __forceinline__ void op_store4(float* __restrict__ a, long long i, long long n, bool wide, float4 r) {
    if (wide && i + 4 <= n) {
        *reinterpret_cast<float4*>(a + i) = r;
        return;
    }
    if (i < n) a[i] = r.x;
    if (i + 1 < n) a[i + 1] = r.y;
    if (i + 2 < n) a[i + 2] = r.z;
    if (i + 3 < n) a[i + 3] = r.w;
}

__device__ __forceinline__ float op_inv_scale(const p2w_optim_state* state, int scaling) {
    return scaling ? (float)(1.0 / (double)state->scale) : 1.0f;
}

__global__ __launch_bounds__(OP_THREADS) void op_norm_kernel(OpGroup G, const p2w_optim_state* __restrict__ state, int scaling,
                                                             double* __restrict__ partial) {
    __shared__ double s_sum[OP_WAVES];
    const int k = op_find(G, blockIdx.x);
    const float* __restrict__ g = G.t[k].g;
    const long long n = G.t[k].n;
    const long long base = (long long)(blockIdx.x - G.first[k]) * P2W_OPTIM_CHUNK + 4 * (long long)threadIdx.x;
    const bool wide = op_al16(g);
    const float inv = op_inv_scale(state, scaling);
    float4 x[OP_GROUPS];
#pragma unroll
    for (int u = 0; u < OP_GROUPS; ++u) x[u] = op_load4(g, base + (long long)u * (4 * OP_THREADS), n, wide);
    double sum = 0.0;
#pragma unroll
    for (int u = 0; u < OP_GROUPS; ++u) {
        const long long i = base + (long long)u * (4 * OP_THREADS);
        const float e[4] = {x[u].x, x[u].y, x[u].z, x[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            if (i + j < n) {
                const double w = (double)(e[j] * inv);             // u = fl32(g * inv_scale); its square is exact in fp64
                sum += w * w;
            }
        }
    }
    sum = op_wave_sum(sum);
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_sum[0];
        for (int w = 1; w < OP_WAVES; ++w) t += s_sum[w];
        partial[G.chunk0 + blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(OP_THREADS) void op_finalise_kernel(const double* __restrict__ partial, long long chunks, p2w_optim_hyper H,
                                                                 p2w_optim_state* __restrict__ state) {
    __shared__ double s_sum[OP_WAVES];
    double t = 0.0;
    for (long long c = threadIdx.x; c < chunks; c += OP_THREADS) t += partial[c];
    t = op_wave_sum(t);
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    if (lane == 0) s_sum[wave] = t;
    __syncthreads();
    if (threadIdx.x != 0) return;
    double sumsq = s_sum[0];
    for (int w = 1; w < OP_WAVES; ++w) sumsq += s_sum[w];

    p2w_optim_state S = *state;
    const int found_inf = !(sumsq - sumsq == 0.0);                 // an inf or a NaN of g is in the sum; finite squares cannot overflow it
    S.sumsq = sumsq;
    S.norm = (float)sqrt(sumsq);
    S.coef = fminf(1.0f, (float)H.max_norm / (S.norm + 1e-6f));
    S.inv_scale = op_inv_scale(state, H.scaling);
    S.found_inf = found_inf;
    if (!H.scaling) S.scale = 1.0f;
    if (found_inf) {
        if (H.scaling) S.scale = S.scale * (float)H.backoff_factor;
        S.growth_tracker = 0;
        S.skipped += 1;
    } else {
        S.t += 1;
        S.growth_tracker += 1;
        if (S.growth_tracker >= H.growth_interval) {
            if (H.scaling) S.scale = S.scale * (float)H.growth_factor;
            S.growth_tracker = 0;
        }
        const double step = (double)S.t;
        S.decay = (float)(1.0 - H.lr * H.weight_decay);
        S.omb1 = (float)(1.0 - H.beta1);
        S.beta2 = (float)H.beta2;
        S.omb2 = (float)(1.0 - H.beta2);
        S.step_size = (float)(H.lr / (1.0 - pow(H.beta1, step)));
        S.rsb2 = (float)(1.0 / sqrt(1.0 - pow(H.beta2, step)));
        S.eps = (float)H.eps;
    }
    *state = S;
}

__global__ __launch_bounds__(OP_THREADS) void op_update_kernel(OpGroup G, const p2w_optim_state* __restrict__ state) {
    if (state->found_inf) return;                                  // (the same in every thread) p, m and v keep their bytes
    const int k = op_find(G, blockIdx.x);
    float* __restrict__ p = G.t[k].p;
    const float* __restrict__ g = G.t[k].g;
    float* __restrict__ m = G.t[k].m;
    float* __restrict__ v = G.t[k].v;
    const long long n = G.t[k].n;
    const long long base = (long long)(blockIdx.x - G.first[k]) * P2W_OPTIM_CHUNK + 4 * (long long)threadIdx.x;
    const bool wide = op_al16(p) && op_al16(g) && op_al16(m) && op_al16(v);
    const float inv = state->inv_scale, coef = state->coef, decay = state->decay, omb1 = state->omb1, beta2 = state->beta2,
                omb2 = state->omb2, step_size = state->step_size, rsb2 = state->rsb2, eps = state->eps;
    float4 xp[OP_GROUPS], xg[OP_GROUPS], xm[OP_GROUPS], xv[OP_GROUPS];
#pragma unroll
    for (int u = 0; u < OP_GROUPS; ++u) {
        const long long i = base + (long long)u * (4 * OP_THREADS);
        xg[u] = op_load4(g, i, n, wide);
        xp[u] = op_load4(p, i, n, wide);
        xm[u] = op_load4(m, i, n, wide);
        xv[u] = op_load4(v, i, n, wide);
    }
#pragma unroll
    for (int u = 0; u < OP_GROUPS; ++u) {
        const long long i = base + (long long)u * (4 * OP_THREADS);
        if (i >= n) continue;
        float ep[4] = {xp[u].x, xp[u].y, xp[u].z, xp[u].w}, em[4] = {xm[u].x, xm[u].y, xm[u].z, xm[u].w},
              ev[4] = {xv[u].x, xv[u].y, xv[u].z, xv[u].w};
        const float eg[4] = {xg[u].x, xg[u].y, xg[u].z, xg[u].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float un = eg[j] * inv;
            const float gc = un * coef;
            const float p1 = ep[j] * decay;
            const float m1 = em[j] + (gc - em[j]) * omb1;
            const float v1 = ev[j] * beta2 + (omb2 * gc) * gc;
            const float d = sqrtf(v1) * rsb2 + eps;
            ep[j] = p1 - step_size * (m1 / d);
            em[j] = m1;
            ev[j] = v1;
        }
        op_store4(p, i, n, wide, float4{ep[0], ep[1], ep[2], ep[3]});
        op_store4(m, i, n, wide, float4{em[0], em[1], em[2], em[3]});
        op_store4(v, i, n, wide, float4{ev[0], ev[1], ev[2], ev[3]});
    }
}

inline long long op_chunks(long long n) { return (n + P2W_OPTIM_CHUNK - 1) / P2W_OPTIM_CHUNK; }

// one partial sum per chunk
double* op_carve(P2wArena& a, long long chunks) { return a.take<double>((size_t)(chunks ? chunks : 1)); }

inline bool op_finite(double x) { return x - x == 0.0; }

// T in range, every n >= 0, at most 2^40 elements in all -> the number of chunks, else -1
template <class Numel> long long op_count(int32_t T, Numel numel) {
    if (T < 0 || T > P2W_OPTIM_MAX_TENSORS) return -1;
    long long total = 0, chunks = 0;
    for (int32_t k = 0; k < T; ++k) {
        const int64_t n = numel(k);
        if (n < 0 || n > ((int64_t)1 << 40)) return -1;
        total += n;
        if (total > ((int64_t)1 << 40)) return -1;
        chunks += op_chunks(n);
    }
    return chunks;
}

}  // namespace

extern "C" size_t p2w_clip_adamw_ws_size(const int64_t* numel, int32_t T) {
    if (T > 0 && numel == nullptr) return 0;
    const long long chunks = op_count(T, [&](int32_t k) { return numel[k]; });
    if (chunks < 0) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { op_carve(a, chunks); });
}

extern "C" int32_t p2w_clip_adamw(const p2w_optim_tensor* tensors, int32_t T, const p2w_optim_hyper* hyper, p2w_optim_state* state,
                                  void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (T < 0 || T > P2W_OPTIM_MAX_TENSORS) return P2W_EINVAL;
    if (T > 0) P2W_CHECK_PTR(tensors);
    P2W_CHECK_PTR(hyper);
    const long long chunks = op_count(T, [&](int32_t k) { return tensors[k].n; });
    if (chunks < 0) return P2W_EINVAL;
    const p2w_optim_hyper& H = *hyper;
    if (!op_finite(H.lr) || !(H.lr >= 0.0) || !(H.beta1 >= 0.0 && H.beta1 < 1.0) || !(H.beta2 >= 0.0 && H.beta2 < 1.0) ||
        !op_finite(H.eps) || !(H.eps >= 0.0) || !op_finite(H.weight_decay) || !(H.weight_decay >= 0.0) || !op_finite(H.max_norm) ||
        !(H.max_norm >= 0.0) || !op_finite(H.growth_factor) || !(H.growth_factor > 1.0) ||
        !(H.backoff_factor > 0.0 && H.backoff_factor < 1.0) || H.growth_interval < 1 || (H.scaling != 0 && H.scaling != 1))
        return P2W_EINVAL;
    if (chunks == 0) return P2W_OK;                                // no tensor, or none with an element: nothing launched or written
    P2W_CHECK_PTR(state); P2W_CHECK_PTR(ws);
    for (int32_t k = 0; k < T; ++k) {
        if (tensors[k].n == 0) continue;
        P2W_CHECK_PTR(tensors[k].p); P2W_CHECK_PTR(tensors[k].g); P2W_CHECK_PTR(tensors[k].m); P2W_CHECK_PTR(tensors[k].v);
    }
    P2W_CHECK_ALIGN16(state); P2W_CHECK_ALIGN16(ws);
    for (int32_t k = 0; k < T; ++k) {
        if (tensors[k].n == 0) continue;
        const uintptr_t bits = reinterpret_cast<uintptr_t>(tensors[k].p) | reinterpret_cast<uintptr_t>(tensors[k].g) |
                               reinterpret_cast<uintptr_t>(tensors[k].m) | reinterpret_cast<uintptr_t>(tensors[k].v);
        if (bits & 3u) return P2W_EALIGN;
    }
    P2wArena arena(ws);
    double* partial = op_carve(arena, chunks);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;

    hipStream_t s = p2w_s(stream);
    for (int pass = 0; pass < 2; ++pass) {                         // every norm launch, the finalise launch, every update launch
        OpGroup G;
        G.count = 0;
        G.first[0] = 0;
        G.chunk0 = 0;
        auto flush = [&]() {
            if (G.count == 0) return;
            const uint32_t grid = G.first[G.count];
            if (pass == 0) op_norm_kernel<<<grid, OP_THREADS, 0, s>>>(G, state, H.scaling, partial);
            else op_update_kernel<<<grid, OP_THREADS, 0, s>>>(G, state);
            G.chunk0 += grid;
            G.count = 0;
        };
        for (int32_t k = 0; k < T; ++k) {
            if (tensors[k].n == 0) continue;
            G.t[G.count] = tensors[k];
            G.first[G.count + 1] = G.first[G.count] + (uint32_t)op_chunks(tensors[k].n);
            if (++G.count == P2W_OPTIM_GROUP) flush();
        }
        flush();
        if (pass == 0) op_finalise_kernel<<<1, OP_THREADS, 0, s>>>(partial, chunks, H, state);
    }
    return P2W_LAUNCH_STATUS();
}
