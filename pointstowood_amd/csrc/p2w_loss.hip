// Poly-1 focal loss of the reference's training step (pointstowood/src/loss.py:28-73, called at pointstowood/src/trainer.py:174-202):
// per-element loss, its derivative with respect to the logit and the fp64 sum of the losses in ONE pass over the logits and labels.
//
//   element  one workgroup per chunk of P2W_LOSS_CHUNK consecutive elements: every lane reads four groups of four logits and labels
//            with 16-byte loads (all issued before the first use), evaluates the composite and its derivative in fp32 registers,
//            statement by statement as the reference writes it, stores what was asked for with 16-byte stores and adds its losses to
//            an fp64 register in ascending index.  Then the 64 lanes of a wave are summed by the xor-shuffle tree of p2w_eval.hip
//            (32, 16, ..., 1), the four waves are added in wave order and the chunk's sum goes to its word of the workspace.
//   sum      one workgroup: thread t adds the chunk sums t, t + 256, ... in ascending order, the same tree sums the lanes, the waves
//            are added in wave order.  Every word it reads was written by the element pass (no memset), and 0 chunks give 0.
//
// No atomics: every order above depends on n alone, so two calls on the same input give the same bits.
//
// The derivative follows PyTorch's autograd conventions for the same composite: a clamp passes the gradient where its input lies in
// the closed range and gives 0 outside (so a NaN input gives 0), the BCE term's derivative is (sigmoid(z) - y) * weight with the
// unclamped sigmoid of the clamped logit, pow's is e * x^(e - 1) and nothing for e = 0.
#include "p2w_common.h"
#include <math.h>

namespace {

constexpr int LF_THREADS = 256;
constexpr int LF_WAVES = LF_THREADS / P2W_WAVE;
constexpr int LF_GROUPS = P2W_LOSS_CHUNK / (4 * LF_THREADS);      // 16-byte groups per lane and chunk
static_assert(LF_GROUPS * 4 * LF_THREADS == P2W_LOSS_CHUNK, "a chunk is a whole number of rounds of the workgroup");

// the scalars as the reference's fp32 tensors meet them: Python evaluates 1 - x and gamma + 1 in double, the tensor operation rounds
// the result to fp32 once
struct LfParams {
    float epsilon, gamma, gamma1, eps_lo, eps_hi, alpha, alpha1, ls_scale, ls_shift;
    int has_alpha, has_ls;
};

__device__ __forceinline__ double lf_wave_sum(double v) {
#pragma unroll
    for (int off = P2W_WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

// x^e as torch.pow(tensor, scalar) evaluates it: products for 2 and 3, the square root for 0.5, ones for 0 (e is the same in every lane)
__host__ __device__ __forceinline__ float lf_pow(float x, float e) {
    if (e == 0.0f) return 1.0f;
    if (e == 1.0f) return x;
    if (e == 2.0f) return x * x;
    if (e == 3.0f) return (x * x) * x;
    if (e == 0.5f) return sqrtf(x);
    return powf(x, e);
}

// loss of one element; d = its derivative with respect to the logit x (computed only when GRAD).  Compiles for the host too, so
// that the arithmetic can be checked without a GPU.
template <bool GRAD>
__host__ __device__ __forceinline__ float lf_element(float x, float y, float w, const LfParams& P, float& d) {
    const bool z_in = x >= -10.0f && x <= 10.0f;
    const float z = x != x ? x : fminf(fmaxf(x, -10.0f), 10.0f);                   // torch.clamp keeps a NaN
    if (P.has_ls) y = y * P.ls_scale + P.ls_shift;
    const float s = 1.0f / (1.0f + expf(-z));
    const bool p_in = s >= P.eps_lo && s <= P.eps_hi;
    const float p = s != s ? s : fminf(fmaxf(s, P.eps_lo), P.eps_hi);
    const float ce = ((fmaxf(z, 0.0f) - z * y) + log1pf(expf(-fabsf(z)))) * w;
    const bool ce_in = ce <= 100.0f;
    const float ce_c = ce > 100.0f ? 100.0f : ce;
    const float y1 = 1.0f - y;
    const float pt = y * p + y1 * (1.0f - p);
    const bool pt_in = pt >= P.eps_lo && pt <= P.eps_hi;
    const float pt_c = pt != pt ? pt : fminf(fmaxf(pt, P.eps_lo), P.eps_hi);
    const float q = 1.0f - pt_c;
    const float fw = lf_pow(q, P.gamma);
    const bool fw_in = fw <= 2.0f;
    const float fw_c = fw > 2.0f ? 2.0f : fw;
    float fl = fw_c * ce_c;
    float at = 1.0f;
    if (P.has_alpha) {
        at = P.alpha * y + P.alpha1 * y1;
        fl = at * fl;
    }
    const float poly = P.epsilon * lf_pow(q, P.gamma1);
    const bool poly_in = poly <= 100.0f;
    const float poly_c = poly > 100.0f ? 100.0f : poly;
    const float l = fl + poly_c;
    const bool l_in = l >= 0.0f && l <= 100.0f;
    const float out = l != l ? 0.0f : fminf(fmaxf(l, 0.0f), 100.0f);               // the final clamp, then NaN -> 0
    if (GRAD) {
        const float g_fl = l_in ? at : 0.0f;
        const float g_fw = fw_in ? g_fl * ce_c : 0.0f;
        const float g_ce = ce_in ? g_fl * fw_c : 0.0f;
        const float g_poly = (l_in && poly_in) ? P.epsilon : 0.0f;
        float g_q = 0.0f;
        if (P.gamma != 0.0f) g_q = g_fw * (P.gamma * lf_pow(q, P.gamma - 1.0f));
        if (P.gamma1 != 0.0f) g_q = g_q + g_poly * (P.gamma1 * lf_pow(q, P.gamma1 - 1.0f));
        const float g_pt = pt_in ? -g_q : 0.0f;
        const float g_p = p_in ? g_pt * y - g_pt * y1 : 0.0f;
        const float g_z = g_p * ((1.0f - s) * s) + g_ce * ((s - y) * w);
        d = z_in ? g_z : 0.0f;
    }
    return out;
}

// WMODE: 0 = no weight, 1 = one element, 2 = n elements
template <bool GRAD, int WMODE>
__global__ __launch_bounds__(LF_THREADS) void lf_element_kernel(const float* __restrict__ logits, const float* __restrict__ labels,
                                                                const float* __restrict__ weight, long long n, LfParams P,
                                                                float* __restrict__ loss, float* __restrict__ dloss,
                                                                double* __restrict__ partial) {
    __shared__ double s_sum[LF_WAVES];
    const long long base = (long long)blockIdx.x * P2W_LOSS_CHUNK + 4 * (long long)threadIdx.x;
    const float w1 = WMODE == 1 ? weight[0] : 1.0f;
    float4 x[LF_GROUPS], y[LF_GROUPS], w[LF_GROUPS];
#pragma unroll
    for (int u = 0; u < LF_GROUPS; ++u) {
        const long long i = base + (long long)u * (4 * LF_THREADS);
        x[u] = y[u] = float4{0.0f, 0.0f, 0.0f, 0.0f};
        w[u] = float4{w1, w1, w1, w1};
        if (i + 4 <= n) {
            x[u] = *reinterpret_cast<const float4*>(logits + i);
            y[u] = *reinterpret_cast<const float4*>(labels + i);
            if (WMODE == 2) w[u] = *reinterpret_cast<const float4*>(weight + i);
        } else if (i < n) {                                        // the last, incomplete group of the arrays: 1 .. 3 elements
            x[u].x = logits[i];
            y[u].x = labels[i];
            if (WMODE == 2) w[u].x = weight[i];
            if (i + 1 < n) {
                x[u].y = logits[i + 1];
                y[u].y = labels[i + 1];
                if (WMODE == 2) w[u].y = weight[i + 1];
            }
            if (i + 2 < n) {
                x[u].z = logits[i + 2];
                y[u].z = labels[i + 2];
                if (WMODE == 2) w[u].z = weight[i + 2];
            }
        }
    }
    double sum = 0.0;
#pragma unroll
    for (int u = 0; u < LF_GROUPS; ++u) {
        const long long i = base + (long long)u * (4 * LF_THREADS);
        if (i >= n) continue;
        float4 l, d = float4{0.0f, 0.0f, 0.0f, 0.0f};
        l.x = lf_element<GRAD>(x[u].x, y[u].x, w[u].x, P, d.x);
        l.y = lf_element<GRAD>(x[u].y, y[u].y, w[u].y, P, d.y);
        l.z = lf_element<GRAD>(x[u].z, y[u].z, w[u].z, P, d.z);
        l.w = lf_element<GRAD>(x[u].w, y[u].w, w[u].w, P, d.w);
        if (i + 4 <= n) {
            sum += (double)l.x; sum += (double)l.y; sum += (double)l.z; sum += (double)l.w;
            if (loss) *reinterpret_cast<float4*>(loss + i) = l;
            if (GRAD) *reinterpret_cast<float4*>(dloss + i) = d;
        } else {
            sum += (double)l.x;
            if (loss) loss[i] = l.x;
            if (GRAD) dloss[i] = d.x;
            if (i + 1 < n) {
                sum += (double)l.y;
                if (loss) loss[i + 1] = l.y;
                if (GRAD) dloss[i + 1] = d.y;
            }
            if (i + 2 < n) {
                sum += (double)l.z;
                if (loss) loss[i + 2] = l.z;
                if (GRAD) dloss[i + 2] = d.z;
            }
        }
    }
    if (partial == nullptr) return;                                // (the same in every thread)
    sum = lf_wave_sum(sum);
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    if (lane == 0) s_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) {
        double t = s_sum[0];
        for (int k = 1; k < LF_WAVES; ++k) t += s_sum[k];
        partial[blockIdx.x] = t;
    }
}

__global__ __launch_bounds__(LF_THREADS) void lf_sum_kernel(const double* __restrict__ partial, long long chunks,
                                                            double* __restrict__ sum) {
    __shared__ double s_sum[LF_WAVES];
    double t = 0.0;
    for (long long c = threadIdx.x; c < chunks; c += LF_THREADS) t += partial[c];
    t = lf_wave_sum(t);
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    if (lane == 0) s_sum[wave] = t;
    __syncthreads();
    if (threadIdx.x == 0) {
        t = s_sum[0];
        for (int k = 1; k < LF_WAVES; ++k) t += s_sum[k];
        sum[0] = t;
    }
}

inline long long lf_chunks(long long n) { return (n + P2W_LOSS_CHUNK - 1) / P2W_LOSS_CHUNK; }

template <bool GRAD>
void lf_launch(int wmode, unsigned grid, hipStream_t s, const float* logits, const float* labels, const float* weight, long long n,
               const LfParams& P, float* loss, float* dloss, double* partial) {
    if (wmode == 0) lf_element_kernel<GRAD, 0><<<grid, LF_THREADS, 0, s>>>(logits, labels, weight, n, P, loss, dloss, partial);
    else if (wmode == 1) lf_element_kernel<GRAD, 1><<<grid, LF_THREADS, 0, s>>>(logits, labels, weight, n, P, loss, dloss, partial);
    else lf_element_kernel<GRAD, 2><<<grid, LF_THREADS, 0, s>>>(logits, labels, weight, n, P, loss, dloss, partial);
}

// one partial sum per chunk
double* lf_carve(P2wArena& a, long long n) {
    const size_t chunks = (size_t)lf_chunks(n);
    return a.take<double>(chunks ? chunks : 1);
}

}  // namespace

extern "C" size_t p2w_poly1_focal_ws_bytes(int64_t n) {
    if (n < 0 || n > ((int64_t)1 << 40)) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { lf_carve(a, n); });
}

extern "C" int32_t p2w_poly1_focal(const float* logits, const float* labels, const float* weight, int64_t weight_n, int64_t n,
                                   double epsilon, double gamma, double alpha, double label_smoothing, double eps, float* loss,
                                   float* dloss, double* sum, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (n < 0 || n > ((int64_t)1 << 40)) return P2W_EINVAL;
    if (weight == nullptr ? weight_n != 0 : (weight_n != 1 && weight_n != n)) return P2W_EINVAL;
    if (!(epsilon - epsilon == 0.0) || !(gamma - gamma == 0.0) || !(gamma >= 0.0)) return P2W_EINVAL;      // finite, gamma >= 0
    if (!(eps > 0.0 && eps < 0.5)) return P2W_EINVAL;
    if (alpha == alpha && !(alpha - alpha == 0.0)) return P2W_EINVAL;                                      // NaN (not set) or finite
    if (label_smoothing == label_smoothing && !(label_smoothing - label_smoothing == 0.0)) return P2W_EINVAL;
    P2wArena arena(sum ? ws : nullptr);
    double* partial = lf_carve(arena, n);                      // nullptr without `sum`
    if (sum) {
        P2W_CHECK_PTR(ws); P2W_CHECK_ALIGN16(ws);
        if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    }
    const int wmode = weight == nullptr ? 0 : weight_n == 1 ? 1 : 2;
    if (n > 0) {
        P2W_CHECK_PTR(logits); P2W_CHECK_PTR(labels);
        P2W_CHECK_ALIGN16(logits); P2W_CHECK_ALIGN16(labels);
        if (wmode == 2) P2W_CHECK_ALIGN16(weight);
        if (loss) P2W_CHECK_ALIGN16(loss);
        if (dloss) P2W_CHECK_ALIGN16(dloss);
    }
    LfParams P;
    P.epsilon = (float)epsilon;
    P.gamma = (float)gamma;
    P.gamma1 = (float)(gamma + 1.0);
    P.eps_lo = (float)eps;
    P.eps_hi = (float)(1.0 - eps);
    P.has_alpha = alpha == alpha;
    P.alpha = P.has_alpha ? (float)alpha : 0.0f;
    P.alpha1 = P.has_alpha ? (float)(1.0 - alpha) : 0.0f;
    P.has_ls = label_smoothing == label_smoothing;
    P.ls_scale = P.has_ls ? (float)(1.0 - label_smoothing) : 1.0f;
    P.ls_shift = P.has_ls ? (float)(0.5 * label_smoothing) : 0.0f;
    hipStream_t s = p2w_s(stream);
    const long long chunks = lf_chunks(n);
    if (chunks > 0 && (loss || dloss || sum)) {
        if (dloss) lf_launch<true>(wmode, (unsigned)chunks, s, logits, labels, weight, n, P, loss, dloss, partial);
        else lf_launch<false>(wmode, (unsigned)chunks, s, logits, labels, weight, n, P, loss, dloss, partial);
    }
    if (sum) lf_sum_kernel<<<1, LF_THREADS, 0, s>>>(partial, chunks, sum);
    return P2W_LAUNCH_STATUS();
}
