// Segmented, weighted C x C confusion matrix: the counting behind the reference's scoring of a classification against truth labels
// (pointstowood/comparetofsct.py:85-106 and pointstowood/src/trainer.py:239-242: precision_score / recall_score / f1_score /
// balanced_accuracy_score of sklearn, each of which re-bins the whole batch on the host).
//
// counts are integers and exact.  The weighted sums are fp64 and must come out with the same bits on every run, so nothing here adds
// floating-point values with atomics (their order would be the arrival order).  The store-and-sum form instead, three launches on the
// caller's stream and no host read:
//
//   table   one workgroup scans the segments: first[s] = the number of chunks of the segments before s, a chunk being
//           P2W_EVAL_CHUNK consecutive points of ONE segment (the last chunk of a segment is shorter).  first[segments] = the chunk
//           count, at most n / P2W_EVAL_CHUNK + segments whatever seg_ptr holds, which is how the host sizes the workspace and the
//           grid without reading seg_ptr.  Boundaries are clamped to [0, n] and a descending pair gives an empty segment, so no
//           later load leaves the arrays even for a seg_ptr that breaks its contract.
//   chunk   one workgroup per chunk finds its segment by bisection of `first`, reads its points with 16-byte loads, and every lane
//           keeps its own count and fp64 sum per cell in registers, its points taken in ascending index (four groups of four
//           points loaded ahead of their adds).  Then, per cell, the 64 lanes of a wave are summed by a fixed xor-shuffle tree
//           (32, 16, ..., 1), the four waves are added in wave order, and the cells go to the chunk's row of the workspace with
//           ordinary vector stores.
//   sum     one workgroup per (segment, cell): thread t adds the rows of chunks t, t + 256, ... of the segment in ascending order,
//           the same shuffle tree sums the lanes, the waves are added in wave order.
//
// Every order above depends on the segment lengths alone, never on scheduling: two calls on the same input give the same bits.
#include "p2w_common.h"
#include <math.h>

namespace {

constexpr int EV_THREADS = 256;
constexpr int EV_WAVES = EV_THREADS / P2W_WAVE;

// the cell grid the chunk pass keeps in registers: classes rounded up to 2, 4 or 8
inline int ev_pad(int classes) { return classes <= 2 ? 2 : classes <= 4 ? 4 : 8; }

struct EvWs { long long* first; int* pcount; double* psum; long long max_chunks; int cells; };

EvWs ev_carve(P2wArena& a, long long n, int segments, int classes) {
    EvWs W;
    W.max_chunks = n / P2W_EVAL_CHUNK + segments;
    W.cells = ev_pad(classes) * ev_pad(classes);
    W.first = a.take<long long>((size_t)segments + 1);
    W.pcount = a.take<int>((size_t)W.max_chunks * (W.cells + 1));      // (+ 1: the chunk's invalid points)
    W.psum = a.take<double>((size_t)W.max_chunks * W.cells);
    return W;
}

__device__ __forceinline__ long long ev_clamp(long long v, long long n) { return v < 0 ? 0 : v > n ? n : v; }

// [a, b) of segment s
__device__ __forceinline__ void ev_segment(const long long* __restrict__ seg_ptr, int s, long long n, long long& a, long long& b) {
    a = seg_ptr ? ev_clamp(seg_ptr[s], n) : 0;
    b = seg_ptr ? ev_clamp(seg_ptr[s + 1], n) : n;
    if (b < a) b = a;
}

__global__ __launch_bounds__(EV_THREADS) void ev_table_kernel(const long long* __restrict__ seg_ptr, long long n, int segments,
                                                              long long max_chunks, long long* __restrict__ first) {
    __shared__ long long wave_total[EV_WAVES];
    __shared__ long long carry_s;
    const int tid = threadIdx.x, lane = tid & (P2W_WAVE - 1), wave = tid / P2W_WAVE;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int s0 = 0; s0 < segments; s0 += EV_THREADS) {
        const int s = s0 + tid;
        long long c = 0;
        if (s < segments) {
            long long a, b;
            ev_segment(seg_ptr, s, n, a, b);
            c = (b - a + P2W_EVAL_CHUNK - 1) / P2W_EVAL_CHUNK;
        }
        long long inc = c;                                         // inclusive scan of the wave
#pragma unroll
        for (int off = 1; off < P2W_WAVE; off <<= 1) {
            const long long v = __shfl_up(inc, off);
            if (lane >= off) inc += v;
        }
        if (lane == P2W_WAVE - 1) wave_total[wave] = inc;
        __syncthreads();
        long long before = carry_s;
        for (int w = 0; w < wave; ++w) before += wave_total[w];
        if (s < segments) {
            const long long f = before + inc - c;
            first[s] = f < max_chunks ? f : max_chunks;
        }
        __syncthreads();
        if (tid == EV_THREADS - 1) carry_s = before + inc;
        __syncthreads();
    }
    if (tid == 0) first[segments] = carry_s < max_chunks ? carry_s : max_chunks;
}

template <typename T>
__device__ __forceinline__ T ev_wave_sum(T v) {
#pragma unroll
    for (int off = P2W_WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

template <int C, bool W>
__global__ __launch_bounds__(EV_THREADS) void ev_chunk_kernel(const float* __restrict__ truth, const float* __restrict__ pred,
                                                              const double* __restrict__ weight, const long long* __restrict__ seg_ptr,
                                                              const long long* __restrict__ first, long long n, int segments,
                                                              int classes, int* __restrict__ pcount, double* __restrict__ psum) {
    constexpr int CELLS = C * C;
    __shared__ int s_count[EV_WAVES][CELLS + 1];
    __shared__ double s_sum[EV_WAVES][CELLS];
    const long long c = blockIdx.x;
    if (c >= first[segments]) return;
    int lo = 0, hi = segments;                                     // the largest s with first[s] <= c: the segment of chunk c
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (first[mid] <= c) lo = mid; else hi = mid;
    }
    long long a, b;
    ev_segment(seg_ptr, lo, n, a, b);
    a += (c - first[lo]) * P2W_EVAL_CHUNK;
    if (b > a + P2W_EVAL_CHUNK) b = a + P2W_EVAL_CHUNK;

    int count[CELLS], bad = 0;
    double sum[CELLS];
#pragma unroll
    for (int k = 0; k < CELLS; ++k) { count[k] = 0; sum[k] = 0.0; }
    const float top = (float)classes;

    auto add = [&](long long i, float t, float p, double w) {
        const bool in = i >= a && i < b;
        bool ok = t >= 0.0f && t < top && t == truncf(t) && p >= 0.0f && p < top && p == truncf(p);     // (false for NaN)
        if (W) ok = ok && w >= 0.0 && w < HUGE_VAL;
        const int cell = (in && ok) ? (int)t * C + (int)p : -1;
        bad += (in && !ok) ? 1 : 0;
#pragma unroll
        for (int k = 0; k < CELLS; ++k) {
            const bool hit = cell == k;
            count[k] += hit ? 1 : 0;
            if (W) sum[k] += hit ? w : 0.0;                        // (w >= 0: adding +0.0 changes no bit of the sum)
        }
    };

    // groups of four points on 16-byte boundaries of the arrays; the points of a group outside [a, b) belong to a neighbour chunk
    long long g = (a >> 2) + threadIdx.x;
    // four groups per lane with every load issued before the first add (an aligned chunk is exactly one such round) ...
    for (; 4 * (g + 3 * EV_THREADS) < b && 4 * (g + 3 * EV_THREADS) + 4 <= n; g += 4 * EV_THREADS) {
        float4 t[4], p[4];
        double2 w[8];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = 4 * (g + u * EV_THREADS);
            t[u] = *reinterpret_cast<const float4*>(truth + i);
            p[u] = *reinterpret_cast<const float4*>(pred + i);
            w[2 * u] = w[2 * u + 1] = double2{0.0, 0.0};
            if (W) {
                w[2 * u] = *reinterpret_cast<const double2*>(weight + i);
                w[2 * u + 1] = *reinterpret_cast<const double2*>(weight + i + 2);
            }
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
            const long long i = 4 * (g + u * EV_THREADS);
            add(i, t[u].x, p[u].x, w[2 * u].x);
            add(i + 1, t[u].y, p[u].y, w[2 * u].y);
            add(i + 2, t[u].z, p[u].z, w[2 * u + 1].x);
            add(i + 3, t[u].w, p[u].w, w[2 * u + 1].y);
        }
    }
    for (; 4 * g < b; g += EV_THREADS) {                           // ... and the groups that are left, one at a time
        const long long i = 4 * g;
        if (i + 4 <= n) {
            const float4 t = *reinterpret_cast<const float4*>(truth + i), p = *reinterpret_cast<const float4*>(pred + i);
            double2 w0 = {0.0, 0.0}, w1 = {0.0, 0.0};
            if (W) {
                w0 = *reinterpret_cast<const double2*>(weight + i);
                w1 = *reinterpret_cast<const double2*>(weight + i + 2);
            }
            add(i, t.x, p.x, w0.x);
            add(i + 1, t.y, p.y, w0.y);
            add(i + 2, t.z, p.z, w1.x);
            add(i + 3, t.w, p.w, w1.y);
        } else {                                                   // the last, incomplete group of the arrays
            for (long long j = i; j < n; ++j) add(j, truth[j], pred[j], W ? weight[j] : 0.0);
        }
    }

    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
#pragma unroll
    for (int k = 0; k < CELLS; ++k) {
        const int cn = ev_wave_sum(count[k]);
        if (lane == 0) s_count[wave][k] = cn;
        if (W) {
            const double sm = ev_wave_sum(sum[k]);
            if (lane == 0) s_sum[wave][k] = sm;
        }
    }
    bad = ev_wave_sum(bad);
    if (lane == 0) s_count[wave][CELLS] = bad;
    __syncthreads();
    const int k = threadIdx.x;
    if (k <= CELLS) {
        int cn = 0;
        for (int w = 0; w < EV_WAVES; ++w) cn += s_count[w][k];
        pcount[c * (CELLS + 1) + k] = cn;
        if (W && k < CELLS) {
            double sm = s_sum[0][k];
            for (int w = 1; w < EV_WAVES; ++w) sm += s_sum[w][k];
            psum[c * CELLS + k] = sm;
        }
    }
}

// blockIdx.x = segment, blockIdx.y = cell of the classes x classes output (row = truth, column = pred); y = classes^2: the invalid points
__global__ __launch_bounds__(EV_THREADS) void ev_sum_kernel(const long long* __restrict__ first, const int* __restrict__ pcount,
                                                            const double* __restrict__ psum, int classes, int pad,
                                                            long long* __restrict__ counts, double* __restrict__ wsum,
                                                            long long* __restrict__ invalid) {
    __shared__ long long s_count[EV_WAVES];
    __shared__ double s_sum[EV_WAVES];
    const int s = blockIdx.x, j = blockIdx.y, cc = classes * classes, cells = pad * pad;
    const int k = j < cc ? (j / classes) * pad + j % classes : cells;
    const bool weighted = wsum != nullptr && j < cc;
    long long cn = 0;
    double sm = 0.0;
    for (long long c = first[s] + threadIdx.x; c < first[s + 1]; c += EV_THREADS) {
        cn += pcount[c * (cells + 1) + k];
        if (weighted) sm += psum[c * cells + k];
    }
    cn = ev_wave_sum(cn);
    if (weighted) sm = ev_wave_sum(sm);
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    if (lane == 0) { s_count[wave] = cn; s_sum[wave] = sm; }
    __syncthreads();
    if (threadIdx.x == 0) {
        cn = s_count[0];
        sm = s_sum[0];
        for (int w = 1; w < EV_WAVES; ++w) { cn += s_count[w]; sm += s_sum[w]; }
        if (j < cc) {
            counts[(size_t)s * cc + j] = cn;
            if (weighted) wsum[(size_t)s * cc + j] = sm;
        } else {
            invalid[s] = cn;
        }
    }
}

template <bool W>
void ev_launch_chunks(int pad, int grid, hipStream_t s, const float* truth, const float* pred, const double* weight,
                      const long long* seg_ptr, const long long* first, long long n, int segments, int classes, int* pcount,
                      double* psum) {
    if (pad == 2) ev_chunk_kernel<2, W><<<grid, EV_THREADS, 0, s>>>(truth, pred, weight, seg_ptr, first, n, segments, classes, pcount, psum);
    else if (pad == 4) ev_chunk_kernel<4, W><<<grid, EV_THREADS, 0, s>>>(truth, pred, weight, seg_ptr, first, n, segments, classes, pcount, psum);
    else ev_chunk_kernel<8, W><<<grid, EV_THREADS, 0, s>>>(truth, pred, weight, seg_ptr, first, n, segments, classes, pcount, psum);
}

}  // namespace

extern "C" size_t p2w_confusion_ws_bytes(int64_t n, int32_t segments, int32_t classes) {
    if (n < 0 || segments < 1 || classes < 2 || classes > P2W_EVAL_MAX_CLASSES) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { ev_carve(a, n, segments, classes); });
}

extern "C" int32_t p2w_confusion(const float* truth, const float* pred, const double* weight, const int64_t* seg_ptr, int64_t n,
                                 int32_t segments, int32_t classes, int64_t* counts, double* wsum, int64_t* invalid, void* ws,
                                 size_t ws_bytes, p2w_stream_t stream) {
    if (n < 0 || n > ((int64_t)1 << 40)) return P2W_EINVAL;
    if (segments < 1 || classes < 2 || classes > P2W_EVAL_MAX_CLASSES) return P2W_EINVAL;
    if (seg_ptr == nullptr && segments != 1) return P2W_EINVAL;
    if ((weight == nullptr) != (wsum == nullptr)) return P2W_EINVAL;
    P2wArena arena(ws);
    const EvWs L = ev_carve(arena, n, segments, classes);
    if (L.max_chunks > 0x7fffffff) return P2W_EINVAL;
    P2W_CHECK_PTR(ws); P2W_CHECK_ALIGN16(ws);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    P2W_CHECK_PTR(counts); P2W_CHECK_PTR(invalid);
    if (n > 0) {
        P2W_CHECK_PTR(truth); P2W_CHECK_PTR(pred);
        P2W_CHECK_ALIGN16(truth); P2W_CHECK_ALIGN16(pred);
        if (weight) P2W_CHECK_ALIGN16(weight);
    }
    hipStream_t s = p2w_s(stream);
    const long long* sp = reinterpret_cast<const long long*>(seg_ptr);
    const int pad = ev_pad(classes);
    ev_table_kernel<<<1, EV_THREADS, 0, s>>>(sp, n, segments, L.max_chunks, L.first);
    if (weight) ev_launch_chunks<true>(pad, (int)L.max_chunks, s, truth, pred, weight, sp, L.first, n, segments, classes, L.pcount, L.psum);
    else ev_launch_chunks<false>(pad, (int)L.max_chunks, s, truth, pred, weight, sp, L.first, n, segments, classes, L.pcount, L.psum);
    ev_sum_kernel<<<dim3((unsigned)segments, (unsigned)(classes * classes + 1)), EV_THREADS, 0, s>>>(
        L.first, L.pcount, L.psum, classes, pad, reinterpret_cast<long long*>(counts), wsum, reinterpret_cast<long long*>(invalid));
    return P2W_LAUNCH_STATUS();
}
