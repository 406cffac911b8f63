// The training feed: gather the voxels of one batch out of a device-resident training set, augment, centre and collate them - what the
// reference does per voxel on the host (pointstowood/src/trainer.py:46-60 TrainingDataset.__getitem__, src/augmentation.py:41-55
// augmentations, PyG's collation) - in two launches on the caller's stream, with no host synchronisation and no host read.
//
// A chunk is P2W_FEED_CHUNK consecutive rows of ONE voxel, counted from the voxel's first row (the last chunk of a voxel is shorter), so
// what a voxel's chunks hold does not depend on the batch it is in.  Chunk ids are handed out without a table and without a scan: slot s
// of the batch owns the ids [g(s), g(s + 1)) with g(s) = out_ptr[s] / CHUNK + s, which is at least ceil(len / CHUNK) ids because
// floor(a + b) >= floor(a) + floor(b); g ascends, so a workgroup finds its slot by bisection of out_ptr, and g(B) = n / CHUNK + B is the
// grid and the workspace size, known to the host from n and B alone.  Ids a slot does not need exit at once.
//
//   sum     one workgroup per chunk, one row per thread (one 16-byte load): the float64 sums of x, y and z over the chunk - lanes by a
//           fixed xor-shuffle tree, the four waves in wave order - stored to the chunk's row of the workspace.  The first B threads of
//           the grid zero sf and nonfinite (there is no memset).
//   write   the same grid.  Every thread adds the partials of its voxel's chunks in ascending order (the same loads in every lane, no
//           LDS), divides by the length in float64, and then per row: d = fl32(x - mean) rounded once from float64, p = d R, the
//           reflectance rule of the voxel's plan record, the outputs, and sf / nonfinite through INTEGER atomics (a maximum of
//           sign-cleared bit patterns and a count: both are order-independent, so the bits are the same on every run).
//
// Every index that reaches memory is clamped: offsets into [0, n] and [0, n_set], a voxel id outside [0, V) is an empty voxel, and a
// voxel is as long as the shorter of its out_ptr and set_ptr ranges.
#include "p2w_common.h"
#include "p2w_philox.h"
#include <math.h>

namespace {

constexpr int FD_THREADS = P2W_FEED_CHUNK;
constexpr int FD_WAVES = FD_THREADS / P2W_WAVE;
static_assert(FD_THREADS == 256, "one row per thread of a 256-thread workgroup");

struct FdWs { double* psum; long long max_chunks; };               // psum[max_chunks][4]: sum x, sum y, sum z, unused

FdWs fd_carve(P2wArena& a, long long n, int B) {
    FdWs W;
    W.max_chunks = n / P2W_FEED_CHUNK + B;
    W.psum = a.take<double>((size_t)W.max_chunks * 4);
    return W;
}

__device__ __forceinline__ long long fd_clamp(long long v, long long hi) { return v < 0 ? 0 : v > hi ? hi : v; }

struct FdChunk {
    int slot, id;          // the batch slot and its voxel
    long long first;       // g(slot): the id of the voxel's chunk 0
    long long src, dst;    // the chunk's first row in the set and in the batch
    long long len;         // rows of the voxel
    int rows;              // rows of this chunk (0: nothing to do)
    long long j;           // chunk within the voxel
};

__device__ __forceinline__ FdChunk fd_locate(const long long* __restrict__ out_ptr, const long long* __restrict__ set_ptr,
                                             const int* __restrict__ ids, int B, int V, long long n, long long n_set, long long c) {
    FdChunk k;
    int lo = 0, hi = B;                                            // the largest s in [0, B) with g(s) <= c
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (fd_clamp(out_ptr[mid], n) / P2W_FEED_CHUNK + mid <= c) lo = mid; else hi = mid;
    }
    k.slot = lo;
    const long long o0 = fd_clamp(out_ptr[lo], n);
    long long o1 = fd_clamp(out_ptr[lo + 1], n);
    if (o1 < o0) o1 = o0;
    k.first = o0 / P2W_FEED_CHUNK + lo;
    k.j = c - k.first;
    k.id = ids[lo];
    long long a0 = 0, a1 = 0;
    if (k.id >= 0 && k.id < V) {
        a0 = fd_clamp(set_ptr[k.id], n_set);
        a1 = fd_clamp(set_ptr[k.id + 1], n_set);
        if (a1 < a0) a1 = a0;
    }
    k.len = o1 - o0 < a1 - a0 ? o1 - o0 : a1 - a0;
    const long long r0 = k.j * P2W_FEED_CHUNK;
    k.rows = (k.j < 0 || r0 >= k.len) ? 0 : (int)(k.len - r0 < P2W_FEED_CHUNK ? k.len - r0 : P2W_FEED_CHUNK);
    k.src = a0 + r0;
    k.dst = o0 + r0;
    return k;
}

template <typename T>
__device__ __forceinline__ T fd_wave_sum(T v) {
#pragma unroll
    for (int off = P2W_WAVE / 2; off >= 1; off >>= 1) v += __shfl_xor(v, off);
    return v;
}

__global__ __launch_bounds__(FD_THREADS) void fd_sum_kernel(const float4* __restrict__ xyzr, const long long* __restrict__ set_ptr,
                                                            const int* __restrict__ ids, const long long* __restrict__ out_ptr, int B,
                                                            int V, long long n, long long n_set, double* __restrict__ psum,
                                                            float* __restrict__ sf, int* __restrict__ nonfinite) {
    __shared__ double s_part[FD_WAVES][3];
    const long long c = blockIdx.x;
    const long long gid = c * FD_THREADS + threadIdx.x;
    if (gid < B) { sf[gid] = 0.0f; nonfinite[gid] = 0; }
    const FdChunk k = fd_locate(out_ptr, set_ptr, ids, B, V, n, n_set, c);
    if (k.rows == 0) return;                                       // (uniform over the workgroup)
    double x = 0.0, y = 0.0, z = 0.0;
    if ((int)threadIdx.x < k.rows) {
        const float4 p = xyzr[k.src + threadIdx.x];
        x = (double)p.x; y = (double)p.y; z = (double)p.z;
    }
    x = fd_wave_sum(x); y = fd_wave_sum(y); z = fd_wave_sum(z);
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    if (lane == 0) { s_part[wave][0] = x; s_part[wave][1] = y; s_part[wave][2] = z; }
    __syncthreads();
    if (threadIdx.x < 3) {
        double s = s_part[0][threadIdx.x];
        for (int w = 1; w < FD_WAVES; ++w) s += s_part[w][threadIdx.x];
        psum[c * 4 + threadIdx.x] = s;
    }
}

// the standard normal of include/p2w.h, bit by bit: u1 in (0, 1] and u2 in [0, 1) from the top 24 bits of words 0 and 1
__device__ __forceinline__ float fd_normal(const unsigned w[4]) {
    const float u1 = (float)((w[0] >> 8) + 1u) * 0x1p-24f;
    const float u2 = (float)(w[1] >> 8) * 0x1p-24f;
    const float r = sqrtf(-2.0f * logf(u1));
    return r * cosf(6.2831855f * u2);
}

__global__ __launch_bounds__(FD_THREADS) void fd_write_kernel(const float4* __restrict__ xyzr, const float* __restrict__ y,
                                                              const long long* __restrict__ set_ptr, const int* __restrict__ ids,
                                                              const long long* __restrict__ out_ptr, int B, int V, long long n,
                                                              long long n_set, const p2w_feed_plan* __restrict__ plan,
                                                              unsigned k0, unsigned k1, unsigned epoch, const float* __restrict__ noise,
                                                              const double* __restrict__ psum, float* __restrict__ pos_out,
                                                              float* __restrict__ refl_out, float* __restrict__ y_out,
                                                              long long* __restrict__ batch_out, float* __restrict__ sf,
                                                              int* __restrict__ nonfinite, unsigned* __restrict__ words_out) {
    const long long c = blockIdx.x;
    const FdChunk k = fd_locate(out_ptr, set_ptr, ids, B, V, n, n_set, c);
    if (k.rows == 0) return;
    const long long chunks = (k.len + P2W_FEED_CHUNK - 1) / P2W_FEED_CHUNK;
    double sx = 0.0, sy = 0.0, sz = 0.0;                           // the voxel's chunks in ascending order
    for (long long q = 0; q < chunks; ++q) {
        const double* p = psum + (k.first + q) * 4;
        sx += p[0]; sy += p[1]; sz += p[2];
    }
    const double cnt = (double)k.len;
    const double mx = sx / cnt, my = sy / cnt, mz = sz / cnt;
    const p2w_feed_plan rec = plan[k.id];

    unsigned bits = 0;
    int bad = 0;
    if ((int)threadIdx.x < k.rows) {
        const long long i = k.src + threadIdx.x, o = k.dst + threadIdx.x;
        const float4 v = xyzr[i];
        const float dx = (float)((double)v.x - mx), dy = (float)((double)v.y - my), dz = (float)((double)v.z - mz);
        float px = dx, py = dy, pz = dz;
        if (rec.rotate) {                                          // p = d R: p_j = fma(dz, R[2][j], fma(dy, R[1][j], dx * R[0][j]))
            px = fmaf(dz, rec.R[6], fmaf(dy, rec.R[3], dx * rec.R[0]));
            py = fmaf(dz, rec.R[7], fmaf(dy, rec.R[4], dx * rec.R[1]));
            pz = fmaf(dz, rec.R[8], fmaf(dy, rec.R[5], dx * rec.R[2]));
        }
        pos_out[3 * o] = px; pos_out[3 * o + 1] = py; pos_out[3 * o + 2] = pz;
        float refl = v.w;
        const bool draw = rec.refl_mode == 2 && noise == nullptr;
        if (draw || words_out != nullptr) {
            unsigned w[4];
            p2w_philox((unsigned)(k.j * P2W_FEED_CHUNK + threadIdx.x), (unsigned)k.id, epoch, P2W_FEED_STREAM, k0, k1, w);
            if (words_out != nullptr) { words_out[4 * o] = w[0]; words_out[4 * o + 1] = w[1]; words_out[4 * o + 2] = w[2]; words_out[4 * o + 3] = w[3]; }
            if (draw) refl = v.w + 0.1f * fd_normal(w);
        }
        if (rec.refl_mode == 2 && noise != nullptr) refl = v.w + noise[o];
        if (rec.refl_mode == 1) refl = 0.0f;
        refl_out[o] = refl;
        y_out[o] = y[i];
        batch_out[o] = k.slot;
        const float nrm = sqrtf((px * px + py * py) + pz * pz);
        bits = __float_as_uint(nrm) & 0x7fffffffu;
        const float fin = ((v.x - v.x) + (v.y - v.y)) + ((v.z - v.z) + (v.w - v.w));       // 0 for a finite row, NaN otherwise
        bad = fin == 0.0f ? 0 : 1;
    }
#pragma unroll
    for (int off = P2W_WAVE / 2; off >= 1; off >>= 1) {
        const unsigned other = __shfl_xor(bits, off);
        bits = other > bits ? other : bits;
    }
    bad = fd_wave_sum(bad);
    if ((threadIdx.x & (P2W_WAVE - 1)) == 0) {
        if (bits != 0) atomicMax(reinterpret_cast<unsigned*>(sf) + k.slot, bits);
        if (bad != 0) atomicAdd(nonfinite + k.slot, bad);
    }
}

}  // namespace

extern "C" size_t p2w_train_feed_ws_size(int64_t n, int32_t B) {
    if (n < 0 || n > ((int64_t)1 << 40) || B < 0) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { fd_carve(a, n, B); });
}

extern "C" int32_t p2w_train_feed(const float* xyzr, const float* y, const int64_t* set_ptr, int64_t n_set, int32_t V, const int32_t* ids,
                                  const int64_t* out_ptr, int32_t B, int64_t n, const p2w_feed_plan* plan, uint64_t seed, uint32_t epoch,
                                  const float* noise, float* pos_out, float* refl_out, float* y_out, int64_t* batch_out, float* sf_out,
                                  int32_t* nonfinite_out, uint32_t* words_out, void* ws, size_t ws_size, p2w_stream_t stream) {
    if (B < 0 || n < 0 || n > ((int64_t)1 << 40) || n_set < 0 || n_set > ((int64_t)1 << 40) || V < 0) return P2W_EINVAL;
    if (B == 0 || n == 0) return P2W_OK;
    if (V < 1) return P2W_EINVAL;
    P2wArena arena(ws);
    const FdWs L = fd_carve(arena, n, B);
    if (L.max_chunks > 0x7fffffff) return P2W_EINVAL;
    P2W_CHECK_PTR(xyzr); P2W_CHECK_PTR(y); P2W_CHECK_PTR(set_ptr); P2W_CHECK_PTR(ids); P2W_CHECK_PTR(out_ptr); P2W_CHECK_PTR(plan);
    P2W_CHECK_PTR(pos_out); P2W_CHECK_PTR(refl_out); P2W_CHECK_PTR(y_out); P2W_CHECK_PTR(batch_out); P2W_CHECK_PTR(sf_out);
    P2W_CHECK_PTR(nonfinite_out); P2W_CHECK_PTR(ws);
    P2W_CHECK_ALIGN16(xyzr); P2W_CHECK_ALIGN16(plan); P2W_CHECK_ALIGN16(ws);
    if (ws_size < arena.bytes()) return P2W_EWORKSPACE;
    hipStream_t s = p2w_s(stream);
    const float4* rows = reinterpret_cast<const float4*>(xyzr);
    const long long* sp = reinterpret_cast<const long long*>(set_ptr);
    const long long* op = reinterpret_cast<const long long*>(out_ptr);
    const int grid = (int)L.max_chunks;
    fd_sum_kernel<<<grid, FD_THREADS, 0, s>>>(rows, sp, ids, op, B, V, n, n_set, L.psum, sf_out, nonfinite_out);
    fd_write_kernel<<<grid, FD_THREADS, 0, s>>>(rows, y, sp, ids, op, B, V, n, n_set, plan, (unsigned)(seed & 0xffffffffu),
                                                (unsigned)(seed >> 32), epoch, noise, L.psum, pos_out, refl_out, y_out,
                                                reinterpret_cast<long long*>(batch_out), sf_out, nonfinite_out, words_out);
    return P2W_LAUNCH_STATUS();
}
