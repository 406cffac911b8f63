// A uniformly random k-subset of {0 .. n-1}, ascending (include/p2w.h p2w_random_subset): the k rows that are smallest in the order of
// (key_i, i), key_i = word 0 of Philox4x32-10 at counter (i, c1, c2, P2W_SAMPLE_STREAM).  An exact k-th-smallest selection (a
// most-significant-digit radix select over four 8-bit digits) and a stable compaction - not a sort.  Integer arithmetic only.
//
// A tile is SM_TILE = 1024 consecutive rows, one workgroup of four waves; wave w owns the tile's rows [256 w, 256 w + 256) and walks them
// 64 at a time, so a lane's rank among the rows before it is a popcount of a ballot below its own bit.
//
//   zero    the four 256-bin histograms (there is no memset)
//   keys    one tile per workgroup: the generator (or the caller's keys) -> the workspace's key array (and keys_out); histogram of digit 3
//           (bits 31..24) in LDS, the bins that are not empty added to the global histogram 0
//   select  x3, digits 2, 1, 0: every wave of every workgroup first finds the prefix decided so far from the global histograms of the
//           passes before (one wave scans 256 bins: four per lane and a shuffle scan; all waves compute the same thing, so nothing is
//           shared and nobody waits), then the tile's rows whose higher digits match that prefix are counted into the pass's histogram
//   count   the threshold T and r = k - #{key < T} from the four histograms (workgroup 0 stores them for the last launch); per tile the
//           number of rows with key < T and with key == T -> cnt[tile], cnt[tiles + tile]
//   scan    xs_exclusive_scan (p2w_sort.h, one to three launches) over the 2 x tiles counters in place: cnt[t] = rows below T before
//           tile t, cnt[tiles + t] - cnt[tiles] = rows equal to T before tile t
//   write   row i is taken iff key < T, or key == T and fewer than r equal rows precede it; with L and E the rows below and equal to T
//           before row i, its place is L + min(E, r): idx_out[place] = i
//
// 1 + 1 + 3 + 1 + (1 or 3) + 1 = 8 or 10 launches.  Cross-workgroup dependencies are launch boundaries; the only atomics are integer
// additions to histogram bins, so the bits are the same on every run.
#include "p2w_common.h"
#include "p2w_philox.h"

namespace {
#include "p2w_sort.h"       // xs_exclusive_scan, with internal linkage in this translation unit

constexpr int SM_THREADS = 256;
constexpr int SM_WAVES = SM_THREADS / P2W_WAVE;
constexpr int SM_TILE = P2W_SAMPLE_TILE;
constexpr int SM_WAVE_ROWS = SM_TILE / SM_WAVES;                   // consecutive rows of one wave
constexpr int SM_ITERS = SM_WAVE_ROWS / P2W_WAVE;
constexpr int SM_BINS = 256;
static_assert(SM_TILE == 1024 && SM_ITERS == 4, "four waves of 256 consecutive rows, 64 at a time");

struct SmWs { unsigned* key; unsigned* hist; unsigned* ctl; int* cnt; void* scan; long long tiles; };
// key[n]; hist[4][256] (pass p = digit 3 - p); ctl[4] = T, r; cnt[2 tiles]; the scan's own workspace

SmWs sm_carve(P2wArena& a, long long n) {
    SmWs W;
    W.tiles = (n + SM_TILE - 1) / SM_TILE;
    W.key = a.take<unsigned>((size_t)n);
    W.hist = a.take<unsigned>(4 * SM_BINS);
    W.ctl = a.take<unsigned>(4);
    W.cnt = a.take<int>((size_t)(2 * W.tiles));
    W.scan = a.raw(xs_ws_bytes(2 * W.tiles));
    return W;
}

__device__ __forceinline__ unsigned long long sm_below(int lane) { return (1ull << lane) - 1ull; }

// the row of a wave's iteration `it` (-1 past the end)
__device__ __forceinline__ long long sm_row(long long n, int it) {
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    const long long i = (long long)blockIdx.x * SM_TILE + wave * SM_WAVE_ROWS + it * P2W_WAVE + lane;
    return i < n ? i : -1;
}

// One wave, one histogram of 256 bins holding `want` or more rows in all, 1 <= want: the digit d whose bin holds the want-th smallest
// row, and how many-th it is inside that bin (1-based).  The same value in every lane.  A histogram that holds fewer rows than `want`
// cannot occur after a complete pass; digit 255 and rank 1 are returned then, so that nothing downstream indexes out of range.
__device__ __forceinline__ void sm_find(const unsigned* __restrict__ hist, unsigned want, unsigned& digit, unsigned& rank) {
    const int lane = threadIdx.x & (P2W_WAVE - 1);
    const uint4 h = reinterpret_cast<const uint4*>(hist)[lane];
    const unsigned b[4] = {h.x, h.y, h.z, h.w};
    const unsigned sum = (b[0] + b[1]) + (b[2] + b[3]);
    unsigned inc = sum;
#pragma unroll
    for (int d = 1; d < P2W_WAVE; d <<= 1) { const unsigned o = __shfl_up(inc, d); if (lane >= d) inc += o; }
    unsigned before = inc - sum;
    const bool mine = before < want && want <= inc;
    unsigned d = 4 * lane, r = 1;
    if (mine) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (before < want && want <= before + b[e]) { d = 4 * lane + e; r = want - before; }
            before += b[e];
        }
    }
    const unsigned long long who = __ballot(mine);
    const int src = who ? __ffsll((long long)who) - 1 : P2W_WAVE - 1;
    digit = who ? __shfl(d, src) : SM_BINS - 1;
    rank = who ? __shfl(r, src) : 1u;
}

// the digits decided by passes 0 .. passes-1 (as the high bits of a key, low bits zero) and the rank still wanted inside them
__device__ __forceinline__ void sm_prefix(const unsigned* __restrict__ hist, int passes, unsigned k, unsigned& prefix, unsigned& want) {
    prefix = 0; want = k;
    for (int p = 0; p < passes; ++p) {
        unsigned d, r;
        sm_find(hist + p * SM_BINS, want, d, r);
        prefix |= d << (24 - 8 * p);
        want = r;
    }
}

__global__ __launch_bounds__(SM_THREADS) void sm_zero_kernel(unsigned* __restrict__ hist) {
    for (int i = threadIdx.x; i < 4 * SM_BINS; i += SM_THREADS) hist[i] = 0u;
}

__device__ __forceinline__ void sm_flush(const unsigned* s_hist, unsigned* __restrict__ hist) {
    __syncthreads();
    const unsigned c = s_hist[threadIdx.x];                         // SM_THREADS == SM_BINS
    if (c != 0u) atomicAdd(hist + threadIdx.x, c);
}
static_assert(SM_THREADS == SM_BINS, "one bin per thread in sm_flush");

__global__ __launch_bounds__(SM_THREADS) void sm_keys_kernel(long long n, unsigned k0, unsigned k1, unsigned c1, unsigned c2,
                                                             const unsigned* __restrict__ keys_in, unsigned* __restrict__ key,
                                                             unsigned* __restrict__ keys_out, unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[SM_BINS];
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        const long long i = sm_row(n, it);
        if (i < 0) continue;
        unsigned v;
        if (keys_in != nullptr) {
            v = keys_in[i];
        } else {
            unsigned w[4];
            p2w_philox((unsigned)i, c1, c2, P2W_SAMPLE_STREAM, k0, k1, w);
            v = w[0];
        }
        key[i] = v;
        if (keys_out != nullptr) keys_out[i] = v;
        atomicAdd(&s_hist[v >> 24], 1u);
    }
    sm_flush(s_hist, hist);
}

// pass = 1, 2, 3: digit 3 - pass of the rows whose higher digits are the prefix
__global__ __launch_bounds__(SM_THREADS) void sm_select_kernel(long long n, unsigned k, int pass, const unsigned* __restrict__ key,
                                                               unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[SM_BINS];
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    unsigned prefix, want;
    sm_prefix(hist, pass, k, prefix, want);
    const int shift = 24 - 8 * pass;                               // 16, 8, 0
    const unsigned high = prefix >> (shift + 8);
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        const long long i = sm_row(n, it);
        if (i < 0) continue;
        const unsigned v = key[i];
        if ((v >> (shift + 8)) == high) atomicAdd(&s_hist[(v >> shift) & 0xffu], 1u);
    }
    sm_flush(s_hist, hist + pass * SM_BINS);
}

__global__ __launch_bounds__(SM_THREADS) void sm_count_kernel(long long n, unsigned k, const unsigned* __restrict__ key,
                                                              const unsigned* __restrict__ hist, unsigned* __restrict__ ctl,
                                                              int* __restrict__ cnt, long long tiles) {
    __shared__ int s_lt[SM_WAVES], s_eq[SM_WAVES];
    unsigned T, r;
    sm_prefix(hist, 4, k, T, r);
    if (blockIdx.x == 0 && threadIdx.x == 0) { ctl[0] = T; ctl[1] = r; }
    int lt = 0, eq = 0;
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        const long long i = sm_row(n, it);
        const unsigned v = i >= 0 ? key[i] : 0u;
        lt += __popcll(__ballot(i >= 0 && v < T));
        eq += __popcll(__ballot(i >= 0 && v == T));
    }
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    if (lane == 0) { s_lt[wave] = lt; s_eq[wave] = eq; }
    __syncthreads();
    if (threadIdx.x == 0) {
        int a = 0, b = 0;
        for (int w = 0; w < SM_WAVES; ++w) { a += s_lt[w]; b += s_eq[w]; }
        cnt[blockIdx.x] = a;
        cnt[tiles + blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(SM_THREADS) void sm_write_kernel(long long n, long long k, const unsigned* __restrict__ key,
                                                              const unsigned* __restrict__ ctl, const int* __restrict__ cnt,
                                                              long long tiles, long long* __restrict__ idx_out) {
    __shared__ int s_lt[SM_WAVES], s_eq[SM_WAVES];
    const unsigned T = ctl[0];
    const long long r = ctl[1];
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    unsigned v[SM_ITERS];
    long long row[SM_ITERS];
    int lt = 0, eq = 0;
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        row[it] = sm_row(n, it);
        v[it] = row[it] >= 0 ? key[row[it]] : 0u;
        lt += __popcll(__ballot(row[it] >= 0 && v[it] < T));
        eq += __popcll(__ballot(row[it] >= 0 && v[it] == T));
    }
    if (lane == 0) { s_lt[wave] = lt; s_eq[wave] = eq; }
    __syncthreads();
    long long L = cnt[blockIdx.x], E = (long long)cnt[tiles + blockIdx.x] - cnt[tiles];   // rows below / equal to T before this wave
    for (int w = 0; w < wave; ++w) { L += s_lt[w]; E += s_eq[w]; }
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        const bool below = row[it] >= 0 && v[it] < T, equal = row[it] >= 0 && v[it] == T;
        const unsigned long long mb = __ballot(below), me = __ballot(equal);
        const long long l = L + __popcll(mb & sm_below(lane)), e = E + __popcll(me & sm_below(lane));
        const long long place = l + (e < r ? e : r);
        if ((below || (equal && e < r)) && place < k) idx_out[place] = row[it];
        L += __popcll(mb); E += __popcll(me);
    }
}

}  // namespace

extern "C" size_t p2w_random_subset_ws_size(int64_t n) {
    if (n < 0 || n > P2W_SAMPLE_N_MAX) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { sm_carve(a, n); });
}

extern "C" int32_t p2w_random_subset(int64_t n, int64_t k, uint64_t seed, uint32_t c1, uint32_t c2, const uint32_t* keys, int64_t* idx_out,
                                     uint32_t* keys_out, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (n < 0 || n > P2W_SAMPLE_N_MAX || k < 0 || k > n) return P2W_EINVAL;
    if (n == 0 || k == 0) return P2W_OK;
    P2wArena arena(ws);
    const SmWs L = sm_carve(arena, n);
    P2W_CHECK_PTR(idx_out); P2W_CHECK_PTR(ws);
    P2W_CHECK_ALIGN16(ws);
    if ((reinterpret_cast<uintptr_t>(idx_out) & 7u) != 0 || (reinterpret_cast<uintptr_t>(keys) & 3u) != 0 ||
        (reinterpret_cast<uintptr_t>(keys_out) & 3u) != 0) return P2W_EALIGN;
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    hipStream_t s = p2w_s(stream);
    const int grid = (int)L.tiles;
    sm_zero_kernel<<<1, SM_THREADS, 0, s>>>(L.hist);
    sm_keys_kernel<<<grid, SM_THREADS, 0, s>>>(n, (unsigned)(seed & 0xffffffffu), (unsigned)(seed >> 32), c1, c2, keys, L.key, keys_out,
                                               L.hist);
    for (int pass = 1; pass < 4; ++pass) sm_select_kernel<<<grid, SM_THREADS, 0, s>>>(n, (unsigned)k, pass, L.key, L.hist);
    sm_count_kernel<<<grid, SM_THREADS, 0, s>>>(n, (unsigned)k, L.key, L.hist, L.ctl, L.cnt, L.tiles);
    const hipError_t e = xs_exclusive_scan(L.scan, L.cnt, L.cnt, (int)(2 * L.tiles), s);
    if (e != hipSuccess) return static_cast<int32_t>(e);
    sm_write_kernel<<<grid, SM_THREADS, 0, s>>>(n, k, L.key, L.ctl, L.cnt, L.tiles, reinterpret_cast<long long*>(idx_out));
    return P2W_LAUNCH_STATUS();
}
