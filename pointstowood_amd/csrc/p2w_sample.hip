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
//
// p2w_cap_subset (second half of the file) runs the same select, count and write steps on the tiles of S segments at once, over the
// float32 keys of an exponential race: the voxeliser's weighted cap.
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

// A tile is the SM_TILE rows from `first` on, as far as they lie before `end`: the row of a wave's iteration `it` (-1 past the end)
__device__ __forceinline__ long long sm_row(long long first, long long end, int it) {
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    const long long i = first + wave * SM_WAVE_ROWS + it * P2W_WAVE + lane;
    return i < end ? i : -1;
}
__device__ __forceinline__ long long sm_first() { return (long long)blockIdx.x * SM_TILE; }   // of the one-segment kernels' tile

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
        const long long i = sm_row(sm_first(), n, it);
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

// The three steps of one tile [first, end) of a range whose histograms are `hist` and of which k rows are wanted.  Both operators of this
// file run them: p2w_random_subset on the tiles of its one range, p2w_cap_subset on the tiles of every segment.  The whole workgroup
// calls them together (they hold barriers).

// pass = 1, 2, 3: digit 3 - pass of the rows whose higher digits are the prefix
__device__ __forceinline__ void sm_select_tile(long long first, long long end, unsigned k, int pass, const unsigned* __restrict__ key,
                                               unsigned* __restrict__ hist, unsigned* s_hist) {
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
    unsigned prefix, want;
    sm_prefix(hist, pass, k, prefix, want);
    const int shift = 24 - 8 * pass;                               // 16, 8, 0
    const unsigned high = prefix >> (shift + 8);
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        const long long i = sm_row(first, end, it);
        if (i < 0) continue;
        const unsigned v = key[i];
        if ((v >> (shift + 8)) == high) atomicAdd(&s_hist[(v >> shift) & 0xffu], 1u);
    }
    sm_flush(s_hist, hist + pass * SM_BINS);
}

// the threshold T and r = k - #{key < T} of the range (the same in every thread); in thread 0, the tile's rows below and equal to T
__device__ __forceinline__ void sm_count_tile(long long first, long long end, unsigned k, const unsigned* __restrict__ key,
                                              const unsigned* __restrict__ hist, int* s_lt, int* s_eq, unsigned& T, unsigned& r,
                                              int& below, int& equal) {
    sm_prefix(hist, 4, k, T, r);
    int lt = 0, eq = 0;
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        const long long i = sm_row(first, end, it);
        const unsigned v = i >= 0 ? key[i] : 0u;
        lt += __popcll(__ballot(i >= 0 && v < T));
        eq += __popcll(__ballot(i >= 0 && v == T));
    }
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    if (lane == 0) { s_lt[wave] = lt; s_eq[wave] = eq; }
    __syncthreads();
    below = 0; equal = 0;
    if (threadIdx.x == 0)
        for (int w = 0; w < SM_WAVES; ++w) { below += s_lt[w]; equal += s_eq[w]; }
}

// L, E: the range's rows below / equal to T before this tile; out[0..k) receives the range's chosen rows
__device__ __forceinline__ void sm_write_tile(long long first, long long end, long long k, unsigned T, long long r, long long L, long long E,
                                              const unsigned* __restrict__ key, int* s_lt, int* s_eq, long long* __restrict__ out) {
    const int lane = threadIdx.x & (P2W_WAVE - 1), wave = threadIdx.x / P2W_WAVE;
    unsigned v[SM_ITERS];
    long long row[SM_ITERS];
    int lt = 0, eq = 0;
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        row[it] = sm_row(first, end, it);
        v[it] = row[it] >= 0 ? key[row[it]] : 0u;
        lt += __popcll(__ballot(row[it] >= 0 && v[it] < T));
        eq += __popcll(__ballot(row[it] >= 0 && v[it] == T));
    }
    if (lane == 0) { s_lt[wave] = lt; s_eq[wave] = eq; }
    __syncthreads();
    for (int w = 0; w < wave; ++w) { L += s_lt[w]; E += s_eq[w]; }                         // ... before this wave
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        const bool below = row[it] >= 0 && v[it] < T, equal = row[it] >= 0 && v[it] == T;
        const unsigned long long mb = __ballot(below), me = __ballot(equal);
        const long long l = L + __popcll(mb & sm_below(lane)), e = E + __popcll(me & sm_below(lane));
        const long long place = l + (e < r ? e : r);
        if ((below || (equal && e < r)) && place < k) out[place] = row[it];
        L += __popcll(mb); E += __popcll(me);
    }
}

__global__ __launch_bounds__(SM_THREADS) void sm_select_kernel(long long n, unsigned k, int pass, const unsigned* __restrict__ key,
                                                               unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[SM_BINS];
    sm_select_tile(sm_first(), n, k, pass, key, hist, s_hist);
}

__global__ __launch_bounds__(SM_THREADS) void sm_count_kernel(long long n, unsigned k, const unsigned* __restrict__ key,
                                                              const unsigned* __restrict__ hist, unsigned* __restrict__ ctl,
                                                              int* __restrict__ cnt, long long tiles) {
    __shared__ int s_lt[SM_WAVES], s_eq[SM_WAVES];
    unsigned T, r;
    int a, b;
    sm_count_tile(sm_first(), n, k, key, hist, s_lt, s_eq, T, r, a, b);
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0) { ctl[0] = T; ctl[1] = r; }
        cnt[blockIdx.x] = a;
        cnt[tiles + blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(SM_THREADS) void sm_write_kernel(long long n, long long k, const unsigned* __restrict__ key,
                                                              const unsigned* __restrict__ ctl, const int* __restrict__ cnt,
                                                              long long tiles, long long* __restrict__ idx_out) {
    __shared__ int s_lt[SM_WAVES], s_eq[SM_WAVES];
    sm_write_tile(sm_first(), n, k, ctl[0], ctl[1], cnt[blockIdx.x], (long long)cnt[tiles + blockIdx.x] - cnt[tiles], key, s_lt, s_eq,
                  idx_out);
}

// ---- p2w_cap_subset: the same selection in every one of S segments of a row space, over keys of an exponential race -----------------
//
// A segment's tiles are the SM_TILE-row pieces of its range (at least one: an empty segment still has its row of idx_out filled), and
// the tiles of all segments are numbered through in segment order, so a large segment is spread over as many workgroups as it has
// tiles while a small one takes one.  No table comes from the host: the tile counts are scanned on the device and a workgroup finds
// its segment by a binary search in the scanned array (all of its threads read the same few words).  Disjoint segments have at most
// n / SM_TILE + S tiles; the grid is that bound, a workgroup past the real total returns.  Every segment has a histogram set, a
// control record and its own offsets in the two scanned counter arrays (the value at its first tile is subtracted).
//
//   plan    zero S x 4 x 256 histogram bins; tiles of every segment -> tile0[0..S], tile0[S] = 0
//   scan    xs_exclusive_scan over S + 1 entries in place: tile0[s] = first tile of segment s, tile0[S] = the total (two levels above
//           4095 segments)
//   keys / select x3 / count / scan (over 2 x the bound) / write: as above, per segment with k_s = min(k, count_s); the first tile of a
//           segment also writes the -1 behind its count
// 1 + (1 or 3) + 1 + 3 + 1 + (1 or 3) + 1 = 9 to 13 launches, whatever S.  Replacement mode is one launch of its own.

struct CpWs { unsigned* key; unsigned* hist; unsigned* ctl; int* tile0; void* scan0; int* cnt; void* scan; long long tiles; };
// key[n]; hist[S][4][256]; ctl[S][2] = T, r; tile0[S + 1]; its scan's workspace; cnt[2 tiles]; the scan's own workspace

CpWs cp_carve(P2wArena& a, long long n, long long S) {
    CpWs W;
    W.tiles = n / SM_TILE + S + 1;
    W.key = a.take<unsigned>((size_t)n);
    W.hist = a.take<unsigned>((size_t)S * 4 * SM_BINS);
    W.ctl = a.take<unsigned>((size_t)S * 2);
    W.tile0 = a.take<int>((size_t)S + 1);
    W.scan0 = a.raw(xs_ws_bytes(S + 1));
    W.cnt = a.take<int>((size_t)(2 * W.tiles));
    W.scan = a.raw(xs_ws_bytes(2 * W.tiles));
    return W;
}

// segment s clamped to the row space: start in [0, n], count in [0, n - start]
__device__ __forceinline__ void cp_range(long long n, const long long* __restrict__ seg_start, const long long* __restrict__ seg_count,
                                         long long s, long long& start, long long& count) {
    const long long a = seg_start[s], c = seg_count[s];
    start = a < 0 ? 0 : (a > n ? n : a);
    count = c < 0 ? 0 : (c > n - start ? n - start : c);
}

struct CpTile { long long seg, first, end, start, count; unsigned k; int j, tile0; };   // seg < 0: no such tile

__device__ __forceinline__ CpTile cp_tile(long long n, int S, long long k, const long long* __restrict__ seg_start,
                                          const long long* __restrict__ seg_count, const int* __restrict__ tile0) {
    CpTile t;
    t.seg = -1;
    if ((int)blockIdx.x >= tile0[S]) return t;
    t.seg = p2w_find_segment(tile0, S, (int)blockIdx.x);
    t.tile0 = tile0[t.seg];
    t.j = (int)blockIdx.x - t.tile0;
    cp_range(n, seg_start, seg_count, t.seg, t.start, t.count);
    t.first = t.start + (long long)t.j * SM_TILE;
    t.end = t.start + t.count;
    t.k = (unsigned)(t.count < k ? t.count : k);
    return t;
}

__global__ __launch_bounds__(SM_THREADS) void cp_plan_kernel(long long n, int S, const long long* __restrict__ seg_start,
                                                             const long long* __restrict__ seg_count, unsigned* __restrict__ hist,
                                                             int* __restrict__ tile0) {
    const long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (i < (long long)S * 4 * SM_BINS) hist[i] = 0u;
    if (i < S) {
        long long start, count;
        cp_range(n, seg_start, seg_count, i, start, count);
        tile0[i] = count > 0 ? (int)((count + SM_TILE - 1) / SM_TILE) : 1;
    }
    if (i == S) tile0[i] = 0;
}

// key = fl32(-log(u) / w) in double, u = (w0 + 0.5) 2^-32 in (0, 1): positive (or +inf), so its pattern orders as an unsigned integer
__device__ __forceinline__ unsigned cp_race_key(float w, unsigned w0) {
    if (!(w > 0.0f && w < __builtin_huge_valf())) return 0xFFFFFFFFu;
    const double u = ((double)w0 + 0.5) * 0x1p-32;
    return __float_as_uint((float)(-log(u) / (double)w));
}

__global__ __launch_bounds__(SM_THREADS) void cp_keys_kernel(long long n, int S, long long k, const long long* __restrict__ seg_start,
                                                             const long long* __restrict__ seg_count, const int* __restrict__ tile0,
                                                             const float* __restrict__ weight, const long long* __restrict__ row_id,
                                                             unsigned k0, unsigned k1, unsigned c1, unsigned c2,
                                                             const unsigned* __restrict__ keys_in, unsigned* __restrict__ key,
                                                             unsigned* __restrict__ keys_out, unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[SM_BINS];
    const CpTile t = cp_tile(n, S, k, seg_start, seg_count, tile0);
    if (t.seg < 0 || t.k == 0u) return;
    s_hist[threadIdx.x] = 0u;
    __syncthreads();
#pragma unroll
    for (int it = 0; it < SM_ITERS; ++it) {
        const long long i = sm_row(t.first, t.end, it);
        if (i < 0) continue;
        unsigned v;
        if (keys_in != nullptr) {
            v = keys_in[i];
        } else {
            unsigned w[4];
            p2w_philox((unsigned)(row_id != nullptr ? row_id[i] : i), c1, c2, P2W_CAP_STREAM, k0, k1, w);
            v = cp_race_key(weight[i], w[0]);
        }
        key[i] = v;
        if (keys_out != nullptr) keys_out[i] = v;
        atomicAdd(&s_hist[v >> 24], 1u);
    }
    sm_flush(s_hist, hist + t.seg * 4 * SM_BINS);
}

__global__ __launch_bounds__(SM_THREADS) void cp_select_kernel(long long n, int S, long long k, const long long* __restrict__ seg_start,
                                                               const long long* __restrict__ seg_count, const int* __restrict__ tile0,
                                                               int pass, const unsigned* __restrict__ key, unsigned* __restrict__ hist) {
    __shared__ unsigned s_hist[SM_BINS];
    const CpTile t = cp_tile(n, S, k, seg_start, seg_count, tile0);
    if (t.seg < 0 || t.k == 0u) return;
    sm_select_tile(t.first, t.end, t.k, pass, key, hist + t.seg * 4 * SM_BINS, s_hist);
}

__global__ __launch_bounds__(SM_THREADS) void cp_count_kernel(long long n, int S, long long k, const long long* __restrict__ seg_start,
                                                              const long long* __restrict__ seg_count, const int* __restrict__ tile0,
                                                              const unsigned* __restrict__ key, const unsigned* __restrict__ hist,
                                                              unsigned* __restrict__ ctl, int* __restrict__ cnt, long long tiles) {
    __shared__ int s_lt[SM_WAVES], s_eq[SM_WAVES];
    const CpTile t = cp_tile(n, S, k, seg_start, seg_count, tile0);
    unsigned T = 0u, r = 0u;
    int a = 0, b = 0;
    if (t.seg >= 0 && t.k != 0u) sm_count_tile(t.first, t.end, t.k, key, hist + t.seg * 4 * SM_BINS, s_lt, s_eq, T, r, a, b);
    if (threadIdx.x == 0) {
        if (t.seg >= 0 && t.j == 0) { ctl[2 * t.seg] = T; ctl[2 * t.seg + 1] = r; }
        cnt[blockIdx.x] = a;                                      // (a workgroup past the last tile writes zeros: the scan reads them)
        cnt[tiles + blockIdx.x] = b;
    }
}

__global__ __launch_bounds__(SM_THREADS) void cp_write_kernel(long long n, int S, long long k, const long long* __restrict__ seg_start,
                                                              const long long* __restrict__ seg_count, const int* __restrict__ tile0,
                                                              const unsigned* __restrict__ key, const unsigned* __restrict__ ctl,
                                                              const int* __restrict__ cnt, long long tiles,
                                                              long long* __restrict__ idx_out) {
    __shared__ int s_lt[SM_WAVES], s_eq[SM_WAVES];
    const CpTile t = cp_tile(n, S, k, seg_start, seg_count, tile0);
    if (t.seg < 0) return;
    long long* out = idx_out + t.seg * k;
    if (t.j == 0)
        for (long long p = t.k + threadIdx.x; p < k; p += SM_THREADS) out[p] = -1;
    if (t.k == 0u) return;
    sm_write_tile(t.first, t.end, t.k, ctl[2 * t.seg], ctl[2 * t.seg + 1], (long long)cnt[blockIdx.x] - cnt[t.tile0],
                  (long long)cnt[tiles + blockIdx.x] - cnt[tiles + t.tile0], key, s_lt, s_eq, out);
}

// replacement mode: draw j of segment s is start + floor(w0 count / 2^32)
__global__ __launch_bounds__(SM_THREADS) void cp_replace_kernel(long long n, int S, long long k, const long long* __restrict__ seg_start,
                                                                const long long* __restrict__ seg_count,
                                                                const long long* __restrict__ row_id, unsigned k0, unsigned k1,
                                                                unsigned c2, long long* __restrict__ idx_out) {
    const long long i = (long long)blockIdx.x * SM_THREADS + threadIdx.x;
    if (i >= S * k) return;
    const long long s = i / k, j = i - s * k;
    long long start, count;
    cp_range(n, seg_start, seg_count, s, start, count);
    long long v = -1;
    if (count > 0) {
        unsigned w[4];
        p2w_philox((unsigned)j, (unsigned)(row_id != nullptr ? row_id[start] : start), c2, P2W_CAP_STREAM ^ 1u, k0, k1, w);
        v = start + __umulhi(w[0], (unsigned)count);
    }
    idx_out[s * k + j] = v;
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

static bool cp_sizes_ok(int64_t n, int64_t S) { return n >= 0 && n <= P2W_CAP_N_MAX && S >= 0 && S <= P2W_CAP_S_MAX; }

extern "C" size_t p2w_cap_subset_ws_size(int64_t n, int64_t S) {
    if (!cp_sizes_ok(n, S)) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { cp_carve(a, n, S); });
}

extern "C" int32_t p2w_cap_subset(int64_t n, const int64_t* seg_start, const int64_t* seg_count, int64_t S, int64_t k, const float* weight,
                                  const int64_t* row_id, uint64_t seed, uint32_t c1, uint32_t c2, const uint32_t* keys, int64_t* idx_out,
                                  uint32_t* keys_out, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (!cp_sizes_ok(n, S) || k < 1 || k > P2W_CAP_N_MAX || S * k > P2W_CAP_OUT_MAX) return P2W_EINVAL;
    if (S == 0) return P2W_OK;
    const bool select = weight != nullptr || keys != nullptr;
    P2wArena arena(ws);
    const CpWs L = cp_carve(arena, n, S);
    P2W_CHECK_PTR(seg_start); P2W_CHECK_PTR(seg_count); P2W_CHECK_PTR(idx_out);
    if (select) { P2W_CHECK_PTR(ws); P2W_CHECK_ALIGN16(ws); }
    if (((reinterpret_cast<uintptr_t>(seg_start) | reinterpret_cast<uintptr_t>(seg_count) | reinterpret_cast<uintptr_t>(idx_out) |
          reinterpret_cast<uintptr_t>(row_id)) & 7u) != 0 ||
        ((reinterpret_cast<uintptr_t>(weight) | reinterpret_cast<uintptr_t>(keys) | reinterpret_cast<uintptr_t>(keys_out)) & 3u) != 0)
        return P2W_EALIGN;
    if (select && ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    hipStream_t s = p2w_s(stream);
    const long long* start = reinterpret_cast<const long long*>(seg_start);
    const long long* count = reinterpret_cast<const long long*>(seg_count);
    const long long* id = reinterpret_cast<const long long*>(row_id);
    long long* out = reinterpret_cast<long long*>(idx_out);
    const unsigned k0 = (unsigned)(seed & 0xffffffffu), k1 = (unsigned)(seed >> 32);
    const int nS = (int)S;
    if (!select) {
        cp_replace_kernel<<<(unsigned)((S * k + SM_THREADS - 1) / SM_THREADS), SM_THREADS, 0, s>>>(n, nS, k, start, count, id, k0, k1, c2, out);
        return P2W_LAUNCH_STATUS();
    }
    const int grid = (int)L.tiles;
    cp_plan_kernel<<<(unsigned)(S * 4 * SM_BINS / SM_THREADS), SM_THREADS, 0, s>>>(n, nS, start, count, L.hist, L.tile0);
    hipError_t e = xs_exclusive_scan(L.scan0, L.tile0, L.tile0, nS + 1, s);
    if (e != hipSuccess) return static_cast<int32_t>(e);
    cp_keys_kernel<<<grid, SM_THREADS, 0, s>>>(n, nS, k, start, count, L.tile0, weight, id, k0, k1, c1, c2, keys, L.key, keys_out, L.hist);
    for (int pass = 1; pass < 4; ++pass) cp_select_kernel<<<grid, SM_THREADS, 0, s>>>(n, nS, k, start, count, L.tile0, pass, L.key, L.hist);
    cp_count_kernel<<<grid, SM_THREADS, 0, s>>>(n, nS, k, start, count, L.tile0, L.key, L.hist, L.ctl, L.cnt, L.tiles);
    e = xs_exclusive_scan(L.scan, L.cnt, L.cnt, (int)(2 * L.tiles), s);
    if (e != hipSuccess) return static_cast<int32_t>(e);
    cp_write_kernel<<<grid, SM_THREADS, 0, s>>>(n, nS, k, start, count, L.tile0, L.key, L.ctl, L.cnt, L.tiles, out);
    return P2W_LAUNCH_STATUS();
}
