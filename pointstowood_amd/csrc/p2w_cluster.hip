// Euclidean clustering on the GPU: EuclideanCluster.cluster (pointstowood/src/euclidean_clustering.py:13-47).
//
// The reference grows every cluster by a breadth-first search over cKDTree.query_ball_point(points[i], r): a cluster is a
// connected component of the graph whose edges join points at float64 distance <= r.  Here the same components come from a
// lock-free union-find over the plot-level cell grid (p2w_voxel_sample's cell-sorted order and keys, p2w_cell_starts' table):
//
//   link      one thread per point p of the cell-sorted order measures every later point of its own cell and every point of the
//             13 neighbour cells of the half stencil (each unordered pair of adjacent cells is visited from one side only) in
//             float64 on the caller's coordinates, ((dx*dx + dy*dy) + dz*dz) <= r*r with every operation rounded on its own
//             (the build's -ffp-contract=off; no fma), and joins the two trees of every edge: the larger root is hooked under
//             the smaller by a compare-and-swap, so a root is always the smallest point index of its tree;
//   compress  root[i] = the smallest point index of i's component, sizes by integer atomics;
//   number    kept = min_size <= size <= max_size; cluster ids by an exclusive scan of the kept roots in ascending index = the
//             order in which the reference's seed loop meets its clusters; labels int64, -1 for every other point.
//
// The link launch reads the parent array only through agent-scope atomic loads and writes it only through agent-scope
// compare-and-swaps: the CU L1s and the per-XCD L2s are not coherent with each other, so a plain load could return a line
// another workgroup rewrote long ago.  A load may still return an OLDER parent than the latest; parents only ever decrease
// and every older parent is still an ancestor, so such a value only lengthens a walk; a hook on a stale root fails, and the
// value its CAS returns (the true parent) is where the walk continues.  No workgroup waits for another: a failed CAS means
// another hook succeeded.
#include "p2w_cells.h"

namespace {            // the hand-written device-wide exclusive scan (p2w_sort.h), with internal linkage in this translation unit
#include "p2w_sort.h"
}

namespace {

__device__ __forceinline__ bool ec_cas(int* p, int& expected, int desired) {
    return __hip_atomic_compare_exchange_strong(p, &expected, desired, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// an ancestor of x that was a root when its parent word was read; halves the path on the way (parent[x] -> grandparent, by CAS)
__device__ __forceinline__ int ec_find(int* parent, int x) {
    while (true) {
        const int p = cells_load(parent + x);
        if (p == x) return x;
        const int gp = cells_load(parent + p);
        if (gp == p) return p;
        int e = p;
        ec_cas(parent + x, e, gp);                 // (fails harmlessly when another thread moved parent[x] first)
        x = gp;
    }
}

// joins the trees of a and b; returns an ancestor of both (the smaller root at the moment of the hook)
__device__ __forceinline__ int ec_unite(int* parent, int a, int b) {
    while (true) {
        a = ec_find(parent, a);
        b = ec_find(parent, b);
        if (a == b) return a;
        if (a < b) { const int t = a; a = b; b = t; }
        int e = a;
        if (ec_cas(parent + a, e, b)) return b;    // the larger root under the smaller
        a = e;                                     // a was hooked meanwhile: go on from its new parent (< a, so a + b falls)
    }
}

__global__ __launch_bounds__(256) void ec_init_kernel(int n, int* __restrict__ parent, int* __restrict__ size) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    parent[i] = i;
    size[i] = 0;
}

__global__ __launch_bounds__(256) void ec_link_kernel(const double* __restrict__ cs, const int* __restrict__ order,
                                                      const unsigned long long* __restrict__ keys, const int* __restrict__ cell_start,
                                                      const p2w_grid* __restrict__ gridp, int n, double r2, int* parent,
                                                      unsigned long long* __restrict__ pairs_out) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    unsigned long long evaluated = 0;
    if (p < n) {
        const CellGrid g{keys, cell_start, n, gridp->dims[0], gridp->dims[1], gridp->dims[2]};
        const long long d0 = g.d0, d1 = g.d1, d2 = g.d2;
        long long cx, cy, cz;
        g.coords((long long)keys[p], cx, cy, cz);
        const long long xlo = cx > 0 ? cx - 1 : 0, xhi = cx + 1 < d0 ? cx + 1 : cx;
        const double px = cs[3 * (size_t)p], py = cs[3 * (size_t)p + 1], pz = cs[3 * (size_t)p + 2];
        int rp = order[p];                         // an ancestor of p's point, kept up to date by the hooks below
        // half stencil as five runs of the sorted order, each one grid row (cells xlo..xhi): (cy, cz) from p + 1 on (the rest of
        // p's own cell and cell cx + 1), (cy + 1, cz), and (cy - 1 .. cy + 1, cz + 1)
#pragma unroll 1
        for (int t = 0; t < 5; ++t) {
            const long long y = cy + (t == 0 ? 0 : t == 1 ? 1 : t - 3), z = cz + (t < 2 ? 0 : 1);
            if (y < 0 || y >= d1 || z >= d2) continue;
            const long long base = (z * d1 + y) * d0;
            const int a = t == 0 ? p + 1 : g.start(base + xlo);
            const int b = g.start(base + xhi + 1);
            for (int q = a; q < b; ++q) {
                const double dx = px - cs[3 * (size_t)q], dy = py - cs[3 * (size_t)q + 1], dz = pz - cs[3 * (size_t)q + 2];
                const double d = (dx * dx + dy * dy) + dz * dz;
                ++evaluated;
                if (d <= r2) rp = ec_unite(parent, rp, order[q]);
            }
        }
    }
    if (pairs_out) {                               // one atomic per wave
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) evaluated += __shfl_xor(evaluated, off);
        if ((threadIdx.x & 63) == 0 && evaluated) atomicAdd(pairs_out, evaluated);
    }
}

// root[i] = the component's smallest index, size[root] += 1.  The points are visited in the cell-sorted order, so that a wave's
// points mostly share one root and add to its size with one atomic: in point order a component of 10^6 points (the ground
// sheet of a plot) would take 10^6 atomics on one word, 17 ms.  The walks halve the paths as they go, through the same atomic
// helpers, so that the threads behind find them short.
__global__ __launch_bounds__(256) void ec_compress_kernel(int* parent, const int* __restrict__ order, int n, int* __restrict__ root,
                                                          int* __restrict__ size) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= n) return;
    const int i = order[p];
    const int x = ec_find(parent, i);
    root[i] = x;
    const int lead = __ffsll((long long)__ballot(1)) - 1;
    const int r0 = __shfl(x, lead);
    const unsigned long long same = __ballot(x == r0);
    if (x != r0) atomicAdd(size + x, 1);
    else if ((int)(threadIdx.x & 63) == lead) atomicAdd(size + r0, __popcll(same));
}

__device__ __forceinline__ bool ec_kept(int s, long long min_size, long long max_size) { return min_size <= s && s <= max_size; }

__global__ __launch_bounds__(256) void ec_keep_kernel(const int* __restrict__ root, const int* __restrict__ size, int n,
                                                      long long min_size, long long max_size, int* __restrict__ keep) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    keep[i] = (root[i] == i && ec_kept(size[i], min_size, max_size)) ? 1 : 0;
}

// cid = the exclusive scan of the keep flags; counts[0] = kept components, counts[1] += noise points (zeroed before)
__global__ __launch_bounds__(256) void ec_label_kernel(const int* __restrict__ root, const int* __restrict__ size,
                                                       const int* __restrict__ cid, int n, long long min_size, long long max_size,
                                                       long long* __restrict__ labels, int* __restrict__ counts) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const int r = root[i];
    const bool kept = ec_kept(size[r], min_size, max_size);
    labels[i] = kept ? (long long)cid[r] : -1ll;
    const unsigned long long noise = __ballot(!kept);
    if ((int)(threadIdx.x & 63) == __ffsll((long long)__ballot(1)) - 1 && noise) atomicAdd(counts + 1, (int)__popcll(noise));
    if (i == n - 1) counts[0] = cid[i] + ((root[i] == i && ec_kept(size[i], min_size, max_size)) ? 1 : 0);
}

struct EcWs { int *parent, *root, *size, *keep; void* temp; };

EcWs ec_carve(P2wArena& a, long long n) {
    const size_t words = (size_t)(n > 0 ? n : 1);
    EcWs W;
    W.parent = a.take<int>(words);
    W.root = a.take<int>(words);
    W.size = a.take<int>(words);
    W.keep = a.take<int>(words);
    W.temp = a.raw(xs_ws_bytes(n));
    return W;
}

}  // namespace

extern "C" size_t p2w_euclid_cluster_ws_bytes(int64_t n) { return p2w_ws_bytes([&](P2wArena& a) { ec_carve(a, n); }); }

extern "C" int32_t p2w_euclid_cluster(const double* xyz_sorted, const int32_t* order, const uint64_t* keys_sorted, const int32_t* cell_start,
                                      const p2w_grid* grid, int64_t n, double tolerance, int64_t min_size, int64_t max_size,
                                      int32_t stages, int64_t* labels_out, int32_t* counts_out, uint64_t* pairs_out, void* ws,
                                      size_t ws_bytes, p2w_stream_t stream) {
    if (n < 0 || n > (int64_t)0x7fffffff - 1) return P2W_EINVAL;
    if (!(tolerance >= 0.0) || tolerance == HUGE_VAL) return P2W_EINVAL;             // NaN, negative or infinite
    if (stages <= 0 || (stages & ~P2W_CLUSTER_ALL) != 0) return P2W_EINVAL;
    P2W_CHECK_PTR(ws); P2W_CHECK_ALIGN16(ws);
    P2wArena arena(ws);
    const EcWs L = ec_carve(arena, n);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    if (stages & P2W_CLUSTER_LINK) { P2W_CHECK_PTR(xyz_sorted); P2W_CHECK_PTR(keys_sorted); P2W_CHECK_PTR(grid); }
    if (stages & (P2W_CLUSTER_LINK | P2W_CLUSTER_COMPRESS)) P2W_CHECK_PTR(order);
    if (stages & P2W_CLUSTER_NUMBER) { P2W_CHECK_PTR(labels_out); P2W_CHECK_PTR(counts_out); }
    hipStream_t s = p2w_s(stream);
    int *parent = L.parent, *root = L.root, *size = L.size, *keep = L.keep;
    const int nn = (int)n, nblk = p2w_cdiv(nn, 256);
    hipError_t e;
    if (stages & P2W_CLUSTER_LINK) {
        if (pairs_out && (e = hipMemsetAsync(pairs_out, 0, sizeof(uint64_t), s)) != hipSuccess) return (int32_t)e;
        if (nn > 0) {
            ec_init_kernel<<<nblk, 256, 0, s>>>(nn, parent, size);
            ec_link_kernel<<<nblk, 256, 0, s>>>(xyz_sorted, order, reinterpret_cast<const unsigned long long*>(keys_sorted), cell_start,
                                                grid, nn, tolerance * tolerance, parent,
                                                reinterpret_cast<unsigned long long*>(pairs_out));
        }
    }
    if ((stages & P2W_CLUSTER_COMPRESS) && nn > 0) ec_compress_kernel<<<nblk, 256, 0, s>>>(parent, order, nn, root, size);
    if (stages & P2W_CLUSTER_NUMBER) {
        if ((e = hipMemsetAsync(counts_out, 0, 2 * sizeof(int32_t), s)) != hipSuccess) return (int32_t)e;
        if (nn > 0) {
            ec_keep_kernel<<<nblk, 256, 0, s>>>(root, size, nn, (long long)min_size, (long long)max_size, keep);
            if ((e = xs_exclusive_scan(L.temp, keep, keep, nn, s)) != hipSuccess) return (int32_t)e;
            ec_label_kernel<<<nblk, 256, 0, s>>>(root, size, keep, nn, (long long)min_size, (long long)max_size,
                                                 reinterpret_cast<long long*>(labels_out), counts_out);
        }
    }
    return P2W_LAUNCH_STATUS();
}
