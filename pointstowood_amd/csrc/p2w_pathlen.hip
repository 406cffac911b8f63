// Path length from the stem base on the GPU: array_to_graph + extract_path_info (pointstowood/utils/shortest_path.py:6-238).
//
//   knn     p2w_knn_wide_f64: the k <= P2W_MAX_K_WIDE nearest points of every point of one cloud (itself included), exactly in
//           float64 and ordered by (distance, index) - the rows of the reference's NearestNeighbors(n_neighbors=knn).kneighbors(arr)
//           (:63-66).  One thread per point of the plot grid's cell-sorted order visits the cells in Chebyshev rings around its own
//           cell and keeps the k best candidates in a max-heap keyed by (sqrt(((dx*dx + dy*dy) + dz*dz)), index), every operation
//           rounded on its own (the build's -ffp-contract=off).  The grid is built on fp32 coordinates, so a cell boundary is known
//           only to within `slack`: after ring s the points not yet seen are at least s * cell - slack away, and the search stops
//           when the heap's largest distance is below that.
//   grow    p2w_pathlen_grow: the level-synchronous growth loop of :80-187.  step[i] = the step at which i was processed, -1 before.
//           A point claimed during step t holds t, and "processed" inside step t means 0 <= step < t, so every launch sees the set
//           processed before its step began whatever the order of the threads.  Frontier steps run back to back with no host
//           round trip (the frontier count lives on the device, a launch whose frontier is empty does nothing); the host reads the
//           state back in batches and at every empty frontier, where one reduction gives the smallest distance m from a remaining
//           point to a processed entry of its row.  The host then repeats the reference's fp64 `thr += step` until m < thr, one
//           step per addition (:175-176), and launches the gap step (:115-170).  m = inf (no remaining row holds a processed
//           point) ends the growth: the reference would raise its threshold for ever there.
//   sssp    p2w_pathlen_sssp: both directions of every edge into a CSR, then frontier Bellman-Ford on the fp64 bit patterns with a
//           64-bit atomic min (weights >= 0, so the bit order is the numeric order).  fp64 addition is monotone, so the fixed point
//           is the minimum over all paths of the left-fold sum: networkx's Dijkstra (:225) bit for bit.  Optional parents: a
//           breadth-first search over the tight edges (dist[u] + w == dist[v]) gives every reached node its hop count, and the
//           parent is the smallest-index tight neighbour one hop nearer - hop counts fall along every chain, so no cycle can form,
//           zero-weight edges included.
#include "p2w_cells.h"

namespace {            // the hand-written device-wide exclusive scan (p2w_sort.h), with internal linkage in this translation unit
#include "p2w_sort.h"
}

namespace {

constexpr int PL_THREADS = 256;
constexpr unsigned long long PL_INF_BITS = 0x7ff0000000000000ull;   // +inf

__device__ __forceinline__ double pl_dist(const double* __restrict__ xyz, int a, int b) {
    const double dx = xyz[3 * (size_t)a] - xyz[3 * (size_t)b];
    const double dy = xyz[3 * (size_t)a + 1] - xyz[3 * (size_t)b + 1];
    const double dz = xyz[3 * (size_t)a + 2] - xyz[3 * (size_t)b + 2];
    return sqrt((dx * dx + dy * dy) + dz * dz);
}

// ---- kNN ----------------------------------------------------------------------------------------------------------------------

__device__ __forceinline__ bool pl_less(double da, int ia, double db, int ib) { return da < db || (da == db && ia < ib); }

// sift the element at slot 0 down a max-heap of `cnt` entries
__device__ __forceinline__ void pl_sift(double* hd, int* hi, int cnt) {
    int j = 0;
    const double d = hd[0];
    const int id = hi[0];
    while (true) {
        int c = 2 * j + 1;
        if (c >= cnt) break;
        if (c + 1 < cnt && pl_less(hd[c], hi[c], hd[c + 1], hi[c + 1])) ++c;
        if (!pl_less(d, id, hd[c], hi[c])) break;
        hd[j] = hd[c];
        hi[j] = hi[c];
        j = c;
    }
    hd[j] = d;
    hi[j] = id;
}

__global__ __launch_bounds__(PL_THREADS) void pl_knn_kernel(const double* __restrict__ cs, const int* __restrict__ order,
                                                           const unsigned long long* __restrict__ keys, const int* __restrict__ cell_start,
                                                           const p2w_grid* __restrict__ gridp, int n, int k, double slack,
                                                           int* __restrict__ nbr) {
    const int p = blockIdx.x * PL_THREADS + threadIdx.x;
    if (p >= n) return;
    double hd[P2W_MAX_K_WIDE];
    int hi[P2W_MAX_K_WIDE];
    const CellGrid g{keys, cell_start, n, gridp->dims[0], gridp->dims[1], gridp->dims[2]};
    const long long d0 = g.d0, d1 = g.d1, d2 = g.d2;
    const double cell = (double)gridp->res;
    long long cx, cy, cz;
    g.coords((long long)keys[p], cx, cy, cz);
    long long reach = cx > d0 - 1 - cx ? cx : d0 - 1 - cx;                 // the ring beyond which no cell is left
    reach = reach > cy ? reach : cy;
    reach = reach > d1 - 1 - cy ? reach : d1 - 1 - cy;
    reach = reach > cz ? reach : cz;
    reach = reach > d2 - 1 - cz ? reach : d2 - 1 - cz;
    const double px = cs[3 * (size_t)p], py = cs[3 * (size_t)p + 1], pz = cs[3 * (size_t)p + 2];
    int cnt = 0;
    auto run = [&](int a, int b) {
        for (int q = a; q < b; ++q) {
            const double dx = px - cs[3 * (size_t)q], dy = py - cs[3 * (size_t)q + 1], dz = pz - cs[3 * (size_t)q + 2];
            const double d = sqrt((dx * dx + dy * dy) + dz * dz);
            const int id = order[q];
            if (cnt < k) {                                                  // heap not full: sift up
                int j = cnt++;
                while (j > 0) {
                    const int up = (j - 1) >> 1;
                    if (!pl_less(hd[up], hi[up], d, id)) break;
                    hd[j] = hd[up];
                    hi[j] = hi[up];
                    j = up;
                }
                hd[j] = d;
                hi[j] = id;
            } else if (pl_less(d, id, hd[0], hi[0])) {
                hd[0] = d;
                hi[0] = id;
                pl_sift(hd, hi, cnt);
            }
        }
    };
#pragma unroll 1
    for (long long s = 0;; ++s) {
        // ring s: the cells whose largest per-axis offset from (cx, cy, cz) is s, as runs of one grid row each
        // (the offsets are clipped to the grid before the loops: a cloud on a line or in a plane has a grid one cell thick, and its
        // searches run to hundreds of rings - walking the (2 s + 1)^2 rows outside it cost 11 s on 400 collinear points at k = 65)
        const long long za = cz - s < 0 ? -cz : -s, zb = cz + s >= d2 ? d2 - 1 - cz : s;
        const long long ya = cy - s < 0 ? -cy : -s, yb = cy + s >= d1 ? d1 - 1 - cy : s;
        for (long long dz = za; dz <= zb; ++dz) {
            const long long z = cz + dz;
            for (long long dy = ya; dy <= yb; ++dy) {
                const long long y = cy + dy;
                const long long row = (z * d1 + y) * d0;
                if (dz == -s || dz == s || dy == -s || dy == s) {
                    const long long xa = cx - s < 0 ? 0 : cx - s, xb = cx + s >= d0 ? d0 - 1 : cx + s;
                    run(g.start(row + xa), g.start(row + xb + 1));
                } else {
                    if (cx - s >= 0) run(g.start(row + cx - s), g.start(row + cx - s + 1));
                    if (cx + s < d0) run(g.start(row + cx + s), g.start(row + cx + s + 1));
                }
            }
        }
        if (s >= reach) break;                                              // every cell visited
        if (cnt == k && hd[0] * (1.0 + 0x1p-40) < (double)s * cell - slack) break;
    }
    // heap -> ascending (distance, index)
    for (int m = cnt - 1; m > 0; --m) {
        const double d = hd[0];
        const int id = hi[0];
        hd[0] = hd[m];
        hi[0] = hi[m];
        pl_sift(hd, hi, m);
        hd[m] = d;
        hi[m] = id;
    }
    int* out = nbr + (size_t)order[p] * k;
    for (int j = 0; j < cnt; ++j) out[j] = hi[j];
}

// ---- growth ---------------------------------------------------------------------------------------------------------------------
// st[0..2]: frontier counts of the steps t with t % 3 == 0, 1, 2; st[3]: the first step whose frontier was found empty (written by
// every launch with a non-empty frontier: t + 1); st[4]: edges appended; st[5]: set when the edge buffer would overflow; st[6]: gap
// scan minimum (fp64 bits); st[7]: gap scan count of remaining points.

enum { ST_CNT = 0, ST_NEXT = 3, ST_EDGES = 4, ST_OVERFLOW = 5, ST_MIN = 6, ST_LEFT = 7, ST_WORDS = 8 };

__device__ __forceinline__ void pl_append_edges(unsigned long long* st, long long cap, int c, int* __restrict__ edges,
                                                unsigned long long& base) {
    base = c ? atomicAdd(st + ST_EDGES, (unsigned long long)c) : 0ull;
    if (c && (long long)(base + c) > cap) st[ST_OVERFLOW] = 1;
}

__device__ __forceinline__ void pl_put_edge(int* __restrict__ edges, long long cap, unsigned long long at, int a, int b) {
    if ((long long)at < cap) *reinterpret_cast<int2*>(edges + 2 * (size_t)at) = make_int2(a, b);
}

// frontier phase (:86-112): each frontier node g takes the first kp1 entries of its row that were not processed before step t
__global__ __launch_bounds__(PL_THREADS) void pl_frontier_kernel(const double* __restrict__ xyz, const int* __restrict__ nbr, int k,
                                                                int kp1, double gthr, int t, const int* __restrict__ fin,
                                                                int* __restrict__ fout, int* step, unsigned long long* st,
                                                                int* __restrict__ edges, long long cap) {
    const int cnt_in = (int)st[ST_CNT + t % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[ST_CNT + (t + 2) % 3] = 0;                                    // the output counter of step t + 1 (the input of t - 1)
        if (cnt_in > 0) st[ST_NEXT] = (unsigned long long)(t + 1);
    }
    unsigned long long* cnt_out = st + ST_CNT + (t + 1) % 3;
    for (int f = blockIdx.x * PL_THREADS + threadIdx.x; f < cnt_in; f += gridDim.x * PL_THREADS) {
        const int g = fin[f];
        const int* row = nbr + (size_t)g * k;
        int c = 0;
        for (int j = 0, taken = 0; j < k && taken < kp1; ++j) {            // pass 1: how many edges
            const int e = row[j];
            const int s = cells_load(step + e);
            if (s >= 0 && s < t) continue;
            ++taken;
            if (pl_dist(xyz, g, e) <= gthr) ++c;
        }
        unsigned long long at;
        pl_append_edges(st, cap, c, edges, at);
        for (int j = 0, taken = 0; j < k && taken < kp1; ++j) {            // pass 2: the same entries (-1 and t both mean "not yet")
            const int e = row[j];
            const int s = cells_load(step + e);
            if (s >= 0 && s < t) continue;
            ++taken;
            if (pl_dist(xyz, g, e) <= gthr) pl_put_edge(edges, cap, at++, g, e);
            if (s == -1 && atomicCAS(step + e, -1, t) == -1) fout[atomicAdd(cnt_out, 1ull)] = e;
        }
    }
}

// the smallest distance from a remaining point to a processed entry of its row (the first one: rows are ascending), and the count
// of remaining points
__global__ __launch_bounds__(PL_THREADS) void pl_gap_scan_kernel(const double* __restrict__ xyz, const int* __restrict__ nbr, int k,
                                                                int n, const int* __restrict__ step, unsigned long long* st) {
    unsigned long long best = PL_INF_BITS, left = 0;
    for (int i = blockIdx.x * PL_THREADS + threadIdx.x; i < n; i += gridDim.x * PL_THREADS) {
        if (step[i] != -1) continue;
        ++left;
        const int* row = nbr + (size_t)i * k;
        for (int j = 0; j < k; ++j) {
            const int e = row[j];
            if (step[e] >= 0) {
                const unsigned long long b = (unsigned long long)__double_as_longlong(pl_dist(xyz, i, e));
                best = b < best ? b : best;
                break;
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        const unsigned long long o = __shfl_xor(best, off);
        best = o < best ? o : best;
        left += __shfl_xor(left, off);
    }
    if ((threadIdx.x & 63) == 0) {
        if (best != PL_INF_BITS) atomicMin(st + ST_MIN, best);
        if (left) atomicAdd(st + ST_LEFT, left);
    }
}

// gap phase (:115-170) at step t with threshold thr: every remaining point with a processed row entry at d < thr joins the next
// frontier, with edges to the first kp1 processed and the first kp1 unprocessed entries of its row (itself included)
__global__ __launch_bounds__(PL_THREADS) void pl_gap_kernel(const double* __restrict__ xyz, const int* __restrict__ nbr, int k, int n,
                                                           int kp1, double thr, double gthr, int t, int* __restrict__ fout, int* step,
                                                           unsigned long long* st, int* __restrict__ edges, long long cap) {
    unsigned long long* cnt_out = st + ST_CNT + (t + 1) % 3;
    for (int i = blockIdx.x * PL_THREADS + threadIdx.x; i < n; i += gridDim.x * PL_THREADS) {
        if (cells_load(step + i) != -1) continue;
        const int* row = nbr + (size_t)i * k;
        bool gap = false;
        for (int j = 0; j < k; ++j) {
            const int s = cells_load(step + row[j]);
            if (s >= 0 && s < t) { gap = pl_dist(xyz, i, row[j]) < thr; break; }
        }
        if (!gap) continue;
        int c = 0;
        for (int side = 0; side < 2; ++side) {
            for (int j = 0, taken = 0; j < k && taken < kp1; ++j) {
                const int e = row[j];
                const int s = cells_load(step + e);
                if ((s >= 0 && s < t) != (side == 0)) continue;
                ++taken;
                if (pl_dist(xyz, i, e) <= gthr) ++c;
            }
        }
        unsigned long long at;
        pl_append_edges(st, cap, c, edges, at);
        for (int side = 0; side < 2; ++side) {
            for (int j = 0, taken = 0; j < k && taken < kp1; ++j) {
                const int e = row[j];
                const int s = cells_load(step + e);
                if ((s >= 0 && s < t) != (side == 0)) continue;
                ++taken;
                if (pl_dist(xyz, i, e) <= gthr) pl_put_edge(edges, cap, at++, i, e);
            }
        }
        __hip_atomic_store(step + i, t, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        fout[atomicAdd(cnt_out, 1ull)] = i;
    }
}

__global__ void pl_set_kernel(unsigned long long* st, int idx, unsigned long long v) { st[idx] = v; }
__global__ void pl_seti_kernel(int* a, int idx, int v) { a[idx] = v; }

// before the first launch t0 of a chain: its output counter is empty and "the first empty frontier" is not yet known
__global__ void pl_begin_kernel(unsigned long long* st, int t0) {
    st[ST_CNT + (t0 + 1) % 3] = 0;
    st[ST_NEXT] = (unsigned long long)t0;
}

__global__ __launch_bounds__(PL_THREADS) void pl_fill_kernel(int* __restrict__ a, int n, int v) {
    const int i = blockIdx.x * PL_THREADS + threadIdx.x;
    if (i < n) a[i] = v;
}

// ---- SSSP -----------------------------------------------------------------------------------------------------------------------

__global__ __launch_bounds__(PL_THREADS) void pl_degree_kernel(const int* __restrict__ edges, long long m, int* __restrict__ deg) {
    for (long long e = blockIdx.x * (long long)PL_THREADS + threadIdx.x; e < m; e += (long long)gridDim.x * PL_THREADS) {
        const int2 uv = reinterpret_cast<const int2*>(edges)[e];
        if (uv.x == uv.y) continue;                                       // self-loops never shorten a path
        atomicAdd(deg + uv.x, 1);
        atomicAdd(deg + uv.y, 1);
    }
}

__global__ __launch_bounds__(PL_THREADS) void pl_csr_fill_kernel(const double* __restrict__ xyz, const int* __restrict__ edges,
                                                                long long m, int* __restrict__ cursor, int* __restrict__ adj,
                                                                double* __restrict__ w) {
    for (long long e = blockIdx.x * (long long)PL_THREADS + threadIdx.x; e < m; e += (long long)gridDim.x * PL_THREADS) {
        const int2 uv = reinterpret_cast<const int2*>(edges)[e];
        if (uv.x == uv.y) continue;
        const double d = pl_dist(xyz, uv.x, uv.y);
        const int a = atomicAdd(cursor + uv.x, 1), b = atomicAdd(cursor + uv.y, 1);
        adj[a] = uv.y;
        w[a] = d;
        adj[b] = uv.x;
        w[b] = d;
    }
}

__global__ __launch_bounds__(PL_THREADS) void pl_sssp_init_kernel(unsigned long long* __restrict__ dist, int* __restrict__ stamp,
                                                                 int* __restrict__ hop, int n) {
    const int i = blockIdx.x * PL_THREADS + threadIdx.x;
    if (i >= n) return;
    dist[i] = PL_INF_BITS;
    stamp[i] = -1;
    hop[i] = -1;
}

// a search from `base`: its distance (dist, when given) and hop count 0, the frontier of round 0 = {base}
__global__ void pl_seed_kernel(unsigned long long* dist, int* stamp, int* hop, int* fin, int base, unsigned long long* st) {
    if (dist) { dist[base] = 0ull; stamp[base] = 0; }
    hop[base] = 0;
    fin[0] = base;
    st[ST_CNT + 0] = 1;
}

// round t of Bellman-Ford over the nodes improved in round t - 1
__global__ __launch_bounds__(PL_THREADS) void pl_relax_kernel(const int* __restrict__ off, const int* __restrict__ adj,
                                                             const double* __restrict__ w, int t, const int* __restrict__ fin,
                                                             int* __restrict__ fout, unsigned long long* dist, int* stamp,
                                                             unsigned long long* st) {
    const int cnt_in = (int)st[ST_CNT + t % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[ST_CNT + (t + 2) % 3] = 0;
        if (cnt_in > 0) st[ST_NEXT] = (unsigned long long)(t + 1);
    }
    unsigned long long* cnt_out = st + ST_CNT + (t + 1) % 3;
    for (int f = blockIdx.x * PL_THREADS + threadIdx.x; f < cnt_in; f += gridDim.x * PL_THREADS) {
        const int u = fin[f];
        const double du = __longlong_as_double((long long)cells_load64(dist + u));
        for (int a = off[u], b = off[u + 1]; a < b; ++a) {
            const int v = adj[a];
            const unsigned long long nd = (unsigned long long)__double_as_longlong(du + w[a]);
            if (nd < cells_load64(dist + v) && nd < atomicMin(dist + v, nd) && atomicMax(stamp + v, t + 1) < t + 1)
                fout[atomicAdd(cnt_out, 1ull)] = v;
        }
    }
}

// level t of the breadth-first search over tight edges: hop[v] = t + 1 for the first time v is met from a node of level t
__global__ __launch_bounds__(PL_THREADS) void pl_hop_kernel(const int* __restrict__ off, const int* __restrict__ adj,
                                                           const double* __restrict__ w, int t, const int* __restrict__ fin,
                                                           int* __restrict__ fout, const unsigned long long* __restrict__ dist,
                                                           int* hop, unsigned long long* st) {
    const int cnt_in = (int)st[ST_CNT + t % 3];
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        st[ST_CNT + (t + 2) % 3] = 0;
        if (cnt_in > 0) st[ST_NEXT] = (unsigned long long)(t + 1);
    }
    unsigned long long* cnt_out = st + ST_CNT + (t + 1) % 3;
    for (int f = blockIdx.x * PL_THREADS + threadIdx.x; f < cnt_in; f += gridDim.x * PL_THREADS) {
        const int u = fin[f];
        const double du = __longlong_as_double((long long)dist[u]);
        for (int a = off[u], b = off[u + 1]; a < b; ++a) {
            const int v = adj[a];
            if ((unsigned long long)__double_as_longlong(du + w[a]) != dist[v]) continue;
            if (cells_load(hop + v) == -1 && atomicCAS(hop + v, -1, t + 1) == -1) fout[atomicAdd(cnt_out, 1ull)] = v;
        }
    }
}

__global__ __launch_bounds__(PL_THREADS) void pl_finish_kernel(const int* __restrict__ off, const int* __restrict__ adj,
                                                               const double* __restrict__ w, const unsigned long long* __restrict__ dist,
                                                               const int* __restrict__ hop, int n, int base, double* __restrict__ dist_out,
                                                               int* __restrict__ parent) {
    const int v = blockIdx.x * PL_THREADS + threadIdx.x;
    if (v >= n) return;
    const unsigned long long dv = dist[v];
    dist_out[v] = dv == PL_INF_BITS ? __longlong_as_double(0x7ff8000000000000ll) : __longlong_as_double((long long)dv);
    if (!parent) return;
    int best = -1;
    if (dv != PL_INF_BITS && v != base) {
        const int h = hop[v];
        for (int a = off[v], b = off[v + 1]; a < b; ++a) {
            const int u = adj[a];
            if (hop[u] != h - 1 || (best >= 0 && u >= best)) continue;
            if ((unsigned long long)__double_as_longlong(__longlong_as_double((long long)dist[u]) + w[a]) == dv) best = u;
        }
    }
    parent[v] = best;
}

__global__ __launch_bounds__(PL_THREADS) void pl_weights_kernel(const double* __restrict__ xyz, const long long* __restrict__ edges,
                                                               long long m, double* __restrict__ w) {
    for (long long e = blockIdx.x * (long long)PL_THREADS + threadIdx.x; e < m; e += (long long)gridDim.x * PL_THREADS)
        w[e] = pl_dist(xyz, (int)edges[2 * e], (int)edges[2 * e + 1]);
}

struct GrowWs { unsigned long long* st; int* fb[2]; };
GrowWs grow_carve(P2wArena& a, long long n) {
    const size_t nn = (size_t)(n > 0 ? n : 1);
    GrowWs W;
    W.st = a.take<unsigned long long>(ST_WORDS);
    W.fb[0] = a.take<int>(nn);
    W.fb[1] = a.take<int>(nn);
    return W;
}

struct SsspWs { unsigned long long* st; int *off, *cursor, *adj; double* w; unsigned long long* dist; int *stamp, *hop, *fb[2]; void* temp; };
SsspWs sssp_carve(P2wArena& a, long long n, long long m) {
    const size_t nn = (size_t)(n > 0 ? n : 1), mm = (size_t)(m > 0 ? m : 1);
    SsspWs W;
    W.st = a.take<unsigned long long>(ST_WORDS);
    W.off = a.take<int>(nn + 1);
    W.cursor = a.take<int>(nn + 1);
    W.adj = a.take<int>(2 * mm);
    W.w = a.take<double>(2 * mm);
    W.dist = a.take<unsigned long long>(nn);
    W.stamp = a.take<int>(nn);
    W.hop = a.take<int>(nn);
    W.fb[0] = a.take<int>(nn);
    W.fb[1] = a.take<int>(nn);
    W.temp = a.raw(xs_ws_bytes((long long)nn + 1));
    return W;
}

int pl_grid_blocks(long long n) {                                         // grid of the frontier launches (grid-stride loops)
    const long long b = (n + PL_THREADS - 1) / PL_THREADS;
    return (int)(b < 1 ? 1 : b > 2048 ? 2048 : b);
}

hipError_t pl_read_state(const unsigned long long* st, unsigned long long* h, hipStream_t s) {
    hipError_t e = hipMemcpyAsync(h, st, ST_WORDS * sizeof(unsigned long long), hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return e;
    return hipStreamSynchronize(s);
}

// Runs frontier launches `launch(t, fin, fout)` from step t0 on, in batches of growing length with one read-back per batch, until
// the frontier of some step is empty; returns that step in *t_end.  The frontier of step t is in buffer t % 2.
template <typename F>
hipError_t pl_drive(F launch, int t0, unsigned long long* st, int* const fb[2], hipStream_t s, int* t_end, long long* launches) {
    unsigned long long h[ST_WORDS];
    int t = t0, batch = 4;
    pl_begin_kernel<<<1, 1, 0, s>>>(st, t0);
    ++*launches;
    while (true) {
        for (int j = 0; j < batch; ++j, ++t) {
            launch(t, fb[t & 1], fb[(t + 1) & 1]);
            ++*launches;
        }
        hipError_t e = hipGetLastError();
        if (e != hipSuccess) return e;
        if ((e = pl_read_state(st, h, s)) != hipSuccess) return e;
        if ((long long)h[ST_NEXT] < t || h[ST_CNT + t % 3] == 0) {
            *t_end = (long long)h[ST_NEXT] < t ? (int)h[ST_NEXT] : t;
            return hipSuccess;
        }
        batch = batch < 64 ? batch * 2 : 64;
    }
}

}  // namespace

extern "C" int32_t p2w_knn_wide_f64(const double* xyz_sorted, const int32_t* order, const uint64_t* keys_sorted, const int32_t* cell_start,
                                    const p2w_grid* grid, int64_t n, int32_t k, double slack, int32_t* nbr_out, p2w_stream_t stream) {
    if (n < 0 || n > (int64_t)0x7fffffff - 1) return P2W_EINVAL;
    if (k < 1 || k > P2W_MAX_K_WIDE || k > n) return n == 0 && k >= 1 && k <= P2W_MAX_K_WIDE ? 0 : P2W_EINVAL;
    if (!(slack >= 0.0) || slack == HUGE_VAL) return P2W_EINVAL;
    P2W_CHECK_PTR(xyz_sorted); P2W_CHECK_PTR(order); P2W_CHECK_PTR(keys_sorted); P2W_CHECK_PTR(grid); P2W_CHECK_PTR(nbr_out);
    pl_knn_kernel<<<p2w_cdiv(n, PL_THREADS), PL_THREADS, 0, p2w_s(stream)>>>(
        xyz_sorted, order, reinterpret_cast<const unsigned long long*>(keys_sorted), cell_start, grid, (int)n, k, slack, nbr_out);
    return P2W_LAUNCH_STATUS();
}

extern "C" size_t p2w_pathlen_grow_ws_bytes(int64_t n) { return p2w_ws_bytes([&](P2wArena& a) { grow_carve(a, n); }); }

extern "C" int32_t p2w_pathlen_grow(const double* xyz, const int32_t* nbr, int64_t n, int32_t k, int32_t base, int32_t kpairs,
                                    double nbrs_threshold, double nbrs_threshold_step, double graph_threshold, int32_t* step_out,
                                    int32_t* edges_out, int64_t edge_cap, int64_t* info_out, double* threshold_out, void* ws,
                                    size_t ws_bytes, p2w_stream_t stream) {
    if (n < 1 || n > (int64_t)0x7fffffff - 1 || k < 1 || k > P2W_MAX_K_WIDE || k > n) return P2W_EINVAL;
    if (base < 0 || base >= n || kpairs < 0 || edge_cap < 0) return P2W_EINVAL;
    if (nbrs_threshold != nbrs_threshold || !(nbrs_threshold_step > 0.0) || nbrs_threshold_step == HUGE_VAL) return P2W_EINVAL;
    if (graph_threshold != graph_threshold) return P2W_EINVAL;
    P2W_CHECK_PTR(xyz); P2W_CHECK_PTR(nbr); P2W_CHECK_PTR(step_out); P2W_CHECK_PTR(edges_out); P2W_CHECK_PTR(info_out);
    P2W_CHECK_PTR(threshold_out); P2W_CHECK_PTR(ws); P2W_CHECK_ALIGN16(ws);
    P2wArena arena(ws);
    const GrowWs L = grow_carve(arena, n);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    hipStream_t s = p2w_s(stream);
    unsigned long long* st = L.st;
    int* const fb[2] = {L.fb[0], L.fb[1]};
    const int nn = (int)n, kp1 = kpairs + 1 < k ? kpairs + 1 : k, G = pl_grid_blocks(n);
    long long launches = 0, gaps = 0, raises = 0;
    unsigned long long h[ST_WORDS];
    hipError_t e;
    // step[] = -1, step[base] = 0, frontier of step 1 = {base}
    pl_fill_kernel<<<p2w_cdiv(n, PL_THREADS), PL_THREADS, 0, s>>>(step_out, nn, -1);
    if ((e = hipMemsetAsync(st, 0, ST_WORDS * sizeof(unsigned long long), s)) != hipSuccess) return (int32_t)e;
    pl_seti_kernel<<<1, 1, 0, s>>>(step_out, base, 0);
    pl_seti_kernel<<<1, 1, 0, s>>>(fb[1], 0, base);
    pl_set_kernel<<<1, 1, 0, s>>>(st, ST_CNT + 1, 1ull);
    double thr = nbrs_threshold;
    int t = 1;
    bool unreached = false;
    auto frontier = [&](int tt, int* fin, int* fout) {
        pl_frontier_kernel<<<G, PL_THREADS, 0, s>>>(xyz, nbr, k, kp1, graph_threshold, tt, fin, fout, step_out, st, edges_out, edge_cap);
    };
    while (true) {
        int t_end = t;
        if ((e = pl_drive(frontier, t, st, fb, s, &t_end, &launches)) != hipSuccess) return (int32_t)e;
        t = t_end;                                                        // the first step whose frontier is empty
        pl_set_kernel<<<1, 1, 0, s>>>(st, ST_MIN, PL_INF_BITS);
        pl_set_kernel<<<1, 1, 0, s>>>(st, ST_LEFT, 0ull);
        pl_gap_scan_kernel<<<G, PL_THREADS, 0, s>>>(xyz, nbr, k, nn, step_out, st);
        launches += 3;
        if ((e = hipGetLastError()) != hipSuccess) return (int32_t)e;
        if ((e = pl_read_state(st, h, s)) != hipSuccess) return (int32_t)e;
        if (h[ST_OVERFLOW]) return P2W_EWORKSPACE;
        if (h[ST_LEFT] == 0) { --t; break; }                              // all processed: the reference's loop ends after step t - 1
        if (h[ST_MIN] == PL_INF_BITS) { unreached = true; --t; break; }   // no remaining row reaches a processed point
        const double m = __builtin_bit_cast(double, (unsigned long long)h[ST_MIN]);
        while (!(m < thr)) {                                              // steps that find nobody and raise the threshold
            const double nt = thr + nbrs_threshold_step;
            if (nt == thr) { unreached = true; break; }
            thr = nt;
            ++t;
            ++raises;
        }
        if (unreached) { --t; break; }
        pl_set_kernel<<<1, 1, 0, s>>>(st, ST_CNT + (t + 1) % 3, 0ull);   // (pl_drive clears the next one)
        pl_gap_kernel<<<G, PL_THREADS, 0, s>>>(xyz, nbr, k, nn, kp1, thr, graph_threshold, t, fb[(t + 1) & 1], step_out, st, edges_out,
                                               edge_cap);
        launches += 2;
        ++gaps;
        ++t;
    }
    if ((e = pl_read_state(st, h, s)) != hipSuccess) return (int32_t)e;
    if (h[ST_OVERFLOW]) return P2W_EWORKSPACE;
    info_out[0] = (int64_t)h[ST_EDGES];
    info_out[1] = t;                                                      // the last step with a frontier or a raise (p2w.h)
    info_out[2] = gaps;
    info_out[3] = raises;
    info_out[4] = launches;
    info_out[5] = unreached ? 1 : 0;
    *threshold_out = thr;
    return 0;
}

extern "C" size_t p2w_pathlen_sssp_ws_bytes(int64_t n, int64_t n_edges) { return p2w_ws_bytes([&](P2wArena& a) { sssp_carve(a, n, n_edges); }); }

extern "C" int32_t p2w_pathlen_sssp(const double* xyz, const int32_t* edges, int64_t n_edges, int64_t n, int32_t base, double* dist_out,
                                    int32_t* parent_out, int64_t* info_out, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (n < 1 || n > (int64_t)0x7fffffff - 1 || base < 0 || base >= n) return P2W_EINVAL;
    if (n_edges < 0 || 2 * n_edges > (int64_t)0x7fffffff - 1) return P2W_EINVAL;
    P2W_CHECK_PTR(xyz); P2W_CHECK_PTR(dist_out); P2W_CHECK_PTR(info_out); P2W_CHECK_PTR(ws); P2W_CHECK_ALIGN16(ws);
    if (n_edges > 0) P2W_CHECK_PTR(edges);
    P2wArena arena(ws);
    const SsspWs L = sssp_carve(arena, n, n_edges);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    hipStream_t s = p2w_s(stream);
    unsigned long long *st = L.st, *dist = L.dist;
    int *off = L.off, *cursor = L.cursor, *adj = L.adj, *stamp = L.stamp, *hop = L.hop;
    double* w = L.w;
    int* const fb[2] = {L.fb[0], L.fb[1]};
    const int nn = (int)n, G = pl_grid_blocks(n), GE = pl_grid_blocks(n_edges);
    hipError_t e;
    if ((e = hipMemsetAsync(off, 0, sizeof(int) * ((size_t)nn + 1), s)) != hipSuccess) return (int32_t)e;
    if (n_edges > 0) pl_degree_kernel<<<GE, PL_THREADS, 0, s>>>(edges, n_edges, off);
    if ((e = xs_exclusive_scan(L.temp, off, off, nn + 1, s)) != hipSuccess) return (int32_t)e;
    if ((e = hipMemcpyAsync(cursor, off, sizeof(int) * ((size_t)nn + 1), hipMemcpyDeviceToDevice, s)) != hipSuccess) return (int32_t)e;
    if (n_edges > 0) pl_csr_fill_kernel<<<GE, PL_THREADS, 0, s>>>(xyz, edges, n_edges, cursor, adj, w);
    pl_sssp_init_kernel<<<p2w_cdiv(n, PL_THREADS), PL_THREADS, 0, s>>>(dist, stamp, hop, nn);
    pl_seed_kernel<<<1, 1, 0, s>>>(dist, stamp, hop, fb[0], base, st);
    long long launches = 4;
    int rounds = 0, levels = 0;
    auto relax = [&](int t, int* fin, int* fout) {
        pl_relax_kernel<<<G, PL_THREADS, 0, s>>>(off, adj, w, t, fin, fout, dist, stamp, st);
    };
    if ((e = pl_drive(relax, 0, st, fb, s, &rounds, &launches)) != hipSuccess) return (int32_t)e;
    if (parent_out) {
        pl_seed_kernel<<<1, 1, 0, s>>>(nullptr, nullptr, hop, fb[0], base, st);
        auto level = [&](int t, int* fin, int* fout) {
            pl_hop_kernel<<<G, PL_THREADS, 0, s>>>(off, adj, w, t, fin, fout, dist, hop, st);
        };
        if ((e = pl_drive(level, 0, st, fb, s, &levels, &launches)) != hipSuccess) return (int32_t)e;
    }
    pl_finish_kernel<<<p2w_cdiv(n, PL_THREADS), PL_THREADS, 0, s>>>(off, adj, w, dist, hop, nn, base, dist_out, parent_out);
    if ((e = hipGetLastError()) != hipSuccess) return (int32_t)e;
    info_out[0] = rounds;
    info_out[1] = levels;
    info_out[2] = launches + 1;
    return 0;
}

extern "C" int32_t p2w_pathlen_weights(const double* xyz, const int64_t* edges, int64_t n_edges, double* w_out, p2w_stream_t stream) {
    if (n_edges < 0) return P2W_EINVAL;
    if (n_edges == 0) return 0;
    P2W_CHECK_PTR(xyz); P2W_CHECK_PTR(edges); P2W_CHECK_PTR(w_out);
    pl_weights_kernel<<<pl_grid_blocks(n_edges), PL_THREADS, 0, p2w_s(stream)>>>(xyz, reinterpret_cast<const long long*>(edges), n_edges,
                                                                               w_out);
    return P2W_LAUNCH_STATUS();
}
