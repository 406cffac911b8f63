// The plot-level cell grid on the device (plotgrid.build on the host: p2w_voxel_sample's cell-sorted keys and p2w_grid,
// p2w_cell_starts' table), shared by p2w_cluster.hip, p2w_pathlen.hip and p2w_geom.hip (the grid searches' run tables and
// knn_refine_kernel): the run of the sorted order that holds a cell, the cell coordinates of a key, and the relaxed agent-scope
// loads the first two files read their shared words with.
//
// (bench.py --full accepts the recorded evaluated-pair counts, profiles/r6_search_evaluated.json, only for the sha256 of
// p2w_geom.hip: an edit of that file - not of this header - needs the counts regenerated with a -DP2W_SLAB_PROFILE build,
// tools/slab_prof.py --json.)
#pragma once
#include "p2w_common.h"

__device__ __forceinline__ int cells_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ unsigned long long cells_load64(const unsigned long long* p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// first position in [lo, hi) of the ascending keys that is not below `key`
__device__ __forceinline__ int cells_lower_bound(const unsigned long long* __restrict__ keys, int lo, int hi, unsigned long long key) {
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (keys[mid] < key) lo = mid + 1; else hi = mid;
    }
    return lo;
}

struct CellGrid {
    const unsigned long long* __restrict__ keys;   // [n] ascending: key = (cz * d1 + cy) * d0 + cx
    const int* __restrict__ cell_start;            // [d0 * d1 * d2 + 1] or null (then the runs are found by bisection)
    int n;
    long long d0, d1, d2;                          // the p2w_grid's dims

    // first position of the sorted order whose key is at least c: cells a .. b are the run [start(a), start(b + 1))
    __device__ __forceinline__ int start(long long c) const {
        return cell_start ? cell_start[c] : cells_lower_bound(keys, 0, n, (unsigned long long)c);
    }
    __device__ __forceinline__ void coords(long long key, long long& cx, long long& cy, long long& cz) const {
        cx = key % d0;
        cy = (key / d0) % d1;
        cz = key / (d0 * d1);
    }
};
