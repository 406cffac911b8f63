/*
 * p2w.h - C ABI of libp2w_gfx950.so: the MI355X (gfx950) kernels behind the
 * PointsToWood inference forward.
 *
 * Boundary rules:
 *   - extern "C", plain pointers + sizes, no C++/torch types, no exceptions;
 *   - every entry point is re-entrant, keeps no global mutable state, reads no
 *     environment variables, never allocates and never synchronises: the caller
 *     owns all device buffers (worst-case sized) and passes the HIP stream to
 *     launch on; behaviour switches are explicit `flags` / `prec` arguments;
 *   - every entry point returns an int32 status: 0 = OK, > 0 = hipError_t from
 *     the launch, < 0 = a P2W_E* argument error; p2w_strerror() names it;
 *   - all index arrays are int32, all features fp32 row-major, positions are
 *     float4 records "xyzr" = (x, y, z, reflectance), 16-byte aligned;
 *   - ragged batches are CSR: ptr[B+1] (int32, DEVICE memory) over the
 *     concatenated voxels; element counts that are only known on the device
 *     are read from ptr[B] by the kernels, the host passes an upper bound.
 *
 * Each function names the reference call site it replaces (paths relative to
 * the reference repo, harryjfowen/PointsToWood @ 2025-09-12).  The third-party
 * operators themselves (torch-cluster / torch-scatter / torch-geometric) are not
 * vendored by the reference; their semantics are fixed by oracle/ops.py.
 */
#ifndef P2W_H
#define P2W_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void* p2w_stream_t; /* hipStream_t */

#define P2W_OK 0
#define P2W_EINVAL (-1)    /* bad scalar argument (k, sizes, strides)        */
#define P2W_ENULL (-2)     /* required pointer is NULL                        */
#define P2W_EALIGN (-3)    /* pointer / stride not 16-byte aligned            */
#define P2W_EWORKSPACE (-4)/* workspace too small                             */
#define P2W_EUNSUPPORTED (-5)

#define P2W_MAX_K 64       /* neighbours per query of the wave-wide searches (wave64: one lane per slot): the grid searches' limit */
#define P2W_MAX_K_WIDE 100 /* p2w_knn / p2w_ball_query also take 65 .. 100 (torch-cluster's limit) on a one-thread-per-query path */
#define P2W_MAX_K_CONV 32  /* neighbour slots per target of p2w_sa_conv*: one 32-row MFMA tile (Net(k=...) <= 32) */

int32_t p2w_version(void);
const char* p2w_strerror(int32_t code);

/* ---- geometry ---------------------------------------------------------- */

/* xyzr[i] = (pos[i*pos_stride + 0..2], refl[i]); batch[i] = voxel of point i (from ptr).
 * Feeds SAModule.forward's cat(pos[:, :3], reflectance) - pointstowood/src/model.py:109. */
int32_t p2w_pack_xyzr(const float* pos, int32_t pos_stride, const float* refl, const int32_t* ptr, int32_t B,
                      int32_t n, float* xyzr, int32_t* batch, p2w_stream_t stream);

/* Grid sub-sampling of one level: SAModule.voxelsample (model.py:103-106) =
 * PyG voxel_grid -> torch-cluster grid_cluster + PyG consecutive_cluster.
 * In : xyzr[n_bound] (records >= ptr[B] ignored), ptr[B+1], cell size `res`.
 * Out: idx_out[<= n_bound] (index into xyzr of the representative = LARGEST point index of each
 *      occupied cell, ascending cell id i.e. voxel-major), ptr_out[B+1] (CSR of the sampled level;
 *      ptr_out[B] = M), batch_out[M]; order_out[n] (optional, may be NULL) = the input point indices in
 *      ascending (voxel, cell id) order - a spatially coherent visiting order for the searches below.
 * ws : p2w_voxel_sample_ws_bytes(n_bound) bytes of scratch.
 * Neither the outputs nor ws need any initial content (p2w_voxel_sample, p2w_voxel_sample_table, p2w_voxel_grid,
 * p2w_consecutive_cluster alike; only p2w_voxel_sample_table_prepared expects the state p2w_voxel_sample_table_prepare leaves);
 * entries behind the written counts (idx_out[M..], inv_out[n..], cell_start_out[cells + 1 ..] ...) are left as they were. */
/* Geometry of the cell grid a sampling call used (device-resident, written by p2w_voxel_sample): cell (cx, cy, cz)
 * of voxel b has key ((( (b - b_lo) * dims[2] + cz) * dims[1] + cy) * dims[0] + cx. */
typedef struct p2w_grid {
    float lo[3];      /* batch-global minimum of the sampled coordinates = grid origin */
    float res;        /* cell size */
    float hi[3];      /* batch-global maximum */
    int32_t b_lo;     /* first non-empty voxel */
    int64_t dims[3];  /* cells per axis */
} p2w_grid;

size_t p2w_voxel_sample_ws_bytes(int32_t n_bound);
/* Optional outputs (NULL to skip) that make the level searchable through p2w_knn_grid / p2w_ball_query_grid:
 * sorted_keys_out[n] = the cell keys of all input points in ascending order (the order of order_out),
 * cell_keys_out[M] = the key of every representative (ascending = the output order), grid_out = the grid,
 * inv_out[n] = for every input point the index (in the output level) of its cell's representative; rank_sorted_out[n]
 * = the same for the i-th point of the sorted order (order_out[i]). */
int32_t p2w_voxel_sample(const float* xyzr, const int32_t* ptr, int32_t B, int32_t n_bound, float res,
                         int32_t* idx_out, int32_t* ptr_out, int32_t* batch_out, int32_t* order_out,
                         uint64_t* sorted_keys_out, uint64_t* cell_keys_out, p2w_grid* grid_out, int32_t* inv_out,
                         int32_t* rank_sorted_out, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* The same sub-sampling WITHOUT a sort, for batches whose cell grid fits a direct table of `table_cells` entries (the
 * per-voxel forward: a few voxels of a few metres): a cell's key is its table index; representatives by atomic max, ranks by
 * a scan of the occupancy flags, the optional sorted order by a counting-sort scatter (the order of points INSIDE a cell is
 * unspecified - every consumer orders candidates by the index they carry).  Outputs as p2w_voxel_sample.  Whether the grid
 * fits is only known on the device: if it does not, *status_out (device int32) is set to 1 and an EMPTY level is returned
 * (ptr_out = 0, so work already queued behind the call finds nothing to do) - the caller checks it (with the level sizes it reads back anyway) and repeats the level with p2w_voxel_sample.
 * ws: p2w_voxel_sample_table_ws_bytes(n_bound, table_cells) bytes (20 B per table entry). */
size_t p2w_voxel_sample_table_ws_bytes(int32_t n_bound, int64_t table_cells);
/* cell_start_out / cell_start_sorted_out (optional, table_cells + 1 int32 each; the second needs order_out): for every cell
 * key t <= the grid's cell count the position of the first element with key >= t in the sampled level / in the cell-sorted
 * order of the input points (the last used entry = the totals): p2w_knn_grid_indexed / p2w_ball_query_grid_indexed find
 * their candidate runs with one load from such a table instead of bisecting the keys. */
int32_t p2w_voxel_sample_table(const float* xyzr, const int32_t* ptr, int32_t B, int32_t n_bound, float res,
                               int32_t* idx_out, int32_t* ptr_out, int32_t* batch_out, int32_t* order_out,
                               uint64_t* sorted_keys_out, uint64_t* cell_keys_out, p2w_grid* grid_out, int32_t* inv_out,
                               int32_t* rank_sorted_out, int32_t* cell_start_out, int32_t* cell_start_sorted_out,
                               int32_t* status_out, int64_t table_cells, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* out[i] = (x, y, z, bit pattern of order[i]) of xyzr[order[i]] for i < ptr[B]: the records of a level in another
 * (e.g. cell-sorted) order, each carrying its own index - input for the P2W_SEARCH_*_IN_W modes below. */
int32_t p2w_index_records(const float* xyzr, const int32_t* order, const int32_t* ptr, int32_t B, int32_t n_bound,
                          float* out, p2w_stream_t stream);

/* The two halves of p2w_voxel_sample as separate operators (the reference calls them separately,
 * model.py:104-105): cell ids exactly as PyG voxel_grid(pos, size, batch) returns them (int64), and
 * consecutive_cluster(cell) -> (inv[n] = rank of each point's cell, perm[count] = largest point index
 * per cell, ascending cell id).  inv_out may be NULL.  ws: p2w_voxel_sample_ws_bytes(n). */
int32_t p2w_voxel_grid(const float* xyzr, const int32_t* ptr, int32_t B, int32_t n, float res, int64_t* cell_out,
                       void* ws, size_t ws_bytes, p2w_stream_t stream);
int32_t p2w_consecutive_cluster(const int64_t* cell, int32_t n, int32_t* inv_out, int32_t* perm_out,
                                int32_t* count_out, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* Next level's records: out[i] = ((p / sf_b) * sf_b, refl) of src[idx[i]] - the in-place scale /
 * un-scale round trip of model.py:122,124 followed by the slices of :126. */
int32_t p2w_level_gather(const float* xyzr_src, const int32_t* idx, const int32_t* batch_dst, const int32_t* ptr_dst,
                         int32_t B, int32_t m_bound, const float* sf, float* xyzr_dst, p2w_stream_t stream);

/* Search modes (flags of p2w_ball_query / p2w_knn).  Both exist so that a level can be searched in a spatially
 * coherent storage order (p2w_index_records) while results keep referring to the level's own numbering:
 *   X_INDEX_IN_W: candidate c is reported as (and ties / "first cap" are ordered by) the int32 in xyzr_x[c].w, not c.
 *   Q_ROW_IN_W  : the results of query q are written to row (int32 in its record's .w) of nbr / deg, not row q.
 *   BOX (grid searches only): bound the gathered region in x as well - one run per grid row instead of one per z
 *   layer; for grids whose rows are much longer than a workgroup's reach (plot-scale searches). */
#define P2W_SEARCH_X_INDEX_IN_W 1
#define P2W_SEARCH_Q_ROW_IN_W 2
#define P2W_SEARCH_BOX 4

/* Ball query: torch-cluster radius(x, y, r, batch_x, batch_y, max_num_neighbors) - model.py:118.
 * Queries are x[qidx[q]] (qidx NULL = identity).  For query q of voxel b the `cap` candidates of lowest index among
 * those of ptr_x[b]..ptr_x[b+1] with d2 < (float)(r*r) (r is a double, as torch-cluster's host code takes it) are
 * written in ascending index order to nbr[q*cap + 0..deg[q]-1]; remaining slots are -1.  tile_bbox: optional, see
 * p2w_tile_bbox.
 * NaN (p2w_ball_query and p2w_knn): a candidate with a NaN coordinate is never reported, deg counts only admitted candidates
 * (p2w_knn: min(k, candidates without NaN)), and every other query's row is what it would be without that candidate; a query
 * with a NaN coordinate gets deg 0. */
int32_t p2w_ball_query(const float* xyzr_x, const int32_t* ptr_x, const float* xyzr_q, const int32_t* qidx,
                       const int32_t* ptr_q, int32_t B, int32_t m_bound, double r, int32_t cap, int32_t* nbr,
                       int32_t* deg, const float* tile_bbox, int32_t flags, p2w_stream_t stream);

/* Exact brute-force kNN: torch-cluster knn(x, y, k, batch_x, batch_y) - model.py:120 and inside
 * PyG knn_interpolate (model.py:149).  Ascending (d2, index); deg[q] = min(k, #candidates). */
int32_t p2w_knn(const float* xyzr_x, const int32_t* ptr_x, const float* xyzr_q, const int32_t* qidx,
                const int32_t* ptr_q, int32_t B, int32_t m_bound, int32_t k, int32_t* nbr, int32_t* deg,
                const float* tile_bbox, int32_t flags, p2w_stream_t stream);

/* The same two searches over candidates stored in ascending cell-key order of `grid` (keys_x[c] = key of candidate c;
 * both come from the p2w_voxel_sample call that produced or ordered the level).  Only the grid rows within reach of a
 * workgroup's queries are gathered (two binary searches on the keys per z layer) instead of the whole voxel; the
 * results are identical to p2w_knn / p2w_ball_query.  Queries should be spatially coherent (any level in its own
 * storage order is). */
int32_t p2w_knn_grid(const float* xyzr_x, const uint64_t* keys_x, const int32_t* ptr_x, const p2w_grid* grid,
                     const float* xyzr_q, const int32_t* qidx, const int32_t* ptr_q, int32_t B, int32_t m_bound,
                     int32_t k, int32_t* nbr, int32_t* deg, const float* hint, int32_t flags, p2w_stream_t stream);
/* hint (optional, NULL = none): hint[q] = an upper bound of query q's k-th squared distance (+inf = none for q).  A
 * workgroup whose queries all have one skips the density probe and gathers exactly the box its bounds require; the
 * bound is verified (k candidates must turn up inside it), a wrong one only costs a rescan.  p2w_knn_hint2 derives
 * bounds for k <= 2 when the candidates are the sampled level of the queries' level (the interpolation searches):
 * rank[i] = index of query i's cell representative among the candidates (p2w_voxel_sample's inv_out, or
 * rank_sorted_out when the queries are given in sorted order).
 * The rule: hint[i] = max(d2 to the own representative xyzr_c[rank[i]], smallest d2 to the representatives rank[i +- s], s = 1 .. 8,
 * that differ from the own one - positions inside query i's own voxel only, no further s once one has been seen and s >= 2),
 * +inf when no second representative turns up (a voxel of one point or of one cell). */
int32_t p2w_knn_hint2(const float* xyzr_q, const int32_t* rank, const int32_t* ptr_q, int32_t B, int32_t m_bound,
                      const float* xyzr_c, float* hint, p2w_stream_t stream);
int32_t p2w_ball_query_grid(const float* xyzr_x, const uint64_t* keys_x, const int32_t* ptr_x, const p2w_grid* grid,
                            const float* xyzr_q, const int32_t* qidx, const int32_t* ptr_q, int32_t B, int32_t m_bound,
                            double r, int32_t cap, int32_t* nbr, int32_t* deg, int32_t flags, p2w_stream_t stream);
/* p2w_voxel_sample_table on a workspace whose between-calls state (24 bytes of bounding-box words at their atomics' identities, one
 * counter at zero) is already in place: p2w_voxel_sample_table_prepare(ws) establishes it once on a fresh (or foreign-written)
 * workspace, every p2w_voxel_sample_table[_prepared] call leaves it in place again - so the three sub-samplings of a forward
 * (model.py:103-106, once per SA level) take 5 launches each instead of 7, none of them a memset.  Same arguments, same results. */
int32_t p2w_voxel_sample_table_prepare(void* ws, size_t ws_bytes, p2w_stream_t stream);
int32_t p2w_voxel_sample_table_prepared(const float* xyzr, const int32_t* ptr, int32_t B, int32_t n_bound, float res,
                                        int32_t* idx_out, int32_t* ptr_out, int32_t* batch_out, int32_t* order_out,
                                        uint64_t* sorted_keys_out, uint64_t* cell_keys_out, p2w_grid* grid_out, int32_t* inv_out,
                                        int32_t* rank_sorted_out, int32_t* cell_start_out, int32_t* cell_start_sorted_out,
                                        int32_t* status_out, int64_t table_cells, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* The same two searches with the sampler's cell -> position table of the candidates (p2w_voxel_sample_table's
 * cell_start_out when the candidates are the level it produced, cell_start_sorted_out when they are its input points in
 * cell-sorted order; NULL = bisect keys_x as p2w_knn_grid does): identical results, the run tables cost one load per run end. */
int32_t p2w_knn_grid_indexed(const float* xyzr_x, const uint64_t* keys_x, const int32_t* ptr_x, const p2w_grid* grid,
                             const int32_t* cell_start, const float* xyzr_q, const int32_t* qidx, const int32_t* ptr_q, int32_t B,
                             int32_t m_bound, int32_t k, int32_t* nbr, int32_t* deg, const float* hint, int32_t flags,
                             p2w_stream_t stream);
int32_t p2w_ball_query_grid_indexed(const float* xyzr_x, const uint64_t* keys_x, const int32_t* ptr_x, const p2w_grid* grid,
                                    const int32_t* cell_start, const float* xyzr_q, const int32_t* qidx, const int32_t* ptr_q,
                                    int32_t B, int32_t m_bound, double r, int32_t cap, int32_t* nbr, int32_t* deg, int32_t flags,
                                    p2w_stream_t stream);

/* ---- plot scale: back-projection of the classification onto the original points (predicter.py:107-142) ---- */

/* order_out[i] = index of the i-th record in ascending Morton (Z-curve) order of its cell in `grid` (21 bits per
 * axis, cells clamped to the grid): consecutive records are close in all three dimensions - the query order for
 * P2W_SEARCH_BOX searches over a plot.  A cell is floor((v - lo) / res) per axis in fp32, below 0 -> 0, above 2^21 - 1 -> 2^21 - 1,
 * NaN -> 0; bit b of axis a goes to bit 3 b + a of the key (x lowest); records of equal keys keep their input order.
 * xyzr[n][4], ws: 16-byte aligned, p2w_morton_order_ws_bytes(n) bytes.
 * Status: n == 0 -> P2W_OK (nothing is read); a NULL xyzr / grid / order_out / ws -> P2W_ENULL; xyzr or ws not 16-byte aligned ->
 * P2W_EALIGN; n < 0 -> P2W_EINVAL; ws_bytes too small -> P2W_EWORKSPACE (order_out is not written). */
size_t p2w_morton_order_ws_bytes(int32_t n);
int32_t p2w_morton_order(const float* xyzr, int32_t n, const p2w_grid* grid, int32_t* order_out, void* ws, size_t ws_bytes,
                         p2w_stream_t stream);

/* ---- plot -> voxels: the grid step of the reference's voxeliser (pointstowood/src/preprocessing.py:55-64, Voxelise.grid) -------
 * cell_out[i] = PyG voxel_grid(P, size) with batch = None over ALL D <= 16 columns of the row-major table P[n, ld] (the
 * reference hands the whole point table - x, y, z, reflectance, ..., n_z - to voxel_grid): sum_d trunc((P_id - lo_d) / size) *
 * stride_d with the column minima lo_d and the running products of the per-column cell counts as strides (fp32 subtract /
 * divide / truncate, int64 result).  A row with a non-finite value takes no part in the minima / maxima and gets the key
 * P2W_CELL_NONFINITE (sorts last; the reference's own result on such input is the cast of a NaN, i.e. undefined).
 * Only columns 0 .. D-1 of a row are read: with ld > D the pad columns may hold anything, NaN included.  P is not modified, exactly
 * cell_out[0 .. n) is written, and neither cell_out nor ws needs initial content.  ws: >= 256 bytes.
 * Status, in this order: n == 0 -> P2W_OK (nothing is read or written); a NULL P / cell_out / ws -> P2W_ENULL; n < 0, D < 1, D > 16,
 * ld < D or a size that is not > 0 (0, negative, NaN) -> P2W_EINVAL; ws_bytes too small -> P2W_EWORKSPACE. */
#define P2W_CELL_NONFINITE INT64_MAX
int32_t p2w_cells_nd(const float* P, int32_t n, int32_t D, int32_t ld, float size, int64_t* cell_out, void* ws, size_t ws_bytes,
                     p2w_stream_t stream);
/* STABLE ascending sort of n (64-bit key, int32 value) pairs - hand-written LSD radix sort, 8-bit digits, as many passes as the
 * largest key has bytes (decided on the device).  vals_in NULL: values = 0..n-1, i.e. vals_out = the stable argsort the
 * voxeliser needs (points of a voxel keep their order, as the reference's nonzero() scan gives them).  Keys compare as
 * UNSIGNED 64-bit integers (a key with bit 63 set sorts behind every key without).  In and out buffers must differ; keys_in and
 * vals_in are not modified, exactly keys_out / vals_out[0 .. n) are written, and neither the outputs nor ws need initial content
 * (the same ws may serve call after call).  ws: 16-byte aligned, p2w_sort_pairs_u64_ws_bytes(n) bytes.
 * Status, in this order: n == 0 -> P2W_OK (nothing is read or written); a NULL keys_in / keys_out / vals_out / ws -> P2W_ENULL; ws
 * not 16-byte aligned -> P2W_EALIGN; n < 0, keys_in == keys_out or a non-NULL vals_in == vals_out -> P2W_EINVAL; ws_bytes too small
 * -> P2W_EWORKSPACE. */
size_t p2w_sort_pairs_u64_ws_bytes(int32_t n);
int32_t p2w_sort_pairs_u64(const uint64_t* keys_in, uint64_t* keys_out, const int32_t* vals_in, int32_t* vals_out, int32_t n, void* ws,
                           size_t ws_bytes, p2w_stream_t stream);
/* Runs of equal keys in a SORTED key array that hold at least min_count elements (the voxeliser's min_pts filter,
 * preprocessing.py:60-62): starts_out / counts_out[0 .. *n_out) in ascending order (buffers of n entries), *n_out on the device.
 * Keys are compared for equality only (any 64-bit pattern).  A run is kept when count >= min_count, so min_count <= 0 keeps every
 * run like min_count == 1.  keys_sorted is not modified, starts_out / counts_out from *n_out on are left as they were, and neither
 * the outputs nor ws need initial content.  ws: 16-byte aligned, p2w_key_runs_ws_bytes(n) bytes.
 * Status, in this order: a NULL n_out -> P2W_ENULL; n == 0 -> *n_out = 0 is enqueued, nothing else is read or written, P2W_OK; a
 * NULL keys_sorted / starts_out / counts_out / ws -> P2W_ENULL; ws not 16-byte aligned -> P2W_EALIGN; n < 0 -> P2W_EINVAL; ws_bytes
 * too small -> P2W_EWORKSPACE. */
size_t p2w_key_runs_ws_bytes(int32_t n);
int32_t p2w_key_runs(const uint64_t* keys_sorted, int32_t n, int32_t min_count, int32_t* starts_out, int32_t* counts_out, int32_t* n_out,
                     void* ws, size_t ws_bytes, p2w_stream_t stream);

/* Cell -> first-candidate table of a plot-level grid: table_out[c] = number of keys_sorted[0..n) below c, for c = 0 .. n_cells
 * (n_cells + 1 entries; n_cells = dims[0] * dims[1] * dims[2] of the p2w_grid the keys were made on, times the voxel count).  It is
 * the cell_start argument of p2w_knn_grid_indexed / p2w_ball_query_grid_indexed for levels that did not come from the table sampler -
 * the back-projection's search over all classified points of a plot (predicter.py:129-142: the reference's KD-tree): one load per
 * search run instead of a bisection of the keys.  n_cells < 2^31 - 1.  ws: 16-byte aligned, p2w_cell_starts_ws_bytes(n_cells) bytes.
 * n == 0 (keys_sorted may then be NULL) still writes the table: all zeros.
 * Status: a NULL table_out / ws (or keys_sorted with n > 0) -> P2W_ENULL; ws not 16-byte aligned -> P2W_EALIGN; n < 0, n_cells < 0 or
 * n_cells >= 2^31 - 1 -> P2W_EINVAL; ws_bytes too small -> P2W_EWORKSPACE. */
size_t p2w_cell_starts_ws_bytes(int64_t n_cells);
int32_t p2w_cell_starts(const uint64_t* keys_sorted, int32_t n, int64_t n_cells, int32_t* table_out, void* ws, size_t ws_bytes,
                        p2w_stream_t stream);

/* Exact fp64 re-ranking of a grid kNN result - the neighbour sets of the reference's KD-tree (predicter.py:136-137: pykdtree over
 * the float64 `classified_pc` of :205, float64 queries), which the fp32 searches above can miss where two candidates' distances
 * differ by less than an fp32 rounding.  cand_sorted[nc][3]: the candidates' float64 coordinates in the cell-sorted order of
 * `grid` (p2w_voxel_sample's order_out); cand_index[p] = the index the result reports for sorted position p, cand_pos = its
 * inverse; keys_sorted / cell_start (optional) / grid: as p2w_knn_grid_indexed; (ox, oy, oz): the offset that was subtracted
 * from the float64 coordinates to make the fp32 ones the grid was built on; q[m][3]: float64 queries.  nbr[m, k] / deg[m]: in
 * = any k candidates per query (the fp32 result; deg < k only where fewer than k candidates exist), out = the k nearest in
 * float64, ascending (squared distance = ((dx^2 + dy^2) + dz^2), candidate index).  k <= P2W_MAX_K.
 * A row with deg < k comes back with its deg entries in that order, the slots behind them and deg unchanged; a row with deg <= 0
 * is left alone.
 * Status: m == 0 or nc == 0 -> P2W_OK (nothing is read); a NULL pointer other than cell_start -> P2W_ENULL; m < 0, nc < 0, k < 1 or
 * k > P2W_MAX_K -> P2W_EINVAL. */
int32_t p2w_knn_refine_f64(const double* cand_sorted, const int32_t* cand_index, const int32_t* cand_pos,
                           const uint64_t* keys_sorted, const int32_t* cell_start, const p2w_grid* grid, double ox, double oy,
                           double oz, const double* q, int32_t m, int32_t nc, int32_t k, int32_t* nbr, int32_t* deg,
                           p2w_stream_t stream);

/* Euclidean clustering - EuclideanCluster.cluster (pointstowood/src/euclidean_clustering.py:13-47): points i and j are joined when
 * their float64 distance is within `tolerance` (cKDTree.query_ball_point(points[i], tolerance), p = 2: here
 * ((dx*dx + dy*dy) + dz*dz) <= tolerance*tolerance, every operation rounded on its own); a cluster is a connected component; the
 * components with min_size <= size <= max_size are numbered 0, 1, ... in ascending order of their smallest point index (the order
 * the reference's seed loop meets them), every other point gets -1.
 * In : the points in the cell-sorted order of a p2w_voxel_sample call over their fp32 coordinates made local to the cloud's minimum:
 *      xyz_sorted[n][3] = the caller's float64 coordinates in that order (finite), order[n] = its order_out (sorted position -> point
 *      index), keys_sorted[n] / grid = its sorted_keys_out / grid_out, cell_start = an optional p2w_cell_starts table of those keys
 *      (NULL: runs are found by bisection).  The grid's cell must be at least the tolerance plus the fp32 rounding of the local
 *      coordinates and of the key division (pointstowood_amd/cluster.py: safe_cell), so that every joined pair lies in adjacent cells.
 *      Any cell at or above it gives the same labels; a grid may be one cell thick on any axis, or one cell in all.
 * Out: labels_out[n] int64; counts_out[2] (device) = {number of kept clusters, number of points labelled -1}; pairs_out (optional,
 *      device uint64) = the number of point pairs whose distance the link stage measured = the number of unordered pairs of distinct
 *      points whose cells are equal or differ by at most 1 on every axis, each pair once (it depends on the grid, not on the tolerance).
 * `stages`: P2W_CLUSTER_ALL, or the stages one at a time in order (link, compress, number) on the same ws - the per-stage timing of
 * tools/cluster_bench.py: the link stage writes pairs_out, the number stage labels_out and counts_out, and the outputs equal those of
 * P2W_CLUSTER_ALL.  Neither ws nor an output needs any initial content; a repeated call gives the same bits.
 * n == 0 -> P2W_OK: counts_out = {0, 0}, pairs_out = 0, labels_out is not written (the pointers of the requested stages are still
 * checked).  n < 2^31 - 1, tolerance finite and >= 0 (P2W_EINVAL otherwise).
 * ws: 16-byte aligned, p2w_euclid_cluster_ws_bytes(n) bytes. */
#define P2W_CLUSTER_LINK 1     /* union-find over the grid: every pair of adjacent cells measured once, the larger root hooked under the smaller */
#define P2W_CLUSTER_COMPRESS 2 /* every point's root (= its component's smallest index) and the component sizes */
#define P2W_CLUSTER_NUMBER 4   /* size filter, scan of the kept roots, labels and counts */
#define P2W_CLUSTER_ALL 7
size_t p2w_euclid_cluster_ws_bytes(int64_t n);
int32_t p2w_euclid_cluster(const double* xyz_sorted, const int32_t* order, const uint64_t* keys_sorted, const int32_t* cell_start,
                           const p2w_grid* grid, int64_t n, double tolerance, int64_t min_size, int64_t max_size, int32_t stages,
                           int64_t* labels_out, int32_t* counts_out, uint64_t* pairs_out, void* ws, size_t ws_bytes,
                           p2w_stream_t stream);

/* Exact fp64 kNN of one cloud against itself for k <= P2W_MAX_K_WIDE - the rows of the reference's path-length graph
 * (pointstowood/utils/shortest_path.py:63-66: NearestNeighbors(n_neighbors=knn, leaf_size=15).fit(arr).kneighbors(arr), every point's
 * own index in its row).  In: as p2w_euclid_cluster (the caller's float64 coordinates in the cell-sorted order of a p2w_voxel_sample
 * call over fp32 coordinates local to the cloud's minimum, its order_out / sorted_keys_out / grid_out, an optional p2w_cell_starts
 * table); `slack` >= how far the fp32 grid can misplace a point across a cell boundary (pointstowood_amd/pathlength.py: knn_slack).
 * Any cell size gives the same result; it only sets how many cells a search visits.  Out: nbr_out[n, k] int32, row i = the k nearest
 * points of point i ascending by (sqrt(((dx*dx + dy*dy) + dz*dz)) in float64, index).  1 <= k <= min(n, P2W_MAX_K_WIDE). */
int32_t p2w_knn_wide_f64(const double* xyz_sorted, const int32_t* order, const uint64_t* keys_sorted, const int32_t* cell_start,
                         const p2w_grid* grid, int64_t n, int32_t k, double slack, int32_t* nbr_out, p2w_stream_t stream);

/* Graph growth of the path-length graph - array_to_graph (pointstowood/utils/shortest_path.py:80-187).  xyz[n][3] float64, nbr[n, k] =
 * p2w_knn_wide_f64's rows (original indices), base = the root, kpairs / nbrs_threshold / nbrs_threshold_step / graph_threshold = the
 * reference's arguments.  Frontier steps (:86-112) and gap steps (:115-176, the threshold raised in fp64 by one step per empty
 * iteration) as the reference takes them; where no remaining row holds a processed point the growth stops (the reference raises its
 * threshold for ever there) and the rest stays -1.  Out: step_out[n] = the step at which each point was processed (base 0, -1 never);
 * edges_out[edge_cap][2] = the edges (g, e) in no particular order, duplicates and self-loops included; info_out (HOST, 6 int64) =
 * {edges, stop step, gap steps, threshold raises, launches, 1 if points were left unreached}; threshold_out (HOST) = the final
 * nbrs_threshold.  Stop step = the last step that had a non-empty frontier or raised the threshold.  The reference's loop ends right
 * after the step S that processed the last point; here the frontier step S + 1 still runs (it finds every row entry processed and
 * adds nothing) and the empty frontier of S + 2 ends the growth, so with every point processed the stop step is max(step_out) + 1 =
 * the reference's final current_step + 1 - and equal to it, 1, for n = 1, where the reference's only step is that empty-handed one.
 * With points left unreached it is the step BEFORE the one that found so (the first empty frontier with no remaining row holding a
 * processed point: max(step_out) + 1 again; or the step whose fp64 threshold addition changed nothing: the last raise).
 * edge_cap >= n * 3 * (min(kpairs + 1, k)) always suffices (P2W_EWORKSPACE when the edges overflow).
 * Blocks the host (the state is read back between launch batches and at every empty frontier).  nbrs_threshold_step finite and > 0.
 * ws: 16-byte aligned, p2w_pathlen_grow_ws_bytes(n) bytes. */
size_t p2w_pathlen_grow_ws_bytes(int64_t n);
int32_t p2w_pathlen_grow(const double* xyz, const int32_t* nbr, int64_t n, int32_t k, int32_t base, int32_t kpairs, double nbrs_threshold,
                         double nbrs_threshold_step, double graph_threshold, int32_t* step_out, int32_t* edges_out, int64_t edge_cap,
                         int64_t* info_out, double* threshold_out, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* Shortest path lengths from `base` over an undirected edge list - extract_path_info (pointstowood/utils/shortest_path.py:195-238,
 * networkx single_source_dijkstra).  edges[n_edges][2] int32 (duplicates and self-loops allowed), weights = the float64 distances of
 * the endpoints' xyz.  Out: dist_out[n] = the minimum over paths of the left-fold fp64 sum (bit-equal to Dijkstra's), NaN where
 * unreached; parent_out[n] (optional) = a neighbour u with dist[u] + w == dist[v], fewest hops first then smallest index (acyclic,
 * every chain ends at base; -1 for base and unreached nodes); info_out (HOST, 3 int64) = {Bellman-Ford rounds, hop levels, launches}.
 * Blocks the host.  ws: 16-byte aligned, p2w_pathlen_sssp_ws_bytes(n, n_edges) bytes. */
size_t p2w_pathlen_sssp_ws_bytes(int64_t n, int64_t n_edges);
int32_t p2w_pathlen_sssp(const double* xyz, const int32_t* edges, int64_t n_edges, int64_t n, int32_t base, double* dist_out,
                         int32_t* parent_out, int64_t* info_out, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* w_out[e] = sqrt(((dx*dx + dy*dy) + dz*dz)) in float64 of the endpoints of edges[e] (int64 pairs): the weights of the graph object
 * pointstowood_amd.pathlength.array_to_graph returns (shortest_path.py:241-266 add_nodes). */
int32_t p2w_pathlen_weights(const double* xyz, const int64_t* edges, int64_t n_edges, double* w_out, p2w_stream_t stream);

/* Segmented, weighted confusion matrix of a classification against truth labels: the counting behind the reference's scores -
 * pointstowood/comparetofsct.py:85-106 and the held-out loop of pointstowood/src/trainer.py:239-242 (sklearn's precision_score,
 * recall_score, f1_score and balanced_accuracy_score, with and without sample_weight, are all functions of this matrix).
 * In : truth[n], pred[n] = class ids stored as floats (PLY columns, Data.y), weight[n] float64 (optional: NULL), seg_ptr[segments + 1]
 *      int64 (DEVICE; ascending, seg_ptr[0] = 0, seg_ptr[segments] = n; NULL = one segment, segments must be 1).  truth, pred and
 *      weight 16-byte aligned.  A point is valid when both ids are integral and in [0, classes) and its weight, where weights are
 *      given, is finite and >= 0.
 * Out: counts[segments][classes][classes] int64 (row = truth, column = pred) = the valid points of every cell; wsum (same shape,
 *      float64; NULL exactly when weight is NULL) = the sum of their weights; invalid[segments] = the points that are not valid
 *      (they enter no cell).  counts are exact; wsum has the same bits on every run (no floating-point atomics: chunks of
 *      P2W_EVAL_CHUNK points cut at the segment boundaries are summed in a fixed order, and so are the chunks of a segment).
 * No host synchronisation and no host read.  0 <= n <= 2^40, segments >= 1, 2 <= classes <= P2W_EVAL_MAX_CLASSES (P2W_EINVAL).
 * ws: 16-byte aligned, p2w_confusion_ws_bytes(n, segments, classes) bytes (sized for n / P2W_EVAL_CHUNK + segments chunks). */
#define P2W_EVAL_CHUNK 4096
#define P2W_EVAL_MAX_CLASSES 8
size_t p2w_confusion_ws_bytes(int64_t n, int32_t segments, int32_t classes);
int32_t p2w_confusion(const float* truth, const float* pred, const double* weight, const int64_t* seg_ptr, int64_t n, int32_t segments,
                      int32_t classes, int64_t* counts, double* wsum, int64_t* invalid, void* ws, size_t ws_bytes,
                      p2w_stream_t stream);

/* Poly-1 focal loss of the reference's training step, forward and backward in one pass: Poly1FocalLoss.forward
 * (pointstowood/src/loss.py:28-73, the criterion of pointstowood/src/trainer.py:174-202) evaluated per element in fp32, statement by
 * statement - logits clamped to [-10, 10], optional label smoothing, sigmoid clamped to [eps, 1 - eps], BCE-with-logits times weight
 * clamped at 100, pt clamped, (1 - pt)^gamma clamped at 2, optional alpha_t, the poly term epsilon * (1 - pt)^(gamma + 1) clamped at
 * 100, the sum clamped to [0, 100], NaN replaced by 0.
 * In : logits[n], labels[n] float32; weight: NULL (weight_n = 0), one element (weight_n = 1) or n elements (weight_n = n), float32,
 *      DEVICE memory; the reference's scalars as doubles, rounded to fp32 where the reference's fp32 tensors meet them.  alpha and
 *      label_smoothing are "not set" (the reference's None) when they are NaN; every other scalar must be finite, gamma >= 0 and
 *      0 < eps < 0.5 (P2W_EINVAL).  logits, labels, an n-element weight, loss and dloss 16-byte aligned.
 * Out, each optional (NULL = not wanted, neither computed nor written): loss[n] float32 = the per-element loss; dloss[n] float32 =
 *      the derivative of element i's loss with respect to logit i under PyTorch's autograd conventions (a clamp passes the gradient
 *      inside its closed range and gives 0 outside; the BCE term's derivative is (sigmoid(z) - y) * weight of the clamped logit z; a
 *      zero exponent contributes nothing) - 0 for a logit beyond +-10 or NaN, never NaN for finite labels and weights; sum[1] float64 =
 *      the sum of the per-element losses, the same bits on every run (no atomics, no memset: one float64 partial per chunk of
 *      P2W_LOSS_CHUNK elements, lanes, waves and chunks added in an order fixed by n alone).  n = 0 writes sum = 0 and reads nothing.
 * Two launches (one without sum), no host synchronisation and no host read.  0 <= n <= 2^40 (P2W_EINVAL).
 * ws: needed only with sum; 16-byte aligned, p2w_poly1_focal_ws_bytes(n) bytes (0 for an n out of range). */
#define P2W_LOSS_CHUNK 4096
size_t p2w_poly1_focal_ws_bytes(int64_t n);
int32_t p2w_poly1_focal(const float* logits, const float* labels, const float* weight, int64_t weight_n, int64_t n, double epsilon,
                        double gamma, double alpha, double label_smoothing, double eps, float* loss, float* dloss, double* sum,
                        void* ws, size_t ws_bytes, p2w_stream_t stream);

/* The training feed: the voxels ids[0..B) of a device-resident training set gathered, augmented, centred and collated into one batch -
 * TrainingDataset.__getitem__ (pointstowood/src/trainer.py:46-60), augmentations (pointstowood/src/augmentation.py:41-55: silence or
 * perturb the reflectance, rotate_3d) and PyG's collation, with the decisions and the rotation matrices made by the host (plan).
 * In : xyzr[n_set] float4 rows (x, y, z, reflectance) and y[n_set] float32 = the whole set, set_ptr[V + 1] int64 (ascending, set_ptr[0]
 *      = 0, set_ptr[V] = n_set); ids[B] int32 = the batch's voxels, DISTINCT; out_ptr[B + 1] int64 (out_ptr[0] = 0, out_ptr[b + 1] -
 *      out_ptr[b] = the length of voxel ids[b], out_ptr[B] = n); plan[V] records indexed by VOXEL ID; seed, epoch; noise[n] (optional:
 *      NULL) = the standard-deviation-0.1 noise of the perturbed rows, by OUTPUT row, in place of the generator.  All DEVICE memory.
 * Out: pos[n][3], reflectance[n], y[n] float32, batch[n] int64 (= b), sf[B] float32, nonfinite[B] int32; words_out[n][4] uint32
 *      (optional: NULL) = the generator's four words of every row (whatever its voxel's refl_mode).
 * Arithmetic of voxel v = ids[b], rows i = 0 .. len - 1, every rounding point:
 *   mean  = S / len in float64, S = the float64 sum of the float32 coordinates (conversions exact): one partial per P2W_FEED_CHUNK
 *           consecutive rows of the voxel (lanes by a fixed xor tree, waves in order), the partials added in ascending order;
 *   d     = fl32(x - mean): the subtraction in float64, rounded ONCE to float32 (centre first, rotate after: mean(x R) = mean(x) R, and
 *           plot coordinates of hundreds of metres then never meet a float32 product);
 *   p     = d when !rotate, else p_j = fmaf(d_z, R[6 + j], fmaf(d_y, R[3 + j], fl32(d_x * R[j]))): three roundings per coordinate;
 *           R (row-major, p = d R) = roll pitch yaw of rotate_3d, formed by the host in float64 from the float32 cos / sin and rounded;
 *   refl  = r (refl_mode 0), +0.0 (1), fl32(r + e) (2) with e = noise[row] or fl32(0.1f * z);
 *   z     : Philox4x32-10, counter = (i, v, epoch, P2W_FEED_STREAM), key = (seed & 0xffffffff, seed >> 32), words w0 .. w3;
 *           u1 = fl32((w0 >> 8) + 1) * 2^-24 in (0, 1], u2 = fl32(w1 >> 8) * 2^-24 in [0, 1), both exact;
 *           z = fl32(sqrtf(fl32(-2 * logf(u1))) * cosf(fl32(6.2831855f * u2))) (Box-Muller's cosine branch; w2, w3 unused) - so a
 *           voxel's noise depends on (seed, epoch, v, i) alone, never on the batch or the slot;
 *   sf[b] = max_i sqrtf(fl32(fl32(fl32(p_x p_x) + fl32(p_y p_y)) + fl32(p_z p_z))) of the WRITTEN p, no contraction: an integer
 *           atomic maximum of the sign-cleared bit patterns (order-independent: the same bits on every run; a NaN's pattern is above
 *           infinity's, so a NaN row gives a NaN sf, as torch.max does); 0 for an empty voxel;
 *   nonfinite[b] = rows with a non-finite x, y, z or INPUT reflectance.  They are passed through (a non-finite coordinate makes the
 *           voxel's mean, and with it all its positions and its sf, non-finite, as in the reference).
 * Two launches, no memset (the first launch zeroes sf and nonfinite), no host synchronisation and no host read.  0 <= n, n_set <= 2^40,
 * B >= 0, V >= 1 (P2W_EINVAL); B = 0 or n = 0: P2W_OK, nothing written, nothing launched.  xyzr, plan and ws 16-byte aligned
 * (P2W_EALIGN); every pointer but noise and words_out required (P2W_ENULL); ws: p2w_train_feed_ws_size(n, B) bytes (n / P2W_FEED_CHUNK +
 * B chunks; 0 = bad sizes; too small: P2W_EWORKSPACE).  A refused call launches nothing.  Offsets are clamped to their arrays and an id
 * outside [0, V) is an empty voxel, so no access leaves the arrays whatever the index arrays hold; len < 2^32. */
#define P2W_FEED_CHUNK 256
#define P2W_FEED_STREAM 0x50325746u /* "P2WF": the counter word that keeps this stream apart from later users of the generator */
typedef struct p2w_feed_plan {
    int32_t refl_mode; /* 0 keep, 1 zero, 2 perturb */
    int32_t rotate;    /* 0: R is the identity and is not applied */
    float R[9];
    int32_t reserved;  /* 48-byte records */
} p2w_feed_plan;
size_t p2w_train_feed_ws_size(int64_t n, int32_t B);
int32_t p2w_train_feed(const float* xyzr, const float* y, const int64_t* set_ptr, int64_t n_set, int32_t V, const int32_t* ids,
                       const int64_t* out_ptr, int32_t B, int64_t n, const p2w_feed_plan* plan, uint64_t seed, uint32_t epoch,
                       const float* noise, float* pos_out, float* refl_out, float* y_out, int64_t* batch_out, float* sf_out,
                       int32_t* nonfinite_out, uint32_t* words_out, void* ws, size_t ws_size, p2w_stream_t stream);

/* The training sample: a uniformly random k-subset of {0 .. n-1}, ascending - the law of SAModule's draw (pointstowood/src/model.py:97-101:
 * the first half of a randperm, sorted) as a function of (seed, c1, c2, n, k) alone, from the feed's generator and not from the reference's
 * random stream.
 *   key_i  = word w0 of Philox4x32-10 with counter (i, c1, c2, P2W_SAMPLE_STREAM) and key (seed & 0xffffffff, seed >> 32);
 *   subset = the k rows that are smallest in the lexicographic order of (key_i, i);
 *   idx_out[0..k) = those rows in ascending row order.
 * As far as the words are independent and uniform, distinct keys make every k-subset equally likely.  Equal keys are ordered by row: with
 * T the k-th smallest key, of the rows whose key is T the lowest ones are taken.  A given row shares the boundary value with another one
 * with probability of order n 2^-32 (0.4 % at n = 2^24, 3e-5 at 131 072), and only then is the lower row preferred: the inclusion
 * probabilities differ from k / n by that order at most.
 * In : keys[n] uint32 (optional: NULL) = the key of every row, used IN PLACE of the generator.  Out: idx_out[k] int64; keys_out[n] uint32
 *      (optional: NULL) = the key of every row.  All DEVICE memory.
 * 0 <= k <= n <= P2W_SAMPLE_N_MAX = 2^24 (P2W_EINVAL; p2w_random_subset_ws_size returns 0 for an n outside).  n = 0 or k = 0: P2W_OK,
 * nothing launched, nothing written.  k = n gives 0 .. n-1.  idx_out and ws required (P2W_ENULL); ws 16-byte, idx_out 8-byte, keys and
 * keys_out 4-byte aligned (P2W_EALIGN); ws: p2w_random_subset_ws_size(n) bytes (4 bytes per row, four 256-bin histograms, two counters
 * per tile of P2W_SAMPLE_TILE rows and their scan's tile sums; too small: P2W_EWORKSPACE).  A refused call launches nothing.
 * An exact selection, not a sort: a radix select of T over four 8-bit digits, the most significant first, then a stable compaction.
 * 8 launches for n <= 2^21, 10 above (zero the histograms, keys, three select passes, count, a scan of one or three launches, write).  No
 * memset, no host synchronisation, no host read; no workgroup waits for another - what one launch needs of all workgroups of an earlier
 * one is a launch boundary.  Integer arithmetic only; the atomics are integer additions to histogram bins (order-independent), so the
 * bits are the same on every run and do not depend on what the workspace held. */
#define P2W_SAMPLE_STREAM 0x50325753u /* "P2WS" */
#define P2W_SAMPLE_TILE 1024
#define P2W_SAMPLE_N_MAX ((int64_t)1 << 24)
size_t p2w_random_subset_ws_size(int64_t n);
int32_t p2w_random_subset(int64_t n, int64_t k, uint64_t seed, uint32_t c1, uint32_t c2, const uint32_t* keys, int64_t* idx_out,
                          uint32_t* keys_out, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* The voxeliser's cap: every one of S segments of a row space of n rows is cut down to k rows in ONE call - the reference's per-voxel
 * torch.multinomial(weight[voxel], max_pts) / torch.randint(len, (max_pts,)) (pointstowood/src/preprocessing.py:116-120) as a function of
 * (seed, c1, c2) and of each segment's own (row_id, weight) pairs, from the feed's generator and not from the reference's random stream.
 * In : seg_start[S], seg_count[S] int64 = disjoint segments in ascending order; weight[n] float32 (optional: NULL); row_id[n] int64
 *      (optional: NULL = the row's own position) = what the generator knows a row by; keys[n] uint32 (optional: NULL) = the key of every
 *      row, used IN PLACE of the generator and the weights.  Out: idx_out[S][k] int64 = positions in the row space; keys_out[n] uint32
 *      (optional: NULL) = the key of every row of every segment (other rows are not written).  All DEVICE memory.
 * Weighted mode (weight or keys given): the law of multinomial without replacement - successive sampling, each draw proportional to the
 * weights of the rows still there - as an exponential race (Efraimidis and Spirakis 2006: the k smallest of independent Exp(w_i)):
 *   w0_i   = word 0 of Philox4x32-10 with counter (row_id_i & 0xffffffff, c1, c2, P2W_CAP_STREAM), key (seed & 0xffffffff, seed >> 32);
 *   u_i    = (w0_i + 0.5) 2^-32, in (0, 1);
 *   key_i  = fl32(-log(u_i) / w_i): logarithm (the device's double log) and division in float64, rounded ONCE to float32; positive or
 *            +inf, so the bit pattern orders as an unsigned integer and is the selection's 32-bit key;
 *            0xFFFFFFFF where w_i is not a finite positive number: behind every valid key, +inf included, taken only when valid rows run
 *            out;
 *   segment s keeps the k rows of its range that are smallest in (key_i, position i); idx_out[s][0..k) = those positions, ascending.
 *   count_s <= k: all its rows, then -1 up to k.
 * Equal keys are ordered by position, as in p2w_random_subset: with T the k-th smallest key of a segment, of the rows whose key is T the
 * lowest positions are taken.  A float32 key has 24 significant bits, so T stands for an interval of relative width 2^-23 at most; the
 * race's keys have density sum_i w_i exp(-w_i t) <= k / T there (about k of the w_i T add up to the k rows below T), so a second row
 * shares the boundary key with probability of order k 2^-23 per segment (2e-3 at k = 16 384), and only then is the lower position
 * preferred: inclusion probabilities differ from the law's by that order at most.
 * Replacement mode (weight == NULL and keys == NULL): k uniform draws WITH replacement, in draw order j = 0 .. k-1:
 *   idx_out[s][j] = start_s + floor(w0 count_s / 2^32), w0 = word 0 at counter (j, row_id[start_s] & 0xffffffff, c2, P2W_CAP_STREAM ^ 1)
 *   (c1 is not used).  Integer arithmetic only; a position's probability differs from 1 / count by at most count 2^-32, relative.
 *   count_s = 0: -1 throughout.  One launch; keys_out and ws are not looked at.
 * Starts are clamped to [0, n] and counts to [0, n - start]: nothing outside the row space is read, whatever the two arrays hold.
 * Segments that overlap get unspecified rows of their own ranges (disjoint segments have at most n / P2W_SAMPLE_TILE + S tiles, which is
 * the launch grid).
 * 0 <= n <= P2W_CAP_N_MAX, 0 <= S <= P2W_CAP_S_MAX, 1 <= k <= P2W_CAP_N_MAX, S k <= P2W_CAP_OUT_MAX (P2W_EINVAL; p2w_cap_subset_ws_size
 * returns 0 for an n or S outside).  S = 0: P2W_OK, nothing launched, nothing written.  seg_start, seg_count, idx_out and - in weighted
 * mode - ws required (P2W_ENULL); ws 16-byte, the int64 arrays 8-byte, the 32-bit arrays 4-byte aligned (P2W_EALIGN); ws:
 * p2w_cap_subset_ws_size(n, S) bytes (4 per row, four 256-bin histograms and a control record per segment, S + 1 tile offsets, two
 * counters per tile of P2W_SAMPLE_TILE rows, n / P2W_SAMPLE_TILE + S + 1 tiles, and the two scans' tile sums; too small:
 * P2W_EWORKSPACE).  A refused call launches nothing.
 * The selection is p2w_random_subset's (radix select of the k-th key over four 8-bit digits, stable compaction), with one histogram set
 * per segment; a segment's tiles are the P2W_SAMPLE_TILE-row pieces of its own range, numbered through all segments by a scan on the
 * device, so one large segment is spread over as many workgroups as it has tiles.  9 launches (11 above 4095 segments, 2 more where
 * 2 (n / P2W_SAMPLE_TILE + S + 1) > 4096), whatever S.  No memset, no host synchronisation, no host read, no wait between workgroups;
 * the atomics are integer additions to histogram bins, no floating-point atomics: the same bits on every run, whatever ws held. */
#define P2W_CAP_STREAM 0x50325743u /* "P2WC"; replacement mode uses P2W_CAP_STREAM ^ 1 */
#define P2W_CAP_N_MAX ((int64_t)1 << 30)
#define P2W_CAP_S_MAX ((int64_t)1 << 20)
#define P2W_CAP_OUT_MAX ((int64_t)1 << 38)
size_t p2w_cap_subset_ws_size(int64_t n, int64_t S);
int32_t p2w_cap_subset(int64_t n, const int64_t* seg_start, const int64_t* seg_count, int64_t S, int64_t k, const float* weight,
                       const int64_t* row_id, uint64_t seed, uint32_t c1, uint32_t c2, const uint32_t* keys, int64_t* idx_out,
                       uint32_t* keys_out, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* The optimiser step behind backward(): unscale, clip to a global norm, AdamW and the loss-scale law, decided and applied on the device -
 * what the reference's loop (pointstowood/src/trainer.py:196-204) composes from scaler.unscale_, clip_grad_norm_(max_norm),
 * scaler.step(AdamW(amsgrad=False, maximize=False)) and scaler.update(), as ONE documented fp32 operation order.
 * In : tensors[T] = a HOST array of records of DEVICE pointers (p, g, m, v: n fp32 elements each, contiguous; an entry with n = 0 is
 *      skipped and its pointers are not looked at); hyper = a HOST structure, read during the call; state = the DEVICE record the caller
 *      owns and keeps across steps (before the first step: scale = the loss scale that multiplied the loss, or 1; all else 0).
 * Out: p, m, v updated in place (or untouched), the record rewritten.  g is only read.
 * Work: a chunk is P2W_OPTIM_CHUNK consecutive elements of ONE tensor (256 threads, 16 elements each; a tensor's last chunk may be
 *      short), numbered through the non-empty tensors in table order.  The table travels BY VALUE in the kernel arguments, one launch
 *      per group of at most P2W_OPTIM_GROUP non-empty tensors: nothing is uploaded, so the table may be rebuilt at every step.  With T'
 *      non-empty tensors a step is 2 ceil(T' / P2W_OPTIM_GROUP) + 1 launches:
 *   norm      inv_scale = fl32(1 / (double)state.scale) (scaling off: 1).  Per chunk: sum of (double)u (double)u, u = fl32(g * inv_scale),
 *             in fp64 (each square exact): thread t takes elements 1024 r + 4 t + j (r, j = 0 .. 3) in ascending order, the 64 lanes of
 *             a wave are added by a xor-shuffle tree (offsets 32, 16, .. 1), the 4 waves in wave order -> the chunk's word of ws.
 *   finalise  one workgroup: thread t adds the words t, t + 256, .. ascending, same tree, same wave order -> sumsq.
 *             found_inf = !isfinite(sumsq): exact, since an fp32 square is below 1.2e77 and 2^40 of them cannot overflow fp64, while an
 *             inf or a NaN anywhere in g reaches the sum.  norm = fl32(sqrt(sumsq)); coef = fminf(1, fl32(max_norm) / (norm + 1e-6f)).
 *             found_inf : scale *= fl32(backoff_factor), growth_tracker = 0, skipped += 1; t and the seven scalars keep their values.
 *             otherwise : t += 1, growth_tracker += 1, and where it reaches growth_interval: scale *= fl32(growth_factor),
 *                         growth_tracker = 0.  Scaling off: scale = 1, the counters move the same way.
 *             The seven scalars, each evaluated in fp64 (the device's double pow) and rounded to fp32 ONCE: decay = 1 - lr weight_decay,
 *             omb1 = 1 - beta1, beta2, omb2 = 1 - beta2, step_size = lr / (1 - beta1^t), rsb2 = 1 / sqrt(1 - beta2^t), eps.
 *   update    every workgroup reads the record; on found_inf it returns without a store.  Otherwise per element, in fp32:
 *                 u  = g * inv_scale          gc = u * coef
 *                 p1 = p * decay
 *                 m' = m + (gc - m) * omb1
 *                 v' = v * beta2 + (omb2 * gc) * gc
 *                 d  = sqrt(v') * rsb2 + eps
 *                 p' = p1 - step_size * (m' / d)
 *             every operation one correctly rounded IEEE operation (no contraction, no fma anywhere in the step; correctly rounded
 *             square root and division; subnormals kept), so a CPU replay in fp32 reproduces the bits.
 * 16 bytes per access where a tensor's addresses allow (norm: g; update: p, g, m and v together), else 4: the same element-to-thread map
 * and the same bits.  No memset, no atomics, no host synchronisation, no host read, no wait between workgroups: equal inputs give equal
 * bits whatever ws held.
 * 0 <= T <= P2W_OPTIM_MAX_TENSORS, every n >= 0, at most 2^40 elements in all; lr, eps, weight_decay, max_norm finite and >= 0,
 * 0 <= beta1, beta2 < 1, growth_factor > 1 and finite, 0 < backoff_factor < 1, growth_interval >= 1, scaling 0 or 1 (P2W_EINVAL).
 * tensors (T > 0), hyper, and - where there is an element - state, ws and the four pointers of every non-empty entry are required
 * (P2W_ENULL); state and ws 16-byte, tensor pointers 4-byte aligned (P2W_EALIGN); ws: p2w_clip_adamw_ws_size(numel, T) bytes, 8 per chunk
 * (0 = bad sizes; too small: P2W_EWORKSPACE).  T = 0 or every n = 0: P2W_OK, nothing launched, nothing written.  A refused call
 * launches nothing. */
#define P2W_OPTIM_CHUNK 4096
#define P2W_OPTIM_GROUP 32
#define P2W_OPTIM_MAX_TENSORS 4096
typedef struct p2w_optim_tensor {
    float* p;
    const float* g;
    float* m;
    float* v;
    int64_t n;
} p2w_optim_tensor;
typedef struct p2w_optim_hyper {
    double lr, beta1, beta2, eps, weight_decay, max_norm, growth_factor, backoff_factor;
    int32_t growth_interval;
    int32_t scaling; /* 0: no loss scale (the scale is 1 and stays 1) */
} p2w_optim_hyper;
typedef struct p2w_optim_state {
    double sumsq;           /* of the unscaled gradients */
    float norm, coef;
    float inv_scale;        /* the one this step used */
    float scale;            /* the loss scale of the NEXT step */
    int32_t found_inf;      /* 1: this step was skipped */
    int32_t growth_tracker;
    int64_t t;              /* steps applied */
    int64_t skipped;        /* steps skipped */
    float decay, omb1, beta2, omb2, step_size, rsb2, eps;
    int32_t reserved;       /* 80-byte record */
} p2w_optim_state;
size_t p2w_clip_adamw_ws_size(const int64_t* numel, int32_t T);
int32_t p2w_clip_adamw(const p2w_optim_tensor* tensors, int32_t T, const p2w_optim_hyper* hyper, p2w_optim_state* state, void* ws,
                       size_t ws_bytes, p2w_stream_t stream);

/* PointCloudClassifier.compute_labels (predicter.py:112-127) over a neighbour table nbr[n,k] (indices into pred /
 * prob, deg[i] valid entries): pwood_out = median of the neighbours' probabilities (np.median: mean of the two middle
 * values for an even count); label_out: any_wood != 1 -> 1 if any neighbour's prediction > any_wood else 0;
 * any_wood == 1 -> argmax_j sum_{pred == j} prob over j in {0, 1} (first maximum, sums in fp64 like numba's).
 * The valid entries of row i are its first min(deg[i], k) slots; the slots behind them are not read.  A row without a valid entry
 * (deg[i] <= 0) gets label_out = 0, pwood_out = 0.
 * Status: n == 0 -> P2W_OK (nothing is read); a NULL nbr / deg / pred / prob / label_out / pwood_out -> P2W_ENULL; n < 0, k < 1 or
 * k > P2W_MAX_K -> P2W_EINVAL. */
int32_t p2w_vote(const int32_t* nbr, const int32_t* deg, int32_t k, const float* pred, const float* prob, int32_t n,
                 float any_wood, float* label_out, float* pwood_out, p2w_stream_t stream);

/* Optional accelerator for the searches (results are identical with or without it): bounding boxes (lo xyz, hi xyz)
 * of the candidate tiles of xyzr_x (1024 consecutive records of one voxel).  bbox holds p2w_tile_bbox_count(B,
 * n_bound) x 6 floats.  With it, p2w_knn skips tiles whose box is farther than a query's current k-th distance and
 * p2w_ball_query tiles farther than r; it pays when the candidates are stored in a spatially coherent order. */
int32_t p2w_tile_bbox(const float* xyzr, const int32_t* ptr, int32_t B, int32_t n_bound, float* bbox, p2w_stream_t stream);
int32_t p2w_tile_bbox_count(int32_t B, int32_t n_bound);

/* ---- features ---------------------------------------------------------- */

/* stem_mlp: out[n,C] = relu(W[C,3] * xyz + b) - model.py:208,228.  C a multiple of 4; xyzr and out 16-byte aligned (P2W_EALIGN:
 * the rows are written 16 bytes at a time). */
int32_t p2w_stem(const float* xyzr, int32_t n, const float* w, const float* b, int32_t C, float* out,
                 p2w_stream_t stream);

/* Epilogue description for p2w_gemm: v = acc + bias; relu0; v = v*sc0+sh0; relu1; v = v*sc1+sh1; relu2;
 * v += residual; relu_final.  NULL scale pointers skip their stage. */
typedef struct p2w_epilogue {
    const float* bias;   /* [N] or NULL */
    const float* sc0;    /* [N] */
    const float* sh0;    /* [N] */
    const float* sc1;    /* [N] */
    const float* sh1;    /* [N] */
    const float* residual; /* [M, ldr] or NULL */
    int32_t ldr;
    int32_t relu0, relu1, relu2, relu_final;
    uint32_t* range;     /* NULL, or the launch's range report (the caller zeroes it; p2w_gemm ignores it): P2W_RANGE_SLOTS word
                            pairs, 64 words apart (P2W_RANGE_WORDS words in all; a workgroup writes the pair of its number modulo
                            the slot count - one hot address would queue every store in one L2 channel).  Word 0 of a pair is set
                            to 1 if an epilogue value lies beyond +-P2W_RANGE_HI (or is NaN), word 1 if one lies beyond
                            +-P2W_RANGE_LO; the report is the OR over the slots.  It is the range watch of the split-fp16
                            arithmetic: past 65504 an H value has lost its low part, and a tensor WITHOUT a value of ordinary
                            size has lost it to fp16's subnormal floor (2^-24 absolute) */
    const void* interp;  /* NULL, or [M] records {int32 n0, int32 n1, float a0, float a1} (p2w_interp_weights; 16-byte aligned):
                            p2w_gemm_h2 / _sk add to output row r not residual[r] but a0 * residual[n0] + a1 * residual[n1] - the
                            rows of a COARSER level's fp32 matrix `residual` [interp_rows, ldr] interpolated on the fly (an FP
                            module's layer 0 by linearity: relu(W [interp(y) | skip] + b) = relu(W_s skip + b + interp(W_i y)),
                            model.py:149-153).  128 x 128 tile only (P2W_GEMM_TILE_256 is ignored); with P2W_GEMM_RESIDUAL_H: P2W_EUNSUPPORTED;
                            p2w_gemm and p2w_gemm_h2_rowdot refuse it (P2W_EUNSUPPORTED) */
    int32_t interp_rows; /* rows of `residual` when `interp` is given: every n0, n1 lies below it */
} p2w_epilogue;

#define P2W_RANGE_HI 6.0e4f
#define P2W_RANGE_LO 0.03125f
#define P2W_RANGE_SLOTS 16
#define P2W_RANGE_WORDS (64 * P2W_RANGE_SLOTS)

/* Packed weight: Wp[N_pad][K_pad] fp32, row n = output channel, k contiguous, zero padded
 * (K_pad = round_up(K, 32), N_pad = round_up(N, 256)); see p2w_packed_dims. */
void p2w_packed_dims(int32_t N, int32_t K, int32_t* N_pad, int32_t* K_pad);

/* out[M,N] = epilogue(A[M,K] * W^T): Linear / 1x1 Conv1d + folded BatchNorm / depthwise affines +
 * ReLU + residual - model.py:75-85 (InvertedResidualBlock), :198-202 (MLP), :241-242 (head).
 * fp32 MFMA (v_mfma_f32_32x32x2_f32), exact fp32 products, fp32 accumulate. */
int32_t p2w_gemm(const float* A, int32_t lda, const float* Wp, int32_t M, int32_t N, int32_t K,
                 const p2w_epilogue* epi, float* out, int32_t ldo, p2w_stream_t stream);

/* Fused PointNetConv (pointnet.py:86-132) for one SA level:
 *   per target i and neighbour slot s (j = nbr[i,s]):
 *     rel  = xyz_s[j] - xyz_s[idx[i]]            on sf-scaled coordinates (model.py:122)
 *     dmax = max_s ||rel||                        (scatter_max, pointnet.py:122)
 *     h1   = relu(P[j] + (rel/(dmax+1e-8)) * W1r + refl_j * W1f)       layer 1, hoisted:
 *            P = x_src * W1x^T + b1 is computed once per source point by p2w_gemm
 *     h2   = relu(h1 * W2^T + b2) * bn_s + bn_t                       layer 2 + BN (model.py:198-202)
 *   out[i] = max over valid slots of h2 (rows without neighbours = 0). */
int32_t p2w_sa_conv(const float* P, int32_t ldp, const float* xyzr_src, const int32_t* idx, const int32_t* batch_dst,
                    const float* sf, const int32_t* nbr, const int32_t* deg, int32_t kw, int32_t M,
                    const float* w1r4 /* [4][C1_pad] */, const float* W2p, int32_t C1, int32_t C2,
                    const float* b2, const float* bn_s, const float* bn_t, float* out, int32_t ldo,
                    p2w_stream_t stream);

/* ---- H family: the same GEMM / PointNetConv on 16-bit MFMA operands ------------------------------------------
 * Precision of an H tensor and of the arithmetic on it (`prec` argument of every entry point below):
 *   P2W_PREC_F16X3  fp16 hi/lo planes, a*w = a_lo*w_hi + a_hi*w_lo + a_hi*w_hi on v_mfma_f32_32x32x16_f16 with fp32
 *                   accumulation (~22-bit operands): the parity mode, meets the 1e-4 probability bar of the fp32 path;
 *   P2W_PREC_F16    one fp16 plane (round to nearest, saturating at +-65504), one MFMA per product;
 *   P2W_PREC_BF16   one bf16 plane, v_mfma_f32_32x32x16_bf16.
 *   The single-plane modes are what the reference's own GPU path computes in (torch.cuda.amp.autocast,
 *   pointstowood/src/predicter.py:197); they do NOT meet the 1e-4 bar (tests report the measured error).
 * H tensor [M, F]: row m holds planes x ldh 16-bit values, ldh >= F, pad columns zero.  Single plane: [v(0..ldh)],
 *   ldh % 64 == 0 when the tensor feeds p2w_gemm_h2.  F16X3: ldh % 32 == 0 and the row is a sequence of blocks of 32
 *   columns, each stored as [hi(32) | lo(32)] (column c: hi at 64*(c/32) + c%32, lo 32 values further; value = hi + lo).
 *   Either way the 64 values a GEMM K-slab takes from a row are one 128-byte cache line, staged by 16-byte direct-to-LDS
 *   copies (8 whole lines per wave-instruction).  F16X3 has the bytes of fp32, the others half.
 * H weights: Wh = [N_pad][planes * K_pad] of W * 2^e, rows (= output channels) laid out like H tensor rows (e chosen at
 *   pack time so that the F16X3 lo part stays a normal fp16; wscale = 2^-e is applied in the epilogue), dims from
 *   p2w_packed_dims_h. */
#define P2W_PREC_F16X3 0
#define P2W_PREC_F16 1
#define P2W_PREC_BF16 2
int32_t p2w_packed_dims_h(int32_t prec, int32_t N, int32_t K, int32_t* N_pad, int32_t* K_pad);

/* flags of p2w_gemm_h2 (0 = let the library choose).  There are no environment switches behind this ABI. */
#define P2W_GEMM_TILE_128 1      /* force the 128 x 128 workgroup tile */
#define P2W_GEMM_TILE_256 2      /* force the 256 x 256 workgroup tile */
#define P2W_GEMM_GENERIC_EPI 4   /* run the runtime-flag epilogue instead of the specialised one */
#define P2W_GEMM_ORDER_ROWS 8    /* tile order: an XCD owns whole row tiles (W re-read from its L2) */
#define P2W_GEMM_ORDER_COLS 16   /* tile order: an XCD owns a slice of column tiles (A streamed per slice) */
#define P2W_GEMM_RESIDUAL_H 32   /* epi->residual is an H tensor of the launch's precision (epi->ldr = its row pitch ldh), not fp32 */
#define P2W_GEMM_STREAMK 64      /* p2w_gemm_h2_sk: run the rows behind the whole chip rounds as a split-K tail even where the cost model says no */
#define P2W_GEMM_NO_STREAMK 128  /* p2w_gemm_h2_sk: never (= p2w_gemm_h2) */
#define P2W_GEMM_TILE_64 (1 << 24)  /* force the 64 x 128 workgroup tile (three workgroups per CU; the library takes it for short-K launches
                                       with one or two column tiles or a mostly empty last round of 128 x 128 tiles) */
#define P2W_GEMM_NO_TILE_64 (1 << 25)  /* never take it */
/* flags of p2w_sa_conv_h (0 = let the library choose the work-item shape by C2) */
#define P2W_SA_ITEM_256 1        /* 4 targets x 256 output columns per work item */
#define P2W_SA_ITEM_128 2        /* 8 targets x 128 output columns per work item */
#define P2W_SA_PACK8 4           /* targets with <= 8 neighbours share a 32-row MFMA tile four at a time (sparse ball-query levels) */
/* bits 8..23 of `flags` of p2w_gemm_h2 / p2w_sa_conv_h are reserved: they must be zero and are ignored. */

/* p2w_gemm with an H A operand, H weights and fp32 and/or H outputs (either pointer may be NULL):
 * Linear / 1x1 Conv1d + folded BatchNorm / depthwise affines + ReLU + residual - model.py:75-85, :198-202, :241-242.
 * ldh_a / ldh_o are row PITCHES: A_h / out_h may point into wider rows (e.g. the skip columns of a concatenated [interp | skip]
 * row, model.py:151: the producer of the skip features writes them in place).  The launch writes its N output columns and the
 * zero pad columns up to min(ldh_o, round_up(N, K granularity)); it never touches columns beyond that. */
int32_t p2w_gemm_h2(int32_t prec, const void* A_h, int32_t ldh_a, const void* Wh, float wscale, int32_t M, int32_t N,
                    int32_t K, const p2w_epilogue* epi, float* out_f32, int32_t ldo, void* out_h, int32_t ldh_o,
                    int32_t flags, p2w_stream_t stream);
/* p2w_gemm_h2 with a caller-owned workspace (the ABI never allocates): the library may then run the rows that do not fill a whole
 * round of the chip's workgroup slots as a second launch - plainly, or as a SPLIT-K tail: each 128 x 128 tile's K range cut into S
 * pieces that run side by side (raw fp32 partial tiles in `ws`) + a fix-up pass that adds a tile's pieces in ascending K order
 * (deterministic) and runs the same epilogue.  What a launch takes is decided from (M, N, K) alone, so equal calls give equal
 * bits; results differ from p2w_gemm_h2's in the last fp32 bits only (the K range is summed in pieces).  ws: 16-byte aligned,
 * p2w_gemm_h2_sk_ws_bytes() bytes (32 MiB on a 256-CU chip) make every plan possible (a smaller one narrows the choice, ws = NULL
 * is p2w_gemm_h2); it must not be shared by launches that may run concurrently (one per stream). */
size_t p2w_gemm_h2_sk_ws_bytes(void);
int32_t p2w_gemm_h2_sk(int32_t prec, const void* A_h, int32_t ldh_a, const void* Wh, float wscale, int32_t M, int32_t N,
                       int32_t K, const p2w_epilogue* epi, float* out_f32, int32_t ldo, void* out_h, int32_t ldh_o,
                       void* ws, size_t ws_bytes, int32_t flags, p2w_stream_t stream);
/* conv1 + BN + ReLU + conv2 for ONE output channel (model.py:241-243) as one operator: out[i] = dot(epilogue(A_h[i,:] * W^T), dot_w) +
 * dot_b.  The [M, N] intermediate never reaches HBM: the GEMM's epilogue leaves one partial sum per row and 64-column slice in
 * ws, a finishing pass adds the slices in a fixed order (deterministic).  epi->residual is not supported (P2W_EUNSUPPORTED).
 * ws: 16-byte aligned, p2w_gemm_h2_rowdot_ws_bytes(M, N) bytes. */
size_t p2w_gemm_h2_rowdot_ws_bytes(int32_t M, int32_t N);
int32_t p2w_gemm_h2_rowdot(int32_t prec, const void* A_h, int32_t ldh_a, const void* Wh, float wscale, int32_t M, int32_t N,
                           int32_t K, const p2w_epilogue* epi, const float* dot_w, float dot_b, float* out, void* ws,
                           size_t ws_bytes, int32_t flags, p2w_stream_t stream);
/* p2w_sa_conv with H weights W2h and fp32 and/or H outputs.  P (the hoisted layer-1 product, fp32) has n_src + 1 rows of
 * ldp >= round_up(C1, K granularity) floats: rows 0..n_src-1 = x_src * W1x^T + b1 with ZERO pad columns; row n_src is the row
 * empty neighbour slots read (the kernel's loads are unconditional): it must EXIST, the call fills it with zeros itself (the only
 * write through P).
 * Outputs (either pointer may be NULL, not both): out[M, ldo] fp32 - the call writes columns 0..C2-1 of rows 0..M-1 and nothing
 * else; out_h = an H tensor of row pitch ldh (ldh >= C2, a multiple of 8; of 32 for F16X3) - the call writes the C2 output
 * columns and ZEROS in the columns from C2 up to min(ldh, round_up(C2, W)), W = the width of a work item's column tile: 256
 * (C2 > 128, or P2W_SA_ITEM_256) or 128 (C2 <= 128, or P2W_SA_ITEM_128).  So the zero pad up to round_up(C2, K granularity)
 * is always written when ldh covers it, a wider row may be zeroed up to the end of the last column tile, and no column from
 * round_up(C2, 256) on is ever touched.  Rows >= M are never written.
 * ws: 16-byte aligned scratch of >= p2w_sa_conv_h_ws_bytes(M, flags) bytes for the per-edge metadata (P2W_EWORKSPACE otherwise; what it
 * holds on entry does not matter: the call's pre-pass writes every word its kernels read);
 * kw <= 32 (one 32-row MFMA tile per target); round_up(C1, K granularity) <= 512, C2 <= 1024 (LDS tables), M < 2^25 and
 * (n_src + 1) * ldp < 2^33 (32-bit offsets) - P2W_EUNSUPPORTED otherwise. */
size_t p2w_sa_conv_h_ws_bytes(int32_t M, int32_t flags);
int32_t p2w_sa_conv_h(int32_t prec, const float* P, int32_t ldp, int32_t n_src, const float* xyzr_src, const int32_t* idx,
                      const int32_t* batch_dst, const float* sf, const int32_t* nbr, const int32_t* deg, int32_t kw,
                      int32_t M, const float* w1r4, const void* W2h, float wscale, int32_t C1, int32_t C2,
                      const float* b2, const float* bn_s, const float* bn_t, float* out, int32_t ldo, void* out_h,
                      int32_t ldh, void* ws, size_t ws_bytes, int32_t flags, p2w_stream_t stream);
/* p2w_sa_conv_h for a P whose rows are NOT in the source points' own order: src_row[j] = the P row of source point j (NULL =
 * identity = p2w_sa_conv_h).  The engine keeps the level-0 features in the sampler's cell order (p2w_stem_h2_indexed): neighbours
 * in space are neighbours in memory for the P gather and for the last interpolation. */
int32_t p2w_sa_conv_h_rows(int32_t prec, const float* P, int32_t ldp, int32_t n_src, const float* xyzr_src, const int32_t* idx,
                           const int32_t* batch_dst, const float* sf, const int32_t* nbr, const int32_t* deg, int32_t kw,
                           int32_t M, const float* w1r4, const void* W2h, float wscale, int32_t C1, int32_t C2,
                           const float* b2, const float* bn_s, const float* bn_t, float* out, int32_t ldo, void* out_h,
                           int32_t ldh, void* ws, size_t ws_bytes, int32_t flags, const int32_t* src_row, uint32_t* range,
                           p2w_stream_t stream);
/* The small kernels writing H (and fp32 where given): stem (model.py:208,228), knn_interpolate + cat (:149-151),
 * cat(x, pos) (:135).  For the stem and the interpolation `ldh` is the row pitch as in p2w_gemm_h2: they write their columns
 * (C, resp. Fc + Fs) plus the zero pad to the next K-slab boundary and leave the rest of a wider row alone (p2w_interp_concat_h2
 * with skip = NULL, Fs = 0 writes only the interpolated part of a row whose skip columns another producer has written).
 * All three write 16 bytes at a time: `out` (fp32, where given) and `out_h` must be 16-byte aligned (P2W_EALIGN), as the inputs
 * they read 16 bytes at a time (xyzr, xc, skip, x). */
/* range (p2w_stem_h2, p2w_stem_h2_indexed, p2w_sa_conv_h_rows; NULL = off): the range watch of p2w_epilogue.range - a device
 * block of P2W_RANGE_WORDS words (the caller zeroes them). */
int32_t p2w_stem_h2(int32_t prec, const float* xyzr, int32_t n, const float* w, const float* b, int32_t C, float* out,
                    void* out_h, int32_t ldh, uint32_t* range, p2w_stream_t stream);
/* ... for records that come in another order (p2w_index_records: e.g. the sampler's cell order) and carry their own row as the
 * int32 in .w: the fp32 row of record i is out[.w], its H row is out_h[i] (model.py:228 stores the stem features on the batch in
 * input order; the H copy feeds the GEMMs in the records' order). */
int32_t p2w_stem_h2_indexed(int32_t prec, const float* xyzr, int32_t n, const float* w, const float* b, int32_t C, float* out,
                            void* out_h, int32_t ldh, uint32_t* range, p2w_stream_t stream);
int32_t p2w_interp_concat_h2(int32_t prec, const float* xc, int32_t Fc, const float* xyzr_c, const float* xyzr_f,
                             const int32_t* nbr, const int32_t* deg, int32_t kw, const float* skip, int32_t Fs, int32_t m,
                             void* out_h, int32_t ldh, p2w_stream_t stream);
/* knn_interpolate's weights alone (model.py:149, kw <= 2), for p2w_epilogue.interp: records[q] = {n0, n1, a0, a1}, a_s = w_s /
 * (w_0 + w_1), w_s = 1 / max(d2, 1e-16); a row with one neighbour gets {n0, n0, 1, 0}.  kw > 2: P2W_EUNSUPPORTED. */
int32_t p2w_interp_weights(const float* xyzr_c, const float* xyzr_f, const int32_t* nbr, const int32_t* deg, int32_t kw, int32_t m,
                           void* records, p2w_stream_t stream);
int32_t p2w_concat_xyz_h2(int32_t prec, const float* x, int32_t F, const float* xyzr, int32_t m, void* out_h, int32_t ldh,
                          p2w_stream_t stream);

/* knn_interpolate (k<=2) + concat with the skip features - model.py:149-151:
 *   out[q, 0:Fc] = (sum_s w_s * xc[nbr[q,s]]) / (sum_s w_s),  w_s = 1/max(d2, 1e-16)
 *   out[q, Fc:Fc+Fs] = skip[q].  Rows padded to ldo are zero-filled. */
int32_t p2w_interp_concat(const float* xc, int32_t Fc, const float* xyzr_c, const float* xyzr_f, const int32_t* nbr,
                          const int32_t* deg, int32_t kw, const float* skip, int32_t Fs, int32_t m, float* out,
                          int32_t ldo, p2w_stream_t stream);

/* [x | xyz] concat feeding GlobalSAModule.NN - model.py:135.  out[q] = [x[q, 0:F] | x, y, z | 0 ...] up to ldo (the record's .w
 * does not enter); F and ldo multiples of 4, ldo >= F + 4; x, xyzr and out 16-byte aligned (P2W_EALIGN). */
int32_t p2w_concat_xyz(const float* x, int32_t F, const float* xyzr, int32_t m, float* out, int32_t ldo,
                       p2w_stream_t stream);

/* global_max_pool - model.py:136: out[b,:] = max over rows ptr[b]..ptr[b+1] (empty = 0). */
int32_t p2w_segment_max(const float* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out,
                        p2w_stream_t stream);

/* conv2 with one output channel - model.py:243: out[i] = dot(x[i,:], w) + b. */
int32_t p2w_rowdot(const float* x, int32_t ldx, int32_t F, const float* w, float b, int32_t m, float* out,
                   p2w_stream_t stream);

/* FPModule 4 (model.py:236): the coarse level has ONE point per voxel: nbr[q] = batch[q], deg = 1. */
int32_t p2w_fill_batch_nbr(const int32_t* batch, int32_t m, int32_t* nbr, int32_t* deg, p2w_stream_t stream);

/* ---- backward passes of the operator route (pointstowood_amd/ops.py) ---- */
/* No floating-point atomics: the same bits on every run.  The fused p2w_sa_conv* and the GEMMs have no backward. */

/* p2w_segment_max plus its winners: out[B, F] (dense) holds the bits p2w_segment_max gives; arg[b, c] (int32, dense [B, F]) = the
 * lowest row of ptr[b] .. ptr[b+1] whose value equals out[b, c], -1 for an empty segment (out = 0) and for a column of NaNs only.
 * 16-byte accesses when F and ldx are multiples of 4 and x, out, arg are 16-byte aligned, 4-byte accesses otherwise. */
int32_t p2w_segment_max_arg(const float* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out, int32_t* arg,
                            p2w_stream_t stream);
/* Its gradient, a gather: grad_x[r, c] = (arg[b(r), c] == r) ? grad_out[b(r), c] : 0 for r < n, c < F, b(r) the segment of row r
 * (ptr[0] = 0; rows from ptr[B] on get 0).  Every element is written exactly once: the caller does not clear grad_x.  The whole
 * gradient of a tied maximum goes to the lowest row. */
int32_t p2w_segment_max_bwd(const float* grad_out, int32_t ldg, const int32_t* arg, const int32_t* ptr, int32_t B, int32_t F,
                            float* grad_x, int32_t ldx, int32_t n, p2w_stream_t stream);
/* Gradient of knn_interpolate (p2w_interp_concat without skip) with respect to the coarse features:
 *   grad_x[j, 0:F] = sum over the slots (q, s), s < deg[q], nbr[q, s] == j, of a(q, s) * grad_out[q, 0:F],
 * a(q, s) = w / sum_s w, w = 1 / max(d2, 1e-16) as in the forward (the sum in slot order), for every j < n_coarse: a row nobody
 * references gets zeros.  The slots are transposed with p2w_sort_pairs_u64 (key = j, value = q kw + s: stable, so a row's slots
 * stay ascending) and p2w_cell_starts; a row's run is summed in fp32 in ascending slot order by the row lanes of one block and,
 * where the mean run is long (one coarse point per voxel), by several blocks, and combined in a tree fixed by the sizes.
 * 1 <= kw <= P2W_MAX_K_WIDE (else P2W_EINVAL); F, ldg, ldx multiples of 4 (else P2W_EINVAL); grad_out, grad_x, xyzr_*, ws 16-byte
 * aligned (else P2W_EALIGN); ws: p2w_interp_bwd_ws_bytes(m, kw, n_coarse) bytes (0 = bad sizes; too small: P2W_EWORKSPACE). */
size_t p2w_interp_bwd_ws_bytes(int32_t m, int32_t kw, int32_t n_coarse);
int32_t p2w_interp_bwd(const float* grad_out, int32_t ldg, int32_t F, const float* xyzr_c, const float* xyzr_f, const int32_t* nbr,
                       const int32_t* deg, int32_t kw, int32_t m, int32_t n_coarse, float* grad_x, int32_t ldx, void* ws,
                       size_t ws_bytes, p2w_stream_t stream);

/* ---- layer 1 of the PointNetConv edge MLP for training (pointstowood_amd/ops.py: edge_layer1) ---- */
/* The hoisted layer 1 of local_nn per edge (pointnet.py:116-132, model.py:198-202).  The caller computes P[n_src, C1] (pitch ldp) =
 * x_src W1[:, :F_in]^T + b1 once per source; the edges are grouped by target: ptr[M + 1] is the CSR over the targets (ptr[0] = 0,
 * ptr[M] = E, any degree), src[E] the source of each edge.  rec_src[n_src, 4] / rec_dst[M, 4] = x, y, z, reflectance;
 * Wg[4, C1] (dense) = the rows of W1's last four columns.  For edge e = (j -> i), in fp32:
 *   geo[e, 0:3] = (pos_j - pos_i) / (maxd_i + 1e-8), maxd_i = max over i's edges of sqrt(((dx*dx)+(dy*dy))+(dz*dz));  geo[e, 3] = refl_j
 *   H1[e, c]    = relu((((P[j, c] + geo0 Wg[0, c]) + geo1 Wg[1, c]) + geo2 Wg[2, c]) + geo3 Wg[3, c])       (pitch ldh; no fma)
 * geo[E, 4] is dense.  A target all of whose neighbours coincide with it gets geo[:, 0:3] = 0 exactly.  The kernel clamps ptr to
 * [0, E], and an edge whose source is outside [0, n_src) gets geo = 0 and H1 = 0, so no index is followed out of bounds; rows of
 * geo / H1 that no target's range covers are not written.  One launch; M = 0 or E = 0 launches nothing.
 * Access width: C1 a multiple of 4 -> 16 bytes per lane, and then ldp, ldh must be multiples of 4 and P, Wg, H1 16-byte aligned
 * (P2W_EALIGN otherwise); any other C1 -> 4 bytes per lane.  rec_src, rec_dst and geo are always 16-byte aligned (P2W_EALIGN).
 * n_src, M, E >= 0, C1 >= 1, ldp, ldh >= C1, E = 0 where M = 0 or n_src = 0 (P2W_EINVAL). */
int32_t p2w_edge_l1(const float* P, int32_t ldp, const float* rec_src, const float* rec_dst, const int32_t* ptr, const int32_t* src,
                    const float* Wg, int32_t n_src, int32_t M, int32_t E, int32_t C1, float* geo, float* H1, int32_t ldh,
                    p2w_stream_t stream);
/* Its backward.  With gZ[e, c] = (H1[e, c] > 0) ? gH[e, c] : 0 (H1 and geo as the forward left them):
 *   gP[s, 0:C1]  = sum of gZ[e, :] over the edges with src[e] == s, for every s < n_src (pitch ldgp; no reference: zeros)
 *   gR[s]        = sum_c gP[s, c] Wg[3, c]  = the gradient with respect to the source's reflectance (no reference: 0)
 *   gWg[d, c]    = sum_e geo[e, d] gZ[e, c]                                                    (dense [4, C1])
 * Positions get no gradient.  No floating-point atomics, the same bits on every run: the edges are transposed by source with
 * p2w_sort_pairs_u64 (stable: a source's edges stay ascending) and p2w_cell_starts, and a source's run is summed like a row of
 * p2w_interp_bwd (ascending edge order over the row lanes of a block, a tree fixed by the sizes); gR adds gP's columns lane by
 * lane and the lanes in a fixed butterfly; gWg adds the edges of each chunk of P2W_EDGE_CHUNK edges over row lanes and a tree,
 * and a second launch adds the chunks in ascending order.  An edge whose source is outside [0, n_src) enters no sum of gP.
 * Every element of gP[0 .. n_src), gR and gWg is written: the caller clears nothing.  Widths and alignment as in the forward
 * (gH, H1, gP, gWg and ldg, ldh, ldgp with C1 a multiple of 4; geo and ws always: P2W_EALIGN); sizes as in the forward
 * (P2W_EINVAL); ws: p2w_edge_l1_bwd_ws_bytes(E, n_src, C1) bytes (0 = bad sizes; too small: P2W_EWORKSPACE). */
#define P2W_EDGE_CHUNK 1024
size_t p2w_edge_l1_bwd_ws_bytes(int32_t E, int32_t n_src, int32_t C1);
int32_t p2w_edge_l1_bwd(const float* gH, int32_t ldg, const float* H1, int32_t ldh, const float* geo, const int32_t* src,
                        const float* Wg, int32_t n_src, int32_t E, int32_t C1, float* gP, int32_t ldgp, float* gR, float* gWg, void* ws,
                        size_t ws_bytes, p2w_stream_t stream);

/* ---- ReLU, training-mode BatchNorm1d and the max over the targets' edges in one (pointstowood_amd/ops.py: relu_bn_max) ---- */
/* The tail of local_nn[1] and the aggregation of the training route (model.py:198-202, pointnet.py:122) on the layer-2 pre-activation
 * z[E, C2] (pitch ldz), grouped by target: ptr[M + 1] is the CSR over the targets (ptr[0] = 0, ptr[M] = E, any degree).  Per column
 * BatchNorm is an affine map, non-decreasing for gamma >= 0 and non-increasing for gamma < 0, so the maximum of BN(relu(z)) over a
 * target's rows is BN of the rows' maximum of relu(z), or of their minimum where gamma < 0.  With y = z > 0 ? z : 0 (a NaN counts as 0):
 *   mean[c]   = (1 / E) sum_e y[e, c],   var[c] = max((1 / E) sum_e y[e, c]^2 - mean[c]^2, 0),   invstd[c] = 1 / sqrt(var[c] + eps)
 *               sums and arithmetic in fp64, each result rounded to fp32 once (var is the biased batch variance)
 *   ext[i, c] = max (gamma[c] >= 0) or min (gamma[c] < 0) of y[e, c] over ptr[i] <= e < ptr[i + 1];      0 for a target without rows
 *   arg[i, c] = the lowest such row that holds ext[i, c] (the tie rule of p2w_segment_max_arg: a segment of ReLU zeros sends
 *               everything to its first row);                                                            -1 for a target without rows
 *   out[i, c] = ((ext[i, c] - mean[c]) * invstd[c]) * gamma[c] + beta[c]     (fp32 on the rounded mean and invstd, no fma);    0 likewise
 *   running_mean[c] = (1 - momentum) running_mean[c] + momentum mean[c],
 *   running_var[c]  = (1 - momentum) running_var[c]  + momentum var[c] E / (E - 1)          (in place, fp64 arithmetic, rounded once)
 * out, ext, arg are dense [M, C2]; gamma, beta, running_*, mean, invstd [C2].  z is read once.  Three launches: the fp64 column sums
 * and the extrema per work item of P2W_BN_GROUP consecutive targets (one lane per column walks the item's rows in ascending order);
 * the items in ascending order, and the statistics; the map on [M, C2].  No floating-point atomics: the bits depend on the inputs
 * alone, not on the run, the grid or the access width.
 * The kernels clamp ptr to [0, E] and make it non-decreasing, so no offset is followed out of bounds; ptr[0] = 0 and ptr[M] = E are
 * the caller's contract (they cannot be checked without a synchronisation: rows outside [ptr[0], ptr[M]) enter no sum).
 * Access width: 16 bytes per lane when C2 and ldz are multiples of 4 and z, gamma, beta, out, ext, arg, mean, invstd are 16-byte
 * aligned, 4 bytes otherwise (same bits).  ws: 16-byte aligned (P2W_EALIGN), p2w_relu_bn_max_ws_bytes(E, M, C2) bytes (0 = bad sizes;
 * too small: P2W_EWORKSPACE).  2 <= E < 2^31 - 1 (one row has no variance), 1 <= M < 2^31 - 1, C2 >= 1, M C2 <= 2^38, ldz >= C2,
 * eps >= 0, 0 <= momentum <= 1 (P2W_EINVAL); every pointer is required (P2W_ENULL).  Nothing is allocated, and a refused call
 * launches nothing. */
#define P2W_BN_GROUP 16
size_t p2w_relu_bn_max_ws_bytes(int32_t E, int32_t M, int32_t C2);
int32_t p2w_relu_bn_max(const float* z, int32_t ldz, const int32_t* ptr, const float* gamma, const float* beta, float* running_mean,
                        float* running_var, double momentum, double eps, int32_t E, int32_t M, int32_t C2, float* out, float* ext,
                        int32_t* arg, float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream);
/* Its backward, on what the forward left (arg, ext, mean, invstd) and the gradient g[M, C2] (dense) of out.  Over the targets with rows:
 *   dbeta[c]  = sum_i g[i, c],      dgamma[c] = sum_i g[i, c] ((ext[i, c] - mean[c]) invstd[c])
 *               fp64 terms on the fp32 inputs, fp64 partials per P2W_BN_GROUP consecutive targets in ascending order, the groups in
 *               ascending order, rounded to fp32 once; k1 = dbeta / E and k2 = dgamma / E likewise
 *   xhat      = (y[e, c] - mean[c]) * invstd[c]
 *   dy[e, c]  = (((arg[i(e), c] == e ? g[i(e), c] : 0) - k1[c]) - xhat * k2[c]) * (gamma[c] * invstd[c])        (fp32, no fma)
 *   dz[e, c]  = z[e, c] > 0 ? dy[e, c] : 0                                                                     (pitch lddz)
 * z is read once and every element of dz's rows [ptr[0], ptr[M]) = [0, E) is written once; dgamma and dbeta [C2] are written, not added
 * to.  Three launches; no floating-point atomics.  Access width as in the forward (g, z, arg, ext, mean, invstd, gamma, dz, ldz and
 * lddz decide it); ws and sizes as in the forward, lddz >= C2. */
int32_t p2w_relu_bn_max_bwd(const float* g, const float* z, int32_t ldz, const int32_t* ptr, const int32_t* arg, const float* ext,
                            const float* mean, const float* invstd, const float* gamma, int32_t E, int32_t M, int32_t C2, float* dz,
                            int32_t lddz, float* dgamma, float* dbeta, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* ---- chains of depthwise convolution, training-mode BatchNorm1d and ReLU between two GEMMs (pointstowood_amd/ops.py: bn_chain) ---- */
/* What the inverted residual block (model.py:46-85) runs between two of its 1x1 convolutions in training mode, on the pre-activation
 * z[M, C] (pitch ldz).  A chain has L stages, 1 <= L <= P2W_BN_CHAIN_MAX; stage s = 1 .. L has the input u_{s-1}, u_0 = z:
 *   v_s = fl(fl(dw_w u_{s-1}) + dw_b)                           the depthwise convolution with kernel size 1 (dw_w = dw_b = NULL: v_s = u_{s-1})
 *   mean_s = (1 / M) sum v_s,  var_s = max((1 / M) sum v_s^2 - mean_s^2, 0),  invstd_s = 1 / sqrt(var_s + eps)
 *            from the fp64 column sums of u_{s-1} and u_{s-1}^2 (mean_s = dw_w mean_u + dw_b, var_s = dw_w^2 var_u), fp64 arithmetic,
 *            each result rounded to fp32 once; var is the biased batch variance
 *   y_s = fl(fl(fl(fl(v_s - mean_s) invstd_s) gamma) + beta)    on the rounded mean and invstd, no fma
 *   u_s = relu ? (y_s < 0 ? 0 : y_s) : y_s                      (a NaN stays a NaN and poisons its column, as in PyTorch)
 *   running_mean = (1 - momentum) running_mean + momentum mean_s,  running_var likewise with var_s M / (M - 1)   (in place, fp64, rounded once)
 * out (pitch ldo) = u_L, or with a residual res[M, C] (pitch ldr; NULL = none) out = max(u_L + res, 0).  mean and invstd are [L, C]
 * (stage s at (s - 1) C).  2 L + 1 launches: per stage the fp64 column sums per work item of P2W_BN_CHAIN_ROWS consecutive rows (one
 * lane per column walks them in ascending order, the stages before it recomputed in fp32 from z) and the items in ascending order with
 * the statistics; then the chain on [M, C].  z is read L + 1 times, out written once, nothing else of that size exists.  No
 * floating-point atomics: the bits depend on the inputs alone, not on the run, the grid or the access width.
 * Access width: 16 bytes per lane when C and every pitch are multiples of 4 and z, res, out, mean, invstd and the stages' dw_w, dw_b,
 * gamma, beta are 16-byte aligned, 4 bytes otherwise (same bits).  ws: 16-byte aligned (P2W_EALIGN), p2w_bn_chain_ws_size(M, C, L) bytes
 * (0 = bad sizes; too small: P2W_EWORKSPACE; one size serves both directions).  2 <= M < 2^31 - 1 (one row has no variance), C >= 1,
 * M C <= 2^38, 1 <= L <= P2W_BN_CHAIN_MAX, every pitch >= C, dw_w and dw_b both or neither, eps >= 0, 0 <= momentum <= 1 (P2W_EINVAL);
 * every other pointer is required (P2W_ENULL).  `stages` is a HOST array read during the call.  A refused call launches nothing. */
#define P2W_BN_CHAIN_MAX 3
#define P2W_BN_CHAIN_ROWS 32
typedef struct p2w_bn_stage {
    const float* dw_w;        /* [C] depthwise weight and bias in front of the BatchNorm; both NULL = none */
    const float* dw_b;
    const float* gamma;       /* [C] BatchNorm's weight and bias */
    const float* beta;
    float* running_mean;      /* [C], updated in place by the forward; the backward does not look at them */
    float* running_var;
    double momentum;          /* the forward's; the backward does not look at them */
    double eps;
    int32_t relu;             /* != 0: ReLU behind the BatchNorm */
} p2w_bn_stage;
size_t p2w_bn_chain_ws_size(int32_t M, int32_t C, int32_t L);
int32_t p2w_bn_chain(const float* z, int32_t ldz, const float* res, int32_t ldr, const p2w_bn_stage* stages, int32_t L, int32_t M,
                     int32_t C, float* out, int32_t ldo, float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream);
/* Its backward, on z, the forward's mean and invstd, the stages' vectors and the gradient g[M, C] (pitch ldg) of out.  `out` (pitch ldo) is
 * the forward's output where the chain had a residual and NULL where it had none: with it g = g [out > 0] first, and dres (pitch lddr;
 * NULL = not wanted) = that g.  The forward is recomputed from z with the forward's code, so every ReLU mask is the forward's.  For
 * s = L .. 1, with xhat_s = fl(fl(v_s - mean_s) invstd_s):
 *   gy = relu_s ? g [u_s > 0] : g,   dbeta_s = sum gy,   dgamma_s = sum gy xhat_s
 *            fp64 terms on the fp32 values, per work item in ascending row order, the items in ascending order, rounded to fp32 once;
 *            k1 = dbeta_s / M and k2 = dgamma_s / M likewise
 *   gv = fl(fl(fl(gy - k1) - fl(xhat_s k2)) fl(gamma invstd_s)),   g = fl(gv dw_w)                                    (fp32, no fma)
 *   ddw_w_s = gamma invstd_s (sum gy u_{s-1} - (dbeta_s / M) sum u_{s-1} - (dgamma_s / M) sum xhat_s u_{s-1})   = sum gv u_{s-1}, in fp64 from
 *            three more fp64 column sums taken beside the other two, rounded once; tiny against its terms (only eps keeps it from 0)
 *   ddw_b_s = 0 exactly: BatchNorm removes a bias added in front of it (sum gv = 0 because sum xhat = 0)
 * and dz (pitch lddz) = g.  dgamma, dbeta, ddw_w, ddw_b are [L, C], written, not added to; ddw_w and ddw_b are 0 for a stage without a
 * depthwise convolution and may be NULL when no stage has one.  2 L + 1 launches; z and g are read L + 1 times, dz (and dres) written once;
 * no other [M, C] tensor, no atomics.  Access width, ws and sizes as in the forward (g, z, out, dz, dres, mean, invstd, the stages' vectors
 * and every pitch decide the width); dres needs out (P2W_EINVAL). */
int32_t p2w_bn_chain_bwd(const float* g, int32_t ldg, const float* z, int32_t ldz, const float* out, int32_t ldo,
                         const p2w_bn_stage* stages, int32_t L, const float* mean, const float* invstd, int32_t M, int32_t C, float* dz,
                         int32_t lddz, float* dres, int32_t lddr, float* dgamma, float* dbeta, float* ddw_w, float* ddw_b, void* ws,
                         size_t ws_bytes, p2w_stream_t stream);

/* ---- ReLU in front of one training-mode BatchNorm1d on rows (pointstowood_amd/ops.py: relu_bn) ---- */
/* The tail of the feature-propagation MLP (model.py:198-202: Linear, ReLU, BatchNorm1d) on the pre-activation z[M, C] (pitch ldz):
 * out = BN(relu(z)).  By definition the one-stage p2w_bn_chain (no depthwise convolution, no ReLU behind the BatchNorm, no residual) on
 *   u = z < 0 ? 0 : z                                           (a NaN stays a NaN and poisons its column)
 * computed as z is loaded - u is never stored.  Formulas, rounding points, the fp64 column sums per P2W_BN_CHAIN_ROWS consecutive rows in
 * ascending order, the work items in ascending order and the running-statistics update are that chain's (the same device code), so out,
 * mean, invstd [C] and running_* equal p2w_bn_chain on a materialised relu(z) bit for bit.  Three launches; z is read twice, out
 * (pitch ldo) written once, no other [M, C] tensor, no atomics.  Access width, alignment, sizes and status codes as p2w_bn_chain with
 * L = 1; ws: p2w_relu_bn_ws_size(M, C) bytes (= p2w_bn_chain_ws_size(M, C, 1); 0 = bad sizes; one size serves both directions).
 * A refused call launches nothing. */
size_t p2w_relu_bn_ws_size(int32_t M, int32_t C);
int32_t p2w_relu_bn(const float* z, int32_t ldz, const float* gamma, const float* beta, float* running_mean, float* running_var,
                    double momentum, double eps, int32_t M, int32_t C, float* out, int32_t ldo, float* mean, float* invstd, void* ws,
                    size_t ws_bytes, p2w_stream_t stream);
/* Its backward, on z, the forward's mean and invstd, gamma and the gradient g[M, C] (pitch ldg) of out: that chain's backward with
 *   xhat = fl(fl(u - mean) invstd),   dbeta = sum g,   dgamma = sum g xhat,   k1 = dbeta / M,   k2 = dgamma / M        (fp64 sums as there)
 *   gv = fl(fl(fl(g - k1) - fl(xhat k2)) fl(gamma invstd)),      dz = z > 0 ? gv : 0                                    (pitch lddz)
 * dgamma, dbeta [C] are written, not added to.  Three launches; z and g are read twice, dz written once; no other [M, C] tensor, no
 * atomics.  Width, ws and sizes as in the forward. */
int32_t p2w_relu_bn_bwd(const float* g, int32_t ldg, const float* z, int32_t ldz, const float* gamma, const float* mean,
                        const float* invstd, int32_t M, int32_t C, float* dz, int32_t lddz, float* dgamma, float* dbeta, void* ws,
                        size_t ws_bytes, p2w_stream_t stream);

/* ---- layer 0 of the feature-propagation module for training (pointstowood_amd/ops.py: interp_add_relu, FPModule) ---- */
/* knn_interpolate is linear in the coarse features and its weights sum to 1, so layer 0 of FPModule's MLP (model.py:142-153) on
 * [interp(xc) | x_skip] is interp(Pc) + S with Pc[n_c, C] (pitch ldp) = xc W0[:, :Fc]^T on the coarse rows and S[m, C] (pitch lds) =
 * x_skip W0[:, Fc:]^T + b0 on the fine rows, both the caller's GEMMs.  For fine row q < m and column c < C, in fp32 without fma:
 *   t = num / den    p2w_interp_concat's arithmetic on Pc: w_s = 1 / max(d2, 1e-16), d2 = (dx dx + dy dy) + dz dz,
 *                    num = ((0 + Pc[n_0, c] w_0) + Pc[n_1, c] w_1) + ... and den = ((0 + w_0) + w_1) + ... in slot order over
 *                    s < min(deg[q], kw), a literal division; t = 0 where deg[q] <= 0
 *   h = fl(t + S[q, c]),    H[q, c] = h < 0 ? 0 : h                              (pitch ldh; a NaN stays a NaN)
 * xyzr_c[n_c, 4], xyzr_f[m, 4] = x, y, z, (unused); nbr[m, kw], deg[m] as the searches write them.  nbr[q, s] for s < deg[q] lies in
 * [0, n_c): the caller's contract (the kernel clamps it into the range, and takes deg as 0 where n_c = 0, so no index is followed out
 * of bounds).  One launch (one wave per row, 16-byte accesses, two 256-column chunks' loads in flight for rows of up to four
 * neighbours), no workspace, no atomics; S is read once, H written once, the rows of Pc are gathered.  Neither the interpolated
 * [m, C] tensor nor the [m, Fc + Fs] concatenation is formed.
 * 1 <= kw <= P2W_MAX_K_WIDE, m kw < 2^31, m, n_c >= 0, C >= 4, C and every pitch multiples of 4, pitches >= C (P2W_EINVAL); every
 * tensor 16-byte aligned (P2W_EALIGN); m = 0: P2W_OK without a launch. */
int32_t p2w_interp_add_relu(const float* Pc, int32_t ldp, const float* S, int32_t lds, const float* xyzr_c, const float* xyzr_f,
                            const int32_t* nbr, const int32_t* deg, int32_t kw, int32_t m, int32_t n_c, int32_t C, float* H, int32_t ldh,
                            p2w_stream_t stream);
/* Its backward, on the forward's output H and the gradient g[m, C] (pitch ldg) of H:
 *   dS[q, c]  = H[q, c] > 0 ? g[q, c] : 0                                        (pitch ldds; one pass: reads g and H, writes dS)
 *   dPc[j, :] = sum over the slots (q, s), s < deg[q], nbr[q, s] == j, of a(q, s) dS[q, :]      (pitch lddp)
 * dPc is p2w_interp_bwd of dS - that entry point itself, on this workspace: the stable sort, the run sums in ascending slot order, the
 * tree fixed by the sizes, the same bits; a coarse row nobody references gets zeros.  Every element of dS [m, C] and dPc [n_c, C] is
 * written: the caller clears nothing.  No floating-point atomics.  Sizes and alignment as in the forward (g, H, dS, dPc, xyzr_*, ws:
 * P2W_EALIGN); ws: p2w_interp_add_relu_bwd_ws_size(m, kw, n_c) bytes (0 = bad sizes; too small: P2W_EWORKSPACE).  A refused call
 * launches nothing. */
size_t p2w_interp_add_relu_bwd_ws_size(int32_t m, int32_t kw, int32_t n_c);
int32_t p2w_interp_add_relu_bwd(const float* g, int32_t ldg, const float* H, int32_t ldh, const float* xyzr_c, const float* xyzr_f,
                                const int32_t* nbr, const int32_t* deg, int32_t kw, int32_t m, int32_t n_c, int32_t C, float* dS,
                                int32_t ldds, float* dPc, int32_t lddp, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* ---- the head behind conv1 for training with one class (pointstowood_amd/ops.py: bn_relu_rowdot) ---- */
/* model.py:242-243 on the pre-activation z[M, C] (pitch ldz) in rows: training-mode BatchNorm1d, ReLU and the 1 x C convolution,
 *   logit[r] = fl(sum_c fl(w[c] u[r, c]) + bias),   u = relu(BN(z)),
 * without u [M, C] or its gradient ever being stored.  gamma, beta, w are [C]; bias is a DEVICE scalar; logit is [M].  By definition
 * the statistics and u are the one-stage p2w_bn_chain's (no depthwise convolution, ReLU behind the BatchNorm, no residual): the same
 * device code, the fp64 column sums per P2W_BN_CHAIN_ROWS consecutive rows in ascending order, the work items in ascending order, the
 * same rounding points of xhat, y and u = y < 0 ? 0 : y, the same running-statistics update - so mean, invstd [C] and running_* equal
 * p2w_bn_chain (L = 1) bit for bit.  Three launches; the third replaces the chain's apply pass: z is read twice, M floats are written.
 * The sum of a row, an order that depends on C alone: one wave takes 16 consecutive rows and sums each of them on its own; lane
 * l = 0 .. 63 owns the columns 256 p + 4 l + e (e = 0 .. 3) of pass p = 0, 1, ...; every lane starts at +0 and adds fl(w[c] u[r, c])
 * over its columns c < C in ascending order; the 64 lanes are then added in a butterfly (partner lane ^ 32, ^ 16, ^ 8, ^ 4, ^ 2, ^ 1),
 * and bias is added last.  fp32, no fma, no atomics: the same bits on every run and at either access width.
 * Access width: 16 bytes per lane when C and ldz are multiples of 4 and z, gamma, beta, w, mean, invstd are 16-byte aligned, 4 bytes
 * otherwise (same columns per lane, same bits).  ws: 16-byte aligned (P2W_EALIGN), p2w_bn_relu_rowdot_ws_size(M, C) bytes (0 = bad
 * sizes; too small: P2W_EWORKSPACE; one size serves both directions).  2 <= M < 2^31 - 1, C >= 1, M C <= 2^38, ldz >= C, eps >= 0,
 * 0 <= momentum <= 1 (P2W_EINVAL); every pointer is required (P2W_ENULL).  A NaN in z poisons its column (and with it every logit), as
 * in PyTorch.  A refused call launches nothing. */
size_t p2w_bn_relu_rowdot_ws_size(int32_t M, int32_t C);
int32_t p2w_bn_relu_rowdot(const float* z, int32_t ldz, const float* gamma, const float* beta, const float* w, const float* bias,
                           float* running_mean, float* running_var, double momentum, double eps, int32_t M, int32_t C, float* logit,
                           float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream);
/* Its backward, on z, the forward's mean and invstd, gamma, beta, w and the gradient g[M] of the logits.  The forward is recomputed from
 * z with the forward's code on the forward's rounded mean and invstd, so the ReLU mask is the forward's.  With xhat = fl(fl(z - mean)
 * invstd) and gy[r, c] = fl(g[r] w[c]) [u[r, c] > 0], formed in registers:
 *   dbeta = sum gy,   dgamma = sum gy xhat,   dw = sum g u   per column,   dbias = sum g
 *            fp64 terms on the fp32 values, per work item of P2W_BN_CHAIN_ROWS rows in ascending row order, the items in ascending order
 *            (dbias: 64 chains over the items i, i + 64, ... and a butterfly over the chains), rounded to fp32 once
 *   dz = fl(fl(fl(gy - k1) - fl(xhat k2)) fl(gamma invstd)),   k1 = dbeta / M,   k2 = dgamma / M        (pitch lddz; fp32, no fma)
 * dz, dgamma and dbeta equal p2w_bn_chain_bwd (L = 1, ReLU) fed the materialised gradient fl(g[r] w[c]) bit for bit.  dgamma, dbeta,
 * dw [C] and dbias (a device scalar) are written, not added to.  Three launches; z is read twice and g (M floats) twice, dz written
 * once; no other [M, C] tensor, no atomics.  Width (dz and lddz count as well), ws, sizes and status codes as in the forward. */
int32_t p2w_bn_relu_rowdot_bwd(const float* g, const float* z, int32_t ldz, const float* gamma, const float* beta, const float* w,
                               const float* mean, const float* invstd, int32_t M, int32_t C, float* dz, int32_t lddz, float* dgamma,
                               float* dbeta, float* dw, float* dbias, void* ws, size_t ws_bytes, p2w_stream_t stream);

/* ---- the training operators on float16 and bfloat16 tensors (pointstowood_amd/ops.py: half_io) ---- */
/* Under autocast the GEMMs between the training operators give and take float16 or bfloat16.  Each entry point below is its namesake
 * with `void*` for the [rows, C] tensors and one dtype code per tensor group, so that a 16-bit tensor is read and written as it is
 * instead of through an fp32 copy.  ONLY the element type at the loads and stores differs: every kernel widens a 16-bit element as it
 * loads it (exact: a bfloat16's 16 bits become the top half of the fp32 pattern) and computes in fp32 / fp64 exactly as its namesake -
 * the same operations, sums, orders, launches and workspace (the *_ws_size functions are shared) - and a 16-bit store rounds the fp32
 * result once, to nearest, ties to the even mantissa:
 *   float16   overflow to +-inf, gradual underflow to subnormals and +-0, a NaN kept a NaN: torch.Tensor.half();
 *   bfloat16  a carry out of the largest finite value gives +-inf (the patterns 0x7F7F8000 and up), fp32 subnormals round to bfloat16
 *             subnormals and +-0 (nothing is flushed), the sign of zero is kept, a NaN stays a NaN - one whose payload lies only in
 *             the low 16 bits included, which a truncation would turn into an infinity: torch.Tensor.bfloat16().
 * So every fp32 result equals the fp32 entry point's on the widened tensors bit for bit, and every 16-bit result is that entry
 * point's fp32 result rounded once.
 *   tz  z and dz          (p2w_bn_chain*, p2w_relu_bn*): P2W_F32, P2W_F16 or P2W_BF16; (p2w_bn_relu_rowdot*): P2W_F32 or P2W_F16
 *   to  out and g         (p2w_bn_chain*, p2w_relu_bn*): P2W_F32, or equal to tz where tz is a 16-bit type
 *   tx  x and grad_x      (p2w_segment_max_*): P2W_F32 or P2W_F16; out, grad_out and arg stay fp32 / int32 (a maximum of widened
 *                         values is exact)
 *   tz  z and dz          (p2w_relu_bn_max_io / _bwd_io): P2W_F32, P2W_F16 or P2W_BF16; g and out stay fp32, like ext, arg and every
 *                         [C2] vector (an extremum of widened values is exact); both directions share p2w_relu_bn_max_ws_bytes
 *   th  H1                (p2w_edge_l1_io): P2W_F32, P2W_F16 or P2W_BF16; P, Wg, rec_* and geo stay fp32
 *   tg  gH                (p2w_edge_l1_bwd_io): P2W_F32, P2W_F16 or P2W_BF16; P, geo, Wg, gP, gR and gWg stay fp32, H1 is no argument
 *                         (the ReLU mask is recomputed); the workspace is p2w_edge_l1_bwd_ws_bytes
 * The four chain entry points take P2W_BF16.  p2w_bn_relu_rowdot_io / _bwd_io and p2w_segment_max_arg_io / _bwd_io have one code
 * each and answer 2 with P2W_EUNSUPPORTED like any other unknown code (tests/test_gpu_half_io.py: test_refusals_launch_nothing
 * asserts it of them); their bfloat16 instantiations are the four p2w_*_bf16 entry points below the _io ones.
 * The residual, dres, the saved out of a chain with a residual, the logits and their gradient, every [C] / [L, C] vector and the
 * workspace stay fp32 / fp64.  Pitches are in elements.  Access width: a lane keeps its 4 adjacent columns, an 8-byte access on a
 * 16-bit tensor - it needs an 8-byte aligned pointer and a pitch divisible by 4 where an fp32 tensor needs 16 bytes; otherwise one
 * column per lane, the same bits.  Any other code, a float16 / bfloat16 mix, or a combination not listed: P2W_EUNSUPPORTED, checked
 * first.  Every other status code is the namesake's; a refused call launches nothing.  With P2W_F32 everywhere these ARE the fp32
 * entry points (which call them). */
#define P2W_F32 0
#define P2W_F16 1
#define P2W_BF16 2
int32_t p2w_bn_chain_io(const void* z, int32_t tz, int32_t ldz, const float* res, int32_t ldr, const p2w_bn_stage* stages, int32_t L,
                        int32_t M, int32_t C, void* out, int32_t to, int32_t ldo, float* mean, float* invstd, void* ws, size_t ws_bytes,
                        p2w_stream_t stream);
int32_t p2w_bn_chain_bwd_io(const void* g, int32_t to, int32_t ldg, const void* z, int32_t tz, int32_t ldz, const float* out, int32_t ldo,
                            const p2w_bn_stage* stages, int32_t L, const float* mean, const float* invstd, int32_t M, int32_t C, void* dz,
                            int32_t lddz, float* dres, int32_t lddr, float* dgamma, float* dbeta, float* ddw_w, float* ddw_b, void* ws,
                            size_t ws_bytes, p2w_stream_t stream);
int32_t p2w_relu_bn_io(const void* z, int32_t tz, int32_t ldz, const float* gamma, const float* beta, float* running_mean,
                       float* running_var, double momentum, double eps, int32_t M, int32_t C, void* out, int32_t to, int32_t ldo,
                       float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream);
int32_t p2w_relu_bn_bwd_io(const void* g, int32_t to, int32_t ldg, const void* z, int32_t tz, int32_t ldz, const float* gamma,
                           const float* mean, const float* invstd, int32_t M, int32_t C, void* dz, int32_t lddz, float* dgamma,
                           float* dbeta, void* ws, size_t ws_bytes, p2w_stream_t stream);
int32_t p2w_bn_relu_rowdot_io(const void* z, int32_t tz, int32_t ldz, const float* gamma, const float* beta, const float* w,
                              const float* bias, float* running_mean, float* running_var, double momentum, double eps, int32_t M,
                              int32_t C, float* logit, float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream);
int32_t p2w_bn_relu_rowdot_bwd_io(const float* g, const void* z, int32_t tz, int32_t ldz, const float* gamma, const float* beta,
                                  const float* w, const float* mean, const float* invstd, int32_t M, int32_t C, void* dz, int32_t lddz,
                                  float* dgamma, float* dbeta, float* dw, float* dbias, void* ws, size_t ws_bytes, p2w_stream_t stream);
int32_t p2w_segment_max_arg_io(const void* x, int32_t tx, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out,
                               int32_t* arg, p2w_stream_t stream);
int32_t p2w_segment_max_bwd_io(const float* grad_out, int32_t ldg, const int32_t* arg, const int32_t* ptr, int32_t B, int32_t F,
                               void* grad_x, int32_t tx, int32_t ldx, int32_t n, p2w_stream_t stream);
int32_t p2w_relu_bn_max_io(const void* z, int32_t tz, int32_t ldz, const int32_t* ptr, const float* gamma, const float* beta,
                           float* running_mean, float* running_var, double momentum, double eps, int32_t E, int32_t M, int32_t C2,
                           float* out, float* ext, int32_t* arg, float* mean, float* invstd, void* ws, size_t ws_bytes,
                           p2w_stream_t stream);
int32_t p2w_relu_bn_max_bwd_io(const float* g, const void* z, int32_t tz, int32_t ldz, const int32_t* ptr, const int32_t* arg,
                               const float* ext, const float* mean, const float* invstd, const float* gamma, int32_t E, int32_t M,
                               int32_t C2, void* dz, int32_t lddz, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                               p2w_stream_t stream);
/* Layer 1 of the edge MLP with H1 in fp32, float16 or bfloat16 (th), and its backward with gH in any of the three (tg).  The forward
 * is p2w_edge_l1 (which calls it with P2W_F32): P, rec_*, Wg and geo stay fp32, the arithmetic and its order are the namesake's, a
 * 16-bit H1 is the namesake's fp32 H1 rounded once.  C1 a multiple of 4: H1 needs 4 sizeof(element) bytes of alignment (8 for a
 * 16-bit type) and ldh a multiple of 4 (P2W_EALIGN).
 * The backward is NOT given H1.  A stored float16 zero may stand for an fp32 h in (0, 2^-25] (bfloat16: below 2^-134), so a mask
 * read back from a 16-bit H1 would differ from the fp32 route's; the kernels recompute
 *   h = relu((((P[j, c] + geo0 Wg[0, c]) + geo1 Wg[1, c]) + geo2 Wg[2, c]) + geo3 Wg[3, c]),  j = src[e],
 * with the forward's own statements (no contraction: the same bits) from P[n_src, C1] (pitch ldp, fp32 - the forward's P), geo, src and
 * Wg, and take gZ[e, c] = (h > 0) ? gH[e, c] : 0; an edge whose source is outside [0, n_src) has gZ = 0 (the forward wrote 0 there).
 * Everything else is p2w_edge_l1_bwd: the sort, the run sums, the chunks, gR, the workspace (p2w_edge_l1_bwd_ws_bytes) and the fp32
 * gP, gR, gWg - bit for bit what p2w_edge_l1_bwd gives on the widened gH and the fp32 H1.  C1 a multiple of 4: ldg, ldp, ldgp
 * multiples of 4, gH aligned to 4 sizeof(element) bytes, P, Wg, gP, gWg to 16 (P2W_EALIGN); geo and ws always 16.
 *   th  H1 (p2w_edge_l1_io), tg  gH (p2w_edge_l1_bwd_io): P2W_F32, P2W_F16 or P2W_BF16; any other code: P2W_EUNSUPPORTED, checked first */
int32_t p2w_edge_l1_io(const float* P, int32_t ldp, const float* rec_src, const float* rec_dst, const int32_t* ptr, const int32_t* src,
                       const float* Wg, int32_t n_src, int32_t M, int32_t E, int32_t C1, float* geo, void* H1, int32_t th, int32_t ldh,
                       p2w_stream_t stream);
int32_t p2w_edge_l1_bwd_io(const void* gH, int32_t tg, int32_t ldg, const float* P, int32_t ldp, const float* geo, const int32_t* src,
                           const float* Wg, int32_t n_src, int32_t E, int32_t C1, float* gP, int32_t ldgp, float* gR, float* gWg,
                           void* ws, size_t ws_bytes, p2w_stream_t stream);
/* The head and the segment max on bfloat16 tensors: what their _io entry points would do for tz / tx = P2W_BF16 - the namesake's
 * arguments without the dtype code, z and dz (x and grad_x) bfloat16, everything else as above: the same launches, sums, workspace and
 * status codes, the widening load exact, every bfloat16 store one rounding to nearest even, 8-byte accesses where an 8-byte aligned
 * pointer and a pitch divisible by 4 allow. */
int32_t p2w_bn_relu_rowdot_bf16(const void* z, int32_t ldz, const float* gamma, const float* beta, const float* w, const float* bias,
                                float* running_mean, float* running_var, double momentum, double eps, int32_t M, int32_t C,
                                float* logit, float* mean, float* invstd, void* ws, size_t ws_bytes, p2w_stream_t stream);
int32_t p2w_bn_relu_rowdot_bwd_bf16(const float* g, const void* z, int32_t ldz, const float* gamma, const float* beta, const float* w,
                                    const float* mean, const float* invstd, int32_t M, int32_t C, void* dz, int32_t lddz,
                                    float* dgamma, float* dbeta, float* dw, float* dbias, void* ws, size_t ws_bytes,
                                    p2w_stream_t stream);
int32_t p2w_segment_max_arg_bf16(const void* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out, int32_t* arg,
                                 p2w_stream_t stream);
int32_t p2w_segment_max_bwd_bf16(const float* grad_out, int32_t ldg, const int32_t* arg, const int32_t* ptr, int32_t B, int32_t F,
                                 void* grad_x, int32_t ldx, int32_t n, p2w_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* P2W_H */
