// Sums of the backward passes that replace a scatter-add (p2w_grad.hip: p2w_interp_bwd, p2w_edge.hip: p2w_edge_l1_bwd): every
// destination row adds the terms of its run of a stably sorted slot list in ascending slot order, in a tree whose shape depends on
// the sizes alone - no floating-point atomics, the same bits on every run.  What a slot contributes is the caller's: a functor
//     term(slot value, column, float (&t)[V])        the V terms of that slot at columns c .. c + V
// V = 4: 16-byte accesses (rows, pitches and pointers must allow them), V = 1: 4-byte accesses, still coalesced.
#pragma once
#include "p2w_common.h"

namespace {     // (template kernels: one private copy per translation unit)

template <int V> __device__ __forceinline__ void gr_ld(const float* p, float (&v)[V]) {
    if constexpr (V == 4) { const float4 t = *reinterpret_cast<const float4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p;
}
template <int V> __device__ __forceinline__ void gr_ld(const int* p, int (&v)[V]) {
    if constexpr (V == 4) { const int4 t = *reinterpret_cast<const int4*>(p); v[0] = t.x; v[1] = t.y; v[2] = t.z; v[3] = t.w; }
    else v[0] = *p;
}
template <int V> __device__ __forceinline__ void gr_st(float* p, const float (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
template <int V> __device__ __forceinline__ void gr_st(int* p, const int (&v)[V]) {
    if constexpr (V == 4) *reinterpret_cast<int4*>(p) = make_int4(v[0], v[1], v[2], v[3]);
    else *p = v[0];
}
inline bool gr_al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

// float16 rows (P2W_F16): the arithmetic stays fp32, only the element type at the loads and stores differs.  A lane keeps its V
// columns: V = 4 is one 8-byte access.  The widening load is exact (subnormals included).  EVERY fp16 store goes through gr_f2h:
// one conversion per element, round to nearest even, overflow to +-inf, gradual underflow to subnormals and +-0, a NaN stays a
// NaN - what torch.Tensor.half() gives.  (The packed conversion that rounds toward zero must not be used.)
typedef _Float16 gr_half;
typedef _Float16 gr_half4 __attribute__((ext_vector_type(4)));
// med3(f, f, f) = f (a NaN stays a NaN, -0 stays -0) keeps the fp32 value apart from the conversion: left alone, the compiler folds
// the conversion into the multiply that produced the value as one mixed-precision FMA with a +0 addend (v_fma_mixlo_f16 a, b, 0) -
// one rounding where the fp32 route has two, and +0 where the product is -0.  One v_med3_f32 per stored element in kernels that
// wait for memory; an empty asm statement would cost nothing, but inline asm is convergent and the row loops are then not unrolled.
__device__ __forceinline__ gr_half gr_f2h(float f) {
    return static_cast<gr_half>(__builtin_amdgcn_fmed3f(f, f, f));
}
template <int V> __device__ __forceinline__ void gr_ld(const gr_half* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const gr_half4 t = *reinterpret_cast<const gr_half4*>(p);
        v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
    } else v[0] = (float)*p;
}
template <int V> __device__ __forceinline__ void gr_st(gr_half* p, const float (&v)[V]) {
    if constexpr (V == 4) {
        gr_half4 t;
        t.x = gr_f2h(v[0]); t.y = gr_f2h(v[1]); t.z = gr_f2h(v[2]); t.w = gr_f2h(v[3]);
        *reinterpret_cast<gr_half4*>(p) = t;
    } else *p = gr_f2h(v[0]);
}
// bfloat16 rows (P2W_BF16): the same scheme.  The widening load is exact - the 16 bits are the top half of the fp32 pattern.  EVERY
// bf16 store goes through gr_f2b: one conversion per element, round to nearest even, a carry out of the largest finite value to
// +-inf, fp32 subnormals to bf16 subnormals and +-0 (nothing flushed), a NaN stays a NaN whatever its payload - what
// torch.Tensor.bfloat16() gives.  med3 stands between the value and the conversion for gr_f2h's reason.
typedef __bf16 gr_bf16;
typedef __bf16 gr_bf164 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ gr_bf16 gr_f2b(float f) {
    return static_cast<gr_bf16>(__builtin_amdgcn_fmed3f(f, f, f));
}
template <int V> __device__ __forceinline__ void gr_ld(const gr_bf16* p, float (&v)[V]) {
    if constexpr (V == 4) {
        const gr_bf164 t = *reinterpret_cast<const gr_bf164*>(p);
        v[0] = (float)t.x; v[1] = (float)t.y; v[2] = (float)t.z; v[3] = (float)t.w;
    } else v[0] = (float)*p;
}
template <int V> __device__ __forceinline__ void gr_st(gr_bf16* p, const float (&v)[V]) {
    if constexpr (V == 4) {
        gr_bf164 t;
        t.x = gr_f2b(v[0]); t.y = gr_f2b(v[1]); t.z = gr_f2b(v[2]); t.w = gr_f2b(v[3]);
        *reinterpret_cast<gr_bf164*>(p) = t;
    } else *p = gr_f2b(v[0]);
}
// a V = 4 access of element type T needs 4 sizeof(T) bytes of alignment: 16 for fp32, 8 for fp16 and bf16
template <class T> inline bool gr_alv(const T* p) { return (reinterpret_cast<uintptr_t>(p) & (4 * sizeof(T) - 1)) == 0; }

constexpr int RUN_SPLIT_MIN = 512;    // mean run length from which the runs are split over blocks
constexpr int RUN_SPLIT_LEN = 256;    // ... into pieces of about this many slots
constexpr int RUN_SPLIT_MAX = 64;
template <int V> constexpr int run_panel() { return 64 * V; }      // columns per block pass: one wave of V-float lanes

// lanes per row: the power of two that covers F columns, at most one wave
template <int V> inline int run_row_lanes(int F) {
    const int q = (F + V - 1) / V;
    int W = 1;
    while (W < q && W < 64) W <<= 1;
    return W;
}
// pieces a run is cut into: from the slot count and the row count alone
inline int run_pieces(long long N, int rows) {
    const long long avg = rows > 0 ? N / rows : 0;
    const long long Z = avg >= RUN_SPLIT_MIN ? avg / RUN_SPLIT_LEN : 1;
    return (int)(Z > RUN_SPLIT_MAX ? RUN_SPLIT_MAX : Z);
}
// the partial rows of run_sum (Z > 1 only; Z rows <= N / 256)
inline size_t run_part_floats(int Z, int rows, int panel) { return Z > 1 ? (size_t)Z * rows * panel : 0; }

// One block per (row j, piece z of its run, panel).  The run [start[j], start[j + 1]) of the sorted slot list is cut into
// gridDim.y = Z pieces at L z / Z; inside a piece the block's P = 256 / W row lanes (W = V-float lanes per row, a power of two
// <= 64) take slots p, p + P, ... in ascending order and are added in a binary tree in LDS.  Z, P and W follow from the sizes
// alone, so the summation order of a row depends only on its run length.  Z == 1 writes the result, Z > 1 a partial row.
template <int V, class Term>
__global__ __launch_bounds__(256) void run_sum_kernel(Term term, int F, const int* __restrict__ start, const int* __restrict__ slot, int W,
                                                      int c0, float* __restrict__ dst, int ldd, int dst_c0) {
    __shared__ __attribute__((aligned(16))) float sm[256 * V];
    const int j = blockIdx.x, z = blockIdx.y, Z = gridDim.y;
    const int cl = threadIdx.x & (W - 1), p = threadIdx.x / W, P = 256 / W;
    const int c = c0 + blockIdx.z * run_panel<V>() + cl * V;
    const int s0 = start[j], L = start[j + 1] - s0;
    const int a0 = s0 + (int)((long long)L * z / Z), a1 = s0 + (int)((long long)L * (z + 1) / Z);
    float acc[V];
#pragma unroll
    for (int u = 0; u < V; ++u) acc[u] = 0.f;
    if (c < F) {
#pragma unroll 4
        for (int i = a0 + p; i < a1; i += P) {
            float t[V];
            term(slot[i], c, t);
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] = acc[u] + t[u];
        }
    }
    for (int h = P >> 1; h >= 1; h >>= 1) {
        gr_st<V>(&sm[threadIdx.x * V], acc);
        __syncthreads();
        if (p < h) {
            float t[V];
            gr_ld<V>(&sm[(threadIdx.x + h * W) * V], t);
#pragma unroll
            for (int u = 0; u < V; ++u) acc[u] = acc[u] + t[u];
        }
        __syncthreads();
    }
    if (p == 0 && c < F)
        gr_st<V>(&dst[((size_t)z * gridDim.x + j) * ldd + dst_c0 + blockIdx.z * run_panel<V>() + cl * V], acc);
}
// the Z partial rows of a panel, added in ascending z
template <int V>
__global__ __launch_bounds__(256) void run_combine_kernel(const float* __restrict__ part, int Z, int rows, int F, int c0,
                                                          float* __restrict__ out, int ldo) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    const int j = (int)(g >> 6), c = c0 + (int)(g & 63) * V;
    if (j >= rows || c >= F) return;
    float acc[V];
    gr_ld<V>(&part[(size_t)j * run_panel<V>() + (c - c0)], acc);
    for (int z = 1; z < Z; ++z) {
        float t[V];
        gr_ld<V>(&part[((size_t)z * rows + j) * run_panel<V>() + (c - c0)], t);
#pragma unroll
        for (int u = 0; u < V; ++u) acc[u] = acc[u] + t[u];
    }
    gr_st<V>(&out[(size_t)j * ldo + c], acc);
}

// out[j, 0:F] = the sum of row j's run for j < rows (rows > 0); Z = run_pieces(N, rows), `part`: run_part_floats(Z, rows, panel) floats
template <int V, class Term>
inline void run_sum(const Term& term, int F, const int* start, const int* slot, int rows, int Z, float* part, float* out, int ldo,
                    hipStream_t s) {
    const int W = run_row_lanes<V>(F), panels = p2w_cdiv(F, run_panel<V>());
    if (Z == 1) {
        run_sum_kernel<V><<<dim3(rows, 1, panels), 256, 0, s>>>(term, F, start, slot, W, 0, out, ldo, 0);
    } else {
        for (int pnl = 0; pnl < panels; ++pnl) {
            const int c0 = pnl * run_panel<V>();
            run_sum_kernel<V><<<dim3(rows, Z, 1), 256, 0, s>>>(term, F, start, slot, W, c0, part, run_panel<V>(), 0);
            run_combine_kernel<V><<<p2w_cdiv((long)rows * 64, 256), 256, 0, s>>>(part, Z, rows, F, c0, out, ldo);
        }
    }
}

}  // namespace
