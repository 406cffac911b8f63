// Backward passes of the operator route (pointstowood_amd/ops.py): the three operators of the reference forward that sit between
// parameters and loss without being plain PyTorch modules - the max aggregation of MessagePassing.propagate (pointnet.py:108),
// global_max_pool (model.py:136) and knn_interpolate (model.py:149).
//
// Same bits on every run: no floating-point atomics anywhere.  The max's winner is combined with integer atomicMax (order
// independent), the max's gradient is a gather, and the interpolation's gradient sums every coarse row's references in ascending
// slot order after a stable sort, in a tree whose shape depends only on the sizes.
// All kernels are bandwidth-bound: one wave covers 256 consecutive columns of a row with 16-byte accesses where rows and pointers
// allow it (V = 4), and falls back to 4-byte accesses (V = 1, still coalesced) for odd widths.
// The segment max also takes a float16 x and writes a float16 grad_x (p2w_segment_max_arg_io / _bwd_io; TX = gr_half, p2w_runsum.h):
// values are widened as they are loaded - a maximum of widened values is exact, so out stays fp32 - and the gathered gradient is
// rounded to nearest even as it is stored; V = 4 is then an 8-byte access.  The same on a bfloat16 x (TX = gr_bf16):
// p2w_segment_max_arg_bf16 / _bwd_bf16.
#include "p2w_runsum.h"
#include "p2w_segmax.h"

namespace {

// the order-preserving key of p2w_segment_max (p2w_feat.hip) and its inverse
__device__ __forceinline__ unsigned gr_f2ord(float f) {
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float gr_ord2f(unsigned o) {
    return __uint_as_float((o & 0x80000000u) ? (o & 0x7fffffffu) : ~o);
}

// ------------------------------------------------------------------------------------------------ segment max + arg
// Many segments (the edge form: one segment per target): one block per (segment, 64 V columns), the four waves take rows
// r, r + 4, ... and are combined in LDS; value and winner are written directly.  A NaN takes no part (fmaxf in p2w_segment_max
// ignores it too); the value is the maximum by the order key (the bits p2w_segment_max's atomicMax leaves), the winner the
// lowest row that compares equal to it.
template <int V, class TX>
__global__ __launch_bounds__(256) void segmax_arg_kernel(const TX* __restrict__ x, int ldx, int F, const int* __restrict__ ptr, int ncg,
                                                         float* __restrict__ out, int* __restrict__ arg) {
    __shared__ float sv[3][64 * V];
    __shared__ unsigned so[3][64 * V];
    __shared__ int sr[3][64 * V];
    const int b = blockIdx.x / ncg, cg = blockIdx.x % ncg;
    const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = (cg * 64 + lane) * V;
    const int s = ptr[b], e = ptr[b + 1];
    float bv[V]; unsigned bo[V]; int br[V];
#pragma unroll
    for (int u = 0; u < V; ++u) { bv[u] = -INFINITY; bo[u] = gr_f2ord(-INFINITY); br[u] = -1; }
    if (c < F) {
#pragma unroll 4
        for (int r = s + rl; r < e; r += 4) {
            float v[V];
            gr_ld<V>(&x[(size_t)r * ldx + c], v);
#pragma unroll
            for (int u = 0; u < V; ++u) {
                if (v[u] == v[u]) {
                    const unsigned o = gr_f2ord(v[u]);
                    bo[u] = o > bo[u] ? o : bo[u];
                    if (v[u] > bv[u] || (br[u] < 0 && v[u] == bv[u])) { bv[u] = v[u]; br[u] = r; }
                }
            }
        }
    }
    if (rl > 0) {
#pragma unroll
        for (int u = 0; u < V; ++u) { sv[rl - 1][lane * V + u] = bv[u]; so[rl - 1][lane * V + u] = bo[u]; sr[rl - 1][lane * V + u] = br[u]; }
    }
    __syncthreads();
    if (rl != 0 || c >= F) return;
    float ov[V]; int oa[V];
#pragma unroll
    for (int u = 0; u < V; ++u) {
        for (int w = 0; w < 3; ++w) {
            const float tv = sv[w][lane * V + u]; const unsigned to = so[w][lane * V + u]; const int tr = sr[w][lane * V + u];
            bo[u] = to > bo[u] ? to : bo[u];
            if (tr >= 0 && (br[u] < 0 || tv > bv[u] || (tv == bv[u] && tr < br[u]))) { bv[u] = tv; br[u] = tr; }
        }
        ov[u] = e > s ? gr_ord2f(bo[u]) : 0.f;
        oa[u] = br[u];
    }
    gr_st<V>(&out[(size_t)b * F + c], ov);
    gr_st<V>(&arg[(size_t)b * F + c], oa);
}

// Few segments (global_max_pool): p2w_segment_max itself gives the values (rows split over 16 blocks per segment, integer
// atomicMax); this kernel then finds the lowest row that equals the value, split the same way, with an integer atomicMax of
// 0xffffffff - row into `arg` (pre-set to 0, which decodes to -1 = no row).
template <int V, class TX>
__global__ __launch_bounds__(256) void segmax_argonly_kernel(const TX* __restrict__ x, int ldx, int F, const int* __restrict__ ptr,
                                                             const float* __restrict__ out, unsigned* __restrict__ arg) {
    __shared__ unsigned sk[3][64 * V];
    const int b = blockIdx.y;
    const int lane = threadIdx.x & 63, rl = threadIdx.x >> 6;
    const int c = (blockIdx.x * 64 + lane) * V;
    const int s = ptr[b], e = ptr[b + 1];
    const int per = (e - s + gridDim.z - 1) / gridDim.z;
    const int r0 = s + blockIdx.z * per, r1 = min(e, r0 + per);
    unsigned key[V];
#pragma unroll
    for (int u = 0; u < V; ++u) key[u] = 0u;
    if (c < F && r1 > r0) {
        float ov[V];
        gr_ld<V>(&out[(size_t)b * F + c], ov);
#pragma unroll 4
        for (int r = r0 + rl; r < r1; r += 4) {
            float v[V];
            gr_ld<V>(&x[(size_t)r * ldx + c], v);
#pragma unroll
            for (int u = 0; u < V; ++u)
                if (key[u] == 0u && v[u] == ov[u]) key[u] = 0xffffffffu - (unsigned)r;     // rows ascend: the first hit is the lowest
        }
    }
    if (rl > 0) {
#pragma unroll
        for (int u = 0; u < V; ++u) sk[rl - 1][lane * V + u] = key[u];
    }
    __syncthreads();
    if (rl != 0 || c >= F) return;
#pragma unroll
    for (int u = 0; u < V; ++u) {
        for (int w = 0; w < 3; ++w) { const unsigned t = sk[w][lane * V + u]; key[u] = t > key[u] ? t : key[u]; }
        if (key[u] != 0u) atomicMax(&arg[(size_t)b * F + c + u], key[u]);
    }
}
__global__ __launch_bounds__(256) void segmax_arg_decode_kernel(unsigned* __restrict__ arg, long long n) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n) arg[i] = 0xffffffffu - arg[i];      // 0 -> -1 as int32
}

// grad_x[r, c] = arg[b(r), c] == r ? grad_out[b(r), c] : 0: one thread per (row, V columns), every element written once.
template <int V, class TX>
__global__ __launch_bounds__(256) void segmax_bwd_kernel(const float* __restrict__ grad_out, int ldg, const int* __restrict__ arg,
                                                         const int* __restrict__ ptr, int B, int F, TX* __restrict__ grad_x, int ldx,
                                                         int n, int q) {
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= (long long)n * q) return;
    const int r = (int)(g / q), c = (int)(g % q) * V;
    float o[V];
#pragma unroll
    for (int u = 0; u < V; ++u) o[u] = 0.f;
    if (r < ptr[B]) {
        const int b = p2w_find_segment(ptr, B, r);
        int a[V]; float gv[V];
        gr_ld<V>(&arg[(size_t)b * F + c], a);
        gr_ld<V>(&grad_out[(size_t)b * ldg + c], gv);
#pragma unroll
        for (int u = 0; u < V; ++u) o[u] = a[u] == r ? gv[u] : 0.f;
    }
    gr_st<V>(&grad_x[(size_t)r * ldx + c], o);
}

// ------------------------------------------------------------------------------------------------ interpolation backward
// one thread per fine row: the forward's weights (p2w_interp_concat / p2w_interp_weights: w = 1 / max(d2, 1e-16), a = w / sum w,
// the sum in slot order) and the sort keys of the row's kw slots - the coarse index, n_coarse for a slot that is not in use
__global__ __launch_bounds__(256) void interp_bwd_prep_kernel(const float4* __restrict__ xyzr_c, const float4* __restrict__ xyzr_f,
                                                              const int* __restrict__ nbr, const int* __restrict__ deg, int kw, int m,
                                                              int n_coarse, unsigned long long* __restrict__ keys,
                                                              float* __restrict__ wgt) {
    const int q = blockIdx.x * 256 + threadIdx.x;
    if (q >= m) return;
    const int d = max(0, min(deg[q], kw));
    const float4 pf = xyzr_f[q];
    float den = 0.f;
    for (int s = 0; s < d; ++s) {
        const int j = nbr[(size_t)q * kw + s];
        if (j < 0 || j >= n_coarse) continue;
        const float4 pc = xyzr_c[j];
        den = den + 1.0f / fmaxf(p2w_d2(pc.x, pc.y, pc.z, pf.x, pf.y, pf.z), 1e-16f);
    }
    for (int s = 0; s < kw; ++s) {
        const int j = s < d ? nbr[(size_t)q * kw + s] : -1;
        const bool on = j >= 0 && j < n_coarse;
        float a = 0.f;
        if (on) {
            const float4 pc = xyzr_c[j];
            a = (1.0f / fmaxf(p2w_d2(pc.x, pc.y, pc.z, pf.x, pf.y, pf.z), 1e-16f)) / den;
        }
        keys[(size_t)q * kw + s] = on ? (unsigned long long)j : (unsigned long long)n_coarse;
        wgt[(size_t)q * kw + s] = a;
    }
}

// a slot's term of the run sums (p2w_runsum.h): its forward weight times the fine row's gradient
struct InterpTerm {
    const float* grad_out; int ldg; const float* wgt; int kw;
    __device__ __forceinline__ void operator()(int sl, int c, float (&t)[4]) const {
        const float a = wgt[sl];
        float g[4];
        gr_ld<4>(&grad_out[(size_t)(sl / kw) * ldg + c], g);
#pragma unroll
        for (int u = 0; u < 4; ++u) t[u] = a * g[u];
    }
};

struct IbWs { unsigned long long *keys_in, *keys_out; int* slot; float* wgt; int* start; float* part; void* sub; size_t sub_bytes; int Z; };
inline IbWs ib_carve(P2wArena& a, long long N, int n_coarse) {
    const size_t n1 = (size_t)(N > 0 ? N : 1);
    IbWs W;
    W.Z = run_pieces(N, n_coarse);
    W.keys_in = a.take<unsigned long long>(n1);
    W.keys_out = a.take<unsigned long long>(n1);
    W.slot = a.take<int>(n1);
    W.wgt = a.take<float>(n1);
    W.start = a.take<int>((size_t)n_coarse + 1);
    W.part = a.take<float>(run_part_floats(W.Z, n_coarse, run_panel<4>()));
    const size_t s = p2w_sort_pairs_u64_ws_bytes((int32_t)n1), c = p2w_cell_starts_ws_bytes(n_coarse);
    W.sub_bytes = P2wArena::up(s > c ? s : c);             // the sort's and the cell table's scratch, in turn
    W.sub = a.raw(W.sub_bytes);
    return W;
}

}  // namespace

namespace {

// the values of the few-segment route, by x's element type
inline int32_t segmax_values(const float* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out, p2w_stream_t stream) {
    return p2w_segment_max(x, ldx, F, ptr, B, out, stream);
}
inline int32_t segmax_values(const gr_half* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out, p2w_stream_t stream) {
    return segment_max_launch(x, ldx, F, ptr, B, out, p2w_s(stream));      // p2w_segment_max's kernels on the float16 element type
}
inline int32_t segmax_values(const gr_bf16* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out, p2w_stream_t stream) {
    return segment_max_launch(x, ldx, F, ptr, B, out, p2w_s(stream));      // ... and on the bfloat16 one
}

template <class TX>
int32_t segmax_arg_t(const TX* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out, int32_t* arg, p2w_stream_t stream) {
    P2W_CHECK_PTR(x); P2W_CHECK_PTR(ptr); P2W_CHECK_PTR(out); P2W_CHECK_PTR(arg);
    if (B <= 0 || F <= 0 || ldx < F) return P2W_EINVAL;
    hipStream_t s = p2w_s(stream);
    const bool v4 = !(F & 3) && !(ldx & 3) && gr_alv(x) && gr_al16(out) && gr_al16(arg);
    const int ncg = p2w_cdiv(F, v4 ? 256 : 64);
    if ((long long)B * ncg >= 256) {
        if ((long long)B * ncg > 0x7fffffffll) return P2W_EINVAL;
        if (v4) segmax_arg_kernel<4, TX><<<B * ncg, 256, 0, s>>>(x, ldx, F, ptr, ncg, out, arg);
        else segmax_arg_kernel<1, TX><<<B * ncg, 256, 0, s>>>(x, ldx, F, ptr, ncg, out, arg);
        return P2W_LAUNCH_STATUS();
    }
    const int32_t st = segmax_values(x, ldx, F, ptr, B, out, stream);
    if (st != P2W_OK) return st;
    hipError_t e = hipMemsetAsync(arg, 0, sizeof(int32_t) * (size_t)B * F, s);
    if (e != hipSuccess) return (int32_t)e;
    auto* ua = reinterpret_cast<unsigned*>(arg);
    if (v4) segmax_argonly_kernel<4, TX><<<dim3(ncg, B, 16), 256, 0, s>>>(x, ldx, F, ptr, out, ua);
    else segmax_argonly_kernel<1, TX><<<dim3(ncg, B, 16), 256, 0, s>>>(x, ldx, F, ptr, out, ua);
    segmax_arg_decode_kernel<<<p2w_cdiv((long)B * F, 256), 256, 0, s>>>(ua, (long long)B * F);
    return P2W_LAUNCH_STATUS();
}

template <class TX>
int32_t segmax_bwd_t(const float* grad_out, int32_t ldg, const int32_t* arg, const int32_t* ptr, int32_t B, int32_t F, TX* grad_x, int32_t ldx,
                     int32_t n, p2w_stream_t stream) {
    P2W_CHECK_PTR(grad_out); P2W_CHECK_PTR(arg); P2W_CHECK_PTR(ptr); P2W_CHECK_PTR(grad_x);
    if (B <= 0 || F <= 0 || ldg < F || ldx < F || n < 0) return P2W_EINVAL;
    if (n == 0) return P2W_OK;
    const bool v4 = !(F & 3) && !(ldg & 3) && !(ldx & 3) && gr_al16(grad_out) && gr_al16(arg) && gr_alv(grad_x);
    const int q = v4 ? F >> 2 : F;
    const long long blocks = ((long long)n * q + 255) / 256;
    if (blocks > 0x7fffffffll) return P2W_EINVAL;
    if (v4) segmax_bwd_kernel<4, TX><<<(unsigned)blocks, 256, 0, p2w_s(stream)>>>(grad_out, ldg, arg, ptr, B, F, grad_x, ldx, n, q);
    else segmax_bwd_kernel<1, TX><<<(unsigned)blocks, 256, 0, p2w_s(stream)>>>(grad_out, ldg, arg, ptr, B, F, grad_x, ldx, n, q);
    return P2W_LAUNCH_STATUS();
}

}  // namespace

extern "C" int32_t p2w_segment_max_arg_io(const void* x, int32_t tx, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out,
                                          int32_t* arg, p2w_stream_t stream) {
    if (tx == P2W_F32) return segmax_arg_t(static_cast<const float*>(x), ldx, F, ptr, B, out, arg, stream);
    if (tx == P2W_F16) return segmax_arg_t(static_cast<const gr_half*>(x), ldx, F, ptr, B, out, arg, stream);
    return P2W_EUNSUPPORTED;
}

extern "C" int32_t p2w_segment_max_arg(const float* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out, int32_t* arg,
                                       p2w_stream_t stream) {
    return p2w_segment_max_arg_io(x, P2W_F32, ldx, F, ptr, B, out, arg, stream);
}

extern "C" int32_t p2w_segment_max_bwd_io(const float* grad_out, int32_t ldg, const int32_t* arg, const int32_t* ptr, int32_t B, int32_t F,
                                          void* grad_x, int32_t tx, int32_t ldx, int32_t n, p2w_stream_t stream) {
    if (tx == P2W_F32) return segmax_bwd_t(grad_out, ldg, arg, ptr, B, F, static_cast<float*>(grad_x), ldx, n, stream);
    if (tx == P2W_F16) return segmax_bwd_t(grad_out, ldg, arg, ptr, B, F, static_cast<gr_half*>(grad_x), ldx, n, stream);
    return P2W_EUNSUPPORTED;
}

extern "C" int32_t p2w_segment_max_bwd(const float* grad_out, int32_t ldg, const int32_t* arg, const int32_t* ptr, int32_t B, int32_t F,
                                       float* grad_x, int32_t ldx, int32_t n, p2w_stream_t stream) {
    return p2w_segment_max_bwd_io(grad_out, ldg, arg, ptr, B, F, grad_x, P2W_F32, ldx, n, stream);
}

// the bfloat16 instantiations (include/p2w.h: the dtype code 2 stays unknown to the two _io entry points above)
extern "C" int32_t p2w_segment_max_arg_bf16(const void* x, int32_t ldx, int32_t F, const int32_t* ptr, int32_t B, float* out, int32_t* arg,
                                            p2w_stream_t stream) {
    return segmax_arg_t(static_cast<const gr_bf16*>(x), ldx, F, ptr, B, out, arg, stream);
}

extern "C" int32_t p2w_segment_max_bwd_bf16(const float* grad_out, int32_t ldg, const int32_t* arg, const int32_t* ptr, int32_t B, int32_t F,
                                            void* grad_x, int32_t ldx, int32_t n, p2w_stream_t stream) {
    return segmax_bwd_t(grad_out, ldg, arg, ptr, B, F, static_cast<gr_bf16*>(grad_x), ldx, n, stream);
}

extern "C" size_t p2w_interp_bwd_ws_bytes(int32_t m, int32_t kw, int32_t n_coarse) {
    if (m < 0 || kw < 1 || kw > P2W_MAX_K_WIDE || n_coarse < 0 || (long long)m * kw > 0x7fffffffll) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { ib_carve(a, (long long)m * kw, n_coarse); });
}

extern "C" int32_t p2w_interp_bwd(const float* grad_out, int32_t ldg, int32_t F, const float* xyzr_c, const float* xyzr_f,
                                  const int32_t* nbr, const int32_t* deg, int32_t kw, int32_t m, int32_t n_coarse, float* grad_x,
                                  int32_t ldx, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (n_coarse == 0) return P2W_OK;
    P2W_CHECK_PTR(grad_x); P2W_CHECK_PTR(ws);
    if (m > 0) { P2W_CHECK_PTR(grad_out); P2W_CHECK_PTR(xyzr_c); P2W_CHECK_PTR(xyzr_f); P2W_CHECK_PTR(nbr); P2W_CHECK_PTR(deg); }
    P2W_CHECK_ALIGN16(grad_out); P2W_CHECK_ALIGN16(xyzr_c); P2W_CHECK_ALIGN16(xyzr_f); P2W_CHECK_ALIGN16(grad_x); P2W_CHECK_ALIGN16(ws);
    if (m < 0 || n_coarse < 0 || kw < 1 || kw > P2W_MAX_K_WIDE || (long long)m * kw > 0x7fffffffll) return P2W_EINVAL;
    if (F <= 0 || (F & 3) || (ldg & 3) || (ldx & 3) || ldg < F || ldx < F) return P2W_EINVAL;
    const int N = m * kw;
    P2wArena arena(ws);
    const IbWs L = ib_carve(arena, N, n_coarse);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    hipStream_t s = p2w_s(stream);
    unsigned long long *keys_in = L.keys_in, *keys_out = L.keys_out;
    int *slot = L.slot, *start = L.start;
    float *wgt = L.wgt, *part = L.part;
    int32_t st;
    if (N > 0) {
        interp_bwd_prep_kernel<<<p2w_cdiv(m, 256), 256, 0, s>>>(reinterpret_cast<const float4*>(xyzr_c), reinterpret_cast<const float4*>(xyzr_f),
                                                                nbr, deg, kw, m, n_coarse, keys_in, wgt);
        st = p2w_sort_pairs_u64(reinterpret_cast<const uint64_t*>(keys_in), reinterpret_cast<uint64_t*>(keys_out), nullptr, slot, N,
                                L.sub, L.sub_bytes, stream);
        if (st != P2W_OK) return st;
    }
    st = p2w_cell_starts(reinterpret_cast<const uint64_t*>(keys_out), N, n_coarse, start, L.sub, L.sub_bytes, stream);
    if (st != P2W_OK) return st;
    run_sum<4>(InterpTerm{grad_out, ldg, wgt, kw}, F, start, slot, n_coarse, L.Z, part, grad_x, ldx, s);
    return P2W_LAUNCH_STATUS();
}
