// Layer 1 of the PointNetConv edge MLP for training (pointnet.py:116-132, model.py:198-202), hoisted: the caller computes
// P = x_src W1[:, :F_in]^T + b1 once per source point, this file adds the four geometry columns per edge and applies the ReLU,
//     geo[e]  = ((pos_j - pos_i) / (maxd_i + 1e-8), refl_j),      maxd_i = max over the target's edges of |pos_j - pos_i|
//     H1[e,:] = relu(P[j,:] + geo[e,0] Wg[0,:] + geo[e,1] Wg[1,:] + geo[e,2] Wg[2,:] + geo[e,3] Wg[3,:])
// and gives the backward with respect to P, Wg and the source's reflectance.  The [E, F_in + 4] message tensor is never formed.
//
// Gather-and-stream kernels, bandwidth-bound: no LDS tiles, no MFMA.  Lanes run across columns: C1 a multiple of 4 -> 16-byte
// accesses (V = 4; pitches must be multiples of 4 and the arrays 16-byte aligned), any other C1 -> 4-byte accesses (V = 1).  The
// width follows from C1 alone, so the summation orders below never depend on where a buffer happens to lie.
// Same bits on every run: no floating-point atomics.  gP sums each source's edges in ascending edge order after a stable sort
// (p2w_runsum.h, the scheme of p2w_interp_bwd); gWg adds fixed chunks of P2W_EDGE_CHUNK edges and then the chunks in order.
// H1 also comes in float16 and bfloat16 (p2w_edge_l1_io; TH = gr_half or gr_bf16, p2w_runsum.h): the arithmetic is the fp32 kernel's,
// the store rounds once.  The backward of that route (p2w_edge_l1_bwd_io) is not given H1: a stored 16-bit zero may stand for an fp32
// h in (0, 2^-25], so the mask is not read back, it is recomputed - edge_h1 below is the forward's statement sequence, called by the
// forward and by both backward kernels, and without contraction the same statements give the same bits.  gH is read in its dtype.
#include "p2w_runsum.h"

namespace {

// H1 of edge (j -> .) at columns c .. c + V, in fp32: P[j, c..] plus the four geometry terms in this order, each product and each
// sum rounded on its own, then the ReLU.  j < 0 (a source outside [0, n_src)): 0.  The ReLU mask of the backward is h > 0.
template <int V>
__device__ __forceinline__ void edge_h1(const float* __restrict__ P, int ldp, int j, int c, float gx, float gy, float gz, float gw,
                                        const float (&w0)[V], const float (&w1)[V], const float (&w2)[V], const float (&w3)[V], float (&h)[V]) {
#pragma unroll
    for (int u = 0; u < V; ++u) h[u] = 0.f;
    if (j >= 0) {
        gr_ld<V>(&P[(size_t)j * ldp + c], h);
#pragma unroll
        for (int u = 0; u < V; ++u) {
            h[u] = h[u] + gx * w0[u];
            h[u] = h[u] + gy * w1[u];
            h[u] = h[u] + gz * w2[u];
            h[u] = h[u] + gw * w3[u];
            h[u] = fmaxf(h[u], 0.f);
        }
    }
}

// One wave per target, two passes over its edges: the largest |rel|, then geo and H1.  In pass 2 the wave takes 64 edges at a
// time: lane l computes and writes geo of edge k0 + l (coalesced), then the wave walks those edges R = 64 / W at a time, W =
// lanes per row, with the edge's source and geo taken from the lane that holds them.  ptr is clamped to [0, E] and a source
// outside [0, n_src) gives geo = 0 and H1 = 0, so no bad index reaches an address.  TH = H1's element type.
template <int V, class TH>
__global__ __launch_bounds__(256) void edge_l1_kernel(const float* __restrict__ P, int ldp, const float4* __restrict__ rec_src,
                                                      const float4* __restrict__ rec_dst, const int* __restrict__ ptr,
                                                      const int* __restrict__ src, const float* __restrict__ Wg, int M, int E, int n_src,
                                                      int C1, int W, float4* __restrict__ geo, TH* __restrict__ H1, int ldh) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= M) return;
    const int s = max(0, min(ptr[t], E)), e = max(s, min(ptr[t + 1], E));
    if (e <= s) return;
    const float4 pi = rec_dst[t];
    float mx = 0.f;
    for (int k = s + lane; k < e; k += 64) {
        const int j = src[k];
        if ((unsigned)j < (unsigned)n_src) {
            const float4 pj = rec_src[j];
            mx = fmaxf(mx, sqrtf(p2w_d2(pj.x, pj.y, pj.z, pi.x, pi.y, pi.z)));
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) mx = fmaxf(mx, __shfl_xor(mx, off));
    const float den = mx + 1e-8f;
    const int cl = lane & (W - 1), r = lane / W, R = 64 / W;
    for (int k0 = s; k0 < e; k0 += 64) {
        const int k = k0 + lane;
        int j = k < e ? src[k] : -1;
        if ((unsigned)j >= (unsigned)n_src) j = -1;
        float4 g = make_float4(0.f, 0.f, 0.f, 0.f);
        if (j >= 0) {
            const float4 pj = rec_src[j];
            g = make_float4((pj.x - pi.x) / den, (pj.y - pi.y) / den, (pj.z - pi.z) / den, pj.w);
        }
        if (k < e) geo[k] = g;
        const int rows = min(64, e - k0);
        for (int c0 = 0; c0 < C1; c0 += 64 * V) {           // (W < 64: one pass; W = 64: one pass per 64 V columns)
            const int c = c0 + cl * V;
            const bool on = c < C1;                         // (the lanes past the row stay in the loop: they hold edges the others read)
            float w0[V], w1[V], w2[V], w3[V];
            if (on) { gr_ld<V>(&Wg[c], w0); gr_ld<V>(&Wg[C1 + c], w1); gr_ld<V>(&Wg[2 * C1 + c], w2); gr_ld<V>(&Wg[3 * C1 + c], w3); }
            for (int q0 = 0; q0 < rows; q0 += R) {
                const int q = q0 + r;                       // < 64
                const int jq = __shfl(j, q);
                const float gx = __shfl(g.x, q), gy = __shfl(g.y, q), gz = __shfl(g.z, q), gw = __shfl(g.w, q);
                if (on && q < rows) {
                    float h[V];
                    edge_h1<V>(P, ldp, jq, c, gx, gy, gz, gw, w0, w1, w2, w3, h);
                    gr_st<V>(&H1[(size_t)(k0 + q) * ldh + c], h);
                }
            }
        }
    }
}

// sort keys of the transposition by source: the source, n_src for an index outside [0, n_src) (such an edge enters no sum)
__global__ __launch_bounds__(256) void edge_keys_kernel(const int* __restrict__ src, int E, int n_src, unsigned long long* __restrict__ keys) {
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= E) return;
    const int j = src[e];
    keys[e] = (unsigned)j < (unsigned)n_src ? (unsigned long long)j : (unsigned long long)n_src;
}

// The ReLU mask of edge e at columns c .. c + V.  MaskH1: read from the fp32 H1 the forward left (p2w_edge_l1_bwd).
struct MaskH1 {
    const float* H1; int ldh;
    template <int V> __device__ __forceinline__ void operator()(int e, int c, bool (&m)[V]) const {
        float h[V];
        gr_ld<V>(&H1[(size_t)e * ldh + c], h);
#pragma unroll
        for (int u = 0; u < V; ++u) m[u] = h[u] > 0.f;
    }
};
// MaskRe: recomputed from P, geo, src and Wg with the forward's own statements (p2w_edge_l1_bwd_io) - the fp32 H1's mask bit for
// bit, whatever the stored H1 was rounded to.  A source outside [0, n_src): false, the forward wrote 0 there.
struct MaskRe {
    const float* P; int ldp; const float4* geo; const int* src; const float* Wg; int n_src, C1;
    template <int V> __device__ __forceinline__ void operator()(int e, int c, bool (&m)[V]) const {
        int j = src[e];
        if ((unsigned)j >= (unsigned)n_src) j = -1;
        const float4 g = geo[e];
        float w0[V], w1[V], w2[V], w3[V], h[V];
        gr_ld<V>(&Wg[c], w0); gr_ld<V>(&Wg[C1 + c], w1); gr_ld<V>(&Wg[2 * C1 + c], w2); gr_ld<V>(&Wg[3 * C1 + c], w3);
        edge_h1<V>(P, ldp, j, c, g.x, g.y, g.z, g.w, w0, w1, w2, w3, h);
#pragma unroll
        for (int u = 0; u < V; ++u) m[u] = h[u] > 0.f;
    }
};

// an edge's term of the run sums: gZ = gH (TG: fp32, float16 or bfloat16, widened exactly) where the forward's H1 is positive
template <int V, class TG, class Mask>
struct EdgeGzTerm {
    const TG* gH; int ldg; Mask mask;
    __device__ __forceinline__ void operator()(int e, int c, float (&t)[V]) const {
        float g[V];
        bool m[V];
        gr_ld<V>(&gH[(size_t)e * ldg + c], g);
        mask.template operator()<V>(e, c, m);
#pragma unroll
        for (int u = 0; u < V; ++u) t[u] = m[u] ? g[u] : 0.f;
    }
};

// gR[s] = sum_c gP[s, c] Wg[3, c] (= the sum over the source's edges of gZ_e . Wg[3, :]): one wave per source, lane l adds columns
// l, l + 64, ... in ascending order, the lanes are added in a fixed butterfly
__global__ __launch_bounds__(256) void edge_refl_kernel(const float* __restrict__ gP, int ldgp, int C1, const float* __restrict__ w3, int n_src,
                                                        float* __restrict__ gR) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n_src) return;
    float acc = 0.f;
    for (int c = lane; c < C1; c += 64) acc = acc + gP[(size_t)row * ldgp + c] * w3[c];
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) acc = acc + __shfl_xor(acc, off);
    if (lane == 0) gR[row] = acc;
}

// gWg, first launch: one block per (chunk of P2W_EDGE_CHUNK edges, 64 V columns).  The block's P = 256 / W row lanes take edges
// p, p + P, ... of the chunk in ascending order; the row lanes are added in a binary tree in LDS, one geometry column at a time.
template <int V, class TG, class Mask>
__global__ __launch_bounds__(256) void edge_gwg_part_kernel(const TG* __restrict__ gH, int ldg, Mask mask, const float4* __restrict__ geo, int E,
                                                            int C1, int W, float* __restrict__ part) {
    __shared__ __attribute__((aligned(16))) float sm[256 * V];
    const int cl = threadIdx.x & (W - 1), p = threadIdx.x / W, P = 256 / W;
    const int c = blockIdx.y * 64 * V + cl * V;
    const int e0 = blockIdx.x * P2W_EDGE_CHUNK, e1 = min(E, e0 + P2W_EDGE_CHUNK);
    float acc[4][V];
#pragma unroll
    for (int d = 0; d < 4; ++d)
#pragma unroll
        for (int u = 0; u < V; ++u) acc[d][u] = 0.f;
    if (c < C1) {
#pragma unroll 2
        for (int e = e0 + p; e < e1; e += P) {
            float g[V];
            bool m[V];
            gr_ld<V>(&gH[(size_t)e * ldg + c], g);
            mask.template operator()<V>(e, c, m);
            const float4 ge = geo[e];
#pragma unroll
            for (int u = 0; u < V; ++u) {
                const float z = m[u] ? g[u] : 0.f;
                acc[0][u] = acc[0][u] + ge.x * z;
                acc[1][u] = acc[1][u] + ge.y * z;
                acc[2][u] = acc[2][u] + ge.z * z;
                acc[3][u] = acc[3][u] + ge.w * z;
            }
        }
    }
#pragma unroll
    for (int d = 0; d < 4; ++d) {
        for (int h = P >> 1; h >= 1; h >>= 1) {
            gr_st<V>(&sm[threadIdx.x * V], acc[d]);
            __syncthreads();
            if (p < h) {
                float t[V];
                gr_ld<V>(&sm[(threadIdx.x + h * W) * V], t);
#pragma unroll
                for (int u = 0; u < V; ++u) acc[d][u] = acc[d][u] + t[u];
            }
            __syncthreads();
        }
        if (p == 0 && c < C1) gr_st<V>(&part[((size_t)blockIdx.x * 4 + d) * C1 + c], acc[d]);
    }
}
// second launch: the chunks in ascending order, one thread per element of gWg
__global__ __launch_bounds__(256) void edge_gwg_sum_kernel(const float* __restrict__ part, int chunks, int n, float* __restrict__ gWg) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    float acc = 0.f;
    for (int ch = 0; ch < chunks; ++ch) acc = acc + part[(size_t)ch * n + i];
    gWg[i] = acc;
}

struct EbWs { unsigned long long *keys_in, *keys_out; int *slot, *start; float *part, *wpart; void* sub; size_t sub_bytes; int Z, chunks; };
inline EbWs eb_carve(P2wArena& a, int E, int n_src, int C1) {
    const size_t n1 = (size_t)(E > 0 ? E : 1);
    const bool v4 = !(C1 & 3);
    EbWs W;
    W.Z = run_pieces(E, n_src);
    W.chunks = p2w_cdiv(E, P2W_EDGE_CHUNK);
    W.keys_in = a.take<unsigned long long>(n1);
    W.keys_out = a.take<unsigned long long>(n1);
    W.slot = a.take<int>(n1);
    W.start = a.take<int>((size_t)n_src + 1);
    W.part = a.take<float>(run_part_floats(W.Z, n_src, v4 ? run_panel<4>() : run_panel<1>()));
    W.wpart = a.take<float>((size_t)W.chunks * 4 * C1);
    const size_t s = p2w_sort_pairs_u64_ws_bytes((int32_t)n1), c = p2w_cell_starts_ws_bytes(n_src);
    W.sub_bytes = P2wArena::up(s > c ? s : c);             // the sort's and the cell table's scratch, in turn
    W.sub = a.raw(W.sub_bytes);
    return W;
}
inline bool eb_sizes_ok(long long a, long long b, int C1) { return C1 > 0 && a >= 0 && b >= 0 && a < 0x7fffffffll && b < 0x7fffffffll; }

// the forward on H1 of element type TH
template <class TH>
int32_t edge_l1_t(const float* P, int32_t ldp, const float* rec_src, const float* rec_dst, const int32_t* ptr, const int32_t* src,
                  const float* Wg, int32_t n_src, int32_t M, int32_t E, int32_t C1, float* geo, TH* H1, int32_t ldh, p2w_stream_t stream) {
    if (!eb_sizes_ok(n_src, M, C1) || E < 0 || ldp < C1 || ldh < C1 || (M == 0 && E != 0) || (n_src == 0 && E != 0)) return P2W_EINVAL;
    if (M == 0 || E == 0) return P2W_OK;
    P2W_CHECK_PTR(P); P2W_CHECK_PTR(rec_src); P2W_CHECK_PTR(rec_dst); P2W_CHECK_PTR(ptr); P2W_CHECK_PTR(src); P2W_CHECK_PTR(Wg);
    P2W_CHECK_PTR(geo); P2W_CHECK_PTR(H1);
    P2W_CHECK_ALIGN16(rec_src); P2W_CHECK_ALIGN16(rec_dst); P2W_CHECK_ALIGN16(geo);
    const bool v4 = !(C1 & 3);
    if (v4) {
        if ((ldp & 3) || (ldh & 3) || !gr_alv(H1)) return P2W_EALIGN;      // (H1: 16 bytes in fp32, 8 in a 16-bit type)
        P2W_CHECK_ALIGN16(P); P2W_CHECK_ALIGN16(Wg);
    }
    const int blocks = p2w_cdiv(M, 4);
    if (v4) edge_l1_kernel<4, TH><<<blocks, 256, 0, p2w_s(stream)>>>(P, ldp, reinterpret_cast<const float4*>(rec_src), reinterpret_cast<const float4*>(rec_dst),
                                                                     ptr, src, Wg, M, E, n_src, C1, run_row_lanes<4>(C1), reinterpret_cast<float4*>(geo), H1, ldh);
    else edge_l1_kernel<1, TH><<<blocks, 256, 0, p2w_s(stream)>>>(P, ldp, reinterpret_cast<const float4*>(rec_src), reinterpret_cast<const float4*>(rec_dst),
                                                                  ptr, src, Wg, M, E, n_src, C1, run_row_lanes<1>(C1), reinterpret_cast<float4*>(geo), H1, ldh);
    return P2W_LAUNCH_STATUS();
}

// the launches of the backward, after the entry point's guards: gH of element type TG, the ReLU mask from `mask`
template <class TG, class Mask>
int32_t edge_bwd_t(const TG* gH, int32_t ldg, const Mask& mask, const float* geo, const int32_t* src, const float* Wg, int32_t n_src, int32_t E,
                   int32_t C1, float* gP, int32_t ldgp, float* gR, float* gWg, const EbWs& L, p2w_stream_t stream) {
    const bool v4 = !(C1 & 3);
    hipStream_t s = p2w_s(stream);
    unsigned long long *keys_in = L.keys_in, *keys_out = L.keys_out;
    int *slot = L.slot, *start = L.start;
    float *part = L.part, *wpart = L.wpart;
    int32_t st;
    if (n_src > 0) {
        if (E > 0) {
            edge_keys_kernel<<<p2w_cdiv(E, 256), 256, 0, s>>>(src, E, n_src, keys_in);
            st = p2w_sort_pairs_u64(reinterpret_cast<const uint64_t*>(keys_in), reinterpret_cast<uint64_t*>(keys_out), nullptr, slot, E,
                                    L.sub, L.sub_bytes, stream);
            if (st != P2W_OK) return st;
        }
        st = p2w_cell_starts(reinterpret_cast<const uint64_t*>(keys_out), E, n_src, start, L.sub, L.sub_bytes, stream);
        if (st != P2W_OK) return st;
        if (v4) run_sum<4>(EdgeGzTerm<4, TG, Mask>{gH, ldg, mask}, C1, start, slot, n_src, L.Z, part, gP, ldgp, s);
        else run_sum<1>(EdgeGzTerm<1, TG, Mask>{gH, ldg, mask}, C1, start, slot, n_src, L.Z, part, gP, ldgp, s);
        edge_refl_kernel<<<p2w_cdiv(n_src, 4), 256, 0, s>>>(gP, ldgp, C1, Wg + 3 * (size_t)C1, n_src, gR);
    }
    if (L.chunks > 0) {
        const auto* geo4 = reinterpret_cast<const float4*>(geo);
        if (v4) edge_gwg_part_kernel<4, TG, Mask><<<dim3(L.chunks, p2w_cdiv(C1, 256)), 256, 0, s>>>(gH, ldg, mask, geo4, E, C1, run_row_lanes<4>(C1), wpart);
        else edge_gwg_part_kernel<1, TG, Mask><<<dim3(L.chunks, p2w_cdiv(C1, 64)), 256, 0, s>>>(gH, ldg, mask, geo4, E, C1, run_row_lanes<1>(C1), wpart);
    }
    edge_gwg_sum_kernel<<<p2w_cdiv(4 * C1, 256), 256, 0, s>>>(wpart, L.chunks, 4 * C1, gWg);
    return P2W_LAUNCH_STATUS();
}

// p2w_edge_l1_bwd_io on gH of element type TG: H1 is not given, the mask is recomputed (P, geo, src, Wg)
template <class TG>
int32_t edge_bwd_io_t(const TG* gH, int32_t ldg, const float* P, int32_t ldp, const float* geo, const int32_t* src, const float* Wg,
                      int32_t n_src, int32_t E, int32_t C1, float* gP, int32_t ldgp, float* gR, float* gWg, void* ws, size_t ws_bytes,
                      p2w_stream_t stream) {
    if (!eb_sizes_ok(E, n_src, C1) || ldg < C1 || ldp < C1 || ldgp < C1 || (n_src == 0 && E != 0)) return P2W_EINVAL;
    P2W_CHECK_PTR(Wg); P2W_CHECK_PTR(gWg); P2W_CHECK_PTR(ws);
    if (n_src > 0) { P2W_CHECK_PTR(gP); P2W_CHECK_PTR(gR); }
    if (E > 0) { P2W_CHECK_PTR(gH); P2W_CHECK_PTR(P); P2W_CHECK_PTR(geo); P2W_CHECK_PTR(src); }
    P2W_CHECK_ALIGN16(geo); P2W_CHECK_ALIGN16(ws);
    if (!(C1 & 3)) {
        if ((ldg & 3) || (ldp & 3) || (ldgp & 3) || !gr_alv(gH)) return P2W_EALIGN;      // (gH: 16 bytes in fp32, 8 in a 16-bit type)
        P2W_CHECK_ALIGN16(P); P2W_CHECK_ALIGN16(Wg); P2W_CHECK_ALIGN16(gP); P2W_CHECK_ALIGN16(gWg);
    }
    P2wArena arena(ws);
    const EbWs L = eb_carve(arena, E, n_src, C1);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    return edge_bwd_t(gH, ldg, MaskRe{P, ldp, reinterpret_cast<const float4*>(geo), src, Wg, n_src, C1}, geo, src, Wg, n_src, E, C1, gP, ldgp,
                      gR, gWg, L, stream);
}

}  // namespace

// H1 by its dtype code (include/p2w.h: P2W_F32, P2W_F16, P2W_BF16); an unknown code is refused before anything else is looked at
extern "C" int32_t p2w_edge_l1_io(const float* P, int32_t ldp, const float* rec_src, const float* rec_dst, const int32_t* ptr,
                                  const int32_t* src, const float* Wg, int32_t n_src, int32_t M, int32_t E, int32_t C1, float* geo,
                                  void* H1, int32_t th, int32_t ldh, p2w_stream_t stream) {
    if (th == P2W_F32) return edge_l1_t(P, ldp, rec_src, rec_dst, ptr, src, Wg, n_src, M, E, C1, geo, static_cast<float*>(H1), ldh, stream);
    if (th == P2W_F16) return edge_l1_t(P, ldp, rec_src, rec_dst, ptr, src, Wg, n_src, M, E, C1, geo, static_cast<gr_half*>(H1), ldh, stream);
    if (th == P2W_BF16) return edge_l1_t(P, ldp, rec_src, rec_dst, ptr, src, Wg, n_src, M, E, C1, geo, static_cast<gr_bf16*>(H1), ldh, stream);
    return P2W_EUNSUPPORTED;
}

extern "C" int32_t p2w_edge_l1(const float* P, int32_t ldp, const float* rec_src, const float* rec_dst, const int32_t* ptr,
                               const int32_t* src, const float* Wg, int32_t n_src, int32_t M, int32_t E, int32_t C1, float* geo,
                               float* H1, int32_t ldh, p2w_stream_t stream) {
    return p2w_edge_l1_io(P, ldp, rec_src, rec_dst, ptr, src, Wg, n_src, M, E, C1, geo, H1, P2W_F32, ldh, stream);
}

extern "C" size_t p2w_edge_l1_bwd_ws_bytes(int32_t E, int32_t n_src, int32_t C1) {
    if (!eb_sizes_ok(E, n_src, C1)) return 0;
    return p2w_ws_bytes([&](P2wArena& a) { eb_carve(a, E, n_src, C1); });
}

extern "C" int32_t p2w_edge_l1_bwd(const float* gH, int32_t ldg, const float* H1, int32_t ldh, const float* geo, const int32_t* src,
                                   const float* Wg, int32_t n_src, int32_t E, int32_t C1, float* gP, int32_t ldgp, float* gR, float* gWg,
                                   void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (!eb_sizes_ok(E, n_src, C1) || ldg < C1 || ldh < C1 || ldgp < C1 || (n_src == 0 && E != 0)) return P2W_EINVAL;
    P2W_CHECK_PTR(Wg); P2W_CHECK_PTR(gWg); P2W_CHECK_PTR(ws);
    if (n_src > 0) { P2W_CHECK_PTR(gP); P2W_CHECK_PTR(gR); }
    if (E > 0) { P2W_CHECK_PTR(gH); P2W_CHECK_PTR(H1); P2W_CHECK_PTR(geo); P2W_CHECK_PTR(src); }
    P2W_CHECK_ALIGN16(geo); P2W_CHECK_ALIGN16(ws);
    const bool v4 = !(C1 & 3);
    if (v4) {
        if ((ldg & 3) || (ldh & 3) || (ldgp & 3)) return P2W_EALIGN;
        P2W_CHECK_ALIGN16(gH); P2W_CHECK_ALIGN16(H1); P2W_CHECK_ALIGN16(gP); P2W_CHECK_ALIGN16(gWg);
    }
    P2wArena arena(ws);
    const EbWs L = eb_carve(arena, E, n_src, C1);
    if (ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    return edge_bwd_t(gH, ldg, MaskH1{H1, ldh}, geo, src, Wg, n_src, E, C1, gP, ldgp, gR, gWg, L, stream);
}

// gH by its dtype code; the mask recomputed, so H1 is no argument.  An unknown code is refused before anything else is looked at.
extern "C" int32_t p2w_edge_l1_bwd_io(const void* gH, int32_t tg, int32_t ldg, const float* P, int32_t ldp, const float* geo,
                                      const int32_t* src, const float* Wg, int32_t n_src, int32_t E, int32_t C1, float* gP, int32_t ldgp,
                                      float* gR, float* gWg, void* ws, size_t ws_bytes, p2w_stream_t stream) {
    if (tg == P2W_F32)
        return edge_bwd_io_t(static_cast<const float*>(gH), ldg, P, ldp, geo, src, Wg, n_src, E, C1, gP, ldgp, gR, gWg, ws, ws_bytes, stream);
    if (tg == P2W_F16)
        return edge_bwd_io_t(static_cast<const gr_half*>(gH), ldg, P, ldp, geo, src, Wg, n_src, E, C1, gP, ldgp, gR, gWg, ws, ws_bytes, stream);
    if (tg == P2W_BF16)
        return edge_bwd_io_t(static_cast<const gr_bf16*>(gH), ldg, P, ldp, geo, src, Wg, n_src, E, C1, gP, ldgp, gR, gWg, ws, ws_bytes, stream);
    return P2W_EUNSUPPORTED;
}
