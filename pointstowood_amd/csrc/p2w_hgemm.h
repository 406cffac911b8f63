// MFMA fp16/bf16 kernels over "H" activations: the GEMM (+ fused epilogue) and the fused PointNetConv.
// Included by p2w_feat.hip (PREC 0 = f16x3, the parity mode) and p2w_feat_h1.hip (PREC 1 = fp16, 2 = bf16, the
// single-plane throughput modes), which instantiate the templates for their precisions - one translation unit per
// family keeps the instantiations out of each other's register allocation.  gfx950 only.
//
// An H tensor [M, F] is a row-major array of 16-bit planes (include/p2w.h):
//   PREC 0 (f16x3): fp16 hi/lo pairs, value = hi + lo (~22 bits), ldh % 32 == 0; a row is a sequence of blocks of 32
//                   columns, each stored as [hi(32) | lo(32)] = 128 contiguous bytes: column c -> hi at 64*(c/32) + c%32,
//                   lo 32 halfs further (row pitch 2*ldh halfs)
//   PREC 1 / 2    : row m = [v(0..ldh)], fp16 / bf16 (round to nearest), ldh % 64 == 0 (row pitch ldh halfs)
// pad columns are zero.  Weights are packed the same way, one row per output channel: [N_pad][planes * K_pad] of W * 2^e.
// Either way the 64 halfs a GEMM slab consumes of a row are ONE 128-byte cache line.
//
// MFMAs: the GEMM (gemm_hp_kernel) uses v_mfma_f32_16x16x32_{f16,bf16} (layout at h_mfma16 below); the fused PointNetConv
// uses v_mfma_f32_32x32x16_{f16,bf16}: lane l supplies A[row l&31][k = 8*(l>>5) + 0..7] (16 contiguous bytes), B alike;
// C/D: col = l&31, row = (reg&3) + 8*(reg>>2) + 4*(l>>5).
// f16x3 contracts a_lo*w_hi + a_hi*w_lo + a_hi*w_hi (three MFMAs per product, fp32 accumulate); the single-plane modes issue one.
#pragma once
#include "p2w_common.h"
#include <type_traits>

typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef _Float16 h8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf8 __attribute__((ext_vector_type(8)));
typedef __fp16 hpair __attribute__((ext_vector_type(2)));
typedef _Float16 hpairn __attribute__((ext_vector_type(2)));
typedef __bf16 bpair __attribute__((ext_vector_type(2)));
typedef float fpair __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(3))) void* lds_vp;
typedef const __attribute__((address_space(1))) void* glb_vp;

constexpr int H_BK = 32;   // k per plane of a PointNetConv slab
constexpr int SA_EPI_COLS = 1024;   // capacity of the fused PointNetConv's LDS table of per-column epilogue parameters (C2 limit)

template <int PREC> struct HCfg {
    static constexpr int planes = PREC == 0 ? 2 : 1;      // 16-bit planes per H row
    static constexpr int kslab = PREC == 0 ? 32 : 64;     // k consumed per GEMM slab (two LDS planes of 32)
    static constexpr int kalign = PREC == 0 ? 32 : 64;    // ldh / K_pad granularity
};

template <int PREC>
__device__ __forceinline__ f32x16 h_mfma(h8 a, h8 b, f32x16 c) {
    if constexpr (PREC == 2)
        return __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_32x32x16_f16(a, b, c, 0, 0, 0);
}

// The GEMM uses the 16x16x32 shape: lane l supplies A[row l&15][k = 8*(l>>4) + 0..7] (one 16-byte chunk: a whole
// 32-k plane row per instruction), B alike; C/D: col = l&15, row = 4*(l>>4) + reg.  Same FLOPs per cycle as 32x32x16, but
// MI355X holds a higher clock on it (MI355X_MICROARCH.md, DVFS item 7): GEMM class -15 % in a same-box A/B.
typedef float f32x4 __attribute__((ext_vector_type(4)));
template <int PREC>
__device__ __forceinline__ f32x4 h_mfma16(h8 a, h8 b, f32x4 c) {
    if constexpr (PREC == 2)
        return __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf8, a), __builtin_bit_cast(bf8, b), c, 0, 0, 0);
    else
        return __builtin_amdgcn_mfma_f32_16x16x32_f16(a, b, c, 0, 0, 0);
}

// fp16 hi/lo split of two values at once: hi = round-toward-zero fp16 of v (v_cvt_pkrtz_f16_f32 converts a PAIR per
// instruction and, rounding toward zero, saturates at +-65504 instead of overflowing to inf), lo = round-to-nearest
// fp16 of the exact fp32 remainder v - hi (v_cvt_pk_f16_f32, also a pair per instruction; nearest keeps the split
// unbiased).  hi + lo reproduces v to <= 2^-22 relative; |v| up to ~1.3e5 still splits exactly enough.
// 6 VALU per pair (2 packed conversions, 2 conversions back, 2 subtractions) instead of 14 with clamps and single
// conversions.
__device__ __forceinline__ void split_pair(float a, float b, unsigned& hi, unsigned& lo) {
    const hpair h = __builtin_amdgcn_cvt_pkrtz(a, b);
    const fpair rem = {a - (float)h[0], b - (float)h[1]};
    const hpairn l = __builtin_convertvector(rem, hpairn);
    hi = __builtin_bit_cast(unsigned, h);
    lo = __builtin_bit_cast(unsigned, l);
}
// single-plane modes: two values -> one packed word, round to nearest; fp16 saturates at +-65504 instead of inf
template <int PREC>
__device__ __forceinline__ unsigned pack_pair(float a, float b) {
    if constexpr (PREC == 2) {
        const fpair p = {a, b};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(p, bpair));
    } else {
        const fpair p = {__builtin_amdgcn_fmed3f(a, -65504.f, 65504.f), __builtin_amdgcn_fmed3f(b, -65504.f, 65504.f)};
        return __builtin_bit_cast(unsigned, __builtin_convertvector(p, hpairn));
    }
}
// store two adjacent columns (col even) of H row `row`
template <int PREC>
__device__ __forceinline__ void h_store2(_Float16* __restrict__ base, unsigned ldh, unsigned row, unsigned col, float a, float b) {
    if constexpr (PREC == 0) {
        unsigned hw, lw;
        split_pair(a, b, hw, lw);
        _Float16* p = base + (size_t)row * (2 * ldh) + 64 * (col >> 5) + (col & 31);   // block of 32 columns: [hi32 | lo32]
        *reinterpret_cast<unsigned*>(p) = hw;
        *reinterpret_cast<unsigned*>(p + 32) = lw;
    } else {
        *reinterpret_cast<unsigned*>(base + (size_t)row * ldh + col) = pack_pair<PREC>(a, b);
    }
}
// store 4 consecutive columns of one row (col % 4 == 0)
template <int PREC>
__device__ __forceinline__ void h_store4(_Float16* __restrict__ base, int ldh, size_t row, int col, const float (&v)[4]) {
    if constexpr (PREC == 0) {
        uint2 hi, lo;
        split_pair(v[0], v[1], hi.x, lo.x);
        split_pair(v[2], v[3], hi.y, lo.y);
        _Float16* p = base + row * (size_t)(2 * ldh) + 64 * (col >> 5) + (col & 31);
        *reinterpret_cast<uint2*>(p) = hi;
        *reinterpret_cast<uint2*>(p + 32) = lo;
    } else {
        uint2 w;
        w.x = pack_pair<PREC>(v[0], v[1]);
        w.y = pack_pair<PREC>(v[2], v[3]);
        *reinterpret_cast<uint2*>(base + row * (size_t)ldh + col) = w;
    }
}

// XCD-aware tile order: blocks L, L+8, L+16.. share an XCD (round-robin dispatch), i.e. one 4 MiB L2.
//  mode 0 (W fits in L2): an XCD owns whole row tiles and walks their column tiles back to back -> the A row tile is
//          fetched once, W is always an L2 hit.
//  mode 1 (W larger than L2, few rows): an XCD owns a slice of column tiles (its W slice stays L2-resident) and sweeps
//          ALL row tiles; A is streamed once per XCD slice instead of W once per row tile.
__device__ __forceinline__ bool tile_coords_at(int L, int nMt, int nNt, int* mt, int* nt, int mode = 0) {
    const int xcd = L & 7, w = L >> 3;
    if (mode == 0) {
        *mt = xcd + 8 * (w / nNt);
        *nt = w % nNt;
        return *mt < nMt;
    }
    if (nNt >= 8) {
        const int cpx = (nNt + 7) >> 3;     // column tiles per XCD
        *mt = w / cpx;
        *nt = xcd + 8 * (w % cpx);
        return *mt < nMt && *nt < nNt;
    }
    const int r = 8 / nNt;                  // XCDs sharing one column tile (nNt in {1, 2, 4})
    *nt = xcd % nNt;
    *mt = xcd / nNt + r * w;
    return *mt < nMt;
}
__device__ __forceinline__ bool tile_coords(int nMt, int nNt, int* mt, int* nt, int mode = 0) {
    return tile_coords_at(blockIdx.x, nMt, nNt, mt, nt, mode);
}
static inline int tile_grid(int nMt, int nNt, int mode = 0) {
    if (mode == 0) return 8 * ((nMt + 7) / 8) * nNt;
    if (nNt >= 8) return 8 * nMt * ((nNt + 7) / 8);
    const int r = 8 / nNt;
    return 8 * ((nMt + r - 1) / r);
}
static inline int p2w_cu_count() {
    int dev = 0, n = 256;
    if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev);
    return n > 0 ? n : 256;
}

// ------------------------------------------------------------------------------------------------
// epilogues
// ------------------------------------------------------------------------------------------------
constexpr int RI_DEPTH = 2;   // steps of source rows in flight in the interpolated-residual epilogue
struct EpiArgs {
    const float *bias, *sc0, *sh0, *sc1, *sh1, *residual;
    int ldr, relu0, relu1, relu2, relu_final;
    const _Float16* res_h;   // P2W_GEMM_RESIDUAL_H: the residual as an H tensor of the launch's precision (row pitch ldr) instead of fp32
    unsigned* range;         // optional range watch (p2w_epilogue.range)
    const int4* imeta;       // p2w_epilogue.interp: row r's residual = a0 * residual[n0] + a1 * residual[n1] (rows of pitch ldr), {n0, n1, a0, a1} = imeta[r]
};
// The wave's range report: a plain store of 1 into one of the launch's OVER / SEEN words.  Every writer of a word writes the same
// value, so no atomic and no look-before-write is needed (both were tried: an atomic OR behind a look through the vector L1 never
// sees the other CUs' bits and drains the epilogue's stores, +14 us per GEMM launch; a scalar glc look serialises at ~25 ns per
// wave).  A launch's report is P2W_RANGE_SLOTS copies of the word pair, 256 bytes apart, the workgroup picks one by its number:
// thousands of stores to ONE address queue up in one L2 channel (measured: +3.5 us per GEMM launch).
__device__ __forceinline__ void range_commit(unsigned* __restrict__ dst, bool over, bool seen, int lane) {
    if (lane == 0) {
        unsigned* p = dst + (blockIdx.x & (P2W_RANGE_SLOTS - 1)) * 64;
        if (over) p[0] = 1u;
        if (seen) p[1] = 1u;
    }
}
// The watch's running maximum must KEEP a NaN (it is reported as OVER: !(m <= P2W_RANGE_HI)); fmaxf returns the other operand,
// so a NaN beside a number - or behind the running maximum's initial 0 - went unreported.  IEEE-754 maximum: v_maximum3_f32 on
// gfx950, the same instruction count as v_max3_f32.
__device__ __forceinline__ float nan_max(float a, float b) { return __builtin_elementwise_maximum(a, b); }
// ... from a per-lane maximum of |value|
__device__ __forceinline__ void range_commit_max(unsigned* __restrict__ dst, float m, int lane) {
    range_commit(dst, __ballot(!(m <= P2W_RANGE_HI)) != 0ull, __ballot(m > P2W_RANGE_LO) != 0ull, lane);
}
// value of two adjacent columns (col even) of H row `row`: the inverse of h_store2
template <int PREC>
__device__ __forceinline__ fpair h_load2(const _Float16* __restrict__ base, unsigned ldh, unsigned row, unsigned col) {
    if constexpr (PREC == 0) {
        const _Float16* p = base + (size_t)row * (2 * ldh) + 64 * (col >> 5) + (col & 31);
        const hpairn hi = *reinterpret_cast<const hpairn*>(p), lo = *reinterpret_cast<const hpairn*>(p + 32);
        return fpair{(float)hi[0] + (float)lo[0], (float)hi[1] + (float)lo[1]};
    } else if constexpr (PREC == 1) {
        const hpairn v = *reinterpret_cast<const hpairn*>(base + (size_t)row * ldh + col);
        return fpair{(float)v[0], (float)v[1]};
    } else {
        const bpair v = *reinterpret_cast<const bpair*>(base + (size_t)row * ldh + col);
        return fpair{(float)v[0], (float)v[1]};
    }
}
// Outputs of a GEMM launch: optional fp32 [M, ldo] and / or optional H [M, ldh]; or (p2w_gemm_h2_rowdot) neither, but the dot
// product of every output row with dotw[N], left as one partial sum per 64-column slice: part[(col0 / 64) * ldpart + row].
// ldh is the H rows' PITCH (a row may be wider than this launch's output: the producer of a skip connection writes its columns
// straight into the concatenated rows the next layer reads, engine.py); hcols = the columns this launch covers, i.e. its N
// outputs and the zero pad columns up to the next K-slab boundary (<= ldh).
struct OutArgs { float* f32; int ldo; _Float16* h2; int ldh; int hcols; const float* dotw; float* part; int ldpart; };

// sum over the 16 lanes of a DPP row (= the 16 column lanes of a 16 x 16 accumulator tile), the total in every lane: quad
// swaps (1,0,3,2), (2,3,0,1), then the half-row and row mirrors; fp32 addition is commutative, so all lanes agree bit for bit.
// Inline asm with its own wait states: hipcc SLP-packs the FMAs that produce `v` of two neighbouring rows into one
// v_pk_fma_f32 and then allows the DPP read of the pair's FIRST register only the 2 wait states of a plain VALU producer -
// measured on gfx950: that element is sporadically stale in lanes 48..63 (the second one, read a cycle later, never), and
// only when the workgroups of a launch drift apart, i.e. when the SIMD partner does not happen to fill the gap.
__device__ __forceinline__ float row16_sum(float v) {
    asm volatile("s_nop 4\n\t"
                 "v_add_f32_dpp %0, %0, %0 quad_perm:[1,0,3,2] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 1\n\t"
                 "v_add_f32_dpp %0, %0, %0 quad_perm:[2,3,0,1] row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 1\n\t"
                 "v_add_f32_dpp %0, %0, %0 row_half_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 1\n\t"
                 "v_add_f32_dpp %0, %0, %0 row_mirror row_mask:0xf bank_mask:0xf bound_ctrl:1\n\ts_nop 1"
                 : "+v"(v));
    return v;
}

// Column ownership.  The W rows of a stage are staged PERMUTED (w_stage_row16): LDS row 16 t + c of a wave's column range
// holds output channel 32 (t >> 1) + 2 c + (t & 1), so lane c of the 16 x 16 accumulator tiles 2 jq and 2 jq + 1 holds the two
// ADJACENT columns col0 + 32 jq + 2 c and + 1 of rows 16 it + 4 (lane >> 4) + reg: an H word (two fp16) or a float2 per lane
// and row without any cross-lane exchange, per-column parameters as float2 loads.
__device__ __forceinline__ int w_stage_row16(int rho) {
    const int t = rho >> 4, c = rho & 15;
    return 32 * (t >> 1) + 2 * c + (t & 1);
}

// EF >= 0: compile-time flags (1 relu0, 2 sc0, 4 relu1, 8 sc1, 16 relu2, 32 residual, 64 relu_final, 128 fp32 out, 256 H out)
// for interior tiles (every row < M, every column < N, even N / ldo / ldr, 8-byte aligned parameter vectors): no guards,
// float2 parameter / residual / fp32 accesses, the residual of the next row in flight while a row is finished and stored
// (on gfx950 loads and stores retire through one counter: a load waited for right behind its issue drains every store).
// EF < 0: runtime flags, every access guarded (edge tiles, odd sizes); pad columns [N, ldh) of the H rows are written as zeros.
template <int PREC, int RT16, int CT16, int EF, bool DOTK = false>   // DOTK: the row-dot kernel (the plain kernel compiles none of it)
__device__ __forceinline__ void gemm_epilogue_16(const f32x4 (&acc)[RT16][CT16], const EpiArgs& ep, float wscale, int row0, int col0,
                                                 int lane, int M, int N, const OutArgs& o, bool seen_report = true) {
    static_assert(CT16 % 2 == 0, "column tiles come in interleaved pairs");
    constexpr bool GEN = EF < 0;
    constexpr int JQ = CT16 / 2, NSTEP = RT16 * 4;
    const bool R0 = GEN ? ep.relu0 != 0 : (EF & 1) != 0, S0 = GEN ? ep.sc0 != nullptr : (EF & 2) != 0;
    const bool R1 = GEN ? ep.relu1 != 0 : (EF & 4) != 0, S1 = GEN ? ep.sc1 != nullptr : (EF & 8) != 0;
    const bool R2 = GEN ? ep.relu2 != 0 : (EF & 16) != 0;
    const bool RES = !DOTK && (GEN ? (ep.residual != nullptr || ep.res_h != nullptr) : (EF & 32) != 0);   // (the row-dot operator takes no residual)
    const bool RF = GEN ? ep.relu_final != 0 : (EF & 64) != 0, OF = GEN ? o.f32 != nullptr : (EF & 128) != 0;
    const bool OH = GEN ? o.h2 != nullptr : (EF & 256) != 0;
    const bool RH = RES && (GEN ? ep.res_h != nullptr : (EF & 1024) != 0);   // the residual is an H tensor
    // ... or interpolated from the rows of a coarser level (ep.imeta).  Not in the 256 x 256 kernel: it has no register to spare
    constexpr bool RI_OK = !DOTK && RT16 <= 4;
    const bool RI = RI_OK && RES && (GEN ? ep.imeta != nullptr : (EF & 2048) != 0);
    const bool DOT = DOTK && (GEN ? o.dotw != nullptr : (EF & 512) != 0);   // row . dotw partials instead of (or beside) the stores
    const int c16 = lane & 15, kg = lane >> 4;
    const int cb = col0 + 2 * c16;   // even column of pair 0; pair jq: + 32 jq
    fpair bias[JQ], s0[JQ], t0[JQ], s1[JQ], t1[JQ], dw[JQ];
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq) {
        const int c = cb + 32 * jq;
        bias[jq] = fpair{0.f, 0.f}; s0[jq] = fpair{1.f, 1.f}; t0[jq] = fpair{0.f, 0.f}; s1[jq] = fpair{1.f, 1.f}; t1[jq] = fpair{0.f, 0.f};
        dw[jq] = fpair{0.f, 0.f};
        if constexpr (GEN) {
#pragma unroll
            for (int e = 0; e < 2; ++e)
                if (c + e < N) {
                    if (ep.bias) bias[jq][e] = ep.bias[c + e];
                    if (S0) { s0[jq][e] = ep.sc0[c + e]; t0[jq][e] = ep.sh0[c + e]; }
                    if (S1) { s1[jq][e] = ep.sc1[c + e]; t1[jq][e] = ep.sh1[c + e]; }
                    if (DOT) dw[jq][e] = o.dotw[c + e];
                }
        } else {
            if (DOT) dw[jq] = *reinterpret_cast<const fpair*>(o.dotw + c);
            if (ep.bias) bias[jq] = *reinterpret_cast<const fpair*>(ep.bias + c);
            if (S0) { s0[jq] = *reinterpret_cast<const fpair*>(ep.sc0 + c); t0[jq] = *reinterpret_cast<const fpair*>(ep.sh0 + c); }
            if (S1) { s1[jq] = *reinterpret_cast<const fpair*>(ep.sc1 + c); t1[jq] = *reinterpret_cast<const fpair*>(ep.sh1 + c); }
        }
    }
    auto row_of = [&](int st) { return row0 + 16 * (st >> 2) + 4 * kg + (st & 3); };
    auto value = [&](float a, float b, float s0v, float t0v, float s1v, float t1v, float res) {
        float v = fmaf(a, wscale, b);
        if (R0) v = fmaxf(v, 0.f);
        if (S0) v = fmaf(v, s0v, t0v);
        if (R1) v = fmaxf(v, 0.f);
        if (S1) v = fmaf(v, s1v, t1v);
        if (R2) v = fmaxf(v, 0.f);
        if (RES) v += res;
        if (RF) v = fmaxf(v, 0.f);
        return v;
    };
    fpair rcur[JQ], rnxt[JQ];
    // interpolated residual: a ring of RI_D steps' raw source rows (two dependent gathers - record, then the rows it names -
    // each issued ahead of its use: the record of step st + RI_D + 1 and the rows of step st + RI_D during step st; what bounds
    // these launches is gather bytes in flight per CU, not arithmetic)
    constexpr int RI_D = RI_OK ? (RI_DEPTH < NSTEP ? RI_DEPTH : NSTEP) : 1;
    fpair z0r[RI_D][RI_OK ? JQ : 1], z1r[RI_D][RI_OK ? JQ : 1];
    float a0r[RI_D], a1r[RI_D];
    int4 m_nxt = make_int4(0, 0, 0, 0);
    auto load_zrows = [&](int slot, const int4& mt) {
        const float* p0 = ep.residual + ((unsigned)mt.x * (unsigned)ep.ldr + (unsigned)cb);
        const float* p1 = ep.residual + ((unsigned)mt.y * (unsigned)ep.ldr + (unsigned)cb);
#pragma unroll
        for (int jq = 0; jq < (RI_OK ? JQ : 1); ++jq) {
            z0r[slot][jq] = *reinterpret_cast<const fpair*>(p0 + 32 * jq);
            z1r[slot][jq] = *reinterpret_cast<const fpair*>(p1 + 32 * jq);
        }
        a0r[slot] = __int_as_float(mt.z); a1r[slot] = __int_as_float(mt.w);
    };
    auto load_res = [&](fpair (&dst)[JQ], int st) {   // specialised path only
        if (RH) {
#pragma unroll
            for (int jq = 0; jq < JQ; ++jq) dst[jq] = h_load2<PREC>(ep.res_h, (unsigned)ep.ldr, (unsigned)row_of(st), (unsigned)(cb + 32 * jq));
        } else {
            const float* rp = ep.residual + ((unsigned)row_of(st) * (unsigned)ep.ldr + (unsigned)cb);
#pragma unroll
            for (int jq = 0; jq < JQ; ++jq) dst[jq] = *reinterpret_cast<const fpair*>(rp + 32 * jq);
        }
    };
#pragma unroll
    for (int jq = 0; jq < JQ; ++jq) { rcur[jq] = fpair{0.f, 0.f}; rnxt[jq] = fpair{0.f, 0.f}; }
    if constexpr (!GEN) {
        if constexpr (RI_OK) {
            if (RI) {
                int4 m0[RI_D];
#pragma unroll
                for (int d = 0; d < RI_D; ++d) m0[d] = ep.imeta[row_of(d)];
                if (RI_D < NSTEP) m_nxt = ep.imeta[row_of(RI_D)];
#pragma unroll
                for (int d = 0; d < RI_D; ++d) load_zrows(d, m0[d]);
            }
        }
        if (RES && !RI) load_res(rcur, 0);
    }
    float dot4[4] = {0.f, 0.f, 0.f, 0.f};
    // range watch (ep.range): wave-uniform masks in scalar registers - this kernel has no vector register to spare
    unsigned long long r_over = 0ull, r_seen = 0ull;
    float m4 = 0.f;   // ... but for the running maximum of four row steps
#pragma unroll
    for (int st = 0; st < NSTEP; ++st) {
        const int it = st >> 2, reg = st & 3;
        const int row = row_of(st);
        if constexpr (!GEN) {
            if constexpr (RI_OK) {
                if (RI) {
#pragma unroll
                    for (int jq = 0; jq < JQ; ++jq)
                        rcur[jq] = fpair{fmaf(a1r[st % RI_D], z1r[st % RI_D][jq][0], a0r[st % RI_D] * z0r[st % RI_D][jq][0]),
                                         fmaf(a1r[st % RI_D], z1r[st % RI_D][jq][1], a0r[st % RI_D] * z0r[st % RI_D][jq][1])};
                    if (st + RI_D < NSTEP) {
                        load_zrows(st % RI_D, m_nxt);
                        if (st + RI_D + 1 < NSTEP) m_nxt = ep.imeta[row_of(st + RI_D + 1)];
                    }
                }
            }
            if (RES && !RI && st + 1 < NSTEP) load_res(rnxt, st + 1);
            __builtin_amdgcn_sched_barrier(0);
            float* fp = OF ? o.f32 + ((unsigned)row * (unsigned)o.ldo + (unsigned)cb) : nullptr;
            _Float16* hp = nullptr;
            if (OH) {
                if constexpr (PREC == 0) hp = o.h2 + ((unsigned)row * (unsigned)(2 * o.ldh) + (unsigned)(64 * (cb >> 5) + (cb & 31)));
                else hp = o.h2 + ((unsigned)row * (unsigned)o.ldh + (unsigned)cb);
            }
            float dsum = 0.f;
#pragma unroll
            for (int jq = 0; jq < JQ; ++jq) {
                const float va = value(acc[it][2 * jq][reg], bias[jq][0], s0[jq][0], t0[jq][0], s1[jq][0], t1[jq][0], rcur[jq][0]);
                const float vb = value(acc[it][2 * jq + 1][reg], bias[jq][1], s0[jq][1], t0[jq][1], s1[jq][1], t1[jq][1], rcur[jq][1]);
                m4 = nan_max(nan_max(m4, fabsf(va)), fabsf(vb));     // (one v_maximum3 per column pair)
                if (DOT) dsum = fmaf(vb, dw[jq][1], fmaf(va, dw[jq][0], dsum));
                if (OF) *reinterpret_cast<fpair*>(fp + 32 * jq) = fpair{va, vb};
                if (OH) {
                    if constexpr (PREC == 0) {
                        unsigned hw, lw;
                        split_pair(va, vb, hw, lw);
                        *reinterpret_cast<unsigned*>(hp + 64 * jq) = hw;        // 32 columns further = the next [hi32 | lo32] block
                        *reinterpret_cast<unsigned*>(hp + 64 * jq + 32) = lw;
                    } else {
                        *reinterpret_cast<unsigned*>(hp + 32 * jq) = pack_pair<PREC>(va, vb);
                    }
                }
            }
            if (reg == 3) {   // the maximum of four row steps goes into the scalar masks: two compares per 4 x JQ column pairs
                r_over |= __ballot(!(m4 <= P2W_RANGE_HI));
                r_seen |= __ballot(m4 > P2W_RANGE_LO);
                m4 = 0.f;
            }
            if (DOT) {   // the four rows of a lane (reg 0..3) are consecutive: one 16-byte store per row tile by the lanes of column 0
                dot4[reg] = row16_sum(dsum);
                if (reg == 3 && c16 == 0)
                    *reinterpret_cast<float4*>(o.part + ((unsigned)(col0 >> 6) * (unsigned)o.ldpart + (unsigned)(row - 3))) =
                        make_float4(dot4[0], dot4[1], dot4[2], dot4[3]);
            }
            if (RES && !RI) {
#pragma unroll
                for (int jq = 0; jq < JQ; ++jq) rcur[jq] = rnxt[jq];
            }
        } else {
            float dsum = 0.f;
            if (row < M) {
                int4 mt = make_int4(0, 0, 0, 0);
                if constexpr (RI_OK) {
                    if (RI) mt = ep.imeta[row];
                }
#pragma unroll
                for (int jq = 0; jq < JQ; ++jq) {
                    const int c = cb + 32 * jq;
                    float v[2];
#pragma unroll
                    for (int e = 0; e < 2; ++e) {
                        const bool cv = c + e < N;
                        float res = 0.f;
                        if (RI && cv) res = fmaf(__int_as_float(mt.w), ep.residual[(size_t)mt.y * ep.ldr + c + e], __int_as_float(mt.z) * ep.residual[(size_t)mt.x * ep.ldr + c + e]);
                        else if (RES && cv) res = RH ? h_load2<PREC>(ep.res_h, (unsigned)ep.ldr, (unsigned)row, (unsigned)c)[e] : ep.residual[(size_t)row * ep.ldr + c + e];
                        v[e] = value(acc[it][2 * jq + e][reg], bias[jq][e], s0[jq][e], t0[jq][e], s1[jq][e], t1[jq][e], res);
                        if (!cv) v[e] = 0.f;                       // pad columns of an H row must be zero
                        if (OF && cv) o.f32[(size_t)row * o.ldo + c + e] = v[e];
                    }
                    {
                        const float m2 = nan_max(fabsf(v[0]), fabsf(v[1]));
                        r_over |= __ballot(!(m2 <= P2W_RANGE_HI));
                        r_seen |= __ballot(m2 > P2W_RANGE_LO);
                    }
                    if (DOT) dsum = fmaf(v[1], dw[jq][1], fmaf(v[0], dw[jq][0], dsum));
                    if (OH && c < o.hcols) h_store2<PREC>(o.h2, o.ldh, row, c, v[0], v[1]);
                }
            }
            if (DOT) {   // (the 16 lanes of a DPP row share `row`, so they are in or out together)
                dsum = row16_sum(dsum);
                if (row < M && c16 == 0 && col0 < N) o.part[(size_t)(col0 >> 6) * o.ldpart + row] = dsum;   // (slices past N have no slot)
            }
        }
    }
    // (wave-uniform branch.  OVER is reported by every tile; SEEN - "the tensor has values of ordinary size", true of nearly every
    // wave - only where the caller asks for it: a persistent workgroup's FIRST tile.  The report stores were the watch's whole
    // cost: 8 000 of them per launch +0.1 ms on the class, the tracking and the compares nothing)
    if (ep.range) range_commit(ep.range, r_over != 0ull, seen_report && r_seen != 0ull, lane);
}

// s_waitcnt immediate of gfx9: vmcnt[3:0] | expcnt << 4 | lgkmcnt << 8 | vmcnt[5:4] << 14 (expcnt / lgkmcnt left at their maxima)
constexpr int p2w_vmcnt_imm(int n) { return (n & 15) | (7 << 4) | (15 << 8) | ((n >> 4) << 14); }

// WAIT_OLDER (persistent kernel): behind the epilogue, wait until everything this wave issued BEFORE the epilogue has
// retired (the next tile's first-slab DMA) without waiting for the epilogue's own stores: loads, stores and LDS-DMA retire
// in order through one counter, so "at most n outstanding" with n = the number of stores the epilogue just issued (capped at
// the counter's 63) is exactly that.  The wait sits here, in the branch that knows n at compile time, through the builtin:
// the compiler's scoreboard then knows on every path that no load is pending (the guarded path drains completely).
template <int PREC, int RT16, int CT16, bool WAIT_OLDER = false, bool DOTK = false>
__device__ __forceinline__ void gemm_epilogue_dispatch16(const f32x4 (&acc)[RT16][CT16], const EpiArgs& ep, float wscale, int row0,
                                                         int col0, int lane, int M, int N, const OutArgs& o, int ef,
                                                         bool seen_report = true) {
    const bool full = (row0 + 16 * RT16 <= M) && (col0 + 16 * CT16 <= N) && ef != 0;
    if (full) {
        if constexpr (DOTK) {   // the row-dot kernel: one specialised class (bias + ReLU, the head: model.py:241-243), the rest generic
            if (ef == 513) {
                gemm_epilogue_16<PREC, RT16, CT16, 513, true>(acc, ep, wscale, row0, col0, lane, M, N, o, seen_report);
                if constexpr (WAIT_OLDER) __builtin_amdgcn_s_waitcnt(p2w_vmcnt_imm(RT16 < 63 ? RT16 : 63));
                return;
            }
        } else
        switch (ef) {
#define P2W_EPI_CASE(E) case E: { \
            gemm_epilogue_16<PREC, RT16, CT16, E>(acc, ep, wscale, row0, col0, lane, M, N, o, seen_report); \
            constexpr int n_st = RT16 * 4 * (CT16 / 2) * (((E) & 128 ? 1 : 0) + ((E) & 256 ? (PREC == 0 ? 2 : 1) : 0)) ; \
            if constexpr (WAIT_OLDER) __builtin_amdgcn_s_waitcnt(p2w_vmcnt_imm(n_st < 63 ? n_st : 63)); \
            return; }
            P2W_EPI_CASE(128) P2W_EPI_CASE(257) P2W_EPI_CASE(263) P2W_EPI_CASE(287) P2W_EPI_CASE(224)
            P2W_EPI_CASE(131) P2W_EPI_CASE(259) P2W_EPI_CASE(387) P2W_EPI_CASE(129)
            // the residual block's last layer: residual + ReLU with fp32 and H outputs (480, residual in fp32: the single-plane
            // modes) / H output, residual read from the H tensor the block's first layer consumed (1376, + fp32 output 1504: f16x3)
            P2W_EPI_CASE(480) P2W_EPI_CASE(1376) P2W_EPI_CASE(1504)
#undef P2W_EPI_CASE
            // bias + interpolated residual + ReLU, H output: an FP module's layer 0 on the skip columns, the coarse level's product
            // interpolated in (engine.py fp_hoist).  128 x 128 tile (and the split-K fix-up) only
            case 2400:
                if constexpr (!DOTK && RT16 <= 4) {
                    gemm_epilogue_16<PREC, RT16, CT16, 2400>(acc, ep, wscale, row0, col0, lane, M, N, o, seen_report);
                    constexpr int n_st = RT16 * 4 * (CT16 / 2) * (PREC == 0 ? 2 : 1);
                    if constexpr (WAIT_OLDER) __builtin_amdgcn_s_waitcnt(p2w_vmcnt_imm(n_st < 63 ? n_st : 63));
                    return;
                }
                break;
            default: break;
        }
    }
    gemm_epilogue_16<PREC, RT16, CT16, -1, DOTK>(acc, ep, wscale, row0, col0, lane, M, N, o, seen_report);
    if constexpr (WAIT_OLDER) __builtin_amdgcn_s_waitcnt(p2w_vmcnt_imm(0));
}

// ------------------------------------------------------------------------------------------------
// GEMM over H operands: both operands are 16-bit planes in HBM, so a K-slab is staged with direct-to-LDS loads
// (global_load_lds_dwordx4: no VGPR round trip, no ds_write) into a 2-stage ring; one barrier per slab, the next
// slab's DMA is in flight during the whole MFMA phase of the current one.
// A slab takes 64 halfs = ONE 128-byte cache line of every A / W row (f16x3: [hi(32 k) | lo(32 k)]; single-plane: 64 k),
// stored as a 128-byte LDS row of 8 chunks with an XOR swizzle: conflict-free ds_read_b128 fragments, and the image, the
// DMA pattern and the fragment reads are the same in every precision - only the MFMA pairing differs.  W rows are staged
// permuted (w_stage_row16) so that a lane owns adjacent output columns.
// Out-of-range A rows are clamped to M-1 (their results are never stored); K padding is zero in both operands.
// LDS image of a stage: rows of 128 B = 8 chunks of 16 B, A rows 0..BM-1 then B rows.  Chunk c of a row (c>>2 = plane:
// hi / lo, or the k half of a single-plane slab; c&3 = 8 k each) is stored at chunk position c ^ ((row >> 1) & 7), so a
// ds_read_b128 of one chunk index by 16 different rows spreads over all 16 slots of the 256-byte bank row: conflict-free.
// A DMA piece (one wave-instruction, 1 KiB) = 8 image rows: lane L -> row 8g + (L >> 3), stored chunk L & 7, reading the
// source chunk (L & 7) ^ swizzle: 8 rows x 128 contiguous bytes = 8 whole cache lines per piece.
// DMA issue.  A piece's source is a scalar base + a 32-bit lane offset (the saddr form of global_load_lds: see "DMA sources"
// in gemm_hp_body), so a piece costs scalar instructions only and the sources hold two vector registers, not 2 NI.
// 8-wave tiles (HALF): waves 0..3 issue the whole stage behind the barrier while waves 4..7 - their SIMD
// partners, which the hardware's oldest-first arbitration makes the losers of every slab (in-kernel stamps: wave 0 waits
// 39 % of the loop at the barrier, wave 4 4 %) - start on the MFMAs at once: the issue time of one half is the other half's
// uncontested MFMA time.  What bounds a slab is therefore waves 4..7, which run the slab's tail alone on their SIMDs: their A
// fragment reads are issued a row tile ahead (below) so that no LDS latency stands in the open there.  That is worth 1 - 2 %
// on the long-K 256 x 256 launches and nothing a step-level A/B can tell from noise; launches of one to four slabs per tile
// measured up to 5 % slower than with per-lane pointers on one box and the same on another (docs/LAB_NOTES.md).  A static
// s_setprio 1 for waves 4..7 on top measured nothing.
// 4-wave tiles: every wave spreads its pieces over the first half of the slab's MFMAs instead of
// issuing them as one burst behind the barrier: a piece costs ~60-180 issue cycles, and with every wave of the workgroup
// re-aligned by the barrier a burst leaves all four MFMA pipes idle for ~1000 cycles of a ~3000-cycle slab.
//
// gemm_hp_kernel runs it on PERSISTENT workgroups.  Workgroup b walks the virtual blocks b, b + gridDim, ... of the XCD-aware tile
// order (gridDim is a multiple of 8, so a workgroup stays on its XCD's tiles), and the K slabs of consecutive tiles form
// one software pipeline: the first slab of the next tile is issued at the top of the last slab of the current one, so it
// lands during that slab's MFMAs and the epilogue.  A workgroup per tile paid the first slab's whole latency (~2 us) and a
// workgroup launch for every tile - 3 % of a 64-slab tile, 25 % of the 4-slab tiles of the expand layers.
// The epilogue's stores must not be waited for at the next tile's first barrier (loads, stores and LDS-DMA retire through
// ONE in-order counter on gfx950): that barrier waits with a COUNTED vmcnt - the DMA is older than every store of the
// epilogue, so "at most n outstanding" with n <= the number of stores behind it means the DMA has landed.
// ------------------------------------------------------------------------------------------------
// SK = the split-K tail form (gemm_hp_sk_kernel below): a workgroup runs ONE piece - the K slabs [j nslab / S, (j + 1) nslab / S)
// of one tile of a (tail) row range - and leaves it as RAW fp32 accumulators in `skws`; gemm_hp_skfix_kernel adds a tile's S
// pieces in a fixed order and runs the epilogue.  Same stage image, DMA, fragment reads and MFMAs.  Pieces are numbered
// split-major (piece = j * tiles + tile) and dealt to the XCDs in contiguous blocks, so the workgroups that share an L2 run
// neighbouring tiles over the SAME K range side by side: a slab of A or W fetched by one is an L2 hit for the others (pieces of
// one tile side by side - the stream-K order - share nothing: measured fabric-bound at 2.2 us per slab instead of 1.1).
// `nvb` carries the tile count, `sk_S` the split count S (0 in the other kernels).
template <int PREC, int WR, int WC, int RT, int CT, bool DOTK, bool SK>
__device__ __forceinline__ void gemm_hp_body(const _Float16* __restrict__ A, int ldh_a, const _Float16* __restrict__ Wh, float wscale,
                                             int M, int N, int Kpad, int nMt, int nNt, int nvb, const EpiArgs& ep, const OutArgs& o,
                                             int ef, int tmode, int sk_S, float* __restrict__ skws) {
    constexpr int KS = HCfg<PREC>::kslab;
    constexpr int BM = 32 * RT * WR, BN = 32 * CT * WC, NW = WR * WC;
    constexpr int A_CH = 8 * BM, STAGE_CH = A_CH + 8 * BN;
    constexpr bool HALF = NW == 8;                        // 8-wave tile: waves 0..3 issue the whole stage (DMA issue above)
    constexpr int NWI = HALF ? NW / 2 : NW;
    constexpr int NI = STAGE_CH / 64 / NWI;
    static_assert(STAGE_CH % (64 * NWI) == 0, "stage must split evenly over the issuing waves");
    __shared__ __attribute__((aligned(16))) char S[2 * STAGE_CH * 16];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave / WC, wc = wave % WC;
    const size_t a_pitch = (size_t)HCfg<PREC>::planes * ldh_a, w_pitch = (size_t)HCfg<PREC>::planes * Kpad;
    auto next_tile = [&](int& L, int& mt_, int& nt_) {   // first valid virtual block at or after L (stepping by the grid)
        while (L < nvb) {
            if (tile_coords_at(L, nMt, nNt, &mt_, &nt_, tmode)) return true;
            L += gridDim.x;
        }
        return false;
    };
    const int nslab = Kpad / KS;
    int L = blockIdx.x, mt, nt;
    int sk_s0 = 0, sk_s1 = 0, sk_piece = 0;   // SK: this workgroup's slab range and piece number
    if constexpr (SK) {
        const int P = nvb * sk_S, per_xcd = (P + 7) >> 3;
        const int w = blockIdx.x >> 3;
        sk_piece = (blockIdx.x & 7) * per_xcd + w;
        if (w >= per_xcd || sk_piece >= P) return;
        const int j = sk_piece / nvb, r = sk_piece - j * nvb;
        sk_s0 = (int)((long long)j * nslab / sk_S);
        sk_s1 = (int)((long long)(j + 1) * nslab / sk_S);
        if (sk_s0 >= sk_s1) return;              // (sk_S <= nslab: never; the fix-up skips empty pieces the same way)
        mt = r / nNt; nt = r - mt * nNt;
    } else if (!next_tile(L, mt, nt)) {
        return;
    }

    // DMA sources: a wave-uniform 64-bit byte address per operand (the tile's first row at the K offset of the next slab to
    // issue, in scalar registers) + ONE 32-bit byte offset per lane and operand, computed once per kernel: the piece's row
    // within the tile (the W rows permuted: w_stage_row16) x the pitch + the lane's source chunk.  Piece i of an issuing wave is
    // rows + 8 NWI i of piece 0, for A and for the permuted W rows alike (w_stage_row16(rho + 32) = w_stage_row16(rho) + 32),
    // and the chunk swizzle does not depend on i (8 NWI is a multiple of 16): piece i adds i x 8 NWI x pitch to the scalar
    // base, the K advance of a slab is a scalar add - no vector instruction and no vector register per piece.  (16 per-lane
    // 64-bit pointers held 32 VGPRs and cost two v_lshl_add_u64 per piece.)  The cut last row tile ((mt + 1) BM > M,
    // wave-uniform) clamps its rows to M - 1: see dma_clamped (8-wave tiles) and issue_piece (4-wave tiles).
    constexpr int IA = BM / (8 * NWI);                    // pieces 0 .. IA-1 of an issuing wave are A rows, the rest W rows
    static_assert(BM % (8 * NWI) == 0 && (8 * NWI) % 32 == 0, "pieces of a wave must be whole 32-row steps apart");
    const unsigned a_pitch_b = 2u * (unsigned)a_pitch, w_pitch_b = 2u * (unsigned)w_pitch;   // bytes (the launcher bounds BM x pitch)
    const unsigned a_step = 8u * NWI * a_pitch_b, w_step = 8u * NWI * w_pitch_b;   // (a part of BM x pitch: 32-bit)
    const bool issuer = wave < NWI;                       // wave-uniform
    const int prow = 8 * (wave % NWI) + (lane >> 3);      // row of piece 0 within the operand's rows of the stage
    const unsigned pch = 16u * (unsigned)((lane & 7) ^ ((prow >> 1) & 7));
    const unsigned offA_l = (unsigned)prow * a_pitch_b + pch, offW_l = (unsigned)w_stage_row16(prow) * w_pitch_b + pch;
    unsigned long long a_cur = 0, w_cur = 0;              // wave-uniform byte addresses: tile base + K offset of the next slab to issue
    bool a_edge = false;                                  // the tile's last rows lie beyond M: clamp (their results are never stored)
    int a_rmax = 0;                                       // ... to this row of the tile
    unsigned offA_p[HALF ? 1 : IA] = {};                  // 4-wave tiles: the lane's offset of every A piece (issue_piece)
    auto uniform64 = [](unsigned long long v) {
        return (unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)v) |
               ((unsigned long long)(unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(v >> 32)) << 32);
    };
    auto setup_src = [&](int mt_, int nt_, int k0) {   // DMA sources of a tile from K offset k0 on (LDS image and DMA pieces: see above)
        if (HALF && !issuer) return;                   // (waves 4..7 of an 8-wave tile issue nothing)
        a_cur = uniform64((unsigned long long)(uintptr_t)(A + (size_t)mt_ * BM * a_pitch + k0));
        w_cur = uniform64((unsigned long long)(uintptr_t)(Wh + (size_t)nt_ * BN * w_pitch + k0));
        a_edge = (mt_ + 1) * BM > M;
        a_rmax = M - 1 - mt_ * BM;
        if constexpr (!HALF) {
#pragma unroll
            for (int i = 0; i < IA; ++i) offA_p[i] = (unsigned)min(prow + 8 * NWI * i, a_rmax) * a_pitch_b + pch;
        }
    };
    // The DMA is issued through inline asm: hipcc never emits a COUNTED vmcnt while a global_load_lds it knows about is
    // pending - it drains to vmcnt(0) at the first use of any loaded value and in front of LDS reads it cannot tell apart
    // from the DMA's destination - which would put the epilogue's stores (and the next tile's first slab) on every wait.
    // Hidden from its bookkeeping, the compiler's own waits can only become stricter than needed, never weaker (the
    // counter retires in order); the slab protocol below waits for the DMA by hand.
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_vp)S;
    // s_nop 3: a scalar register written by a VECTOR instruction needs 5 wait states before a memory instruction reads it as
    // its base, and the compiler pads nothing for the instructions inside an asm statement.  The bases are computed by scalar
    // instructions, but the kernel spills scalar registers to VGPR lanes and may reload a base (v_readlane, or the
    // v_readfirstlane of setup_src) directly in front of a piece: s_mov + s_nop 3 are the 5 states, whatever stands before.
    // (It also covers the one state between the write of m0 and the load.)  In dma_clamped the four vector instructions do it.
    auto dma = [&](unsigned off, unsigned long long base, unsigned dst) {
        asm volatile("s_mov_b32 m0, %2\n\ts_nop 3\n\tglobal_load_lds_dwordx4 %0, %1"
                     :: "v"(off), "s"(base), "s"(dst) : "m0", "memory");
    };
    // ... of a cut row tile: the lane's offset from the tile's base, its row clamped, computed inside the statement (as plain
    // C++ the compiler computes it ahead of the branch for every tile and keeps it in registers)
    auto dma_clamped = [&](int row_step, unsigned dst) {
        unsigned off;
        asm volatile("v_add_u32 %0, %1, %2\n\tv_min_i32 %0, %3, %0\n\tv_mul_lo_u32 %0, %0, %4\n\tv_add_u32 %0, %0, %5\n\t"
                     "s_mov_b32 m0, %7\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %0, %6"
                     : "=&v"(off) : "s"(row_step), "v"(prow), "s"(a_rmax), "s"(a_pitch_b), "v"(pch), "s"(a_cur), "s"(dst) : "m0", "memory");
    };
    // The pieces of a stage are issued in ascending order, each from a running scalar address: + one step per piece, two
    // scalar adds (a table of i x step per piece costs more scalar registers than the kernel has left)
    unsigned long long a_run = 0, w_run = 0;
    auto stage_dst = [&](int stage) {   // LDS byte address of the wave's piece 0 in a stage; piece i: + i NWI KiB
        return (unsigned)__builtin_amdgcn_readfirstlane(lds_base + (unsigned)(stage * STAGE_CH + (wave % NWI) * 64) * 16u);
    };
    // 4-wave tiles issue their pieces one by one between the MFMA groups: a branch per piece there would cut the MFMA stream,
    // so they keep one offset per A piece, clamped for every tile alike when the tile is set up (IA <= 4 registers)
    auto issue_piece = [&](int i, unsigned dst0) {
        const unsigned dst = dst0 + (unsigned)(i * NWI * 1024);
        if (i == IA) w_run = w_cur;
        if (i >= IA) { dma(offW_l, w_run, dst); w_run += w_step; }
        else dma(offA_p[HALF ? 0 : i], a_cur, dst);
    };
    auto issue_stage = [&](int stage) {   // a whole stage as one burst: one branch for the cut row tile, not one per piece
        const unsigned dst0 = stage_dst(stage);
        a_run = a_cur; w_run = w_cur;
        if (a_edge) {
#pragma unroll
            for (int i = 0; i < IA; ++i) dma_clamped(8 * NWI * i, dst0 + (unsigned)(i * NWI * 1024));
        } else {
#pragma unroll
            for (int i = 0; i < IA; ++i) { dma(offA_l, a_run, dst0 + (unsigned)(i * NWI * 1024)); a_run += a_step; }
        }
#pragma unroll
        for (int i = IA; i < NI; ++i) { dma(offW_l, w_run, dst0 + (unsigned)(i * NWI * 1024)); w_run += w_step; }
    };
    auto advance_src = [&]() { a_cur += 2 * 64; w_cur += 2 * 64; };   // one slab = 64 halfs of every row, in every precision
    // fragment read offsets (bytes within a stage) of plane 0: lane (row l & 15 of a 16-row tile, k octet l >> 4) reads the
    // chunk of its octet; plane 1 (f16x3: lo; single plane: k 32..63) = ^ 64
    constexpr int RT16 = 2 * RT, CT16 = 2 * CT;
    const int r16 = lane & 15, kg = lane >> 4;
    int offA[RT16], offB[CT16];
#pragma unroll
    for (int t = 0; t < RT16; ++t) {
        const int ra = wr * 32 * RT + 16 * t + r16;
        offA[t] = (ra * 8 + (kg ^ ((ra >> 1) & 7))) * 16;
    }
#pragma unroll
    for (int t = 0; t < CT16; ++t) {
        const int rb = BM + wc * 32 * CT + 16 * t + r16;
        offB[t] = (rb * 8 + (kg ^ ((rb >> 1) & 7))) * 16;
    }
    setup_src(mt, nt, SK ? sk_s0 * 64 : 0);
    if constexpr (HALF) {
        if (issuer) issue_stage(0);
    } else {
        const unsigned dst0 = stage_dst(0);
#pragma unroll
        for (int i = 0; i < NI; ++i) issue_piece(i, dst0);
    }
    advance_src();
    int gs = 0;        // slabs done by this workgroup: stage of the current slab = gs & 1
    bool landed = false;   // the DMA of the slab about to start has been waited for already (behind the previous tile's epilogue)
    f32x4 acc[RT16][CT16];
    h8 ah[2], al[2], bh[CT16], bl[CT16];   // A fragments of two row tiles (the one in use, the one being read), B of all column tiles
    // one slab.  LAST: the slab behind it belongs to the next tile (mtn, ntn) - or, past the last tile, is a replay nobody reads
    auto slab = [&](int s, auto last_c, int mtn, int ntn) {
        constexpr bool LAST = decltype(last_c)::value;
        // s_waitcnt through the builtin (simm16: vmcnt[3:0] | expcnt 7 << 4 | lgkmcnt << 8 | vmcnt[5:4] << 14): unlike an asm
        // statement it also updates the compiler's own scoreboard, so it does not re-wait later for loads that are done
        asm volatile("" ::: "memory");
        if (landed) __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0) only: this slab's DMA was waited for behind the epilogue
        else __builtin_amdgcn_s_waitcnt(0x0070);          // vmcnt(0) lgkmcnt(0)
        landed = false;
        __builtin_amdgcn_s_barrier();   // slab gs has landed for every wave, the other stage is free
        asm volatile("" ::: "memory");
        if constexpr (LAST) setup_src(mtn, ntn, 0);
        constexpr int HR = RT16 / 2;                 // row tiles per half
        constexpr int NG = 2 * HR * CT16;            // tile pairs (MFMA groups) of a slab
        constexpr int GAP = (NG / (2 * NI)) > 0 ? NG / (2 * NI) : 1;
        if constexpr (HALF) {
            if (issuer) issue_stage((gs + 1) & 1);
        }
        const char* st = S + (size_t)(gs & 1) * STAGE_CH * 16;
        const unsigned dst_next = HALF ? 0u : stage_dst((gs + 1) & 1);
        // Fragment reads run one row tile ahead: the A fragments of row tile t + 1 are read into the other (ah, al) set behind
        // the first of the CT16 MFMA groups of row tile t, so their LDS latency lies behind the remaining groups (9 MFMAs in
        // f16x3) instead of behind one MFMA.  The scheduling fences pin that order: left alone, the compiler sinks every read to
        // just in front of its first use.  Top of the slab: what the first MFMAs need (A tile 0, B tile 0) is read first.
        auto read_a = [&](int t) {
            al[t & 1] = *reinterpret_cast<const h8*>(st + (offA[t] ^ 64));
            ah[t & 1] = *reinterpret_cast<const h8*>(st + offA[t]);
        };
        auto read_b = [&](int t) {
            bh[t] = *reinterpret_cast<const h8*>(st + offB[t]);
            bl[t] = *reinterpret_cast<const h8*>(st + (offB[t] ^ 64));
        };
        read_a(0);
        read_b(0);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 1; t < CT16; ++t) read_b(t);
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int t = 0; t < RT16; ++t) {
#pragma unroll
            for (int j = 0; j < CT16; ++j) {
                f32x4& c = acc[t][j];
                if constexpr (PREC == 0) {
                    c = h_mfma16<PREC>(al[t & 1], bh[j], c);
                    c = h_mfma16<PREC>(ah[t & 1], bl[j], c);
                    c = h_mfma16<PREC>(ah[t & 1], bh[j], c);
                } else {
                    c = h_mfma16<PREC>(ah[t & 1], bh[j], c);
                    c = h_mfma16<PREC>(al[t & 1], bl[j], c);
                }
                if (j == 0) {   // (behind the first group: the MFMAs that last read the other set are then past their operand reads)
                    __builtin_amdgcn_sched_barrier(0);
                    if (t + 1 < RT16) read_a(t + 1);
                    __builtin_amdgcn_sched_barrier(0);
                }
                if constexpr (!HALF) {   // 4-wave tile: every wave spreads its pieces over the first half of its MFMAs
                    const int g = t * CT16 + j;
                    if ((g % GAP) == GAP - 1 && g / GAP < NI) {
                        issue_piece(g / GAP, dst_next);
                        __builtin_amdgcn_sched_barrier(0);
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        advance_src();
        ++gs;
    };
    if constexpr (SK) {
#pragma unroll
        for (int i = 0; i < RT16; ++i)
#pragma unroll
            for (int j = 0; j < CT16; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = sk_s0; s + 1 < sk_s1; ++s) slab(s, std::false_type{}, 0, 0);
        slab(sk_s1 - 1, std::true_type{}, mt, nt);   // (behind the last slab: a replay of this tile's slab 0 nobody reads)
        // raw accumulators in register order
        f32x4* dst = reinterpret_cast<f32x4*>(skws) + (size_t)sk_piece * (size_t)(BM * BN / 4) + tid;
#pragma unroll
        for (int i = 0; i < RT16; ++i)
#pragma unroll
            for (int j = 0; j < CT16; ++j) dst[(i * CT16 + j) * (64 * NW)] = acc[i][j];
    } else {
    while (true) {
        int Ln = L + gridDim.x, mtn = mt, ntn = nt;
        const bool more = next_tile(Ln, mtn, ntn);
        if (!more) { mtn = mt; ntn = nt; }
#pragma unroll
        for (int i = 0; i < RT16; ++i)
#pragma unroll
            for (int j = 0; j < CT16; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};
        for (int s = 0; s + 1 < nslab; ++s) slab(s, std::false_type{}, 0, 0);
        slab(nslab - 1, std::true_type{}, mtn, ntn);
        gemm_epilogue_dispatch16<PREC, RT16, CT16, true, DOTK>(acc, ep, wscale, mt * BM + wr * 32 * RT, nt * BN + wc * 32 * CT, lane, M, N, o, ef,
                                                               gs == nslab && wave == 0);   // (range watch: SEEN from wave 0 of the workgroup's first tile)
        landed = true;
        if (!more) break;
        L = Ln; mt = mtn; nt = ntn;
    }
    }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the replayed stage behind the last tile
}

template <int PREC, int WR, int WC, int RT, int CT, bool DOTK = false>
__global__ __launch_bounds__(64 * WR * WC, 2) void gemm_hp_kernel(const _Float16* __restrict__ A, int ldh_a,
                                                               const _Float16* __restrict__ Wh, float wscale, int M, int N,
                                                               int Kpad, int nMt, int nNt, int nvb, EpiArgs ep, OutArgs o, int ef,
                                                               int tmode) {
    gemm_hp_body<PREC, WR, WC, RT, CT, DOTK, false>(A, ldh_a, Wh, wscale, M, N, Kpad, nMt, nNt, nvb, ep, o, ef, tmode, 0, nullptr);
}

// 64 x 128 tiles, three workgroups per CU (4 waves of 32 x 64): for the short-K layers (expand, hoists, the FP modules' skip GEMMs:
// 1 - 8 slabs per tile) whose tiles are half epilogue - more independent workgroups per CU overlap one's stores with another's slabs
template <int PREC>
__global__ __launch_bounds__(256, 3) void gemm_hp64_kernel(const _Float16* __restrict__ A, int ldh_a, const _Float16* __restrict__ Wh,
                                                        float wscale, int M, int N, int Kpad, int nMt, int nNt, int nvb, EpiArgs ep,
                                                        OutArgs o, int ef, int tmode) {
    gemm_hp_body<PREC, 2, 2, 1, 2, false, false>(A, ldh_a, Wh, wscale, M, N, Kpad, nMt, nNt, nvb, ep, o, ef, tmode, 0, nullptr);
}

// Split-K tail (see gemm_hp_body): A = first row of the tail range, M = its rows; tiles are numbered row-major (tile r: row
// tile r / nNt, column tile r % nNt); grid = 8 * ceil(tiles * S / 8) workgroups.
template <int PREC, int WR, int WC, int RT, int CT>
__global__ __launch_bounds__(64 * WR * WC, 2) void gemm_hp_sk_kernel(const _Float16* __restrict__ A, int ldh_a,
                                                                  const _Float16* __restrict__ Wh, int M, int Kpad, int nNt,
                                                                  int tiles, int S, float* __restrict__ skws) {
    const EpiArgs ep = {};
    const OutArgs o = {};
    gemm_hp_body<PREC, WR, WC, RT, CT, false, true>(A, ldh_a, Wh, 1.f, M, 0, Kpad, 0, nNt, tiles, ep, o, 0, 0, S, skws);
}

// The fix-up behind gemm_hp_sk_kernel: RT16 workgroups (of the GEMM's shape) per tail tile, one per 16-row block of every wave's
// rows, add the tile's S pieces in ascending K order - a fixed order: results do not depend on timing - and run the GEMM's
// epilogue on the sums.  (One workgroup per tile walked S x 64 KiB serially: 25 us per launch for 36 tiles x 14 pieces, twice the
// time of the MFMA launch it finishes.)
template <int PREC, int WR, int WC, int RT, int CT>
__global__ __launch_bounds__(64 * WR * WC) void gemm_hp_skfix_kernel(const float* __restrict__ skws, int tiles, int S, int nslab, int nNt,
                                                                      float wscale, int M, int N, EpiArgs ep, OutArgs o, int ef) {
    constexpr int BM = 32 * RT * WR, BN = 32 * CT * WC, NW = WR * WC, RT16 = 2 * RT, CT16 = 2 * CT;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave / WC, wc = wave % WC;
    const int r = blockIdx.x / RT16, i = blockIdx.x - r * RT16;
    f32x4 acc[1][CT16];
#pragma unroll
    for (int j = 0; j < CT16; ++j) acc[0][j] = f32x4{0.f, 0.f, 0.f, 0.f};
    for (int p = 0; p < S; ++p) {
        if ((int)((long long)p * nslab / S) >= (int)((long long)(p + 1) * nslab / S)) continue;   // an empty piece was never written
        const f32x4* src = reinterpret_cast<const f32x4*>(skws) + (size_t)(p * tiles + r) * (size_t)(BM * BN / 4) + tid;
#pragma unroll
        for (int jj = 0; jj < CT16; ++jj) acc[0][jj] += src[(i * CT16 + jj) * (64 * NW)];
    }
    const int mt = r / nNt, nt = r - mt * nNt;
    gemm_epilogue_dispatch16<PREC, 1, CT16, false, false>(acc, ep, wscale, mt * BM + wr * 32 * RT + 16 * i, nt * BN + wc * 32 * CT, lane, M, N, o, ef);
}

// host side of p2w_gemm_h2 for one precision (argument checks that do not depend on it are done by the caller)
template <int PREC>
static int32_t launch_gemm_h(const _Float16* Ah, int32_t ldh_a, const _Float16* Wp, float wscale, int32_t M, int32_t N, int32_t K,
                             const EpiArgs& ep, float* out_f32, int32_t ldo, _Float16* out_h2, int32_t ldh_o, int32_t flags,
                             hipStream_t stream, const float* dotw = nullptr, float* part = nullptr, int32_t ldpart = 0,
                             float* skws = nullptr, size_t skws_bytes = 0, int sk_S = 0) {
    constexpr int KA = HCfg<PREC>::kalign;
    const int Npad = (N + 255) / 256 * 256, Kpad = (K + KA - 1) / KA * KA;
    if (ep.imeta) flags = (flags & ~P2W_GEMM_TILE_256) | P2W_GEMM_TILE_128;   // the interpolated residual lives in the 128 x 128 kernel only
    if ((ldh_a % KA) != 0 || ldh_a < Kpad) return P2W_EINVAL;     // K padding must exist (and be zero) in A as well
    if (out_h2 && (ldh_o & 7)) return P2W_EINVAL;
    // the DMA addresses a tile's rows as a 64-bit tile base + a 32-bit byte offset per lane (gemm_hp_body): the rows of the
    // largest tile must lie within 2 GiB of its first (W's pitch, Kpad, is at most A's)
    if ((size_t)256 * HCfg<PREC>::planes * (size_t)ldh_a * 2 >= ((size_t)1 << 31)) return P2W_EINVAL;
    const int hcols = ldh_o < (N + KA - 1) / KA * KA ? ldh_o : (N + KA - 1) / KA * KA;   // outputs + zero pad to the K-slab boundary
    OutArgs o = {out_f32, ldo, out_h2, ldh_o, hcols, dotw, part, ldpart};
    // 256x256 tiles halve the L2->LDS bytes per MFMA; they need enough tiles to fill the CUs and a wide N:
    // one 256x256 workgroup per CU is worth it when N has no column padding at that width and the tiles fill >= 78 % of
    // whole rounds of the chip, from 3/4 of one round up (per-launch A/B over the network's GEMMs: 207 tiles on
    // 256 CUs still win by 8 %, 340 of 512 or N = 640 padded to 768 lose by 10-25 %)
    const int n_cu = p2w_cu_count();
    auto pick_big = [&](int rows) {
        const long tiles256 = (long)p2w_cdiv(rows, 256) * (Npad / 256);
        const long rounds = (tiles256 + n_cu - 1) / n_cu;
        const bool fills = tiles256 * 100 >= rounds * n_cu * 78;
        bool b = N >= 256 && (N % 256) == 0 && tiles256 * 4 >= 3 * n_cu && fills;
        // (a rule that also took long-K layers with only half a round of 256-tiles to the large tile paid off with one workgroup
        // per tile and 32x32x16 MFMAs; with persistent workgroups on 16x16x32 the small tile wins there: M = 32768, K = 1024,
        // N = 256: 48 vs 68 us; M = 17506, K = 2048, N = 512: 113 vs 130 us)
        if (flags & P2W_GEMM_TILE_256) b = true;
        if (flags & P2W_GEMM_TILE_128) b = false;
        return b;
    };
    const bool big = pick_big(M);
    // Tail plan (needs the caller's workspace).  A launch whose tiles do not fill whole rounds of the chip's workgroup slots pays a
    // whole round for the last, partial one (M = 17506, N = K = 2048: 552 tiles of 256 x 256 = 2.16 rounds on 256 CUs cost 3).
    // With a workspace the rows of the WHOLE rounds run as one launch and the remaining rows as a second one: either plainly (on
    // the tile the rule above picks for so few rows) or as a SPLIT-K tail - 128 x 128 tiles, each tile's K range cut into S pieces
    // that run side by side (gemm_hp_sk_kernel: raw fp32 pieces in the workspace) + a fix-up launch (gemm_hp_skfix_kernel: pieces
    // added in a fixed order, the same epilogue code).  The choice is a cost model over measured slab times - a function of the
    // shape alone, so equal calls give equal bits.
    // The 64 x 128 tile (three workgroups per CU) where per-launch A/Bs over the network's layers say it wins (tools/gemm_launches.py):
    // one or two column tiles (N <= 192: the hoists and the narrow project layer, -10 ... -18 %), and launches of at most two
    // rounds of 128 x 128 tiles whose last round is mostly empty while the smaller tile's is not (the 17 506-row layers of the bench
    // batch's level 3: -10 ... -17 %).  MFMA-heavy layers lose on it (W crosses L2 -> LDS twice as often per product).
    bool t64 = false;
    if (!dotw && sk_S == 0 && !ep.imeta && !(flags & (P2W_GEMM_TILE_128 | P2W_GEMM_TILE_256 | P2W_GEMM_NO_TILE_64))) {
        if (flags & P2W_GEMM_TILE_64) t64 = true;
        else if (K <= 1024 && N <= 192) t64 = true;
        else if (K <= 1024 && !big) {
            const long nNt1 = p2w_cdiv(N, 128), T128 = (long)p2w_cdiv(M, 128) * nNt1, T64 = (long)p2w_cdiv(M, 64) * nNt1;
            const long S128 = 2L * n_cu, S64 = 3L * n_cu;
            const double w128 = (double)((T128 + S128 - 1) / S128 * S128) / (double)T128, w64 = (double)((T64 + S64 - 1) / S64 * S64) / (double)T64;
            t64 = T128 <= 2 * S128 && w128 >= 1.3 * w64;
        }
    }
    if (sk_S == 0 && skws && !dotw && !t64 && !(flags & P2W_GEMM_NO_STREAMK)) {
        const int nslab = Kpad / HCfg<PREC>::kslab;
        // per-slab times (us) of a workgroup, measured (tools/gemm_sk_ab.py, tools/gemm_launches.py): 128 x 128 tile alone on its
        // CU / two per CU, 256 x 256 tile (one per CU)
        const double f = PREC == 0 ? 1.0 : 0.7, ts1 = 0.9 * f, ts2 = 1.65 * f, tsb = 2.25 * f;
        auto t_small = [&](long tiles) { return tiles > n_cu ? ts2 : ts1; };
        // (a round of few 256 x 256 tiles runs far above the full-chip rate - clock and fabric to itself: 40 tiles 0.73 us per slab)
        auto t_big = [&](long tiles) { return tiles >= n_cu ? tsb : (0.75 * f + (tsb - 0.75 * f) * (double)tiles / n_cu); };
        // one launch on a given tile: the whole rounds + the partial one (whose workgroups have their CUs to themselves)
        auto one_launch = [&](bool b, int rows) {
            const long T = b ? (long)p2w_cdiv(rows, 256) * (Npad / 256) : (long)p2w_cdiv(rows, 128) * p2w_cdiv(N, 128);
            const long G = b ? n_cu : 2 * n_cu, qq = T / G, R = T % G;
            return (double)nslab * ((double)qq * (b ? tsb : ts2) + (R ? (b ? t_big(R) : t_small(R)) : 0.0));
        };
        const bool big_ok = N >= 256 && (N % 256) == 0;
        double best_cost = one_launch(big, M);
        int best_mode = 0, best_rows_full = 0, best_S = 0;
        bool best_big = big, sk_big = big, tail_big = false;
        double sk_cost = 1e30;
        int sk_rows_full = 0, sk_S_best = 0;
        const size_t piece_b = (size_t)128 * 128 * 4;
        for (int cand = 0; cand < 2; ++cand) {   // tile of the whole rounds: 256 x 256 (where N allows it), 128 x 128
            const bool b = cand == 0;
            if (b && !(N >= 256 && (N % 256) == 0)) continue;
            if ((flags & P2W_GEMM_TILE_256) && !b) continue;
            if ((flags & P2W_GEMM_TILE_128) && b) continue;
            const int BMm = b ? 256 : 128, G_m = n_cu * (b ? 1 : 2);
            const int nNt_m = b ? Npad / 256 : p2w_cdiv(N, 128), nMt_m = p2w_cdiv(M, BMm);
            const long T = (long)nMt_m * nNt_m, q = T / G_m;
            const int mt_full = (int)((q * G_m) / nNt_m);          // row tiles of the whole rounds
            if ((long)mt_full * nNt_m >= T) continue;               // no partial round
            if (q == 0 && b != big) continue;                       // (nothing but a tail: one candidate is enough)
            const int rows_full = mt_full * BMm, m_t = M - rows_full;
            const double main_t = (double)q * nslab * (b ? tsb : ts2) + (q > 0 ? 4.0 : 0.0);
            const long T_t = (long)p2w_cdiv(m_t, 128) * p2w_cdiv(N, 128);
            if (q > 0) {   // whole rounds + a plain second launch, on the cheaper tile for so few rows
                for (int tb = 0; tb < 2; ++tb) {
                    if (tb == 1 && (!big_ok || (flags & P2W_GEMM_TILE_128))) continue;
                    if (tb == 0 && (flags & P2W_GEMM_TILE_256)) continue;
                    const double c = main_t + one_launch(tb == 1, m_t);
                    if (c < 0.95 * best_cost) { best_cost = c; best_mode = 1; best_rows_full = rows_full; best_big = b; best_S = 0; tail_big = tb == 1; }
                }
            }
            for (int S = 2; S <= nslab && T_t * S <= 2 * n_cu; ++S) {   // ... + a split-K tail
                if ((size_t)(T_t * S) * piece_b > skws_bytes) break;
                const double c = main_t + (double)((nslab + S - 1) / S) * 1.0 * f + 18.0 + (double)(T_t * S) * piece_b * 2.0 / 8.0e6;   // fitted (tools/gemm_sk_ab.py): pieces share
                                                                                       // their L2 (~ the uncontended slab time); two more launches + the fix-up's latency ~ 18 us
                if (c < sk_cost) { sk_cost = c; sk_rows_full = rows_full; sk_big = b; sk_S_best = S; }
            }
        }
        if (sk_S_best > 0 && (sk_cost < 0.9 * best_cost || (flags & P2W_GEMM_STREAMK))) {
            best_mode = 2; best_rows_full = sk_rows_full; best_big = sk_big; best_S = sk_S_best;
        }
        if (best_mode != 0) {
            constexpr int PL = HCfg<PREC>::planes;
            const int fl = (flags & ~(P2W_GEMM_STREAMK | P2W_GEMM_TILE_128 | P2W_GEMM_TILE_256)) | P2W_GEMM_NO_STREAMK;
            const int rows_full = best_rows_full, m_t = M - rows_full;
            if (rows_full > 0) {
                const int32_t rc = launch_gemm_h<PREC>(Ah, ldh_a, Wp, wscale, rows_full, N, K, ep, out_f32, ldo, out_h2, ldh_o,
                                                       fl | (best_big ? P2W_GEMM_TILE_256 : P2W_GEMM_TILE_128), stream);
                if (rc != P2W_OK) return rc;
            }
            const size_t r0 = (size_t)rows_full;
            EpiArgs ept = ep;
            if (ept.imeta) ept.imeta += r0;                       // (the interpolated residual's rows are named by the records)
            else if (ept.residual) ept.residual += r0 * ep.ldr;
            if (ept.res_h) ept.res_h += r0 * PL * ep.ldr;
            return launch_gemm_h<PREC>(Ah + r0 * PL * ldh_a, ldh_a, Wp, wscale, m_t, N, K, ept, out_f32 ? out_f32 + r0 * ldo : nullptr, ldo,
                                       out_h2 ? out_h2 + r0 * PL * ldh_o : nullptr, ldh_o,
                                       best_mode == 2 ? fl : (fl | (tail_big ? P2W_GEMM_TILE_256 : P2W_GEMM_TILE_128)), stream, nullptr, nullptr, 0,
                                       best_mode == 2 ? skws : nullptr, skws_bytes, best_mode == 2 ? best_S : 0);
        }
    }
    // epilogue class for the specialised interior-tile path (0 = generic); needs 32-bit element offsets
    int ef = (ep.relu0 ? 1 : 0) | (ep.sc0 ? 2 : 0) | (ep.relu1 ? 4 : 0) | (ep.sc1 ? 8 : 0) | (ep.relu2 ? 16 : 0) |
             ((ep.residual || ep.res_h) ? 32 : 0) | (ep.relu_final ? 64 : 0) | (out_f32 ? 128 : 0) | (out_h2 ? 256 : 0) | (dotw ? 512 : 0) |
             (ep.res_h ? 1024 : 0) | (ep.imeta ? 2048 : 0);
    const size_t lim = (size_t)1 << 31;
    if ((size_t)M * (size_t)(ldo > 2 * ldh_o ? ldo : 2 * ldh_o) >= lim || ((ep.residual || ep.res_h) && !ep.imeta && (size_t)M * (size_t)ep.ldr * (ep.res_h ? 2 : 1) >= lim) ||
        (N & 1) || (flags & P2W_GEMM_GENERIC_EPI))
        ef = 0;
    // the specialised epilogue moves column PAIRS (float2 / one H word per lane): even pitches, 8-byte aligned vectors
    auto odd8 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 7) != 0; };
    if ((out_f32 && ((ldo & 1) || odd8(out_f32))) || (ep.residual && ((ep.ldr & 1) || odd8(ep.residual))) || odd8(ep.bias) ||
        (ep.res_h && ((ep.ldr & 7) || (reinterpret_cast<uintptr_t>(ep.res_h) & 15))) ||
        odd8(ep.sc0) || odd8(ep.sh0) || odd8(ep.sc1) || odd8(ep.sh1) || odd8(dotw) || (part && ((ldpart & 3) || (reinterpret_cast<uintptr_t>(part) & 15))))
        ef = 0;
    // tile order (see tile_coords): the one that moves fewer bytes over the fabric.  Both orders were timed on every layer of
    // the network: where they differ in time the one with less traffic is the faster one, and on the MFMA-bound layers the
    // time is the same while the traffic differs up to 2.7 x (M = 16384, K = N = 2048: 408 MB against 1117 MB).
    //  rows order:    the wpx workgroups of an XCD run R = wpx / nNt row tiles x all nNt column tiles side by side (they start
    //                 together and their tiles are equally long, so a slab fetched by one is an L2 hit for the others):
    //                 A once; W once per XCD when it stays in L2, else once per R row tiles of every XCD.
    //  columns order: an XCD keeps its column slice of W and streams all of A (nNt >= 8), or 8 / nNt XCDs share a column tile.
    const size_t w_bytes = (size_t)N * Kpad * 2 * HCfg<PREC>::planes, a_bytes = (size_t)M * Kpad * 2 * HCfg<PREC>::planes;
    auto pick_mode = [&](int nNtx, int nMtx, int per_cu) {
        const bool ok = nNtx >= 8 || (nNtx > 0 && 8 % nNtx == 0);
        if (!ok) return 0;
        if (flags & P2W_GEMM_ORDER_ROWS) return 0;
        if (flags & P2W_GEMM_ORDER_COLS) return 1;
        const size_t l2_keep = (size_t)3 * 1024 * 1024;        // what an XCD's 4 MiB L2 keeps beside the streamed operand
        const int wpx = n_cu / 8 * per_cu;                     // workgroups of an XCD in flight
        const int R = wpx / nNtx > 0 ? wpx / nNtx : 1;
        const int rows_px = p2w_cdiv(nMtx, 8), xcds = nMtx < 8 ? nMtx : 8;
        const size_t t_rows = a_bytes * (size_t)p2w_cdiv(nNtx, wpx) + w_bytes * xcds * (w_bytes <= l2_keep ? 1 : p2w_cdiv(rows_px, R));
        size_t t_cols;
        if (nNtx >= 8) {
            const int cpx = p2w_cdiv(nNtx, 8), Rc = wpx / cpx > 0 ? wpx / cpx : 1;
            t_cols = a_bytes * 8 + w_bytes * (w_bytes / 8 <= l2_keep ? 1 : p2w_cdiv(nMtx, Rc));
        } else {
            t_cols = a_bytes * nNtx + w_bytes * 8 / nNtx;
        }
        return t_cols * 10 < t_rows * 9 ? 1 : 0;
    };
    auto pgrid = [&](int nvb, int per_cu) {   // persistent grid: whole XCD rounds, at most per_cu workgroups per CU
        const int cap = n_cu * per_cu;
        int g = nvb < cap ? nvb : cap;
        if (g >= 8) g &= ~7;
        return g;
    };
    if (sk_S > 0) {   // this call IS a split-K tail (planned above)
        const int nslab = Kpad / HCfg<PREC>::kslab, nNt1 = p2w_cdiv(N, 128), T_t = p2w_cdiv(M, 128) * nNt1;
        gemm_hp_sk_kernel<PREC, 2, 2, 2, 2><<<8 * p2w_cdiv(T_t * sk_S, 8), 256, 0, stream>>>(Ah, ldh_a, Wp, M, Kpad, nNt1, T_t, sk_S, skws);
        gemm_hp_skfix_kernel<PREC, 2, 2, 2, 2><<<T_t * 4, 256, 0, stream>>>(skws, T_t, sk_S, nslab, nNt1, wscale, M, N, ep, o, ef);   // (RT16 = 4 row blocks per tile)
    } else if (t64) {
        const int nMt = p2w_cdiv(M, 64), nNt1 = p2w_cdiv(N, 128);
        const int tm = pick_mode(nNt1, nMt, 3), nvb = tile_grid(nMt, nNt1, tm);
        gemm_hp64_kernel<PREC><<<pgrid(nvb, 3), 256, 0, stream>>>(Ah, ldh_a, Wp, wscale, M, N, Kpad, nMt, nNt1, nvb, ep, o, ef, tm);
    } else if (big) {
        const int nMt = p2w_cdiv(M, 256), nNt2 = Npad / 256;
        const int tm = pick_mode(nNt2, nMt, 1), nvb = tile_grid(nMt, nNt2, tm);
        if (dotw) gemm_hp_kernel<PREC, 2, 4, 4, 2, true><<<pgrid(nvb, 1), 512, 0, stream>>>(Ah, ldh_a, Wp, wscale, M, N, Kpad, nMt, nNt2, nvb, ep, o, ef, tm);
        else gemm_hp_kernel<PREC, 2, 4, 4, 2><<<pgrid(nvb, 1), 512, 0, stream>>>(Ah, ldh_a, Wp, wscale, M, N, Kpad, nMt, nNt2, nvb, ep, o, ef, tm);
    } else {
        const int nMt = p2w_cdiv(M, 128), nNt1 = p2w_cdiv(N, 128);
        const int tm = pick_mode(nNt1, nMt, 2), nvb = tile_grid(nMt, nNt1, tm);
        if (dotw) gemm_hp_kernel<PREC, 2, 2, 2, 2, true><<<pgrid(nvb, 2), 256, 0, stream>>>(Ah, ldh_a, Wp, wscale, M, N, Kpad, nMt, nNt1, nvb, ep, o, ef, tm);
        else gemm_hp_kernel<PREC, 2, 2, 2, 2><<<pgrid(nvb, 2), 256, 0, stream>>>(Ah, ldh_a, Wp, wscale, M, N, Kpad, nMt, nNt1, nvb, ep, o, ef, tm);
    }
    return P2W_LAUNCH_STATUS();
}

// ------------------------------------------------------------------------------------------------
// fused PointNetConv over H weights, two kernels:
//  1. sa_edge_meta_kernel (p2w_feat.hip): one thread per (target, slot): source index j and g = (rel/(dmax+1e-8),
//     refl_j) (pointnet.py:119-129) -> meta_j[M*32], meta_g[M*32] (20 B per slot).  The chain of dependent loads
//     (deg -> nbr -> xyzr) is hidden by plain occupancy there instead of stalling a GEMM-shaped workgroup.
//  2. sa_conv16p_kernel: PERSISTENT workgroups (one per CU, 8 waves) walk (row tile, column tile) work items; the
//     K slabs of consecutive items form ONE software pipeline: while slab g runs on the MFMAs, slab g+1's W2 DMA,
//     P-row gather and A production (possibly of the NEXT item) are in flight, and the next item's metadata is
//     prefetched a whole item ahead.  Rows of the GEMM = (target, neighbour slot); a 32-row MFMA tile = one target,
//     so the max over neighbours is a max over the accumulator tile's rows (16 registers + one lane^32 exchange) and
//     the [E, C] edge tensors of the reference never exist in HBM.
// ------------------------------------------------------------------------------------------------
// Tile descriptors.  The metadata pre-pass lays the GEMM's rows out in 32-row MFMA tiles of 32 / G targets with G neighbour
// slots each (G = 32: one target per tile; G = 8: four low-degree targets per tile, see p2w_sa_conv_h's P2W_SA_PACK8) and
// writes one descriptor per target slot group: (target row << 6) | neighbour count, or -1 for an unused group.
template <int RT, int GPT> struct SaEpiRegs { float bias[2], s[2], t[2]; int dsc[RT][GPT]; };
// layer-2 bias + ReLU + BN affine, then max over the target's valid neighbour slots (rows of its group in the MFMA tile).
// bias + ReLU + BN are monotone in the accumulator (wscale > 0: non-decreasing for s >= 0, non-increasing for s < 0) and
// every rounding step keeps (weak) monotonicity, so the maximum over the slots of the transformed values IS the transform
// of the maximum (s >= 0) or minimum (s < 0) of the raw accumulators, bit for bit: 2 VALU per value instead of 5 and
// the transform once per column.
template <int PREC, int RT, int G>   // RT 32-row tiles per wave, G rows (neighbour slots) per target
__device__ __forceinline__ void sa_epilogue_regs(const f32x16 (&acc)[RT][2], float wscale, int n0, int wc, int lane,
                                                 const SaEpiRegs<RT, 32 / G>& e, int C2, float* __restrict__ out, int ldo,
                                                 _Float16* __restrict__ out_h2, int ldh, float& amax) {
    static_assert(G == 32 || G == 8, "one or four targets per 32-row tile");
    constexpr int GPT = 32 / G;
    const int h = lane >> 5;
#pragma unroll
    for (int i = 0; i < RT; ++i) {
#pragma unroll
        for (int q = 0; q < GPT; ++q) {
            const int dsc = __builtin_amdgcn_readfirstlane(e.dsc[i][q]);   // the same for every lane
            if (dsc < 0) continue;
            const int tgt = dsc >> 6, d = dsc & 63;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = n0 + wc * 64 + j * 32 + (lane & 31);
                const bool cv = col < C2;
                const float sgn = e.s[j] < 0.f ? -1.f : 1.f;
                const fpair sg2 = {sgn, sgn};
                float ext;
                if constexpr (G == 32) {
                    if (d >= 32) {   // every slot valid (the kNN levels): packed sign multiply, three-input maxima, no masks
                        fpair p[8];
#pragma unroll
                        for (int u = 0; u < 8; ++u) p[u] = fpair{acc[i][j][2 * u], acc[i][j][2 * u + 1]} * sg2;
                        float m0 = fmaxf(fmaxf(p[0][0], p[0][1]), p[1][0]);
                        float m1 = fmaxf(fmaxf(p[1][1], p[2][0]), p[2][1]);
                        float m2 = fmaxf(fmaxf(p[3][0], p[3][1]), p[4][0]);
                        float m3 = fmaxf(fmaxf(p[4][1], p[5][0]), p[5][1]);
                        m0 = fmaxf(fmaxf(m0, p[6][0]), p[6][1]);
                        m1 = fmaxf(fmaxf(m1, p[7][0]), p[7][1]);
                        ext = fmaxf(fmaxf(m0, m1), fmaxf(m2, m3));
                    } else {
                        ext = -INFINITY;
#pragma unroll
                        for (int r = 0; r < 16; ++r) {
                            const int slot = (r & 3) + 8 * (r >> 2) + 4 * h;
                            if (slot < d) ext = fmaxf(ext, sgn * acc[i][j][r]);
                        }
                    }
                } else {   // rows 8 q .. 8 q + 7 of the tile: registers 4 q .. 4 q + 3 of both half-waves
                    ext = -INFINITY;
#pragma unroll
                    for (int r = 0; r < 4; ++r) {
                        const int slot = r + 4 * h;
                        if (slot < d) ext = fmaxf(ext, sgn * acc[i][j][4 * q + r]);
                    }
                }
                {   // the other half of the group's rows lives in lane ^ 32: one v_permlane32_swap instead of an LDS round trip
                    const auto sw = __builtin_amdgcn_permlane32_swap(__float_as_uint(ext), __float_as_uint(ext), false, false);
                    ext = fmaxf(__uint_as_float(sw[0]), __uint_as_float(sw[1]));
                }
                float vmax = fmaf(fmaxf(fmaf(sgn * ext, wscale, e.bias[j]), 0.f), e.s[j], e.t[j]);
                if (d == 0 || !cv) vmax = 0.f;   // rows without neighbours; pad columns of an H row stay zero
                amax = nan_max(amax, fabsf(vmax));   // (keeps a NaN: range_commit_max reports it as OVER)
                if (cv && h == 0 && out) out[(size_t)tgt * ldo + col] = vmax;
                if (out_h2) {  // lanes (2p, 2p+1) hold adjacent columns: the even lane stores both as one word per plane
                    const float nb = __uint_as_float(__builtin_amdgcn_update_dpp(0, __float_as_uint(vmax), 0xB1, 0xf, 0xf, false));
                    if (h == 0 && (lane & 1) == 0 && col < ldh) h_store2<PREC>(out_h2, ldh, tgt, col, vmax, nb);
                }
            }
        }
    }
}

// <BN, RT>: <256, 2>: 4 targets x 256 columns (waves 2 x 4, wave tile 64 x 64);  <128, 2>: 8 targets x 128 columns (waves 4 x 2)
// (one workgroup per CU either way: LDS).  The A operand is produced on the VALU; in the single-plane modes a slab is
// 32 k of ONE plane (half the LDS image and DMA, one MFMA per tile pair and k step).
// M = number of 32-row tiles (read from tiles_dev when given: the packed pre-pass only knows it on the device); desc: see SaEpiRegs.
template <int PREC, int BN, int RT, int G>
__global__ __launch_bounds__(512, 2) void sa_conv16p_kernel(const float* __restrict__ P, int ldp, const int* __restrict__ meta_j,
                                                            const float4* __restrict__ meta_g, const int* __restrict__ desc,
                                                            const int* __restrict__ tiles_dev, int M, const float* __restrict__ w1r4, int C1, int C1pad,
                                                            const _Float16* __restrict__ W2h, size_t plane, float wscale, int C2,
                                                            int nMt_, int nNt, const float* __restrict__ b2,
                                                            const float* __restrict__ bn_s, const float* __restrict__ bn_t,
                                                            float* __restrict__ out, int ldo, _Float16* __restrict__ out_h2,
                                                            int ldh, unsigned* __restrict__ range) {
    constexpr int NP = HCfg<PREC>::planes;
    constexpr int WCn = BN / 64, BM = 32 * RT * (8 / WCn), NW = 8, NR = BM / 128;   // NR producer rows per thread
    constexpr int GPT = 32 / G;                                                     // targets per 32-row tile
    if (tiles_dev) M = *tiles_dev;
    const int nMt = tiles_dev ? (M + BM / 32 - 1) / (BM / 32) : nMt_;
    if (M <= 0) return;
    constexpr int A_CH = 4 * NP * BM, STAGE_CH = A_CH + 4 * NP * BN;
    // the W2 DMA of a slab is issued by waves 0..3 only: in-kernel stamps show them 26 % of the loop at the barrier while
    // their SIMD partners (waves 4..7, the losers of the oldest-first arbitration) wait 4 % - the same asymmetry as in the GEMM
    constexpr int NWI = 4;
    constexpr int NI = (4 * NP * BN) / 64 / NWI;
    static_assert(NI >= 1, "every issuing wave has at least one W2 DMA piece per slab");
    // ONE __shared__ object: with a second one beside the DMA staging array hipcc cannot tell the LDS-DMA's destination from
    // the other object and drains vmcnt(0) in front of the first ds_read of every slab (cdna_hip_programming.md, .s-level trap a)
    __shared__ __attribute__((aligned(16))) char S[2 * STAGE_CH * 16 + 4 * 512 * 4 + 3 * SA_EPI_COLS * 4];
    float* const Wr = reinterpret_cast<float*>(S + 2 * STAGE_CH * 16);   // layer-1 geometry weights (rx, ry, rz, refl rows), C1pad <= 512
    float* const Ep = Wr + 4 * 512;   // the epilogue's per-column parameters [bias | BN scale | BN shift][C2 <= SA_EPI_COLS]: read when an
                                      // item is finished instead of being prefetched (6 loads + their addresses) in every slab
    const int tid = threadIdx.x, lane = tid & 63;
    for (int i = tid; i < 4 * C1pad; i += 512) Wr[i] = w1r4[i];
    for (int i = tid; i < C2; i += 512) { Ep[i] = b2[i]; Ep[SA_EPI_COLS + i] = bn_s[i]; Ep[2 * SA_EPI_COLS + i] = bn_t[i]; }
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), wr = wave / WCn, wc = wave % WCn;
    const int nitems = nMt * nNt, nslab = C1pad / H_BK;
    // XCD-aware work assignment: workgroups b, b+8, b+16.. share an XCD (round-robin dispatch) and therefore an L2.
    // Each XCD walks ONE contiguous chunk of work items, its workgroups taking consecutive items at every step, so the
    // P rows gathered by an XCD at any time belong to spatially adjacent targets (levels are stored in grid-cell
    // order) and are re-used out of that XCD's L2 instead of being streamed by all eight.
    int first, stride, limit;
    if ((gridDim.x & 7) == 0) {
        const int xcd = blockIdx.x & 7, slot = blockIdx.x >> 3, per = gridDim.x >> 3;
        const int chunk = (nitems + 7) >> 3;
        first = xcd * chunk + slot; stride = per; limit = min((xcd + 1) * chunk, nitems);
    } else {
        first = blockIdx.x; stride = gridDim.x; limit = nitems;
    }
    if (first >= limit) return;
    const int my_items = (limit - first + stride - 1) / stride;
    const int total = my_items * nslab;

    // item -> (row tile, column tile): column tiles of one row tile are adjacent work items.  The division runs once per item
    // (in nxt(), when a slab counter wraps), not in every slab.
    auto item_mt = [&](int it) { return (first + it * stride) / nNt; };
    auto item_nt = [&](int it) { return (first + it * stride) % nNt; };

    // LDS image of a stage.  f16x3: the GEMM kernel's (rows of 128 B = [hi 4 chunks | lo 4 chunks], chunk c stored at
    // c ^ ((row >> 1) & 7), A rows then B rows); single plane: rows of 64 B, chunk q stored at q ^ ((row >> 2) & 3).
    constexpr int RCH = 4 * NP;                                   // 16-byte chunks per image row
    auto img = [](int row, int chunk) { return (row * RCH + (NP == 2 ? (chunk ^ ((row >> 1) & 7)) : (chunk ^ ((row >> 2) & 3)))) * 16; };
    // The A rows (written by the producer's ds_write_b128, not by the DMA) take one more swizzle bit in f16x3: odd rows swap their
    // hi and lo halves.  A ds_write_b128 is served in groups of 8 lanes on 32 banks (one 128-byte image row = one bank row): the
    // group's lanes 0-3 write the 4 hi chunks of row r, lanes 4-7 those of row r + 1 - with the B image's swizzle both land on the
    // same half of the bank row (2-way conflict on every store: SQ_LDS_BANK_CONFLICT 12 - 20 % of the LDS cycles, r5 profiles);
    // with the halves swapped on odd rows they fill one bank row.  The fragment reads (16-lane groups over 64 banks) stay
    // conflict-free: rows {0-3, 12-15, 20-27} of a group still map to 16 distinct 16-byte slots.
    auto imgA = [](int row, int chunk) { return (row * RCH + (NP == 2 ? (chunk ^ ((row >> 1) & 7) ^ ((row & 1) << 2)) : (chunk ^ ((row >> 2) & 3)))) * 16; };
    const int prow = tid >> 2, pq = tid & 3;   // rows prow + 128*u, u < NR (the swizzle term is the same for all of them)
    const int a_dst = imgA(prow, pq);          // hi plane chunk; the lo chunk (f16x3) is at a_dst ^ 64
    // per-lane pieces of the B DMA source that do not depend on the item
    size_t boff[NI];
    int dstc[NI];
    (void)plane;
#pragma unroll
    for (int i = 0; i < NI; ++i) {   // a piece = 1 KiB of the B image: 8 rows x 128 B (f16x3: whole cache lines) / 16 rows x 64 B
        const int g2 = (wave % NWI) + NWI * i;
        const int row = (NP == 2 ? 8 : 16) * g2 + (lane >> (NP == 2 ? 3 : 2));
        const int c = NP == 2 ? ((lane & 7) ^ ((row >> 1) & 7)) : ((lane & 3) ^ ((row >> 2) & 3));
        boff[i] = (size_t)row * (NP * C1pad) + 8 * c;
        dstc[i] = A_CH + g2 * 64;
    }
    constexpr int KADV = NP == 2 ? 2 : 1;   // halfs a 32-k slab advances in a W2 row: 64 (hi + lo interleaved) or 32
    auto issue = [&](int stage, const _Float16* wbase, int k0) {   // wbase = W2h + nt * BN * NP * C1pad (per item); k0 in k units
        if (wave >= NWI) return;
#pragma unroll
        for (int i = 0; i < NI; ++i)
            __builtin_amdgcn_global_load_lds((glb_vp)(wbase + boff[i] + KADV * k0),
                                             (lds_vp)(S + ((size_t)stage * STAGE_CH + dstc[i]) * 16), 16, 0, 0);
    };
    // metadata of the producer's edge row (clamped: rows past the last target replay the last valid row)
    struct Meta { int j[NR]; float4 g[NR]; };
    struct Vals { float4 v[NR][2]; };
    const int last_row = M * 32 - 1;   // < 2^31 (launcher)
    auto load_meta = [&](int mt_, Meta& m) {
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const int row = min(mt_ * BM + prow + 128 * u, last_row);
            m.j[u] = meta_j[row];      // offset of the source's P row in float4 units (P's zero row for an empty neighbour slot)
            m.g[u] = meta_g[row];
        }
    };
    // Unconditional loads (a load behind a per-lane condition makes hipcc branch around it and drain vmcnt(0) at the join -
    // with the W2 DMA and the gather itself in flight that exposed the whole gather latency in every slab).  No masks
    // either: an empty neighbour slot points at P's all-zero row n_src and carries a zero offset (sa_edge_meta_kernel),
    // and P's pad columns up to C1pad are zero, so relu(0 + 0) = 0 falls out of the arithmetic.
    auto gather = [&](const Meta& m, int k0, Vals& dst) {
        const unsigned k4 = (unsigned)(k0 >> 2) + 2u * pq;
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            const float4* p = reinterpret_cast<const float4*>(P) + ((unsigned)m.j[u] + k4);
            dst.v[u][0] = p[0];
            dst.v[u][1] = p[1];
        }
    };
    // layer-1 geometry weights of the producer's 8 k values: read from LDS BEFORE the slab's DMA is issued (an LDS read
    // behind a pending LDS-DMA makes hipcc wait for the DMA: it cannot tell the two LDS regions apart)
    struct WRegs { float4 w[2][4]; };
    auto load_w = [&](int k0, WRegs& wr_) {
        const int k = k0 + 8 * pq;
#pragma unroll
        for (int half = 0; half < 2; ++half)
#pragma unroll
            for (int c = 0; c < 4; ++c) wr_.w[half][c] = *reinterpret_cast<const float4*>(&Wr[c * C1pad + k + 4 * half]);
    };
    const unsigned lds_base = (unsigned)(uintptr_t)(lds_vp)S;   // LDS byte address of the staging array
    auto produce = [&](int stage, const Meta& m, int k0, const Vals& src, const WRegs& wr_) {
        const int k = k0 + 8 * pq;
#pragma unroll
      for (int u = 0; u < NR; ++u) {
        const float4 rg = m.g[u];
        unsigned hiw[4], low[4];
#pragma unroll
        for (int half = 0; half < 2; ++half) {
            const int kk = k + 4 * half;
            // branch-free (so the scheduler can interleave it with MFMAs): Wr is zero-padded to C1pad
            const float4 wx = wr_.w[half][0], wy = wr_.w[half][1], wz = wr_.w[half][2], wf = wr_.w[half][3];
            const float4 p = src.v[u][half];
            const float gx = rg.x, gy = rg.y, gz = rg.z, gw = rg.w;
            // scalar FMAs: as packed v_pk_fma_f32 pairs (the same bits) they measured +3 % on the class (1.88 against 1.82 ms): the
            // packed form issues no faster and co-executes worse with the MFMAs
            float v[4];
            v[0] = fmaxf(fmaf(gw, wf.x, fmaf(gz, wz.x, fmaf(gy, wy.x, fmaf(gx, wx.x, p.x)))), 0.f);
            v[1] = fmaxf(fmaf(gw, wf.y, fmaf(gz, wz.y, fmaf(gy, wy.y, fmaf(gx, wx.y, p.y)))), 0.f);
            v[2] = fmaxf(fmaf(gw, wf.z, fmaf(gz, wz.z, fmaf(gy, wy.z, fmaf(gx, wx.z, p.z)))), 0.f);
            v[3] = fmaxf(fmaf(gw, wf.w, fmaf(gz, wz.w, fmaf(gy, wy.w, fmaf(gx, wx.w, p.w)))), 0.f);
            if constexpr (PREC == 0) {
                unsigned h01, l01, h23, l23;
                split_pair(v[0], v[1], h01, l01);
                split_pair(v[2], v[3], h23, l23);
                hiw[2 * half] = h01; hiw[2 * half + 1] = h23;
                low[2 * half] = l01; low[2 * half + 1] = l23;
            } else {
                hiw[2 * half] = pack_pair<PREC>(v[0], v[1]); hiw[2 * half + 1] = pack_pair<PREC>(v[2], v[3]);
            }
        }
        // The A rows go to LDS through inline asm: a store the compiler knows about, issued while the W2 DMA of the same
        // stage is in flight, makes hipcc drain vmcnt(0) first (it cannot tell the A region from the DMA's B region) -
        // in the middle of the slab.  The asm store is invisible to that bookkeeping; its own completion is waited for by
        // the `s_waitcnt lgkmcnt(0)` in front of the loop's barrier.
        const unsigned sa = lds_base + (unsigned)stage * (STAGE_CH * 16) + (unsigned)(a_dst + u * 128 * RCH * 16);
        {
            typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
            const u32x4 hv = {hiw[0], hiw[1], hiw[2], hiw[3]};
            asm volatile("ds_write_b128 %0, %1" :: "v"(sa), "v"(hv) : "memory");
            if constexpr (PREC == 0) {
                const u32x4 lv = {low[0], low[1], low[2], low[3]};
                asm volatile("ds_write_b128 %0, %1" :: "v"(sa ^ 64u), "v"(lv) : "memory");
            }
        }
      }
    };

    const int r = lane & 31, h = lane >> 5;
    int offA[RT], offB[2];   // plane 0 (hi), k step 0; the lo plane is ^ 64, k step 1 is ^ 32
#pragma unroll
    for (int t = 0; t < RT; ++t) offA[t] = imgA(wr * 32 * RT + 32 * t + r, h);
#pragma unroll
    for (int t = 0; t < 2; ++t) offB[t] = A_CH * 16 + img(wc * 64 + 32 * t + r, h);
    f32x16 acc[RT][2];
#pragma unroll
    for (int i = 0; i < RT; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[i][j][e] = 0.f;

    // Software pipeline over the flattened slab sequence g = 0..total-1 of this workgroup's items.  Iteration g:
    //   top      : barrier; register loads: gather of slab g+2 (P rows -> `vb`, addresses from metadata `mb`), metadata of
    //              slab g+3 -> `mc`, epilogue parameters of slab g+1's item -> `ep_n`; then the W2 DMA of slab g+1
    //   k step 0 : fragment reads + MFMAs of slab g, interleaved with the PRODUCER of slab g+1 (A rows: VALU on the
    //              P values `va` gathered in iteration g-1 and metadata `ma`, written to stage (g+1)&1)
    //   k step 1 : fragment reads + MFMAs
    //   end      : epilogue if the item is complete; rotate va <- vb, ma <- mb <- mc, ep_ <- ep_n (these copies are where
    //              the compiler waits for this iteration's loads: right in front of the next barrier)
    // Every global load in the loop is unconditional, straight-line code issued before the slab's DMA: hipcc drains
    // vmcnt(0) at any join behind a branch that contains a load, and with the DMA in flight such a drain in front of the
    // fragment reads serialises the DMA, the gather latency and the MFMAs (the previous form of this loop did that in
    // every slab: 3.3x the MFMA time).  Slabs past the end replay the last slab's addresses and are never consumed.
    struct Cur { int it, s, mt, nt; };   // item, slab, the item's row / column tile (items past the end replay the last one)
    auto nxt = [&](Cur c) {
        if (++c.s == nslab) {
            c.s = 0; ++c.it;
            const int itc = min(c.it, my_items - 1);
            c.mt = item_mt(itc); c.nt = item_nt(itc);
        }
        return c;
    };
    auto meta_of = [&](Cur c, Meta& m) { load_meta(c.mt, m); };
    auto k_of = [&](Cur c) { return (c.it < my_items ? c.s : nslab - 1) * H_BK; };
    Cur c0 = {0, 0, item_mt(0), item_nt(0)}, c1 = nxt(c0), c2 = nxt(c1), c3 = nxt(c2);
    Meta ma, mb, mc;
    Vals va;
    {   // prologue: slab 0 complete in stage 0, slab 1 gathered, metadata of slabs 2 and 3 on their way
        Meta m0;
        meta_of(c0, m0);
        meta_of(c1, ma);
        meta_of(c2, mb);
        meta_of(c3, mc);
        __syncthreads();   // Wr staged
        issue(0, W2h + (size_t)c0.nt * BN * NP * C1pad, 0);
        gather(m0, 0, va);
        WRegs w0;
        load_w(0, w0);
        produce(0, m0, 0, va, w0);
        gather(ma, k_of(c1), va);
        // enter the loop with no register load pending (as every later iteration does, behind its barrier): otherwise the
        // merged loop-head state makes hipcc wait vmcnt(0) - DMA included - at the producer's first use of `va` in EVERY slab
#pragma unroll
        for (int u = 0; u < NR; ++u)
#pragma unroll
            for (int hh = 0; hh < 2; ++hh)   // an opaque use: the compiler waits for the gather here, once
                asm volatile("" : "+v"(va.v[u][hh].x), "+v"(va.v[u][hh].y), "+v"(va.v[u][hh].z), "+v"(va.v[u][hh].w));
    }
    // neighbour counts of the wave's targets (clamped addresses, no conditions: see the loop's rule about loads); the
    // per-column parameters come from the LDS table when the item is finished
    struct Degs { int d[RT][GPT]; };   // descriptors of the wave's tiles (tiles past the end read the last tile's, masked below)
    auto load_deg = [&](int mt_, Degs& e) {
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int q = 0; q < GPT; ++q) e.d[i][q] = desc[min(mt_ * (BM / 32) + wr * RT + i, M - 1) * GPT + q];
    };
    Degs dg_;
    load_deg(c0.mt, dg_);   // item 0; later items' counts arrive one iteration ahead (dg_n)
    float amax = 0.f;       // range watch: max |output| of this wave's items, committed once at the end
    for (int g = 0; g < total; ++g) {
        // B(g) landed (waited for in front of the previous iteration's epilogue, see there), A(g) written, stage (g+1)&1 free.
        // No __syncthreads(): its fence would wait (vmcnt(0)) for the stores of an epilogue issued a moment ago.
        asm volatile("" ::: "memory");
        __builtin_amdgcn_s_waitcnt(0xC07F);   // lgkmcnt(0): the producer's asm ds_writes of A(g) (see produce)
        __builtin_amdgcn_s_barrier();
        asm volatile("" ::: "memory");
        // All register loads of the iteration go out HERE, before the DMA: the gather of slab g+2 (into `vb`: the producer
        // still needs `va`), the metadata of slab g+3 and the epilogue parameters of slab g+1's item.  Nothing reads them
        // before the rotation at the end of the iteration, so the only wait on them sits in front of the next barrier.
        Vals vb;
        gather(mb, k_of(c2), vb);
        meta_of(c3, mc);
        Degs dg_n;
        load_deg(c1.mt, dg_n);
        WRegs wk;
        load_w(k_of(c1), wk);
        __builtin_amdgcn_sched_barrier(0);
        if (g + 1 < total)
            issue((g + 1) & 1, W2h + (size_t)c1.nt * BN * NP * C1pad, c1.s * H_BK);
        const char* st = S + (size_t)(g & 1) * STAGE_CH * 16;
        // both k steps' fragments are requested up front (the kernel has the registers: 212 of 256): the second step's reads
        // would otherwise sit behind the sched_barrier that closes the first step's producer interleave, i.e. be issued when
        // their values are needed (A/B against reading each step's fragments at its start: fused PointNetConv class -2.9 %)
        h8 afq[2][NP][RT], bfq[2][NP][2];
#pragma unroll
        for (int kk = 0; kk < 2; ++kk)
#pragma unroll
            for (int p = 0; p < NP; ++p) {
#pragma unroll
                for (int t = 0; t < RT; ++t) afq[kk][p][t] = *reinterpret_cast<const h8*>(st + (offA[t] ^ (kk << 5) ^ (p << 6)));
#pragma unroll
                for (int t = 0; t < 2; ++t) bfq[kk][p][t] = *reinterpret_cast<const h8*>(st + (offB[t] ^ (kk << 5) ^ (p << 6)));
            }
#pragma unroll
        for (int kk = 0; kk < 2; ++kk) {
            auto& af = afq[kk];
            auto& bf = bfq[kk];
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if constexpr (PREC == 0) {
                        acc[i][j] = h_mfma<PREC>(af[1][i], bf[0][j], acc[i][j]);
                        acc[i][j] = h_mfma<PREC>(af[0][i], bf[1][j], acc[i][j]);
                    }
                    acc[i][j] = h_mfma<PREC>(af[0][i], bf[0][j], acc[i][j]);
                }
            if (kk == 0) {   // producer VALU work is interleaved into the gaps of the MFMAs above
                produce((g + 1) & 1, ma, k_of(c1), va, wk);   // unconditional: after the last slab it fills a stage nobody reads
                constexpr int NM = 2 * RT * (PREC == 0 ? 3 : 1);   // MFMAs of this half slab
#pragma unroll
                for (int q = 0; q < NM; ++q) {
                    __builtin_amdgcn_sched_group_barrier(0x008, 1, 0);   // MFMA
                    __builtin_amdgcn_sched_group_barrier(0x002, (PREC == 0 ? 16 : 40) * NR / RT, 0);   // VALU
                }
                __builtin_amdgcn_sched_barrier(0);
            }
        }
        // Everything this iteration loaded (gather of slab g+2, metadata of slab g+3, next item's degrees) and the W2 DMA of slab
        // g+1 is waited for HERE, by an opaque use of the loaded registers: in front of the epilogue's stores, which then stay in
        // flight across the next barrier (loads, stores and LDS-DMA retire through one counter: a wait placed behind the
        // stores would wait for them too, 1-2 us per item).
#pragma unroll
        for (int u = 0; u < NR; ++u) {
            asm volatile("" : "+v"(vb.v[u][0].x), "+v"(vb.v[u][0].y), "+v"(vb.v[u][0].z), "+v"(vb.v[u][0].w),
                              "+v"(vb.v[u][1].x), "+v"(vb.v[u][1].y), "+v"(vb.v[u][1].z), "+v"(vb.v[u][1].w));
            asm volatile("" : "+v"(mc.j[u]), "+v"(mc.g[u].x), "+v"(mc.g[u].y), "+v"(mc.g[u].z), "+v"(mc.g[u].w));
        }
#pragma unroll
        for (int i = 0; i < RT; ++i)
#pragma unroll
            for (int q = 0; q < GPT; ++q) asm volatile("" : "+v"(dg_n.d[i][q]));
        __builtin_amdgcn_s_waitcnt(p2w_vmcnt_imm(0));   // ... and the DMA (the compiler's own wait above normally is vmcnt(0) already)
        if (c0.s == nslab - 1) {  // item finished: reduce over neighbour slots and store, then start the next accumulation
            SaEpiRegs<RT, GPT> e;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int col = min(c0.nt * BN + wc * 64 + j * 32 + (lane & 31), C2 - 1);
                e.bias[j] = Ep[col]; e.s[j] = Ep[SA_EPI_COLS + col]; e.t[j] = Ep[2 * SA_EPI_COLS + col];
            }
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int q = 0; q < GPT; ++q) e.dsc[i][q] = (c0.mt * (BM / 32) + wr * RT + i >= M) ? -1 : dg_.d[i][q];
            sa_epilogue_regs<PREC, RT, G>(acc, wscale, c0.nt * BN, wc, lane, e, C2, out, ldo, out_h2, ldh, amax);
#pragma unroll
            for (int i = 0; i < RT; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int e2 = 0; e2 < 16; ++e2) acc[i][j][e2] = 0.f;
        }
        __builtin_amdgcn_sched_barrier(0);
        va = vb; ma = mb; mb = mc; dg_ = dg_n;
        c0 = c1; c1 = c2; c2 = c3; c3 = nxt(c3);
    }
    if (range) range_commit_max(range, amax, lane);
}


// pre-pass kernels (p2w_feat.hip)
__global__ __launch_bounds__(256) void sa_edge_meta_kernel(const float4* __restrict__ xyzr, const int* __restrict__ idx, const int* __restrict__ batch_dst,
                                    const float* __restrict__ sf, const int* __restrict__ nbr, const int* __restrict__ deg, int kw,
                                    int M, int n_src, int ldp4, int G, const int* __restrict__ list, const int* __restrict__ n_list_dev,
                                    const int* __restrict__ src_row, int* __restrict__ meta_j, float4* __restrict__ meta_g, int* __restrict__ desc,
                                    float4* __restrict__ zero_row);
constexpr int SA_PART_BLOCK = 1024;
__global__ __launch_bounds__(SA_PART_BLOCK) void sa_part_count_kernel(const int* __restrict__ deg, int kw, int M, int* __restrict__ blk_small);
__global__ __launch_bounds__(1024) void sa_part_scan_kernel(int* __restrict__ blk_small, int nblk, int M, int* __restrict__ counts);
__global__ __launch_bounds__(SA_PART_BLOCK) void sa_part_scatter_kernel(const int* __restrict__ deg, int kw, int M, const int* __restrict__ blk_small,
                                                                     int* __restrict__ list_small, int* __restrict__ list_large);

// workspace of p2w_sa_conv_h: per-row metadata (20 B per row of a 32-row tile) + tile descriptors; with P2W_SA_PACK8 both
// target classes have their own rows (worst case: every target in either class), the two target lists and the partition's counters
// It is packed, not 256-aligned: every array starts where the one before it ends (all sizes are multiples of 4 bytes, those
// in front of a float4 array multiples of 16).  Without P2W_SA_PACK8 there are no small-class tiles (t8 = 0) and no lists.
struct SaWs {
    float4 *mg_l, *mg_s;                          // per-row geometry of the large / small class
    int *mj_l, *mj_s, *desc_l, *desc_s;           // per-row source offsets, tile descriptors
    int *list_s, *list_l, *blk, *counts;          // P2W_SA_PACK8: the two target lists, the partition's block counters and
    long t32, t8, nblk;                           //   counts: [0] small targets, [1] large targets, [2] / [3] their tiles
};
static inline SaWs sa_conv_carve(P2wArena& a, long M, int flags) {
    const bool pack8 = (flags & P2W_SA_PACK8) != 0;
    SaWs W = {};
    W.t32 = M;
    W.t8 = pack8 ? (M + 3) / 4 : 0;
    W.nblk = pack8 ? (M + SA_PART_BLOCK - 1) / SA_PART_BLOCK : 0;
    W.mg_l = a.take<float4>((size_t)W.t32 * 32, 16);
    W.mg_s = a.take<float4>((size_t)W.t8 * 32, 16);
    W.mj_l = a.take<int>((size_t)W.t32 * 32, 4);
    W.mj_s = a.take<int>((size_t)W.t8 * 32, 4);
    W.desc_l = a.take<int>((size_t)W.t32, 4);
    W.desc_s = a.take<int>((size_t)W.t8 * 4, 4);
    if (!pack8) { a.raw(256, 1); return W; }      // slack
    W.list_s = a.take<int>((size_t)M, 4);
    W.list_l = a.take<int>((size_t)M, 4);
    W.blk = a.take<int>((size_t)W.nblk, 4);
    W.counts = a.take<int>(16, 4);
    a.raw(1024, 1);                               // slack
    return W;
}

// host side of p2w_sa_conv_h for one precision (pointer / size checks are done by the caller)
template <int PREC>
static int32_t launch_sa_conv_h(const float* P, int32_t ldp, int32_t n_src, const float* xyzr_src, const int32_t* idx, const int32_t* batch_dst,
                                const float* sf, const int32_t* nbr, const int32_t* deg, int32_t kw, int32_t M,
                                const float* w1r4, const _Float16* W2h, float wscale, int32_t C1, int32_t C2, const float* b2,
                                const float* bn_s, const float* bn_t, float* out, int32_t ldo, _Float16* out_h2, int32_t ldh,
                                void* ws, size_t ws_bytes, int32_t flags, hipStream_t stream, const int32_t* src_row = nullptr,
                                unsigned* range = nullptr) {
    constexpr int KA = HCfg<PREC>::kalign;
    const int C2pad = (C2 + 255) / 256 * 256, C1pad = (C1 + KA - 1) / KA * KA;
    // LDS tables (layer-1 geometry weights, per-column epilogue parameters) and 32-bit offsets: edge rows, P rows in float4 units
    if (C1pad > 512 || C2 > SA_EPI_COLS || (long)M >= (1L << 25) || ((long)n_src + 1) * (ldp / 4) >= (1L << 31)) return P2W_EUNSUPPORTED;   // (descriptors hold target << 6)
    if (ldp < C1pad) return P2W_EINVAL;   // P rows are read in whole K slabs: pad columns (zero) must exist
    P2wArena arena(ws);
    const SaWs L = sa_conv_carve(arena, M, flags);
    if (ws == nullptr || ws_bytes < arena.bytes()) return P2W_EWORKSPACE;
    if (reinterpret_cast<uintptr_t>(ws) & 15u) return P2W_EALIGN;
    const int n_cu = p2w_cu_count();
    // 256-column items halve the A production per output column; measured on levels 2 / 3 (C2 = 256 / 512): 2.73 vs 2.82-2.97 ms
    const bool wide = (flags & (P2W_SA_ITEM_256 | P2W_SA_ITEM_128)) ? (flags & P2W_SA_ITEM_256) != 0 : C2 > 128;
    const int tpi = wide ? 4 : 8, nNt3 = p2w_cdiv(C2, wide ? 256 : 128);   // tiles per work item, column tiles
    const float4* x4 = reinterpret_cast<const float4*>(xyzr_src);
    // one class of targets: metadata pre-pass over `rows_max` rows + the persistent kernel over at most `tiles_max` tiles
    auto run = [&](auto g_c, const int* list, const int* n_list_dev, const int* tiles_dev, long tiles_max, float4* meta_g, int* meta_j,
                   int* desc) {
        constexpr int G = decltype(g_c)::value;
        const long rows_max = tiles_max * 32;
        // (the pre-pass also zeroes P's row n_src - the row empty neighbour slots gather: the caller need not)
        sa_edge_meta_kernel<<<p2w_cdiv(rows_max, 256), 256, 0, stream>>>(x4, idx, batch_dst, sf, nbr, deg, kw, M, n_src, ldp / 4, G,
                                                                       list, n_list_dev, src_row, meta_j, meta_g, desc,
                                                                       reinterpret_cast<float4*>(const_cast<float*>(P) + (size_t)n_src * ldp));
        const long items = p2w_cdiv(tiles_max, tpi) * nNt3;
        int grid = (int)(items < n_cu ? items : n_cu);
        if (grid >= 8) grid &= ~7;   // whole XCD rounds (see the kernel's work assignment)
        const int nMt3 = (int)p2w_cdiv(tiles_max, tpi);
        if (wide)
            sa_conv16p_kernel<PREC, 256, 2, G><<<grid, 512, 0, stream>>>(
                P, ldp, meta_j, meta_g, desc, tiles_dev, (int)tiles_max, w1r4, C1, C1pad, W2h, (size_t)C2pad * C1pad, wscale, C2, nMt3,
                nNt3, b2, bn_s, bn_t, out, ldo, out_h2, ldh, range);
        else
            sa_conv16p_kernel<PREC, 128, 2, G><<<grid, 512, 0, stream>>>(
                P, ldp, meta_j, meta_g, desc, tiles_dev, (int)tiles_max, w1r4, C1, C1pad, W2h, (size_t)C2pad * C1pad, wscale, C2, nMt3,
                nNt3, b2, bn_s, bn_t, out, ldo, out_h2, ldh, range);
    };
    if (!(flags & P2W_SA_PACK8)) {
        run(std::integral_constant<int, 32>{}, nullptr, nullptr, nullptr, M, L.mg_l, L.mj_l, L.desc_l);
        return P2W_LAUNCH_STATUS();
    }
    // P2W_SA_PACK8: targets with at most 8 neighbours (the sparse ball-query level) share a 32-row MFMA tile four at a time,
    // the others keep a tile each.  Stable partition on the device (no host synchronisation: the kernels read their tile
    // counts from `counts`), then one pre-pass + persistent kernel per class.
    int* counts = L.counts;
    sa_part_count_kernel<<<(int)L.nblk, SA_PART_BLOCK, 0, stream>>>(deg, kw, M, L.blk);
    sa_part_scan_kernel<<<1, 1024, 0, stream>>>(L.blk, (int)L.nblk, M, counts);
    sa_part_scatter_kernel<<<(int)L.nblk, SA_PART_BLOCK, 0, stream>>>(deg, kw, M, L.blk, L.list_s, L.list_l);
    run(std::integral_constant<int, 8>{}, L.list_s, counts + 0, counts + 2, L.t8, L.mg_s, L.mj_s, L.desc_s);
    run(std::integral_constant<int, 32>{}, L.list_l, counts + 1, counts + 3, L.t32, L.mg_l, L.mj_l, L.desc_l);
    return P2W_LAUNCH_STATUS();
}

// entry points of the single-plane family (defined in p2w_feat_h1.hip, called by the extern "C" dispatchers)
int32_t p2w_gemm_h1_impl(int32_t prec, const _Float16* Ah, int32_t ldh_a, const _Float16* Wp, float wscale, int32_t M, int32_t N,
                         int32_t K, const EpiArgs& ep, float* out_f32, int32_t ldo, _Float16* out_h2, int32_t ldh_o,
                         int32_t flags, hipStream_t stream, const float* dotw = nullptr, float* part = nullptr, int32_t ldpart = 0,
                         float* skws = nullptr, size_t skws_bytes = 0);
int32_t p2w_sa_conv_h1_impl(int32_t prec, const float* P, int32_t ldp, int32_t n_src, const float* xyzr_src, const int32_t* idx,
                            const int32_t* batch_dst, const float* sf, const int32_t* nbr, const int32_t* deg, int32_t kw,
                            int32_t M, const float* w1r4, const _Float16* W2h, float wscale, int32_t C1, int32_t C2,
                            const float* b2, const float* bn_s, const float* bn_t, float* out, int32_t ldo, _Float16* out_h2,
                            int32_t ldh, void* ws, size_t ws_bytes, int32_t flags, hipStream_t stream, const int32_t* src_row = nullptr,
                            unsigned* range = nullptr);
