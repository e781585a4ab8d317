// The one text of the attention backward arithmetic (head dim 64, non-causal), shared by attention_bwd.hip (yv_attention_bwd),
// attention_bwd_long.hip (yv_attention_bwd_long) and attention_bwd_short.hip (yv_attention_bwd_short).  DESIGN.md section 16.1.
//
// Seven products, P recomputed from the forward's log2-sum-exp, P and dS fed to the next MFMA from the accumulator registers, no
// cross-wave sums, no atomics.  A wave owns 32 rows of one axis (row on the lane) and walks the other axis in groups of 32 rows:
//   dq_group   owner = 32 QUERIES: S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T * (dP^T - delta) * scale, dQ^T += K^T.dS^T
//   dkv_group  owner = 32 KEYS:    S = Q.K^T, dP = dO.V^T, dV^T += dO^T.P, dK^T += Q^T.dS
// Every element-wise expression, cast and MFMA order of the three entry points is here, so their dqkv and delta can differ only
// through the order in which a kernel walks the groups: ascending in all of them (their own bit tests and
// tests/golden/attn_bwd_bits.json hold that).  A position past N contributes an exact zero.  Blocking, LDS carving, staging,
// barriers and the loops stay in each .hip.
#pragma once
#include "yv_common.h"

namespace {

constexpr int HD = 64;
constexpr float LOG2E = 1.4426950408889634f;             // the kernels take scale * LOG2E: exp2f instead of expf

// A layout reads MFMA fragments of an LDS image of 32 n rows x 64 bf16 for the lane it was made for (rl = lane & 31 the row or
// column on the lane, hh = lane >> 5 the half):
//   rows(img, row0, ks)  rows row0 .. row0 + 31, columns 16 ks + 8 hh .. + 7: A operand of the S / dP products (row0 a multiple of 32)
//   cols(img, mt, r0)    columns 32 mt .. + 31, rows r0 + 4 hh .. + 3 and 8 further: A operand of the dQ / dK / dV products (r0 a
//                        multiple of 16)
// TAIL_BRANCH: whether a group step tests for the group that straddles N (wave-uniform) and spares the others the mask.  The
// kernels of attention_bwd.hip mask every group: one of their loops is fully unrolled and would carry both bodies NT times.

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;

__device__ __forceinline__ int swz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }
// byte offset of 16-byte chunk c (0..7) of row `row` in a swizzled image
__device__ __forceinline__ int img_off(int row, int c) { return row * 128 + ((c ^ swz(row)) << 4); }

__device__ __forceinline__ bf16x8 frag_rows(const unsigned char* img, int row, int chunk) {
    return *(const bf16x8*)(img + img_off(row, chunk));
}

// Lane offsets of the transposed A fragment (attention_long.hip): 16-lane group G = lane >> 4 takes d columns 32 mt + (G & 1) * 16
// .. + 15 of the rows r0 + 4 (G >> 1) + q (first read) and 8 rows further (second read); lane 4 q + p of the group addresses row q,
// columns 4 p .. 4 p + 3.  r0 is a multiple of 16, so swz does not depend on it: offsets [mt][first | second], plus r0 * 128.
struct TrOff { int o[2][2]; };
__device__ __forceinline__ TrOff tr_offsets(int lane) {
    const int tG = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int row = 4 * (tG >> 1) + tq;
    TrOff t;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int h = 0; h < 2; ++h) t.o[mt][h] = img_off(row + 8 * h, mt * 4 + (tG & 1) * 2 + (tp >> 1)) + (tp & 1) * 8;
    return t;
}
__device__ __forceinline__ bf16x8 frag_tr(const unsigned char* img, const TrOff& t, int mt, int r0) {
    const unsigned char* p = img + r0 * 128;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(p + t.o[mt][0]));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(p + t.o[mt][1]));
    const u32x2 lo2 = __builtin_bit_cast(u32x2, lo), hi2 = __builtin_bit_cast(u32x2, hi);
    const u32x4 pk = {lo2[0], lo2[1], hi2[0], hi2[1]};
    return __builtin_bit_cast(bf16x8, pk);
}

// ONE image per tensor (attention_bwd_long.hip, attention_bwd_short.hip): 128-byte rows, 16-byte chunk c of row r at chunk
// c ^ swz(r); ds_read_b128 for the rows, ds_read_b64_tr_b16 for the columns.
struct SwizzledImage {
    static constexpr bool TAIL_BRANCH = true;
    typedef const unsigned char* Image;
    int rl, hh;
    TrOff tro;
    __device__ __forceinline__ explicit SwizzledImage(int lane) : rl(lane & 31), hh(lane >> 5), tro(tr_offsets(lane)) {}
    __device__ __forceinline__ bf16x8 rows(Image m, int row0, int ks) const { return frag_rows(m, row0 + rl, 2 * ks + hh); }
    __device__ __forceinline__ bf16x8 cols(Image m, int mt, int r0) const { return frag_tr(m, tro, mt, r0); }
};

// TWO images per tensor of NP rows (attention_bwd.hip): 128-byte rows with the 16-byte chunk XOR-swizzled by (row >> 1) & 7 for the
// rows, and a transposed image [64][NP] with a row stride of TS bytes (8 bytes of padding) for the columns.  `t` may be null where a
// kernel never reads a tensor's columns (V in the dQ kernel).
template <int NP>
struct PaddedPair {
    static constexpr bool TAIL_BRANCH = false;
    static constexpr int TS = NP * 2 + 8;
    struct Image { const unsigned char* r; const unsigned char* t; };
    int rl, hh;
    __device__ __forceinline__ explicit PaddedPair(int lane) : rl(lane & 31), hh(lane >> 5) {}
    __device__ __forceinline__ bf16x8 rows(const Image& m, int row0, int ks) const {
        const int row = row0 + rl;
        return *(const bf16x8*)(m.r + row * 128 + (((2 * ks + hh) ^ ((row >> 1) & 7)) << 4));
    }
    __device__ __forceinline__ bf16x8 cols(const Image& m, int mt, int r0) const {
        const unsigned char* p = m.t + (mt * 32 + rl) * TS + (r0 + 4 * hh) * 2;
        const uint2 lo = *(const uint2*)p, hi = *(const uint2*)(p + 16);
        const u32x4 pk = {lo.x, lo.y, hi.x, hi.y};
        return __builtin_bit_cast(bf16x8, pk);
    }
};

// The dQ side's per-lane operands of query q of (crop r, head hd): fq / fdo = the halves of the Q and dO rows that lane half hh
// feeds to the MFMAs, dl = delta[q] = sum_d dO * O (64 products in f32: 32 per half, then the half-wave exchange; stored by
// hh == 0), lq = lse[q].  A q past N reads row N - 1 and stores nothing.  `base` = qkv + crop r's first row + hd * HD.
__device__ __forceinline__ void owner_query(const uint16_t* base, const uint16_t* o, const uint16_t* dout, const float* lse,
                                            float* delta, int r, int hd, int N, int H, int q, int hh, bf16x8 (&fq)[4],
                                            bf16x8 (&fdo)[4], float& dl, float& lq) {
    const int D = H * HD, ld = 3 * D, qc = q < N ? q : N - 1;
    const uint16_t* orow = o + ((size_t)r * N + qc) * D + hd * HD;
    const uint16_t* drow = dout + ((size_t)r * N + qc) * D + hd * HD;
    dl = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        fq[ks] = *(const bf16x8*)(base + (size_t)qc * ld + ks * 16 + hh * 8);
        fdo[ks] = *(const bf16x8*)(drow + ks * 16 + hh * 8);
        const bf16x8 fo = *(const bf16x8*)(orow + ks * 16 + hh * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) dl += (float)fdo[ks][j] * (float)fo[j];
    }
    dl += __shfl_xor(dl, 32, 64);
    if (q < N && hh == 0) delta[((size_t)r * H + hd) * N + q] = dl;
    lq = lse[((size_t)r * H + hd) * N + qc];
}

__device__ __forceinline__ void zero(f32x16 (&a)[2]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) a[mt][e] = 0.f;
}

// The element-wise step between the products of a group.  Accumulator element e of a lane is row (e & 3) + 8 (e >> 2) + 4 hh of the
// group: `first` is that row of e = 0 as a global index, and lse_s / del_s point at its constants.  MASKED: rows >= N give P = 0.
// (Not lambdas of the group steps: with those attn_bwd_dq_kernel<1> took 200 registers for 156, one wave per SIMD less.)
// dS^T = P^T * (dP^T - delta) * scale with P^T = exp2(S^T*c - lse[q]); s: S^T in, dS^T out
template <bool MASKED>
__device__ __forceinline__ void to_ds(f32x16& s, const f32x16& dp, int first, int N, float lq, float dl, float scale,
                                      float scale_log2e) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int key = first + (e & 3) + 8 * (e >> 2);
        const float pv = !MASKED || key < N ? exp2f(s[e] * scale_log2e - lq) : 0.f;
        s[e] = pv * (dp[e] - dl) * scale;
    }
}
// P = exp2(S*c - lse[q]) and dS = P * (dP - delta[q]) * scale; sv: S in, P out; dp: dP in, dS out
template <bool MASKED>
__device__ __forceinline__ void to_p_ds(f32x16& sv, f32x16& dp, int first, int N, const float* lse_s, const float* del_s,
                                        float scale, float scale_log2e) {
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int i = (e & 3) + 8 * (e >> 2);
        const float pv = !MASKED || first + i < N ? exp2f(sv[e] * scale_log2e - lse_s[i]) : 0.f;
        sv[e] = pv;
        dp[e] = pv * (dp[e] - del_s[i]) * scale;
    }
}

// One group of 32 keys for 32 owner queries: image rows row0 .. row0 + 31 of K and V hold keys key0 .. key0 + 31.
template <class L>
__device__ __forceinline__ void dq_group(const L& lay, const typename L::Image& K, const typename L::Image& V, int row0, int key0,
                                         int N, const bf16x8 (&fq)[4], const bf16x8 (&fdo)[4], float lq, float dl, float scale,
                                         float scale_log2e, f32x16 (&acc)[2]) {
    f32x16 s, dp;
#pragma unroll
    for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lay.rows(K, row0, ks), fq[ks], s, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lay.rows(V, row0, ks), fdo[ks], dp, 0, 0, 0);
    }
    const int first = key0 + 4 * lay.hh;
    if (!L::TAIL_BRANCH || key0 + 32 > N) to_ds<true>(s, dp, first, N, lq, dl, scale, scale_log2e);      // the group that straddles N
    else to_ds<false>(s, dp, first, N, lq, dl, scale, scale_log2e);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        bf16x8 fp;
#pragma unroll
        for (int j = 0; j < 8; ++j) fp[j] = (__bf16)s[8 * st + j];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
            acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lay.cols(K, mt, row0 + 16 * st), fp, acc[mt], 0, 0, 0);
    }
}

// One group of 32 queries for 32 owner keys: image rows row0 .. row0 + 31 of Q and dO and lse_s / del_s [row0 .. row0 + 31] hold
// queries q0 .. q0 + 31.  An owner key past N accumulates finite values that are never stored.
template <class L>
__device__ __forceinline__ void dkv_group(const L& lay, const typename L::Image& Q, const typename L::Image& dO, const float* lse_s,
                                          const float* del_s, int row0, int q0, int N, const bf16x8 (&fk)[4], const bf16x8 (&fv)[4],
                                          float scale, float scale_log2e, f32x16 (&dk)[2], f32x16 (&dv)[2]) {
    f32x16 sv, dp;
#pragma unroll
    for (int e = 0; e < 16; ++e) sv[e] = dp[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lay.rows(Q, row0, ks), fk[ks], sv, 0, 0, 0);
        dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lay.rows(dO, row0, ks), fv[ks], dp, 0, 0, 0);
    }
    const int first = q0 + 4 * lay.hh, at = row0 + 4 * lay.hh;
    if (!L::TAIL_BRANCH || q0 + 32 > N) to_p_ds<true>(sv, dp, first, N, lse_s + at, del_s + at, scale, scale_log2e);   // straddles N
    else to_p_ds<false>(sv, dp, first, N, lse_s + at, del_s + at, scale, scale_log2e);
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        bf16x8 fp, fs;
#pragma unroll
        for (int j = 0; j < 8; ++j) { fp[j] = (__bf16)sv[8 * st + j]; fs[j] = (__bf16)dp[8 * st + j]; }
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) {
            dv[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lay.cols(dO, mt, row0 + 16 * st), fp, dv[mt], 0, 0, 0);
            dk[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(lay.cols(Q, mt, row0 + 16 * st), fs, dk[mt], 0, 0, 0);
        }
    }
}

// A lane's 2 x 16 accumulator elements are columns mt * 32 + 8 g4 + 4 hh .. + 3 of its row: eight 8-byte stores of bf16 (RNE).
__device__ __forceinline__ void store_head_row(uint16_t* dst, int hh, const f32x16 (&a)[2]) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
            *(uint2*)(dst + mt * 32 + 8 * g4 + 4 * hh) =
                make_uint2(pack_bf16x2(a[mt][4 * g4], a[mt][4 * g4 + 1]), pack_bf16x2(a[mt][4 * g4 + 2], a[mt][4 * g4 + 3]));
}
// `row` = the owner's global row (crop * N + token), < R * N; dqkv rows are [dQ | dK | dV] of D = H * HD columns each
__device__ __forceinline__ void store_dq(uint16_t* dqkv, size_t row, int hd, int H, int hh, const f32x16 (&acc)[2]) {
    store_head_row(dqkv + row * (3 * H * HD) + hd * HD, hh, acc);
}
__device__ __forceinline__ void store_dkv(uint16_t* dqkv, size_t row, int hd, int H, int hh, const f32x16 (&dk)[2],
                                          const f32x16 (&dv)[2]) {
    uint16_t* dst = dqkv + row * (3 * H * HD) + hd * HD;
    store_head_row(dst + H * HD, hh, dk);
    store_head_row(dst + 2 * H * HD, hh, dv);
}

struct BwdArgs {
    const uint16_t* qkv; const uint16_t* o; const uint16_t* dout; const float* lse;
    int R, N, H;
    float scale;
    uint16_t* dqkv; float* delta;
    hipStream_t st;
};

inline BwdArgs bwd_args(const void* qkv, const void* out, const void* dout, const float* lse, int R, int N, int H, float scale,
                        void* dqkv, float* delta_ws, void* stream) {
    return BwdArgs{(const uint16_t*)qkv, (const uint16_t*)out, (const uint16_t*)dout, lse, R, N, H, scale,
                   (uint16_t*)dqkv, delta_ws, (hipStream_t)stream};
}

// The check of yv_attention_bwd_long and yv_attention_bwd_short, whose staging moves 16-byte chunks: pointers, sizes (R == 0 is
// valid: the caller returns YV_OK after its own limits), 16-byte alignment of the bf16 tensors and 4-byte alignment of lse and
// delta_ws, and a grid of R * H * blocks workgroups that fits an int.  NOT the check of yv_attention_bwd, which keeps its own
// contract: YV_ERR_ARG for R == 0 and no alignment requirement.  yv_attention_bwd_short adds YV_ERR_LIMIT for N > 224.
inline int bwd_args_check(const BwdArgs& a, int blocks) {
    if (!a.qkv || !a.o || !a.dout || !a.lse || !a.dqkv || !a.delta || a.R < 0 || a.N <= 0 || a.H <= 0) return YV_ERR_ARG;
    if (((uintptr_t)a.qkv | (uintptr_t)a.o | (uintptr_t)a.dout | (uintptr_t)a.dqkv) & 15) return YV_ERR_ARG;   // 16-byte row chunks
    if (((uintptr_t)a.lse | (uintptr_t)a.delta) & 3) return YV_ERR_ARG;
    if ((long long)a.R * a.H * blocks > 0x7fffffffLL) return YV_ERR_LIMIT;
    return YV_OK;
}

}  // namespace
