// The MXFP8 block format of this library (DESIGN.md sections 10 / 11), stated once: every quantiser - yv_quant_mxfp8, its map and
// two-form variants and every fused producer (GEMM and convolution epilogues, LayerNorm, attention) - calls these functions, so a
// fused producer writes the bytes of the bf16 operation followed by yv_quant_mxfp8 by construction.
//   block    32 consecutive elements of a row (K index) / 32 consecutive channels of a pixel
//   scale    E8M0 byte e + 127, e = ceil(log2(amax / 448)) clamped to [-127, 127] (so that amax * 2^-e <= 448), all-zero block: -127
//   element  RNE_e4m3(x * 2^-e), x the bf16-rounded value
#pragma once
#include "yv_common.h"

// E8M0 exponent of a block from its amax.  amax / 448 = mant * 2^ex with mant in [0.5, 1): ceil(log2) is ex, or ex - 1 at mant == 0.5
__device__ __forceinline__ int mx_block_exp(float amax) {
    int e = -127;
    if (amax > 0.f) {
        int ex;
        const float mant = frexpf(amax * (1.0f / 448.0f), &ex);
        e = mant == 0.5f ? ex - 1 : ex;
        e = e < -127 ? -127 : (e > 127 ? 127 : e);
    }
    return e;
}

// A lane's N values of a block (bf16-representable f32) whose other values sit in the lanes at the xor distances XOR... (ascending;
// none: the lane holds the whole block) -> the block exponent and N / 4 dwords of e4m3 bytes, value 4 i + k in byte k of dword i.
// The amax is taken over the lane's values in ascending order, then over the xor steps in the order given.  Every lane of a block
// must call it together (the shuffles); lanes whose values are not stored may pass anything finite their partners do not depend on.
template <int... XOR, int N>
__device__ __forceinline__ int mx_quant_block(const float (&v)[N], uint32_t (&out)[N / 4]) {
    static_assert(N == 4 || N == 8 || N == 16 || N == 32, "values per lane");
    float amax = 0.f;
#pragma unroll
    for (int i = 0; i < N; ++i) amax = fmaxf(amax, fabsf(v[i]));
    ((amax = fmaxf(amax, __shfl_xor(amax, XOR, 64))), ...);
    const int e = mx_block_exp(amax);
    const float inv = ldexpf(1.0f, -e);
#pragma unroll
    for (int i = 0; i < N / 4; ++i) {
        int p = 0;
        p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i] * inv, v[4 * i + 1] * inv, p, false);
        p = __builtin_amdgcn_cvt_pk_fp8_f32(v[4 * i + 2] * inv, v[4 * i + 3] * inv, p, true);
        out[i] = (uint32_t)p;
    }
    return e;
}

// Lane-stride form: a 16-row x 32-column piece of an MFMA accumulator tile (C^T layout, two 16-column fragments).  Lane (fr, fq) =
// (lane & 15, lane >> 4) holds, of row fr's one block, columns 4 fq .. 4 fq + 3 (v[0 .. 3]) and 16 + 4 fq .. (v[4 .. 7]); the rest
// of the block sits in the lanes at stride 16 (fr + 16, fr + 32, fr + 48), i.e. at the xor distances 16 and 32.  out[0] / out[1]
// are the four bytes at column 4 fq / 16 + 4 fq of the block.
__device__ __forceinline__ int mx_quant_piece16x32(const float (&v)[8], uint32_t (&out)[2]) { return mx_quant_block<16, 32>(v, out); }

// Where the scale byte of block bk (= k / 32) of a row lives.  K-step-major (K / 128, rows_pad, 4): the four bytes of a row's
// 128-deep K step are one dword (the operand layout of the block-scaled MFMA loops).  MX map: (pixel, C / 32), ldq bytes per pixel.
__device__ __forceinline__ long long mx_scale_kmajor(int bk, long long rows_pad, long long row) {
    return ((long long)(bk >> 2) * rows_pad + row) * 4 + (bk & 3);
}
__device__ __forceinline__ long long mx_scale_map(long long pixel, long long ldq, int bk) { return pixel * (ldq >> 5) + bk; }

// One 32-element block of a bf16 row (src: 16-byte aligned, global or LDS) -> its 32 e4m3 bytes at dst; returns the scale byte
__device__ __forceinline__ uint8_t mx_quant_row32(const uint16_t* src, uint8_t* dst) {
    float v[32];
#pragma unroll
    for (int c = 0; c < 4; ++c) unpack_bf16x8(*(const u32x4*)(src + c * 8), reinterpret_cast<float (&)[8]>(v[c * 8]));
    uint32_t out[8];
    const int e = mx_quant_block(v, out);
    ((uint4*)dst)[0] = make_uint4(out[0], out[1], out[2], out[3]);
    ((uint4*)dst)[1] = make_uint4(out[4], out[5], out[6], out[7]);
    return (uint8_t)(e + 127);
}
