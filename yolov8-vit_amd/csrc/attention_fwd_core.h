// The one text of the attention forward arithmetic and addresses (head dim 64, non-causal, bf16 in, f32 accumulate), shared by
// attention.hip (attention_kernel, attention_pipe_kernel) and attention_long.hip (attention_long_kernel).  DESIGN.md section 15.3.
//
// MFMA plan (v_mfma_f32_32x32x16_bf16): a wave owns 32 queries (query on the lane: rl = lane & 31, hh = lane >> 5 the half) and
// walks the keys in groups of 32.
//   S^T = K_group (A: 32 keys x 64 d) . Q^T (B: 64 d x 32 queries): the accumulator has the KEY on the register axis (key_of), so
//     the softmax row reduction is in-lane + one lane ^ 32 exchange, and
//   O^T += V^T (A: 64 d x keys) . P^T (B: keys x 32 queries) takes the exponentiated accumulator registers directly as its B operand
//     (registers 8 st .. + 7 -> k step st; k order inside a step 8 (j >> 2) + 4 hh + (j & 3), matched by the V^T fragment reads): P
//     never touches LDS.  Afterwards a lane holds d = 32 mt + 8 g4 + 4 hh .. + 3 of its query in o[mt][4 g4 .. + 3].
// Every element-wise expression, cast, mask, address and output format is here.  A key past N is fetched from row N - 1 (finite),
// its score is masked to -inf, its probability is exactly 0.  Blocking, LDS carving, staging, barriers, loops and the whole hand
// schedule of attention_pipe_kernel (which takes only the addresses, the mask and the epilogue from here) stay in each .hip;
// tests/golden/attn_fwd_bits.json holds what every instance writes.
#pragma once
#include "mx_quant.h"

namespace {

constexpr int HD = 64;
constexpr float LOG2E = 1.4426950408889634f;             // the kernels take scale * LOG2E: exp2f instead of expf

// optional MXFP8 image of the output (operand of the proj GEMM of yv_linear_mxfp8): e4m3 bytes + E8M0 per 32 columns
struct AttnMx { uint8_t* q; long long ldq; uint8_t* s; long long rows; };

typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;

// ---- LDS images: 128-byte rows of 8 chunks of 16 bytes; chunk c of row `row` lives at chunk position k_chunk / v_chunk (each its
// own inverse: a DMA lane that fills position c fetches source chunk k_chunk(row, c)) -----------------------------------------
//   K (and the Q rows of attention_pipe_kernel): c ^ ((row >> 1) & 7), conflict-free ds_read_b128 of the 32-row A fragment;
//   V, row-major, for the transposing read: c ^ 4 ((row >> 1) & 1).  A 32-lane half of ds_read_b64_tr_b16 takes rows 0..3 of a
//     4-key block, 64 bytes each; rows 0 / 2 (and 1 / 3) start on the same bank and the swizzle sends them to opposite halves.
__device__ __forceinline__ int k_chunk(int row, int c) { return c ^ ((row >> 1) & 7); }
__device__ __forceinline__ int v_chunk(int row, int c) { return c ^ (((row >> 1) & 1) << 2); }
__device__ __forceinline__ int k_off(int row, int c) { return row * 128 + (k_chunk(row, c) << 4); }
__device__ __forceinline__ int v_off(int row, int c) { return row * 128 + (v_chunk(row, c) << 4); }
// write / DMA-source side: slot i (a thread's trip index, or a lane of an 8-row piece) is chunk i & 7 of row i >> 3
struct RowChunk { int row, c; };
__device__ __forceinline__ RowChunk row_chunk(int i) { return {i >> 3, i & 7}; }

// ---- fragments ------------------------------------------------------------------------------------------------------------------
// Q (B operand) of query q, straight from global; a query past N reads row N - 1 and stores nothing
__device__ __forceinline__ void q_frags(const uint16_t* base, int q, int N, int ld, int hh, bf16x8 (&fq)[4]) {
    const int qc = q < N ? q : N - 1;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fq[ks] = *(const bf16x8*)(base + (size_t)qc * ld + ks * 16 + hh * 8);
}
// d columns 16 ks + 8 hh .. + 7 of this lane's row of a K image
__device__ __forceinline__ bf16x8 k_frag(const unsigned char* img, int row, int ks, int hh) {
    return *(const bf16x8*)(img + k_off(row, 2 * ks + hh));
}

// key (within its group of 32) of accumulator register e
__device__ __forceinline__ int key_of(int e, int hh) { return (e & 3) + 8 * (e >> 2) + 4 * hh; }
// the group that straddles N: keys past N to -inf (key0 = the group's first key)
__device__ __forceinline__ void mask_group(f32x16& sv, int key0, int N, int hh) {
#pragma unroll
    for (int e = 0; e < 16; ++e) sv[e] = key0 + key_of(e, hh) < N ? sv[e] : -INFINITY;
}
// S^T of the 32 keys whose K rows start at row0 of the image
__device__ __forceinline__ f32x16 score_group(const unsigned char* Kimg, int row0, const bf16x8 (&fq)[4], int rl, int hh) {
    f32x16 sv;
#pragma unroll
    for (int e = 0; e < 16; ++e) sv[e] = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_frag(Kimg, row0 + rl, ks, hh), fq[ks], sv, 0, 0, 0);
    return sv;
}
// One group of the online softmax: sv (masked scores) -> probabilities against the running maximum; O and this lane's share of the
// row sum (lane ^ 32 holds the rest) are rescaled only when some query's maximum grew (wave-uniform).  The first group holds a
// valid key for every row, so m_run is finite from then on.
__device__ __forceinline__ void online_step(f32x16& sv, float& m_run, float& l_lane, f32x16 (&o)[2], float scale_log2e) {
    float mx = sv[0];
#pragma unroll
    for (int e = 1; e < 16; ++e) mx = fmaxf(mx, sv[e]);
    mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
    const float m_new = fmaxf(m_run, mx);
    if (__any(m_new > m_run)) {
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2e);   // 1 for unchanged rows, 0 at the start
        l_lane *= alpha;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[mt][e] *= alpha;
        m_run = m_new;
    }
    const float mb = m_run * scale_log2e;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        sv[e] = __builtin_amdgcn_exp2f(fmaf(sv[e], scale_log2e, -mb));               // one v_fma + one v_exp
        l_lane += sv[e];
    }
}
// B operand of PV k step st (16 keys) of a group
__device__ __forceinline__ bf16x8 p_frag(const f32x16& sv, int st) {
    bf16x8 fp;
#pragma unroll
    for (int j = 0; j < 8; ++j) fp[j] = (__bf16)sv[8 * st + j];
    return fp;
}
// O^T += V^T . P^T of one group; vt(mt, st) = the V^T fragment of d columns 32 mt .. + 31, keys 16 st + 4 hh .. + 3 and 8 further
template <class F>
__device__ __forceinline__ void pv_product(const f32x16& sv, f32x16 (&o)[2], F&& vt) {
#pragma unroll
    for (int st = 0; st < 2; ++st) {
        const bf16x8 fp = p_frag(sv, st);
#pragma unroll
        for (int mt = 0; mt < 2; ++mt) o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt(mt, st), fp, o[mt], 0, 0, 0);
    }
}

// V^T fragment from the explicitly transposed image of attention_kernel: [64 d][keys], `stride` bytes per row (an odd multiple of
// 8 bytes: conflict-free ds_read_b64 over 32 rows); key0 = first key of the k step within the image
__device__ __forceinline__ bf16x8 vt_frag_padded(const unsigned char* Vt, int stride, int mt, int key0, int rl, int hh) {
    const unsigned char* vr = Vt + (mt * 32 + rl) * stride + (key0 + 4 * hh) * 2;
    const uint2 lo = *(const uint2*)vr, hi = *(const uint2*)(vr + 16);
    const u32x4 pk = {lo.x, lo.y, hi.x, hi.y};
    return __builtin_bit_cast(bf16x8, pk);
}
// V^T fragment from the row-major V image by the transposing read: 16-lane group G = lane >> 4 takes d columns 32 mt + (G & 1) * 16
// .. + 15 of the key rows kb + 4 (G >> 1) + q (first read) and 8 rows further (second read); lane 4 q + p of the group addresses
// row q, columns 4 p .. 4 p + 3.  kb is a multiple of 16, so the swizzle does not depend on it: o[mt], plus kb * 128.
struct VtOff { int o[2]; };
__device__ __forceinline__ VtOff vt_offsets(int lane) {
    const int tG = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int row = 4 * (tG >> 1) + tq;
    VtOff t;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) t.o[mt] = v_off(row, mt * 4 + (tG & 1) * 2 + (tp >> 1)) + (tp & 1) * 8;
    return t;
}
__device__ __forceinline__ bf16x8 vt_frag_tr(const unsigned char* Vs, const VtOff& t, int mt, int kb) {
    const unsigned char* va = Vs + t.o[mt] + kb * 128;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(va));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(va + 8 * 128));
    const u32x2 lo2 = __builtin_bit_cast(u32x2, lo), hi2 = __builtin_bit_cast(u32x2, hi);
    const u32x4 pk = {lo2[0], lo2[1], hi2[0], hi2[1]};
    return __builtin_bit_cast(bf16x8, pk);
}

// ---- MXFP8 operands (attention_fp8.hip) ------------------------------------------------------------------
// v_mfma_scale_f32_32x32x64_f8f6f4 (layout measured with yv_mx_probe32, tests/test_gpu_attn_fp8.py::test_mx_mfma32_layout): lane
// (row / column rl = lane & 31, half hh = lane >> 5) holds K elements 16 hh .. + 15 in its first 16 bytes and 32 + 16 hh .. + 15 in
// its second 16 bytes, i.e. the 16-byte chunks hh and 2 + hh of a 64-byte row; the scale of the MX block j (k = 32 j .. + 31) of that
// row is byte `opsel` of the scale register of lane (rl, half j).  C/D as the 32x32x16 forms (key_of).
typedef __attribute__((ext_vector_type(8))) int i32x8;
__device__ __forceinline__ i32x8 mx_frag(const u32x4 lo, const u32x4 hi) {
    return i32x8{(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
}
// K image of e4m3 bytes: 64-byte rows of 4 chunks of 16 bytes, chunk c of row `row` at position c ^ ((row >> 2) & 3) (its own
// inverse).  A 16-lane group of ds_read_b128 ({0-3, 12-15, 20-27} / {4-11, 16-19, 28-31} and the same + 32) reads one chunk index of
// 16 rows: four rows of each row & 3 (which picks the 64-byte quarter of the 256-byte bank row), whose row >> 2 are {0, 3, 5, 6} /
// {1, 2, 4, 7} - distinct modulo 4, so the xor sends them to the four 16-byte slots of that quarter: conflict-free
// (tests/test_attn_fp8_cpu.py::test_k8_swizzle_is_conflict_free enumerates it).
__device__ __forceinline__ int k8_off(int row, int c) { return row * 64 + ((c ^ ((row >> 2) & 3)) << 4); }
// write side: slot i is chunk i & 3 of row i >> 2
__device__ __forceinline__ RowChunk row_chunk8(int i) { return {i >> 2, i & 3}; }
// where the two scale bytes of head hd's blocks of `row` live in a K-step-major scale array (kstep0: the K step of the tensor's
// column 0: 0 for Q, D / 128 for K, 2 D / 128 for V); 2-byte aligned, byte 0 = d 0..31, byte 1 = d 32..63
__device__ __forceinline__ long long mx_head_scales(int kstep0, int hd, long long rows_pad, long long row) {
    return mx_scale_kmajor((kstep0 << 2) + 2 * hd, rows_pad, row);
}
// Q (B operand) of query q with its scale register (block hh's byte in byte 0), straight from global: qb = the crop's Q bytes of
// this head, sq = the scale pair of the crop's row 0 (4 bytes per row); a query past N reads row N - 1
__device__ __forceinline__ void q8_frag(const uint8_t* qb, long long ld, const uint8_t* sq, int q, int N, int hh, i32x8& fq, int& sc) {
    const int qc = q < N ? q : N - 1;
    const uint8_t* p = qb + (size_t)qc * ld + hh * 16;
    fq = mx_frag(*(const u32x4*)p, *(const u32x4*)(p + 32));
    sc = sq[(size_t)qc * 4 + hh];
}
// S^T of the 32 keys whose rows start at row0 of the byte image Kimg; Ksc: the keys' scale pairs (2 bytes per key)
__device__ __forceinline__ f32x16 score_group8(const unsigned char* Kimg, const unsigned char* Ksc, int row0, const i32x8& fq, int sq,
                                               int rl, int hh) {
    f32x16 sv;
#pragma unroll
    for (int e = 0; e < 16; ++e) sv[e] = 0.f;
    const int row = row0 + rl;
    const i32x8 fk = mx_frag(*(const u32x4*)(Kimg + k8_off(row, hh)), *(const u32x4*)(Kimg + k8_off(row, 2 + hh)));
    const int sk = Ksc[2 * row + hh];
    return __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(fk, fq, sv, 0, 0, 0, sk, 0, sq);
}
// 2^(s - 127) of an E8M0 byte s <= 254 (s = 0: the f32 denormal 2^-127)
__device__ __forceinline__ float mx_scale_f32(uint32_t s) { return __uint_as_float(s ? s << 23 : 0x00400000u); }
// four e4m3 bytes at the block scale sf -> four bf16 (v_cvt_scalef32_pk_bf16_fp8: e4m3 * 2^e has 4 significant bits, exact in bf16
// wherever it is a bf16 normal)
__device__ __forceinline__ u32x2 mx_dequant4_bf16(uint32_t w, float sf) {
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const bf16x2_t lo = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, sf, false);
    const bf16x2_t hi = __builtin_amdgcn_cvt_scalef32_pk_bf16_fp8(w, sf, true);
    return u32x2{__builtin_bit_cast(uint32_t, lo), __builtin_bit_cast(uint32_t, hi)};
}
// 16 bytes of V row `row` (d = 16 c .. + 15, block c >> 1) -> the bf16 chunks 2 c and 2 c + 1 of the row-major V image
__device__ __forceinline__ void stash_v8(unsigned char* Vimg, int row, int c, const u32x4 bytes, float sf) {
    const u32x2 a = mx_dequant4_bf16(bytes[0], sf), b = mx_dequant4_bf16(bytes[1], sf);
    const u32x2 d = mx_dequant4_bf16(bytes[2], sf), e = mx_dequant4_bf16(bytes[3], sf);
    *(u32x4*)(Vimg + v_off(row, 2 * c)) = u32x4{a[0], a[1], b[0], b[1]};
    *(u32x4*)(Vimg + v_off(row, 2 * c + 1)) = u32x4{d[0], d[1], e[0], e[1]};
}

// ---- epilogue: query q < N of (crop r, head hd); inv = 1 / row sum ------------------------------------------------------------
// log2-sum-exp for the backward: mb = the row maximum * scale_log2e, l = the row sum
__device__ __forceinline__ void store_lse(float* lse, int r, int H, int hd, int N, int q, int hh, float mb, float l) {
    if (lse && hh == 0 && q < N) lse[((size_t)r * H + hd) * N + q] = mb + log2f(l);
}
// MXFP8 image: a head's 64 columns are two MX blocks (d 0..31 = mt 0, d 32..63 = mt 1); a query's values of one block sit in this
// lane and in lane ^ 32; the bf16 rounding of the ordinary output is kept; scale bytes K-step-major
__device__ __forceinline__ void store_mx(const f32x16 (&o)[2], float inv, const AttnMx& mx, int r, int N, int hd, int q, int hh) {
    const long long row = (long long)r * N + q;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt) {
        float f[16];
#pragma unroll
        for (int k = 0; k < 16; ++k) f[k] = bf16_to_f32(f32_to_bf16(o[mt][k] * inv));
        uint32_t p[4];
        const int e = mx_quant_block<32>(f, p);
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4) *(uint32_t*)(mx.q + row * mx.ldq + hd * HD + mt * 32 + 8 * g4 + 4 * hh) = p[g4];
        if (hh == 0) mx.s[mx_scale_kmajor(hd * 2 + mt, mx.rows, row)] = (uint8_t)(e + 127);
    }
}
// bf16 output, 16 bytes at a time: the 4-column groups (g4, g4 + 1), g4 even, are exchanged between the half-waves
// (v_permlane32_swap), so that this lane owns d = swapped_col .. + 7 of its query: the packet returned.  8 per query row.
__device__ __forceinline__ int swapped_col(int mt, int g4, int hh) { return mt * 32 + 8 * (g4 + hh); }
__device__ __forceinline__ u32x4 swapped_rows(const f32x16 (&o)[2], float inv, int mt, int g4) {
    const uint32_t a0 = pack_bf16x2(o[mt][4 * g4] * inv, o[mt][4 * g4 + 1] * inv);
    const uint32_t a1 = pack_bf16x2(o[mt][4 * g4 + 2] * inv, o[mt][4 * g4 + 3] * inv);
    const uint32_t b0 = pack_bf16x2(o[mt][4 * g4 + 4] * inv, o[mt][4 * g4 + 5] * inv);
    const uint32_t b1 = pack_bf16x2(o[mt][4 * g4 + 6] * inv, o[mt][4 * g4 + 7] * inv);
    const auto x0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
    const auto x1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
    return u32x4{x0[0], x1[0], x0[1], x1[1]};
}
// bf16 output, 8 bytes at a time, no exchange (attention_kernel): orow = the query's row of this head
__device__ __forceinline__ void store_direct(uint16_t* orow, const f32x16 (&o)[2], float inv, int hh) {
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g4 = 0; g4 < 4; ++g4)
            *(uint2*)(orow + mt * 32 + 8 * g4 + 4 * hh) = make_uint2(pack_bf16x2(o[mt][4 * g4] * inv, o[mt][4 * g4 + 1] * inv),
                                                                     pack_bf16x2(o[mt][4 * g4 + 2] * inv, o[mt][4 * g4 + 3] * inv));
}

}  // namespace
