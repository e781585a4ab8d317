// Attention backward for sequences of up to 224 tokens (ViT-x/16 at 224: 197), head dim 64, non-causal, in ONE launch:
// yv_attention_bwd_short.  DESIGN.md section 23.
//
// At N <= 224 the whole (crop, head) problem fits a CU: Q, K, V and dO are 4 x NP x 128 bytes (NP = 32 NT rows, NT = ceil(N / 32);
// 114,688 bytes at NT = 7).  The workgroup that owns every query also owns every key, so the two kernels of attention_bwd.hip are
// two PHASES of one workgroup of NT waves over images that are fetched once:
//   phase 1  wave owns 32 QUERIES (query on the lane): S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T * (dP^T - delta) * scale,
//            dQ^T += K^T.dS^T; writes dQ and delta, and hands lse / delta to phase 2 through LDS;
//   phase 2  wave owns 32 KEYS (key on the lane): S = Q.K^T, dP = dO.V^T, dV^T += dO^T.P, dK^T += Q^T.dS; its K / V fragments
//            are row reads of the K / V images.
// The arithmetic and every element-wise expression are those of attention_bwd.hip (seven products, P recomputed from the forward's
// log2-sum-exp, P and dS fed to the next MFMA from the accumulator registers, no cross-wave sums, no atomics), and a row's
// reduction walks the other axis in ascending 16-row MFMA steps inside one wave, so dqkv and delta are bit-identical to
// yv_attention_bwd.  Rows NP > row >= N of every image are zeros: their P and dS are exactly 0.
//   * K and V are fetched first (registers, then ds_write_b128); the fetch of Q and dO is issued right behind them and is written
//     to its own LDS region only after phase 1, so it lands under phase 1's MFMA and exp work.  Plain loads: every wait is the
//     compiler's.
//   * ONE image per tensor serves the row reads (ds_read_b128) and the transposed reads (ds_read_b64_tr_b16): the layout and the
//     swizzle of attention_bwd_long.hip, 128-byte rows with 16-byte chunk c of row r at chunk c ^ swz(r).  swz reads row bits
//     1 .. 3 only, and the transposed reads start at multiples of 16 rows, so a taller image changes none of its premises.
//     No 2-byte LDS store anywhere.
//   * One (crop, head) item per workgroup: 116,480 bytes of LDS are one workgroup per CU whatever a workgroup walks, so the number
//     of rounds is ceil(R H / CUs) either way (section 23.4).
// 64-bit addressing throughout: no 2 GB limit on the tensors.
#include "yv_common.h"

namespace {

constexpr int HD = 64;

typedef __attribute__((ext_vector_type(4))) short bs_s16x4;
typedef __attribute__((address_space(3))) bs_s16x4* bs_lds_s16x4_t;

__device__ __forceinline__ int swz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }
// byte offset of 16-byte chunk c (0..7) of row `row` in an image
__device__ __forceinline__ int img_off(int row, int c) { return row * 128 + ((c ^ swz(row)) << 4); }

__device__ __forceinline__ bf16x8 frag_rows(const unsigned char* img, int row, int chunk) {
    return *(const bf16x8*)(img + img_off(row, chunk));
}

// Lane offsets of the transposed A fragment (attention_bwd_long.hip): 16-lane group G = lane >> 4 takes d columns
// 32 mt + (G & 1) * 16 .. + 15 of the rows r0 + 4 (G >> 1) + q (first read) and 8 rows further (second read); lane 4 q + p of the
// group addresses row q, columns 4 p .. 4 p + 3.  r0 is a multiple of 16, so swz does not depend on it.
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
    const bs_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bs_lds_s16x4_t)(p + t.o[mt][0]));
    const bs_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bs_lds_s16x4_t)(p + t.o[mt][1]));
    const u32x2 lo2 = __builtin_bit_cast(u32x2, lo), hi2 = __builtin_bit_cast(u32x2, hi);
    const u32x4 pk = {lo2[0], lo2[1], hi2[0], hi2[1]};
    return __builtin_bit_cast(bf16x8, pk);
}

// blockIdx.x = crop * H + head.  NT waves; wave w owns rows 32 w .. 32 w + 31 of the item on both axes.
template <int NT>
__global__ __launch_bounds__(NT * 64) void attn_bwds_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o,
                                                            const uint16_t* __restrict__ dout, const float* __restrict__ lse,
                                                            int N, int H, float scale, float scale_log2e,
                                                            uint16_t* __restrict__ dqkv, float* __restrict__ delta) {
    constexpr int NP = NT * 32, T = NT * 64;
    constexpr int IMG = NP * 128;                        // bytes of one tensor's image
    constexpr int TRIPS = 4;                             // NP * 8 chunks of 16 bytes / T threads
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* Ks = smem;
    unsigned char* Vs = smem + IMG;
    unsigned char* Qs = smem + 2 * IMG;
    unsigned char* Os = smem + 3 * IMG;
    float* lse_s = (float*)(smem + 4 * IMG);
    float* del_s = lse_s + NP;
    const int rh = blockIdx.x;
    const int r = rh / H, hd = rh - r * H;
    const int D = H * HD, ld = 3 * D;
    const uint16_t* base = qkv + (size_t)r * N * ld + hd * HD;
    const uint16_t* dbase = dout + (size_t)r * N * D + hd * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 31, hh = lane >> 5;
    const int own = wave * 32 + rl;                      // this lane's query (phase 1) and key (phase 2)
    const int oc = own < N ? own : N - 1;

    // K and V first, then the owner's query-side rows, then Q and dO (written to LDS after phase 1)
    u32x4 kst[TRIPS], vst[TRIPS], qst[TRIPS], ost[TRIPS];
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        const int it = tid + i * T, row = it >> 3, c = it & 7;
        kst[i] = vst[i] = u32x4{0, 0, 0, 0};
        if (row < N) {
            const uint16_t* p = base + (size_t)row * ld + D + c * 8;
            kst[i] = *(const u32x4*)p;
            vst[i] = *(const u32x4*)(p + D);
        }
    }
    const uint16_t* orow = o + ((size_t)r * N + oc) * D + hd * HD;
    const uint16_t* drow = dbase + (size_t)oc * D;
    bf16x8 fq[4], fdo[4];
    float dl = 0.f;
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        fq[ks] = *(const bf16x8*)(base + (size_t)oc * ld + ks * 16 + hh * 8);
        fdo[ks] = *(const bf16x8*)(drow + ks * 16 + hh * 8);
        const bf16x8 fo = *(const bf16x8*)(orow + ks * 16 + hh * 8);
#pragma unroll
        for (int j = 0; j < 8; ++j) dl += (float)fdo[ks][j] * (float)fo[j];
    }
    dl += __shfl_xor(dl, 32, 64);
    if (own < N && hh == 0) delta[((size_t)r * H + hd) * N + own] = dl;
    float lq = lse[((size_t)r * H + hd) * N + oc];
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        const int it = tid + i * T, row = it >> 3, c = it & 7;
        qst[i] = ost[i] = u32x4{0, 0, 0, 0};
        if (row < N) {
            qst[i] = *(const u32x4*)(base + (size_t)row * ld + c * 8);
            ost[i] = *(const u32x4*)(dbase + (size_t)row * D + c * 8);
        }
    }
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        const int it = tid + i * T;
        const int off = img_off(it >> 3, it & 7);
        *(u32x4*)(Ks + off) = kst[i];
        *(u32x4*)(Vs + off) = vst[i];
    }
    // the owner's fragments and row constants are complete BEFORE the loop (attention_bwd_long.hip): left pending, their first
    // use inside it would wait for the fetch of Q and dO as well
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(fq[ks]), "+v"(fdo[ks]));
    asm volatile("" : "+v"(dl), "+v"(lq));
    const TrOff tro = tr_offsets(lane);
    __syncthreads();

    // ---- phase 1: dQ (query on the lane) ----------------------------------------------------------------------------------------
    {
        f32x16 acc[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 16; ++e) acc[mt][e] = 0.f;
#pragma unroll 1
        for (int g = 0; g < NT; ++g) {
            f32x16 s, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
            const int row = g * 32 + rl;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                s = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Ks, row, 2 * ks + hh), fq[ks], s, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Vs, row, 2 * ks + hh), fdo[ks], dp, 0, 0, 0);
            }
            // dS^T = P^T * (dP^T - delta) * scale with P^T = exp2(S^T*c - lse[q])
            if (g * 32 + 32 > N) {                       // the group that straddles N
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = g * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                    const float pv = key < N ? exp2f(s[e] * scale_log2e - lq) : 0.f;
                    s[e] = pv * (dp[e] - dl) * scale;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float pv = exp2f(s[e] * scale_log2e - lq);
                    s[e] = pv * (dp[e] - dl) * scale;
                }
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                bf16x8 fp;
#pragma unroll
                for (int j = 0; j < 8; ++j) fp[j] = (__bf16)s[8 * st + j];
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Ks, tro, mt, g * 32 + 16 * st), fp, acc[mt], 0, 0, 0);
            }
        }
        if (own < N) {
            uint16_t* dst = dqkv + ((size_t)r * N + own) * ld + hd * HD;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int g4 = 0; g4 < 4; ++g4)
                    *(uint2*)(dst + mt * 32 + 8 * g4 + 4 * hh) =
                        make_uint2(pack_bf16x2(acc[mt][4 * g4], acc[mt][4 * g4 + 1]), pack_bf16x2(acc[mt][4 * g4 + 2], acc[mt][4 * g4 + 3]));
        }
    }

    // ---- hand-over: Q / dO images and the per-query constants; the key-side fragments of this wave from the K / V images -------
#pragma unroll
    for (int i = 0; i < TRIPS; ++i) {
        const int it = tid + i * T;
        const int off = img_off(it >> 3, it & 7);
        *(u32x4*)(Qs + off) = qst[i];
        *(u32x4*)(Os + off) = ost[i];
    }
    if (hh == 0) {
        lse_s[own] = own < N ? lq : 0.f;
        del_s[own] = own < N ? dl : 0.f;
    }
    bf16x8 fk[4], fv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        fk[ks] = frag_rows(Ks, own, 2 * ks + hh);
        fv[ks] = frag_rows(Vs, own, 2 * ks + hh);
    }
    __syncthreads();

    // ---- phase 2: dK and dV (key on the lane) -----------------------------------------------------------------------------------
    f32x16 dk[2], dv[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) dk[mt][e] = dv[mt][e] = 0.f;
#pragma unroll 1
    for (int g = 0; g < NT; ++g) {
        f32x16 sv, dp;
#pragma unroll
        for (int e = 0; e < 16; ++e) sv[e] = dp[e] = 0.f;
        const int row = g * 32 + rl;
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) {
            sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Qs, row, 2 * ks + hh), fk[ks], sv, 0, 0, 0);
            dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Os, row, 2 * ks + hh), fv[ks], dp, 0, 0, 0);
        }
        if (g * 32 + 32 > N) {                           // the group that straddles N
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ql = g * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                const float pv = ql < N ? exp2f(sv[e] * scale_log2e - lse_s[ql]) : 0.f;
                sv[e] = pv;
                dp[e] = pv * (dp[e] - del_s[ql]) * scale;
            }
        } else {
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const int ql = g * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                const float pv = exp2f(sv[e] * scale_log2e - lse_s[ql]);
                sv[e] = pv;
                dp[e] = pv * (dp[e] - del_s[ql]) * scale;
            }
        }
#pragma unroll
        for (int st = 0; st < 2; ++st) {
            bf16x8 fp, fs;
#pragma unroll
            for (int j = 0; j < 8; ++j) { fp[j] = (__bf16)sv[8 * st + j]; fs[j] = (__bf16)dp[8 * st + j]; }
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                dv[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Os, tro, mt, g * 32 + 16 * st), fp, dv[mt], 0, 0, 0);
                dk[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qs, tro, mt, g * 32 + 16 * st), fs, dk[mt], 0, 0, 0);
            }
        }
    }
    if (own < N) {
        uint16_t* dst = dqkv + ((size_t)r * N + own) * ld + hd * HD;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4) {
                const int d = mt * 32 + 8 * g4 + 4 * hh;
                *(uint2*)(dst + D + d) = make_uint2(pack_bf16x2(dk[mt][4 * g4], dk[mt][4 * g4 + 1]),
                                                    pack_bf16x2(dk[mt][4 * g4 + 2], dk[mt][4 * g4 + 3]));
                *(uint2*)(dst + 2 * D + d) = make_uint2(pack_bf16x2(dv[mt][4 * g4], dv[mt][4 * g4 + 1]),
                                                        pack_bf16x2(dv[mt][4 * g4 + 2], dv[mt][4 * g4 + 3]));
            }
    }
}

template <int NT>
int launch_bwds(const uint16_t* qkv, const uint16_t* o, const uint16_t* dout, const float* lse, int R, int N, int H, float scale,
                uint16_t* dqkv, float* delta, hipStream_t st) {
    constexpr int NP = NT * 32;
    const size_t lds = (size_t)4 * NP * 128 + 2 * NP * 4;
    auto k = attn_bwds_kernel<NT>;
    if (!yv_grant_lds((const void*)k, lds)) return YV_ERR_LAUNCH;
    hipLaunchKernelGGL(k, dim3(R * H), dim3(NT * 64), lds, st, qkv, o, dout, lse, N, H, scale, scale * 1.4426950408889634f, dqkv,
                       delta);
    return yv_launch_status();
}

}  // namespace

extern "C" int yv_attention_bwd_short(const void* qkv, const void* out, const void* dout, const float* lse, int R, int N, int H,
                                      float scale, void* dqkv, float* delta_ws, void* stream) {
    if (!qkv || !out || !dout || !lse || !dqkv || !delta_ws || R < 0 || N <= 0 || H <= 0) return YV_ERR_ARG;
    if (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv) & 15) return YV_ERR_ARG;      // 16-byte row chunks
    if (((uintptr_t)lse | (uintptr_t)delta_ws) & 3) return YV_ERR_ARG;
    if (N > 224) return YV_ERR_LIMIT;                      // one (crop, head) item = one workgroup's LDS
    if ((long long)R * H > 0x7fffffffLL) return YV_ERR_LIMIT;
    if (R == 0) return YV_OK;
    const uint16_t* q = (const uint16_t*)qkv;
    const uint16_t* o = (const uint16_t*)out;
    const uint16_t* d = (const uint16_t*)dout;
    uint16_t* g = (uint16_t*)dqkv;
    hipStream_t st = (hipStream_t)stream;
    switch ((N + 31) / 32) {
        case 1: return launch_bwds<1>(q, o, d, lse, R, N, H, scale, g, delta_ws, st);
        case 2: return launch_bwds<2>(q, o, d, lse, R, N, H, scale, g, delta_ws, st);
        case 3: return launch_bwds<3>(q, o, d, lse, R, N, H, scale, g, delta_ws, st);
        case 4: return launch_bwds<4>(q, o, d, lse, R, N, H, scale, g, delta_ws, st);
        case 5: return launch_bwds<5>(q, o, d, lse, R, N, H, scale, g, delta_ws, st);
        case 6: return launch_bwds<6>(q, o, d, lse, R, N, H, scale, g, delta_ws, st);
        default: return launch_bwds<7>(q, o, d, lse, R, N, H, scale, g, delta_ws, st);
    }
}
