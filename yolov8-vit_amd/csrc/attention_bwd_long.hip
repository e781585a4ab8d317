// Attention backward for sequences that do not fit one tile (ViT-B/8 at 224: 785 tokens; ViT-x/16 at 384: 577), head dim 64,
// non-causal: yv_attention_bwd_long.  DESIGN.md section 16.
//
// The algorithm and every element-wise expression are those of attention_bwd.hip (two kernels, no atomics, no cross-wave sums; P is
// recomputed from the forward's log2-sum-exp; P and dS reach the next MFMA from the accumulator registers), so dqkv and delta are
// bit-identical to yv_attention_bwd: a row's reduction walks the other axis in ascending 16-row MFMA steps inside one wave in both
// files, and a skipped or masked position contributes an exact zero.  The blocking and the staging are those of attention_long.hip:
//   * an owner workgroup is 4 waves x 32 rows = 128 rows of one (crop, head): queries in attn_bwdl_dq_kernel (writes dQ and delta),
//     keys in attn_bwdl_dkv_kernel (writes dK and dV).  The N % 128 rows left over go to a second launch whose workgroups have
//     ceil((N % 128) / 32) waves: no wave exists for a 32-row group that lies wholly past N;
//   * the other axis is walked in tiles of 64 rows (two 32-row groups; 32 in the one-wave workgroup) up to ceil(N / 32) groups: a
//     group wholly past N is skipped, only the group that straddles N is masked.  Rows past N are fetched from row N - 1 (finite;
//     their P and dS are exactly 0);
//   * tiles are double-buffered in LDS by register staging with the issue-early / write-late split: the global loads of tile t + 1
//     (and, in the dK/dV kernel, its lse / delta values) are issued in front of tile t's work and written to the other buffer
//     behind it, one barrier per tile.  Plain loads and 16-byte LDS stores: every wait is the compiler's;
//   * ONE image per tensor and tile serves the row reads (ds_read_b128: K and V for S^T and dP^T, Q and dO for S and dP) and the
//     transposed reads (ds_read_b64_tr_b16: K^T for dQ^T, Q^T and dO^T for dK^T and dV^T): 128-byte rows, 16-byte chunk c of row r
//     at chunk c ^ swz(r), swz(r) = ((r >> 1) & 1) << 2 | ((r >> 2) & 3).  That is a bit permutation of the (r >> 1) & 7 of
//     attention_long's K image, so the 16-lane groups of ds_read_b128 still meet eight different chunk positions per bank half; its
//     bit 2 is attention_long's V swizzle, so the 4 rows x 64 bytes that a 32-lane half of the transposed read takes cover all 64
//     banks once; the low bits only permute chunks inside such a 64-byte half row.  No 2-byte LDS store anywhere.
// 64-bit addressing throughout: no 2 GB limit on the tensors.
#include "yv_common.h"

namespace {

constexpr int HD = 64;

typedef __attribute__((ext_vector_type(4))) short bl_s16x4;
typedef __attribute__((address_space(3))) bl_s16x4* bl_lds_s16x4_t;

__device__ __forceinline__ int swz(int row) { return (((row >> 1) & 1) << 2) | ((row >> 2) & 3); }
// byte offset of 16-byte chunk c (0..7) of row `row` in a tile image
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
    const bl_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bl_lds_s16x4_t)(p + t.o[mt][0]));
    const bl_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((bl_lds_s16x4_t)(p + t.o[mt][1]));
    const u32x2 lo2 = __builtin_bit_cast(u32x2, lo), hi2 = __builtin_bit_cast(u32x2, hi);
    const u32x4 pk = {lo2[0], lo2[1], hi2[0], hi2[1]};
    return __builtin_bit_cast(bf16x8, pk);
}

// blockIdx.x = (crop * H + head) * QBL + (query block - qb0); a query block = 128 rows, of which this launch's workgroups hold the
// first NW * 32.  Wave owns 32 QUERIES (query on the lane): S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T * (dP^T - delta) * scale,
// dQ^T += K^T.dS^T; also emits delta[q] = sum_d dO * O for the second kernel.
template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwdl_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o,
                                                                  const uint16_t* __restrict__ dout, const float* __restrict__ lse,
                                                                  int N, int H, int qb0, int QBL, float scale, float scale_log2e,
                                                                  uint16_t* __restrict__ dqkv, float* __restrict__ delta) {
    constexpr int KT = NW == 1 ? 32 : 64, GPT = KT / 32;
    constexpr int TILE = KT * 128;                       // bytes of a K (or V) tile
    constexpr int T = NW * 64;
    constexpr int CH = KT * 8;                           // 16-byte chunks of one tensor's tile
    constexpr int TRIPS = (CH + T - 1) / T;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILE];       // [buffer][K | V]
    const int rh = blockIdx.x / QBL;
    const int qb = qb0 + (blockIdx.x - rh * QBL);
    const int r = rh / H, hd = rh - r * H;
    const int D = H * HD, ld = 3 * D;
    const uint16_t* base = qkv + (size_t)r * N * ld + hd * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 31, hh = lane >> 5;
    const int q = qb * 128 + wave * 32 + rl, qc = q < N ? q : N - 1;
    const uint16_t* orow = o + ((size_t)r * N + qc) * D + hd * HD;
    const uint16_t* drow = dout + ((size_t)r * N + qc) * D + hd * HD;
    bf16x8 fq[4], fdo[4];
    float dl = 0.f;
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
    float lq = lse[((size_t)r * H + hd) * N + qc];

    u32x4 kst[TRIPS], vst[TRIPS];
    auto fetch = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            const int kl = (it < CH ? it : CH - 1) >> 3, c = it & 7;
            int key = t * KT + kl;
            key = key < N ? key : N - 1;
            const uint16_t* p = base + (size_t)key * ld + D + c * 8;
            kst[i] = *(const u32x4*)p;
            vst[i] = *(const u32x4*)(p + D);
        }
    };
    auto stash = [&](int buf) __attribute__((always_inline)) {
        unsigned char* Kb = smem + buf * 2 * TILE;
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            if (CH % T != 0 && it >= CH) break;
            const int off = img_off(it >> 3, it & 7);
            *(u32x4*)(Kb + off) = kst[i];
            *(u32x4*)(Kb + TILE + off) = vst[i];
        }
    };
    const TrOff tro = tr_offsets(lane);

    f32x16 acc[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[mt][e] = 0.f;

    const int G = (N + 31) >> 5;                         // live 32-key groups
    const int NTILE = (G + GPT - 1) / GPT;
    fetch(0);
    stash(0);
    // the owner's fragments and row constants are complete BEFORE the loop (attention_long.hip): left pending, their first use
    // inside it would drain the fetch of tile t + 1 in every iteration
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(fq[ks]), "+v"(fdo[ks]));
    asm volatile("" : "+v"(dl), "+v"(lq));
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < NTILE; ++t) {
        const bool more = t + 1 < NTILE;
        if (more) fetch(t + 1);                          // in flight under this tile's MFMA and exp work
        const unsigned char* Ks = smem + (t & 1) * 2 * TILE;
        const unsigned char* Vs = Ks + TILE;
#pragma unroll
        for (int gl = 0; gl < GPT; ++gl) {
            const int g = GPT * t + gl;
            if (g >= G) break;                           // wholly past N (wave- and block-uniform)
            f32x16 s, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) s[e] = dp[e] = 0.f;
            const int row = gl * 32 + rl;
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
                    acc[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Ks, tro, mt, gl * 32 + 16 * st), fp, acc[mt], 0, 0, 0);
            }
        }
        if (more) stash((t + 1) & 1);                    // that buffer's last readers passed the previous barrier
        __syncthreads();
    }
    if (q < N) {
        uint16_t* dst = dqkv + ((size_t)r * N + q) * ld + hd * HD;
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int g4 = 0; g4 < 4; ++g4)
                *(uint2*)(dst + mt * 32 + 8 * g4 + 4 * hh) =
                    make_uint2(pack_bf16x2(acc[mt][4 * g4], acc[mt][4 * g4 + 1]), pack_bf16x2(acc[mt][4 * g4 + 2], acc[mt][4 * g4 + 3]));
    }
}

// blockIdx.x = (crop * H + head) * KBL + (key block - kb0).  Wave owns 32 KEYS (key on the lane): S = Q.K^T, dP = dO.V^T, then
// dV^T += dO^T.P and dK^T += Q^T.dS with P / dS taken from the accumulator registers as the B operand.
template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attn_bwdl_dkv_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout,
                                                                   const float* __restrict__ lse, const float* __restrict__ delta,
                                                                   int N, int H, int kb0, int KBL, float scale, float scale_log2e,
                                                                   uint16_t* __restrict__ dqkv) {
    constexpr int QT = NW == 1 ? 32 : 64, GPT = QT / 32;
    constexpr int TILE = QT * 128;                       // bytes of a Q (or dO) tile
    constexpr int T = NW * 64;
    constexpr int CH = QT * 8;
    constexpr int TRIPS = (CH + T - 1) / T;
    static_assert(2 * QT <= T, "one thread per staged lse / delta value");
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILE];       // [buffer][Q | dO]
    __shared__ __attribute__((aligned(16))) float rows_s[2][2 * QT];            // [buffer][lse | delta]
    const int rh = blockIdx.x / KBL;
    const int kb = kb0 + (blockIdx.x - rh * KBL);
    const int r = rh / H, hd = rh - r * H;
    const int D = H * HD, ld = 3 * D;
    const uint16_t* base = qkv + (size_t)r * N * ld + hd * HD;
    const uint16_t* dbase = dout + (size_t)r * N * D + hd * HD;
    const float* lrow = lse + ((size_t)r * H + hd) * N;
    const float* erow = delta + ((size_t)r * H + hd) * N;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 31, hh = lane >> 5;
    const int key = kb * 128 + wave * 32 + rl, kc = key < N ? key : N - 1;
    bf16x8 fk[4], fv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        fk[ks] = *(const bf16x8*)(base + (size_t)kc * ld + D + ks * 16 + hh * 8);
        fv[ks] = *(const bf16x8*)(base + (size_t)kc * ld + 2 * D + ks * 16 + hh * 8);
    }

    u32x4 qst[TRIPS], ost[TRIPS];
    float rst = 0.f;
    auto fetch = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            const int ql = (it < CH ? it : CH - 1) >> 3, c = it & 7;
            int qq = t * QT + ql;
            qq = qq < N ? qq : N - 1;
            qst[i] = *(const u32x4*)(base + (size_t)qq * ld + c * 8);
            ost[i] = *(const u32x4*)(dbase + (size_t)qq * D + c * 8);
        }
        if (tid < 2 * QT) {
            int qq = t * QT + (tid < QT ? tid : tid - QT);
            qq = qq < N ? qq : N - 1;
            rst = (tid < QT ? lrow : erow)[qq];
        }
    };
    auto stash = [&](int buf) __attribute__((always_inline)) {
        unsigned char* Qb = smem + buf * 2 * TILE;
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            if (CH % T != 0 && it >= CH) break;
            const int off = img_off(it >> 3, it & 7);
            *(u32x4*)(Qb + off) = qst[i];
            *(u32x4*)(Qb + TILE + off) = ost[i];
        }
        if (tid < 2 * QT) rows_s[buf][tid] = rst;
    };
    const TrOff tro = tr_offsets(lane);

    f32x16 dk[2], dv[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) dk[mt][e] = dv[mt][e] = 0.f;

    const int G = (N + 31) >> 5;                         // live 32-query groups
    const int NTILE = (G + GPT - 1) / GPT;
    fetch(0);
    stash(0);
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(fk[ks]), "+v"(fv[ks]));
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < NTILE; ++t) {
        const bool more = t + 1 < NTILE;
        if (more) fetch(t + 1);
        const unsigned char* Qs = smem + (t & 1) * 2 * TILE;
        const unsigned char* Os = Qs + TILE;
        const float* lse_s = rows_s[t & 1];
        const float* del_s = lse_s + QT;
#pragma unroll
        for (int gl = 0; gl < GPT; ++gl) {
            const int g = GPT * t + gl;
            if (g >= G) break;                           // wholly past N (wave- and block-uniform)
            f32x16 sv, dp;
#pragma unroll
            for (int e = 0; e < 16; ++e) sv[e] = dp[e] = 0.f;
            const int row = gl * 32 + rl;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Qs, row, 2 * ks + hh), fk[ks], sv, 0, 0, 0);
                dp = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_rows(Os, row, 2 * ks + hh), fv[ks], dp, 0, 0, 0);
            }
            if (g * 32 + 32 > N) {                       // the group that straddles N
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ql = gl * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                    const bool ok = g * 32 - gl * 32 + ql < N;
                    const float pv = ok ? exp2f(sv[e] * scale_log2e - lse_s[ql]) : 0.f;
                    sv[e] = pv;
                    dp[e] = pv * (dp[e] - del_s[ql]) * scale;
                }
            } else {
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int ql = gl * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
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
                    dv[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Os, tro, mt, gl * 32 + 16 * st), fp, dv[mt], 0, 0, 0);
                    dk[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(frag_tr(Qs, tro, mt, gl * 32 + 16 * st), fs, dk[mt], 0, 0, 0);
                }
            }
        }
        if (more) stash((t + 1) & 1);
        __syncthreads();
    }
    if (key < N) {
        uint16_t* dst = dqkv + ((size_t)r * N + key) * ld + hd * HD;
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

struct BwdArgs {
    const uint16_t* qkv; const uint16_t* o; const uint16_t* dout; const float* lse;
    int R, N, H;
    float scale;
    uint16_t* dqkv; float* delta;
    hipStream_t st;
};

template <int NW>
int launch_dq(const BwdArgs& a, int b0, int BL) {
    hipLaunchKernelGGL(attn_bwdl_dq_kernel<NW>, dim3(a.R * a.H * BL), dim3(NW * 64), 0, a.st, a.qkv, a.o, a.dout, a.lse, a.N, a.H, b0,
                       BL, a.scale, a.scale * 1.4426950408889634f, a.dqkv, a.delta);
    return yv_launch_status();
}
template <int NW>
int launch_dkv(const BwdArgs& a, int b0, int BL) {
    hipLaunchKernelGGL(attn_bwdl_dkv_kernel<NW>, dim3(a.R * a.H * BL), dim3(NW * 64), 0, a.st, a.qkv, a.dout, a.lse, a.delta, a.N,
                       a.H, b0, BL, a.scale, a.scale * 1.4426950408889634f, a.dqkv);
    return yv_launch_status();
}

// whole 128-row owner blocks, then the rows past the last whole block with only their live waves
template <bool DQ>
int launch_axis(const BwdArgs& a) {
    const int full = a.N / 128, rem = a.N - full * 128;
    if (full > 0) {
        const int rc = DQ ? launch_dq<4>(a, 0, full) : launch_dkv<4>(a, 0, full);
        if (rc != YV_OK) return rc;
    }
    switch ((rem + 31) / 32) {
        case 0: return YV_OK;
        case 1: return DQ ? launch_dq<1>(a, full, 1) : launch_dkv<1>(a, full, 1);
        case 2: return DQ ? launch_dq<2>(a, full, 1) : launch_dkv<2>(a, full, 1);
        case 3: return DQ ? launch_dq<3>(a, full, 1) : launch_dkv<3>(a, full, 1);
        default: return DQ ? launch_dq<4>(a, full, 1) : launch_dkv<4>(a, full, 1);
    }
}

}  // namespace

extern "C" int yv_attention_bwd_long(const void* qkv, const void* out, const void* dout, const float* lse, int R, int N, int H,
                                     float scale, void* dqkv, float* delta_ws, void* stream) {
    if (!qkv || !out || !dout || !lse || !dqkv || !delta_ws || R < 0 || N <= 0 || H <= 0) return YV_ERR_ARG;
    if (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)dout | (uintptr_t)dqkv) & 15) return YV_ERR_ARG;      // 16-byte row chunks
    if (((uintptr_t)lse | (uintptr_t)delta_ws) & 3) return YV_ERR_ARG;
    const int QB = (N + 127) / 128;
    if ((long long)R * H * QB > 0x7fffffffLL) return YV_ERR_LIMIT;
    if (R == 0) return YV_OK;
    const BwdArgs a{(const uint16_t*)qkv, (const uint16_t*)out, (const uint16_t*)dout, lse, R, N, H, scale,
                    (uint16_t*)dqkv, delta_ws, (hipStream_t)stream};
    const int rc = launch_axis<true>(a);                   // dQ and delta first: the dK/dV kernels read delta
    return rc != YV_OK ? rc : launch_axis<false>(a);
}
