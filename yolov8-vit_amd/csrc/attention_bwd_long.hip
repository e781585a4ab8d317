// Attention backward for sequences that do not fit one tile (ViT-B/8 at 224: 785 tokens; ViT-x/16 at 384: 577), head dim 64,
// non-causal: yv_attention_bwd_long.  DESIGN.md section 16.
//
// The algorithm is that of attention_bwd.hip (two kernels, no atomics, no cross-wave sums; P is recomputed from the forward's
// log2-sum-exp; P and dS reach the next MFMA from the accumulator registers) and the arithmetic is the same text,
// attention_bwd_core.h, so dqkv and delta are bit-identical to yv_attention_bwd: a row's reduction walks the other axis in ascending
// 16-row MFMA steps inside one wave in both files, and a skipped or masked position contributes an exact zero.  This file holds the
// blocking and the staging, which are those of attention_long.hip:
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
//     transposed reads (ds_read_b64_tr_b16: K^T for dQ^T, Q^T and dO^T for dK^T and dV^T): the SwizzledImage of the header,
//     16-byte chunk c of row r at chunk c ^ swz(r).  swz is a bit permutation of the (r >> 1) & 7 of attention_long's K image, so
//     the 16-lane groups of ds_read_b128 still meet eight different chunk positions per bank half; its bit 2 is attention_long's
//     V swizzle, so the 4 rows x 64 bytes that a 32-lane half of the transposed read takes cover all 64 banks once; the low bits
//     only permute chunks inside such a 64-byte half row.  No 2-byte LDS store anywhere.
// 64-bit addressing throughout: no 2 GB limit on the tensors.
#include "attention_bwd_core.h"

namespace {

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
    const SwizzledImage lay(lane);
    const int q = qb * 128 + wave * 32 + lay.rl;
    bf16x8 fq[4], fdo[4];
    float dl, lq;
    owner_query(base, o, dout, lse, delta, r, hd, N, H, q, lay.hh, fq, fdo, dl, lq);

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

    f32x16 acc[2];
    zero(acc);

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
            dq_group(lay, Ks, Vs, gl * 32, g * 32, N, fq, fdo, lq, dl, scale, scale_log2e, acc);
        }
        if (more) stash((t + 1) & 1);                    // that buffer's last readers passed the previous barrier
        __syncthreads();
    }
    if (q < N) store_dq(dqkv, (size_t)r * N + q, hd, H, lay.hh, acc);
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
    const SwizzledImage lay(lane);
    const int hh = lay.hh;
    const int key = kb * 128 + wave * 32 + lay.rl, kc = key < N ? key : N - 1;
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

    f32x16 dk[2], dv[2];
    zero(dk);
    zero(dv);

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
            dkv_group(lay, Qs, Os, lse_s, del_s, gl * 32, g * 32, N, fk, fv, scale, scale_log2e, dk, dv);
        }
        if (more) stash((t + 1) & 1);
        __syncthreads();
    }
    if (key < N) store_dkv(dqkv, (size_t)r * N + key, hd, H, hh, dk, dv);
}

template <int NW>
int launch_dq(const BwdArgs& a, int b0, int BL) {
    hipLaunchKernelGGL(attn_bwdl_dq_kernel<NW>, dim3(a.R * a.H * BL), dim3(NW * 64), 0, a.st, a.qkv, a.o, a.dout, a.lse, a.N, a.H, b0,
                       BL, a.scale, a.scale * LOG2E, a.dqkv, a.delta);
    return yv_launch_status();
}
template <int NW>
int launch_dkv(const BwdArgs& a, int b0, int BL) {
    hipLaunchKernelGGL(attn_bwdl_dkv_kernel<NW>, dim3(a.R * a.H * BL), dim3(NW * 64), 0, a.st, a.qkv, a.dout, a.lse, a.delta, a.N,
                       a.H, b0, BL, a.scale, a.scale * LOG2E, a.dqkv);
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
    const BwdArgs a = bwd_args(qkv, out, dout, lse, R, N, H, scale, dqkv, delta_ws, stream);
    const int ok = bwd_args_check(a, (N + 127) / 128);     // a launch has at most R * H * ceil(N / 128) workgroups
    if (ok != YV_OK || R == 0) return ok;
    const int rc = launch_axis<true>(a);                   // dQ and delta first: the dK/dV kernels read delta
    return rc != YV_OK ? rc : launch_axis<false>(a);
}
