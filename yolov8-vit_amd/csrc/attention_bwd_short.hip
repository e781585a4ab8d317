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
// The arithmetic is the text that attention_bwd.hip compiles, attention_bwd_core.h (seven products, P recomputed from the forward's
// log2-sum-exp, P and dS fed to the next MFMA from the accumulator registers, no cross-wave sums, no atomics), and a row's
// reduction walks the other axis in ascending 16-row MFMA steps inside one wave, so dqkv and delta are bit-identical to
// yv_attention_bwd.  Rows NP > row >= N of every image are zeros: their P and dS are exactly 0.  This file holds the phases' order,
// the staging and the launch.
//   * K and V are fetched first (registers, then ds_write_b128); the fetch of Q and dO is issued right behind them and is written
//     to its own LDS region only after phase 1, so it lands under phase 1's MFMA and exp work.  Plain loads: every wait is the
//     compiler's.
//   * ONE image per tensor serves the row reads (ds_read_b128) and the transposed reads (ds_read_b64_tr_b16): the SwizzledImage
//     of the header, as in attention_bwd_long.hip, 128-byte rows with 16-byte chunk c of row r at chunk c ^ swz(r).  swz reads row bits
//     1 .. 3 only, and the transposed reads start at multiples of 16 rows, so a taller image changes none of its premises.
//     No 2-byte LDS store anywhere.
//   * One (crop, head) item per workgroup: 116,480 bytes of LDS are one workgroup per CU whatever a workgroup walks, so the number
//     of rounds is ceil(R H / CUs) either way (section 23.4).
// 64-bit addressing throughout: no 2 GB limit on the tensors.
#include "attention_bwd_core.h"

namespace {

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
    const SwizzledImage lay(lane);
    const int hh = lay.hh;
    const int own = wave * 32 + lay.rl;                  // this lane's query (phase 1) and key (phase 2)

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
    bf16x8 fq[4], fdo[4];
    float dl, lq;
    owner_query(base, o, dout, lse, delta, r, hd, N, H, own, hh, fq, fdo, dl, lq);
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
    __syncthreads();

    // ---- phase 1: dQ (query on the lane) ----------------------------------------------------------------------------------------
    {
        f32x16 acc[2];
        zero(acc);
#pragma unroll 1
        for (int g = 0; g < NT; ++g) dq_group(lay, Ks, Vs, g * 32, g * 32, N, fq, fdo, lq, dl, scale, scale_log2e, acc);
        if (own < N) store_dq(dqkv, (size_t)r * N + own, hd, H, hh, acc);
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
    zero(dk);
    zero(dv);
#pragma unroll 1
    for (int g = 0; g < NT; ++g) dkv_group(lay, Qs, Os, lse_s, del_s, g * 32, g * 32, N, fk, fv, scale, scale_log2e, dk, dv);
    if (own < N) store_dkv(dqkv, (size_t)r * N + own, hd, H, hh, dk, dv);
}

template <int NT>
int launch_bwds(const BwdArgs& a) {
    constexpr int NP = NT * 32;
    const size_t lds = (size_t)4 * NP * 128 + 2 * NP * 4;
    auto k = attn_bwds_kernel<NT>;
    if (!yv_grant_lds((const void*)k, lds)) return YV_ERR_LAUNCH;
    hipLaunchKernelGGL(k, dim3(a.R * a.H), dim3(NT * 64), lds, a.st, a.qkv, a.o, a.dout, a.lse, a.N, a.H, a.scale, a.scale * LOG2E,
                       a.dqkv, a.delta);
    return yv_launch_status();
}

}  // namespace

extern "C" int yv_attention_bwd_short(const void* qkv, const void* out, const void* dout, const float* lse, int R, int N, int H,
                                      float scale, void* dqkv, float* delta_ws, void* stream) {
    const BwdArgs a = bwd_args(qkv, out, dout, lse, R, N, H, scale, dqkv, delta_ws, stream);
    const int ok = bwd_args_check(a, 1);                   // one workgroup per (crop, head)
    if (ok != YV_OK) return ok;
    if (N > 224) return YV_ERR_LIMIT;                      // one (crop, head) item = one workgroup's LDS
    if (R == 0) return YV_OK;
    switch ((N + 31) / 32) {
        case 1: return launch_bwds<1>(a);
        case 2: return launch_bwds<2>(a);
        case 3: return launch_bwds<3>(a);
        case 4: return launch_bwds<4>(a);
        case 5: return launch_bwds<5>(a);
        case 6: return launch_bwds<6>(a);
        default: return launch_bwds<7>(a);
    }
}
