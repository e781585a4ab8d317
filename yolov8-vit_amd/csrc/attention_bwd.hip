// Attention backward (flash-style recompute; 197 tokens = one tile, 785 tokens = 256-row tiles; head dim 64) for the ViT
// fine-tune step (timm Attention, README.md:21-23).
//
// P is never stored: it is recomputed from Q, K and the forward's log-sum-exp.  Two kernels, each a sibling of
// the forward kernel and each free of cross-wave reductions and atomics (bitwise reproducible):
//   attn_bwd_dq   wave owns 32 QUERIES (query on the lane): S^T = K.Q^T, dP^T = V.dO^T, dS^T = P^T*(dP^T - delta),
//                 dQ^T = K^T.dS^T with dS^T fed to the MFMA straight from the accumulator registers; also emits
//                 delta[q] = sum_d dO*O for the second kernel.
//   attn_bwd_dkv  wave owns 32 KEYS (key on the lane): S = Q.K^T, dP = dO.V^T, then dV^T += dO^T.P and
//                 dK^T += Q^T.dS, again with P / dS taken from the accumulator registers as the B operand.
// S and dP are computed twice (7 products instead of 5); in exchange nothing is summed across waves.
// The arithmetic (owner prologue, the two group steps, the stores) is the text of attention_bwd_core.h; this file holds the
// blocking, the staging of the PaddedPair images and the launches.
#include "attention_bwd_core.h"

namespace {

__device__ __forceinline__ void stage_rows(unsigned char* dst, const uint16_t* base, size_t ld, int N, int NP, int tid,
                                           int T) {
    // NP rows x 64 bf16 -> 128-byte LDS rows, 16-byte chunk XOR-swizzled by ((row>>1)&7)
    for (int it = tid; it < NP * 8; it += T) {
        const int row = it >> 3, c = it & 7;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < N) v = *(const uint4*)(base + (size_t)row * ld + c * 8);
        *(uint4*)(dst + row * 128 + ((c ^ ((row >> 1) & 7)) << 4)) = v;
    }
}
__device__ __forceinline__ void stage_rows_t(unsigned char* dst, int stride, const uint16_t* base, size_t ld, int N, int NP,
                                             int tid, int T) {
    // transposed image [64][NP] (row stride `stride` bytes): dst[d][row] = src[row][d]
    for (int it = tid; it < NP * 8; it += T) {
        const int row = it >> 3, c = it & 7;
        uint4 v = make_uint4(0, 0, 0, 0);
        if (row < N) v = *(const uint4*)(base + (size_t)row * ld + c * 8);
        const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
        for (int e = 0; e < 8; ++e)
            *(uint16_t*)(dst + (c * 8 + e) * stride + row * 2) = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
    }
}

template <int NT>
__global__ __launch_bounds__(NT * 64) void attn_bwd_dq_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ o,
                                                              const uint16_t* __restrict__ dout, const float* __restrict__ lse,
                                                              int N, int H, int QB, float scale, float scale_log2e,
                                                              uint16_t* __restrict__ dqkv, float* __restrict__ delta) {
    // blockIdx.x = ((crop*H + head)*QB + query block); a query block = NT waves x 32 queries.  K/V are walked in
    // tiles of NP = 32*NT keys; the forward's log2-sum-exp makes every tile independent (no running max).
    typedef PaddedPair<NT * 32> Layout;
    constexpr int NP = NT * 32, TS = Layout::TS, T = NT * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* Ks = smem;
    unsigned char* Vs = smem + NP * 128;
    unsigned char* Kt = smem + 2 * NP * 128;
    const int qb = blockIdx.x % QB, rh = blockIdx.x / QB;
    const int r = rh / H, hd = rh - r * H;
    const int D = H * HD, ld = 3 * D;
    const uint16_t* base = qkv + (size_t)r * N * ld + hd * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Layout lay(lane);
    const int q = qb * NP + wave * 32 + lay.rl;
    bf16x8 fq[4], fdo[4];
    float dl, lq;
    owner_query(base, o, dout, lse, delta, r, hd, N, H, q, lay.hh, fq, fdo, dl, lq);
    f32x16 acc[2];
    zero(acc);

    for (int kv0 = 0; kv0 < N; kv0 += NP) {
        if (kv0 > 0) __syncthreads();
        const int nv = N - kv0;                               // valid keys of this tile (may exceed NP)
        stage_rows(Ks, base + (size_t)kv0 * ld + D, ld, nv, NP, tid, T);
        stage_rows(Vs, base + (size_t)kv0 * ld + 2 * D, ld, nv, NP, tid, T);
        stage_rows_t(Kt, TS, base + (size_t)kv0 * ld + D, ld, nv, NP, tid, T);
        __syncthreads();
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
            dq_group(lay, {Ks, Kt}, {Vs, nullptr}, kt * 32, kv0 + kt * 32, N, fq, fdo, lq, dl, scale, scale_log2e, acc);
    }
    if (q < N) store_dq(dqkv, (size_t)r * N + q, hd, H, lay.hh, acc);
}

template <int NT>
__global__ __launch_bounds__(NT * 64) void attn_bwd_dkv_kernel(const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout,
                                                               const float* __restrict__ lse, const float* __restrict__ delta,
                                                               int N, int H, int KB, float scale, float scale_log2e,
                                                               uint16_t* __restrict__ dqkv) {
    // blockIdx.x = ((crop*H + head)*KB + key block); wave owns 32 keys; the queries are walked in tiles of NP rows
    typedef PaddedPair<NT * 32> Layout;
    constexpr int NP = NT * 32, TS = Layout::TS, T = NT * 64;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* Qs = smem;
    unsigned char* Os = smem + NP * 128;
    unsigned char* Qt = smem + 2 * NP * 128;
    unsigned char* Ot = Qt + 64 * TS;
    float* lse_s = (float*)(Ot + 64 * TS);
    float* del_s = lse_s + NP;
    const int kb = blockIdx.x % KB, rh = blockIdx.x / KB;
    const int r = rh / H, hd = rh - r * H;
    const int D = H * HD, ld = 3 * D;
    const uint16_t* base = qkv + (size_t)r * N * ld + hd * HD;
    const uint16_t* dbase = dout + (size_t)r * N * D + hd * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const Layout lay(lane);
    const int hh = lay.hh;
    const int key = kb * NP + wave * 32 + lay.rl, kc = key < N ? key : N - 1;
    bf16x8 fk[4], fv[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) {
        fk[ks] = *(const bf16x8*)(base + (size_t)kc * ld + D + ks * 16 + hh * 8);
        fv[ks] = *(const bf16x8*)(base + (size_t)kc * ld + 2 * D + ks * 16 + hh * 8);
    }
    f32x16 dk[2], dv[2];
    zero(dk);
    zero(dv);

    for (int q0 = 0; q0 < N; q0 += NP) {
        if (q0 > 0) __syncthreads();
        const int nv = N - q0;
        stage_rows(Qs, base + (size_t)q0 * ld, ld, nv, NP, tid, T);
        stage_rows(Os, dbase + (size_t)q0 * D, D, nv, NP, tid, T);
        stage_rows_t(Qt, TS, base + (size_t)q0 * ld, ld, nv, NP, tid, T);
        stage_rows_t(Ot, TS, dbase + (size_t)q0 * D, D, nv, NP, tid, T);
        for (int i = tid; i < NP; i += T) {
            lse_s[i] = q0 + i < N ? lse[((size_t)r * H + hd) * N + q0 + i] : 0.f;
            del_s[i] = q0 + i < N ? delta[((size_t)r * H + hd) * N + q0 + i] : 0.f;
        }
        __syncthreads();
#pragma unroll 1
        for (int qt = 0; qt < NT; ++qt)
            dkv_group(lay, {Qs, Qt}, {Os, Ot}, lse_s, del_s, qt * 32, q0 + qt * 32, N, fk, fv, scale, scale_log2e, dk, dv);
    }
    if (key < N) store_dkv(dqkv, (size_t)r * N + key, hd, H, hh, dk, dv);
}

template <int NT>
int launch_bwd(const BwdArgs& a) {
    typedef PaddedPair<NT * 32> Layout;
    constexpr int NP = NT * 32, TS = Layout::TS;
    const size_t lds_q = (size_t)2 * NP * 128 + 64 * TS;
    const size_t lds_kv = (size_t)2 * NP * 128 + 2 * 64 * TS + 2 * NP * 4;
    auto kq = attn_bwd_dq_kernel<NT>;
    auto kkv = attn_bwd_dkv_kernel<NT>;
    if (!yv_grant_lds((const void*)kq, lds_q) || !yv_grant_lds((const void*)kkv, lds_kv)) return YV_ERR_LAUNCH;
    const float c = a.scale * LOG2E;
    const int QB = (a.N + NP - 1) / NP;
    hipLaunchKernelGGL(kq, dim3(a.R * a.H * QB), dim3(NT * 64), lds_q, a.st, a.qkv, a.o, a.dout, a.lse, a.N, a.H, QB, a.scale, c,
                       a.dqkv, a.delta);
    hipLaunchKernelGGL(kkv, dim3(a.R * a.H * QB), dim3(NT * 64), lds_kv, a.st, a.qkv, a.dout, a.lse, a.delta, a.N, a.H, QB, a.scale,
                       c, a.dqkv);
    return yv_launch_status();
}

}  // namespace

extern "C" int yv_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, int R, int N, int H,
                                float scale, void* dqkv, float* delta_ws, void* stream) {
    // this entry point's own contract (not bwd_args_check): R == 0 is an error, alignment is not checked
    if (!qkv || !out || !dout || !lse || !dqkv || !delta_ws || R <= 0 || N <= 0 || H <= 0) return YV_ERR_ARG;
    const BwdArgs a = bwd_args(qkv, out, dout, lse, R, N, H, scale, dqkv, delta_ws, stream);
    switch (N > 256 ? 8 : (N + 31) / 32) {             // > 256 tokens: 256-row tiles on both axes
        case 1: return launch_bwd<1>(a);
        case 2: return launch_bwd<2>(a);
        case 3: return launch_bwd<3>(a);
        case 4: return launch_bwd<4>(a);
        case 5: return launch_bwd<5>(a);
        case 6: return launch_bwd<6>(a);
        case 7: return launch_bwd<7>(a);
        default: return launch_bwd<8>(a);
    }
}
