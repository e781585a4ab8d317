// Residual GEMM + LayerNorm in one launch (yv_linear_res_ln): the proj / fc2 step of a ViT block together with the LayerNorm
// that reads its result (timm Block: x = x + attn(norm1(x)); x = x + mlp(norm2(x)); README.md:21-29):
//     x[M,N] (f32, read-modify-write) = x + a[M,K] (bf16) . w[N,K]^T (bf16) + bias[N]
//     h[M,N] (bf16)                   = LayerNorm(x_new; gamma, beta, eps)
// A workgroup owns COMPLETE output rows - a tile is 64 rows x all N columns - so the statistics of a row never leave the chip
// and the separate LayerNorm pass over the residual stream (4 B read + 2 B written per element) disappears.
//
// 8 waves; wave w holds the 64 rows x N/8 columns [w N/8, (w+1) N/8) of the tile: 4 row fragments x N/128 column fragments of
// mfma_f32_16x16x32_bf16 = 16 N/128 accumulator registers (96 at N = 768, 128 at N = 1024).  A K tile is 32 deep: 64-byte LDS
// rows, 4 KB of activations + 64 N bytes of weights per stage (52 KB at N = 768: three stages; 68 KB at N = 1024: two).
// Operands arrive by LDS-DMA in 1 KB pieces of 16 rows (lane l -> row l / 4, 16-byte slot l % 4); the slot a chunk lands in is
// chunk ^ ((row / 2) & 3), applied on the SOURCE address, which makes the fragment reads (16 rows x one chunk per quarter wave)
// conflict-free.  One barrier per K tile: [counted vmcnt: K tile t landed] barrier [issue K tile t + S - 1 into the stage
// that K tile t - 1 just left] [fragment reads + MFMAs of K tile t].  No register-destination load is in flight inside the
// loop (hipcc would drain the DMA in front of its first use), the residual values are fetched in the epilogue.
//
// Epilogue, per lane 4 N/128 float4 values (MFMA C layout: lane (fr, fq) holds row fr, columns 16 i + 4 fq .. + 3):
//   v = (acc + bias) + x  ->  x (16-byte stores)  ->  two-pass statistics in f32 (mean, then the centred sum of squares) in the very
//   summation order of layernorm_kernel: the per-chunk sums of a row meet in LDS and one wave adds them as that kernel's wave
//   does  ->  h = (v - mean) * rstd * gamma + beta, bf16 (8-byte stores).  Given the same x, h has layernorm_kernel's bits.
// Every step of a row's arithmetic has a fixed order that involves that row alone: a row's two outputs are bit-identical whatever
// M, the device row count, the tile it falls in and the grid size (what PipelinedRunner's half batches rely on).
// ONE kernel per width for every M: persistent, workgroup b walks tiles b, b + grid, ...; the grid is the thread's CU budget.
#include "gemm_common.h"

using namespace yvgemm;

namespace {

struct ResLnArgs {
    const uint16_t* a; int lda;
    const uint16_t* w;
    const float* bias;
    int M, K;
    float* x; int ldx;
    const float* gamma; const float* beta; float eps;
    uint16_t* h; int ldh;
    const int32_t* m_dev; int m_mul;
};

typedef __attribute__((address_space(3))) void* lds_void_t;

constexpr int RL_BM = 64;                  // rows of a tile
constexpr int RL_ROWB = 64;                // bytes of an LDS row: a 32-deep K tile

template <int V> __device__ __forceinline__ void wait_vm() { asm volatile("s_waitcnt vmcnt(%0)" ::"n"(V) : "memory"); }
__device__ __forceinline__ void bar_lds() {       // LDS traffic of this wave retired, then the workgroup barrier (no vmcnt drain)
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_barrier" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}

constexpr size_t res_ln_lds(int N, int S) { return (size_t)S * (RL_BM * RL_ROWB + N * RL_ROWB) + 2 * RL_BM * sizeof(float); }

template <int N, int S>
__global__ __launch_bounds__(512) void gemm_res_ln_kernel(ResLnArgs g) {
    constexpr int BM = RL_BM, MF = BM / 16, NW = N / 8, NF = NW / 16;     // columns / column fragments per wave
    constexpr int PW = N / 128;                                            // weight pieces (16 rows) per wave and K tile
    constexpr int A_BYTES = BM * RL_ROWB, STAGE = A_BYTES + N * RL_ROWB, RED0 = S * STAGE;
    constexpr int NCH = N / 4, PST = NCH + 4;                              // float4 chunks of a row; row stride of their LDS image (4 fr + fq: distinct banks)
    static_assert(BM * PST * 4 <= STAGE && NCH <= 256, "the chunk image fits a stage; layernorm_kernel's four chunks per lane");
    static_assert(N % 128 == 0 && (S == 2 || S == 3), "8 waves x 16-column fragments; two or three stages");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    if (M <= 0) return;
    const int ntiles = (M + BM - 1) / BM;
    const int K = g.K, nk = K / 32;

    const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)g.a, 0, (int)(((long long)(g.M - 1) * g.lda + K) * 2), 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)g.w, 0, (int)((long long)N * K * 2), 0x00020000);
    const auto rsX = __builtin_amdgcn_make_buffer_rsrc((void*)g.x, 0, (int)(((long long)(M - 1) * g.ldx + N) * 4), 0x00020000);
    const auto rsH = __builtin_amdgcn_make_buffer_rsrc((void*)g.h, 0, (int)(((long long)(M - 1) * g.ldh + N) * 2), 0x00020000);

    const int mfr = lane & 15, mfq = lane >> 4;                            // fragment coordinates of the main loop
    const int drow = lane >> 2, dch = (lane & 3) ^ ((drow >> 1) & 3);      // DMA: row inside a piece, source chunk of this lane's slot
    const uint32_t ow = (uint32_t)(drow * K * 2 + dch * 16);              // weight pieces: + piece * 16 rows and the K tile as scalar offset
    const bool has_a = wave < BM / 16;                                    // waves 0..3 also bring one activation piece per K tile
    const int ncol0 = wave * NW;
    float* const red = (float*)(smem + RED0);                             // mean[64] | rstd[64]

    for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int m0 = tile * BM;
        uint32_t oa = 0x80000000u;                                         // rows past the matrix read as zeros (range check)
        if (has_a) {
            const int ma = m0 + wave * 16 + drow;
            if (ma < g.M) oa = (uint32_t)((long long)ma * g.lda * 2 + dch * 16);
        }
        auto issue = [&](int t, int st) __attribute__((always_inline)) {
            unsigned char* base = smem + st * STAGE;
            if (has_a) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t)(base + wave * 1024), 16, (int)oa, t * 64, 0, 0);
#pragma unroll
            for (int jj = 0; jj < PW; ++jj) {
                const int q = wave * PW + jj;
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lds_void_t)(base + A_BYTES + q * 1024), 16, (int)ow,
                                                         q * 32 * K + t * 64, 0, 0);
            }
        };

        f32x4 acc[NF][MF];
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

#pragma unroll
        for (int s = 0; s < S - 1; ++s) issue(s, s);                       // nk >= 4 > S - 1
        int st = 0;                                                        // stage of K tile t
        for (int t = 0; t < nk; ++t) {
            // K tile t landed (this wave's pieces; behind the barrier everybody's), K tile t + 1 may stay in flight
            // (the count assumes what holds on gfx9: loads and stores share ONE vmcnt, loads retire in issue order among themselves, and
            // the previous tile's x / h stores are older than every piece counted here - so "at most one K tile's pieces outstanding"
            // implies K tile t landed.  A register-destination load or a store issued inside this loop would break the count.)
            if (S == 3 && t + 1 < nk) { if (has_a) wait_vm<PW + 1>(); else wait_vm<PW>(); }
            else wait_vm<0>();
            __builtin_amdgcn_sched_barrier(0);
            asm volatile("s_barrier" ::: "memory");                       // also: every wave is past its reads of K tile t - 1
            __builtin_amdgcn_sched_barrier(0);
            {
                const int tn = t + S - 1;
                int sn = st + S - 1; sn = sn >= S ? sn - S : sn;
                if (tn < nk) issue(tn, sn);
            }
            const unsigned char* A = smem + st * STAGE;
            const unsigned char* W = A + A_BYTES;
            bf16x8 fa[MF];
#pragma unroll
            for (int j = 0; j < MF; ++j) {
                const int rr = j * 16 + mfr;
                fa[j] = *(const bf16x8*)(A + rr * RL_ROWB + ((mfq ^ ((rr >> 1) & 3)) << 4));
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int rr = ncol0 + i * 16 + mfr;
                const bf16x8 fw = *(const bf16x8*)(W + rr * RL_ROWB + ((mfq ^ ((rr >> 1) & 3)) << 4));
#pragma unroll
                for (int j = 0; j < MF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw, fa[j], acc[i][j], 0, 0, 0);
            }
            st = st + 1 == S ? 0 : st + 1;
        }

        // ---- epilogue (no DMA in flight: the last K tile waited for everything) ----------------------------------------------
        // bias | gamma | beta go through LDS (3 N floats in the last stage, which the next tile's DMA reaches only behind its first
        // K-tile barrier): as global loads inside the loops below hipcc hoists them all and spills
        // (lane coordinates through an opaque copy: what the epilogue derives from them is then computed here, per tile, instead of
        // being carried - and at N = 1024 spilled to scratch - across the main loop)
        int lane_e = lane;
        asm volatile("" : "+v"(lane_e));
        const int fr = lane_e & 15, fq = lane_e >> 4;
        uint32_t offx[MF], offh[MF];
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            const int m = m0 + j * 16 + fr;
            offx[j] = m < M ? (uint32_t)(((long long)m * g.ldx + ncol0 + fq * 4) * 4) : 0x80000000u;
            offh[j] = m < M ? (uint32_t)(((long long)m * g.ldh + ncol0 + fq * 4) * 2) : 0x80000000u;
        }
        constexpr int XB = 2;
        u32x4 xr[XB][NF];                                                  // residual values of two row fragments: one in use, one in flight
        auto fetch_x = [&](int j) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < NF; ++i) xr[j % XB][i] = __builtin_amdgcn_raw_buffer_load_b128(rsX, offx[j] + i * 64, 0, 0);
        };
        fetch_x(0);
        float* const par = (float*)(smem + (S - 1) * STAGE);
        bar_lds();                                                         // every wave is past its last fragment reads
        for (int c = (lane_e & 63) + wave * 64; c < 3 * N / 4; c += 512) {
            const float* src = c < N / 4 ? g.bias + c * 4 : c < N / 2 ? g.gamma + (c - N / 4) * 4 : g.beta + (c - N / 2) * 4;
            *(float4*)(par + c * 4) = *(const float4*)src;
        }
        bar_lds();
        const float* const pl = par + ncol0 + fq * 4;                      // this lane's columns of fragment i: pl + 16 i (+ N: gamma, + 2 N: beta)
        // Statistics exactly as layernorm_kernel sums them, so that h has the bits of the unfused pair: the row's N / 4 float4 chunks
        // c each give p_c = (v0 + v1) + (v2 + v3); "lane" l of that kernel adds p_l, p_(l+64), ... in this order, then the 64 lane
        // sums go through wave_sum's xor butterfly.  The chunk values of the 64 rows meet in LDS (stage 0: dead, and the next tile's
        // DMA comes after the last barrier below); wave w then plays layernorm_kernel's wave for rows 8 w .. 8 w + 7.
        float* const pbuf = (float*)smem;                                  // [64 rows][PST]
        float* const pme = pbuf + (ncol0 >> 2) + fq;                       // this lane's chunk of fragment i, row r: pme[r * PST + 4 i]
        auto row_stat = [&](float* out, bool second) __attribute__((always_inline)) {
            bar_lds();                                                     // chunk values complete
#pragma unroll
            for (int rr = 0; rr < BM / 8; ++rr) {
                const int row = wave * (BM / 8) + rr;
                float s = 0.f;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int c = (lane_e & 63) + 64 * i;
                    if (c < NCH) s += pbuf[row * PST + c];
                }
                s = wave_sum(s);
                const float r = second ? 1.0f / sqrtf(s / (float)N + g.eps) : s / (float)N;
                if ((lane_e & 63) == 0) out[row] = r;
            }
            bar_lds();                                                     // row results complete; every wave is past its chunk reads
        };
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            if (j + 1 < MF) fetch_x(j + 1);
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const float4 bv = *(const float4*)(pl + i * 16);
                const u32x4 xv = xr[j % XB][i];
                f32x4 v;
                v[0] = (acc[i][j][0] + bv.x) + __uint_as_float(xv[0]);
                v[1] = (acc[i][j][1] + bv.y) + __uint_as_float(xv[1]);
                v[2] = (acc[i][j][2] + bv.z) + __uint_as_float(xv[2]);
                v[3] = (acc[i][j][3] + bv.w) + __uint_as_float(xv[3]);
                acc[i][j] = v;
                // the column step is an immediate offset, never a register soffset (store-data hazard of 16-byte stores, see
                // gemm_p9_kernel's f32 epilogue)
                __builtin_amdgcn_raw_buffer_store_b128((u32x4){__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]),
                                                               __float_as_uint(v[3])}, rsX, offx[j] + i * 64, 0, 0);
                pme[(j * 16 + fr) * PST + 4 * i] = (v[0] + v[1]) + (v[2] + v[3]);
            }
            __builtin_amdgcn_sched_barrier(0);
        }
        row_stat(red, false);
        float mean[MF];
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            mean[j] = red[j * 16 + fr];
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const float a = acc[i][j][0] - mean[j], b = acc[i][j][1] - mean[j], c = acc[i][j][2] - mean[j], d = acc[i][j][3] - mean[j];
                pme[(j * 16 + fr) * PST + 4 * i] = (a * a + b * b) + (c * c + d * d);
            }
        }
        row_stat(red + BM, true);
        float rstd[MF];
#pragma unroll
        for (int j = 0; j < MF; ++j) rstd[j] = red[BM + j * 16 + fr];
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const float4 gm = *(const float4*)(pl + N + i * 16), bt = *(const float4*)(pl + 2 * N + i * 16);
#pragma unroll
            for (int j = 0; j < MF; ++j) {
                const float o0 = (acc[i][j][0] - mean[j]) * rstd[j] * gm.x + bt.x, o1 = (acc[i][j][1] - mean[j]) * rstd[j] * gm.y + bt.y;
                const float o2 = (acc[i][j][2] - mean[j]) * rstd[j] * gm.z + bt.z, o3 = (acc[i][j][3] - mean[j]) * rstd[j] * gm.w + bt.w;
                __builtin_amdgcn_raw_buffer_store_b64((u32x2){pack_bf16x2(o0, o1), pack_bf16x2(o2, o3)}, rsH, offh[j] + i * 32, 0, 0);
            }
        }
        // the next tile's first DMAs go to stages 0 .. S-2 (every wave is past its fragment and chunk reads); stage S-1 - the parameter
        // image - and `red` are next written behind the next tile's first K-tile barrier, which every wave reaches only after its last read
    }
}

template <int N, int S>
int launch_res_ln(const ResLnArgs& g, hipStream_t st) {
    constexpr size_t lds = res_ln_lds(N, S);
    void (*kern)(ResLnArgs) = gemm_res_ln_kernel<N, S>;
    if (!yv_grant_lds((const void*)kern, lds)) return YV_ERR_LAUNCH;          // remembered per kernel and device
    const int n_cu = persistent_cus();
    if (!n_cu) return YV_ERR_LAUNCH;
    const int tiles = (g.M + RL_BM - 1) / RL_BM;
    launch_timed(kern, (unsigned)(tiles < n_cu ? tiles : n_cu), 512, lds, st, g);
    return yv_launch_status();
}

}  // namespace

extern "C" int yv_linear_res_ln(const void* a, int lda, const void* w, const float* bias, int M, int N, int K, float* x, int ldx,
                                const float* gamma, const float* beta, float eps, void* h, int ldh, const int32_t* m_dev,
                                int m_mul, void* stream) {
    if (!a || !w || !bias || !x || !gamma || !beta || !h || M < 0) return YV_ERR_ARG;
    if (!(N == 128 || N == 768 || N == 1024)) return YV_ERR_ARG;              // one instance per width: a tile spans the row
    if (K < 128 || (K % 64)) return YV_ERR_ARG;
    if ((lda & 7) || (ldx & 7) || (ldh & 7) || lda < K || ldx < N || ldh < N) return YV_ERR_ARG;
    if (((uintptr_t)a | (uintptr_t)w | (uintptr_t)bias | (uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)h) & 15)
        return YV_ERR_ARG;
    if (M == 0) return YV_OK;
    // 32-bit byte offsets behind buffer descriptors
    if (((long long)(M - 1) * lda + K) * 2 >= 0x7fffffffLL || (long long)N * K * 2 >= 0x7fffffffLL ||
        ((long long)(M - 1) * ldx + N) * 4 >= 0x7fffffffLL || ((long long)(M - 1) * ldh + N) * 2 >= 0x7fffffffLL)
        return YV_ERR_LIMIT;
    ResLnArgs g = {(const uint16_t*)a, lda, (const uint16_t*)w, bias, M, K, x, ldx, gamma, beta, eps, (uint16_t*)h, ldh, m_dev, m_mul};
    switch (N) {
        case 128: return launch_res_ln<128, 3>(g, (hipStream_t)stream);
        case 768: return launch_res_ln<768, 3>(g, (hipStream_t)stream);
        default: return launch_res_ln<1024, 2>(g, (hipStream_t)stream);
    }
}
