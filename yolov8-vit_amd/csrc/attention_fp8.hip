// Attention forward on an MXFP8 qkv operand (what yv_linear_mxfp8_q writes for the qkv product: e4m3 bytes + one E8M0 per 32 columns,
// i.e. two blocks per head), head dim 64, non-causal, inference only: yv_attention_fp8.  DESIGN.md section 40.
//
// attention_long_kernel's organisation, unchanged: 4 waves x 32 queries with a second launch of the live waves for the N % 128 rows,
// 64-key tiles (32 in the one-wave form) double-buffered by register staging with one barrier per tile, online softmax per 32-key
// group in index order, P never in LDS, the epilogues of attention_fwd_core.h.  What differs:
//   * Q fragments are e4m3 bytes + the row's two scale bytes, straight from global;
//   * a K tile is staged as bytes (64-byte rows, swizzle k8_off) with its keys' scale pairs beside it, and a score group is ONE
//     v_mfma_scale_f32_32x32x64_f8f6f4 (K rows as A, Q as B) instead of four 32x32x16 bf16 MFMAs;
//   * a V tile is staged as bytes and dequantised exactly to bf16 on its way into today's row-major V image (stash_v8): the
//     transposing reads, p_frag, pv_product and the bf16 PV MFMAs are attention_long_kernel's.  P is not quantised.
// Rows past N are fetched from row N - 1, bytes and scales alike: no read leaves rows [0, R * N) of either input array.
#include "attention_fwd_core.h"

namespace {

// blockIdx.x as attention_long_kernel
template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attention_fp8_kernel(const uint8_t* __restrict__ qkv, long long ld,
                                                                   const uint8_t* __restrict__ scales, long long rows_pad, int R, int N,
                                                                   int H, int qb0, int QBL, float scale_log2e,
                                                                   uint16_t* __restrict__ out, const int32_t* __restrict__ r_dev,
                                                                   AttnMx mx) {
    constexpr int KT = NW == 1 ? 32 : 64, GPT = KT / 32;
    constexpr int KTILE = KT * 64, VTILE = KT * 128, STILE = KT * 2;      // K bytes, V bf16 image, K scale pairs
    constexpr int BUF = KTILE + VTILE + STILE;
    constexpr int T = NW * 64;
    constexpr int CH = KT * 4;                           // 16-byte chunks of one tensor's tile of bytes
    constexpr int TRIPS = (CH + T - 1) / T;
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * BUF];        // [buffer][K | V | K scales]
    const int rh = blockIdx.x / QBL;
    const int qb = qb0 + (blockIdx.x - rh * QBL);
    const int r = rh / H, hd = rh - r * H;
    if (r_dev) { const int c = r_dev[0]; if (r >= (c < R ? c : R)) return; }
    const int D = H * HD, KS = D >> 7;                   // K steps (128 columns) of one of the three tensors
    const long long row0 = (long long)r * N;
    const uint8_t* base = qkv + row0 * ld + hd * HD;
    const uint8_t* sq = scales + mx_head_scales(0, hd, rows_pad, row0);
    const uint8_t* sk = scales + mx_head_scales(KS, hd, rows_pad, row0);
    const uint8_t* sv_ = scales + mx_head_scales(2 * KS, hd, rows_pad, row0);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 31, hh = lane >> 5;

    // ---- Q fragment (B operand) and its scale register, straight from global ----------------------------
    const int q = qb * 128 + wave * 32 + rl;
    i32x8 fq;
    int scq;
    q8_frag(base, ld, sq, q, N, hh, fq, scq);

    // ---- K / V staging: issue (global -> registers) and write (registers -> LDS, V dequantised) are separate steps ------
    u32x4 kst[TRIPS], vst[TRIPS];
    uint32_t ksc[TRIPS], vsc[TRIPS];                     // the key's K scale pair; the V scale byte of this chunk's block
    auto fetch = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            const int kl = row_chunk8(it < CH ? it : CH - 1).row, c = row_chunk8(it).c;
            int key = t * KT + kl;
            key = key < N ? key : N - 1;
            const uint8_t* p = base + (size_t)key * ld + D + c * 16;
            kst[i] = *(const u32x4*)p;
            vst[i] = *(const u32x4*)(p + D);
            ksc[i] = *(const uint16_t*)(sk + (size_t)key * 4);
            vsc[i] = sv_[(size_t)key * 4 + (c >> 1)];
        }
    };
    auto stash = [&](int buf) __attribute__((always_inline)) {
        unsigned char* Kb = smem + buf * BUF;
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            if (CH % T != 0 && it >= CH) break;
            const auto [kl, c] = row_chunk8(it);
            *(u32x4*)(Kb + k8_off(kl, c)) = kst[i];
            if (c == 0) *(uint16_t*)(Kb + KTILE + VTILE + 2 * kl) = (uint16_t)ksc[i];
            stash_v8(Kb + KTILE, kl, c, vst[i], mx_scale_f32(vsc[i]));
        }
    };
    const VtOff vto = vt_offsets(lane);                  // V^T fragment addressing of the transposing read

    f32x16 o[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[mt][e] = 0.f;
    float m_run = -INFINITY, l_lane = 0.f;              // l_lane: this lane's share of the row sum (lane ^ 32 holds the rest)

    const int G = (N + 31) >> 5;                         // live 32-key groups
    const int NTILE = (G + GPT - 1) / GPT;
    fetch(0);
    stash(0);
    // the query fragment is complete BEFORE the loop (see attention_long_kernel: a pending load's first use inside the loop would
    // drain the fetch of tile t + 1 in every iteration)
    asm volatile("" : "+v"(fq), "+v"(scq));
    __syncthreads();
#pragma unroll 1
    for (int t = 0; t < NTILE; ++t) {
        const bool more = t + 1 < NTILE;
        if (more) fetch(t + 1);                          // in flight under this tile's MFMA and exp work
        const unsigned char* Ks = smem + (t & 1) * BUF;
        const unsigned char* Vs = Ks + KTILE;
        const unsigned char* Ss = Vs + VTILE;
#pragma unroll
        for (int gl = 0; gl < GPT; ++gl) {
            const int g = GPT * t + gl;
            if (g >= G) break;                           // wholly past N (wave- and block-uniform)
            f32x16 sv = score_group8(Ks, Ss, gl * 32, fq, scq, rl, hh);
            if (g * 32 + 32 > N) mask_group(sv, g * 32, N, hh);       // the group that straddles N
            online_step(sv, m_run, l_lane, o, scale_log2e);
            pv_product(sv, o, [&](int mt, int st) __attribute__((always_inline)) { return vt_frag_tr(Vs, vto, mt, gl * 32 + 16 * st); });
        }
        if (more) stash((t + 1) & 1);                    // that buffer's last readers passed the previous barrier
        __syncthreads();
    }
    const float l_run = l_lane + __shfl_xor(l_lane, 32, 64);

    // ---- normalise and store (both lanes of a query are here: the exchanges run before the `q < N` of the stores) ------------
    const float inv = 1.0f / l_run;
    if (mx.q && q < N) store_mx(o, inv, mx, r, N, hd, q, hh);
    if (!out) return;
    uint16_t* orow = out + ((size_t)r * N + (q < N ? q : N - 1)) * D + hd * HD;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g4 = 0; g4 < 4; g4 += 2) {
            const u32x4 pk = swapped_rows(o, inv, mt, g4);
            if (q < N) *(u32x4*)(orow + swapped_col(mt, g4, hh)) = pk;
        }
}

struct Fp8In { const uint8_t* q; long long ld; const uint8_t* s; long long rows_pad; };

template <int NW>
int launch_fp8(const Fp8In& in, int R, int N, int H, int qb0, int QBL, float scale, uint16_t* out, const int32_t* r_dev,
               hipStream_t st, AttnMx mx) {
    hipLaunchKernelGGL(attention_fp8_kernel<NW>, dim3(R * H * QBL), dim3(NW * 64), 0, st, in.q, in.ld, in.s, in.rows_pad, R, N, H,
                       qb0, QBL, scale * LOG2E, out, r_dev, mx);
    return yv_launch_status();
}

// one MFMA on caller-provided register images: the executable statement of the operand layout (tests/test_gpu_attn_fp8.py)
__global__ __launch_bounds__(64) void mx_probe32_kernel(const i32x8* __restrict__ a, const i32x8* __restrict__ b,
                                                        const int* __restrict__ sa, const int* __restrict__ sb, int opsel,
                                                        f32x16* __restrict__ d) {
    const int l = threadIdx.x;
    f32x16 acc;
#pragma unroll
    for (int e = 0; e < 16; ++e) acc[e] = 0.f;
    if (opsel == 0) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[l], b[l], acc, 0, 0, 0, sa[l], 0, sb[l]);
    else if (opsel == 1) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[l], b[l], acc, 0, 0, 1, sa[l], 1, sb[l]);
    else if (opsel == 2) acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[l], b[l], acc, 0, 0, 2, sa[l], 2, sb[l]);
    else acc = __builtin_amdgcn_mfma_scale_f32_32x32x64_f8f6f4(a[l], b[l], acc, 0, 0, 3, sa[l], 3, sb[l]);
    d[l] = acc;
}

// the V dequantisation of the stash step on its own: one dword of bytes per thread
__global__ __launch_bounds__(256) void fp8_dequant_kernel(const uint32_t* __restrict__ q, long long n4, uint32_t scale_byte,
                                                          u32x2* __restrict__ out) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i < n4) out[i] = mx_dequant4_bf16(q[i], mx_scale_f32(scale_byte));
}

}  // namespace

extern "C" int yv_attention_fp8(const void* qkv_q, long long ld_in, const void* qkv_scales, long long in_rows_pad, int R, int N, int H,
                                float scale, void* out, const int32_t* r_dev, void* out_q, long long ldq, void* out_scales,
                                long long rows_pad, void* stream) {
    if (!qkv_q || !qkv_scales || (!out && !out_q) || R < 0 || N <= 0 || H <= 0) return YV_ERR_ARG;
    if ((out_q == nullptr) != (out_scales == nullptr)) return YV_ERR_ARG;
    // the input is a GEMM's MX output: whole 128-column K steps per tensor (H even), 16-byte rows, scale rows padded to the row tile
    if ((H & 1) || (ld_in & 15) || ld_in < 3LL * 64 * H || in_rows_pad < (long long)R * N || (in_rows_pad & 127)) return YV_ERR_ARG;
    if (out_q && ((ldq & 15) || ldq < (long long)H * 64 || rows_pad < (long long)R * N || (rows_pad & 127))) return YV_ERR_ARG;
    if (((uintptr_t)qkv_q | (uintptr_t)out | (uintptr_t)out_q) & 15) return YV_ERR_ARG;     // 16-byte row chunks
    if ((uintptr_t)qkv_scales & 3) return YV_ERR_ARG;                                       // a row's K step is one dword
    const int QB = (N + 127) / 128;
    if ((long long)R * H * QB > 0x7fffffffLL) return YV_ERR_LIMIT;
    if (R == 0) return YV_OK;
    const Fp8In in{(const uint8_t*)qkv_q, ld_in, (const uint8_t*)qkv_scales, in_rows_pad};
    uint16_t* o = (uint16_t*)out;
    hipStream_t st = (hipStream_t)stream;
    const AttnMx mx{(uint8_t*)out_q, ldq, (uint8_t*)out_scales, rows_pad};
    const int full = N / 128, rem = N - full * 128;
    if (full > 0) {
        const int rc = launch_fp8<4>(in, R, N, H, 0, full, scale, o, r_dev, st, mx);
        if (rc != YV_OK) return rc;
    }
    switch ((rem + 31) / 32) {                            // the rows past the last whole query block: only their live waves
        case 0: return YV_OK;
        case 1: return launch_fp8<1>(in, R, N, H, full, 1, scale, o, r_dev, st, mx);
        case 2: return launch_fp8<2>(in, R, N, H, full, 1, scale, o, r_dev, st, mx);
        case 3: return launch_fp8<3>(in, R, N, H, full, 1, scale, o, r_dev, st, mx);
        default: return launch_fp8<4>(in, R, N, H, full, 1, scale, o, r_dev, st, mx);
    }
}

extern "C" int yv_mx_probe32(const void* a, const void* b, const void* sa, const void* sb, int opsel, void* d, void* stream) {
    if (!a || !b || !sa || !sb || !d || opsel < 0 || opsel > 3) return YV_ERR_ARG;
    hipLaunchKernelGGL(mx_probe32_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const i32x8*)a, (const i32x8*)b,
                       (const int*)sa, (const int*)sb, opsel, (f32x16*)d);
    return yv_launch_status();
}

extern "C" int yv_attention_fp8_dequant(const void* q, long long n, int scale_byte, void* out, void* stream) {
    if (!q || !out || n <= 0 || (n & 3) || scale_byte < 0 || scale_byte > 254) return YV_ERR_ARG;
    if (((uintptr_t)q & 3) || ((uintptr_t)out & 7)) return YV_ERR_ARG;
    const long long n4 = n >> 2;
    if ((n4 + 255) / 256 > 0x7fffffffLL) return YV_ERR_LIMIT;
    hipLaunchKernelGGL(fp8_dequant_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint32_t*)q, n4, (uint32_t)scale_byte, (u32x2*)out);
    return yv_launch_status();
}
