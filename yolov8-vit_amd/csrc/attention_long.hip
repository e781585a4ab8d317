// Attention forward for sequences that do not fit one K/V tile (ViT-B/8 at 224: 785 tokens; ViT-x/16 at 384: 577), head dim 64,
// non-causal, bf16 in, f32 accumulate: yv_attention_long.  DESIGN.md section 15.
//
// The MFMA plan, the LDS images, the online-softmax group step and the output formats are csrc/attention_fwd_core.h, shared with
// attention.hip; the blocking is this file's:
//   * a workgroup is 4 waves x 32 query rows = 128 queries of one (crop, head).  The N % 128 rows left over go to a second launch
//     whose workgroups have ceil((N % 128) / 32) waves: no wave exists for a 32-row group that lies wholly past N;
//   * keys are walked in tiles of 64 (two 32-key groups; 32 in the one-wave workgroup) up to ceil(N / 32) groups: a group wholly past N is skipped, only the
//     group that straddles N is masked.  Rows past N are fetched from row N - 1 (finite; their probabilities are exactly 0);
//   * online softmax per 32-key group (running max / sum per query; O rescaled only when some query's maximum grew): a wave holds
//     one score group (16 registers), not eight;
//   * K and V tiles are double-buffered in LDS by register staging with the issue-early / write-late split: the global loads of
//     tile t + 1 are issued in front of tile t's MFMA / exp work and written to the other buffer behind it, one barrier per tile.
//     Plain loads and 16-byte LDS stores: every wait is the compiler's;
//   * images as in attention_pipe_kernel: swizzled K rows; V stays row-major and is read with the transposing ds_read_b64_tr_b16;
//   * a query's reduction runs over the key groups in index order whatever the grid: a crop's output does not depend on R, on the
//     crop's index or on the launch.
// 64-bit addressing throughout: no 2 GB limit on the tensors.
#include "attention_fwd_core.h"

namespace {

// blockIdx.x = (crop * H + head) * QBL + (query block - qb0); a query block = 128 rows, of which this launch's workgroups hold
// the first NW * 32
template <int NW>
__global__ __launch_bounds__(NW * 64, 2) void attention_long_kernel(const uint16_t* __restrict__ qkv, int R, int N, int H, int qb0,
                                                                    int QBL, float scale_log2e, uint16_t* __restrict__ out,
                                                                    const int32_t* __restrict__ r_dev, float* __restrict__ lse,
                                                                    AttnMx mx) {
    // keys per tile: 64; the one-wave workgroup (N % 128 <= 32: 785 and 577 tokens) takes 32, which halves its LDS and staging
    // registers - 10 instead of 5 such workgroups share a CU, and R * H of them fit the chip in one round at 128 crops x 12 heads
    constexpr int KT = NW == 1 ? 32 : 64, GPT = KT / 32;
    constexpr int TILE = KT * 128;                       // bytes of a K (or V) tile
    constexpr int T = NW * 64;
    constexpr int CH = KT * 8;                           // 16-byte chunks of one tensor's tile
    constexpr int TRIPS = (CH + T - 1) / T;
    __shared__ __attribute__((aligned(16))) unsigned char smem[4 * TILE];       // [buffer][K | V]
    const int rh = blockIdx.x / QBL;
    const int qb = qb0 + (blockIdx.x - rh * QBL);
    const int r = rh / H, hd = rh - r * H;
    if (r_dev) { const int c = r_dev[0]; if (r >= (c < R ? c : R)) return; }
    const int D = H * HD, ld = 3 * D;
    const uint16_t* base = qkv + (size_t)r * N * ld + hd * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int rl = lane & 31, hh = lane >> 5;

    // ---- Q fragments (B operand), straight from global ---------------------------------------------
    const int q = qb * 128 + wave * 32 + rl;
    bf16x8 fq[4];
    q_frags(base, q, N, ld, hh, fq);

    // ---- K / V staging: issue (global -> registers) and write (registers -> LDS) are separate steps ------
    u32x4 kst[TRIPS], vst[TRIPS];
    auto fetch = [&](int t) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            const int kl = row_chunk(it < CH ? it : CH - 1).row, c = row_chunk(it).c;
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
            const auto [kl, c] = row_chunk(it);
            *(u32x4*)(Kb + k_off(kl, c)) = kst[i];
            *(u32x4*)(Kb + TILE + v_off(kl, c)) = vst[i];
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
    // the query fragments are complete BEFORE the loop: left pending, their first use inside it makes hipcc wait vmcnt(0) in every
    // iteration (its wait counting is per program point, not per trip), which drains the fetch of tile t + 1 in front of the S MFMAs
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) asm volatile("" : "+v"(fq[ks]));
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
            f32x16 sv = score_group(Ks, gl * 32, fq, rl, hh);
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
    store_lse(lse, r, H, hd, N, q, hh, m_run * scale_log2e, l_run);
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

template <int NW>
int launch_long(const uint16_t* qkv, int R, int N, int H, int qb0, int QBL, float scale, uint16_t* out, const int32_t* r_dev,
                float* lse, hipStream_t st, AttnMx mx) {
    hipLaunchKernelGGL(attention_long_kernel<NW>, dim3(R * H * QBL), dim3(NW * 64), 0, st, qkv, R, N, H, qb0, QBL,
                       scale * LOG2E, out, r_dev, lse, mx);
    return yv_launch_status();
}

}  // namespace

extern "C" int yv_attention_long(const void* qkv, int R, int N, int H, float scale, void* out, const int32_t* r_dev, float* lse,
                                 void* out_q, long long ldq, void* out_scales, long long rows_pad, void* stream) {
    if (!qkv || (!out && !out_q) || R < 0 || N <= 0 || H <= 0) return YV_ERR_ARG;
    if ((out_q == nullptr) != (out_scales == nullptr)) return YV_ERR_ARG;
    if (out_q) {
        // the proj GEMM's operand: whole 128-column K steps (H even), 16-byte rows, scale rows padded to the GEMM's row tile
        if ((H & 1) || (ldq & 15) || ldq < (long long)H * 64 || rows_pad < (long long)R * N || (rows_pad & 127)) return YV_ERR_ARG;
    }
    if (((uintptr_t)qkv | (uintptr_t)out | (uintptr_t)out_q) & 15) return YV_ERR_ARG;       // 16-byte row chunks
    if ((uintptr_t)lse & 3) return YV_ERR_ARG;
    const int QB = (N + 127) / 128;
    if ((long long)R * H * QB > 0x7fffffffLL) return YV_ERR_LIMIT;
    if (R == 0) return YV_OK;
    const uint16_t* q = (const uint16_t*)qkv;
    uint16_t* o = (uint16_t*)out;
    hipStream_t st = (hipStream_t)stream;
    const AttnMx mx{(uint8_t*)out_q, ldq, (uint8_t*)out_scales, rows_pad};
    const int full = N / 128, rem = N - full * 128;
    if (full > 0) {
        const int rc = launch_long<4>(q, R, N, H, 0, full, scale, o, r_dev, lse, st, mx);
        if (rc != YV_OK) return rc;
    }
    switch ((rem + 31) / 32) {                            // the rows past the last whole query block: only their live waves
        case 0: return YV_OK;
        case 1: return launch_long<1>(q, R, N, H, full, 1, scale, o, r_dev, lse, st, mx);
        case 2: return launch_long<2>(q, R, N, H, full, 1, scale, o, r_dev, lse, st, mx);
        case 3: return launch_long<3>(q, R, N, H, full, 1, scale, o, r_dev, lse, st, mx);
        default: return launch_long<4>(q, R, N, H, full, 1, scale, o, r_dev, lse, st, mx);
    }
}
