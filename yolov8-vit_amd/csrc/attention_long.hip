// Attention forward for sequences that do not fit one K/V tile (ViT-B/8 at 224: 785 tokens; ViT-x/16 at 384: 577), head dim 64,
// non-causal, bf16 in, f32 accumulate: yv_attention_long.  DESIGN.md section 15.
//
// Same MFMA plan as attention.hip (v_mfma_f32_32x32x16_bf16; S^T = K . Q^T has the key on the register axis and the query on the
// lane; the exponentiated accumulator registers are the B operand of O^T = V^T . P^T, so P never touches LDS), other blocking:
//   * a workgroup is 4 waves x 32 query rows = 128 queries of one (crop, head).  The N % 128 rows left over go to a second launch
//     whose workgroups have ceil((N % 128) / 32) waves: no wave exists for a 32-row group that lies wholly past N;
//   * keys are walked in tiles of 64 (two 32-key groups; 32 in the one-wave workgroup) up to ceil(N / 32) groups: a group wholly past N is skipped, only the
//     group that straddles N is masked.  Rows past N are fetched from row N - 1 (finite; their probabilities are exactly 0);
//   * online softmax per 32-key group (running max / sum per query; O rescaled only when some query's maximum grew): a wave holds
//     one score group (16 registers), not eight;
//   * K and V tiles are double-buffered in LDS by register staging with the issue-early / write-late split: the global loads of
//     tile t + 1 are issued in front of tile t's MFMA / exp work and written to the other buffer behind it, one barrier per tile.
//     Plain loads and 16-byte LDS stores: every wait is the compiler's;
//   * images as in attention_pipe_kernel: K chunk ^ ((row >> 1) & 7) (conflict-free ds_read_b128 of the 32-row A fragment); V stays
//     row-major, chunk ^ 4 ((row >> 1) & 1), and is read with the transposing ds_read_b64_tr_b16;
//   * a query's reduction runs over the key groups in index order whatever the grid: a crop's output does not depend on R, on the
//     crop's index or on the launch.
// 64-bit addressing throughout: no 2 GB limit on the tensors.
#include "mx_quant.h"

namespace {

constexpr int HD = 64;
struct AttnMx { uint8_t* q; long long ldq; uint8_t* s; long long rows; };

typedef __attribute__((ext_vector_type(4))) short al_s16x4;
typedef __attribute__((address_space(3))) al_s16x4* al_lds_s16x4_t;

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
    const int qc = q < N ? q : N - 1;
    bf16x8 fq[4];
#pragma unroll
    for (int ks = 0; ks < 4; ++ks) fq[ks] = *(const bf16x8*)(base + (size_t)qc * ld + ks * 16 + hh * 8);

    // ---- K / V staging: issue (global -> registers) and write (registers -> LDS) are separate steps ------
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
            const int kl = it >> 3, c = it & 7;
            *(u32x4*)(Kb + kl * 128 + ((c ^ ((kl >> 1) & 7)) << 4)) = kst[i];
            *(u32x4*)(Kb + TILE + kl * 128 + ((c ^ (((kl >> 1) & 1) << 2)) << 4)) = vst[i];
        }
    };
    // V^T fragment addressing of the transposing read (attention_pipe_kernel): 16-lane group G = lane >> 4 takes d columns
    // (G & 1) * 16 .. + 15 of the key rows kb + 4 (G >> 1) + q; lane 4 q + p of the group addresses row q, columns 4 p .. 4 p + 3
    const int tG = lane >> 4, tq = (lane >> 2) & 3, tp = lane & 3;
    const int tkq = 4 * (tG >> 1) + tq;
    const int tsw = ((tkq >> 1) & 1) << 2;
    const int tc = (tG & 1) * 2 + (tp >> 1);
    const int voff0 = tkq * 128 + (((0 ^ tsw) + tc) << 4) + (tp & 1) * 8;      // mt = 0: chunks 0..3
    const int voff1 = tkq * 128 + (((4 ^ tsw) + tc) << 4) + (tp & 1) * 8;      // mt = 1: chunks 4..7

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
            f32x16 sv;
#pragma unroll
            for (int e = 0; e < 16; ++e) sv[e] = 0.f;
            const int row = gl * 32 + rl;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) {
                const bf16x8 fk = *(const bf16x8*)(Ks + row * 128 + (((2 * ks + hh) ^ ((row >> 1) & 7)) << 4));
                sv = __builtin_amdgcn_mfma_f32_32x32x16_bf16(fk, fq[ks], sv, 0, 0, 0);
            }
            if (g * 32 + 32 > N) {                       // the group that straddles N
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const int key = g * 32 + (e & 3) + 8 * (e >> 2) + 4 * hh;
                    sv[e] = key < N ? sv[e] : -INFINITY;
                }
            }
            float mxv = sv[0];
#pragma unroll
            for (int e = 1; e < 16; ++e) mxv = fmaxf(mxv, sv[e]);
            mxv = fmaxf(mxv, __shfl_xor(mxv, 32, 64));
            const float m_new = fmaxf(m_run, mxv);       // every live group holds >= 1 valid key for every row: finite from group 0 on
            if (__any(m_new > m_run)) {                  // wave-uniform: some query's maximum grew
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
                sv[e] = __builtin_amdgcn_exp2f(fmaf(sv[e], scale_log2e, -mb));
                l_lane += sv[e];
            }
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                bf16x8 fp;
#pragma unroll
                for (int j = 0; j < 8; ++j) fp[j] = (__bf16)sv[8 * st + j];
                const int kb = gl * 32 + 16 * st;
#pragma unroll
                for (int mt = 0; mt < 2; ++mt) {
                    const unsigned char* va = Vs + (mt ? voff1 : voff0) + kb * 128;
                    const al_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((al_lds_s16x4_t)(va));
                    const al_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((al_lds_s16x4_t)(va + 8 * 128));
                    const u32x2 lo2 = __builtin_bit_cast(u32x2, lo), hi2 = __builtin_bit_cast(u32x2, hi);
                    const u32x4 pk = {lo2[0], lo2[1], hi2[0], hi2[1]};
                    o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pk), fp, o[mt], 0, 0, 0);
                }
            }
        }
        if (more) stash((t + 1) & 1);                    // that buffer's last readers passed the previous barrier
        __syncthreads();
    }
    const float l_run = l_lane + __shfl_xor(l_lane, 32, 64);

    // ---- normalise and store: lane owns d = 32 mt + 8 g + 4 hh .. + 3 of its query -------------------
    const float inv = 1.0f / l_run;
    if (lse && hh == 0 && q < N) lse[((size_t)r * H + hd) * N + q] = m_run * scale_log2e + log2f(l_run);   // log2 domain
    if (mx.q && q < N) {
        // a head's 64 columns are two MX blocks (d 0..31 = mt 0, d 32..63 = mt 1); a query's values of one block sit in this lane
        // and in lane ^ 32 (same q: both are here); the bf16 rounding of the ordinary output is kept
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
    if (!out) return;
    // pairs of 4-column groups (g, g + 1) are exchanged between the half-waves so that lane hh = 0 owns d = 8 g .. 8 g + 7 and
    // lane hh = 1 owns d = 8 (g + 1) .. + 7: 8 stores of 16 bytes per query row
    uint16_t* orow = out + ((size_t)r * N + qc) * D + hd * HD;
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int g4 = 0; g4 < 4; g4 += 2) {
            const uint32_t a0 = pack_bf16x2(o[mt][4 * g4] * inv, o[mt][4 * g4 + 1] * inv);
            const uint32_t a1 = pack_bf16x2(o[mt][4 * g4 + 2] * inv, o[mt][4 * g4 + 3] * inv);
            const uint32_t b0 = pack_bf16x2(o[mt][4 * g4 + 4] * inv, o[mt][4 * g4 + 5] * inv);
            const uint32_t b1 = pack_bf16x2(o[mt][4 * g4 + 6] * inv, o[mt][4 * g4 + 7] * inv);
            const auto x0 = __builtin_amdgcn_permlane32_swap(a0, b0, false, false);
            const auto x1 = __builtin_amdgcn_permlane32_swap(a1, b1, false, false);
            if (q < N) *(uint4*)(orow + mt * 32 + 8 * (g4 + hh)) = make_uint4(x0[0], x1[0], x0[1], x1[1]);
        }
}

template <int NW>
int launch_long(const uint16_t* qkv, int R, int N, int H, int qb0, int QBL, float scale, uint16_t* out, const int32_t* r_dev,
                float* lse, hipStream_t st, AttnMx mx) {
    hipLaunchKernelGGL(attention_long_kernel<NW>, dim3(R * H * QBL), dim3(NW * 64), 0, st, qkv, R, N, H, qb0, QBL,
                       scale * 1.4426950408889634f, out, r_dev, lse, mx);
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
