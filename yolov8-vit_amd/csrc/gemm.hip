// Implicit-GEMM on CDNA4 MFMA: one kernel family for
//   * Linear  out[M,N] = A[M,K] . W[N,K]^T            (timm Attention.qkv/proj, Mlp.fc1/fc2, PatchEmbed, head)
//   * Conv2d  k in {1,3}, stride {1,2}, NHWC bf16     (ultralytics Conv/C2f/SPPF/Detect)
// with the whole elementwise tail fused into the epilogue (folded-BN bias, SiLU,
// erf-form GELU (erfc approximated to 1.5e-7), f32 residual-stream accumulate, bf16 shortcut add, pos_embed add).
//
// Tiling (wave = 64 lanes, v_mfma_f32_16x16x32_bf16):
//   workgroup = 256 threads = 4 waves, output tile BM x BN, K step 64 (128 B per row).
//   Both operands are K-contiguous ("NT" GEMM), staged global -> registers -> LDS
//   (issue-early / write-late, two LDS buffers, one barrier per K step).  Rows are
//   128 B in LDS with the 16-byte chunk index XOR-swizzled by (row & 7): the
//   ds_read_b128 fragment reads (16 rows x one chunk per lane group) are conflict free.
//   The MFMA "A" operand is the WEIGHT tile and "B" the activation tile, i.e. the
//   accumulator holds C^T: each lane owns 4 consecutive output channels of one
//   pixel/token, so the epilogue emits 8-byte (bf16) / 16-byte (f32) stores.
//   The conv gather (im2col, zero padding, optional 2x nearest upsample and
//   2-source channel concat) happens in the global->register stage: nothing is
//   materialised.
//   blockIdx is remapped so that the 8 XCDs each walk contiguous N tiles of the same
//   M tile (activation rows stay in that XCD's L2).
#include <string.h>
#include <type_traits>
#include <algorithm>
#include <map>
#include <mutex>
#include <vector>
#include "gemm_common.h"
#include "mx_quant.h"
#include "bn_act_grad.h"

using namespace yvgemm;

thread_local hipEvent_t yvgemm::t_time_start = nullptr, yvgemm::t_time_stop = nullptr;   // yv_set_launch_timing: next timed launch (launch_timed)

namespace {

int g_opt_wgrad_split = 0;           // > 0: forced number of token slices of a matrix-shaped weight gradient (tools/wgrad_bench.py)
int g_opt_wgrad_cap = 128;          // token slices of a conv-shaped weight gradient (few output tiles, 10^5+ rows)
int g_opt_variant = 1;            // 1 = auto; tuning knobs (yv_set_option): linear kernel variant, M-group size, persistent grid
int g_opt_group_m = 8;
int g_opt_staged = 1;
int g_opt_p8 = 3;                  // persistent kernels: 0 off, 1 8-phase kernel for wide bf16-output linears only (qkv, fc1), 2 for every
                                   // eligible linear incl. the f32 residual ones (proj, fc2), 3 the free-running kernel (gemm_p9_kernel): "linear_p8"
std::mutex g_ws_mu;
std::map<void*, std::pair<void*, size_t>> g_ws;   // per-stream split-K workspace (yv_set_workspace)
static bool ws_lookup(void* stream, void** ws, size_t* bytes) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    auto it = g_ws.find(stream);
    if (it == g_ws.end()) return false;
    *ws = it->second.first; *bytes = it->second.second;
    return true;
}
int g_opt_linear_splitk = 1;
int g_opt_splitk = 0;           // measured neutral end-to-end (tools/e2e_ab.py): the reduce pass costs what the shorter chain saves
constexpr int THREADS = 256;

// x * sigmoid(x) through the hardware reciprocal (1 ulp) instead of an IEEE division: the division's scale / fixup sequence was
// ~12 of the ~20 VALU instructions per output value of every detector convolution, in kernels that are VALU-issue-bound.
__device__ __forceinline__ float silu_f(float x) { return x * __builtin_amdgcn_rcpf(1.0f + __expf(-x)); }
// XCD-aware bijective remap of a 1-D grid of nwg workgroups: the hardware deals workgroups round robin over the eight XCDs, so XCD
// x takes the x-th contiguous run of tiles (q + 1 tiles for the first nwg & 7 XCDs, q for the rest) and neighbours share its L2
__device__ __forceinline__ int xcd_remap(int bid, int nwg) {
    const int q = nwg >> 3, r = nwg & 7, x = bid & 7;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + (bid >> 3);
}
// what a DMA lane passes for a row that reads nothing: past the descriptor's range, i.e. zeros in LDS
constexpr uint32_t DMA_OOB = 0x80000000u;
// 256 bytes of zeros: where a staged chunk is padding (outside the image, past K, past the last row) the conv / linear gather
// reads THIS instead of branching around the load or masking the data afterwards
__device__ __attribute__((aligned(256))) uint32_t g_zero_page[64];
// STATS (yv_conv2d_stats): cs / cq (NF * 4 floats each, zeroed by the caller) receive this lane's column sums of the bf16-rounded
// values it stores and of their squares, rows in ascending fragment order; rows >= M and columns >= N add nothing.
// PHASE (yv_conv2d_dgrad_s2): row m = (b, i, j) of the Hout x Wout gradient grid is pixel (b, 2i + py, 2j + px) of the output and of
// the residual, ph = py * 2 + px being the workgroup's phase.
// BNBWD (yv_conv2d_bnbwd): the value stored is the gradient da of a BatchNorm block's output; cs / cq (as STATS) receive this lane's
// column sums of g = da * act'(u) and of g * xhat (bn_act_grad_term: the text of chan_reduce_kernel<1>), da being the bf16-rounded
// value it stores and z the block's pre-activation at the same row and column.  The z loads of all of the lane's rows are issued
// before the first store, so that their latency lies under the bias / residual / store work of the fragment.
template <bool PHASE>
__device__ __forceinline__ long long phase_row(const GemmArgs& g, int m, int ph) {
    if constexpr (!PHASE) return m;
    const int hw = g.Hout * g.Wout;
    const int b = m / hw, rem = m - b * hw;
    const int i = rem / g.Wout, j = rem - i * g.Wout;
    return ((long long)b * (2 * g.Hout) + 2 * i + (ph >> 1)) * (2 * g.Wout) + 2 * j + (ph & 1);
}

template <int MF, int NF, bool STATS = false, bool PHASE = false, bool BNBWD = false>
__device__ __forceinline__ void epilogue(const GemmArgs& g, f32x4 (&acc)[NF][MF], int M, int m0, int n0, int wrow_m,
                                         int wrow_n, int fr, int fq, float* cs = nullptr, float* cq = nullptr, int ph = 0) {
    // ---- epilogue: lane owns channels n..n+3 of row m --------------------------------------
    static_assert(!(BNBWD && (STATS || PHASE)), "one kind of column sums, none of a phase launch");
    const int flags = g.flags;
    [[maybe_unused]] float4 c_mu[NF], c_rs[NF], c_ga[NF], c_be[NF];
    [[maybe_unused]] uint2 zz[NF][MF];
    if constexpr (BNBWD) {
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int n = n0 + wrow_n + i * 16 + fq * 4;
            const bool ok = n < g.N;
            const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
            c_mu[i] = ok ? *(const float4*)(g.bn_mean + n) : zero; c_rs[i] = ok ? *(const float4*)(g.bn_rstd + n) : zero;
            c_ga[i] = ok ? *(const float4*)(g.bn_gamma + n) : zero; c_be[i] = ok ? *(const float4*)(g.bn_beta + n) : zero;
#pragma unroll
            for (int j = 0; j < MF; ++j) {
                const int m = m0 + wrow_m + j * 16 + fr;
                zz[i][j] = (ok && m < M) ? *(const uint2*)(g.z + (long long)m * g.ldz + n) : make_uint2(0u, 0u);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MF; ++j) {
        const int m = m0 + wrow_m + j * 16 + fr;
        if (m >= M) continue;
        long long orow = m;
        if constexpr (PHASE) orow = phase_row<true>(g, m, ph);
        const float* posrow = nullptr;
        if (flags & YV_EPI_POSEMB) {
            const int r = m / g.tok, t = m - r * g.tok;
            orow = (long long)r * (g.tok + 1) + 1 + t;
            posrow = g.pos + (long long)(1 + t) * g.N;
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int n = n0 + wrow_n + i * 16 + fq * 4;
            if (n >= g.N) continue;
            float v[4] = {acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]};
            if (flags & YV_EPI_BIAS) {
                const float4 b = *(const float4*)(g.bias + n);
                v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
            }
            if (flags & YV_EPI_SILU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = silu_f(v[q]);
            }
            if (flags & YV_EPI_GELU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = gelu_f(v[q]);
            }
            if (flags & YV_EPI_RES_BF16) {
                const uint2 rr = *(const uint2*)(g.res + orow * g.ldres + n);
                v[0] += bf16_to_f32((uint16_t)(rr.x & 0xffff)); v[1] += bf16_to_f32((uint16_t)(rr.x >> 16));
                v[2] += bf16_to_f32((uint16_t)(rr.y & 0xffff)); v[3] += bf16_to_f32((uint16_t)(rr.y >> 16));
            }
            if (posrow) {
                const float4 pp = *(const float4*)(posrow + n);
                v[0] += pp.x; v[1] += pp.y; v[2] += pp.z; v[3] += pp.w;
            }
            if (flags & (YV_EPI_OUT_F32 | YV_EPI_RES_F32)) {
                float* o = (float*)g.out + orow * g.ldo + n;
                if (flags & YV_EPI_RES_F32) {
                    const float4 x = *(const float4*)o;
                    v[0] += x.x; v[1] += x.y; v[2] += x.z; v[3] += x.w;
                }
                *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
            } else {
                uint16_t* o = (uint16_t*)g.out + orow * g.ldo + n;
                *(uint2*)o = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
                if constexpr (STATS) {
                    const uint32_t pk[2] = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float f = bf16_to_f32((uint16_t)(q & 1 ? pk[q >> 1] >> 16 : pk[q >> 1] & 0xffff));
                        cs[i * 4 + q] += f; cq[i * 4 + q] += f * f;
                    }
                }
                if constexpr (BNBWD) {
                    const uint32_t pk[2] = {pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3])}, zk[2] = {zz[i][j].x, zz[i][j].y};
                    const float mu[4] = {c_mu[i].x, c_mu[i].y, c_mu[i].z, c_mu[i].w}, rs[4] = {c_rs[i].x, c_rs[i].y, c_rs[i].z, c_rs[i].w};
                    const float ga[4] = {c_ga[i].x, c_ga[i].y, c_ga[i].z, c_ga[i].w}, be[4] = {c_be[i].x, c_be[i].y, c_be[i].z, c_be[i].w};
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        const float d = bf16_to_f32((uint16_t)(q & 1 ? pk[q >> 1] >> 16 : pk[q >> 1] & 0xffff));
                        const float z = bf16_to_f32((uint16_t)(q & 1 ? zk[q >> 1] >> 16 : zk[q >> 1] & 0xffff));
                        float xh;
                        const float gr = bn_act_grad_term(d, z, mu[q], rs[q], ga[q], be[q], g.bn_act, xh);
                        cs[i * 4 + q] += gr; cq[i * 4 + q] += gr * xh;
                    }
                }
            }
        }
    }
}


// The bf16 slab of the staged epilogues: a wave's MF * 16 rows x 128 B, the 16-byte chunk index XOR-swizzled with row & 7.
// slab_put: the four values of accumulator fragment (i, j) of lane (fr, fq); slab_row: the 8 consecutive columns ch * 8 .. of a row.
__device__ __forceinline__ void slab_put(unsigned char* stage, int i, int j, int fr, int fq, const float* v) {
    const int row = j * 16 + fr, c16 = i * 2 + (fq >> 1);
    *(uint2*)(stage + row * 128 + ((c16 ^ (row & 7)) << 4) + (fq & 1) * 8) = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
}
__device__ __forceinline__ uint4 slab_row(const unsigned char* stage, int row, int ch) {
    return *(const uint4*)(stage + row * 128 + ((ch ^ (row & 7)) << 4));
}
// a + b of 8 bf16 values each, in f32, rounded to bf16 (the bf16 shortcut / residual)
__device__ __forceinline__ uint4 add_bf16x8(const uint4 pa, const uint4 pb) {
    const uint32_t a[4] = {pa.x, pa.y, pa.z, pa.w}, b[4] = {pb.x, pb.y, pb.z, pb.w};
    uint32_t o[4];
#pragma unroll
    for (int q = 0; q < 4; ++q)
        o[q] = pack_bf16x2(bf16_to_f32((uint16_t)(a[q] & 0xffff)) + bf16_to_f32((uint16_t)(b[q] & 0xffff)),
                           bf16_to_f32((uint16_t)(a[q] >> 16)) + bf16_to_f32((uint16_t)(b[q] >> 16)));
    return make_uint4(o[0], o[1], o[2], o[3]);
}
// 8 bf16 values of a lane, 32-column block shared with the lanes at xor 1 and 2 -> 8 e4m3 bytes; returns the block exponent
__device__ __forceinline__ int mx_quant_bf16x8(const uint4 pk, uint2& q8) {
    float f[8];
    unpack_bf16x8((u32x4){pk.x, pk.y, pk.z, pk.w}, f);
    uint32_t p[2];
    const int e = mx_quant_block<1, 2>(f, p);
    q8 = make_uint2(p[0], p[1]);
    return e;
}

// Coalesced epilogue for 64-column wave tiles (NF == 4).  The ablation of the first version showed
// the direct epilogue (8-byte stores, 32-byte row segments) costing 41 % of a K = 768 GEMM: the
// output left at ~2 TB/s.  Here each wave transposes its tile through a private, XOR-swizzled LDS
// slab (reusing the main-loop buffers after the loop's last barrier) and writes whole 128-byte
// (bf16) / 256-byte (f32) row segments with 16-byte stores; residual reads are coalesced the same way.
// STATS (yv_conv2d_stats, bf16 output): cs / cq (8 floats each, zeroed by the caller) receive the column sums of the 8 channels
// this lane stores (n = n0 + wrow_n + (lane & 7) * 8 ..) and of their squares, its rows (lane >> 3) + 8 * it in ascending order.
// BNBWD (yv_conv2d_bnbwd, bf16 output): cs / cq likewise receive the sums of g and g * xhat (see epilogue); the 16-byte z loads of
// the lane's first MF rows are issued before the slab is written, so that the transpose covers them, those of the other MF rows and
// the constants behind the slab writes, where the accumulators' registers are free (all at the top: one workgroup per CU fewer on
// the 128-wide tiles).
template <int MF, bool STATS = false, bool PHASE = false /* bf16 output only: the row map of phase_row */, bool BNBWD = false>
__device__ __forceinline__ void epilogue_staged(const GemmArgs& g, f32x4 (&acc)[4][MF], int M, int m0, int n0,
                                                int wrow_m, int wrow_n, int lane, unsigned char* stage, float* cs = nullptr,
                                                float* cq = nullptr, int ph = 0) {
    static_assert(!(BNBWD && (STATS || PHASE)), "one kind of column sums, none of a phase launch");
    const int flags = g.flags;
    const int fr = lane & 15, fq = lane >> 4;
    const int nb = n0 + wrow_n;
    [[maybe_unused]] uint4 zq[MF * 2];
    [[maybe_unused]] float c_mu[8], c_rs[8], c_ga[8], c_be[8];
    auto z_rows = [&](int first) {                   // the 16-byte z loads of MF of the lane's MF * 2 rows
        const int n = nb + (lane & 7) * 8;
#pragma unroll
        for (int it = first; it < first + MF; ++it) {
            const int m = m0 + wrow_m + it * 8 + (lane >> 3);
            zq[it] = (m < M && n < g.N) ? *(const uint4*)(g.z + (long long)m * g.ldz + n) : make_uint4(0u, 0u, 0u, 0u);
        }
    };
    if constexpr (BNBWD) z_rows(0);                  // in flight under the slab writes
    float4 bv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int n = nb + i * 16 + fq * 4;
        bv[i] = ((flags & YV_EPI_BIAS) && n < g.N) ? *(const float4*)(g.bias + n) : make_float4(0.f, 0.f, 0.f, 0.f);
    }
    auto value = [&](int i, int j, float* v, bool act = true) {
        v[0] = acc[i][j][0] + bv[i].x; v[1] = acc[i][j][1] + bv[i].y;
        v[2] = acc[i][j][2] + bv[i].z; v[3] = acc[i][j][3] + bv[i].w;
        if (!act) return;
        if (flags & YV_EPI_SILU) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = silu_f(v[q]);
        }
        if (flags & YV_EPI_GELU) {
#pragma unroll
            for (int q = 0; q < 4; ++q) v[q] = gelu_f(v[q]);
        }
    };
    if (!(flags & (YV_EPI_OUT_F32 | YV_EPI_RES_F32))) {
        // ---- bf16 output: MF*16 rows x 128 B slab -------------------------------------------------
        if (flags & YV_EPI_SAVE_PRE) {           // training: keep the pre-activation (GELU'(u) needs it)
#pragma unroll
            for (int j = 0; j < MF; ++j)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v[4];
                    value(i, j, v, false);
                    slab_put(stage, i, j, fr, fq, v);
                }
#pragma unroll
            for (int it = 0; it < MF * 2; ++it) {
                const int row = it * 8 + (lane >> 3), ch = lane & 7;
                const int m = m0 + wrow_m + row, n = nb + ch * 8;
                const uint4 pk = slab_row(stage, row, ch);
                if (m < M && n < g.N) *(uint4*)(g.aux + (long long)m * g.ldaux + n) = pk;
            }
        }
#pragma unroll
        for (int j = 0; j < MF; ++j)
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float v[4];
                value(i, j, v);
                slab_put(stage, i, j, fr, fq, v);
            }
        if constexpr (BNBWD) {                   // (here, not at the top: the accumulators are in the slab, their registers free)
            z_rows(MF);                              // the other half: in flight under the first half's terms
            const int n = nb + (lane & 7) * 8;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const bool ok = n < g.N;                 // (N % 8 == 0: a lane's 8 columns are inside or outside together)
                const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
                const float4 a = ok ? *(const float4*)(g.bn_mean + n + h * 4) : zero, b = ok ? *(const float4*)(g.bn_rstd + n + h * 4) : zero;
                const float4 c = ok ? *(const float4*)(g.bn_gamma + n + h * 4) : zero, d = ok ? *(const float4*)(g.bn_beta + n + h * 4) : zero;
                c_mu[h * 4] = a.x; c_mu[h * 4 + 1] = a.y; c_mu[h * 4 + 2] = a.z; c_mu[h * 4 + 3] = a.w;
                c_rs[h * 4] = b.x; c_rs[h * 4 + 1] = b.y; c_rs[h * 4 + 2] = b.z; c_rs[h * 4 + 3] = b.w;
                c_ga[h * 4] = c.x; c_ga[h * 4 + 1] = c.y; c_ga[h * 4 + 2] = c.z; c_ga[h * 4 + 3] = c.w;
                c_be[h * 4] = d.x; c_be[h * 4 + 1] = d.y; c_be[h * 4 + 2] = d.z; c_be[h * 4 + 3] = d.w;
            }
        }
#pragma unroll
        for (int it = 0; it < MF * 2; ++it) {
            const int row = it * 8 + (lane >> 3), ch = lane & 7;
            const int m = m0 + wrow_m + row, n = nb + ch * 8;
            uint4 pk = slab_row(stage, row, ch);
            if (m < M && n < g.N) {
                [[maybe_unused]] long long om = 0;
                if constexpr (PHASE) om = phase_row<true>(g, m, ph);
                if (flags & YV_EPI_RES_BF16) pk = add_bf16x8(pk, *(const uint4*)(g.res + (PHASE ? om : (long long)m) * g.ldres + n));
                if (flags & YV_EPI_OUT_MXFP8) {
                    // the consumer is another MXFP8 GEMM: quantise the 8 (bf16-rounded) values of this lane together with
                    // the 3 lanes that hold the rest of their 32-column block, skip the bf16 store
                    uint2 q8;
                    const int e = mx_quant_bf16x8(pk, q8);
                    *(uint2*)(g.mxq + (long long)m * g.ldmxq + n) = q8;
                    if ((ch & 3) == 0) g.mxs[mx_scale_kmajor(n >> 5, g.mx_rows, m)] = (uint8_t)(e + 127);
                    continue;
                }
                if (flags & YV_EPI_GELU_BWD) {      // out = dg * gelu'(u), u = saved pre-activation (bf16)
                    const uint4 uu = *(const uint4*)(g.aux + (long long)m * g.ldaux + n);
                    const uint32_t a[4] = {pk.x, pk.y, pk.z, pk.w}, b[4] = {uu.x, uu.y, uu.z, uu.w};
                    uint32_t o[4];
#pragma unroll
                    for (int q = 0; q < 4; ++q)
                        o[q] = pack_bf16x2(bf16_to_f32((uint16_t)(a[q] & 0xffff)) * gelu_grad_f(bf16_to_f32((uint16_t)(b[q] & 0xffff))),
                                           bf16_to_f32((uint16_t)(a[q] >> 16)) * gelu_grad_f(bf16_to_f32((uint16_t)(b[q] >> 16))));
                    pk = make_uint4(o[0], o[1], o[2], o[3]);
                }
                *(uint4*)((uint16_t*)g.out + (PHASE ? om : (long long)m) * g.ldo + n) = pk;
                if constexpr (STATS) {
                    const uint32_t a[4] = {pk.x, pk.y, pk.z, pk.w};
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const float f = bf16_to_f32((uint16_t)(q & 1 ? a[q >> 1] >> 16 : a[q >> 1] & 0xffff));
                        cs[q] += f; cq[q] += f * f;
                    }
                }
                if constexpr (BNBWD) {
                    const uint32_t a[4] = {pk.x, pk.y, pk.z, pk.w}, b[4] = {zq[it].x, zq[it].y, zq[it].z, zq[it].w};
#pragma unroll
                    for (int q = 0; q < 8; ++q) {
                        const float d = bf16_to_f32((uint16_t)(q & 1 ? a[q >> 1] >> 16 : a[q >> 1] & 0xffff));
                        const float z = bf16_to_f32((uint16_t)(q & 1 ? b[q >> 1] >> 16 : b[q >> 1] & 0xffff));
                        float xh;
                        const float gr = bn_act_grad_term(d, z, c_mu[q], c_rs[q], c_ga[q], c_be[q], g.bn_act, xh);
                        cs[q] += gr; cq[q] += gr * xh;
                    }
                }
            }
        }
    } else {
        // ---- f32 output / residual stream: two passes of MF*8 rows x 256 B ----------------------------
#pragma unroll
        for (int half = 0; half < 2; ++half) {
#pragma unroll
            for (int jj = 0; jj < MF / 2; ++jj)
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    float v[4];
                    value(i, half * (MF / 2) + jj, v);
                    const int row = jj * 16 + fr, c16 = i * 4 + fq;
                    *(float4*)(stage + row * 256 + ((c16 ^ (row & 15)) << 4)) = make_float4(v[0], v[1], v[2], v[3]);
                }
#pragma unroll
            for (int it = 0; it < MF * 2; ++it) {
                const int row = it * 4 + (lane >> 4), ch = lane & 15;
                const int m = m0 + wrow_m + half * (MF * 8) + row, n = nb + ch * 4;
                float4 v = *(const float4*)(stage + row * 256 + ((ch ^ (row & 15)) << 4));
                if (m < M && n < g.N) {
                    long long orow = m;
                    if (flags & YV_EPI_POSEMB) {
                        const int r = m / g.tok, t = m - r * g.tok;
                        orow = (long long)r * (g.tok + 1) + 1 + t;
                        const float4 pp = *(const float4*)(g.pos + (long long)(1 + t) * g.N + n);
                        v.x += pp.x; v.y += pp.y; v.z += pp.z; v.w += pp.w;
                    }
                    float* o = (float*)g.out + orow * g.ldo + n;
                    if (flags & YV_EPI_RES_F32) {
                        const float4 x = g.resf ? *(const float4*)(g.resf + orow * g.ldo + n) : *(const float4*)o;
                        v.x += x.x; v.y += x.y; v.z += x.z; v.w += x.w;
                    }
                    *(float4*)o = v;
                }
            }
        }
    }
}

// STATS (yv_conv2d_stats; WM row-group waves, BN tile columns, tm the tile's row index): the workgroup also writes the column sums
// of what it stored to g.stats[(tm * 2 + which) * N + n] (which 0: sum, 1: sum of squares), each float by one plain store.
// Summation order: a lane's rows in ascending order (the epilogues), then the lanes that hold the same columns by an xor
// butterfly (both partners compute the same sum), then the WM waves in wave order through LDS.  The scratch (WM x 2 x BN floats)
// lies at the start of the tile buffers, i.e. inside the staged epilogue's slabs: a barrier that every wave reaches (its rows
// may all lie past M - it then adds zeros) separates the two uses.  g.staged is the same for the whole launch.
// BNBWD (yv_conv2d_bnbwd): the same path and layout with the epilogues' other pair of sums (which 0: sum g, 1: sum g * xhat).
template <int MF, int NF, bool STATS = false, int WM = 1, int BN = 16, bool PHASE = false, bool BNBWD = false>
__device__ __forceinline__ void finish_tile(const GemmArgs& g, f32x4 (&acc)[NF][MF], int M, int m0, int n0, int wrow_m,
                                            int wrow_n, int lane, int wave, unsigned char* smem, int tm = 0, int ph = 0) {
    static_assert(!((STATS || BNBWD) && PHASE), "no column sums of a phase launch");
    static_assert(!(STATS && BNBWD), "one kind of column sums");
    if constexpr (STATS || BNBWD) {
        float* const sc = (float*)smem + (wrow_m / (MF * 16)) * 2 * BN + wrow_n;      // this wave's [which][column] rows
        bool staged = false;
        if constexpr (NF == 4 && (MF % 2) == 0) staged = g.staged;
        if constexpr (NF == 4 && (MF % 2) == 0) {
            if (staged) {
                float cs[8], cq[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) cs[q] = cq[q] = 0.f;
                epilogue_staged<MF, STATS, false, BNBWD>(g, acc, M, m0, n0, wrow_m, wrow_n, lane, smem + wave * (MF * 16 * 128), cs, cq);
#pragma unroll
                for (int q = 0; q < 8; ++q)
#pragma unroll
                    for (int d = 8; d < 64; d <<= 1) { cs[q] += __shfl_xor(cs[q], d, 64); cq[q] += __shfl_xor(cq[q], d, 64); }
                __syncthreads();                              // every wave is done with its slab
                if (lane < 8) {
#pragma unroll
                    for (int q = 0; q < 8; ++q) { sc[lane * 8 + q] = cs[q]; sc[BN + lane * 8 + q] = cq[q]; }
                }
            }
        }
        if (!staged) {
            // one 16-column fragment at a time (8 sums live); the direct epilogue leaves the tile buffers idle: no barrier before
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                float cs[4] = {0.f, 0.f, 0.f, 0.f}, cq[4] = {0.f, 0.f, 0.f, 0.f};
                epilogue<MF, 1, STATS, false, BNBWD>(g, reinterpret_cast<f32x4 (&)[1][MF]>(acc[i]), M, m0, n0, wrow_m, wrow_n + i * 16,
                                                     lane & 15, lane >> 4, cs, cq);
#pragma unroll
                for (int q = 0; q < 4; ++q)
#pragma unroll
                    for (int d = 1; d < 16; d <<= 1) { cs[q] += __shfl_xor(cs[q], d, 64); cq[q] += __shfl_xor(cq[q], d, 64); }
                if ((lane & 15) == 0) {
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        sc[i * 16 + (lane >> 4) * 4 + q] = cs[q];
                        sc[BN + i * 16 + (lane >> 4) * 4 + q] = cq[q];
                    }
                }
            }
        }
        __syncthreads();
        for (int idx = threadIdx.x; idx < 2 * BN; idx += THREADS) {
            const int which = idx / BN, col = idx - which * BN;
            float t = 0.f;
#pragma unroll
            for (int w = 0; w < WM; ++w) t += ((const float*)smem)[(w * 2 + which) * BN + col];
            if (n0 + col < g.N) g.stats[((long long)tm * 2 + which) * g.N + n0 + col] = t;
        }
        return;
    }
    if constexpr (NF == 4 && (MF % 2) == 0) {
        if (g.staged) {          // wave-private slab of MF*16 rows x 128 B inside the (now idle) tile buffers
            epilogue_staged<MF, false, PHASE>(g, acc, M, m0, n0, wrow_m, wrow_n, lane, smem + wave * (MF * 16 * 128), nullptr, nullptr,
                                              ph);
            return;
        }
    }
    epilogue<MF, NF, false, PHASE>(g, acc, M, m0, n0, wrow_m, wrow_n, lane & 15, lane >> 4, nullptr, nullptr, ph);
}

// ---- PHASE form of the convolution kernels (yv_conv2d_dgrad_s2): the data gradient of a 3 x 3 / stride 2 convolution --------------
// One launch holds the four parity phases (py, px) of the output pixel (2i + py, 2j + px), heaviest first: the workgroup id picks the
// phase (ph = py * 2 + px), then the tile inside it.  Per axis parity 0 takes wd slot row 1 at displacement 0, parity 1 takes slot
// row 0 at displacement 0 and slot row 2 at displacement + 1; the phase's taps are walked in ascending slot (3 * row + col) order,
// which is the order the stride-1 convolution over the zero-inserted gradient meets its non-zero terms.  The source grid is the
// Hout x Wout gradient itself (g.Hin = g.Hout, g.stride = 1), g.c0 its channels (a multiple of 64: a K step lies inside one tap),
// g.K = 9 * g.c0 the row stride of wd (Cin, 9, Cout); no tap lies before the pixel, so the descriptor needs no negative bias.
__device__ __forceinline__ int phase_of_block(const GemmArgs& g, int& bid) {
    const int per = g.tiles_m * g.tiles_n;
    const int q = bid / per;                      // launch order 0 .. 3: (1,1) four taps, (1,0) and (0,1) two, (0,0) one
    bid -= q * per;
    return 3 - (g.group_m + q);
}
__device__ __forceinline__ int phase_ksteps(const GemmArgs& g, int ph) { return ((ph >> 1) + 1) * ((ph & 1) + 1) * (g.c0 / BK); }
// validity of the nine wd slots for the pixel (oy, ox): slot row / column 2 reads the next gradient row / column
__device__ __forceinline__ uint32_t phase_taps(const GemmArgs& g, int oy, int ox) {
    const uint32_t rows = oy + 1 < g.Hout ? 0x1ffu : 0x03fu, cols = ox + 1 < g.Wout ? 0x1ffu : 0x0dbu;
    return rows & cols;
}
// K step at element kb of phase ph -> wd slot, byte displacement of its source pixel (+ channel), byte column in a wd row
struct PhaseStep { int slot; uint32_t src, wcol; };
__device__ __forceinline__ PhaseStep phase_step(const GemmArgs& g, int ph, int kb) {
    const int t = g.cin_shift >= 0 ? (kb >> g.cin_shift) : kb / g.c0;
    const int c = kb - t * g.c0;
    const int px = ph & 1, py = ph >> 1;
    const int row = py ? 2 * (px ? t >> 1 : t) : 1, col = px ? 2 * (t & 1) : 1;
    PhaseStep s;
    s.slot = 3 * row + col;
    s.src = (uint32_t)((((row >> 1) * g.Win + (col >> 1)) * g.lda0 + c) * 2);
    s.wcol = (uint32_t)((s.slot * g.c0 + c) * 2);
    return s;
}

template <int MODE /*0 linear, 1 conv*/, int BM, int BN, int WM, int WN, bool TWO = false /*conv with two concatenated sources*/,
          bool STATS = false /*conv that also writes its tile's column sums (finish_tile)*/,
          bool PHASE = false /*stride-2 data gradient by parity phase (above)*/,
          bool BNBWD = false /*data gradient that also writes its tile's BatchNorm backward sums (finish_tile)*/>
__global__ __launch_bounds__(THREADS) void igemm_kernel(GemmArgs g) {
    static_assert(!PHASE || (MODE == 1 && !TWO && !STATS), "the phase form is a one-source convolution");
    static_assert(!BNBWD || (MODE == 1 && !TWO && !STATS && !PHASE), "the sums form is a one-source convolution, no phase form");
    constexpr int MF = BM / WM / 16;               // activation fragments per wave
    constexpr int NF = BN / WN / 16;               // weight fragments per wave
    constexpr int A_CH = BM * 8 / THREADS;         // 16-byte chunks per thread per K step (activations)
    constexpr int W_CH = (BN * 8 + THREADS - 1) / THREADS;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    // [buf][A tile | W tile]
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }

    // XCD-aware bijective remap of the 1-D grid
    int bid = blockIdx.x;
    int nwg = gridDim.x, ph = 0;
    if constexpr (PHASE) { ph = phase_of_block(g, bid); nwg = g.tiles_m * g.tiles_n; }
    bid = xcd_remap(bid, nwg);
    const int S = g.splitk > 1 ? g.splitk : 1;
    const int slice = bid % S;                 // K slices of one tile are neighbours: their A/W rows share L2
    bid /= S;
    const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    // ---- per-thread staging coordinates -------------------------------------------------
    // Everything that does not change along K is worked out once per tile: per activation row the byte offset of the output
    // pixel's centre in each source and the 3 x 3 taps that fall inside the image (9 bits), per weight row its byte offset.  A K
    // step then costs one tap decode per thread (its 8-channel chunk is fixed) and an add + a bit test per 16-byte load - the
    // first version redid the pixel arithmetic (64-bit multiplies, a division) for every load: 45 VALU instructions per load,
    // 330 per wave and step against 32 MFMAs (SQ_INSTS_VALU / SQ_INSTS_VMEM_RD over the detector's launches).
    const int ch = tid & 7;                        // chunk (8 elements) within the 64-wide K step
    const int r_in = tid >> 3;                     // 0..31
    // activation rows handled by this thread: r_in + 32*p
    int a_valid[A_CH];
    long long a_base[A_CH];                        // linear: row offset
    uint32_t a_off0[A_CH], a_off1[A_CH], a_taps[A_CH];      // conv (32-bit byte offsets: conv_impl bounds the tensors)
    const int pad = g.ksize >> 1;
    const int Cin = g.c0 + g.c1;
#pragma unroll
    for (int p = 0; p < A_CH; ++p) {
        const int m = m0 + r_in + 32 * p;
        a_valid[p] = m < M;
        if (MODE == 0) {
            a_base[p] = (long long)m * g.lda0;
        } else {
            const int hw = g.Hout * g.Wout;
            const int b = m / hw, rem = m - b * hw;
            const int oy = rem / g.Wout;
            const int cy = oy * g.stride, cx = (rem - oy * g.Wout) * g.stride;
            // (both include this lane's 8-channel chunk; a_off1 is kept as the DIFFERENCE to a_off0: a runtime choice between two
            //  register arrays would put both in scratch)
            a_off0[p] = (uint32_t)((((long long)b * (g.Hin >> g.up0) + (cy >> g.up0)) * (g.Win >> g.up0) + (cx >> g.up0)) * g.lda0 * 2) + ch * 16;
            a_off1[p] = g.c1 ? (uint32_t)((((long long)b * (g.Hin >> g.up1) + (cy >> g.up1)) * (g.Win >> g.up1) + (cx >> g.up1)) * g.lda1 * 2) + ch * 16 - a_off0[p] : 0u;
            uint32_t taps = 0;
            if (a_valid[p]) {
                if constexpr (PHASE) {
                    taps = phase_taps(g, cy, cx);
                } else if (g.ksize == 3) {
#pragma unroll
                    for (int t = 0; t < 9; ++t) {
                        const int iy = cy + t / 3 - 1, ix = cx + t % 3 - 1;
                        taps |= (iy >= 0 && iy < g.Hin && ix >= 0 && ix < g.Win) ? (1u << t) : 0u;
                    }
                } else {
                    taps = 1u;
                }
            }
            a_taps[p] = taps;
        }
    }
    uint32_t w_off[W_CH];
    bool w_ok[W_CH];
#pragma unroll
    for (int p = 0; p < W_CH; ++p) {
        const int rr = r_in + 32 * p;
        w_ok[p] = rr < BN && (n0 + rr) < g.N;
        w_off[p] = (uint32_t)(((long long)(n0 + rr) * g.K + ch * 8) * 2);
    }

    // Loads are UNCONDITIONAL.  Written as "if (valid) r = load" hipcc branches around every load and waits vmcnt(0) before the
    // next one - 8 dependent memory round trips per K step instead of 8 loads in flight (s_waitcnt vmcnt(0) in front of every
    // global_load of the first version).  Conv: buffer loads, a chunk that is padding / past K / past the last row gets an
    // out-of-range offset and reads zeros through the descriptor's range check; whatever is the same for the whole workgroup in a
    // K step (the tap's displacement, the channel base, the weight column) travels in the instruction's SCALAR offset, so a load
    // costs a bit test and a select.  The scalar offset is unsigned, hence the descriptor's base one row + one pixel before the
    // tensor.  Linear: a 64-bit address chosen between the operand and g_zero_page.
    uint4 ra[A_CH], rw[W_CH];
    const unsigned char* zp = (const unsigned char*)g_zero_page;
    typedef const __attribute__((address_space(1))) u32x4* g16_t;   // (global, not generic: a flat load would also count in lgkmcnt)
    auto ld16 = [&](bool ok, const unsigned char* ptr) __attribute__((always_inline)) {
        g16_t q = (g16_t)(ok ? ptr : zp);
        asm volatile("" : "+v"(q));                         // an opaque VALUE: hipcc would turn the choice back into two branches
        const u32x4 v = *q;
        return make_uint4(v[0], v[1], v[2], v[3]);
    };
    constexpr uint32_t OOB = 0x80000000u;
    const uint32_t bias0 = MODE == 1 && !PHASE && g.ksize == 3 ? (uint32_t)((g.Win + 1) * g.lda0 * 2) : 0u;
    // (copies first: a ternary between two FIELDS of the by-value kernel argument selects between their addresses; and the
    //  descriptors are built inside the lambda - captured by reference they are objects hipcc cannot keep out of memory, and the
    //  whole closure, kernel argument included, lands in scratch)
    const unsigned char* const a0p = (const unsigned char*)g.a0 - bias0;
    const unsigned char* const a1p = (const unsigned char*)g.a1;
    const unsigned char* const wp = (const unsigned char*)g.w;
    auto load_tile = [&](int kt) __attribute__((always_inline)) {
        const int kb = kt * BK;                                // (uniform)
        const int k = kb + ch * 8;
        const bool k_ok = k < g.K;
        if (MODE == 0) {
#pragma unroll
            for (int p = 0; p < A_CH; ++p)
                ra[p] = ld16(k_ok && a_valid[p], (const unsigned char*)(g.a0 + a_base[p] + k));
#pragma unroll
            for (int p = 0; p < W_CH; ++p)
                rw[p] = ld16(w_ok[p] && k_ok, (const unsigned char*)g.w + (uint32_t)(w_off[p] + (uint32_t)kb * 2));
        } else if constexpr (TWO) {
            // two concatenated sources (1 x 1 convolutions after a Concat): the source is a per-lane property in general, so this
            // instance keeps 64-bit addresses (a choice between two descriptors - as objects, as base pointers, or as two
            // branches that both load into ra[] - makes hipcc keep the arrays and the kernel argument in scratch)
            const bool s1 = k_ok && k >= g.c0;
            const unsigned char* src = (const unsigned char*)(s1 ? a1p : a0p);
            const uint32_t m1 = s1 ? 0xFFFFFFFFu : 0u;
            const uint32_t d = (uint32_t)((s1 ? k - g.c0 : k) * 2) - ch * 16;
#pragma unroll
            for (int p = 0; p < A_CH; ++p)
                ra[p] = ld16(k_ok && (a_taps[p] & 1u), src + (uint32_t)(a_off0[p] + (a_off1[p] & m1) + d));
#pragma unroll
            for (int p = 0; p < W_CH; ++p)
                rw[p] = ld16(w_ok[p] && k_ok, wp + (uint32_t)(w_off[p] + (uint32_t)kb * 2));
        } else {
            int tap = 0;                                       // (per lane only when a K step spans several taps: Cin < 64)
            uint32_t soff = bias0, dl = 0, wcol = 0;            // (wcol: PHASE only)
            if constexpr (PHASE) {
                const PhaseStep ps = phase_step(g, ph, kb);
                tap = ps.slot;
                soff = (uint32_t)__builtin_amdgcn_readfirstlane((int)ps.src);
                wcol = (uint32_t)__builtin_amdgcn_readfirstlane((int)ps.wcol);
            } else if (g.ksize == 3) {
                const int kk = g.tap_uniform ? kb : k;
                tap = g.cin_shift >= 0 ? (kk >> g.cin_shift) : kk / Cin;
                const int cin = kk - tap * Cin;
                const int ky = tap >= 6 ? 2 : (tap >= 3 ? 1 : 0), kx = tap - ky * 3;
                const uint32_t d = (uint32_t)((((ky - pad) * g.Win + (kx - pad)) * g.lda0 + cin) * 2);
                if (g.tap_uniform) soff += (uint32_t)__builtin_amdgcn_readfirstlane((int)d);
                else dl = d - ch * 16;
            } else {
                soff = (uint32_t)(kb * 2);
            }
            const auto rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)a0p, 0, 0x7fffffff, 0x00020000);
#pragma unroll
            for (int p = 0; p < A_CH; ++p) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rs0, (k_ok && ((a_taps[p] >> tap) & 1u)) ? a_off0[p] + dl : OOB, soff, 0);
                ra[p] = make_uint4(v[0], v[1], v[2], v[3]);
            }
            const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)wp, 0, 0x7fffffff, 0x00020000);
#pragma unroll
            for (int p = 0; p < W_CH; ++p) {
                const u32x4 v = __builtin_amdgcn_raw_buffer_load_b128(rsW, (w_ok[p] && k_ok) ? w_off[p] : OOB, PHASE ? wcol : (uint32_t)kb * 2, 0);
                rw[p] = make_uint4(v[0], v[1], v[2], v[3]);
            }
        }
    };
    auto store_tile = [&](int buf) __attribute__((always_inline)) {
        unsigned char* A = smem + buf * (A_BYTES + W_BYTES);
        unsigned char* W = A + A_BYTES;
#pragma unroll
        for (int p = 0; p < A_CH; ++p) {
            const int rr = r_in + 32 * p;
            *(uint4*)(A + rr * 128 + ((ch ^ (rr & 7)) << 4)) = ra[p];
        }
#pragma unroll
        for (int p = 0; p < W_CH; ++p) {
            const int rr = r_in + 32 * p;
            if (rr < BN) *(uint4*)(W + rr * 128 + ((ch ^ (rr & 7)) << 4)) = rw[p];
        }
    };

    f32x4 acc[NF][MF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};

    const int wm = wave / WN, wn = wave - wm * WN;
    const int wrow_m = wm * (BM / WM), wrow_n = wn * (BN / WN);
    const int fr = lane & 15, fq = lane >> 4;

    const int nk_all = PHASE ? phase_ksteps(g, ph) : (g.K + BK - 1) / BK;
    const int kt0 = (int)((long long)nk_all * slice / S), nk = (int)((long long)nk_all * (slice + 1) / S);
    // ONE LDS buffer: the next step's operands wait in registers while this step's MFMAs read the tile, and go to LDS between
    // two barriers.  The launches are latency-bound (a gather per step, ~0.2 us of MFMAs), so what counts is how many workgroups
    // a CU holds, and half the LDS (32 KB at 128 x 128) lets the register budget decide: 3 per CU instead of 2.
    load_tile(kt0);
    store_tile(0);
    __syncthreads();
    for (int kt = kt0; kt < nk; ++kt) {
        constexpr int cur = 0;
        if (kt + 1 < nk) load_tile(kt + 1);
        const unsigned char* A = smem + cur * (A_BYTES + W_BYTES);
        const unsigned char* W = A + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[MF], fw[NF];
            const int kc = ks * 4 + fq;
#pragma unroll
            for (int j = 0; j < MF; ++j) {
                const int rr = wrow_m + j * 16 + fr;
                fa[j] = *(const bf16x8*)(A + rr * 128 + ((kc ^ (rr & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int rr = wrow_n + i * 16 + fr;
                fw[i] = *(const bf16x8*)(W + rr * 128 + ((kc ^ (rr & 7)) << 4));
            }
#pragma unroll
            for (int i = 0; i < NF; ++i)
#pragma unroll
                for (int j = 0; j < MF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fa[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();                                       // every wave has read the tile
        if (kt + 1 < nk) store_tile(0);
        __syncthreads();
    }

    if (S > 1) {                               // raw partial sums; bias / activation happen in splitk_reduce_kernel
        float* P = g.partial + (long long)slice * g.M * g.N;
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            const int m = m0 + wrow_m + j * 16 + fr;
            if (m >= M) continue;
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int n = n0 + wrow_n + i * 16 + fq * 4;
                if (n < g.N) *(float4*)(P + (long long)m * g.N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            }
        }
        return;
    }
    finish_tile<MF, NF, STATS, WM, BN, PHASE, BNBWD>(g, acc, M, m0, n0, wrow_m, wrow_n, lane, wave, smem, tm, ph);
}

// second stage of a split-K conv: sum the K slices, then the usual epilogue (bias, SiLU, bf16 shortcut, store)
__global__ __launch_bounds__(256) void splitk_reduce_kernel(GemmArgs g) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    const int n4 = g.N >> 2;
    if (i >= (long long)g.M * n4) return;
    const int m = (int)(i / n4), n = (int)(i - (long long)m * n4) * 4;
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    // four slices per trip, loads first: a pure read pass lives on the loads in flight; summation order unchanged
    const float* base = g.partial + (long long)m * g.N + n;
    const long long slice = (long long)g.M * g.N;
    int s = 0;
    for (; s + 3 < g.splitk; s += 4) {
        const float4 p0 = *(const float4*)(base + (s + 0) * slice), p1 = *(const float4*)(base + (s + 1) * slice);
        const float4 p2 = *(const float4*)(base + (s + 2) * slice), p3 = *(const float4*)(base + (s + 3) * slice);
        v.x += p0.x; v.y += p0.y; v.z += p0.z; v.w += p0.w;
        v.x += p1.x; v.y += p1.y; v.z += p1.z; v.w += p1.w;
        v.x += p2.x; v.y += p2.y; v.z += p2.z; v.w += p2.w;
        v.x += p3.x; v.y += p3.y; v.z += p3.z; v.w += p3.w;
    }
    for (; s < g.splitk; ++s) {
        const float4 p = *(const float4*)(base + s * slice);
        v.x += p.x; v.y += p.y; v.z += p.z; v.w += p.w;
    }
    const int flags = g.flags;
    if (flags & YV_EPI_BIAS) {
        const float4 b = *(const float4*)(g.bias + n);
        v.x += b.x; v.y += b.y; v.z += b.z; v.w += b.w;
    }
    if (flags & YV_EPI_SILU) { v.x = silu_f(v.x); v.y = silu_f(v.y); v.z = silu_f(v.z); v.w = silu_f(v.w); }
    if (flags & YV_EPI_RES_BF16) {
        const uint2 rr = *(const uint2*)(g.res + (long long)m * g.ldres + n);
        v.x += bf16_to_f32((uint16_t)(rr.x & 0xffff)); v.y += bf16_to_f32((uint16_t)(rr.x >> 16));
        v.z += bf16_to_f32((uint16_t)(rr.y & 0xffff)); v.w += bf16_to_f32((uint16_t)(rr.y >> 16));
    }
    if (flags & YV_EPI_OUT_F32) *(float4*)((float*)g.out + (long long)m * g.ldo + n) = v;
    else *(uint2*)((uint16_t*)g.out + (long long)m * g.ldo + n) = make_uint2(pack_bf16x2(v.x, v.y), pack_bf16x2(v.z, v.w));
}

// the tail of every launcher that may split K: the reduce pass over g.partial when g.splitk > 1, then the status
int launch_splitk_reduce(const GemmArgs& g, hipStream_t st) {
    if (g.splitk > 1) {
        const long long items = (long long)g.M * (g.N >> 2);
        hipLaunchKernelGGL(splitk_reduce_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, st, g);
    }
    return yv_launch_status();
}


// ---------------------------------------------------------------------------------------------
// Linear fast path (K % 64 == 0): both tiles go global -> LDS by LDS-DMA (global_load_lds, 16 B per
// lane, no staging VGPRs, no ds_write pass).  One wave-instruction fills 8 rows x 128 B of the
// lane-linear LDS image, so the chunk swizzle is applied to the SOURCE address (chunk' ^ (row & 7))
// and again on the fragment read - the same involution on both sides.  Two LDS buffers; the DMA of
// K step t+1 is issued before the MFMAs of step t and drained (vmcnt(0)) at the step's only barrier.
// Rows past the end of a matrix are clamped to its last row: their results are never stored.
// ---------------------------------------------------------------------------------------------
typedef const __attribute__((address_space(1))) void* gptr_t;
typedef __attribute__((address_space(3))) void* lptr_t;
typedef __attribute__((ext_vector_type(4))) short s16x4;
typedef __attribute__((address_space(3))) s16x4* lds_s16x4_t;

// reduction-major tiles ([64 reduction rows][128 columns] bf16, 256-byte LDS rows): chunk swizzle and the
// hardware-transposing fragment read (8 consecutive reduction elements 32*ks + 8*(lane>>4) + 0..7 of column
// col0 + (lane&15)): two ds_read_b64_tr_b16, lane 4q+p of a 16-lane group addressing row q, columns 4p..4p+3
// COLS = 64 / 32 (the dY tile of gemm_tn_narrow_kernel: 128- / 64-byte rows, dense): the same read from a swizzle derived for
// that pitch.  A 32-lane half reads rows r + {0..3, 8..11}, 32 bytes (8 banks) of each; bank = (addr / 4) % 64, so the eight rows
// must land in eight different 32-byte groups of a 256-byte span.  group = (addr / 32) % 8:
//   128: ch >> 1 - the pitch contributes nothing, row bits 0, 1 and 3 are XORed into chunk bits 1, 2 and 3;
//    64: (row & 1) << 2 | ch >> 1 - row bit 0 comes from the pitch, row bits 1 and 3 are XORed into chunk bits 1 and 2;
//    32: (row & 3) << 1 | ch >> 1 - row bits 0 and 1 come from the pitch, row bit 3 is XORed into chunk bit 1.
// Chunk bit 0 is never touched: the two chunks (32 bytes) a 16-lane group reads of a row stay adjacent.
template <int COLS = 128>
__device__ __forceinline__ int tn_swz(int row) {
    if constexpr (COLS == 128) return ((row & 3) << 1) | (((row >> 3) & 1) << 3);
    else if constexpr (COLS == 64) return (((row >> 1) & 1) << 1) | (((row >> 3) & 1) << 2);
    else return ((row >> 3) & 1) << 1;
}
template <int COLS = 128>
__device__ __forceinline__ bf16x8 tr_frag(const unsigned char* tile, int ks, int lane, int col0) {
    static_assert(COLS == 128 || COLS == 64 || COLS == 32, "row pitch of a reduction-major tile");
    constexpr int P = COLS * 2;
    const int fi = lane & 15, mg = lane >> 4, q = fi >> 2, p = fi & 3;
    const int row = ks * 32 + mg * 8 + q;
    const int ch = (col0 + 4 * p) >> 3, off = ((col0 + 4 * p) & 7) * 2;
    const s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(tile + row * P + ((ch ^ tn_swz<COLS>(row)) << 4) + off));
    const s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t)(tile + (row + 4) * P + ((ch ^ tn_swz<COLS>(row + 4)) << 4) + off));
    const u32x4 pk = {__builtin_bit_cast(u32x2, lo)[0], __builtin_bit_cast(u32x2, lo)[1],
                      __builtin_bit_cast(u32x2, hi)[0], __builtin_bit_cast(u32x2, hi)[1]};
    return __builtin_bit_cast(bf16x8, pk);
}

template <int BM, int BN, int WM, int WN, int ABL = 0, bool WT = false>
__global__ __launch_bounds__(WM * WN * 64) void gemm_dma_kernel(GemmArgs g) {
    // ABL (diagnostic builds only): 1 no in-loop DMA, 2 no MFMA, 3 no fragment reads, 4 no epilogue
    // WT: the weight operand is stored REDUCTION-major, W (K, N) with row stride g.ldw (dgrad: dX = dY . W reads the
    //     master-layout weight directly): its tile is [64 k][BN n] and its fragments are hardware-transposed reads
    constexpr int NW = WM * WN;                                // waves per workgroup
    constexpr int MF = BM / WM / 16, NF = BN / WN / 16;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128;
    constexpr int A_INS = BM / (8 * NW), W_INS = BN / (8 * NW);   // wave-instructions per wave per K step
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;

    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    // split-K (wgrad-shaped problems: few output tiles, long K): slices of one tile are neighbouring workgroups
    const int S = g.splitk > 1 ? g.splitk : 1;
    const int slice = bid % S;
    bid /= S;
    // grouped order inside the XCD's chunk: GM consecutive M tiles share each W tile while it is hot in L2
    int tm, tn;
    {
        const int GM = g.group_m, per = GM * g.tiles_n;
        const int grp = bid / per, first = grp * GM;
        const int gsz = (g.tiles_m - first) < GM ? (g.tiles_m - first) : GM;
        const int in = bid - grp * per;
        tm = first + in % gsz;
        tn = in / gsz;
    }
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    // per-lane source rows (swizzled chunk) for every DMA instruction of this wave
    const int lrow = lane >> 3, lch = lane & 7;
    const uint16_t* a_src[A_INS];
    const uint16_t* w_src[W_INS];
#pragma unroll
    for (int j = 0; j < A_INS; ++j) {
        const int r = (j * NW + wave) * 8 + lrow;
        int m = m0 + r;
        m = m < g.M ? m : g.M - 1;
        a_src[j] = g.a0 + (long long)m * g.lda0 + ((lch ^ (r & 7)) << 3);
    }
#pragma unroll
    for (int j = 0; j < W_INS; ++j) {
        if constexpr (!WT) {
            const int r = (j * NW + wave) * 8 + lrow;
            int n = n0 + r;
            n = n < g.N ? n : g.N - 1;
            w_src[j] = g.w + (long long)n * g.K + ((lch ^ (r & 7)) << 3);
        } else {                                           // 4 reduction rows x 256 B per wave-instruction
            static_assert(!WT || BN == 128, "reduction-major weight tiles are 128 columns wide");
            const int r = (j * NW + wave) * 4 + (lane >> 4);
            int cn = n0 + (((lane & 15) ^ tn_swz(r)) << 3);
            cn = cn < g.N ? cn : g.N - 8;
            w_src[j] = g.w + (long long)r * g.ldw + cn;
        }
    }
    auto issue = [&](int kt, int buf) {
        unsigned char* A = smem + buf * (A_BYTES + W_BYTES);
        unsigned char* W = A + A_BYTES;
#pragma unroll
        for (int j = 0; j < A_INS; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(a_src[j] + kt * BK), (lptr_t)(A + (j * NW + wave) * 1024), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < W_INS; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(w_src[j] + (WT ? (long long)kt * BK * g.ldw : (long long)kt * BK)),
                                             (lptr_t)(W + (j * NW + wave) * 1024), 16, 0, 0);
    };

    f32x4 acc[NF][MF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wm = wave / WN, wn = wave - wm * WN;
    const int wrow_m = wm * (BM / WM), wrow_n = wn * (BN / WN);
    const int fr = lane & 15, fq = lane >> 4;

    const int nk_all = g.K / BK;
    const int kt0 = (int)((long long)nk_all * slice / S), nk = (int)((long long)nk_all * (slice + 1) / S);
    issue(kt0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = kt0; kt < nk; ++kt) {
        const int cur = (kt - kt0) & 1;
        if (ABL != 1 && kt + 1 < nk) issue(kt + 1, cur ^ 1);
        const unsigned char* A = smem + cur * (A_BYTES + W_BYTES);
        const unsigned char* W = A + A_BYTES;
#pragma unroll
        for (int ks = 0; ks < 2; ++ks) {
            bf16x8 fa[MF], fw[NF];
            const int kc = ks * 4 + fq;
#pragma unroll
            for (int j = 0; j < MF; ++j) {
                const int rr = wrow_m + j * 16 + fr;
                if (ABL != 3) fa[j] = *(const bf16x8*)(A + rr * 128 + ((kc ^ (rr & 7)) << 4));
                else { u32x4 z = {(uint32_t)rr, 1u, 2u, 3u}; fa[j] = __builtin_bit_cast(bf16x8, z); }
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int rr = wrow_n + i * 16 + fr;
                if (ABL != 3) {
                    if constexpr (!WT) fw[i] = *(const bf16x8*)(W + rr * 128 + ((kc ^ (rr & 7)) << 4));
                    else fw[i] = tr_frag(W, ks, lane, wrow_n + i * 16);
                }
                else { u32x4 z = {(uint32_t)rr, 5u, 6u, 7u}; fw[i] = __builtin_bit_cast(bf16x8, z); }
            }
#pragma unroll
            for (int i = 0; i < NF; ++i)
#pragma unroll
                for (int j = 0; j < MF; ++j)
                    if (ABL != 2) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fa[j], acc[i][j], 0, 0, 0);
                    else { asm volatile("" :: "v"(fw[i]), "v"(fa[j])); }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (S > 1) {                               // raw partial sums; the epilogue runs in splitk_reduce_kernel
        float* P = g.partial + (long long)slice * g.M * g.N;
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            const int m = m0 + wrow_m + j * 16 + fr;
            if (m >= M) continue;
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int n = n0 + wrow_n + i * 16 + fq * 4;
                if (n < g.N) *(float4*)(P + (long long)m * g.N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            }
        }
        return;
    }
    if (ABL != 4) finish_tile<MF, NF>(g, acc, M, m0, n0, wrow_m, wrow_n, lane, wave, smem);
    else if (acc[0][0][0] == 12345.678f) finish_tile<MF, NF>(g, acc, M, m0, n0, wrow_m, wrow_n, lane, wave, smem);
}


// ---------------------------------------------------------------------------------------------
// Convolution on the LDS-DMA GEMM structure (round 3): the implicit-GEMM gather of igemm_kernel expressed as the per-lane offset of
// a `buffer_load ... lds`.  For layers whose input channels are a multiple of 64 a K step lies inside ONE 3 x 3 tap and ONE source,
// so everything that changes along K - the tap's pixel displacement, the channel base, the source of a two-source 1 x 1 - is
// wave-uniform and travels in the instruction's scalar offset; what a lane contributes is fixed for the whole tile: the byte
// offset of its output pixel's centre (+ its swizzled 16-byte chunk) and nine tap-validity bits (padding -> an out-of-range
// offset -> zeros through the descriptor's range check).  No staging registers, no address arithmetic in the loop, no LDS stores:
// the K step is the linear kernel's (two LDS stages, DMA of step k+1 under the MFMAs of step k).  igemm_kernel was bound by the
// VALU issue of exactly that gather and staging.  Epilogues: finish_tile (bias, SiLU, bf16 shortcut, f32 output).
// Eligibility (host): (c0 + c1) % 64 == 0, c1 == 0 or (1 x 1 and c0 % 64 == 0), Cout >= 64, staged epilogue usable.
// ---------------------------------------------------------------------------------------------
// ---- device text shared by the LDS-DMA convolution kernels ----
// Geometry of output pixel m (cgemm_dma_kernel, cgemm_dma32_kernel, cgemm_small_kernel, cgemm_mx_kernel): the index of the pixel at
// its centre in each source (the upsampled-source shifts applied; p1 = 0 without a second source) and the nine tap-validity bits
// (none for a row past M: every read of it is out of range, i.e. zeros).
template <bool PHASE>
__device__ __forceinline__ void conv_pixel_geom(const GemmArgs& g, int M, int hw, int m, long long& p0, long long& p1, uint32_t& tap_bits) {
    const int mc = m < M ? m : M - 1;
    const int b = mc / hw, rem = mc - b * hw;
    const int oy = rem / g.Wout;
    const int cy = oy * g.stride, cx = (rem - oy * g.Wout) * g.stride;
    p0 = ((long long)b * (g.Hin >> g.up0) + (cy >> g.up0)) * (g.Win >> g.up0) + (cx >> g.up0);
    p1 = g.c1 ? ((long long)b * (g.Hin >> g.up1) + (cy >> g.up1)) * (g.Win >> g.up1) + (cx >> g.up1) : 0;
    uint32_t taps = 0;
    if (m < M) {
        if constexpr (PHASE) {
            taps = phase_taps(g, cy, cx);
        } else if (g.ksize == 3) {
#pragma unroll
            for (int t = 0; t < 9; ++t) {
                const int iy = cy + t / 3 - 1, ix = cx + t % 3 - 1;
                taps |= (iy >= 0 && iy < g.Hin && ix >= 0 && ix < g.Win) ? (1u << t) : 0u;
            }
        } else {
            taps = 1u;
        }
    }
    tap_bits = taps;
}
// What lane (lrow, lch) of the wave-instruction that fills tile row r contributes for the whole tile (bf16 kernels): the geometry
// of output pixel m as the byte offset of its centre in each source + the lane's swizzled 16-byte chunk ...
template <bool PHASE>
__device__ __forceinline__ void cdma_lane_pixel(const GemmArgs& g, int M, int hw, int m, int r, int lch, uint32_t& off0, uint32_t& off1,
                                                uint32_t& tap_bits) {
    long long p0, p1;
    conv_pixel_geom<PHASE>(g, M, hw, m, p0, p1, tap_bits);
    const uint32_t sw = (uint32_t)((lch ^ (r & 7)) << 4);
    off0 = (uint32_t)(p0 * g.lda0 * 2) + sw;
    off1 = g.c1 ? (uint32_t)(p1 * g.lda1 * 2) + sw : 0u;
}
// ... and for weight row r of the column tile at n0 (rows past N: the last row, never stored)
__device__ __forceinline__ uint32_t cdma_lane_weight(const GemmArgs& g, int n0, int r, int lch) {
    int n = n0 + r;
    n = n < g.N ? n : g.N - 1;
    return (uint32_t)(((long long)n * g.K + ((lch ^ (r & 7)) << 3)) * 2);
}
// the scalar offset is unsigned: source 0's descriptor starts one row + one pixel before the tensor (3 x 3 only)
template <bool PHASE>
__device__ __forceinline__ uint32_t cdma_bias0(const GemmArgs& g) {
    return !PHASE && g.ksize == 3 ? (uint32_t)((g.Win + 1) * g.lda0 * 2) : 0u;
}
// The wave-uniform part of the K step at element kb (not the phase form): the tap whose validity bit gates the lanes and the scalar
// offset of the step in source 0's descriptor - the tap's pixel displacement + the channel base.  (The second source of a
// two-source 1 x 1, kb >= g.c0, has tap 0 and the offset (kb - g.c0) * 2 in its own descriptor.)
// Cin = g.c0 + g.c1 and pad = g.ksize >> 1 are the caller's, computed once per tile.
__device__ __forceinline__ uint32_t cdma_step0(const GemmArgs& g, int kb, uint32_t bias0, int Cin, int pad, int& tap) {
    tap = 0;
    uint32_t so = bias0 + (uint32_t)(kb * 2);
    if (g.ksize == 3) {
        tap = g.cin_shift >= 0 ? (kb >> g.cin_shift) : kb / Cin;
        const int cin = kb - tap * Cin;
        const int ky = tap >= 6 ? 2 : (tap >= 3 ? 1 : 0), kx = tap - ky * 3;
        so = bias0 + (uint32_t)((((ky - pad) * g.Win + (kx - pad)) * g.lda0 + cin) * 2);
    }
    return so;
}
// What a lane holds for the life of a tile, stated ONCE for cdma_tile and csmall_tile, whose stage is filled by NWG waves, wave w
// of them writing 8 rows x 128 B per wave-instruction (instruction j: rows (j * NWG + w) * 8 .., lane -> row lane >> 3, chunk
// lane & 7): for each of its AI activation and WI weight instructions of a K step the offsets of cdma_lane_pixel /
// cdma_lane_weight and the tap bits, and what is uniform: bias0, Cin and pad (cdma_step0's).
template <int AI, int WI, int NWG>
struct CdmaLanes {
    uint32_t a_off0[AI], a_off1[AI], a_taps[AI], w_off[WI], bias0;
    int Cin, pad;
};
// the buffer descriptor of a DMA source at p: raw, byte offsets, range to 2 GB (a lane's DMA_OOB lies past it).  The bodies build
// theirs once per tile: built at the loads, a grouped launch re-read the fields from the kernel arguments in every K step.
__device__ __forceinline__ auto cdma_rsrc(const void* p) { return __builtin_amdgcn_make_buffer_rsrc((void*)p, 0, 0x7fffffff, 0x00020000); }
template <bool PHASE, int AI, int WI, int NWG>
__device__ __forceinline__ CdmaLanes<AI, WI, NWG> cdma_lanes(const GemmArgs& g, int M, int m0, int n0, int w, int lane) {
    CdmaLanes<AI, WI, NWG> L;
    const int hw = g.Hout * g.Wout, lrow = lane >> 3, lch = lane & 7;
#pragma unroll
    for (int j = 0; j < AI; ++j) {
        const int r = (j * NWG + w) * 8 + lrow;
        cdma_lane_pixel<PHASE>(g, M, hw, m0 + r, r, lch, L.a_off0[j], L.a_off1[j], L.a_taps[j]);
    }
#pragma unroll
    for (int j = 0; j < WI; ++j) L.w_off[j] = cdma_lane_weight(g, n0, (j * NWG + w) * 8 + lrow, lch);
    L.bias0 = cdma_bias0<PHASE>(g);
    L.Cin = g.c0 + g.c1;
    L.pad = g.ksize >> 1;
    return L;
}
// The activations of the K step at element kb (uniform; not the phase form), instruction j to LDS address dst(j): the second
// source of a two-source 1 x 1, or source 0 at cdma_step0's offset under the tap's validity bit
template <int AI, int WI, int NWG, class R, class Dst>
__device__ __forceinline__ void cdma_gather(const GemmArgs& g, const CdmaLanes<AI, WI, NWG>& L, const R rs0, const R rs1, int kb,
                                            const Dst& dst) {
    if (g.c1 && kb >= g.c0) {
        const int so = (kb - g.c0) * 2;
#pragma unroll
        for (int j = 0; j < AI; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (lptr_t)dst(j), 16, (int)((L.a_taps[j] & 1u) ? L.a_off1[j] : DMA_OOB), so, 0, 0);
    } else {
        int tap;
        const uint32_t so = cdma_step0(g, kb, L.bias0, L.Cin, L.pad, tap);
#pragma unroll
        for (int j = 0; j < AI; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lptr_t)dst(j), 16, (int)(((L.a_taps[j] >> tap) & 1u) ? L.a_off0[j] : DMA_OOB), (int)so, 0, 0);
    }
}
// The K loop of cdma_tile (cgemm_dma32_kernel keeps its own copy): a ring of ST stages, ST - 1 K steps in flight, INS wave-instructions per step.
// The launches are latency-bound (9 .. 36 K steps per tile, one L2 / HBM round trip each when only the next step is in flight), and
// inside the pipeline the detector runs on the few CUs the classifier leaves free, where a tile's latency is all that counts.
// Step kt: counted wait (the ST - 2 younger steps stay in flight), ONE raw barrier (step kt visible to every wave; every wave is
// done with step kt-1, whose stage the next issue refills), issue(step, stage), step(stage): the MFMAs.  Closing barrier: the
// staged epilogue reuses the tile buffers.
template <int ST, int INS, class Issue, class Step>
__device__ __forceinline__ void cdma_ring(int nk, const Issue& issue, const Step& step) {
    static_assert(ST >= 2 && ST <= 4, "the counted waits below");
    int issued = 0;
#pragma unroll
    for (int p = 0; p < ST - 1; ++p)
        if (p < nk) { issue(p, p); ++issued; }
    int slot = 0, islot = (ST - 1) % ST;
    for (int kt = 0; kt < nk; ++kt) {
        // steps issued so far: `issued` (all of them once the prologue / earlier iterations ran out of steps)
        if (issued - kt - 1 >= ST - 2 && ST > 2) {
            if constexpr (ST == 3) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(INS) : "memory");
            else asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * INS) : "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (issued < nk) { issue(issued, islot); ++issued; islot = islot + 1 == ST ? 0 : islot + 1; }
        const int cur = slot;
        slot = slot + 1 == ST ? 0 : slot + 1;
        step(cur);
    }
    asm volatile("s_barrier" ::: "memory");
}
// A wave's share of a BM x BN tile cut into WM x WN wave tiles of MF x NF fragments: the first row and column of wave tile
// `wave`, the lane's fragment row and quad, and the accumulators at zero.
struct WaveTile { int wrow_m, wrow_n, fr, fq; };
template <int BM, int BN, int WM, int WN, int MF, int NF>
__device__ __forceinline__ WaveTile wave_tile(int wave, int lane, f32x4 (&acc)[NF][MF]) {
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wm = wave / WN, wn = wave - wm * WN;
    return {wm * (BM / WM), wn * (BN / WN), lane & 15, lane >> 4};
}
// one 64-deep K step of a wave tile of MF x NF fragments at rows wrow_m of A and wrow_n of W (128-byte rows, chunks swizzled)
template <int MF, int NF>
__device__ __forceinline__ void cdma_mfma_step(const unsigned char* A, const unsigned char* W, int wrow_m, int wrow_n, int fr, int fq,
                                               f32x4 (&acc)[NF][MF]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 fa[MF], fw[NF];
        const int kc = ks * 4 + fq;
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            const int rr = wrow_m + j * 16 + fr;
            fa[j] = *(const bf16x8*)(A + rr * 128 + ((kc ^ (rr & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int rr = wrow_n + i * 16 + fr;
            fw[i] = *(const bf16x8*)(W + rr * 128 + ((kc ^ (rr & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < MF; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fa[j], acc[i][j], 0, 0, 0);
    }
}

// One tile of cgemm_dma_kernel: ONE text for the kernel below and for cgemm_dma_group_kernel.  bid: the workgroup's index among the
// nwg workgroups that walk g's tiles (the launch's grid, a phase's share of it, or a group member's share), ph: the phase (PHASE).
// The LDS base is the launch's dynamic LDS, named here as the kernels named it: handed in as a pointer argument it changed the
// register allocation of the BNBWD instances (136 -> 134 VGPRs), declared here every existing instance compiles to the parent's
// report (profiles/conv_group_resources.txt).
template <int BN, int WM, int WN, int ST, bool STATS, bool PHASE, bool BNBWD>
__device__ __forceinline__ void cdma_tile(const GemmArgs& g, int bid, const int nwg, const int ph = 0) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    static_assert(!(PHASE && STATS), "the phase form is a plain convolution");
    static_assert(!(BNBWD && (PHASE || STATS)), "one kind of column sums, none of a phase launch");
    constexpr int BM = 128, NW = 4;
    static_assert(WM * WN == NW, "four waves");
    constexpr int MF = BM / WM / 16, NF = BN / WN / 16;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128;
    constexpr int A_INS = BM / (8 * NW), W_INS = BN / (8 * NW);
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = g.M;
    bid = xcd_remap(bid, nwg);
    const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    const CdmaLanes<A_INS, W_INS, NW> L = cdma_lanes<PHASE, A_INS, W_INS, NW>(g, M, m0, n0, wave, lane);
    const auto rs0 = cdma_rsrc((const unsigned char*)g.a0 - L.bias0), rs1 = cdma_rsrc(g.c1 ? g.a1 : g.a0), rsW = cdma_rsrc(g.w);
    const auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        unsigned char* A = smem + buf * (A_BYTES + W_BYTES);
        const int kb = kt * BK;                                  // (uniform)
        uint32_t wcol = (uint32_t)(kb * 2);
        if constexpr (PHASE) {
            const PhaseStep ps = phase_step(g, ph, kb);
            wcol = ps.wcol;
#pragma unroll
            for (int j = 0; j < A_INS; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lptr_t)(A + (j * NW + wave) * 1024), 16,
                                                         (int)(((L.a_taps[j] >> ps.slot) & 1u) ? L.a_off0[j] : DMA_OOB), (int)ps.src, 0, 0);
        } else {
            cdma_gather(g, L, rs0, rs1, kb, [&](int j) __attribute__((always_inline)) { return A + (j * NW + wave) * 1024; });
        }
#pragma unroll
        for (int j = 0; j < W_INS; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lptr_t)(A + A_BYTES + (j * NW + wave) * 1024), 16, (int)L.w_off[j], (int)wcol, 0, 0);
    };

    f32x4 acc[NF][MF];
    const WaveTile wt = wave_tile<BM, BN, WM, WN>(wave, lane, acc);
    const auto step = [&](int buf) __attribute__((always_inline)) {
        const unsigned char* A = smem + buf * (A_BYTES + W_BYTES);
        cdma_mfma_step<MF, NF>(A, A + A_BYTES, wt.wrow_m, wt.wrow_n, wt.fr, wt.fq, acc);
    };
    cdma_ring<ST, A_INS + W_INS>(PHASE ? phase_ksteps(g, ph) : g.K / BK, issue, step);
    finish_tile<MF, NF, STATS, WM, BN, PHASE, BNBWD>(g, acc, M, m0, n0, wt.wrow_m, wt.wrow_n, lane, wave, smem, tm, ph);
}

template <int BN, int WM, int WN, int ST = 2 /* LDS stages: ST - 1 K steps of DMA in flight */, bool STATS = false /* as igemm_kernel */,
          bool PHASE = false /* as igemm_kernel */, bool BNBWD = false /* as igemm_kernel */>
__global__ __launch_bounds__(256) void cgemm_dma_kernel(GemmArgs g) {
    int bid = blockIdx.x;
    int nwg = gridDim.x, ph = 0;
    if constexpr (PHASE) { ph = phase_of_block(g, bid); nwg = g.tiles_m * g.tiles_n; }
    cdma_tile<BN, WM, WN, ST, STATS, PHASE, BNBWD>(g, bid, nwg, ph);
}

// ---------------------------------------------------------------------------------------------
// LDS-DMA convolution for 32-aligned input channels ("conv_dma32", off by default): cgemm_dma_kernel's
// organisation for the layers its eligibility leaves on igemm_kernel - Cin % 32 == 0 but not % 64 (YOLOv8m's 96 and 288) - as a
// plain inference convolution (no STATS, PHASE or BNBWD form).  A 64-deep K step is two 32-channel BLOCKS, each its own LDS panel
// of 64-byte rows ([rows][32 bf16]; a stage: two A panels, then two W panels).  A block never straddles a tap or a source
// (Cin % 32 == 0; c0 % 32 == 0 for a two-source 1 x 1), so what changes along K stays in the DMA's scalar offset, per block
// (cdma_step0 at the block's element); a wave-instruction fills 16 rows x 64 B = 1,024 contiguous bytes of one panel
// (lane -> row lane >> 2, chunk lane & 3), and what a lane contributes is fixed for the tile, by cdma_lane_pixel / cdma_lane_weight.
// Swizzle: chunk c of row r lies at slot c ^ cdma32_swz(r).  ds_read_b128 serves four 16-lane groups, {0-3, 12-15, 20-27},
// {4-11, 16-19, 28-31} and the same + 32; a fragment read has lane = fq * 16 + fr at row fr, chunk fq, i.e. 16-byte slot
// (fr & 3) * 4 + (fq ^ swz) of the 256-byte bank row.  With swz = (r >> 2) & 3 lanes 0-3 and 20-23 (and 12-15 and 24-27) of a group
// meet on the same four slots: 2-way.  With swz = -(r >> 2) & 3 = {0, 3, 2, 1} the four quads of every group take
// {0, 1, 2, 3} ^ const: conflict-free.
// K ascends, one mfma_f32_16x16x32_bf16 per block and fragment into the same accumulators: a tile's accumulation order is
// cgemm_dma_kernel's.  Odd block count (K = 9 * 96: 13.5 steps; Cin = 32 at 1 x 1: half a step): the last step's missing block is
// ISSUED, activations and weights, at the out-of-range offset, so the descriptor's range check leaves zeros in both panels and
// the counted vmcnt is the same in every step (in range the weight read would reach the next output channel's row).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ int cdma32_swz(int r) { return (0 - (r >> 2)) & 3; }
// the chunk argument with which cdma_lane_pixel / cdma_lane_weight, whose swizzle is arg ^ (r & 7), read source chunk
// lch ^ cdma32_swz(r) for the lane that fills slot lch of row r
__device__ __forceinline__ int cdma32_lane_chunk(int r, int lch) { return lch ^ cdma32_swz(r) ^ (r & 7); }
// one 64-deep K step (two blocks) of a wave tile of MF x NF fragments: panels of AP / WP bytes, 64-byte rows
template <int MF, int NF, int AP, int WP>
__device__ __forceinline__ void cdma32_mfma_step(const unsigned char* A, const unsigned char* W, int wrow_m, int wrow_n, int fr, int fq,
                                                 f32x4 (&acc)[NF][MF]) {
#pragma unroll
    for (int ks = 0; ks < 2; ++ks) {
        bf16x8 fa[MF], fw[NF];
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            const int rr = wrow_m + j * 16 + fr;
            fa[j] = *(const bf16x8*)(A + ks * AP + rr * 64 + ((fq ^ cdma32_swz(rr)) << 4));
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int rr = wrow_n + i * 16 + fr;
            fw[i] = *(const bf16x8*)(W + ks * WP + rr * 64 + ((fq ^ cdma32_swz(rr)) << 4));
        }
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < MF; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fa[j], acc[i][j], 0, 0, 0);
    }
}

template <int BN, int WM, int WN, int ST>
__global__ __launch_bounds__(256) void cgemm_dma32_kernel(GemmArgs g) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BM = 128, NW = 4;
    static_assert(WM * WN == NW, "four waves");
    constexpr int MF = BM / WM / 16, NF = BN / WN / 16;
    constexpr int AP = BM * 64, WP = BN * 64, STAGE = 2 * (AP + WP);     // bytes: a panel of A, of W; one K step
    constexpr int A_RG = BM / (16 * NW);                                  // 16-row groups of an A panel per wave (both panels)
    constexpr int W_RG = BN / 16, W_INS = 2 * W_RG / NW;                  // 16-row groups of a W panel; W instructions per wave
    static_assert(2 * W_RG % NW == 0 && NF == 4, "every wave issues the same count; 64-column wave tiles (the staged epilogue)");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = g.M;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    const int lrow = lane >> 2, lch = lane & 3;
    uint32_t a_off0[A_RG], a_off1[A_RG], a_taps[A_RG], w_off[W_INS];
    const int hw = g.Hout * g.Wout;
#pragma unroll
    for (int q = 0; q < A_RG; ++q) {
        const int r = (q * NW + wave) * 16 + lrow;
        cdma_lane_pixel<false>(g, M, hw, m0 + r, r, cdma32_lane_chunk(r, lch), a_off0[q], a_off1[q], a_taps[q]);
    }
    // W instruction j of this wave: index j * NW + wave among the 2 * W_RG of a step, panel-major
#pragma unroll
    for (int j = 0; j < W_INS; ++j) {
        const int r = ((j * NW + wave) % W_RG) * 16 + lrow;
        w_off[j] = cdma_lane_weight(g, n0, r, cdma32_lane_chunk(r, lch));
    }
    const uint32_t bias0 = cdma_bias0<false>(g);
    const auto rs0 = cdma_rsrc((const unsigned char*)g.a0 - bias0), rs1 = cdma_rsrc(g.c1 ? g.a1 : g.a0), rsW = cdma_rsrc(g.w);
    const int Cin = g.c0 + g.c1;
    const int pad = g.ksize >> 1;
    auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        unsigned char* A = smem + buf * STAGE;
        unsigned char* W = A + 2 * AP;
#pragma unroll
        for (int p = 0; p < 2; ++p) {
            const int kb = kt * BK + p * 32;                         // (uniform) the block's first element
            const bool live = kb < g.K;                              // false: the missing block of an odd count - zeros
            if (g.c1 && kb >= g.c0) {                                // second source of a two-source 1 x 1
                const int so = (kb - g.c0) * 2;
#pragma unroll
                for (int q = 0; q < A_RG; ++q)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (lptr_t)(A + p * AP + (q * NW + wave) * 1024), 16,
                                                             (int)((live && (a_taps[q] & 1u)) ? a_off1[q] : DMA_OOB), so, 0, 0);
            } else {
                int tap;
                const uint32_t so = cdma_step0(g, kb, bias0, Cin, pad, tap);
#pragma unroll
                for (int q = 0; q < A_RG; ++q)
                    __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lptr_t)(A + p * AP + (q * NW + wave) * 1024), 16,
                                                             (int)((live && ((a_taps[q] >> tap) & 1u)) ? a_off0[q] : DMA_OOB), (int)so, 0, 0);
            }
        }
#pragma unroll
        for (int j = 0; j < W_INS; ++j) {
            const int idx = j * NW + wave, p = idx / W_RG, rg = idx - p * W_RG;
            const int kb = kt * BK + p * 32;
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lptr_t)(W + p * WP + rg * 1024), 16, (int)(kb < g.K ? w_off[j] : DMA_OOB), kb * 2, 0,
                                                     0);
        }
    };

    f32x4 acc[NF][MF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wm = wave / WN, wn = wave - wm * WN;
    const int wrow_m = wm * (BM / WM), wrow_n = wn * (BN / WN);
    const int fr = lane & 15, fq = lane >> 4;
    const int nk = (g.K / 32 + 1) / 2;
    // cdma_ring's loop, and above cdma_lanes' set-up and cdma_gather's issue, in this kernel's own text: on the shared ones the
    // 128-wide instance took 4 more SGPRs and measured 0.5 % slower (profiles/conv_one_text_bench.txt)
    constexpr int INS = 2 * A_RG + W_INS;
    int issued = 0;
#pragma unroll
    for (int p = 0; p < ST - 1; ++p)
        if (p < nk) { issue(p, p); ++issued; }
    int slot = 0, islot = (ST - 1) % ST;
    for (int kt = 0; kt < nk; ++kt) {
        if (issued - kt - 1 >= ST - 2 && ST > 2) {
            if constexpr (ST == 3) asm volatile("s_waitcnt vmcnt(%0)" :: "n"(INS) : "memory");
            else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        } else {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        }
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (issued < nk) { issue(issued, islot); ++issued; islot = islot + 1 == ST ? 0 : islot + 1; }
        const unsigned char* A = smem + slot * STAGE;
        slot = slot + 1 == ST ? 0 : slot + 1;
        cdma32_mfma_step<MF, NF, AP, WP>(A, A + 2 * AP, wrow_m, wrow_n, fr, fq, acc);
    }
    asm volatile("s_barrier" ::: "memory");                       // the staged epilogue reuses the tile buffers
    finish_tile<MF, NF, false, WM, BN>(g, acc, M, m0, n0, wrow_m, wrow_n, lane, wave, smem, tm);
}

// ---------------------------------------------------------------------------------------------
// Small-map convolution ("conv_small", off by default): the detector at the one or few images a request
// carries.  A 20 x 20 map is four 128-row tiles per 64 columns - 8 or 16 workgroups on 256 CUs, each walking 18 K steps alone.
// Here a workgroup owns BM x 64 outputs and splits K inside itself, as gemm_mid_kernel does for the linears: its 8 waves are KS
// groups of 8 / KS waves, group q taking the 64-deep K steps q, q + KS, ... into its own two-stage ring.
//   <64, 2>: two halves x (2 x 2 waves of 32 x 32), 2 x 2 x (64 + 64) rows x 128 B = 64 KB, two workgroups per CU;
//   <32, 4>: four quarters x (1 x 2 waves of 32 x 32), 4 x 2 x (32 + 64) rows x 128 B = 96 KB, one workgroup per CU.
// The gather is cgemm_dma_kernel's, by the same device text: per-lane pixel offset and tap bits once per tile, padding through the
// descriptor's range check, tap displacement / channel base / source of a K step in the DMA's scalar offset.  One barrier per trip
// (KS K steps), shared by the groups; a group whose step does not exist on the last trip idles through it (K of one step: group 0
// alone works, the others add zeros).
// The partial tiles meet in LDS, overlaying the rings after the last barrier: every group writes its four 16 x 16 fragments, and
// wave w of group q finishes the 4 / KS fragments f = q, q + KS (f = column fragment * 2 + row fragment) of wave tile w as
// group 0 + group 1 (+ group 2 + group 3), left to right in that order, whichever group the wave belongs to.  All 8 waves then run
// finish_tile on the sums (the direct epilogue: bias, SiLU, bf16 shortcut, f32 output, channel offset and pixel stride through
// out / ldo).  One launch, no workspace, no atomics: the result does not depend on the launch.
// Eligibility (host): cgemm_dma_kernel's.  No STATS, PHASE, BNBWD or MXFP8 form.
// ---------------------------------------------------------------------------------------------
// One tile of cgemm_small_kernel: ONE text for the kernel below and for cgemm_small_group_kernel (bid, nwg, the LDS: as cdma_tile).
template <int BM, int KS>
__device__ __forceinline__ void csmall_tile(const GemmArgs& g, int bid, const int nwg) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    constexpr int BN = 64, GW = 8 / KS, WGM = GW / 2;            // waves per group, as WGM x 2 wave tiles of 32 x 32
    static_assert((KS == 2 || KS == 4) && BM == WGM * 32, "64-row halves or 32-row quarters");
    constexpr int MF = 2, NF = 2, NS = 4 / KS;                   // fragments of a wave tile; those a wave finishes
    constexpr int STAGE = (BM + BN) * 128, RING = 2 * STAGE;     // bytes: one K step of a group, a group's two stages
    constexpr int A_INS = BM / (8 * GW), W_INS = BN / (8 * GW);
    static_assert(8 * 4 * 64 * 16 <= KS * RING, "the exchange overlays the rings");
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int grp = wave / GW, gw = wave - grp * GW;
    const int M = g.M;
    bid = xcd_remap(bid, nwg);
    const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    // a group's waves fill its stage
    const CdmaLanes<A_INS, W_INS, GW> L = cdma_lanes<false, A_INS, W_INS, GW>(g, M, m0, n0, gw, lane);
    const auto rs0 = cdma_rsrc((const unsigned char*)g.a0 - L.bias0), rs1 = cdma_rsrc(g.c1 ? g.a1 : g.a0), rsW = cdma_rsrc(g.w);
    unsigned char* const ring = smem + grp * RING;
    const auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        unsigned char* A = ring + buf * STAGE;
        cdma_gather(g, L, rs0, rs1, kt * BK, [&](int j) __attribute__((always_inline)) { return A + (j * GW + gw) * 1024; });
#pragma unroll
        for (int j = 0; j < W_INS; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lptr_t)(A + (BM + j * GW * 8 + gw * 8) * 128), 16, (int)L.w_off[j], kt * BK * 2, 0, 0);
    };

    f32x4 acc[NF][MF];
    // (wave_tile<BM, BN, WGM, 2> written out: through the helper these kernels take 4 more VGPRs, profiles/conv_one_text_resources.txt)
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wrow_m = (gw >> 1) * 32, wrow_n = (gw & 1) * 32;
    const int fr = lane & 15, fq = lane >> 4;

    const int nk = g.K / BK, trips = (nk + KS - 1) / KS;         // trip t: K step KS t + grp (the last trip may lack it)
    if (grp < nk) issue(grp, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < trips; ++t) {
        const int cur = t & 1, kt = KS * t + grp;
        if (kt + KS < nk) issue(kt + KS, cur ^ 1);              // (the stage read on trip t - 1: every wave passed its barrier)
        if (kt < nk) {
            const unsigned char* A = ring + cur * STAGE;
            cdma_mfma_step<MF, NF>(A, A + BM * 128, wrow_m, wrow_n, fr, fq, acc);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                        // (the last one: every fragment read is done, the rings are free)
    }
    // exchange: xch[grp][gw][f][lane], f = i * 2 + j, holds fragment (i, j) of that wave's partial tile
    f32x4* const xch = (f32x4*)smem;
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) xch[((grp * GW + gw) * 4 + i * 2 + j) * 64 + lane] = acc[i][j];
    __syncthreads();
    f32x4 sum[NS][1];
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        const int f = grp + KS * s;
        f32x4 v = xch[(gw * 4 + f) * 64 + lane];
#pragma unroll
        for (int p = 1; p < KS; ++p) v = v + xch[((p * GW + gw) * 4 + f) * 64 + lane];      // group 0 + 1 (+ 2 + 3), in that order
        sum[s][0] = v;
    }
    // f = grp + KS s: row fragment grp & 1, column fragments (grp >> 1) + (KS / 2) s - consecutive for NS = 2 (grp >> 1 = 0)
    finish_tile<1, NS>(g, sum, M, m0, n0, wrow_m + (grp & 1) * 16, wrow_n + (grp >> 1) * 16, lane, wave, smem);
}

template <int BM, int KS>
__global__ __launch_bounds__(512, KS == 2 ? 2 : 1) void cgemm_small_kernel(GemmArgs g) {
    csmall_tile<BM, KS>(g, blockIdx.x, gridDim.x);
}

// ---------------------------------------------------------------------------------------------
// Grouped launch ("conv2d_group"): ONE grid whose workgroups belong to up to YV_CONV_GROUP_MAX independent
// convolutions of one kernel instance - the Detect head's three levels in one step.  The members travel in the kernel arguments by
// value (no device table, no copy): their GemmArgs, in launch order, and first[i], the first workgroup of member i (first[n]: the
// grid).  Every first[i] is a multiple of 8, so a workgroup's position in the round robin over the eight XCDs is the same in the
// grid and inside its member, and the tile bodies' remap runs on the member-local index with the member's own workgroup count
// (tiles_m * tiles_n): what it means in a single launch.  The workgroups between a member's last tile and the next multiple of 8
// return at once.  A workgroup finds its member by a uniform scan of first[]; the member's descriptor is then read where it lies, in
// the kernel-argument segment, through scalar loads (no private copy: the resource report shows no scratch).
// No state crosses members: each member's output is, bit for bit, what the single launch of the same instance writes.
// ---------------------------------------------------------------------------------------------
struct ConvGroupArgs {
    GemmArgs m[YV_CONV_GROUP_MAX];
    int first[YV_CONV_GROUP_MAX + 1];
    int n;
};
static_assert(sizeof(ConvGroupArgs) + 256 <= 4096, "the member table (+ the hidden arguments) stays inside the 4 KB kernel-argument segment");

// the member of workgroup bid (uniform) and bid's index inside it; false: a padding workgroup
__device__ __forceinline__ bool conv_group_member(const ConvGroupArgs& p, int bid, int& member, int& local) {
    int i = 0;
    while (i + 1 < p.n && bid >= p.first[i + 1]) ++i;
    member = i;
    local = bid - p.first[i];
    return local < p.m[i].tiles_m * p.m[i].tiles_n;
}

template <int BN, int WM, int WN, int ST>
__global__ __launch_bounds__(256) void cgemm_dma_group_kernel(ConvGroupArgs p) {
    int i, local;
    if (!conv_group_member(p, blockIdx.x, i, local)) return;
    const GemmArgs& g = p.m[i];
    cdma_tile<BN, WM, WN, ST, false, false, false>(g, local, g.tiles_m * g.tiles_n);
}

template <int BM, int KS>
__global__ __launch_bounds__(512, KS == 2 ? 2 : 1) void cgemm_small_group_kernel(ConvGroupArgs p) {
    int i, local;
    if (!conv_group_member(p, blockIdx.x, i, local)) return;
    const GemmArgs& g = p.m[i];
    csmall_tile<BM, KS>(g, local, g.tiles_m * g.tiles_n);
}

// ---------------------------------------------------------------------------------------------
// MXFP8 variant of the LDS-DMA GEMM (BASELINE.json configs[4]: FP8 classifier GEMMs).  Operands are OCP e4m3 bytes
// with one E8M0 scale per 32 consecutive K elements of a row (the OCP "MX" block format); the block-scaled
// v_mfma_scale_f32_16x16x128_f8f6f4 applies both scales in hardware and runs at twice the bf16 MFMA rate.  A 128-byte LDS
// row holds 128 K elements (one MFMA K step), so tile shape, DMA, swizzle and epilogues are those of gemm_dma_kernel:
// the L2->LDS traffic per flop - what bounds the bf16 main loop - is halved.
//   operand layout (measured with yv_mx_probe, tests/test_gpu_fp8.py::test_mx_mfma_layout): lane l = (row l&15, group
//   g = l>>4) holds K elements 16g..16g+15 in its first 16 bytes and 64+16g..64+16g+15 in its second 16 bytes, i.e. the
//   16-byte chunks g and 4+g of the 128-byte row; the scale of the MX block k = 32j..32j+31 of that row is byte `opsel`
//   of the scale VGPR of lane (row, group j) - so lane (row, g) loads the scale of block g of the current K step.
// Scales are read with ordinary byte loads one K step ahead (issued behind the DMA of that step, consumed after the
// step's vmcnt(0)), so they never add a wait of their own.
// ---------------------------------------------------------------------------------------------

struct MxArgs {
    GemmArgs g;                 // a0 / w point at the fp8 bytes (row strides lda0 / K bytes); epilogue fields as usual
    const uint8_t* sa;          // E8M0 scales, K-step-major: (K/128, rows_a, 4) - the 4 blocks of one 128-deep K step of a row
    const uint8_t* sw;          // (K/128, rows_w, 4)                               are one aligned dword
    long long rows_a, rows_w;   // row counts of the scale arrays (multiples of 128: a tile's 128 dwords are one DMA half)
};

template <int BM, int BN, int WM, int WN>
__global__ __launch_bounds__(WM * WN * 64) void gemm_mx_kernel(MxArgs a) {
    const GemmArgs& g = a.g;
    constexpr int NW = WM * WN, MF = BM / WM / 16, NF = BN / WN / 16, A_BYTES = BM * 128, W_BYTES = BN * 128;
    constexpr int A_INS = BM / (8 * NW), W_INS = BN / (8 * NW);
    constexpr int S_INS = (BM + BN + 255) / 256;              // wave-instructions that fetch the tile's scale dwords
    constexpr int S_BYTES = S_INS * 1024;                      // one scale dword per tile row and K step (+ slack of the last DMA)
    constexpr int STAGE = A_BYTES + W_BYTES + S_BYTES;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    int bid = xcd_remap(blockIdx.x, gridDim.x);
    // split-K (the MX weight gradient, yv_wgrad_mxfp8: few output tiles, long token reduction): the slices of one tile are
    // neighbouring workgroups; partial sums go to g.partial, splitk_reduce_kernel adds them in slice order
    const int nsplit = g.splitk > 1 ? g.splitk : 1;
    const int slice = bid % nsplit;
    bid /= nsplit;
    int tm, tn;
    {
        const int GM = g.group_m, per = GM * g.tiles_n;
        const int grp = bid / per, first = grp * GM;
        const int gsz = (g.tiles_m - first) < GM ? (g.tiles_m - first) : GM;
        const int in = bid - grp * per;
        tm = first + in % gsz;
        tn = in / gsz;
    }
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;
    const long long ldwb = g.ldw > 0 ? g.ldw : g.K;            // W row stride in bytes (0: dense, K)
    const int lrow = lane >> 3, lch = lane & 7;
    const uint8_t* a_src[A_INS];
    const uint8_t* w_src[W_INS];
#pragma unroll
    for (int j = 0; j < A_INS; ++j) {
        const int r = (j * NW + wave) * 8 + lrow;
        int m = m0 + r; m = m < g.M ? m : g.M - 1;
        a_src[j] = (const uint8_t*)g.a0 + (long long)m * g.lda0 + ((lch ^ (r & 7)) << 4);
    }
#pragma unroll
    for (int j = 0; j < W_INS; ++j) {
        const int r = (j * NW + wave) * 8 + lrow;
        int n = n0 + r; n = n < g.N ? n : g.N - 1;
        w_src[j] = (const uint8_t*)g.w + (long long)n * ldwb + ((lch ^ (r & 7)) << 4);
    }
    // scale DMA: the tile's BM A dwords then its BN W dwords, 4 dwords (16 bytes) per lane, lane-linear in LDS; the
    // (BM + BN) / 256 wave-instructions are dealt to waves 0, 1, ...
    const int s_dw = (wave * 64 + lane) * 4;                   // first dword this lane would fetch if its wave takes part
    const bool s_on = wave < S_INS && s_dw < BM + BN;
    const uint8_t* s_src = s_dw < BM ? a.sa + ((long long)m0 + s_dw) * 4 : a.sw + ((long long)n0 + (s_dw - BM)) * 4;
    const long long s_step = (s_dw < BM ? a.rows_a : a.rows_w) * 4;
    auto issue = [&](int kt, int buf) {
        unsigned char* A = smem + buf * STAGE;
        unsigned char* W = A + A_BYTES;
#pragma unroll
        for (int j = 0; j < A_INS; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(a_src[j] + kt * 128), (lptr_t)(A + (j * NW + wave) * 1024), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < W_INS; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(w_src[j] + kt * 128), (lptr_t)(W + (j * NW + wave) * 1024), 16, 0, 0);
        if (wave < S_INS) {
            // lanes past the end of the scale block re-fetch its last 16 bytes into their (unused) slot: exec stays full
            const uint8_t* sp = s_on ? s_src + kt * s_step : a.sw + (long long)n0 * 4 + kt * a.rows_w * 4;
            __builtin_amdgcn_global_load_lds((gptr_t)sp, (lptr_t)(W + W_BYTES + wave * 1024), 16, 0, 0);
        }
    };
    const int wm = wave / WN, wn = wave - wm * WN;
    const int wrow_m = wm * (BM / WM), wrow_n = wn * (BN / WN);
    const int fr = lane & 15, fq = lane >> 4;
    f32x4 acc[NF][MF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int nk_all = g.K >> 7;
    const int kt0 = (int)((long long)nk_all * slice / nsplit), nk = (int)((long long)nk_all * (slice + 1) / nsplit);
    issue(kt0, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int kt = kt0; kt < nk; ++kt) {
        const int cur = (kt - kt0) & 1;
        if (kt + 1 < nk) issue(kt + 1, cur ^ 1);
        const unsigned char* A = smem + cur * STAGE;
        const unsigned char* W = A + A_BYTES;
        const unsigned char* S = W + W_BYTES;
        i32x8 fa[MF], fw[NF];
        int sca[MF], scw[NF];
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            const int rr = wrow_m + j * 16 + fr;
            const u32x4 lo = *(const u32x4*)(A + rr * 128 + (((fq) ^ (rr & 7)) << 4));
            const u32x4 hi = *(const u32x4*)(A + rr * 128 + (((4 + fq) ^ (rr & 7)) << 4));
            fa[j] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            sca[j] = (int)(*(const uint32_t*)(S + rr * 4) >> (8 * fq));              // byte 0 = scale of block fq
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int rr = wrow_n + i * 16 + fr;
            const u32x4 lo = *(const u32x4*)(W + rr * 128 + (((fq) ^ (rr & 7)) << 4));
            const u32x4 hi = *(const u32x4*)(W + rr * 128 + (((4 + fq) ^ (rr & 7)) << 4));
            fw[i] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
            scw[i] = (int)(*(const uint32_t*)(S + BM * 4 + rr * 4) >> (8 * fq));
        }
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < MF; ++j)
                acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[i], fa[j], acc[i][j], 0, 0, 0, scw[i], 0, sca[j]);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    if (nsplit > 1) {                          // raw partial sums; the epilogue runs in splitk_reduce_kernel
        float* P = g.partial + (long long)slice * g.M * g.N;
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            const int m = m0 + wrow_m + j * 16 + fr;
            if (m >= M) continue;
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int n = n0 + wrow_n + i * 16 + fq * 4;
                if (n < g.N) *(float4*)(P + (long long)m * g.N + n) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
            }
        }
        return;
    }
    finish_tile<MF, NF>(g, acc, M, m0, n0, wrow_m, wrow_n, lane, wave, smem);
}

// one MFMA on caller-provided register images (layout probe used while bringing the MX path up; tests keep it as the
// executable statement of the operand layout)
__global__ __launch_bounds__(64) void mx_probe_kernel(const i32x8* __restrict__ a, const i32x8* __restrict__ b,
                                                      const int* __restrict__ sa, const int* __restrict__ sb, int opsel,
                                                      f32x4* __restrict__ d) {
    const int l = threadIdx.x;
    f32x4 acc = {0.f, 0.f, 0.f, 0.f};
    if (opsel == 0) acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[l], b[l], acc, 0, 0, 0, sa[l], 0, sb[l]);
    else if (opsel == 1) acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[l], b[l], acc, 0, 0, 1, sa[l], 1, sb[l]);
    else if (opsel == 2) acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[l], b[l], acc, 0, 0, 2, sa[l], 2, sb[l]);
    else acc = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(a[l], b[l], acc, 0, 0, 3, sa[l], 3, sb[l]);
    d[l] = acc;
}

// x (rows, K) bf16 -> q (rows, K) e4m3 bytes + one E8M0 scale per 32-element block (the format: mx_quant.h), one thread per block.
// yv_quant_mxfp8: scales K-step-major (K/128, rows_pad, 4).  yv_quant_mxfp8_map (MAP; a row is a pixel of a bf16 NHWC view, K its
// channels): scales (pixel, C/32), ldq bytes per pixel.
template <bool MAP>
__device__ __forceinline__ void quant_mx_rows(const uint16_t* __restrict__ x, long long ldx, long long rows, int K,
                                              uint8_t* __restrict__ q, long long ldq, uint8_t* __restrict__ sc, long long rows_pad) {
    const int kb = K >> 5;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= rows * kb) return;
    const long long r = idx / kb;
    const int b = (int)(idx - r * kb);
    const uint8_t s = mx_quant_row32(x + r * ldx + b * 32, q + r * ldq + b * 32);
    sc[MAP ? mx_scale_map(r, ldq, b) : mx_scale_kmajor(b, rows_pad, r)] = s;
}
__global__ __launch_bounds__(256) void quant_mx_kernel(const uint16_t* __restrict__ x, long long ldx, long long rows, int K,
                                                       uint8_t* __restrict__ q, long long ldq, uint8_t* __restrict__ sc,
                                                       long long rows_pad) {
    quant_mx_rows<false>(x, ldx, rows, K, q, ldq, sc, rows_pad);
}
__global__ __launch_bounds__(256) void quant_mx_map_kernel(const uint16_t* __restrict__ x, long long ldx, long long pixels, int C,
                                                           uint8_t* __restrict__ q, long long ldq, uint8_t* __restrict__ sc) {
    quant_mx_rows<true>(x, ldx, pixels, C, q, ldq, sc, 0);
}

// ---------------------------------------------------------------------------------------------
// MXFP8 convolution (cgemm_mx_kernel; BASELINE.json configs[4]: FP8 detector convolutions, opt-in).  cgemm_dma_kernel's
// structure - per-lane pixel offsets, tap-validity bits, everything that changes along K in the DMA's scalar offset - on
// the block-scaled MFMA of gemm_mx_kernel: e4m3 bytes, so a 128-byte LDS row is one 128-deep K step, half the DMA
// instructions, LDS bytes and L2 reads per flop of the bf16 kernel.
//   Inputs are MX maps (yv_mx_view): e4m3 NHWC bytes + one E8M0 scale per (pixel, 32-channel block).  With Cin % 128 != 0 a
//   K step straddles taps (or the two sources of a 1 x 1), but each of its four 32-element blocks lies inside ONE tap and
//   ONE source.  So the LDS tile is stored BLOCK-major, [block 0..3][row][32 B], and wave w fetches block w of every row:
//   one wave-instruction = 32 rows x 32 B of one block, whose (tap, source, channel base) is wave-uniform and travels in the
//   scalar offset exactly as in cgemm_dma_kernel - no per-lane select, no per-element work, for any Cin % 32 == 0.
//   Inside a 32-byte row the two 16-byte halves are swapped on rows with bit 3 set (source side of the DMA, undone on the
//   fragment read): the ds_read_b128 of 16 rows x one half are then conflict free.
//   Fragment of lane (row r, group g) (layout of test_mx_mfma_layout): K chunks g and 4 + g of the step = half g & 1 of
//   blocks g >> 1 and 2 + (g >> 1).  Scales: lane (r, g) supplies the scale of block g of row r - for the activation the
//   byte of block g at ITS tap pixel (zero-data taps read scale 0), for the weight byte g of the K-step-major dword
//   yv_quant_mxfp8 writes.  They are loaded into registers one K step ahead, behind the DMA of that step.
//   K is zero-padded to a multiple of 128 (the weight's padding is zeros, the activation's padding blocks read zeros).
//   Epilogue: finish_tile (bias, SiLU, bf16 shortcut, bf16 / f32 output), or - when an MX-map output is wanted - the bf16
//   staged epilogue followed by the block quantiser of mx_quant.h on the bf16-rounded values (byte-identical to the bf16
//   output quantised afterwards), with or without the bf16 store.
// ---------------------------------------------------------------------------------------------
struct ConvMxArgs {
    GemmArgs g;                 // a0 / a1 -> e4m3 bytes (lda0 / lda1: bytes per pixel), w -> (N, K) e4m3, K = padded depth
    const uint8_t* s0;          // per-pixel scales of the sources (pixel stride lda / 32 bytes)
    const uint8_t* s1;
    int kreal;                  // k * k * Cin
    const uint8_t* sw;          // weight scales (K / 128, rows_w, 4)
    long long rows_w;
    uint8_t* oq;                // MX-map output (pixel stride ldq bytes, scales ldq / 32) or null
    uint8_t* os;
    int ldq;
};

// The MX-map output of cgemm_mx_kernel: bias, SiLU and bf16 shortcut as the bf16 branch of epilogue_staged (its slab, its adds), then
// the bf16 store (if wanted) and the block quantiser on the same bf16-rounded values.
template <int MF>
__device__ __forceinline__ void epilogue_conv_mx(const ConvMxArgs& a, f32x4 (&acc)[4][MF], int M, int m0, int n0,
                                                 int wrow_m, int wrow_n, int lane, unsigned char* stage) {
    const GemmArgs& g = a.g;
    const int flags = g.flags;
    const int fr = lane & 15, fq = lane >> 4;
    const int nb = n0 + wrow_n;
#pragma unroll
    for (int j = 0; j < MF; ++j)
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int n = nb + i * 16 + fq * 4;
            float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
            if ((flags & YV_EPI_BIAS) && n < g.N) b = *(const float4*)(g.bias + n);
            float v[4] = {acc[i][j][0] + b.x, acc[i][j][1] + b.y, acc[i][j][2] + b.z, acc[i][j][3] + b.w};
            if (flags & YV_EPI_SILU) {
#pragma unroll
                for (int q = 0; q < 4; ++q) v[q] = silu_f(v[q]);
            }
            slab_put(stage, i, j, fr, fq, v);
        }
#pragma unroll
    for (int it = 0; it < MF * 2; ++it) {
        const int row = it * 8 + (lane >> 3), ch = lane & 7;
        const int m = m0 + wrow_m + row, n = nb + ch * 8;
        uint4 pk = slab_row(stage, row, ch);
        if (m < M && n < g.N) {           // (N % 32 == 0: the four lanes of a 32-channel block agree)
            if (flags & YV_EPI_RES_BF16) pk = add_bf16x8(pk, *(const uint4*)(g.res + (long long)m * g.ldres + n));
            if (g.out) *(uint4*)((uint16_t*)g.out + (long long)m * g.ldo + n) = pk;
            uint2 q8;
            const int e = mx_quant_bf16x8(pk, q8);
            *(uint2*)(a.oq + (long long)m * a.ldq + n) = q8;
            if ((ch & 3) == 0) a.os[mx_scale_map(m, a.ldq, n >> 5)] = (uint8_t)(e + 127);
        }
    }
}

template <int BN, int WM, int WN>
__global__ __launch_bounds__(256) void cgemm_mx_kernel(ConvMxArgs a) {
    const GemmArgs& g = a.g;
    constexpr int BM = 128, NW = 4;
    static_assert(WM * WN == NW, "four waves");
    constexpr int MF = BM / WM / 16, NF = BN / WN / 16;
    static_assert(NF == 4 && (MF % 2) == 0, "staged epilogue shapes");
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128, STAGE = A_BYTES + W_BYTES;
    constexpr int A_INS = BM / 32, W_INS = BN / 32;            // wave-instructions per wave and K step: 32 rows x one block
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int M = g.M;
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    const int tm = bid / g.tiles_n, tn = bid - tm * g.tiles_n;
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    const int Cin = g.c0 + g.c1, KK = g.ksize * g.ksize;
    const int hw = g.Hout * g.Wout;
    const int sld0 = g.lda0 >> 5, sld1 = g.lda1 >> 5;
    // DMA lanes: lane l writes half l & 1 of row l >> 1 of a 32-row piece; the half it fetches is swapped on rows with bit 3 set.
    // The pixel geometry of an output row is conv_pixel_geom's, here times the pixel stride in bytes (e4m3) + the half.
    const int lr = lane >> 1, hsrc = ((lane & 1) ^ ((lr >> 3) & 1)) << 4;
    uint32_t a_off0[A_INS], a_off1[A_INS], a_taps[A_INS], w_off[W_INS];
#pragma unroll
    for (int j = 0; j < A_INS; ++j) {
        long long p0, p1;
        conv_pixel_geom<false>(g, M, hw, m0 + j * 32 + lr, p0, p1, a_taps[j]);
        a_off0[j] = (uint32_t)(p0 * g.lda0 + hsrc);
        a_off1[j] = (uint32_t)(p1 * g.lda1 + hsrc);
    }
#pragma unroll
    for (int j = 0; j < W_INS; ++j) {
        int n = n0 + j * 32 + lr;
        n = n < g.N ? n : g.N - 1;
        w_off[j] = (uint32_t)(n * g.K + hsrc);
    }
    f32x4 acc[NF][MF];
    const WaveTile wv = wave_tile<BM, BN, WM, WN>(wave, lane, acc);
    const int wrow_m = wv.wrow_m, wrow_n = wv.wrow_n, fr = wv.fr, fq = wv.fq;
    // scale lanes: lane (fr, fq) of fragment row j / column i
    int s_pix0[MF], s_pix1[MF];
    uint32_t s_taps[MF];
#pragma unroll
    for (int j = 0; j < MF; ++j) {
        long long p0, p1;
        conv_pixel_geom<false>(g, M, hw, m0 + wrow_m + j * 16 + fr, p0, p1, s_taps[j]);
        s_pix0[j] = (int)(p0 * sld0);
        s_pix1[j] = (int)(p1 * sld1);
    }
    const uint8_t* sw_row[NF];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        int n = n0 + wrow_n + i * 16 + fr;
        n = n < g.N ? n : g.N - 1;
        sw_row[i] = a.sw + (long long)n * 4 + fq;
    }

    // source 0's descriptor starts one row + one pixel before the tensor (3 x 3 only): the scalar offset is unsigned
    const uint32_t bias0 = g.ksize == 3 ? (uint32_t)((g.Win + 1) * g.lda0) : 0u;
    const auto rs0 = __builtin_amdgcn_make_buffer_rsrc((void*)((const unsigned char*)g.a0 - bias0), 0, 0x7fffffff, 0x00020000);
    const auto rs1 = __builtin_amdgcn_make_buffer_rsrc((void*)(g.c1 ? g.a1 : g.a0), 0, 0x7fffffff, 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)g.w, 0, 0x7fffffff, 0x00020000);

    // (tap, channel) of the K position this wave's block / this lane's scale block has in the NEXT step to be fetched
    int wt = 0, wc = 32 * wave;
    while (wc >= Cin) { wc -= Cin; ++wt; }
    int lt = 0, lc = 32 * fq;
    while (lc >= Cin) { lc -= Cin; ++lt; }

    auto issue = [&](int kt, int buf) __attribute__((always_inline)) {
        unsigned char* A = smem + buf * STAGE + wave * (BM * 32);
        unsigned char* W = smem + buf * STAGE + A_BYTES + wave * (BN * 32);
        if (wt >= KK) {                                          // K padding: zeros
#pragma unroll
            for (int j = 0; j < A_INS; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lptr_t)(A + j * 1024), 16, (int)DMA_OOB, 0, 0, 0);
        } else if (g.c1 && wc >= g.c0) {                         // second source of a two-source 1 x 1
#pragma unroll
            for (int j = 0; j < A_INS; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs1, (lptr_t)(A + j * 1024), 16,
                                                         (int)((a_taps[j] & 1u) ? a_off1[j] : DMA_OOB), wc - g.c0, 0, 0);
        } else {
            uint32_t so = (uint32_t)wc;
            if (g.ksize == 3) {
                const int ky = wt >= 6 ? 2 : (wt >= 3 ? 1 : 0), kx = wt - ky * 3;
                so = bias0 + (uint32_t)(((ky - 1) * g.Win + (kx - 1)) * g.lda0 + wc);
            }
#pragma unroll
            for (int j = 0; j < A_INS; ++j)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rs0, (lptr_t)(A + j * 1024), 16,
                                                         (int)(((a_taps[j] >> wt) & 1u) ? a_off0[j] : DMA_OOB), (int)so, 0, 0);
        }
#pragma unroll
        for (int j = 0; j < W_INS; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lptr_t)(W + j * 1024), 16, (int)w_off[j], kt * 128 + 32 * wave, 0, 0);
        wc += 128;
        while (wc >= Cin) { wc -= Cin; ++wt; }
    };
    int sca[MF], scw[NF];
    auto load_scales = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            int s = 0;
            if (lt < KK) {
                if (g.c1 && lc >= g.c0) {
                    if (s_taps[j] & 1u) s = a.s1[s_pix1[j] + ((lc - g.c0) >> 5)];
                } else if ((s_taps[j] >> lt) & 1u) {
                    int d = 0;
                    if (g.ksize == 3) {
                        const int ky = lt >= 6 ? 2 : (lt >= 3 ? 1 : 0), kx = lt - ky * 3;
                        d = ((ky - 1) * g.Win + (kx - 1)) * sld0;
                    }
                    s = a.s0[s_pix0[j] + d + (lc >> 5)];
                }
            }
            sca[j] = s;
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) scw[i] = sw_row[i][(long long)kt * a.rows_w * 4];
        lc += 128;
        while (lc >= Cin) { lc -= Cin; ++lt; }
    };

    const int nk = g.K >> 7;
    issue(0, 0);
    load_scales(0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    const int hrd = ((fq & 1) << 4);
    for (int kt = 0; kt < nk; ++kt) {
        const int cur = kt & 1;
        int sa_c[MF], sw_c[NF];
#pragma unroll
        for (int j = 0; j < MF; ++j) sa_c[j] = sca[j];
#pragma unroll
        for (int i = 0; i < NF; ++i) sw_c[i] = scw[i];
        if (kt + 1 < nk) { issue(kt + 1, cur ^ 1); load_scales(kt + 1); }
        const unsigned char* A = smem + cur * STAGE;
        const unsigned char* W = A + A_BYTES;
        i32x8 fa[MF], fw[NF];
#pragma unroll
        for (int j = 0; j < MF; ++j) {
            const int rr = wrow_m + j * 16 + fr;
            const int o = rr * 32 + (hrd ^ ((rr & 8) << 1));
            const u32x4 lo = *(const u32x4*)(A + (fq >> 1) * (BM * 32) + o);
            const u32x4 hi = *(const u32x4*)(A + (2 + (fq >> 1)) * (BM * 32) + o);
            fa[j] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        }
#pragma unroll
        for (int i = 0; i < NF; ++i) {
            const int rr = wrow_n + i * 16 + fr;
            const int o = rr * 32 + (hrd ^ ((rr & 8) << 1));
            const u32x4 lo = *(const u32x4*)(W + (fq >> 1) * (BN * 32) + o);
            const u32x4 hi = *(const u32x4*)(W + (2 + (fq >> 1)) * (BN * 32) + o);
            fw[i] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
        }
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < MF; ++j)
                // inline asm, as in gemm_p9_kernel<MX> (the builtin's register allocation spilled there); operands come from
                // LDS reads and scale loads the compiler waits for (inputs of the statement): the s_nop covers a just-written
                // operand, the accumulator chains MFMA -> MFMA
#if defined(__HIP_DEVICE_COMPILE__)       // (the host pass cannot place 32-byte "v" operands)
                asm volatile("s_nop 1\n\tv_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
                             : "+v"(acc[i][j]) : "v"(fw[i]), "v"(fa[j]), "v"(sw_c[i]), "v"(sa_c[j]));
#endif
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // the last MFMAs' results are read by ordinary VALU code next: their write-back latency is not tracked for asm
    asm volatile("s_nop 7\n\ts_nop 7\n\ts_nop 7" ::: "memory");
    if (a.oq) epilogue_conv_mx<MF>(a, acc, M, m0, n0, wrow_m, wrow_n, lane, smem + wave * (MF * 16 * 128));
    else finish_tile<MF, NF>(a.g, acc, M, m0, n0, wrow_m, wrow_n, lane, wave, smem);
}

// Two-form quantiser (yv_quant_mxfp8_2d; the MX trainer's operands).  A workgroup stages a tile of 64 rows (t) x 128 columns
// (c) of the bf16 input in LDS (rows past T read as zeros) and writes, from the one read:
//   row form:    thread (row tid / 4, block tid % 4): one 32-column block through mx_quant_row32, the body of quant_mx_kernel;
//   column form: thread (column tid % 128, half tid / 128): the 32 rows of that column as one MX block of the TRANSPOSE, i.e.
//                bytes (C, T_pad) (row stride ldqt) and scales K-step-major along t, (T_pad/128, c_rows_pad, 4) - what
//                yv_quant_mxfp8 writes for x^T padded with zero rows up to T_pad (the weight-gradient operands).
// LDS rows are 272 bytes (16-byte pad): the row-form reads of a wave (16 rows x 4 blocks) spread over the banks; the column-form
// reads of a wave are 64 consecutive bf16 of one row.
__global__ __launch_bounds__(256) void quant_mx_2d_kernel(const uint16_t* __restrict__ x, long long ldx, long long T, int C,
                                                          uint8_t* __restrict__ q, long long ldq, uint8_t* __restrict__ sc,
                                                          long long rows_pad, uint8_t* __restrict__ qt, long long ldqt,
                                                          uint8_t* __restrict__ sct, long long c_rows_pad) {
    constexpr int PITCH = 272;
    __shared__ __attribute__((aligned(16))) unsigned char tile[64 * PITCH];
    const int tid = threadIdx.x;
    const long long t0 = (long long)blockIdx.x * 64;
    const int c0 = blockIdx.y * 128;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int id = tid + 256 * i, r = id >> 4, ch = id & 15;
        uint4 u = make_uint4(0u, 0u, 0u, 0u);
        if (t0 + r < T) u = *(const uint4*)(x + (t0 + r) * ldx + c0 + ch * 8);
        *(uint4*)(tile + r * PITCH + ch * 16) = u;
    }
    __syncthreads();
    if (q) {
        const int r = tid >> 2, b = tid & 3;
        const long long t = t0 + r;
        if (t < T) {
            const uint8_t s = mx_quant_row32((const uint16_t*)(tile + r * PITCH + b * 64), q + t * ldq + c0 + b * 32);
            sc[mx_scale_kmajor((c0 >> 5) + b, rows_pad, t)] = s;
        }
    }
    if (qt) {
        const int c = tid & 127, h = tid >> 7;
        float v[32];
#pragma unroll
        for (int i = 0; i < 32; ++i) v[i] = bf16_to_f32(*(const uint16_t*)(tile + (h * 32 + i) * PITCH + c * 2));
        uint32_t out[8];
        const int e = mx_quant_block(v, out);
        const long long tb = (t0 >> 5) + h;                      // 32-row block of t
        uint4* dst = (uint4*)(qt + (long long)(c0 + c) * ldqt + tb * 32);
        dst[0] = make_uint4(out[0], out[1], out[2], out[3]);
        dst[1] = make_uint4(out[4], out[5], out[6], out[7]);
        sct[mx_scale_kmajor((int)tb, c_rows_pad, c0 + c)] = (uint8_t)(e + 127);
    }
}

// ---------------------------------------------------------------------------------------------
// Weight-gradient GEMM ("TN"): dW[n][k] = sum_t dY[t][n] * X[t][k], t = token (the reduction index).
// Both operands are stored token-major, i.e. the reduction index is the ROW of the LDS tiles, so the MFMA
// fragments (8 consecutive reduction elements per lane) are COLUMNS of those tiles: they are read with the
// gfx950 hardware-transposing LDS read ds_read_b64_tr_b16 (two reads per fragment), and no transposed copy of
// the activations or of the incoming gradient is ever materialised.
//   tiles: [64 tokens][128 columns] bf16 = 256-byte LDS rows, filled by LDS-DMA (4 rows per wave-instruction);
//   the 16-byte chunk index is XOR-swizzled with ((row&3)<<1 | ((row>>3)&1)<<3) on the SOURCE address and on the
//   read, which spreads the 4 rows x 4 chunks a 16-lane group touches (and the two groups of a 32-lane half)
//   over distinct banks.
//   MFMA A operand = X columns (rows of the result = k), B operand = dY columns (result columns = n), so a lane
//   owns 4 consecutive k of one n: 16-byte f32 stores into dW (n, k).
// Token rows must be padded with ZERO rows up to a multiple of 64 (the trainer allocates its activations so).
// Few output tiles, long reduction -> always split over the token dimension (deterministic slice-order reduce).
// ---------------------------------------------------------------------------------------------

// The gather form (yv_wgrad_conv3_gather): X is not a (T, K) matrix but the virtual im2col of a 3 x 3 / pad 1
// convolution's input x (B, Hin, Win, Cin), row stride ldx: row m = output pixel (b, oy, ox), column k = (ky * 3 + kx) * Cin + ci,
// the K order of yv_im2col3.  A lane's 16-byte chunk lies inside one tap (Cin % 8 == 0), so its source is x's own pixel
// (b, oy * stride + ky - 1, ox * stride + kx - 1) or, for a tap in the padding or a row past T, a zero chunk of the library's.
// The LDS then holds what the im2col path puts there, and everything behind the DMA is unchanged.
// m -> (b, oy, ox) without a division: q = (m * mul) >> sh with mul = ceil(2^sh / d), sh = 31 + ceil(log2 d), exact for every
// 0 <= m < 2^31 (Granlund & Montgomery 1994, theorem 4.2 with N = 31; mul < 2^32).  ONE function computes the index, for the
// kernels and, through yv_wgrad_conv3_gather_src, for the host.
struct ConvGather {
    const uint16_t* x;
    long long ldx;
    int T, Hin, Win, Hout, Wout, stride, Cin;
    uint32_t mul_w, mul_h;          // m / Wout, (m / Wout) / Hout
    int sh_w, sh_h;
};
__device__ uint4 g_zero_chunk = {0u, 0u, 0u, 0u};            // what a tap in the padding reads

inline void gather_magic(int d, uint32_t* mul, int* sh) {
    int l = 0;
    while ((1LL << l) < d) ++l;
    *sh = 31 + l;
    *mul = (uint32_t)(((1ULL << *sh) + (unsigned long long)d - 1) / (unsigned long long)d);
}
inline ConvGather conv_gather_of(const void* x, long long ldx, int B, int Hin, int Win, int stride, int Cin) {
    ConvGather q = {};
    q.x = (const uint16_t*)x; q.ldx = ldx; q.Hin = Hin; q.Win = Win; q.stride = stride; q.Cin = Cin;
    q.Hout = (Hin - 1) / stride + 1; q.Wout = (Win - 1) / stride + 1;
    q.T = B * q.Hout * q.Wout;
    gather_magic(q.Wout, &q.mul_w, &q.sh_w);
    gather_magic(q.Hout, &q.mul_h, &q.sh_h);
    return q;
}
// input pixel index (b * Hin + iy) * Win + ix that tap (ky, kx) of output pixel m reads, -1: zero (padding, or m >= T)
__host__ __device__ __forceinline__ long long conv_gather_pixel(const ConvGather& q, int m, int ky, int kx) {
    if (m >= q.T) return -1;
    const uint32_t r = (uint32_t)(((unsigned long long)(uint32_t)m * q.mul_w) >> q.sh_w);
    const int ox = m - (int)r * q.Wout;
    const int b = (int)(((unsigned long long)r * q.mul_h) >> q.sh_h);
    const int oy = (int)r - b * q.Hout;
    const int iy = oy * q.stride + ky - 1, ix = ox * q.stride + kx - 1;
    if ((unsigned)iy >= (unsigned)q.Hin || (unsigned)ix >= (unsigned)q.Win) return -1;
    return ((long long)b * q.Hin + iy) * q.Win + ix;
}
// the source of a lane's chunk of token m: tap (ky, kx), channel ci (fixed per lane in the prologue)
__device__ __forceinline__ const uint16_t* conv_gather_src(const ConvGather& q, int m, int ky, int kx, int ci) {
    const long long p = conv_gather_pixel(q, m, ky, kx);
    return p < 0 ? (const uint16_t*)&g_zero_chunk : q.x + p * q.ldx + ci;
}

// ONE text (gemm_tn_body) for every tile shape.  A workgroup owns TN (n) x TK (k) of dW and walks the tokens in stages of TB; a
// stage holds each operand as images [TB][COLS] in the layout above (COLS * 2-byte rows, tn_swz<COLS>, tr_frag<COLS>).  Its four
// waves are WK along k (64 k columns = 4 fragments each) by WN along n (NF fragments each).
//   tile          | TN x TK      | TB | dY images      | X images       | in a buffer | (wk, wn) of wave w | NF      | edges | LDS
//   Tn128         | 128 x 128    | 64 | 1 x [64][128]  | 1 x [64][128]  | dY, X       | w >> 1, w & 1      | 4       | clamp | 64 KB
//   TnNarrow<TN>  | 64, 32 x 256 | 64 | 1 x [64][TN]   | 2 x [64][128]  | X, dY       | w, 0               | TN / 16 | live  | 80, 72 KB
//   TnWide        | 256 x 128    | 32 | 2 x [32][128]  | 1 x [32][128]  | dY, X       | w & 1, w >> 1      | 8       | live  | 48 KB
// Tn128: gemm_tn_kernel, every weight gradient unless a route says otherwise.
// TnNarrow (wgrad_route picks it; opt-in): few output channels - a workgroup keeps the 128 x 128 tile's 64
//   accumulators per lane only where dW has columns.
// TnWide (wgrad_wide_route picks it; opt-in): large dW - a workgroup moves 24 KB through the LDS-DMA path per
//   32 tokens where two 128 x 128 workgroups move 32 KB for the same MFMAs.  The swizzle and tr_frag's row mapping repeat every 32
//   rows, so a 32-token stage reads as step ks = 0 of a 64-token tile; a 64-token double buffer would be 96 KB (a ring of three
//   stages with a counted wait measured equal or slower).
// Edges.  Chunks past N / K are clamped to N - 8 / K - 8 (results of clamped columns are not stored).  "live" tiles besides give a
//   16-column fragment that lies wholly past N (or K) no DMA (its lanes are masked off the load: the LDS destination is
//   base + 16 * lane whatever the mask; nothing at all is issued for an image past the edge), no LDS read and no MFMA: a wave picks
//   the loop instance for its count of live k and n fragments once (wave-uniform), so the transposing reads run with every lane on
//   and the loop bodies have no branches (a wave with runtime guards around each read and MFMA holds the whole workgroup back at
//   the barrier: measured).  Tn128 always runs 4 x 4.
// Pipeline: two buffers; the DMA of stage s + 1 is issued before the MFMAs of stage s and drained (vmcnt(0)) at the stage's only
//   barrier.  ALTERNATE: the dY and X instructions of a stage are issued in turns (Tn128), otherwise dY first.
// Summation: the MFMA, tr_frag's token-to-slot mapping per 32 tokens, the ascending token walk and the slice boundaries (whole
//   64-token tiles, t0 = nt * slice / S) do not depend on the tile, so for an equal slice count every dW element is the same chain
//   of operations on the same values whatever the tile: bit-identical results (tests/golden/wgrad_bits.json pins them).
// GATHER: only the X side of the DMA changes; the ConvGather block is then the kernel's second argument.
template <int TN_, int TK_, int TB_>
struct TnShape {
    static constexpr int TN = TN_, TK = TK_, TB = TB_;
    static constexpr int YC = TN < 128 ? TN : 128, YS = TN / YC, XS = TK / 128;       // columns of a dY image; images of dY, of X
    static constexpr int YSUB = TB * YC * 2, XSUB = TB * 256;                        // bytes of an image
    static constexpr int YPI = YSUB / 4096, XPI = XSUB / 4096;                       // DMA instructions (1 KB) per wave and image
    static constexpr int BUF = YS * YSUB + XS * XSUB, LDS = 2 * BUF;                 // bytes of a buffer; dynamic LDS of the launch
    static constexpr int WK = TK / 64, WN = 4 / WK, NF = TN / WN / 16;
    static_assert(YS * YC == TN && XS * 128 == TK && (TB == 64 || TB == 32) && YPI >= 1 && WK * WN == 4 && NF * WN * 16 == TN, "tile");
};
struct Tn128 : TnShape<128, 128, 64> { static constexpr bool LIVE = false, K_OUTER = true, Y_FIRST = true, ALTERNATE = true; };
template <int TN>
struct TnNarrow : TnShape<TN, 256, 64> { static constexpr bool LIVE = true, K_OUTER = true, Y_FIRST = false, ALTERNATE = false; };
struct TnWide : TnShape<256, 128, 32> { static constexpr bool LIVE = true, K_OUTER = false, Y_FIRST = true, ALTERNATE = false; };

// DMA instruction j of an operand with images [TB][COLS], PI instructions per wave and image: lane -> row of the image
// (64 / CH rows per instruction, CH = COLS / 8 chunks per row) and first column of the operand tile; source chunk = chunk' ^ swz(row)
template <int COLS, int PI>
__device__ __forceinline__ void tn_dma_lane(int j, int wave, int lane, int& row, int& col) {
    constexpr int CH = COLS / 8;
    row = ((j % PI) * 4 + wave) * (64 / CH) + lane / CH;
    col = (j / PI) * COLS + (((lane % CH) ^ tn_swz<COLS>(row)) << 3);
}
// f(std::integral_constant<int, n>) for a runtime LO <= n <= HI
template <int LO, int HI, class F>
__device__ __forceinline__ void tn_dispatch(int n, F& f) {
    if constexpr (LO == HI) f(std::integral_constant<int, LO>{});
    else if (n >= HI) f(std::integral_constant<int, HI>{});
    else tn_dispatch<LO, HI - 1>(n, f);
}

template <class D, bool GATHER>
__device__ __forceinline__ void gemm_tn_body(const GemmArgs& g, const ConvGather& q) {
    // g.a0 = dY (T, N) ld lda0 ; g.w = X (T, K) ld lda1 ; T = g.K (multiple of 64) ; out (N, K) f32 ld ldo
    constexpr int TB = D::TB, NF = D::NF, YI = D::YS * D::YPI, XI = D::XS * D::XPI;   // YI, XI: DMA instructions of a wave per stage
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = D::LIVE ? __builtin_amdgcn_readfirstlane(tid >> 6) : tid >> 6;   // the dispatch below wants provably uniform counts
    const int Nw = g.M, Kw = g.N, T = g.K;
    int bid = blockIdx.x;
    const int S = g.splitk > 1 ? g.splitk : 1;
    const int slice = bid % S;
    bid /= S;
    const int tn_ = bid / g.tiles_n, tk_ = bid - tn_ * g.tiles_n;
    const int n0 = tn_ * D::TN, k0 = tk_ * D::TK;
    const int n_live = Nw - n0 < D::TN ? Nw - n0 : D::TN, k_live = Kw - k0 < D::TK ? Kw - k0 : D::TK;   // columns inside dW: > 0, multiples of 8
    const int wk = D::K_OUTER ? wave / D::WN : wave % D::WK, wn = D::K_OUTER ? wave % D::WN : wave / D::WK;
    int nnf = (n_live - wn * NF * 16 + 15) >> 4;              // live n fragments of this wave
    nnf = nnf < 0 ? 0 : nnf > NF ? NF : nnf;
    int nkf = (k_live - wk * 64 + 15) >> 4;                   // live k fragments of this wave
    nkf = nkf < 0 || nnf == 0 ? 0 : nkf > 4 ? 4 : nkf;        // a wave with no live fragment only feeds the DMA

    // DMA sources.  A lane whose source chunk lies in a dead fragment issues nothing (LIVE).
    const uint16_t* ysrc[YI];
    const uint16_t* xsrc[XI];
    int xtap[XI], xrow[XI];                                   // GATHER: in place of xsrc
    unsigned ylive = 0, xlive = 0;
#pragma unroll
    for (int j = 0; j < YI; ++j) {
        int row, c;
        tn_dma_lane<D::YC, D::YPI>(j, wave, lane, row, c);
        ylive |= (unsigned)((c & ~15) < n_live) << j;
        ysrc[j] = g.a0 + (long long)row * g.lda0 + n0 + (c < n_live ? c : n_live - 8);
    }
#pragma unroll
    for (int j = 0; j < XI; ++j) {
        int row, c;
        tn_dma_lane<128, D::XPI>(j, wave, lane, row, c);
        xlive |= (unsigned)((c & ~15) < k_live) << j;
        const int ck = k0 + (c < k_live ? c : k_live - 8);
        if constexpr (GATHER) {                               // the chunk's tap and channel: ky | kx << 2 | ci << 4
            const int tap = ck / q.Cin;
            xtap[j] = tap / 3 | (tap % 3) << 2 | (ck - tap * q.Cin) << 4;
            xrow[j] = row;
        } else {
            long long xoff = ck;
            if (g.seg_len) { const int sg = ck / g.seg_len; xoff = (long long)sg * g.seg_stride + (ck - sg * g.seg_len); }
            xsrc[j] = g.w + (long long)row * g.lda1 + xoff;
        }
    }
    auto ydma = [&](int s, unsigned char* Yt, int j) {
        if (D::LIVE && ((j / D::YPI) * D::YC >= n_live || !(ylive >> j & 1))) return;     // the first test is wave-uniform
        __builtin_amdgcn_global_load_lds((gptr_t)(ysrc[j] + (long long)s * TB * g.lda0),
                                         (lptr_t)(Yt + (j / D::YPI) * D::YSUB + ((j % D::YPI) * 4 + wave) * 1024), 16, 0, 0);
    };
    auto xdma = [&](int s, unsigned char* Xt, int j) {
        if (D::LIVE && ((j / D::XPI) * 128 >= k_live || !(xlive >> j & 1))) return;
        const uint16_t* xs;
        if constexpr (GATHER) xs = conv_gather_src(q, s * TB + xrow[j], xtap[j] & 3, xtap[j] >> 2 & 3, xtap[j] >> 4);
        else xs = xsrc[j] + (long long)s * TB * g.lda1;
        __builtin_amdgcn_global_load_lds((gptr_t)xs, (lptr_t)(Xt + (j / D::XPI) * D::XSUB + ((j % D::XPI) * 4 + wave) * 1024), 16, 0, 0);
    };
    constexpr int Y_AT = D::Y_FIRST ? 0 : D::XS * D::XSUB, X_AT = D::Y_FIRST ? D::YS * D::YSUB : 0;   // the operands inside a buffer
    auto issue = [&](int s, int buf) {
        unsigned char* Yt = smem + buf * D::BUF + Y_AT;
        unsigned char* Xt = smem + buf * D::BUF + X_AT;
        if constexpr (D::ALTERNATE) {
            static_assert(!D::ALTERNATE || YI == XI, "instructions in turns");
#pragma unroll
            for (int j = 0; j < YI; ++j) { ydma(s, Yt, j); xdma(s, Xt, j); }
        } else {
#pragma unroll
            for (int j = 0; j < YI; ++j) ydma(s, Yt, j);
#pragma unroll
            for (int j = 0; j < XI; ++j) xdma(s, Xt, j);
        }
    };
    f32x4 acc[4][NF];                                         // [k fragment][n fragment]
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < NF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int fi = lane & 15, mg = lane >> 4;
    const int nt_all = T / 64;                                // slices are whole 64-token tiles; stages of TB tokens
    const int s0 = 64 / TB * (int)((long long)nt_all * slice / S), s1 = 64 / TB * (int)((long long)nt_all * (slice + 1) / S);
    if (s0 < s1) {
        issue(s0, 0);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
    }
    // the token walk of a wave with NK live k fragments and NN live n fragments
    auto walk = [&](auto nk, auto nn) {
        constexpr int NK = decltype(nk)::value, NN = decltype(nn)::value;
        for (int s = s0; s < s1; ++s) {
            const int cur = (s - s0) & 1;
            if (s + 1 < s1) issue(s + 1, cur ^ 1);
            if constexpr (NK > 0) {
                const unsigned char* Yt = smem + cur * D::BUF + Y_AT + wn * NF * 16 / D::YC * D::YSUB;   // the wave's images
                const unsigned char* Xt = smem + cur * D::BUF + X_AT + wk * 64 / 128 * D::XSUB;
#pragma unroll
                for (int ks = 0; ks < TB / 32; ++ks) {
                    bf16x8 fx[NK], fy[NN];
#pragma unroll
                    for (int i = 0; i < NK; ++i) fx[i] = tr_frag(Xt, ks, lane, wk * 64 % 128 + i * 16);
#pragma unroll
                    for (int j = 0; j < NN; ++j) fy[j] = tr_frag<D::YC>(Yt, ks, lane, wn * NF * 16 % D::YC + j * 16);
#pragma unroll
                    for (int i = 0; i < NK; ++i)
#pragma unroll
                        for (int j = 0; j < NN; ++j)
                            acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fx[i], fy[j], acc[i][j], 0, 0, 0);
                }
            }
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __syncthreads();
        }
    };
    if constexpr (D::LIVE) {
        auto by_n = [&](auto nk) {
            if constexpr (decltype(nk)::value == 0) walk(nk, std::integral_constant<int, 1>{});
            else {
                auto with_n = [&](auto nn) { walk(nk, nn); };
                tn_dispatch<1, NF>(nnf, with_n);
            }
        };
        tn_dispatch<0, 4>(nkf, by_n);
    } else {
        walk(std::integral_constant<int, 4>{}, std::integral_constant<int, NF>{});
    }
    // D[row = k (lane>>4)*4 + reg][col = n (lane&15)]  ->  dW[n][k..k+3]
    float* out = S > 1 ? g.partial + (long long)slice * Nw * Kw : (float*)g.out;
    const long long ldo = S > 1 ? Kw : g.ldo;
#pragma unroll
    for (int j = 0; j < NF; ++j) {
        const int n = n0 + wn * NF * 16 + j * 16 + fi;
        if (n >= Nw) continue;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int k = k0 + wk * 64 + i * 16 + mg * 4;
            if (k < Kw) *(float4*)(out + (long long)n * ldo + k) = make_float4(acc[i][j][0], acc[i][j][1], acc[i][j][2], acc[i][j][3]);
        }
    }
}
__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(GemmArgs g) { gemm_tn_body<Tn128, false>(g, ConvGather{}); }
__global__ __launch_bounds__(256, 2) void gemm_tn_gather_kernel(GemmArgs g, ConvGather q) { gemm_tn_body<Tn128, true>(g, q); }
template <int TN>
__global__ __launch_bounds__(256, 2) void gemm_tn_narrow_kernel(GemmArgs g) { gemm_tn_body<TnNarrow<TN>, false>(g, ConvGather{}); }
template <int TN>
__global__ __launch_bounds__(256, 2) void gemm_tn_narrow_gather_kernel(GemmArgs g, ConvGather q) { gemm_tn_body<TnNarrow<TN>, true>(g, q); }
__global__ __launch_bounds__(256, 2) void gemm_tn_wide_kernel(GemmArgs g) { gemm_tn_body<TnWide, false>(g, ConvGather{}); }

// ---------------------------------------------------------------------------------------------
// Skinny-M linear (M <= 256: one row per crop - the classifier's last-block tail on the cls rows, and its head).  Such a product
// is a pass over the weight matrix (fc2 of ViT-B: 4.7 MB against 64 x 768 outputs); 128 x 128 tiles make 6 .. 24 workgroups of it,
// each walking the whole K range alone.  Here a workgroup owns 64 rows x 16 columns and its 8 waves each take one eighth of K
// (N / 16 workgroups per 64 rows: 48 .. 192 for the ViT-B shapes, every one with 8 independent load streams).  A wave reads its
// MFMA fragments straight from global memory (16 B per lane: 16 weight rows and 64 activation rows per 32-wide K step; no LDS
// stage, no barrier in the loop - nothing is reused inside a wave), four K steps of loads in flight at a time.
// The eight partial tiles meet in LDS and are added in slice order 0 .. 7, so the result does not depend on the launch; the
// epilogue (bias, GELU, f32 residual read-modify-write at any row stride, f32 / bf16 store, device-side row count) runs on the sums.
// Host: N % 16 == 0, K % 32 == 0, flags within BIAS | GELU | RES_F32 | OUT_F32.
// ---------------------------------------------------------------------------------------------
int g_opt_skinny = 256;             // largest M taken by gemm_skinny_kernel ("linear_skinny"; 0 = off)

__global__ __launch_bounds__(512) void gemm_skinny_kernel(GemmArgs g) {
    constexpr int NW = 8, MF = 4;
    __shared__ f32x4 red[NW][MF][64];                          // 32 KB
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int fr = lane & 15, fq = lane >> 4;
    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    const int tm = blockIdx.x / g.tiles_n, tn = blockIdx.x - tm * g.tiles_n;
    const int m0 = tm * (16 * MF), n0 = tn * 16;
    if (m0 >= M) return;

    const int nk = g.K >> 5;
    const int k0 = (int)((long long)nk * wave / NW), k1 = (int)((long long)nk * (wave + 1) / NW);
    const uint16_t* wp = g.w + (long long)(n0 + fr) * g.K + fq * 8;
    const uint16_t* ap[MF];
#pragma unroll
    for (int j = 0; j < MF; ++j) {
        int m = m0 + j * 16 + fr;
        m = m < g.M ? m : g.M - 1;                              // rows past the end: the last row, never stored
        ap[j] = g.a0 + (long long)m * g.lda0 + fq * 8;
    }
    f32x4 acc[MF];
#pragma unroll
    for (int j = 0; j < MF; ++j) acc[j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    // U K steps per trip: all their loads are issued before the first MFMA waits, so a wave's 3 (K = 768) .. 12 (K = 3072) steps
    // cost one to three memory round trips instead of one each (this kernel is bound by latency, not by bytes)
    constexpr int U = 4;
    for (int k = k0; k < k1; k += U) {
        bf16x8 fw[U], fa[U][MF];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int kk = k + u < k1 ? k + u : k1 - 1;         // past the slice: a repeated (cached) load, its MFMAs skipped
            fw[u] = *(const bf16x8*)(wp + kk * 32);
#pragma unroll
            for (int j = 0; j < MF; ++j) fa[u][j] = *(const bf16x8*)(ap[j] + kk * 32);
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (k + u < k1) {
#pragma unroll
                for (int j = 0; j < MF; ++j) acc[j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[u], fa[u][j], acc[j], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < MF; ++j) red[wave][j][lane] = acc[j];
    __syncthreads();
    if (tid >= MF * 64) return;
    const int j = tid >> 6;
    f32x4 s = red[0][j][lane];
#pragma unroll
    for (int w = 1; w < NW; ++w) s += red[w][j][lane];
    const int m = m0 + j * 16 + fr, n = n0 + fq * 4;          // lane owns columns n .. n + 3 of row m
    if (m >= M) return;
    const int flags = g.flags;
    float v[4] = {s[0], s[1], s[2], s[3]};
    if (flags & YV_EPI_BIAS) {
        const float4 b = *(const float4*)(g.bias + n);
        v[0] += b.x; v[1] += b.y; v[2] += b.z; v[3] += b.w;
    }
    if (flags & YV_EPI_GELU) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = gelu_f(v[q]);
    }
    if (flags & (YV_EPI_OUT_F32 | YV_EPI_RES_F32)) {
        float* o = (float*)g.out + (long long)m * g.ldo + n;
        if (flags & YV_EPI_RES_F32) {
            const float4 x = *(const float4*)o;
            v[0] += x.x; v[1] += x.y; v[2] += x.z; v[3] += x.w;
        }
        *(float4*)o = make_float4(v[0], v[1], v[2], v[3]);
    } else {
        uint16_t* o = (uint16_t*)g.out + (long long)m * g.ldo + n;
        *(uint2*)o = make_uint2(pack_bf16x2(v[0], v[1]), pack_bf16x2(v[2], v[3]));
    }
}

int launch_skinny(GemmArgs& g, hipStream_t st) {
    g.tiles_m = (g.M + 63) / 64;
    g.tiles_n = g.N >> 4;
    launch_timed(gemm_skinny_kernel, g.tiles_m * g.tiles_n, 512, 0, st, g);
    return yv_launch_status();
}

// ---------------------------------------------------------------------------------------------
// Mid-M linear (256 < M <= "linear_mid": the classifier at the handful of crops one request carries).  128 x 128 tiles make
// 42 .. 168 workgroups of the ViT-B products at 788 rows, each walking all of K alone; the skinny kernel's global fragment reads
// fetch A once per 16 columns.  Here a workgroup owns 64 x 64 outputs (four times the workgroups) and splits K inside itself: its
// 8 waves are two K halves x (2 x 2 waves of 32 x 32), half h taking the 64-deep K steps h, h + 2, ...  Each half stages its own
// steps by LDS-DMA (the 128-byte rows, source-side chunk swizzle and fragment reads of gemm_dma_kernel) into its own two-stage
// ring: 2 halves x 2 stages x (64 + 64) rows x 128 B = 64 KB, two workgroups per CU.  One barrier per pair of K steps, shared
// by the halves; with an odd step count half 1 idles through the last one.
// The two partial tiles meet in LDS, overlaying the rings after the last step: each half hands the other the 16-row fragments it
// does not finish (half 0 keeps rows 0 .. 15 of every wave tile, half 1 rows 16 .. 31), the sum is half 0 + half 1 in that order
// on both sides, and all 8 waves run gemm_dma_kernel's direct epilogue on the sums.  One launch, no workspace, no atomics.
// Host: N % 64 == 0, K % 64 == 0, flags within BIAS | GELU | RES_F32 | OUT_F32.
// ---------------------------------------------------------------------------------------------
int g_opt_mid = 0;                  // largest M taken by gemm_mid_kernel ("linear_mid"; 0 = off)
constexpr int MID_FLOOR = 256;      // ... and the M it starts above, whatever "linear_skinny" says
int g_opt_mid_fill = 5;             // ... where 128 x 128 tiles number at most this many eighths of the CU count ("linear_mid_fill";
                                    // tools/mid_gemm_bench.py raises it to time the kernel on the shapes the rule leaves out)

__global__ __launch_bounds__(512, 2) void gemm_mid_kernel(GemmArgs g) {
    constexpr int BM = 64, BN = 64, MF = 2, NF = 2;
    constexpr int STAGE = (BM + BN) * 128, RING = 2 * STAGE;    // bytes: one K step of a half, a half's two stages
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = wave >> 2, w4 = wave & 3;

    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    {
        const int GM = g.group_m, per = GM * g.tiles_n;
        const int grp = bid / per, first = grp * GM;
        const int gsz = (g.tiles_m - first) < GM ? (g.tiles_m - first) : GM;
        const int in = bid - grp * per;
        tm = first + in % gsz;
        tn = in / gsz;
    }
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    // a half's four waves fill its stage: 8 rows x 128 B per wave-instruction, 2 for A and 2 for W per wave
    const int lrow = lane >> 3, lch = lane & 7;
    const uint16_t* a_src[2];
    const uint16_t* w_src[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (j * 4 + w4) * 8 + lrow;
        int m = m0 + r;
        m = m < g.M ? m : g.M - 1;                              // rows past the end: the last row, never stored
        a_src[j] = g.a0 + (long long)m * g.lda0 + ((lch ^ (r & 7)) << 3);
        w_src[j] = g.w + (long long)(n0 + r) * g.K + ((lch ^ (r & 7)) << 3);
    }
    unsigned char* const ring = smem + half * RING;
    auto issue = [&](int kt, int buf) {
        unsigned char* A = ring + buf * STAGE;
        unsigned char* W = A + BM * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(a_src[j] + kt * BK), (lptr_t)(A + (j * 4 + w4) * 1024), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(w_src[j] + kt * BK), (lptr_t)(W + (j * 4 + w4) * 1024), 16, 0, 0);
    };

    f32x4 acc[NF][MF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wrow_m = (w4 >> 1) * 32, wrow_n = (w4 & 1) * 32;
    const int fr = lane & 15, fq = lane >> 4;

    const int nk = g.K / BK, trips = (nk + 1) >> 1;             // trip t: K step 2 t + half (half 1 may lack the last one)
    if (half < nk) issue(half, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < trips; ++t) {
        const int cur = t & 1, kt = 2 * t + half;
        if (kt + 2 < nk) issue(kt + 2, cur ^ 1);
        if (kt < nk) {
            const unsigned char* A = ring + cur * STAGE;
            const unsigned char* W = A + BM * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[MF], fw[NF];
                const int kc = ks * 4 + fq;
#pragma unroll
                for (int j = 0; j < MF; ++j) {
                    const int rr = wrow_m + j * 16 + fr;
                    fa[j] = *(const bf16x8*)(A + rr * 128 + ((kc ^ (rr & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    const int rr = wrow_n + i * 16 + fr;
                    fw[i] = *(const bf16x8*)(W + rr * 128 + ((kc ^ (rr & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < NF; ++i)
#pragma unroll
                    for (int j = 0; j < MF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fa[j], acc[i][j], 0, 0, 0);
            }
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                        // (the last one: every fragment read is done, the rings are free)
    }
    // exchange: xch[half][w4][i][lane] holds the fragments (i, 1 - half) of that wave, which the OTHER half finishes
    f32x4* const xch = (f32x4*)smem;
#pragma unroll
    for (int i = 0; i < NF; ++i) xch[((half * 4 + w4) * NF + i) * 64 + lane] = half ? acc[i][0] : acc[i][1];
    __syncthreads();
    f32x4 sum[NF][1];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const f32x4 other = xch[(((1 - half) * 4 + w4) * NF + i) * 64 + lane];
        sum[i][0] = half ? other + acc[i][1] : acc[i][0] + other;           // half 0 + half 1
    }
    epilogue<1, NF>(g, sum, M, m0, n0, wrow_m + half * 16, wrow_n, fr, fq);
}

int launch_mid(GemmArgs& g, hipStream_t st) {
    g.tiles_m = (g.M + 63) / 64;
    g.tiles_n = g.N >> 6;
    const size_t lds = 2 * 2 * (size_t)(64 + 64) * 128;
    if (!yv_grant_lds((const void*)gemm_mid_kernel, lds)) return YV_ERR_LAUNCH;
    launch_timed(gemm_mid_kernel, g.tiles_m * g.tiles_n, 512, lds, st, g);
    return yv_launch_status();
}

// ---------------------------------------------------------------------------------------------
// Mid-M MXFP8 linear (1 <= M <= "linear_mx_mid": the mxfp8 classifier at the handful of crops one request carries; DESIGN.md
// section 38).  gemm_mid_kernel's organisation on gemm_mx_kernel's operands: a workgroup owns 64 x 64 outputs, its 8 waves are two
// K groups x (2 x 2 waves of 32 x 32), group h taking the 128-element K steps h, h + 2, ...  Each group fills its own two-stage ring
// by LDS-DMA: per stage 64 A rows and 64 W rows of 128 B (gemm_mx_kernel's source-side chunk swizzle, its fragment reads of chunks
// fq and 4 + fq) and the tile's 128 scale dwords of that K step (A's 64, then W's 64; one wave-instruction of the group's first
// wave, whose upper 32 lanes re-fetch a valid address into the slack of the 1 KB slot so that exec stays full).
// 2 groups x 2 stages x (16 KB + 1 KB) = 68 KB, two workgroups per CU.  One vmcnt(0) + barrier per trip, shared by the groups;
// with an odd step count group 1 idles through the last trip, with K = 128 it adds zeros.
// Exchange and sum as in gemm_mid_kernel (group 0 + group 1 on both sides, over the rings after the last barrier), then every wave
// finishes a 16-row x 32-column piece: the direct epilogue, or - YV_EPI_OUT_MXFP8 - the piece IS one MX block per row, held by the
// lanes fr, fr + 16, fr + 32, fr + 48: value (bias, GELU), bf16 rounding, mx_quant_piece16x32, the e4m3 bytes and one scale byte.
// Host: N % 64 == 0, K % 128 == 0, flags within BIAS | GELU | RES_F32 | OUT_F32 | OUT_MXFP8, no separate residual source.
// ---------------------------------------------------------------------------------------------
int g_opt_mx_mid = 0;               // largest M taken by gemm_mx_mid_kernel ("linear_mx_mid"; 0 = off)
int g_opt_mx_mid_fill = 5;          // ... where 128 x 128 tiles number at most this many eighths of the CU count ("linear_mx_mid_fill";
                                    // measured: up to 150 tiles x 0.46 - 0.92 of the 128 x 128 route's time, at 168 x 0.84 - 1.02, beyond slower)

__global__ __launch_bounds__(512, 2) void gemm_mx_mid_kernel(MxArgs a) {
    const GemmArgs& g = a.g;
    constexpr int BM = 64, BN = 64, MF = 2, NF = 2;
    constexpr int A_BYTES = BM * 128, W_BYTES = BN * 128, S_BYTES = 1024;   // (scales: 512 B + the slack of the DMA's upper lanes)
    constexpr int STAGE = A_BYTES + W_BYTES + S_BYTES, RING = 2 * STAGE;    // bytes: one K step of a group, a group's two stages
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = wave >> 2, w4 = wave & 3;

    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    {
        const int GM = g.group_m, per = GM * g.tiles_n;
        const int grp = bid / per, first = grp * GM;
        const int gsz = (g.tiles_m - first) < GM ? (g.tiles_m - first) : GM;
        const int in = bid - grp * per;
        tm = first + in % gsz;
        tn = in / gsz;
    }
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    // a group's four waves fill its stage: 8 rows x 128 B per wave-instruction, 2 for A and 2 for W per wave
    const int lrow = lane >> 3, lch = lane & 7;
    const uint8_t* a_src[2];
    const uint8_t* w_src[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (j * 4 + w4) * 8 + lrow;
        int m = m0 + r;
        m = m < g.M ? m : g.M - 1;                              // rows past the end: the last row, never stored
        a_src[j] = (const uint8_t*)g.a0 + (long long)m * g.lda0 + ((lch ^ (r & 7)) << 4);
        w_src[j] = (const uint8_t*)g.w + (long long)(n0 + r) * g.K + ((lch ^ (r & 7)) << 4);
    }
    // scale DMA (the group's wave 0): lane l < 32 fetches the dwords 4 l .. 4 l + 3 of the tile's 64 A + 64 W scale dwords
    const int s_dw = lane * 4;
    const bool s_on = s_dw < BM + BN;
    const uint8_t* const s_src = s_dw < BM ? a.sa + ((long long)m0 + s_dw) * 4 : a.sw + ((long long)n0 + (s_on ? s_dw - BM : 0)) * 4;
    const long long s_step = (s_dw < BM ? a.rows_a : a.rows_w) * 4;
    unsigned char* const ring = smem + half * RING;
    auto issue = [&](int kt, int buf) {
        unsigned char* A = ring + buf * STAGE;
        unsigned char* W = A + A_BYTES;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(a_src[j] + kt * 128), (lptr_t)(A + (j * 4 + w4) * 1024), 16, 0, 0);
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(w_src[j] + kt * 128), (lptr_t)(W + (j * 4 + w4) * 1024), 16, 0, 0);
        if (w4 == 0)        // (lanes past the 128 dwords re-fetch the first W dwords into their unused slot: exec stays full)
            __builtin_amdgcn_global_load_lds((gptr_t)(s_src + kt * s_step), (lptr_t)(W + W_BYTES), 16, 0, 0);
    };

    f32x4 acc[NF][MF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wrow_m = (w4 >> 1) * 32, wrow_n = (w4 & 1) * 32;
    const int fr = lane & 15, fq = lane >> 4;

    const int nk = g.K >> 7, trips = (nk + 1) >> 1;             // trip t: K step 2 t + half (group 1 may lack the last one)
    if (half < nk) issue(half, 0);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < trips; ++t) {
        const int cur = t & 1, kt = 2 * t + half;
        if (kt + 2 < nk) issue(kt + 2, cur ^ 1);
        if (kt < nk) {
            const unsigned char* A = ring + cur * STAGE;
            const unsigned char* W = A + A_BYTES;
            const unsigned char* S = W + W_BYTES;
            i32x8 fa[MF], fw[NF];
            int sca[MF], scw[NF];
#pragma unroll
            for (int j = 0; j < MF; ++j) {
                const int rr = wrow_m + j * 16 + fr;
                const u32x4 lo = *(const u32x4*)(A + rr * 128 + (((fq) ^ (rr & 7)) << 4));
                const u32x4 hi = *(const u32x4*)(A + rr * 128 + (((4 + fq) ^ (rr & 7)) << 4));
                fa[j] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                sca[j] = (int)(*(const uint32_t*)(S + rr * 4) >> (8 * fq));              // byte 0 = scale of block fq
            }
#pragma unroll
            for (int i = 0; i < NF; ++i) {
                const int rr = wrow_n + i * 16 + fr;
                const u32x4 lo = *(const u32x4*)(W + rr * 128 + (((fq) ^ (rr & 7)) << 4));
                const u32x4 hi = *(const u32x4*)(W + rr * 128 + (((4 + fq) ^ (rr & 7)) << 4));
                fw[i] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                scw[i] = (int)(*(const uint32_t*)(S + BM * 4 + rr * 4) >> (8 * fq));
            }
#pragma unroll
            for (int i = 0; i < NF; ++i)
#pragma unroll
                for (int j = 0; j < MF; ++j)
                    acc[i][j] = __builtin_amdgcn_mfma_scale_f32_16x16x128_f8f6f4(fw[i], fa[j], acc[i][j], 0, 0, 0, scw[i], 0, sca[j]);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                        // (the last one: every fragment read is done, the rings are free)
    }
    // exchange: xch[half][w4][i][lane] holds the fragments (i, 1 - half) of that wave, which the OTHER group finishes
    f32x4* const xch = (f32x4*)smem;
#pragma unroll
    for (int i = 0; i < NF; ++i) xch[((half * 4 + w4) * NF + i) * 64 + lane] = half ? acc[i][0] : acc[i][1];
    __syncthreads();
    f32x4 sum[NF][1];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const f32x4 other = xch[(((1 - half) * 4 + w4) * NF + i) * 64 + lane];
        sum[i][0] = half ? other + acc[i][1] : acc[i][0] + other;           // group 0 + group 1
    }
    if (!(g.flags & YV_EPI_OUT_MXFP8)) {
        epilogue<1, NF>(g, sum, M, m0, n0, wrow_m + half * 16, wrow_n, fr, fq);
        return;
    }
    // the fc1 -> fc2 hand-over: this lane holds columns fq * 4 .. + 3 and 16 + fq * 4 .. + 3 of the block nb .. nb + 31 of row m
    const int m = m0 + wrow_m + half * 16 + fr, nb = n0 + wrow_n;
    float v[8];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const int n = nb + i * 16 + fq * 4;
        float4 b = make_float4(0.f, 0.f, 0.f, 0.f);
        if (g.flags & YV_EPI_BIAS) b = *(const float4*)(g.bias + n);
        float u[4] = {sum[i][0][0] + b.x, sum[i][0][1] + b.y, sum[i][0][2] + b.z, sum[i][0][3] + b.w};
        if (g.flags & YV_EPI_GELU) {
#pragma unroll
            for (int q = 0; q < 4; ++q) u[q] = gelu_f(u[q]);
        }
        const uint32_t p0 = pack_bf16x2(u[0], u[1]), p1 = pack_bf16x2(u[2], u[3]);      // the bf16 value the staged epilogue quantises
        v[i * 4] = bf16_to_f32((uint16_t)(p0 & 0xffff)); v[i * 4 + 1] = bf16_to_f32((uint16_t)(p0 >> 16));
        v[i * 4 + 2] = bf16_to_f32((uint16_t)(p1 & 0xffff)); v[i * 4 + 3] = bf16_to_f32((uint16_t)(p1 >> 16));
    }
    uint32_t q8[2];
    const int e = mx_quant_piece16x32(v, q8);                   // (every lane: rows past M quantise the clamped row, store nothing)
    if (m >= M) return;
    uint8_t* const o = g.mxq + (long long)m * g.ldmxq + nb + fq * 4;
    *(uint32_t*)o = q8[0];
    *(uint32_t*)(o + 16) = q8[1];
    if (fq == 0) g.mxs[mx_scale_kmajor(nb >> 5, g.mx_rows, m)] = (uint8_t)(e + 127);
}

int launch_mx_mid(MxArgs& a, hipStream_t st) {
    GemmArgs& g = a.g;
    g.tiles_m = (g.M + 63) / 64;
    g.tiles_n = g.N >> 6;
    const size_t lds = 2 * 2 * (size_t)((64 + 64) * 128 + 1024);
    if (!yv_grant_lds((const void*)gemm_mx_mid_kernel, lds)) return YV_ERR_LAUNCH;
    launch_timed(gemm_mx_mid_kernel, g.tiles_m * g.tiles_n, 512, lds, st, a);
    return yv_launch_status();
}

// ---------------------------------------------------------------------------------------------
// gemm_mid_kernel with the LayerNorm that feeds it as a prologue ("linear_ln_mid": norm1 -> qkv and norm2 -> fc1 of the classifier
// at a handful of crops).  The A operand is the f32 residual stream x (M, K <= 1024): a 64 x 64 tile walks
// the whole row of its 64 input rows anyway, so it computes their statistics itself and normalises while it stages them, and the
// LayerNorm launch in front of the GEMM goes away.
//   statistics  wave w plays layernorm_kernel's wave for rows 8 w .. 8 w + 7 of the tile: lane l adds float4 chunks l, l + 64, ...
//               as (x + y) + (z + w), wave_sum, the second pass over v - mean in the same form (the summation-order contract at the
//               top of vit_misc.hip).  mean / rstd of the 64 rows and gamma / beta go to LDS behind the rings.  The first weight
//               step is on its way by LDS-DMA while this runs.
//   A staging   per K step of a half its four waves load the 64 x 64 f32 sub-tile into registers (two (row, 8-element) units per
//               lane), form (v - mean) * rstd * g + b in layernorm_kernel's expression order, pack to bf16 and write the 16-byte
//               chunk where gemm_mid_kernel's LDS-DMA would have put it: fragment reads, MFMA chain, exchange and epilogue are
//               that kernel's text, and so are the result's bits.  Step kt + 2 is loaded before the MFMAs of step kt and
//               converted after them, in front of the trip's wait and barrier.
// W stays on LDS-DMA.  LDS: 64 KB of rings + 2 x 4 KB gamma / beta + 512 B statistics = 72.5 KB, two workgroups per CU.
// The LayerNorm operands travel in a second argument block: GemmArgs keeps its layout (and every kernel its hidden arguments).
// ---------------------------------------------------------------------------------------------
int g_opt_ln_mid = 0;               // largest M the fused LayerNorm + linear takes ("linear_ln_mid"; 0 = the step does not exist)
int g_opt_ln_mid_fill = 0;          // ... where 128 x 128 tiles number at most this many eighths of the CU count ("linear_ln_fill").
                                    // 0: nowhere - the fused launch measured x 1.5 - 4.2 of the pair's time at every shape
                                    // (profiles/ln_mid_kernels.txt); tools/ln_mid_bench.py and the tests raise it
constexpr int LN_MID_MAXK = 1024;   // layernorm_kernel's LN_MAXC float4 chunks per lane

struct LnOps { const float* x; long long ldx; const float* gamma; const float* beta; float eps; };

__global__ __launch_bounds__(512, 2) void gemm_mid_ln_kernel(GemmArgs g, LnOps p) {
    constexpr int BM = 64, BN = 64, MF = 2, NF = 2;
    constexpr int STAGE = (BM + BN) * 128, RING = 2 * STAGE;    // bytes: one K step of a half, a half's two stages
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    float* const s_gamma = (float*)(smem + 2 * RING);
    float* const s_beta = s_gamma + LN_MID_MAXK;
    float* const s_mean = s_beta + LN_MID_MAXK;
    float* const s_rstd = s_mean + BM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int half = wave >> 2, w4 = wave & 3;

    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    const int bid = xcd_remap(blockIdx.x, gridDim.x);
    int tm, tn;
    {
        const int GM = g.group_m, per = GM * g.tiles_n;
        const int grp = bid / per, first = grp * GM;
        const int gsz = (g.tiles_m - first) < GM ? (g.tiles_m - first) : GM;
        const int in = bid - grp * per;
        tm = first + in % gsz;
        tn = in / gsz;
    }
    const int m0 = tm * BM, n0 = tn * BN;
    if (m0 >= M) return;

    // a half's four waves fill its stage: W by LDS-DMA (8 rows x 128 B per wave-instruction, 2 per wave), A through registers
    // (lane = row lrow of the same 8-row group, 8-element chunk lch of the K step)
    const int lrow = lane >> 3, lch = lane & 7;
    const float* x_src[2];
    const uint16_t* w_src[2];
    int a_dst[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (j * 4 + w4) * 8 + lrow;
        int m = m0 + r;
        m = m < g.M ? m : g.M - 1;                              // rows past the end: the last row, never stored
        x_src[j] = p.x + (long long)m * p.ldx + (lch << 3);
        w_src[j] = g.w + (long long)(n0 + r) * g.K + ((lch ^ (r & 7)) << 3);
        a_dst[j] = r * 128 + ((lch ^ (r & 7)) << 4);
    }
    unsigned char* const ring = smem + half * RING;
    auto issue_w = [&](int kt, int buf) {
        unsigned char* W = ring + buf * STAGE + BM * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_global_load_lds((gptr_t)(w_src[j] + kt * BK), (lptr_t)(W + (j * 4 + w4) * 1024), 16, 0, 0);
    };

    const int nk = g.K / BK, trips = (nk + 1) >> 1;             // trip t: K step 2 t + half (half 1 may lack the last one)
    if (half < nk) issue_w(half, 0);

    // ---- prologue: gamma / beta to LDS, statistics of the tile's 64 rows ----
    const int D = g.K, nch = D >> 2;
    if (tid < nch) {
        ((float4*)s_gamma)[tid] = ((const float4*)p.gamma)[tid];
        ((float4*)s_beta)[tid] = ((const float4*)p.beta)[tid];
    }
    for (int r4 = 0; r4 < 8; r4 += 4) {                          // four rows' loads in flight at a time
        float4 v[4][4];
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            int m = m0 + wave * 8 + r4 + rr;
            m = m < g.M ? m : g.M - 1;
            const float* xr = p.x + (long long)m * p.ldx;
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const int c = lane + 64 * i;
                v[rr][i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (c < nch) v[rr][i] = ((const float4*)xr)[c];
            }
        }
#pragma unroll
        for (int rr = 0; rr < 4; ++rr) {
            float s = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (lane + 64 * i < nch) s += (v[rr][i].x + v[rr][i].y) + (v[rr][i].z + v[rr][i].w);
            const float mean = wave_sum(s) / (float)D;
            float q = 0.f;
#pragma unroll
            for (int i = 0; i < 4; ++i)
                if (lane + 64 * i < nch) {
                    const float a = v[rr][i].x - mean, b = v[rr][i].y - mean, cc = v[rr][i].z - mean, d = v[rr][i].w - mean;
                    q += (a * a + b * b) + (cc * cc + d * d);
                }
            const float rstd = 1.0f / sqrtf(wave_sum(q) / (float)D + p.eps);
            if (lane == 0) { s_mean[wave * 8 + r4 + rr] = mean; s_rstd[wave * 8 + r4 + rr] = rstd; }
        }
    }
    __syncthreads();
    float mean[2], rstd[2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int r = (j * 4 + w4) * 8 + lrow;
        mean[j] = s_mean[r]; rstd[j] = s_rstd[r];
    }

    float4 xa[2][2];                                            // the K step in flight: [unit][low / high four elements]
    auto load_a = [&](int kt) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            xa[j][0] = *(const float4*)(x_src[j] + kt * BK);
            xa[j][1] = *(const float4*)(x_src[j] + kt * BK + 4);
        }
    };
    auto store_a = [&](int kt, int buf) {
        unsigned char* A = ring + buf * STAGE;
        const int k = kt * BK + (lch << 3);
        const float4 g0 = *(const float4*)(s_gamma + k), g1 = *(const float4*)(s_gamma + k + 4);
        const float4 b0 = *(const float4*)(s_beta + k), b1 = *(const float4*)(s_beta + k + 4);
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float mu = mean[j], rs = rstd[j];
            const float o0 = (xa[j][0].x - mu) * rs * g0.x + b0.x, o1 = (xa[j][0].y - mu) * rs * g0.y + b0.y;
            const float o2 = (xa[j][0].z - mu) * rs * g0.z + b0.z, o3 = (xa[j][0].w - mu) * rs * g0.w + b0.w;
            const float o4 = (xa[j][1].x - mu) * rs * g1.x + b1.x, o5 = (xa[j][1].y - mu) * rs * g1.y + b1.y;
            const float o6 = (xa[j][1].z - mu) * rs * g1.z + b1.z, o7 = (xa[j][1].w - mu) * rs * g1.w + b1.w;
            *(uint4*)(A + a_dst[j]) = make_uint4(pack_bf16x2(o0, o1), pack_bf16x2(o2, o3), pack_bf16x2(o4, o5), pack_bf16x2(o6, o7));
        }
    };

    f32x4 acc[NF][MF];
#pragma unroll
    for (int i = 0; i < NF; ++i)
#pragma unroll
        for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
    const int wrow_m = (w4 >> 1) * 32, wrow_n = (w4 & 1) * 32;
    const int fr = lane & 15, fq = lane >> 4;

    if (half < nk) { load_a(half); store_a(half, 0); }
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    for (int t = 0; t < trips; ++t) {
        const int cur = t & 1, kt = 2 * t + half;
        const bool more = kt + 2 < nk;
        if (more) { issue_w(kt + 2, cur ^ 1); load_a(kt + 2); }
        if (kt < nk) {
            const unsigned char* A = ring + cur * STAGE;
            const unsigned char* W = A + BM * 128;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) {
                bf16x8 fa[MF], fw[NF];
                const int kc = ks * 4 + fq;
#pragma unroll
                for (int j = 0; j < MF; ++j) {
                    const int rr = wrow_m + j * 16 + fr;
                    fa[j] = *(const bf16x8*)(A + rr * 128 + ((kc ^ (rr & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < NF; ++i) {
                    const int rr = wrow_n + i * 16 + fr;
                    fw[i] = *(const bf16x8*)(W + rr * 128 + ((kc ^ (rr & 7)) << 4));
                }
#pragma unroll
                for (int i = 0; i < NF; ++i)
#pragma unroll
                    for (int j = 0; j < MF; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i], fa[j], acc[i][j], 0, 0, 0);
            }
        }
        if (more) store_a(kt + 2, cur ^ 1);
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();                                        // (the last one: every fragment read is done, the rings are free)
    }
    // exchange: xch[half][w4][i][lane] holds the fragments (i, 1 - half) of that wave, which the OTHER half finishes
    f32x4* const xch = (f32x4*)smem;
#pragma unroll
    for (int i = 0; i < NF; ++i) xch[((half * 4 + w4) * NF + i) * 64 + lane] = half ? acc[i][0] : acc[i][1];
    __syncthreads();
    f32x4 sum[NF][1];
#pragma unroll
    for (int i = 0; i < NF; ++i) {
        const f32x4 other = xch[(((1 - half) * 4 + w4) * NF + i) * 64 + lane];
        sum[i][0] = half ? other + acc[i][1] : acc[i][0] + other;           // half 0 + half 1
    }
    epilogue<1, NF>(g, sum, M, m0, n0, wrow_m + half * 16, wrow_n, fr, fq);
}

int launch_mid_ln(GemmArgs& g, const LnOps& p, hipStream_t st) {
    g.tiles_m = (g.M + 63) / 64;
    g.tiles_n = g.N >> 6;
    const size_t lds = 2 * 2 * (size_t)(64 + 64) * 128 + 2 * LN_MID_MAXK * sizeof(float) + 2 * 64 * sizeof(float);
    if (!yv_grant_lds((const void*)gemm_mid_ln_kernel, lds)) return YV_ERR_LAUNCH;
    const dim3 grid(g.tiles_m * g.tiles_n), block(512);
    if (t_time_start || t_time_stop) {                          // (launch_timed, for a kernel of two argument blocks)
        hipExtLaunchKernelGGL(gemm_mid_ln_kernel, grid, block, (uint32_t)lds, st, t_time_start, t_time_stop, 0, g, p);
        t_time_start = t_time_stop = nullptr;
    } else {
        hipLaunchKernelGGL(gemm_mid_ln_kernel, grid, block, lds, st, g, p);
    }
    return yv_launch_status();
}

// The route of yv_linear_ln: ONE rule for its launch and for yv_linear_ln_route.  Pure: shape, flags and options in.  Fused where the
// step exists ("linear_ln_mid" > 0) and the shape is one gemm_mid_ln_kernel takes - MID_FLOOR < M <= "linear_ln_mid", whole 64-wide
// tiles and K steps, K within layernorm_kernel's bound, the epilogues of a qkv / fc1 product - and 128 x 128 tiles would number at
// most "linear_ln_fill" eighths of the CU count; everywhere else the pair yv_layernorm + yv_linear.
bool linear_ln_fused(int M, int N, int K, int flags, int n_cu) {
    if (g_opt_variant != 1 || g_opt_ln_mid <= 0 || M <= MID_FLOOR || M > g_opt_ln_mid) return false;
    if ((N & 63) || (K & 63) || K > LN_MID_MAXK || (flags & ~(YV_EPI_BIAS | YV_EPI_GELU | YV_EPI_OUT_F32))) return false;
    const long long tiles128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
    return tiles128 * 8 <= (long long)g_opt_ln_mid_fill * n_cu;
}

template <int BM, int BN, int WM, int WN, int ABL = 0, bool WT = false>
int launch_dma(GemmArgs& g, hipStream_t st) {
    g.tiles_m = (g.M + BM - 1) / BM;
    g.tiles_n = (g.N + BN - 1) / BN;
    const size_t lds = 2 * (size_t)(BM + BN) * 128;
    auto kern = gemm_dma_kernel<BM, BN, WM, WN, ABL, WT>;
    if (!yv_grant_lds((const void*)kern, lds)) return YV_ERR_LAUNCH;
    const int S = g.splitk > 1 ? g.splitk : 1;
    launch_timed(kern, g.tiles_m * g.tiles_n * S, WM * WN * 64, lds, st, g);
    return launch_splitk_reduce(g, st);
}

// What every tiled convolution launch does first: g's tile counts for BM x BN tiles and the grant of kern's dynamic LDS ...
bool tiles_and_lds(void (*kern)(GemmArgs), GemmArgs& g, int BM, int BN, size_t lds) {
    g.tiles_m = (g.M + BM - 1) / BM;
    g.tiles_n = (g.N + BN - 1) / BN;
    return yv_grant_lds((const void*)kern, lds);
}
// ... and the launch of one workgroup per tile (timed where yv_set_launch_timing armed events: the tools/conv_*_bench.py)
int launch_tiles(void (*kern)(GemmArgs), GemmArgs& g, int BM, int BN, int threads, size_t lds, hipStream_t st) {
    if (!tiles_and_lds(kern, g, BM, BN, lds)) return YV_ERR_LAUNCH;
    launch_timed(kern, g.tiles_m * g.tiles_n, threads, lds, st, g);
    return yv_launch_status();
}

template <int MODE, int BM, int BN, int WM, int WN>
int launch(GemmArgs& g, hipStream_t st) {
    size_t lds = (size_t)(BM + BN) * 128;
    if (lds < (size_t)THREADS / 64 * (BM / WM) * 128) lds = (size_t)THREADS / 64 * (BM / WM) * 128;   // the staged epilogue's slabs
    void (*kern)(GemmArgs) = igemm_kernel<MODE, BM, BN, WM, WN, false>;
    if constexpr (MODE == 1) { if (g.c1 > 0) kern = igemm_kernel<MODE, BM, BN, WM, WN, true>; }
    if constexpr (MODE == 1 && BM == 128) {                  // (g.z: yv_conv2d_bnbwd, the BatchNorm backward sums in place of STATS')
        if (g.stats) kern = g.z ? igemm_kernel<MODE, BM, BN, WM, WN, false, false, false, true> : igemm_kernel<MODE, BM, BN, WM, WN, false, true>;
    }
    if (!tiles_and_lds(kern, g, BM, BN, lds)) return YV_ERR_LAUNCH;
    const int S = g.splitk > 1 ? g.splitk : 1;
    // (a convolution attaches armed timing events - tools/conv_dma32_bench.py times this route as the parent's; unarmed, and for
    // the linears, the launch is the plain one)
    if constexpr (MODE == 1) launch_timed(kern, g.tiles_m * g.tiles_n * S, THREADS, lds, st, g);
    else hipLaunchKernelGGL(kern, dim3(g.tiles_m * g.tiles_n * S), dim3(THREADS), lds, st, g);
    return launch_splitk_reduce(g, st);
}


// 16-byte row segments need 8-element (bf16) / 4-element (f32) aligned widths, strides and bases
bool epi_can_stage(const GemmArgs& g) {
    const bool f32 = g.flags & (YV_EPI_OUT_F32 | YV_EPI_RES_F32);
    const int al = f32 ? 4 : 8;
    if ((g.N % al) || (g.ldo % al) || ((uintptr_t)g.out & 15)) return false;
    if ((g.flags & YV_EPI_RES_BF16) && ((g.ldres % 8) || ((uintptr_t)g.res & 15))) return false;
    if ((g.flags & (YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD)) && ((g.ldaux % 8) || ((uintptr_t)g.aux & 15))) return false;
    return true;
}

int g_opt_dgrad_s2_split = 0;       // yv_conv2d_dgrad_s2: 1 = one launch per phase ("dgrad_s2_split"; measured slower)
int g_opt_conv_dma = 8;             // convolutions with 64-aligned input channels on the LDS-DMA structure ("conv_dma": 0 off, 1..8 see dispatch)

template <int BN, int WM, int WN, int ST>
int launch_cdma(GemmArgs& g, hipStream_t st) {
    void (*kern)(GemmArgs) = cgemm_dma_kernel<BN, WM, WN, ST>;
    if (g.stats) kern = g.z ? cgemm_dma_kernel<BN, WM, WN, ST, false, false, true> : cgemm_dma_kernel<BN, WM, WN, ST, true>;
    return launch_tiles(kern, g, 128, BN, 256, ST * (size_t)(128 + BN) * 128, st);
}

template <int BN, int WM, int WN, int ST>
int launch_cdma32(GemmArgs& g, hipStream_t st) {
    return launch_tiles(cgemm_dma32_kernel<BN, WM, WN, ST>, g, 128, BN, 256, ST * (size_t)(128 + BN) * 128, st);
}

template <int BM, int KS>
int launch_csmall(GemmArgs& g, hipStream_t st) {
    return launch_tiles(cgemm_small_kernel<BM, KS>, g, BM, 64, 512, KS * 2 * (size_t)(BM + 64) * 128, st);
}

template <int BN, int WM, int WN>
int launch_cmx(ConvMxArgs& a, hipStream_t st) {       // two LDS stages of 128 + BN rows: <= 64 KB
    a.g.tiles_m = (a.g.M + 127) / 128;
    a.g.tiles_n = (a.g.N + BN - 1) / BN;
    auto kern = cgemm_mx_kernel<BN, WM, WN>;
    hipLaunchKernelGGL(kern, dim3(a.g.tiles_m * a.g.tiles_n), dim3(256), 2 * (128 + BN) * 128, st, a);
    return yv_launch_status();
}

// Kernel instances of a convolution (the low four bits of yv_conv2d_instance's code, include/yv_hip.h)
enum ConvKern {
    CK_IGEMM_16 = 0, CK_IGEMM_32 = 1, CK_IGEMM_64 = 2, CK_IGEMM_128 = 3,              // igemm_kernel<1, 128, BN, ..>
    CK_CDMA_64_2 = 4, CK_CDMA_64_3 = 5, CK_CDMA_64_4 = 6, CK_CDMA_128_2 = 7, CK_CDMA_128_3 = 8,  // cgemm_dma_kernel<BN, .., ST>
    CK_SMALL_64 = 9, CK_SMALL_32 = 10,                                                            // cgemm_small_kernel<BM, KS>
    CK_DMA32_64 = 11, CK_DMA32_128 = 13           // cgemm_dma32_kernel<BN, ..> (12: the 96-wide instance, measured and not built)
};

int g_opt_conv_small = 0;           // largest M (output pixels) taken by cgemm_small_kernel ("conv_small"; 0 = the step does not exist)
int g_opt_conv_small_fill = 5;      // ... where 128 x 64 tiles number at most this many eighths of the CU count ("conv_small_fill")
constexpr int SMALL_32_BELOW = 128;  // ... on 32-pixel tiles where 64-pixel tiles would number fewer than this, else on 64-pixel tiles
int g_opt_conv_small_rows = 0;      // ... unless forced: 64 or 32 = that instance for every launch the step takes ("conv_small_rows";
                                    // tools/conv_small_bench.py and the tests time and check each instance on every shape)

// CU count for the fill rule: that of the device current at the first call, kept for the life of the process (one kind of device
// per process is assumed); 256 where no device is present (a route query on a host without one)
int conv_cus() {
    static int n_cu = 0;
    if (!n_cu) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
        n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return n_cu;
}

int g_opt_conv_dma32 = 0;           // non-zero: the convolutions with 32- but not 64-aligned input channels on cgemm_dma32_kernel
                                    // ("conv_dma32"; 0 = the step does not exist)
int g_opt_conv_dma32_cols = 0;      // ... 64 or 128: that instance for every launch the step takes; else the measured rule
                                    // ("conv_dma32_cols"; tools/conv_dma32_bench.py and the tests time and check each instance)

// a K block of `al` (64 or 32) channels lies inside one tap and one source: what the LDS-DMA gathers ask of a layer's channels
bool chan_aligned(const GemmArgs& g, int al) { return ((g.c0 + g.c1) % al) == 0 && (g.c1 == 0 || (g.ksize == 1 && (g.c0 % al) == 0)); }
// the large-map rule of "conv_dma" 8, of the phase launches and of the MXFP8 convolution: from 100 k output pixels the layers
// with more than 64 output channels read their pixels once, on 128-wide tiles
constexpr int LARGE_MAP = 100000;
bool large_map_wide(long long M, int N) { return M >= LARGE_MAP && N > 64; }

int igemm_pick(int N) { return N > 64 ? CK_IGEMM_128 : (N > 32 ? CK_IGEMM_64 : (N > 16 ? CK_IGEMM_32 : CK_IGEMM_16)); }

// The route of one convolution launch: ONE rule for conv_impl_one (which launches it) and yv_conv2d_instance (which reports it).
// Reads the shape, flags, strides and base pointers of g; writes g.staged and g.splitk (g.partial is the caller's) and returns the
// kernel instance.  sums: a yv_conv2d_stats / yv_conv2d_bnbwd call (g.stats / g.z) or a query on the trainer's behalf, which keep
// their route whatever "conv_small" says.
int conv_route(GemmArgs& g, bool have_ws, size_t ws_bytes, bool sums) {
    g.staged = g_opt_staged && epi_can_stage(g);
    // what cgemm_dma_kernel and cgemm_small_kernel ask of a layer
    const bool dma_ok = g.N >= 64 && chan_aligned(g, 64) && g.staged && !g.m_dev && (g.K % BK) == 0;
    // small maps ("conv_small", off by default): the detector at a request's one or few images.  Ahead of
    // split-K and of the "conv_dma" rule, as step 2a of linear_route is ahead of its split-K.  Measured
    // (tools/conv_small_bench.py, profiles/conv_small_layers.txt: every eligible layer of YOLOv8n / s at 1, 2, 4 images of 640 x 640
    // and one of 384 x 640): up to 150 tiles of 128 x 64 every layer takes x 0.46 - 0.86 of cgemm_dma_kernel<64, 4, 1, 3>'s time on
    // the instance chosen below; at 200 tiles the 64-pixel instance takes x 0.85 - 1.04, at 300 x 1.10, at 400 x 1.24 - 1.35.  Hence
    // "conv_small_fill" = 5 (at most 5/8 of a 128 x 64 tile per CU: 160 on 256 CUs; the 200-tile layers stay on the parent's
    // route), and engines.SMALL_MAP_PIXELS = 12,800, the largest M of a layer inside that count.  The 32-pixel tiles where 64-pixel
    // tiles would number fewer than 128: up to 120 such tiles they are the faster instance on all but a few layers (x 0.46 - 0.82
    // against x 0.59 - 0.85), from 150 on the slower one (x 0.83 - 0.90 against x 0.70 - 0.72; at 200, x 0.86 - 1.19 against x 0.67 - 0.86).
    if (g_opt_conv_small > 0 && !sums && dma_ok && g.M <= g_opt_conv_small) {
        const long long cols = (g.N + 63) / 64;
        const long long tiles128 = (long long)((g.M + 127) / 128) * cols, tiles64 = (long long)((g.M + 63) / 64) * cols;
        if (tiles128 * 8 <= (long long)g_opt_conv_small_fill * conv_cus()) {
            g.splitk = 1;
            if (g_opt_conv_small_rows == 64 || g_opt_conv_small_rows == 32) return g_opt_conv_small_rows == 32 ? CK_SMALL_32 : CK_SMALL_64;
            return tiles64 < SMALL_32_BELOW ? CK_SMALL_32 : CK_SMALL_64;
        }
    }
    // split-K: deep small-resolution layers (20x20 / 40x40 maps) give 100-400 tiles for 256 CUs and a serial chain of
    // 9-36 K steps per tile at one workgroup per CU; slicing K puts >= 2 workgroups on every CU and shortens the chain
    g.splitk = 1;
    if (have_ws && g_opt_splitk) {
        const int bn = g.N > 64 ? 128 : (g.N > 32 ? 64 : (g.N > 16 ? 32 : 16));
        const long long tiles = (long long)((g.M + 127) / 128) * ((g.N + bn - 1) / bn);
        const int nk = (g.K + BK - 1) / BK;
        int S = (int)(640 / tiles);
        if (S > nk / 2) S = nk / 2;
        if (S > 8) S = 8;
        if (S >= 2 && (size_t)S * g.M * g.N * sizeof(float) <= ws_bytes && !(g.N & 3)) g.splitk = S;
    }
    if (g_opt_conv_dma && dma_ok && g.splitk <= 1) {
        // conv_dma: 1 = two stages (128-wide tiles for Cout > 64), 2 = three stages, 64-wide tiles (two workgroups per CU, four K
        // steps in flight per CU), 3 = three stages, 128-wide tiles (one workgroup per CU), 4 = four stages, 64-wide tiles,
        // 5 .. 8 mixtures.  Shipped: 8 = three stages / 64-wide, except the 128-channel layers of the large maps (>= 100 k output
        // pixels: the 80 x 80 head convolution at batch 32), which read their pixels once on two-stage 128-wide tiles (70 -> 57 us
        // alone; detect stage 1.175 -> 1.163 ms, YOLOv8m + ViT-L/16 1,376 -> 1,397 images/s; tools/conv_dma_ab.py)
        const int two_stage = g.N > 64 ? CK_CDMA_128_2 : CK_CDMA_64_2;
        if (g_opt_conv_dma == 2) return CK_CDMA_64_3;
        if (g_opt_conv_dma == 3) return g.N > 64 ? CK_CDMA_128_3 : CK_CDMA_64_3;
        if (g_opt_conv_dma == 4) return CK_CDMA_64_4;
        if (g_opt_conv_dma == 5)        // by reduction depth: deep K (>= 1024) three stages / 64-wide, shallow K two stages
            return g.K >= 1024 ? CK_CDMA_64_3 : two_stage;
        if (g_opt_conv_dma == 7)        // by rows: the large maps (>= 100 k output pixels) two stages, 128-wide where Cout allows
            return g.M >= LARGE_MAP ? two_stage : CK_CDMA_64_3;
        if (g_opt_conv_dma == 8)        // as 7, only the 128-wide layers of the large maps
            return large_map_wide(g.M, g.N) ? CK_CDMA_128_2 : CK_CDMA_64_3;
        if (g_opt_conv_dma == 6)        // as 5, but 64-wide tiles everywhere
            return g.K >= 1024 ? CK_CDMA_64_3 : CK_CDMA_64_2;
        return two_stage;
    }
    // 32- but not 64-aligned input channels ("conv_dma32", off by default): what dma_ok asks, with 32 for 64.
    // The 64-aligned layers (Cin % 64 == 0, and c0 % 64 == 0 where there are two sources) keep their route above, whatever
    // "conv_dma" says; a two-source 1 x 1 of 64-aligned Cin whose boundary is only 32-aligned (96 + 32) is this step's.  A sums
    // call and a split-K launch keep igemm_kernel.
    if (g_opt_conv_dma32 && !sums && g.N >= 64 && chan_aligned(g, 32) && !chan_aligned(g, 64) && g.staged && !g.m_dev && g.splitk <= 1) {
        if (g_opt_conv_dma32_cols == 64) return CK_DMA32_64;
        if (g_opt_conv_dma32_cols == 128) return CK_DMA32_128;
        // Measured (tools/conv_dma32_bench.py, profiles/conv_dma32_layers.txt: the 22 layers of YOLOv8m at 64, 4 and 1 images of
        // 640 x 640, the 32 -> 64 and 96 -> 64 layers of YOLOv8s / n at 32, against igemm_kernel, launch by launch): the 128-wide
        // two-stage tiles from 25,600 output pixels on a shallow reduction (K < 1024: the 96-channel layers, x 0.85 - 0.93 of the
        // parent's time, where the 64-wide tiles take x 0.80 - 1.26), the 64-wide three-stage tiles below that and on a deep one
        // (the 288-channel layers x 0.72 - 0.84, the 6,400-pixel layers of one image x 0.69 - 0.70; the 128-wide tiles x 0.85 -
        // 0.90 there).  Cout = 64 stays out: all three such layers measured slower on either instance (x 1.06 - 1.13 on the
        // 64-wide tiles, x 1.38 - 1.46 on the 128-wide ones).  A 96-wide instance was fastest on no layer and is not built.
        if (g.N > 64) return (g.M >= 25600 && g.K < 1024) ? CK_DMA32_128 : CK_DMA32_64;
    }
    return igemm_pick(g.N);
}

template <int MODE>
int launch_igemm(GemmArgs& g, int kern, hipStream_t st) {
    switch (kern) {
    case CK_IGEMM_128: return launch<MODE, 128, 128, 2, 2>(g, st);
    case CK_IGEMM_64: return launch<MODE, 128, 64, 4, 1>(g, st);
    case CK_IGEMM_32: return launch<MODE, 128, 32, 4, 1>(g, st);
    default: return launch<MODE, 128, 16, 4, 1>(g, st);
    }
}

int launch_conv(GemmArgs& g, int kern, hipStream_t st) {
    switch (kern) {
    case CK_CDMA_64_2: return launch_cdma<64, 4, 1, 2>(g, st);
    case CK_CDMA_64_3: return launch_cdma<64, 4, 1, 3>(g, st);
    case CK_CDMA_64_4: return launch_cdma<64, 4, 1, 4>(g, st);
    case CK_CDMA_128_2: return launch_cdma<128, 2, 2, 2>(g, st);
    case CK_CDMA_128_3: return launch_cdma<128, 2, 2, 3>(g, st);
    case CK_SMALL_64: return launch_csmall<64, 2>(g, st);
    case CK_SMALL_32: return launch_csmall<32, 4>(g, st);
    case CK_DMA32_64: return launch_cdma32<64, 4, 1, 3>(g, st);
    case CK_DMA32_128: return launch_cdma32<128, 2, 2, 2>(g, st);
    default: return launch_igemm<1>(g, kern, st);
    }
}

// ---- yv_conv2d_dgrad_s2: the phase form of the two kernel families, the four phases in ONE launch (4 x tiles workgroups) ----------
int launch_phases(void (*kern)(GemmArgs), GemmArgs& g, int threads, size_t lds, hipStream_t st) {
    const int per = g.tiles_m * g.tiles_n;
    if (!g_opt_dgrad_s2_split) {
        g.group_m = 0;
        hipLaunchKernelGGL(kern, dim3(4 * per), dim3(threads), lds, st, g);
        return yv_launch_status();
    }
    for (int q = 0; q < 4; ++q) {                // (tools/dgrad_s2_bench.py --split: the comparison DESIGN 24 reports)
        g.group_m = q;
        hipLaunchKernelGGL(kern, dim3(per), dim3(threads), lds, st, g);
        const int rc = yv_launch_status();
        if (rc != YV_OK) return rc;
    }
    return YV_OK;
}

template <int BN, int WM, int WN>
int launch_phase_igemm(GemmArgs& g, hipStream_t st) {
    size_t lds = (size_t)(128 + BN) * 128;
    if (lds < (size_t)THREADS / 64 * (128 / WM) * 128) lds = (size_t)THREADS / 64 * (128 / WM) * 128;   // the staged epilogue's slabs
    void (*kern)(GemmArgs) = igemm_kernel<1, 128, BN, WM, WN, false, false, true>;
    if (!tiles_and_lds(kern, g, 128, BN, lds)) return YV_ERR_LAUNCH;
    return launch_phases(kern, g, THREADS, lds, st);
}

template <int BN, int WM, int WN, int ST>
int launch_phase_cdma(GemmArgs& g, hipStream_t st) {
    const size_t lds = ST * (size_t)(128 + BN) * 128;
    void (*kern)(GemmArgs) = cgemm_dma_kernel<BN, WM, WN, ST, false, true>;
    if (!tiles_and_lds(kern, g, 128, BN, lds)) return YV_ERR_LAUNCH;
    return launch_phases(kern, g, 256, lds, st);
}

// The route of one phase launch: ONE rule for dgrad_s2_one (which launches it) and yv_conv2d_dgrad_s2_route (which reports it).
// The LDS-DMA form from 64 output columns (= input channels of the layer) where the staged epilogue is usable, 64-wide three-stage
// tiles except the 128-wide two-stage ones of conv_route's large-map rule; igemm_kernel's tiles below that.  Never split-K.
int dgrad_s2_route(GemmArgs& g) {
    g.staged = g_opt_staged && epi_can_stage(g);
    g.splitk = 1;
    if (g_opt_conv_dma && g.N >= 64 && g.staged) return large_map_wide(g.M, g.N) ? CK_CDMA_128_2 : CK_CDMA_64_3;
    return igemm_pick(g.N);
}

int launch_dgrad_s2(GemmArgs& g, int kern, hipStream_t st) {
    switch (kern) {
    case CK_CDMA_64_3: return launch_phase_cdma<64, 4, 1, 3>(g, st);
    case CK_CDMA_128_2: return launch_phase_cdma<128, 2, 2, 2>(g, st);
    case CK_IGEMM_128: return launch_phase_igemm<128, 2, 2>(g, st);
    case CK_IGEMM_64: return launch_phase_igemm<64, 4, 1>(g, st);
    case CK_IGEMM_32: return launch_phase_igemm<32, 4, 1>(g, st);
    default: return launch_phase_igemm<16, 4, 1>(g, st);
    }
}

// the code yv_conv2d_instance documents: the staged bit is set where the staged epilogue RUNS (finish_tile takes it on the 64-column
// wave tiles only, and a split-K launch leaves the epilogue to splitk_reduce_kernel; cgemm_small_kernel's 32-column wave tiles take
// the direct one)
int conv_instance_code(const GemmArgs& g, int kern) {
    const bool split = g.splitk > 1;
    const bool staged = g.staged && !split && ((kern >= CK_IGEMM_64 && kern < CK_SMALL_64) || kern == CK_DMA32_64 || kern == CK_DMA32_128);
    const bool two = g.c1 > 0 && kern <= CK_IGEMM_128;
    return kern | (staged ? 16 : 0) | (split ? 32 : 0) | (two ? 64 : 0);
}

// The route of a linear: ONE rule per operand type (linear_route: bf16, mx_linear_route: MXFP8) for the launch path and for
// yv_linear_route, which reports it without a device.  Pure: shape, flags, strides, null-ness of the pointers and options in, a
// LinearRoute out.  Pinned by tests/test_linear_routes_cpu.py; order, reasons and measurements: DESIGN.md section 19.
using LinearRoute = yv_linear_route_t;
struct LinearQuery { LinearRoute* out; size_t ws_bytes; int n_cu; };     // yv_linear_route: report the route, launch nothing
long long tiles_of(int M, int N, int rows) { return (long long)((M + rows - 1) / rows) * (N >> 8); }     // rows x 256 tiles

LinearRoute route_of(const GemmArgs& g, int kernel, int bm, int bn, int splitk = 1, int abl = 0) {
    LinearRoute r = {};
    r.kernel = kernel; r.tile_rows = bm; r.tile_cols = bn; r.abl = abl; r.splitk = splitk; r.staged = g.staged;
    r.grid = ((g.M + bm - 1) / bm) * ((g.N + bn - 1) / bn) * splitk;
    return r;
}

LinearRoute persistent_route(const GemmArgs& g, int kernel, int rows, bool mx, int n_cu) {
    LinearRoute r = route_of(g, kernel, rows, 256);
    if (r.grid > n_cu) r.grid = n_cu;
    const bool f32o = g.flags & (YV_EPI_RES_F32 | YV_EPI_OUT_F32);
    r.mx = mx;
    r.ext = kernel != YV_LIN_P9 ? 0 : (g.flags & YV_EPI_SAVE_PRE) ? 1 : (g.flags & YV_EPI_GELU_BWD) ? 2 : 0;
    r.f32out = f32o && !r.ext && (kernel == YV_LIN_P9 || rows <= 192);      // (gemm_p8_kernel: launch_p8_inst)
    return r;
}

// What the persistent kernels ask of a linear's shape (kstep: 64 bf16 / 128 MXFP8 elements): 256-column tiles up to 4,096 columns,
// two K steps, output rows of 8-element stride ...
bool persistent_shape(int N, int K, int ldo, int kstep) { return !(N & 255) && N <= 4096 && K >= 2 * kstep && !(ldo & 7); }
// ... and of the launch (esz: bytes per operand element): no GELU before an f32 output, 32-bit byte offsets everywhere
bool persistent_ok(int M, int N, int K, long long lda, int ldo, int flags, bool aux, int ldaux, int esz) {
    const long long lim = 0x7fffffffLL;
    return persistent_shape(N, K, ldo, 128 / esz) && !((flags & YV_EPI_GELU) && (flags & (YV_EPI_RES_F32 | YV_EPI_OUT_F32))) &&
           ((long long)(M - 1) * lda + K) * esz < lim && (long long)N * K * esz < lim &&
           ((long long)(M - 1) * ldo + N) * 4 < lim && (!aux || ((long long)(M - 1) * ldaux + N) * 2 < lim);
}

// the forms split-K takes (linear_impl looks the stream's workspace up for these only: a lock the classifier's linears never take)
bool splitk_form(const GemmArgs& g) { return g_opt_linear_splitk && !(g.flags & ~(YV_EPI_BIAS | YV_EPI_OUT_F32)) && !g.m_dev; }

LinearRoute linear_route(const GemmArgs& g, bool have_ws, size_t ws_bytes, int n_cu) {
    const int M = g.M, N = g.N, K = g.K, flags = g.flags, v = g_opt_variant;
    const bool f32o = flags & (YV_EPI_RES_F32 | YV_EPI_OUT_F32), ext = flags & (YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD);
    // (plain: the forms every family takes - no pos_embed, nothing of yv_linear_ex)
    const bool plain = !(flags & ~(YV_EPI_BIAS | YV_EPI_GELU | YV_EPI_RES_F32 | YV_EPI_OUT_F32)) && !g.resf && !g.aux;
    // 1. one row per crop (the classifier's cls-row tail, the head): gemm_skinny_kernel; 2. register-staged tiles
    if (v == 1 && M <= g_opt_skinny && !(N & 15) && !(K & 31) && plain) return route_of(g, YV_LIN_SKINNY, 64, 16);
    if ((K % BK) || N <= 64 || v == 0) return route_of(g, YV_LIN_IGEMM, 128, 16 << igemm_pick(N));
    // 2a. a handful of crops ("linear_mid", off by default; section 31): gemm_mid_kernel's 64 x 64 tiles with the K range split
    // inside the workgroup, for the rows above the skinny kernel's - never below 257, whatever "linear_skinny" says - where
    // 128 x 128 tiles would make at most "linear_mid_fill" / 8 = 5/8 of a workgroup per CU (160 on 256 CUs).  Measured: up to that count the kernel takes
    // x 0.46 - 0.91 of the 128 x 128 route's time, from 168 tiles on (qkv / fc1 of ViT-L at 4 crops, of ViT-B at 8) x 1.03 - 1.86:
    // those shapes go on to the steps below
    const long long tiles128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
    if (v == 1 && M > (g_opt_skinny > MID_FLOOR ? g_opt_skinny : MID_FLOOR) && M <= g_opt_mid && !(N & 63) && plain &&
        tiles128 * 8 <= (long long)g_opt_mid_fill * n_cu)
        return route_of(g, YV_LIN_MID, 64, 64);
    // 3. split-K for wgrad-shaped problems (few 128 x 128 tiles, a long reduction), partial sums in the stream's workspace, added in
    // slice order by splitk_reduce_kernel; not where the free-running kernel's 96-row tiles fill the chip (the 6,304 x 768 x 768
    // data gradients).  It comes before a forced variant, which it overrides.
    const bool small_fills = g_opt_p9_small && tiles_of(M, N, 96) >= 128;
    const bool p9_small_shape = v == 1 && g_opt_p8 >= 3 && M >= 2048 && persistent_shape(N, K, g.ldo, BK) && small_fills;
    if (have_ws && splitk_form(g) && !p9_small_shape) {
        const long long tiles = (long long)((M + 127) / 128) * ((N + 127) / 128);
        const int nk = K / BK;
        int S = (int)(768 / tiles);
        if (S > nk / 4) S = nk / 4;
        if (S > 8) S = 8;
        if (S >= 2 && (size_t)S * M * N * sizeof(float) <= ws_bytes) return route_of(g, YV_LIN_DMA, 128, 128, S);
    }
    // 4. a forced LDS-DMA instance (101 .. 104 / 201 .. 204: the ablations ABL of gemm_dma_kernel)
    switch (v) {
        case 2: return route_of(g, YV_LIN_DMA, 256, 128);
        case 3: return route_of(g, YV_LIN_DMA, 256, 256);
        case 4: return route_of(g, YV_LIN_DMA, 128, 256);
        case 101: case 102: case 103: case 104: return route_of(g, YV_LIN_DMA, 128, 128, 1, v - 100);
        case 201: case 202: case 203: case 204: return route_of(g, YV_LIN_DMA, 256, 256, 1, v - 200);
    }
    // 5. the persistent kernels, by the shape under "linear_p8" or forced ("linear_variant" 9 / 11).  train: the forms of
    // yv_linear_ex, which only the free-running kernel has (K / 64 even)
    const bool train = g_opt_p8 >= 3 && !(flags & ~(YV_EPI_BIAS | YV_EPI_GELU | YV_EPI_RES_F32 | YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD)) &&
                       (!g.resf || (flags & YV_EPI_RES_F32)) && (!(flags & YV_EPI_SAVE_PRE) || (flags & YV_EPI_GELU)) &&
                       !((flags & YV_EPI_GELU_BWD) && (flags & (YV_EPI_GELU | YV_EPI_SAVE_PRE))) && (g.resf || g.aux) && !((K / BK) & 1);
    const bool asked = v == 1 ? g_opt_p8 && M >= 2048 && (N >= 1536 || g_opt_p8 >= 2) : (v == 9 || v == 11);
    if (asked && (train || plain) && g.staged && persistent_ok(M, N, K, g.lda0, g.ldo, flags, g.aux != nullptr, g.ldaux, 2)) {
        const bool free_running = v == 1 ? g_opt_p8 >= 3 : v == 11;
        // enough tiles for the chip: 192 of 160 rows or, without a trainer epilogue, 128 of 96 rows
        const bool fills = v != 1 || tiles_of(M, N, 160) >= 192 || (small_fills && !ext);
        // (f32 outputs: 160-row tiles, whose K tiles are walked in pairs; the 8-phase kernel takes an odd K / 64)
        if (free_running && fills && !(f32o && ((K / BK) & 1)))
            return persistent_route(g, YV_LIN_P9, p9_tile_rows(M, N, K, flags, false, n_cu, 0), false, n_cu);
        if (free_running ? fills : !train) return persistent_route(g, YV_LIN_P8, p8_tile_rows(M, N, flags, n_cu), false, n_cu);
    }
    // 6. 128 x 128 tiles, two workgroups per CU
    return route_of(g, YV_LIN_DMA, 128, 128);
}

// MXFP8 operands: the mid-M step where "linear_mx_mid" admits the shape (off by default), then the free-running persistent kernel
// (tests/test_gpu_mx_train.py::test_mx_linear_ex_epilogues reaches each epilogue family on it and on the other), else
// gemm_mx_kernel<128, 128, 2, 2>
LinearRoute mx_linear_route(const GemmArgs& g, long long lda, long long a_rows, long long w_rows, int n_cu) {
    const int M = g.M, N = g.N, K = g.K, flags = g.flags, nkm = K >> 7;
    const bool f32o = flags & (YV_EPI_RES_F32 | YV_EPI_OUT_F32), ext = flags & (YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD);
    // a handful of crops ("linear_mx_mid", off by default; section 38): gemm_mx_mid_kernel's 64 x 64 tiles with the K steps dealt to
    // two wave groups, from one row on (the MX route has no skinny kernel), where 128 x 128 tiles would make at most
    // "linear_mx_mid_fill" / 8 of a workgroup per CU.  The forms of the inference engine only: no trainer epilogue, no separate
    // residual source
    const long long tiles128 = (long long)((M + 127) / 128) * ((N + 127) / 128);
    if (M >= 1 && M <= g_opt_mx_mid && !(N & 63) && N > 64 && !(K & 127) &&
        !(flags & ~(YV_EPI_BIAS | YV_EPI_GELU | YV_EPI_RES_F32 | YV_EPI_OUT_F32 | YV_EPI_OUT_MXFP8)) && !((flags & YV_EPI_OUT_MXFP8) && f32o) &&
        !g.resf && !g.aux && tiles128 * 8 <= (long long)g_opt_mx_mid_fill * n_cu) {
        LinearRoute r = route_of(g, YV_LIN_MX_MID, 64, 64);
        return r.mx = 1, r;
    }
    if (g_opt_p8 >= 3 && g_opt_variant == 1 && M >= 2048 && tiles_of(M, N, 160) >= 192 &&
        persistent_ok(M, N, K, lda, g.ldo, flags, ext, g.ldaux, 1) && !((flags & YV_EPI_OUT_MXFP8) && f32o) && !(f32o && (nkm & 1)) &&
        (long long)nkm * a_rows * 4 < 0x7fffffffLL && (long long)nkm * w_rows * 4 < 0x7fffffffLL)
        return persistent_route(g, YV_LIN_P9, p9_tile_rows(M, N, K, flags, true, n_cu, 0), true, n_cu);
    LinearRoute r = route_of(g, YV_LIN_MX, 128, 128);
    return r.mx = 1, r;
}

// Token slices of a weight gradient of `tiles` 128 x 128 output tiles (out_bytes together) over T tokens (1: no split).  Conv
// shapes (1-16 tiles over 10^5+ output pixels): up to "wgrad_split_cap" slices of >= 512 rows.  Matrix shapes: ONE round of the
// 512 workgroup slots - a second, partly filled round costs more than the longer slices of the first save (tools/wgrad_bench.py:
// dW 2304 x 768 over 6,336 tokens 43 us at S = 4, 65 us at S = 5)
int wgrad_slices(long long tiles, int T, size_t out_bytes, size_t ws_bytes) {
    int S = (int)((tiles <= 16 ? 1024 : 512) / tiles);
    if (S < 1) S = 1;
    const int cap = tiles <= 16 ? g_opt_wgrad_cap : 16;
    const int min_rows = tiles <= 16 ? 512 : 128;
    if (S > T / min_rows) S = T / min_rows;
    if (S > cap) S = cap;
    if (tiles > 16 && g_opt_wgrad_split > 0) S = g_opt_wgrad_split;
    const size_t fit = ws_bytes / out_bytes;
    if ((size_t)S > fit) S = (int)fit;
    return S >= 2 ? S : 1;
}

// The route of a weight gradient: ONE rule for wgrad_impl's launch and for yv_wgrad_route, which reports it without a device.
// Pure: shape, the requested N tile (128: gemm_tn_kernel, the decision from before the narrow tiles; 64 / 32:
// gemm_tn_narrow_kernel, x 256 k columns; 0: choose), the workspace size, the CU count and the options in, a WgradRoute out.
// tile_n = 0, in this order (measurements: DESIGN.md section 20, profiles/wgrad_narrow_layers_column_rule.txt):
//   1. the tile with the fewest padded columns ceil(N / tile) * tile, ties to the wider tile - so 128 stays wherever a narrow
//      tile would compute as many columns (every N % 128 == 0, and e.g. N = 104);
//   2. a 64-wide tile goes back to 128 when it would launch FEWER workgroups than the 128 x 128 tiles and those fit one round of
//      the 2 * n_cu workgroup slots.  A 64 x 256 workgroup does the MFMA work of a 128 x 128 one per step over twice the useful
//      k range: half the workgroups at the same pace each lose to a machine the 128 x 128 launch does not even fill (K = 192,
//      288 at any T; every K >= 576 at <= 28 k tokens: x 1.03 - 1.14 measured), and win once that launch needs a second round
//      (K >= 576 at 10^5 tokens: x 0.67 - 0.76) or where the count does not change (K <= 128: x 0.84 - 0.94).  A 32-wide tile
//      stays: its workgroup carries half the accumulators and MFMAs, and it won at every measured shape (x 0.70 - 0.93).
// n_cu = 0 stands for 256, the part wgrad_slices' slot constants are for.  Pinned by tests/test_wgrad_routes_cpu.py.
using WgradRoute = yv_wgrad_route_t;
static WgradRoute wgrad_tiled_route(int T, int N, int K, int tile_n, size_t ws_bytes) {
    WgradRoute r = {};
    r.tile_n = tile_n;
    r.tile_k = tile_n == 128 ? 128 : 256;
    r.tiles = ((N + r.tile_n - 1) / r.tile_n) * ((K + r.tile_k - 1) / r.tile_k);
    r.slices = ws_bytes ? wgrad_slices(r.tiles, T, (size_t)N * K * sizeof(float), ws_bytes) : 1;
    r.workgroups = r.tiles * r.slices;
    return r;
}
WgradRoute wgrad_route(int T, int N, int K, int tile_n, size_t ws_bytes, int n_cu) {
    if (tile_n) return wgrad_tiled_route(T, N, K, tile_n, ws_bytes);
    const WgradRoute wide = wgrad_tiled_route(T, N, K, 128, ws_bytes);
    tile_n = 128;
    for (int t = 64; t >= 32; t >>= 1)
        if ((N + t - 1) / t * t < (N + tile_n - 1) / tile_n * tile_n) tile_n = t;
    if (tile_n == 128) return wide;
    const WgradRoute r = wgrad_tiled_route(T, N, K, tile_n, ws_bytes);
    if (tile_n == 64 && r.workgroups < wide.workgroups && wide.workgroups <= 2 * (n_cu > 0 ? n_cu : 256)) return wide;
    return r;
}

// The route of yv_wgrad_wide: ONE rule for its launch and for yv_wgrad_wide_route (measurements: DESIGN.md section 21,
// profiles/wgrad_wide_layers.txt, profiles/wgrad_wide_slices.txt).  mode 1: the 256 (n) x 128 (k) tiles of gemm_tn_wide_kernel.
// mode 0: those tiles where N >= 256, K >= 128, the 128 x 128 launch has more than 16 tiles (matrix shapes, not the conv regime)
// AND those tiles times the 64-token tiles of T number at least 25,000; everywhere else exactly wgrad_route(T, N, K, 128).  The
// wide tile's gain grows with the MFMA work, its price (half the workgroups, twice the slices to reduce) does not: every measured
// shape below the bound was no faster wide (all of ViT-B/16 at 32 crops x 1.00 - 1.47, qkv at 64 crops x 1.04, every proj, head and
// patch embedding x 1.15 - 1.49), every one above it faster (x 0.85 - 0.98).
// Slices of the wide tile: one round of the 2 * n_cu workgroup slots, at least 128 token rows per slice, at most 16, and EVEN
// when more than two: slice = workgroup % S and workgroups b, b + 8 share an XCD's L2, so under an odd S every XCD reads every
// token slice (qkv of ViT-B/16: S = 8 48 us, S = 9 54 us at 32 crops, 114 against 136 us at 128).  "wgrad_split" > 0 forces the
// count at any tile count; then what the workspace holds.
static int wgrad_wide_slices(long long tiles, int T, size_t out_bytes, size_t ws_bytes, int n_cu) {
    int S = (int)(2LL * n_cu / tiles);
    if (S > T / 128) S = T / 128;
    if (S > 16) S = 16;
    if (S > 2) S &= ~1;
    if (g_opt_wgrad_split > 0) S = g_opt_wgrad_split;
    const size_t fit = ws_bytes / out_bytes;
    if ((size_t)S > fit) S = (int)fit;
    return S >= 2 ? S : 1;
}
WgradRoute wgrad_wide_route(int T, int N, int K, int mode, size_t ws_bytes, int n_cu) {
    const WgradRoute base = wgrad_tiled_route(T, N, K, 128, ws_bytes);
    if (mode == 0 && !(N >= 256 && K >= 128 && base.tiles > 16 && (long long)base.tiles * (T / 64) >= 25000)) return base;
    WgradRoute r = {};
    r.tile_n = 256;
    r.tile_k = 128;
    r.tiles = ((N + 255) / 256) * ((K + 127) / 128);
    r.slices = ws_bytes ? wgrad_wide_slices(r.tiles, T, (size_t)N * K * sizeof(float), ws_bytes, n_cu > 0 ? n_cu : 256) : 1;
    r.workgroups = r.tiles * r.slices;
    return r;
}

// Images per sub-batch of a convolution (32-bit byte offsets: each source below 2 GB): s0 / s1 bytes per image of the sources
// (s1 = 0: one source), `lead` bytes addressed in front of source 0.  < 1: a single image is too large.
long long conv_sub_batch(long long s0, long long s1, long long lead) {
    const long long cap = 0x7ffffff0LL;
    long long nb = s0 > 0 ? (cap - lead) / s0 : 0x7fffffffLL;
    if (s1 > 0 && cap / s1 < nb) nb = cap / s1;
    return nb;
}

}  // namespace

extern "C" int yv_set_workspace(void* stream, void* ws, size_t bytes) {
    std::lock_guard<std::mutex> lk(g_ws_mu);
    if (!ws || !bytes) g_ws.erase(stream);
    else g_ws[stream] = std::make_pair(ws, bytes);
    return YV_OK;
}

extern "C" int yv_mx_probe(const void* a, const void* b, const void* sa, const void* sb, int opsel, void* d, void* stream) {
    if (!a || !b || !sa || !sb || !d || opsel < 0 || opsel > 3) return YV_ERR_ARG;
    hipLaunchKernelGGL(mx_probe_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, (const i32x8*)a, (const i32x8*)b,
                       (const int*)sa, (const int*)sb, opsel, (f32x4*)d);
    return yv_launch_status();
}

extern "C" int yv_quant_mxfp8(const void* x, long long ldx, long long rows, int K, void* q, long long ldq, void* scales,
                              long long rows_pad, void* stream) {
    if (!x || !q || !scales || rows <= 0 || K <= 0 || (K & 127) || (ldx & 7) || (ldq & 15)) return YV_ERR_ARG;
    if (rows_pad < rows || (rows_pad & 127)) return YV_ERR_ARG;
    if (((uintptr_t)x | (uintptr_t)q) & 15) return YV_ERR_ARG;
    const long long items = rows * (K >> 5);
    hipLaunchKernelGGL(quant_mx_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)x, ldx, rows, K, (uint8_t*)q, ldq, (uint8_t*)scales, rows_pad);
    return yv_launch_status();
}

static int linear_mx_impl(const void* Aq, long long lda, const void* Ascale, long long a_rows_pad, const void* Wq,
                          const void* Wscale, long long w_rows_pad, const float* bias, int M, int N, int K, void* out,
                          int ldo, int flags, const int32_t* m_dev, int m_mul, void* out_q, long long ldq, void* out_scales,
                          long long out_rows_pad, void* stream, const float* res_f32 = nullptr, void* aux = nullptr,
                          int ldaux = 0, const LinearQuery* q = nullptr);

extern "C" int yv_linear_mxfp8(const void* Aq, long long lda, const void* Ascale, long long a_rows_pad, const void* Wq,
                               const void* Wscale, long long w_rows_pad, const float* bias, int M, int N, int K, void* out,
                               int ldo, int flags, const int32_t* m_dev, int m_mul, void* stream) {
    if (flags & YV_EPI_OUT_MXFP8) return YV_ERR_ARG;
    return linear_mx_impl(Aq, lda, Ascale, a_rows_pad, Wq, Wscale, w_rows_pad, bias, M, N, K, out, ldo, flags, m_dev, m_mul,
                          nullptr, 0, nullptr, 0, stream);
}

// what the _q form asks on top of linear_mx_impl (yv_linear_mxfp8_q and its route report)
static bool mx_q_args_ok(const void* out_q, const void* out_scales, int M, int N, int flags, long long ldq, long long out_rows_pad) {
    if (!out_q || !out_scales || (N & 127) || (ldq & 15) || ldq < N || out_rows_pad < M || (out_rows_pad & 127)) return false;
    return !(flags & ~(YV_EPI_BIAS | YV_EPI_GELU));
}

extern "C" int yv_linear_mxfp8_q(const void* Aq, long long lda, const void* Ascale, long long a_rows_pad, const void* Wq,
                                 const void* Wscale, long long w_rows_pad, const float* bias, int M, int N, int K, int flags,
                                 const int32_t* m_dev, int m_mul, void* out_q, long long ldq, void* out_scales,
                                 long long out_rows_pad, void* stream) {
    if (!mx_q_args_ok(out_q, out_scales, M, N, flags, ldq, out_rows_pad)) return YV_ERR_ARG;
    return linear_mx_impl(Aq, lda, Ascale, a_rows_pad, Wq, Wscale, w_rows_pad, bias, M, N, K, out_q, (int)ldq,
                          flags | YV_EPI_OUT_MXFP8, m_dev, m_mul, out_q, ldq, out_scales, out_rows_pad, stream);
}

// gemm_mx_kernel<128, 128, 2, 2> (split-K when g.splitk > 1: partials into g.partial, then splitk_reduce_kernel)
static int launch_mx128(MxArgs& a, hipStream_t stream) {
    GemmArgs& g = a.g;
    g.tiles_m = (g.M + 127) / 128; g.tiles_n = (g.N + 127) / 128;
    const int S = g.splitk > 1 ? g.splitk : 1;
    // (a 4-stage ring with ONE workgroup per CU and three K steps in flight was built in round 1, measured 35 % slower than two
    // co-resident 2-stage workgroups, and removed in round 2: see DESIGN.md section 6, "MX deep ring")
    const int threads = 256;
    const size_t lds = 2 * (size_t)(128 * 128 * 2 + 1024);
    auto kern = gemm_mx_kernel<128, 128, 2, 2>;
    if (!yv_grant_lds((const void*)kern, lds)) return YV_ERR_LAUNCH;
    launch_timed(kern, (unsigned)(g.tiles_m * g.tiles_n * S), threads, lds, stream, a);
    return launch_splitk_reduce(g, stream);
}

// flags of the MX linears' epilogues: yv_linear_mxfp8 (+ YV_EPI_OUT_MXFP8 from yv_linear_mxfp8_q) and, with a separate f32
// residual source / the bf16 side tensor, the training forms of yv_linear_mxfp8_ex
static bool mx_flags_ok(int flags, const float* res_f32, const void* aux, int ldaux) {
    if (flags & ~(YV_EPI_BIAS | YV_EPI_GELU | YV_EPI_RES_F32 | YV_EPI_OUT_F32 | YV_EPI_OUT_MXFP8 | YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD))
        return false;
    if (res_f32 && !(flags & YV_EPI_RES_F32)) return false;
    const bool ext = flags & (YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD);
    if (ext && (!aux || ldaux <= 0 || (ldaux & 7) || ((uintptr_t)aux & 15))) return false;
    if (ext && (flags & (YV_EPI_OUT_F32 | YV_EPI_RES_F32 | YV_EPI_OUT_MXFP8))) return false;        // bf16 output only
    if ((flags & YV_EPI_SAVE_PRE) && ((flags & YV_EPI_GELU_BWD) || !(flags & YV_EPI_GELU))) return false;
    if ((flags & YV_EPI_GELU_BWD) && (flags & YV_EPI_GELU)) return false;
    if (!ext && aux) return false;
    return true;
}

static int linear_mx_impl(const void* Aq, long long lda, const void* Ascale, long long a_rows_pad, const void* Wq,
                          const void* Wscale, long long w_rows_pad, const float* bias, int M, int N, int K, void* out,
                          int ldo, int flags, const int32_t* m_dev, int m_mul, void* out_q, long long ldq, void* out_scales,
                          long long out_rows_pad, void* stream, const float* res_f32, void* aux, int ldaux, const LinearQuery* q) {
    if (!Aq || !Ascale || !Wq || !Wscale || !out || M < 0 || N <= 0 || K <= 0) return YV_ERR_ARG;
    if ((K & 127) || (lda & 15) || (N & 7) || (ldo & 7)) return YV_ERR_ARG;             // whole 128-element K steps
    if (a_rows_pad < M || (a_rows_pad & 127) || w_rows_pad < N || (w_rows_pad & 127)) return YV_ERR_ARG;
    if (((uintptr_t)Ascale | (uintptr_t)Wscale) & 15) return YV_ERR_ARG;
    if ((flags & YV_EPI_BIAS) && !bias) return YV_ERR_ARG;
    if (!mx_flags_ok(flags, res_f32, aux, ldaux)) return YV_ERR_ARG;
    if (((uintptr_t)Aq | (uintptr_t)Wq | (uintptr_t)out | (uintptr_t)res_f32) & 15) return YV_ERR_ARG;
    if (M == 0) return YV_OK;
    MxArgs a = {};
    GemmArgs& g = a.g;
    g.a0 = (const uint16_t*)Aq; g.lda0 = (int)lda; g.w = (const uint16_t*)Wq; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.out = out; g.ldo = ldo; g.flags = flags; g.m_dev = m_dev; g.m_mul = m_mul;
    g.resf = res_f32; g.aux = (uint16_t*)aux; g.ldaux = ldaux;
    g.ksize = 1; g.stride = 1; g.splitk = 1;
    g.staged = epi_can_stage(g);
    if (!g.staged) return YV_ERR_ARG;
    g.group_m = g_opt_group_m > 0 ? g_opt_group_m : 8;
    a.sa = (const uint8_t*)Ascale; a.sw = (const uint8_t*)Wscale; a.rows_a = a_rows_pad; a.rows_w = w_rows_pad;
    g.mxq = (uint8_t*)out_q; g.ldmxq = ldq; g.mxs = (uint8_t*)out_scales; g.mx_rows = out_rows_pad;
    // (persistent kernel: the bf16 schedule with one block-scaled MFMA per fragment pair and K tile)
    g.mx_sa = a.sa; g.mx_sw = a.sw; g.mx_rows_a = a.rows_a; g.mx_rows_w = a.rows_w;
    const int n_cu = q ? q->n_cu : persistent_cus();
    if (!n_cu) return YV_ERR_LAUNCH;
    const LinearRoute r = mx_linear_route(g, lda, a_rows_pad, w_rows_pad, n_cu);
    if (q) { *q->out = r; return YV_OK; }
    if (r.kernel == YV_LIN_P9) return launch_p9(g, (hipStream_t)stream, r.tile_rows, n_cu, true);
    if (r.kernel == YV_LIN_MX_MID) return launch_mx_mid(a, (hipStream_t)stream);
    return launch_mx128(a, (hipStream_t)stream);
}

extern "C" int yv_linear_mxfp8_ex(const void* Aq, long long lda, const void* Ascale, long long a_rows_pad, const void* Wq,
                                  const void* Wscale, long long w_rows_pad, const float* bias, int M, int N, int K, void* out,
                                  int ldo, int flags, const float* res_f32, void* aux, int ldaux, void* stream) {
    if (flags & YV_EPI_OUT_MXFP8) return YV_ERR_ARG;
    return linear_mx_impl(Aq, lda, Ascale, a_rows_pad, Wq, Wscale, w_rows_pad, bias, M, N, K, out, ldo, flags, nullptr, 1,
                          nullptr, 0, nullptr, 0, stream, res_f32, aux, ldaux);
}

extern "C" int yv_linear_mxfp8_instance(int M, int N, int K, int flags) {
    // dense operands (lda = K, ldo = ldaux = N); the kernel family does not depend on the CU count
    LinearRoute r;
    const int rc = yv_linear_route(M, N, K, K, N, flags, 0, (flags & (YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD)) ? N : 0, 1, 0, 256, &r);
    return rc != YV_OK ? rc : r.kernel == YV_LIN_P9;
}

int g_opt_wgrad_mx_split = 0;      // > 0: forced number of token slices of the MX weight gradient ("wgrad_mx_split"; 1 = off)

// dW (N, K) f32 = dY^T . X over T_pad tokens from the column forms of yv_quant_mxfp8_2d: dYt (N, T_pad) and Xt (K, T_pad) e4m3
// bytes (row strides ldy / ldx bytes) with their token-block scales (T_pad/128, rows_pad, 4).  gemm_mx_kernel with M = N,
// N = K, K = T_pad; the split over tokens follows yv_wgrad's matrix-shaped rule (one round of two workgroups per CU).
extern "C" int yv_wgrad_mxfp8(const void* dYt, long long ldy, const void* sdy, long long dy_rows_pad, const void* Xt, long long ldx,
                              const void* sx, long long x_rows_pad, int T_pad, int N, int K, float* dW, int ldw, void* stream) {
    if (!dYt || !sdy || !Xt || !sx || !dW || T_pad <= 0 || N <= 0 || K <= 0) return YV_ERR_ARG;
    if ((T_pad & 127) || ldy < T_pad || ldx < T_pad || (ldy & 15) || (ldx & 15) || (N & 7) || (K & 7) || ldw < K || (ldw & 3))
        return YV_ERR_ARG;
    if (dy_rows_pad < N || (dy_rows_pad & 127) || x_rows_pad < K || (x_rows_pad & 127)) return YV_ERR_ARG;
    if (((uintptr_t)dYt | (uintptr_t)Xt | (uintptr_t)dW | (uintptr_t)sdy | (uintptr_t)sx) & 15) return YV_ERR_ARG;
    if ((long long)(N - 1) * ldy + T_pad >= 0x7fffffffLL || (long long)(K - 1) * ldx + T_pad >= 0x7fffffffLL) return YV_ERR_LIMIT;
    MxArgs a = {};
    GemmArgs& g = a.g;
    g.a0 = (const uint16_t*)dYt; g.lda0 = (int)ldy; g.w = (const uint16_t*)Xt; g.ldw = (int)ldx;
    g.M = N; g.N = K; g.K = T_pad; g.out = dW; g.ldo = ldw; g.flags = YV_EPI_OUT_F32; g.m_mul = 1;
    g.ksize = 1; g.stride = 1; g.splitk = 1;
    g.staged = epi_can_stage(g);
    if (!g.staged) return YV_ERR_ARG;
    g.group_m = g_opt_group_m > 0 ? g_opt_group_m : 8;
    a.sa = (const uint8_t*)sdy; a.sw = (const uint8_t*)sx; a.rows_a = dy_rows_pad; a.rows_w = x_rows_pad;
    void* ws = nullptr; size_t wsb = 0;
    if (ws_lookup(stream, &ws, &wsb)) {
        const long long tiles = (long long)((N + 127) / 128) * ((K + 127) / 128);
        const int nk = T_pad >> 7;
        int S = g_opt_wgrad_mx_split > 0 ? g_opt_wgrad_mx_split : (int)(512 / tiles);
        if (g_opt_wgrad_mx_split <= 0 && S > nk / 2) S = nk / 2;      // at least two 128-token K steps per slice
        if (S > nk) S = nk;
        if (S > 16) S = 16;
        const size_t fit = wsb / ((size_t)N * K * sizeof(float));
        if ((size_t)S > fit) S = (int)fit;
        if (S >= 2) { g.splitk = S; g.partial = (float*)ws; }
    }
    return launch_mx128(a, (hipStream_t)stream);
}

extern "C" int yv_quant_mxfp8_2d(const void* x, long long ldx, long long T, int C, void* q, long long ldq, void* scales,
                                 long long rows_pad, void* qt, long long ldqt, void* scales_t, long long c_rows_pad,
                                 long long T_pad, void* stream) {
    if (!x || T <= 0 || C <= 0 || (C & 127) || (ldx & 7) || ldx < C || ((uintptr_t)x & 15)) return YV_ERR_ARG;
    if (!q && !qt) return YV_ERR_ARG;
    if ((q == nullptr) != (scales == nullptr) || (qt == nullptr) != (scales_t == nullptr)) return YV_ERR_ARG;
    if (q && ((ldq & 15) || ldq < C || rows_pad < T || (rows_pad & 127) || ((uintptr_t)q & 15))) return YV_ERR_ARG;
    if (qt && (T_pad < T || (T_pad & 127) || ldqt < T_pad || (ldqt & 15) || c_rows_pad < C || (c_rows_pad & 127) ||
               ((uintptr_t)qt & 15)))
        return YV_ERR_ARG;
    const long long rows = qt ? T_pad : (T + 63) / 64 * 64;
    if (rows / 64 > 0x7fffffffLL) return YV_ERR_LIMIT;
    hipLaunchKernelGGL(quant_mx_2d_kernel, dim3((unsigned)(rows / 64), (unsigned)(C / 128)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)x, ldx, T, C, (uint8_t*)q, ldq, (uint8_t*)scales, rows_pad, (uint8_t*)qt, ldqt,
                       (uint8_t*)scales_t, c_rows_pad);
    return yv_launch_status();
}

extern "C" int yv_set_launch_timing(void* start_event, void* stop_event) {
    t_time_start = (hipEvent_t)start_event;
    t_time_stop = (hipEvent_t)stop_event;
    return YV_OK;
}

// key -> the option's storage (an accessor, not an address: linear_p8_cus is thread_local, so its address depends on the caller)
static const struct { const char* key; int* (*at)(); } k_options[] = {
    {"linear_variant", [] { return &g_opt_variant; }},
    {"wgrad_split_cap", [] { return &g_opt_wgrad_cap; }},
    {"wgrad_split", [] { return &g_opt_wgrad_split; }},
    {"linear_p9_small", [] { return &g_opt_p9_small; }},
    {"linear_p9_small_fixed", [] { return &g_opt_p9_small_fixed; }},
    {"linear_group_m", [] { return &g_opt_group_m; }},
    {"staged_epilogue", [] { return &g_opt_staged; }},
    {"linear_p8", [] { return &g_opt_p8; }},
    {"linear_p8_rows", [] { return &g_opt_p8_rows; }},
    {"linear_p8_cus", [] { return &g_opt_p8_cus; }},
    {"linear_p8_sched", [] { return &g_opt_p8_sched; }},
    {"conv_splitk", [] { return &g_opt_splitk; }},
    {"linear_splitk", [] { return &g_opt_linear_splitk; }},
    {"linear_skinny", [] { return &g_opt_skinny; }},
    {"linear_mid", [] { return &g_opt_mid; }},
    {"linear_mid_fill", [] { return &g_opt_mid_fill; }},
    {"linear_mx_mid", [] { return &g_opt_mx_mid; }},
    {"linear_mx_mid_fill", [] { return &g_opt_mx_mid_fill; }},
    {"linear_ln_mid", [] { return &g_opt_ln_mid; }},
    {"linear_ln_fill", [] { return &g_opt_ln_mid_fill; }},
    {"wgrad_mx_split", [] { return &g_opt_wgrad_mx_split; }},
    {"conv_dma", [] { return &g_opt_conv_dma; }},
    {"conv_small", [] { return &g_opt_conv_small; }},
    {"conv_small_fill", [] { return &g_opt_conv_small_fill; }},
    {"conv_small_rows", [] { return &g_opt_conv_small_rows; }},
    {"conv_dma32", [] { return &g_opt_conv_dma32; }},
    {"conv_dma32_cols", [] { return &g_opt_conv_dma32_cols; }},
    {"dgrad_s2_split", [] { return &g_opt_dgrad_s2_split; }},
};
static int* option_at(const char* key) {
    for (const auto& o : k_options)
        if (key && !strcmp(key, o.key)) return o.at();
    return nullptr;
}

extern "C" int yv_set_option(const char* key, int value) {
    int* const opt = option_at(key);
    if (!opt) return YV_ERR_ARG;
    *opt = value;
    return YV_OK;
}

extern "C" int yv_get_option(const char* key, int* value) {
    const int* const opt = option_at(key);
    if (!opt || !value) return YV_ERR_ARG;
    *value = *opt;
    return YV_OK;
}

// Launches the route: no decisions.  ws: the workspace the route was told of.
static int launch_linear(GemmArgs& g, const LinearRoute& r, void* ws, int n_cu, hipStream_t st) {
    g.splitk = r.splitk;
    if (r.splitk > 1) g.partial = (float*)ws;
    switch (r.kernel) {
        case YV_LIN_SKINNY: return launch_skinny(g, st);
        case YV_LIN_MID: return launch_mid(g, st);
        case YV_LIN_P8: return launch_p8(g, st, r.tile_rows, n_cu);
        case YV_LIN_P9: return launch_p9(g, st, r.tile_rows, n_cu, r.mx);
    }
    if (r.kernel == YV_LIN_DMA)
        switch ((r.tile_rows >> 7) * 100 + (r.tile_cols >> 7) * 10 + r.abl) {      // gemm_dma_kernel<rows, columns, waves, ABL>
            case 210: return launch_dma<256, 128, 4, 2>(g, st);
            case 220: return launch_dma<256, 256, 2, 4>(g, st);
            case 120: return launch_dma<128, 256, 2, 4>(g, st);
            case 221: return launch_dma<256, 256, 2, 4, 1>(g, st);
            case 222: return launch_dma<256, 256, 2, 4, 2>(g, st);
            case 223: return launch_dma<256, 256, 2, 4, 3>(g, st);
            case 224: return launch_dma<256, 256, 2, 4, 4>(g, st);
            case 111: return launch_dma<128, 128, 2, 2, 1>(g, st);
            case 112: return launch_dma<128, 128, 2, 2, 2>(g, st);
            case 113: return launch_dma<128, 128, 2, 2, 3>(g, st);
            case 114: return launch_dma<128, 128, 2, 2, 4>(g, st);
            default: return launch_dma<128, 128, 2, 2>(g, st);
        }
    // (named last, as before: kernels are emitted in the order they are named, and igemm_kernel addresses g_zero_page pc-relative)
    return launch_igemm<0>(g, igemm_pick(r.tile_cols), st);
}

static int linear_impl(const void* A, int lda, const void* W, const float* bias, int M, int N, int K, void* out, int ldo,
                       const float* pos, int tok, int flags, const int32_t* m_dev, int m_mul, const float* res_f32,
                       void* aux, int ldaux, hipStream_t stream, const LinearQuery* q = nullptr) {
    if (!A || !W || !out || M < 0 || N <= 0 || K <= 0) return YV_ERR_ARG;
    if ((K & 7) || (lda & 7) || (N & 3) || (ldo & 3)) return YV_ERR_ARG;            // 16-byte operand chunks, 4-wide stores
    if ((flags & YV_EPI_BIAS) && !bias) return YV_ERR_ARG;
    if ((flags & YV_EPI_POSEMB) && (!pos || tok <= 0)) return YV_ERR_ARG;
    if (flags & (YV_EPI_SILU | YV_EPI_RES_BF16)) return YV_ERR_ARG;
    if ((flags & (YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD)) && (!aux || (flags & (YV_EPI_OUT_F32 | YV_EPI_RES_F32)))) return YV_ERR_ARG;
    if (((uintptr_t)A | (uintptr_t)W | (uintptr_t)out) & 15) return YV_ERR_ARG;
    if (M == 0) return YV_OK;
    GemmArgs g = {};
    g.a0 = (const uint16_t*)A; g.lda0 = lda; g.c0 = K;
    g.w = (const uint16_t*)W; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.out = out; g.ldo = ldo; g.pos = pos; g.tok = tok; g.flags = flags; g.m_dev = m_dev; g.m_mul = m_mul;
    g.resf = res_f32; g.aux = (uint16_t*)aux; g.ldaux = ldaux;
    g.ksize = 1; g.stride = 1;
    g.staged = g_opt_staged && epi_can_stage(g);
    if ((flags & (YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD)) && (!g.staged || (K % BK) || N <= 64)) return YV_ERR_ARG;
    if (res_f32 && (!g.staged || (K % BK) || N <= 64)) return YV_ERR_ARG;
    g.group_m = g_opt_group_m > 0 ? g_opt_group_m : 8;
    void* ws = nullptr; size_t wsb = 0;
    if (q) { ws = q->ws_bytes ? out : nullptr; wsb = q->ws_bytes; }
    else if (splitk_form(g)) ws_lookup((void*)stream, &ws, &wsb);
    const int n_cu = q ? q->n_cu : persistent_cus();
    if (!n_cu) return YV_ERR_LAUNCH;
    const LinearRoute r = linear_route(g, ws != nullptr, wsb, n_cu);
    if (q) { *q->out = r; return YV_OK; }
    return launch_linear(g, r, ws, n_cu, stream);
}

extern "C" int yv_linear(const void* A, int lda, const void* W, const float* bias, int M, int N, int K, void* out,
                         int ldo, const float* pos, int tok, int flags, const int32_t* m_dev, int m_mul, void* stream) {
    return linear_impl(A, lda, W, bias, M, N, K, out, ldo, pos, tok, flags, m_dev, m_mul, nullptr, nullptr, 0,
                       (hipStream_t)stream);
}

extern "C" int yv_linear_ex(const void* A, int lda, const void* W, const float* bias, int M, int N, int K, void* out,
                            int ldo, int flags, const float* res_f32, void* aux, int ldaux, void* stream) {
    return linear_impl(A, lda, W, bias, M, N, K, out, ldo, nullptr, 0, flags, nullptr, 1, res_f32, aux, ldaux,
                       (hipStream_t)stream);
}

// The launch path on dummy 16-byte-aligned bases with a LinearQuery, i.e. its argument checks and its route; nothing is
// dereferenced or launched.  MX: scale rows rounded up to 128, as the trainer allocates them.
extern "C" int yv_linear_route(int M, int N, int K, int lda, int ldo, int flags, int has_res_f32, int ldaux, int mx, size_t ws_bytes,
                               int n_cu, yv_linear_route_t* out) {
    static unsigned char dummy[16] __attribute__((aligned(16)));
    if (!out || M <= 0 || n_cu < 0) return YV_ERR_ARG;
    const LinearQuery q = {out, ws_bytes, persistent_cus(n_cu)};
    const float* f = (const float*)dummy;
    const int32_t* m_dev = (flags & YV_ROUTE_M_DEV) ? (const int32_t*)dummy : nullptr;
    flags &= ~YV_ROUTE_M_DEV;
    if (!mx)
        return linear_impl(dummy, lda, dummy, f, M, N, K, dummy, ldo, f, 1, flags, m_dev, 1, has_res_f32 ? f : nullptr,
                           ldaux > 0 ? dummy : nullptr, ldaux, nullptr, &q);
    if (flags & YV_EPI_OUT_MXFP8) return YV_ERR_ARG;               // as yv_linear_mxfp8 / yv_linear_mxfp8_ex
    return linear_mx_impl(dummy, lda, dummy, (M + 127) / 128 * 128LL, dummy, dummy, (N + 127) / 128 * 128LL, f, M, N, K, dummy, ldo,
                          flags, m_dev, 1, nullptr, 0, nullptr, 0, nullptr, has_res_f32 ? f : nullptr, ldaux > 0 ? dummy : nullptr,
                          ldaux, &q);
}

// yv_linear_mxfp8_q's checks and route on dummy bases: dense operands (lda = ldq = K / N bytes), scale rows rounded up to 128
extern "C" int yv_linear_mxfp8_q_route(int M, int N, int K, int flags, int n_cu, yv_linear_route_t* out) {
    static unsigned char dummy[16] __attribute__((aligned(16)));
    if (!out || M <= 0 || n_cu < 0) return YV_ERR_ARG;
    const LinearQuery q = {out, 0, persistent_cus(n_cu)};
    const int32_t* m_dev = (flags & YV_ROUTE_M_DEV) ? (const int32_t*)dummy : nullptr;
    flags &= ~YV_ROUTE_M_DEV;
    const long long rows_pad = (M + 127) / 128 * 128LL;
    if (!mx_q_args_ok(dummy, dummy, M, N, flags, N, rows_pad)) return YV_ERR_ARG;
    return linear_mx_impl(dummy, K, dummy, rows_pad, dummy, dummy, (N + 127) / 128 * 128LL, (const float*)dummy, M, N, K, dummy, N,
                          flags | YV_EPI_OUT_MXFP8, m_dev, 1, dummy, N, dummy, rows_pad, nullptr, nullptr, nullptr, 0, &q);
}

extern "C" int yv_linear_ln_route(int M, int N, int K, int flags, int n_cu, yv_linear_ln_route_t* out) {
    if (!out || M <= 0 || N <= 0 || K <= 0 || n_cu < 0) return YV_ERR_ARG;
    n_cu = persistent_cus(n_cu);
    if (!n_cu) return YV_ERR_LAUNCH;
    *out = yv_linear_ln_route_t{};
    if (linear_ln_fused(M, N, K, flags, n_cu)) {
        out->fused = 1; out->tiles_m = (M + 63) / 64; out->tiles_n = N >> 6; out->workgroups = out->tiles_m * out->tiles_n;
    }
    return YV_OK;
}

extern "C" int yv_linear_ln(const float* x, size_t ldx, const float* gamma, const float* beta, float eps, void* h, int ldh,
                            const void* w, const float* bias, void* out, int ldo, int M, int N, int K, int flags,
                            const int32_t* m_dev, int m_mul, void* stream) {
    if (!x || !gamma || !beta || !h || !w || !out || M < 0 || N <= 0 || K <= 0) return YV_ERR_ARG;
    if ((K & 63) || (N & 63) || (ldx & 3) || ldx < (size_t)K || (ldh & 7) || ldh < K || (ldo & 3) || ldo < N) return YV_ERR_ARG;
    if (flags & ~(YV_EPI_BIAS | YV_EPI_GELU | YV_EPI_OUT_F32)) return YV_ERR_ARG;
    if ((flags & YV_EPI_BIAS) && !bias) return YV_ERR_ARG;
    if (((uintptr_t)x | (uintptr_t)gamma | (uintptr_t)beta | (uintptr_t)h | (uintptr_t)w | (uintptr_t)out) & 15) return YV_ERR_ARG;
    if ((flags & YV_EPI_BIAS) && ((uintptr_t)bias & 15)) return YV_ERR_ARG;
    if (K > LN_MID_MAXK) return YV_ERR_LIMIT;
    if (M == 0) return YV_OK;
    const int n_cu = persistent_cus();
    if (!n_cu) return YV_ERR_LAUNCH;
    if (!linear_ln_fused(M, N, K, flags, n_cu)) {               // the pair, exactly the two launches of a caller without this entry
        const int rc = yv_layernorm(x, ldx, gamma, beta, M, K, eps, h, (size_t)ldh, m_dev, m_mul, stream);
        return rc != YV_OK ? rc : yv_linear(h, ldh, w, bias, M, N, K, out, ldo, nullptr, 0, flags, m_dev, m_mul, stream);
    }
    GemmArgs g = {};
    g.c0 = K;                                                   // (a0 stays null: the A operand lies behind LnOps)
    g.w = (const uint16_t*)w; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.out = out; g.ldo = ldo; g.flags = flags; g.m_dev = m_dev; g.m_mul = m_mul;
    g.ksize = 1; g.stride = 1; g.splitk = 1;
    g.group_m = g_opt_group_m > 0 ? g_opt_group_m : 8;
    const LnOps p = {x, (long long)ldx, gamma, beta, eps};
    return launch_mid_ln(g, p, (hipStream_t)stream);
}

// yv_conv2d_bnbwd: the BatchNorm block whose output gradient the convolution stores
struct BnBwdOps { const void* z; int ldz; const float *mean, *rstd, *gamma, *beta; int act; };

// The argument checks of one convolution launch and its GemmArgs (everything but the route): ONE text for conv_impl_one and for
// conv_group_partition, which checks every member of a group before anything is launched.
static int conv_args(const yv_view* in0, const yv_view* in1, int B, int Hout, int Wout, int ksize, int stride, const void* weight,
                     const float* bias, int Cout, void* out, int out_ld, const void* res, int res_ld, int flags, GemmArgs& g) {
    if (!in0 || !in0->ptr || !weight || !out || B <= 0 || Hout <= 0 || Wout <= 0 || Cout <= 0) return YV_ERR_ARG;
    if (!(ksize == 1 || ksize == 3) || !(stride == 1 || stride == 2)) return YV_ERR_ARG;
    if (in1 && in1->ptr && ksize != 1) return YV_ERR_ARG;
    const int c1 = (in1 && in1->ptr) ? in1->c : 0;
    const int Cin = in0->c + c1;
    if ((in0->c & 7) || (c1 & 7) || (in0->ld & 7) || (c1 && (in1->ld & 7)) || (Cout & 3) || (out_ld & 3))
        return YV_ERR_ARG;
    if ((flags & YV_EPI_BIAS) && !bias) return YV_ERR_ARG;
    if ((flags & YV_EPI_RES_BF16) && (!res || (res_ld & 3))) return YV_ERR_ARG;
    if (flags & (YV_EPI_GELU | YV_EPI_POSEMB | YV_EPI_RES_F32)) return YV_ERR_ARG;
    if ((long long)B * Hout * Wout > 0x7fffffffLL) return YV_ERR_LIMIT;
    if (ksize == 3 && in0->up) return YV_ERR_ARG;                 // the fused 2x upsample is a property of 1 x 1 (concat) inputs
    {   // the kernel addresses activations and weights with 32-bit byte offsets
        const long long px = (long long)B * Hout * stride * Wout * stride;
        // (+ one row and one pixel: the 3 x 3 descriptor starts that far before the tensor, see igemm_kernel)
        if ((px + Wout * stride + 1) * in0->ld * 2 >= 0x7fffffffLL || (c1 && px * in1->ld * 2 >= 0x7fffffffLL) ||
            (long long)Cout * ksize * ksize * Cin * 2 >= 0x7fffffffLL)
            return YV_ERR_LIMIT;
    }
    g = GemmArgs{};
    g.cin_shift = (Cin & (Cin - 1)) == 0 ? __builtin_ctz((unsigned)Cin) : -1;
    g.tap_uniform = (Cin % 64) == 0;
    g.a0 = (const uint16_t*)in0->ptr; g.lda0 = in0->ld; g.c0 = in0->c; g.up0 = in0->up;
    if (c1) { g.a1 = (const uint16_t*)in1->ptr; g.lda1 = in1->ld; g.c1 = c1; g.up1 = in1->up; }
    g.Hin = Hout * stride; g.Win = Wout * stride;
    g.Hout = Hout; g.Wout = Wout; g.ksize = ksize; g.stride = stride;
    g.w = (const uint16_t*)weight; g.bias = bias;
    g.M = B * Hout * Wout; g.N = Cout; g.K = ksize * ksize * Cin;
    g.out = out; g.ldo = out_ld; g.res = (const uint16_t*)res; g.ldres = res_ld; g.flags = flags;
    return YV_OK;
}

static int conv_impl_one(const yv_view* in0, const yv_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                         const void* weight, const float* bias, int Cout, void* out, int out_ld, const void* res,
                         int res_ld, int flags, void* ws, size_t ws_bytes, void* stream, bool query = false,
                         float* stats = nullptr /* yv_conv2d_stats / _bnbwd: the tile partials; never split-K */,
                         const BnBwdOps* bb = nullptr /* yv_conv2d_bnbwd: the sums are the BatchNorm backward's */,
                         bool trainer = false /* a query for the trainer's plain call, which never sets "conv_small" */) {
    GemmArgs g;
    const int rc = conv_args(in0, in1, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, res, res_ld, flags, g);
    if (rc != YV_OK) return rc;
    const int kern = conv_route(g, ws != nullptr && !stats, ws_bytes, stats != nullptr || bb != nullptr || trainer);
    if (query) return conv_instance_code(g, kern);                // yv_conv2d_instance: the route, no launch
    if (g.splitk > 1) g.partial = (float*)ws;
    g.stats = stats;
    if (bb) {
        g.z = (const uint16_t*)bb->z; g.ldz = bb->ldz; g.bn_act = bb->act;
        g.bn_mean = bb->mean; g.bn_rstd = bb->rstd; g.bn_gamma = bb->gamma; g.bn_beta = bb->beta;
    }
    return launch_conv(g, kern, (hipStream_t)stream);
}

// The kernel addresses each source with 32-bit byte offsets (< 2 GB): larger batches are taken in sub-batches, images being
// independent (e.g. the 48-channel C2f buffer of YOLOv8n at 320 x 320 passes 2 GB at 218 images).
static int conv_impl(const yv_view* in0, const yv_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                     const void* weight, const float* bias, int Cout, void* out, int out_ld, const void* res,
                     int res_ld, int flags, void* ws, size_t ws_bytes, void* stream, bool query = false) {
    if (!in0 || !in0->ptr || B <= 0 || Hout <= 0 || Wout <= 0 || !out)
        return conv_impl_one(in0, in1, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, res, res_ld, flags, ws, ws_bytes,
                             stream, query);
    const long long Hin = (long long)Hout * stride, Win = (long long)Wout * stride;
    const bool two = in1 && in1->ptr;
    const long long s0 = (Hin >> in0->up) * (Win >> in0->up) * in0->ld * 2;
    const long long s1 = two ? (Hin >> in1->up) * (Win >> in1->up) * in1->ld * 2 : 0;
    const long long nb = conv_sub_batch(s0, s1, (Win + 1) * in0->ld * 2);
    if (nb >= B)
        return conv_impl_one(in0, in1, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, res, res_ld, flags, ws, ws_bytes,
                             stream, query);
    if (nb < 1) return YV_ERR_LIMIT;                              // a single image beyond 2 GB
    const long long esz = (flags & YV_EPI_OUT_F32) ? 4 : 2;
    for (long long b0 = 0; b0 < B; b0 += nb) {
        const int n = (int)(B - b0 < nb ? B - b0 : nb);
        yv_view v0 = *in0, v1 = two ? *in1 : yv_view{};
        v0.ptr = (unsigned char*)in0->ptr + b0 * s0;
        if (two) v1.ptr = (unsigned char*)in1->ptr + b0 * s1;
        const int rc = conv_impl_one(&v0, two ? &v1 : nullptr, n, Hout, Wout, ksize, stride, weight, bias, Cout,
                                     (unsigned char*)out + b0 * Hout * Wout * out_ld * esz, out_ld,
                                     res ? (const unsigned char*)res + b0 * Hout * Wout * res_ld * 2 : nullptr, res_ld, flags, ws, ws_bytes,
                                     stream, query);
        if (rc != YV_OK || query) return rc;                       // a query reports the first sub-batch
    }
    return YV_OK;
}

extern "C" int yv_linear_nn(const void* A, int lda, const void* Wkn, int ldw, const float* bias, int M, int N, int K,
                            void* out, int ldo, int flags, void* aux, int ldaux, void* stream) {
    // out[M,N] = A[M,K] . Wkn[K,N] : the weight is read in its reduction-major layout (dgrad on the master layout)
    if (!A || !Wkn || !out || M <= 0 || N <= 0 || K <= 0) return YV_ERR_ARG;
    if ((K % BK) || (lda & 7) || (ldw & 7) || (N & 7) || (ldo & 7)) return YV_ERR_ARG;
    if (flags & ~(YV_EPI_BIAS | YV_EPI_GELU_BWD)) return YV_ERR_ARG;
    if ((flags & YV_EPI_BIAS) && !bias) return YV_ERR_ARG;
    if ((flags & YV_EPI_GELU_BWD) && !aux) return YV_ERR_ARG;
    if (((uintptr_t)A | (uintptr_t)Wkn | (uintptr_t)out) & 15) return YV_ERR_ARG;
    GemmArgs g = {};
    g.a0 = (const uint16_t*)A; g.lda0 = lda; g.c0 = K;
    g.w = (const uint16_t*)Wkn; g.ldw = ldw; g.bias = bias; g.M = M; g.N = N; g.K = K;
    g.out = out; g.ldo = ldo; g.flags = flags; g.aux = (uint16_t*)aux; g.ldaux = ldaux;
    g.ksize = 1; g.stride = 1; g.splitk = 1;
    g.staged = epi_can_stage(g);
    if (!g.staged) return YV_ERR_ARG;
    g.group_m = g_opt_group_m > 0 ? g_opt_group_m : 8;
    return launch_dma<128, 128, 2, 2, 0, true>(g, (hipStream_t)stream);
}

static bool wgrad_tile_ok(int tile_n) { return tile_n == 0 || tile_n == 32 || tile_n == 64 || tile_n == 128; }
static bool wgrad_shape_ok(int T, int N, int K) { return T > 0 && N > 0 && K > 0 && !((T & 63) || (N & 7) || (K & 7)); }
static bool wgrad_args_ok(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, const float* dW, int ldw) {
    if (!dY || !X || !dW || !wgrad_shape_ok(T, N, K) || (ldy & 7) || (ldx & 7) || (ldw & 3)) return false;
    return !(((uintptr_t)dY | (uintptr_t)X | (uintptr_t)dW) & 15);
}
// the split-K workspace registered for the stream (yv_set_workspace); none: no bytes
struct StreamWs { void* ptr = nullptr; size_t bytes = 0; };
static StreamWs stream_ws(void* stream) {
    StreamWs w;
    if (!ws_lookup(stream, &w.ptr, &w.bytes)) w.bytes = 0;
    return w;
}

// The instances of gemm_tn_body: tile_n of the route -> dynamic LDS bytes and kernel, plain and gather form (no wide gather form)
constexpr int TN_TILE[4] = {128, 64, 32, 256};
constexpr size_t TN_LDS[4] = {Tn128::LDS, TnNarrow<64>::LDS, TnNarrow<32>::LDS, TnWide::LDS};
static const void* const TN_KERNEL[2][4] = {
    {(const void*)gemm_tn_kernel, (const void*)gemm_tn_narrow_kernel<64>, (const void*)gemm_tn_narrow_kernel<32>, (const void*)gemm_tn_wide_kernel},
    {(const void*)gemm_tn_gather_kernel, (const void*)gemm_tn_narrow_gather_kernel<64>, (const void*)gemm_tn_narrow_gather_kernel<32>, nullptr}};

// Launches the route: no decisions.  ws: the workspace the route was told of.  q: the gather form (X lies behind q->x; seg_len = 0).
static int wgrad_launch(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, float* dW, int ldw, int seg_len,
                        long long seg_stride, const WgradRoute& r, void* ws, void* stream, const ConvGather* q = nullptr) {
    GemmArgs g = {};
    g.seg_len = seg_len; g.seg_stride = seg_stride;
    g.a0 = (const uint16_t*)dY; g.lda0 = ldy; g.w = (const uint16_t*)X; g.lda1 = ldx;
    g.M = N; g.N = K; g.K = T; g.out = dW; g.ldo = ldw; g.flags = YV_EPI_OUT_F32;
    g.tiles_m = (N + r.tile_n - 1) / r.tile_n; g.tiles_n = (K + r.tile_k - 1) / r.tile_k;
    g.splitk = r.slices;
    if (g.splitk > 1) g.partial = (float*)ws;
    int t = 0;
    while (t < 4 && TN_TILE[t] != r.tile_n) ++t;
    const void* kern = t < 4 ? TN_KERNEL[q != nullptr][t] : nullptr;
    if (!kern) return YV_ERR_ARG;                                 // no route names such a tile
    if (!yv_grant_lds(kern, TN_LDS[t])) return YV_ERR_LAUNCH;
    void* args[2] = {&g, (void*)q};
    hipLaunchKernel(kern, dim3(r.workgroups), dim3(256), args, TN_LDS[t], (hipStream_t)stream);
    return launch_splitk_reduce(g, (hipStream_t)stream);
}

static int wgrad_impl(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, float* dW, int ldw, int seg_len,
                      long long seg_stride, int tile_n, void* stream) {
    if (!wgrad_args_ok(dY, ldy, X, ldx, T, N, K, dW, ldw) || !wgrad_tile_ok(tile_n)) return YV_ERR_ARG;
    const StreamWs ws = stream_ws(stream);
    return wgrad_launch(dY, ldy, X, ldx, T, N, K, dW, ldw, seg_len, seg_stride, wgrad_route(T, N, K, tile_n, ws.bytes, 0), ws.ptr, stream);
}

extern "C" int yv_wgrad(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, float* dW, int ldw,
                        void* stream) {
    return wgrad_impl(dY, ldy, X, ldx, T, N, K, dW, ldw, 0, 0, 128, stream);
}

extern "C" int yv_wgrad_tiled(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, float* dW, int ldw,
                              int tile_n, void* stream) {
    return wgrad_impl(dY, ldy, X, ldx, T, N, K, dW, ldw, 0, 0, tile_n, stream);
}

extern "C" int yv_wgrad_route(int T, int N, int K, int tile_n, size_t ws_bytes, int n_cu, yv_wgrad_route_t* out) {
    if (!out || n_cu < 0 || !wgrad_shape_ok(T, N, K) || !wgrad_tile_ok(tile_n)) return YV_ERR_ARG;
    *out = wgrad_route(T, N, K, tile_n, ws_bytes, n_cu);
    return YV_OK;
}

extern "C" int yv_wgrad_wide(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, float* dW, int ldw, int mode,
                             void* stream) {
    if (!wgrad_args_ok(dY, ldy, X, ldx, T, N, K, dW, ldw) || (mode != 0 && mode != 1)) return YV_ERR_ARG;
    const StreamWs ws = stream_ws(stream);
    return wgrad_launch(dY, ldy, X, ldx, T, N, K, dW, ldw, 0, 0, wgrad_wide_route(T, N, K, mode, ws.bytes, 0), ws.ptr, stream);
}

extern "C" int yv_wgrad_wide_route(int T, int N, int K, int mode, size_t ws_bytes, int n_cu, yv_wgrad_route_t* out) {
    if (!out || n_cu < 0 || (mode != 0 && mode != 1) || !wgrad_shape_ok(T, N, K)) return YV_ERR_ARG;
    *out = wgrad_wide_route(T, N, K, mode, ws_bytes, n_cu);
    return YV_OK;
}

// 3x3 / stride 1 / pad 1 weight gradient without an im2col buffer.  Both operands are laid out over the PADDED pixel grid
// (B, H+2, W+2): there the tap (dy, dx) of pixel m is pixel m + dy * (W+2) + dx - a constant row offset - and, the
// activation being dense (row stride Cin), the three dx taps of one dy are 3*Cin CONSECUTIVE elements.  Column
// k = ((dy+1)*3 + dx+1)*Cin + ci of the virtual (T, 9*Cin) operand therefore sits at
//   Xp + (m - pitch - 1) * Cin + (k / 3Cin) * pitch * Cin + k % 3Cin,       pitch = W + 2,
// which is what gemm_tn's segment addressing reads.  dYp must be ZERO on the padding ring and on the tail rows; the
// activation ring must be zero too, and pitch + 1 readable rows of finite values must surround the activation.
extern "C" int yv_wgrad_conv3(const void* dYp, int ldy, const void* Xp, int Cin, int pitch, int T, int N, float* dW, int ldw,
                              void* stream) {
    return yv_wgrad_conv3_tiled(dYp, ldy, Xp, Cin, pitch, T, N, dW, ldw, 128, stream);
}

extern "C" int yv_wgrad_conv3_tiled(const void* dYp, int ldy, const void* Xp, int Cin, int pitch, int T, int N, float* dW, int ldw,
                                    int tile_n, void* stream) {
    if (!Xp || Cin < 8 || (Cin & 7) || pitch < 3) return YV_ERR_ARG;
    const uint16_t* base = (const uint16_t*)Xp - (long long)(pitch + 1) * Cin;
    return wgrad_impl(dYp, ldy, base, Cin, T, N, 9 * Cin, dW, ldw, 3 * Cin, (long long)pitch * Cin, tile_n, stream);
}

// 3x3 / pad 1 / stride 1 or 2 weight gradient with no operand copy at all: the gather form of the kernels above reads dY and x in
// place.  The route is wgrad_route's for (r64(T), N, 9 * Cin): the same tiles and slices as yv_im2col3 + yv_wgrad_tiled, hence the
// same bits.  `use`: 0 where the per-layer measurement had the gather form slower; it was faster on all seven stride-2 layers of
// YOLOv8s and YOLOv8n at 16 x 640^2 with either tile (x 0.53 - 0.94, profiles/wgrad_gather_layers.txt), so 1 everywhere
// (DESIGN.md section 26).
static bool gather_grid_ok(int B, int Hin, int Win, int stride, int Cin, int N, int tile_n) {
    if (B <= 0 || Hin <= 0 || Win <= 0 || !(stride == 1 || stride == 2) || Cin < 8 || !wgrad_tile_ok(tile_n)) return false;
    const long long T = (long long)B * ((Hin - 1) / stride + 1) * ((Win - 1) / stride + 1);
    if (T > (1LL << 31) - 64 || 9LL * Cin >= (1LL << 31)) return false;
    return wgrad_shape_ok((int)((T + 63) & ~63LL), N, 9 * Cin);      // 9 * Cin % 8 == 0: Cin % 8 == 0
}

extern "C" int yv_wgrad_conv3_gather_route(int B, int Hin, int Win, int stride, int Cin, int N, int tile_n, size_t ws_bytes, int n_cu,
                                           yv_wgrad_route_t* gemm, int* use) {
    if (!gemm || !use || n_cu < 0 || !gather_grid_ok(B, Hin, Win, stride, Cin, N, tile_n)) return YV_ERR_ARG;
    const ConvGather q = conv_gather_of(nullptr, Cin, B, Hin, Win, stride, Cin);
    *gemm = wgrad_route((q.T + 63) & ~63, N, 9 * Cin, tile_n, ws_bytes, n_cu);
    *use = 1;
    return YV_OK;
}

extern "C" int yv_wgrad_conv3_gather_src(int B, int Hin, int Win, int stride, int m, int tap, long long* pixel) {
    if (!pixel || m < 0 || tap < 0 || tap > 8 || !gather_grid_ok(B, Hin, Win, stride, 8, 8, 0)) return YV_ERR_ARG;
    *pixel = conv_gather_pixel(conv_gather_of(nullptr, 8, B, Hin, Win, stride, 8), m, tap / 3, tap % 3);
    return YV_OK;
}

extern "C" int yv_wgrad_conv3_gather(const void* dY, int ldy, const void* X, long long ldx, int B, int Hin, int Win, int stride,
                                     int Cin, int N, float* dW, int ldw, int tile_n, void* stream) {
    if (!dY || !X || !dW || !gather_grid_ok(B, Hin, Win, stride, Cin, N, tile_n)) return YV_ERR_ARG;
    if ((ldy & 7) || ldy < N || (ldx & 7) || ldx < Cin || (ldw & 3) || ldw < 9 * Cin) return YV_ERR_ARG;
    if (((uintptr_t)dY | (uintptr_t)X | (uintptr_t)dW) & 15) return YV_ERR_ARG;
    const ConvGather q = conv_gather_of(X, ldx, B, Hin, Win, stride, Cin);
    const int T = (q.T + 63) & ~63, K = 9 * Cin;
    const StreamWs ws = stream_ws(stream);
    return wgrad_launch(dY, ldy, nullptr, 0, T, N, K, dW, ldw, 0, 0, wgrad_route(T, N, K, tile_n, ws.bytes, 0), ws.ptr, stream, &q);
}

extern "C" int yv_conv2d(const yv_view* in0, const yv_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                         const void* weight, const float* bias, int Cout, void* out, int out_ld, const void* res,
                         int res_ld, int flags, void* stream) {
    return conv_impl(in0, in1, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, res, res_ld, flags, nullptr, 0,
                     stream);
}

extern "C" int yv_conv2d_ws(const yv_view* in0, const yv_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                            const void* weight, const float* bias, int Cout, void* out, int out_ld, const void* res,
                            int res_ld, int flags, void* ws, size_t ws_bytes, void* stream) {
    return conv_impl(in0, in1, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, res, res_ld, flags, ws, ws_bytes,
                     stream);
}

extern "C" int yv_conv2d_stats(const yv_view* in0, int B, int Hout, int Wout, int ksize, int stride, const void* weight,
                               const float* bias, int Cout, void* out, int out_ld, int flags, float* stats_ws, size_t stats_ws_floats,
                               void* ws, size_t ws_bytes, void* stream) {
    if (!stats_ws || (flags & ~YV_EPI_BIAS) || Cout <= 0 || (Cout & 7)) return YV_ERR_ARG;
    // the argument checks of yv_conv2d_ws, by its route query: nothing is launched
    const int code = conv_impl_one(in0, nullptr, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, nullptr, 0, flags, ws,
                                   ws_bytes, stream, true, stats_ws);
    if (code < 0) return code;
    {   // one launch, one tile sequence: not what yv_conv2d_ws takes in sub-batches
        const long long Hin = (long long)Hout * stride, Win = (long long)Wout * stride;
        const long long s0 = (Hin >> in0->up) * (Win >> in0->up) * in0->ld * 2;
        if (conv_sub_batch(s0, 0, (Win + 1) * in0->ld * 2) < B) return YV_ERR_LIMIT;
    }
    if (stats_ws_floats < yv_conv_stats_ws_floats((long long)B * Hout * Wout, Cout)) return YV_ERR_WORKSPACE;
    return conv_impl_one(in0, nullptr, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, nullptr, 0, flags, ws, ws_bytes,
                         stream, false, stats_ws);
}

// One launch, one tile sequence: false where yv_conv2d_ws would take the batch in sub-batches
static bool conv_one_batch(const yv_view* in0, int B, int Hout, int Wout, int stride) {
    const long long Hin = (long long)Hout * stride, Win = (long long)Wout * stride;
    const long long s0 = (Hin >> in0->up) * (Win >> in0->up) * in0->ld * 2;
    return conv_sub_batch(s0, 0, (Win + 1) * in0->ld * 2) >= B;
}

extern "C" int yv_conv2d_bnbwd(const yv_view* in0, int B, int Hout, int Wout, int ksize, int stride, const void* weight,
                               const float* bias, int Cout, void* out, int out_ld, const void* res, int res_ld, int flags,
                               const void* z, int ldz, const float* mean, const float* rstd, const float* gamma, const float* beta,
                               int act, float* stats_ws, size_t stats_ws_floats, void* ws, size_t ws_bytes, void* stream) {
    if (!stats_ws || !z || !mean || !rstd || !gamma || !beta || (flags & ~(YV_EPI_BIAS | YV_EPI_RES_BF16)) || Cout <= 0 || (Cout & 7))
        return YV_ERR_ARG;
    if ((ldz & 7) || ldz < Cout || (act & ~1)) return YV_ERR_ARG;
    if (((uintptr_t)z | (uintptr_t)out | (uintptr_t)res | (uintptr_t)stats_ws | (uintptr_t)mean | (uintptr_t)rstd | (uintptr_t)gamma |
         (uintptr_t)beta) & 15)
        return YV_ERR_ARG;
    // the argument checks of yv_conv2d_ws, by its route query: nothing is launched
    const int code = conv_impl_one(in0, nullptr, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, res, res_ld, flags, ws,
                                   ws_bytes, stream, true, stats_ws);
    if (code < 0) return code;
    if (!conv_one_batch(in0, B, Hout, Wout, stride)) return YV_ERR_LIMIT;
    if (stats_ws_floats < yv_conv_bnbwd_ws_floats((long long)B * Hout * Wout, Cout)) return YV_ERR_WORKSPACE;
    const BnBwdOps bb = {z, ldz, mean, rstd, gamma, beta, act};
    return conv_impl_one(in0, nullptr, B, Hout, Wout, ksize, stride, weight, bias, Cout, out, out_ld, res, res_ld, flags, ws, ws_bytes,
                         stream, false, stats_ws, &bb);
}

extern "C" int yv_conv2d_bnbwd_route(int B, int Hout, int Wout, int ksize, int stride, int Cin, int in_ld, int Cout, int out_ld,
                                     int res_ld, int ldz, int flags, size_t ws_bytes, yv_conv_bnbwd_route_t* route) {
    // 16-byte aligned bases; nothing is dereferenced or launched
    static unsigned char dummy[16] __attribute__((aligned(16)));
    if (!route || Cin <= 0 || (flags & ~(YV_EPI_BIAS | YV_EPI_RES_BF16)) || Cout <= 0 || (Cout & 7) || (ldz & 7) || ldz < Cout)
        return YV_ERR_ARG;
    const yv_view v = {dummy, in_ld, Cin, 0};
    const void* res = (flags & YV_EPI_RES_BF16) ? dummy : nullptr;
    const int own = conv_impl_one(&v, nullptr, B, Hout, Wout, ksize, stride, dummy, (const float*)dummy, Cout, dummy, out_ld, res, res_ld,
                                  flags, ws_bytes ? dummy : nullptr, ws_bytes, nullptr, true, (float*)dummy);
    if (own < 0) return own;
    if (!conv_one_batch(&v, B, Hout, Wout, stride)) return YV_ERR_LIMIT;
    // (the unfused call is the trainer's, which never sets "conv_small": its route is asked with the step absent)
    const int plain = conv_impl_one(&v, nullptr, B, Hout, Wout, ksize, stride, dummy, (const float*)dummy, Cout, dummy, out_ld, res,
                                    res_ld, flags, ws_bytes ? dummy : nullptr, ws_bytes, nullptr, true, nullptr, nullptr, true);
    if (plain < 0) return plain;
    const int kern = own & 15, bn = (kern == CK_IGEMM_128 || kern >= CK_CDMA_128_2) ? 128 : (kern == CK_IGEMM_32 ? 32 : (kern == CK_IGEMM_16 ? 16 : 64));
    const long long tiles = ((long long)B * Hout * Wout + 127) / 128;
    route->kernel = kern;
    route->staged = (own & 16) != 0;
    route->tiles = (int)tiles;
    route->workgroups = (int)(tiles * ((Cout + bn - 1) / bn));
    route->splitk = (plain & 32) != 0;
    // use: 0 where the unfused call splits K (its bits differ from a one-pass convolution's), and 0 where the per-pair measurement
    // (profiles/bn_bwd_fused_layers.txt, DESIGN.md section 27: YOLOv8s and YOLOv8n at 16 x 640^2) had the fused pair slower than
    // conv + bn_act_bwd by more than the spread of its rounds: there the z read and the terms at the end of every tile cost more
    // than the pass over da and z they replace.  That is (a) every 64- and 128-wide instance on the large maps (>= 100 k rows, the
    // 80 x 80 maps and above: x 1.06 - 1.13, the 128-wide igemm tile, which loses a workgroup per CU, x 1.42), and (b) the 32-wide
    // tile on >= 400 k rows with K >= 512 (the two 3 x 3 gradients from 64 channels: x 1.06 and x 1.01).  Every pair below 100 k
    // rows and every 16-wide one was faster (x 0.53 - 0.97).
    const long long M = (long long)B * Hout * Wout;
    const int K = ksize * ksize * Cin;
    const bool slow = (kern >= CK_IGEMM_64 && M >= 100000) || (kern == CK_IGEMM_32 && M >= 400000 && K >= 512);
    route->use = !route->splitk && !slow;
    return YV_OK;
}

extern "C" int yv_conv2d_instance(int B, int Hout, int Wout, int ksize, int stride, int c0, int c1, int Cout, int out_ld,
                                  int res_ld, int flags, size_t ws_bytes) {
    // dense sources (pixel stride = channels read) at 16-byte aligned bases; nothing is dereferenced or launched
    static unsigned char dummy[16] __attribute__((aligned(16)));
    if (c0 <= 0 || c1 < 0) return YV_ERR_ARG;
    const yv_view v0 = {dummy, c0, c0, 0}, v1 = {dummy, c1, c1, 0};
    return conv_impl(&v0, c1 ? &v1 : nullptr, B, Hout, Wout, ksize, stride, dummy, (const float*)dummy, Cout, dummy, out_ld,
                     (flags & YV_EPI_RES_BF16) ? dummy : nullptr, res_ld, flags, ws_bytes ? dummy : nullptr, ws_bytes, nullptr, true);
}

// ------------------------------------------------------------------------------------------------ grouped convolution launch
// (kernels and their contract: the comment at cgemm_dma_group_kernel)
struct GroupMember {
    GemmArgs g;                     // routed; tiles_m / tiles_n those of its instance where it is eligible
    int kern;                       // ConvKern, -1: a call conv_impl takes in sub-batches
    bool eligible;
    yv_conv2d_group_plan_t plan;
};
struct GroupLaunch { int kern; std::vector<int> members; };     // members: indices into the call's array, in grid order

static int group_tile_rows(int kern) { return kern == CK_CDMA_64_3 ? 128 : (kern == CK_SMALL_64 ? 64 : 32); }

// The partition of a group: ONE rule for yv_conv2d_group (which launches it) and yv_conv2d_group_plan (which reports it).  Checks
// every member (conv_args, the 2 GB limits), routes it as yv_conv2d would alone (conv_route without a workspace), then: the
// eligible members per instance by descending work (tiles x K steps, as yv_conv2d_dgrad_s2 orders its phases; ties in the order
// given), YV_CONV_GROUP_MAX to a launch, each member's first workgroup rounded up to a multiple of 8; the others one launch each.
// query: a plan on dummy pointers - the outputs are taken to be distinct.
static int conv_group_partition(const yv_conv2d_desc* d, int n, bool query, std::vector<GroupMember>& ms, std::vector<GroupLaunch>& launches) {
    if (!d || n <= 0) return YV_ERR_ARG;
    ms.assign((size_t)n, GroupMember{});
    launches.clear();
    for (int i = 0; i < n; ++i) {
        const yv_conv2d_desc& m = d[i];
        GroupMember& x = ms[i];
        const yv_view* in1 = m.in1.ptr ? &m.in1 : nullptr;
        const int rc = conv_args(&m.in0, in1, m.B, m.Hout, m.Wout, m.ksize, m.stride, m.weight, m.bias, m.Cout, m.out, m.out_ld, m.res,
                                 m.res_ld, m.flags, x.g);
        if (rc != YV_OK) return rc;
        const long long Hin = (long long)m.Hout * m.stride, Win = (long long)m.Wout * m.stride;
        const long long s0 = (Hin >> m.in0.up) * (Win >> m.in0.up) * m.in0.ld * 2;
        const long long s1 = in1 ? (Hin >> in1->up) * (Win >> in1->up) * in1->ld * 2 : 0;
        const long long nb = conv_sub_batch(s0, s1, (Win + 1) * m.in0.ld * 2);
        if (nb < 1) return YV_ERR_LIMIT;
        if (nb < m.B) {                                           // sub-batches: conv_impl's loop, the first one's route reported
            x.kern = -1;
            x.plan.instance = conv_impl(&m.in0, in1, m.B, m.Hout, m.Wout, m.ksize, m.stride, m.weight, m.bias, m.Cout, m.out, m.out_ld,
                                        m.res, m.res_ld, m.flags, nullptr, 0, nullptr, true);
            if (x.plan.instance < 0) return x.plan.instance;
            continue;
        }
        x.kern = conv_route(x.g, false, 0, false);
        x.plan.instance = conv_instance_code(x.g, x.kern);
        x.eligible = x.kern == CK_CDMA_64_3 || x.kern == CK_SMALL_64 || x.kern == CK_SMALL_32;
        if (x.eligible) {
            const int rows = group_tile_rows(x.kern);
            x.g.tiles_m = (x.g.M + rows - 1) / rows;
            x.g.tiles_n = (x.g.N + 63) / 64;
            const long long work = (long long)x.g.tiles_m * x.g.tiles_n * (x.g.K / BK);
            x.plan.work = (int)(work < 0x7fffffffLL ? work : 0x7fffffffLL);
        }
    }
    if (!query)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < i; ++j)
                if (d[i].out == d[j].out) return YV_ERR_ARG;
    for (const int kern : {(int)CK_CDMA_64_3, (int)CK_SMALL_64, (int)CK_SMALL_32}) {
        std::vector<int> idx;
        for (int i = 0; i < n; ++i)
            if (ms[i].eligible && ms[i].kern == kern) idx.push_back(i);
        std::stable_sort(idx.begin(), idx.end(), [&](int a, int b) { return ms[a].plan.work > ms[b].plan.work; });
        for (size_t at = 0; at < idx.size(); at += YV_CONV_GROUP_MAX) {
            const size_t end = at + YV_CONV_GROUP_MAX < idx.size() ? at + YV_CONV_GROUP_MAX : idx.size();
            long long first = 0;
            for (size_t k = at; k < end; ++k) {
                GroupMember& x = ms[idx[k]];
                x.plan.launch = (int)launches.size();
                x.plan.position = (int)(k - at);
                x.plan.first_wg = (int)first;
                first = (first + (long long)x.g.tiles_m * x.g.tiles_n + 7) & ~7LL;
                if (first > 0x7fffffffLL) return YV_ERR_LIMIT;
            }
            launches.push_back(GroupLaunch{kern, std::vector<int>(idx.begin() + at, idx.begin() + end)});
        }
    }
    for (int i = 0; i < n; ++i)
        if (!ms[i].eligible) {
            ms[i].plan.launch = (int)launches.size();
            launches.push_back(GroupLaunch{ms[i].kern, std::vector<int>(1, i)});
        }
    return YV_OK;
}

static int launch_conv_group(int kern, const ConvGroupArgs& p, hipStream_t st) {
    void (*k)(ConvGroupArgs) = cgemm_dma_group_kernel<64, 4, 1, 3>;
    unsigned threads = 256;
    size_t lds = 3 * (size_t)(128 + 64) * 128;                    // (launch_cdma<64, 4, 1, 3>'s)
    if (kern == CK_SMALL_64) { k = cgemm_small_group_kernel<64, 2>; threads = 512; lds = 2 * 2 * (size_t)(64 + 64) * 128; }
    if (kern == CK_SMALL_32) { k = cgemm_small_group_kernel<32, 4>; threads = 512; lds = 4 * 2 * (size_t)(32 + 64) * 128; }
    if (!yv_grant_lds((const void*)k, lds)) return YV_ERR_LAUNCH;
    launch_timed(k, (unsigned)p.first[p.n], threads, lds, st, p);
    return yv_launch_status();
}

extern "C" int yv_conv2d_group(const yv_conv2d_desc* d, int n, void* stream) {
    std::vector<GroupMember> ms;
    std::vector<GroupLaunch> launches;
    int rc = conv_group_partition(d, n, false, ms, launches);
    for (size_t l = 0; rc == YV_OK && l < launches.size(); ++l) {
        const GroupLaunch& L = launches[l];
        if (L.members.size() == 1) {
            const yv_conv2d_desc& m = d[L.members[0]];
            GroupMember& x = ms[L.members[0]];
            rc = x.kern >= 0 ? launch_conv(x.g, x.kern, (hipStream_t)stream)
                             : conv_impl(&m.in0, m.in1.ptr ? &m.in1 : nullptr, m.B, m.Hout, m.Wout, m.ksize, m.stride, m.weight, m.bias,
                                         m.Cout, m.out, m.out_ld, m.res, m.res_ld, m.flags, nullptr, 0, stream);
            continue;
        }
        ConvGroupArgs p = {};
        p.n = (int)L.members.size();
        for (int k = 0; k < p.n; ++k) {
            const GroupMember& x = ms[L.members[k]];
            p.m[k] = x.g;
            p.first[k] = x.plan.first_wg;
            p.first[k + 1] = x.plan.first_wg + x.g.tiles_m * x.g.tiles_n;      // (the last one: the grid)
        }
        rc = launch_conv_group(L.kern, p, (hipStream_t)stream);
    }
    return rc;
}

extern "C" int yv_conv2d_group_plan(const yv_conv2d_shape* shapes, int n, yv_conv2d_group_plan_t* out, int* n_launches) {
    // dense sources at 16-byte aligned bases, as yv_conv2d_instance; nothing is dereferenced or launched
    static unsigned char dummy[16] __attribute__((aligned(16)));
    if (!shapes || !out || !n_launches || n <= 0) return YV_ERR_ARG;
    std::vector<yv_conv2d_desc> d((size_t)n);
    for (int i = 0; i < n; ++i) {
        const yv_conv2d_shape& s = shapes[i];
        if (s.c0 <= 0 || s.c1 < 0) return YV_ERR_ARG;
        d[i] = yv_conv2d_desc{{dummy, s.c0, s.c0, 0}, {s.c1 ? dummy : nullptr, s.c1, s.c1, 0}, s.B, s.Hout, s.Wout, s.ksize, s.stride,
                              dummy, (const float*)dummy, s.Cout, dummy, s.out_ld, (s.flags & YV_EPI_RES_BF16) ? dummy : nullptr,
                              s.res_ld, s.flags};
    }
    std::vector<GroupMember> ms;
    std::vector<GroupLaunch> launches;
    const int rc = conv_group_partition(d.data(), n, true, ms, launches);
    if (rc != YV_OK) return rc;
    for (int i = 0; i < n; ++i) out[i] = ms[i].plan;
    *n_launches = (int)launches.size();
    return YV_OK;
}

// ---------------------------------------------------------------------------------------------------- stride-2 data gradient by phase
// One sub-batch (sources below 2 GB).  route != nullptr: report, launch nothing.
static int dgrad_s2_one(const yv_view* dz, int B, int Hout, int Wout, const void* wd, int Cin, int Cout, void* dx, int dx_ld,
                        const void* res, int res_ld, void* stream, yv_dgrad_s2_route_t* route) {
    GemmArgs g = {};
    g.cin_shift = (Cout & (Cout - 1)) == 0 ? __builtin_ctz((unsigned)Cout) : -1;
    g.tap_uniform = 1;
    g.a0 = (const uint16_t*)dz->ptr; g.lda0 = dz->ld; g.c0 = Cout;
    g.Hin = Hout; g.Win = Wout; g.Hout = Hout; g.Wout = Wout; g.ksize = 3; g.stride = 1;       // the source grid (see phase_step)
    g.w = (const uint16_t*)wd;
    g.M = B * Hout * Wout; g.N = Cin; g.K = 9 * Cout;
    g.out = dx; g.ldo = dx_ld; g.res = (const uint16_t*)res; g.ldres = res_ld; g.flags = res ? YV_EPI_RES_BF16 : 0;
    const int kern = dgrad_s2_route(g);
    if (route) {
        const int bn = kern == CK_CDMA_128_2 || kern == CK_IGEMM_128 ? 128 : (kern == CK_IGEMM_32 ? 32 : (kern == CK_IGEMM_16 ? 16 : 64));
        route->kernel = kern;
        route->staged = g.staged && kern >= CK_IGEMM_64;
        for (int q = 0; q < 4; ++q) route->ksteps[q] = (q == 0 ? 4 : (q == 3 ? 1 : 2)) * (Cout / BK);
        route->tiles = ((g.M + 127) / 128) * ((g.N + bn - 1) / bn);
        route->workgroups = 4 * route->tiles;
        route->use = 1;
        return YV_OK;
    }
    return launch_dgrad_s2(g, kern, (hipStream_t)stream);
}

static int dgrad_s2_impl(const yv_view* dz, int B, int Hout, int Wout, const void* wd, int Cin, int Cout, void* dx, int dx_ld,
                         const void* res, int res_ld, void* stream, yv_dgrad_s2_route_t* route) {
    if (!dz || !dz->ptr || !wd || !dx || B <= 0 || Hout <= 0 || Wout <= 0 || Cin <= 0 || Cout <= 0) return YV_ERR_ARG;
    if ((Cout % 64) || (Cin & 7) || dz->c != Cout || dz->up || dz->ld < Cout || (dz->ld & 7) || dx_ld < Cin || (dx_ld & 7) ||
        (res && (res_ld < Cin || (res_ld & 7))))
        return YV_ERR_ARG;
    if (((uintptr_t)dz->ptr | (uintptr_t)wd | (uintptr_t)dx | (uintptr_t)res) & 15) return YV_ERR_ARG;
    if (4LL * B * Hout * Wout > 0x7fffffffLL || 9LL * Cin * Cout * 2 >= 0x7fffffffLL) return YV_ERR_LIMIT;
    // 32-bit byte offsets into the gradient: sub-batches as conv_impl takes them (lead: the + 1 row / + 1 pixel displacement)
    const long long s0 = (long long)Hout * Wout * dz->ld * 2;
    const long long nb = conv_sub_batch(s0, 0, (long long)(Wout + 1) * dz->ld * 2);
    if (nb < 1) return YV_ERR_LIMIT;
    if (nb >= B || route) return dgrad_s2_one(dz, (int)(nb < B ? nb : B), Hout, Wout, wd, Cin, Cout, dx, dx_ld, res, res_ld, stream, route);
    for (long long b0 = 0; b0 < B; b0 += nb) {
        const int n = (int)(B - b0 < nb ? B - b0 : nb);
        yv_view v = *dz;
        v.ptr = (unsigned char*)dz->ptr + b0 * s0;
        const long long opix = b0 * 4 * Hout * Wout;
        const int rc = dgrad_s2_one(&v, n, Hout, Wout, wd, Cin, Cout, (unsigned char*)dx + opix * dx_ld * 2, dx_ld,
                                    res ? (const unsigned char*)res + opix * res_ld * 2 : nullptr, res_ld, stream, nullptr);
        if (rc != YV_OK) return rc;
    }
    return YV_OK;
}

extern "C" int yv_conv2d_dgrad_s2(const yv_view* dz, int B, int Hout, int Wout, const void* wd, int Cin, int Cout, void* dx, int dx_ld,
                                  const void* res, int res_ld, void* ws, size_t ws_bytes, void* stream) {
    (void)ws; (void)ws_bytes;                                     // no route splits K
    return dgrad_s2_impl(dz, B, Hout, Wout, wd, Cin, Cout, dx, dx_ld, res, res_ld, stream, nullptr);
}

extern "C" int yv_conv2d_dgrad_s2_route(int B, int Hin, int Win, int ksize, int Cin, int Cout, int dz_ld, int dx_ld, int res_ld,
                                        yv_dgrad_s2_route_t* out) {
    // 16-byte aligned bases; nothing is dereferenced or launched
    static unsigned char dummy[16] __attribute__((aligned(16)));
    if (!out || ksize != 3 || Hin <= 0 || Win <= 0 || (Hin & 1) || (Win & 1)) return YV_ERR_ARG;
    const yv_view v = {dummy, dz_ld, Cout, 0};
    return dgrad_s2_impl(&v, B, Hin / 2, Win / 2, dummy, Cin, Cout, dummy, dx_ld, res_ld > 0 ? dummy : nullptr, res_ld, nullptr, out);
}

// ---------------------------------------------------------------------------------------------------- MXFP8 convolutions
extern "C" int yv_quant_mxfp8_map(const void* x, long long ldx, long long pixels, int C, void* q, long long ldq, void* scales,
                                  void* stream) {
    if (!x || !q || !scales || pixels < 0 || C <= 0 || (C & 31) || (ldx & 7) || (ldq & 31) || ldx < C || ldq < C) return YV_ERR_ARG;
    if (((uintptr_t)x | (uintptr_t)q) & 15) return YV_ERR_ARG;
    if (pixels == 0) return YV_OK;
    const long long items = pixels * (C >> 5);
    hipLaunchKernelGGL(quant_mx_map_kernel, dim3((unsigned)((items + 255) / 256)), dim3(256), 0, (hipStream_t)stream,
                       (const uint16_t*)x, ldx, pixels, C, (uint8_t*)q, ldq, (uint8_t*)scales);
    return yv_launch_status();
}

// instance of cgemm_mx_kernel for M output pixels, N output channels: the rule of the bf16 kernel (conv_dma 8) - 128-wide
// tiles for the layers of the large maps (>= 100 k output pixels) with more than 64 output channels, else 64-wide
static int conv_mx_pick(long long M, int N) { return large_map_wide(M, N) ? 1 : 0; }

static int conv_mx_impl_one(const yv_mx_view* in0, const yv_mx_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                            const void* wq, const void* wscale, long long w_rows_pad, const float* bias, int Cout,
                            void* out, int out_ld, void* out_q, void* out_s, int outq_ld, const void* res, int res_ld,
                            int flags, void* stream) {
    const bool two = in1 && in1->q;
    const int c1 = two ? in1->c : 0;
    const int Cin = in0->c + c1;
    const long long kpad = ((long long)ksize * ksize * Cin + 127) / 128 * 128;
    {   // 32-bit byte offsets: each source (+ one row and one pixel before it, 3 x 3) and the weights
        const long long px = (long long)B * Hout * stride * Wout * stride;
        if ((px + Wout * stride + 1) * in0->ld >= 0x7fffffffLL || (two && px * in1->ld >= 0x7fffffffLL) ||
            (long long)Cout * kpad >= 0x7fffffffLL)
            return YV_ERR_LIMIT;
    }
    ConvMxArgs a = {};
    GemmArgs& g = a.g;
    g.a0 = (const uint16_t*)in0->q; g.lda0 = in0->ld; g.c0 = in0->c; g.up0 = in0->up;
    a.s0 = (const uint8_t*)in0->s;
    if (two) { g.a1 = (const uint16_t*)in1->q; g.lda1 = in1->ld; g.c1 = c1; g.up1 = in1->up; a.s1 = (const uint8_t*)in1->s; }
    g.Hin = Hout * stride; g.Win = Wout * stride;
    g.Hout = Hout; g.Wout = Wout; g.ksize = ksize; g.stride = stride;
    g.w = (const uint16_t*)wq; g.bias = bias;
    g.M = B * Hout * Wout; g.N = Cout; g.K = (int)kpad;
    g.out = out; g.ldo = out ? out_ld : 8; g.res = (const uint16_t*)res; g.ldres = res_ld; g.flags = flags;
    g.splitk = 1;
    // (the MX-map epilogue is always the staged one: "staged_epilogue" = 0 only switches the bf16 / f32-only launches)
    g.staged = (g_opt_staged || out_q) && epi_can_stage(g);
    if (out_q && !g.staged) return YV_ERR_ARG;
    a.kreal = ksize * ksize * Cin;
    a.sw = (const uint8_t*)wscale; a.rows_w = w_rows_pad;
    a.oq = (uint8_t*)out_q; a.os = (uint8_t*)out_s; a.ldq = outq_ld;
    const hipStream_t st = (hipStream_t)stream;
    if (conv_mx_pick(g.M, Cout) == 1)
        return launch_cmx<128, 2, 2>(a, st);
    return launch_cmx<64, 4, 1>(a, st);
}

static int conv_mx_check(const yv_mx_view* in0, const yv_mx_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                         int Cout) {
    if (!in0 || !in0->q || !in0->s || B <= 0 || Hout <= 0 || Wout <= 0 || Cout <= 0 || (Cout & 31)) return YV_ERR_ARG;
    if (!(ksize == 1 || ksize == 3) || !(stride == 1 || stride == 2)) return YV_ERR_ARG;
    const bool two = in1 && in1->q;
    if (two && (ksize != 1 || !in1->s)) return YV_ERR_ARG;
    if (ksize == 3 && in0->up) return YV_ERR_ARG;                 // the fused 2x upsample is a property of 1 x 1 inputs
    if (in0->c <= 0 || (in0->c & 31) || (in0->ld & 31) || in0->ld < in0->c || (in0->up & ~1) || ((uintptr_t)in0->q & 15))
        return YV_ERR_ARG;
    if (two && (in1->c <= 0 || (in1->c & 31) || (in1->ld & 31) || in1->ld < in1->c || (in1->up & ~1) || ((uintptr_t)in1->q & 15)))
        return YV_ERR_ARG;
    if ((long long)B * Hout * Wout > 0x7fffffffLL) return YV_ERR_LIMIT;
    return YV_OK;
}

extern "C" int yv_conv2d_mxfp8(const yv_mx_view* in0, const yv_mx_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                               const void* wq, const void* wscale, long long w_rows_pad, const float* bias, int Cout,
                               void* out_bf16, int out_ld, void* out_q, void* out_scales, int outq_ld, const void* res,
                               int res_ld, int flags, void* stream) {
    int rc = conv_mx_check(in0, in1, B, Hout, Wout, ksize, stride, Cout);
    if (rc != YV_OK) return rc;
    if (!wq || !wscale || w_rows_pad < Cout || (!out_bf16 && !out_q)) return YV_ERR_ARG;
    if (flags & ~(YV_EPI_BIAS | YV_EPI_SILU | YV_EPI_RES_BF16 | YV_EPI_OUT_F32)) return YV_ERR_ARG;
    if ((flags & YV_EPI_BIAS) && !bias) return YV_ERR_ARG;
    if ((flags & YV_EPI_RES_BF16) && (!res || (res_ld & 7) || ((uintptr_t)res & 15))) return YV_ERR_ARG;
    if ((flags & YV_EPI_OUT_F32) && (!out_bf16 || out_q)) return YV_ERR_ARG;
    if (out_bf16 && ((out_ld & 3) || out_ld < Cout)) return YV_ERR_ARG;
    if (out_q && (!out_scales || (outq_ld & 31) || outq_ld < Cout || ((uintptr_t)out_q & 15))) return YV_ERR_ARG;
    if (((uintptr_t)wq & 15)) return YV_ERR_ARG;
    // sub-batches keep each source below 2 GB (images are independent), as yv_conv2d
    const long long Hin = (long long)Hout * stride, Win = (long long)Wout * stride;
    const bool two = in1 && in1->q;
    const long long s0 = (Hin >> in0->up) * (Win >> in0->up) * in0->ld;
    const long long s1 = two ? (Hin >> in1->up) * (Win >> in1->up) * in1->ld : 0;
    long long nb = conv_sub_batch(s0, s1, (Win + 1) * in0->ld);
    if (nb < 1) return YV_ERR_LIMIT;                              // a single image beyond 2 GB
    if (nb > B) nb = B;
    const long long opix = (long long)Hout * Wout;
    const long long esz = (flags & YV_EPI_OUT_F32) ? 4 : 2;
    for (long long b0 = 0; b0 < B; b0 += nb) {
        const int n = (int)(B - b0 < nb ? B - b0 : nb);
        yv_mx_view v0 = *in0, v1 = two ? *in1 : yv_mx_view{};
        v0.q = (const unsigned char*)in0->q + b0 * s0;
        v0.s = (const unsigned char*)in0->s + b0 * (s0 >> 5);
        if (two) { v1.q = (const unsigned char*)in1->q + b0 * s1; v1.s = (const unsigned char*)in1->s + b0 * (s1 >> 5); }
        rc = conv_mx_impl_one(&v0, two ? &v1 : nullptr, n, Hout, Wout, ksize, stride, wq, wscale, w_rows_pad, bias, Cout,
                              out_bf16 ? (unsigned char*)out_bf16 + b0 * opix * out_ld * esz : nullptr, out_ld,
                              out_q ? (unsigned char*)out_q + b0 * opix * outq_ld : nullptr,
                              out_q ? (unsigned char*)out_scales + b0 * opix * (outq_ld >> 5) : nullptr, outq_ld,
                              res ? (const unsigned char*)res + b0 * opix * res_ld * 2 : nullptr, res_ld, flags, stream);
        if (rc != YV_OK) return rc;
    }
    return YV_OK;
}

extern "C" int yv_conv2d_mxfp8_instance(int B, int Hout, int Wout, int ksize, int stride, int Cin, int Cout) {
    if (Cin <= 0 || (Cin & 31)) return YV_ERR_ARG;
    unsigned char dummy[16] __attribute__((aligned(16)));
    const yv_mx_view v = {dummy, dummy, Cin, Cin, 0};
    const int rc = conv_mx_check(&v, nullptr, B, Hout, Wout, ksize, stride, Cout);
    if (rc != YV_OK) return rc;
    // first sub-batch of a dense source (pixel stride = Cin), as yv_conv2d_mxfp8 would take it
    const long long Win = (long long)Wout * stride, s0 = (long long)Hout * stride * Win * Cin;
    long long nb = conv_sub_batch(s0, 0, (Win + 1) * Cin);
    if (nb < 1) return YV_ERR_LIMIT;
    if (nb > B) nb = B;
    return conv_mx_pick(nb * Hout * Wout, Cout);
}
