// Shared by the GEMM translation units (gemm.hip, gemm_persistent.hip, gemm_res_ln.hip): the argument block of every GEMM / convolution kernel,
// the GELU of the epilogues, the timed launch, and the declarations of what one unit defines and the other uses.  Tiling and
// layout conventions: the comment at the top of gemm.hip.  Kernels stay in the anonymous namespace of their unit; what crosses
// a unit lives in namespace yvgemm.
#pragma once
#include "yv_common.h"
#include <hip/hip_ext.h>

namespace yvgemm {

constexpr int BK = 64;            // bf16 elements per K step

struct GemmArgs {
    // A operand (activations)
    const uint16_t* a0;
    const uint16_t* a1;          // second concat source (1x1 conv only) or null
    int lda0, lda1;              // pixel / row stride in elements
    int seg_len;                 // gemm_tn only: X column k lives at (k / seg_len) * seg_stride + k % seg_len (0: plain)
    long long seg_stride;
    int c0, c1;                  // channels per source (c0 + c1 = Cin); linear: c0 = K
    int up0, up1;                // nearest-2x upsample flags
    int Hin, Win;                // logical input grid (after upsample)
    int Hout, Wout, ksize, stride;
    // W operand
    const uint16_t* w;           // (N, K) bf16
    const float* bias;
    int M, N, K;
    // output
    void* out;
    int ldo;
    const uint16_t* res;         // bf16 residual view
    int ldres;
    const float* pos;            // pos_embed (tok+1, N) f32
    int tok;
    int flags;
    const int32_t* m_dev;
    int m_mul;
    int tiles_m, tiles_n;
    int group_m;                 // linear kernels; PHASE convolutions (yv_conv2d_dgrad_s2) keep the launch-order index of the grid's
                                 // first phase here: a field of its own would move the hidden arguments of every GemmArgs kernel
    int ldw;                     // WT kernels: row stride of the reduction-major weight (K, N)
    const float* resf;           // f32 residual source (null: read-modify-write `out`)
    uint16_t* aux;               // bf16 side buffer: SAVE_PRE target / GELU_BWD pre-activation
    int ldaux;
    int cin_shift;               // conv: log2(c0 + c1) when that is a power of two, else -1
    int tap_uniform;             // conv: (c0 + c1) % 64 == 0, a K step lies inside one tap
    int splitk;                  // conv only: K range split over `splitk` workgroups per tile (partials in `partial`)
    float* partial;              // (splitk, M, N) f32
    int staged;                  // coalesced LDS-staged epilogue usable (alignment / width checked on the host)
    int sched;                   // gemm_p8: 0 = the grid strides through the tile sequence round by round, 1 = one contiguous
                                 //          share of the sequence per XCD
    uint8_t* mxq;                // YV_EPI_OUT_MXFP8: e4m3 image of the output (row stride ldmxq bytes) ...
    long long ldmxq;
    uint8_t* mxs;                // ... and its E8M0 block scales, K-step-major (N/128, mx_rows, 4)
    long long mx_rows;
    // gemm_p9_kernel<MX>: E8M0 scales of the fp8 operands, K-step-major (K/128, rows, 4) (a0 / w then point at e4m3 bytes, lda0 in bytes)
    const uint8_t* mx_sa;
    const uint8_t* mx_sw;
    long long mx_rows_a, mx_rows_w;
    float* stats;                // STATS convolutions (yv_conv2d_stats): per-tile column sums (tiles_m, 2, N), see finish_tile
    // BNBWD convolutions (yv_conv2d_bnbwd; sums to `stats`): the BatchNorm block that produced this data gradient's target -
    const uint16_t* z;           // its pre-activation, same rows and columns as `out` (row stride ldz) ...
    int ldz;
    int bn_act;                  // ... its activation (1 SiLU, 0 identity) and its per-channel constants (N floats each)
    const float *bn_mean, *bn_rstd, *bn_gamma, *bn_beta;
};

// tuning options read in both units (defined and described in gemm_persistent.hip) and the persistent launchers
extern int g_opt_p8_sched, g_opt_p8_rows, g_opt_p9_small, g_opt_p9_small_fixed;
extern thread_local int g_opt_p8_cus;
extern thread_local hipEvent_t t_time_start, t_time_stop;   // yv_set_launch_timing (gemm.hip): the next timed launch of this thread
int persistent_cus(int n_cu = 0);      // grid of a persistent launch made by this thread (gemm_persistent.hip)
// tile height of a persistent launch on n_cu workgroups (pure: shape, flags and options in, rows out) ...
int p8_tile_rows(int M, int N, int flags, int n_cu);
int p9_tile_rows(int M, int N, int K, int flags, bool mx, int n_cu, int forced_rows);
// ... and the launch of the instance with that height
int launch_p8(GemmArgs& g, hipStream_t st, int rows, int n_cu);
int launch_p9(GemmArgs& g, hipStream_t st, int rows, int n_cu, bool mx);

// Launches kern(arg).  Events armed by yv_set_launch_timing on this thread get the timestamps of the kernel's own dispatch packet
// (no extra barrier packets in the queue, unlike a pair of hipEventRecord calls around the launch) and are cleared: one launch.
template <typename Arg>
inline void launch_timed(void (*kern)(Arg), unsigned grid, unsigned block, size_t lds, hipStream_t st, const Arg& arg) {
    if (t_time_start || t_time_stop) {
        hipExtLaunchKernelGGL(kern, dim3(grid), dim3(block), (uint32_t)lds, st, t_time_start, t_time_stop, 0, arg);
        t_time_start = t_time_stop = nullptr;
    } else {
        hipLaunchKernelGGL(kern, dim3(grid), dim3(block), lds, st, arg);
    }
}

// erf-form GELU through x * sigmoid(x * (p0 + p1 x^2 + p2 x^4)), coefficients fitted (minimax, |x| <= 8) against
// 0.5 x (1 + erf(x / sqrt 2)): max abs error 2.5e-5 - below half a bf16 step of the output everywhere the output exceeds
// 0.01 in magnitude.  x^2 is clamped at 64 (beyond |x| = 8 the result is x or 0 to f32 precision; the quartic would turn over).
__device__ __forceinline__ float gelu_f(float x) {
    const float x2 = fminf(x * x, 64.0f);
    float q = fmaf(-7.03039117e-4f * -1.4426950408889634f, x2, 7.40113286e-2f * -1.4426950408889634f);
    q = fmaf(q, x2, 1.59501573f * -1.4426950408889634f);
    const float e = __builtin_amdgcn_exp2f(x * q);                  // exp(-z)
    return x * __builtin_amdgcn_rcpf(1.0f + e);
}

// (round 1 evaluated erfc by Abramowitz-Stegun 7.1.26: 14 operations per value against 9 here.  ONE definition for every forward
// kernel: schedules that route a linear through different kernels - full batch vs half batches - must agree bit for bit.)
// d/dx gelu(x) = Phi(x) + x * phi(x) of the erf form (erfc by Abramowitz-Stegun 7.1.26, |abs err| <= 1.5e-7); the forward's
// sigmoid fit differs from the erf form by <= 2.5e-5, i.e. this is its derivative to ~1e-4
__device__ __forceinline__ float gelu_grad_f(float x) {
    const float t = __builtin_amdgcn_rcpf(fmaf(0.3275911f * 0.70710678118654752f, fabsf(x), 1.0f));
    float p = fmaf(0.5f * 1.061405429f, t, 0.5f * -1.453152027f);
    p = fmaf(p, t, 0.5f * 1.421413741f);
    p = fmaf(p, t, 0.5f * -0.284496736f);
    p = fmaf(p, t, 0.5f * 0.254829592f);
    const float e = __builtin_amdgcn_exp2f(x * x * -0.72134752044448170368f);     // exp(-x^2/2)
    const float w = p * t * e;                                                       // 0.5*erfc(|x|/sqrt2)
    const float cdf = x >= 0.f ? 1.0f - w : w;
    return cdf + x * e * 0.39894228040143267794f;
}

typedef int i32x8 __attribute__((ext_vector_type(8)));

}  // namespace yvgemm
