// cls-query attention for the trainer's last block (VitTrainer(cls_tail=True)), head dim 64, non-causal: yv_attention_cls_train and
// yv_attention_cls_bwd.  DESIGN.md section 17.
//
// Nothing after the last block reads tokens 1..N-1, so its attention has ONE live query per crop: the forward is the streaming pass of
// attention_cls_kernel (attention.hip) that also keeps the log2-sum-exp, the backward a streaming pass that writes dK and dV for every
// key and dQ for the cls row.  Both kernels: one workgroup of 256 threads per (crop, head); 8 lanes share a 128-byte row (16 bytes
// each), 32 rows per trip; no MFMA, no atomics; every reduction has a fixed order, so a crop's results do not depend on the launch.
//
// Forward: the text of attention_cls_kernel for scores, max, exp2, sum and PV (out is bit-identical to yv_attention_cls); q is read with
// a row stride, there is no device-side row count, and lse = max + log2(sum) is written in the scaled log2 domain of yv_attention_train.
//
// Backward, in f32, with p_n recomputed from lse:
//   pass 1 (K and V read once): s_n = q.k_n * scale * log2e, p_n = exp2(s_n - lse), dp_n = dO.v_n; dv_n = p_n dO is written at once;
//           p_n and dp_n stay in LDS; delta = sum_n p_n dp_n (per 8-lane group in ascending n, then the 32 groups in ascending order);
//   pass 2 (K read a second time): ds_n = p_n (dp_n - delta) * scale; dk_n = ds_n q is written, with zeros in the Q third of every row
//           n >= 1; dq = sum_n ds_n k_n (per group in ascending n, then 4 groups of a wave by shuffles, then the 4 waves) goes to row 0.
// K is read twice and V once; every element of rows [r*N, r*N + N) of dqkv is written exactly once, nothing past them.
// 64-bit addressing throughout: no 2 GB limit on the tensors.
#include "yv_common.h"

namespace {

__device__ __forceinline__ u32x4 pack_bf16x8(const float (&f)[8]) {
    u32x4 v;
#pragma unroll
    for (int i = 0; i < 4; ++i) v[i] = pack_bf16x2(f[2 * i], f[2 * i + 1]);
    return v;
}

// the dot product of two 64-wide rows spread over 8 lanes (every lane of the group gets the sum)
__device__ __forceinline__ float dot8(const float (&a)[8], const float (&b)[8]) {
    float d = 0.f;
#pragma unroll
    for (int i = 0; i < 8; ++i) d += a[i] * b[i];
    d += __shfl_xor(d, 1, 64);
    d += __shfl_xor(d, 2, 64);
    d += __shfl_xor(d, 4, 64);
    return d;
}

__global__ __launch_bounds__(256) void attention_cls_train_kernel(const uint16_t* __restrict__ q, long long ldq,
                                                                  const uint16_t* __restrict__ qkv, int N, int H, float scale_log2,
                                                                  uint16_t* __restrict__ out, float* __restrict__ lse) {
    extern __shared__ __attribute__((aligned(16))) float cls_sm[];       // N scores (padded to 4) | 4 x 64 partial outputs | 8 scalars
    const int r = blockIdx.x / H, hd = blockIdx.x - r * H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = tid & 7, grp = tid >> 3;
    float* sc = cls_sm;
    float* part = cls_sm + ((N + 3) & ~3);
    float* red = part + 256;
    const long long ld = 3LL * H * 64;
    const uint16_t* kb = qkv + (long long)r * N * ld + (long long)(H + hd) * 64 + c * 8;
    const uint16_t* vb = kb + (long long)H * 64;
    float qf[8];
    unpack_bf16x8(*(const u32x4*)(q + (long long)r * ldq + hd * 64 + c * 8), qf);

    float mx = -3.0e38f;
#pragma unroll 4
    for (int n0 = 0; n0 < N; n0 += 32) {
        const int n = n0 + grp, nn = n < N ? n : N - 1;
        float kf[8];
        unpack_bf16x8(*(const u32x4*)(kb + nn * ld), kf);
        float d = 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) d += qf[i] * kf[i];
        d += __shfl_xor(d, 1, 64);
        d += __shfl_xor(d, 2, 64);
        d += __shfl_xor(d, 4, 64);
        d *= scale_log2;
        if (n < N) {
            if (c == 0) sc[n] = d;
            mx = fmaxf(mx, d);
        }
    }
    mx = wave_max(mx);
    if (lane == 0) red[wave] = mx;
    __syncthreads();
    mx = fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
    float sum = 0.f;
    for (int n = tid; n < N; n += 256) {
        const float p = __builtin_amdgcn_exp2f(sc[n] - mx);
        sc[n] = p;
        sum += p;
    }
    sum = wave_sum(sum);
    if (lane == 0) red[4 + wave] = sum;
    __syncthreads();
    sum = (red[4] + red[5]) + (red[6] + red[7]);
    if (tid == 0) lse[(long long)r * H + hd] = mx + log2f(sum);          // log2 domain, as yv_attention_train

    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll 4
    for (int n0 = 0; n0 < N; n0 += 32) {
        const int n = n0 + grp, nn = n < N ? n : N - 1;
        float vf[8];
        unpack_bf16x8(*(const u32x4*)(vb + nn * ld), vf);
        const float p = n < N ? sc[nn] : 0.f;
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[i] += p * vf[i];
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float a = acc[i];
        a += __shfl_xor(a, 8, 64);
        a += __shfl_xor(a, 16, 64);
        a += __shfl_xor(a, 32, 64);
        if (lane < 8) part[wave * 64 + c * 8 + i] = a;
    }
    __syncthreads();
    if (tid < 32) {
        const int d = tid * 2;
        const float inv = 1.0f / sum;
        const float o0 = ((part[d] + part[64 + d]) + (part[128 + d] + part[192 + d])) * inv;
        const float o1 = ((part[d + 1] + part[64 + d + 1]) + (part[128 + d + 1] + part[192 + d + 1])) * inv;
        *(uint32_t*)(out + ((long long)r * H + hd) * 64 + d) = pack_bf16x2(o0, o1);
    }
}

__global__ __launch_bounds__(256) void attention_cls_bwd_kernel(const uint16_t* __restrict__ q, long long ldq,
                                                                const uint16_t* __restrict__ qkv, const uint16_t* __restrict__ dout,
                                                                const float* __restrict__ lse, int N, int H, float scale,
                                                                float scale_log2, uint16_t* __restrict__ dqkv) {
    extern __shared__ __attribute__((aligned(16))) float cls_sm[];       // N p | N dp (each padded to 4) | 4 x 64 partial dq | 32 deltas
    const int r = blockIdx.x / H, hd = blockIdx.x - r * H;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = tid & 7, grp = tid >> 3;
    const int N4 = (N + 3) & ~3;
    float* pp = cls_sm;
    float* dp = cls_sm + N4;
    float* part = dp + N4;
    float* red = part + 256;
    const long long ld = 3LL * H * 64;
    const long long row0 = (long long)r * N * ld + (long long)hd * 64 + c * 8;        // this lane's chunk of the crop's row 0, Q third
    const uint16_t* kb = qkv + row0 + (long long)H * 64;
    const uint16_t* vb = kb + (long long)H * 64;
    uint16_t* gq = dqkv + row0;
    uint16_t* gk = gq + (long long)H * 64;
    uint16_t* gv = gk + (long long)H * 64;
    float qf[8], dof[8];
    unpack_bf16x8(*(const u32x4*)(q + (long long)r * ldq + hd * 64 + c * 8), qf);
    unpack_bf16x8(*(const u32x4*)(dout + ((long long)r * H + hd) * 64 + c * 8), dof);
    const float l = lse[(long long)r * H + hd];

    // ---- pass 1: p, dp, dV, delta
    float dl = 0.f;
#pragma unroll 4
    for (int n0 = 0; n0 < N; n0 += 32) {
        const int n = n0 + grp, nn = n < N ? n : N - 1;
        float kf[8], vf[8];
        unpack_bf16x8(*(const u32x4*)(kb + nn * ld), kf);
        unpack_bf16x8(*(const u32x4*)(vb + nn * ld), vf);
        const float p = __builtin_amdgcn_exp2f(dot8(qf, kf) * scale_log2 - l);
        const float d = dot8(dof, vf);
        if (n < N) {
            if (c == 0) { pp[n] = p; dp[n] = d; }
            dl += p * d;
            float dv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) dv[i] = p * dof[i];
            *(u32x4*)(gv + nn * ld) = pack_bf16x8(dv);
        }
    }
    if (c == 0) red[grp] = dl;
    __syncthreads();
    float delta = 0.f;
    for (int g = 0; g < 32; ++g) delta += red[g];

    // ---- pass 2: dS, dK, the zero rows of dQ, dq
    float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const u32x4 zero = {0u, 0u, 0u, 0u};
#pragma unroll 4
    for (int n0 = 0; n0 < N; n0 += 32) {
        const int n = n0 + grp, nn = n < N ? n : N - 1;
        float kf[8];
        unpack_bf16x8(*(const u32x4*)(kb + nn * ld), kf);
        if (n < N) {
            const float ds = pp[nn] * (dp[nn] - delta) * scale;
            float dk[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                dk[i] = ds * qf[i];
                acc[i] += ds * kf[i];
            }
            *(u32x4*)(gk + nn * ld) = pack_bf16x8(dk);
            if (n > 0) *(u32x4*)(gq + nn * ld) = zero;
        }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        float a = acc[i];
        a += __shfl_xor(a, 8, 64);
        a += __shfl_xor(a, 16, 64);
        a += __shfl_xor(a, 32, 64);
        if (lane < 8) part[wave * 64 + c * 8 + i] = a;
    }
    __syncthreads();
    if (tid < 32) {
        const int d = tid * 2;
        const float q0 = (part[d] + part[64 + d]) + (part[128 + d] + part[192 + d]);
        const float q1 = (part[d + 1] + part[64 + d + 1]) + (part[128 + d + 1] + part[192 + d + 1]);
        *(uint32_t*)(dqkv + (long long)r * N * ld + (long long)hd * 64 + d) = pack_bf16x2(q0, q1);
    }
}

// the checks that both entries share; YV_OK: launch (or R == 0)
int check_cls_args(const void* q, long long ldq, int R, int N, int H) {
    if (R < 0 || N <= 0 || H <= 0) return YV_ERR_ARG;
    if (((uintptr_t)q & 15) || (ldq & 7) || ldq < (long long)H * 64) return YV_ERR_ARG;   // 16-byte row chunks at every row of q
    if (N > 8192 || (long long)R * H > 0x7fffffffLL) return YV_ERR_LIMIT;                  // one query's scores live in LDS
    return YV_OK;
}

}  // namespace

extern "C" int yv_attention_cls_train(const void* q, long long ldq, const void* qkv, int R, int N, int H, float scale, void* out,
                                      float* lse, void* stream) {
    if (!q || !qkv || !out || !lse) return YV_ERR_ARG;
    if ((((uintptr_t)qkv | (uintptr_t)out) & 15) || ((uintptr_t)lse & 3)) return YV_ERR_ARG;
    const int rc = check_cls_args(q, ldq, R, N, H);
    if (rc != YV_OK || R == 0) return rc;
    const size_t lds = ((size_t)((N + 3) & ~3) + 256 + 8) * sizeof(float);
    hipLaunchKernelGGL(attention_cls_train_kernel, dim3(R * H), dim3(256), lds, (hipStream_t)stream, (const uint16_t*)q, ldq,
                       (const uint16_t*)qkv, N, H, scale * 1.4426950408889634f, (uint16_t*)out, lse);
    return yv_launch_status();
}

extern "C" int yv_attention_cls_bwd(const void* q, long long ldq, const void* qkv, const void* dout, const float* lse, int R, int N,
                                    int H, float scale, void* dqkv, void* stream) {
    if (!q || !qkv || !dout || !lse || !dqkv) return YV_ERR_ARG;
    if ((((uintptr_t)qkv | (uintptr_t)dout | (uintptr_t)dqkv) & 15) || ((uintptr_t)lse & 3)) return YV_ERR_ARG;
    const int rc = check_cls_args(q, ldq, R, N, H);
    if (rc != YV_OK || R == 0) return rc;
    const size_t lds = (2 * (size_t)((N + 3) & ~3) + 256 + 32) * sizeof(float);             // 66.7 KB at N = 8192
    if (!yv_grant_lds((const void*)attention_cls_bwd_kernel, lds)) return YV_ERR_LAUNCH;
    hipLaunchKernelGGL(attention_cls_bwd_kernel, dim3(R * H), dim3(256), lds, (hipStream_t)stream, (const uint16_t*)q, ldq,
                       (const uint16_t*)qkv, (const uint16_t*)dout, lse, N, H, scale, scale * 1.4426950408889634f, (uint16_t*)dqkv);
    return yv_launch_status();
}
