// The one text of the BatchNorm + SiLU backward term, shared by its three sites: chan_reduce_kernel<1> (the sums), bn_act_kernel<true>
// (the apply pass, which recomputes the term) - both yolo_train.hip - and the BNBWD form of the convolution epilogues (gemm.hip:
// the same sums, taken where the data gradient is stored).  The sums and the apply pass must agree term by term, so there is ONE
// definition; the library is built with -ffp-contract=off, every product and sum below is its own rounding.
#pragma once
#include "yv_common.h"

// IEEE division, not the hardware reciprocal of gemm.hip's silu_f: the backward kernels have always used this form
__device__ __forceinline__ float sigmoid_f(float x) { return 1.0f / (1.0f + __expf(-x)); }

// xh = (z - mean) * rstd; returns g = d * act'(u), u = gamma * xh + beta (act 1: SiLU, 0: identity)
__device__ __forceinline__ float bn_act_grad_term(float d, float z, float mean, float rstd, float gamma, float beta, int act, float& xh) {
    xh = (z - mean) * rstd;
    float gr = d;
    if (act) {
        const float u = gamma * xh + beta;
        const float sg = sigmoid_f(u);
        gr *= sg * (1.0f + u * (1.0f - sg));
    }
    return gr;
}
