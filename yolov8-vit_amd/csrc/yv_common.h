// Shared device/host helpers for libyvhip (gfx950 only: wave = 64 lanes).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <atomic>
#include <mutex>
#include "yv_hip.h"

#define YV_WAVE 64

typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;
typedef __attribute__((ext_vector_type(4))) uint32_t u32x4;
typedef __attribute__((ext_vector_type(2))) uint32_t u32x2;

static inline int yv_launch_status() {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? YV_OK : YV_ERR_LAUNCH;
}

// A launch may ask for more than 64 KB of dynamic LDS only after the kernel has been granted that much
// (hipFuncAttributeMaxDynamicSharedMemorySize).  The grant belongs to the DEVICE's copy of the kernel, so it is remembered per
// kernel function and device; a kernel whose request differs between calls is re-granted only to grow.  The steady state (the
// size is already granted) takes no lock: a probe of a fixed table of atomics, as launches come from the request threads of
// every stream; granting itself is serialised so that a smaller concurrent request cannot undo a larger one.  False: the runtime
// refused, or more than YV_LDS_KERNELS kernels / 64 devices.
constexpr int YV_LDS_KERNELS = 256;
struct YvLdsGrant { std::atomic<const void*> kern; std::atomic<size_t> bytes[64]; };
inline bool yv_grant_lds(const void* kern, size_t lds) {
    if (lds <= 65536) return true;
    static YvLdsGrant table[YV_LDS_KERNELS];
    static std::mutex mu;
    int dev = 0;
    if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return false;
    for (size_t n = 0, i = ((uintptr_t)kern >> 4) % YV_LDS_KERNELS; n < YV_LDS_KERNELS; ++n, i = (i + 1) % YV_LDS_KERNELS) {
        const void* k = table[i].kern.load(std::memory_order_acquire);
        if (!k && table[i].kern.compare_exchange_strong(k, kern, std::memory_order_acq_rel)) k = kern;     // claim a free slot
        if (k != kern) continue;
        std::atomic<size_t>& have = table[i].bytes[dev];
        if (lds <= have.load(std::memory_order_acquire)) return true;
        std::lock_guard<std::mutex> lk(mu);
        if (lds <= have.load(std::memory_order_relaxed)) return true;
        if (hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds) != hipSuccess) return false;
        have.store(lds, std::memory_order_release);
        return true;
    }
    return false;
}

__device__ __forceinline__ float bf16_to_f32(uint16_t h) { return __uint_as_float(((uint32_t)h) << 16); }

// round-to-nearest-even f32 -> bf16 through the hardware convert (NaN stays NaN)
__device__ __forceinline__ uint16_t f32_to_bf16(float f) {
    __bf16 b = (__bf16)f;
    return __builtin_bit_cast(uint16_t, b);
}
__device__ __forceinline__ uint32_t pack_bf16x2(float lo, float hi) {      // one v_cvt_pk_bf16_f32 (RNE)
    typedef float f32x2_t __attribute__((ext_vector_type(2)));
    typedef __bf16 bf16x2_t __attribute__((ext_vector_type(2)));
    const f32x2_t v = {lo, hi};
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, bf16x2_t));
}

// 16 bytes of bf16 -> 8 floats
__device__ __forceinline__ void unpack_bf16x8(const u32x4 v, float (&f)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        f[2 * i] = __uint_as_float(v[i] << 16);
        f[2 * i + 1] = __uint_as_float(v[i] & 0xffff0000u);
    }
}

__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
    return v;
}
