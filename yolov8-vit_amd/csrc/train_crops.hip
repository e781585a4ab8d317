// Training / validation crops of the classifier taken on the device from source images that were decoded once.
//
// Replaces, per annotated object and epoch (SURVEY.md section 8 rows B1 tail, B2 and 8(f) N4):
//   Image.open + PIL crop                                  utils/trainClass.py:70-93     (right/bottom exclusive)
//   A.Resize(S,S,INTER_NEAREST) + A.Normalize(.5,.5)       utils/trainClass.py:199-221   (head of both transforms)
//   HWC -> CHW, per-item tensors, collate                  utils/trainClass.py:250-273
// and the stochastic tail of data_transforms['train'] that yv_augment_patchify applies (same record, same arithmetic).
//
// One gather pass: an output value is the bilinear blend (BORDER_REFLECT_101, record tables, channel permutation, holes)
// of four taps of the NORMALISED S x S crop, and a tap of that crop is one u8 of the pool, found through the nearest-
// neighbour row / column rule of the resize and normalised in f32 with the two roundings of Normalize.  The normalised
// crop never exists in memory.  Per value this is exactly
//   oracle.boxes.crop_resize_normalize(image, rect, (S,S))  then  oracle.augment.apply_record(., geo, idx, P)
// with every f32 operation rounded once, in augment_kernel's order (-ffp-contract=off), so the result is bit-exact.
//
// The source is interleaved RGB: coordinates, reflect folds, table look-ups and the four tap addresses of an output
// pixel are the same for its three channels, so they are computed once per pixel (augment_kernel walks plane by plane);
// a tap is one 3-byte read and the record's channel permutation picks the byte.
//
// Nothing that comes from the host is trusted (see the clamps stated in include/yv_hip.h): a block first folds the crop
// into the record's integer tables,  col[i] = clamp(x0 + nearest(clamp(mapx[i], 0, S-1), S, max(x1-x0, 1)), 0, W-1)  (rows
// alike), in LDS, with the f64 sequence of OpenCV's INTER_NEAREST (== oracle.boxes.nearest_index_table); the byte address
// of a tap is additionally clamped to the pool.
#include "yv_common.h"

namespace {

constexpr int TC_THREADS = 256;
constexpr int TC_MAX_S = 4096;                   // 2 S ints of LDS per block
constexpr long long TC_MAX_DIM = 1 << 24;        // width / height bound: 3 * W * row stays far inside 64 bits

__device__ __forceinline__ int tc_reflect101(int i, int n) {       // as in augment.hip: |i| <= 4n + 1
    if (n == 1) return 0;
    const int per = 2 * n - 2;
    int m = i < 0 ? -i : i;
#pragma unroll
    for (int k = 0; k < 3; ++k) m = m >= per ? m - per : m;
    while (m >= per) m -= per;
    return m < n ? m : per - m;
}

__device__ __forceinline__ long long tc_clamp(long long v, long long lo, long long hi) { return v < lo ? lo : (v > hi ? hi : v); }

// s = min(floor(d * (1 / (dst / src))), src - 1) in f64, one rounding per operation
__device__ __forceinline__ long long tc_nearest(int d, int dst, long long src) {
    const double fx = __ddiv_rn((double)dst, (double)src);
    const double ifx = __ddiv_rn(1.0, fx);
    const long long s = (long long)floor(__dmul_rn((double)d, ifx));
    return s < src - 1 ? s : src - 1;
}

// (x - 127.5) * fl32(1/127.5): albumentations' Normalize in f32, two roundings
__device__ __forceinline__ float tc_norm(uint32_t v, float rcp) { return __fmul_rn(__fsub_rn((float)v, 127.5f), rcp); }

// the three bytes of one source pixel in the low 24 bits
__device__ __forceinline__ uint32_t tc_px(const uint8_t* __restrict__ pool, long long last, long long a) {
    const uint8_t* p = pool + tc_clamp(a, 0, last);
    return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16);
}

// grid: (ceil(S*S/8 / TC_THREADS), B); one thread = 8 consecutive output pixels of a row, all three channels
template <int LAYOUT>
__global__ __launch_bounds__(TC_THREADS) void train_crops_kernel(const uint8_t* __restrict__ pool, long long pool_bytes,
                                                                 const long long* __restrict__ table, int n_images,
                                                                 const int32_t* __restrict__ plan, int S, int P,
                                                                 const float* __restrict__ geo, const int32_t* __restrict__ idx,
                                                                 float rcp, void* __restrict__ out) {
    extern __shared__ int tc_tab[];               // col[S] then row[S]: source column / row of the record's table entries
    const int b = blockIdx.y;
    const float* ge = geo + (size_t)b * (6 + 2 * S);
    const int32_t* id = idx + (size_t)b * (36 + 2 * S);
    const int32_t* pl = plan + (size_t)b * 5;
    int img = pl[0];
    img = img < 0 ? 0 : (img >= n_images ? n_images - 1 : img);
    const long long off = tc_clamp(table[(size_t)img * 3], 0, pool_bytes);
    const long long W = tc_clamp(table[(size_t)img * 3 + 1], 1, TC_MAX_DIM), H = tc_clamp(table[(size_t)img * 3 + 2], 1, TC_MAX_DIM);
    {
        const long long rx0 = pl[1], ry0 = pl[2], rx1 = pl[3], ry1 = pl[4];
        const long long cw = rx1 - rx0 > 1 ? rx1 - rx0 : 1, ch = ry1 - ry0 > 1 ? ry1 - ry0 : 1;
        for (int i = threadIdx.x; i < 2 * S; i += TC_THREADS) {
            const bool isy = i >= S;
            int m = id[36 + i];
            m = m < 0 ? 0 : (m > S - 1 ? S - 1 : m);
            const long long s = (isy ? ry0 : rx0) + tc_nearest(m, S, isy ? ch : cw);
            tc_tab[i] = (int)tc_clamp(s, 0, (isy ? H : W) - 1);
        }
    }
    __syncthreads();
    const int it = blockIdx.x * TC_THREADS + threadIdx.x;
    if (it >= (S * S) >> 3) return;
    int oy, ox0;
    if (LAYOUT == 2) {
        // patch-major order: the 16-byte stores of consecutive lanes are consecutive in a (patch, channel) block of the operand
        const int per_p = P * (P >> 3), g = S / P;
        const int patch = it / per_p, rem = it - patch * per_p;
        const int py = rem / (P >> 3), p8 = rem - py * (P >> 3);
        oy = (patch / g) * P + py;
        ox0 = (patch % g) * P + p8 * 8;
    } else {
        oy = it / (S >> 3);
        ox0 = (it - oy * (S >> 3)) * 8;
    }
    const float a0 = ge[0], a1 = ge[1], a2 = ge[2], a3 = ge[3], a4 = ge[4], a5 = ge[5];
    const float* lutx = ge + 6;
    const float* luty = lutx + S;
    int nh = id[3];
    nh = nh < 0 ? 0 : (nh > 8 ? 8 : nh);
    const int32_t* holes = id + 4;
    int sh[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const int sc = id[c];
        sh[c] = 8 * (sc < 0 ? 0 : (sc > 2 ? 2 : sc));
    }
    const int* col = tc_tab;
    const int* rowt = tc_tab + S;
    const long long last = pool_bytes - 3;
    const float lim = (float)(4 * S);
    const float cy = luty[oy];
    float vals[3][8];
#pragma unroll
    for (int j = 0; j < 8; ++j) {
        const int ox = ox0 + j;
        const float cx = lutx[ox];
        float u = __fadd_rn(__fadd_rn(__fmul_rn(a0, cx), __fmul_rn(a1, cy)), a2);
        float v = __fadd_rn(__fadd_rn(__fmul_rn(a3, cx), __fmul_rn(a4, cy)), a5);
        u = fminf(fmaxf(u, -lim), lim);                      // also maps NaN to -lim: never an out-of-range index
        v = fminf(fmaxf(v, -lim), lim);
        const float uf = floorf(u), vf = floorf(v);
        const float fx = __fsub_rn(u, uf), fy = __fsub_rn(v, vf);
        const int ix = (int)uf, iy = (int)vf;
        const long long x0 = 3LL * col[tc_reflect101(ix, S)], x1 = 3LL * col[tc_reflect101(ix + 1, S)];
        const long long y0 = off + 3LL * W * rowt[tc_reflect101(iy, S)], y1 = off + 3LL * W * rowt[tc_reflect101(iy + 1, S)];
        const uint32_t p00 = tc_px(pool, last, y0 + x0), p01 = tc_px(pool, last, y0 + x1);
        const uint32_t p10 = tc_px(pool, last, y1 + x0), p11 = tc_px(pool, last, y1 + x1);
        const float gx1 = __fsub_rn(1.0f, fx), gy1 = __fsub_rn(1.0f, fy);
        bool hole = false;
        for (int h = 0; h < nh; ++h) {
            const int32_t* q = holes + h * 4;                                 // x1, y1, x2, y2 (right / bottom exclusive)
            hole |= ox >= q[0] && ox < q[2] && oy >= q[1] && oy < q[3];
        }
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            const float v00 = tc_norm((p00 >> sh[c]) & 255u, rcp), v01 = tc_norm((p01 >> sh[c]) & 255u, rcp);
            const float v10 = tc_norm((p10 >> sh[c]) & 255u, rcp), v11 = tc_norm((p11 >> sh[c]) & 255u, rcp);
            const float top = __fadd_rn(__fmul_rn(v00, gx1), __fmul_rn(v01, fx));
            const float bot = __fadd_rn(__fmul_rn(v10, gx1), __fmul_rn(v11, fx));
            const float r = __fadd_rn(__fmul_rn(top, gy1), __fmul_rn(bot, fy));
            vals[c][j] = hole ? 0.0f : r;
        }
    }
    if (LAYOUT == 2) {
        const int g = S / P;
        const size_t row = (size_t)b * g * g + (size_t)(oy / P) * g + (ox0 / P);
        uint16_t* o = (uint16_t*)out + row * (size_t)(3 * P * P) + (oy % P) * P + (ox0 % P);
#pragma unroll
        for (int c = 0; c < 3; ++c)
            *(uint4*)(o + (size_t)c * P * P) = make_uint4(pack_bf16x2(vals[c][0], vals[c][1]), pack_bf16x2(vals[c][2], vals[c][3]),
                                                          pack_bf16x2(vals[c][4], vals[c][5]), pack_bf16x2(vals[c][6], vals[c][7]));
    } else {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            float* o = (float*)out + (((size_t)b * 3 + c) * S + oy) * S + ox0;
            ((float4*)o)[0] = make_float4(vals[c][0], vals[c][1], vals[c][2], vals[c][3]);
            ((float4*)o)[1] = make_float4(vals[c][4], vals[c][5], vals[c][6], vals[c][7]);
        }
    }
}

}  // namespace

extern "C" int yv_train_crops(const uint8_t* pool, size_t pool_bytes, const int64_t* table, int n_images, const int32_t* plan,
                              int B, int S, int P, const float* geo, const int32_t* idx, int layout, void* out, void* stream) {
    if (!pool || !table || !plan || !geo || !idx || !out) return YV_ERR_ARG;
    if (pool_bytes < 3 || n_images <= 0 || B < 0 || S <= 0 || (S & 7)) return YV_ERR_ARG;
    if (layout != 0 && layout != 2) return YV_ERR_ARG;
    if (layout == 2 && (P < 8 || (P & 7) || S % P)) return YV_ERR_ARG;
    if (S > TC_MAX_S || B > 65535) return YV_ERR_LIMIT;
    if (B == 0) return YV_OK;
    const float rcp = 1.0f / 127.5f;                 // fl32(1/127.5), computed once on the host
    const dim3 grid((unsigned)(((S * S >> 3) + TC_THREADS - 1) / TC_THREADS), (unsigned)B), block(TC_THREADS);
    const size_t lds = (size_t)2 * S * sizeof(int);
    hipStream_t st = (hipStream_t)stream;
    if (layout == 2)
        hipLaunchKernelGGL(train_crops_kernel<2>, grid, block, lds, st, pool, (long long)pool_bytes, (const long long*)table,
                           n_images, plan, S, P, geo, idx, rcp, out);
    else
        hipLaunchKernelGGL(train_crops_kernel<0>, grid, block, lds, st, pool, (long long)pool_bytes, (const long long*)table,
                           n_images, plan, S, P, geo, idx, rcp, out);
    return yv_launch_status();
}
