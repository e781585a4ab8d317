// Request-sized calls (yvhip.request.RequestSession): the one device kernel a session adds.
//   yv_pack_results     the join of crop_list with the detection arrays and the classifier's outputs that inferdet.main does in
//                       Python after seven device-to-host copies, done on the device into ONE buffer of 32-bit words, so that a
//                       request's result is one copy.  A pure gather: one launch, no workspace, no atomics.
#include "yv_common.h"

#define PK_THREADS 256

// One thread per output word; a row's W = 9 + nc words are written by adjacent lanes (idx = row * W + col), so a wave's stores
// cover 256 contiguous bytes.  Every word of out (1 + cap, W) is written by exactly one thread on every launch: rows past the
// count are zeroed here, not by a memset, so a replay never shows a previous request's rows.
__global__ void __launch_bounds__(PK_THREADS)
pack_results_kernel(const int32_t* __restrict__ crop_list, const int32_t* __restrict__ crop_total,
                    const int32_t* __restrict__ det_box, const float* __restrict__ det_score,
                    const int32_t* __restrict__ det_label, const int32_t* __restrict__ cls_label,
                    const float* __restrict__ cls_logits, int B, int slots, int cap, int nc, int32_t* __restrict__ out) {
    const int W = 9 + nc;
    const long long n = (long long)(1 + cap) * W;
    const long long idx = (long long)blockIdx.x * PK_THREADS + threadIdx.x;
    if (idx >= n) return;
    const int row = (int)(idx / W), col = (int)(idx - (long long)row * W);
    int total = crop_total[0];
    total = total < 0 ? 0 : (total > cap ? cap : total);
    int32_t v = 0;
    if (row == 0) {
        v = col == 0 ? total : col == 1 ? B : col == 2 ? slots : col == 3 ? cap : col == 4 ? nc : 0;
    } else if (row - 1 < total) {
        const int k = row - 1;
        const int image = crop_list[(size_t)k * 6], slot = crop_list[(size_t)k * 6 + 5];
        if (image >= 0 && image < B && slot >= 0 && slot < slots) {          // (a crop list of yv_compact_crops always is)
            const size_t d = (size_t)image * slots + slot;
            if (col == 0) v = image;
            else if (col == 1) v = slot;
            else if (col < 6) v = det_box[d * 4 + (col - 2)];
            else if (col == 6) v = det_label[d];
            else if (col == 7) v = cls_label[k];
            else if (col == 8) v = __float_as_int(det_score[d]);
            else v = __float_as_int(cls_logits[(size_t)k * nc + (col - 9)]);
        }
    }
    out[idx] = v;
}

extern "C" int yv_pack_results(const int32_t* crop_list, const int32_t* crop_total, const int32_t* det_box,
                               const float* det_score, const int32_t* det_label, const int32_t* cls_label,
                               const float* cls_logits, int B, int slots, int cap, int nc, int32_t* out, void* stream) {
    if (!crop_list || !crop_total || !det_box || !det_score || !det_label || !cls_label || !cls_logits || !out)
        return YV_ERR_ARG;
    if (B <= 0 || slots <= 0 || nc <= 0 || cap < 0) return YV_ERR_ARG;
    const long long n = (long long)(1 + (long long)cap) * (9 + (long long)nc);
    const long long blocks = (n + PK_THREADS - 1) / PK_THREADS;
    if (blocks > 0x7fffffffLL) return YV_ERR_LIMIT;
    hipLaunchKernelGGL(pack_results_kernel, dim3((unsigned)blocks), dim3(PK_THREADS), 0, (hipStream_t)stream, crop_list,
                       crop_total, det_box, det_score, det_label, cls_label, cls_logits, B, slots, cap, nc, out);
    return yv_launch_status();
}
