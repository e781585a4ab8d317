/* yv_hip.h - C ABI of the MI355X (gfx950) hot-path library `libyvhip.so`.
 *
 * Drop-in boundary of the detect -> NMS/inflate/crop -> ViT-classify path of
 * Voyager0587/yolov8-vit.  The reference has NO native/FFI interface (SURVEY.md
 * section 8(b)): its boundary is a Python call surface.  Each entry point below
 * therefore cites the reference *Python site* whose arithmetic it replaces; the
 * Python host side (yolov8-vit_amd/) binds these symbols with ctypes and mirrors
 * the reference's names.
 *
 * Conventions
 *  - every pointer is a DEVICE pointer unless its name ends in `_host`;
 *  - `stream` is a hipStream_t passed as void*; every call only enqueues work on
 *    it (no allocation, no synchronisation, graph-capturable);
 *  - the caller owns all buffers, including `ws` workspaces whose minimum size
 *    is returned by the matching `*_ws_bytes` function;
 *  - return value: 0 = YV_OK, negative = error (yv_error_string), never throws;
 *  - bf16 tensors are raw uint16_t storage; "NHWC view" = base pointer + pixel
 *    stride `ld` in elements (lets producers write straight into concat
 *    buffers and consumers read channel slices: no concat/split kernels).
 */
#ifndef YV_HIP_H
#define YV_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define YV_OK 0
#define YV_ERR_ARG (-1)        /* bad size / null pointer / unsupported shape */
#define YV_ERR_LIMIT (-2)      /* exceeds a documented kernel limit           */
#define YV_ERR_WORKSPACE (-3)  /* workspace too small                          */
#define YV_ERR_LAUNCH (-4)     /* hipLaunch failed (hipGetLastError != 0)     */

int yv_version(void);
const char* yv_error_string(int code);
/* 1 if the current HIP device is gfx950, 0 otherwise, <0 on HIP error. */
int yv_device_is_gfx950(void);
/* Tuning knobs (process-wide, not part of the reference surface): "linear_group_m" (M tiles per L2 group) and "linear_variant",
 * the kernel of yv_linear / yv_linear_ex (yv_linear_route reports what a value selects for a shape):
 *   1          the shipped rule: skinny, register-staged, mid-M ("linear_mid": the largest M gemm_mid_kernel takes, 0 = off,
 *              the default; "linear_mid_fill": it takes a shape that makes at most this many eighths of the CU count in
 *              128 x 128 tiles, 5), split-K, persistent or 128 x 128 LDS-DMA tiles by shape and flags;
 *   0          igemm_kernel, register-staged 128 x 16 / 32 / 64 / 128 tiles, for every shape;
 *   2, 3, 4    gemm_dma_kernel with 256 x 128, 256 x 256, 128 x 256 tiles;
 *   9, 11      the persistent gemm_p8_kernel / gemm_p9_kernel where the shape and flags allow them, at any M (else 128 x 128);
 *   101 .. 104 gemm_dma_kernel 128 x 128 with one stage of its main loop taken out (ablations 1 .. 4, tools/gemm_bench.py);
 *   201 .. 204 the same ablations on 256 x 256 tiles;
 *   any other  128 x 128 LDS-DMA tiles.
 * Every value but 1 switches the skinny and the mid-M kernel off; N <= 64 or K % 64 != 0 always runs igemm_kernel; a split-K launch (a
 * registered workspace, few tiles, a long K) takes 128 x 128 tiles whatever the value says.  The forced instances check less
 * than the shipped rule does: they are for benchmarks at shapes known to suit them.
 * "linear_ln_mid" / "linear_ln_fill": the fused LayerNorm + linear step of yv_linear_ln (see there; 0 / 0: it does not exist).
 * "linear_mx_mid" / "linear_mx_mid_fill": the mid-M step of the MXFP8 linears (yv_linear_mxfp8 / yv_linear_mxfp8_q), ahead of their
 * persistent rule.  "linear_mx_mid" is the largest M gemm_mx_mid_kernel takes (0 = the step does not exist, the default;
 * "linear_variant" does not bear on it); it takes 1 <= M <= that, N % 64 == 0, N > 64, K % 128 == 0, flags within BIAS | GELU |
 * RES_F32 | OUT_F32 (| OUT_MXFP8 from yv_linear_mxfp8_q), no separate residual source and no aux tensor, where 128 x 128 tiles
 * number at most "linear_mx_mid_fill" eighths of the CU count. */
int yv_set_option(const char* key, int value);
/* Current value of a knob.  "linear_p8_cus" (workgroups of the persistent classifier GEMMs; 0 = every CU) is PER THREAD: it
 * applies to the launches the calling thread makes (a pipelined runner lowers it around its own classifier submissions so that
 * kernels of its other streams find free CUs, and restores it; other threads and later callers are not affected). */
int yv_get_option(const char* key, int* value);

/* MXFP8 linears (BASELINE.json configs[4], FP8 classifier GEMMs; OCP e4m3 bytes + one E8M0 scale per 32 consecutive K
 * elements of a row, consumed by the block-scaled gfx950 MFMA).
 * Scale arrays are K-step-major: (K/128, rows_pad, 4) bytes - the four block scales of one 128-deep K step of a row form
 * one dword, a tile's 128 dwords are contiguous (one LDS-DMA half); rows_pad = row count rounded up to 128.
 * yv_quant_mxfp8: x (rows, K) bf16 -> q (rows, K) bytes (row stride ldq) + scales; scale exponent
 *   e = ceil(log2(amax/448)) per block, q = RNE_e4m3(x * 2^-e); K a multiple of 128.
 * yv_linear_mxfp8: out[M,N] = (Aq*2^sa)[M,K] . (Wq*2^sw)[N,K]^T with the epilogues of yv_linear (bias, GELU, f32 residual
 *   read-modify-write, f32 output). */
/* yv_linear_mxfp8 whose OUTPUT is again an MXFP8 operand (bias / GELU applied, rounded to bf16, then quantised in the
 * epilogue): the fc1 -> fc2 hand-off of the MLP without a bf16 round trip through HBM.  N a multiple of 128. */
int yv_linear_mxfp8_q(const void* Aq, long long lda, const void* Ascale, long long a_rows_pad, const void* Wq, const void* Wscale,
                      long long w_rows_pad, const float* bias, int M, int N, int K, int flags, const int32_t* m_dev, int m_mul,
                      void* out_q, long long ldq, void* out_scales, long long out_rows_pad, void* stream);

/* yv_attention with the output written directly in the MXFP8 operand format of the proj GEMM (same numbers as
 * yv_attention followed by yv_quant_mxfp8); H even. */
int yv_attention_mxfp8(const void* qkv, int R, int N, int H, float scale, void* out_q, long long ldq, void* out_scales,
                       long long rows_pad, const int32_t* r_dev, void* stream);

/* yv_layernorm with the output written directly in the MXFP8 operand format (same numbers as yv_layernorm followed by
 * yv_quant_mxfp8: the bf16 rounding is kept); D a multiple of 128. */
int yv_layernorm_mxfp8(const float* x, size_t ldx, const float* gamma, const float* beta, int rows, int D, float eps, void* q,
                       size_t ldq, void* scales, long long rows_pad, const int32_t* count_dev, int rows_per_count,
                       void* stream);

/* Diagnostic: ONE v_mfma_scale_f32_16x16x128_f8f6f4 on caller-provided register images: a, b (64 lanes x 32 bytes),
 * sa, sb (64 x int32 scale registers), opsel 0..3 for both; d (64 lanes x 4 f32). */
int yv_mx_probe(const void* a, const void* b, const void* sa, const void* sb, int opsel, void* d, void* stream);
/* The same for ONE v_mfma_scale_f32_32x32x64_f8f6f4 (the QK^T product of yv_attention_fp8): a, b (64 lanes x 32 bytes), sa, sb
 * (64 x int32), opsel 0..3 for both; d (64 lanes x 16 f32, the C/D layout of the 32x32x16 forms). */
int yv_mx_probe32(const void* a, const void* b, const void* sa, const void* sb, int opsel, void* d, void* stream);

int yv_quant_mxfp8(const void* x, long long ldx, long long rows, int K, void* q, long long ldq, void* scales,
                   long long rows_pad, void* stream);
int yv_linear_mxfp8(const void* Aq, long long lda, const void* Ascale, long long a_rows_pad, const void* Wq, const void* Wscale,
                    long long w_rows_pad, const float* bias, int M, int N, int K, void* out, int ldo, int flags,
                    const int32_t* m_dev, int m_mul, void* stream);

/* MXFP8 training (VitTrainer(dtype="mxfp8")).
 * yv_quant_mxfp8_2d: x (T, C) bf16 (row stride ldx, C a multiple of 128) read once -> either or both of
 *   row form    q (T, C) bytes (row stride ldq) + scales (C/128, rows_pad, 4): exactly what yv_quant_mxfp8 writes;
 *   column form qt (C, T_pad) bytes (row stride ldqt) + scales_t (T_pad/128, c_rows_pad, 4): exactly what yv_quant_mxfp8
 *               writes for x^T with T zero-padded to T_pad (a multiple of 128): the token-reduction operands of a weight
 *               gradient.  Pass null q / scales or qt / scales_t to skip a form. */
int yv_quant_mxfp8_2d(const void* x, long long ldx, long long T, int C, void* q, long long ldq, void* scales, long long rows_pad,
                      void* qt, long long ldqt, void* scales_t, long long c_rows_pad, long long T_pad, void* stream);
/* yv_linear_mxfp8 with the training epilogues of yv_linear_ex: YV_EPI_RES_F32 with a separate f32 residual source res_f32
 * (same layout as out; null: read-modify-write of out), YV_EPI_SAVE_PRE (with YV_EPI_GELU; pre-activation -> aux) and
 * YV_EPI_GELU_BWD (out = bf16(acc + bias) * gelu'(aux)); aux is bf16 with row stride ldaux (multiple of 8). */
int yv_linear_mxfp8_ex(const void* Aq, long long lda, const void* Ascale, long long a_rows_pad, const void* Wq, const void* Wscale,
                       long long w_rows_pad, const float* bias, int M, int N, int K, void* out, int ldo, int flags,
                       const float* res_f32, void* aux, int ldaux, void* stream);
/* Diagnostic: the kernel instance an MX linear of this shape and flags launches with dense operands (0: 128 x 128 tiles,
 * gemm_mx_kernel; 1: the persistent kernel), or a negative YV_ERR_* code if the arguments are not accepted. */
int yv_linear_mxfp8_instance(int M, int N, int K, int flags);
/* The route of a linear: the kernel yv_linear / yv_linear_ex (mx = 0) or yv_linear_mxfp8 / yv_linear_mxfp8_ex (mx = 1) launches
 * for this shape, flags and strides under the current options, decided by the function the launch path itself calls.  Host
 * only: nothing is dereferenced or launched, bases count as 16-byte aligned, MX operands as dense (scale rows rounded up to 128).
 *   flags        as the launch takes them, plus YV_ROUTE_M_DEV where the launch would pass a device row count (m_dev);
 *   has_res_f32  a separate f32 residual source (yv_linear_ex / yv_linear_mxfp8_ex);  ldaux > 0: an aux tensor of that row stride;
 *   lda          in elements (mx: bytes);  ws_bytes: the split-K workspace registered for the stream (0: none);
 *   n_cu         workgroups of a persistent launch before "linear_p8_cus" clips them; 0 = the CU count of the current device
 *                (YV_ERR_LAUNCH where there is none).
 * Returns YV_OK and fills *out, or the YV_ERR_* code with which the launch would reject the arguments. */
#define YV_LIN_SKINNY 0 /* gemm_skinny_kernel, 64 x 16 tiles, K split over its eight waves                                  */
#define YV_LIN_IGEMM 1  /* igemm_kernel<0, 128, tile_cols, ..>: register-staged                                             */
#define YV_LIN_DMA 2    /* gemm_dma_kernel<tile_rows, tile_cols, .., abl>: LDS-DMA, with splitk > 1 + splitk_reduce_kernel  */
#define YV_LIN_P8 3     /* gemm_p8_kernel<.., f32out>: persistent, 8-phase, tile_rows x 256                                 */
#define YV_LIN_P9 4     /* gemm_p9_kernel<tile_rows / 32, f32out, 0, ext, mx>: persistent, free-running, tile_rows x 256    */
#define YV_LIN_MX 5     /* gemm_mx_kernel<128, 128, 2, 2> (mx = 1 only)                                                     */
#define YV_LIN_MID 6    /* gemm_mid_kernel, 64 x 64 tiles, K split over its two wave groups ("linear_mid" > 0 only)         */
#define YV_LIN_MX_MID 7 /* gemm_mx_mid_kernel, 64 x 64 tiles, K steps dealt to two wave groups (mx = 1, "linear_mx_mid" > 0)   */
#define YV_ROUTE_M_DEV 0x40000000 /* yv_linear_route's `flags` only */
typedef struct {
    int kernel;               /* YV_LIN_* */
    int tile_rows, tile_cols; /* output tile of a workgroup */
    int f32out;               /* persistent kernels: the f32 epilogue instance (f32 output or f32 residual) */
    int ext;                  /* gemm_p9_kernel: trainer epilogue instance, 1 YV_EPI_SAVE_PRE, 2 YV_EPI_GELU_BWD */
    int abl;                  /* gemm_dma_kernel: ablation 1 .. 4 ("linear_variant" 10x / 20x), else 0 */
    int mx;                   /* MXFP8 operands */
    int splitk;               /* K slices per tile (1: none) */
    int staged;               /* GemmArgs::staged: the LDS-staged epilogue is usable */
    int grid;                 /* workgroups launched (persistent kernels: min(tiles, CUs)) */
} yv_linear_route_t;
int yv_linear_route(int M, int N, int K, int lda, int ldo, int flags, int has_res_f32, int ldaux, int mx, size_t ws_bytes,
                    int n_cu, yv_linear_route_t* out);
/* The route of yv_linear_mxfp8_q (which yv_linear_route, like yv_linear_mxfp8, rejects: YV_EPI_OUT_MXFP8 is internal).  Host only,
 * as yv_linear_route: dense operands and output (lda = K, ldq = N bytes), scale rows rounded up to 128; flags within YV_EPI_BIAS |
 * YV_EPI_GELU (| YV_ROUTE_M_DEV), N a multiple of 128 - what yv_linear_mxfp8_q checks, else its YV_ERR_ARG. */
int yv_linear_mxfp8_q_route(int M, int N, int K, int flags, int n_cu, yv_linear_route_t* out);
/* MX weight gradient: dW (N, K) f32 (row stride ldw) = dY^T . X over T_pad tokens, from the column forms of
 * yv_quant_mxfp8_2d: dYt (N, T_pad) bytes (row stride ldy) + scales (T_pad/128, dy_rows_pad, 4), Xt (K, T_pad) bytes (row
 * stride ldx) + scales (T_pad/128, x_rows_pad, 4).  Split over tokens through the stream's workspace (yv_set_workspace);
 * option "wgrad_mx_split" > 0 forces the number of slices (1 = no split). */
int yv_wgrad_mxfp8(const void* dYt, long long ldy, const void* sdy, long long dy_rows_pad, const void* Xt, long long ldx,
                   const void* sx, long long x_rows_pad, int T_pad, int N, int K, float* dW, int ldw, void* stream);

/* Measurement hook (bench.py): the NEXT LDS-DMA GEMM launch issued by the calling thread (yv_linear / yv_linear_ex /
 * yv_linear_nn; yv_conv2d / yv_conv2d_ws on cgemm_dma_kernel or cgemm_small_kernel; the first such launch of yv_conv2d_group,
 * grouped or single) records its start / stop timestamps into these hipEvent_t handles through hipExtLaunchKernel, i.e. from
 * the kernel's own dispatch packet.  Either may be null; the setting is consumed by that launch. */
int yv_set_launch_timing(void* start_event, void* stop_event);
/* Registers (ws != NULL) or removes a caller-owned f32 scratch buffer for split-K partial sums used by launches
 * on `stream`.  One buffer per stream: launches of a stream are ordered, different streams must not share one. */
int yv_set_workspace(void* stream, void* ws, size_t bytes);

/* ------------------------------------------------------------------ boxes */

/* custom_nms(boxes, scores, iou_threshold=0.45)  -- README.md:62-84 (== tech.md:72-94).
 * Class-agnostic greedy NMS, strict `<`, returns ORIGINAL indices in
 * (score desc, index asc) order.  Batched: set s uses rows [s*n_max, s*n_max+count[s]).
 * boxes (S,n_max,4) f32 xyxy; scores (S,n_max) f32; counts (S) i32 or NULL (= n_max);
 * keep (S,n_max) i32 (tail filled with -1); num_keep (S) i32.  n_max <= 16384. */
size_t yv_custom_nms_ws_bytes(int n_sets, int n_max);
int yv_custom_nms(const float* boxes, const float* scores, const int32_t* counts, int n_sets, int n_max,
                  float iou_threshold, int32_t* keep, int32_t* num_keep, void* ws, size_t ws_bytes, void* stream);

/* EfficientNMS_TRT output contract -- tech.md:41-47, test.ipynb:20-24 (KAT-2).
 * boxes (B,A,4) f32 xyxy; scores (B,A,nc) f32 (already sigmoid).  Outputs:
 * num_dets (B,1) i32, out_boxes (B,max_out,4) f32, out_scores (B,max_out) f32,
 * out_labels (B,max_out) i32, zero padded, sorted by score.  pre_topk <= 4096. */
int yv_efficient_nms(const float* boxes, const float* scores, int B, int A, int nc, float score_threshold,
                     float iou_threshold, int max_out, int pre_topk, int32_t* num_dets, float* out_boxes,
                     float* out_scores, int32_t* out_labels, void* stream);

/* Same contract (tech.md:41-47, test.ipynb:20-24), multi-workgroup form: the candidate filter streams the scores at
 * HBM rate over (A*nc / 4096, B) workgroups; one workgroup per image then resolves a prefix of the ranking (all the
 * sequential scan looks at before the max_out-th kept box: radix cut, rank sort, 64-wide tiles), and only images it
 * cannot finish go through the exact top-pre_topk select, per-class greedy NMS and a merge - bit-identical to
 * yv_efficient_nms.  `ws`: caller-owned scratch of yv_efficient_nms_ws_bytes() bytes, 256-byte aligned, private to the
 * call while it is in flight.  This is the form the pipeline uses; the single-kernel form above needs no scratch. */
size_t yv_efficient_nms_ws_bytes(int B, int A, int nc, int max_out, int pre_topk);
int yv_efficient_nms_ws(const float* boxes, const float* scores, int B, int A, int nc, float score_threshold,
                        float iou_threshold, int max_out, int pre_topk, int32_t* num_dets, float* out_boxes,
                        float* out_scores, int32_t* out_labels, void* ws, size_t ws_bytes, void* stream);

/* det_postprocess + coordinate restore + score filter + int cast
 * (YOLOTensorRT_yolodet_py_解读.md:82-99), then custom_nms dedupe (README.md:41,62-84),
 * then crop_image's integer inflate/clamp (utils/trainClass.py:70-93, eval branch).
 * Per image b: ratio[b], dwdh[b] (2 f32), img_wh[b] (2 i32: original width,height).
 * coord_mode 0 = trunc toward zero (Python int()), 1 = round-half-even then int.
 * Outputs per image (slots = max_out of the NMS stage, e.g. 100):
 *   det_count (B) i32            number of reported detections (score order)
 *   det_box (B,slots,4) i32      xmin,ymin,xmax,ymax in original-image pixels
 *   det_score (B,slots) f32, det_label (B,slots) i32
 *   crop_rect (B,slots,4) i32    inflated+clamped rect (x0,y0,x1,y1), right/bottom exclusive
 *   crop_ok (B,slots) i32        0 when the rect is degenerate (PIL would raise)
 * max_crops: cap of detections kept per image (<=0: no cap).                 */
int yv_postprocess_dets(const int32_t* num_dets, const float* bboxes, const float* scores, const int32_t* labels,
                        int B, int slots, const float* ratio, const float* dwdh, const int32_t* img_wh,
                        float conf_threshold, float dedupe_iou, int coord_mode, int max_crops,
                        int32_t* det_count, int32_t* det_box, float* det_score, int32_t* det_label,
                        int32_t* crop_rect, int32_t* crop_ok, void* stream);

/* Device-side compaction of the per-image crop lists into one batch:
 * crop_list (cap,6) i32 rows {image, x0, y0, x1, y1, slot}; crop_total (1) i32.
 * Order: image ascending, then detection (score) order.  Rows >= total are zeroed. */
int yv_compact_crops(const int32_t* det_count, const int32_t* crop_rect, const int32_t* crop_ok, int B, int slots,
                     int cap, int32_t* crop_list, int32_t* crop_total, void* stream);
/* The same, for a classifier that runs the crop list as `parts` (<= 64) equal slices of ceil(cap / parts) entries on concurrent
 * streams (reference site: the per-image loop of YOLOTensorRT inferdet.main, YOLOTensorRT_yolodet_py_解读.md:57-116 - batch
 * assembly has no reference counterpart): crop_total (1 + parts) i32 = {total, crops in slice 0, crops in slice 1, ...}, so
 * that no host-side or torch arithmetic on the device-resident count is needed between detect and classify. */
int yv_compact_crops_split(const int32_t* det_count, const int32_t* crop_rect, const int32_t* crop_ok, int B, int slots,
                           int cap, int parts, int32_t* crop_list, int32_t* crop_total, void* stream);

/* crop + A.Resize(224,224,INTER_NEAREST) + A.Normalize(.5,.5) + HWC->CHW
 * (utils/trainClass.py:92,218-221,265-266; app.py:39-42).
 * images: (B,H,W,3) u8 RGB with per-image byte stride img_stride; crop_list as above;
 * crop_total: device i32 (NULL = all `cap` rows valid).
 * layout 0: out = (cap,3,S,S) f32 CHW     layout 1: out = (cap,3,S,S) bf16 CHW
 * layout 2: out = (cap*(S/P)^2, 3*P*P) bf16 patch-major rows (col = c*P*P + py*P + px),
 *           the A operand of the patch-embed GEMM.  S = out_size (224), P = patch. */
int yv_crop_resize_norm(const uint8_t* images, int B, int H, int W, size_t img_stride, const int32_t* crop_list,
                        const int32_t* crop_total, int cap, int out_size, int patch, int layout, void* out,
                        void* stream);
/* One packed result record per request (yvhip.request.RequestSession): the join of crop_list with the detection arrays and the
 * classifier's outputs that YOLOTensorRT inferdet.main does per object (YOLOTensorRT_yolodet_py_解读.md:100-116), as one buffer
 * of 32-bit words that one copy brings to the host.  out (1 + cap, W) i32, W = 9 + nc:
 *   row 0      {total, B, slots, cap, nc, 0, ...} with total = min(crop_total[0], cap)
 *   row 1 + k  (k < total), from crop_list[k] = {image, x0, y0, x1, y1, slot}:
 *              {image, slot, det_box[image, slot, 0..3], det_label[image, slot], cls_label[k], bits of det_score[image, slot],
 *               bits of cls_logits[k, 0..nc)}
 *   rows past total: zero (every word of out is written on every launch).
 * The order is crop_list's: image ascending, then score order.  det_* are yv_postprocess_dets' (B, slots, ..) outputs;
 * cls_label (>= cap) i32 and cls_logits (>= cap, nc) f32 the classifier's.  One launch, no workspace, no atomics, nothing but
 * the launch in the call (it is captured into graphs).  A null pointer, B, slots or nc <= 0, cap < 0: YV_ERR_ARG, decided on the
 * host before any HIP call; cap == 0 writes the header only. */
int yv_pack_results(const int32_t* crop_list, const int32_t* crop_total, const int32_t* det_box, const float* det_score,
                    const int32_t* det_label, const int32_t* cls_label, const float* cls_logits, int B, int slots, int cap,
                    int nc, int32_t* out, void* stream);

/* Diagnostics: forced number of 16-row groups a block of the crop kernel walks (0 = chosen from the crop count). */
int yv_crop_debug(int groups_per_block);

/* letterbox (YOLOTensorRT_yolodet_py_解读.md:67-69): src (B,Hc,Wc,3) u8 canvas holding image b in its top-left
 * w x h corner; geom (B,6) i32 rows {w, h, nw, nh, left, top} (host-computed);
 * out (B,S,S,3) u8: bilinear resample into the window, 114 elsewhere. */
int yv_letterbox(const uint8_t* src, int B, int Hc, int Wc, const int32_t* geom, int S, uint8_t* out, void* stream);
/* The same kernel with a rectangular output (B,H,W,3): the stride-32 rectangles of the detector (YoloEngine(size=(H, W))).
 * H, W <= 0 or not multiples of 32: YV_ERR_ARG. */
int yv_letterbox_hw(const uint8_t* src, int B, int Hc, int Wc, const int32_t* geom, int H, int W, uint8_t* out,
                    void* stream);

/* Training augmentation of classifier crops fused with the patch-embed operand builder: replaces the stochastic part
 * of data_transforms['train'] (utils/trainClass.py:199-216: HorizontalFlip, RandomCrop+PadIfNeeded, ShiftScaleRotate,
 * ChannelShuffle, OneOf[GridDistortion|ElasticTransform], CoarseDropout) that follows Resize + Normalize.
 * x (B,3,S,S) f32 normalised crops; one host-drawn record per sample:
 *   geo (B, 6 + 2S) f32: inverse affine {a0..a5} (u = a0*cx + a1*cy + a2, v = a3*cx + a4*cy + a5), then the per-axis
 *                        distortion tables lutx[S], luty[S] (identity: lut[i] = i);
 *   idx (B, 36 + 2S) i32: source channel of output channel 0..2, hole count (0..8), 8 holes {x1,y1,x2,y2} (exclusive
 *                        right/bottom), then integer column / row tables mapx[S], mapy[S] (flip, crop offset + reflected pad).
 * Sampling is bilinear with BORDER_REFLECT_101 in the flipped / crop-padded frame; holes are filled with 0.
 * out (B*(S/P)^2, 3*P*P) bf16 patch-major rows (same layout as yv_crop_resize_norm layout 2). */
int yv_augment_patchify(const float* x, int B, int S, int P, const float* geo, const int32_t* idx, void* out, void* stream);

/* Classifier training / validation crops straight out of decoded source images (device-resident crop loader): replaces
 * crop_image + the Resize / Normalize head of both transforms + the per-item tensor work of build_dataset
 * (utils/trainClass.py:70-93, :199-221, :250-273), fused with what yv_augment_patchify does.  Per output value it is exactly
 * yv_augment_patchify applied to the S x S crop that yv_crop_resize_norm (layout 0) would produce; that crop is never stored.
 *   pool   (pool_bytes) u8: every source image, RGB, row-major, tightly packed, one after the other;
 *   table  (n_images, 3) i64 rows {byte offset into the pool, width, height};
 *   plan   (B, 5) i32 rows {image id, x0, y0, x1, y1}: crop rectangle, right / bottom exclusive (the crop_list convention);
 *   geo (B, 6 + 2S) f32, idx (B, 36 + 2S) i32: the records of yv_augment_patchify (identity records for validation).
 * layout 2: out = (B*(S/P)^2, 3*P*P) bf16 patch-major rows; layout 0: out = (B,3,S,S) f32 CHW (P unused).  S % 8 == 0.
 * Every input is clamped, never trusted: image id to [0, n_images-1]; width / height to [1, 2^24]; rectangle extents
 * w = max(x1-x0, 1), h = max(y1-y0, 1); table entries mapx / mapy to [0, S-1]; source column
 * clamp(x0 + min(floor(m * (1/(S/w))), w-1), 0, width-1) (f64, rows alike); tap byte address clamp(offset + 3*(row*width + col),
 * 0, pool_bytes-3); channel ids to [0,2], hole count to [0,8], affine coordinates to [-4S, 4S] (NaN -> -4S). */
int yv_train_crops(const uint8_t* pool, size_t pool_bytes, const int64_t* table, int n_images, const int32_t* plan, int B, int S,
                   int P, const float* geo, const int32_t* idx, int layout, void* out, void* stream);

/* Detector training augmentation, what `model.train()` (utils/trainYolo.py:28) applies by default: Mosaic(4) ->
 * RandomPerspective(scale, translate) -> HSV gains -> horizontal flip in one gather pass per output image.
 * tiles (n_tiles,S,S,3) u8: sources resized to long side S in the top-left corner of their slot (yv_letterbox, fill 114).
 *   rec_f (B,6) f32: inverse affine, output pixel -> mosaic-canvas coordinate;
 *   rec_i (B,34) i32: {tiles used (1..4), flip}, then per tile {id, x1a, y1a, x2a, y2a, x1b, y1b, 0}: the canvas rectangle
 *                     [x1a,x2a) x [y1a,y2a) shows tile `id` starting at its pixel (x1b, y1b);
 *   lut (B,3,256) u8: hue / saturation / value tables applied in 8-bit HSV (H in [0,180)).
 * Bilinear; canvas pixels outside every rectangle are 114.  out (B,S,S,3) u8 NHWC (the detector's input layout). */
int yv_mosaic_augment(const uint8_t* tiles, int n_tiles, int B, int S, const float* rec_f, const int32_t* rec_i,
                      const uint8_t* lut, uint8_t* out, void* stream);

/* The same pass for the non-default knobs of the detector trainer (degrees, shear, perspective, flipud, mixup).
 * `layers` is 1 or 2; per image b and layer L:
 *   rec_h (B,layers,9) f32: inverse homography, output pixel -> canvas: w = (h6*xs + h7*ys) + h8,
 *                           u = ((h0*xs + h1*ys) + h2) / w, v = ((h3*xs + h4*ys) + h5) / w; where !(w > 0) the layer
 *                           shows the fill value 114;
 *   rec_i (B,layers,34) i32: per layer as above; the flip word rec_i[b,0,1] (bit 0 mirrors x, bit 1 mirrors y) applies to
 *                           both layers;
 *   mix (B) f32: weight m = clamp(mix, 0, 1) of layer 0 (NaN -> 0); the layers, each a whole 8-bit value, blend to
 *                           floor(m*c0 + (1-m)*c1) before the HSV tables.  May be null when layers == 1.
 * With layers == 1 and the last row (0, 0, 1) the output equals yv_mosaic_augment on the same record bit for bit.
 * A null pointer, layers outside {1, 2} or a null mix with layers == 2: YV_ERR_ARG. */
int yv_mosaic_augment_ex(const uint8_t* tiles, int n_tiles, int B, int S, int layers, const float* rec_h,
                         const int32_t* rec_i, const float* mix, const uint8_t* lut, uint8_t* out, void* stream);

/* DFL decode + anchors + sigmoid (docs/YOLO_TensorRT_Technical.md:14-30,72-77).
 * Per scale s (3 scales, strides 8/16/32): box logits (B,Hs,Ws,64) f32 and class
 * logits (B,Hs,Ws,cls_ld) f32, NHWC.  Outputs boxes (B,A,4) f32 xyxy input pixels,
 * scores (B,A,nc) f32; anchor order = scale, then y*W+x. */
int yv_detect_decode(const float* box0, const float* box1, const float* box2, const float* cls0, const float* cls1,
                     const float* cls2, int cls_ld, int B, int size, int nc, float* boxes, float* scores,
                     void* stream);
/* The same for an H x W network input (both multiples of 32, else YV_ERR_ARG): Hs = H / stride, Ws = W / stride, anchor order
 * = scale, then y*Ws+x, A = sum Hs*Ws.  yv_detect_decode is this with H = W = size. */
int yv_detect_decode_hw(const float* box0, const float* box1, const float* box2, const float* cls0, const float* cls1,
                        const float* cls2, int cls_ld, int B, int H, int W, int nc, float* boxes, float* scores,
                        void* stream);

/* Fused Detect tail: the last 1 x 1 convolutions of both branches (ultralytics Detect cv2.i.2: 64 -> 4 x reg_max box logits,
 * cv3.i.2: c3 -> nc class logits; TensorRT builder docs/YOLO_TensorRT_Technical.md:160-212) + yv_detect_decode, three scales in
 * one launch; bit-identical to the unfused sequence.  feat_s (B*Hs*Ws, ld) bf16: box-branch features in channels 0..63, class
 * branch features in 64..64+c3-1.  w2[s] (64,64) bf16, b2[s] (64) f32, w3[s] (16,c3) bf16 with rows >= nc zero, b3[s] (16) f32
 * (host arrays of three device pointers).  c3 in {64,128,192}, nc <= 16; otherwise YV_ERR_LIMIT (use the unfused path). */
int yv_detect_tail(const void* feat0, const void* feat1, const void* feat2, int ld, int c3, const void* const* w2,
                   const float* const* b2, const void* const* w3, const float* const* b3, int B, int size, int nc,
                   float* boxes, float* scores, void* stream);
/* The same for an H x W network input (both multiples of 32, else YV_ERR_ARG); yv_detect_tail is this with H = W = size. */
int yv_detect_tail_hw(const void* feat0, const void* feat1, const void* feat2, int ld, int c3, const void* const* w2,
                      const float* const* b2, const void* const* w3, const float* const* b3, int B, int H, int W, int nc,
                      float* boxes, float* scores, void* stream);

/* ------------------------------------------------------------ dense math */

/* Operand view for the implicit-GEMM kernel: NHWC bf16 tensor slice.
 * up = 1: the tensor is read through a nearest 2x upsample (K4). */
typedef struct yv_view {
    const void* ptr; /* bf16 */
    int ld;          /* elements between consecutive pixels */
    int c;           /* channels read from this view        */
    int up;          /* 0 | 1                               */
} yv_view;

/* epilogue flags */
#define YV_EPI_BIAS 1
#define YV_EPI_SILU 2
#define YV_EPI_GELU 4       /* exact erf GELU */
#define YV_EPI_RES_F32 8    /* out_f32 += (read-modify-write residual stream) */
#define YV_EPI_RES_BF16 16  /* + bf16 residual view (Bottleneck shortcut)     */
#define YV_EPI_OUT_F32 32   /* store f32 instead of bf16                      */
#define YV_EPI_POSEMB 64    /* patch-embed row remap + pos_embed add          */
#define YV_EPI_SAVE_PRE 128 /* also store the pre-activation (bf16) to `aux`   */
#define YV_EPI_GELU_BWD 256 /* out = acc * gelu'(aux)  (MLP backward)         */
#define YV_EPI_OUT_MXFP8 512 /* internal to yv_linear_mxfp8_q: e4m3 + E8M0 output */

/* Conv2d(k in {1,3}, stride in {1,2}, pad k/2) + folded-BN bias + SiLU as an
 * implicit GEMM on MFMA (ultralytics Conv/C2f/SPPF/Detect convs; structure per
 * docs/YOLO_TensorRT_Technical.md:160-212, fusion per test.ipynb:25,1285).
 * in0 (+ optional in1 = channel concat, 1x1 only) are (B,Hin,Win,*) views;
 * weight (Cout, k*k*Cin) bf16 with K order (ky,kx,cin); bias (Cout) f32;
 * out = (B,Hout,Wout,*) view with pixel stride out_ld (bf16, or f32 with YV_EPI_OUT_F32);
 * res = optional bf16 residual view (same pixel grid as out).
 * Limits: the fused 2x upsample (yv_view.up) is a property of 1x1 inputs (YV_ERR_ARG with ksize 3); the kernel
 * addresses each source and the weights with 32-bit byte offsets: a batch whose source passes 2 GB is taken in
 * sub-batches by this entry, one IMAGE (Hin*Win*ld*2) and the weights (Cout*k*k*Cin*2) must stay below 2 GB
 * (YV_ERR_LIMIT).
 * Epilogue order: bias -> SiLU -> + bf16 residual -> store.  With YV_EPI_RES_BF16 and a bf16 output the number of roundings
 * depends on the route (yv_conv2d_instance reports it):
 *   direct epilogue (staged bit clear: 16- / 32-wide tiles, an output or residual that is not 16-byte aligned with a stride
 *   that is a multiple of 8, "staged_epilogue" = 0, split-K):  out = bf16(y + r), ONE rounding;
 *   staged epilogue (staged bit set: every LDS-DMA route, the 64- / 128-wide tiles otherwise):  out = bf16(bf16(y) + r), the
 *   activation is rounded to bf16 BEFORE the residual is added, TWO roundings.
 * Without a residual, and with YV_EPI_OUT_F32, both forms give the same bits. */
int yv_conv2d(const yv_view* in0, const yv_view* in1, int B, int Hout, int Wout, int ksize, int stride,
              const void* weight, const float* bias, int Cout, void* out, int out_ld, const void* res, int res_ld,
              int flags, void* stream);

/* Diagnostic, host only (no HIP call, except that once "conv_small" is set the CU count of the then-current device is queried
 * and kept for the life of the process - one kind of device per process is assumed; 256 where there is no device):
 * the route yv_conv2d_ws takes for this shape under the current options, for dense sources
 * (pixel stride = c0 / c1, no upsample - neither changes the route) and base pointers aligned to 16 bytes (a base that is not
 * clears the staged bit and with it every LDS-DMA route); ws_bytes = 0: no workspace (yv_conv2d).  For a batch that is taken in
 * sub-batches, the route of the first one.  Returns a negative YV_ERR_* code where yv_conv2d rejects the arguments, else
 *   bits 0-3  kernel instance: 0 .. 3 igemm_kernel with 128 x 16 / 32 / 64 / 128 tiles;
 *             4 cgemm_dma_kernel<64,4,1,2>, 5 <64,4,1,3>, 6 <64,4,1,4>, 7 <128,2,2,2>, 8 <128,2,2,3>  (<tile width, waves, stages>);
 *             9 cgemm_small_kernel<64,2>, 10 <32,4>  (<tile rows, K groups>; only with the option "conv_small" > 0: at most that
 *             many output pixels, 128 x 64 tiles at most "conv_small_fill" eighths of the CU count, eligibility of 4 .. 8; they
 *             take the direct epilogue, so bit 4 is clear);
 *             11 cgemm_dma32_kernel<64,4,1,3>, 13 <128,2,2,2>  (<tile width, waves, stages>; only with the option "conv_dma32"
 *             != 0, which is 0 by default: Cout >= 64, every source a multiple of 32 channels but not what 4 .. 8 ask (64), one
 *             source or a 1 x 1, a stageable output, no device row count, no split-K, a plain yv_conv2d / yv_conv2d_ws call;
 *             "conv_dma32_cols" = 64 / 128 forces that instance, any other value is the measured rule of conv_route, which
 *             leaves Cout = 64 on igemm_kernel; both take the staged epilogue; 12 is the 96-wide instance, which measured
 *             fastest on no layer and is not built: no route reports it)
 *   bit 4 (16) the staged epilogue runs (see yv_conv2d for what that means for the shortcut's rounding)
 *   bit 5 (32) split-K: partial sums in the workspace, epilogue in the reduce pass
 *   bit 6 (64) the two-source instantiation of igemm_kernel (c1 > 0; the LDS-DMA kernels have no separate one). */
int yv_conv2d_instance(int B, int Hout, int Wout, int ksize, int stride, int c0, int c1, int Cout, int out_ld, int res_ld,
                       int flags, size_t ws_bytes);

/* Grouped convolution launch (opt-in: YoloEngine(grouped_head=True)): n independent yv_conv2d problems,
 * the eligible ones as ONE grid per kernel instance.  A member is the argument list of yv_conv2d (in1.ptr null: one source). */
#define YV_CONV_GROUP_MAX 8   /* members of one grouped launch: their descriptors travel in the 4 KB kernel-argument segment */
typedef struct yv_conv2d_desc {
    yv_view in0, in1;
    int B, Hout, Wout, ksize, stride;
    const void* weight;
    const float* bias;
    int Cout;
    void* out;
    int out_ld;
    const void* res;
    int res_ld;
    int flags;
} yv_conv2d_desc;

/* Runs the n members.  Each member is routed as yv_conv2d routes it alone (no workspace, hence never split-K) under the current
 * options.  Members on cgemm_dma_kernel<64,4,1,3>, cgemm_small_kernel<64,2> or cgemm_small_kernel<32,4> (instance 5, 9, 10 of
 * yv_conv2d_instance) that yv_conv2d would not take in sub-batches are eligible: per instance they are ordered by descending work
 * (tiles x K steps) and issued YV_CONV_GROUP_MAX at a time as one launch each, a single leftover member as its ordinary launch.
 * Every other member (igemm_kernel, the 128-wide tiles, a sub-batched call) is then launched alone, in the order given.
 * yv_conv2d_group_plan reports the partition.
 * Each member's output is, bit for bit, what yv_conv2d writes for that member alone under the same options.
 * The argument rules are yv_conv2d's, per member, and all are checked before anything is launched: the first member that breaks
 * one gives its code and nothing has run.  n <= 0, a null d, or two members with the same `out` pointer: YV_ERR_ARG.  Beyond that
 * it is the CALLER's contract that no member reads (source, residual) what another member writes, and that no two members'
 * outputs overlap: the members run concurrently, in no order. */
int yv_conv2d_group(const yv_conv2d_desc* d, int n, void* stream);

/* Host only, in the manner of yv_conv2d_instance (nothing is dereferenced or launched; works without a device): the partition
 * yv_conv2d_group makes of n members of these shapes (dense sources, 16-byte aligned bases, distinct outputs) under the current
 * options, decided by the function yv_conv2d_group itself uses.  out[i] describes member i. */
typedef struct yv_conv2d_shape {
    int B, Hout, Wout, ksize, stride, c0, c1, Cout, out_ld, res_ld, flags;
} yv_conv2d_shape;
typedef struct yv_conv2d_group_plan_t {
    int launch;     /* index of the launch that runs the member, in issue order: the grouped launches first, then the single ones */
    int instance;   /* the member's yv_conv2d_instance code (ws_bytes = 0) */
    int first_wg;   /* its first workgroup in that launch's grid, a multiple of 8 (0 for a member launched alone) */
    int position;   /* its position among the members of that launch (descending work) */
    int work;       /* tiles x K steps of the member on its instance */
} yv_conv2d_group_plan_t;
/* Returns YV_OK and fills out[0 .. n) and *n_launches (a member yv_conv2d takes in sub-batches counts as one launch), or the
 * YV_ERR_* code with which yv_conv2d_group would reject the arguments. */
int yv_conv2d_group_plan(const yv_conv2d_shape* shapes, int n, yv_conv2d_group_plan_t* out, int* n_launches);

/* MXFP8 convolutions (BASELINE.json configs[4]: FP8 detector convolutions; opt-in, YoloEngine(dtype="mxfp8")).
 * An "MX map" is an NHWC activation in the operand format of the block-scaled MFMA: e4m3 bytes q (B,H,W,ld) and one E8M0
 * scale byte per (pixel, 32-channel block) s (B,H,W,ld/32).  A view points at the first channel it reads in both arrays
 * (q + c_off, s + c_off/32); c_off, c and ld are multiples of 32.  up = 1: read through a nearest 2x upsample (1x1 only). */
typedef struct yv_mx_view {
    const void* q;   /* e4m3 bytes                                    */
    const void* s;   /* E8M0 scales, pixel stride ld/32 bytes         */
    int ld;          /* bytes (= channels) between consecutive pixels */
    int c;           /* channels read from this view                  */
    int up;          /* 0 | 1                                         */
} yv_mx_view;

/* bf16 NHWC view x (pixels rows, pixel stride ldx elements, C channels read) -> MX map (q pixel stride ldq bytes, scales
 * pixel stride ldq/32 bytes), the rule of yv_quant_mxfp8: e = ceil(log2(amax/448)) per 32 channels of a pixel (all-zero
 * blocks e = -127), q = RNE_e4m3(x * 2^-e).  C, ldq multiples of 32, ldx of 8; x, q 16-byte aligned. */
int yv_quant_mxfp8_map(const void* x, long long ldx, long long pixels, int C, void* q, long long ldq, void* scales,
                       void* stream);

/* yv_conv2d on MX operands: in0 (+ in1, 1x1 only) MX maps, wq (Cout, Kpad) e4m3 with K order (ky,kx,cin) zero-padded to
 * Kpad = k*k*Cin rounded up to 128, wscale K-step-major (Kpad/128, w_rows_pad, 4) exactly as yv_quant_mxfp8 writes it.
 * Epilogue as yv_conv2d (bias, SiLU, bf16 residual), then either or both of
 *   out_bf16: bf16 view with pixel stride out_ld (f32 with YV_EPI_OUT_F32),
 *   out_q / out_scales: MX map (pixel strides outq_ld / outq_ld/32 bytes) of the bf16-rounded result - byte-identical to
 *   out_bf16 followed by yv_quant_mxfp8_map (not with YV_EPI_OUT_F32).
 * NULL for an output that is not wanted.  Requires Cin % 32 == 0 per source, Cout % 32 == 0.  Each image and the weights
 * stay below 2 GB (larger batches are taken in sub-batches). */
int yv_conv2d_mxfp8(const yv_mx_view* in0, const yv_mx_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                    const void* wq, const void* wscale, long long w_rows_pad, const float* bias, int Cout, void* out_bf16,
                    int out_ld, void* out_q, void* out_scales, int outq_ld, const void* res, int res_ld, int flags,
                    void* stream);
/* Diagnostic: the kernel instance yv_conv2d_mxfp8 launches for this shape (0: 128 x 64 tiles, 1: 128 x 128 tiles), or
 * a negative YV_ERR_* code if the shape is not accepted. */
int yv_conv2d_mxfp8_instance(int B, int Hout, int Wout, int ksize, int stride, int Cin, int Cout);

/* One launch for a whole C2f block of the detector backbone (ultralytics C2f with shortcut, as in layers model.2 / model.4 of the
 * YOLOv8 models the reference loads - utils/utils.py:126, test.ipynb): cv1 (1x1, 2c -> 2c), n bottlenecks of two 3x3 layers
 * c -> c with the residual add, cv2 (1x1, (2+n)c -> 2c), SiLU after every layer (BN folded).  x (B,H,W,>=2c) bf16 with pixel
 * stride ldx, out (B,H,W,>=2c) bf16 with pixel stride ldo; weights (Cout, k*k*Cin) bf16 with K order (ky,kx,cin) and f32
 * biases exactly as yv_conv2d takes them; w_m / b_m: 2n entries {m0.cv1, m0.cv2, m1.cv1, m1.cv2}.  c in {16, 32}, n in {1, 2}
 * (anything else: YV_ERR_ARG - run the block layer by layer).  Same arithmetic per output as the layer-by-layer path at these
 * widths (K order, f32 accumulation, bias -> SiLU -> + residual -> one bf16 rounding: layers of 16 / 32 output channels take
 * yv_conv2d's direct epilogue.  Wider Bottlenecks, c >= 64, run layer by layer on the staged epilogue, which rounds the
 * activation to bf16 BEFORE it adds the shortcut - see yv_conv2d). */
int yv_c2f_fused(const void* x, long long ldx, int B, int H, int W, int c, int n, const void* w_cv1, const float* b_cv1,
                 const void* const* w_m, const float* const* b_m, const void* w_cv2, const float* b_cv2, void* out,
                 long long ldo, void* stream);
/* Diagnostics: buf = 64 x 8 uint64 on the device receives cycle stamps (phase boundaries of wave 0 of the first 64 workgroups)
 * of every following yv_c2f_fused launch; NULL switches them off. */
int yv_c2f_debug(void* buf);

/* Same, with a caller-owned f32 workspace: deep small-resolution layers then run split-K (K range sliced over
 * several workgroups per tile + a reduce/epilogue pass).  ws_bytes >= 8 * M * Cout * 4 enables every split. */
int yv_conv2d_ws(const yv_view* in0, const yv_view* in1, int B, int Hout, int Wout, int ksize, int stride,
                 const void* weight, const float* bias, int Cout, void* out, int out_ld, const void* res, int res_ld,
                 int flags, void* ws, size_t ws_bytes, void* stream);

/* yv_conv2d_ws with the BatchNorm batch statistics of its output taken in the epilogue (opt-in: YoloTrainer(fused_bn_stats=True)).
 * out (bf16) receives the same bits yv_conv2d_ws writes for the same arguments.  Every workgroup also writes, for its tile of
 * 128 rows (tm = first row / 128) and each of its columns n < Cout,
 *   stats_ws[(tm * 2 + 0) * Cout + n] = sum over the tile's rows m < B*Hout*Wout of v,   stats_ws[(tm * 2 + 1) * Cout + n] = sum of v * v,
 * v = the bf16-rounded value stored to out, back in f32; f32 sums in an order the code fixes (bitwise reproducible), each float
 * written by one plain store (nothing is zeroed or accumulated in memory).  This is the (chunks, 2, C) layout of yv_bn_stats'
 * first stage with chunks = ceil(T / 128); yv_bn_stats_finish turns it into mean / rstd.
 * Accepted: one source, bf16 output, flags = 0 or YV_EPI_BIAS (anything else YV_ERR_ARG), Cout % 8 == 0, the other argument
 * rules of yv_conv2d.  A batch yv_conv2d_ws would take in sub-batches (a source beyond 2 GB) is YV_ERR_LIMIT: the tiles are one
 * sequence.  stats_ws_floats < yv_conv_stats_ws_floats(B*Hout*Wout, Cout): YV_ERR_WORKSPACE.  All of these are decided on the
 * host before any HIP call.  The call never splits K (ws / ws_bytes are accepted for symmetry with yv_conv2d_ws); otherwise its
 * route is yv_conv2d_ws's: yv_conv2d_instance under "conv_splitk" = 0 reports it. */
int yv_conv2d_stats(const yv_view* in0, int B, int Hout, int Wout, int ksize, int stride, const void* weight,
                    const float* bias, int Cout, void* out, int out_ld, int flags, float* stats_ws, size_t stats_ws_floats,
                    void* ws, size_t ws_bytes, void* stream);
/* Floats of yv_conv2d_stats' workspace for T output rows: ceil(T / 128) * 2 * Cout tile partials and, where there are more
 * than 2048 tiles, the chunk partials yv_bn_stats_finish folds them into (at most 2048 * 2 * Cout).  0 for T or Cout <= 0. */
size_t yv_conv_stats_ws_floats(long long T, int Cout);

/* yv_conv2d_ws as a DATA GRADIENT that also takes the two reductions of the BatchNorm backward of the block that produced its
 * target (opt-in: YoloTrainer(fused_bn_bwd=True)).  out (bf16) is the gradient da of that block's output and receives the bits
 * yv_conv2d_ws writes for the same arguments under "conv_splitk" = 0.  z (row stride ldz), mean, rstd, gamma, beta (Cout floats
 * each) and act are the producer's operands as yv_bn_act_bwd takes them.  Every workgroup also writes, for its tile of 128 rows
 * (tm = first row / 128) and each of its columns n < Cout,
 *   stats_ws[(tm * 2 + 0) * Cout + n] = sum over the tile's rows m < B*Hout*Wout of g,   stats_ws[(tm * 2 + 1) * Cout + n] = sum of g * xhat,
 * xhat = (z - mean) * rstd, g = d * act'(gamma * xhat + beta), d = the bf16-rounded value stored to out, back in f32: term by
 * term what yv_bn_act_bwd's first pass adds (one device text), in the summation order and layout of yv_conv2d_stats (each float
 * one plain store, nothing zeroed or accumulated in memory, bitwise reproducible).  Rows of z at or behind B*Hout*Wout are not
 * read.  yv_bn_act_bwd_finish turns the partials into dgamma, dbeta and dz.
 * Accepted: one source, bf16 output, flags of YV_EPI_BIAS | YV_EPI_RES_BF16 only (anything else YV_ERR_ARG), Cout % 8 == 0,
 * ldz % 8 == 0, ldz >= Cout, act 0 or 1, 16-byte aligned z, out, res, stats_ws and constants, the other argument rules of
 * yv_conv2d.  A batch yv_conv2d_ws would take in sub-batches is YV_ERR_LIMIT; stats_ws_floats <
 * yv_conv_bnbwd_ws_floats(B*Hout*Wout, Cout) is YV_ERR_WORKSPACE.  All of these are decided on the host before any HIP call.
 * The call never splits K (ws / ws_bytes are accepted for symmetry). */
int yv_conv2d_bnbwd(const yv_view* in0, int B, int Hout, int Wout, int ksize, int stride, const void* weight, const float* bias,
                    int Cout, void* out, int out_ld, const void* res, int res_ld, int flags, const void* z, int ldz,
                    const float* mean, const float* rstd, const float* gamma, const float* beta, int act, float* stats_ws,
                    size_t stats_ws_floats, void* ws, size_t ws_bytes, void* stream);
/* Floats of yv_conv2d_bnbwd's workspace: yv_conv_stats_ws_floats(T, Cout) + 2 * Cout (the finaliser's mean(g), mean(g * xhat),
 * behind the partials).  0 for T or Cout <= 0. */
size_t yv_conv_bnbwd_ws_floats(long long T, int Cout);

/* The route of yv_conv2d_bnbwd for a data gradient (B, Hout, Wout) x Cin (pixel stride in_ld) -> Cout, decided by the function the
 * launch path itself calls.  Host only: nothing is dereferenced, launched or queried; 16-byte aligned bases are assumed; flags,
 * out_ld, res_ld, ldz as the call takes them; ws_bytes is the split-K workspace yv_conv2d_ws would be given for the same call.
 * Returns a negative YV_ERR_* code where yv_conv2d_bnbwd rejects the arguments, else YV_OK and *out. */
typedef struct {
    int kernel;     /* instance, numbered as yv_conv2d_instance bits 0-3, in its BNBWD form */
    int staged;     /* 1: the staged epilogue runs (16-byte z loads), 0: the direct one (8-byte z loads) */
    int tiles;      /* 128-row tiles = rows of the partials */
    int workgroups; /* the launch: tiles x column tiles */
    int splitk;     /* 1: yv_conv2d_ws would split K for the same call under the current options */
    int use;        /* 0: keep yv_conv2d_ws + yv_bn_act_bwd - where splitk is 1 (the unfused call's bits are a split sum's) and where
                       the fused pair was measured slower: the 64- / 128-wide instances at >= 100,000 rows, the 32-wide one at
                       >= 400,000 rows with K >= 512 */
} yv_conv_bnbwd_route_t;
int yv_conv2d_bnbwd_route(int B, int Hout, int Wout, int ksize, int stride, int Cin, int in_ld, int Cout, int out_ld, int res_ld,
                          int ldz, int flags, size_t ws_bytes, yv_conv_bnbwd_route_t* out);

/* Linear: out[M,N] = A[M,K] @ W[N,K]^T (+bias)(+GELU)(+residual) on MFMA
 * (timm Attention.qkv/proj, Mlp.fc1/fc2, head; README.md:21-35).
 * A (M,K) bf16 row stride lda; W (N,K) bf16; bias (N) f32.
 * m_dev: optional device i32; rows at run time = min(M, m_dev[0]*m_mul) (tiles beyond exit):
 *        the crop count of a batch is only known on the device (no host sync).
 * YV_EPI_POSEMB: row m -> out row (m/tok)*(tok+1)+1+(m%tok), adds pos[(1+m%tok)*N + n]. */
int yv_linear(const void* A, int lda, const void* W, const float* bias, int M, int N, int K, void* out, int ldo,
              const float* pos, int tok, int flags, const int32_t* m_dev, int m_mul, void* stream);

/* Training form of yv_linear: res_f32 = separate f32 residual source (out = res_f32 + acc + bias, so the
 * residual stream of every layer can be kept for backward); aux/ldaux = bf16 side buffer for
 * YV_EPI_SAVE_PRE / YV_EPI_GELU_BWD.  Requires K % 64 == 0, N > 64 and 16-byte aligned rows. */
int yv_linear_ex(const void* A, int lda, const void* W, const float* bias, int M, int N, int K, void* out, int ldo,
                 int flags, const float* res_f32, void* aux, int ldaux, void* stream);

/* LayerNorm over the last dim (timm blocks.*.norm1/2, norm; eps 1e-6; README.md:21-29).
 * x (rows, D) f32 with row stride ldx -> y (rows, D) bf16 row stride ldy.
 * count_dev: optional device i32; rows at run time = min(rows, count_dev[0]*rows_per_count).
 * D, ldx, ldy multiples of 4; x, gamma, beta 16-byte aligned and y 8-byte aligned (YV_ERR_ARG, checked on the host before any
 * HIP call: the kernel reads float4 and writes uint2); D <= 1024 (YV_ERR_LIMIT). */
int yv_layernorm(const float* x, size_t ldx, const float* gamma, const float* beta, int rows, int D, float eps,
                 void* y, size_t ldy, const int32_t* count_dev, int rows_per_count, void* stream);

/* LayerNorm + Linear, the norm1 -> qkv and norm2 -> fc1 steps of a timm Block (README.md:21-29):
 *   out[M,N] = LayerNorm(x[M,K]; gamma[K], beta[K], eps) @ w[N,K]^T (+bias)(+GELU), bf16 or (YV_EPI_OUT_F32) f32, row stride ldo
 * x f32 with row stride ldx, w bf16, h (M,K) bf16 with row stride ldh: the LayerNorm output where the call writes it.
 * Where yv_linear_ln_route answers fused = 1 the call is ONE launch of gemm_mid_ln_kernel - gemm_mid_kernel's 64 x 64 tiles, each
 * computing the statistics of its 64 rows and normalising them while it stages them - and h is not touched.  Everywhere else it
 * is yv_layernorm into h followed by yv_linear, the two launches of a caller without this entry.  Either way `out` has the bits of
 * yv_layernorm followed by yv_linear on the YV_LIN_MID route.
 * Fused: "linear_variant" 1, 256 < M <= option "linear_ln_mid" (0, the default: never) and the shape makes at most option
 * "linear_ln_fill" eighths of the CU count in 128 x 128 tiles.  "linear_ln_fill" ships at 0 - no shape: the fused launch measured
 * slower than the pair at every shape - and is raised by tools/ln_mid_bench.py and the tests.
 * Checked before anything is launched, whatever the route: K % 64 == 0, N % 64 == 0, ldx % 4 == 0, ldh % 8 == 0, ldo % 4 == 0,
 * strides not below the row length, flags within YV_EPI_BIAS | YV_EPI_GELU | YV_EPI_OUT_F32, bias where its flag is set, every
 * pointer 16-byte aligned (YV_ERR_ARG); K <= 1024 (YV_ERR_LIMIT).  m_dev / m_mul as in yv_linear. */
int yv_linear_ln(const float* x, size_t ldx, const float* gamma, const float* beta, float eps, void* h, int ldh, const void* w,
                 const float* bias, void* out, int ldo, int M, int N, int K, int flags, const int32_t* m_dev, int m_mul,
                 void* stream);
/* The decision yv_linear_ln makes for this shape and flags under the current options, by the function the entry itself calls.
 * Host only.  n_cu as in yv_linear_route.  A shape or flag set the fused kernel does not take answers fused = 0 (the entry may
 * still reject it).  fused = 0: the other fields are 0. */
typedef struct {
    int fused;            /* 1: one launch of gemm_mid_ln_kernel, 0: yv_layernorm + yv_linear */
    int tiles_m, tiles_n; /* 64 x 64 tiles of the fused launch: ceil(M / 64), N / 64 */
    int workgroups;       /* tiles_m * tiles_n */
} yv_linear_ln_route_t;
int yv_linear_ln_route(int M, int N, int K, int flags, int n_cu, yv_linear_ln_route_t* out);

/* Residual Linear + LayerNorm in one launch (timm Block: x = x + proj(attn) followed by norm2, x = x + fc2(mlp) followed
 * by the next block's norm1; README.md:21-29):
 *   x[M,N] (f32, row stride ldx, read-modify-write) = x + a[M,K] (bf16, row stride lda) @ w[N,K]^T (bf16) + bias[N] (f32)
 *   h[M,N] (bf16, row stride ldh)                   = LayerNorm(x; gamma[N], beta[N], eps), statistics in f32, two-pass
 * One kernel for every M (64-row tiles that span the output row; persistent, grid = "linear_p8_cus" budget of the calling thread).
 * N in {128, 768, 1024}, K % 64 == 0, K >= 128, strides multiples of 8 elements, every pointer 16-byte aligned (YV_ERR_ARG,
 * checked on the host before any HIP call); a, w, x, h are addressed with 32-bit byte offsets (YV_ERR_LIMIT past 2 GB).
 * m_dev / m_mul as in yv_linear: rows >= min(M, m_dev[0]*m_mul) are neither read-modify-written in x nor written in h.
 * A row's two outputs depend on that row's inputs only: bit-identical whatever M, the device count and the grid size. */
int yv_linear_res_ln(const void* a, int lda, const void* w, const float* bias, int M, int N, int K, float* x, int ldx,
                     const float* gamma, const float* beta, float eps, void* h, int ldh, const int32_t* m_dev, int m_mul,
                     void* stream);

/* Fused attention forward, non-causal: softmax(Q K^T * scale) V (timm Attention; README.md:21-23).
 * qkv (R*N, 3*H*64) bf16 as produced by the qkv Linear ([q|k|v], head-major);
 * out (R*N, H*64) bf16.  head dim 64; N <= 256 is one K/V tile (ViT-x/16: 197), longer sequences
 * (ViT-B/8: 785) are tiled with an online softmax. */
int yv_attention(const void* qkv, int R, int N, int H, float scale, void* out, const int32_t* r_dev, void* stream);

/* Attention of the cls query only (row 0 of each crop), for the last block of the classifier, whose other rows nothing reads:
 * out[r, h*64 ..] = softmax(q[r, h] . K_r^T * scale) . V_r for r < min(R, r_dev[0]); rows past the count keep their contents.
 * q (R, H*64) bf16 compact; K and V are read from the ordinary qkv buffer (R*N, 3*H*64) (its q third is not read);
 * out (R, H*64) bf16 compact.  q, qkv, out 16-byte aligned (YV_ERR_ARG); N <= 8192 (YV_ERR_LIMIT). */
int yv_attention_cls(const void* q, const void* qkv, int R, int N, int H, float scale, void* out, const int32_t* r_dev,
                     void* stream);

/* Attention forward for sequences longer than one K/V tile (ViT-B/8 at 224: 785 tokens; ViT-x/16 at 384: 577); the same product
 * as yv_attention from another kernel: 128-row query blocks whose last one has only its live 32-row waves, 64-key K/V tiles
 * double-buffered in LDS with the next tile's fetch under the current tile's work, an online softmax per 32-key group, key groups
 * wholly past N skipped.  Any N >= 1 is accepted; the engines use it for N > 224 (VitEngine / VitTrainer long_attn).
 * qkv (R*N, 3*H*64) bf16.  Outputs, any combination with at least one of out / out_q:
 *   out (R*N, H*64) bf16, or NULL;
 *   lse (R, H, N) f32, log2 domain (m * scale * log2 e + log2 l: the input of yv_attention_bwd), or NULL;
 *   out_q / out_scales: the MXFP8 operand image of yv_attention_mxfp8 (same numbers as out followed by yv_quant_mxfp8), both or
 *   neither (NULL, 0, NULL, 0): H even, ldq % 16 == 0, ldq >= 64 H, rows_pad % 128 == 0, rows_pad >= R*N;
 *   r_dev: device-side crop count, or NULL; crops >= min(r_dev[0], R) are not touched.
 * qkv, out, out_q 16-byte aligned; breaking a rule is YV_ERR_ARG, a grid past 2^31 - 1 workgroups YV_ERR_LIMIT; R = 0 is YV_OK
 * without a launch.  Addresses are 64-bit: no 2 GB limit.  A crop's outputs depend on that crop's inputs only: bit-identical
 * whatever R, the crop's index and the grid. */
int yv_attention_long(const void* qkv, int R, int N, int H, float scale, void* out, const int32_t* r_dev, float* lse,
                      void* out_q, long long ldq, void* out_scales, long long rows_pad, void* stream);

/* yv_attention_long on an MXFP8 qkv operand (inference only: no lse), the blocking and the softmax unchanged.  The input is what
 * yv_linear_mxfp8_q writes for N = 3 * H * 64 output columns: qkv_q (R*N, 3*H*64) e4m3 bytes, row stride ld_in bytes; qkv_scales
 * K-step-major (3*H*64 / 128, in_rows_pad, 4) E8M0 - a head's 64 dimensions are two 32-blocks, bytes {0, 1} or {2, 3} of one dword.
 * QK^T is one block-scaled v_mfma_scale_f32_32x32x64_f8f6f4 per 32 x 32 score group (K rows and Q rows as stored, scales applied by
 * the instruction); V is dequantised exactly to bf16 on its way into LDS (e4m3 * 2^e) and PV runs as in yv_attention_long, P in
 * bf16.  On operands whose scores are exact in f32 the outputs are the bytes of yv_attention_long on the dequantised bf16 qkv.
 * Outputs out / out_q / out_scales / r_dev as yv_attention_long, with its rules.  YV_ERR_ARG, before any device call: a NULL
 * qkv_q / qkv_scales, neither output or out_q without out_scales, R < 0, N <= 0, H <= 0, H odd ((64 H) % 128 != 0),
 * ld_in < 3 * 64 * H or ld_in % 16 != 0, in_rows_pad < R*N or in_rows_pad % 128 != 0, qkv_q / out / out_q not 16-byte or
 * qkv_scales not 4-byte aligned.  A grid past 2^31 - 1 workgroups is YV_ERR_LIMIT; R = 0 is YV_OK without a launch.  No read
 * leaves rows [0, R*N) of either input array. */
int yv_attention_fp8(const void* qkv_q, long long ld_in, const void* qkv_scales, long long in_rows_pad, int R, int N, int H,
                     float scale, void* out, const int32_t* r_dev, void* out_q, long long ldq, void* out_scales,
                     long long rows_pad, void* stream);
/* Diagnostic: the V dequantisation of yv_attention_fp8 on its own: q (n e4m3 bytes, n % 4 == 0, 4-byte aligned) at the block scale
 * byte `scale_byte` (E8M0, 0 .. 254) -> out (n bf16). */
int yv_attention_fp8_dequant(const void* q, long long n, int scale_byte, void* out, void* stream);

/* Diagnostic builds of the attention kernel (0 = normal; 1 no K/V loads, 2 no compute, 3 no V^T writes). */
int yv_attention_debug(int ablate);

/* cls rows of the token stream: x[r*(tok+1), :] = cls + pos[0]  (timm cls_token + pos_embed) */
int yv_cls_rows(const float* cls, const float* pos, int R, int tok, int D, float* x, void* stream);

/* Network_Wrapper.fc on backbone logits + argmax (utils/utils.py:64-72, utils/trainClass.py:112):
 * w1t = fc.1.weight TRANSPOSED, (1000,128) f32 (coalesced rows); w2 = fc.3.weight (nc,128).
 * feats (R, ldf) f32 (first 1000 used) -> logits (R,nc) f32 [accumulated when accumulate!=0,
 * scaled by `scale`: mean-of-logits ensemble over model_list], labels (R) i32 (argmax, first max). */
int yv_wrapper_head(const float* feats, int ldf, const float* w1t, const float* b1, const float* w2, const float* b2,
                    int R, int nc, float scale, int accumulate, float* logits, int32_t* labels,
                    const int32_t* r_dev, void* stream);

/* SPPF: three chained 5x5/s1/p2 max-pools (== windows 5/9/13) in one pass (model.9).
 * buf: (B,H,W,ld) bf16; reads channels [0,c), writes [c,2c), [2c,3c), [3c,4c). */
int yv_sppf_pool(void* buf, int B, int H, int W, int ld, int c, void* stream);

/* Stem: blob (u8 RGB /255, 解读.md:70-74) + Conv 3x3 s2 + bias + SiLU (model.0).
 * images (B,H,W,3) u8; weight (27,Cout) f32, row = (ky*3+kx)*3+c; Cout in {16,32,48};
 * out (B,H/2,W/2,Cout) bf16, ld = out_ld. */
int yv_stem_conv(const uint8_t* images, int B, int H, int W, const float* weight, const float* bias, int Cout,
                 void* out, int out_ld, void* stream);

/* ------------------------------------------------------------- training */

/* Forward attention that also returns the per-(crop, head, query) log2-sum-exp for the backward pass. */
int yv_attention_train(const void* qkv, int R, int N, int H, float scale, void* out, float* lse, void* stream);

/* Attention backward (timm Attention, README.md:21-23): qkv/out/dout as in the forward, lse from
 * yv_attention_train; writes dqkv (R*N, 3*H*64) bf16; delta_ws: R*H*N floats of scratch. */
int yv_attention_bwd(const void* qkv, const void* out, const void* dout, const float* lse, int R, int N, int H,
                     float scale, void* dqkv, float* delta_ws, void* stream);

/* Attention backward for sequences longer than one tile (785 / 577 tokens); the same two kernels and the same arithmetic as
 * yv_attention_bwd with the blocking and staging of yv_attention_long: 128-row owner blocks whose last one has only its live
 * 32-row waves, the other axis walked in 64-row tiles double-buffered in LDS with the next tile's fetch under the current tile's
 * work, groups wholly past N skipped, K^T / Q^T / dO^T read with transposing LDS reads from the row-major tile image.  Any
 * N >= 1 is accepted; VitTrainer(long_attn_bwd=True) uses it for N > 224.
 * Operands as yv_attention_bwd: qkv, dqkv (R*N, 3*H*64) bf16; out, dout (R*N, H*64) bf16; lse (R, H, N) f32, log2 domain, from
 * yv_attention_train or yv_attention_long; delta_ws: R*H*N floats of scratch.  dqkv and delta_ws are bit-identical to
 * yv_attention_bwd on finite inputs, for every N; rows of dqkv past R*N and floats of delta_ws past R*H*N are never written.
 * qkv, out, dout, dqkv 16-byte aligned; a NULL pointer (but stream), R < 0, N <= 0, H <= 0 or a misaligned pointer is
 * YV_ERR_ARG, a grid past 2^31 - 1 workgroups YV_ERR_LIMIT; R = 0 is YV_OK without a launch.  Addresses are 64-bit: no 2 GB
 * limit.  A crop's gradients depend on that crop's inputs only: bit-identical whatever R, the crop's index and the grid. */
int yv_attention_bwd_long(const void* qkv, const void* out, const void* dout, const float* lse, int R, int N, int H,
                          float scale, void* dqkv, float* delta_ws, void* stream);

/* Attention backward for sequences of up to 224 tokens (197) in ONE launch; the same arithmetic as yv_attention_bwd with its two
 * kernels as two phases of one workgroup per (crop, head): Q, K, V and dO are fetched once into LDS images of ceil(N / 32) * 32
 * rows (the swizzled row-major layout of yv_attention_bwd_long, read row-wise and with transposing LDS reads), phase 1 owns the
 * queries (dQ, delta), phase 2 the keys (dK, dV) and takes lse / delta from LDS; the fetch of Q and dO lands under phase 1.
 * VitTrainer(short_attn_bwd=True) uses it for N <= 224.
 * Operands as yv_attention_bwd: qkv, dqkv (R*N, 3*H*64) bf16; out, dout (R*N, H*64) bf16; lse (R, H, N) f32, log2 domain, from
 * yv_attention_train or yv_attention_long; delta_ws: R*H*N floats, written as yv_attention_bwd writes them.  dqkv and delta_ws
 * are bit-identical to yv_attention_bwd on finite inputs, for every 1 <= N <= 224; rows of dqkv past R*N and floats of delta_ws
 * past R*H*N are never written.
 * qkv, out, dout, dqkv 16-byte aligned; a NULL pointer (but stream), R < 0, N <= 0, H <= 0 or a misaligned pointer is
 * YV_ERR_ARG, N > 224 or a grid past 2^31 - 1 workgroups YV_ERR_LIMIT; R = 0 is YV_OK without a launch.  Addresses are 64-bit:
 * no 2 GB limit.  A crop's gradients depend on that crop's inputs only: bit-identical whatever R, the crop's index and the grid. */
int yv_attention_bwd_short(const void* qkv, const void* out, const void* dout, const float* lse, int R, int N, int H,
                           float scale, void* dqkv, float* delta_ws, void* stream);

/* yv_attention_cls for the trainer (VitTrainer(cls_tail=True)): attention of the cls query of each crop, with the log2-sum-exp
 * its backward needs.  One workgroup per (crop, head), a streaming pass over K and V, every reduction in a fixed order.
 * q: bf16, row r at q + r*ldq elements, H*64 wide (ldq = N*3*H*64 reads the cls rows of the qkv buffer itself, ldq = H*64 a
 * compact copy); K and V from qkv (R*N, 3*H*64) bf16; out (R, H*64) bf16 compact, bit-identical to yv_attention_cls on the same
 * operands; lse[r*H + h] = max + log2(sum) f32 in the scaled log2 domain of yv_attention_train, so that
 * p_n = exp2(q.k_n * scale * log2 e - lse).  There is no device-side row count.
 * q, qkv, out 16-byte aligned, ldq a multiple of 8 and >= H*64; a NULL pointer (but stream), R < 0, N <= 0, H <= 0 or a broken
 * alignment rule is YV_ERR_ARG; N > 8192 or a grid past 2^31 - 1 workgroups YV_ERR_LIMIT; R = 0 is YV_OK without a launch.
 * Addresses are 64-bit. */
int yv_attention_cls_train(const void* q, long long ldq, const void* qkv, int R, int N, int H, float scale, void* out, float* lse,
                           void* stream);

/* Backward of yv_attention_cls_train.  q, ldq, qkv as there; dout (R, H*64) bf16 compact; lse from the forward.  In f32, per
 * (crop r, head h): s_n = q.k_n * scale * log2 e, p_n = exp2(s_n - lse), dp_n = dO.v_n, delta = sum_n p_n dp_n,
 * ds_n = p_n (dp_n - delta) * scale; dq = sum_n ds_n k_n, dk_n = ds_n q, dv_n = p_n dO.
 * Writes EVERY element of rows [0, R*N) of dqkv (R*N, 3*H*64) bf16, each rounded once: dk_n and dv_n in the K and V thirds of
 * row r*N + n, dq in the Q third of row r*N and zeros in the Q third of rows r*N + 1 .. r*N + N - 1.  Nothing past row R*N is
 * written.  K is read twice and V once (delta is summed from p and dp, not taken from the forward's output).
 * One workgroup per (crop, head), no atomics, every reduction in a fixed order: a crop's gradients are bit-identical whatever R
 * and the crop's index.  Argument rules, limits and return codes as yv_attention_cls_train (dout and dqkv 16-byte aligned). */
int yv_attention_cls_bwd(const void* q, long long ldq, const void* qkv, const void* dout, const float* lse, int R, int N, int H,
                         float scale, void* dqkv, void* stream);

/* out[M,N] (bf16) = A[M,K] . Wkn[K,N] with the weight in reduction-major layout (row stride ldw): the data
 * gradient dX = dY . W reads the (N_w, K_w) weight as it is stored, through transposing LDS reads (no W^T copy).
 * flags: YV_EPI_BIAS, YV_EPI_GELU_BWD (aux = saved pre-activation). */
int yv_linear_nn(const void* A, int lda, const void* Wkn, int ldw, const float* bias, int M, int N, int K, void* out,
                 int ldo, int flags, void* aux, int ldaux, void* stream);

/* Weight gradient dW (N,K) f32 = dY^T . X with dY (T,N) and X (T,K) bf16 token-major (T = tokens, a multiple of 64
 * whose tail rows are ZERO): the fragments are columns of the LDS tiles, read with ds_read_b64_tr_b16; no transposed
 * copies.  Split over T when a workspace is registered for the stream (deterministic). */
int yv_wgrad(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, float* dW, int ldw, void* stream);
/* yv_wgrad with the output tile chosen by the caller: tile_n = 128 is yv_wgrad (gemm_tn_kernel, 128 (n) x 128 (k) tiles);
 * 64 / 32 run gemm_tn_narrow_kernel, 64 / 32 (n) x 256 (k) tiles that issue no load, LDS read or MFMA for 16-column fragments
 * past N or K (few output channels: the detector's early layers); 0 lets yv_wgrad_route choose.  Any other value:
 * YV_ERR_ARG.  For an equal number of token slices every tile gives the same bits. */
int yv_wgrad_tiled(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, float* dW, int ldw, int tile_n,
                   void* stream);
/* The route of a weight gradient (yv_wgrad, yv_wgrad_tiled, and yv_wgrad_conv3* with K = 9 * Cin), decided by the function the
 * launch path itself calls.  Host only: nothing is dereferenced, launched or queried.  tile_n as yv_wgrad_tiled takes it.
 * tile_n = 0 chooses: the tile from {32, 64, 128} with the fewest padded columns ceil(N / tile) * tile, ties to the wider one;
 * then a 64-wide tile goes back to 128 when it would launch fewer workgroups than the 128 x 128 tiles and those fit one round of
 * the 2 * n_cu workgroup slots (measured slower there).  ws_bytes: the workspace registered for the stream (0: none, no token
 * split); n_cu: CUs of the device, 0 = 256 (what the launch path passes: the slice rule's slot constants are that part's).
 * Returns YV_OK and fills *out, or YV_ERR_ARG where the launch would reject T, N, K or tile_n. */
typedef struct {
    int tile_n, tile_k; /* output tile of a workgroup: 128 x 128, 64 x 256 or 32 x 256 (yv_wgrad_wide_route: or 256 x 128) */
    int tiles;          /* ceil(N / tile_n) * ceil(K / tile_k) */
    int slices;         /* token slices S (1: no split, no reduce pass) */
    int workgroups;     /* tiles * slices */
} yv_wgrad_route_t;
int yv_wgrad_route(int T, int N, int K, int tile_n, size_t ws_bytes, int n_cu, yv_wgrad_route_t* out);

/* yv_wgrad on 256 (n) x 128 (k) output tiles (gemm_tn_wide_kernel: three quarters of the LDS-DMA traffic of the 128 x 128 tiles
 * per MFMA; matrix-shaped dW, e.g. the classifier's linears).  Operands and preconditions are yv_wgrad's.  mode 1: always the wide
 * tile; mode 0: routed - the wide tile where yv_wgrad_wide_route picks it, otherwise exactly the launch of yv_wgrad; any other
 * mode: YV_ERR_ARG.  For an equal number of token slices the wide tile gives the bits of yv_wgrad. */
int yv_wgrad_wide(const void* dY, int ldy, const void* X, int ldx, int T, int N, int K, float* dW, int ldw, int mode,
                  void* stream);
/* The route of yv_wgrad_wide, decided by the function its launch calls; host only, as yv_wgrad_route.  Wide (tile_n = 256,
 * tile_k = 128) under mode 1, and under mode 0 where N >= 256, K >= 128, the 128 x 128 launch has more than 16 tiles and those
 * tiles times T / 64 are at least 25,000 (below that the wide tile measured slower); else the result of
 * yv_wgrad_route(T, N, K, 128, ...).  Slices of the wide tile: one round of the 2 * n_cu workgroup slots, at least 128 token
 * rows per slice, at most 16, even when more than two; option "wgrad_split" > 0 forces the count; never more than ws_bytes holds. */
int yv_wgrad_wide_route(int T, int N, int K, int mode, size_t ws_bytes, int n_cu, yv_wgrad_route_t* out);

/* Weight gradient of a 3x3 / stride 1 / pad 1 convolution with no im2col buffer: dW (N, 9*Cin) f32, column
 * ((dy+1)*3 + dx+1)*Cin + ci.  Operands over the zero-padded pixel grid (B, H+2, W+2), T = that pixel count rounded up to
 * a multiple of 64: dYp (T, N) bf16, ZERO on the ring and the tail rows; Xp (T, Cin) bf16 DENSE (row stride Cin), zero on
 * the ring, with pitch + 1 = W + 3 readable rows of finite values before its first and after its last row (tap offsets
 * reach there, always multiplied by a zero row of dYp).  yv_view_op mode 6 writes both layouts. */
int yv_wgrad_conv3(const void* dYp, int ldy, const void* Xp, int Cin, int pitch, int T, int N, float* dW, int ldw,
                   void* stream);
/* yv_wgrad_conv3 with the output tile of yv_wgrad_tiled (tile_n = 128: yv_wgrad_conv3). */
int yv_wgrad_conv3_tiled(const void* dYp, int ldy, const void* Xp, int Cin, int pitch, int T, int N, float* dW, int ldw,
                         int tile_n, void* stream);

/* Weight gradient of a 3x3 / pad 1 convolution of stride 1 or 2 with no operand copy: dW (N, 9*Cin) f32, column
 * (ky*3 + kx)*Cin + ci, equal bit for bit to yv_im2col3 + yv_wgrad_tiled on the same operands (the same route, hence the same
 * token slices).  X is the convolution's input (B, Hin, Win, Cin) bf16 as any view with row stride ldx >= Cin (a multiple of 8),
 * read in place: the kernel computes each tap's source pixel itself, and a tap in the padding reads a zero chunk the library
 * owns.  The output grid is Hout = (Hin - 1) / stride + 1, Wout likewise (odd grids allowed), as in yv_im2col3.  dY (r64(T), N)
 * bf16, T = B * Hout * Wout, r64 = rounded up to a multiple of 64, its tail rows ZERO, row stride ldy >= N (a multiple of 8).
 * Cin and N multiples of 8, ldw >= 9*Cin a multiple of 4, bases 16-byte aligned, T <= 2^31 - 64, tile_n as yv_wgrad_tiled takes
 * it; anything else: YV_ERR_ARG, nothing launched. */
int yv_wgrad_conv3_gather(const void* dY, int ldy, const void* X, long long ldx, int B, int Hin, int Win, int stride, int Cin, int N,
                          float* dW, int ldw, int tile_n, void* stream);
/* The route of yv_wgrad_conv3_gather; host only, as yv_wgrad_route.  *gemm is yv_wgrad_route(r64(T), N, 9*Cin, tile_n, ws_bytes,
 * n_cu).  *use: 0 where the per-layer measurement had the gather form slower than yv_im2col3 + yv_wgrad_tiled (a trainer then
 * keeps that layer on im2col); no measured layer was slower, so 1 everywhere today. */
int yv_wgrad_conv3_gather_route(int B, int Hin, int Win, int stride, int Cin, int N, int tile_n, size_t ws_bytes, int n_cu,
                                yv_wgrad_route_t* gemm, int* use);
/* The index function of yv_wgrad_conv3_gather's kernels, run on the host with the multiply-shift constants the launch computes:
 * *pixel = (b*Hin + iy)*Win + ix, the input pixel that tap (0..8, ky*3 + kx) of output pixel m reads, or -1 where it reads
 * zero (padding, or m >= B*Hout*Wout).  Host only. */
int yv_wgrad_conv3_gather_src(int B, int Hin, int Win, int stride, int m, int tap, long long* pixel);

/* out_t[c][r] = in[r][c] (bf16), rows of out_t zero padded up to the next multiple of 64 (ld_out >= that). */
int yv_transpose_bf16(const void* in, int rows, int cols, long long ld_in, void* out_t, long long ld_out, void* stream);

/* f32 master weight (N,K) -> bf16 (N,K) working copy and bf16 transposed (K, ld_t >= round64(N)) copy. */
int yv_cast_weights(const float* w, int N, int K, void* w_bf16, void* wt_bf16, long long ld_t, void* stream);

/* x f32 (rows, cols) -> optional bf16 copy y and optional column sums (bias gradients; deterministic two-stage).
 * ws: yv_colsum_ws_floats(rows, cols) floats. */
size_t yv_colsum_ws_floats(int rows, int cols);
int yv_cast_colsum(const float* x, int rows, int cols, void* y_bf16, float* colsum, int accumulate, float* ws,
                   void* stream);
int yv_colsum_bf16(const void* x, int rows, int cols, long long ld, float* colsum, int accumulate, float* ws,
                   void* stream);

/* LayerNorm backward: dx += dLN(dy) (f32 stream), dgamma / dbeta (D) f32; statistics recomputed from x.
 * D, ldx, lddy, lddx multiples of 4; x, gamma, dx 16-byte aligned and dy 8-byte aligned (YV_ERR_ARG, checked on the host before
 * any HIP call: the kernel reads float4 / uint2); D <= 1024 (YV_ERR_LIMIT).  ws: yv_layernorm_bwd_ws_floats(rows, D) floats, any
 * 4-byte alignment (a workspace that is not 16-byte aligned takes the scalar second stage: the same sums in another order). */
size_t yv_layernorm_bwd_ws_floats(int rows, int D);
int yv_layernorm_bwd(const float* x, long long ldx, const float* gamma, const void* dy, long long lddy, int rows, int D,
                     float eps, float* dx, long long lddx, float* dgamma, float* dbeta, float* ws, void* stream);

/* out (N,D) = sum over the R crops of dx (R,N,D): d pos_embed (row 0 is also d cls_token). */
int yv_token_reduce(const float* dx, int R, int N, int D, float* out, void* stream);

/* Network_Wrapper.fc backward (utils/utils.py:64-72): feats (R,ldf) f32 backbone logits, dlogits (R,nc) ->
 * dW1 (128,1000), db1, dW2 (nc,128), db2 (f32) and d feats (R,ldd) bf16 (columns >= 1000 zero).
 * ws: 2*R*128 floats. */
int yv_head_bwd(const float* feats, int ldf, const float* w1t, const float* b1, const float* w2, const float* dlogits,
                int R, int nc, float* dw1, float* db1, float* dw2, float* db2, void* dfeats_bf16, int ldd, float* ws,
                void* stream);

/* build_loss = LSCE(0.1)/6 + Focal(1,2,'mean')*5/6 (utils/trainClass.py:46-66,162-185,362-370)
 * loss = w_lsce*LSCE + w_focal*Focal (build_loss: 1/6, 5/6; each term alone: (1,0) / (0,1)).
 * logits (B,nc) f32, labels (B) i32 -> loss (1) f32, grad (B,nc) f32 (d loss / d logits). */
int yv_loss_fwd_bwd(const float* logits, const int32_t* labels, int B, int nc, float w_lsce, float w_focal,
                    float* loss, float* grad, void* stream);

/* torch.optim.SGD(momentum, weight_decay) step (utils/trainClass.py:442-443), fp32, in place:
 * g = g*grad_scale + wd*p; m = first ? g : mu*m + g; p -= lr*m.  (grad_scale: 1/world_size after a SUM all-reduce) */
int yv_sgd_step(float* p, const float* g, float* m, size_t n, float lr, float momentum, float weight_decay,
                float grad_scale, int first, void* bf16_mirror /* optional: bf16 copy of the updated p */, void* stream);

/* Batched bf16 transpose dst[b] (cols, rows) = src[b] (rows, cols)^T; matrix b starts `*_stride` elements after matrix b-1.
 * rows, cols multiples of 8, 16-byte aligned.  The trainer (autograd of every nn.Linear of timm's Block, reference loop
 * utils/trainClass.py:403-407 `loss.backward()`) keeps a transposed bf16 mirror of the block weights so that the data
 * gradient dX = dY . W runs as an ordinary yv_linear on W^T. */
int yv_transpose_bf16_batched(const void* src, void* dst, int rows, int cols, int batch, long long src_stride,
                              long long dst_stride, void* stream);

/* Optimisers ultralytics builds for `optimizer='auto'` (the reference calls `.train(..., lr0=1e-4, lrf=1e-4)` with that
 * default, utils/trainYolo.py:33), element-wise in the operation order of torch's single-tensor implementations:
 * kind 1 = torch.optim.SGD(momentum=beta1, nesterov=True, weight_decay) (v unused), kind 2 = torch.optim.AdamW(betas,
 * eps, weight_decay).  step counts from 1 (bias corrections; step 1 initialises the state).  g is scaled by grad_scale. */
int yv_optim_step(int kind, float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                  float eps, float weight_decay, float grad_scale, int step, void* bf16_mirror, void* stream);

/* Global-norm gradient clipping: torch.nn.utils.clip_grad_norm_(parameters, max_norm) ahead of the optimiser step (the
 * published YOLOv8 trainer: max_norm 10), as a four-float record in device memory that the *_rec steps below read, so that no
 * step waits on the host.  rec, each line one correctly rounded f32 operation:
 *   rec[0] = S = f32(sum_i (double)g[i]^2)   accumulated in f64 (squares are exact there) in an order n alone decides, without
 *                                            atomics: the same bits on every run and every device
 *   rec[1] = N = sqrt(S) * |grad_scale|      the norm of the gradient as the optimiser sees it
 *   rec[2] = c = min(1, max_norm / (N + 1e-6))
 *   rec[3] = s = grad_scale * c              what the step multiplies g by
 * N not finite (a NaN or Inf element, or S past f32): rec[2] = rec[3] = 0 and *skipped (optional) is incremented by one.
 * Two launches: one f64 partial per workgroup into ws, then one workgroup for the record.
 * ws: yv_grad_clip_ws_bytes(n) bytes (0 for n = 0; non-decreasing in n, constant once the grid is at its cap); less is
 * YV_ERR_LIMIT.  g and ws 16-byte aligned, max_norm > 0 (+inf: measure, never clip), grad_scale finite, n > 0, no null g / ws /
 * rec: otherwise YV_ERR_ARG.  All of these are decided on the host before any HIP call. */
size_t yv_grad_clip_ws_bytes(size_t n);
int yv_grad_clip_record(const float* g, size_t n, float grad_scale, float max_norm, void* ws, size_t ws_bytes, float* rec,
                        int32_t* skipped, void* stream);

/* yv_sgd_step / yv_optim_step with the record of yv_grad_clip_record in place of grad_scale: g is scaled by rec[3]; where
 * rec[1] is not finite the launch stores nothing (p, m, v and the mirror keep their bits; a first step's m / v stay unread).
 * Otherwise the bits of yv_sgd_step / yv_optim_step called with grad_scale = rec[3]: one device text serves both forms. */
int yv_sgd_step_rec(float* p, const float* g, float* m, size_t n, float lr, float momentum, float weight_decay,
                    const float* rec, int first, void* bf16_mirror, void* stream);
int yv_optim_step_rec(int kind, float* p, const float* g, float* m, float* v, size_t n, float lr, float beta1, float beta2,
                      float eps, float weight_decay, const float* rec, int step, void* bf16_mirror, void* stream);

/* dst = a*dst + b*src (gradient accumulation over `accumulate` batches: a = b = 1). */
int yv_axpby(float* dst, const float* src, size_t n, float a, float b, void* stream);

/* ultralytics ModelEMA: ema = decay*ema + (1-decay)*src. */
int yv_ema_update(float* ema, const float* src, size_t n, float decay, void* stream);

/* ---- detector training (the ultralytics trainer behind utils/trainYolo.py:13-35) --------
 * Conv = conv(no bias) -> BatchNorm2d(eps 1e-3, momentum 0.03) -> SiLU, un-folded; activations are NHWC bf16 views:
 * (rows = B*H*W, C) with a row stride `ld` (elements, a multiple of 8, at least C), C a multiple of 8, pointers 16-byte
 * aligned; anything else is YV_ERR_ARG. */

/* u8 RGB pixels -> bf16 value/255, channels padded 3 -> 8 with zeros (`blob`, YOLOTensorRT_yolodet_py_解读.md:70-74). */
int yv_blob_nhwc8(const void* images_u8, long long pixels, void* out_bf16, void* stream);

/* Per-channel batch statistics of z (T,C): mean, rstd = 1/sqrt(biased var + eps); optional running estimates
 * (run = (1-momentum)*run + momentum*{mean, unbiased var}, both or neither).  ws: yv_bn_ws_floats(T,C) floats. */
size_t yv_bn_ws_floats(long long T, int C);
int yv_bn_stats(const void* z, long long ldz, long long T, int C, float eps, float momentum, float* mean, float* rstd,
                float* run_mean, float* run_var, float* ws, size_t ws_floats, void* stream);

/* Second half of yv_bn_stats for tile partials written by yv_conv2d_stats (stats_ws as that call left it, T = B*Hout*Wout rows,
 * C = Cout): more than 2048 tiles are first folded, groups of ceil(tiles / 2048) consecutive tiles in ascending order in
 * double, into chunk partials behind the tile partials; then yv_bn_stats' finaliser (same double-precision formulas, same
 * running-estimate rule: both of run_mean / run_var or neither). */
int yv_bn_stats_finish(float* stats_ws, long long T, int C, float eps, float momentum, float* mean, float* rstd,
                       float* run_mean, float* run_var, void* stream);

/* a = act(gamma*(z-mean)*rstd + beta) [+ res]   (act 1 = SiLU, 0 = identity); a, res bf16 views. */
int yv_bn_act_fwd(const void* z, long long ldz, long long T, int C, const float* mean, const float* rstd,
                  const float* gamma, const float* beta, const void* res, long long ldres, void* out, long long ldo,
                  int act, void* stream);

/* Backward of the above: g = da*act'(u); dbeta = sum g; dgamma = sum g*xhat;
 * dz = gamma*rstd*(g - mean(g) - xhat*mean(g*xhat)) with batch statistics, gamma*rstd*g with frozen ones. */
int yv_bn_act_bwd(const void* da, long long ldda, const void* z, long long ldz, long long T, int C, const float* mean,
                  const float* rstd, const float* gamma, const float* beta, int act, int batch_stats, float* dgamma,
                  float* dbeta, void* dz, long long lddz, float* ws, size_t ws_floats, void* stream);

/* yv_bn_act_bwd behind yv_conv2d_bnbwd: stats_ws holds that call's tile partials of (sum g, sum g * xhat) over T = B*Hout*Wout
 * rows of C = Cout channels (yv_conv_bnbwd_ws_floats(T, C) floats).  More than 2048 tiles are first folded as yv_bn_stats_finish
 * folds them; then yv_bn_act_bwd's finaliser and apply pass run unchanged (dgamma, dbeta, dz as there; da is the gradient the
 * convolution stored).  No pass over da and z for the sums. */
int yv_bn_act_bwd_finish(const void* da, long long ldda, const void* z, long long ldz, long long T, int C, const float* mean,
                         const float* rstd, const float* gamma, const float* beta, int act, int batch_stats, float* dgamma,
                         float* dbeta, void* dz, long long lddz, float* stats_ws, void* stream);

/* Element-wise view operations on (B,H,W,C) bf16 views.  mode 0 copy, 1 dst += src, 2 nearest-2x upsample
 * (dst (B,2H,2W) <- src (B,H,W)), 3 its adjoint accumulated (dst (B,H,W) += 2x2 block sums of src (B,2H,2W)),
 * 4 zero insertion (dst (B,2H,2W): [2y][2x] = src[y][x], 0 elsewhere: stride-2 data gradient), 5 zero fill,
 * 6 zero-ring padding (dst (B,H+2,W+2): interior = src (B,H,W), ring = 0: the operand layout of yv_wgrad_conv3). */
int yv_view_op(int mode, const void* src, long long ld_src, void* dst, long long ld_dst, int B, int H, int W, int C,
               void* stream);

/* din += adjoint of max_pool2d(k 5, s 1, p 2) at dout, the maximum of a window being its first one in scan order.
 * ws: B*H*W*C bytes (per-window argmax offsets). */
int yv_maxpool5_bwd(const void* x, long long ldx, const void* dout, long long lddo, void* din, long long lddi, int B, int H,
                    int W, int C, void* ws, size_t ws_bytes, void* stream);

/* col (B*Hout*Wout, 9*C) = 3x3 / pad 1 patches of x (B,Hin,Win,C), K order (ky,kx,c): the X operand of yv_wgrad. */
int yv_im2col3(const void* x, long long ldx, int B, int Hin, int Win, int C, int stride, void* col, void* stream);

/* wd (Cin, taps, Cout) = 180-degree tap flip + in/out transpose of w (Cout, taps, Cin) bf16: the data gradient of a
 * stride-1 conv is yv_conv2d(dz, wd); of a stride-2 conv the same over the zero-inserted dz (yv_view_op mode 4), or - 3 x 3,
 * without the zero-inserted copy and its products with zeros - yv_conv2d_dgrad_s2(dz, wd), which reads the same wd. */
int yv_conv_weight_dgrad(const void* w, int Cout, int taps, int Cin, void* wd, void* stream);

/* Data gradient of a 3 x 3 / stride 2 / pad 1 convolution without zero insertion: dx (B, 2*Hout, 2*Wout, Cin) = [res +] the
 * gradient of z = conv(x, w) at dz (B, Hout, Wout, Cout), wd = yv_conv_weight_dgrad(w) (Cin, 9, Cout).  The output pixel
 * (2i + py, 2j + px) belongs to parity phase (py, px); per axis parity 0 takes wd slot row 1 at dz row i, parity 1 takes slot
 * row 0 at dz row i and slot row 2 at dz row i + 1 (zero past the last row); the 2-D slot is 3 * row + col.  The phases have
 * 1 / 2 / 2 / 4 taps - 9 tap products per 2 x 2 output block where the zero-inserted convolution spends 36 - and each is an
 * implicit GEMM (B*Hout*Wout rows, Cin columns, K = taps * Cout, taps in ascending slot order) on the phase form of the
 * convolution kernels; the four run in ONE launch, heaviest first.  bf16 in and out, f32 accumulation, no bias, no activation.
 * Eligibility (else YV_ERR_ARG, nothing is written): Cout a multiple of 64, Cin a multiple of 8, dz->c == Cout, no upsample,
 * strides that are multiples of 8 and cover the channels, every base 16-byte aligned.  res (same grid and type as dx, may be dx
 * itself) is optional.  32-bit byte offsets address dz: a batch whose dz passes 2 GB is taken in sub-batches, one image and wd
 * must stay below 2 GB (YV_ERR_LIMIT).  ws / ws_bytes: reserved, no route splits K.
 * With res the number of roundings depends on the route (yv_conv2d_dgrad_s2_route reports it):
 *   direct epilogue (staged 0: 16- / 32-wide tiles, "staged_epilogue" = 0):  dx = bf16(y + r), ONE rounding;
 *   staged epilogue (staged 1: every LDS-DMA route, the 64- / 128-wide tiles otherwise):  dx = bf16(bf16(y) + r), the
 *   gradient is rounded to bf16 BEFORE the residual is added, TWO roundings.
 * Without a residual both forms give the same bits.  Where yv_conv2d over the zero-inserted dz takes the same epilogue form and
 * does not split K, its result has the same bits: its other K steps add products with zeros. */
int yv_conv2d_dgrad_s2(const yv_view* dz, int B, int Hout, int Wout, const void* wd, int Cin, int Cout, void* dx, int dx_ld,
                       const void* res, int res_ld, void* ws, size_t ws_bytes, void* stream);

/* The route of yv_conv2d_dgrad_s2 for the data gradient of a ksize x ksize / stride 2 layer with input (B, Hin, Win, Cin) and
 * Cout output channels, decided by the function the launch path itself calls.  Host only: nothing is dereferenced, launched or
 * queried; dense 16-byte aligned bases are assumed, dz_ld / dx_ld / res_ld are the pixel strides (res_ld = 0: no residual).
 * Returns a negative YV_ERR_* code where yv_conv2d_dgrad_s2 rejects the arguments or cannot express the layer (ksize != 3, odd
 * Hin or Win), else YV_OK and *out; for a batch taken in sub-batches, the route of the first one. */
typedef struct {
    int kernel;     /* instance, numbered as yv_conv2d_instance bits 0-3: 0 .. 3 igemm_kernel 128 x 16 / 32 / 64 / 128 tiles,
                       5 cgemm_dma_kernel<64,4,1,3>, 7 <128,2,2,2>; each in its phase form */
    int ksteps[4];  /* 64-deep K steps per tile of the phases in launch order (1,1), (1,0), (0,1), (0,0): 4, 2, 2, 1 x Cout / 64 */
    int staged;     /* 1: the staged epilogue runs (two roundings with a residual, see yv_conv2d_dgrad_s2) */
    int tiles;      /* tiles of ONE phase */
    int workgroups; /* 4 * tiles: the launch */
    int use;        /* 1: measured no slower than zero insertion + yv_conv2d for this shape; 0: keep that path */
} yv_dgrad_s2_route_t;
int yv_conv2d_dgrad_s2_route(int B, int Hin, int Win, int ksize, int Cin, int Cout, int dz_ld, int dx_ld, int res_ld,
                             yv_dgrad_s2_route_t* out);

/* v8 detection loss and its gradient (the objective of `YOLO(pt).train(...)`, utils/trainYolo.py:33; published
 * ultralytics v8DetectionLoss restated in oracle/yolo_train.py - parity unpinned): DFL decode, TaskAlignedAssigner
 * (topk 10, alpha 0.5, beta 6; top-k ties by ascending anchor index among the anchors inside the box), CIoU + DFL + BCE,
 * normalised by the batch sum of target scores, times B.
 * box[s] (B*h_s*h_s, 64) / cls[s] (B*h_s*h_s, ncp) f32 logits of the three scales (h_s = size / {8,16,32}) and the
 * matching gradient buffers; gt_boxes (B,G,4) xyxy input pixels, gt_labels (B,G), gt_counts (B) valid boxes per image;
 * loss (4) = {total*B, box, cls, dfl}.  ws: yv_detect_loss_ws_bytes(B, A, G), A = sum h_s^2. */
size_t yv_detect_loss_ws_bytes(int B, int A, int G);
int yv_detect_loss(const float* const* box, const float* const* cls, float* const* dbox, float* const* dcls, int B, int size,
                   int nc, int ncp, const float* gt_boxes, const int32_t* gt_labels, const int32_t* gt_counts, int G,
                   float gain_box, float gain_cls, float gain_dfl, float* loss, void* ws, size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* YV_HIP_H */
