// Fused non-causal attention forward for ViT token counts (197 single-tile, 785 tiled), head dim 64:
//   O = softmax(Q K^T * scale) V              timm Attention (README.md:21-23), SURVEY.md row B3 / K10.
//
// One workgroup per (crop, head, query block); wave w owns 32 query rows.  K (row major) and V^T tiles
// live in LDS; at N = 197 the whole sequence is ONE tile (28 KB + 29 KB) so there is no online-softmax
// rescale and each wave computes its full 32 x N score block in registers; longer sequences (ViT-B/8:
// 785 tokens) walk 256-row K/V tiles with running max / sum.
//
// The MFMA plan, the LDS images (swizzled K rows, padded V^T rows, row-major swizzled V for the transposing read), the softmax
// group step and the output formats are csrc/attention_fwd_core.h, shared with attention_long.hip.
#include "attention_fwd_core.h"
#include <type_traits>

namespace {

int g_attn_abl = 0;               // diagnostic builds (yv_attention_debug)

// SINGLE (N <= NP, the ViT-x/16 case: 197 tokens in one 224-row tile): the 32-key score groups are consumed one at a time with
// an online softmax (running max / sum per query, O rescaled only when some row's maximum really grew - typically 2-3 of the
// 7 groups) instead of holding all NT groups (16 f32 registers each) across the softmax: ~100 VGPRs instead of 194, i.e. TWO
// workgroups per CU, so that one workgroup's global -> LDS staging (HBM-bound: 155 MB per launch at 128 crops) runs under the
// other's MFMA / exp work.  Round-1 form: one 7-wave workgroup per CU, staging (29 us) and compute (40 us) back to back.
template <int NT, int ABL = 0, bool SINGLE = false>
__global__ __launch_bounds__(NT * 64, SINGLE ? 4 : 1) void attention_kernel(const uint16_t* __restrict__ qkv, int N, int H, int QB,
                                                            float scale_log2e, uint16_t* __restrict__ out,
                                                            const int32_t* __restrict__ r_dev, float* __restrict__ lse, AttnMx mx) {
    // blockIdx.x = ((crop * H + head) * QB + query block); a query block = NT waves x 32 queries = NP rows.
    // Keys/values are consumed in tiles of NP rows with an online softmax (running max m, sum l, rescaled
    // O); N <= NP (ViT-x/16: 197 <= 224) is the single-tile case and pays no rescale.
    constexpr int NP = NT * 32;
    constexpr int VT_STRIDE = NP * 2 + 8;               // bytes per V^T row
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    unsigned char* Ks = smem;                            // NP x 128 B
    unsigned char* Vt = smem + NP * 128;                 // 64 x VT_STRIDE
    const int qb = blockIdx.x % QB;
    const int rh = blockIdx.x / QB;
    const int r = rh / H, hd = rh - r * H;
    if (r_dev && r >= r_dev[0]) return;
    const int D = H * HD, ld = 3 * D;
    const uint16_t* base = qkv + (size_t)r * N * ld + hd * HD;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    constexpr int T = NT * 64;

    // ---- Q fragments (B operand), straight from global --------------------------------------
    const int rl = lane & 31, hh = lane >> 5;
    const int q = qb * NP + wave * 32 + rl;
    bf16x8 fq[4];
    q_frags(base, q, N, ld, hh, fq);

    f32x16 o[2];
#pragma unroll
    for (int mt = 0; mt < 2; ++mt)
#pragma unroll
        for (int e = 0; e < 16; ++e) o[mt][e] = 0.f;
    float m_run = -INFINITY, l_run = 0.f;

    for (int kv0 = 0; kv0 < N; kv0 += NP) {
        if (kv0 > 0) __syncthreads();                    // every wave is done reading the previous tile
        // ---- stage K (swizzled rows) and V^T (explicit transpose) -------------------------
        // All of a thread's K / V chunks are fetched before the first one is stored (NP * 8 / T = 4 trips, 8 loads in flight), from
        // a CLAMPED row instead of behind `if (key < N)`: rows past N only have to be finite (their scores are masked to -inf,
        // their probabilities are exactly 0), and a conditional load is a branch + vmcnt(0) per trip - the staging phase of the
        // first version was 4 dependent HBM round trips per workgroup.
        constexpr int TRIPS = (NP * 8 + T - 1) / T;
        uint4 kvr[TRIPS], vvr[TRIPS];
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            const int kl = row_chunk(it < NP * 8 ? it : NP * 8 - 1).row, c = row_chunk(it).c;
            int key = kv0 + kl;
            key = key < N ? key : N - 1;
            kvr[i] = vvr[i] = make_uint4(0, 0, 0, 0);
            if (ABL != 1) {
                kvr[i] = *(const uint4*)(base + (size_t)key * ld + D + c * 8);
                vvr[i] = *(const uint4*)(base + (size_t)key * ld + 2 * D + c * 8);
            }
        }
#pragma unroll
        for (int i = 0; i < TRIPS; ++i) {
            const int it = tid + i * T;
            if (it >= NP * 8) break;
            const auto [kl, c] = row_chunk(it);
            *(uint4*)(Ks + k_off(kl, c)) = kvr[i];
            const uint32_t w[4] = {vvr[i].x, vvr[i].y, vvr[i].z, vvr[i].w};
            if (ABL != 3) {
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    const uint16_t val = (uint16_t)(w[e >> 1] >> ((e & 1) * 16));
                    *(uint16_t*)(Vt + (c * 8 + e) * VT_STRIDE + kl * 2) = val;
                }
            }
        }
        __syncthreads();
        if (ABL == 2) continue;

        if constexpr (SINGLE) {
            float l_lane = 0.f;                               // this lane's share of the row sum (lane ^ 32 holds the rest)
#pragma unroll 1
            for (int kt = 0; kt < NT; ++kt) {                // rolled: unrolled, the scheduler hoists every group's MFMAs again
                f32x16 sv = score_group(Ks, kt * 32, fq, rl, hh);
                if (kt * 32 + 32 > N) mask_group(sv, kt * 32, N, hh);
                online_step(sv, m_run, l_lane, o, scale_log2e);
                pv_product(sv, o, [&](int mt, int st) __attribute__((always_inline)) { return vt_frag_padded(Vt, VT_STRIDE, mt, kt * 32 + 16 * st, rl, hh); });
            }
            l_run = l_lane + __shfl_xor(l_lane, 32, 64);
            continue;
        }

        // ---- S^T = K . Q^T ------------------------------------------------------------------
        f32x16 s[NT];
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kt][e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(k_frag(Ks, kt * 32 + rl, ks, hh), fq[ks], s[kt], 0, 0, 0);
        }

        // ---- online softmax over this tile's keys (register axis + lane^32) -----------------
        // only a 32-key group that straddles N needs masking (197 tokens: the last of 7 groups)
        float mx = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            if (kv0 + kt * 32 + 32 > N) mask_group(s[kt], kv0 + kt * 32, N, hh);
#pragma unroll
            for (int e = 0; e < 16; ++e) mx = fmaxf(mx, s[kt][e]);
        }
        mx = fmaxf(mx, __shfl_xor(mx, 32, 64));
        const float m_new = fmaxf(m_run, mx);            // every tile holds >= 1 valid key -> finite
        const float alpha = __builtin_amdgcn_exp2f((m_run - m_new) * scale_log2e);   // first tile: exp2(-inf) = 0
        const float mb = m_new * scale_log2e;
        float l = 0.f;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt)
#pragma unroll
            for (int e = 0; e < 16; ++e) {
                const float p = __builtin_amdgcn_exp2f(fmaf(s[kt][e], scale_log2e, -mb));    // one v_fma + one v_exp
                s[kt][e] = p;
                l += p;
            }
        l += __shfl_xor(l, 32, 64);
        l_run = l_run * alpha + l;
        m_run = m_new;
        if (kv0 > 0) {
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int e = 0; e < 16; ++e) o[mt][e] *= alpha;
        }

        // ---- O^T += V^T . P^T ---------------------------------------------------------------
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
#pragma unroll
            for (int st = 0; st < 2; ++st) {
                const bf16x8 fp = p_frag(s[kt], st);
#pragma unroll
                for (int mt = 0; mt < 2; ++mt)
                    o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(vt_frag_padded(Vt, VT_STRIDE, mt, kt * 32 + 16 * st, rl, hh), fp, o[mt], 0, 0, 0);
            }
        }
    }

    // ---- normalise and store -----------------------------------------------------------------
    if (q < N) {
        store_lse(lse, r, H, hd, N, q, hh, m_run * scale_log2e, l_run);
        const float inv = 1.0f / l_run;
        if (mx.q) store_mx(o, inv, mx, r, N, hd, q, hh);
        else store_direct(out + ((size_t)r * N + q) * D + hd * HD, o, inv, hh);
    }
}

// ---------------------------------------------------------------------------------------------
// Single-tile case, round 3 (N <= 32 NT <= 224: every ViT-x/16): a workgroup walks `per` consecutive (crop, head) items with K and V
// DOUBLE-BUFFERED in LDS, so that item i+1's 2 x NP x 128 bytes are in flight while item i is computed (the one-item kernel was a
// staging phase and a compute phase back to back, overlapped only by chance between the two workgroups of a CU):
//   * K and V rows (128-byte strips of the 3 D-wide token rows = one cache line each) go global -> LDS by LDS-DMA, 8 pieces of
//     8 rows per wave and tensor pair; no staging registers, no LDS stores, V is NOT transposed: the PV product's A operand
//     (V^T: 32 d x 16 keys) is read from the row-major image with the transposing LDS read ds_read_b64_tr_b16 (two per fragment:
//     keys kb + 4h + 0..3 and kb + 8 + 4h + 0..3 - the k order the exponentiated accumulator registers have);
//   * images: k_chunk / v_chunk of attention_fwd_core.h; the swizzles act on the DMA's SOURCE chunk;
//   * one workgroup per CU (140 KB of LDS at NT = 7), so a wave may hold all NT score groups (16 NT registers): one softmax pass,
//     no running maximum, no rescale;
//   * one barrier per item: behind it item i has landed for every wave AND every wave is done with item i-1, whose buffer the
//     DMA of item i+1 then refills; the output stores of item i-1 stay in flight across it (counted vmcnt);
//   * output rows leave as 16-byte stores (v_permlane32_swap pairs the two half-waves' 8-byte pieces of a query row).
// Rows past N are fetched from row N-1 (finite; their scores are masked to -inf, their probabilities are exactly 0).
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* at_lptr_t;
typedef float at_f32x2 __attribute__((ext_vector_type(2)));

// transposing reads of PV step n (inline asm: see the kernel) and the counted wait for them
template <int N_>
__device__ __forceinline__ void at_vread(u32x2 (&vr)[2][4], uint32_t va0, uint32_t va1) {
    constexpr int off = (N_ >> 1) * 32 * 128 + (N_ & 1) * 16 * 128;
    asm volatile("ds_read_b64_tr_b16 %0, %4 offset:%6\n\tds_read_b64_tr_b16 %1, %4 offset:%7\n\t"
                 "ds_read_b64_tr_b16 %2, %5 offset:%6\n\tds_read_b64_tr_b16 %3, %5 offset:%7"
                 : "=&v"(vr[N_ & 1][0]), "=&v"(vr[N_ & 1][1]), "=&v"(vr[N_ & 1][2]), "=&v"(vr[N_ & 1][3])
                 : "v"(va0), "v"(va1), "i"(off), "i"(off + 8 * 128) : "memory");
}
template <int N_, bool LAST>
__device__ __forceinline__ void at_vwait(u32x2 (&vr)[2][4]) {
    if constexpr (LAST) asm volatile("s_waitcnt lgkmcnt(0)" : "+v"(vr[N_ & 1][0]), "+v"(vr[N_ & 1][1]), "+v"(vr[N_ & 1][2]), "+v"(vr[N_ & 1][3]) :: "memory");
    else asm volatile("s_waitcnt lgkmcnt(4)" : "+v"(vr[N_ & 1][0]), "+v"(vr[N_ & 1][1]), "+v"(vr[N_ & 1][2]), "+v"(vr[N_ & 1][3]) :: "memory");
}

template <int NT, int ABL = 0 /* timing only: 1 no K / V / Q fetch, 2 no compute, 3 no output stores */>
__global__ __launch_bounds__(NT * 64) void attention_pipe_kernel(const uint16_t* __restrict__ qkv, int N, int H, int R, int per,
                                                                  float scale_log2e, uint16_t* __restrict__ out,
                                                                  const int32_t* __restrict__ r_dev, float* __restrict__ lse, AttnMx mx) {
    constexpr int NP = NT * 32, TILE = NP * 128, BUF = 2 * TILE;
    constexpr int PIECES = 2 * NT * 4;                          // 8-row pieces of K and V together; PIECES / NT = 8 per wave
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int Re = r_dev ? (r_dev[0] < R ? r_dev[0] : R) : R;
    const int n_items = Re * H;
    const int it0 = blockIdx.x * per;
    const int it1 = it0 + per < n_items ? it0 + per : n_items;
    if (it0 >= it1) return;
    const int D = H * HD, ld = 3 * D;
    const int rl = lane & 31, hh = lane >> 5;

    // DMA source: lane (row = lane >> 3 of the piece, LDS chunk = lane & 7) fetches the chunk its LDS position holds.  Buffer form
    // (32-bit offsets; the host checks the tensor is below 2 GB): behind the global_load_lds form hipcc waited vmcnt(0) in front of
    // the first transposing LDS read of every item (it takes the DMA for a possible writer of the bytes read)
    const auto rsQ = __builtin_amdgcn_make_buffer_rsrc((void*)qkv, 0, 0x7fffffff, 0x00020000);
    auto issue = [&](int item, int buf) __attribute__((always_inline)) {
        const int r = item / H, hd = item - r * H;
        const uint32_t base = (uint32_t)(((size_t)r * N * ld + hd * HD) * 2);      // wave-uniform: the instruction's scalar offset
        unsigned char* B = smem + buf * BUF;
#pragma unroll
        for (int j = 0; j < 8; ++j) {
            const int pid = wave * 8 + j;                       // wave-uniform
            const int tensor = pid >= NT * 4 ? 1 : 0;
            const int prow = (pid - tensor * NT * 4) * 8;
            const int row = prow + row_chunk(lane).row, c = row_chunk(lane).c;
            const int key = row < N ? row : N - 1;
            const int cs = tensor ? v_chunk(row, c) : k_chunk(row, c);
            const uint32_t voff = (uint32_t)((key * ld + (tensor + 1) * D + cs * 8) * 2);
            if (ABL != 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (at_lptr_t)(B + tensor * TILE + prow * 128), 16, (int)voff, (int)base, 0, 0);
        }
    };
    // Query rows: by LDS-DMA as well, into ONE buffer: a wave reads only its own 32 rows, so it refills them (item i+1) right after
    // its own S MFMAs of item i, no barrier involved.  (Ordinary loads to registers made hipcc wait vmcnt(0) - drain the DMA of item
    // i+1 - before their first use: staging and compute ran back to back, 13 + 30 us; hidden in inline asm, the loop-carried
    // registers were copied by compiler-placed moves before the data had landed.)
    auto issue_q = [&](int item) __attribute__((always_inline)) {
        const int r = item / H, hd = item - r * H;
        const uint32_t base = (uint32_t)(((size_t)r * N * ld + hd * HD) * 2);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int prow = wave * 32 + j * 8;
            const int row = prow + row_chunk(lane).row, c = row_chunk(lane).c;
            const int qr = row < N ? row : N - 1;
            const uint32_t voff = (uint32_t)((qr * ld + k_chunk(row, c) * 8) * 2);
            if (ABL != 1) __builtin_amdgcn_raw_ptr_buffer_load_lds(rsQ, (at_lptr_t)(smem + 2 * BUF + prow * 128), 16, (int)voff, (int)base, 0, 0);
        }
    };
    const VtOff vto = vt_offsets(lane);                                    // V^T fragment addressing of the transposing read

    const bool plain = !lse && !mx.q && ABL == 0;                          // exactly 4 output stores per wave and item (the counted wait below)
    issue(it0, 0);
    issue_q(it0);
    for (int item = it0; item < it1; ++item) {
        const int buf = (item - it0) & 1;
        const bool more = item + 1 < it1;
        // item's K / V have landed (this wave's pieces; the barrier covers the others'); the previous item's output stores - the
        // youngest memory operations - stay in flight
        if (item > it0 && plain) asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        asm volatile("s_barrier" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        if (more) issue(item + 1, buf ^ 1);
        const unsigned char* Ks = smem + buf * BUF;
        const unsigned char* Vs = Ks + TILE;
        if (ABL == 2) { if (more) issue_q(item + 1); continue; }
        bf16x8 fq[4];
#pragma unroll
        for (int ks = 0; ks < 4; ++ks) fq[ks] = k_frag(smem + 2 * BUF, wave * 32 + rl, ks, hh);

        // ---- S^T = K . Q^T: all NT groups ----------------------------------------------------
        // (the four K fragments of group kt+1 are read before group kt's MFMAs: left to itself hipcc reads every fragment into the same
        // four registers right before its MFMA and waits lgkmcnt(0) for it - 28 exposed LDS round trips per item)
        f32x16 s[NT];
        bf16x8 kf[2][4];
        auto read_k = [&](int kt, bf16x8 (&f)[4]) __attribute__((always_inline)) {
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) f[ks] = k_frag(Ks, kt * 32 + rl, ks, hh);
        };
        read_k(0, kf[0]);
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            if (kt + 1 < NT) read_k(kt + 1, kf[(kt + 1) & 1]);
#pragma unroll
            for (int e = 0; e < 16; ++e) s[kt][e] = 0.f;
#pragma unroll
            for (int ks = 0; ks < 4; ++ks) s[kt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(kf[kt & 1][ks], fq[ks], s[kt], 0, 0, 0);
            __builtin_amdgcn_sched_barrier(0);
        }
        if (more) issue_q(item + 1);                          // this wave's query rows had their last use (the fragments are in registers)
        // ---- softmax over the register axis + lane ^ 32, in two passes: the maximum first (it follows the S MFMAs group by group),
        // then exp / sum / pack of group kt+1 INTERLEAVED with the four PV MFMAs of group kt: left alone hipcc emits 28 S MFMAs, one
        // block of ~450 vector instructions, 28 PV MFMAs - neither pipe ever works beside the other (measured: 32 us of compute per
        // 128 crops for 7 us of MFMA time) ---------------------------------------------------------
        float mxv = -INFINITY;
#pragma unroll
        for (int kt = 0; kt < NT; ++kt) {
            if (kt == NT - 1) mask_group(s[kt], kt * 32, N, hh);  // only the last group can straddle N (N > 32 (NT - 1)); branch-free
#pragma unroll
            for (int e = 0; e < 16; ++e) mxv = fmaxf(mxv, s[kt][e]);
        }
        mxv = fmaxf(mxv, __shfl_xor(mxv, 32, 64));
        const float mb = mxv * scale_log2e;
        // packed fp32 for the scale and the row sums (v_pk_fma_f32 / v_pk_add_f32: half the vector instructions; two waves share a
        // SIMD's vector pipe here and it is the pipe this kernel is bound by - tools/valu_rate.hip)
        at_f32x2 l2 = {0.f, 0.f};
        const at_f32x2 sc2 = {scale_log2e, scale_log2e}, nmb2 = {-mb, -mb};
        bf16x8 fp[NT][2];
        auto expg = [&](int kt) __attribute__((always_inline)) {
#pragma unroll
            for (int e = 0; e < 16; e += 2) {
                // elements e .. e + 3 of every lane are keys >= 32 kt + 8 (e >> 2): past N (last group only) they are exactly 0
                if (kt == NT - 1 && kt * 32 + key_of(e & ~3, 0) >= N) {
                    fp[kt][e >> 3][e & 7] = (__bf16)0.f; fp[kt][e >> 3][(e & 7) + 1] = (__bf16)0.f;
                    continue;
                }
                const at_f32x2 x = __builtin_elementwise_fma(at_f32x2{s[kt][e], s[kt][e + 1]}, sc2, nmb2);
                const at_f32x2 pp = {__builtin_amdgcn_exp2f(x[0]), __builtin_amdgcn_exp2f(x[1])};
                l2 += pp;
                fp[kt][e >> 3][e & 7] = (__bf16)pp[0]; fp[kt][e >> 3][(e & 7) + 1] = (__bf16)pp[1];
            }
        };
        f32x16 o[2];
#pragma unroll
        for (int mt = 0; mt < 2; ++mt)
#pragma unroll
            for (int e = 0; e < 16; ++e) o[mt][e] = 0.f;
        // The transposing reads are inline asm (their builtin makes hipcc wait vmcnt(0) - drain item i+1's DMA - before the first
        // one: it cannot see that they read the OTHER buffer), so their completion is counted by hand: the four reads of step n+1
        // are issued before the wait for step n's (lgkmcnt(4): LDS results return in order; LDS operations hipcc issues in between
        // only make the wait stricter).  Step n = (key group kt, 16-key half st); a step's reads: (mt 0, mt 1) x (keys +0..3, +8..11).
        u32x2 vr[2][4];
        const uint32_t vbase = (uint32_t)(uintptr_t)(at_lptr_t)(const_cast<unsigned char*>(Vs));
        const uint32_t va0 = vbase + vto.o[0], va1 = vbase + vto.o[1];
        auto pv_step = [&](auto n_c) __attribute__((always_inline)) {
            constexpr int n = decltype(n_c)::value, kt = n >> 1, st = n & 1;
            if constexpr (n + 1 < 2 * NT) at_vread<n + 1>(vr, va0, va1);
            at_vwait<n, !(n + 1 < 2 * NT)>(vr);
#pragma unroll
            for (int mt = 0; mt < 2; ++mt) {
                const u32x4 pkv = {vr[n & 1][2 * mt][0], vr[n & 1][2 * mt][1], vr[n & 1][2 * mt + 1][0], vr[n & 1][2 * mt + 1][1]};
                o[mt] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8, pkv), fp[kt][st], o[mt], 0, 0, 0);
            }
        };
        expg(0);
        at_vread<0>(vr, va0, va1);
        auto pv_group = [&](auto kt_c) __attribute__((always_inline)) {
            constexpr int kt = decltype(kt_c)::value;
            if constexpr (kt < NT) {
                pv_step(std::integral_constant<int, 2 * kt>{});
                pv_step(std::integral_constant<int, 2 * kt + 1>{});
                if constexpr (kt + 1 < NT) expg(kt + 1);
            }
        };
        pv_group(std::integral_constant<int, 0>{}); pv_group(std::integral_constant<int, 1>{}); pv_group(std::integral_constant<int, 2>{});
        pv_group(std::integral_constant<int, 3>{}); pv_group(std::integral_constant<int, 4>{}); pv_group(std::integral_constant<int, 5>{});
        pv_group(std::integral_constant<int, 6>{});
        const float l = (l2[0] + l2[1]) + __shfl_xor(l2[0] + l2[1], 32, 64);
        // ---- normalise and store -------------------------------------------------------------------
        const int r = item / H, hd = item - r * H;
        const int q = wave * 32 + rl;
        const float inv = 1.0f / l;
        store_lse(lse, r, H, hd, N, q, hh, mb, l);
        if (mx.q) {
            if (q < N) store_mx(o, inv, mx, r, N, hd, q, hh);
        } else {
            const auto rsO = __builtin_amdgcn_make_buffer_rsrc((void*)out, 0, 0x7fffffff, 0x00020000);   // (offsets checked by the host: < 2 GB)
            const uint32_t ob = q < N ? (uint32_t)((((size_t)r * N + q) * D + hd * HD) * 2) : 0x80000000u;
#pragma unroll
            for (int mt = 0; mt < 2; ++mt)
#pragma unroll
                for (int g4 = 0; g4 < 4; g4 += 2) {
                    const u32x4 pkv = swapped_rows(o, inv, mt, g4);
                    if (ABL != 3) __builtin_amdgcn_raw_buffer_store_b128(pkv, rsO, ob + (uint32_t)(swapped_col(mt, g4, hh) * 2), 0, 0);
                    else asm volatile("" :: "v"(pkv));
                }
        }
    }
}

template <int NT>
int launch_attn_pipe(const uint16_t* qkv, int R, int N, int H, float scale, uint16_t* out, const int32_t* r_dev, float* lse,
                     hipStream_t st, AttnMx mx) {
    constexpr int NP = NT * 32;
    const size_t lds = (size_t)5 * NP * 128;                   // K, V double-buffered + this item's query rows
    auto kern = g_attn_abl == 11 ? attention_pipe_kernel<NT, 1> : g_attn_abl == 12 ? attention_pipe_kernel<NT, 2> :
                g_attn_abl == 13 ? attention_pipe_kernel<NT, 3> : attention_pipe_kernel<NT, 0>;
    if (!yv_grant_lds((const void*)kern, lds)) return YV_ERR_LAUNCH;
    // items per workgroup: enough to amortise the pipeline fill, few enough that the grid still fills and balances the chip
    const int items = R * H;
    int per = items / 256;
    per = per < 1 ? 1 : (per > 6 ? 6 : per);
    const int grid = (items + per - 1) / per;
    hipLaunchKernelGGL(kern, dim3(grid), dim3(NT * 64), lds, st, qkv, N, H, R, per, scale * LOG2E, out, r_dev, lse, mx);
    return yv_launch_status();
}

template <int NT>
int launch_attn(const uint16_t* qkv, int R, int N, int H, float scale, uint16_t* out, const int32_t* r_dev, float* lse,
                hipStream_t st, AttnMx mx) {
    constexpr int NP = NT * 32;
    const size_t lds = (size_t)NP * 128 + 64 * (size_t)(NP * 2 + 8);
    const bool single = N <= NP && g_attn_abl != 4;           // ablation 4: the round-1 form of the single-tile case (all groups held)
    auto kern = g_attn_abl == 1 ? attention_kernel<NT, 1> : g_attn_abl == 2 ? attention_kernel<NT, 2> : g_attn_abl == 3 ? attention_kernel<NT, 3> :
                single ? attention_kernel<NT, 0, true> : attention_kernel<NT, 0, false>;
    if (!yv_grant_lds((const void*)kern, lds)) return YV_ERR_LAUNCH;
    const int QB = (N + NP - 1) / NP;
    hipLaunchKernelGGL(kern, dim3(R * H * QB), dim3(NT * 64), lds, st, qkv, N, H, QB, scale * LOG2E, out,
                       r_dev, lse, mx);
    return yv_launch_status();
}

// ---------------------------------------------------------------------------------------------
// cls-query attention (last block of the classifier: only the cls row of each crop is read after it).  One query against N keys
// is a streaming pass over K and V (2 * N * 128 B per crop and head) with two dot products per byte pair: no MFMA, no tiling.
// One workgroup of 256 threads per (crop, head); 8 lanes share a 128-byte K / V row (16 B each), 32 rows per trip.
//   1. s[n] = q . K[n] * scale (log2 domain) into LDS, 2. block max / exp2 / sum, 3. o = sum_n p[n] V[n] / sum.
// Every reduction has a fixed order: the result does not depend on the launch.
// ---------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void attention_cls_kernel(const uint16_t* __restrict__ q, const uint16_t* __restrict__ qkv, int R,
                                                            int N, int H, float scale_log2, uint16_t* __restrict__ out,
                                                            const int32_t* __restrict__ r_dev) {
    extern __shared__ __attribute__((aligned(16))) float cls_sm[];       // N scores (padded to 4) | 4 x 64 partial outputs | 8 scalars
    const int r = blockIdx.x / H, hd = blockIdx.x - r * H;
    int Rr = R;
    if (r_dev) { const int c = r_dev[0]; Rr = c < Rr ? c : Rr; }
    if (r >= Rr) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, c = tid & 7, grp = tid >> 3;
    float* sc = cls_sm;
    float* part = cls_sm + ((N + 3) & ~3);
    float* red = part + 256;
    const long long ld = 3LL * H * 64;
    const uint16_t* kb = qkv + (long long)r * N * ld + (long long)(H + hd) * 64 + c * 8;
    const uint16_t* vb = kb + (long long)H * 64;
    float qf[8];
    unpack_bf16x8(*(const u32x4*)(q + ((long long)r * H + hd) * 64 + c * 8), qf);

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

}  // namespace

static int attention_impl(const void* qkv, int R, int N, int H, float scale, void* out, const int32_t* r_dev, float* lse,
                          void* stream, AttnMx mx = AttnMx{nullptr, 0, nullptr, 0}) {
    if (!qkv || (!out && !mx.q) || R < 0 || N <= 0 || H <= 0) return YV_ERR_ARG;
    if ((long long)R * H * ((N + 255) / 256) > 0x7fffffffLL) return YV_ERR_LIMIT;
    if (R == 0) return YV_OK;
    const uint16_t* q = (const uint16_t*)qkv;
    uint16_t* o = (uint16_t*)out;
    hipStream_t st = (hipStream_t)stream;
    const int nt = N > 256 ? 8 : (N + 31) / 32;        // > 256 tokens: 256-row tiles, online softmax
    if (nt <= 7 && (g_attn_abl == 0 || g_attn_abl > 10) && (long long)R * N * H * HD * 6 < 0x7fffffffLL) {      // single tile: the pipelined kernel
        switch (nt) {
            case 1: return launch_attn_pipe<1>(q, R, N, H, scale, o, r_dev, lse, st, mx);
            case 2: return launch_attn_pipe<2>(q, R, N, H, scale, o, r_dev, lse, st, mx);
            case 3: return launch_attn_pipe<3>(q, R, N, H, scale, o, r_dev, lse, st, mx);
            case 4: return launch_attn_pipe<4>(q, R, N, H, scale, o, r_dev, lse, st, mx);
            case 5: return launch_attn_pipe<5>(q, R, N, H, scale, o, r_dev, lse, st, mx);
            case 6: return launch_attn_pipe<6>(q, R, N, H, scale, o, r_dev, lse, st, mx);
            default: return launch_attn_pipe<7>(q, R, N, H, scale, o, r_dev, lse, st, mx);
        }
    }
    switch (nt) {
        case 1: return launch_attn<1>(q, R, N, H, scale, o, r_dev, lse, st, mx);
        case 2: return launch_attn<2>(q, R, N, H, scale, o, r_dev, lse, st, mx);
        case 3: return launch_attn<3>(q, R, N, H, scale, o, r_dev, lse, st, mx);
        case 4: return launch_attn<4>(q, R, N, H, scale, o, r_dev, lse, st, mx);
        case 5: return launch_attn<5>(q, R, N, H, scale, o, r_dev, lse, st, mx);
        case 6: return launch_attn<6>(q, R, N, H, scale, o, r_dev, lse, st, mx);
        case 7: return launch_attn<7>(q, R, N, H, scale, o, r_dev, lse, st, mx);
        default: return launch_attn<8>(q, R, N, H, scale, o, r_dev, lse, st, mx);
    }
}

extern "C" int yv_attention_debug(int ablate) { g_attn_abl = ablate; return YV_OK; }

extern "C" int yv_attention(const void* qkv, int R, int N, int H, float scale, void* out, const int32_t* r_dev,
                            void* stream) {
    return attention_impl(qkv, R, N, H, scale, out, r_dev, nullptr, stream);
}

extern "C" int yv_attention_cls(const void* q, const void* qkv, int R, int N, int H, float scale, void* out, const int32_t* r_dev,
                                void* stream) {
    if (!q || !qkv || !out || R < 0 || N <= 0 || H <= 0) return YV_ERR_ARG;
    if (((uintptr_t)q | (uintptr_t)qkv | (uintptr_t)out) & 15) return YV_ERR_ARG;          // 16-byte row chunks
    if (N > 8192 || (long long)R * H > 0x7fffffffLL) return YV_ERR_LIMIT;                  // the scores of one query live in LDS
    if (R == 0) return YV_OK;
    const size_t lds = ((size_t)((N + 3) & ~3) + 256 + 8) * sizeof(float);
    hipLaunchKernelGGL(attention_cls_kernel, dim3(R * H), dim3(256), lds, (hipStream_t)stream, (const uint16_t*)q,
                       (const uint16_t*)qkv, R, N, H, scale * 1.4426950408889634f, (uint16_t*)out, r_dev);
    return yv_launch_status();
}

extern "C" int yv_attention_mxfp8(const void* qkv, int R, int N, int H, float scale, void* out_q, long long ldq,
                                  void* out_scales, long long rows_pad, const int32_t* r_dev, void* stream) {
    if (!out_q || !out_scales || (ldq & 15) || ldq < (long long)H * 64 || rows_pad < (long long)R * N || (rows_pad & 127))
        return YV_ERR_ARG;
    if ((H & 1)) return YV_ERR_ARG;                         // whole 128-column K steps of the consumer: H*64 % 128 == 0
    return attention_impl(qkv, R, N, H, scale, nullptr, r_dev, nullptr, stream,
                          AttnMx{(uint8_t*)out_q, ldq, (uint8_t*)out_scales, rows_pad});
}

extern "C" int yv_attention_train(const void* qkv, int R, int N, int H, float scale, void* out, float* lse, void* stream) {
    if (!lse) return YV_ERR_ARG;
    return attention_impl(qkv, R, N, H, scale, out, nullptr, lse, stream);
}
