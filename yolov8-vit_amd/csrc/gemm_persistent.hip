// Persistent classifier GEMMs: gemm_p8_kernel (8-phase schedule) and gemm_p9_kernel (free-running; bf16 and MXFP8 operands), their
// launchers and tuning options.  GemmArgs and the conventions of the family: gemm_common.h, gemm.hip.
#include <type_traits>
#include "gemm_common.h"
#include "mx_quant.h"

using namespace yvgemm;

int yvgemm::g_opt_p9_small = 1;              // gemm_p9_kernel: 128 / 96-row tiles allowed ("linear_p9_small")
int yvgemm::g_opt_p9_small_fixed = 48;       // ... and the fixed part of their cost per K tile, in rows ("linear_p9_small_fixed")
int yvgemm::g_opt_p8_sched = 1;            // tile schedule of the persistent kernel (GemmArgs::sched): "linear_p8_sched"
thread_local int yvgemm::g_opt_p8_cus = 0; // persistent grid size OF LAUNCHES MADE BY THIS THREAD; 0 = every CU ("linear_p8_cus": leave CUs to concurrent streams)
int yvgemm::g_opt_p8_rows = 0;             // 0 = pick the tile height per launch; 128 / 160 / 192 / 224 / 256 force it ("linear_p8_rows")

namespace {

// ---------------------------------------------------------------------------------------------
// 256 x 256 x 64 "8-phase" schedule (cdna_hip_programming.md section 5 template, re-derived for this operand
// convention; the non-persistent round-1 kernel of this shape was removed in round 3, gemm_p8_kernel below is its
// persistent form).  8 waves = 2 groups (wm = 0/1, 128 activation rows each) x 4 (64 weight rows each); one
// workgroup per CU, 128 KB of LDS = 2 stages x {A tile, W tile}.  A K tile is consumed in 4 phases, one
// 64 x 32 quadrant of the wave tile each (16 MFMAs): (m0,n0) (m0,n1) (m1,n1) (m1,n0); every phase is
//     [ds_read this phase's operand half | issue ONE half-tile of LDS-DMA] barrier [16 MFMA] barrier
// and the two wave groups run ONE BARRIER APART, so that on every SIMD one wave is in its MFMA segment while
// its partner reads LDS / issues DMA.  The DMA stream runs 3 half-tiles ahead and is retired once per K
// tile by a COUNTED s_waitcnt vmcnt(6) (never 0 in the loop), raw s_barrier (a __syncthreads would drain).
//
// Half-tiles: A-half h = rows {wm*128 + h*64 + [0,64)} (both groups), W-half h = rows {wn*64 + h*32 + [0,32)}:
// each half holds what every wave reads in ONE phase, so it dies as a unit:
//     phase 1 reads A0,W0   phase 2 reads W1   phase 3 reads A1   phase 4 reads nothing  (W0,W1 stay in VGPRs)
//     restage (one phase after the last read; reads are retired by lgkmcnt(0) BEFORE the phase's first barrier):
//     phase 1: A1(t+1)   phase 2: A0(t+2)   phase 3: W0(t+2)   phase 4: W1(t+2), then vmcnt(6) = tile t+1 landed
// RAW: a half-tile is read at the earliest one phase after the wait that retires it (two barriers later, which
// covers the one-barrier stagger between the groups).
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void bar() { asm volatile("s_barrier" ::: "memory"); }

// ---------------------------------------------------------------------------------------------
// Persistent form of the 8-phase schedule (round 2).  One workgroup per CU walks its tiles; what changes against
// a one-tile-per-workgroup kernel:
//   * the LDS-DMA stream never drains between tiles: during the last two K tiles of a tile the restage slots load the FIRST two
//     K tiles of the workgroup's next tile, so the pipeline fill (one HBM/L2 round trip per tile) and the first waits are hidden
//     behind the epilogue, and the epilogue's stores drain in the shadow of the next main loop instead of in a burst;
//   * the epilogue does not alias the stage buffers (they are being refilled): every wave transposes 16 output rows at a time
//     through a private 2 KB slab; the bias vector sits in LDS for the whole launch (a global bias load inside the epilogue
//     would make hipcc drain the in-flight DMA with vmcnt(0));
//   * operands are addressed through buffer descriptors (32-bit offsets: half the address registers of flat pointers, which
//     pays for the second - next tile - offset set; rows past M read as zeros through the range check instead of a clamp);
//   * GELU by a 9-operation sigmoid form (see gelu_fast_f).
// LDS map: [stage 0 | stage 1] 2 x 64 KB, 8 slabs x 2 KB, bias 16 KB = 160 KB exactly.
// Restrictions (checked by the host, everything else takes the 128 x 128 kernel): N % 256 == 0, N <= 4096, K % 64 == 0,
// bf16 output, flags within {BIAS, GELU}, operand images below 2 GB.
// ---------------------------------------------------------------------------------------------
typedef __attribute__((address_space(3))) void* lds_void_t;

// MF0 / MF1: 16-row activation fragments per wave group in the first / second half of its rows; tile = 32 (MF0 + MF1) rows x
// 256 columns.  (4,4) = 256 rows is the template of the guide; the smaller instances exist for tile-count quantisation: a
// persistent grid of 256 workgroups runs ceil(tiles / 256) rounds, and e.g. the 297 tiles of a 25,216 x 768 output cost two
// rounds at 256 rows but 474 tiles = 1.85 rounds of 160-row tiles (-37 %).  The host picks the instance that minimises
// rounds x rows.  A-operand DMA slots that a smaller tile does not need are issued with an out-of-range offset (the buffer
// range check turns them into no-ops) so that every wave keeps issuing the same number of DMA instructions per phase, which
// is what the counted vmcnt relies on.
template <int MF0, int MF1, bool F32OUT, int DIAG = 0 /* tools/gemm_lab.hip only: per-segment cycle sums into g.partial */>
__global__ __launch_bounds__(512) void gemm_p8_kernel(GemmArgs g) {
    constexpr int MF = MF0 + MF1, NF = 4;
    constexpr int RG = MF * 16, BM = 2 * RG;                   // rows per wave group / per tile
    constexpr int A_BYTES = 256 * 128, W_BYTES = 256 * 128, STAGE = A_BYTES + W_BYTES;
    constexpr int SLAB0 = 2 * STAGE, SLAB = 2048, BIAS0 = SLAB0 + 8 * SLAB;
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    const int tiles_m = (M + BM - 1) / BM, tiles_n = g.N >> 8;
    const int ntiles = tiles_m * tiles_n;
    const int G = gridDim.x;
    // tile schedule (blockIdx & 7 = XCD under round-robin placement - speed only, never correctness): see GemmArgs::sched
    int Lx, seq0, seq1, lid;
    if (g.sched == 1) {
        const int nx = G < 8 ? G : 8;                           // (grids smaller than 8 blocks: one sequence share per block)
        const int xcd = (int)blockIdx.x % nx;
        lid = (int)blockIdx.x / nx;
        Lx = (G - xcd + nx - 1) / nx;                           // blocks that share this part of the sequence
        int cum = 0;                                            // blocks of the parts before this one
        for (int y = 0; y < xcd; ++y) cum += (G - y + nx - 1) / nx;
        // parts proportional to their block counts: with tiles == blocks every block gets exactly one tile (equal parts would
        // hand a 29-block XCD 30 tiles and double the launch time)
        seq0 = (int)((long long)ntiles * cum / G); seq1 = (int)((long long)ntiles * (cum + Lx) / G);
    } else {
        // round r covers sequence positions [r G, r G + G); inside a round XCD x walks a contiguous chunk of it
        const int q = G >> 3, r = G & 7, x = blockIdx.x & 7;
        lid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + ((int)blockIdx.x >> 3);
        Lx = G; seq0 = 0; seq1 = ntiles;
    }
    if (seq0 + lid >= seq1) return;
    {   // bias -> LDS once (plain loads, before any DMA is in flight)
        float* bl = (float*)(smem + BIAS0);
        for (int i = tid; i < g.N; i += 512) bl[i] = (g.flags & YV_EPI_BIAS) ? g.bias[i] : 0.0f;
    }
    const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)g.a0, 0, (int)(((long long)(g.M - 1) * g.lda0 + g.K) * 2), 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)g.w, 0, (int)((long long)g.N * g.K * 2), 0x00020000);

    const int wm = wave >> 2, wn = wave & 3;
    const int wrow_m = wm * RG, wrow_n = wn * 64;
    const int fr = lane & 15, fq = lane >> 4;
    const int lrow = lane >> 3, lch = lane & 7;
    auto coords = [&](int seq, int& m0, int& n0) __attribute__((always_inline)) {   // grouped order: GM consecutive M tiles share a W tile
        const int GM = g.group_m, per = GM * tiles_n;
        const int grp = seq / per, first = grp * GM;
        const int gsz = (tiles_m - first) < GM ? (tiles_m - first) : GM;
        const int in = seq - grp * per;
        m0 = (first + in % gsz) * BM;
        n0 = (in / gsz) << 8;
    };
    // A half h of a stage: rows {group * RG + off_h + [0, len_h)} of both groups = 2 * len_h / 8 pieces of 8 rows; piece slots
    // s = wave * 2 + j (16 per half); slots past the piece count are dummies
    auto a_piece_row = [&](int h, int s) __attribute__((always_inline)) -> int {      // first tile row of piece s, or -1
        const int len8 = (h == 0 ? MF0 : MF1) * 2;                                      // pieces per group
        if (s >= 2 * len8) return -1;
        const int grp = s / len8, r8 = s - grp * len8;
        return grp * RG + (h == 0 ? 0 : MF0 * 16) + r8 * 8;
    };
    auto set_offsets = [&](uint32_t (&o)[4][2], int m0, int n0) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int s_ = wave * 2 + j;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r0 = a_piece_row(h, s_);
                const int ra = r0 + lrow, m = m0 + ra;
                o[h][j] = (r0 >= 0 && m < g.M) ? (uint32_t)(((long long)m * g.lda0 + ((lch ^ (ra & 7)) << 3)) * 2) : 0x80000000u;
                const int rh = s_ * 8 + lrow;
                const int rw = (rh >> 5) * 64 + h * 32 + (rh & 31);
                o[2 + h][j] = (uint32_t)(((long long)(n0 + rw) * g.K + ((lch ^ (rw & 7)) << 3)) * 2);
            }
        }
    };
    auto lds_dst = [&](int kind, int j) __attribute__((always_inline)) -> int {   // wave-uniform destination of a piece inside a stage
        const int s_ = wave * 2 + j;
        if (kind < 2) {
            const int r0 = a_piece_row(kind, s_);
            return (r0 >= 0 ? r0 : BM) * 128;                   // dummy pieces land in the unused rows BM.. of the A region
        }
        const int rb = s_ * 8;
        return A_BYTES + ((rb >> 5) * 64 + (kind - 2) * 32 + (rb & 31)) * 128;
    };

    const int nk = g.K / BK;
    uint32_t ocur[4][2], onxt[4][2];
    int seq = seq0 + lid, m0, n0, m0n = 0, n0n = 0;
    coords(seq, m0, n0);
    set_offsets(ocur, m0, n0);
    bool has_next = seq + Lx < seq1;
    if (has_next) { coords(seq + Lx, m0n, n0n); set_offsets(onxt, m0n, n0n); }
    int gk = 0;                                                // K tiles consumed so far by this workgroup (stage = gk & 1)

    // half-tile `kind` of K tile t of the CURRENT tile into stage `st` / of K tile tt of the NEXT tile (separate functions:
    // a run-time choice between the two offset sets makes hipcc index them through scratch memory, and scratch loads count
    // in vmcnt like the DMA does)
    auto issue_cur = [&](int kind, int t, int st) __attribute__((always_inline)) {
        unsigned char* base = smem + (st & 1) * STAGE;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(kind < 2 ? rsA : rsW, (lds_void_t)(base + lds_dst(kind, j)), 16,
                                                     (int)ocur[kind][j], t * 128, 0, 0);
    };
    auto issue_nxt = [&](int kind, int tt, int st) __attribute__((always_inline)) {
        if (!has_next) return;
        unsigned char* base = smem + (st & 1) * STAGE;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(kind < 2 ? rsA : rsW, (lds_void_t)(base + lds_dst(kind, j)), 16,
                                                     (int)onxt[kind][j], tt * 128, 0, 0);
    };

    f32x4 acc[NF][MF];
    bf16x8 fa[4][2], fw[4][2];
    auto read_a = [&](const unsigned char* A, int h) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < (h == 0 ? MF0 : MF1); ++j) {
            const int rr = wrow_m + (h == 0 ? 0 : MF0 * 16) + j * 16 + fr;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) fa[j][ks] = *(const bf16x8*)(A + rr * 128 + (((ks * 4 + fq) ^ (rr & 7)) << 4));
        }
    };
    auto read_w = [&](const unsigned char* W, int h) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int rr = wrow_n + h * 32 + i * 16 + fr;
#pragma unroll
            for (int ks = 0; ks < 2; ++ks) fw[h * 2 + i][ks] = *(const bf16x8*)(W + rr * 128 + (((ks * 4 + fq) ^ (rr & 7)) << 4));
        }
    };
    auto mma = [&](int mh, int nh) __attribute__((always_inline)) {
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int ks = 0; ks < 2; ++ks)
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < (mh == 0 ? MF0 : MF1); ++j)
                    acc[nh * 2 + i][(mh == 0 ? 0 : MF0) + j] =
                        __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[nh * 2 + i][ks], fa[j][ks], acc[nh * 2 + i][(mh == 0 ? 0 : MF0) + j], 0, 0, 0);
        __builtin_amdgcn_s_setprio(0);
    };
    auto sync_reads = [&]() __attribute__((always_inline)) {
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        __builtin_amdgcn_sched_barrier(0);
        bar();
        __builtin_amdgcn_sched_barrier(0);
    };
    auto sync_mma = [&]() __attribute__((always_inline)) {
        __builtin_amdgcn_sched_barrier(0);
        bar();
        __builtin_amdgcn_sched_barrier(0);
    };

    // DIAG build: cycle sums per segment of a phase (s_memtime stamps; a stamp is consumed one natural lgkmcnt(0) later, so
    // that reading it never adds a wait).  [0] read + DMA issue, [1] lgkmcnt wait of phases 1-3, [2] lgkmcnt + vmcnt wait of
    // phase 4, [3] first barrier, [4] MFMA segment, [5] second barrier, [6] epilogue, [7] phases
    uint32_t dg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, ds0 = 0, ds1 = 0, dp1 = 0, dp2 = 0, dp3 = 0, dp4 = 0, dp_is4 = 0;
    auto stamp = [&]() __attribute__((always_inline)) -> uint32_t { return (uint32_t)__builtin_amdgcn_s_memtime(); };
    auto dg_flush = [&]() __attribute__((always_inline)) {      // right after a natural lgkmcnt(0): every older stamp has landed
        if constexpr (DIAG) {
            if (dg[7]) {
                if (dp_is4) dg[2] += dp2 - dp1; else dg[1] += dp2 - dp1;
                dg[3] += dp3 - dp2; dg[4] += dp4 - dp3; dg[5] += ds0 - dp4;
            }
            dg[0] += ds1 - ds0; dg[7] += 1; dp1 = ds1;
        }
    };
    __syncthreads();                                           // bias image complete (no DMA in flight yet: a plain barrier)
    // ---- prologue of the first tile: K tile 0 complete, first three half-tiles of K tile 1 in flight (nk >= 2) ----------
    issue_cur(0, 0, 0); issue_cur(2, 0, 0); issue_cur(3, 0, 0); issue_cur(1, 0, 0);
    issue_cur(0, 1, 1); issue_cur(2, 1, 1); issue_cur(3, 1, 1);
    asm volatile("s_waitcnt vmcnt(6)" ::: "memory");
    bar();
    if (wm == 1) bar();                                        // group 1 runs one barrier behind group 0

    // one K tile = 4 phases.  TAIL 0: K tiles t+1, t+2 belong to this tile; 1: t = nk-2 (t+2 is K tile 0 of the next tile);
    // 2: t = nk-1 (t+1, t+2 are K tiles 0, 1 of the next tile).  Stage of a K tile = parity of the running counter gk.
    auto ktile = [&](int t, auto tail_c) __attribute__((always_inline)) {
        constexpr int TAIL = decltype(tail_c)::value;
        const unsigned char* A = smem + (gk & 1) * STAGE;
        const unsigned char* W = A + A_BYTES;
        auto seg_reads = [&](int is4) __attribute__((always_inline)) {     // end of a read segment (DIAG: stamped)
            if constexpr (DIAG) {
                if (!is4) ds1 = stamp();                          // phase 4 stamps in front of its vmcnt wait
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                __builtin_amdgcn_sched_barrier(0);
                dg_flush(); dp_is4 = is4;
                dp2 = stamp();
                __builtin_amdgcn_sched_barrier(0);
                bar();
                __builtin_amdgcn_sched_barrier(0);
                dp3 = stamp();
            } else sync_reads();
        };
        auto seg_mma = [&]() __attribute__((always_inline)) {
            if constexpr (DIAG) {
                __builtin_amdgcn_sched_barrier(0);
                dp4 = stamp();
                bar();
                __builtin_amdgcn_sched_barrier(0);
                ds0 = stamp();
            } else sync_mma();
        };
        read_a(A, 0); read_w(W, 0);
        if constexpr (TAIL == 2) issue_nxt(1, 0, gk + 1); else issue_cur(1, t + 1, gk + 1);
        seg_reads(0);
        mma(0, 0);
        seg_mma();
        read_w(W, 1);
        if constexpr (TAIL == 0) issue_cur(0, t + 2, gk); else issue_nxt(0, TAIL - 1, gk);
        seg_reads(0);
        mma(0, 1);
        seg_mma();
        read_a(A, 1);
        if constexpr (TAIL == 0) issue_cur(2, t + 2, gk); else issue_nxt(2, TAIL - 1, gk);
        seg_reads(0);
        mma(1, 1);
        seg_mma();
        if constexpr (TAIL == 0) issue_cur(3, t + 2, gk); else issue_nxt(3, TAIL - 1, gk);
        if constexpr (DIAG) ds1 = stamp();
        if (TAIL == 0 || has_next) asm volatile("s_waitcnt vmcnt(6)" ::: "memory");     // three half-tiles stay in flight
        else asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        seg_reads(1);
        mma(1, 0);
        seg_mma();
        ++gk;
    };

    uint32_t de0_ = 0;
    const uint32_t dk0 = DIAG ? stamp() : 0;
    if constexpr (DIAG) ds0 = dk0;
    for (;;) {
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        for (int t = 0; t < nk - 2; ++t) ktile(t, std::integral_constant<int, 0>{});
        ktile(nk - 2, std::integral_constant<int, 1>{});
        ktile(nk - 1, std::integral_constant<int, 2>{});
        // ---- epilogue: 16 rows at a time through this wave's slab; no workgroup barrier (the groups stay one barrier apart) ----
        {
            if constexpr (DIAG) de0_ = stamp();
            unsigned char* slab = smem + SLAB0 + wave * SLAB;
            const float* bl = (const float*)(smem + BIAS0) + n0 + wrow_n + fq * 4;
            if constexpr (!F32OUT) {
                const bool gelu = g.flags & YV_EPI_GELU;
                uint16_t* outp = (uint16_t*)g.out;
#pragma unroll
                for (int j = 0; j < MF; ++j) {
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float4 bvi = *(const float4*)(bl + i * 16);
                        float v0 = acc[i][j][0] + bvi.x, v1 = acc[i][j][1] + bvi.y;
                        float v2 = acc[i][j][2] + bvi.z, v3 = acc[i][j][3] + bvi.w;
                        if (gelu) { v0 = gelu_f(v0); v1 = gelu_f(v1); v2 = gelu_f(v2); v3 = gelu_f(v3); }
                        const int c16 = i * 2 + (fq >> 1);
                        *(uint2*)(slab + fr * 128 + ((c16 ^ (fr & 7)) << 4) + (fq & 1) * 8) =
                            make_uint2(pack_bf16x2(v0, v1), pack_bf16x2(v2, v3));
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // the slab is wave-private: LDS executes a wave's ops in order
#pragma unroll
                    for (int it = 0; it < 2; ++it) {
                        const int row = it * 8 + (lane >> 3), ch = lane & 7;
                        const int m = m0 + wrow_m + j * 16 + row;
                        const uint4 pk = *(const uint4*)(slab + row * 128 + ((ch ^ (row & 7)) << 4));
                        if (m < M) *(uint4*)(outp + (long long)m * g.ldo + n0 + wrow_n + ch * 8) = pk;
                    }
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");   // reads retired before the next chunk overwrites the slab
                }
            } else {
                // f32 output / residual stream (x += A . W^T + b): 16 rows x 32 columns per pass (128-byte row segments).
                // The residual values are fetched for a half / quarter of the wave tile at once, in the row-segment layout of the
                // stores (8-12 independent 16-byte loads per lane in flight): fetched chunk by chunk, each of the 16 passes of a tile
                // waited for its own HBM round trip (proj: 67 us for a 39 us memory floor)
                // Loads and stores go through a buffer descriptor over the output with an out-of-range offset for rows past M
                // (reads return 0, writes are dropped) instead of `if (m < M)`: inside a branch hipcc cannot count the memory
                // operations in flight and waits vmcnt(0) before every use of a fetched residual value - and vmcnt counts STORES
                // on this chip, so each 16-row pass waited for the previous pass's stores to be acknowledged (proj 57 us / fc2
                // 131 us against 40 / 118 us with a plain bf16 epilogue).
                const bool rmw = g.flags & YV_EPI_RES_F32;
                const auto rsO = __builtin_amdgcn_make_buffer_rsrc(g.out, 0, (int)(((long long)(M - 1) * g.ldo + g.N) * 4), 0x00020000);
                constexpr int NPART = MF <= 5 ? 2 : 4;             // residual registers in flight: 16 * JA (the accumulators hold 16 * MF)
                constexpr int JA = (MF + NPART - 1) / NPART;
                auto out_off = [&](int j, int ip, int it) __attribute__((always_inline)) {
                    const int row = it * 8 + (lane >> 3), ch = lane & 7;
                    const int m = m0 + wrow_m + j * 16 + row;
                    return m < M ? (uint32_t)((m * g.ldo + n0 + wrow_n + ip * 32 + ch * 4) * 4) : 0x80000000u;
                };
#pragma unroll
                for (int half = 0; half < NPART; ++half) {
                    const int j0 = half * JA, jn = (MF - j0) < JA ? (MF - j0 > 0 ? MF - j0 : 0) : JA;
                    u32x4 xr[JA][2][2];
                    if (rmw) {
#pragma unroll
                        for (int jj = 0; jj < JA; ++jj)
#pragma unroll
                            for (int ip = 0; ip < 2; ++ip)
#pragma unroll
                                for (int it = 0; it < 2; ++it)
                                    xr[jj][ip][it] = __builtin_amdgcn_raw_buffer_load_b128(rsO, jj < jn ? out_off(j0 + jj, ip, it) : 0x80000000u, 0, 0);
                    }
#pragma unroll
                    for (int jj = 0; jj < JA; ++jj) {
                        if (jj >= jn) continue;
                        const int j = j0 + jj;
#pragma unroll
                        for (int ip = 0; ip < 2; ++ip) {
#pragma unroll
                            for (int ii = 0; ii < 2; ++ii) {
                                const int i = ip * 2 + ii;
                                const float4 bvi = *(const float4*)(bl + i * 16);
                                *(float4*)(slab + fr * 128 + (((ii * 4 + fq) ^ (fr & 7)) << 4)) =
                                    make_float4(acc[i][j][0] + bvi.x, acc[i][j][1] + bvi.y, acc[i][j][2] + bvi.z, acc[i][j][3] + bvi.w);
                            }
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
#pragma unroll
                            for (int it = 0; it < 2; ++it) {
                                const int row = it * 8 + (lane >> 3), ch = lane & 7;
                                float4 v = *(const float4*)(slab + row * 128 + ((ch ^ (row & 7)) << 4));
                                if (rmw) {
                                    const u32x4 x = xr[jj][ip][it];
                                    v.x += __uint_as_float(x[0]); v.y += __uint_as_float(x[1]);
                                    v.z += __uint_as_float(x[2]); v.w += __uint_as_float(x[3]);
                                }
                                const u32x4 pk = {__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w)};
                                __builtin_amdgcn_raw_buffer_store_b128(pk, rsO, out_off(j, ip, it), 0, 0);
                            }
                            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                        }
                    }
                }
            }
        }
        if constexpr (DIAG) {
            asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
            const uint32_t de1 = stamp();
            dg[6] += de1 - de0_; ds0 = de1;
        }
        if (!has_next) break;
        seq += Lx;
        m0 = m0n; n0 = n0n;
#pragma unroll
        for (int k = 0; k < 4; ++k) { ocur[k][0] = onxt[k][0]; ocur[k][1] = onxt[k][1]; }
        has_next = seq + Lx < seq1;
        if (has_next) { coords(seq + Lx, m0n, n0n); set_offsets(onxt, m0n, n0n); }
    }
    if (wm == 0) bar();                                        // group 0 waits for group 1's last barrier
    if constexpr (DIAG) {
        const uint32_t dk1 = stamp();
        if (lane == 0) {
            uint32_t* o = (uint32_t*)g.partial + ((long long)blockIdx.x * 8 + wave) * 16;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = dg[i];
            o[8] = dk1 - dk0;
        }
    }
}

// ---------------------------------------------------------------------------------------------
// one persistent launch: tiles of bm rows x 256 columns, a grid of at most n_cu workgroups of 512 threads
int launch_persistent(void (*kern)(GemmArgs), int bm, size_t lds, GemmArgs& g, hipStream_t st, int n_cu) {
    g.tiles_m = (g.M + bm - 1) / bm;
    g.tiles_n = g.N / 256;
    if (!yv_grant_lds((const void*)kern, lds)) return YV_ERR_LAUNCH;
    const int tiles = g.tiles_m * g.tiles_n;
    launch_timed(kern, tiles < n_cu ? tiles : n_cu, 512, lds, st, g);
    return yv_launch_status();
}

template <int MF0, int MF1, bool F32OUT>
int launch_p8_inst2(GemmArgs& g, hipStream_t st, int n_cu) {
    return launch_persistent(gemm_p8_kernel<MF0, MF1, F32OUT>, 32 * (MF0 + MF1), 2 * 65536 + 8 * 2048 + 16384, g, st, n_cu);
}

template <int MF0, int MF1>
int launch_p8_inst(GemmArgs& g, hipStream_t st, int n_cu) {
    // the f32 epilogue keeps a residual prefetch next to the accumulators: only the tiles up to 192 rows have the registers for it
    if constexpr (MF0 + MF1 <= 6) {
        if (g.flags & (YV_EPI_RES_F32 | YV_EPI_OUT_F32)) return launch_p8_inst2<MF0, MF1, true>(g, st, n_cu);
    }
    return launch_p8_inst2<MF0, MF1, false>(g, st, n_cu);
}

// ---------------------------------------------------------------------------------------------
// gemm_p9_kernel (round 3): the persistent tile walk, LDS map and LDS-DMA addressing of gemm_p8_kernel with a FREE-RUNNING main
// loop.  What the per-segment stamps of the DIAG build showed for gemm_p8_kernel (tools/gemm_lab.hip): a phase costs
// ~890 cycles where its two MFMA segments need 512; the read segment is not LDS latency but the ISSUE of the two LDS-DMA
// instructions (~85 cycles each while the four waves of a group issue theirs at once; the waits on landing DMA are ~25 cycles
// per K tile), and each of the 8 barriers of a K tile costs the last arriver ~65 cycles.  So here:
//   * ONE barrier per K tile instead of eight.  A wave's program for a K tile is P = ceil(MF / 2) phases of 16 MFMAs (two row
//     fragments x four column fragments x two 32-deep steps); the fragment reads of phase p+1 are issued at the top of phase p into
//     the other half of a two-deep register ring (16 registers each), the weight fragments of K tile t+1 replace those of K tile t
//     in place inside the last phase (after their last use), so LDS latency is covered by the wave's OWN MFMAs and the two waves of
//     a SIMD are not forced to alternate: whichever has operands issues, and the waves of a workgroup drift apart instead of
//     bursting on the LDS-DMA path together;
//   * the sync point S (end of phase P-2: vmcnt(0) + lgkmcnt(0) + barrier) retires K tile t+1 and frees the whole stage of K tile
//     t at once (its last fragment reads were issued one phase earlier); the 8 DMA instructions per wave and K tile are spread over
//     the phases that follow S (activation pieces first: they can miss L2; weight pieces last: they never do; none in the phase
//     that ends in the next S);
//   * LDS-free epilogue.  bf16 outputs: the weight rows of a wave's 64 columns are PERMUTED on the DMA source side so that MFMA
//     fragment i, row r holds column (r >> 2) * 16 + i * 4 + (r & 3): a lane's 16 accumulator values of one output row are 16
//     consecutive columns = two 16-byte stores straight from registers (64-byte row segments per wave-instruction).  f32 outputs
//     keep the plain order (a lane's four values per fragment are 16 bytes, a fragment's 16 columns one 64-byte segment).  The
//     slabs, their lgkmcnt round trips (5.5 k cycles per 256 x 256 tile) and 16 KB of LDS are gone.
// Instances: MF (16-row fragments per wave group; tile = 32 MF rows x 256 columns) in 5..8; K / 64 >= 2, even when P is odd.
// ---------------------------------------------------------------------------------------------
template <int V> using ic = std::integral_constant<int, V>;
#ifndef YV_P9_STORE_AUX
#define YV_P9_STORE_AUX 0              // cache policy bits of the bf16 output stores (2 = nt: streaming; experiment builds only)
#endif

template <int MF, bool F32OUT, int DIAG = 0 /* tools/gemm_lab.hip only: cycle sums into g.partial */,
          int EXT = 0 /* trainer epilogues of the bf16 output: 1 = YV_EPI_SAVE_PRE (fc1 forward), 2 = YV_EPI_GELU_BWD (fc2 data gradient) */,
          bool MX = false /* OCP MXFP8 operands (e4m3 bytes + one E8M0 scale per 32 K): a 128-byte LDS row is 128 K elements = ONE
                             block-scaled MFMA (v_mfma_scale_f32_16x16x128_f8f6f4) per fragment pair and K tile; same DMA, LDS images,
                             fragment reads and schedule, twice the flops per K tile; the two 1 KB scale rows of a K tile travel with
                             its activation / weight pieces (issued by waves 0 / 1) */>
__global__ __launch_bounds__(512) void gemm_p9_kernel(GemmArgs g) {
    constexpr int NF = 4, P = (MF + 1) / 2;
    static_assert(EXT == 0 || (!F32OUT && MF <= 7), "aux epilogues: bf16 output, tiles of up to 224 rows (registers)");
    constexpr int MF0 = (MF + 1) / 2, MF1 = MF - MF0;          // DMA halves of the activation rows of a group (piece bookkeeping of p8)
    constexpr int RG = MF * 16, BM = 2 * RG;
    constexpr int A_BYTES = 256 * 128, SC0 = 2 * A_BYTES, STAGE = 2 * A_BYTES + (MX ? 2048 : 0), BIAS0 = 2 * STAGE;
    constexpr int ESZ = MX ? 1 : 2;                               // bytes per operand element; K elements per 128-byte row: 128 / ESZ
    constexpr int KT = 128 / ESZ;
    constexpr bool PERM = !F32OUT;
    static_assert(MF >= 3 && MF <= 8, "tile heights 96..256");
    static_assert(MF >= 5 || (!MX && EXT == 0), "96 / 128-row tiles: plain bf16 operands only");
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    const int tid = threadIdx.x, lane = tid & 63, wave = __builtin_amdgcn_readfirstlane(tid >> 6);

    int M = g.M;
    if (g.m_dev) { long long md = (long long)g.m_dev[0] * g.m_mul; M = md < M ? (int)md : M; }
    const int tiles_m = (M + BM - 1) / BM, tiles_n = g.N >> 8;
    const int ntiles = tiles_m * tiles_n;
    const int G = gridDim.x;
    int Lx, seq0, seq1, lid;
    if (g.sched == 1) {
        const int nx = G < 8 ? G : 8;
        const int xcd = (int)blockIdx.x % nx;
        lid = (int)blockIdx.x / nx;
        Lx = (G - xcd + nx - 1) / nx;
        int cum = 0;
        for (int y = 0; y < xcd; ++y) cum += (G - y + nx - 1) / nx;
        seq0 = (int)((long long)ntiles * cum / G); seq1 = (int)((long long)ntiles * (cum + Lx) / G);
    } else {
        const int q = G >> 3, r = G & 7, x = blockIdx.x & 7;
        lid = (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + ((int)blockIdx.x >> 3);
        Lx = G; seq0 = 0; seq1 = ntiles;
    }
    if (seq0 + lid >= seq1) return;
    {
        float* bl = (float*)(smem + BIAS0);
        for (int i = tid; i < g.N; i += 512) bl[i] = (g.flags & YV_EPI_BIAS) ? g.bias[i] : 0.0f;
    }
    const auto rsA = __builtin_amdgcn_make_buffer_rsrc((void*)g.a0, 0, (int)(((long long)(g.M - 1) * g.lda0 + g.K) * ESZ), 0x00020000);
    const auto rsW = __builtin_amdgcn_make_buffer_rsrc((void*)g.w, 0, (int)((long long)g.N * g.K * ESZ), 0x00020000);
    const int nk_all = g.K / KT;
    const auto rsSA = __builtin_amdgcn_make_buffer_rsrc((void*)(MX ? (const void*)g.mx_sa : (const void*)g.a0), 0,
                                                        MX ? (int)((long long)nk_all * g.mx_rows_a * 4) : 16, 0x00020000);
    const auto rsSW = __builtin_amdgcn_make_buffer_rsrc((void*)(MX ? (const void*)g.mx_sw : (const void*)g.w), 0,
                                                        MX ? (int)((long long)nk_all * g.mx_rows_w * 4) : 16, 0x00020000);
    const auto rsO = __builtin_amdgcn_make_buffer_rsrc(g.out, 0, (int)(((long long)(M - 1) * g.ldo + g.N) * (F32OUT ? 4 : 2)), 0x00020000);
    // f32 residual read from another tensor of the output's layout (trainer: x_mid = x_in + ...), else read-modify-write of `out`
    const auto rsR = __builtin_amdgcn_make_buffer_rsrc(F32OUT && g.resf ? (void*)g.resf : g.out, 0,
                                                       (int)(((long long)(M - 1) * g.ldo + g.N) * (F32OUT ? 4 : 2)), 0x00020000);
    // bf16 side tensor of the trainer epilogues (EXT): pre-activation, written (SAVE_PRE) or read (GELU_BWD)
    const auto rsX = __builtin_amdgcn_make_buffer_rsrc(EXT ? (void*)g.aux : g.out, 0, (int)(((long long)(M - 1) * (EXT ? g.ldaux : g.ldo) + g.N) * 2), 0x00020000);

    const int wm = wave >> 2, wn = wave & 3;
    const int wrow_m = wm * RG, wrow_n = wn * 64;
    const int fr = lane & 15, fq = lane >> 4;
    const int lrow = lane >> 3, lch = lane & 7;
    auto coords = [&](int seq, int& m0, int& n0) __attribute__((always_inline)) {
        const int GM = g.group_m, per = GM * tiles_n;
        const int grp = seq / per, first = grp * GM;
        const int gsz = (tiles_m - first) < GM ? (tiles_m - first) : GM;
        const int in = seq - grp * per;
        m0 = (first + in % gsz) * BM;
        n0 = (in / gsz) << 8;
    };
    auto a_piece_row = [&](int h, int s) __attribute__((always_inline)) -> int {
        const int len8 = (h == 0 ? MF0 : MF1) * 2;
        if (s >= 2 * len8) return -1;
        const int grp = s / len8, r8 = s - grp * len8;
        return grp * RG + (h == 0 ? 0 : MF0 * 16) + r8 * 8;
    };
    // DMA source offsets.  Activation pieces: per-lane byte offset of (tile row, swizzled chunk) - ONE set, pointed at the next
    // tile from K tile nk-2 on (the current tile's last activation pieces are issued in K tile nk-3); rows past M get an
    // out-of-range offset (the range check returns zeros).  Weight pieces: a lane part that never changes + the tile's n0 * K
    // in the instruction's scalar offset.
    auto set_a_offsets = [&](uint32_t (&o)[2][2], int m0, bool valid) __attribute__((always_inline)) {
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const int s_ = wave * 2 + j;
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int r0 = a_piece_row(h, s_);
                const int ra = r0 + lrow, m = m0 + ra;
                o[h][j] = (valid && r0 >= 0 && m < g.M) ? (uint32_t)((long long)m * g.lda0 * ESZ + ((lch ^ (ra & 7)) << 4)) : 0x80000000u;
            }
        }
    };
    uint32_t ow[2][2];
#pragma unroll
    for (int j = 0; j < 2; ++j) {
        const int rh = (wave * 2 + j) * 8 + lrow;
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int rw = (rh >> 5) * 64 + h * 32 + (rh & 31);          // LDS row of the W tile
            // PERM: LDS row (block b, fragment i, row r) holds weight row b * 64 + (r >> 2) * 16 + i * 4 + (r & 3)
            const int rsrc = PERM ? ((rw & ~63) | (((rw & 15) >> 2) << 4) | (((rw >> 4) & 3) << 2) | (rw & 3)) : rw;
            ow[h][j] = (uint32_t)(rsrc * g.K * ESZ + ((lch ^ (rw & 7)) << 4));
        }
    }
    auto lds_dst = [&](int kind, int j) __attribute__((always_inline)) -> int {
        const int s_ = wave * 2 + j;
        if (kind < 2) {
            const int r0 = a_piece_row(kind, s_);
            return (r0 >= 0 ? r0 : BM) * 128;
        }
        const int rb = s_ * 8;
        return A_BYTES + ((rb >> 5) * 64 + (kind - 2) * 32 + (rb & 31)) * 128;
    };

    const int nk = g.K / KT;
    int sa_row0 = 0;                                             // MX: first activation row of the tile the `oa` offsets point at
    uint32_t oa[2][2];
    int seq = seq0 + lid, m0, n0, m0n = 0, n0n = 0;
    coords(seq, m0, n0);
    set_a_offsets(oa, m0, true);
    sa_row0 = m0;
    bool has_next = seq + Lx < seq1;
    if (has_next) coords(seq + Lx, m0n, n0n);
    int gk = 0;                                                // K tiles consumed so far (stage of a K tile = parity)

    // piece `kind` (0, 1 activation halves; 2, 3 weight halves) of K tile k of the tile whose column origin is nb
    // MX: the K tile's 256 activation-row scale dwords (wave 0, with activation half 0) / weight-row scale dwords (wave 1, with weight
    // half 0): 1 KB each = one wave instruction; rows past the scale array read zeros (those rows are never stored)
    auto issue_a = [&](int kind, int k, int st) __attribute__((always_inline)) {
        unsigned char* base = smem + (st & 1) * STAGE;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsA, (lds_void_t)(base + lds_dst(kind, j)), 16, (int)oa[kind][j], k * 128, 0, 0);
        if constexpr (MX) {
            if (kind == 0 && wave == 0)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsSA, (lds_void_t)(base + SC0), 16, lane * 16,
                                                         (int)(((long long)k * g.mx_rows_a + sa_row0) * 4), 0, 0);
        }
    };
    auto issue_w = [&](int kind, int k, int st, int nb) __attribute__((always_inline)) {
        unsigned char* base = smem + (st & 1) * STAGE;
        const int so = nb * g.K * ESZ + k * 128;
#pragma unroll
        for (int j = 0; j < 2; ++j)
            __builtin_amdgcn_raw_ptr_buffer_load_lds(rsW, (lds_void_t)(base + lds_dst(kind, j)), 16, (int)ow[kind - 2][j], so, 0, 0);
        if constexpr (MX) {
            if (kind == 2 && wave == 1)
                __builtin_amdgcn_raw_ptr_buffer_load_lds(rsSW, (lds_void_t)(base + SC0 + 1024), 16, lane * 16,
                                                         (int)(((long long)k * g.mx_rows_w + nb) * 4), 0, 0);
        }
    };
    // K tile t + d (d in {1, 2}) of this tile or, past its end, of the next tile
    auto issue_rel = [&](int kind, int t, int d, auto tail_c) __attribute__((always_inline)) {
        constexpr int TAIL = decltype(tail_c)::value;             // 0: t <= nk-3, 1: t = nk-2, 2: t = nk-1
        const int st = gk + d;
        if (kind < 2) issue_a(kind, TAIL + d <= 2 ? t + d : TAIL + d - 3, st);       // `oa` already points at the right tile
        else if (TAIL + d <= 2) issue_w(kind, t + d, st, n0);
        else if (has_next) issue_w(kind, TAIL + d - 3, st, n0n);
    };

    f32x4 acc[NF][MF];
    bf16x8 fa[2][2][2];                                         // [ring half][row fragment of the pair][k step]
    bf16x8 fw[4][2];                                            // [column fragment][k step] of the current K tile
    // MX: a fragment is the 8-register operand of the 128-deep MFMA (chunks fq and 4 + fq of the row), built where it is read
    i32x8 fa8[2][2], fw8[4];
    int sca[2][2], scw[4];                                       // this lane's block scale (byte 0) per row fragment
    auto read_pair = [&](auto half_c, const unsigned char* A, int pr) __attribute__((always_inline)) {
        constexpr int HALF = decltype(half_c)::value;
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) {
            if (2 * pr + jj >= MF) continue;
            const int rr = wrow_m + (2 * pr + jj) * 16 + fr;
            if constexpr (MX) {
                const u32x4 lo = *(const u32x4*)(A + rr * 128 + ((fq ^ (rr & 7)) << 4));
                const u32x4 hi = *(const u32x4*)(A + rr * 128 + (((4 + fq) ^ (rr & 7)) << 4));
                fa8[HALF][jj] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                sca[HALF][jj] = (int)(*(const uint32_t*)(A + SC0 + rr * 4) >> (8 * fq));
            } else {
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) fa[HALF][jj][ks] = *(const bf16x8*)(A + rr * 128 + (((ks * 4 + fq) ^ (rr & 7)) << 4));
            }
        }
    };
    auto read_w = [&](const unsigned char* W, int ks) __attribute__((always_inline)) {   // W = stage base + A_BYTES
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int rr = wrow_n + i * 16 + fr;
            if constexpr (MX) {
                if (ks == 0) {
                    const u32x4 lo = *(const u32x4*)(W + rr * 128 + ((fq ^ (rr & 7)) << 4));
                    const u32x4 hi = *(const u32x4*)(W + rr * 128 + (((4 + fq) ^ (rr & 7)) << 4));
                    fw8[i] = (i32x8){(int)lo[0], (int)lo[1], (int)lo[2], (int)lo[3], (int)hi[0], (int)hi[1], (int)hi[2], (int)hi[3]};
                    // LDS row rr holds weight row (rr & ~63) | ((rr & 15) >> 2) << 4 | ((rr >> 4) & 3) << 2 | (rr & 3) when PERM
                    const int rs_ = PERM ? ((rr & ~63) | (((rr & 15) >> 2) << 4) | (((rr >> 4) & 3) << 2) | (rr & 3)) : rr;
                    scw[i] = (int)(*(const uint32_t*)(W + (SC0 - A_BYTES) + 1024 + rs_ * 4) >> (8 * fq));
                }
            } else {
                fw[i][ks] = *(const bf16x8*)(W + rr * 128 + (((ks * 4 + fq) ^ (rr & 7)) << 4));
            }
        }
    };
    auto mma = [&](auto half_c, int pr, int ks) __attribute__((always_inline)) {
        constexpr int HALF = decltype(half_c)::value;
        if constexpr (MX) { if (ks == 0) return; }                // one 128-deep MFMA per fragment pair: issued in the second slot
        __builtin_amdgcn_s_setprio(1);
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) {
                if (2 * pr + jj >= MF) continue;
                if constexpr (MX) {
                    // inline asm: around the builtin hipcc's register allocation needs ~100 more VGPRs (every instance spilled 120-360
                    // registers into the K loop; with bf16 MFMAs in its place none did).  Operands come from LDS reads (waited for by
                    // the compiler, which sees them as inputs) and a shift issued a phase earlier: no hazard window inside the string
                    // beyond the s_nop; the accumulator chains MFMA -> MFMA (no wait states) and is next read in the epilogue.
                    asm volatile("s_nop 1\n\tv_mfma_scale_f32_16x16x128_f8f6f4 %0, %1, %2, %0, %3, %4 op_sel_hi:[0,0,0]"
                                 : "+v"(acc[i][2 * pr + jj]) : "v"(fw8[i]), "v"(fa8[HALF][jj]), "v"(scw[i]), "v"(sca[HALF][jj]));
                } else {
                    acc[i][2 * pr + jj] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fw[i][ks], fa[HALF][jj][ks], acc[i][2 * pr + jj], 0, 0, 0);
                }
            }
        __builtin_amdgcn_s_setprio(0);
    };
    uint32_t dg[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dtb = 0, dtc = 0;   // DIAG: [0] sync waits [1] barrier waits [2] main loops [3] epilogues
    auto stamp = [&]() __attribute__((always_inline)) -> uint32_t { return (uint32_t)__builtin_amdgcn_s_memtime(); };   // [4] first sync of a tile [5] tiles [6] syncs
    // DMA pieces of the window that follows a sync point: phase P-1 (of the K tile of the sync point) takes both activation halves
    // of K tile t+2, the first phases of the next K tile the weight halves of (its) K tile t+1; phase P-2 - the one that ends in
    // the next sync point - issues nothing, so the youngest piece has a whole phase to land before it is waited for
    auto dma_for_phase = [&](int p, int t, auto tail_c) __attribute__((always_inline)) {
        if constexpr (P == 2) {
            // 96 / 128-row tiles: the phase that follows the sync point is also the only one that does not end in the next: all eight
            // pieces of K tile t+2 go here (its stage - K tile t's - is free: the weight fragments of K tile t were read a K tile ago)
            if (p == 1) { issue_rel(0, t, 2, tail_c); issue_rel(1, t, 2, tail_c); issue_rel(2, t, 2, tail_c); issue_rel(3, t, 2, tail_c); }
            return;
        }
        if (p == P - 1) { issue_rel(0, t, 2, tail_c); issue_rel(1, t, 2, tail_c); return; }
        if constexpr (P == 4) { if (p < 2) issue_rel(2 + p, t, 1, tail_c); }
        else { if (p == 0) { issue_rel(2, t, 1, tail_c); issue_rel(3, t, 1, tail_c); } }
    };
    // one K tile.  PAR: ring half that holds row pair 0 of this K tile (odd P: alternates).  LASTK: t = nk - 1
    auto ktile = [&](int t, auto tail_c, auto par_c) __attribute__((always_inline)) {
        constexpr int TAIL = decltype(tail_c)::value, PAR = decltype(par_c)::value;
        if constexpr (TAIL == 1) { set_a_offsets(oa, m0n, has_next); sa_row0 = m0n; }   // from here on activation pieces belong to the next tile
        const unsigned char* A = smem + (gk & 1) * STAGE;
        const unsigned char* An = smem + ((gk + 1) & 1) * STAGE;
        auto phase = [&](auto p_c) __attribute__((always_inline)) {
            constexpr int p = decltype(p_c)::value;
            constexpr int CUR = (PAR + p) & 1, NXT = CUR ^ 1;
            if constexpr (p + 1 < P) read_pair(ic<NXT>{}, A, p + 1);
            else if constexpr (TAIL != 2) read_pair(ic<NXT>{}, An, 0);          // row pair 0 of the next K tile
            dma_for_phase(p, t, tail_c);
            mma(ic<CUR>{}, p, 0);
            if constexpr (p == P - 1 && TAIL != 2 && !MX) {
                __builtin_amdgcn_sched_barrier(0);
                read_w(An + A_BYTES, 0);                                        // in place: k step 0 of K tile t had its last use
            }
            mma(ic<CUR>{}, p, 1);
            if constexpr (p == P - 1 && TAIL != 2) {
                __builtin_amdgcn_sched_barrier(0);
                if constexpr (MX) read_w(An + A_BYTES, 0);                      // (MX: both halves feed the one MFMA of a fragment pair)
                else read_w(An + A_BYTES, 1);
            }
            if constexpr (p == P - 2) {
                // sync point: every DMA issued so far (all of K tile t+1) has landed, this wave's fragment reads are retired;
                // behind the barrier K tile t+1 is visible to every wave and the stage of K tile t is free
                if constexpr (DIAG) {
                    __builtin_amdgcn_sched_barrier(0);
                    const uint32_t ta = stamp();
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    if (dg[6]) dg[1] += dtc - dtb;                 // barrier wait of the previous sync point (stamp landed by now)
                    const uint32_t tb = stamp();
                    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    dg[0] += tb - ta; if (t == 0) dg[4] += tb - ta; dg[6] += 1; dtb = tb;
                    bar();
                    __builtin_amdgcn_sched_barrier(0);
                    dtc = stamp();
                } else {
                    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
                    __builtin_amdgcn_sched_barrier(0);
                    bar();
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        };
        phase(ic<0>{});
        if constexpr (P > 1) phase(ic<1>{});
        if constexpr (P > 2) phase(ic<2>{});
        if constexpr (P > 3) phase(ic<3>{});
        ++gk;
    };

    __syncthreads();                                           // bias image complete (no DMA in flight yet)
    // ---- first tile: K tile 0 complete, the activation halves of K tile 1 in flight ---------------------------------------
    issue_a(0, 0, 0); issue_a(1, 0, 0); issue_w(2, 0, 0, n0); issue_w(3, 0, 0, n0);
    issue_a(0, 1, 1); issue_a(1, 1, 1);
    if constexpr (P == 2) {                                    // (no phase 0 issue of K tile 1's weight halves in this schedule)
        issue_w(2, 1, 1, n0); issue_w(3, 1, 1, n0);
        asm volatile("s_waitcnt vmcnt(8)" ::: "memory");
    } else asm volatile("s_waitcnt vmcnt(4)" ::: "memory");
    bar();

    const uint32_t dk0 = DIAG ? stamp() : 0;
    for (;;) {
        uint32_t dt0 = 0, dt1 = 0;
        if constexpr (DIAG) dt0 = stamp();
#pragma unroll
        for (int i = 0; i < NF; ++i)
#pragma unroll
            for (int j = 0; j < MF; ++j) acc[i][j] = (f32x4){0.f, 0.f, 0.f, 0.f};
        {   // tile prologue: weight fragments and row pair 0 of K tile 0 (landed and visible since the previous sync point)
            const unsigned char* A = smem + (gk & 1) * STAGE;
            read_w(A + A_BYTES, 0); read_w(A + A_BYTES, 1);
            read_pair(ic<0>{}, A, 0);
        }
        if constexpr (P & 1) {
            for (int t = 0; t < nk - 2; t += 2) { ktile(t, ic<0>{}, ic<0>{}); ktile(t + 1, ic<0>{}, ic<1>{}); }
            ktile(nk - 2, ic<1>{}, ic<0>{});
            ktile(nk - 1, ic<2>{}, ic<1>{});
        } else {
            for (int t = 0; t < nk - 2; ++t) ktile(t, ic<0>{}, ic<0>{});
            ktile(nk - 2, ic<1>{}, ic<0>{});
            ktile(nk - 1, ic<2>{}, ic<0>{});
        }
        // ---- epilogue: straight from the accumulators ------------------------------------------------------------------------
        if constexpr (DIAG) { dt1 = stamp(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); dg[2] += dt1 - dt0; dg[5] += 1; }
        if constexpr (!F32OUT) {
            const bool gelu = g.flags & YV_EPI_GELU;
            const float* bl = (const float*)(smem + BIAS0) + n0 + wrow_n + fq * 16;
            float4 bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[i] = *(const float4*)(bl + i * 4);
            if constexpr (EXT == 2) {
                // out = bf16(acc + b) * gelu'(u), u = the pre-activation the forward saved (same rounding steps as the 128 x 128 kernel's
                // epilogue); u of two row fragments is in flight together
#pragma unroll
                for (int j0 = 0; j0 < MF; j0 += 2) {
                    u32x4 ur[2][2];
                    uint32_t offx[2];
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        const int m = m0 + wrow_m + (j0 + jj) * 16 + fr;
                        offx[jj] = (j0 + jj < MF && m < M) ? (uint32_t)((m * g.ldaux + n0 + wrow_n + fq * 16) * 2) : 0x80000000u;
                        ur[jj][0] = __builtin_amdgcn_raw_buffer_load_b128(rsX, offx[jj], 0, 0);
                        ur[jj][1] = __builtin_amdgcn_raw_buffer_load_b128(rsX, offx[jj] + 16, 0, 0);
                    }
#pragma unroll
                    for (int jj = 0; jj < 2; ++jj) {
                        if (j0 + jj >= MF) continue;
                        const int j = j0 + jj;
                        const int m = m0 + wrow_m + j * 16 + fr;
                        uint32_t pk[8];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            const uint32_t d01 = pack_bf16x2(acc[i][j][0] + bv[i].x, acc[i][j][1] + bv[i].y);
                            const uint32_t d23 = pack_bf16x2(acc[i][j][2] + bv[i].z, acc[i][j][3] + bv[i].w);
                            const uint32_t u01 = ur[jj][i >> 1][(i & 1) * 2], u23 = ur[jj][i >> 1][(i & 1) * 2 + 1];
                            pk[2 * i] = pack_bf16x2(bf16_to_f32((uint16_t)(d01 & 0xffff)) * gelu_grad_f(bf16_to_f32((uint16_t)(u01 & 0xffff))),
                                                    bf16_to_f32((uint16_t)(d01 >> 16)) * gelu_grad_f(bf16_to_f32((uint16_t)(u01 >> 16))));
                            pk[2 * i + 1] = pack_bf16x2(bf16_to_f32((uint16_t)(d23 & 0xffff)) * gelu_grad_f(bf16_to_f32((uint16_t)(u23 & 0xffff))),
                                                        bf16_to_f32((uint16_t)(d23 >> 16)) * gelu_grad_f(bf16_to_f32((uint16_t)(u23 >> 16))));
                        }
                        const uint32_t off = m < M ? (uint32_t)((m * g.ldo + n0 + wrow_n + fq * 16) * 2) : 0x80000000u;
                        __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk[0], pk[1], pk[2], pk[3]}, rsO, off, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk[4], pk[5], pk[6], pk[7]}, rsO, off, 16, 0);
                    }
                }
            } else if (MX && (g.flags & YV_EPI_OUT_MXFP8)) {
                // the consumer is another MXFP8 GEMM (fc1 -> fc2): the lane's 16 consecutive (bf16-rounded) outputs + the 16 of lane ^ 16
                // are one 32-column MX block; the quantiser of mx_quant.h, as the 128 x 128 kernel's epilogue (byte-identical images)
#pragma unroll
                for (int j = 0; j < MF; ++j) {
                    const int m = m0 + wrow_m + j * 16 + fr;
                    float f[16];
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v0 = acc[i][j][0] + bv[i].x, v1 = acc[i][j][1] + bv[i].y;
                        float v2 = acc[i][j][2] + bv[i].z, v3 = acc[i][j][3] + bv[i].w;
                        if (gelu) { v0 = gelu_f(v0); v1 = gelu_f(v1); v2 = gelu_f(v2); v3 = gelu_f(v3); }
                        f[4 * i] = bf16_to_f32(f32_to_bf16(v0)); f[4 * i + 1] = bf16_to_f32(f32_to_bf16(v1));
                        f[4 * i + 2] = bf16_to_f32(f32_to_bf16(v2)); f[4 * i + 3] = bf16_to_f32(f32_to_bf16(v3));
                    }
                    uint32_t q4[4];
                    const int e = mx_quant_block<16>(f, q4);
                    if (m < M) {
                        const int n = n0 + wrow_n + fq * 16;
                        *(uint4*)(g.mxq + (long long)m * g.ldmxq + n) = make_uint4(q4[0], q4[1], q4[2], q4[3]);
                        if (!(fq & 1)) g.mxs[mx_scale_kmajor(n >> 5, g.mx_rows, m)] = (uint8_t)(e + 127);
                    }
                }
            } else {
#pragma unroll
                for (int j = 0; j < MF; ++j) {
                    const int m = m0 + wrow_m + j * 16 + fr;
                    uint32_t pk[8];
                    if constexpr (EXT == 1) {                     // the pre-activation, bf16 (the backward's gelu'(u) reads it)
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            pk[2 * i] = pack_bf16x2(acc[i][j][0] + bv[i].x, acc[i][j][1] + bv[i].y);
                            pk[2 * i + 1] = pack_bf16x2(acc[i][j][2] + bv[i].z, acc[i][j][3] + bv[i].w);
                        }
                        const uint32_t offx = m < M ? (uint32_t)((m * g.ldaux + n0 + wrow_n + fq * 16) * 2) : 0x80000000u;
                        __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk[0], pk[1], pk[2], pk[3]}, rsX, offx, 0, 0);
                        __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk[4], pk[5], pk[6], pk[7]}, rsX, offx, 16, 0);
                    }
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v0 = acc[i][j][0] + bv[i].x, v1 = acc[i][j][1] + bv[i].y;
                        float v2 = acc[i][j][2] + bv[i].z, v3 = acc[i][j][3] + bv[i].w;
                        if (gelu) { v0 = gelu_f(v0); v1 = gelu_f(v1); v2 = gelu_f(v2); v3 = gelu_f(v3); }
                        pk[2 * i] = pack_bf16x2(v0, v1); pk[2 * i + 1] = pack_bf16x2(v2, v3);
                    }
                    const uint32_t off = m < M ? (uint32_t)((m * g.ldo + n0 + wrow_n + fq * 16) * 2) : 0x80000000u;
                    __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk[0], pk[1], pk[2], pk[3]}, rsO, off, 0, YV_P9_STORE_AUX);
                    __builtin_amdgcn_raw_buffer_store_b128((u32x4){pk[4], pk[5], pk[6], pk[7]}, rsO, off, 16, YV_P9_STORE_AUX);
                }
            }
        } else {
            const bool rmw = g.flags & YV_EPI_RES_F32;
            const float* bl = (const float*)(smem + BIAS0) + n0 + wrow_n + fq * 4;
            float4 bv[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) bv[i] = *(const float4*)(bl + i * 16);
            constexpr int JA = 2;                                // row fragments whose residual values are in flight together
#pragma unroll
            for (int j0 = 0; j0 < MF; j0 += JA) {
                u32x4 xr[JA][4];
                uint32_t off[JA];
#pragma unroll
                for (int jj = 0; jj < JA; ++jj) {
                    const int m = m0 + wrow_m + (j0 + jj) * 16 + fr;
                    off[jj] = (j0 + jj < MF && m < M) ? (uint32_t)((m * g.ldo + n0 + wrow_n + fq * 4) * 4) : 0x80000000u;
                    if (rmw) {
#pragma unroll
                        for (int i = 0; i < 4; ++i) xr[jj][i] = __builtin_amdgcn_raw_buffer_load_b128(rsR, off[jj] + i * 64, 0, 0);
                    }
                }
#pragma unroll
                for (int jj = 0; jj < JA; ++jj) {
                    if (j0 + jj >= MF) continue;
                    const int j = j0 + jj;
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        float v0 = acc[i][j][0] + bv[i].x, v1 = acc[i][j][1] + bv[i].y;
                        float v2 = acc[i][j][2] + bv[i].z, v3 = acc[i][j][3] + bv[i].w;
                        if (rmw) {
                            v0 += __uint_as_float(xr[jj][i][0]); v1 += __uint_as_float(xr[jj][i][1]);
                            v2 += __uint_as_float(xr[jj][i][2]); v3 += __uint_as_float(xr[jj][i][3]);
                        }
                        // the column step goes into the instruction's immediate offset, never into an SGPR soffset: behind a 16-byte
                        // store with a REGISTER soffset hipcc pads nothing before the next write of the data registers (LLVM takes that
                        // form to be free of the store-data hazard) and on gfx950 the store then read overwritten values (measured:
                        // 0.9 % of the outputs wrong, always the columns whose step needed a register: 128 and 192 bytes)
                        __builtin_amdgcn_raw_buffer_store_b128((u32x4){__float_as_uint(v0), __float_as_uint(v1), __float_as_uint(v2),
                                                                       __float_as_uint(v3)}, rsO, off[jj] + i * 64, 0, 0);
                    }
                }
            }
        }
        if constexpr (DIAG) { const uint32_t dt2 = stamp(); asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory"); dg[3] += dt2 - dt1; }
        if (!has_next) break;
        seq += Lx;
        m0 = m0n; n0 = n0n;
        has_next = seq + Lx < seq1;
        if (has_next) coords(seq + Lx, m0n, n0n);
    }
    if constexpr (DIAG) {
        const uint32_t dk1 = stamp();
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        dg[7] = dk1 - dk0;
        if (lane == 0) {
            uint32_t* o = (uint32_t*)g.partial + ((long long)blockIdx.x * 8 + wave) * 16;
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = dg[i];
        }
    }
}

template <int MF, bool F32OUT, int EXT = 0, bool MX = false>
int launch_p9_inst(GemmArgs& g, hipStream_t st, int n_cu) {
    return launch_persistent(gemm_p9_kernel<MF, F32OUT, 0, EXT, MX>, 32 * MF, 2 * 65536 + 16384 + (MX ? 4096 : 0), g, st, n_cu);
}

// The tile heights of one epilogue family (F32OUT, EXT, MX): what p9_tile_rows returns for it.
template <bool F32OUT, int EXT, bool MX>
int launch_p9_rows(GemmArgs& g, hipStream_t st, int n_cu, int rows) {
    if constexpr (!EXT && !MX) {
        if (rows == 128) return launch_p9_inst<4, F32OUT>(g, st, n_cu);
        if (rows == 96) return launch_p9_inst<3, F32OUT>(g, st, n_cu);
    }
    switch (rows) {
        case 224: return launch_p9_inst<7, F32OUT, EXT, MX>(g, st, n_cu);
        case 192: return launch_p9_inst<6, F32OUT, EXT, MX>(g, st, n_cu);
        case 160: return launch_p9_inst<5, F32OUT, EXT, MX>(g, st, n_cu);
        default: return launch_p9_inst<EXT ? 7 : 8, F32OUT, EXT, MX>(g, st, n_cu);
    }
}

}  // namespace

// grid of a persistent launch: the CU count of the current device (looked up once: the same value from every thread; n_cu != 0:
// that count instead, yv_linear_route), clipped by the calling thread's "linear_p8_cus"; 0: the device query failed
int yvgemm::persistent_cus(int n_cu) {
    static int n_cu_dev = 0;
    if (n_cu) return (g_opt_p8_cus > 0 && g_opt_p8_cus < n_cu) ? g_opt_p8_cus : n_cu;
    if (!n_cu_dev) {
        int dev = 0; hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) return 0;
        n_cu_dev = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    }
    return (g_opt_p8_cus > 0 && g_opt_p8_cus < n_cu_dev) ? g_opt_p8_cus : n_cu_dev;
}

// Tile height of gemm_p8_kernel: "linear_p8_rows", else minimise rounds x (rows + ~24 rows of epilogue and pipeline turn-around)
int yvgemm::p8_tile_rows(int M, int N, int flags, int n_cu) {
    const bool f32out = flags & (YV_EPI_RES_F32 | YV_EPI_OUT_F32);
    int best = f32out ? 192 : 256;
    if (g_opt_p8_rows) {
        best = g_opt_p8_rows < 128 ? 128 : g_opt_p8_rows;          // (96: a tile height of the free-running kernel only)
        if (f32out && best > 192) best = 192;
    } else {
        long long best_cost = -1;
        const int cand[5] = {256, 224, 192, 160, 128};
        for (int c = f32out ? 2 : 0; c < 5; ++c) {
            const long long tiles = (long long)((M + cand[c] - 1) / cand[c]) * (N / 256);
            const long long rounds = (tiles + n_cu - 1) / n_cu;
            const long long cost = rounds * (cand[c] + 24);
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = cand[c]; }
        }
    }
    return (best == 224 || best == 192 || best == 160 || best == 128) ? best : 256;    // a height without an instance: 256 rows
}

// Tile height of gemm_p9_kernel: forced_rows, else "linear_p8_rows", else minimise rounds x (rows + per-tile cost).  Instances:
// 160 / 192 / 224 rows in every epilogue family, 256 for the plain epilogues, 128 / 96 for the plain bf16-operand ones.
int yvgemm::p9_tile_rows(int M, int N, int K, int flags, bool mx, int n_cu, int forced_rows) {
    const bool f32out = flags & (YV_EPI_RES_F32 | YV_EPI_OUT_F32);
    const bool even_nk = ((K / (mx ? 128 : BK)) & 1) == 0;           // odd-P instances (160 / 192 rows) walk K tiles in pairs
    const bool ext = flags & (YV_EPI_SAVE_PRE | YV_EPI_GELU_BWD);
    int best = forced_rows ? forced_rows : g_opt_p8_rows;
    if (ext && best > 224) best = 224;
    if (!best) {
        long long best_cost = -1;
        const int cand[6] = {256, 224, 192, 160, 128, 96};
        const bool small_ok = !mx && !ext && g_opt_p9_small;       // 128 / 96-row tiles: instances exist for the plain epilogues
        for (int c = 0; c < (small_ok ? 6 : 4); ++c) {
            if (cand[c] <= 192 && cand[c] >= 160 && !even_nk) continue;
            if (cand[c] > 192 && f32out && even_nk) continue;      // f32 outputs: the residual prefetch next to the accumulators spills above 192 rows
            if (cand[c] > 224 && ext) continue;                     // trainer epilogues: up to 224 rows
            if (cand[c] > 160 && mx && f32out) continue;            // MX with f32 output: 160 rows (registers)
            const long long tiles = (long long)((M + cand[c] - 1) / cand[c]) * (N / 256);
            const long long rounds = (tiles + n_cu - 1) / n_cu;
            // a K tile of a tile costs its rows + a fixed part (weight pieces, sync point); the short tiles pay the weight fetch
            // over fewer rows and are worth it only where the taller ones leave CUs idle (tools/gemm_lab.hip, LAB_M=6304)
            const long long cost = rounds * (cand[c] + (cand[c] < 160 ? g_opt_p9_small_fixed : 16));
            if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = cand[c]; }
        }
    }
    if (best <= 192 && best >= 160 && !even_nk) best = 224;
    if (best == 224 || best == 192 || best == 160 || ((best == 128 || best == 96) && !ext && !mx)) return best;
    return ext ? 224 : 256;                                         // a height without an instance in this family
}

int yvgemm::launch_p8(GemmArgs& g, hipStream_t st, int rows, int n_cu) {
    g.sched = g_opt_p8_sched;
    switch (rows) {
        case 224: return launch_p8_inst<4, 3>(g, st, n_cu);
        case 192: return launch_p8_inst<3, 3>(g, st, n_cu);
        case 160: return launch_p8_inst<3, 2>(g, st, n_cu);
        case 128: return launch_p8_inst<2, 2>(g, st, n_cu);
        default: return launch_p8_inst<4, 4>(g, st, n_cu);
    }
}

// (the families and heights are reached by tests/test_gpu_dense.py and tests/test_gpu_mx_train.py, which assert their routes)
int yvgemm::launch_p9(GemmArgs& g, hipStream_t st, int rows, int n_cu, bool mx) {
    g.sched = g_opt_p8_sched;
    const bool f32out = g.flags & (YV_EPI_RES_F32 | YV_EPI_OUT_F32);
    const int ext = (g.flags & YV_EPI_SAVE_PRE) ? 1 : (g.flags & YV_EPI_GELU_BWD) ? 2 : 0;
    switch ((mx ? 4 : 0) + (ext ? ext : f32out ? 3 : 0)) {      // the family: a trainer epilogue (1 SAVE_PRE, 2 GELU_BWD) before f32out
        case 0: return launch_p9_rows<false, 0, false>(g, st, n_cu, rows);
        case 1: return launch_p9_rows<false, 1, false>(g, st, n_cu, rows);
        case 2: return launch_p9_rows<false, 2, false>(g, st, n_cu, rows);
        case 3: return launch_p9_rows<true, 0, false>(g, st, n_cu, rows);
        case 4: return launch_p9_rows<false, 0, true>(g, st, n_cu, rows);
        case 5: return launch_p9_rows<false, 1, true>(g, st, n_cu, rows);     // MX trainer: fc1 forward (GELU + saved pre-activation)
        case 6: return launch_p9_rows<false, 2, true>(g, st, n_cu, rows);     // MX trainer: fc2 data gradient (GELU backward)
        default: return launch_p9_rows<true, 0, true>(g, st, n_cu, rows);
    }
}
