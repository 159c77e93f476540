// FilterBlock.forward for the 16- and 8-channel scales of the decoder's U-Net (/root/reference/module/decoder.py:105-150),
// fused into ONE kernel per scale: input conv 1x1 + three FilterResBlocks (six GELU -> FiLM -> reflect-left causal k5 convs,
// dilations 1, 1, 2, 2, 4, 4) + the U-Net skip, per tile of 1024 (C = 16) / 2048 (C = 8) samples (56 of them the recomputed
// causal halo).  Conv by conv these scales (72 000 / 144 000 samples per window) are HBM-bound: ~14 tensor passes each.
//
// Round 4: rewritten on the design of the 64-channel block (filter_mid.hip, DESIGN.md 3.2b'), i.e. on the split-bf16 product
// (a*b ~= a_hi*b_hi + a_hi*b_lo + a_lo*b_hi, fp32 accumulate, ~2^-16 per product) of v_mfma_f32_32x32x16_bf16 instead of the exact
// f32 MFMA 16x16x4 of rounds 1-3: that kernel spent 2.5 matrix-pipe cycles and ~25 serialised vector instructions per output element
// (16.4 ms per step for the two scales, pipe 0.35-0.41 busy, two waves per SIMD taking turns on one issue port); the three-product
// bf16 form needs 0.6 pipe cycles per element and leaves the epilogue as the bound, which is then hidden as in filter_mid.hip:
//   * activations live in LDS as two bf16 planes [column][C channels] (32 / 16 B rows), two buffers; output channels are padded
//     to the MFMA's 32 rows (rows >= C have zero weights and are never read back), K = 5 C: one tap per k-step at C = 16, two taps
//     per k-step at C = 8 (the lane halves lh = 0 / 1 read different taps; the sixth tap of the last k-step has zero weights);
//   * a block is 4 waves, one per SIMD; wave w owns column tiles w, w + 4, w + 8, ... of 32 columns (8 / 16 tiles); its A fragments
//     (40 / 24 registers per conv) and the residual stream of its tiles (64 registers) stay in registers;
//   * ONE software pipeline over (conv, tile) steps: a step runs the tile's 15 / 9 MFMAs and, beside them, the epilogue of the
//     previous step's tile in stages of four independent dependency chains (GELU -> FiLM -> re-split -> LDS); the interleaved tile
//     ownership lets it run across conv boundaries, with ONE barrier per half conv (tile t of conv q + 1 needs tiles t - 1, t of
//     conv q, which were written at least NT / 2 steps earlier);
//   * C = 16: the two 16-byte halves of a row are swapped by (column >> 3) & 1, which makes the 32-lane fragment reads conflict-free.
// Parity: the block's outputs move from "bit for bit an fp32 fmaf chain" to the split-bf16 error of the 64- and 256-channel scales
// (unit tests: 4e-5 relative instead of 5e-6; the decoder fixtures' waveform RMS error is unchanged at 1.1e-4, bar 1e-3).
#include <type_traits>
#include <stdlib.h>

#ifndef ALIVE_FILTER_MID_NO_SLP
#error "filter_small.hip must be compiled with the flags of filter_mid.hip: -fno-slp-vectorize -DALIVE_FILTER_MID_NO_SLP -mllvm -amdgpu-sched-strategy=max-ilp (see csrc/Makefile)"
#endif
#include "filter_pipeline.h"           // the pieces shared with filter_mid.hip

static long long* g_stamps_small = nullptr;
extern "C" void alive_debug_set_stamps_small(long long* p) { g_stamps_small = p; }

namespace {

constexpr int HALO = 56;                // causal reach of the six k5 convs: 4 (1 + 1 + 2 + 2 + 4 + 4)
constexpr int NCONV = 6;
// What the store phase emits -- a compile-time choice, so that the plain instantiations keep their registers, LDS and code:
//   TAIL_NONE  the block's output (+ U-Net skip) [C][L];
//   TAIL_UP    C = 16: the ConvTranspose1d(16, 8, 2, 2) behind the block (ups[3]) applied to the finished tile, [8][2 L] -- the
//              16-channel tensor is never written.  The sums are conv_gemm_kernel's chains term for term (conv.hip: the f32 MFMA
//              16x16x4 is a fmaf chain from the bias in which step s of lane group q takes k = 4 q + s);
//   TAIL_WAVE  C = 8: source_out Conv1d(8, 1, 7, pad 3) applied to the finished tile, [L] -- source_out_kernel's fmaf chain in
//              (ci, m) order from b[0], zeros outside [0, L).  The conv is not causal, so a tile recomputes 8 more columns on its left
//              (HALO 64: h valid on [t0 - 8, t0 + TT)) and emits the samples [t0 - 3, t0 + TT - 3); the tile that holds column L - 1
//              emits the window's last three as well.
constexpr int TAIL_NONE = 0, TAIL_UP = 1, TAIL_WAVE = 2;
constexpr int NFP = 10;                 // FiLM frames a tile may span (1024 columns at 160 per frame = 6.4, + 3 of slack)
constexpr int NFS = NFP + 1;            // staged frames per channel (i0 <= NFP - 1, i1 = i0 + 1)
constexpr int PLANE_BATCH = 32768;      // bytes per plane of the batch tiles: BL * ROWB in both configurations

// PL = bytes per plane.  The batch path runs 32-KB planes (1024 / 2048 columns per tile: the 56-column halo is 3 - 5 % of the work);
// a signal of a few thousand samples (the streaming step: 1600 / 3200) would be TWO such tiles on two CUs, each walking 8 / 16
// column tiles per wave and conv -- 50 us of a 0.9-ms step.  There the planes are 8 KB (256 / 512 columns, 2 / 4 column tiles per
// wave): 8 blocks, a quarter of the chain each.
template <int C, int PL = PLANE_BATCH, int TAIL = TAIL_NONE>
struct Cfg {
    static constexpr int HL = TAIL == TAIL_WAVE ? HALO + 8 : HALO;      // recomputed columns on a tile's left
    static constexpr int PLANE = PL;
    static constexpr int BUF = 2 * PL;                  // hi + lo
    static constexpr int ROWB = 2 * C;                  // bytes per LDS row
    static constexpr int BL = PLANE / ROWB;             // columns per tile incl. halo (batch: 1024 / 2048)
    static constexpr int TT = BL - HL;                  // output columns per tile
    static constexpr int NT = BL / 128;                 // column tiles of 32 per wave (8 / 16)
    static constexpr int TSTEP = 128 * ROWB;            // a wave's consecutive tiles are four column tiles apart
    static constexpr int G = C / 8;                     // channel groups of 8 (rows 8 g + 4 lh + e) that hold real channels
    static constexpr int KS = C == 16 ? 5 : 3;          // k-steps of a k5 conv (K = 5 C, padded to 48 at C = 8)
    static constexpr int KP = 16 * KS;                  // padded K
    static constexpr int GUARD = 16 * ROWB;             // rows left of the image the leftmost tile may read
    static constexpr int W_IN = 2 * 32 * 16;            // bf16 elements of the input conv [2 planes][32 rows][16]
    static constexpr int W_K5 = 2 * 32 * KP;            // of a k5 conv [2][32][KP]
    static constexpr int WFLOATS = 7 * 32 + (W_IN + NCONV * W_K5) / 2;       // fp32 biases [7][32], then the bf16 weights
    static constexpr int LDS = GUARD + 2 * BUF + NCONV * C * NFS * 8 + BL * 8;
};

// tw / tb: weights and bias of the conv a TAIL applies (TAIL_UP: [16 rows (co, j)][16] and [16]; TAIL_WAVE: [8][7] and [1])
template <int C, bool FIRST, int PL = PLANE_BATCH, int TAIL = TAIL_NONE>
__global__ __launch_bounds__(256, PL == 16384 ? 2 : 1) void filter_block_small_kernel(const float* __restrict__ U, int L, const float* __restrict__ wpack,
                                                                   const float* __restrict__ film, int film_rows, int Lf, int film_off,
                                                                   float ratio, int t_off, int f_off, int film_ld,
                                                                   const float* __restrict__ skip, float* __restrict__ out, long long* stamps,
                                                                   const float* __restrict__ tw, const float* __restrict__ tb) {
    static_assert(TAIL == TAIL_NONE || (TAIL == TAIL_UP && C == 16) || (TAIL == TAIL_WAVE && C == 8), "TAIL_UP is ups[3], TAIL_WAVE source_out");
    using K = Cfg<C, PL, TAIL>;
    constexpr int HALO = K::HL;
    constexpr int PLANE = K::PLANE, BUF = K::BUF;
#ifdef ALIVE_STAMPS                 // diagnostic build only (tools/ab_build.sh x.so filter_small.hip -DALIVE_STAMPS; tools/stamp_fbs.py)
    long long tsx[12];
    int nts = 0;
#define STAMPS() tsx[nts++] = wall_clock64()
#else
#define STAMPS()
#endif
    STAMPS();
    constexpr int ROWB = K::ROWB, BL = K::BL, TT = K::TT, NT = K::NT, TSTEP = K::TSTEP, G = K::G, KS = K::KS, KP = K::KP;
    extern __shared__ __attribute__((aligned(16))) unsigned char sm[];
    unsigned char* bufZ = sm + K::GUARD;
    unsigned char* bufY = bufZ + BUF;
    f32x2* Fs = (f32x2*)(bufZ + 2 * BUF);             // [NCONV][C][NFS] (scale / 2, shift)
    uint2* Xc = (uint2*)(Fs + NCONV * C * NFS);       // [BL] per column: (8 * i0 relative to the staged frames, w1)

    const int tid = threadIdx.x, lane = tid & 63;
    const int w = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n32 = lane & 31, lh = lane >> 5;
    const int n = blockIdx.y;
    const int t0 = FIRST ? blockIdx.x * TT : (blockIdx.x + 1) * TT;
    const int tbase = t0 - HALO;
    const float* Un = U + (size_t)n * C * L;
    const float* biases = wpack;                                              // [7][32]
    const unsigned short* W16 = (const unsigned short*)(wpack + 7 * 32);

    // swap of the two 16-byte halves of a 32-byte row (C = 16): (column >> 3) & 1
    auto hsw = [](int r) { return C == 16 ? (r >> 3) & 1 : 0; };

    // ---- prologue: raw input tile -> planes, FiLM rows, interpolation coordinates; every global load before the first LDS write ----
    const int f_lo = lerp_coord((tbase < 0 ? 0 : tbase) + t_off, ratio, Lf).i0;     // frames of the WINDOW (t_off: range mode)
    {
        constexpr int NCOL = BL / 256;                        // columns per thread: tid, tid + 256, ...
        float v[NCOL][C];
#pragma unroll
        for (int j = 0; j < NCOL; ++j) {
            const int t = tbase + tid + 256 * j;
            const bool ok = t >= 0 && t < L;
            const float* uc = Un + (ok ? t : 0);
#pragma unroll
            for (int c = 0; c < C; ++c) v[j][c] = ok ? uc[(size_t)c * L] : 0.0f;
        }
        constexpr int NFT = NCONV * 2 * C * NFS;              // FiLM values of the tile
        constexpr int NFL = (NFT + 255) / 256;
        float fv[NFL];
#pragma unroll
        for (int k = 0; k < NFL; ++k) {
            const int e = tid + 256 * k;
            const int f = e % NFS, c = (e / NFS) % C, sel = (e / (NFS * C)) & 1, q = e / (NFS * C * 2);
            int fr = f_lo + f;
            fr = fr < Lf ? fr : Lf - 1;
            int fc = fr - f_off;                             // frame of the window -> column of the film tensor
            fc = fc < 0 ? 0 : (fc < film_ld ? fc : film_ld - 1);
            fv[k] = e < NFT ? film[((size_t)n * film_rows + film_off + q * 2 * C + sel * C + c) * film_ld + fc] : 0.0f;
        }
#pragma unroll
        for (int j = 0; j < NCOL; ++j) {
            const int col = tid + 256 * j;
            Xc[col] = film_column_coord<NFP>(tbase + col, L, t_off, ratio, Lf, f_lo);
#pragma unroll
            for (int ck = 0; ck < C / 8; ++ck) {
                u32x4 hi, lo;
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const float x0 = v[j][ck * 8 + 2 * e], x1 = v[j][ck * 8 + 2 * e + 1];
                    hi[e] = pack_bf16x2(x0, x1);
                    lo[e] = pack_bf16x2_lo(x0, x1, hi[e]);
                }
                unsigned char* dst = bufZ + col * ROWB + ((ck ^ hsw(col)) << 4);
                *(u32x4*)dst = hi;
                *(u32x4*)(dst + PLANE) = lo;
            }
        }
#pragma unroll
        for (int k = 0; k < NFL; ++k) {
            const int e = tid + 256 * k;
            const int f = e % NFS, c = (e / NFS) % C, sel = (e / (NFS * C)) & 1, q = e / (NFS * C * 2);
            // the scale rows are stored halved (exact): gelu(x) * sc + sh = (x + |x| erf|x / sqrt 2|) * (sc / 2) + sh
            if (e < NFT) ((float*)Fs)[((q * C + c) * NFS + f) * 2 + sel] = sel == 0 ? 0.5f * fv[k] : fv[k];
        }
    }
    __syncthreads();
    STAMPS();

    // residual stream of the wave's tiles: h[i][4 g + e] = channel 8 g + 4 lh + e of column 32 (4 i + w) + n32 (MFMA C layout)
    float h[NT][4 * G];
    const int colw = 32 * w + n32;                                                 // column of tile i: colw + 128 i
    int st_off[G];                                                                 // modulated planes: channels 8 g + 4 lh .. +3
#pragma unroll
    for (int g = 0; g < G; ++g) st_off[g] = colw * ROWB + ((g ^ hsw(colw)) << 4) + 8 * lh;
    const uint2* xcw = Xc + colw;
    const unsigned char* fsw = (const unsigned char*)(Fs + 4 * lh * NFS);

    // the epilogue of a column tile in stages (filter_pipeline.h); here: this wave's FiLM rows, Xc column, residual row and planes
    auto epi_begin = [&](Epi& E, int qf, int t) { ::epi_begin<C, NFS>(E, fsw, qf, xcw[128 * t]); };
    auto epi_stage = [&](Epi& E, bool second, bool emit, int qf, unsigned char* dstp, int t, const f32x16& accv, int g, int st) {
        if (st == 0) epi_stage0<C, NFS, G>(E, fsw, second, emit, qf, h[t], accv, g);
        else if (!emit) return;
        else if (st < 4) epi_stage13(E, g, st);
        else epi_store_split(E, dstp + st_off[g] + t * TSTEP, PLANE);
    };

    // weights of the k5 convs: k-step s covers k = 16 s .. 16 s + 15 (k = tap * C + ci), lane half lh the second eight of them
    bf16x8 a[KS][2];
    auto load_weights = [&](int q) {
        const unsigned short* Wq = W16 + K::W_IN + (size_t)q * K::W_K5 + (size_t)n32 * KP + 8 * lh;
#pragma unroll
        for (int s = 0; s < KS; ++s)
#pragma unroll
            for (int pl = 0; pl < 2; ++pl) a[s][pl] = *(const bf16x8*)(Wq + (size_t)pl * 32 * KP + s * 16);
    };

    f32x16 acc[2];
    // 16-KB planes (two blocks per CU, 256 registers per wave): ONE epilogue record, filled at the top of its step -- the two dependent LDS
    // latencies that the prefetch one step ahead hides in the one-block form are covered by the co-resident block's wave here, and the
    // second record's ~60 registers are what the 16-channel scale spilled
    constexpr bool ONE_EPI = PL == 16384;
    Epi EP[ONE_EPI ? 1 : 2];
    // ---- input_conv (1x1, one k-step): h = Win * U + b ----
    {
        bf16x8 ai[2];
#pragma unroll
        for (int pl = 0; pl < 2; ++pl) ai[pl] = *(const bf16x8*)(W16 + (size_t)pl * 32 * 16 + (size_t)n32 * 16 + 8 * lh);
        f32x16 b16;
#pragma unroll
        for (int r = 0; r < 16; ++r) b16[r] = biases[8 * (r >> 2) + 4 * lh + (r & 3)];
        // C = 16: channels 8 lh .. of the column; C = 8: the column's eight channels for both halves (the upper half's weights are zero)
        const int bw = colw * ROWB + (C == 16 ? ((lh ^ hsw(colw)) << 4) : 0);
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const unsigned char* bp = bufZ + bw + i * TSTEP;
            const bf16x8 bh = *(const bf16x8*)bp, bl = *(const bf16x8*)(bp + PLANE);
#ifndef ALIVE_FBS_NO_CHAIN_GAP
            if (i > 0) ALIVE_CHAIN_GAP(7);                    // (hipcc may read the previous tile's result behind this tile's MFMAs)
#endif
            f32x16 c = b16;
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ai[1], bh, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ai[0], bl, c, 0, 0, 0);
            c = __builtin_amdgcn_mfma_f32_32x32x16_bf16(ai[0], bh, c, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4 * G; ++r) h[i][r] = c[r];
        }
    }
    __syncthreads();                       // every wave has read the raw columns
    load_weights(0);
    // z0 = mod_0(h) over the raw columns: all tiles but the last here, the last one under the first MFMAs of conv 0 as a "c2 item"
    // whose chain result is zero (v = 0 + h)
    {
        f32x16 zero16;
#pragma unroll
        for (int r = 0; r < 16; ++r) zero16[r] = 0.0f;
        acc[1] = zero16;
#pragma unroll
        for (int i = 0; i < NT - 1; ++i) {
            Epi E;
            epi_begin(E, 0, i);
#pragma unroll
            for (int g = 0; g < G; ++g)
#pragma unroll
                for (int st = 0; st < 5; ++st) epi_stage(E, true, true, 0, bufZ, i, zero16, g, st);
        }
    }
    __syncthreads();
    STAMPS();
    if (!ONE_EPI) epi_begin(EP[0], 0, NT - 1);           // the pending item of the first step

    // ---- three FilterResBlocks: q = 2 j (c1), 2 j + 1 (c2), dilation 2^j    (decoder.py:128-134) ----
    // SECOND: the c2 of its block (adds into the residual stream); EMIT: a next conv exists and takes the modulated output -- a
    // compile-time flag: tested at run time it puts a branch into every k-step region of the c2 bodies (+1.5 .. 2.5 us per conv)
    auto conv = [&](auto second_tag, auto emit_tag, const int q) {
        constexpr bool SECOND = decltype(second_tag)::value;
        constexpr bool emit = decltype(emit_tag)::value;
        const unsigned char* in = SECOND ? bufY : bufZ;
        unsigned char* dst = SECOND ? bufZ : bufY;
        f32x16 b16;
#pragma unroll
        for (int r = 0; r < 16; ++r) b16[r] = biases[(1 + q) * 32 + 8 * (r >> 2) + 4 * lh + (r & 3)];
        const int d = 1 << (q >> 1);
        // B fragment of k-step s of tile i.  C = 16: tap s, channels 8 lh ..: row r = colw + 128 i + (s - 4) d, 16 B at
        // r * 32 + ((lh ^ hsw(r)) << 4).  C = 8: tap 2 s + lh (the phantom sixth tap reads the fifth's row; its weights are zero): the
        // whole 16-byte row r = colw + 128 i + (tap - 4) d.  hsw does not depend on i: base[s] + i * TSTEP.
        auto tap_of = [&](int s) { return C == 16 ? s : (2 * s + lh < 5 ? 2 * s + lh : 4); };
        int base[KS];
#pragma unroll
        for (int s = 0; s < KS; ++s) {
            const int r0 = colw + (tap_of(s) - 4) * d;          // >= -16: the guard
            base[s] = r0 * ROWB + (C == 16 ? ((lh ^ hsw(r0)) << 4) : 0);
        }
        auto frag_off = [&](int i, int s) -> int {
            if (FIRST) {                                        // reflect at t = 0 (column HALO of this tile), per lane
                int ta = tbase + colw + 128 * i + (tap_of(s) - 4) * d;
                ta = ta < 0 ? -ta : ta;
                int r = ta - tbase;
                r = r < BL ? r : BL - 1;
                return r * ROWB + (C == 16 ? ((lh ^ hsw(r)) << 4) : 0);
            }
            return base[s] + i * TSTEP;
        };
        constexpr int NJ = 5 * G;                               // stage jobs of an item, spread over the KS k-step regions
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            // the item of this step: tile i - 1 of this conv, or (i == 0) the last tile of the previous conv -- the other type, which
            // always has a next conv, whose FiLM rows are this conv's and whose planes are this conv's input
            const bool it_second = i > 0 ? SECOND : !SECOND;
            const bool it_emit = i > 0 ? emit : true;
            const int it_qf = i > 0 ? q + 1 : q;
            unsigned char* it_dst = i > 0 ? dst : (unsigned char*)in;
            const int it_t = i > 0 ? i - 1 : NT - 1;
            const f32x16& it_acc = acc[(i + 1) & 1];
#ifndef ALIVE_FBS_NO_CHAIN_GAP
            ALIVE_CHAIN_GAP(7);                               // distance between two accumulation chains (filter_mid.hip, DESIGN.md 3.2b')
#endif
            // the item's coordinates and first FiLM group were requested one step ago (two dependent LDS latencies that nothing
            // in a 9- or 15-MFMA step could cover); now the same for the next step's item, which is always tile i of this conv
            Epi& E = EP[ONE_EPI ? 0 : (i & 1)];
            if (ONE_EPI) { if (it_emit) epi_begin(E, it_qf, it_t); }
            else if (emit) epi_begin(EP[(i + 1) & 1], q + 1, i);
            acc[i & 1] = b16;
            bf16x8 fh[KS], fl[KS];
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                const unsigned char* bp = in + frag_off(i, s);
                fh[s] = *(const bf16x8*)bp;
                fl[s] = *(const bf16x8*)(bp + PLANE);
            }
#pragma unroll
            for (int s = 0; s < KS; ++s) {
                acc[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][1], fh[s], acc[i & 1], 0, 0, 0);
                acc[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][0], fl[s], acc[i & 1], 0, 0, 0);
                acc[i & 1] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[s][0], fh[s], acc[i & 1], 0, 0, 0);
#pragma unroll
                for (int j = s * NJ / KS; j < (s + 1) * NJ / KS; ++j) epi_stage(E, it_second, it_emit, it_qf, it_dst, it_t, it_acc, j / 5, j % 5);
                __builtin_amdgcn_sched_barrier(0);           // one scheduling region per k-step
            }
            if (i == NT - 1 && emit) load_weights(q + 1);    // the A registers are free: the next conv's weights travel under its first steps' wait
            if (i == NT / 2 - 1 || i == NT - 1) __syncthreads();      // what the next half conv reads was written >= NT / 2 steps ago
        }
    };
#pragma unroll 1
    for (int j = 0; j < 3; ++j) {
        conv(std::false_type{}, std::true_type{}, 2 * j);
        STAMPS();
        if (j < 2) conv(std::true_type{}, std::true_type{}, 2 * j + 1);
        else conv(std::true_type{}, std::false_type{}, 2 * j + 1);
        STAMPS();
    }
    // drain: the last conv's last tile only adds into the residual stream
#pragma unroll
    for (int r = 0; r < 4 * G; ++r) h[NT - 1][r] = acc[1][r] + h[NT - 1][r];

    // ---- store the tile (+ U-Net skip, decoder.py:191): through LDS so that global accesses are 16-B vectors along t ----
    float* Ht = (float*)bufZ;                         // [C][BL + 4] fp32 over bufZ / bufY
    constexpr int HP = BL + 4;
#pragma unroll
    for (int i = 0; i < NT; ++i)
#pragma unroll
        for (int g = 0; g < G; ++g)
#pragma unroll
            for (int e = 0; e < 4; ++e) Ht[(8 * g + 4 * lh + e) * HP + colw + 128 * i] = h[i][4 * g + e];
    if constexpr (TAIL == TAIL_UP) {
        // U8[co][2 t + j] = chain of row (co, j) over x = h + skip of column t; a lane takes a column, a wave's store is one 512-byte run
        __syncthreads();
#pragma unroll 1
        for (int c = tid; c < TT; c += 256) {
            const int t = t0 + c;
            if (t >= L) break;
            float x[C];
#pragma unroll
            for (int ci = 0; ci < C; ++ci)
                x[ci] = Ht[ci * HP + HALO + c] + (skip != nullptr ? skip[((size_t)n * C + ci) * L + t] : 0.0f);
            float* o = out + (size_t)n * (C / 2) * 2 * L + 2 * (size_t)t;
#pragma unroll
            for (int co = 0; co < C / 2; ++co) {
                f32x2 v;
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int row = 2 * co + j;
                    float a = tb[row];
#pragma unroll
                    for (int s = 0; s < 4; ++s)
#pragma unroll
                        for (int q = 0; q < 4; ++q) a = fmaf(tw[row * 16 + 4 * q + s], x[4 * q + s], a);
                    v[j] = a;
                }
                *(f32x2*)(o + (size_t)co * 2 * L) = v;
            }
        }
        return;
    }
    if constexpr (TAIL == TAIL_WAVE) {
        __syncthreads();
        const int lo = t0 - 3 < 0 ? 0 : t0 - 3;
        const int hi = t0 + TT >= L ? L : t0 + TT - 3;
#pragma unroll 1
        for (int t = lo + tid; t < hi; t += 256) {
            float a = tb[0];
#pragma unroll
            for (int ci = 0; ci < C; ++ci)
#pragma unroll
                for (int m = 0; m < 7; ++m) {
                    const int ti = t + m - 3;                          // column ti - tbase of the tile: 58 .. BL + 2 < HP
                    const float hv = Ht[ci * HP + (ti - tbase)];
                    a = fmaf(tw[ci * 7 + m], (ti >= 0 && ti < L) ? hv : 0.0f, a);
                }
            out[(size_t)n * L + t] = a;
        }
        return;
    }
    // (the skip loads of the whole tile are in flight together; prefetching them under the last conv spills: 64 more registers)
    constexpr int NV = (C * (TT / 4) + 255) / 256;          // vectors of 4 output columns per thread
    f32x4 sk[NV];
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int g = tid + 256 * u;
        const int co = g / (TT / 4), c4 = (g - co * (TT / 4)) * 4;
        const int t = t0 + c4;
        sk[u] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        if (skip != nullptr && g < C * (TT / 4) && t + 3 < L) sk[u] = *(const f32x4*)(skip + ((size_t)n * C + co) * L + t);
    }
    __syncthreads();
#pragma unroll
    for (int u = 0; u < NV; ++u) {
        const int g = tid + 256 * u;
        const int co = g / (TT / 4), c4 = (g - co * (TT / 4)) * 4;
        const int t = t0 + c4;
        if (g >= C * (TT / 4) || t >= L) continue;
        const size_t o = ((size_t)n * C + co) * L + t;
        const f32x4 v = *(const f32x4*)&Ht[co * HP + HALO + c4];
        if (t + 3 < L) {
            *(f32x4*)(out + o) = v + sk[u];
        } else {
            for (int e = 0; e < 4 && t + e < L; ++e) out[o + e] = v[e] + (skip != nullptr ? skip[o + e] : 0.0f);
        }
    }
#ifdef ALIVE_STAMPS
    if (stamps != nullptr && tid == 0 && !FIRST) {
        long long* o = stamps + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * 16;
        for (int i = 0; i + 1 < nts; ++i) o[i] = tsx[i + 1] - tsx[i];
        o[nts - 1] = wall_clock64() - tsx[nts - 1];
    }
#endif
}

template <int C, int PL, int TAIL = TAIL_NONE>
int launch_small(const float* U, int N, int L, const float* wpack, const float* film, int film_rows, int Lf, int film_off,
                 int t0, int f0, int film_ld, const float* skip, float* out, hipStream_t s, const float* tw = nullptr, const float* tb = nullptr) {
    using K = Cfg<C, PL, TAIL>;
    {
        static LdsOptIn optin;                               // one per instantiation <C, PL>
        hipError_t e = optin.ensure({(const void*)filter_block_small_kernel<C, false, PL, TAIL>, (const void*)filter_block_small_kernel<C, true, PL, TAIL>},
                                    K::LDS);
        if (e != hipSuccess) {
            alive_set_error("alive_filter_block_small: cannot reserve %d B of LDS: %s", K::LDS, hipGetErrorString(e));
            return ALIVE_ERR_LAUNCH;
        }
    }
    const float ratio = (float)film_ld / (float)L;       // == window frames / window samples at this rate
    ALIVE_CHECK_ARG((double)K::BL * film_ld / L + 3.0 <= NFP, "alive_filter_block_small: tile spans more than %d frames (L %d, frames %d)", NFP, L, film_ld);
    const int tiles = cdiv(L, K::TT);
    // the first tile of a window reflects at t = 0 (per-lane fragment addresses); a problem that does not fill the chip runs all its
    // tiles through that form in one launch (filter_mid.hip)
    const bool small = (int64_t)tiles * N <= 256;
    filter_block_small_kernel<C, true, PL, TAIL><<<dim3(small ? tiles : 1, N), 256, K::LDS, s>>>(U, L, wpack, film, film_rows, Lf, film_off, ratio,
                                                                                           t0, f0, film_ld, skip, out, g_stamps_small, tw, tb);
    if (tiles > 1 && !small)
        filter_block_small_kernel<C, false, PL, TAIL><<<dim3(tiles - 1, N), 256, K::LDS, s>>>(U, L, wpack, film, film_rows, Lf, film_off, ratio, t0,
                                                                                        f0, film_ld, skip, out, g_stamps_small, tw, tb);
    ALIVE_CHECK_LAUNCH("alive_filter_block_small");
    return ALIVE_OK;
}

}  // namespace

extern "C" int alive_filter_block_small_weights(int C) {
    return C == 8 ? Cfg<8>::WFLOATS : (C == 16 ? Cfg<16>::WFLOATS : -1);
}

extern "C" int alive_filter_block_small(const float* U, int N, int C, int L, const float* wpack, const float* film,
                                        int film_rows, int Lf, int film_off, const float* skip, float* out, void* stream) {
    return alive_filter_block_small_range(U, N, C, L, wpack, film, film_rows, Lf, film_off, 0, 0, Lf, skip, out, stream);
}

extern "C" int alive_filter_block_small_range(const float* U, int N, int C, int L, const float* wpack, const float* film,
                                              int film_rows, int Lf, int film_off, int t0, int f0, int film_ld,
                                              const float* skip, float* out, void* stream) {
    // (C keeps its place in the order of the checks -- third, behind null pointers and sizes, which the helper reports before
    //  anything else: a call that is wrong in several arguments hears the same message as before)
    ALIVE_CHECK_ARG(!(U && wpack && film && out && N > 0 && L > 16 && Lf > 0) || C == 8 || C == 16, "alive_filter_block_small: C must be 8 or 16, got %d", C);
    if (int rc = filter_block_check_args("alive_filter_block_small", U && wpack && film && out, U, out, N, L, Lf,
                                         (uintptr_t)U | (uintptr_t)out | (uintptr_t)skip | (uintptr_t)wpack, "U / out / skip / wpack", film_ld, t0, f0))
        return rc;
    // a signal that would be a handful of batch tiles runs on 8-KB planes (see Cfg)
    static const int pl_env = getenv("ALIVE_FBS_PLANE") ? atoi(getenv("ALIVE_FBS_PLANE")) : 0;
    const int big_tiles = cdiv(L, (C == 8 ? Cfg<8>::TT : Cfg<16>::TT)) * N;
    const bool tiny = pl_env ? pl_env < 16384 : big_tiles <= 16;
    hipStream_t s = (hipStream_t)stream;
    // 16-KB planes (round 5, the batch default): 77 KB of LDS per block and 256 registers per wave = TWO blocks per CU, one block's
    // prologue / store under the other's convs, for 3 % (C = 8) / 6 % (C = 16) more halo work.  Measured per 64 windows: C = 8 1.03 ->
    // 0.96 ms, C = 16 1.03 -> 0.95 ms (with ONE epilogue record: with two it needs 284+ registers, spills 40 - 68 and runs 1.10 ms).
    // ALIVE_FBS_PLANE=32768 forces the one-block form.  Same bits either way (tools/run_fused_once.py digests).
    if (!tiny && (pl_env == 16384 || pl_env == 0)) {
        if (C == 8) return launch_small<8, 16384>(U, N, L, wpack, film, film_rows, Lf, film_off, t0, f0, film_ld, skip, out, s);
        return launch_small<16, 16384>(U, N, L, wpack, film, film_rows, Lf, film_off, t0, f0, film_ld, skip, out, s);
    }
    if (C == 8) return tiny ? launch_small<8, 8192>(U, N, L, wpack, film, film_rows, Lf, film_off, t0, f0, film_ld, skip, out, s)
                            : launch_small<8, PLANE_BATCH>(U, N, L, wpack, film, film_rows, Lf, film_off, t0, f0, film_ld, skip, out, s);
    return tiny ? launch_small<16, 8192>(U, N, L, wpack, film, film_rows, Lf, film_off, t0, f0, film_ld, skip, out, s)
                : launch_small<16, PLANE_BATCH>(U, N, L, wpack, film, film_rows, Lf, film_off, t0, f0, film_ld, skip, out, s);
}

// ---- the block with the small conv behind it folded into its store phase (TAIL_UP / TAIL_WAVE): the batch route of the decoder ----
// Always the 16-KB-plane tiles (two blocks per CU); a column's value does not depend on the tile form.
extern "C" int alive_filter_block_small_up_range(const float* U, int N, int L, const float* wpack, const float* film, int film_rows, int Lf,
                                                 int film_off, int t0, int f0, int film_ld, const float* skip, const float* upW,
                                                 const float* upb, float* out, void* stream) {
    if (int rc = filter_block_check_args("alive_filter_block_small_up", U && wpack && film && upW && upb && out, U, out, N, L, Lf,
                                         (uintptr_t)U | (uintptr_t)out | (uintptr_t)skip | (uintptr_t)wpack, "U / out / skip / wpack", film_ld, t0, f0))
        return rc;
    return launch_small<16, 16384, TAIL_UP>(U, N, L, wpack, film, film_rows, Lf, film_off, t0, f0, film_ld, skip, out, (hipStream_t)stream, upW, upb);
}

extern "C" int alive_filter_block_small_wave_range(const float* U, int N, int L, const float* wpack, const float* film, int film_rows, int Lf,
                                                   int film_off, int t0, int f0, int film_ld, const float* oW, const float* ob, float* wave,
                                                   void* stream) {
    if (int rc = filter_block_check_args("alive_filter_block_small_wave", U && wpack && film && oW && ob && wave, U, wave, N, L, Lf,
                                         (uintptr_t)U | (uintptr_t)wpack, "U / wpack", film_ld, t0, f0))
        return rc;
    return launch_small<8, 16384, TAIL_WAVE>(U, N, L, wpack, film, film_rows, Lf, film_off, t0, f0, film_ld, nullptr, wave, (hipStream_t)stream, oW, ob);
}
