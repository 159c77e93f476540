// The pipeline pieces that the fused split-bf16 FilterBlocks share (filter_mid.hip: 64 channels; filter_small.hip: 16 and 8; DESIGN.md
// 3.2b'): the per-column FiLM coordinate of the prologue, the epilogue of a column tile in five stages, and the host-side argument
// checks.  Parameters are what differs between the scales -- C, NFS (staged frames per channel), the
// channel groups a wave owns, the plane stride -- never which kernel is asking.  What stays with the kernels is theirs: tile ownership and
// address forms, swizzles, k-loops, chain gaps, tails -- and the FiLM staging loops and the store phase, which are the same text in
// both but whose listings change in every instantiation when they are called instead of written out (DESIGN.md 3.2b'); on the host,
// the frame bound and the FIRST / plain launch rule, which tests/test_host_filter_split.py restates file by file.
#pragma once
#include "conv_epilogue.h"

// The staged epilogue below needs the flags of filter_mid.hip (the reasons are at that file's guard and in csrc/Makefile) as much as
// the two sources do, so a third includer cannot drop them silently either.
#ifndef ALIVE_FILTER_MID_NO_SLP
#error "filter_pipeline.h: compile with -fno-slp-vectorize -DALIVE_FILTER_MID_NO_SLP -mllvm -amdgpu-sched-strategy=max-ilp (FLAGS_filter_mid in csrc/Makefile)"
#endif

// ---- prologue ----
// Xc entry of column t of the window: (8 * i0 relative to the staged frames, w1) -- the F.interpolate coordinates of the column (i1 = i0 + 1:
// the table repeats the window's last frame, which is what the clamp of upsample_linear1d reads there)
template <int NFP>
__device__ __forceinline__ uint2 film_column_coord(int t, int L, int t_off, float ratio, int Lf, int f_lo) {
    const int tc = t < 0 ? 0 : (t < L ? t : L - 1);
    const Lerp lp = lerp_coord(tc + t_off, ratio, Lf);
    int i0 = lp.i0 - f_lo;
    i0 = i0 < NFP - 1 ? i0 : NFP - 1;                        // NFP = FiLM frames a tile may span (i1 = i0 + 1 <= NFP, the last staged one)
    return make_uint2((unsigned)(i0 * 8), __float_as_uint(lp.w1));
}

// ---- the epilogue of one column tile (an "item"): v = chain result (+ residual, c2) -> GELU -> FiLM of the next conv's input ->
// re-split -> LDS planes, per channel group g (4 channels of a lane) in five stages of four independent chains each ----
// FiLM operands of one channel group of a column: (scale, shift) at frames i0 and i0 + 1
struct FilmG {
    f32x2 a0[4], a1[4];
};
struct Epi {
    int off;
    float w0, w1;
    FilmG F[2];
    float z[4], jt[4], je[4], jsc[4], jsh[4], jx[4];
};
// fsw: the lane's first channel in Fs; one ds_read2_b64 per element fetches both frames
template <int C, int NFS>
__device__ __forceinline__ void film_fetch(const unsigned char* fsw, int qf, int off, int g, FilmG& F) {
    const unsigned char* f = fsw + qf * (C * NFS * 8) + off;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const f32x2* fp = (const f32x2*)(f + ((8 * g + e) * NFS) * 8);
        F.a0[e] = fp[0];
        F.a1[e] = fp[1];
    }
}
// xc: the item's column in Xc
template <int C, int NFS>
__device__ __forceinline__ void epi_begin(Epi& E, const unsigned char* fsw, int qf, const uint2 xc) {
    E.off = (int)xc.x;
    E.w1 = __uint_as_float(xc.y);
    E.w0 = 1.0f - E.w1;
    film_fetch<C, NFS>(fsw, qf, E.off, 0, E.F[0]);
}
// Stage 0 of channel group g of G: every item runs it.  second: the item is a c2 result (v = chain + residual stream hrow, which it
// replaces); emit: a next conv exists (FiLM rows qf) and takes the modulated planes -- stages 1..3 (epi_stage13) and 4
// (epi_store_split or the kernel's own form) run for such items only.
// (the empty asm pins a stage's results to its own scheduling region: pure arithmetic otherwise sinks to its consumer's)
template <int C, int NFS, int G, class HRow>
__device__ __forceinline__ void epi_stage0(Epi& E, const unsigned char* fsw, bool second, bool emit, int qf, HRow& hrow, const f32x16& accv, int g) {
    if (emit && g + 1 < G) film_fetch<C, NFS>(fsw, qf, E.off, g + 1, E.F[(g + 1) & 1]);
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        float x = accv[4 * g + e];                 // one v_accvgpr_read per element (8 cycles beside an MFMA): kept for stage 3
        if (second) {
            x = x + hrow[4 * g + e];
            hrow[4 * g + e] = x;
        }
        E.jx[e] = x;
        E.jt[e] = __builtin_amdgcn_rcpf(fmaf(fabsf(x), 0.3275911f * 0.70710678118654752440f, 1.0f));
        const float xs = x * 0.84932180028801904272f;         // exp(-x^2 / 2) = exp2(-(x sqrt(log2(e) / 2))^2)
        E.je[e] = __builtin_amdgcn_exp2f(-(xs * xs));
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(E.jt[e]), "+v"(E.je[e]), "+v"(E.jx[e]));
}
__device__ __forceinline__ void epi_stage13(Epi& E, int g, int st) {
    const FilmG& Fg = E.F[g & 1];
    if (st == 1) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            E.jsc[e] = fmaf(E.w0, Fg.a0[e][0], E.w1 * Fg.a1[e][0]);        // fma(w0, a, round(w1 * b)): ATen's linear interp
            E.jsh[e] = fmaf(E.w0, Fg.a0[e][1], E.w1 * Fg.a1[e][1]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(E.jsc[e]), "+v"(E.jsh[e]));
    } else if (st == 2) {          // erf by Abramowitz-Stegun 7.1.26 (|err| <= 1.5e-7), like gelu_fast
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            float p = fmaf(1.061405429f, E.jt[e], -1.453152027f);
            p = fmaf(p, E.jt[e], 1.421413741f);
            p = fmaf(p, E.jt[e], -0.284496736f);
            p = fmaf(p, E.jt[e], 0.254829592f);
            E.jt[e] = p * E.jt[e];
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(E.jt[e]));
    } else if (st == 3) {          // x (1 + sign(x) erf|x / sqrt 2|) = x + |x| erf_abs = 2 gelu(x); jsc is half the FiLM scale
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float erf_abs = fmaf(-E.jt[e], E.je[e], 1.0f);
            E.z[e] = fmaf(fmaf(fabsf(E.jx[e]), erf_abs, E.jx[e]), E.jsc[e], E.jsh[e]);
        }
#pragma unroll
        for (int e = 0; e < 4; ++e) asm volatile("" : "+v"(E.z[e]));
    }
}
// stage 4 in the split form: the group's four values as hi and lo bf16 pairs, `plane` bytes apart
__device__ __forceinline__ void epi_store_split(const Epi& E, unsigned char* p, int plane) {
    const float* z = E.z;
    const unsigned h01 = pack_bf16x2(z[0], z[1]), h23 = pack_bf16x2(z[2], z[3]);
    const unsigned l01 = pack_bf16x2_lo(z[0], z[1], h01), l23 = pack_bf16x2_lo(z[2], z[3], h23);
    *(uint2*)p = make_uint2(h01, h23);
    *(uint2*)(p + plane) = make_uint2(l01, l23);
}

// ---- host side ----
// The checks every entry point of the two files makes; `who` is the entry point that was called, ptrs_ok its own list of required
// pointers, align_bits the OR of the addresses it needs 16-byte aligned and align_names how the message lists them.
static inline int filter_block_check_args(const char* who, bool ptrs_ok, const void* U, const void* out, int N, int L, int Lf,
                                          uintptr_t align_bits, const char* align_names, int film_ld, int t0, int f0) {
    ALIVE_CHECK_ARG(ptrs_ok, "%s: null pointer", who);
    ALIVE_CHECK_ARG(N > 0 && L > 16 && Lf > 0, "%s: bad sizes (L must exceed the largest reflect pad, 16)", who);
    ALIVE_CHECK_ARG(U != out, "%s: in-place not supported (tiles read a halo of their left neighbour)", who);
    ALIVE_CHECK_ARG((L & 3) == 0 && (align_bits & 15) == 0, "%s: L must be a multiple of 4 and %s 16-byte aligned", who, align_names);
    ALIVE_CHECK_ARG(film_ld > 0 && t0 >= 0 && f0 >= 0, "%s: bad frame range", who);
    return ALIVE_OK;
}
