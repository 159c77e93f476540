// Seam crossfade of the streaming paths (module/multistream.py: MultiStreamConverter(crossfade=True); module/realtime.py:
// crossfade_ms=): every tick re-decodes the whole ring and emits its centre span, so successive chunks come from two independent
// decodes.  The previous tick's wave went on beyond the span it emitted: its samples [span_lo + shift, span_lo + shift + X) are that
// tick's prediction of what this tick emits as [span_lo, span_lo + X).  alive_seam_rows keeps those X samples per row (`tail`) and
// fades from them into this tick's decode, in place on the final waves, after the output resample and before the gate's edge.
//   one block of 256 threads per row: thread tid owns i = tid, tid + 256, ... of the fade AND of the tail, so no sample is read by
//   one thread and written by another; the two regions of y are disjoint because X <= shift.
// The seam statistic (sum of squared differences, sum of squares of the unfaded head) is summed in fp64 in the gate's FIXED order --
// the strided partial sums, then a pairwise tree over the 256 of them -- so it is bitwise reproducible and the same for a row alone
// and inside any batch.  No floating-point atomics; every store is a plain vector store.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void seam_rows_kernel(float* __restrict__ y, int ld, const int* __restrict__ span_lo,
                                                        const int* __restrict__ shift, const int* __restrict__ xlen,
                                                        const unsigned char* __restrict__ emit, const float* __restrict__ g0,
                                                        const float* __restrict__ g1, float* __restrict__ tail, int ld_tail,
                                                        int* __restrict__ stored, double* __restrict__ stats) {
    __shared__ double acc_d[256];
    __shared__ double acc_e[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    if (emit[n] == 0) {                                     // (block-uniform) a filling or closed slot: y, tail and stored stay
        if (stats && tid == 0) {
            stats[2 * n] = 0.0;
            stats[2 * n + 1] = 0.0;
        }
        return;
    }
    const int lo = span_lo[n], sh = shift[n], X = xlen[n];
    const bool fits = lo >= 0 && X >= 0 && X <= ld_tail && X <= sh && (int64_t)lo + sh + X <= (int64_t)ld;
    if (X == 0 || !fits) {                                  // crossfade off for the row, or regions outside the row: y stays
        if (tid == 0) {
            stored[n] = 0;
            if (stats) {
                stats[2 * n] = 0.0;
                stats[2 * n + 1] = 0.0;
            }
        }
        return;
    }
    const int st = stored[n];
    const int Xe = st < X ? (st > 0 ? st : 0) : X;          // the fade covers only what the tail really holds (0 <= Xe <= X)
    __syncthreads();                                        // every thread has read stored[n] before thread 0 rewrites it
    float* yr = y + (size_t)n * ld;
    float* tr = tail + (size_t)n * ld_tail;
    const float den = (float)(Xe + 1);
    double d2 = 0.0, e2 = 0.0;
    for (int i = tid; i < Xe; i += 256) {
        const float t = tr[i], c = yr[lo + i];
        const double d = (double)c - (double)t, v = (double)c;
        d2 = d2 + d * d;
        e2 = e2 + v * v;
        const float w = (float)(i + 1) / den;
        yr[lo + i] = t + (c - t) * w;                       // (-ffp-contract=off: every operation rounded on its own)
    }
    for (int i = tid; i < X; i += 256) tr[i] = yr[lo + sh + i];       // the new tail: [lo + sh, lo + sh + X) is past [lo, lo + Xe)
    if (stats) {
        acc_d[tid] = d2;
        acc_e[tid] = e2;
        __syncthreads();
        for (int o = 128; o > 0; o >>= 1) {
            if (tid < o) {
                acc_d[tid] = acc_d[tid] + acc_d[tid + o];
                acc_e[tid] = acc_e[tid] + acc_e[tid + o];
            }
            __syncthreads();
        }
    }
    if (tid == 0) {
        if (stats) {
            stats[2 * n] = acc_d[0];
            stats[2 * n + 1] = acc_e[0];
        }
        // a tick whose search the gate skipped decoded the passed-through source: its tail must never be faded from
        stored[n] = (g0 && g0[n] == 0.0f && g1[n] == 0.0f) ? 0 : X;
    }
}

}  // namespace

extern "C" int alive_seam_rows(float* y, int N, int ld, const int* span_lo, const int* shift, const int* xlen,
                               const unsigned char* emit, const float* g0, const float* g1, float* tail, int ld_tail, int* stored,
                               double* stats, void* stream) {
    ALIVE_CHECK_ARG(y && span_lo && shift && xlen && emit && tail && stored, "alive_seam_rows: null pointer");
    ALIVE_CHECK_ARG((g0 == nullptr) == (g1 == nullptr), "alive_seam_rows: g0 and g1 go together");
    ALIVE_CHECK_ARG(N > 0 && ld > 0 && ld_tail > 0, "alive_seam_rows: bad args");
    seam_rows_kernel<<<N, 256, 0, (hipStream_t)stream>>>(y, ld, span_lo, shift, xlen, emit, g0, g1, tail, ld_tail, stored, stats);
    ALIVE_CHECK_LAUNCH("alive_seam_rows");
    return ALIVE_OK;
}
