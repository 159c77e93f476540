// Input gate of the streaming paths (module/multistream.py: MultiStreamConverter(gate=True); module/realtime.py: gate_db=): which rows
// hear something this tick, decided on the device inside the captured step, and an output edge that fades instead of clicking.
//   the decision, one block per row          alive_gate_rows         (after the input resample and gain, before the spectrogram)
//   the output edge, in place on the waves   alive_gate_apply_rows   (after the output resample)
// The level of a row is the mean square of its 16 kHz ring over the detection window [w_lo, w_hi), summed in fp64 in a FIXED order --
// thread tid takes samples w_lo + tid, + 256, ..., then a pairwise tree over the 256 partial sums, as world_f0.hip's mean kernel -- so
// it is bitwise reproducible and the same for a row alone and inside any batch.  A square of a float32 is exact in fp64.  The state
// machine (hold, the two gains of the chunk's ends, the row masks of the search, WORLD and the auto-pitch follower) is integer work of
// thread 0.  No floating-point atomics; every store is a plain vector store.
#include "common.h"

namespace {

__global__ __launch_bounds__(256) void gate_rows_kernel(const float* __restrict__ x, int ld, int w_lo, int w_hi,
                                                        const int* __restrict__ gate_on, const double* __restrict__ thr_ms,
                                                        const int* __restrict__ hold_ticks, const unsigned char* __restrict__ emit,
                                                        const int* __restrict__ world_on, int S, const int* __restrict__ seg_len,
                                                        int* __restrict__ state, float* __restrict__ g0, float* __restrict__ g1,
                                                        int* __restrict__ seg_len_eff, unsigned char* __restrict__ follow,
                                                        int* __restrict__ world_eff, double* __restrict__ ms_out) {
    __shared__ double acc[256];
    __shared__ int s_skip;
    const int n = blockIdx.x, tid = threadIdx.x;
    const unsigned char em = emit[n];
    if (gate_on[n] == 0 || em == 0) {                       // (block-uniform) an ungated or filling row: everything passes, state stays
        for (int s = tid; s < S; s += 256) seg_len_eff[(size_t)n * S + s] = seg_len[(size_t)n * S + s];
        if (tid == 0) {
            g0[n] = 1.0f;
            g1[n] = 1.0f;
            follow[n] = em;
            if (world_on && world_eff) world_eff[n] = world_on[n];
            if (ms_out) ms_out[n] = 0.0;
        }
        return;
    }
    const float* xr = x + (size_t)n * ld;
    double a = 0.0;
    for (int i = w_lo + tid; i < w_hi; i += 256) {
        const double v = (double)xr[i];
        a = a + v * v;
    }
    acc[tid] = a;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) acc[tid] = acc[tid] + acc[tid + o];
        __syncthreads();
    }
    if (tid == 0) {
        const double ms = acc[0] / (double)(w_hi - w_lo);
        int left = state[2 * n];
        const int was = state[2 * n + 1] != 0;
        int open;
        if (ms >= thr_ms[n]) {                              // (a NaN level is not loud)
            left = hold_ticks[n];
            open = 1;
        } else {
            open = left > 0;
            left = left - 1 > 0 ? left - 1 : 0;
        }
        state[2 * n] = left;
        state[2 * n + 1] = open;
        g0[n] = was ? 1.0f : 0.0f;
        g1[n] = open ? 1.0f : 0.0f;
        const int skip = !was && !open;                     // closed at both ends of the chunk: nothing of it is heard
        follow[n] = (unsigned char)(open ? 1 : 0);          // (emit[n] != 0 here)
        if (world_on && world_eff) world_eff[n] = (world_on[n] != 0 && !skip) ? 1 : 0;
        if (ms_out) ms_out[n] = ms;
        s_skip = skip;
    }
    __syncthreads();
    const int skip = s_skip;
    for (int s = tid; s < S; s += 256) seg_len_eff[(size_t)n * S + s] = skip ? 0 : seg_len[(size_t)n * S + s];
}

// grid (ceil(ld / 256), N): thread i of row n owns sample i of the row; only those inside the row's clamped span do anything
__global__ __launch_bounds__(256) void gate_apply_rows_kernel(float* __restrict__ y, int ld, const int* __restrict__ span_lo,
                                                              const int* __restrict__ span_len, const float* __restrict__ g0,
                                                              const float* __restrict__ g1) {
    const int n = blockIdx.y;
    const float a = g0[n], b = g1[n];
    if (a == 1.0f && b == 1.0f) return;                     // an open row: not touched (no load, no store)
    const int lo = span_lo[n], len = span_len[n];
    const int p = blockIdx.x * 256 + threadIdx.x;           // (p < ld + 255: no overflow for ld < 2^31 - 256)
    if (len <= 0 || p >= ld || p < lo) return;
    const int64_t i64 = (int64_t)p - lo;                    // lo may be negative: the span's own index still counts from lo
    if (i64 >= len) return;
    const int i = (int)i64;
    float* q = y + (size_t)n * ld + p;
    if (a == 0.0f && b == 0.0f) {                           // a closed row: +0, whatever was there (a NaN does not leak)
        *q = 0.0f;
        return;
    }
    const float t = (float)(i + 1) / (float)len;
    const float m = a + (b - a) * t;                        // (-ffp-contract=off: every operation rounded on its own)
    *q = *q * m;
}

}  // namespace

extern "C" int alive_gate_rows(const float* x, int N, int ld, int w_lo, int w_hi, const int* gate_on, const double* thr_ms,
                               const int* hold_ticks, const unsigned char* emit, const int* world_on, int S, const int* seg_len,
                               int* state, float* g0, float* g1, int* seg_len_eff, unsigned char* follow, int* world_eff,
                               double* ms_out, void* stream) {
    ALIVE_CHECK_ARG(x && gate_on && thr_ms && hold_ticks && emit && seg_len && state && g0 && g1 && seg_len_eff && follow,
                    "alive_gate_rows: null pointer");
    ALIVE_CHECK_ARG((world_on == nullptr) == (world_eff == nullptr), "alive_gate_rows: world_on and world_eff go together");
    ALIVE_CHECK_ARG(N > 0 && ld > 0 && S > 0 && (int64_t)N * S < (int64_t)1 << 31, "alive_gate_rows: bad args");
    ALIVE_CHECK_ARG(0 <= w_lo && w_lo < w_hi && w_hi <= ld, "alive_gate_rows: window [%d, %d) outside [0, %d) or empty", w_lo, w_hi, ld);
    gate_rows_kernel<<<N, 256, 0, (hipStream_t)stream>>>(x, ld, w_lo, w_hi, gate_on, thr_ms, hold_ticks, emit, world_on, S, seg_len,
                                                         state, g0, g1, seg_len_eff, follow, world_eff, ms_out);
    ALIVE_CHECK_LAUNCH("alive_gate_rows");
    return ALIVE_OK;
}

extern "C" int alive_gate_apply_rows(float* y, int N, int ld, const int* span_lo, const int* span_len, const float* g0,
                                     const float* g1, void* stream) {
    ALIVE_CHECK_ARG(y && span_lo && span_len && g0 && g1, "alive_gate_apply_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535 && ld > 0 && ld < (1 << 30), "alive_gate_apply_rows: bad args");
    gate_apply_rows_kernel<<<dim3(cdiv(ld, 256), N), 256, 0, (hipStream_t)stream>>>(y, ld, span_lo, span_len, g0, g1);
    ALIVE_CHECK_LAUNCH("alive_gate_apply_rows");
    return ALIVE_OK;
}
