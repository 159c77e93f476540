// Output limiter (module/multistream.py: MultiStreamConverter(limiter=True); module/realtime.py: limit_db=; limit_waves offline): a
// lookahead peak limiter in front of the int16 edge, which wraps whatever leaves [-1, 1).  With ceiling c, lookahead L >= 1 and hold
// H >= 0 (P = L - 1 + H), for stream index i of the emitted signal y:
//   a[j]   = c / fmaxf(|y[j]|, c)                     the required gain: exactly 1.0f where |y[j]| <= c, 1 for a NaN, 0 for an inf
//   m[k]   = min a[k - H .. k + L - 1]
//   g[i]   = (float)(sum_{k = i - L + 1 .. i, ascending, in double from 0.0} (double)m[k] / (double)L)
//   out[i] = fminf(fmaxf(y[i] * g[i], -c), c)         (-ffp-contract=off: every operation rounded on its own)
// Every window that enters g[i] contains i, so g[i] <= a[i] and |out[i]| <= c whatever the neighbours are.
//   one block of 256 threads per row (alive_limit_rows) or per tile of a row (alive_limit_waves).  The required gains of everything a
//   tile of ALIVE_LIMIT_TILE samples depends on lie in LDS; the window minima are formed there by doubling (min over 1, 2, 4, ...
//   samples, then two overlapping power-of-two windows per m[k]): min is exact, so the order is free.  The fp64 sum is NOT order-free:
//   every thread adds its L minima in ascending order.  Every pass over LDS that reads what another thread writes stages its results
//   in registers between two barriers; a sample of y is read and written by the same thread; the history is read into LDS once and
//   written back once.  Every store is a plain vector store; the only atomic is the integer min of alive_limit_waves' gmin.
#include "common.h"

namespace {

constexpr int TILE = ALIVE_LIMIT_TILE, MAXH = ALIVE_LIMIT_MAX_HIST;
constexpr int CAP = 2 * MAXH + TILE;                        // history (>= P) + tile + lookahead (L - 1 <= P <= MAXH)
constexpr int EPT = CAP / 256;
static_assert(CAP % 256 == 0 && 2 * CAP * 4 + 1024 <= 64 * 1024, "two staging arrays and the reduction must fit 64 KB of LDS");

__device__ __forceinline__ float required_gain(float v, float c) { return c / fmaxf(fabsf(v), c); }

__device__ __forceinline__ bool ceil_ok(float c) { return c > 0.0f && c <= 1.0f; }

// M[0, n) holds required gains; on return M[s] = min of the W of them from s on, for s < n - W + 1 (1 <= W <= n <= CAP).  Called by
// the whole block.
__device__ __forceinline__ void window_min(float* M, int n, int W, int tid) {
    float r[EPT];
    int step = 1;
    for (; 2 * step <= W; step *= 2) {                      // M[j] = min over [j, j + step) -> over [j, j + 2 step), where that fits
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int j = tid + e * 256;
            if (j < n) r[e] = j + step < n ? fminf(M[j], M[j + step]) : M[j];
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < EPT; ++e) {
            const int j = tid + e * 256;
            if (j < n) M[j] = r[e];
        }
        __syncthreads();
    }
    const int cnt = n - W + 1, off = W - step;              // step <= W < 2 step: two windows of `step` cover W; j + off + step <= n
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int j = tid + e * 256;
        if (j < cnt) r[e] = fminf(M[j], M[j + off]);
    }
    __syncthreads();
#pragma unroll
    for (int e = 0; e < EPT; ++e) {
        const int j = tid + e * 256;
        if (j < cnt) M[j] = r[e];
    }
    __syncthreads();
}

// the gain of the sample whose L window minima start at m[0]: their mean, summed in double in ascending order from 0.0
__device__ __forceinline__ float mean_gain(const float* m, int L) {
    double s = 0.0;
    for (int k = 0; k < L; ++k) s = s + (double)m[k];
    return (float)(s / (double)L);
}

__device__ __forceinline__ float block_min(float v, float* red, int tid) {
    red[tid] = v;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) red[tid] = fminf(red[tid], red[tid + o]);
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(256) void limit_rows_kernel(float* __restrict__ y, int ld, const int* __restrict__ span_lo,
                                                         const int* __restrict__ span_len, const int* __restrict__ shift,
                                                         const int* __restrict__ look, const int* __restrict__ hold,
                                                         const float* __restrict__ ceil, const unsigned char* __restrict__ emit,
                                                         float* __restrict__ hist, int ld_hist, float* __restrict__ gmin) {
    __shared__ float A[CAP];                                // [0, ld_hist): the history; then the tile's gains and its lookahead
    __shared__ float M[CAP];
    __shared__ float red[256];
    const int n = blockIdx.x, tid = threadIdx.x;
    if (emit[n] == 0) return;                               // (block-uniform) a filling or closed slot: y, hist and gmin stay
    float* hr = hist + (size_t)n * ld_hist;
    const int lo = span_lo[n], S = span_len[n], sh = shift[n], L = look[n], H = hold[n];
    const float c = ceil[n];
    const bool fits = L >= 1 && H >= 0 && lo >= 0 && S >= 0 && S <= sh && L <= sh && (int64_t)lo + sh + L - 1 <= (int64_t)ld &&
                      (int64_t)L - 1 + H <= (int64_t)ld_hist;
    if (!fits || !ceil_ok(c)) {                             // the limiter off for the row, or regions outside the row: y stays
        for (int q = tid; q < ld_hist; q += 256) hr[q] = 1.0f;
        if (gmin && tid == 0) gmin[n] = 1.0f;
        return;
    }
    const int P = L - 1 + H;
    float* yr = y + (size_t)n * ld;
    for (int q = tid; q < ld_hist; q += 256) A[q] = hr[q];
    float gm = 1.0f;
    for (int t0 = 0; t0 < S; t0 += TILE) {
        const int T = S - t0 < TILE ? S - t0 : TILE;
        // stream indices t0 .. t0 + T + L - 2: the present from the span (later tiles are not written yet), the future from one
        // chunk on, where the next tick's span will come from; the largest index read is lo + sh + L - 2 < ld
        for (int q = tid; q < T + L - 1; q += 256) {
            const int i = t0 + q;
            A[ld_hist + q] = required_gain(yr[i < S ? lo + i : lo + sh + (i - S)], c);
        }
        __syncthreads();
        const int o = ld_hist - P, nA = P + T + L - 1;      // the gains of stream indices t0 - P .. t0 + T + L - 2
        for (int q = tid; q < nA; q += 256) M[q] = A[o + q];
        __syncthreads();
        window_min(M, nA, L + H, tid);                      // M[s] = m[t0 - (L - 1) + s], s < T + L - 1
        for (int q = tid; q < T; q += 256) {
            const float g = mean_gain(M + q, L);
            const float v = yr[lo + t0 + q];
            yr[lo + t0 + q] = fminf(fmaxf(v * g, -c), c);
            gm = fminf(gm, g);
        }
        __syncthreads();
        for (int q = tid; q < ld_hist; q += 256) M[q] = A[T + q];        // the history moves on by the tile, through M
        __syncthreads();
        for (int q = tid; q < ld_hist; q += 256) A[q] = M[q];
        __syncthreads();
    }
    __syncthreads();
    for (int q = tid; q < ld_hist; q += 256) hr[q] = A[q];
    if (gmin) {                                             // (block-uniform)
        const float v = block_min(gm, red, tid);
        if (tid == 0) gmin[n] = v;
    }
}

__global__ void limit_fill_kernel(float* __restrict__ v, int n, float value) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) v[i] = value;
}

__global__ __launch_bounds__(256) void limit_waves_kernel(float* __restrict__ out, const float* __restrict__ y, int ld,
                                                          const int* __restrict__ len, int L, int H, const float* __restrict__ ceil,
                                                          int* __restrict__ gmin_bits) {
    __shared__ float M[CAP];
    __shared__ float red[256];
    const int n = blockIdx.y, tid = threadIdx.x, t0 = blockIdx.x * TILE;
    const int T = ld - t0 < TILE ? ld - t0 : TILE;          // (t0 < ld: the grid has ceil(ld / TILE) tiles)
    const float* yr = y + (size_t)n * ld;
    float* orow = out + (size_t)n * ld;
    const float c = ceil[n];
    int ln = len[n];
    ln = ln < 0 ? 0 : (ln > ld ? ld : ln);
    if (t0 >= ln || !ceil_ok(c)) {                          // (block-uniform) past the signal, or no valid ceiling: copied
        for (int q = tid; q < T; q += 256) orow[t0 + q] = yr[t0 + q];
        return;
    }
    const int Tl = ln - t0 < T ? ln - t0 : T, P = L - 1 + H;
    const int nA = P + Tl + L - 1;                          // the gains of indices t0 - P .. t0 + Tl + L - 2, 1 outside [0, ln)
    for (int q = tid; q < nA; q += 256) {
        const int j = t0 - P + q;
        M[q] = j >= 0 && j < ln ? required_gain(yr[j], c) : 1.0f;
    }
    __syncthreads();
    window_min(M, nA, L + H, tid);
    float gm = 1.0f;
    for (int q = tid; q < T; q += 256) {
        const float v = yr[t0 + q];
        if (q < Tl) {
            const float g = mean_gain(M + q, L);
            orow[t0 + q] = fminf(fmaxf(v * g, -c), c);
            gm = fminf(gm, g);
        } else {
            orow[t0 + q] = v;
        }
    }
    if (gmin_bits) {                                        // (block-uniform) every g is >= +0: the order of the bits is that of the values
        const float v = block_min(gm, red, tid);
        if (tid == 0) atomicMin(gmin_bits + n, __float_as_int(v));
    }
}

}  // namespace

extern "C" int alive_limit_rows(float* y, int N, int ld, const int* span_lo, const int* span_len, const int* shift, const int* look,
                                const int* hold, const float* ceil, const unsigned char* emit, float* hist, int ld_hist, float* gmin,
                                void* stream) {
    ALIVE_CHECK_ARG(y && span_lo && span_len && shift && look && hold && ceil && emit && hist, "alive_limit_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && ld > 0 && ld_hist > 0 && ld_hist <= ALIVE_LIMIT_MAX_HIST, "alive_limit_rows: bad args");
    limit_rows_kernel<<<N, 256, 0, (hipStream_t)stream>>>(y, ld, span_lo, span_len, shift, look, hold, ceil, emit, hist, ld_hist, gmin);
    ALIVE_CHECK_LAUNCH("alive_limit_rows");
    return ALIVE_OK;
}

extern "C" int alive_limit_waves(float* out, const float* y, int N, int ld, const int* len, int look, int hold, const float* ceil,
                                 float* gmin, void* stream) {
    ALIVE_CHECK_ARG(out && y && len && ceil, "alive_limit_waves: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535 && ld > 0 && look >= 1 && hold >= 0 && (int64_t)look - 1 + hold <= ALIVE_LIMIT_MAX_HIST,
                    "alive_limit_waves: bad args");
    const size_t bytes = (size_t)N * ld * sizeof(float);
    const char *a = (const char*)out, *b = (const char*)y;
    ALIVE_CHECK_ARG(a + bytes <= b || b + bytes <= a, "alive_limit_waves: out overlaps y (a tile's halo is another tile's output)");
    if (gmin) {
        limit_fill_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)stream>>>(gmin, N, 1.0f);
        ALIVE_CHECK_LAUNCH("alive_limit_waves");
    }
    limit_waves_kernel<<<dim3((ld + TILE - 1) / TILE, N), 256, 0, (hipStream_t)stream>>>(out, y, ld, len, look, hold, ceil, (int*)gmin);
    ALIVE_CHECK_LAUNCH("alive_limit_waves");
    return ALIVE_OK;
}
