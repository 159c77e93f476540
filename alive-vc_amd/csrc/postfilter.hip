// Post filter (module/multistream.py: post_filter, MultiStreamConverter(post_filter=True); module/realtime.py: post_filter=): an adaptive
// formant post filter (Chen & Gersho 1995) on the converted 16 kHz wave y.  Per frame of `hop` samples an LPC analysis of the frame's
// window gives A(z); the frame's filter is A(z / b) / A(z / a) (a = alpha[row], b = a * ratio) with a first-order tilt compensation, as
// a 128-tap impulse response h_f; the frame's gain g[f] brings the filtered frame back to the level of the unfiltered one; between the
// frame centres the output moves linearly from g[f] U(f, i) to g[f + 1] U(f + 1, i), U(f, i) = sum_k h_f[k] y[i - k].  The arithmetic
// and every order in it are fixed by include/alive_vc.h "Post filter" and restated by tools/postfilter_ref.py: integer sums for the
// autocorrelation (exact, so their partition cannot show), then fp64 with only + - * / and sqrt, each rounded on its own
// (-ffp-contract=off).  Bitwise the restatement.
//   grid (tiles, rows), 256 threads.  The output of a row is cut at the frame CENTRES: unit u covers [u hop + hop / 2, (u + 1) hop +
//   hop / 2) and needs the filters and gains of frames u and u + 1 alone; unit -1 is the first half frame (frame 0 alone) and unit
//   F - 1 the rest behind the last centre (frame F - 1 alone).  A tile is ALIVE_POSTFILTER_TILE units, 16 t - 1 .. 16 t + 14, and so
//   needs the TILE + 1 frames 16 t - 1 .. 16 t + 15: it recomputes the two it shares with its neighbours.  A frame's filter and gain
//   depend on the frame's place in its row alone, so every block that forms them gets the same bits.
//     1  one wave per frame: s = q * win into LDS, the order + 1 lags as int64 sums across the lanes, r[k] = (double)R[k] * lag[k]
//     2  one lane per frame: Levinson-Durbin, the impulse response and the tilt, in LDS
//     3  one wave per frame: the frame's samples and 128 before them into LDS, U(f, .) over the frame, Ein and Eout in envelope.hip's
//        frame_sum order (lane l holds accumulators 4 l .. 4 l + 3), g[f]
//     4  one wave per unit: the unit's samples likewise, both dot products per sample, the interpolation, the store
//   In 3 and 4 a lane owns 4 adjacent samples: per 4 taps it reads ONE 16-byte group of samples (the window slides in registers) and
//   the 4 taps of each filter as broadcast reads.  No workspace, no dependency between blocks, no floating-point atomics; every store
//   is a plain vector store; the only atomics are the integer min / max of gain_minmax.
#include "common.h"

#include <cmath>

namespace {

constexpr int TAPS = ALIVE_POSTFILTER_TAPS, MAXP = ALIVE_POSTFILTER_MAX_ORDER, TILE = ALIVE_POSTFILTER_TILE;
constexpr int NF = TILE + 1;                               // the frames a tile needs
constexpr int HS = TAPS + 2;                               // the stride of a filter in LDS (doubles): 16-byte rows, lanes on other banks
constexpr int AS = MAXP + 1;                               // the stride of r and A (33 doubles: consecutive lanes two banks apart)
constexpr int WB = TAPS + 1024;                            // a wave's sample buffer: 128 of history and at most 1024 samples
constexpr int ROUNDS = (NF + 3) / 4;
static_assert(TAPS == 128 && TAPS % 4 == 0, "the dot product walks the taps in groups of 4 from sample buffer offset 128");
static_assert(NF <= 64, "one lane per frame");

__device__ __forceinline__ int quantise(float x) {         // the int16 grid; NaN -> 0
    const float v = x * 32768.0f;
    if (v != v) return 0;
    return (int)fminf(fmaxf(rintf(v), -32767.0f), 32767.0f);
}

// U over the lane's 4 adjacent samples wb[4 b .. 4 b + 3] for one filter (TWO: two filters), taps ascending from 0.0.  Tap 4 m + r of
// sample s reads wb[4 (b - m) + s - r]: of the 8 floats in v, entry 4 + s - r
template <bool TWO>
__device__ __forceinline__ void dot4(const float* wb, int b, const double* hA, const double* hB, double (&uA)[4], double (&uB)[4]) {
    const float4* w4 = reinterpret_cast<const float4*>(wb);
    float4 cur = w4[b];
#pragma unroll
    for (int s = 0; s < 4; ++s) uA[s] = 0.0, uB[s] = 0.0;
#pragma unroll 2
    for (int m = 0; m < TAPS / 4; ++m) {
        const float4 prev = w4[b - m - 1];
        const double v[8] = {(double)prev.x, (double)prev.y, (double)prev.z, (double)prev.w,
                             (double)cur.x,  (double)cur.y,  (double)cur.z,  (double)cur.w};
        const double2 a01 = *reinterpret_cast<const double2*>(hA + 4 * m), a23 = *reinterpret_cast<const double2*>(hA + 4 * m + 2);
        const double ha[4] = {a01.x, a01.y, a23.x, a23.y};
#pragma unroll
        for (int r = 0; r < 4; ++r)
#pragma unroll
            for (int s = 0; s < 4; ++s) uA[s] = uA[s] + ha[r] * v[4 + s - r];
        if (TWO) {
            const double2 b01 = *reinterpret_cast<const double2*>(hB + 4 * m), b23 = *reinterpret_cast<const double2*>(hB + 4 * m + 2);
            const double hb[4] = {b01.x, b01.y, b23.x, b23.y};
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int s = 0; s < 4; ++s) uB[s] = uB[s] + hb[r] * v[4 + s - r];
        }
        cur = prev;
    }
}

// samples [start - 128, start + cnt) of the row into wb[0, 128 + cnt rounded up to 4): 0 before the row and at or beyond start + cnt
__device__ __forceinline__ void stage(float* wb, const float* __restrict__ yr, int start, int cnt, int lane) {
    const int total = TAPS + ((cnt + 3) & ~3);
    for (int j = lane; j < total; j += 64) {
        const int i = start - TAPS + j;
        wb[j] = (i >= 0 && j < TAPS + cnt) ? yr[i] : 0.0f;
    }
}

__global__ void postfilter_fill_kernel(int* __restrict__ mm_bits, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {                                            // (+inf, +0): every filtered frame lowers and raises them
        mm_bits[2 * i] = 0x7f800000;
        mm_bits[2 * i + 1] = 0;
    }
}

__global__ __launch_bounds__(256) void postfilter_kernel(float* __restrict__ out, const float* __restrict__ y, int ld,
                                                         const int* __restrict__ len, const float* __restrict__ alpha, int hop,
                                                         int window, int order, const int16_t* __restrict__ win,
                                                         const double* __restrict__ lag, double ratio, double tilt, double e,
                                                         double g_lo, double g_hi, int* __restrict__ mm_bits) {
    __shared__ __attribute__((aligned(16))) double H[NF * HS];          // the filters
    __shared__ double Rr[NF * AS], A[NF * AS], G[NF];                   // r[k]; A[j], then den[j]; the gains
    __shared__ __attribute__((aligned(16))) float Wb[4 * WB];           // per wave: s (as ints) in 1, the samples in 3 and 4
    const int row = blockIdx.y, tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const int c = hop >> 1;
    const long long u0 = (long long)blockIdx.x * TILE - 1;              // the tile's first unit = its first frame
    const long long lo_l = u0 < 0 ? 0 : u0 * hop + c, hi_l = (u0 + TILE) * hop + c;
    const int lo = (int)lo_l, hi = hi_l < (long long)ld ? (int)hi_l : ld;    // (lo < ld: the grid ends with the tile that holds ld - 1)
    const float* yr = y + (size_t)row * ld;
    float* orow = out + (size_t)row * ld;
    int n = len ? len[row] : ld;
    n = n < 0 ? 0 : (n > ld ? ld : n);
    const float al = alpha[row];
    const bool filters = al > 0.0f && al <= 0.85f && n > 0;             // (block-uniform; a NaN fails both)
    for (int i = (filters && n > lo ? n : lo) + tid; i < hi; i += 256) orow[i] = yr[i];      // what is not filtered is copied
    if (!filters) {
        if (mm_bits && blockIdx.x == 0 && tid == 0) {
            atomicMin(mm_bits + 2 * row, __float_as_int(1.0f));
            atomicMax(mm_bits + 2 * row + 1, __float_as_int(1.0f));
        }
        return;
    }
    if (lo >= n) return;
    const int F = (int)(((long long)n + hop - 1) / hop);
    const int fa = (int)u0;                                             // slot q: frame fa + q
    float* wb = Wb + wave * WB;

    // 1: the autocorrelation of each frame's window
    int* sb = reinterpret_cast<int*>(wb);
    const int half = (window - hop) >> 1;
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int q = 4 * rd + wave, f = fa + q;
        const bool live = q < NF && f >= 0 && f < F;                    // (wave-uniform)
        if (live) {
            const long long at = (long long)f * hop - half;
            for (int i = lane; i < window; i += 64) {
                const long long p = at + i;
                sb[i] = (p >= 0 && p < (long long)n) ? quantise(yr[p]) * (int)win[i] : 0;
            }
        }
        __syncthreads();
        if (live) {
            for (int k = 0; k <= order; ++k) {
                long long acc = 0;
                for (int i = lane; i + k < window; i += 64) acc += (long long)sb[i] * (long long)sb[i + k];
#pragma unroll
                for (int o = 32; o > 0; o >>= 1) acc += __shfl_down(acc, o, 64);
                if (lane == 0) Rr[q * AS + k] = (double)acc * lag[k];
            }
        }
        __syncthreads();
    }

    // 2: Levinson-Durbin, the impulse response of num / den and the tilt compensation: one lane per frame
    if (tid < NF && fa + tid >= 0 && fa + tid < F) {
        double* r = Rr + tid * AS;
        double* a = A + tid * AS;
        double* h = H + tid * HS;
        const double r0 = r[0] * 1.0001;
        bool ident = !(r0 > 0.0);
        double err = r0;
        for (int m = 1; m <= order && !ident; ++m) {
            double acc = r[m];
            for (int j = 1; j < m; ++j) acc = acc + a[j] * r[m - j];
            const double k = -acc / err;
            if (!std::isfinite(k) || !(fabs(k) < 1.0)) {
                ident = true;
                break;
            }
            int j = 1, jj = m - 1;
            for (; j < jj; ++j, --jj) {                                 // A'[j] = A[j] + k A[m - j], both ends at once
                const double x0 = a[j], x1 = a[jj];
                a[j] = x0 + k * x1;
                a[jj] = x1 + k * x0;
            }
            if (j == jj) {
                const double x0 = a[j];
                a[j] = x0 + k * x0;
            }
            a[m] = k;
            err = err * (1.0 - k * k);
            if (!(err > 0.0)) ident = true;
        }
        if (ident) {
            for (int k = 0; k < TAPS; ++k) h[k] = k == 0 ? 1.0 : 0.0;
        } else {
            const double da = (double)al, db = da * ratio;
            double pa = 1.0, pb = 1.0;
            h[0] = 1.0;
            for (int j = 1; j <= order; ++j) {
                pa = pa * da;
                pb = pb * db;
                const double x = a[j];
                h[j] = x * pb;                                          // num[j], where h0[j] starts from
                a[j] = x * pa;                                          // den[j]
            }
            for (int k = 1; k < TAPS; ++k) {
                double acc = 0.0;
                const int top = k < order ? k : order;
                for (int j = 1; j <= top; ++j) acc = acc + a[j] * h[k - j];
                h[k] = (k <= order ? h[k] : 0.0) - acc;
            }
            double c0 = 0.0, c1 = 0.0;
            for (int k = 0; k < TAPS; ++k) c0 = c0 + h[k] * h[k];
            for (int k = 0; k + 1 < TAPS; ++k) c1 = c1 + h[k] * h[k + 1];
            const double t = tilt * (c1 / c0);
            for (int k = TAPS - 1; k >= 1; --k) h[k] = h[k] - t * h[k - 1];
        }
    }
    __syncthreads();

    // 3: the gains: Ein and Eout over each frame's own samples
    for (int rd = 0; rd < ROUNDS; ++rd) {
        const int q = 4 * rd + wave, f = fa + q;
        const bool live = q < NF && f >= 0 && f < F;
        const int at = live ? f * hop : 0, cnt = live ? (n - at < hop ? n - at : hop) : 0;
        if (live) stage(wb, yr, at, cnt, lane);
        __syncthreads();
        if (live) {
            double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0, b0 = 0.0, b1 = 0.0, b2 = 0.0, b3 = 0.0;
            for (int x = 4 * lane; x < cnt; x += 256) {
                double u[4], unused[4];
                dot4<false>(wb, (TAPS + x) >> 2, H + q * HS, nullptr, u, unused);
                const float4 t = reinterpret_cast<const float4*>(wb)[(TAPS + x) >> 2];      // (0 beyond cnt: adds +0.0)
                a0 = a0 + (double)t.x * (double)t.x;
                a1 = a1 + (double)t.y * (double)t.y;
                a2 = a2 + (double)t.z * (double)t.z;
                a3 = a3 + (double)t.w * (double)t.w;
                const double p1 = x + 1 < cnt ? u[1] : 0.0, p2 = x + 2 < cnt ? u[2] : 0.0, p3 = x + 3 < cnt ? u[3] : 0.0;
                b0 = b0 + u[0] * u[0];
                b1 = b1 + p1 * p1;
                b2 = b2 + p2 * p2;
                b3 = b3 + p3 * p3;
            }
            double si = (a0 + a1) + (a2 + a3), so = (b0 + b1) + (b2 + b3);
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) {
                si = si + __shfl_down(si, o, 64);
                so = so + __shfl_down(so, o, 64);
            }
            if (lane == 0) {
                const double ee = e * (double)cnt;
                const double den = so + ee, qq = (si + ee) / den;
                double g = 1.0;
                if (std::isfinite(qq) && std::isfinite(den)) {          // (an infinite Eout gives qq = 0: no level to restore either)
                    g = sqrt(qq);
                    g = g > g_lo ? g : g_lo;
                    g = g < g_hi ? g : g_hi;
                }
                G[q] = g;
                if (mm_bits && q >= 1) {                                // (slot 0 is the previous tile's slot TILE; g > 0: the order
                    const int bits = __float_as_int((float)g);          //  of the bits is that of the values)
                    atomicMin(mm_bits + 2 * row, bits);
                    atomicMax(mm_bits + 2 * row + 1, bits);
                }
            }
        }
        __syncthreads();
    }

    // 4: the output, unit by unit
    for (int rd = 0; rd < TILE / 4; ++rd) {
        const int q = 4 * rd + wave;                                    // unit fa + q: frames fa + q (slot q) and fa + q + 1
        const long long u = u0 + q;
        int at = 0, cnt = 0;
        if (u < (long long)F) {
            const long long s0 = u < 0 ? 0 : u * hop + c;
            long long s1 = u < 0 ? c : (u == F - 1 ? (long long)n : (u + 1) * hop + c);
            s1 = s1 < (long long)n ? s1 : (long long)n;
            if (s1 > s0) at = (int)s0, cnt = (int)(s1 - s0);
        }
        const bool live = cnt > 0;                                      // (wave-uniform)
        if (live) stage(wb, yr, at, cnt, lane);
        __syncthreads();
        if (live) {
            const bool first = u < 0, edge = first || u == F - 1;       // one frame alone: frame 0 (slot q + 1) / frame F - 1 (slot q)
            const int qa = first ? q + 1 : q;
            const double ga = G[qa], gb = edge ? 0.0 : G[q + 1];
            for (int x = 4 * lane; x < cnt; x += 256) {
                double ua[4], ub[4];
                float o[4];
                if (edge) {
                    dot4<false>(wb, (TAPS + x) >> 2, H + qa * HS, nullptr, ua, ub);
#pragma unroll
                    for (int s = 0; s < 4; ++s) o[s] = (float)(ga * ua[s]);
                } else {
                    dot4<true>(wb, (TAPS + x) >> 2, H + q * HS, H + (q + 1) * HS, ua, ub);
#pragma unroll
                    for (int s = 0; s < 4; ++s) {
                        const double w = (double)(x + s) / (double)hop, z0 = ga * ua[s], z1 = gb * ub[s];
                        o[s] = (float)(z0 + (z1 - z0) * w);
                    }
                }
                float* p = orow + at + x;
                if (x + 3 < cnt && ((uintptr_t)p & 15) == 0) {
                    *reinterpret_cast<float4*>(p) = make_float4(o[0], o[1], o[2], o[3]);
                } else {
#pragma unroll
                    for (int s = 0; s < 4; ++s)
                        if (x + s < cnt) p[s] = o[s];
                }
            }
        }
        __syncthreads();
    }
}

}  // namespace

extern "C" int alive_postfilter_waves(float* out, const float* y, int ld, int N, const int* len, const float* alpha, int hop,
                                      int window, int order, const int16_t* win, const double* lag, double ratio, double tilt,
                                      double floor_ms, double g_lo, double g_hi, float* gain_minmax, void* stream) {
    ALIVE_CHECK_ARG(out && y && alpha && win && lag, "alive_postfilter_waves: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535 && ld > 0, "alive_postfilter_waves: bad args");
    ALIVE_CHECK_ARG(hop >= 2 && hop <= 1024 && hop % 2 == 0, "alive_postfilter_waves: hop must be even and in [2, 1024]");
    ALIVE_CHECK_ARG(window >= hop && window <= 1024 && (window - hop) % 2 == 0,
                    "alive_postfilter_waves: window must be hop plus an even excess >= 0, at most 1024");
    ALIVE_CHECK_ARG(order >= 1 && order <= ALIVE_POSTFILTER_MAX_ORDER && order < window, "alive_postfilter_waves: order outside [1, %d]",
                    ALIVE_POSTFILTER_MAX_ORDER);
    ALIVE_CHECK_ARG(std::isfinite(ratio) && ratio >= 0.0 && ratio <= 1.0, "alive_postfilter_waves: ratio must be finite and in [0, 1]");
    ALIVE_CHECK_ARG(std::isfinite(tilt) && tilt >= 0.0 && tilt <= 1.0, "alive_postfilter_waves: tilt must be finite and in [0, 1]");
    ALIVE_CHECK_ARG(std::isfinite(floor_ms) && floor_ms > 0.0, "alive_postfilter_waves: the floor must be finite and > 0");
    ALIVE_CHECK_ARG(std::isfinite(g_lo) && std::isfinite(g_hi) && g_lo > 0.0 && g_lo <= 1.0 && g_hi >= 1.0,
                    "alive_postfilter_waves: the range needs 0 < g_lo <= 1 <= g_hi, both finite");
    const char *o = (const char*)out, *a = (const char*)y;
    const size_t by = (size_t)N * ld * sizeof(float);
    ALIVE_CHECK_ARG(o + by <= a || a + by <= o, "alive_postfilter_waves: out overlaps y (a tile reads the samples around its own)");
    if (gain_minmax) {
        postfilter_fill_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)stream>>>((int*)gain_minmax, N);
        ALIVE_CHECK_LAUNCH("alive_postfilter_waves");
    }
    const int c = hop / 2;                                  // the tiles end where (16 T - 1) hop + c >= ld
    const long long span = (long long)TILE * hop, tiles = ((long long)ld + hop - c + span - 1) / span;
    postfilter_kernel<<<dim3((unsigned)tiles, N), 256, 0, (hipStream_t)stream>>>(out, y, ld, len, alpha, hop, window, order, win, lag,
                                                                                ratio, tilt, floor_ms, g_lo, g_hi, (int*)gain_minmax);
    ALIVE_CHECK_LAUNCH("alive_postfilter_waves");
    return ALIVE_OK;
}
