// Envelope follow (module/multistream.py: follow_envelope, MultiStreamConverter(envelope=True); module/realtime.py: envelope=): the
// converted wave y takes on the loudness contour of the source x, which lies beside it sample for sample at 16 kHz.  Per row, with
// frames of `hop` samples, F = ceil(n / hop), radius R, amount m, floor e (a mean square) and range [g_lo, g_hi]:
//   Sx[f], Sy[f]  fp64 sums of squares over [f hop, min((f + 1) hop, n)), in the fixed order of frame_sum below
//   Px, Py        sums of Sx / Sy over t = a .. b (a = max(f - R, 0), b = min(f + R, F - 1)), ascending from 0.0
//   Cn            (double)(min((b + 1) hop, n) - a hop)
//   q             (Px / Cn + e) / (Py / Cn + e);  rc = min(max(sqrt(q), g_lo), g_hi) if q is finite, else 1.0
//   G[f]          1.0 + (double)m * (rc - 1.0)
//   g[i]          G[0] for i < hop / 2, G[F - 1] for i >= hop / 2 + (F - 1) hop, else G[f] + (G[f + 1] - G[f]) * w with
//                 f = (i - hop / 2) / hop and w = (double)((i - hop / 2) - f hop) / (double)hop
//   out[i]        (float)((double)y[i] * g[i])        (-ffp-contract=off: every operation rounded on its own)
// Only + - * / and sqrt, all fp64: bitwise tools/envelope_ref.py.
//   grid (tiles of ALIVE_ENVELOPE_TILE frames, rows), 256 threads.  A block needs G of its own frames and of one frame on each side,
//   and so the frame sums of R + 1 more frames on each side: it recomputes those, one wave per frame and both signals at once, and
//   keeps Sx, Sy and G in LDS as doubles.  A frame's sum depends on the frame's place in its row alone -- not on N, the other rows or
//   the tile -- so every block that forms it gets the same bits.  No workspace, no dependency between blocks, no floating-point
//   atomics; every store is a plain vector store; the only atomics are the integer min / max of gain_minmax.
#include "common.h"

#include <cmath>

namespace {

constexpr int TILE = ALIVE_ENVELOPE_TILE, MAXR = ALIVE_ENVELOPE_MAX_RADIUS;
constexpr int NS = TILE + 2 * (MAXR + 1);                   // the frame sums a tile may need
static_assert(TILE + 2 <= 256, "one thread per frame gain");

// The sum of squares of v[0, cnt), 1 <= cnt <= 1024, by one wave; every lane returns it.  The order: 256 accumulators, accumulator a
// adds v[a + 256 j]^2 for ascending j from 0.0 (a square of a float is exact in fp64; a missing sample adds +0.0, which is exact for
// these non-negative sums); lane l holds accumulators 4 l .. 4 l + 3 -- one 16-byte load per step where the frame starts on a 16-byte
// boundary, four 4-byte loads with the same result otherwise -- and combines them as (a0 + a1) + (a2 + a3); then a pairwise tree over
// the lanes with offsets 32, 16, .., 1.
__device__ __forceinline__ double frame_sum(const float* __restrict__ v, int cnt, int lane) {
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    const bool vec = ((uintptr_t)v & 15) == 0;              // (wave-uniform)
    for (int e = 4 * lane; e < cnt; e += 256) {
        float p0, p1, p2, p3;
        if (vec && e + 3 < cnt) {
            const float4 t = *reinterpret_cast<const float4*>(v + e);
            p0 = t.x, p1 = t.y, p2 = t.z, p3 = t.w;
        } else {
            p0 = v[e];
            p1 = e + 1 < cnt ? v[e + 1] : 0.0f;
            p2 = e + 2 < cnt ? v[e + 2] : 0.0f;
            p3 = e + 3 < cnt ? v[e + 3] : 0.0f;
        }
        a0 = a0 + (double)p0 * (double)p0;
        a1 = a1 + (double)p1 * (double)p1;
        a2 = a2 + (double)p2 * (double)p2;
        a3 = a3 + (double)p3 * (double)p3;
    }
    double s = (a0 + a1) + (a2 + a3);
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) s = s + __shfl_down(s, o, 64);      // lane l < o: s[l] + s[l + o]; lane 0 ends with the sum
    return __shfl(s, 0, 64);
}

// the gain of sample i < n of a row with F frames; G points at the gain of frame fb
__device__ __forceinline__ double sample_gain(const double* G, int fb, int i, int hop, int F, long long last) {
    const int c = hop >> 1;
    if (i < c) return G[0 - fb];
    if ((long long)i >= last) return G[F - 1 - fb];
    const int d = i - c, f = d / hop;
    const double w = (double)(d - f * hop) / (double)hop;
    const double g0 = G[f - fb], g1 = G[f + 1 - fb];
    return g0 + (g1 - g0) * w;
}

__device__ __forceinline__ float follow_sample(float v, const double* G, int fb, int i, int n, int hop, int F, long long last) {
    return i < n ? (float)((double)v * sample_gain(G, fb, i, hop, F, last)) : v;
}

__global__ void envelope_fill_kernel(int* __restrict__ mm_bits, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) {                                            // (+inf, +0): every row's first tile lowers and raises them
        mm_bits[2 * i] = 0x7f800000;
        mm_bits[2 * i + 1] = 0;
    }
}

__global__ __launch_bounds__(256) void envelope_kernel(float* __restrict__ out, const float* __restrict__ y, int ld_y,
                                                       const float* __restrict__ x, int ld_x, const int* __restrict__ len,
                                                       const float* __restrict__ amount, int hop, int R, double e, double g_lo,
                                                       double g_hi, int* __restrict__ mm_bits) {
    __shared__ double Sx[NS], Sy[NS], G[TILE + 2];
    const int row = blockIdx.y, tid = threadIdx.x, f0 = blockIdx.x * TILE;
    const long long t0l = (long long)f0 * hop, t1l = t0l + (long long)TILE * hop;
    const int t0 = (int)t0l, t1 = t1l < (long long)ld_y ? (int)t1l : ld_y;       // (t0 < ld_y: the grid has ceil(F_max / TILE) tiles)
    const float* yr = y + (size_t)row * ld_y;
    const float* xr = x + (size_t)row * ld_x;
    float* orow = out + (size_t)row * ld_y;
    const int cap = ld_y < ld_x ? ld_y : ld_x;
    int n = len ? len[row] : ld_y;
    n = n < 0 ? 0 : (n > cap ? cap : n);
    const float m = amount[row];
    const bool follows = m > 0.0f && m <= 1.0f && n > 0;    // (block-uniform; a NaN amount fails both)
    const bool vec = ((((uintptr_t)(yr + t0)) | ((uintptr_t)(orow + t0))) & 15) == 0;
    const int nv = vec ? (t1 - t0) >> 2 : 0;
    if (!follows || t0 >= n) {                              // a row that does not follow, or a tile past the signal: copied
        for (int q = tid; q < nv; q += 256)
            reinterpret_cast<float4*>(orow + t0)[q] = reinterpret_cast<const float4*>(yr + t0)[q];
        for (int i = t0 + 4 * nv + tid; i < t1; i += 256) orow[i] = yr[i];
        if (!follows && mm_bits && blockIdx.x == 0 && tid == 0) {
            atomicMin(mm_bits + 2 * row, __float_as_int(1.0f));
            atomicMax(mm_bits + 2 * row + 1, __float_as_int(1.0f));
        }
        return;
    }
    const int F = (int)(((long long)n + hop - 1) / hop);
    const int fs0 = f0 - (R + 1), nS = TILE + 2 * (R + 1);  // Sx[q], Sy[q]: frame fs0 + q
    const int wave = tid >> 6, lane = tid & 63;
    for (int q = wave; q < nS; q += 4) {                    // (wave-uniform)
        const int f = fs0 + q;
        double sx = 0.0, sy = 0.0;
        if (f >= 0 && f < F) {
            const int at = f * hop, cnt = n - at < hop ? n - at : hop;
            sx = frame_sum(xr + at, cnt, lane);
            sy = frame_sum(yr + at, cnt, lane);
        }
        if (lane == 0) {
            Sx[q] = sx;
            Sy[q] = sy;
        }
    }
    __syncthreads();
    const int fb = f0 - 1;                                  // G[q]: frame fb + q
    if (tid < TILE + 2) {
        const int f = fb + tid;
        double g = 1.0;
        if (f >= 0 && f < F) {
            const int a = f - R > 0 ? f - R : 0, b = f + R < F - 1 ? f + R : F - 1;
            double px = 0.0, py = 0.0;
            for (int t = a; t <= b; ++t) {
                px = px + Sx[t - fs0];
                py = py + Sy[t - fs0];
            }
            const long long hi = (long long)(b + 1) * hop;
            const double cn = (double)((hi < (long long)n ? hi : (long long)n) - (long long)a * hop);
            const double q = (px / cn + e) / (py / cn + e);
            double rc = 1.0;
            if (std::isfinite(q)) {
                rc = sqrt(q);
                rc = rc > g_lo ? rc : g_lo;
                rc = rc < g_hi ? rc : g_hi;
            }
            g = 1.0 + (double)m * (rc - 1.0);
            if (mm_bits && tid >= 1 && tid <= TILE) {       // the tile's own frames; g > 0: the order of the bits is that of the values
                const int bits = __float_as_int((float)g);
                atomicMin(mm_bits + 2 * row, bits);
                atomicMax(mm_bits + 2 * row + 1, bits);
            }
        }
        G[tid] = g;
    }
    __syncthreads();
    const long long last = (long long)(hop >> 1) + (long long)(F - 1) * hop;
    for (int q = tid; q < nv; q += 256) {
        const int i = t0 + 4 * q;
        float4 v = reinterpret_cast<const float4*>(yr + t0)[q];
        v.x = follow_sample(v.x, G, fb, i, n, hop, F, last);
        v.y = follow_sample(v.y, G, fb, i + 1, n, hop, F, last);
        v.z = follow_sample(v.z, G, fb, i + 2, n, hop, F, last);
        v.w = follow_sample(v.w, G, fb, i + 3, n, hop, F, last);
        reinterpret_cast<float4*>(orow + t0)[q] = v;
    }
    for (int i = t0 + 4 * nv + tid; i < t1; i += 256) orow[i] = follow_sample(yr[i], G, fb, i, n, hop, F, last);
}

}  // namespace

extern "C" int alive_envelope_waves(float* out, const float* y, int ld_y, const float* x, int ld_x, int N, const int* len,
                                    const float* amount, int hop, int radius, double floor_ms, double g_lo, double g_hi,
                                    float* gain_minmax, void* stream) {
    ALIVE_CHECK_ARG(out && y && x && amount, "alive_envelope_waves: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535 && ld_y > 0 && ld_x > 0, "alive_envelope_waves: bad args");
    ALIVE_CHECK_ARG(hop >= 2 && hop <= 1024 && hop % 2 == 0, "alive_envelope_waves: hop must be even and in [2, 1024]");
    ALIVE_CHECK_ARG(radius >= 0 && radius <= ALIVE_ENVELOPE_MAX_RADIUS, "alive_envelope_waves: radius outside [0, %d]",
                    ALIVE_ENVELOPE_MAX_RADIUS);
    ALIVE_CHECK_ARG(std::isfinite(floor_ms) && floor_ms > 0.0, "alive_envelope_waves: the floor must be finite and > 0");
    ALIVE_CHECK_ARG(std::isfinite(g_lo) && std::isfinite(g_hi) && g_lo > 0.0 && g_lo <= 1.0 && g_hi >= 1.0,
                    "alive_envelope_waves: the range needs 0 < g_lo <= 1 <= g_hi, both finite");
    const char *o = (const char*)out, *a = (const char*)y, *b = (const char*)x;
    const size_t by = (size_t)N * ld_y * sizeof(float), bx = (size_t)N * ld_x * sizeof(float);
    ALIVE_CHECK_ARG(o + by <= a || a + by <= o, "alive_envelope_waves: out overlaps y (a tile's halo is another tile's output)");
    ALIVE_CHECK_ARG(o + by <= b || b + bx <= o, "alive_envelope_waves: out overlaps x (a tile's halo is another tile's output)");
    if (gain_minmax) {
        envelope_fill_kernel<<<(N + 255) / 256, 256, 0, (hipStream_t)stream>>>((int*)gain_minmax, N);
        ALIVE_CHECK_LAUNCH("alive_envelope_waves");
    }
    const long long frames = ((long long)ld_y + hop - 1) / hop;
    const long long tiles = (frames + ALIVE_ENVELOPE_TILE - 1) / ALIVE_ENVELOPE_TILE;
    envelope_kernel<<<dim3((unsigned)tiles, N), 256, 0, (hipStream_t)stream>>>(out, y, ld_y, x, ld_x, len, amount, hop, radius, floor_ms,
                                                                              g_lo, g_hi, (int*)gain_minmax);
    ALIVE_CHECK_LAUNCH("alive_envelope_waves");
    return ALIVE_OK;
}
