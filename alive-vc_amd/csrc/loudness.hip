// Loudness normalisation after ITU-R BS.1770-4 / EBU R 128 (module/multistream.py: measure_loudness, normalize_loudness,
// MultiStreamConverter(loudness=True)).  Everything is fp64 with every operation rounded on its own (-ffp-contract=off); the device uses
// only + - * / sqrt and compares, every 10^x, 2^x and tan is the host's: bitwise tools/loudness_ref.py.  The full definitions are in
// include/alive_vc.h.
//   K-weighting: two biquads in transposed direct form II, the second fed the first's output; a non-finite sample counts as 0.0.
//   Offline (alive_loudness_measure_waves): a tile is a sub-block of `hop` samples and every tile is ONE LANE, run twice.  Pass E runs
//   the recurrence over the tile from zero state and leaves its 4-state e[j]; one lane per row then carries s[j + 1] = AP s[j] + e[j]
//   (AP: the state left by `hop` zero samples from each unit state, the host's); pass Q runs the tile again from s[j] and sums the
//   squares into q[j]; one lane per row forms the 400-ms blocks and gates them twice.  9 doubles per tile of workspace, no [N][ld]
//   fp64 copy of the signal.  A lane reads its tile 8 samples ahead of the dependent chain.
//   Streaming (alive_loudness_rows): one block of 64 threads per row, so that no two sessions share a serial chain.  The span is staged
//   in LDS by the whole block, lane 0 runs the filter and the running loudness over it, and the whole block applies the gain ramp.
//   No atomics; every store is a plain vector store.
#include "common.h"

namespace {

constexpr int NST = ALIVE_LOUDNESS_STATE, NPAR = ALIVE_LOUDNESS_PARAMS;
constexpr int STAGE = 1024;                                 // samples of a span staged in LDS at a time

__device__ __forceinline__ double clean(float v) {          // a NaN fails the compare too
    return fabsf(v) <= 3.4028234663852886e38f ? (double)v : 0.0;
}

struct KW {
    double c[10];
    __device__ __forceinline__ void load(const double* p) {
#pragma unroll
        for (int i = 0; i < 10; ++i) c[i] = p[i];
    }
    // one sample through both stages; z = (stage 1's z1, z2, stage 2's z1, z2)
    __device__ __forceinline__ double step(double v, double* z) const {
        const double o1 = c[0] * v + z[0];
        z[0] = (c[1] * v - c[3] * o1) + z[1];
        z[1] = c[2] * v - c[4] * o1;
        const double o2 = c[5] * o1 + z[2];
        z[2] = (c[6] * o1 - c[8] * o2) + z[3];
        z[3] = c[7] * o1 - c[9] * o2;
        return o2;
    }
};

__device__ __forceinline__ bool row_tiles(const int* len, const int* hop, int n, int ld, int max_tiles, int& H, int& nb) {
    int ln = len[n];
    ln = ln < 0 ? 0 : (ln > ld ? ld : ln);
    H = hop[n];
    nb = H >= 1 ? ln / H : 0;
    if (nb > max_tiles) nb = 0;                             // a row the workspace does not hold is not measured
    return nb > 0;
}

// SUM: false -> e[j], the state after the tile from zero state; true -> q[j], the sum of squares of the tile run from s[j]
template <bool SUM>
__global__ __launch_bounds__(64) void tile_kernel(const float* __restrict__ y, int ld, const int* __restrict__ len,
                                                  const int* __restrict__ hop, const double* __restrict__ coef, int max_tiles,
                                                  double* __restrict__ E, const double* __restrict__ S, double* __restrict__ Q) {
    const int n = blockIdx.y, j = blockIdx.x * 64 + threadIdx.x;
    int H, nb;
    if (!row_tiles(len, hop, n, ld, max_tiles, H, nb) || j >= nb) return;
    KW k;
    k.load(coef + (size_t)n * 10);
    const size_t t = (size_t)n * max_tiles + j;
    double z[4] = {0.0, 0.0, 0.0, 0.0};
    if (SUM) {
#pragma unroll
        for (int r = 0; r < 4; ++r) z[r] = S[t * 4 + r];
    }
    const float* p = y + (size_t)n * ld + (size_t)j * H;   // (j + 1) H <= len <= ld
    double acc = 0.0;
    int i = 0;
    for (; i + 8 <= H; i += 8) {
        float v[8];
#pragma unroll
        for (int u = 0; u < 8; ++u) v[u] = p[i + u];
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const double o = k.step(clean(v[u]), z);
            if (SUM) acc = acc + o * o;
        }
    }
    for (; i < H; ++i) {
        const double o = k.step(clean(p[i]), z);
        if (SUM) acc = acc + o * o;
    }
    if (SUM) {
        Q[t] = acc;
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) E[t * 4 + r] = z[r];
    }
}

// one lane per row: s[0] = 0, s[j + 1] = (((AP[:,0] s[j][0] + AP[:,1] s[j][1]) + AP[:,2] s[j][2]) + AP[:,3] s[j][3]) + e[j]
__global__ __launch_bounds__(64) void carry_kernel(int ld, const int* __restrict__ len, const int* __restrict__ hop,
                                                   const double* __restrict__ ap, int max_tiles, const double* __restrict__ E,
                                                   double* __restrict__ S) {
    const int n = blockIdx.x;
    int H, nb;
    if (threadIdx.x != 0 || !row_tiles(len, hop, n, ld, max_tiles, H, nb)) return;
    double A[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) A[i] = ap[(size_t)n * 16 + i];
    const size_t t0 = (size_t)n * max_tiles;
    double s[4] = {0.0, 0.0, 0.0, 0.0};
    for (int j = 0; j < nb; ++j) {
        double w[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            S[(t0 + j) * 4 + r] = s[r];
            w[r] = (((A[r * 4] * s[0] + A[r * 4 + 1] * s[1]) + A[r * 4 + 2] * s[2]) + A[r * 4 + 3] * s[3]) + E[(t0 + j) * 4 + r];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) s[r] = w[r];
    }
}

__device__ __forceinline__ double block_z(const double* q, int b, int H) {
    return (((q[b] + q[b + 1]) + q[b + 2]) + q[b + 3]) / (double)(4 * (int64_t)H);
}

// one lane per row: the 400-ms blocks and the two gating passes
__global__ __launch_bounds__(64) void gate_kernel(int ld, const int* __restrict__ len, const int* __restrict__ hop, int max_tiles,
                                                  const double* __restrict__ Q, double z_abs, double* __restrict__ zI,
                                                  int* __restrict__ c1, int* __restrict__ c2) {
    const int n = blockIdx.x;
    if (threadIdx.x != 0) return;
    int H, nb;
    row_tiles(len, hop, n, ld, max_tiles, H, nb);
    const double* q = Q + (size_t)n * max_tiles;
    double sum1 = 0.0, sum2 = 0.0;
    int n1 = 0, n2 = 0;
    for (int b = 0; b + 4 <= nb; ++b) {
        const double z = block_z(q, b, H);
        if (z > z_abs) {
            sum1 = sum1 + z;
            ++n1;
        }
    }
    if (n1 > 0) {
        const double rel = 0.1 * (sum1 / (double)n1);
        for (int b = 0; b + 4 <= nb; ++b) {
            const double z = block_z(q, b, H);
            if (z > z_abs && z > rel) {
                sum2 = sum2 + z;
                ++n2;
            }
        }
    }
    zI[n] = n2 > 0 ? sum2 / (double)n2 : 0.0;
    c1[n] = n1;
    c2[n] = n2;
}

__device__ __forceinline__ double clamp_gain(double r, double gmax) {
    const double lo = 1.0 / gmax;
    r = r > lo ? r : lo;                                    // max(r, lo), then min(.., gmax)
    return r < gmax ? r : gmax;
}

__global__ __launch_bounds__(256) void apply_kernel(float* __restrict__ out, const float* __restrict__ y, int ld,
                                                    const int* __restrict__ len, const double* __restrict__ zI,
                                                    const int* __restrict__ c2, const double* __restrict__ z_t, double gmax,
                                                    double* __restrict__ gain) {
    const int n = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    const double zt = z_t[n];
    int ln = len[n];
    ln = ln < 0 ? 0 : (ln > ld ? ld : ln);
    const bool copy = !(zt == zt);                          // a NaN target: the row is copied bit for bit
    const double g = copy || c2[n] <= 0 ? 1.0 : clamp_gain(sqrt(zt / zI[n]), gmax);
    if (gain && i == 0) gain[n] = g;
    if (i >= ld) return;
    const float v = y[(size_t)n * ld + i];
    out[(size_t)n * ld + i] = copy || i >= ln ? v : (float)((double)v * g);
}

__global__ __launch_bounds__(64) void rows_kernel(float* __restrict__ y, int ld, const int* __restrict__ span_lo,
                                                  const int* __restrict__ span_len, const unsigned char* __restrict__ emit,
                                                  const unsigned char* __restrict__ on, const int* __restrict__ hop,
                                                  const double* __restrict__ coef, const double* __restrict__ par,
                                                  double* __restrict__ state) {
    __shared__ float buf[STAGE];
    __shared__ double ramp[2];
    const int n = blockIdx.x, tid = threadIdx.x;
    if (emit[n] == 0) return;                               // (block-uniform) a filling, stalled or closed slot: y and its state stay
    double* st = state + (size_t)n * NST;
    const int lo = span_lo[n], S = span_len[n], H = hop[n];
    const bool fits = on[n] != 0 && H >= 1 && lo >= 0 && S >= 1 && (int64_t)lo + S <= (int64_t)ld;
    if (!fits) {                                            // off for the row, or a span outside the row: y stays, the state starts over
        if (tid < NST) st[tid] = tid == 12 ? 1.0 : 0.0;
        return;
    }
    float* yr = y + (size_t)n * ld + lo;
    const double* pr = par + (size_t)n * NPAR;
    KW k;
    double z[4], acc, cnt, q0, q1, q2, nsub, Sm, W, g;
    if (tid == 0) {
        k.load(coef + (size_t)n * 10);
        z[0] = st[0], z[1] = st[1], z[2] = st[2], z[3] = st[3];
        acc = st[4], cnt = st[5], q0 = st[6], q1 = st[7], q2 = st[8], nsub = st[9], Sm = st[10], W = st[11], g = st[12];
    }
    const double z_abs = pr[0], z_t = pr[1], d = pr[2], P = pr[3], gmax = pr[4], qs = pr[5];
    const double Hd = (double)H, H4 = (double)(4 * (int64_t)H);
    for (int t0 = 0; t0 < S; t0 += STAGE) {
        const int T = S - t0 < STAGE ? S - t0 : STAGE;
        for (int q = tid; q < T; q += 64) buf[q] = yr[t0 + q];
        __syncthreads();
        if (tid == 0) {
            for (int i = 0; i < T; ++i) {
                const double o = k.step(clean(buf[i]), z);
                acc = acc + o * o;
                cnt = cnt + 1.0;
                if (cnt >= Hd) {                            // a sub-block is complete: the 400-ms block that ends with it
                    nsub = nsub < 3.0 ? nsub + 1.0 : 4.0;
                    const double zb = (((q0 + q1) + q2) + acc) / H4;
                    Sm = Sm * d;
                    W = W * d;
                    if (nsub == 4.0 && zb > z_abs && (W < P || zb * W > 0.1 * Sm)) {
                        Sm = Sm + zb;
                        W = W + 1.0;
                    }
                    q0 = q1, q1 = q2, q2 = acc;
                    acc = 0.0, cnt = 0.0;
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double G = 1.0;
        if (W != 0.0) {
            const double r = clamp_gain(sqrt(z_t / (Sm / W)), gmax);
            double a = W / P;
            a = a < 1.0 ? a : 1.0;
            G = 1.0 + a * (r - 1.0);
        }
        const double lo_g = g / qs, hi_g = g * qs;          // the slew: at most qs up or down from the previous tick's gain
        G = G > lo_g ? G : lo_g;
        G = G < hi_g ? G : hi_g;
        ramp[0] = g, ramp[1] = G;
        st[0] = z[0], st[1] = z[1], st[2] = z[2], st[3] = z[3];
        st[4] = acc, st[5] = cnt, st[6] = q0, st[7] = q1, st[8] = q2, st[9] = nsub, st[10] = Sm, st[11] = W, st[12] = G;
    }
    __syncthreads();
    const double g0 = ramp[0], dg = ramp[1] - ramp[0], Sd = (double)S;
    for (int i = tid; i < S; i += 64) yr[i] = (float)((double)yr[i] * (g0 + dg * ((double)(i + 1) / Sd)));
}

bool overlap(const void* a, const void* b, size_t bytes) {
    const char *p = (const char*)a, *q = (const char*)b;
    return !(p + bytes <= q || q + bytes <= p);
}

}  // namespace

extern "C" size_t alive_loudness_workspace_bytes(int N, int max_tiles) {
    if (N <= 0 || N > 65535 || max_tiles <= 0) return 0;
    return (size_t)N * (size_t)max_tiles * 9 * sizeof(double);
}

extern "C" int alive_loudness_measure_waves(const float* y, int N, int ld, const int* len, const int* hop, const double* coef,
                                            const double* ap, double z_abs, int max_tiles, double* zI, int* c1, int* c2,
                                            void* workspace, size_t workspace_bytes, void* stream) {
    ALIVE_CHECK_ARG(y && len && hop && coef && ap && zI && c1 && c2 && workspace, "alive_loudness_measure_waves: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535 && ld > 0 && max_tiles > 0 && z_abs > 0.0 && z_abs < 1e300,
                    "alive_loudness_measure_waves: bad args");
    ALIVE_CHECK_ARG(workspace_bytes >= alive_loudness_workspace_bytes(N, max_tiles),
                    "alive_loudness_measure_waves: workspace of %zu bytes, %zu needed", workspace_bytes,
                    alive_loudness_workspace_bytes(N, max_tiles));
    const size_t tiles = (size_t)N * max_tiles;
    double *E = (double*)workspace, *S = E + tiles * 4, *Q = S + tiles * 4;
    const dim3 grid((max_tiles + 63) / 64, N);
    hipStream_t s = (hipStream_t)stream;
    tile_kernel<false><<<grid, 64, 0, s>>>(y, ld, len, hop, coef, max_tiles, E, nullptr, nullptr);
    ALIVE_CHECK_LAUNCH("alive_loudness_measure_waves");
    carry_kernel<<<N, 64, 0, s>>>(ld, len, hop, ap, max_tiles, E, S);
    ALIVE_CHECK_LAUNCH("alive_loudness_measure_waves");
    tile_kernel<true><<<grid, 64, 0, s>>>(y, ld, len, hop, coef, max_tiles, nullptr, S, Q);
    ALIVE_CHECK_LAUNCH("alive_loudness_measure_waves");
    gate_kernel<<<N, 64, 0, s>>>(ld, len, hop, max_tiles, Q, z_abs, zI, c1, c2);
    ALIVE_CHECK_LAUNCH("alive_loudness_measure_waves");
    return ALIVE_OK;
}

extern "C" int alive_loudness_apply_waves(float* out, const float* y, int N, int ld, const int* len, const double* zI, const int* c2,
                                          const double* z_t, double gmax, double* gain, void* stream) {
    ALIVE_CHECK_ARG(out && y && len && zI && c2 && z_t, "alive_loudness_apply_waves: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535 && ld > 0 && gmax >= 1.0 && gmax < 1e300, "alive_loudness_apply_waves: bad args");
    ALIVE_CHECK_ARG(!overlap(out, y, (size_t)N * ld * sizeof(float)), "alive_loudness_apply_waves: out overlaps y");
    apply_kernel<<<dim3((ld + 255) / 256, N), 256, 0, (hipStream_t)stream>>>(out, y, ld, len, zI, c2, z_t, gmax, gain);
    ALIVE_CHECK_LAUNCH("alive_loudness_apply_waves");
    return ALIVE_OK;
}

extern "C" int alive_loudness_rows(float* y, int N, int ld, const int* span_lo, const int* span_len, const unsigned char* emit,
                                   const unsigned char* on, const int* hop, const double* coef, const double* par, double* state,
                                   void* stream) {
    ALIVE_CHECK_ARG(y && span_lo && span_len && emit && on && hop && coef && par && state, "alive_loudness_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && ld > 0, "alive_loudness_rows: bad args");
    rows_kernel<<<N, 64, 0, (hipStream_t)stream>>>(y, ld, span_lo, span_len, emit, on, hop, coef, par, state);
    ALIVE_CHECK_LAUNCH("alive_loudness_rows");
    return ALIVE_OK;
}
