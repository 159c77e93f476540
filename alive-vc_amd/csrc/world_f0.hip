// WORLD pitch estimation (DIO + StoneMask) on a batch of rows, in fp64 as WORLD computes it   (reference module/common.py:113-137,
// the f0 of `-wpe`).  Restated from the published algorithm; tools/world_ref.py is the NumPy restatement these kernels follow
// operation by operation (DESIGN.md "WORLD pitch").
//
//   mean     one block per row: the row's mean in a fixed order (256 strided sums, then a pairwise tree)
//   lowcut   the 50-Hz low cut (2c+1 taps, c = round(fs/50)) of the mean-removed row, a zero-extended linear convolution,
//            kept at every lag it reaches: yl[n], n in [-c, Ly + c), Ly = L + 1 (DIO's y_length: one zero sample past the end)
//   bands    one block per (row, band) sweeps the row in tiles of 1024 samples: the band's Nuttall low-pass (4h taps, delay 2h)
//            from an LDS tile of yl, the four event streams (negative / positive zero crossings of the band signal and of its
//            first difference) marked and compacted in sample order, and every frame's interp1 of each stream's intervals
//            resolved as soon as an interval lies past the frame's time (a wave per stream); only [N][bands][4][F] values and
//            the interval counts leave the block
//   select   one wave per row: candidate and score per (band, frame), the best band per frame, then FixF0Contour's four steps
//   stone    one wave per (row, frame): StoneMask, the DFT evaluated at the harmonic bins it reads only
// Every sum runs in a fixed order with mul and add rounded separately (-ffp-contract=off): the DIO contour is bitwise the
// restatement's on the same input and the same taps (alive_world_f0_taps computes them on the host with the C library's cos).
#include "common.h"
#include <math.h>
#include <string.h>
#include <vector>

namespace {

constexpr int WF_MAX_BANDS = 32;
constexpr int WF_TILE = 1024;         // band samples per sweep step
constexpr int WF_BT = 256;            // threads of a sweep block
constexpr int WF_MAX_NUTTALL = 1024;  // 4h of the lowest band
constexpr int WF_MAX_WIN = 1216;      // StoneMask window samples (2 round(3 fs / 80) + 1 at 16 kHz = 1201)
constexpr double WF_SAFE = 1e-12;     // WORLD's kMySafeGuardMinimum
constexpr double WF_KMAX = 100000.0;  // WORLD's kMaximumValue
constexpr double WF_LOG2 = 0.69314718055994529;
constexpr double WF_PI = 3.1415926535897932384;

struct WfPlan {
    int N, L, Ly, F, fs, nb, c;                  // c: low-cut half width
    int h[WF_MAX_BANDS], woff[WF_MAX_BANDS];     // band half-delay, offset of its taps in the table
    double bound[WF_MAX_BANDS];
    double f0_floor, f0_ceil, frame_period;
    int64_t yl_ld;                               // Ly + 2c
    size_t off_mean, off_yl, off_iv, off_ni, off_best, off_s1, off_s2, off_s3, off_pi, off_ng, total;
};

__host__ __device__ inline int mround(double x) { return x > 0 ? (int)(x + 0.5) : (int)(x - 0.5); }

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

int plan(WfPlan& p, int N, int L, int fs, double f0_floor, double f0_ceil, double frame_period) {
    if (N <= 0 || L <= 0 || fs <= 0 || fs > 16000 || !(f0_floor > 0) || !(f0_ceil > f0_floor) || !(frame_period > 0)) return -1;
    p.N = N, p.L = L, p.Ly = L + 1, p.fs = fs;
    p.f0_floor = f0_floor, p.f0_ceil = f0_ceil, p.frame_period = frame_period;
    p.F = (int)(1000.0 * L / fs / frame_period) + 1;
    p.nb = 1 + (int)(log(f0_ceil / f0_floor) / WF_LOG2 * 2.0);
    if (p.nb > WF_MAX_BANDS) return -2;
    p.c = mround(fs / 50.0);
    int off = 2 * p.c + 1;
    for (int i = 0; i < p.nb; ++i) {
        p.bound[i] = f0_floor * pow(2.0, (i + 1) / 2.0);
        p.h[i] = mround(fs / p.bound[i] / 2.0);
        if (p.h[i] < 1 || 4 * p.h[i] > WF_MAX_NUTTALL) return -3;
        p.woff[i] = off;
        off += 4 * p.h[i];
    }
    p.yl_ld = p.Ly + 2 * p.c;
    size_t o = 0;
    p.off_mean = o; o = align256(o + sizeof(double) * N);
    p.off_yl = o;   o = align256(o + sizeof(double) * N * p.yl_ld);
    p.off_iv = o;   o = align256(o + sizeof(double) * N * p.nb * 4 * (size_t)p.F);
    p.off_ni = o;   o = align256(o + sizeof(int) * N * p.nb * 4);
    p.off_best = o; o = align256(o + sizeof(double) * N * (size_t)p.F);
    p.off_s1 = o;   o = align256(o + sizeof(double) * N * (size_t)p.F);
    p.off_s2 = o;   o = align256(o + sizeof(double) * N * (size_t)p.F);
    p.off_s3 = o;   o = align256(o + sizeof(double) * N * (size_t)p.F);
    p.off_pi = o;   o = align256(o + sizeof(int) * N * (size_t)p.F);
    p.off_ng = o;   o = align256(o + sizeof(int) * N * (size_t)p.F);
    p.total = o;
    return 0;
}

int taps_count(const WfPlan& p) { return p.woff[p.nb - 1] + 4 * p.h[p.nb - 1]; }

// ---------------------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) wf_mean_kernel(const float* __restrict__ x, int L, const int32_t* __restrict__ row_on,
                                                     double* __restrict__ mean) {
    __shared__ double acc[256];
    const int r = blockIdx.x, t = threadIdx.x;
    if (row_on && !row_on[r]) return;                       // (uniform across the block)
    const float* xr = x + (int64_t)r * L;
    double a = 0.0;
    for (int i = t; i < L; i += 256) a = a + (double)xr[i];
    acc[t] = a;
    __syncthreads();
    for (int s = 128; s > 0; s >>= 1) {
        if (t < s) acc[t] = acc[t] + acc[t + s];
        __syncthreads();
    }
    if (t == 0) mean[r] = acc[0] / (double)(L + 1);
}

// yl[n] = sum_{j=0}^{2c} lc[j] y[n - (j - c)], n in [-c, Ly + c), y = x - mean on [0, L), -mean at L, 0 elsewhere
__global__ void __launch_bounds__(256) wf_lowcut_kernel(const float* __restrict__ x, const double* __restrict__ mean,
                                                        const double* __restrict__ lc, int L, int c, int64_t ld,
                                                        const int32_t* __restrict__ row_on, double* __restrict__ yl) {
    __shared__ double ys[256 + 2 * 400];
    const int r = blockIdx.y, t = threadIdx.x;
    if (row_on && !row_on[r]) return;
    const int n0 = (int)blockIdx.x * 256 - c;               // first output lag of the block
    const float* xr = x + (int64_t)r * L;
    const double m = mean[r];
    // ys[q] = y[n0 - c + q], q in [0, 256 + 2c)
    for (int q = t; q < 256 + 2 * c; q += 256) {
        const int i = n0 - c + q;
        ys[q] = (i >= 0 && i < L) ? (double)xr[i] - m : (i == L ? 0.0 - m : 0.0);
    }
    __syncthreads();
    const int n = n0 + t;
    if (n >= L + 1 + c) return;
    double a = 0.0;
    for (int j = 0; j <= 2 * c; ++j) a = a + lc[j] * ys[t + 2 * c - j];   // y[n - j + c] = ys[n - j + c - (n0 - c)]
    yl[(int64_t)r * ld + n + c] = a;
}

__device__ inline double fine_edge(int e, double a, double b) { return (double)e - a / (b - a); }   // a = sig[e-1], b = sig[e]

// one block per (band, row)
__global__ void __launch_bounds__(WF_BT) wf_bands_kernel(const double* __restrict__ yl_all, const double* __restrict__ taps,
                                                         WfPlan p, const int32_t* __restrict__ row_on, double* __restrict__ iv_all,
                                                         int* __restrict__ ni_all) {
    __shared__ double ybuf[WF_TILE + WF_MAX_NUTTALL];
    __shared__ double sbuf[WF_TILE + 2];
    __shared__ double ebuf[4][WF_TILE + 3];
    __shared__ int cnt[4][4][4];                // [round][wave][stream]
    __shared__ int tile_n[4];
    const int b = blockIdx.x, r = blockIdx.y, t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (row_on && !row_on[r]) return;
    const int h = p.h[b], nt = 4 * h, Ly = p.Ly, F = p.F;
    const double fs = (double)p.fs;
    const double* w = taps + p.woff[b];
    const double* yl = yl_all + (int64_t)r * p.yl_ld;      // yl[n] at n + c
    double* iv = iv_all + ((int64_t)r * p.nb + b) * 4 * F;
    // per-stream state (held by every lane of wave `wv`, stream wv)
    int ne = 0, fp = 0;
    for (int i0 = 0; i0 < Ly; i0 += WF_TILE) {
        // ybuf[q] = yl[i0 - 2h + 1 + q], q < TILE + 4h - 1
        for (int q = t; q < WF_TILE + nt - 1; q += WF_BT) {
            const int n = i0 - 2 * h + 1 + q;
            ybuf[q] = (n >= -p.c && n < Ly + p.c) ? yl[n + p.c] : 0.0;
        }
        __syncthreads();
        // s[i0 + u] = sum_j w[j] yl[i0 + u + 2h - j] = sum_j w[j] ybuf[u + 4h - 1 - j]
        double s[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) s[k] = 0.0;
        for (int j = 0; j < nt; ++j) {
            const double wj = w[j];
#pragma unroll
            for (int k = 0; k < 4; ++k) s[k] = s[k] + wj * ybuf[t + k * WF_BT + nt - 1 - j];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) sbuf[2 + t + k * WF_BT] = s[k];
        __syncthreads();
        // events at p = i0 + u: neg / pos crossing between p-1 and p, peak / dip crossing of d between p-2 and p-1 (edge p-1)
        double fe[4][4];
        unsigned fl[4] = {0, 0, 0, 0};
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int u = t + k * WF_BT, pp = i0 + u;
            if (pp < Ly) {
                const double s0 = sbuf[2 + u - 2], s1 = sbuf[2 + u - 1], s2 = sbuf[2 + u];
                if (pp >= 1) {
                    if (0.0 < s1 && s2 <= 0.0) { fl[0] |= 1u << k; fe[0][k] = fine_edge(pp, s1, s2); }
                    const double n1 = -s1, n2 = -s2;
                    if (0.0 < n1 && n2 <= 0.0) { fl[1] |= 1u << k; fe[1][k] = fine_edge(pp, n1, n2); }
                }
                if (pp >= 2) {
                    const double d0 = (-s0) - (-s1), d1 = (-s1) - (-s2);
                    if (0.0 < d0 && d1 <= 0.0) { fl[2] |= 1u << k; fe[2][k] = fine_edge(pp - 1, d0, d1); }
                    const double m0 = -d0, m1 = -d1;
                    if (0.0 < m0 && m1 <= 0.0) { fl[3] |= 1u << k; fe[3][k] = fine_edge(pp - 1, m0, m1); }
                }
            }
        }
        const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
        uint64_t bal[4][4];
#pragma unroll
        for (int k = 0; k < 4; ++k)
#pragma unroll
            for (int st = 0; st < 4; ++st) {
                bal[k][st] = __ballot((fl[st] >> k) & 1u);
                if (lane == 0) cnt[k][wv][st] = __popcll(bal[k][st]);
            }
        __syncthreads();
        // compacted slots: ebuf[st][3 + rank], rank in (round, wave, lane) order = sample order
#pragma unroll
        for (int st = 0; st < 4; ++st) {
            int base = 0;
            for (int k = 0; k < 4; ++k) {
                for (int ww = 0; ww < 4; ++ww) {
                    if (ww == wv) {
                        if ((fl[st] >> k) & 1u) ebuf[st][3 + base + __popcll(bal[k][st] & below)] = fe[st][k];
                    }
                    base += cnt[k][ww][st];
                }
            }
            if (t == 0) tile_n[st] = base;
        }
        __syncthreads();
        // wave wv: stream wv -- resolve the frames whose time lies before the newest interval
        {
            const int st = wv, kt = tile_n[st];
            const int ne_after = ne + kt, ni = ne_after > 0 ? ne_after - 1 : 0;
            const int base = ne - 3;                         // global edge g sits in slot g - base
            const double* E = ebuf[st];
            const int qlo = ne - 3 > 0 ? ne - 3 : 0;          // first interval whose two edges are in slots
            const bool last = i0 + WF_TILE >= Ly;
            auto loc = [&](int q) { return (E[q - base] + E[q + 1 - base]) / 2.0 / fs; };
            auto val = [&](int q) { return fs / (E[q + 1 - base] - E[q - base]); };
            if (ni >= 2) {
                const double newest = loc(ni - 1);
                while (fp < F) {
                    const int f = fp + lane;
                    const double tf = (double)f * p.frame_period / 1000.0;
                    const bool ok = f < F && (last || tf < newest);
                    const uint64_t m = __ballot(ok);
                    if (ok) {
                        int lo = qlo, hi = ni;                // c = qlo + #{q in [qlo, ni): loc_q <= tf}
                        while (lo < hi) {
                            const int mid = (lo + hi) >> 1;
                            if (loc(mid) <= tf) lo = mid + 1; else hi = mid;
                        }
                        int k = lo < 1 ? 1 : lo;
                        if (k > ni - 1) k = ni - 1;
                        const double x0 = loc(k - 1), x1 = loc(k), y0 = val(k - 1), y1 = val(k);
                        const double hh = x1 - x0, sfrac = (tf - x0) / hh;
                        iv[(int64_t)st * F + f] = y0 + sfrac * (y1 - y0);
                    }
                    const int adv = __popcll(m);
                    fp += adv;
                    if (adv < 64) break;
                }
            }
            if (last && lane == 0) ni_all[((int64_t)r * p.nb + b) * 4 + st] = ni;
            // carry the newest three edges into slots 0..2
            double keep = 0.0;
            if (lane < 3 && ne_after - 3 + lane >= 0) keep = E[ne_after - 3 + lane - base];
            __builtin_amdgcn_wave_barrier();
            if (lane < 3) ebuf[st][lane] = keep;
            ne = ne_after;
        }
        if (t < 2) sbuf[t] = sbuf[WF_TILE + t];
        __syncthreads();
    }
}

// one wave per row: candidates / scores, best band, FixF0Contour
__device__ inline double select_best(const double* cand, int64_t bstride, int nb, int j, double cur, double past, double allowed,
                                     int lane) {
    const double ref = (cur * 3.0 - past) / 2.0;
    double cv = lane < nb ? cand[(int64_t)lane * bstride + j] : 0.0;
    double err = lane < nb ? fabs(ref - cv) : INFINITY;
    int idx = lane < nb ? lane : 1 << 20;
    for (int o = 32; o > 0; o >>= 1) {
        const double e2 = __shfl_xor(err, o), c2 = __shfl_xor(cv, o);
        const int i2 = __shfl_xor(idx, o);
        if (e2 < err || (e2 == err && i2 < idx)) err = e2, cv = c2, idx = i2;
    }
    return fabs(1.0 - cv / ref) > allowed ? 0.0 : cv;
}

__global__ void __launch_bounds__(64) wf_select_kernel(WfPlan p, const int32_t* __restrict__ row_on, double* __restrict__ iv_all,
                                                       const int* __restrict__ ni_all,
                                                       double* __restrict__ best_all, double* __restrict__ s1_all,
                                                       double* __restrict__ s2_all, double* __restrict__ s3_all,
                                                       int* __restrict__ pi_all, int* __restrict__ ng_all) {
    const int r = blockIdx.x, lane = threadIdx.x, F = p.F, nb = p.nb;
    if (row_on && !row_on[r]) return;
    double* iv = iv_all + (int64_t)r * nb * 4 * F;
    const int* ni = ni_all + (int64_t)r * nb * 4;
    double* best = best_all + (int64_t)r * F;
    double* s1 = s1_all + (int64_t)r * F;
    double* s2 = s2_all + (int64_t)r * F;
    double* s3 = s3_all + (int64_t)r * F;
    const int64_t bstride = 4 * (int64_t)F;                  // the candidate of band b replaces its stream-0 value
    for (int f = lane; f < F; f += 64) {
        double low = 0.0, bf = 0.0;
        for (int b = 0; b < nb; ++b) {
            double cand = 0.0, score = WF_KMAX;
            double* v = iv + b * bstride;
            if (ni[b * 4] > 2 && ni[b * 4 + 1] > 2 && ni[b * 4 + 2] > 2 && ni[b * 4 + 3] > 2) {
                const double a0 = v[f], a1 = v[F + f], a2 = v[2 * F + f], a3 = v[3 * F + f];
                cand = (((a0 + a1) + a2) + a3) / 4.0;
                const double d0 = a0 - cand, d1 = a1 - cand, d2 = a2 - cand, d3 = a3 - cand;
                score = sqrt((((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3) / 3.0);
                const double bd = p.bound[b];
                if (cand > bd || cand < bd / 2.0 || cand > p.f0_ceil || cand < p.f0_floor) cand = 0.0, score = WF_KMAX;
            }
            v[f] = cand;
            const double sc = score / (cand + WF_SAFE);
            if (b == 0 || low > sc) low = sc, bf = cand;
        }
        best[f] = bf;
    }
    __syncthreads();
    const int vr = (int)(0.5 + 1000.0 / p.frame_period / p.f0_floor) * 2 + 1;
    const double allowed = 0.1;
    if (F <= vr) {
        for (int f = lane; f < F; f += 64) s3[f] = 0.0;
        return;
    }
    // step 1
    for (int i = lane; i < F; i += 64) {
        double v = 0.0;
        if (i >= vr) {
            const double cb = (i < F - vr) ? best[i] : 0.0;
            const double pb = (i - 1 >= vr && i - 1 < F - vr) ? best[i - 1] : 0.0;
            v = fabs((cb - pb) / (WF_SAFE + cb)) < allowed ? cb : 0.0;
        }
        s1[i] = v;
    }
    __syncthreads();
    // step 2
    const int ctr = (vr - 1) / 2;
    for (int i = lane; i < F; i += 64) {
        double v = s1[i];
        if (i >= ctr && i < F - ctr)
            for (int j = -ctr; j <= ctr; ++j)
                if (s1[i + j] == 0) { v = 0.0; break; }
        s2[i] = v;
        s3[i] = v;
    }
    __syncthreads();
    // voiced sections of step 2 (every lane walks the same list)
    int* pos = pi_all + (int64_t)r * F;
    int* neg = ng_all + (int64_t)r * F;
    int npos = 0, nneg = 0;
    if (lane == 0) {
        for (int i = 1; i < F; ++i) {
            if (s2[i] == 0 && s2[i - 1] != 0) neg[nneg++] = i - 1;
            else if (s2[i - 1] == 0 && s2[i] != 0) pos[npos++] = i;
        }
    }
    npos = __shfl(npos, 0);
    nneg = __shfl(nneg, 0);
    __syncthreads();
    // step 3 (forward from every section end) and step 4 (backward from every section start), in place on s3
    for (int i = 0; i < nneg; ++i) {
        const int limit = i == nneg - 1 ? F - 1 : neg[i + 1];
        for (int j = neg[i]; j < limit; ++j) {
            const double v = select_best(iv, bstride, nb, j + 1, s3[j], s3[j - 1], allowed, lane);
            __syncthreads();
            if (lane == 0) s3[j + 1] = v;
            __syncthreads();
            if (v == 0) break;
        }
    }
    for (int i = npos - 1; i >= 0; --i) {
        const int limit = i == 0 ? 1 : pos[i - 1];
        for (int j = pos[i]; j > limit; --j) {
            const double v = select_best(iv, bstride, nb, j - 1, s3[j], s3[j + 1], allowed, lane);
            __syncthreads();
            if (lane == 0) s3[j - 1] = v;
            __syncthreads();
            if (v == 0) break;
        }
    }
}

// StoneMask: one wave per (row, frame), 2 waves per block
__device__ inline void dft_bin(const double* mw, const double* dw, int m, int n, int k, int lane, double out[4]) {
    double mr = 0, mi = 0, dr = 0, di = 0;
    k %= n;
    for (int i = lane; i < m; i += 64) {
        const int q = (int)(((int64_t)k * i) % n);
        double sn, cs;
        sincospi(2.0 * q / n, &sn, &cs);
        mr = mr + mw[i] * cs; mi = mi - mw[i] * sn;
        dr = dr + dw[i] * cs; di = di - dw[i] * sn;
    }
    for (int o = 32; o > 0; o >>= 1) {
        mr += __shfl_xor(mr, o); mi += __shfl_xor(mi, o);
        dr += __shfl_xor(dr, o); di += __shfl_xor(di, o);
    }
    out[0] = mr, out[1] = mi, out[2] = dr, out[3] = di;
}

__device__ double fix_f0(const double* mw, const double* dw, int m, int n, double fs, double f0, int harmonics, int lane) {
    double num = 0.0, den = 0.0;
    for (int i = 0; i < harmonics; ++i) {
        const int idx = mround(f0 * n / fs * (i + 1));
        double s[4];
        dft_bin(mw, dw, m, n, idx, lane, s);
        const double num_i = s[0] * s[3] - s[1] * s[2];
        const double pw = s[0] * s[0] + s[1] * s[1];
        const double inst = pw == 0.0 ? 0.0 : (double)idx * fs / n + num_i / pw * fs / 2.0 / WF_PI;
        const double amp = sqrt(pw);
        num += amp * inst;
        den += amp * (i + 1);
    }
    return den != 0.0 ? num / den : 0.0;        // a window without energy (WORLD divides 0 by 0 here): no refinement
}

__global__ void __launch_bounds__(128) wf_stone_kernel(const float* __restrict__ x8, WfPlan p, const double* __restrict__ dio_all,
                                                       const int32_t* __restrict__ row_on, float* __restrict__ out) {
    __shared__ double mwin[2][WF_MAX_WIN], dwin[2][WF_MAX_WIN];
    const int r = blockIdx.y, wv = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int f = blockIdx.x * 2 + wv;
    if (f >= p.F) return;
    if (row_on && !row_on[r]) {                             // an off row: unvoiced, nothing read
        if (lane == 0) out[(int64_t)r * p.F + f] = 0.0f;
        return;
    }
    const int L = p.L;
    const double fs = (double)p.fs;
    const float* x = x8 + (int64_t)r * L;
    const double f0 = dio_all[(int64_t)r * p.F + f];
    const double tpos = (double)f * p.frame_period / 1000.0;
    float res = 0.0f;
    if (!(f0 <= 40.0 || f0 > fs / 12.0)) {
        const double hw = 3.0 / f0 / 2.0;
        const int rr = mround(hw * fs), m = rr * 2 + 1;
        const double wl = (double)(rr * 2 + 1) / fs;
        // WORLD's (int)pow(2.0, 2.0 + (int)(...)) as a shift: the device pow(2.0, 11.0) lies below 2048 and truncated to 2047, the
        // DFT length of every frame with f0 in (40, 46.875] Hz at 16 kHz
        const int n = 1 << (2 + (int)(log(hw * fs + WF_SAFE) / WF_LOG2));
        const int basic = mround((tpos + (double)(-rr) / fs) * fs + 0.001);
        double* mw = mwin[wv];
        double* dw = dwin[wv];
        for (int i = lane; i < m; i += 64) {
            const double tmp = ((double)(basic + i) - 1.0) / fs - tpos;
            mw[i] = 0.42 + 0.5 * cos(2.0 * WF_PI * tmp / wl) + 0.08 * cos(4.0 * WF_PI * tmp / wl);
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        for (int i = lane; i < m; i += 64) {
            double d;
            if (i == 0) d = -mw[1] / 2.0;
            else if (i == m - 1) d = mw[m - 2] / 2.0;
            else d = -(mw[i + 1] - mw[i - 1]) / 2.0;
            int si = basic + i - 1;
            si = si < 0 ? 0 : (si > L - 1 ? L - 1 : si);
            const double xv = (double)x[si];
            dw[i] = xv * d;
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        for (int i = lane; i < m; i += 64) {
            int si = basic + i - 1;
            si = si < 0 ? 0 : (si > L - 1 ? L - 1 : si);
            mw[i] = (double)x[si] * mw[i];
        }
        __builtin_amdgcn_wave_barrier();
        __threadfence_block();
        double tent = fix_f0(mw, dw, m, n, fs, f0, 2, lane);
        if (tent <= 0.0 || tent > f0 * 2) tent = 0.0;
        else tent = fix_f0(mw, dw, m, n, fs, tent, 6, lane);
        res = (float)(fabs(tent - f0) > f0 * 0.2 ? f0 : tent);
    }
    if (lane == 0) out[(int64_t)r * p.F + f] = res;
}

// torch's F.interpolate(mode='linear', align_corners=False) on float32 rows, as its CPU kernel rounds
__global__ void __launch_bounds__(256) wf_resize_kernel(const float* __restrict__ x, int Lin, float* __restrict__ y, int Lout) {
    const int r = blockIdx.y, i = blockIdx.x * 256 + threadIdx.x;
    if (i >= Lout) return;
    const float* xr = x + (int64_t)r * Lin;
    float v;
    if (Lin == Lout) {
        v = xr[i];
    } else {
        const float scale = (float)Lin / (float)Lout;
        float src = fmaf(scale, (float)i + 0.5f, -0.5f);
        src = src < 0.0f ? 0.0f : src;
        int i0 = (int)floorf(src);
        i0 = i0 < Lin - 1 ? i0 : Lin - 1;
        const int i1 = i0 + (i0 < Lin - 1 ? 1 : 0);
        const float l1 = fminf(fmaxf(src - (float)i0, 0.0f), 1.0f), l0 = 1.0f - l1;
        v = fmaf(xr[i0], l0, xr[i1] * l1);
    }
    y[(int64_t)r * Lout + i] = v;
}

}  // namespace

extern "C" int alive_world_f0_frames(int L8, int fs, double frame_period) {
    if (L8 <= 0 || fs <= 0 || !(frame_period > 0)) return -1;
    return (int)(1000.0 * L8 / fs / frame_period) + 1;
}

extern "C" int alive_world_f0_taps_count(int fs, double f0_floor, double f0_ceil) {
    WfPlan p;
    if (plan(p, 1, 1, fs, f0_floor, f0_ceil, 5.0) != 0) return -1;
    return taps_count(p);
}

extern "C" int alive_world_f0_taps(int fs, double f0_floor, double f0_ceil, double* host_taps) {
    WfPlan p;
    ALIVE_CHECK_ARG(host_taps && plan(p, 1, 1, fs, f0_floor, f0_ceil, 5.0) == 0,
                    "alive_world_f0_taps: bad args (fs %d, f0 range [%g, %g])", fs, f0_floor, f0_ceil);
    const int n = 2 * p.c + 1;
    std::vector<double> hann(n);
    for (int i = 1; i <= n; ++i) hann[i - 1] = 0.5 - 0.5 * cos(i * 2.0 * WF_PI / (n + 1));
    double total = 0.0;
    for (int i = 0; i < n; ++i) total += hann[i];
    for (int i = 0; i < n; ++i) host_taps[i] = -hann[i] / total;
    host_taps[p.c] += 1.0;
    for (int b = 0; b < p.nb; ++b) {
        const int m = 4 * p.h[b];
        double* w = host_taps + p.woff[b];
        for (int i = 0; i < m; ++i) {
            const double t = i / (m - 1.0);
            w[i] = 0.355768 - 0.487396 * cos(2.0 * WF_PI * t) + 0.144232 * cos(4.0 * WF_PI * t) - 0.012604 * cos(6.0 * WF_PI * t);
        }
    }
    return ALIVE_OK;
}

extern "C" size_t alive_world_f0_workspace_bytes(int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period) {
    WfPlan p;
    if (plan(p, N, L8, fs, f0_floor, f0_ceil, frame_period) != 0) return 0;
    return p.total;
}

namespace {

// row_on == nullptr: every row.  stages: how many of the five launches to issue (5: all; fewer only from alive_world_f0_stages)
int world_f0_launch(const char* who, const float* x8, int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period,
                    const double* taps, const int32_t* row_on, float* f0_out, void* ws, size_t ws_bytes, int stages, void* stream) {
    WfPlan p;
    ALIVE_CHECK_ARG(x8 && taps && f0_out && ws, "%s: null pointer", who);
    ALIVE_CHECK_ARG(stages >= 1 && stages <= 5, "%s: %d stages (1 .. 5)", who, stages);
    const int pr = plan(p, N, L8, fs, f0_floor, f0_ceil, frame_period);
    ALIVE_CHECK_ARG(pr == 0, "%s: bad args (N %d, L8 %d, fs %d, f0 range [%g, %g], frame period %g; fs <= 16000, at most "
                    "%d bands, lowest band <= %d taps)", who, N, L8, fs, f0_floor, f0_ceil, frame_period, WF_MAX_BANDS, WF_MAX_NUTTALL);
    ALIVE_CHECK_ARG(ws_bytes >= p.total, "%s: workspace of %zu bytes, %zu needed", who, ws_bytes, p.total);
    ALIVE_CHECK_ARG(2 * p.c + 1 <= 801, "%s: low cut of %d taps exceeds 801", who, 2 * p.c + 1);
    hipStream_t s = (hipStream_t)stream;
    char* w = (char*)ws;
    double* mean = (double*)(w + p.off_mean);
    double* yl = (double*)(w + p.off_yl);
    double* iv = (double*)(w + p.off_iv);
    int* ni = (int*)(w + p.off_ni);
    double* best = (double*)(w + p.off_best);
    double* s1 = (double*)(w + p.off_s1);
    double* s2 = (double*)(w + p.off_s2);
    double* s3 = (double*)(w + p.off_s3);
    wf_mean_kernel<<<N, 256, 0, s>>>(x8, L8, row_on, mean);
    if (stages >= 2) wf_lowcut_kernel<<<dim3(cdiv(p.yl_ld, 256), N), 256, 0, s>>>(x8, mean, taps, L8, p.c, p.yl_ld, row_on, yl);
    if (stages >= 3) wf_bands_kernel<<<dim3(p.nb, N), WF_BT, 0, s>>>(yl, taps, p, row_on, iv, ni);
    if (stages >= 4)
        wf_select_kernel<<<N, 64, 0, s>>>(p, row_on, iv, ni, best, s1, s2, s3, (int*)(w + p.off_pi), (int*)(w + p.off_ng));
    if (stages >= 5) wf_stone_kernel<<<dim3(cdiv(p.F, 2), N), 128, 0, s>>>(x8, p, s3, row_on, f0_out);
    ALIVE_CHECK_LAUNCH(who);
    return ALIVE_OK;
}

}  // namespace

extern "C" int alive_world_f0(const float* x8, int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period,
                              const double* taps, float* f0_out, void* ws, size_t ws_bytes, void* stream) {
    return world_f0_launch("alive_world_f0", x8, N, L8, fs, f0_floor, f0_ceil, frame_period, taps, nullptr, f0_out, ws, ws_bytes,
                           5, stream);
}

// TEST ONLY: alive_world_f0 stopped after the first `stages` of its five launches (mean, low cut, bands, select, StoneMask); the
// buffers of the later stages and, below 5, f0_out are not touched.  alive_world_f0_layout says where the buffers are.
extern "C" int alive_world_f0_stages(const float* x8, int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period,
                                     const double* taps, float* f0_out, void* ws, size_t ws_bytes, int stages, void* stream) {
    return world_f0_launch("alive_world_f0_stages", x8, N, L8, fs, f0_floor, f0_ceil, frame_period, taps, nullptr, f0_out, ws,
                           ws_bytes, stages, stream);
}

// TEST ONLY, host arithmetic: the plan of a call as int64 words (include/alive_vc.h lists them); the count written, or plan()'s
// negative code, or -10 for a missing / short `out`
extern "C" int alive_world_f0_layout(int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period, int64_t* out,
                                     int n_out) {
    WfPlan p;
    const int pr = plan(p, N, L8, fs, f0_floor, f0_ceil, frame_period);
    if (pr != 0) return pr;
    const int n = 16 + 3 * p.nb;
    if (!out || n_out < n) return -10;
    const int64_t head[16] = {p.F, p.nb, p.c, p.Ly, p.yl_ld, (int64_t)p.total, (int64_t)p.off_mean, (int64_t)p.off_yl,
                              (int64_t)p.off_iv, (int64_t)p.off_ni, (int64_t)p.off_best, (int64_t)p.off_s1, (int64_t)p.off_s2,
                              (int64_t)p.off_s3, (int64_t)p.off_pi, (int64_t)p.off_ng};
    for (int i = 0; i < 16; ++i) out[i] = head[i];
    for (int b = 0; b < p.nb; ++b) {
        out[16 + b] = p.h[b];
        out[16 + p.nb + b] = p.woff[b];
        memcpy(&out[16 + 2 * p.nb + b], &p.bound[b], sizeof(double));
    }
    return n;
}

// the rows whose row_on[r] (device int32 [N]) is nonzero: bitwise alive_world_f0 of those rows; the others get 0 (unvoiced) at every
// frame and touch nothing else.  Every kernel tests the row of its block first, so a captured call serves any mask.
extern "C" int alive_world_f0_rows(const float* x8, int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period,
                                   const double* taps, const int32_t* row_on, float* f0_out, void* ws, size_t ws_bytes,
                                   void* stream) {
    ALIVE_CHECK_ARG(row_on, "alive_world_f0_rows: null row mask");
    return world_f0_launch("alive_world_f0_rows", x8, N, L8, fs, f0_floor, f0_ceil, frame_period, taps, row_on, f0_out, ws,
                           ws_bytes, 5, stream);
}

extern "C" int alive_linear_resize(const float* x, int rows, int Lin, float* y, int Lout, void* stream) {
    ALIVE_CHECK_ARG(x && y && rows > 0 && Lin > 0 && Lout > 0, "alive_linear_resize: bad args (rows %d, Lin %d, Lout %d)", rows, Lin, Lout);
    wf_resize_kernel<<<dim3(cdiv(Lout, 256), rows), 256, 0, (hipStream_t)stream>>>(x, Lin, y, Lout);
    ALIVE_CHECK_LAUNCH("alive_linear_resize");
    return ALIVE_OK;
}
