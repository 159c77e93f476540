// Voicing decision (module/ops.py: voicing_rows_; Converter.convert(voicing=)): f0 = 0 on the frames of a row whose 16 kHz source is
// not periodic, decided by a normalised cross-correlation that does not look at the f0 estimator at all.
//   launch 1, grid (frame tiles, rows)   voicing_score_kernel    per frame: r = max over the lags of rho, its lowest lag, silent
//   launch 2, one block per row          voicing_decide_kernel   hysteresis, bridge, minimum run (one lane), then the apply
// The arithmetic is fixed by include/alive_vc.h "Voicing" and restated by tools/voicing_ref.py.  The samples are quantised to the
// int16 grid first (q = clamp(rintf(32768 x)), NaN -> 0, 0 outside [0, L)), so Sxy, Sxx, Syy and the frame energy are EXACT integer
// sums (int64; at W <= 4096 nothing exceeds 2^42) and the order in which they are added cannot matter; rho is three fp64 operations,
// each rounded on its own; a max with a lowest-lag tie-break is associative.  So the result is bitwise the restatement whatever the
// partition below.
//   A tile is FRAMES consecutive frames of one row.  Its samples lie in LDS as int16 beside an exact int64 prefix sum of their
//   squares: Sxx and Syy of a lag are two subtractions each, and only Sxy is a loop.  One wave per frame, lanes over the lags: the
//   window of lag tau starts at c - floor((W + tau) / 2), so neighbouring lanes read the same or the next int16 -- two lanes per LDS
//   dword, 64 lanes on 16 or 17 consecutive dwords, which is a broadcast and not a bank conflict (MI355X: 32 banks of 4 B per half
//   wave).  A product of two int16 reaches 2^30 and two of them do not fit 32 bits, so every product is widened to 64 bits before it
//   is added.  The LDS of a tile is dynamic and sized by the call: 19 KB at the defaults beside 2 KB of static LDS, seven tiles per CU.
//   The decision of a row is sequential over its frames and is the work of one lane over the row's bytes in the workspace (two
//   passes); the block's other threads classify the frames before it and apply the decision after it.
// A row that is off returns before any barrier in both launches.  No atomics, no host synchronisation, no allocation: capturable.
#include "common.h"

namespace {

constexpr int THREADS = 256, WAVES = THREADS / 64;
constexpr int FRAMES = WAVES;                                // frames per tile at most: one per wave
constexpr int UNROLL = 8;                                    // products of one lag whose operands are read before the first is used
constexpr int MAX_SPAN = 6000;                               // samples of a tile: 8 (span + 1) + 2 span bytes of dynamic LDS
static_assert((MAX_SPAN + 1) * 8 + MAX_SPAN * 2 + THREADS * 8 <= 65536, "LDS without an opt-in");
static_assert(ALIVE_VOICING_MAX_WINDOW + ALIVE_VOICING_MAX_LAG + 1 <= MAX_SPAN, "the widest frame fits a tile");

// the samples a frame needs on either side of its centre c = hop t + hop / 2: the windows of every lag, and the frame itself
__host__ __device__ inline int ext_lo(int hop, int W, int lag_hi) {
    const int a = (W + lag_hi) / 2, b = hop / 2;
    return a > b ? a : b;
}
__host__ __device__ inline int ext_hi(int hop, int W, int lag_hi) {
    const int a = (W + lag_hi + 1) / 2, b = hop - hop / 2;
    return a > b ? a : b;
}

__device__ __forceinline__ int quantise(float x) {
    const float v = x * 32768.0f;
    if (v != v) return 0;
    return (int)fminf(fmaxf(rintf(v), -32768.0f), 32767.0f);
}

// the better of two (value, lag) candidates: the larger value, the lower lag among equals
__device__ __forceinline__ void keep_best(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

// workspace of N rows of T frames: r double [N][T], lag int32 [N][T], silent then voiced bytes [N][T] each
struct Ws {
    double* r;
    int32_t* lag;
    unsigned char* silent;
    unsigned char* voiced;
    size_t bytes;
    Ws(void* p, int N, int T) {
        Arena a(p);
        const size_t n = (size_t)N * T;
        r = a.take<double>(n);
        lag = a.take<int32_t>(n);
        silent = a.take<unsigned char>(n);
        voiced = a.take<unsigned char>(n);
        bytes = a.used();
    }
};

__global__ __launch_bounds__(THREADS) void voicing_score_kernel(const float* __restrict__ x, int ld, int L, int hop, int T, int lag_lo,
                                                                int lag_hi, int W, int frames, int span,
                                                                const int32_t* __restrict__ on, const double* __restrict__ floor_e,
                                                                double* __restrict__ r_ws, int32_t* __restrict__ lag_ws,
                                                                unsigned char* __restrict__ silent_ws) {
    extern __shared__ __align__(16) unsigned char lds[];
    __shared__ int64_t part[THREADS];
    const int row = blockIdx.y, tid = threadIdx.x;
    if (on && on[row] == 0) return;                         // (block-uniform)
    int64_t* P = reinterpret_cast<int64_t*>(lds);           // P[k] = sum of q[base + j]^2 over j < k, k = 0 .. span
    short* q = reinterpret_cast<short*>(P + span + 1);
    const int t0 = blockIdx.x * frames;
    const int base = hop * t0 + hop / 2 - ext_lo(hop, W, lag_hi);       // the tile's first sample (may be negative)
    const float* xr = x + (size_t)row * ld;
    for (int j = tid; j < span; j += THREADS) {
        const int i = base + j;
        q[j] = (short)((i >= 0 && i < L) ? quantise(xr[i]) : 0);
    }
    __syncthreads();
    const int per = (span + THREADS - 1) / THREADS;         // thread tid owns samples [tid per, tid per + per) of the tile
    const int j0 = min(tid * per, span), j1 = min(j0 + per, span);
    int64_t sum = 0;
    for (int j = j0; j < j1; ++j) sum += (int64_t)((int)q[j] * (int)q[j]);
    part[tid] = sum;
    __syncthreads();
    int64_t run = 0;
    for (int k = 0; k < tid; ++k) run += part[k];
    if (tid == 0) P[0] = 0;
    for (int j = j0; j < j1; ++j) {
        run += (int64_t)((int)q[j] * (int)q[j]);
        P[j + 1] = run;
    }
    __syncthreads();
    const int wave = tid >> 6, lane = tid & 63;
    const int t = t0 + wave;                                // (wave-uniform)
    if (wave >= frames || t >= T) return;
    const int c = hop * wave + ext_lo(hop, W, lag_hi);      // the frame's centre, counted from base
    double bv = -1.0;                                       // below every rho (rho >= 0)
    int bi = 0x7fffffff;
    for (int tau = lag_lo + lane; tau <= lag_hi; tau += 64) {
        const int s = c - ((W + tau) >> 1);                 // 0 <= s and s + tau + W <= span by ext_lo / ext_hi
        const short* qa = q + s;
        const short* qb = qa + tau;
        int64_t sxy = 0;
        int i = 0;
        for (; i + UNROLL <= W; i += UNROLL) {               // UNROLL pairs of LDS reads in flight: one wave per SIMD has no other
            int a[UNROLL], b[UNROLL];                       // way to hide their latency
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) a[u] = qa[i + u], b[u] = qb[i + u];
#pragma unroll
            for (int u = 0; u < UNROLL; ++u) sxy += (int64_t)a[u] * (int64_t)b[u];
        }
        for (; i < W; ++i) sxy += (int64_t)qa[i] * (int64_t)qb[i];
        const int64_t sxx = P[s + W] - P[s], syy = P[s + tau + W] - P[s + tau];
        double rho = 0.0;
        if (sxy > 0 && sxx > 0 && syy > 0) rho = (double)sxy / __dsqrt_rn((double)sxx * (double)syy);
        keep_best(bv, bi, rho, tau);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) keep_best(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
    if (lane == 0) {
        const int e0 = c - hop / 2;                         // the frame [hop t, hop t + hop), counted from base
        const int64_t e = P[e0 + hop] - P[e0];
        const size_t o = (size_t)row * T + t;
        r_ws[o] = bv;
        lag_ws[o] = bv == 0.0 ? lag_lo : bi;
        silent_ws[o] = (double)e < floor_e[row] ? 1 : 0;
    }
}

__global__ __launch_bounds__(THREADS) void voicing_decide_kernel(int T, int min_run, int bridge, const int32_t* __restrict__ on,
                                                                 const double* __restrict__ thr_on, const double* __restrict__ thr_off,
                                                                 float* __restrict__ f0, int ld_f0, const double* __restrict__ r_ws,
                                                                 const int32_t* __restrict__ lag_ws,
                                                                 const unsigned char* __restrict__ silent_ws,
                                                                 unsigned char* __restrict__ voiced_ws, double* __restrict__ r_out,
                                                                 int32_t* __restrict__ lag_out, int32_t* __restrict__ voiced_out,
                                                                 int32_t* __restrict__ changed) {
    __shared__ int cnt[THREADS];
    const int row = blockIdx.x, tid = threadIdx.x;
    if (on && on[row] == 0) return;                         // (block-uniform)
    const size_t o = (size_t)row * T;
    const double* r = r_ws + o;
    const unsigned char* sil = silent_ws + o;
    unsigned char* v = voiced_ws + o;
    const double hi = thr_on[row], lo = thr_off[row];
    // what a frame does to the hysteresis state: 0 clears it, 1 sets it, 2 keeps it
    for (int t = tid; t < T; t += THREADS) v[t] = sil[t] ? 0 : r[t] >= hi ? 1 : r[t] < lo ? 0 : 2;
    __syncthreads();
    if (tid == 0) {
        // (a) hysteresis and (b) bridge in one pass: [u0, t) is the unvoiced run that ends here, quiet: a silent frame lies in it
        int s = 0, u0 = 0, quiet = 0;
        for (int t = 0; t < T; ++t) {
            const int code = v[t];
            s = code == 2 ? s : code;
            v[t] = (unsigned char)s;
            if (s) {
                if (u0 >= 1 && t - u0 >= 1 && t - u0 <= bridge && !quiet)
                    for (int k = u0; k < t; ++k) v[k] = 1;
                u0 = t + 1;
                quiet = 0;
            } else {
                quiet |= sil[t];
            }
        }
        // (c) minimum run: [v0, t) is the voiced run that ends here
        int v0 = 0;
        for (int t = 0; t < T; ++t) {
            if (v[t]) continue;
            if (v0 >= 1 && t - v0 >= 1 && t - v0 < min_run)
                for (int k = v0; k < t; ++k) v[k] = 0;
            v0 = t + 1;
        }
    }
    __syncthreads();
    float* fr = f0 + (size_t)row * ld_f0;
    int n = 0;
    for (int t = tid; t < T; t += THREADS) {
        const int voiced = v[t];
        if (!voiced) {
            n += fr[t] != 0.0f;                             // (a NaN is not zero)
            fr[t] = 0.0f;
        }
        if (r_out) r_out[o + t] = r[t];
        if (lag_out) lag_out[o + t] = lag_ws[o + t];
        if (voiced_out) voiced_out[o + t] = voiced;
    }
    if (!changed) return;                                   // (block-uniform)
    cnt[tid] = n;
    __syncthreads();
    for (int k = THREADS / 2; k > 0; k >>= 1) {
        if (tid < k) cnt[tid] += cnt[tid + k];
        __syncthreads();
    }
    if (tid == 0) changed[row] = cnt[0];
}

}  // namespace

extern "C" size_t alive_voicing_workspace_bytes(int N, int T) {
    if (N < 1 || T < 1) return 0;
    return Ws(nullptr, N, T).bytes;
}

extern "C" int alive_voicing_rows(const float* x, int N, int ld, int L, int hop, int T, int lag_lo, int lag_hi, int W, int min_run,
                                  int bridge, const int32_t* on, const double* thr_on, const double* thr_off, const double* floor_e,
                                  float* f0, int ld_f0, double* r_out, int32_t* lag_out, int32_t* voiced_out, int32_t* changed,
                                  void* ws, void* stream) {
    ALIVE_CHECK_ARG(x && thr_on && thr_off && floor_e && f0 && ws, "alive_voicing_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535, "alive_voicing_rows: N outside [1, 65535]");
    ALIVE_CHECK_ARG(T >= 1 && ld_f0 >= T, "alive_voicing_rows: needs 1 <= T <= ld_f0, got T %d, ld_f0 %d", T, ld_f0);
    ALIVE_CHECK_ARG(0 <= L && L <= ld, "alive_voicing_rows: needs 0 <= L <= ld, got L %d, ld %d", L, ld);
    ALIVE_CHECK_ARG(hop >= 1, "alive_voicing_rows: hop < 1");
    ALIVE_CHECK_ARG(W >= 1 && W <= ALIVE_VOICING_MAX_WINDOW, "alive_voicing_rows: W %d outside [1, %d]", W, ALIVE_VOICING_MAX_WINDOW);
    ALIVE_CHECK_ARG(1 <= lag_lo && lag_lo <= lag_hi && lag_hi <= ALIVE_VOICING_MAX_LAG,
                    "alive_voicing_rows: needs 1 <= lag_lo <= lag_hi <= %d, got [%d, %d]", ALIVE_VOICING_MAX_LAG, lag_lo, lag_hi);
    ALIVE_CHECK_ARG(min_run >= 0 && bridge >= 0, "alive_voicing_rows: min_run %d or bridge %d below 0", min_run, bridge);
    const int64_t ext = (int64_t)ext_lo(hop, W, lag_hi) + ext_hi(hop, W, lag_hi);
    ALIVE_CHECK_ARG(ext <= MAX_SPAN, "alive_voicing_rows: a frame spans %lld samples (hop %d, W %d, lag_hi %d), at most %d",
                    (long long)ext, hop, W, lag_hi, MAX_SPAN);
    ALIVE_CHECK_ARG((int64_t)hop * T + MAX_SPAN < (int64_t)1 << 31, "alive_voicing_rows: hop * T does not fit 32 bits");
    ALIVE_CHECK_ARG((int64_t)N * T < (int64_t)1 << 31, "alive_voicing_rows: N * T does not fit 32 bits");
    int frames = 1 + (int)((MAX_SPAN - ext) / hop);         // the frames whose samples fit one tile, one per wave at most
    frames = frames < FRAMES ? frames : FRAMES;
    frames = frames < T ? frames : T;
    const int span = (int)ext + (frames - 1) * hop;
    const size_t lds = (size_t)(span + 1) * 8 + align_up((size_t)span * 2, 8);
    const Ws w(ws, N, T);
    voicing_score_kernel<<<dim3(cdiv(T, frames), N), THREADS, lds, (hipStream_t)stream>>>(x, ld, L, hop, T, lag_lo, lag_hi, W, frames,
                                                                                         span, on, floor_e, w.r, w.lag, w.silent);
    ALIVE_CHECK_LAUNCH("alive_voicing_rows (scores)");
    voicing_decide_kernel<<<N, THREADS, 0, (hipStream_t)stream>>>(T, min_run, bridge, on, thr_on, thr_off, f0, ld_f0, w.r, w.lag,
                                                                 w.silent, w.voiced, r_out, lag_out, voiced_out, changed);
    ALIVE_CHECK_LAUNCH("alive_voicing_rows (decision)");
    return ALIVE_OK;
}
