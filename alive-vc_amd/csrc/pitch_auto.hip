// Auto pitch: the source's register measured on the device and turned into a pitch shift towards the target voice's register, without a
// host read (module/multistream.py: MultiStreamConverter(auto_pitch=True); module/pipeline.py: convert_many(auto_pitch=...)).
//   pitch statistics of row groups                alive_pitch_stats_groups   (offline: one group per utterance; enrolment: one group)
//   per-utterance shift, expanded to the windows  alive_pitch_shift_groups
//   streaming: running register + shift per row   alive_pitch_follow_rows
// Pitch range (the second moment; MultiStreamConverter(pitch_range=True), convert_many(auto_range=...)): the source's pitch variance beside
// its mean, an intonation factor that scales the excursions around a centre it is given, and with auto range the factor that maps the
// source's standard deviation onto the target voice's (the mean-variance transform of log-f0).
//   (sum, count, sum of squares) of row groups    alive_pitch_stats2_groups
//   per-utterance intonation and centre           alive_pitch_range_groups
//   streaming: (S, W, Q) + shift, intonation, centre per row   alive_pitch_follow2_rows
//   the transform around a given centre           alive_pitch_transform_rows_centred
// Every fp64 operation of these is one of + - * / sqrt, each rounded on its own (-ffp-contract=off), so a host restatement in the same
// order (tools/pitch_range_ref.py) agrees bit for bit.
// "pitch" is the reference's 12*log2(f0/440) - 9 (inference.py:119) exactly as blocks.hip's pitch_kernel forms it: log2 in fp64, rounded
// once to float32; a frame is voiced when that value is finite (inference.py:121), so class 0, NaN and inf are unvoiced.  Every sum is in
// fp64 in a FIXED order -- thread tid of a row takes frames tid, tid + 256, ..., then pitch_kernel's tree over the 256 partial sums, then
// the rows of a group in index order -- with no floating-point atomics: results are bitwise reproducible, a group's result does not depend
// on the other groups of the call, and a one-row group's (float)(sum / count) is bitwise pitch_kernel's mode-0 mean of that row.
#include "common.h"

#include <cmath>

namespace {

__device__ __forceinline__ float pitch_of(float f0) { return 12.0f * (float)log2((double)(f0 / 440.0f)) - 9.0f; }

// (sum, count) of the voiced pitch of f[t] * scale (SCALED) or f[t], t in [t_lo, t_hi): pitch_kernel's per-thread order and tree.  Every
// thread of the block calls it; the result is valid in s_sum[0] / s_cnt[0] after it returns (a barrier has passed).
template <bool SCALED>
__device__ __forceinline__ void row_stats(const float* __restrict__ f, int t_lo, int t_hi, float scale, double* s_sum, int* s_cnt) {
    const int tid = threadIdx.x;
    double sum = 0.0;
    int cnt = 0;
    for (int t = t_lo + tid; t < t_hi; t += 256) {
        float x = f[t];
        if constexpr (SCALED) x = x * scale;
        const float p = pitch_of(x);
        if (!isinf(p) && !isnan(p)) { sum += (double)p; ++cnt; }
    }
    s_sum[tid] = sum;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
        __syncthreads();
    }
}

// One block per group: its rows one after the other (each a full-block tree), added in index order by thread 0.
__global__ __launch_bounds__(256) void pitch_stats_groups_kernel(const float* __restrict__ f0, int N, int T, int t_lo, int t_hi,
                                                                 const int* __restrict__ first, double* __restrict__ stats) {
    __shared__ double s_sum[256];
    __shared__ int s_cnt[256];
    const int g = blockIdx.x;
    int r0 = first[g], r1 = first[g + 1];
    r0 = r0 < 0 ? 0 : r0;                                   // (a bad table reads no row outside f0)
    r1 = r1 > N ? N : r1;
    double sum = 0.0, cnt = 0.0;
    for (int r = r0; r < r1; ++r) {
        row_stats<false>(f0 + (size_t)r * T, t_lo, t_hi, 1.0f, s_sum, s_cnt);
        if (threadIdx.x == 0) { sum += s_sum[0]; cnt += (double)s_cnt[0]; }
        __syncthreads();                                    // s_sum[0] is read before the next row overwrites it
    }
    if (threadIdx.x == 0) {
        stats[2 * g] = sum;
        stats[2 * g + 1] = cnt;
    }
}

// One block per group: shift of its rows = offset (+ target - the group's mean pitch, in float32, on an auto group that has voiced frames)
__global__ __launch_bounds__(64) void pitch_shift_groups_kernel(const double* __restrict__ stats, const int* __restrict__ first, int N,
                                                               const float* __restrict__ offset, const int* __restrict__ auto_on,
                                                               const float* __restrict__ target, float* __restrict__ shift_out) {
    const int g = blockIdx.x;
    int r0 = first[g], r1 = first[g + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > N ? N : r1;
    float shift = offset[g];
    if (auto_on[g] != 0) {
        const double sum = stats[2 * g], cnt = stats[2 * g + 1];
        if (cnt != 0.0) shift = shift + (target[g] - (float)(sum / cnt));
    }
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 64) shift_out[r] = shift;
}

// One block per row (session): the running register (S, W) of the row's source and the shift the mode-1 transform then adds.
__global__ __launch_bounds__(256) void pitch_follow_rows_kernel(const float* __restrict__ f0, int T, const float* __restrict__ f0_rate,
                                                                const float* __restrict__ offset, const int* __restrict__ auto_on,
                                                                const float* __restrict__ target, const unsigned char* __restrict__ emit,
                                                                double decay, double prior, double* __restrict__ state,
                                                                float* __restrict__ shift_out) {
    __shared__ double s_sum[256];
    __shared__ int s_cnt[256];
    const int n = blockIdx.x;
    const float off = offset[n];
    if (auto_on[n] == 0) {                                  // (block-uniform)
        if (threadIdx.x == 0) shift_out[n] = off;           // bit for bit; the state is not touched
        return;
    }
    const bool update = emit[n] != 0;                       // (block-uniform: the barriers below are reached by all threads or none)
    if (update) row_stats<true>(f0 + (size_t)n * T, 0, T, f0_rate[n], s_sum, s_cnt);
    if (threadIdx.x == 0) {
        double S = state[2 * n], W = state[2 * n + 1];
        if (update) {
            S = decay * S + s_sum[0];
            W = decay * W + (double)s_cnt[0];
            state[2 * n] = S;
            state[2 * n + 1] = W;
        }
        float a = 0.0f;                                     // exactly 0 before any voiced frame (W == 0, whatever the prior)
        if (W != 0.0) a = (float)(W / (W + prior) * ((double)target[n] - S / W));
        shift_out[n] = off + a;
    }
}

// row_stats with the sum of squares beside the sum: the same per-thread order and tree, so s_sum[0] / s_cnt[0] are bitwise row_stats'.
// (double)p * (double)p is exact: a float32 has 24 significant bits.
template <bool SCALED>
__device__ __forceinline__ void row_stats2(const float* __restrict__ f, int t_lo, int t_hi, float scale, double* s_sum, double* s_sq,
                                           int* s_cnt) {
    const int tid = threadIdx.x;
    double sum = 0.0, sq = 0.0;
    int cnt = 0;
    for (int t = t_lo + tid; t < t_hi; t += 256) {
        float x = f[t];
        if constexpr (SCALED) x = x * scale;
        const float p = pitch_of(x);
        if (!isinf(p) && !isnan(p)) { sum += (double)p; sq += (double)p * (double)p; ++cnt; }
    }
    s_sum[tid] = sum;
    s_sq[tid] = sq;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (tid < o) { s_sum[tid] += s_sum[tid + o]; s_sq[tid] += s_sq[tid + o]; s_cnt[tid] += s_cnt[tid + o]; }
        __syncthreads();
    }
}

// The range factor target_sd / sqrt(v) clamped to [1 / range_max, range_max]; 1 when there is no usable variance or target.
__device__ __forceinline__ double range_factor(double v, double sd, double range_max) {
    if (!(v > 0.0) || !(sd > 0.0) || isinf(v) || isinf(sd)) return 1.0;     // (NaN fails both comparisons)
    double r = sd / __dsqrt_rn(v);
    const double lo = 1.0 / range_max;
    r = r < lo ? lo : r;
    r = r > range_max ? range_max : r;
    return r;
}

// pitch_stats_groups_kernel with the third sum
__global__ __launch_bounds__(256) void pitch_stats2_groups_kernel(const float* __restrict__ f0, int N, int T, int t_lo, int t_hi,
                                                                  const int* __restrict__ first, double* __restrict__ stats3) {
    __shared__ double s_sum[256];
    __shared__ double s_sq[256];
    __shared__ int s_cnt[256];
    const int g = blockIdx.x;
    int r0 = first[g], r1 = first[g + 1];
    r0 = r0 < 0 ? 0 : r0;                                   // (a bad table reads no row outside f0)
    r1 = r1 > N ? N : r1;
    double sum = 0.0, cnt = 0.0, sq = 0.0;
    for (int r = r0; r < r1; ++r) {
        row_stats2<false>(f0 + (size_t)r * T, t_lo, t_hi, 1.0f, s_sum, s_sq, s_cnt);
        if (threadIdx.x == 0) { sum += s_sum[0]; cnt += (double)s_cnt[0]; sq += s_sq[0]; }
        __syncthreads();                                    // the three [0] entries are read before the next row overwrites them
    }
    if (threadIdx.x == 0) {
        stats3[3 * g] = sum;
        stats3[3 * g + 1] = cnt;
        stats3[3 * g + 2] = sq;
    }
}

// One block per group: the intonation, centre and centre switch of its rows
__global__ __launch_bounds__(64) void pitch_range_groups_kernel(const double* __restrict__ stats3, const int* __restrict__ first, int N,
                                                               const float* __restrict__ inton, const int* __restrict__ range_on,
                                                               const double* __restrict__ target_sd, double range_max,
                                                               float* __restrict__ inton_out, float* __restrict__ centre_out,
                                                               int* __restrict__ centre_on_out) {
    const int g = blockIdx.x;
    int r0 = first[g], r1 = first[g + 1];
    r0 = r0 < 0 ? 0 : r0;
    r1 = r1 > N ? N : r1;
    float I = inton[g], c = 0.0f;
    int on = 0;
    const double sum = stats3[3 * g], cnt = stats3[3 * g + 1], sq = stats3[3 * g + 2];
    if (range_on[g] != 0 && cnt > 0.0) {
        const double m = sum / cnt;
        const double v = sq / cnt - m * m;
        I = (float)((double)I * range_factor(v, target_sd[g], range_max));
        c = (float)m;
        on = 1;
    }
    for (int r = r0 + (int)threadIdx.x; r < r1; r += 64) {
        inton_out[r] = I;
        centre_out[r] = c;
        centre_on_out[r] = on;
    }
}

// pitch_follow_rows_kernel on (S, W, Q): one block per row; S, W and the shift are bitwise that kernel's on an auto row.
__global__ __launch_bounds__(256) void pitch_follow2_rows_kernel(const float* __restrict__ f0, int T, const float* __restrict__ f0_rate,
                                                                 const float* __restrict__ offset, const int* __restrict__ auto_on,
                                                                 const float* __restrict__ target, const float* __restrict__ inton,
                                                                 const int* __restrict__ range_on, const double* __restrict__ target_sd,
                                                                 const unsigned char* __restrict__ emit, double decay, double prior,
                                                                 double range_max, double* __restrict__ state3,
                                                                 float* __restrict__ shift_out, float* __restrict__ inton_out,
                                                                 float* __restrict__ centre_out, int* __restrict__ centre_on_out) {
    __shared__ double s_sum[256];
    __shared__ double s_sq[256];
    __shared__ int s_cnt[256];
    const int n = blockIdx.x;
    const float off = offset[n];
    const bool is_auto = auto_on[n] != 0, ranged = range_on[n] != 0;
    const float I0 = inton[n];
    if (!(is_auto || ranged || I0 != 1.0f)) {               // (block-uniform)
        if (threadIdx.x == 0) {                             // the state is not touched
            shift_out[n] = off;                             // bit for bit
            inton_out[n] = 1.0f;
            centre_out[n] = 0.0f;
            centre_on_out[n] = 0;
        }
        return;
    }
    const bool update = emit[n] != 0;                       // (block-uniform: the barriers below are reached by all threads or none)
    if (update) row_stats2<true>(f0 + (size_t)n * T, 0, T, f0_rate[n], s_sum, s_sq, s_cnt);
    if (threadIdx.x == 0) {
        double S = state3[3 * n], W = state3[3 * n + 1], Q = state3[3 * n + 2];
        if (update) {
            S = decay * S + s_sum[0];
            W = decay * W + (double)s_cnt[0];
            Q = decay * Q + s_sq[0];
            state3[3 * n] = S;
            state3[3 * n + 1] = W;
            state3[3 * n + 2] = Q;
        }
        float shift = off, I = 1.0f, c = 0.0f;              // the automatic parts exactly 0 before any voiced frame (W == 0)
        if (W != 0.0) {
            const double a = W / (W + prior);
            const double m = S / W;
            double r = 1.0;
            if (ranged) r = range_factor(Q / W - m * m, target_sd[n], range_max);
            const double Ie = (double)I0 * r;
            I = (float)(1.0 + a * (Ie - 1.0));
            c = (float)m;
            if (is_auto) shift = off + (float)(a * ((double)target[n] - m));
        }
        shift_out[n] = shift;
        inton_out[n] = I;
        centre_out[n] = c;
        centre_on_out[n] = (I != 1.0f) ? 1 : 0;
    }
}

// blocks.hip's pitch_kernel with per-row parameters and a per-row centre: a row with centre_on == 0 runs that kernel's arithmetic
// (mode 0: around its own window mean; mode 1: p + shift), a row with centre_on != 0 scales its excursions around centre[n] in
// either mode.  centre_on[n] is block-uniform, so every barrier is reached by all threads of a block or by none.
__global__ __launch_bounds__(256) void pitch_centred_kernel(float* f0, int T, int mode, const float* __restrict__ rate_r,
                                                            const float* __restrict__ shift_r, const float* __restrict__ inton_r,
                                                            const float* __restrict__ centre_r, const int* __restrict__ centre_on) {
    __shared__ double s_sum[256];
    __shared__ int s_cnt[256];
    const float f0_rate = rate_r[blockIdx.x], shift = shift_r[blockIdx.x], inton = inton_r[blockIdx.x];
    const bool centred = centre_on[blockIdx.x] != 0;
    float* f = f0 + (size_t)blockIdx.x * T;
    const int tid = threadIdx.x;
    float mean = 0.0f;
    if (centred) {
        mean = centre_r[blockIdx.x];
    } else if (mode == 0) {
        row_stats<false>(f, 0, T, 1.0f, s_sum, s_cnt);
        mean = (float)(s_sum[0] / (double)s_cnt[0]);
    }
    for (int t = tid; t < T; t += 256) {
        float x = f[t];
        if (mode == 1) x = x * f0_rate;
        float p = pitch_of(x);
        if (mode == 0 || centred) p = mean + (p - mean) * inton + shift;
        else p = p + shift;
        const float e = (p + 9.0f) / 12.0f;
        float y = 440.0f * (float)exp2((double)e);
        if (isnan(y) || isinf(y)) y = 0.0f;
        if (mode == 0) y = y * f0_rate;
        f[t] = y;
    }
}

}  // namespace

extern "C" int alive_pitch_stats_groups(const float* f0, int N, int T, int t_lo, int t_hi, const int* first, int G, double* stats,
                                        void* stream) {
    ALIVE_CHECK_ARG(f0 && first && stats, "alive_pitch_stats_groups: null pointer");
    ALIVE_CHECK_ARG(N > 0 && T > 0 && G > 0, "alive_pitch_stats_groups: bad args");
    ALIVE_CHECK_ARG(0 <= t_lo && t_lo <= t_hi && t_hi <= T, "alive_pitch_stats_groups: frames [%d, %d) outside [0, %d)", t_lo, t_hi, T);
    pitch_stats_groups_kernel<<<G, 256, 0, (hipStream_t)stream>>>(f0, N, T, t_lo, t_hi, first, stats);
    ALIVE_CHECK_LAUNCH("alive_pitch_stats_groups");
    return ALIVE_OK;
}

extern "C" int alive_pitch_shift_groups(const double* stats, const int* first, int G, int N, const float* offset, const int* auto_on,
                                        const float* target, float* shift_out, void* stream) {
    ALIVE_CHECK_ARG(stats && first && offset && auto_on && target && shift_out, "alive_pitch_shift_groups: null pointer");
    ALIVE_CHECK_ARG(N > 0 && G > 0, "alive_pitch_shift_groups: bad args");
    pitch_shift_groups_kernel<<<G, 64, 0, (hipStream_t)stream>>>(stats, first, N, offset, auto_on, target, shift_out);
    ALIVE_CHECK_LAUNCH("alive_pitch_shift_groups");
    return ALIVE_OK;
}

extern "C" int alive_pitch_follow_rows(const float* f0, int N, int T, const float* f0_rate, const float* offset, const int* auto_on,
                                       const float* target, const unsigned char* emit, double decay, double prior, double* state,
                                       float* shift_out, void* stream) {
    ALIVE_CHECK_ARG(f0 && f0_rate && offset && auto_on && target && emit && state && shift_out, "alive_pitch_follow_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && T > 0, "alive_pitch_follow_rows: bad args");
    ALIVE_CHECK_ARG(decay >= 0.0 && decay <= 1.0 && prior >= 0.0, "alive_pitch_follow_rows: decay %g outside [0, 1] or prior %g < 0", decay,
                    prior);
    pitch_follow_rows_kernel<<<N, 256, 0, (hipStream_t)stream>>>(f0, T, f0_rate, offset, auto_on, target, emit, decay, prior, state,
                                                                 shift_out);
    ALIVE_CHECK_LAUNCH("alive_pitch_follow_rows");
    return ALIVE_OK;
}

extern "C" int alive_pitch_stats2_groups(const float* f0, int N, int T, int t_lo, int t_hi, const int* first, int G, double* stats3,
                                         void* stream) {
    ALIVE_CHECK_ARG(f0 && first && stats3, "alive_pitch_stats2_groups: null pointer");
    ALIVE_CHECK_ARG(N > 0 && T > 0 && G > 0, "alive_pitch_stats2_groups: bad args");
    ALIVE_CHECK_ARG(0 <= t_lo && t_lo <= t_hi && t_hi <= T, "alive_pitch_stats2_groups: frames [%d, %d) outside [0, %d)", t_lo, t_hi, T);
    pitch_stats2_groups_kernel<<<G, 256, 0, (hipStream_t)stream>>>(f0, N, T, t_lo, t_hi, first, stats3);
    ALIVE_CHECK_LAUNCH("alive_pitch_stats2_groups");
    return ALIVE_OK;
}

extern "C" int alive_pitch_range_groups(const double* stats3, const int* first, int G, int N, const float* inton, const int* range_on,
                                        const double* target_sd, double range_max, float* inton_out, float* centre_out,
                                        int* centre_on_out, void* stream) {
    ALIVE_CHECK_ARG(stats3 && first && inton && range_on && target_sd && inton_out && centre_out && centre_on_out,
                    "alive_pitch_range_groups: null pointer");
    ALIVE_CHECK_ARG(N > 0 && G > 0, "alive_pitch_range_groups: bad args");
    ALIVE_CHECK_ARG(std::isfinite(range_max) && range_max >= 1.0, "alive_pitch_range_groups: range_max %g must be finite and >= 1",
                    range_max);
    pitch_range_groups_kernel<<<G, 64, 0, (hipStream_t)stream>>>(stats3, first, N, inton, range_on, target_sd, range_max, inton_out,
                                                                 centre_out, centre_on_out);
    ALIVE_CHECK_LAUNCH("alive_pitch_range_groups");
    return ALIVE_OK;
}

extern "C" int alive_pitch_follow2_rows(const float* f0, int N, int T, const float* f0_rate, const float* offset, const int* auto_on,
                                        const float* target, const float* inton, const int* range_on, const double* target_sd,
                                        const unsigned char* emit, double decay, double prior, double range_max, double* state3,
                                        float* shift_out, float* inton_out, float* centre_out, int* centre_on_out, void* stream) {
    ALIVE_CHECK_ARG(f0 && f0_rate && offset && auto_on && target && inton && range_on && target_sd && emit && state3 && shift_out &&
                        inton_out && centre_out && centre_on_out,
                    "alive_pitch_follow2_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && T > 0, "alive_pitch_follow2_rows: bad args");
    ALIVE_CHECK_ARG(decay >= 0.0 && decay <= 1.0 && prior >= 0.0, "alive_pitch_follow2_rows: decay %g outside [0, 1] or prior %g < 0", decay,
                    prior);
    ALIVE_CHECK_ARG(std::isfinite(range_max) && range_max >= 1.0, "alive_pitch_follow2_rows: range_max %g must be finite and >= 1",
                    range_max);
    pitch_follow2_rows_kernel<<<N, 256, 0, (hipStream_t)stream>>>(f0, T, f0_rate, offset, auto_on, target, inton, range_on, target_sd, emit,
                                                                  decay, prior, range_max, state3, shift_out, inton_out, centre_out,
                                                                  centre_on_out);
    ALIVE_CHECK_LAUNCH("alive_pitch_follow2_rows");
    return ALIVE_OK;
}

extern "C" int alive_pitch_transform_rows_centred(float* f0, int N, int T, int mode, const float* f0_rate, const float* shift,
                                                  const float* inton, const float* centre, const int* centre_on, void* stream) {
    ALIVE_CHECK_ARG(f0 && f0_rate && shift && inton && centre && centre_on, "alive_pitch_transform_rows_centred: null pointer");
    ALIVE_CHECK_ARG(N > 0 && T > 0 && (mode == 0 || mode == 1), "alive_pitch_transform_rows_centred: bad args");
    pitch_centred_kernel<<<N, 256, 0, (hipStream_t)stream>>>(f0, T, mode, f0_rate, shift, inton, centre, centre_on);
    ALIVE_CHECK_LAUNCH("alive_pitch_transform_rows_centred");
    return ALIVE_OK;
}
