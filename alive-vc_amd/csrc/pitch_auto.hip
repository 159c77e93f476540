// Auto pitch: the source's register measured on the device and turned into a pitch shift towards the target voice's register, without a
// host read (module/multistream.py: MultiStreamConverter(auto_pitch=True); module/pipeline.py: convert_many(auto_pitch=...)).
//   pitch statistics of row groups                alive_pitch_stats_groups   (offline: one group per utterance; enrolment: one group)
//   per-utterance shift, expanded to the windows  alive_pitch_shift_groups
//   streaming: running register + shift per row   alive_pitch_follow_rows
// "pitch" is the reference's 12*log2(f0/440) - 9 (inference.py:119) exactly as blocks.hip's pitch_kernel forms it: log2 in fp64, rounded
// once to float32; a frame is voiced when that value is finite (inference.py:121), so class 0, NaN and inf are unvoiced.  Every sum is in
// fp64 in a FIXED order -- thread tid of a row takes frames tid, tid + 256, ..., then pitch_kernel's tree over the 256 partial sums, then
// the rows of a group in index order -- with no floating-point atomics: results are bitwise reproducible, a group's result does not depend
// on the other groups of the call, and a one-row group's (float)(sum / count) is bitwise pitch_kernel's mode-0 mean of that row.
#include "common.h"

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
