// Pitch tracking (module/common.py: pitch_track, F0Estimator.estimate(track=)): a Viterbi path over the f0 estimator's class scores
// instead of the per-frame argmax.  Per row, with states i = 0 .. S - 1 standing for the classes lo + i, the host tables
// s[i] = 12 log2(lo + i) and [blo[i], bhi[i]] (the states within `band` semitones of i), weight w and jump k:
//   x[t][i]   (double) of logits[n][lo + i][t] with NaN -> -FLT_MAX, else clamped to +-FLT_MAX
//   e[t][i]   x[t][i] - max_j x[t][j]        the frame's scores below its best one (the path does not depend on a frame's constant):
//             a frame that is all NaN or all equal is e = 0 and the path passes through it, where -FLT_MAX + m would round m away
//   D[0][i]   e[0][i]
//   t >= 1:   g = max_j D[t - 1][j] - k                                    gi: the lowest j attaining the max
//             a = max_{j = blo[i] .. bhi[i]} (D[t - 1][j] - w |s[i] - s[j]|)  ai: the lowest j attaining it
//             (m, back[t][i]) = a >= g ? (a, ai) : (g, gi);  D[t][i] = e[t][i] + m
//   p[T - 1] = the lowest i attaining max D[T - 1];  p[t - 1] = back[t][p[t]];  f0[n][t] = (float)(lo + p[t])
// Only + - * abs and compares, all fp64 (-ffp-contract=off): a max is exact and every tie goes to the lowest index, so the order in
// which the candidates are combined does not matter and the result is bitwise tools/pitch_track_ref.py.
//   One block of 1024 threads per row; a row that is off returns at once.  The two score columns D[t - 1] and D[t] are doubles in
//   LDS (2 x 4000 x 8 B = 64000 B: under the 64 KB a kernel gets without an opt-in); up to 2000 states the three tables lie behind
//   them in the same array (4 S doubles in all), so that the band loop reads LDS only.  A band is about 0.23 c states wide at
//   band = 2, so a state's band is spread over the LPS lanes of a lane group, four candidates per lane and step, and the groups take
//   the states round-robin: the LPS-lane groups of a wave hold neighbouring states (bands of nearly the same width) and every wave's
//   states are spread over the whole range.  A row is one block and so one CU: at 1051 states a frame is 1.4e5 candidates of about a
//   dozen instructions each, and that issue time is what a frame costs (DESIGN.md 5.4 "Pitch tracking").
//   The frame loop is sequential with one barrier pair per frame: every thread puts the frame's scores e[t] (loaded into registers
//   during the frame before) into the column of the frame's parity, which nobody has read since the barrier that ended frame t - 1,
//   and asks for those of frame t + 1; barrier; the lane groups turn their states' e into D[t] in place, reading D[t - 1] from the
//   other column, and every wave leaves its (max, argmax) of D[t] and its max of the scores of frame t + 1 in the buffers of the
//   frame's parity; barrier.  (The best score of frame 0 takes a barrier of its own before the loop.)
//   Back pointers (uint16 per row, frame and state) go to the workspace through plain vector stores; one lane traces the path back.
//   No floating-point atomics, no host synchronisation, no allocation: capturable.
#include "common.h"

#include <cfloat>

namespace {

constexpr int MAXS = ALIVE_F0_TRACK_MAX_STATES;
constexpr int THREADS = 1024, WAVES = THREADS / 64;
constexpr int LPS = 8, GROUPS = THREADS / LPS;              // lanes per state; lane groups per block
constexpr int PER = (MAXS + THREADS - 1) / THREADS;         // scores of a frame per thread
constexpr int TAB_MAXS = MAXS / 2;                          // the most states whose tables fit behind the two columns
static_assert(2 * MAXS * sizeof(double) + 2 * WAVES * (2 * sizeof(double) + sizeof(int)) <= 65536, "static LDS");

// the better of two (value, index) candidates: the larger value, the lower index among equals
__device__ __forceinline__ void keep_best(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

__device__ __forceinline__ double score(float x) {
    if (x != x) return (double)-FLT_MAX;
    x = x > FLT_MAX ? FLT_MAX : x;
    x = x < -FLT_MAX ? -FLT_MAX : x;
    return (double)x;
}

// the largest of a wave's scores en[] of one frame (thread tid holds the states tid, tid + THREADS, ..), in every lane
__device__ __forceinline__ double wave_best(const double (&en)[PER], int tid, int S) {
    double em = -__builtin_huge_val();
#pragma unroll
    for (int q = 0; q < PER; ++q)
        if (tid + q * THREADS < S && en[q] > em) em = en[q];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(em, o, 64);
        em = ov > em ? ov : em;
    }
    return em;
}

// TAB: the tables were copied behind the score columns (S <= TAB_MAXS); else they are read where they lie
template <bool TAB>
__global__ __launch_bounds__(THREADS) void f0_track_kernel(const float* __restrict__ logits, int C, int T, int lo, int S,
                                                           const double* __restrict__ semis, const int32_t* __restrict__ band_lo,
                                                           const int32_t* __restrict__ band_hi, const int32_t* __restrict__ on,
                                                           const double* __restrict__ weight, const double* __restrict__ jump,
                                                           float* __restrict__ f0, int32_t* __restrict__ changed,
                                                           unsigned short* __restrict__ back) {
    __shared__ double L[2 * MAXS];                          // D of even frames [S], D of odd frames [S], TAB: s [S], blo [S], bhi [S]
    __shared__ double wv[2][WAVES];
    __shared__ int wi[2][WAVES];
    __shared__ double wm[2][WAVES];                         // every wave's best score of the frame to come
    const int row = blockIdx.x, tid = threadIdx.x;
    if (on && on[row] == 0) return;                         // (block-uniform)
    const int wave = tid >> 6, lane = tid & 63, grp = tid / LPS, sub = tid % LPS;
    const float* x = logits + ((size_t)row * C + lo) * T;
    unsigned short* bk = back + (size_t)row * T * S;
    const double w = weight[row], kj = jump[row];
    const double NEG = -__builtin_huge_val();               // below every score: D is finite
    int* const Lb = reinterpret_cast<int*>(L + 3 * S);      // (TAB) blo [S], then bhi [S]
    if (TAB) {
        for (int i = tid; i < S; i += THREADS) {
            L[2 * S + i] = semis[i];
            Lb[i] = band_lo[i] > 0 ? band_lo[i] : 0;        // (valid tables: no-ops)
            Lb[S + i] = band_hi[i] < S - 1 ? band_hi[i] : S - 1;
        }
    }
    double en[PER];                                         // the scores of the frame to come: states tid, tid + THREADS, ..
#pragma unroll
    for (int q = 0; q < PER; ++q) {
        const int i = tid + q * THREADS;
        en[q] = i < S ? score(x[(size_t)i * T]) : 0.0;
    }
    double em = wave_best(en, tid, S);                      // the best score of the frame to come, in every thread
    if (lane == 0) wm[1][wave] = em;                        // (the parity frame 1 writes next, after the first barrier of frame 1)
    __syncthreads();
    em = wm[1][0];
#pragma unroll
    for (int q = 1; q < WAVES; ++q) em = wm[1][q] > em ? wm[1][q] : em;
    double gv = NEG;                                        // max_j D[t - 1][j] and its lowest j, in every thread
    int gi = 0x7fffffff;
    for (int t = 0; t < T; ++t) {
        const int cur = (t & 1) * S, prev = S - cur;        // the columns of this frame and of the one before
#pragma unroll
        for (int q = 0; q < PER; ++q) {
            const int i = tid + q * THREADS;
            if (i < S) L[cur + i] = en[q] - em;
            if (i < S && t + 1 < T) en[q] = score(x[(size_t)i * T + t + 1]);
        }
        __syncthreads();
        const double g = gv - kj;
        double tv = NEG;                                    // this thread's best new score
        int ti = 0x7fffffff;
        for (int i0 = 0; i0 < S; i0 += GROUPS) {            // (the trip count is block-uniform: the shuffles below need whole waves)
            const int i = i0 + grp;
            const bool live = i < S;
            double d = live ? L[cur + i] : 0.0;
            if (t > 0) {
                double av = NEG;
                int ai = 0x7fffffff;
                if (live) {
                    double si;
                    int b0, b1;
                    if (TAB) {
                        si = L[2 * S + i], b0 = Lb[i], b1 = Lb[S + i];
                    } else {
                        si = semis[i];
                        b0 = band_lo[i] > 0 ? band_lo[i] : 0, b1 = band_hi[i] < S - 1 ? band_hi[i] : S - 1;
                    }
                    for (int j = b0 + sub; j <= b1; j += 4 * LPS) {
                        double c[4];
#pragma unroll
                        for (int u = 0; u < 4; ++u) {       // four candidates in flight; one past the band: a copy of the last, never kept
                            const int ju = j + u * LPS <= b1 ? j + u * LPS : b1;
                            const double df = si - (TAB ? L[2 * S + ju] : semis[ju]);
                            c[u] = L[prev + ju] - w * (df < 0.0 ? -df : df);
                        }
#pragma unroll
                        for (int u = 0; u < 4; ++u)         // ascending j: the first of equals stays
                            if (j + u * LPS <= b1 && c[u] > av) {
                                av = c[u];
                                ai = j + u * LPS;
                            }
                    }
                }
#pragma unroll
                for (int o = LPS / 2; o > 0; o >>= 1) keep_best(av, ai, __shfl_xor(av, o, 64), __shfl_xor(ai, o, 64));
                const bool band = av >= g;
                d = d + (band ? av : g);
                if (live && sub == 0) bk[(size_t)t * S + i] = (unsigned short)(band ? ai : gi);
            }
            if (live && sub == 0) {
                L[cur + i] = d;
                keep_best(tv, ti, d, i);
            }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) keep_best(tv, ti, __shfl_xor(tv, o, 64), __shfl_xor(ti, o, 64));
        em = wave_best(en, tid, S);                         // (past the last frame: the scores of frame T - 1 again, unused)
        if (lane == 0) {
            wv[t & 1][wave] = tv;
            wi[t & 1][wave] = ti;
            wm[t & 1][wave] = em;
        }
        __syncthreads();
        gv = wv[t & 1][0];
        gi = wi[t & 1][0];
#pragma unroll
        for (int q = 1; q < WAVES; ++q) keep_best(gv, gi, wv[t & 1][q], wi[t & 1][q]);
        em = wm[t & 1][0];
#pragma unroll
        for (int q = 1; q < WAVES; ++q) em = wm[t & 1][q] > em ? wm[t & 1][q] : em;
    }
    if (tid == 0) {                                         // (the barrier of the last frame ordered this block's back pointers)
        float* fr = f0 + (size_t)row * T;
        int p = gi, diff = 0;
        for (int t = T - 1; t >= 0; --t) {
            const float v = (float)(lo + p);
            diff += fr[t] != v;
            fr[t] = v;
            if (t > 0) p = bk[(size_t)t * S + p];
        }
        if (changed) changed[row] = diff;
    }
}

}  // namespace

extern "C" size_t alive_f0_track_workspace_bytes(int N, int T, int S) {
    if (N < 1 || T < 1 || S < 1) return 0;
    return align_up((size_t)N * T * S * sizeof(unsigned short), 256);
}

extern "C" int alive_f0_track_rows(const float* logits, int N, int C, int T, int lo, int S, const double* semis, const int32_t* band_lo,
                                   const int32_t* band_hi, const int32_t* on, const double* weight, const double* jump, float* f0,
                                   int32_t* changed, void* ws, void* stream) {
    ALIVE_CHECK_ARG(semis && band_lo && band_hi, "alive_f0_track_rows: null tables");
    ALIVE_CHECK_ARG(logits && weight && jump && f0 && ws, "alive_f0_track_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535, "alive_f0_track_rows: N outside [1, 65535]");
    ALIVE_CHECK_ARG(T >= 1, "alive_f0_track_rows: T < 1");
    ALIVE_CHECK_ARG(S >= 1 && S <= MAXS, "alive_f0_track_rows: %d states outside [1, %d]", S, MAXS);
    ALIVE_CHECK_ARG(lo >= 1, "alive_f0_track_rows: lo < 1 (class 0 is not a state)");
    ALIVE_CHECK_ARG(lo + S <= C, "alive_f0_track_rows: classes [%d, %d] outside the %d class scores", lo, lo + S - 1, C);
    if (S <= TAB_MAXS)
        f0_track_kernel<true><<<N, THREADS, 0, (hipStream_t)stream>>>(logits, C, T, lo, S, semis, band_lo, band_hi, on, weight, jump, f0,
                                                                     changed, (unsigned short*)ws);
    else
        f0_track_kernel<false><<<N, THREADS, 0, (hipStream_t)stream>>>(logits, C, T, lo, S, semis, band_lo, band_hi, on, weight, jump, f0,
                                                                      changed, (unsigned short*)ws);
    ALIVE_CHECK_LAUNCH("alive_f0_track_rows");
    return ALIVE_OK;
}
