// Lost-chunk concealment at the input edge of a sparse MultiStreamConverter (module/multistream.py "Lost chunks"): a session whose
// chunk never arrived, while its clock must go on, has the hole in its int16 ring filled by waveform substitution (G.711 Appendix I
// style) instead of zeros.  alive_conceal_rows runs in FRONT of alive_ring_push_rows, once per tick and only on a tick that has a lost
// or a recovering row: it rewrites those rows of the uploaded chunk buffer in place, the push then moves them into the rings as if
// they had arrived.  tools/conceal_ref.py restates it bit for bit.
//   one block per row:  lost, first of a run   the newest max(W + lag_hi, 2 lag_hi) ring samples -> LDS as int16, once; thread t takes
//                                              the lags lag_lo + t, + 256, ...: C(l) and E(l) in int64 over the 20 ms window (at step i
//                                              the lanes of a wave read consecutive int16 of the ring image, two lanes per bank word, and
//                                              one broadcast word of the window: conflict-free), score C^2 / E in fp64; the argmax goes
//                                              through LDS, the lowest lag wins a tie; the template (the last period, its last quarter
//                                              faded into the period before) -> LDS and the row of tmpl
//                       lost, later            the template comes back from tmpl: the ring, which now holds made-up samples, is not read
//                       lost                   chunk[i] = rint(t[(q + i) mod P] att(q + i)); state (q + cl, P)
//                       recovering             the head of the real chunk faded in from the continuation; state (0, 0)
//                       lost, on == 0          zeros; state (0, 0)
// Integer sums and fp64 operations rounded one by one (-ffp-contract=off): the device and NumPy agree bit for bit.  Plain C++, vector
// memory stores only, no atomics; 16-byte stores where the chunk length and the stride are multiples of 8 samples, scalar ones otherwise.
#include "common.h"

namespace {

constexpr int CONCEAL_THREADS = 256;
constexpr int SPAN = ALIVE_CONCEAL_MAX_SPAN;

__device__ __forceinline__ double conceal_att(int64_t k, int hold, int fade) {
    const int64_t d = (int64_t)hold + fade - k;
    return d <= 0 ? 0.0 : d >= fade ? 1.0 : (double)d / (double)fade;
}

// the unrounded continuation at sample i of the chunk: t[(q + i) mod P] att(q + i); qm = q mod P
__device__ __forceinline__ double conceal_cont(const short* t, int P, int qm, int q, int i, int hold, int fade) {
    return (double)t[(qm + i) % P] * conceal_att((int64_t)q + i, hold, fade);
}

__device__ __forceinline__ short conceal_blend(double s, short c, int i, int rec) {
    double v = rint(s + (((double)c - s) * (double)(i + 1)) / (double)(rec + 1));
    v = v < -32768.0 ? -32768.0 : v > 32767.0 ? 32767.0 : v;
    return (short)(int)v;
}

__device__ __forceinline__ uint4 pack8(const short* v) {
    uint4 p;
    p.x = (unsigned)(unsigned short)v[0] | ((unsigned)(unsigned short)v[1] << 16);
    p.y = (unsigned)(unsigned short)v[2] | ((unsigned)(unsigned short)v[3] << 16);
    p.z = (unsigned)(unsigned short)v[4] | ((unsigned)(unsigned short)v[5] << 16);
    p.w = (unsigned)(unsigned short)v[6] | ((unsigned)(unsigned short)v[7] << 16);
    return p;
}

__global__ __launch_bounds__(CONCEAL_THREADS) void conceal_rows_kernel(
    const short* __restrict__ ring, int ld, const int* __restrict__ ring_len, short* __restrict__ chunks, int ld_chunk,
    const int* __restrict__ chunk_len, const unsigned char* __restrict__ present, const unsigned char* __restrict__ lost,
    const unsigned char* __restrict__ on, const int* __restrict__ lag_lo, const int* __restrict__ lag_hi, const int* __restrict__ window,
    const int* __restrict__ hold, const int* __restrict__ fade, const int* __restrict__ recover, int* __restrict__ state,
    short* __restrict__ tmpl, int ld_tmpl, int vec_ok) {
    __shared__ short xs[SPAN];                               // the newest `need` ring samples, oldest first
    __shared__ short ts[SPAN / 2];                           // the template (P <= lag_hi <= need / 2)
    __shared__ double best_sc[CONCEAL_THREADS];
    __shared__ int best_lag[CONCEAL_THREADS];
    const int n = blockIdx.x, tid = threadIdx.x;
    // everything below is block-uniform; the state is read by every thread here and written by thread 0 behind a barrier
    if (present[n] == 0) return;                             // absent (a stall): nothing of the row moves
    const bool is_lost = lost[n] != 0;
    const int q = state[2 * n], P0 = state[2 * n + 1];
    if (!is_lost && q <= 0) return;                          // neither lost nor recovering: nothing read, nothing written
    const int cl = chunk_len[n], rl = ring_len[n];
    const int lo = lag_lo[n], hi = lag_hi[n], w = window[n], hd = hold[n], fd = fade[n], rc = recover[n];
    // a row takes part if its lengths fit the strides and its ring holds what its lags need; device data never leads outside a row
    if (cl < 1 || cl > ld_chunk || rl < 1 || rl > ld || cl > rl) return;
    if (lo < 1 || hi < lo || hi > ld_tmpl || hi > SPAN / 2 || w < 1 || w > SPAN) return;
    if (fd < 1 || fd > ALIVE_CONCEAL_QMAX || hd < 0 || hd > ALIVE_CONCEAL_QMAX || rc < 0) return;
    const int need = w + hi > 2 * hi ? w + hi : 2 * hi;
    if (need > rl || need > SPAN) return;
    if (q < 0 || (q > 0 && (P0 < 1 || P0 > hi))) return;     // (a state no run of this kernel leaves behind)
    short* c = chunks + (size_t)n * ld_chunk;
    short* tg = tmpl + (size_t)n * ld_tmpl;
    const bool vec = vec_ok && (cl & 7) == 0;

    if (is_lost && on[n] == 0) {                             // concealment off: the lost chunk is a chunk of zeros
        if (vec) {
            for (int g = tid * 8; g < cl; g += CONCEAL_THREADS * 8) *reinterpret_cast<uint4*>(c + g) = make_uint4(0u, 0u, 0u, 0u);
        } else {
            for (int i = tid; i < cl; i += CONCEAL_THREADS) c[i] = 0;
        }
        __syncthreads();
        if (tid == 0) state[2 * n] = state[2 * n + 1] = 0;
        return;
    }

    int P = P0;
    if (q == 0) {                                            // the first lost chunk of a run: the period and the template, once
        const short* r = ring + (size_t)n * ld + (rl - need);
        for (int k = tid; k < need; k += CONCEAL_THREADS) xs[k] = r[k];
        __syncthreads();
        const int a0 = need - w;                             // the window a[i] = xs[a0 + i]; lag l reads xs[a0 - l + i] (a0 - hi >= 0)
        double bs = -1.0;
        int bl = 0x7fffffff;
        for (int l = lo + tid; l <= hi; l += CONCEAL_THREADS) {
            const short* y = xs + (a0 - l);
            int64_t C = 0, E = 0;
#pragma unroll 4
            for (int i = 0; i < w; ++i) {
                const int b = y[i];
                C += (int64_t)xs[a0 + i] * b;
                E += (int64_t)b * b;
            }
            const double sc = (C > 0 && E > 0) ? ((double)C * (double)C) / (double)E : 0.0;
            if (sc > bs) {                                   // (ascending lags: the lowest of equal scores stays)
                bs = sc;
                bl = l;
            }
        }
        best_sc[tid] = bs;
        best_lag[tid] = bl;
        __syncthreads();
        for (int o = CONCEAL_THREADS / 2; o > 0; o >>= 1) {
            if (tid < o) {
                const double s2 = best_sc[tid + o];
                const int l2 = best_lag[tid + o];
                if (s2 > best_sc[tid] || (s2 == best_sc[tid] && l2 < best_lag[tid])) {
                    best_sc[tid] = s2;
                    best_lag[tid] = l2;
                }
            }
            __syncthreads();
        }
        P = best_lag[0];                                     // (thread 0 always has lag lo: lo <= P <= hi)
        const int V = P / 4;
        for (int j = tid; j < P; j += CONCEAL_THREADS) {
            const int a = xs[need - P + j];
            int v = a;
            if (j >= P - V) {                                // faded into the period before, so that the template wraps without a step
                const int m = j - (P - V) + 1, b = xs[need - 2 * P + j];
                v = (int)rint((double)a + (double)((b - a) * m) / (double)(V + 1));
            }
            ts[j] = (short)v;
            tg[j] = (short)v;
        }
    } else {
        for (int j = tid; j < P; j += CONCEAL_THREADS) ts[j] = tg[j];
    }
    __syncthreads();

    const int qm = q % P;
    if (is_lost) {
        if (vec) {
            for (int g = tid * 8; g < cl; g += CONCEAL_THREADS * 8) {
                short v[8];
                for (int e = 0; e < 8; ++e) v[e] = (short)(int)rint(conceal_cont(ts, P, qm, q, g + e, hd, fd));
                *reinterpret_cast<uint4*>(c + g) = pack8(v);
            }
        } else {
            for (int i = tid; i < cl; i += CONCEAL_THREADS) c[i] = (short)(int)rint(conceal_cont(ts, P, qm, q, i, hd, fd));
        }
    } else {                                                 // recovering: the head of the real chunk, faded in from the continuation
        const int rec = rc < cl ? rc : cl;
        if (vec) {
            for (int g = tid * 8; g < rec; g += CONCEAL_THREADS * 8) {
                const uint4 p = *reinterpret_cast<const uint4*>(c + g);
                const unsigned u[4] = {p.x, p.y, p.z, p.w};
                short v[8];
                for (int e = 0; e < 8; ++e) {
                    v[e] = (short)((e & 1) ? (u[e >> 1] >> 16) : (u[e >> 1] & 0xffffu));
                    if (g + e < rec) v[e] = conceal_blend(conceal_cont(ts, P, qm, q, g + e, hd, fd), v[e], g + e, rec);
                }
                *reinterpret_cast<uint4*>(c + g) = pack8(v);
            }
        } else {
            for (int i = tid; i < rec; i += CONCEAL_THREADS) c[i] = conceal_blend(conceal_cont(ts, P, qm, q, i, hd, fd), c[i], i, rec);
        }
    }
    __syncthreads();
    if (tid == 0) {
        const int qn = q + cl;                               // (q <= QMAX = 2^30 and cl < 2^30: no overflow)
        state[2 * n] = is_lost ? (qn < ALIVE_CONCEAL_QMAX ? qn : ALIVE_CONCEAL_QMAX) : 0;
        state[2 * n + 1] = is_lost ? P : 0;
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int alive_conceal_rows(const int16_t* ring, int N, int ld, const int* ring_len, int16_t* chunks, int ld_chunk,
                                  const int* chunk_len, const unsigned char* present, const unsigned char* lost, const unsigned char* on,
                                  const int* lag_lo, const int* lag_hi, const int* window, const int* hold, const int* fade,
                                  const int* recover, int* state, int16_t* tmpl, int ld_tmpl, void* stream) {
    ALIVE_CHECK_ARG(ring && ring_len && chunks && chunk_len && present && lost && on && lag_lo && lag_hi && window && hold && fade &&
                        recover && state && tmpl,
                    "alive_conceal_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && ld > 0 && ld_chunk > 0 && ld_chunk < (1 << 30) && ld_tmpl > 0, "alive_conceal_rows: bad args");
    const int vec_ok = aligned16(chunks) && ld_chunk % 8 == 0;
    conceal_rows_kernel<<<N, CONCEAL_THREADS, 0, (hipStream_t)stream>>>(ring, ld, ring_len, chunks, ld_chunk, chunk_len, present, lost, on,
                                                                        lag_lo, lag_hi, window, hold, fade, recover, state, tmpl,
                                                                        ld_tmpl, vec_ok);
    ALIVE_CHECK_LAUNCH("alive_conceal_rows");
    return ALIVE_OK;
}
