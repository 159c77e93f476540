// Match path (module/common.py: path_options, ops.knn_path_rows): out of each frame's K candidates of a top-k list, one library row per
// frame by a Viterbi path -- unit selection between a search and its gather.  Per list row of T frames, lists val / idx [T][k_max] best
// first with K = k_row[r] entries in use, the fp32 rows table [P][768] with its norms, and a weight w >= 0:
//   active frame  idx[t][0] >= 0 and no idx[t][i] >= P among i < K      (an index outside the table is never dereferenced)
//   state i       exists when the frame is active, i < K and idx[t][i] >= 0
//   e[t][i]       (double) val[t][i] - (double) val[t][0]               the candidate's cosine below the frame's best one
//   c[t][i][j]    dot(a, b) / ((double) norms[a] * (double) norms[b]),  a = idx[t][i], b = idx[t - 1][j]: the cosine between two rows
//   D[t][i]       e[t][i] at t = 0 and after an inactive frame (a new segment), else
//                 e[t][i] + max_j (D[t - 1][j] + w * c[t][i][j]) over the existing j, the lowest j on ties: back[t][i]
//   p             a segment ends at T - 1 or before an inactive frame: its end takes the lowest i attaining max D; p[t - 1] = back[t][p[t]]
// (a NaN candidate counts as -inf in both maxima).  Entry 0 of the output list of frame t is (val[t][p], idx[t][p]), the others and
// every entry of an inactive frame are (-inf, -1); moved[r] counts the frames with p != 0; a row that is off is copied.
// All fp64, every operation rounded on its own, and the dot in ONE fixed order: lane l of 64 sums (double) x[l + 64 q] * (double) y[l + 64 q]
// over q = 0 .. 11 ascending from 0.0 (a product of two floats is exact in double, so contraction could not change a bit), then
// p[l] = p[l] + p[l + o] for o = 32 .. 1.  The result is bitwise tools/match_path_ref.py.
//   Two launches.  JOIN: one block of k_max waves per (list row, frame t >= 1); a block whose row is off or whose frame or the frame
//   before is inactive returns at once (block-uniform, before the barrier).  Wave j stages row idx[t - 1][j] in LDS (k_max x 3 KB: 24 KB
//   at k_max = 8, static), wave i holds row idx[t][i] in registers, 12 floats per lane, and takes the K dots against LDS (lane l reads
//   l + 64 q: conflict-free); lane 0 divides and stores J[r][t][i][j].  Entries of states that do not exist are not written.
//   PATH: one wave per list row, lane = 8 i + j.  D stays in registers (lane 8 i + j holds D[i]); per frame a lane takes D[t - 1][j] from
//   lane 8 j, forms its candidate and the eight lanes of a state reduce it (xor 4, 2, 1), then the states' lanes reduce the frame's
//   best state (xor 32, 16, 8).  The lists and J of frame t + 1 are loaded while frame t is computed.  Back pointers (uint8 [R][T][k_max])
//   go to the workspace and the frame's best state (-1: inactive) to out_idx[t][0] through plain vector stores; after a barrier lane 0
//   traces back, leaving p[t] where the best state was; after another barrier all lanes write the output lists.
//   No atomics, no host synchronisation, no allocation: capturable.  The output lists must not overlap the input lists.
#include "common.h"

namespace {

constexpr int D = 768, QS = D / 64;
constexpr int KP = 8;                                       // lanes per state in the path kernel (k_max <= 8)
static_assert(ALIVE_KNN_PATH_MAX_K == KP, "lane = 8 i + j");

// the better of two (value, index) candidates: the larger value, the lower index among equals
__device__ __forceinline__ void keep_best(double& v, int& i, double ov, int oi) {
    if (ov > v || (ov == v && oi < i)) {
        v = ov;
        i = oi;
    }
}

__device__ __forceinline__ bool row_on(const int32_t* on, const int32_t* k_row, int r, int k_max, int& K) {
    K = k_row[r];
    return on[r] != 0 && K >= 1 && K <= k_max;
}

// whether frame f of a list (ix: its k_max indices) is active, for every thread alike
__device__ __forceinline__ bool frame_active(const int32_t* __restrict__ ix, int K, int64_t P) {
    bool ok = ix[0] >= 0;
    for (int i = 0; i < K; ++i) ok = ok && (int64_t)ix[i] < P;
    return ok;
}

// RT: the row table's element type (float, or _Float16 of a half pool widened as it is read -- exact, so the dots are those of the
// fp32 table of the widened values)
template <typename RT>
__global__ __launch_bounds__(64 * KP) void path_join_kernel(const int32_t* __restrict__ idx, const int32_t* __restrict__ k_row, int k_max,
                                                            const int32_t* __restrict__ on, const RT* __restrict__ rows,
                                                            const float* __restrict__ norms, int64_t P, int T, double* __restrict__ J) {
    __shared__ float prev[KP][D];
    const int r = blockIdx.x / (T - 1), t = blockIdx.x % (T - 1) + 1;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    int K;
    if (!row_on(on, k_row, r, k_max, K)) return;            // (block-uniform, like the two below)
    const int32_t* it = idx + ((size_t)r * T + t) * k_max;  // frame t; frame t - 1 lies k_max entries before it
    if (!frame_active(it, K, P) || !frame_active(it - k_max, K, P)) return;
    const int mine = wave < K ? it[wave] : -1;              // state `wave` of frame t (< P: the frame is active)
    const int theirs = wave < K ? it[wave - k_max] : -1;    // state `wave` of frame t - 1
    if (theirs >= 0) {
        const RT* y = rows + (size_t)theirs * D;
#pragma unroll
        for (int q = 0; q < QS; ++q) prev[wave][lane + 64 * q] = (float)y[lane + 64 * q];
    }
    float x[QS];
    if (mine >= 0) {
        const RT* xr = rows + (size_t)mine * D;
#pragma unroll
        for (int q = 0; q < QS; ++q) x[q] = (float)xr[lane + 64 * q];
    }
    __syncthreads();
    if (mine < 0) return;
    const double na = (double)norms[mine];
    double* out = J + (((size_t)r * T + t) * k_max + wave) * k_max;
    for (int j = 0; j < K; ++j) {
        const int b = it[j - k_max];
        if (b < 0) continue;                                // (wave-uniform)
        double p = 0.0;
#pragma unroll
        for (int q = 0; q < QS; ++q) p = p + (double)x[q] * (double)prev[j][lane + 64 * q];
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) p = p + __shfl_down(p, o, 64);     // (lane 0 depends on lanes < 2 o alone)
        if (lane == 0) out[j] = p / (na * (double)norms[b]);
    }
}

__global__ __launch_bounds__(64) void path_kernel(const float* __restrict__ val, const int32_t* __restrict__ idx,
                                                  const int32_t* __restrict__ k_row, int k_max, const int32_t* __restrict__ on,
                                                  const double* __restrict__ weight, int64_t P, int T, const double* __restrict__ J,
                                                  float* __restrict__ out_val, int32_t* __restrict__ out_idx, int32_t* __restrict__ moved,
                                                  unsigned char* __restrict__ back) {
    const int r = blockIdx.x, lane = threadIdx.x;
    const size_t base = (size_t)r * T * k_max;
    const float* v = val + base;
    const int32_t* ix = idx + base;
    float* ov = out_val + base;
    int32_t* oi = out_idx + base;
    int K;
    if (!row_on(on, k_row, r, k_max, K)) {                  // a row that is off: its lists as they are
        for (size_t e = lane; e < (size_t)T * k_max; e += 64) {
            ov[e] = v[e];
            oi[e] = ix[e];
        }
        if (lane == 0) moved[r] = 0;
        return;
    }
    const int i = lane >> 3, j = lane & 7;
    const bool in = i < K && j < k_max;                     // lanes that load: state i's entry, and J[t][i][j] where j < k_max
    const double w = weight[r];
    const double NEG = -__builtin_huge_val();
    const double* Jr = J + base * k_max;
    unsigned char* bk = back + base;
    // the frame to come: state i's list entry and join cost, loaded one frame ahead
    int ni = in ? ix[i] : -1;
    float nv = in ? v[i] : 0.0f;
    double nc = 0.0;
    double Dp = NEG;                                        // D[t - 1][i]
    bool ep = false, ap = false;                            // state i of frame t - 1 exists; frame t - 1 is active
    for (int t = 0; t < T; ++t) {
        const int ci = ni;
        const float cv = nv;
        const double c = nc;
        if (t + 1 < T) {
            ni = in ? ix[(size_t)(t + 1) * k_max + i] : -1;
            nv = in ? v[(size_t)(t + 1) * k_max + i] : 0.0f;
            nc = in && j < K ? Jr[((size_t)(t + 1) * k_max + i) * k_max + j] : 0.0;     // (may be fill where no state exists: not used then)
        }
        const bool act = __shfl(ci, 0, 64) >= 0 && !__any(in && (int64_t)ci >= P);
        const bool ex = act && in && ci >= 0;
        const double e = (double)cv - (double)__shfl(cv, 0, 64);
        double d = e;
        if (ap) {                                           // (wave-uniform)
            const double dj = __shfl(Dp, 8 * j, 64);
            const bool ej = __shfl((int)ep, 8 * j, 64) != 0;
            double m = dj + w * c;
            m = (ex && ej && m == m) ? m : NEG;
            int bj = j;
#pragma unroll
            for (int o = 4; o > 0; o >>= 1) keep_best(m, bj, __shfl_xor(m, o, 64), __shfl_xor(bj, o, 64));
            d = e + m;
            if (j == 0 && i < k_max) bk[(size_t)t * k_max + i] = (unsigned char)bj;
        }
        d = ex ? d : NEG;
        double bv = d == d ? d : NEG;                       // the frame's best state, the lowest on ties
        int bi = i;
#pragma unroll
        for (int o = 32; o >= 8; o >>= 1) keep_best(bv, bi, __shfl_xor(bv, o, 64), __shfl_xor(bi, o, 64));
        if (lane == 0) oi[(size_t)t * k_max] = act ? bi : -1;
        Dp = d;
        ep = ex;
        ap = act;
    }
    __syncthreads();                                        // (one wave: orders this block's stores before lane 0's loads)
    if (lane == 0) {
        int p = -1, n = 0;                                  // p: the state of frame t + 1, -1 when it is inactive or t = T - 1
        for (int t = T - 1; t >= 0; --t) {
            const int best = oi[(size_t)t * k_max];
            if (best < 0) {
                p = -1;
                continue;
            }
            p = p < 0 ? best : bk[(size_t)(t + 1) * k_max + p];
            p = p < k_max ? p : 0;                          // (always so: a chosen state exists)
            n += p != 0;
            oi[(size_t)t * k_max] = p;
        }
        moved[r] = n;
    }
    __syncthreads();
    for (int e = lane; e < T * k_max; e += 64) {            // (R T <= 2^20 frames of at most 8 entries)
        if (e % k_max != 0) {
            ov[e] = -__builtin_huge_valf();
            oi[e] = -1;
        } else {
            const int p = oi[e];                            // (only this lane touches out_idx[t][0])
            ov[e] = p < 0 ? -__builtin_huge_valf() : v[e + p];
            oi[e] = p < 0 ? -1 : ix[e + p];
        }
    }
}

bool path_sizes(int R, int T, int k_max) {
    return R >= 1 && T >= 1 && k_max >= 1 && k_max <= ALIVE_KNN_PATH_MAX_K && (int64_t)R * T <= ALIVE_KNN_PATH_MAX_FRAMES;
}

}  // namespace

extern "C" int alive_knn_path_layout(int R, int T, int k_max, int64_t* off) {
    ALIVE_CHECK_ARG(off, "alive_knn_path_layout: null pointer");
    ALIVE_CHECK_ARG(path_sizes(R, T, k_max), "alive_knn_path_layout: needs R, T >= 1, R * T <= 2^20 and k_max in [1, %d]",
                    ALIVE_KNN_PATH_MAX_K);
    off[0] = 0;                                                                             // J: double [R][T][k_max][k_max]
    off[1] = (int64_t)align_up((size_t)R * T * k_max * k_max * sizeof(double), 256);        // back pointers: uint8 [R][T][k_max]
    return ALIVE_OK;
}

extern "C" size_t alive_knn_path_workspace_bytes(int R, int T, int k_max) {
    if (!path_sizes(R, T, k_max)) return 0;
    return align_up((size_t)R * T * k_max * k_max * sizeof(double), 256) + align_up((size_t)R * T * k_max, 256);
}

namespace {

// both entry points (RT = float: alive_knn_path_rows; _Float16: alive_knn_path_rows_f16)
template <typename RT>
int path_rows(const char* who, const float* val, const int32_t* idx, const int32_t* k_row, int k_max, const int32_t* on, const double* weight,
              const RT* rows, const float* norms, int64_t P, int R, int T, float* out_val, int32_t* out_idx, int32_t* moved, void* ws,
              void* stream) {
    ALIVE_CHECK_ARG(val && idx && out_val && out_idx, "%s: null lists", who);
    ALIVE_CHECK_ARG(k_row && on && weight && moved, "%s: null per-row array", who);
    ALIVE_CHECK_ARG(rows && norms && ws, "%s: null pointer", who);
    ALIVE_CHECK_ARG(k_max >= 1 && k_max <= ALIVE_KNN_PATH_MAX_K, "%s: k_max %d outside [1, %d]", who, k_max, ALIVE_KNN_PATH_MAX_K);
    ALIVE_CHECK_ARG(R >= 1 && T >= 1, "%s: empty lists", who);
    ALIVE_CHECK_ARG((int64_t)R * T <= ALIVE_KNN_PATH_MAX_FRAMES, "%s: R * T = %lld exceeds 2^20 frames", who, (long long)R * T);
    ALIVE_CHECK_ARG(P > 0 && P <= 0x7fffffffLL, "%s: P outside [1, 2^31)", who);
    ALIVE_CHECK_ARG(val != out_val && idx != out_idx, "%s: the output lists must not be the input lists", who);
    int64_t off[2];
    alive_knn_path_layout(R, T, k_max, off);
    double* J = (double*)((char*)ws + off[0]);
    unsigned char* back = (unsigned char*)ws + off[1];
    if (T > 1) {                                            // (a one-frame list has no join: one launch)
        path_join_kernel<RT><<<R * (T - 1), 64 * k_max, 0, (hipStream_t)stream>>>(idx, k_row, k_max, on, rows, norms, P, T, J);
        ALIVE_CHECK_LAUNCH(who);
    }
    path_kernel<<<R, 64, 0, (hipStream_t)stream>>>(val, idx, k_row, k_max, on, weight, P, T, J, out_val, out_idx, moved, back);
    ALIVE_CHECK_LAUNCH(who);
    return ALIVE_OK;
}

}  // namespace

extern "C" int alive_knn_path_rows(const float* val, const int32_t* idx, const int32_t* k_row, int k_max, const int32_t* on,
                                   const double* weight, const float* rows_f32, const float* norms, int64_t P, int R, int T,
                                   float* out_val, int32_t* out_idx, int32_t* moved, void* ws, void* stream) {
    return path_rows("alive_knn_path_rows", val, idx, k_row, k_max, on, weight, rows_f32, norms, P, R, T, out_val, out_idx, moved, ws, stream);
}

// half pool: the row table as fp16 [P][768]; bitwise alive_knn_path_rows on the widened table
extern "C" int alive_knn_path_rows_f16(const float* val, const int32_t* idx, const int32_t* k_row, int k_max, const int32_t* on,
                                       const double* weight, const void* rows_f16, const float* norms, int64_t P, int R, int T,
                                       float* out_val, int32_t* out_idx, int32_t* moved, void* ws, void* stream) {
    return path_rows("alive_knn_path_rows_f16", val, idx, k_row, k_max, on, weight, (const _Float16*)rows_f16, norms, P, R, T, out_val, out_idx,
                     moved, ws, stream);
}
