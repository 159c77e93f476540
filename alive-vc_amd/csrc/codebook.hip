// Voice codebooks (module/codebook.py: build_codebook): the two device passes of a k-means iteration that are not the search.
//   the centroid update   alive_codebook_update   centroid c <- the mean of the raw fp32 rows of cluster c, read through an inverted index
//   the stop test         alive_codebook_stats    the fp64 sum of the rows' best cosines and the number of rows that changed cluster
// The assignment itself is the library's strict search (alive_knn_search_strict) and the inverted index a stable sort of the
// assignment, both done by the caller.
//
// Update (tools/codebook_ref.py is the float64 restatement; the result is bitwise its):  `order` lists the rows of cluster 0, then of
// cluster 1, ..., each list in ascending row index; seg_off[C + 1] holds the boundaries.  A list is cut into chunks of 512 rows.  One
// wave takes one chunk: lane l owns the 12 columns 4l .. 4l+3, 256 + 4l .. and 512 + 4l .. (three 16-byte loads, so a 3072-byte row is
// three fully coalesced wave loads), keeps twelve fp64 accumulators that start at +0.0 and adds the chunk's rows in list order, four
// rows in flight.  A list of one chunk is finished by its wave: sum / count in fp64, rounded to fp32 once.  A longer list's waves
// write their chunk sums to the workspace, and a second launch adds them in chunk order (from +0.0) and finishes the mean.  An empty
// list writes nothing.  No floating-point atomics, every add a plain add (-ffp-contract=off), every store a plain vector store.
// Which wave takes which chunk is laid out on the device by a one-block plan kernel (the lists' lengths are device data): the grids
// depend on M and C alone.  A malformed index (boundaries that fall or leave [0, M], a row index outside [0, M)) is never followed:
// such a list counts as empty and such a row is skipped.
#include "common.h"

namespace {

constexpr int CB_D = 768;
constexpr int CB_CHUNK = 512;          // rows per wave: the split rule of long lists
constexpr int CB_PLAN_THREADS = 1024;
constexpr int CB_STATS_THREADS = 1024;

struct CodebookWs {
    unsigned* item_off;                // [C + 1] first work item of each list (a work item = one chunk of one list)
    unsigned* pslot_off;               // [C + 1] first partial-sum slot of each list (only lists of >= 2 chunks take slots)
    int* item_list;                    // [max_items] the list of each work item
    double* partial;                   // [max_slots][768] chunk sums of the split lists
    size_t bytes;
};

inline size_t cb_max_items(int64_t M, int64_t C) { return (size_t)(C < M ? C : M) + (size_t)(M / CB_CHUNK); }
inline size_t cb_max_slots(int64_t M) { return (size_t)(M / CB_CHUNK) + (size_t)(M / (CB_CHUNK + 1)) + 1; }

CodebookWs cb_layout(void* ws, int64_t M, int64_t C) {
    Arena a(ws);
    CodebookWs w;
    w.item_off = a.take<unsigned>((size_t)C + 1);
    w.pslot_off = a.take<unsigned>((size_t)C + 1);
    w.item_list = a.take<int>(cb_max_items(M, C));
    w.partial = a.take<double>(cb_max_slots(M) * CB_D);
    w.bytes = a.used();
    return w;
}

__device__ __forceinline__ int cb_list_len(const int* __restrict__ seg_off, int c, int M, int* lo_out) {
    const int lo = seg_off[c], hi = seg_off[c + 1];
    *lo_out = lo;
    return (lo >= 0 && hi >= lo && hi <= M) ? hi - lo : 0;
}

// one block: exclusive scans of the lists' chunk counts (work items) and of the split lists' chunk counts (partial slots), and the
// item -> list table.  Thread t takes the lists [t * per, (t + 1) * per).
__global__ __launch_bounds__(CB_PLAN_THREADS) void codebook_plan_kernel(const int* __restrict__ seg_off, int C, int M,
                                                                        unsigned* __restrict__ item_off,
                                                                        unsigned* __restrict__ pslot_off, int* __restrict__ item_list) {
    __shared__ unsigned s_items[CB_PLAN_THREADS], s_slots[CB_PLAN_THREADS];
    const int tid = threadIdx.x;
    const int per = (int)(((int64_t)C + CB_PLAN_THREADS - 1) / CB_PLAN_THREADS);
    const int64_t c0 = (int64_t)tid * per;
    const int64_t c1 = c0 + per < C ? c0 + per : C;
    unsigned items = 0, slots = 0;
    for (int64_t c = c0; c < c1; ++c) {
        int lo;
        const int len = cb_list_len(seg_off, (int)c, M, &lo);
        const unsigned n = (unsigned)((len + CB_CHUNK - 1) / CB_CHUNK);
        items += n;
        slots += n > 1 ? n : 0;
    }
    s_items[tid] = items;
    s_slots[tid] = slots;
    __syncthreads();
    for (int o = 1; o < CB_PLAN_THREADS; o <<= 1) {          // inclusive scan over the threads' totals
        unsigned a = 0, b = 0;
        if (tid >= o) {
            a = s_items[tid - o];
            b = s_slots[tid - o];
        }
        __syncthreads();
        s_items[tid] += a;
        s_slots[tid] += b;
        __syncthreads();
    }
    unsigned item = s_items[tid] - items, slot = s_slots[tid] - slots;
    for (int64_t c = c0; c < c1; ++c) {
        int lo;
        const int len = cb_list_len(seg_off, (int)c, M, &lo);
        const unsigned n = (unsigned)((len + CB_CHUNK - 1) / CB_CHUNK);
        item_off[c] = item;
        pslot_off[c] = slot;
        for (unsigned j = 0; j < n; ++j) item_list[item + j] = (int)c;
        item += n;
        slot += n > 1 ? n : 0;
    }
    if (tid == CB_PLAN_THREADS - 1) {
        item_off[C] = s_items[tid];
        pslot_off[C] = s_slots[tid];
    }
}

__device__ __forceinline__ void cb_add_row(double (&acc)[12], const f32x4& a, const f32x4& b, const f32x4& c) {
    acc[0] = acc[0] + (double)a.x;
    acc[1] = acc[1] + (double)a.y;
    acc[2] = acc[2] + (double)a.z;
    acc[3] = acc[3] + (double)a.w;
    acc[4] = acc[4] + (double)b.x;
    acc[5] = acc[5] + (double)b.y;
    acc[6] = acc[6] + (double)b.z;
    acc[7] = acc[7] + (double)b.w;
    acc[8] = acc[8] + (double)c.x;
    acc[9] = acc[9] + (double)c.y;
    acc[10] = acc[10] + (double)c.z;
    acc[11] = acc[11] + (double)c.w;
}

// one wave per work item (grid-stride over the items): the hot pass, every row read once
__global__ __launch_bounds__(256) void codebook_sum_kernel(const float* __restrict__ rows, int M, const int* __restrict__ order,
                                                           const int* __restrict__ seg_off, int C,
                                                           const unsigned* __restrict__ item_off,
                                                           const unsigned* __restrict__ pslot_off, const int* __restrict__ item_list,
                                                           float* __restrict__ centroids, double* __restrict__ partial) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const unsigned n_items = item_off[C];
    const unsigned stride = gridDim.x * 4u;
    for (unsigned item = blockIdx.x * 4u + wave; item < n_items; item += stride) {
        const int c = item_list[item];
        int lo;
        const int len = cb_list_len(seg_off, c, M, &lo);
        const int chunk = (int)(item - item_off[c]);
        const int r0 = chunk * CB_CHUNK;
        if (len <= 0 || r0 >= len) continue;                  // (cannot happen with the plan of the same seg_off)
        const int n = len - r0 < CB_CHUNK ? len - r0 : CB_CHUNK;
        const int* __restrict__ ord = order + lo + r0;
        double acc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = 0.0;
        for (int r = 0; r < n; r += 4) {                      // four rows in flight (fewer at the list's end), added in list order
            const int cnt = n - r < 4 ? n - r : 4;            // (wave-uniform)
            f32x4 v[4][3] = {};
            bool ok[4] = {false, false, false, false};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (j < cnt) {
                    const int m = ord[r + j];
                    ok[j] = (unsigned)m < (unsigned)M;
                    if (ok[j]) {
                        const f32x4* p = (const f32x4*)(rows + (size_t)m * CB_D) + lane;
                        v[j][0] = p[0];
                        v[j][1] = p[64];
                        v[j][2] = p[128];
                    }
                }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j)
                if (ok[j]) cb_add_row(acc, v[j][0], v[j][1], v[j][2]);
        }
        if (len <= CB_CHUNK) {                                // the whole list: finish the mean here
            const double cnt = (double)len;
            f32x4* q = (f32x4*)(centroids + (size_t)c * CB_D) + lane;
#pragma unroll
            for (int g = 0; g < 3; ++g) {
                f32x4 o;
                o.x = (float)(acc[4 * g + 0] / cnt);
                o.y = (float)(acc[4 * g + 1] / cnt);
                o.z = (float)(acc[4 * g + 2] / cnt);
                o.w = (float)(acc[4 * g + 3] / cnt);
                q[64 * g] = o;
            }
        } else {
            double* q = partial + ((size_t)pslot_off[c] + chunk) * CB_D;
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) q[256 * g + 4 * lane + e] = acc[4 * g + e];
        }
    }
}

// one wave per list (grid-stride over the lists); only a list of two or more chunks does anything: its chunk sums in chunk order
__global__ __launch_bounds__(256) void codebook_finish_kernel(const int* __restrict__ seg_off, int C, int M,
                                                              const unsigned* __restrict__ pslot_off,
                                                              const double* __restrict__ partial, float* __restrict__ centroids) {
    const int lane = threadIdx.x & 63;
    const unsigned wave = (unsigned)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int64_t stride = (int64_t)gridDim.x * 4;
    for (int64_t c = (int64_t)blockIdx.x * 4 + wave; c < C; c += stride) {
        int lo;
        const int len = cb_list_len(seg_off, (int)c, M, &lo);
        if (len <= CB_CHUNK) continue;
        const int n = (len + CB_CHUNK - 1) / CB_CHUNK;
        const double* p = partial + (size_t)pslot_off[c] * CB_D;
        double acc[12];
#pragma unroll
        for (int i = 0; i < 12; ++i) acc[i] = 0.0;
        for (int j = 0; j < n; ++j) {
#pragma unroll
            for (int g = 0; g < 3; ++g)
#pragma unroll
                for (int e = 0; e < 4; ++e) acc[4 * g + e] = acc[4 * g + e] + p[(size_t)j * CB_D + 256 * g + 4 * lane + e];
        }
        const double cnt = (double)len;
        f32x4* q = (f32x4*)(centroids + (size_t)c * CB_D) + lane;
#pragma unroll
        for (int g = 0; g < 3; ++g) {
            f32x4 o;
            o.x = (float)(acc[4 * g + 0] / cnt);
            o.y = (float)(acc[4 * g + 1] / cnt);
            o.z = (float)(acc[4 * g + 2] / cnt);
            o.w = (float)(acc[4 * g + 3] / cnt);
            q[64 * g] = o;
        }
    }
}

// one block.  objective: thread tid adds val[tid], val[tid + 1024], ... in turn from +0.0 in fp64, then acc[i] += acc[i + o] for
// o = 512, 256, ..., 1 (gate.hip's order at four times the width).  moved: integer counts, any order.
__global__ __launch_bounds__(CB_STATS_THREADS) void codebook_stats_kernel(const int* __restrict__ assign, const int* __restrict__ prev,
                                                                          const float* __restrict__ val, int M,
                                                                          double* __restrict__ objective, int64_t* __restrict__ moved) {
    __shared__ double s_acc[CB_STATS_THREADS];
    __shared__ int s_cnt[CB_STATS_THREADS];
    const int tid = threadIdx.x;
    double a = 0.0;
    int cnt = 0;
    for (int64_t m = tid; m < M; m += CB_STATS_THREADS) {
        a = a + (double)val[m];
        cnt += prev ? (assign[m] != prev[m] ? 1 : 0) : 1;
    }
    s_acc[tid] = a;
    s_cnt[tid] = cnt;
    __syncthreads();
    for (int o = CB_STATS_THREADS / 2; o > 0; o >>= 1) {
        if (tid < o) {
            s_acc[tid] = s_acc[tid] + s_acc[tid + o];
            s_cnt[tid] = s_cnt[tid] + s_cnt[tid + o];
        }
        __syncthreads();
    }
    if (tid == 0) {
        *objective = s_acc[0];
        *moved = (int64_t)s_cnt[0];
    }
}

int cb_check_sizes(const char* who, int64_t M, int64_t C) {
    ALIVE_CHECK_ARG(M >= 1 && M < (int64_t)1 << 31, "%s: M=%lld outside [1, 2^31)", who, (long long)M);
    ALIVE_CHECK_ARG(C >= 1 && C <= M, "%s: C=%lld outside [1, M=%lld]", who, (long long)C, (long long)M);
    return ALIVE_OK;
}

}  // namespace

extern "C" size_t alive_codebook_workspace_bytes(int64_t M, int64_t C) {
    if (!(M >= 1 && M < (int64_t)1 << 31 && C >= 1 && C <= M)) return 0;
    return cb_layout(nullptr, M, C).bytes;
}

extern "C" int alive_codebook_update(const float* rows, int64_t M, int Dd, const int32_t* order, const int32_t* seg_off, int64_t C,
                                     float* centroids, void* ws, void* stream) {
    ALIVE_CHECK_ARG(rows && order && seg_off && centroids && ws, "alive_codebook_update: null pointer");
    ALIVE_CHECK_ARG(Dd == CB_D, "alive_codebook_update: feature dim %d, expected %d", Dd, CB_D);
    if (int rc = cb_check_sizes("alive_codebook_update", M, C)) return rc;
    ALIVE_CHECK_ARG((((uintptr_t)rows | (uintptr_t)centroids) & 15) == 0, "alive_codebook_update: rows and centroids must be 16-byte aligned");
    const CodebookWs w = cb_layout(ws, M, C);
    hipStream_t s = (hipStream_t)stream;
    codebook_plan_kernel<<<1, CB_PLAN_THREADS, 0, s>>>(seg_off, (int)C, (int)M, w.item_off, w.pslot_off, w.item_list);
    const size_t items = cb_max_items(M, C);
    const unsigned sum_blocks = (unsigned)(items / 4 + 1 < ((size_t)1 << 20) ? items / 4 + 1 : (size_t)1 << 20);
    codebook_sum_kernel<<<sum_blocks, 256, 0, s>>>(rows, (int)M, order, seg_off, (int)C, w.item_off, w.pslot_off, w.item_list, centroids,
                                                   w.partial);
    if (M > CB_CHUNK) {                                       // (no list can be split otherwise)
        const unsigned fin_blocks = (unsigned)(C / 4 + 1 < ((int64_t)1 << 20) ? C / 4 + 1 : (int64_t)1 << 20);
        codebook_finish_kernel<<<fin_blocks, 256, 0, s>>>(seg_off, (int)C, (int)M, w.pslot_off, w.partial, centroids);
    }
    ALIVE_CHECK_LAUNCH("alive_codebook_update");
    return ALIVE_OK;
}

extern "C" int alive_codebook_stats(const int32_t* assign, const int32_t* prev, const float* val, int64_t M, double* objective,
                                    int64_t* moved, void* stream) {
    ALIVE_CHECK_ARG(assign && val && objective && moved, "alive_codebook_stats: null pointer");
    ALIVE_CHECK_ARG(M >= 1 && M < (int64_t)1 << 31, "alive_codebook_stats: M=%lld outside [1, 2^31)", (long long)M);
    codebook_stats_kernel<<<1, CB_STATS_THREADS, 0, (hipStream_t)stream>>>(assign, prev, val, (int)M, objective, moved);
    ALIVE_CHECK_LAUNCH("alive_codebook_stats");
    return ALIVE_OK;
}
