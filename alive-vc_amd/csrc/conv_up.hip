// ConvTranspose1d(k == stride == up) of the decoder's coarse scales on two-plane split bf16 (precision 1), input stationary.
//
// conv_split.hip tiles the GEMM rows over the grid: for the decoder's ups[0] (256 -> 256 x 10) twenty blocks, for ups[1]
// (256 -> 64 x 8) four, load, split and store the SAME 256-channel input tile, and with KW == 1 each of them meets a block barrier
// and the whole fp32 -> bf16 staging chain every 24 MFMAs per wave.  Here a block owns one (window, 64-column tile):
//   * it stages ALL Ci <= 256 channels of the tile once -- fp32 loads, the split of conv_split.hip's store_X (v_cvt_pk_bf16_f32),
//     two bf16 planes in LDS, 64 KB, [plane][channel block of 32][column][32 channels], the 16-B chunks of a row XOR-swizzled by
//     (column >> 2) & 3 like conv_split.hip's plane form, which keeps every ds_read_b128 of a B fragment conflict-free;
//   * ONE barrier; then every wave walks row tiles of 32 GEMM rows (wave w: tiles w, w + 4, ...) under the resident image with no
//     barrier at all: A fragments straight from L2 (the weight image of module/_pack.py::pack_conv_split), three channel blocks
//     ahead, across the row-tile boundary; B fragments from LDS one k16 step ahead;
//   * a row tile leaves straight from the accumulators.  Register group q of lane (lr, lh) holds GEMM rows 8 q + 4 lh .. + 3 of
//     column lr, i.e. the consecutive samples Y[co][t up + j .. j + 3] when up is a multiple of 4 (one 16-byte store; at up = 8 the
//     64 lanes of one store instruction write 1 KB of consecutive samples), and two pairs of consecutive samples when up is even
//     (8-byte stores: a pair never straddles a channel).  No LDS staging, no per-element division.
// Two blocks are resident per CU (2 x 64 KB of LDS, 8 waves): one block's staging and stores run under the other's MFMAs.
//
// Same bits as conv_split_kernel<128, 2> (and <64, 2>): an accumulator starts at the bias, takes the channel blocks in ascending
// order, the two k16 halves of a block in order and in each half a_hi b_lo, a_lo b_hi, a_hi b_hi; columns >= Tin stage zeros.
//
// The accumulation-chain rule (common.h ALIVE_CHAIN_GAP, DESIGN.md 3.2b'): a row tile's accumulators are read completely -- by
// the stores -- before the first MFMA of the next tile's chains; scheduling barriers pin the store phase between the two, so no
// chain starts beside an unread accumulator (tests/test_host_upconv.py scans the listing: no such chain switch exists).
#include <atomic>
#include <type_traits>
#include "common.h"
#include "planes_layout.h"

namespace {

constexpr int UBN = 64;                          // columns per block
constexpr int UKC = 32;                          // channels per block of the reduction
constexpr int UCI_MAX = 256;                     // channels the resident image holds
constexpr int UROW = 64;                         // bytes per LDS row: 32 channels bf16, chunks swizzled by the column
constexpr int UCB = UBN * UROW;                  // bytes per (plane, channel block)
constexpr int UPLANE = (UCI_MAX / UKC) * UCB;    // bytes per plane
// The new form takes a launch only when its grid, N x column tiles, puts two blocks on each of the MI355X's 256 CUs: below that,
// the row-tile dimension of conv_split.hip's grid is the only parallelism there is.
constexpr int UP_MIN_BLOCKS = 512;
std::atomic<int> g_up_min_blocks{UP_MIN_BLOCKS};      // (alive_conv_up_min_blocks: the tests reach the kernel with small shapes)

typedef float f32x2 __attribute__((ext_vector_type(2)));

std::atomic<int> g_up_launches{0};

// ST: how a row tile leaves.  0: up % 4 == 0, 16-byte stores; 1: up even, 8-byte stores; 2: any up, 4-byte stores
template <int ST, int NCB>
__global__ __launch_bounds__(256, 2) void conv_up_kernel(AliveConv p, unsigned inv_up) {
    __shared__ __attribute__((aligned(16))) unsigned char smem[2 * UPLANE];

    const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
    const int lr = lane & 31, lh = lane >> 5;
    const int n = blockIdx.y, t0 = blockIdx.x * UBN;
    const int co_pad = (p.Co + 15) & ~15;
    const int ncb = p.Ci / UKC;
    const int ntile = (p.Co + 31) >> 5;
    const unsigned short* W16 = (const unsigned short*)p.W;
    const size_t wplane = (size_t)p.Ci * co_pad;               // elements per weight plane (planes_layout.h, K = Ci)

    // ---- A fragments: lane (row lr, half lh) loads the 16 B of (channel block, k16 step, plane) it feeds to the MFMA.  NCB == 8
    // (Ci = 256, the decoder's): a ring of four fragment sets, fetched THREE channel blocks ahead and across the row-tile boundary;
    // the channel-block loop is unrolled, so a set's ring slot is a compile-time constant and 8 % 4 == 0 brings every tile back to
    // slot 0 -- nothing is copied, and no fetch is waited for before its use.  NCB == 0 (any other Ci): fetched where it is used.
    auto fetch = [&](int tile, int cb, bf16x8 (&a)[2][2]) {    // [k16 step][plane]
        if (tile < ntile) {                                    // wave-uniform
            int grow = tile * 32 + lr;
            grow = grow < co_pad ? grow : co_pad - 1;
            const unsigned short* w = W16 + ((size_t)cb * co_pad + grow) * PLANES_KB + lh * 8;
#pragma unroll
            for (int s2 = 0; s2 < 2; ++s2)
#pragma unroll
                for (int pl = 0; pl < 2; ++pl) a[s2][pl] = *(const bf16x8*)(w + pl * wplane + s2 * 16);
        }
    };
    constexpr int RING = NCB == 8 ? 4 : 1;
    bf16x8 a_ring[RING][2][2];
    if constexpr (NCB == 8) {                                  // in flight under the staging
#pragma unroll
        for (int cb = 0; cb < 3; ++cb) fetch(wid, cb, a_ring[cb]);
    }

    // ---- staging: wave w owns the 8-channel group w of every channel block, lane = column (loads coalesced along time) ----
    {
        const int tcol = t0 + lane;
        const bool ok = tcol < p.Tin;
        const float* Xl = p.X + ((size_t)n * p.Ci + wid * 8) * p.Tin + (ok ? tcol : p.Tin - 1);
        unsigned char* dst = smem + lane * UROW + ((wid ^ ((lane >> 2) & 3)) << 4);
        for (int cb0 = 0; cb0 < ncb; cb0 += 4) {               // four channel blocks of loads in flight
            float x[4][8];
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (cb0 + u < ncb) {
#pragma unroll
                    for (int c = 0; c < 8; ++c) x[u][c] = Xl[(size_t)((cb0 + u) * UKC + c) * p.Tin];
                }
#pragma unroll
            for (int u = 0; u < 4; ++u)
                if (cb0 + u < ncb) {
                    u32x4 hv, lv;
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const float x0 = ok ? x[u][2 * e] : 0.0f, x1 = ok ? x[u][2 * e + 1] : 0.0f;
                        hv[e] = pack_bf16x2(x0, x1);
                        lv[e] = pack_bf16x2_lo(x0, x1, hv[e]);
                    }
                    *(u32x4*)(dst + (cb0 + u) * UCB) = hv;
                    *(u32x4*)(dst + (cb0 + u) * UCB + UPLANE) = lv;
                }
        }
    }
    __syncthreads();                                           // the only barrier: the image is read-only from here on

    // ---- B fragments: column nn * 32 + lr, channels 16 s2 + 8 lh .. + 7 of a block (the swizzle does not depend on nn) ----
    const unsigned char* bbase = smem + lr * UROW;
    const int bsw0 = ((0 + lh) ^ ((lr >> 2) & 3)) << 4, bsw1 = ((2 + lh) ^ ((lr >> 2) & 3)) << 4;
    auto load_B = [&](int cb, int s2, bf16x8 (&b)[2][2]) {     // [plane][column tile]
        const unsigned char* q = bbase + cb * UCB + (s2 ? bsw1 : bsw0);
#pragma unroll
        for (int pl = 0; pl < 2; ++pl)
#pragma unroll
            for (int nn = 0; nn < 2; ++nn) b[pl][nn] = *(const bf16x8*)(q + pl * UPLANE + nn * 32 * UROW);
    };
    auto load_bias = [&](int tile, f32x16& raw) {              // clamped loads; the select waits until the values are used
        if (p.bias != nullptr) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                raw[r] = p.bias[row < p.Co ? row : p.Co - 1];
            }
        }
    };

    const size_t Lout = (size_t)p.Tout * p.up;
    float* Yn = p.Y + (size_t)n * (p.Co / p.up) * Lout;
    // TWO: the block's second 32 columns hold a valid one (block-uniform; false only in the last tile of a row of tiles)
    auto walk = [&](auto two_c) {
        constexpr bool TWO = decltype(two_c)::value;
        constexpr int NR = TWO ? 2 : 1;
        f32x16 acc[NR];
        auto mfma6 = [&](const bf16x8 (&a)[2], const bf16x8 (&b)[2][2]) {      // a_hi b_lo, a_lo b_hi, a_hi b_hi per column tile
#pragma unroll
            for (int nn = 0; nn < NR; ++nn) {
                acc[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1][nn], acc[nn], 0, 0, 0);
                acc[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0][nn], acc[nn], 0, 0, 0);
                acc[nn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0][nn], acc[nn], 0, 0, 0);
            }
        };
        bf16x8 b0[2][2], b1[2][2];
        f32x16 bias_raw;
#pragma unroll
        for (int r = 0; r < 16; ++r) bias_raw[r] = 0.0f;
        load_bias(wid, bias_raw);
        load_B(0, 0, b0);
        for (int tile = wid; tile < ntile; tile += 4) {
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int row = tile * 32 + (r & 3) + 8 * (r >> 2) + 4 * lh;
                const float v = row < p.Co ? bias_raw[r] : 0.0f;
#pragma unroll
                for (int nn = 0; nn < NR; ++nn) acc[nn][r] = v;
            }
            if (tile + 4 < ntile) load_bias(tile + 4, bias_raw);       // lands under this tile's MFMAs
            auto step = [&](int cb, const bf16x8 (&a)[2][2]) {
                load_B(cb, 1, b1);
                mfma6(a[0], b0);
                load_B(cb + 1 < ncb ? cb + 1 : 0, 0, b0);      // (the image does not depend on the row tile)
                mfma6(a[1], b1);
            };
            if constexpr (NCB == 8) {
#pragma unroll
                for (int cb = 0; cb < 8; ++cb) {
                    fetch(cb + 3 < 8 ? tile : tile + 4, (cb + 3) & 7, a_ring[(cb + 3) & 3]);
                    step(cb, a_ring[cb & 3]);
                }
            } else {
                for (int cb = 0; cb < ncb; ++cb) {
                    fetch(tile, cb, a_ring[0]);
                    step(cb, a_ring[0]);
                }
            }
            // ---- the tile leaves: every accumulator register is read here, before the next tile's chains start ----
            __builtin_amdgcn_sched_barrier(0);
#pragma unroll
            for (int nn = 0; nn < NR; ++nn) {
                const int t = t0 + nn * 32 + lr;
                if (t >= p.Tout) continue;
                float* yt = Yn + (size_t)t * p.up;
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    const int R0 = tile * 32 + 8 * q + 4 * lh;     // GEMM rows R0 .. R0 + 3 = (co, j) in row-major order
                    if (ST == 0) {
                        if (R0 < p.Co) {
                            const int co = (int)__umulhi((unsigned)R0, inv_up), j = R0 - co * p.up;
                            *(f32x4*)(yt + (size_t)co * Lout + j) = f32x4{acc[nn][4 * q], acc[nn][4 * q + 1], acc[nn][4 * q + 2], acc[nn][4 * q + 3]};
                        }
                    } else if (ST == 1) {
#pragma unroll
                        for (int h = 0; h < 2; ++h) {
                            const int R = R0 + 2 * h;
                            if (R < p.Co) {
                                const int co = (int)__umulhi((unsigned)R, inv_up), j = R - co * p.up;
                                *(f32x2*)(yt + (size_t)co * Lout + j) = f32x2{acc[nn][4 * q + 2 * h], acc[nn][4 * q + 2 * h + 1]};
                            }
                        }
                    } else {
#pragma unroll
                        for (int h = 0; h < 4; ++h) {
                            const int R = R0 + h;
                            if (R < p.Co) {
                                const int co = (int)__umulhi((unsigned)R, inv_up), j = R - co * p.up;
                                yt[(size_t)co * Lout + j] = acc[nn][4 * q + h];
                            }
                        }
                    }
                }
            }
            __builtin_amdgcn_sched_barrier(0);
        }
    };
    if (p.Tout - t0 > 32) walk(std::true_type{});
    else walk(std::false_type{});
}

}  // namespace

// true if the descriptor takes the stationary-input form (then *rc is the launch's status).  Called by alive_conv_split_launch
// behind its argument checks; everything that does not qualify launches what it launched before.
bool alive_conv_up_try(const AliveConv* d, hipStream_t s, int* rc) {
    if (d->precision != 1 || d->KW != 1 || d->stride != 1 || d->up <= 1 || d->pad_left != 0) return false;
    if (d->Ci % UKC != 0 || d->Ci != d->Ci_pad || d->Ci > UCI_MAX) return false;
    if (d->act != 0 || d->post_add || d->ch_scale || d->residual || d->skip || d->Z || d->Zp || d->Xp || !d->X || !d->Y) return false;
    if (d->Co % d->up != 0 || d->Co > (1 << 24) || d->Tout > d->Tin || d->N > 65535) return false;
    const int64_t tiles = cdiv(d->Tout, UBN);
    if ((int64_t)d->N * tiles < g_up_min_blocks.load(std::memory_order_relaxed)) return false;
    const unsigned inv_up = (unsigned)((0x100000000ull + (unsigned)d->up - 1) / (unsigned)d->up);      // exact floor(x / up), x < 2^25
    dim3 g((unsigned)tiles, (unsigned)d->N);
    const int st = d->up % 4 == 0 ? 0 : d->up % 2 == 0 ? 1 : 2;
    if (d->Ci == 8 * UKC) {
        if (st == 0) conv_up_kernel<0, 8><<<g, 256, 0, s>>>(*d, inv_up);
        else if (st == 1) conv_up_kernel<1, 8><<<g, 256, 0, s>>>(*d, inv_up);
        else conv_up_kernel<2, 8><<<g, 256, 0, s>>>(*d, inv_up);
    } else {
        if (st == 0) conv_up_kernel<0, 0><<<g, 256, 0, s>>>(*d, inv_up);
        else if (st == 1) conv_up_kernel<1, 0><<<g, 256, 0, s>>>(*d, inv_up);
        else conv_up_kernel<2, 0><<<g, 256, 0, s>>>(*d, inv_up);
    }
    g_up_launches.fetch_add(1, std::memory_order_relaxed);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        alive_set_error("alive_conv1d(up): %s", hipGetErrorString(e));
        *rc = ALIVE_ERR_LAUNCH;
    } else {
        *rc = ALIVE_OK;
    }
    return true;
}

extern "C" int alive_conv_up_min_blocks(int blocks) {
    if (blocks > 0) g_up_min_blocks.store(blocks, std::memory_order_relaxed);
    else if (blocks < 0) g_up_min_blocks.store(UP_MIN_BLOCKS, std::memory_order_relaxed);
    return g_up_min_blocks.load(std::memory_order_relaxed);
}

extern "C" int alive_conv_up_launches(int reset) {
    return reset ? g_up_launches.exchange(0, std::memory_order_relaxed) : g_up_launches.load(std::memory_order_relaxed);
}
