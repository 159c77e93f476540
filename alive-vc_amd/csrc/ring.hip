// The device edge of a sparse MultiStreamConverter (module/multistream.py: MultiStreamConverter(sparse=True)): the sessions' int16 rings
// live on the device and stand still for a session that sent nothing this tick, and the emitted centre spans are cut on the device.
//   the input edge, one block per row     alive_ring_push_rows   (once per tick, before the captured step)
//   the output edge                       alive_emit_rows        (after the step, on its final waves)
// The ring is kept in TIME ORDER and advanced in place: a row's new ring is ring[cl:rl] ++ chunk[0:cl].  The shift moves data towards
// lower addresses, so the block walks the row in ascending tiles: every thread reads its part of a tile (from cl further on, or from the
// chunk) into registers, the block meets at a barrier, and only then is the tile written.  A tile's stores end where the next tile's
// loads begin or before it, and a later tile's stores come after that tile's own barrier, which every thread reaches only after its
// loads of all earlier tiles: no sample is overwritten before it is read.  The float input row is written from the same registers.
// Plain C++, no atomics; 16-byte accesses where the row's lengths and the strides are multiples of 8 samples, scalar ones otherwise.
#include "common.h"

namespace {

constexpr int PUSH_THREADS = 256;

// the sample that row position j holds after the push
__device__ __forceinline__ short pushed_sample(const short* ring, const short* chunk, int j, int cl, int rl) {
    const int s = j + cl;                                    // (j < rl <= ld and cl <= rl: no overflow)
    return s < rl ? ring[s] : chunk[s - rl];
}

__global__ __launch_bounds__(PUSH_THREADS) void ring_push_rows_kernel(short* __restrict__ ring, int ld, const short* __restrict__ chunks,
                                                                      int ld_chunk, const int* __restrict__ chunk_len,
                                                                      const int* __restrict__ ring_len,
                                                                      const unsigned char* __restrict__ present, float* __restrict__ x,
                                                                      int ld_x, int S, const int* __restrict__ seg_len,
                                                                      int* __restrict__ seg_len_tick, const int* __restrict__ world_on,
                                                                      int* __restrict__ world_tick, int vec_ok) {
    const int n = blockIdx.x, tid = threadIdx.x;
    const int cl = chunk_len[n], rl = ring_len[n];
    // (block-uniform) a row takes part if it sent a chunk and its lengths fit the strides; device data never leads outside a row
    const bool live = present[n] != 0 && cl >= 0 && cl <= rl && rl <= ld && rl <= ld_x && cl <= ld_chunk;
    if (seg_len_tick)
        for (int s = tid; s < S; s += PUSH_THREADS) seg_len_tick[(size_t)n * S + s] = live ? seg_len[(size_t)n * S + s] : 0;
    if (world_tick && tid == 0) world_tick[n] = live ? world_on[n] : 0;
    if (!live) return;                                       // an absent row: ring and x neither read nor written
    short* r = ring + (size_t)n * ld;
    const short* c = chunks + (size_t)n * ld_chunk;
    float* xr = x + (size_t)n * ld_x;
    if (vec_ok && (cl & 7) == 0 && (rl & 7) == 0) {          // every group of 8 samples comes whole from the ring or from the chunk
        for (int base = 0; base < rl; base += PUSH_THREADS * 8) {
            const int j = base + tid * 8;
            uint4 v = make_uint4(0u, 0u, 0u, 0u);
            if (j < rl) {
                const int s = j + cl;
                v = s < rl ? *reinterpret_cast<const uint4*>(r + s) : *reinterpret_cast<const uint4*>(c + (s - rl));
            }
            __syncthreads();                                 // the tile is in registers: now it may be overwritten
            if (j < rl) {
                *reinterpret_cast<uint4*>(r + j) = v;
                const unsigned w[4] = {v.x, v.y, v.z, v.w};
                float f[8];
                for (int q = 0; q < 4; ++q) {
                    f[2 * q] = alive_pcm16_as_float((short)(w[q] & 0xffffu));
                    f[2 * q + 1] = alive_pcm16_as_float((short)(w[q] >> 16));
                }
                *reinterpret_cast<float4*>(xr + j) = make_float4(f[0], f[1], f[2], f[3]);
                *reinterpret_cast<float4*>(xr + j + 4) = make_float4(f[4], f[5], f[6], f[7]);
            }
        }
    } else {
        for (int base = 0; base < rl; base += PUSH_THREADS * 4) {
            short v[4];
            for (int q = 0; q < 4; ++q) {
                const int j = base + q * PUSH_THREADS + tid;
                v[q] = j < rl ? pushed_sample(r, c, j, cl, rl) : (short)0;
            }
            __syncthreads();
            for (int q = 0; q < 4; ++q) {
                const int j = base + q * PUSH_THREADS + tid;
                if (j < rl) {
                    r[j] = v[q];
                    xr[j] = alive_pcm16_as_float(v[q]);
                }
            }
        }
    }
    for (int j = rl + tid; j < ld_x; j += PUSH_THREADS) xr[j] = 0.0f;
}

// grid (ceil(ld_out / 2048), N): thread t of a block owns 8 consecutive samples of the row's output
__global__ __launch_bounds__(256) void emit_rows_kernel(const float* __restrict__ wave, int ld, const int* __restrict__ span_lo,
                                                        const int* __restrict__ span_len, const unsigned char* __restrict__ take,
                                                        short* __restrict__ out, int ld_out, int vec_ok) {
    const int n = blockIdx.y;
    const int i0 = (blockIdx.x * 256 + threadIdx.x) * 8;     // (< ld_out + 2048: no overflow for ld_out < 2^30)
    if (i0 >= ld_out) return;
    int lo = span_lo[n], len = span_len[n];
    // a row that is not taken, or whose span leaves the wave or the output row, is written as zeros
    if (take[n] == 0 || lo < 0 || len < 0 || len > ld_out || (int64_t)lo + len > ld) lo = len = 0;
    const float* w = wave + (size_t)n * ld + lo;
    short v[8];
    for (int q = 0; q < 8; ++q) v[q] = i0 + q < len ? alive_float_as_pcm16(w[i0 + q]) : (short)0;
    short* o = out + (size_t)n * ld_out + i0;
    if (vec_ok && i0 + 8 <= ld_out) {
        uint4 p;
        p.x = (unsigned)(unsigned short)v[0] | ((unsigned)(unsigned short)v[1] << 16);
        p.y = (unsigned)(unsigned short)v[2] | ((unsigned)(unsigned short)v[3] << 16);
        p.z = (unsigned)(unsigned short)v[4] | ((unsigned)(unsigned short)v[5] << 16);
        p.w = (unsigned)(unsigned short)v[6] | ((unsigned)(unsigned short)v[7] << 16);
        *reinterpret_cast<uint4*>(o) = p;
    } else {
        for (int q = 0; q < 8 && i0 + q < ld_out; ++q) o[q] = v[q];
    }
}

inline bool aligned16(const void* p) { return ((uintptr_t)p & 15u) == 0; }

}  // namespace

extern "C" int alive_ring_push_rows(int16_t* ring, int N, int ld, const int16_t* chunks, int ld_chunk, const int* chunk_len,
                                    const int* ring_len, const unsigned char* present, float* x, int ld_x, int S, const int* seg_len,
                                    int* seg_len_tick, const int* world_on, int* world_tick, void* stream) {
    ALIVE_CHECK_ARG(ring && chunks && chunk_len && ring_len && present && x, "alive_ring_push_rows: null pointer");
    ALIVE_CHECK_ARG((seg_len == nullptr) == (seg_len_tick == nullptr), "alive_ring_push_rows: seg_len and seg_len_tick go together");
    ALIVE_CHECK_ARG((world_on == nullptr) == (world_tick == nullptr), "alive_ring_push_rows: world_on and world_tick go together");
    ALIVE_CHECK_ARG(N > 0 && ld > 0 && ld_chunk > 0 && ld_x > 0 && S > 0 && (int64_t)N * S < (int64_t)1 << 31,
                    "alive_ring_push_rows: bad args");
    const int vec_ok = aligned16(ring) && aligned16(chunks) && aligned16(x) && ld % 8 == 0 && ld_chunk % 8 == 0 && ld_x % 8 == 0;
    ring_push_rows_kernel<<<N, PUSH_THREADS, 0, (hipStream_t)stream>>>(ring, ld, chunks, ld_chunk, chunk_len, ring_len, present, x, ld_x,
                                                                       S, seg_len, seg_len_tick, world_on, world_tick, vec_ok);
    ALIVE_CHECK_LAUNCH("alive_ring_push_rows");
    return ALIVE_OK;
}

extern "C" int alive_emit_rows(const float* wave, int N, int ld, const int* span_lo, const int* span_len, const unsigned char* take,
                               int16_t* out, int ld_out, void* stream) {
    ALIVE_CHECK_ARG(wave && span_lo && span_len && take && out, "alive_emit_rows: null pointer");
    ALIVE_CHECK_ARG(N > 0 && N <= 65535 && ld > 0 && ld_out > 0 && ld_out < (1 << 30), "alive_emit_rows: bad args");
    const int vec_ok = aligned16(out) && ld_out % 8 == 0;
    emit_rows_kernel<<<dim3(cdiv(ld_out, 2048), N), 256, 0, (hipStream_t)stream>>>(wave, ld, span_lo, span_len, take, out, ld_out, vec_ok);
    ALIVE_CHECK_LAUNCH("alive_emit_rows");
    return ALIVE_OK;
}
