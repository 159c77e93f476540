"""NumPy restatement of the device edge of a sparse multi-session converter (csrc/ring.hip; include/alive_vc.h "The device edge"):
the CPU yardstick of alive_ring_push_rows and alive_emit_rows, as tools/gate_ref.py is the gate's.

Everything is integer work except the two int16 edges: int16 -> float32 is an exact conversion and one float32 division by 2^15
(exact too), and float32 -> int16 is a float32 product truncated toward zero to int32 whose low 16 bits are kept.  The latter is
defined here for finite products inside int32's range only (what a hardware conversion makes of the others is the device's business:
the GPU test compares those against alive_float_to_pcm16 of the same floats).
"""
import numpy as np


def fits(chunk_len, ring_len, ld, ld_chunk, ld_x):
    """whether a row's device lengths fit the strides (a row that does not is absent)"""
    cl, rl = int(chunk_len), int(ring_len)
    return 0 <= cl <= rl and cl <= ld_chunk and rl <= ld and rl <= ld_x


def push_rows(ring, chunks, chunk_len, ring_len, present, x, seg_len=None, S=1, world_on=None):
    """one alive_ring_push_rows call on copies: ring int16 [N, ld] in time order, chunks int16 [N, ld_chunk], x float32 [N, ld_x] ->
    dict(ring, x, seg_len_tick (int32 [N * S], None without seg_len), world_tick (int32 [N], None without world_on)).
    A row that takes part (present, lengths fit): ring[n, :rl] = ring[n, cl:rl] ++ chunks[n, :cl], x[n, :rl] = ring / 32768 in
    float32, x[n, rl:] = 0; an absent row keeps its ring and its row of x, and gets zeros in the masked arrays."""
    ring = np.array(ring, dtype=np.int16)
    x = np.array(x, dtype=np.float32)
    chunks = np.asarray(chunks, dtype=np.int16)
    n = ring.shape[0]
    live = np.array([bool(present[r]) and fits(chunk_len[r], ring_len[r], ring.shape[1], chunks.shape[1], x.shape[1])
                     for r in range(n)])
    for r in range(n):
        if not live[r]:
            continue
        cl, rl = int(chunk_len[r]), int(ring_len[r])
        ring[r, :rl] = np.concatenate([ring[r, cl:rl], chunks[r, :cl]])
        x[r, :rl] = ring[r, :rl].astype(np.float32) / np.float32(32768.0)
        x[r, rl:] = np.float32(0.0)
    out = dict(ring=ring, x=x, seg_len_tick=None, world_tick=None)
    if seg_len is not None:
        out["seg_len_tick"] = (np.asarray(seg_len, dtype=np.int32).reshape(n, S) * live[:, None]).astype(np.int32).reshape(-1)
    if world_on is not None:
        out["world_tick"] = (np.asarray(world_on, dtype=np.int32) * live).astype(np.int32)
    return out


def float_to_pcm16(v):
    """float32 -> int16 as alive_float_to_pcm16: (short)(int)(v * 32768.0f), for finite products inside int32's range"""
    p = np.asarray(v, dtype=np.float32) * np.float32(32768.0)
    return np.trunc(p).astype(np.int64).astype(np.int32).astype(np.int16)      # (the casts wrap: the low 16 bits)


def emit_rows(wave, span_lo, span_len, take, ld_out):
    """alive_emit_rows: wave float32 [N, ld] -> int16 [N, ld_out]; out[n, :span_len[n]] = float_to_pcm16(wave[n, span_lo[n]:][:span_len[n]])
    on taken rows whose span fits the wave and the output row, zeros everywhere else"""
    wave = np.asarray(wave, dtype=np.float32)
    n, ld = wave.shape
    out = np.zeros((n, ld_out), dtype=np.int16)
    for r in range(n):
        lo, ln = int(span_lo[r]), int(span_len[r])
        if take[r] and lo >= 0 and 0 <= ln <= ld_out and lo + ln <= ld:
            out[r, :ln] = float_to_pcm16(wave[r, lo:lo + ln])
    return out


def session_ring(chunks, buffersize, chunk_len):
    """what a session's ring holds after it supplied `chunks` (a list of int16 arrays of chunk_len samples), whatever ticks they
    arrived in: its last `buffersize` chunks in order, zeros in front while it fills"""
    ring = np.zeros(buffersize * chunk_len, dtype=np.int16)
    last = [np.asarray(c, dtype=np.int16) for c in chunks[-buffersize:]] if chunks else []
    if last:
        tail = np.concatenate(last)
        ring[len(ring) - len(tail):] = tail
    return ring
