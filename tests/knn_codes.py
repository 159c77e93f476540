"""NumPy reference of the number formats the kNN candidate stages score on (csrc/knn.hip): OCP fp6 e2m3 and its 32-byte slot
image, OCP fp8 e4m3fn, bf16 -- written from the formats' definitions (tables of the representable values, nearest with ties to the
even code), not from the kernels' bit tricks.  tests/test_host_knn_codes.py checks it on the CPU; tests/test_gpu_knn_stage.py decodes
the device's operand images with it and scores them in float64.

Also here: the shapes of the stage tests, shared with the host test that checks on the plans (alive_debug_knn_stage_view, host
arithmetic) that the shapes still reach every edge of the split loop."""
import numpy as np

# ---- e2m3: sign (bit 5) | exponent (2 bits, bias 1) | mantissa (3 bits); exponent 0 is subnormal: m / 8 ----------------------------
E2M3_MAG = np.array([m / 8.0 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 1) for e in range(4) for m in range(8)])   # code & 31 -> |value|
E2M3_MAX = 7.5


def _nearest_even(a, mags):
    """index of the entry of the ascending table `mags` nearest to a >= 0 (float64; a beyond the table saturates at its end); a tie
    between two neighbours goes to the even index"""
    a = np.minimum(np.asarray(a, np.float64), mags[-1])
    mid = (mags[:-1] + mags[1:]) / 2.0                      # exact in float64: the tables have few mantissa bits
    lo = np.searchsorted(mid, a, side="left")               # number of midpoints strictly below a
    tie = (lo < len(mid)) & (mid[np.minimum(lo, len(mid) - 1)] == a)
    return np.where(tie & (lo % 2 == 1), lo + 1, lo).astype(np.int64)


def e2m3_encode(y):
    """codes (uint8, 0 .. 63) of y: round to nearest even on the e2m3 grid, saturating at 7.5; the sign bit is y's (-0.0 -> 32)"""
    y = np.asarray(y, np.float64)
    return (_nearest_even(np.abs(y), E2M3_MAG) | (np.signbit(y).astype(np.int64) << 5)).astype(np.uint8)


def e2m3_decode(codes):
    codes = np.asarray(codes).astype(np.int64)
    return np.where(codes & 32, -1.0, 1.0) * E2M3_MAG[codes & 31]


def slots_pack(codes):
    """codes [..., 32] (0 .. 63) -> the 32-byte slot image [..., 32]: the codes as a little-endian bit stream in bytes 0 .. 23 (code j
    occupies bits 6 j .. 6 j + 5), bytes 24 .. 31 zero"""
    codes = np.asarray(codes).astype(np.uint8)
    assert codes.shape[-1] == 32 and int(codes.max(initial=0)) < 64
    bits = (codes[..., :, None] >> np.arange(6, dtype=np.uint8)) & 1                  # [..., 32, 6], least significant bit first
    stream = bits.reshape(codes.shape[:-1] + (192,))
    body = np.packbits(stream, axis=-1, bitorder="little")                            # [..., 24]
    return np.concatenate([body, np.zeros(codes.shape[:-1] + (8,), np.uint8)], axis=-1)


def slots_unpack(image):
    """the slot image [..., 32] bytes -> (codes [..., 32], tail bytes [..., 8])"""
    image = np.asarray(image, np.uint8)
    assert image.shape[-1] == 32
    stream = np.unpackbits(image[..., :24], axis=-1, bitorder="little").reshape(image.shape[:-1] + (32, 6))
    codes = (stream.astype(np.uint8) << np.arange(6, dtype=np.uint8)).sum(-1).astype(np.uint8)
    return codes, image[..., 24:]


def fp6_image(values):
    """values [rows, 32 n] (already scaled) -> the byte image [rows, 32 n] of their e2m3 codes, slot by slot"""
    values = np.asarray(values, np.float64)
    rows, d = values.shape
    return slots_pack(e2m3_encode(values).reshape(rows, d // 32, 32)).reshape(rows, d)


def fp6_image_decode(image):
    """byte image [rows, 32 n] -> decoded values [rows, 32 n] (float64)"""
    image = np.asarray(image, np.uint8)
    rows, d = image.shape
    codes, _ = slots_unpack(image.reshape(rows, d // 32, 32))
    return e2m3_decode(codes).reshape(rows, d)


# ---- e4m3fn: sign | exponent (4 bits, bias 7) | mantissa (3 bits); no infinities, S.1111.111 is NaN, largest value 448 ---------------
E4M3_MAG = np.array([m / 8.0 * 2.0 ** -6 if e == 0 else (1.0 + m / 8.0) * 2.0 ** (e - 7) for e in range(16) for m in range(8)][:127])


def e4m3_decode(codes):
    """bytes -> float64 values (NaN for 0x7f / 0xff)"""
    codes = np.asarray(codes).astype(np.int64)
    mag = np.append(E4M3_MAG, np.nan)[codes & 127]
    return np.where(codes & 128, -1.0, 1.0) * mag


def e4m3_encode(y):
    """bytes of y: round to nearest even on the e4m3fn grid (|y| <= 448: the stage's operands are unit vectors x 256)"""
    y = np.asarray(y, np.float64)
    assert float(np.abs(y).max(initial=0.0)) <= 448.0
    return (_nearest_even(np.abs(y), E4M3_MAG) | (np.signbit(y).astype(np.int64) << 7)).astype(np.uint8)


def bf16_decode(words):
    """uint16 bf16 patterns -> float32"""
    return (np.asarray(words).astype(np.uint32) << 16).view(np.float32)


# ---- the stage tests' shapes: (N, T, M), the smallest at which each path of the stage exists (tests/test_gpu_knn_stage.py) ----------
SHAPES = [(1, 17, 20), (1, 40, 129), (3, 130, 1000), (1, 384, 2048), (1, 385, 2048), (2, 250, 4097)]
# the subspace stage runs on content-encoder frames (one window of 100 frames) against the same library sizes and one more: 6017 rows
# is the smallest size at which the plan of a single frame block leaves a split empty
SUB_T = 100
SUB_SHAPES = [(1, SUB_T, m) for m in (20, 129, 1000, 2048, 4097, 6017)]
K = 4

VIEW_WORDS = 25


def stage_view(L, Tt, M, k, sub):
    """alive_debug_knn_stage_view as a dict: byte offsets of the stage's buffers in the search workspace, the three plans, constants"""
    import ctypes
    out = (ctypes.c_int64 * VIEW_WORDS)()
    rc = L.alive_debug_knn_stage_view(Tt, M, k, 1 if sub else 0, ctypes.cast(out, ctypes.c_void_p), VIEW_WORDS)
    assert rc == 0, L.alive_last_error()
    o = list(out)
    v = dict(zip(("s_bf16", "s_f8", "clip6", "sub_f6", "sub_g", "cv", "ci", "bytes"), o[:8]))
    for i, name in enumerate(("p16", "p8", "p6")):
        v[name] = dict(zip(("Tt_pad", "tiles_total", "tiles_per_split", "P"), o[8 + 4 * i:12 + 4 * i]))
    v.update(KP=o[20], KP8=o[21], FT=o[22], FT6=o[23], LT=o[24])
    return v


def split_tiles(plan):
    """tiles of every library split of a plan (0: an empty split)"""
    return [max(0, min((s + 1) * plan["tiles_per_split"], plan["tiles_total"]) - s * plan["tiles_per_split"]) for s in range(plan["P"])]
