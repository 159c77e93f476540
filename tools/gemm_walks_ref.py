"""Host restatement of how alive_gemm_planes (csrc/gemm_planes.hip) addresses its B operand, and the builders the plane-GEMM walk
tests share (tests/test_host_gemm_walks.py on the CPU, tests/test_gpu_gemm_walks.py on the device).

In the custom row forms (AliveGemm.b_row != 0) the kernel's LDS-DMA reads, per plane, column and k-block, 32 elements (64 B) at
    plane * b_plane + n * b_win + t * b_row + walk            (column = n * T + t, clamped to the last real column)
where `walk` comes from make_walk / StepWalk::advance: `ncb` k-blocks per tap, b_blk apart, then one row segment (32 elements) on.
Only the column is clamped, so a buffer that is one row short is read out of bounds: `operand_extent` says how many elements a
geometry reads, and the GPU tests assert it against the buffer they allocate before every launch.  `piece_offsets` follows the
kernels step by step -- one walk, 32 deep, in the split-plane kernels; two walks one k-block apart, both advanced twice per 64-deep
step, in the one-plane KB2 kernel -- so a geometry whose step straddles a tap (odd ncb) is restated the way the kernel runs it.

Everything here is CPU torch; nothing touches the device.
"""
from dataclasses import dataclass, field

import torch

GM = GN = 128
GK = 32


def cdiv(a, b):
    return (a + b - 1) // b


def pad32(c):
    return (c + 31) // 32 * 32


def pad_cols(cols):
    return cdiv(cols, GN) * GN


@dataclass
class Geo:
    """the AliveGemm fields that place the B operand"""
    N: int
    T: int
    Ci: int
    Co: int
    planes: int
    b_plane: int = 0
    b_win: int = 0
    b_row: int = 0
    b_cblk: int = 0
    b_blk: int = 0

    @property
    def cols(self):
        return self.N * self.T

    def placement(self):
        return dict(b_plane=self.b_plane, b_win=self.b_win, b_row=self.b_row, b_cblk=self.b_cblk, b_blk=self.b_blk)


def make_walk(g):
    """(b_blk, b_tap, ncb) of make_walk in gemm_planes.hip"""
    if g.b_row == 0:
        return pad_cols(g.cols) * GK, 0, pad32(g.Ci) // GK
    if g.b_cblk == 0:
        return 0, GK, 1
    return g.b_blk, GK, g.b_cblk


class StepWalk:
    def __init__(self, walk):
        self.b_blk, self.b_tap, self.ncb = walk
        self.b = 0
        self.blk = 0

    def advance(self):
        self.b += self.b_blk
        self.blk += 1
        if self.blk == self.ncb:
            self.blk = 0
            self.b += self.b_tap - self.ncb * self.b_blk


def is_kb2(g):
    """one plane with K a multiple of 64, at least 128: the 64-deep step in the two-plane kernel's slots"""
    return g.planes == 1 and pad32(g.Ci) % 64 == 0 and pad32(g.Ci) >= 128


def kernel_instance(g):
    """which kernel alive_gemm_planes launches for this geometry (its dispatch conditions, no fp16 split planes):
    "persistent" (gemm_planes_lw_kernel), "KB2" (the one-tile kernel with 64-deep one-plane steps) or "one-tile" """
    ntiles = cdiv(g.Co, GM) * cdiv(g.cols, GN)
    nsteps = pad32(g.Ci) // GK
    span = g.planes * pad_cols(g.cols) * pad32(g.Ci) if g.b_row == 0 else g.planes * g.b_plane
    can_persist = ntiles >= 512 and span * 2 < (1 << 32)
    if g.planes == 1:
        return "KB2" if is_kb2(g) else "one-tile"
    if g.planes == 2:
        return "one-tile"
    return "persistent" if can_persist and nsteps >= 3 else "one-tile"


def piece_offsets(g):
    """the walk's B offset (elements) of every k-block, in K order, as the kernel that runs `g` produces them"""
    walk = make_walk(g)
    offs = []
    if is_kb2(g):
        w0, w1 = StepWalk(walk), StepWalk(walk)
        w1.advance()
        for _ in range(pad32(g.Ci) // (2 * GK)):
            offs += [w0.b, w1.b]
            w0.advance(), w0.advance(), w1.advance(), w1.advance()
    else:
        w0 = StepWalk(walk)
        for _ in range(pad32(g.Ci) // GK):
            offs.append(w0.b)
            w0.advance()
    return offs


def operand_indices(g):
    """int64 [planes][cols][K / 32]: the element index at which the 32-element piece (plane, column, k-block) starts.  (Columns past
    the end repeat the last real column in the custom forms, so the real columns are every address the DMA forms.)"""
    offs = torch.tensor(piece_offsets(g), dtype=torch.int64)
    col = torch.arange(g.cols, dtype=torch.int64)
    pl = torch.arange(g.planes, dtype=torch.int64)
    if g.b_row == 0:
        kb = pad32(g.Ci) // GK
        base = (pl.view(-1, 1) * kb * pad_cols(g.cols) + col.view(1, -1)) * GK            # planes_at(plane, col, 0, cols_pad, kpad)
    else:
        n, t = col // g.T, col % g.T
        base = pl.view(-1, 1) * g.b_plane + (n * g.b_win + t * g.b_row).view(1, -1)
    return base.unsqueeze(2) + offs.view(1, 1, -1)


def operand_extent(g):
    """elements a launch of `g` reads from its B buffer: the largest piece start + 32"""
    return int(operand_indices(g).max()) + GK


def gather(buf, g):
    """the operand as the kernel sees it: flat 16-bit buffer -> [planes][cols][K]"""
    idx = operand_indices(g).unsqueeze(3) + torch.arange(GK, dtype=torch.int64)
    return buf.reshape(-1)[idx.reshape(-1)].view(g.planes, g.cols, -1)


# ---- operands ----------------------------------------------------------------------------------------------------------
def split_bits(x, planes):
    """fp32 tensor -> [planes] + x.shape int16: the bits of its split-bf16 planes (module/_pack.py::split_bf16), or of its ONE fp16
    plane (planes = 1, saturated at +-65504): what alive_to_planes stores per element"""
    from module._pack import split_bf16
    if planes == 1:
        return x.float().clamp(-65504.0, 65504.0).half().view(torch.int16).unsqueeze(0)
    return torch.stack([h.view(torch.int16) for h in split_bf16(x, planes)], 0)


def planes_image(x, planes):
    """alive_to_planes on the host: fp32 [N][C][T] -> int16 [planes][C_pad / 32][cols_pad][32], zero padded (csrc/planes_layout.h)"""
    n, c, t = x.shape
    cp, cpd = pad32(c), pad_cols(n * t)
    full = torch.zeros(cpd, cp, dtype=torch.float32)
    full[:n * t, :c] = x.float().permute(0, 2, 1).reshape(n * t, c)
    return split_bits(full, planes).view(planes, cpd, cp // 32, 32).permute(0, 2, 1, 3).contiguous()


def unfolded_bits(x_unf, planes):
    """the unfolded operand [N][K][T] of check A as [planes][cols][K] bits: what `gather` must reproduce"""
    n, k, t = x_unf.shape
    return split_bits(x_unf.permute(0, 2, 1).reshape(n * t, k), planes)


def frames_row_len(hop, ci, t):
    return ((t - 1) * hop + ci + 7) // 8 * 8


def frames_operand(sig, hop, ci, t, co, planes):
    """form 1 (overlapping k-contiguous rows: the STFT): sig fp32 [N][Lrow] -> (flat int16 buffer of `planes` planes of it, Geo,
    the frames unfolded [N][ci][t])"""
    n, lrow = sig.shape
    assert lrow == frames_row_len(hop, ci, t)
    g = Geo(n, t, ci, co, planes, b_plane=n * lrow, b_win=lrow, b_row=hop)
    idx = torch.arange(t).view(1, -1) * hop + torch.arange(ci).view(-1, 1)              # [ci][t]
    return split_bits(sig, planes).reshape(-1).contiguous(), g, sig[:, idx].contiguous()


def conv_geo(n, c, length, r, co, planes):
    """form 2 (Conv1d(k == stride == r) over the k-blocked plane image of x [n][c][length]): the Geo networks.hip::decoder_run fills"""
    cpad, rows = pad32(c), pad_cols(n * length)
    return Geo(n, length // r, r * cpad, co, planes, b_plane=rows * cpad, b_win=length * 32, b_row=r * 32, b_cblk=cpad // 32,
               b_blk=rows * 32)


def conv_unfold(x, r):
    """x [n][c][length] -> the tap-major patches [n][r * c_pad][length // r], k = tap * c_pad + channel (the K order of
    module/_pack.py::pack_conv_split), zero in the channel padding"""
    n, c, length = x.shape
    cpad, t = pad32(c), length // r
    out = torch.zeros(n, r, cpad, t, dtype=torch.float32)
    out[:, :, :c, :] = x[:, :, :t * r].reshape(n, c, t, r).permute(0, 3, 1, 2)
    return out.reshape(n, r * cpad, t)


# ---- the cases -----------------------------------------------------------------------------------------------------------
# form 1: id -> (hop, Ci, N, T, Co, planes tried, kernel per planes)
FRAMES = {
    "1a": (8, 32, 1, 40, 40, (3, 2)),          # one K-step (fewer than the ring depth), one ragged tile, columns 40.. clamped
    "1b": (24, 96, 3, 50, 200, (3, 2)),        # 150 columns: tile 0 holds the row changes n = 0 -> 1 -> 2; ragged Co; three steps = NS
    "1c": (320, 1280, 2, 64, 1282, (3, 2)),    # the production geometry at the smallest full tile: exactly 128 columns
    "1d": (8, 64, 2, 129, 64, (3, 2)),         # two steps, two column tiles
    "1e": (8, 96, 4, 1024, 2048, (3,)),        # 512 tiles: the persistent kernel
    "1f": (8, 96, 4, 1030, 2048, (3,)),        # 33 column tiles: the last has 24 columns, windows change row inside tiles
}
FRAMES_KERNEL = {("1e", 3): "persistent", ("1f", 3): "persistent"}          # every other (case, planes): one-tile

# form 2: id -> (C, r, N, len, Co, planes)
CONVS = {
    "down2": (64, 8, 2, 1040, 256, 2),         # the downs[2] geometry
    "down3": (256, 10, 1, 1300, 256, 2),       # the downs[3] geometry
    "chpad": (40, 3, 3, 400, 72, 2),           # c_pad 64 with channel padding present, len no multiple of 128, len % r != 0
    "ncb1": (32, 2, 1, 300, 40, 2),
    "ncb3": (96, 2, 2, 260, 128, 2),
    "h-ncb1": (32, 4, 2, 130, 72, 1),          # one plane, K = 128: KB2
    "h-ncb3": (96, 2, 2, 260, 128, 1),         # K = 192: a 64-deep KB2 step that straddles a tap
    "h-ncb2": (64, 8, 2, 1040, 256, 1),        # KB2, the production pairing
    "h-k96": (32, 3, 2, 200, 72, 1),           # K = 96: the 32-deep one-plane kernel
    "persist": (32, 3, 4, 3074, 2048, 3),      # 4 x 1024 columns x 16 row tiles: the persistent kernel
}
CONVS_KERNEL = {"h-ncb1": "KB2", "h-ncb3": "KB2", "h-ncb2": "KB2", "persist": "persistent"}      # the others: one-tile

# y_split: (Co, y_split, Ci, N, T, planes tried)
SPLITS = [
    (168, 128, 64, 3, 50, (3, 2)),             # the second tensor has 40 rows, one ragged tile
    (300, 256, 96, 2, 129, (3, 2)),
    (768, 512, 641, 1, 130, (3, 2)),           # production
    (2120, 1024, 96, 1, 3968, (3,)),           # 17 x 31 = 527 tiles: persistent; ragged last row tile in Y2
]
# act 4 on the standard walk: (Co, Ci, N, T); the form-1 pairing (case 1c) is a test of its own
MAGS = [(66, 64, 2, 40), (2050, 96, 1, 3968)]
# Pout of the persistent kernel: (Co, Ci, N, T)
POUTS = [(2048, 96, 4, 1024), (2120, 96, 4, 1024), (2120, 96, 2, 2045)]


def gauss(name, shape, scale=1.0):
    from module import synthetic
    return synthetic.gaussian(name, 7, shape, scale)


def frames_case(cid, planes):
    """seeded inputs of a form-1 case: signal, weight [Co][Ci][1], bias, the raw buffer, its Geo and the unfolded frames"""
    hop, ci, n, t, co, _ = FRAMES[cid]
    sig = gauss(f"gw.sig.{cid}", (n, frames_row_len(hop, ci, t)))
    buf, g, x_unf = frames_operand(sig, hop, ci, t, co, planes)
    return dict(sig=sig, w=gauss(f"gw.w.{cid}", (co, ci, 1), ci ** -0.5), b=gauss(f"gw.b.{cid}", (co,), 0.1), buf=buf, geo=g, x_unf=x_unf)


def conv_case(cid):
    """seeded inputs of a form-2 case: x [N][C][len], weight [Co][C][r], bias, its Geo and the unfolded patches"""
    c, r, n, length, co, planes = CONVS[cid]
    x = gauss(f"gw.x.{cid}", (n, c, length))
    return dict(x=x, r=r, w=gauss(f"gw.cw.{cid}", (co, c, r), (c * r) ** -0.5), b=gauss(f"gw.cb.{cid}", (co,), 0.1),
                geo=conv_geo(n, c, length, r, co, planes), x_unf=conv_unfold(x, r))


# ---- refusals --------------------------------------------------------------------------------------------------------------
@dataclass
class Refusal:
    name: str
    message: str                               # a piece of the library's message
    fields: dict = field(default_factory=dict)             # integer fields that differ from REFUSAL_BASE
    pointers: tuple = ("W", "P", "Y")          # the pointer fields that are set


REFUSAL_BASE = dict(N=1, T=8, Ci=32, Co=256, planes=3, act=0)
_PLACE, _SPLIT, _MAG = "multiples of 8 elements", "y_split must be a multiple of 128 below Co", "act 4 (magnitude of row pairs)"
REFUSALS = [
    Refusal("b_row-not-x8", _PLACE, dict(b_row=12, b_win=64, b_plane=64)),
    Refusal("b_row-ragged-ci", "needs Ci % 32 == 0", dict(Ci=40, b_row=8, b_win=64, b_plane=64)),
    Refusal("b_cblk-not-dividing", "must divide Ci / 32 = 3", dict(Ci=96, b_row=32, b_win=256, b_plane=1024, b_cblk=2, b_blk=256)),
    Refusal("b_cblk-without-b_row", "with b_row and b_blk set", dict(b_cblk=1, b_blk=256)),
    Refusal("y_split-not-x128", _SPLIT, dict(y_split=64), ("W", "P", "Y", "Y2")),
    Refusal("y_split-is-co", _SPLIT, dict(y_split=256), ("W", "P", "Y", "Y2")),
    Refusal("y_split-above-co", _SPLIT, dict(y_split=384), ("W", "P", "Y", "Y2")),
    Refusal("y_split-residual", _SPLIT, dict(y_split=128), ("W", "P", "Y", "Y2", "residual")),
    Refusal("y_split-pout", _SPLIT, dict(y_split=128), ("W", "P", "Y", "Y2", "Pout")),
    Refusal("y_split-no-y2", _SPLIT, dict(y_split=128), ("W", "P", "Y")),
    Refusal("act4-odd-co", _MAG, dict(act=4, Co=255), ("W", "P", "Pout")),
    Refusal("act4-bias", _MAG, dict(act=4), ("W", "P", "Pout", "bias")),
    Refusal("act4-two-planes", _MAG, dict(act=4, planes=2), ("W", "P", "Pout")),
]


def refusal_descriptor(cls, case, pointer_of):
    """an AliveGemm (`cls` = module._native.AliveGemm) for a Refusal; pointer_of(name) -> the address to put into a set pointer field"""
    d = cls()
    for k, v in {**REFUSAL_BASE, **case.fields}.items():
        setattr(d, k, v)
    for name in case.pointers:
        setattr(d, name, pointer_of(name))
    return d
