"""The stationary-input form of the split-bf16 transposed conv (csrc/conv_up.hip: KW 1, up > 1, Ci a multiple of 32 up to 256, only a
bias) against the tiled kernel it replaces (csrc/conv_split.hip through alive_conv1d_tiled):
  * bit for bit on seeded Gaussian data, with and without a bias: ups[0]'s own shape on two windows; rate 8 with Tin on either side of
    the column tile BN = 64 (63, 64, 65, 130); one and two channel blocks; ragged rows (Co 40 at rate 10: the last MFMA row group is
    partly beyond Co and channels straddle two row groups; Co 24 at rates 2, 3, 4, 8);
  * on both sides of the dispatch threshold of 512 blocks of 64 columns, which form ran is read from alive_conv_up_launches;
  * exact operands (small integers, at most 8 significant bits, every partial sum exact in fp32): equal to the float64 product;
  * Y filled with NaN between two guard bands: the bands keep their pattern, every element of Y is written;
  * 20 launches of the first shape give identical bits.
The small shapes reach the new kernel through alive_conv_up_min_blocks (test only); every test states the form that ran and asserts it
on the launch counter.  Needs an MI355X."""
import ctypes as C

import pytest
import torch

from module import _native as nat
from module._pack import pack_convT_split

pytestmark = pytest.mark.gpu
DEV = "cuda"
BN = 64                  # columns per block of conv_up.hip
MIN_BLOCKS = 512         # its dispatch threshold: N * ceil(Tout / BN)
BAND = 4096              # floats per guard band (a multiple of 4: Y stays 16-byte aligned)
GUARD = 0x5A5A5A5A


@pytest.fixture
def reach():
    """the new form at any grid size, for the duration of one test"""
    L = nat.lib()
    assert L.alive_conv_up_min_blocks(0) == MIN_BLOCKS
    L.alive_conv_up_min_blocks(1)
    yield
    assert L.alive_conv_up_min_blocks(-1) == MIN_BLOCKS


def operands(n, ci, co, up, tin, bias, seed, integers=False):
    """x [n, ci, tin], ConvTranspose1d weight [ci, co, up] and bias [co] in the reference layout, packed for alive_conv1d"""
    g = torch.Generator().manual_seed(seed)
    if integers:
        x = torch.randint(-8, 9, (n, ci, tin), generator=g).float()
        w = torch.randint(-8, 9, (ci, co, up), generator=g).float()
        b = torch.randint(-64, 65, (co,), generator=g).float() if bias else None
    else:
        x = torch.randn(n, ci, tin, generator=g)
        w = torch.randn(ci, co, up, generator=g) * (ci ** -0.5)
        b = torch.randn(co, generator=g) if bias else None
    W, brows = pack_convT_split(w, b if bias else torch.zeros(co))
    return x.to(DEV), w, b, W.to(DEV), (brows.to(DEV) if bias else None)


def launch(entry, x, W, brows, co, up, y):
    n, ci, tin = x.shape
    d = nat.AliveConv()
    d.W, d.bias, d.X = nat.ptr(W), nat.ptr(brows), nat.ptr(x)
    d.N, d.Ci, d.Tin, d.Co, d.K_pad = n, ci, tin, co * up, W.shape[1] * 32
    d.precision, d.Ci_pad = 1, ci
    d.KW, d.stride, d.dil, d.pad_left, d.pad_mode = 1, 1, 1, 0, 0
    d.Tout, d.up, d.act = tin, up, 0
    d.Y = y.data_ptr()
    nat.check(getattr(nat.lib(), entry)(C.byref(d), nat.stream()), entry)


def run(entry, x, W, brows, co, up):
    """(Y, launches that took the new form)"""
    n, _, tin = x.shape
    y = torch.full((n, co, tin * up), float("nan"), device=DEV)
    L = nat.lib()
    L.alive_conv_up_launches(1)
    launch(entry, x, W, brows, co, up, y)
    torch.cuda.synchronize()
    return y, L.alive_conv_up_launches(1)


def same_bits(a, b):
    return bool(torch.equal(a.view(torch.int32), b.view(torch.int32)))


# (n, ci, co, up, tin)
CASES = [(2, 256, 256, 10, 450)] + \
        [(3, 256, 64, 8, t) for t in (BN - 1, BN, BN + 1, 2 * BN + 2)] + \
        [(2, 32, 8, 8, 100), (2, 64, 8, 8, 100)] + \
        [(2, 64, 4, 10, 70)] + [(2, 64, 24 // r, r, 70) for r in (2, 3, 4, 8)]


@pytest.mark.parametrize("bias", (True, False), ids=("bias", "nobias"))
@pytest.mark.parametrize("case", CASES, ids=lambda c: "n%d_ci%d_co%d_up%d_t%d" % c)
def test_new_form_equals_the_tiled_kernel_bit_for_bit(reach, case, bias):
    """alive_conv1d runs conv_up.hip (one launch counted), alive_conv1d_tiled runs conv_split.hip (none counted)"""
    n, ci, co, up, tin = case
    x, _, _, W, brows = operands(n, ci, co, up, tin, bias, 100 + ci + co * up + tin)
    y_new, took_new = run("alive_conv1d", x, W, brows, co, up)
    y_old, took_old = run("alive_conv1d_tiled", x, W, brows, co, up)
    assert (took_new, took_old) == (1, 0)
    assert not bool(torch.isnan(y_old).any()) and not bool(torch.isnan(y_new).any())
    assert same_bits(y_new, y_old), (y_new - y_old).abs().max().item()


def test_dispatch_threshold_picks_the_form():
    """The rule, not luck: with Tin = 7 * 64 + 1 (8 column tiles) 64 windows make 512 blocks -- the new form -- and 63 windows 504 --
    the tiled kernel; the test hook that lowers the threshold is not in force here.  Both agree with alive_conv1d_tiled bit for bit."""
    assert nat.lib().alive_conv_up_min_blocks(0) == MIN_BLOCKS
    ci, co, up, tin = 32, 3, 8, 7 * BN + 1
    for n, want in ((MIN_BLOCKS // 8, 1), (MIN_BLOCKS // 8 - 1, 0)):
        x, _, _, W, brows = operands(n, ci, co, up, tin, True, n)
        y, took = run("alive_conv1d", x, W, brows, co, up)
        y_old, took_old = run("alive_conv1d_tiled", x, W, brows, co, up)
        assert (took, took_old) == (want, 0), (n, took, took_old)
        assert same_bits(y, y_old)


@pytest.mark.parametrize("co,up", ((8, 10), (16, 8), (8, 3)), ids=("up10", "up8", "up3"))
def test_exact_operands_equal_the_float64_product(reach, co, up):
    """new form (one launch counted).  x, w in [-8, 8], bias in [-64, 64], all integers: the lo planes are zero and every partial sum is
    below 256 * 64 + 64 < 2^24, so fp32 accumulation is exact in any order and the result must BE the float64 product"""
    n, ci, tin = 2, 256, 2 * BN + 2
    x, w, b, W, brows = operands(n, ci, co, up, tin, True, 7 + up, integers=True)
    y, took = run("alive_conv1d", x, W, brows, co, up)
    assert took == 1
    ref = torch.einsum("nit,ioj->notj", x.cpu().double(), w.double()) + b.double()[None, :, None, None]
    assert bool(torch.equal(y.cpu().double(), ref.reshape(n, co, tin * up)))


@pytest.mark.parametrize("case", ((2, 256, 256, 10, 450), (3, 256, 64, 8, BN + 1), (2, 64, 4, 10, 70), (2, 64, 8, 3, 70)),
                         ids=lambda c: "n%d_ci%d_co%d_up%d_t%d" % c)
def test_writes_all_of_y_and_nothing_else(reach, case):
    """new form (one launch counted): Y lies between two guard bands and starts as NaN"""
    n, ci, co, up, tin = case
    x, _, _, W, brows = operands(n, ci, co, up, tin, True, 31)
    numel = n * co * tin * up
    raw = torch.full((numel + 2 * BAND,), GUARD, dtype=torch.int32, device=DEV)
    y = raw[BAND:BAND + numel].view(torch.float32)
    y.fill_(float("nan"))
    L = nat.lib()
    L.alive_conv_up_launches(1)
    launch("alive_conv1d", x, W, brows, co, up, y)
    torch.cuda.synchronize()
    assert L.alive_conv_up_launches(1) == 1
    assert bool((raw[:BAND] == GUARD).all() and (raw[-BAND:] == GUARD).all()), "wrote outside Y"
    assert not bool(torch.isnan(y).any()), "an element of Y was not written"
    y_old, _ = run("alive_conv1d_tiled", x, W, brows, co, up)
    assert same_bits(y.view(n, co, tin * up), y_old)


def test_twenty_launches_give_identical_bits(reach):
    """new form (20 launches counted): the run-time companion of the rule that a row tile's accumulators are read before the next
    tile's chains start (csrc/conv_up.hip header)"""
    n, ci, co, up, tin = CASES[0]
    x, _, _, W, brows = operands(n, ci, co, up, tin, True, 5)
    first, took = run("alive_conv1d", x, W, brows, co, up)
    for _ in range(19):
        y, t1 = run("alive_conv1d", x, W, brows, co, up)
        took += t1
        assert same_bits(y, first)
    assert took == 20
