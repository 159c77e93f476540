"""What tests/test_gpu_conv_exact.py relies on, proved on the CPU for every case of its matrix (tests/conv_cases.py): the packed weight
planes decode to the designed hi / lo / zero, the operands split as designed, no partial sum can leave the exact range, torch's
float64 conv equals an int64 sum written index by index, and the dispatch table the cases encode is consistent.  Plus the index
arithmetic of the exact kernel's (channel, tap) split."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as cc  # noqa: E402

from module import _pack  # noqa: E402

CASES = cc.all_exact_operand_cases()


def _as_conv_weight(c, w):
    """[co][ci][kw], or the rows (co, j) of a transposed conv as the 1x1 conv the kernels run"""
    return w.permute(1, 2, 0).reshape(c.co * c.r, c.ci, 1) if c.r else w


def _tap_major(c, w):
    """[rows][ci][kw] -> [rows_pad16][kw * ci_pad32] with k = j * ci_pad + ci, zero padded: the layout the planes are packed in"""
    rows, ci, kw = w.shape
    a = torch.zeros(cc.pad16(rows), kw, cc.pad32(ci), dtype=torch.float64)
    a[:rows, :, :ci] = w.permute(0, 2, 1)
    return a.reshape(cc.pad16(rows), -1)


def test_the_matrix_is_well_formed():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids)
    for c in CASES:
        assert cc.dispatch(c).split("/")[0] == c.kernel, (c.id, cc.dispatch(c))
        assert (c.cols <= cc.SKINNY_COLS) == (c.kernel == "skinny"), c.id
        assert c.regime == "I" or c.prec != "fp16", c.id                       # 2 + 2^-10 is no fp16 number
        assert c.regime != "IIwx" or (c.kernel == "split" and c.prec == "bf16x3"), c.id
        assert c.act is None or c.wexp == -6, c.id
    seen = {cc.dispatch(c) for c in CASES}
    for k in ("exact/bm16", "exact/bm16/upv", "exact/bm64", "exact/bm64/ypl", "exact/bm128", "split/bm64/np1", "split/bm64/np2",
              "split/bm64/np3", "split/bm128/np1", "split/bm128/np2", "split/bm128/np3", "split/bm128/np1/xp", "split/bm128/np2/xp"):
        assert k in seen, k
    for np_ in (0, 2, 3):
        for pw in ("pw", "gen"):
            for wv in (8, 16):
                assert pw == "pw" and wv == 16 or f"skinny/np{np_}/{pw}/waves{wv}" in seen, (np_, pw, wv)


@pytest.mark.parametrize("chunk", range(8))
def test_operands_decode_to_the_designed_planes_and_sums_stay_exact(chunk):
    for c in CASES[chunk::8]:
        o = cc.make(c)
        for k in ("x", "w", "bias", "post_add", "ch_scale", "residual", "skip"):
            if k in o:
                assert torch.equal(o[k].float().double(), o[k]), (c.id, k)              # every operand is an fp32 number
        assert torch.equal(o["w_hi"] + o["w_lo"], o["w"]) and torch.equal(o["x_hi"] + o["x_lo"], o["x"]), c.id
        assert cc.unit_sum_bound(c, o) < 2 ** 24, (c.id, cc.unit_sum_bound(c, o))
        # the activation operand as the kernels split it: hi, lo as designed, nothing left for a third plane
        xs = _pack.split_bf16(o["x"].float(), 3)
        assert torch.equal(xs[0].double(), o["x_hi"]) and torch.equal(xs[1].double(), o["x_lo"]) and not xs[2].any(), c.id
        if c.regime == "I":
            assert torch.equal(o["x"].half().double(), o["x"]), c.id
        if c.prec == "fp32":
            continue
        w = _as_conv_weight(c, o["w"])
        want_hi, want_lo = _tap_major(c, _as_conv_weight(c, o["w_hi"])), _tap_major(c, _as_conv_weight(c, o["w_lo"]))
        for planes in (2, 3):
            P = _pack.unpack_conv_split(_pack.pack_conv_split(w.float(), planes)).double()
            assert torch.equal(P[0], want_hi) and torch.equal(P[1], want_lo), (c.id, planes)
            assert planes == 2 or not P[2].any(), c.id
        if c.regime == "I":
            H = _pack.unpack_conv_split(_pack.pack_conv_split_h(w.float()))[2].contiguous().view(torch.float16).double()
            assert torch.equal(H, want_hi), c.id
        if c.regime != "I":
            assert float((o["w_lo"] != 0).double().mean() + (o["x_lo"] != 0).double().mean()) > 0.6, c.id      # a real lo plane


@pytest.mark.parametrize("chunk", range(8))
def test_the_float64_conv_is_the_integer_sum(chunk):
    for c in CASES[chunk::8]:
        o = cc.make(c)
        wu = 2.0 ** -10 if c.regime in ("IIw", "IIwx") else 2.0 ** c.wexp
        xu = 2.0 ** -10 if c.regime in ("IIx", "IIwx") else 1.0
        q = lambda t, u: (t / u).to(torch.int64)
        for k, u in (("w", wu), ("w_hi", wu), ("w_lo", wu), ("x", xu), ("x_hi", xu), ("x_lo", xu)):
            assert torch.equal(q(o[k], u).double() * u, o[k]), (c.id, k)
        pairs = [("w", "x")]
        if c.kernel == "split" and c.prec == "bf16x3":
            pairs = [("w_hi", "x_hi"), ("w_hi", "x_lo"), ("w_lo", "x_hi")]
        tot = sum(cc.lin_int(c, q(o[a], wu), q(o[b], xu)) for a, b in pairs)
        want = tot.double() * (wu * xu) + o["bias"].view(1, -1, 1)
        v = cc.conv_value(c, o)
        assert torch.equal(v, want), (c.id, cc.first_diff(v, want))
        ref = cc.reference(c, o)
        if c.act is None:
            assert not ref["yerr"].any() and torch.equal(ref["y"].float().double(), ref["y"]), c.id     # the expected output is an fp32 number
        else:
            assert torch.equal(v * 64.0, (v * 64.0).round()), c.id                                  # v: multiples of 1 / 64 ...
            assert 2.0 < float(v.std()) < 4.0 and float(v.abs().max()) < 24.0, (c.id, float(v.std()), float(v.abs().max()))


def test_three_product_sum_differs_from_the_true_product_by_lo_times_lo():
    c = next(c for c in CASES if c.regime == "IIwx" and not c.r)
    o = cc.make(c)
    full = cc.lin(c, o["w"], o["x"]) + o["bias"].view(1, -1, 1)
    assert torch.equal(full - cc.conv_value(c, o), cc.lin(c, o["w_lo"], o["x_lo"])) and (full != cc.conv_value(c, o)).any()


def test_channel_tap_split_of_the_exact_kernel_is_exact_for_every_admitted_k():
    """conv.hip: ci = (k * ceil(2^s / KW)) >> s on 32-bit registers, s = 18 (KW 2 .. 3), 19 (4 .. 7), 20 (8 .. 16), must be k // KW
    for every k < 32768 (alive_conv1d admits Ci * KW < 32768, padded to 16) and every KW in 2 .. 16, without the product
    wrapping.  The fixed s = 20 it replaces wrapped for 2 <= KW <= 7 from about k = 4096 KW on."""
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alive-vc_amd", "csrc", "conv.hip")).read()
    assert "d->KW < 4 ? 18u : d->KW < 8 ? 19u : 20u" in src and "((1u << shift) + d->KW - 1) / d->KW" in src     # the formula proved here
    k = np.arange(32768, dtype=np.uint64)
    for kw in range(2, 17):
        s = 18 if kw < 4 else 19 if kw < 8 else 20
        magic = np.uint64((2 ** s + kw - 1) // kw)
        assert int(k[-1] * magic) < 2 ** 32, kw
        assert np.array_equal(((k * magic) & np.uint64(0xFFFFFFFF)) >> np.uint64(s), k // np.uint64(kw)), kw
        hi = np.uint64((2 ** 32 + kw - 1) // kw)                                # the multiply-high form (conv_split.hip's divisions)
        assert np.array_equal((k * hi) >> np.uint64(32), k // np.uint64(kw)), kw
    old = lambda k, kw: ((k * ((2 ** 20 + kw - 1) // kw)) & 0xFFFFFFFF) >> 20
    assert (old(8190, 2), old(8192, 2), old(16383, 2)) == (4095, 0, 4095)
    for kw in range(8, 17):
        assert all(old(int(q), kw) == int(q) // kw for q in range(0, 32768, 7))


def test_lerp_coord_matches_torch_interpolate_indices():
    """the NumPy lerp_coord the frame-range test builds its column set with, against F.interpolate on a ramp"""
    for lf, tout in ((13, 130), (40, 400), (200, 130), (1, 50)):
        i0, i1 = cc.lerp_coord(np.arange(tout), np.float32(lf) / np.float32(tout), lf)
        ramp = torch.arange(lf, dtype=torch.float32).view(1, 1, -1)
        got = torch.nn.functional.interpolate(ramp, size=tout, mode="linear", align_corners=False)[0, 0].numpy()
        assert np.all(i0 <= got + 1e-4) and np.all(got <= i1 + 1e-4) and np.all(i1 - i0 <= 1) and i1.max() <= lf - 1
