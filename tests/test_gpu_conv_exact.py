"""alive_conv1d's three kernels (csrc/conv.hip, conv_split.hip, conv_skinny.hip) bit for bit on operands whose right answer has no
rounding (tests/conv_cases.py: the regimes, the references and the derived bounds of the activations and the FiLM output), case by
case along the paths of each kernel.  Every case states the kernel alive_conv1d's dispatch must choose for it; a change of the
thresholds fails test_host_conv_operands.py::test_the_matrix_is_well_formed and the assertion in _run."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import conv_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
_ids = lambda cs: [c.id for c in cs]


def _call(c, o, **over):
    from module import ops
    d = lambda k: o[k].float().to(DEV) if k in o else None
    kw = dict(stride=c.stride, dilation=c.dil, pad_left=c.pad, pad_mode=c.mode, out_len=None if c.r else c.tout, act=c.act,
              post_add=d("post_add"), ch_scale=d("ch_scale"), residual=d("residual"), skip=d("skip"), film=d("film"),
              film_scale_row=o.get("film_scale_row", 0), film_shift_row=o.get("film_shift_row", 0), want_raw=c.want_raw,
              transposed=bool(c.r), precision=c.prec, z_planes=c.zp, y_planes=c.yp)
    if c.xp and "x_planes" not in over:
        kw["x_planes"] = ops.to_planes(d("x"), 1 if c.prec == "fp16" else 2)
    kw.update(over)
    return ops.conv1d(d("x"), d("w"), d("bias"), **kw)


def _where(c, what, a, b, bad=None):
    idx, va, vb = cc.first_diff(a, b, bad)
    return f"{c.id} [{cc.dispatch(c)}] {what}: first mismatch at (n, row, t) = {idx}: kernel {va!r}, reference {vb!r}"


def _check(c, ref, Y, Z):
    """Y against ref["y"]: bit for bit where the reference is exact, within the derived bound behind an activation; Z in its bound"""
    if c.want_raw:
        y, want = Y.cpu().double(), ref["y"]
        assert y.shape == want.shape, (c.id, y.shape, want.shape)
        if not ref["yerr"].any():
            assert torch.equal(Y.cpu(), want.float()), _where(c, "Y", y, want)
        else:
            bad = ~((y - want).abs() <= ref["yerr"])
            assert not bad.any(), _where(c, f"Y beyond the bound of {c.act}", y, want, bad)
    else:
        assert Y is None
    if c.lf and not c.zp:
        z, want = Z.cpu().double(), ref["z"]
        bad = ~((z - want).abs() <= ref["zerr"])
        assert not bad.any(), _where(c, "Z beyond the gelu / FiLM bound", z, want, bad) + f" (bound {float(ref['zerr'][tuple(bad.nonzero()[0])]):.3e})"


def _zp_columns(c, P):
    """the N * Tout columns of a plane-packed second output [planes][Co / 32][cols_pad][32] (16-bit elements)"""
    return P.view(torch.int16).view(1 if c.prec == "fp16" else 2, c.co // 32, (c.cols + 127) // 128 * 128, 32)[:, :, :c.cols]


def _run(c):
    from module import ops
    assert cc.dispatch(c).split("/")[0] == c.kernel, (c.id, cc.dispatch(c))
    print(c.id, "->", cc.dispatch(c))
    o = cc.make(c)
    ref = cc.reference(c, o)
    Y, Z = _call(c, o)
    _check(c, ref, Y, Z)
    if c.yp:
        # the plane image of Y: the bytes of alive_to_planes(Y), zeros in the padding columns and channels
        want = ops.to_planes(Y, c.yp)
        assert torch.equal(Z, want), f"{c.id} [{cc.dispatch(c)}]: Yp differs from to_planes(Y) at byte {int((Z != want).nonzero()[0])}"
        P = Z.view(torch.int16).view(c.yp, cc.pad32(c.co) // 32, (c.cols + 127) // 128 * 128, 32)
        assert not P[:, :, c.cols:].any() and not P.permute(0, 2, 1, 3).reshape(c.yp, -1, cc.pad32(c.co))[:, :, c.co:].any(), c.id
    if c.zp:
        # the plane-packed second output: the bytes of to_planes of the fp32 Z of the same conv (1 plane fp16, 2 planes bf16)
        Yf, Zf = _call(c, o, z_planes=False)
        _check(cc.replace(c, zp=False), ref, Yf, Zf)
        # (the kernel writes the columns it computes: the padding columns behind N * Tout, which to_planes zeroes, are the caller's)
        got, want = _zp_columns(c, Z), _zp_columns(c, ops.to_planes(Zf, 1 if c.prec == "fp16" else 2))
        assert torch.equal(got, want), (f"{c.id} [{cc.dispatch(c)}]: Zp differs from to_planes(Z) at (plane, channel block, column, channel) "
                                        f"{tuple(int(i) for i in (got != want).nonzero()[0])}")
    if c.xp:
        Y2, Z2 = _call(c, o, x_planes=None)                                  # the fp32-staged kernel of the same conv: the same bits
        for a, b in ((Y, Y2), (_zp_columns(c, Z), _zp_columns(c, Z2)) if c.zp else (Z, Z2)):
            assert (a is None and b is None) or torch.equal(a, b), f"{c.id}: plane input and fp32 input differ"


@pytest.mark.parametrize("c", cc.exact_cases(), ids=_ids(cc.exact_cases()))
def test_exact_kernel(c):
    """conv.hip on regime I: tile rows, padded reduction, strides, the single-channel path, every pad_mode at its limit, the
    transposed stores, the plane image of Y, every epilogue subset, the activations and FiLM from LDS and from global memory.
    The two `wrap` cases (Ci 4100: reduction indices past 4096 KW) fail on the 20-bit (channel, tap) split this change replaces."""
    _run(c)


@pytest.mark.parametrize("c", cc.split_cases(), ids=_ids(cc.split_cases()))
def test_split_kernel(c):
    """conv_split.hip: bf16x3 in regimes I, IIw, IIx, IIwx (the three-product sum), bf16x6 in I and one-sided II, fp16 in I"""
    _run(c)


@pytest.mark.parametrize("c", cc.skinny_cases(), ids=_ids(cc.skinny_cases()))
def test_skinny_kernel(c):
    """conv_skinny.hip: fp32 rows and 2 / 3 weight planes in regimes I and one-sided II (the kernel multiplies the SUM of the planes
    with the fp32 x on the f32 MFMA, so with both sides split lo x lo would not be exact)"""
    _run(c)


@pytest.mark.parametrize("pair", cc.seam_cases(), ids=[a.id for a, _ in cc.seam_cases()])
def test_seam_between_96_and_97_columns(pair):
    """the same conv at 96 columns (few-column kernel) and at 97 (a batch kernel): the shared columns carry the same bits"""
    a, b = pair
    assert cc.dispatch(a).startswith("skinny") and not cc.dispatch(b).startswith("skinny")
    print(a.id, "->", cc.dispatch(a), "|", cc.dispatch(b))
    oa = cc.make(a)                                                          # one set of operands for both lengths
    ra, rb = cc.reference(a, oa), cc.reference(b, oa)
    assert torch.equal(ra["y"], rb["y"][:, :, :96])
    Ya, _ = _call(a, oa)
    Yb, _ = _call(b, oa)
    _check(a, ra, Ya, None)
    _check(b, rb, Yb, None)
    assert torch.equal(Ya, Yb[:, :, :96]), _where(a, f"against [{cc.dispatch(b)}]", Ya.cpu().double(), Yb[:, :, :96].cpu().double())


def test_film_frame_range_equals_the_whole_window():
    """a 1x1 conv on samples [t0, t0 + L) of a window with the FiLM rows of frames [f0, f0 + ld) only (film_t0 / film_f0 / film_ld)
    gives the whole-window call's Z bit for bit on every column whose two interpolation frames lie inside the table"""
    from module import ops
    n, ci, co, lfw, tw = 2, 24, 129, 40, 400
    # (ld 15 -> 150 columns: the scalar epilogue, Tout % 4 != 0; the range's ld / L is the window's 40 / 400 in fp32 either way)
    for prec, f0, ld in (("bf16x3", 10, 16), ("fp16", 10, 16), ("bf16x3", 22, 15)):
        t0, L = 10 * f0, 10 * ld
        assert np.float32(ld) / np.float32(L) == np.float32(lfw) / np.float32(tw)
        c = cc.Case(kernel="split", prec=prec, tag="range", n=n, ci=ci, co=co, tin=tw, lf=lfw, wexp=-6, wa=20)
        o = cc.make(c)
        Yw, Zw = _call(c, o)
        _check(c, cc.reference(c, o), Yw, Zw)
        x = o["x"][:, :, t0:t0 + L].contiguous().float().to(DEV)
        film = o["film"][:, :, f0:f0 + ld].contiguous().to(DEV)
        Yr, Zr = ops.conv1d(x, o["w"].float().to(DEV), o["bias"].float().to(DEV), precision=prec, film=film, film_scale_row=o["film_scale_row"],
                            film_shift_row=o["film_shift_row"], film_t0=t0, film_f0=f0, film_ld=ld, film_lf=lfw)
        assert torch.equal(Yr, Yw[:, :, t0:t0 + L])
        i0, i1 = cc.lerp_coord(np.arange(t0, t0 + L), np.float32(lfw) / np.float32(tw), lfw)
        cols = torch.from_numpy((i0 >= f0) & (i1 < f0 + ld))
        assert float(cols.double().mean()) >= 0.8, float(cols.double().mean())
        a, b = Zr.cpu()[:, :, cols], Zw.cpu()[:, :, t0:t0 + L][:, :, cols]
        assert torch.equal(a, b), _where(c, "range Z against window Z (index among the covered columns)", a.double(), b.double())


REFUSED = {
    "stride 2": dict(c=dict(stride=2, tin=260)),
    "pad_mode 2": dict(c=dict(mode=2, pad=2)),
    "act sin": dict(c=dict(act="sin", wexp=-6)),
    "halo 17": dict(c=dict(kw=2, dil=17, tin=160)),
    "Tout > Tin + pad_left": dict(c=dict(out_len=140, pad=3)),
    "film span over 20 frames": dict(c=dict(lf=32, tin=128)),
    "Xp reads past the signal": dict(c=dict(kw=5, ci=32, co=128, tin=128, out_len=128, xp=True)),
    "film_t0 without a range, split": dict(c=dict(lf=13), over=dict(film_t0=5)),
    "film_f0 without a range, exact": dict(c=dict(lf=13, prec="fp32", kernel="exact"), over=dict(film_f0=2)),
    "film_t0 without a range, skinny": dict(c=dict(lf=13, prec="fp32", kernel="skinny", n=1, tin=40), over=dict(film_t0=5)),
}


@pytest.mark.parametrize("name", list(REFUSED))
def test_refusals_leave_the_outputs_untouched(name, monkeypatch):
    """what the split kernel cannot do is refused through nat.check at more than 96 columns (where the few-column kernel would
    not take it), and film_t0 / film_f0 without film_ld by every kernel; nothing is launched: pre-filled outputs keep their bytes"""
    from module import ops
    spec = REFUSED[name]
    c = cc.Case(**{**dict(kernel="split", prec="bf16x3", tag="refuse", n=2, ci=24, co=40, tin=130), **spec["c"]})
    assert cc.dispatch(c).split("/")[0] == c.kernel and (c.cols > 96) == (c.kernel != "skinny")
    o = cc.make(c)
    xp = ops.to_planes(o["x"].float().to(DEV), 2) if c.xp else None
    made, real = [], torch.empty

    def filled(*a, **k):
        t = real(*a, **k)
        t.fill_(0x5A if t.dtype == torch.uint8 else -77.0)
        made.append(t)
        return t

    monkeypatch.setattr(torch, "empty", filled)
    with pytest.raises(ValueError, match="alive_conv1d"):
        _call(c, o, **({"x_planes": xp} if c.xp else {}), **spec.get("over", {}))
    monkeypatch.undo()
    torch.cuda.synchronize()
    assert made and all(bool((t == (0x5A if t.dtype == torch.uint8 else -77.0)).all()) for t in made)


@pytest.mark.parametrize("prec", ["bf16x3", "bf16x6", "fp16"])
def test_split_kernel_per_element_on_gaussian_operands(prec):
    """what cannot be exact -- the third plane of bf16x6, bf16x6 with both operands split, fp16 off its grid -- per element against the
    float64 conv of the operands as the kernel decodes them, within the first-order worst case of an fp32 accumulation
    (K + 4) 2^-24 (sum |w| |x| + |b|) plus the plane products the precision drops"""
    c, o, ref, bound = cc.tolerance_case(prec)
    assert cc.dispatch(c) == f"split/bm128/np{cc.NPLANES[prec]}"
    Y, _ = _call(c, {k: v.double() for k, v in o.items()})
    y = Y.cpu().double()
    err = (y - ref).abs()
    print(c.id, "max err / bound", float((err / bound).max()), "max err", float(err.max()))
    bad = ~(err <= bound)
    assert not bad.any(), _where(c, "Y", y, ref, bad)
