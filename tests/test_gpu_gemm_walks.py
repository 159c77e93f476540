"""alive_gemm_planes (csrc/gemm_planes.hip) in the forms its standard tests do not reach: the custom row walks (overlapping
k-contiguous rows: the STFT; strided rows inside a k-blocked plane image: the decoder's down convs as GEMMs), the split output
(y_split), the magnitude epilogue (act 4) and the plane-packed output of the persistent kernel.  Needs an MI355X.

Every custom walk is compared twice.  (A) BITWISE with the standard walk: the operand is unfolded on the host into an ordinary
[N][K][T] tensor, packed by alive_to_planes and multiplied with b_row = 0 -- every element goes through the same round-to-nearest
split, the K order, tile shape and kernel instance are the same, so a single differing bit is a wrong address, tap order or clamp.
(B) Against the float64 product of the un-rounded operands, with the bars of test_gpu_ops.py::test_gemm_planes_vs_float64 (K here
never exceeds the K those bars were set for), which guards (A) against both sides being wrong together.

In the custom forms the kernel clamps only the column, so before every launch the buffer is checked against the addresses the walk
forms (tools/gemm_walks_ref.py::operand_extent; tests/test_host_gemm_walks.py proves the same on the CPU, together with the K order
of the unfold).  Which kernel a case reaches (one-tile, KB2, persistent) is asserted from the dispatch conditions there too.
"""
import os
import sys

import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gemm_walks_ref as GW                                          # noqa: E402
from module import _native as nat                                    # noqa: E402
from module import ops                                               # noqa: E402
from module._pack import pack_conv_split, pack_conv_split_h          # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
TOL = {2: 2e-5, 3: 4e-7}                       # relerr bars of test_gemm_planes_vs_float64


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)).item()


def packed(w, planes):
    """the weight operand: `planes` bf16 planes, or the ONE fp16 plane (slab 2 of pack_conv_split_h)"""
    w = w.to(DEV)
    return pack_conv_split_h(w)[2].contiguous() if planes == 1 else pack_conv_split(w, planes)


def run(P, g, W, bias=None, custom=True, **kw):
    """one launch on geometry g (custom = False: the same GEMM on the standard walk); the operand buffer is checked first"""
    if custom:
        assert GW.operand_extent(g) * 2 <= P.numel() * P.element_size(), "the walk leaves its buffer"
    place = g.placement() if custom else {}
    Y = kw.pop("Y", None)
    if Y is None and kw.get("act") != 4:
        Y = torch.empty(g.N, g.Co, g.T, device=DEV)
    ops.gemm_planes_raw(P, g.N, g.T, g.Ci, g.Co, W, bias, planes=g.planes, Y=Y, **place, **kw)
    return Y


def plane_bits(P, planes, c, cols):
    """a plane-packed buffer as int16 [planes][c_pad / 32][real columns][32]"""
    return P.view(torch.int16).view(planes, GW.pad32(c) // 32, GW.pad_cols(cols), 32)[:, :, :cols].contiguous()


def check_against_float64(y, g, ref64):
    if g.planes == 1:
        # one fp16 plane: the float64 product of the fp16 operands, bar of test_gemm_planes_one_plane_is_the_float64_product_...
        assert (y.cpu().double() - ref64).abs().max().item() <= 3e-5 * max(1.0, ref64.abs().max().item())
    else:
        e = relerr(y, ref64)
        print(f"relerr {e:.3e} (bar {TOL[g.planes]:.0e})")
        assert e < TOL[g.planes], e


# ---- form 1: overlapping k-contiguous rows (b_row = hop, b_cblk = 0) -----------------------------------------------------------
@pytest.mark.parametrize("cid,planes", [(cid, pl) for cid, c in GW.FRAMES.items() for pl in c[5]])
def test_overlapping_rows_equal_the_unfolded_frames(cid, planes):
    """Check B is test_gemm_planes_vs_float64's, term for term: bias, a layer scale and a residual around the product, so its bars
    are met on the quantity they were set for (the residual's unit variance and the 0.5 scale make relerr 0.45 x that of the bare
    product).  On the bare product, case 1c at three planes (K = 1280) measured 5.5e-07 on an MI355X while bit-identical to the
    standard walk: the fp32 accumulation of 480 MFMAs per output, about 2.4e-07 in that test's terms."""
    c = GW.frames_case(cid, planes)
    g, W, b = c["geo"], packed(c["w"], planes), c["b"].to(DEV)
    res, sc = GW.gauss(f"gw.r.{cid}", (g.N, g.Co, g.T)), GW.gauss(f"gw.s.{cid}", (g.Co,), 0.5)
    kw = dict(ch_scale=sc.to(DEV), residual=res.to(DEV))
    y = run(c["buf"].to(DEV), g, W, b, **kw)
    y_std = run(ops.to_planes(c["x_unf"].to(DEV), planes), g, W, b, custom=False, **kw)
    assert torch.equal(y, y_std), f"{(y != y_std).sum().item()} of {y.numel()} values differ from the standard walk"
    ref = F.conv1d(c["x_unf"].double(), c["w"].double(), c["b"].double()) * sc.double().view(1, -1, 1) + res.double()
    check_against_float64(y, g, ref)


# ---- form 2: strided conv as a GEMM over the k-blocked plane image (b_cblk = c_pad / 32) --------------------------------------
def _conv_outputs(cid, want_planes=False):
    c = GW.conv_case(cid)
    g = c["geo"]
    W, b = packed(c["w"], g.planes), c["b"].to(DEV)
    P = ops.to_planes(c["x"].to(DEV), g.planes)
    # the image the host twin proved the walk on is the image the device wrote
    assert torch.equal(P.view(torch.int16).cpu(), GW.planes_image(c["x"], g.planes).reshape(-1))
    kw = {}
    if want_planes:
        kw["Pout"] = torch.full((nat.lib().alive_planes_bytes(g.cols, g.Co, g.planes),), 0xFF, dtype=torch.uint8, device=DEV)
    y = run(P, g, W, b, **kw)
    y_std = run(ops.to_planes(c["x_unf"].to(DEV), g.planes), g, W, b, custom=False)
    return c, g, y, y_std, kw.get("Pout")


@pytest.mark.parametrize("cid", list(GW.CONVS))
def test_strided_rows_equal_the_unfolded_patches_and_the_strided_conv(cid):
    c, g, y, y_std, _ = _conv_outputs(cid)
    assert torch.equal(y, y_std), f"{(y != y_std).sum().item()} of {y.numel()} values differ from the standard walk"
    x, w = (c["x"].half(), c["w"].half()) if g.planes == 1 else (c["x"], c["w"])
    check_against_float64(y, g, F.conv1d(x.double(), w.double(), c["b"].double(), stride=c["r"]))


def test_strided_rows_with_both_outputs_like_the_decoder():
    """downs[2]: Y feeds a skip, Pout is the operand of downs[3] -- on real columns the planes are alive_to_planes(Y, 2), bit for bit"""
    c, g, y, y_std, Po = _conv_outputs("down2", want_planes=True)
    assert torch.equal(y, y_std)
    assert torch.equal(plane_bits(Po, 2, g.Co, g.cols), plane_bits(ops.to_planes(y, 2), 2, g.Co, g.cols))


# ---- y_split: one GEMM, two tensors ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["bias", "gelu", "scale"])
@pytest.mark.parametrize("co,ys,ci,n,t,planes", [c[:5] + (pl,) for c in GW.SPLITS for pl in c[5]])
def test_split_output_is_the_single_output_cut_in_two(co, ys, ci, n, t, planes, variant):
    tag = f"gw.ys.{co}.{ci}"
    x, w, b = GW.gauss(tag + ".x", (n, ci, t)), GW.gauss(tag + ".w", (co, ci, 1), ci ** -0.5), GW.gauss(tag + ".b", (co,), 0.1)
    kw = {"gelu": dict(act="gelu"),
          "scale": dict(ch_scale=GW.gauss(tag + ".s", (co,), 0.5).to(DEV), post_add=GW.gauss(tag + ".p", (co,), 0.3).to(DEV))}.get(variant, {})
    g = GW.Geo(n, t, ci, co, planes)
    P, W, b = ops.to_planes(x.to(DEV), planes), packed(w, planes), b.to(DEV)
    whole = run(P, g, W, b, custom=False, **kw)
    n1, n2, G = n * ys * t, n * (co - ys) * t, 4096
    o1 = torch.full((G + n1 + G,), 7.0, device=DEV)
    o2 = torch.full((G + n2 + G,), 7.0, device=DEV)
    run(P, g, W, b, custom=False, Y=o1[G:], Y2=o2[G:], y_split=ys, **kw)
    assert torch.equal(o1[G:G + n1].view(n, ys, t), whole[:, :ys])
    assert torch.equal(o2[G:G + n2].view(n, co - ys, t), whole[:, ys:])
    for o, m in ((o1, n1), (o2, n2)):
        assert bool((o[:G] == 7.0).all() and (o[G + m:] == 7.0).all()), "a split output was written outside its tensor"


# ---- act 4: magnitudes of (re, im) row pairs as three k-blocked planes ---------------------------------------------------------
def _check_magnitudes(P, g, W, custom):
    """act 4 against float64 hypot of the row pairs of the act-0 output of the same GEMM.
    Bar per element: 2^-21 |ref| -- 2^-22 for the three-plane split (test_to_planes_roundtrip) + 2^-22 (2 fp32 ulp) for hypotf --
    plus the smallest normal fp32 where ref is an exact zero.  The faults this is for (row pair, bin, swizzle chunk) are of order 1."""
    bins, cols = g.Co // 2, g.cols
    cp, cols_pad = GW.pad32(bins), GW.pad_cols(cols)
    y = run(P, g, W, custom=custom)
    Po = torch.full((nat.lib().alive_planes_bytes(cols, bins, 3),), 0xFF, dtype=torch.uint8, device=DEV)
    assert Po.numel() == 3 * cp * cols_pad * 2
    run(P, g, W, custom=custom, act=4, Pout=Po)
    ref = torch.hypot(y[:, 0::2].double(), y[:, 1::2].double())
    got = ops.planes_to_float(Po, g.N, bins, g.T, 3).double()
    excess = ((got - ref).abs() - (2.0 ** -21 * ref.abs() + torch.finfo(torch.float32).tiny)).max().item()
    print(f"act 4: largest relative error {((got - ref).abs() / ref.abs().clamp_min(1e-30)).max().item():.3e} (bar 2^-21 = {2.0 ** -21:.3e})")
    assert excess <= 0.0, excess
    # the padding the next GEMM multiplies by zero weights: channels bins .. c_pad of every column, columns cols .. cols_pad of every block
    raw = Po.view(torch.int16).view(3, cp // 32, cols_pad, 32)
    chan = raw.permute(0, 2, 1, 3).reshape(3, cols_pad, cp)
    assert not bool(chan[:, :, bins:].any()), "channel padding of the magnitude planes is not zero"
    assert not bool(raw[:, :, cols:].any()), "column padding of the magnitude planes is not zero"
    assert bool(ref.abs().max() > 0.1)


@pytest.mark.parametrize("co,ci,n,t", GW.MAGS)
def test_magnitude_epilogue_is_hypot_of_the_row_pairs(co, ci, n, t):
    x, w = GW.gauss(f"gw.mg.x{co}", (n, ci, t)), GW.gauss(f"gw.mg.w{co}", (co, ci, 1), ci ** -0.5)
    _check_magnitudes(ops.to_planes(x.to(DEV), 3), GW.Geo(n, t, ci, co, 3), packed(w, 3), custom=False)


def test_magnitude_epilogue_on_overlapping_rows():
    """the production pairing of walk and epilogue (alive_front_end): operand and shape of form-1 case 1c"""
    c = GW.frames_case("1c", 3)
    _check_magnitudes(c["buf"].to(DEV), c["geo"], packed(c["w"], 3), custom=True)


# ---- Pout of the persistent kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("co,ci,n,t", GW.POUTS)
def test_persistent_kernel_plane_output_is_to_planes_of_its_fp32_output(co, ci, n, t):
    """the stage_small path: on real columns the planes are alive_to_planes(Y, 3) bit for bit, zero channel padding included
    (columns past the end are deliberately not written by this path: nothing is asserted about them)"""
    x, w, b = GW.gauss(f"gw.po.x{co}{t}", (n, ci, t)), GW.gauss(f"gw.po.w{co}", (co, ci, 1), ci ** -0.5), GW.gauss(f"gw.po.b{co}", (co,), 0.1)
    g = GW.Geo(n, t, ci, co, 3)
    Po = torch.full((nat.lib().alive_planes_bytes(g.cols, co, 3),), 0xFF, dtype=torch.uint8, device=DEV)
    y = run(ops.to_planes(x.to(DEV), 3), g, packed(w, 3), b.to(DEV), custom=False, act="gelu", Pout=Po)
    assert torch.equal(plane_bits(Po, 3, co, g.cols), plane_bits(ops.to_planes(y, 3), 3, co, g.cols))
    assert bool(torch.isfinite(y).all())


# ---- refusals: no kernel is launched ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", GW.REFUSALS, ids=lambda c: c.name)
def test_gemm_planes_placement_and_epilogue_argument_errors(case):
    import ctypes
    room = torch.zeros(64, device=DEV)
    d = GW.refusal_descriptor(nat.AliveGemm, case, lambda name: room.data_ptr())
    with pytest.raises(ValueError) as e:
        nat.check(nat.lib().alive_gemm_planes(ctypes.byref(d), nat.stream()), "alive_gemm_planes")
    assert case.message in str(e.value), str(e.value)
