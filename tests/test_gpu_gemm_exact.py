"""alive_gemm_planes (csrc/gemm_planes.hip) bit for bit on operands whose right answer has no rounding (tests/gemm_cases.py: the regimes,
the references, the derived bounds of the activations), in every form its dispatch reaches: the 32-deep and the 64-deep one-plane
kernel, two bf16 planes, the fp16 split pair, three planes one tile per block and persistent.  Every case names the form it must reach;
the thresholds are read from the source by tests/test_host_gemm_operands.py, which also proves on the CPU that a missing or an extra
plane product would change the expected bits in every tile.

Every output lies between two sentinel bands and is pre-filled with the sentinel: every element of the problem must be written and
nothing outside it.  Of a plane-packed output the kernel writes the columns below N T in all pad32(Co) rows (rows from Co on as zeros:
the next GEMM reads them as K padding) and does NOT write the padding columns from N T up to the next multiple of 128: they keep the
caller's bytes, which is asserted here; a consumer computes columns from them that it never stores."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAND = 4096                       # elements (bytes of a plane buffer) of sentinel on either side of an output
SENT_F, SENT_I, SENT_B = -1.2345e30, -123456789, 0x5A
_ids = lambda cs: [c.id for c in cs]


def _banded(numel, dtype, fill):
    buf = torch.full((numel + 2 * BAND,), fill, dtype=dtype, device=DEV)
    return buf, buf[BAND:BAND + numel]


def _bands_intact(buf, fill):
    return bool((buf[:BAND] == fill).all()) and bool((buf[-BAND:] == fill).all())


def _where(c, what, a, b, bad=None):
    idx, va, vb = gc.first_diff(a, b, bad)
    return f"{c.id} [{gc.dispatch_case(c)}] {what}: first mismatch at {idx}: kernel {va!r}, reference {vb!r}"


def _device_operands(c, o):
    """(P, W, wscale) on the device: the activation image through alive_to_planes (checked bit for bit against the host codec, padding
    included) or, for the fp16 split pair, from the host codec; the weight through the packers"""
    from module import ops, _pack
    w3 = o["w"].float().unsqueeze(2)
    ws = None
    if c.f16s:
        W5, ws = _pack.pack_conv_split_f16s(w3)
        W, ws = W5[3:].contiguous().to(DEV), ws.to(DEV)
        P = gc.host_planes(o["x"], "f16s", gc.F16S_ACT_SCALE).to(DEV)
    else:
        W = (_pack.pack_conv_split_h(w3)[2].contiguous() if c.planes == 1 else _pack.pack_conv_split(w3, c.planes)).to(DEV)
        P = ops.to_planes(o["x"].float().to(DEV), c.planes)
        got, want = P.cpu().view(torch.int16), gc.host_planes(o["x"], c.planes).reshape(-1)
        assert got.numel() == want.numel() and torch.equal(got, want), \
            f"{c.id}: alive_to_planes differs from the host codec at 16-bit element {int((got != want).nonzero()[0])}"
    return P, W, ws


def _launch(c, o, dev, out):
    """one launch with the outputs `out` in sentinel-banded buffers -> (Y on the CPU or None, plane image int16 [planes][pad32(Co) / 32]
    [cols_pad][32] on the CPU or None); the bands and the padding columns are checked here"""
    from module import ops, _native as nat
    P, W, ws = dev
    d = lambda k: o[k].float().to(DEV) if o.get(k) is not None else None
    ybuf = yv = pbuf = pv = None
    res = d("residual")
    if "y" in out:
        ybuf, yv = _banded(c.n * c.co * c.t, torch.float32, SENT_F)
        yv = yv.view(c.n, c.co, c.t)
        if c.alias:
            yv.copy_(res)
            res = yv
    if "p" in out:
        nbytes = c.planes * c.cols_pad * gc.pad32(c.co) * 2
        assert nbytes == nat.lib().alive_planes_bytes(c.cols, c.co, c.planes)
        pbuf, pv = _banded(nbytes, torch.uint8, SENT_B)
    ops.gemm_planes_raw(P, c.n, c.t, c.ci, c.co, W, bias=d("bias"), planes=c.planes, act=gc.ACTS[c.act], post_add=d("post_add"),
                        ch_scale=d("ch_scale"), residual=res, Y=yv, Pout=pv, f16s=c.f16s, wscale=ws,
                        in_unscale=1.0 / gc.F16S_ACT_SCALE if c.f16s else 0.0,
                        pout_scale=gc.F16S_ACT_SCALE if c.f16s and pv is not None else 0.0)
    torch.cuda.synchronize()
    Y = img = None
    if yv is not None:
        assert _bands_intact(ybuf, SENT_F), f"{c.id}: Y written outside [n][co][t]"
        Y = yv.cpu()
        assert not bool((Y == SENT_F).any()), _where(c, "Y element never written", Y.double(), torch.zeros_like(Y).double(), Y == SENT_F)
    if pv is not None:
        assert _bands_intact(pbuf, SENT_B), f"{c.id}: Pout written outside its buffer"
        img = pv.cpu().view(torch.int16).view(c.planes, gc.pad32(c.co) // 32, c.cols_pad, 32)
        assert bool((img[:, :, c.cols:] == SENT_B * 0x0101).all()), f"{c.id}: Pout written in the padding columns >= N T"
    return Y, img


def _check_y(c, ref, Y):
    y, want = Y.double(), ref["y"]
    assert y.shape == want.shape
    if not ref["yerr"].any():
        assert torch.equal(Y, want.float()), _where(c, "Y (n, row, t)", y, want)
    else:
        bad = ~((y - want).abs() <= ref["yerr"])
        assert not bad.any(), _where(c, f"Y (n, row, t) beyond the bound of {c.act}", y, want, bad)


def _check_planes(c, ref, Y, img):
    """the plane image against the host split of the fp32 Y of the same launch, bit for bit; rows [Co, pad32(Co)) zero; where Y is
    exact, the values against the split of the reference too"""
    real = img[:, :, :c.cols]
    own = gc.host_planes(Y, gc.plane_kind(c), gc.F16S_ACT_SCALE)[:, :, :c.cols]
    at = lambda bad: tuple(int(i) for i in bad.nonzero()[0])
    assert torch.equal(real, own), (f"{c.id} [{gc.dispatch_case(c)}]: Pout differs from the split of its own Y at (plane, channel block, column, "
                                    f"channel) {at(real != own)}")
    rows = real.permute(0, 2, 1, 3).reshape(c.planes, c.cols, gc.pad32(c.co))
    assert not rows[:, :, c.co:].any(), f"{c.id}: rows [Co, pad32(Co)) of Pout are not zero at {at(rows[:, :, c.co:] != 0)}"
    if not ref["yerr"].any():
        want = gc.host_planes(ref["y"].float(), gc.plane_kind(c), gc.F16S_ACT_SCALE)[:, :, :c.cols]
        a, b = gc.planes_as_float(real.contiguous(), c), gc.planes_as_float(want.contiguous(), c)
        assert torch.equal(a, b), f"{c.id}: Pout differs from the split of the reference at (plane, channel block, column, channel) {at(a != b)}"


def _run(c):
    from module import ops
    assert os.environ.get("ALIVE_GEMM_VARIANT") is None, "the dispatch under test is the default one"
    assert gc.dispatch_case(c) == c.form, (c.id, gc.dispatch_case(c))
    print(c.id, "->", c.form, f"{c.nsteps} steps, {c.ntiles} tiles")
    fp16 = c.f16s or c.planes == 1
    if fp16:
        ops.f16_saturations(reset=True)
    o = gc.make(c)
    ref = gc.reference(c, o)
    dev = _device_operands(c, o)
    if c.act == "argmax":
        # act = 3: the candidates of every 64-row block bit for bit (value, and on ties the first row), then alive_argmax_merge =
        # the first index of the maximum of the exact values in every column
        P, W, ws = dev
        val, idx, first, ties = gc.argmax_reference(c, ref["v"])
        assert ties >= 0.1, (c.id, ties)
        nblk = gc.cdiv(c.co, 64)
        vbuf, vv = _banded(nblk * c.cols, torch.float32, SENT_F)
        ibuf, iv = _banded(nblk * c.cols, torch.int32, SENT_I)
        vv, iv = vv.view(nblk, c.cols), iv.view(nblk, c.cols)
        ops.gemm_planes_raw(P, c.n, c.t, c.ci, c.co, W, bias=None if o["bias"] is None else o["bias"].float().to(DEV), planes=c.planes,
                            act=3, f16s=c.f16s, wscale=ws, in_unscale=1.0 / gc.F16S_ACT_SCALE if c.f16s else 0.0, arg_val=vv, arg_idx=iv)
        merged = ops.argmax_merge(vv, iv, c.n, c.t)
        torch.cuda.synchronize()
        assert _bands_intact(vbuf, SENT_F) and _bands_intact(ibuf, SENT_I), f"{c.id}: candidates written outside [blocks][n t]"
        gv, gi = vv.cpu(), iv.cpu().long()
        assert not bool((gv == SENT_F).any()) and not bool((gi == SENT_I).any()), f"{c.id}: a candidate was never written"
        wv, wi = torch.from_numpy(val).float(), torch.from_numpy(idx)
        assert torch.equal(gv, wv), f"{c.id}: candidate value (block, column) " + str(gc.first_diff(gv.double(), wv.double()))
        assert torch.equal(gi, wi), f"{c.id}: candidate row (block, column) " + str(gc.first_diff(gi.double(), wi.double()))
        got = merged.cpu().view(-1).double()
        want = torch.from_numpy(first).double()
        assert torch.equal(got, want), f"{c.id}: argmax (column) " + str(gc.first_diff(got, want))
    else:
        Y, img = _launch(c, o, dev, "yp" if c.out == "p" else c.out)
        _check_y(c, ref, Y)
        if img is not None:
            _check_planes(c, ref, Y, img)
        if c.out == "p":
            # planes only: the same bits as with Y beside them (checked above against that Y and the reference)
            Y2, img2 = _launch(c, o, dev, "p")
            assert Y2 is None and torch.equal(img2, img), (f"{c.id}: Pout without Y differs from Pout with Y at (plane, channel block, column, channel) "
                                                           f"{tuple(int(i) for i in (img2 != img).nonzero()[0])}")
    if fp16:
        assert ops.f16_saturations(reset=True) == 0, c.id


@pytest.mark.parametrize("c", gc.step_cases(), ids=_ids(gc.step_cases()))
def test_every_form_at_each_depth_of_its_ring(c):
    """fewer k-steps than the DMA ring holds, as many, more; regimes I, H, II, III and F by form"""
    _run(c)


@pytest.mark.parametrize("c", gc.act_cases(), ids=_ids(gc.act_cases()))
def test_activations_within_their_derived_bounds(c):
    """gelu_fast and expf on an exact v, with and without the whole linear tail behind them"""
    _run(c)


@pytest.mark.parametrize("c", gc.network_cases(), ids=_ids(gc.network_cases()))
def test_the_fp16_split_form_as_the_networks_use_it_and_the_argmax(c):
    """pw1 (GELU, planes times pout_scale), pw2 (ch_scale, Y is the residual), the classifier's argmax with ties across 64-row blocks"""
    _run(c)


@pytest.mark.parametrize("c", gc.edge_cases(), ids=_ids(gc.edge_cases()))
def test_edges_of_rows_reduction_columns_and_epilogue(c):
    """Co and Ci around the tile, pad16 and pad32 edges, columns around one tile and across batch items, every epilogue subset"""
    _run(c)


@pytest.mark.parametrize("c", gc.persistent_cases(), ids=_ids(gc.persistent_cases()))
def test_persistent_kernel_across_its_tile_seams(c):
    """gemm_planes_lw_kernel with 3, 4 and 5 k-steps (every ring position at a seam), uneven XCD chunks, a partial last row tile,
    ragged columns, planes through the 2-KB stage, argmax, and a real third plane on either operand"""
    _run(c)
