"""alive_dwconv_norm_planes / _f16s at the widths the networks run (C = 64, 128, 256, 512: the kernel that keeps each thread's channel
column in registers) and at widths that take the LDS-resident kernel (C = 288, 1024):
  * against float64 (F.conv1d groups = C, padding 3; unbiased std + eps; affine) with the bounds of
    tests/test_gpu_ops.py::test_dwconv_norm_planes_single_pass (rms relative error 1e-5 on two bf16 planes, 2e-6 on three), 2^-11 on
    one fp16 plane (one fp16 rounding of values in fp16's normal range; the rms of roundings of at most 2^-11 relative each is at most
    2^-11 of the rms), and the fp16 split form as test_dwconv_norm_planes_fp16_split has it: within 2^-21 of the largest element of
    alive_dwconv_norm's fp32 output (dw off: the same kernel with the taps (0, 0, 0, 1, 0, 0, 0) and no bias, whose fma chain returns x);
  * bitwise against alive_dwconv_norm_planes_ref, the LDS-resident kernel, on every column < N T;
  * every byte outside the written plane pieces (the padding columns of each plane, a band on either side of the buffer) keeps its
    sentinel;
  * 20 launches on one input at batch scale give equal buffers.
Needs an MI355X."""
import pytest
import torch
import torch.nn.functional as F

from module import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAND = 4096
SENT = 0x5A
SCALE = 256.0           # the activation scale of the fp16 split form (csrc/networks.hip)

# C = 512: TW = 32 columns per block.  T <= 6 clips every tap set on both sides; 66 is the last T with no interior tile, 67 the first
# with one (t0 >= 3 && t0 + TW + 3 <= T); 101 has two interior tiles and a ragged last one.  C = 256, 64: TW = 64.
SHAPES = [(512, t) for t in (1, 3, 6, 7, 31, 32, 33, 66, 67, 70, 101)] + \
         [(c, t) for c in (256, 64) for t in (5, 63, 64, 65, 130, 131, 200)] + [(288, 70), (1024, 70)]
REGISTER_WIDTHS = (64, 128, 256, 512)


def g(name, shape, scale=1.0):
    return synthetic.gaussian(name, 11, shape, scale)


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)).item()


def guarded(nbytes):
    """a plane buffer of nbytes between two sentinel bands, itself filled with the sentinel"""
    raw = torch.full((nbytes + 2 * BAND,), SENT, dtype=torch.uint8, device=DEV)
    return raw, raw[BAND:BAND + nbytes]


def planes_view(P, n, c, t, planes):
    cols_pad = (n * t + 127) // 128 * 128
    return P.view(torch.int16).view(planes, c // 32, cols_pad, 32)


def decode(P, n, c, t, planes, dtype):
    """sum of the planes as fp32 [N][C][T] (k-blocked layout, csrc/planes_layout.h)"""
    v = planes_view(P, n, c, t, planes).view(dtype).float().sum(0)
    return v.permute(1, 0, 2).reshape(-1, c)[:n * t].view(n, t, c).permute(0, 2, 1)


def check_untouched(raw, n, c, t, planes):
    assert bool((raw[:BAND] == SENT).all() and (raw[-BAND:] == SENT).all()), "wrote outside the plane buffer"
    pad = planes_view(raw[BAND:-BAND], n, c, t, planes)[:, :, n * t:]
    assert bool((pad.contiguous().view(torch.uint8) == SENT).all()), "wrote a padding column"


@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("c,t", SHAPES)
def test_dwconv_norm_planes_all_forms(n, c, t, monkeypatch):
    from module import ops, _native as nat
    L = nat.lib()
    x = g(f"x{c}.{t}", (n, c, t))
    w, b = g(f"w{c}", (c, 1, 7), 0.3), g(f"b{c}", (c,), 0.1)
    gain, off = g(f"g{c}", (c,), 0.5) + 1.0, g(f"o{c}", (c,), 0.2)
    rows = 2 * c + 5
    cond = g(f"c{c}.{t}", (n, rows, t))
    ident = torch.zeros(c, 1, 7)
    ident[:, 0, 3] = 1.0
    xd, wd, bd, gd, od, cd = (v.to(DEV) for v in (x, w, b, gain, off, cond))
    identd, zerod = ident.to(DEV), torch.zeros(c, device=DEV)
    w7, ident7 = wd.reshape(-1).contiguous(), identd.reshape(-1).contiguous()

    real_empty = torch.empty
    made = []

    def guarded_empty(*size, **kw):
        if kw.get("dtype") is torch.uint8 and len(size) == 1:
            raw, P = guarded(int(size[0]))
            made.append(raw)
            return P
        return real_empty(*size, **kw)

    for dw in (True, False):
        y = F.conv1d(x.double(), w.double(), b.double(), padding=3, groups=c) if dw else x.double()
        mu, sd = y.mean(dim=1, keepdim=True), y.std(dim=1, keepdim=True) + 1e-4
        norm = (y - mu) / sd
        for adaptive in (False, True):
            ref = norm * cond[:, 5:5 + c].double() + cond[:, 5 + c:5 + 2 * c].double() if adaptive \
                else norm * gain.double().view(1, -1, 1) + off.double().view(1, -1, 1)
            # the fp32 kernel, the yardstick of the split form (dw off: identity taps)
            y32 = ops.dwconv_norm(xd, wd if dw else identd, bd if dw else zerod, gain=None if adaptive else gd,
                                  offset=None if adaptive else od, cond=cd if adaptive else None, scale_row=5, shift_row=5 + c)
            head = (nat.ptr(xd), n, c, t, nat.ptr(w7) if dw else None, nat.ptr(bd) if dw else None, 1 if adaptive else 0,
                    None if adaptive else nat.ptr(gd), None if adaptive else nat.ptr(od), nat.ptr(cd) if adaptive else None,
                    rows if adaptive else 0, 5, 5 + c, 1e-4)
            for planes, scale in ((1, 0.0), (2, 0.0), (3, 0.0), (2, SCALE)):
                what = f"dw {dw} adaptive {adaptive} planes {planes} scale {scale}"
                if scale:
                    raw, P = guarded(L.alive_planes_bytes(n * t, c, 2))
                    nat.check(L.alive_dwconv_norm_planes_f16s(*head, scale, nat.ptr(P), nat.stream()), "alive_dwconv_norm_planes_f16s")
                else:
                    monkeypatch.setattr(ops.torch, "empty", guarded_empty)
                    P = ops.dwconv_norm_planes(xd, wd if dw else None, bd if dw else None, None if adaptive else gd,
                                               None if adaptive else od, cd if adaptive else None, 5, 5 + c, planes=planes)
                    monkeypatch.undo()
                    raw = made.pop()
                    assert not made
                torch.cuda.synchronize()
                check_untouched(raw, n, c, t, planes)
                if scale:
                    got = decode(P, n, c, t, 2, torch.float16) / scale
                    e, bound = (got - y32).abs().max().item(), 2.0 ** -21 * y32.abs().max().item()
                elif planes == 1:
                    e, bound = relerr(decode(P, n, c, t, 1, torch.float16), ref), 2.0 ** -11
                else:
                    got = ops.planes_to_float(P, n, c, t, planes)
                    e, bound = relerr(got, ref), (1e-5 if planes == 2 else 2e-6)
                    assert torch.equal(got, decode(P, n, c, t, planes, torch.bfloat16))
                print(f"C {c} T {t} N {n} {what}: error {e:.3e} (bound {bound:.3e})")
                assert e <= bound if scale else e < bound, (what, e, bound)
                # bitwise against the LDS-resident kernel
                raw_r, Pr = guarded(P.numel())
                nat.check(L.alive_dwconv_norm_planes_ref(*head, planes, nat.ptr(Pr), nat.stream(), scale), "alive_dwconv_norm_planes_ref")
                torch.cuda.synchronize()
                check_untouched(raw_r, n, c, t, planes)
                if c in REGISTER_WIDTHS:
                    cols = n * t
                    assert torch.equal(planes_view(P, n, c, t, planes)[:, :, :cols], planes_view(Pr, n, c, t, planes)[:, :, :cols]), what


@pytest.mark.parametrize("form", ["decoder", "content_encoder"])
def test_dwconv_norm_planes_is_deterministic_at_batch_scale(form):
    """192 windows x 450 frames, C = 512, 20 launches on one input: the decoder's form (adaptive, one fp16 plane) and the
    ContentEncoder's (plain affine, fp16 split)"""
    from module import _native as nat
    L = nat.lib()
    n, c, t = 192, 512, 450
    gen = torch.Generator(device=DEV).manual_seed(5)
    r = lambda *s: torch.randn(*s, device=DEV, generator=gen)
    x, w, b = r(n, c, t), r(c * 7) * 0.3, r(c) * 0.1
    adaptive = form == "decoder"
    rows = 2 * c + 5
    cond = r(n, rows, t) if adaptive else None
    gain, off = r(c) * 0.5 + 1.0, r(c) * 0.2
    planes = 1 if adaptive else 2
    head = (nat.ptr(x), n, c, t, nat.ptr(w), nat.ptr(b), 1 if adaptive else 0, None if adaptive else nat.ptr(gain),
            None if adaptive else nat.ptr(off), nat.ptr(cond) if adaptive else None, rows if adaptive else 0, 5, 5 + c, 1e-4)
    first = None
    for i in range(20):
        P = torch.zeros(L.alive_planes_bytes(n * t, c, planes), dtype=torch.uint8, device=DEV)
        if adaptive:
            nat.check(L.alive_dwconv_norm_planes(*head, planes, nat.ptr(P), nat.stream()), "alive_dwconv_norm_planes")
        else:
            nat.check(L.alive_dwconv_norm_planes_f16s(*head, SCALE, nat.ptr(P), nat.stream()), "alive_dwconv_norm_planes_f16s")
        if first is None:
            first = P
        else:
            assert torch.equal(P, first), f"launch {i} differs from the first"
