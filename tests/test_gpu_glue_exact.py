"""The fp32 glue kernels bit for bit on the exact cases of tests/glue_cases.py (proved on the CPU by tests/test_host_glue_cases.py):
  A. alive_dwconv_norm and alive_channel_norm, both kernels each (T <= 32: one block per frame; T > 32: 64 columns per block), static
     and adaptive affine, two eps; the same cases through alive_dwconv_norm_planes / _ref with three planes;
  B. alive_argmax_channels, both kernels, and the act = 3 GEMM + alive_argmax_merge on ties, NaNs and -inf: torch.argmax's answer;
  C. alive_filter_source_in / _out against the float64 F.conv1d chain;
  D. alive_resample on impulses (the device's own bank) and on a synthetic integer bank, alive_resample_rows row by row,
     alive_resample_filter against the float64 formula;
  E. alive_pitch_transform / _rows on rows whose log2 / exp2 arguments are integer powers;
  F. alive_gelu_film on a frame range against the whole window's slice.
Every output is filled with NaN (or a sentinel) before the call; bit equality with a finite expectation then says that every element was
written.  Needs an MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import glue_cases as G  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
NAN = float("nan")


def dev(a):
    return torch.as_tensor(a).to(torch.float32).to(DEV).contiguous()


def filled(*shape, value=NAN, dtype=torch.float32):
    return torch.full(shape, value, dtype=dtype, device=DEV)


def same(got, want, what):
    """bit equality (NaN nowhere, +0 == -0 aside), naming the first element that differs"""
    got = got.detach().cpu()
    want = torch.as_tensor(want).to(got.dtype)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    assert not torch.isnan(got).any(), f"{what}: {int(torch.isnan(got).sum())} elements not written (or NaN)"
    if not torch.equal(got, want):
        bad = (got != want).nonzero()
        i = tuple(bad[0].tolist())
        raise AssertionError(f"{what}: {len(bad)} of {got.numel()} elements differ; first at {i}: got {got[i].item()!r}, want {want[i].item()!r}")


# ---- A. dw conv + norm, channel norm ------------------------------------------------------------------------------------------------
def _norm_operands(case):
    c = case["c"]
    return dict(x=dev(case["x"]), y=dev(case["y"]), w=dev(case["w"]).reshape(-1), b=dev(case["b"]), gain=dev(case["gain"]),
                offset=dev(case["offset"]), cond=dev(case["cond"]), ident=dev(np.tile(np.array([0, 0, 0, 1, 0, 0, 0.0]), c)),
                zero=torch.zeros(c, device=DEV))


def _affine_args(nat, case, d, adaptive):
    return (1 if adaptive else 0, None if adaptive else nat.ptr(d["gain"]), None if adaptive else nat.ptr(d["offset"]),
            nat.ptr(d["cond"]) if adaptive else None, case["rows"] if adaptive else 0, case["scale_row"], case["shift_row"])


@pytest.mark.parametrize("c,t", G.NORM_SHAPES)
def test_dwconv_norm_and_channel_norm_exact_columns(c, t):
    from module import _native as nat
    L = nat.lib()
    case = G.norm_case(c, t)
    n, d = case["n"], _norm_operands(case)
    for eps in G.NORM_EPS:
        for adaptive in (False, True):
            want = G.norm_expected(case, eps, adaptive)
            out = filled(n, c, t)
            nat.check(L.alive_dwconv_norm(nat.ptr(d["x"]), n, c, t, nat.ptr(d["w"]), nat.ptr(d["b"]), *_affine_args(nat, case, d, adaptive),
                                          eps, nat.ptr(out), nat.stream()), "alive_dwconv_norm")
            same(out, want, f"alive_dwconv_norm C {c} T {t} eps {eps} adaptive {adaptive}")
            # the conv switched off by identity taps: y itself as the input
            out = filled(n, c, t)
            nat.check(L.alive_dwconv_norm(nat.ptr(d["y"]), n, c, t, nat.ptr(d["ident"]), nat.ptr(d["zero"]),
                                          *_affine_args(nat, case, d, adaptive), eps, nat.ptr(out), nat.stream()), "alive_dwconv_norm")
            same(out, want, f"alive_dwconv_norm (identity taps) C {c} T {t} eps {eps} adaptive {adaptive}")
        out = filled(n, c, t)
        nat.check(L.alive_channel_norm(nat.ptr(d["y"]), n, c, t, nat.ptr(d["gain"]), nat.ptr(d["offset"]), eps, nat.ptr(out), nat.stream()),
                  "alive_channel_norm")
        same(out, G.norm_expected(case, eps, False), f"alive_channel_norm C {c} T {t} eps {eps}")


@pytest.mark.parametrize("c,t", G.PLANE_SHAPES)
def test_dwconv_norm_planes_three_planes_decode_to_the_exact_columns(c, t):
    """a three-way bf16 split of these expected values is lossless (host twin), so the decoded planes are the same bits: the absolute
    anchor of the register-resident and of the LDS-resident plane kernel"""
    from module import ops, _native as nat
    L = nat.lib()
    case = G.norm_case(c, t)
    n, d = case["n"], _norm_operands(case)
    nbytes = L.alive_planes_bytes(n * t, c, 3)
    for eps in G.NORM_EPS:
        for adaptive in (False, True):
            want = G.norm_expected(case, eps, adaptive)
            for dw in (True, False):
                head = (nat.ptr(d["x"] if dw else d["y"]), n, c, t, nat.ptr(d["w"]) if dw else None, nat.ptr(d["b"]) if dw else None,
                        *_affine_args(nat, case, d, adaptive), eps, 3)
                for entry, tail in (("alive_dwconv_norm_planes", ()), ("alive_dwconv_norm_planes_ref", (0.0,))):
                    P = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)          # 0xFFFF is a bf16 NaN
                    nat.check(getattr(L, entry)(*head, nat.ptr(P), nat.stream(), *tail), entry)
                    same(ops.planes_to_float(P, n, c, t, 3), want, f"{entry} C {c} T {t} eps {eps} adaptive {adaptive} dw {dw}")


# ---- B. argmax ----------------------------------------------------------------------------------------------------------------------
def _columns_differ(got, want, names):
    got, want = got.cpu().reshape(-1), want.reshape(-1)
    return [(names[q % len(names)], got[q].item(), want[q].item()) for q in (got != want).nonzero().reshape(-1).tolist()]


@pytest.mark.parametrize("t", G.ARGMAX_T)
@pytest.mark.parametrize("c", G.ARGMAX_C)
def test_argmax_channels_is_torch_argmax_on_ties_nans_and_infs(c, t):
    from module import _native as nat
    x, want, pats = G.argmax_case(c, t)
    n = x.shape[0]
    xd, out = x.to(DEV), filled(n, 1, t, value=-1.0)
    nat.check(nat.lib().alive_argmax_channels(nat.ptr(xd), n, c, t, nat.ptr(out), nat.stream()), "alive_argmax_channels")
    bad = _columns_differ(out, want, [p[0] for p in pats])
    assert not bad, f"C {c} T {t}: (pattern, got, torch.argmax) {bad[:8]}"


@pytest.mark.parametrize("co", G.GEMM_ARGMAX_CO)
def test_gemm_planes_argmax_is_torch_argmax_on_ties_nans_and_infs(co):
    """the same patterns through the act = 3 epilogue and alive_argmax_merge, planted through the bias over a zero weight row"""
    from module import ops, _native as nat
    from module._pack import pack_conv_split
    L = nat.lib()
    bad = []
    for name, w, x, b, want, _ in G.gemm_argmax_cases(co):
        ci, cols = x.shape[1], x.shape[2]
        P = ops.to_planes(x.to(DEV), 3)
        nblk = (co + 63) // 64
        val, idx = filled(nblk, cols), filled(nblk, cols, value=-7, dtype=torch.int32)
        ops.gemm_planes_raw(P, 1, cols, ci, co, pack_conv_split(w.to(DEV), 3), bias=b.to(DEV), planes=3, act=3, arg_val=val, arg_idx=idx)
        out = filled(1, 1, cols, value=-1.0)
        nat.check(L.alive_argmax_merge(nat.ptr(val), nat.ptr(idx), nblk, cols, nat.ptr(out), nat.stream()), "alive_argmax_merge")
        assert bool((idx.cpu() != -7).all()), f"{name}: a candidate was not written"
        bad += _columns_differ(out, want, [name])
    assert not bad, f"Co {co}: (pattern, got, torch.argmax) {bad[:8]}"


# ---- C. filter edges ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lw", G.SOURCE_IN_LW)
def test_filter_source_in_exact(lw):
    from module import _native as nat
    c = G.source_in_case(lw)
    n = c["src"].shape[0]
    src, w_in, b_in, w_d, b_d = (dev(c[k]).reshape(-1) for k in ("src", "w_in", "b_in", "w_d", "b_d"))
    out = filled(n, 16, lw // 2)
    nat.check(nat.lib().alive_filter_source_in(nat.ptr(src), n, lw, nat.ptr(w_in), nat.ptr(b_in), nat.ptr(w_d), nat.ptr(b_d), nat.ptr(out),
                                               nat.stream()), "alive_filter_source_in")
    same(out, c["ref"].float(), f"alive_filter_source_in Lw {lw}")


@pytest.mark.parametrize("lw", G.SOURCE_OUT_LW)
def test_filter_source_out_exact(lw):
    from module import _native as nat
    c = G.source_out_case(lw)
    n = c["h"].shape[0]
    h, w, b = dev(c["h"]), dev(c["w"]).reshape(-1), dev(c["b"])
    out = filled(n, 1, lw)
    nat.check(nat.lib().alive_filter_source_out(nat.ptr(h), n, lw, nat.ptr(w), nat.ptr(b), nat.ptr(out), nat.stream()), "alive_filter_source_out")
    same(out, c["ref"].float(), f"alive_filter_source_out Lw {lw}")


@pytest.mark.parametrize("lw", [0, 1, 7, 511])
def test_filter_source_in_refuses_odd_and_empty_windows(lw):
    from module import _native as nat
    c = G.source_in_case(8)
    w_in, b_in, w_d, b_d = (dev(c[k]).reshape(-1) for k in ("w_in", "b_in", "w_d", "b_d"))
    src = torch.ones(3 * max(lw, 1), device=DEV)
    out = filled(3, 16, max(lw // 2, 1), value=-5.0)
    with pytest.raises(ValueError, match="alive_filter_source_in"):
        nat.check(nat.lib().alive_filter_source_in(nat.ptr(src), 3, lw, nat.ptr(w_in), nat.ptr(b_in), nat.ptr(w_d), nat.ptr(b_d), nat.ptr(out),
                                                   nat.stream()), "")
    torch.cuda.synchronize()
    assert bool((out == -5.0).all()), "the output keeps its fill"


# ---- D. resampler -------------------------------------------------------------------------------------------------------------------
def _device_bank(nat, orig, new):
    taps = G.resample_taps(orig, new)
    bank = filled(new * taps)
    nat.check(nat.lib().alive_resample_filter(orig, new, nat.ptr(bank), nat.stream()), "alive_resample_filter")
    return bank


def _resample(nat, x, orig, new, filt, pre, post, lout, rows=False):
    b, length = x.shape
    y = filled(b, lout)
    if rows:
        nat.check(nat.lib().alive_resample_rows(nat.ptr(x), b, length, orig, new, nat.ptr(filt), nat.ptr(pre), nat.ptr(post), nat.ptr(y), lout,
                                                nat.stream()), "alive_resample_rows")
    else:
        nat.check(nat.lib().alive_resample(nat.ptr(x), b, length, orig, new, nat.ptr(filt), pre, post, nat.ptr(y), lout, nat.stream()),
                  "alive_resample")
    return y


@pytest.mark.parametrize("orig,new", G.RESAMPLE_PAIRS)
def test_resample_filter_taps_and_length_are_the_formulas(orig, new):
    from module import _native as nat
    L = nat.lib()
    assert L.alive_resample_taps(orig, new) == G.resample_taps(orig, new)
    for length in (1, orig - 1, orig, orig + 1, 1000, G.impulse_case(orig, new)["L"]):
        assert L.alive_resample_length(length, orig, new) == G.resample_length(length, orig, new)
    b64 = G.resample_bank64(orig, new)
    want = b64.astype(np.float32).reshape(-1)
    got = _device_bank(nat, orig, new).cpu().numpy()
    assert not np.isnan(got).any(), "a tap was not written"
    loose = G.bank_sensitive(b64).reshape(-1)
    diff = got != want
    assert not (diff & ~loose).any(), f"{int((diff & ~loose).sum())} taps differ from the float64 formula; first {np.flatnonzero(diff & ~loose)[:5]}"
    one_ulp = np.abs(got.view(np.int32).astype(np.int64) - want.view(np.int32).astype(np.int64)) <= 1
    assert one_ulp[loose].all()


@pytest.mark.parametrize("orig,new", G.RESAMPLE_PAIRS)
def test_resample_impulses_read_the_bank_at_the_formulas_entries(orig, new):
    """impulses of 2^-1, pre 2, post 1/2: every output sample is bitwise 0 or half an entry filt[p][j], s = m orig - width + j"""
    from module import _native as nat
    c = G.impulse_case(orig, new)
    bank = _device_bank(nat, orig, new)
    bank_cpu = bank.cpu()
    x = dev(c["x"])
    for lout in c["louts"]:
        idx = torch.from_numpy(c["idx"](lout))
        want = torch.where(idx >= 0, bank_cpu[idx.clamp(min=0)] * 0.5, torch.zeros(()))
        same(_resample(nat, x, orig, new, bank, 2.0, 0.5, lout), want, f"alive_resample {orig} -> {new} L {c['L']} Lout {lout}")
        ones = torch.ones(2, device=DEV)
        same(_resample(nat, x, orig, new, bank, 2.0 * ones, 0.5 * ones, lout, rows=True), want,
             f"alive_resample_rows {orig} -> {new} L {c['L']} Lout {lout}")
    for rows in (False, True):
        pre, post = (torch.ones(2, device=DEV),) * 2 if rows else (1.0, 1.0)
        with pytest.raises(ValueError, match="alive_resample_rows" if rows else "alive_resample"):
            _resample(nat, x, orig, new, bank, pre, post, c["full"] + 1, rows=rows)


@pytest.mark.parametrize("orig,new,length", G.DENSE_PAIRS)
def test_resample_dense_sums_exact_on_an_integer_bank(orig, new, length):
    from module import _native as nat
    c = G.dense_case(orig, new, length)
    filt, x = dev(c["filt"]).reshape(-1), dev(c["x"])
    for lout in (c["full"], c["full"] - 1):
        want = torch.from_numpy(c["y"][:, :lout]).float()
        same(_resample(nat, x, orig, new, filt, c["pre"], c["post"], lout), want, f"alive_resample {orig} -> {new} L {length} Lout {lout}")


def test_resample_rows_is_alive_resample_row_by_row():
    from module import _native as nat
    gen = torch.Generator().manual_seed(11)
    for orig, new, length in ((3, 2, 1001), (441, 160, 1500)):
        x = torch.randn(3, length, generator=gen).to(DEV)
        bank = _device_bank(nat, orig, new)
        pre, post = torch.tensor([0.7, 1.0, 1.9], device=DEV), torch.tensor([1.3, 0.25, 1.0], device=DEV)
        lout = G.resample_length(length, orig, new)
        got = _resample(nat, x, orig, new, bank, pre, post, lout, rows=True)
        for b in range(3):
            want = _resample(nat, x[b:b + 1].contiguous(), orig, new, bank, pre[b].item(), post[b].item(), lout)
            same(got[b:b + 1], want.cpu(), f"alive_resample_rows {orig} -> {new} row {b}")
    # equal rates, no bank: (x * pre) * post, one rounding each
    x = torch.randn(3, 777, generator=gen).to(DEV)
    y = filled(3, 777)
    nat.check(nat.lib().alive_resample_rows(nat.ptr(x), 3, 777, 5, 5, None, nat.ptr(pre), nat.ptr(post), nat.ptr(y), 777, nat.stream()),
              "alive_resample_rows")
    same(y, (x.cpu() * pre.cpu()[:, None]) * post.cpu()[:, None], "alive_resample_rows at equal rates")
    with pytest.raises(ValueError, match="alive_resample_rows"):
        nat.check(nat.lib().alive_resample_rows(nat.ptr(x), 3, 777, 5, 5, None, nat.ptr(pre), nat.ptr(post), nat.ptr(y), 776, nat.stream()), "")


# ---- E. pitch transform -------------------------------------------------------------------------------------------------------------
def _pitch(nat, f0, mode, params):
    f = f0.clone()
    nat.check(nat.lib().alive_pitch_transform(nat.ptr(f), f.shape[0], f.shape[-1], mode, *params, nat.stream()), "alive_pitch_transform")
    return f


def _pitch_rows(nat, f0, mode, params):
    f = f0.clone()
    rate, shift, inton = (torch.tensor([p[k] for p in params], dtype=torch.float32, device=DEV) for k in range(3))
    nat.check(nat.lib().alive_pitch_transform_rows(nat.ptr(f), f.shape[0], f.shape[-1], mode, nat.ptr(rate), nat.ptr(shift), nat.ptr(inton),
                                                   nat.stream()), "alive_pitch_transform_rows")
    return f


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("t", G.PITCH_T)
def test_pitch_transform_exact_rows(t, mode):
    from module import _native as nat
    kinds = [k for k in G.PITCH_KINDS if k != "last stride" or t > 256]
    for params in G.PITCH_PARAMS:
        rows = [G.pitch_case(kind, t, mode, params) for kind in kinds]
        f0 = dev(np.stack([r[0] for r in rows])).view(len(kinds), 1, t)
        want = torch.from_numpy(np.stack([r[1] for r in rows])).view(len(kinds), 1, t)
        same(_pitch(nat, f0, mode, params), want, f"alive_pitch_transform T {t} mode {mode} {params} rows {kinds}")
        same(_pitch_rows(nat, f0, mode, [params] * len(kinds)), want, f"alive_pitch_transform_rows T {t} mode {mode} {params} rows {kinds}")


@pytest.mark.parametrize("mode", [0, 1])
def test_pitch_transform_rows_is_five_scalar_calls(mode):
    from module import _native as nat
    t = 450
    kinds = ("dense", "none", "one", "last stride", "dense")
    rows = [G.pitch_case(kind, t, mode, p) for kind, p in zip(kinds, G.PITCH_PARAMS)]
    f0 = dev(np.stack([r[0] for r in rows])).view(5, 1, t)
    got = _pitch_rows(nat, f0, mode, G.PITCH_PARAMS)
    same(got, torch.from_numpy(np.stack([r[1] for r in rows])).view(5, 1, t), f"alive_pitch_transform_rows mode {mode}, exact rows")
    # general values: voiced frames 80 .. 400 Hz with gaps, general parameters
    gen = torch.Generator().manual_seed(3)
    f0 = (80.0 + 320.0 * torch.rand(5, 1, 333, generator=gen)) * (torch.rand(5, 1, 333, generator=gen) > 0.3)
    f0[3] = 0.0
    f0 = f0.to(DEV)
    params = ((1.0, 0.0, 1.0), (0.9, 3.5, 0.7), (1.1, -2.25, 1.4), (1.0, 7.0, 1.0), (2.0, -12.0, 0.3))
    got = _pitch_rows(nat, f0, mode, params)
    for n, p in enumerate(params):
        same(got[n:n + 1], _pitch(nat, f0[n:n + 1].contiguous(), mode, p).cpu(), f"row {n} mode {mode}")
    assert bool((got[3] == 0).all())


# ---- F. gelu + FiLM in a frame range ------------------------------------------------------------------------------------------------
def _plane_bits(P, n, c, length, planes=2):
    """the planes as int16 [planes][n][c][length] (k-blocked, csrc/planes_layout.h)"""
    cols = n * length
    cols_pad = (cols + 127) // 128 * 128
    v = P.view(torch.int16).view(planes, c // 32, cols_pad, 32)[:, :, :cols]
    return v.permute(0, 2, 1, 3).reshape(planes, n, length, c).permute(0, 1, 3, 2).cpu()


def _gelu_film(nat, h, film, frames, t0, f0, planes):
    n, c, length = h.shape
    L = nat.lib()
    z = None if planes else filled(n, c, length)
    zp = torch.full((L.alive_planes_bytes(n * length, c, 2),), 0xFF, dtype=torch.uint8, device=DEV) if planes else None
    nat.check(L.alive_gelu_film(nat.ptr(h), n, c, length, nat.ptr(film), film.shape[1], frames, G.FILM_OFF, G.FILM_OFF + c, t0, f0,
                                film.shape[2], nat.ptr(z), nat.ptr(zp), nat.stream()), "alive_gelu_film")
    return _plane_bits(zp, n, c, length) if planes else z.cpu()


@pytest.mark.parametrize("planes", [False, True])
@pytest.mark.parametrize("c,spf", G.FILM_SHAPES)
def test_gelu_film_on_a_frame_range_is_the_windows_slice(c, spf, planes):
    """as the streaming decoder calls it (csrc/networks.hip: t0 = first frame x samples per frame, f0 = first frame, film_ld = the range's
    frames, the film tensor holding the range's columns only)"""
    from module import _native as nat
    h, film = G.film_case(c, spf)
    hd, fd = h.to(DEV), film.to(DEV)
    whole = _gelu_film(nat, hd, fd, G.FILM_FRAMES, 0, 0, planes)
    assert bool(torch.isfinite(whole.view(torch.bfloat16).float() if planes else whole).all()), "every element of the window was written"
    for lo, hi in G.FILM_RANGES:
        ok = torch.from_numpy(G.film_range_columns(spf, (lo, hi)))
        part = _gelu_film(nat, hd[:, :, lo * spf:hi * spf].contiguous(), fd[:, :, lo:hi].contiguous(), G.FILM_FRAMES, lo * spf, lo, planes)
        ref = whole[..., lo * spf:hi * spf]
        assert torch.equal(part[..., ok], ref[..., ok]), f"C {c} range {lo} .. {hi - 1}: differs where both frames lie inside the range"
        vals = part.view(torch.bfloat16).float() if planes else part
        assert bool(torch.isfinite(vals).all()), "finite (and written) outside that set too"
