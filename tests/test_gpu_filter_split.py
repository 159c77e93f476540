"""The fused split-bf16 FilterBlocks -- csrc/filter_small.hip (C = 8, 16: ops.filter_block_small[_range]) and csrc/filter_mid.hip (C = 64:
ops.filter_block64) -- per column and in every tile form.  Needs an MI355X; tests/test_host_filter_split.py is the host twin.

A. The noise profile against the exact float64 block, per instantiation: rms error per column and per channel, total and largest error,
   kernel over emulation, inside the bars derived from the null band of two emulations (tools/filter_split_ref.py::BARS) -- at both
   ends; the largest frame density the launchers admit, and their refusal of one frame more.
B. A window's samples do not depend on the form that computed them: the batch forms against the short-signal forms of the same window
   alone, the fp16 sweep form against the tiled form, bit for bit in one process.
C. Range mode against the whole signal: bitwise inside the margins, inside the bars as a whole.
Every case asserts through small_plan / mid_plan which instantiation it runs.
"""
import os
import sys

import pytest
import torch

import alive_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import filter_split_ref as R                                         # noqa: E402


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)).item()


def _device_film(cnd, fw):
    from module import ops
    film, _ = ops.conv1d(cnd.to(DEV), fw[0].to(DEV), fw[1].to(DEV), post_add=fw[2].to(DEV))
    return film


def _block(c, ranged=False):
    from module import ops
    return ops.filter_block64 if c == 64 else ops.filter_block_small_range if ranged else ops.filter_block_small


def _run_nan_filled(c, x, sd, film, skip, group, **kw):
    """the block on x in calls of `group` windows, each into an output pre-filled with NaN -> the outputs, on the host"""
    outs = []
    for s in range(0, x.shape[0], group):
        out = torch.full((min(group, x.shape[0] - s),) + tuple(x.shape[1:]), float("nan"), device=DEV)
        got = _block(c)(x[s:s + group].to(DEV), sd, "n", film[s:s + group].contiguous(), R.PAD_ROWS, skip=skip[s:s + group].to(DEV), out=out, **kw)
        assert got is out
        outs.append(out.cpu())
    return torch.cat(outs)


def _assert_bars(name, key, out, emu, exact):
    assert out.shape == exact.shape and not bool(torch.isnan(out).any()), f"{name}: columns left unwritten"
    r = R.profile_ratios(out, emu, exact)
    bars = R.BARS[key]
    print(f"{name}: " + R.describe(r) + "; bars " + ", ".join(f"{s} {lo:.3f} .. {hi:.3f}" for s, (lo, hi) in bars.items()))
    bad = R.check_bars(r, key)
    assert not bad, (name, bad)


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.ACCURACY, ids=lambda s: s.name)
def test_noise_profile_against_the_exact_block(case):
    """kernel over the "f32" emulation of its operand splits on the device's own fp32 FiLM table, errors against the exact float64 block:
    per column, per channel, total and largest inside the bars; every output written; the global figure of
    test_fused_filter_block_small against the fp32 oracle.  A non-identity input conv, a skip, FiLM rows at PAD_ROWS."""
    p = case.plan()                                                    # (asserts the form the case names)
    sd, fw = R.block_weights(case.C)
    x, cnd, skip = R.inputs(case.C, case.l, case.lf, case.n)
    film = _device_film(cnd, fw)
    out = _run_nan_filled(case.C, x, {k: v.to(DEV) for k, v in sd.items()}, film, skip, case.per_call)
    film = film.cpu()
    exact = R.filter_block_split(x, film, R.PAD_ROWS, sd, "n", skip=skip, rounding=False)
    emu = R.filter_block_split(x, film, R.PAD_ROWS, sd, "n", skip=skip, flavour="f32")
    e = relerr(out, O.filter_block(sd, "n", x, cnd) + skip)
    print(f"{case.name}: forms {p.forms}, {p.tiles} tiles x {case.per_call} windows per call, global {e:.3e}")
    _assert_bars(case.name, case.key, out, emu, exact)
    assert e < 4e-5, e


def _raw_call(c, n, l, film, out, lf):
    """the entry point itself on zero inputs and weights: -> its return code"""
    from module import _native as nat
    L_ = nat.lib()
    x = torch.zeros(n, c, l, device=DEV)
    s = torch.cuda.current_stream().cuda_stream
    if c == 64:
        w = torch.zeros(L_.alive_filter_block64_weights(), dtype=torch.bfloat16, device=DEV)
        b = torch.zeros(7, 64, device=DEV)
        rc = L_.alive_filter_block64(x.data_ptr(), n, l, w.data_ptr(), b.data_ptr(), film.data_ptr(), film.shape[1], lf, 0, None, out.data_ptr(), s)
    else:
        w = torch.zeros(L_.alive_filter_block_small_weights(c), device=DEV)
        rc = L_.alive_filter_block_small(x.data_ptr(), n, c, l, w.data_ptr(), film.data_ptr(), film.shape[1], lf, 0, None, out.data_ptr(), s)
    torch.cuda.synchronize()
    return rc


@pytest.mark.parametrize("c,n,l,lf,l_bad,lf_bad", [(c, n, l, lf, l, lf + 1) for c, n, l, lf in R.DENSEST] + [(c, n, l, lf, l - 4, lf) for c, n, l, lf in R.SHORTEST])
def test_one_frame_more_than_the_densest_table_is_refused(c, n, l, lf, l_bad, lf_bad):
    """the launchers' bound BL lf / L + 3 <= NFP: the densest tables are exactly at it and run (zeros in, the bias-free block of zeros
    out), as do the shortest windows with one frame; one frame more, or one vector of columns less, is refused with an error that
    names the entry point and nothing is launched -- the output keeps its fill; frames_admitted says the same on the host"""
    from module import _native as nat
    assert R.plan_for(c, n, l).frames_admitted(l, lf) and not R.plan_for(c, n, l_bad).frames_admitted(l_bad, lf_bad)
    out = torch.full((n, c, l_bad), 7.0, device=DEV)
    rc = _raw_call(c, n, l_bad, torch.zeros(n, 12 * c, lf_bad, device=DEV), out, lf_bad)
    assert rc != 0
    with pytest.raises(ValueError) as err:
        nat.check(rc)
    assert ("alive_filter_block64" if c == 64 else "alive_filter_block_small") in str(err.value) and "frames" in str(err.value), str(err.value)
    assert bool((out == 7.0).all()), "a refused call wrote its output"
    out = torch.full((n, c, l), 7.0, device=DEV)
    nat.check(_raw_call(c, n, l, torch.zeros(n, 12 * c, lf, device=DEV), out, lf))
    assert bool((out == 0.0).all())


# ---- B ---------------------------------------------------------------------------------------------------------------------
def _random_block(c, n, l, lf, seed):
    gen = torch.Generator(device=DEV).manual_seed(seed)
    sd, _ = R.block_weights(c)
    return ({k: v.to(DEV) for k, v in sd.items()}, torch.randn(n, c, l, device=DEV, generator=gen),
            torch.randn(n, 12 * c + R.PAD_ROWS, lf, device=DEV, generator=gen) * 0.3, torch.randn(n, c, l, device=DEV, generator=gen))


ALONE = {"16-16k-rest": ((16, True, 8192),), "8-16k-rest": ((8, True, 8192),), "64-nt4-rest": ((True, 2, False, False),),
         "64-plain-sweep": ((True, 4, True, False),)}


@pytest.mark.parametrize("name", list(ALONE))
def test_a_windows_samples_do_not_depend_on_the_form(name):
    """every window of a call that runs tile 0 by the FIRST form and the others by the lane-constant form (16-KB planes, NTT 4; with
    plain=True the fp16 sweep form, whose comment claims the tiled form's bits) equals, bit for bit, the same window run alone, where the
    launch rules pick the short-signal form (8-KB planes, NTT 2) or, for the fp16 block, the tiled FIRST form for every tile"""
    plain, alone_form = name == "64-plain-sweep", ALONE[name]
    if plain:
        c, n, l, lf = 64, 17, 3204, 40
        p = R.mid_plan(n, l, h16=True)
        assert p.forms == ((True, 4, True, False), (False, 4, True, True)) and p.tiles * n > R.FIRST_ONLY_TILES and p.segments > 1
    else:
        case = next(k for k in R.ACCURACY if k.name == name)
        c, n, l, lf = case.C, case.n, case.l, case.lf
        p = case.plan()
        assert len(p.forms) == 2 and not p.forms[1][1 if c != 64 else 0]
    alone = R.plan_for(c, 1, l, plain)
    assert alone.forms == alone_form and alone.frames_admitted(l, lf) and p.frames_admitted(l, lf)
    sd, x, film, skip = _random_block(c, n, l, lf, 23)
    kw = dict(plain=True) if plain else {}
    whole = _block(c)(x, sd, "n", film, R.PAD_ROWS, skip=skip, **kw)
    assert bool(torch.isfinite(whole).all())
    differ = [i for i in range(n)
              if not torch.equal(_block(c)(x[i:i + 1], sd, "n", film[i:i + 1].contiguous(), R.PAD_ROWS, skip=skip[i:i + 1], **kw), whole[i:i + 1])]
    assert not differ, f"windows {differ} differ from their own call"


# ---- C ---------------------------------------------------------------------------------------------------------------------
def _range_against_the_whole(rc, plain):
    """-> (the range run with its inputs on the host); asserts what is bitwise"""
    c, up, t0, l = rc.C, rc.up, rc.up * rc.f0, rc.up * rc.nf
    n = rc.n
    pw, pr = R.plan_for(c, n, up * rc.frames, plain), R.plan_for(c, n, l, plain)
    assert pr.frames_admitted(l, rc.nf) and pw.frames_admitted(up * rc.frames, rc.frames)
    assert len(pw.forms) == 2 and pw.sweep == plain if c == 64 else len(pw.forms) == 2, "the whole signal runs the batch forms"
    assert pr.all_first == rc.range_all_first, pr
    print(f"C {c} frames {rc.f0} .. {rc.f0 + rc.nf - 1}: range forms {pr.forms} ({pr.tiles} tiles), whole {pw.forms} ({pw.tiles} tiles)")
    sd, fw = R.block_weights(c)
    x, cnd, skip = R.inputs(c, up * rc.frames, rc.frames, n)
    film = _device_film(cnd, fw)
    sdd = {k: v.to(DEV) for k, v in sd.items()}
    kw = dict(plain=True) if plain else {}
    whole = _block(c, True)(x.to(DEV), sdd, "n", film, R.PAD_ROWS, skip=skip.to(DEV), **kw)
    xs, ss, fs = x[:, :, t0:t0 + l].contiguous(), skip[:, :, t0:t0 + l].contiguous(), film[:, :, rc.f0:rc.f0 + rc.nf].contiguous()
    part = torch.full((n, c, l), float("nan"), device=DEV)
    _block(c, True)(xs.to(DEV), sdd, "n", fs, R.PAD_ROWS, skip=ss.to(DEV), t0=t0, f0=rc.f0, frames=rc.frames, out=part, **kw)
    lo, hi = rc.margins
    assert not bool(torch.isnan(part).any())
    assert torch.equal(part[:, :, lo:hi], whole[:, :, t0 + lo:t0 + hi])
    assert not torch.equal(part[:, :, :16], whole[:, :, t0:t0 + 16])
    return sd, xs, ss, fs.cpu(), part.cpu()


@pytest.mark.parametrize("rc", R.RANGES, ids=lambda r: f"{r.C}-f{r.f0}")
def test_a_frame_range_is_the_whole_signals_run_inside_its_margins(rc):
    """frames f0 .. f0 + nf - 1 of a 128-frame signal at the scale's samples per frame, from their FiLM columns only (t0 / f0 / frames):
    past the reach of the range's start (its first columns interpolate towards frame f0 - 1, which the table does not hold, and the
    reflected context reaches 56 columns further) and short of its last frame the samples are the whole run's, bit for bit, whatever
    tile and form they fall into; the first 16 columns are the range's own (its reflected start); and the whole range run, edges
    included, meets the bars against the host's restatement of the clamped table columns and the reflected start"""
    sd, xs, ss, fs, part = _range_against_the_whole(rc, False)
    rng = dict(t0=rc.up * rc.f0, f0=rc.f0, frames=rc.frames)
    exact = R.filter_block_split(xs, fs, R.PAD_ROWS, sd, "n", skip=ss, rounding=False, **rng)
    emu = R.filter_block_split(xs, fs, R.PAD_ROWS, sd, "n", skip=ss, flavour="f32", **rng)
    _assert_bars(f"{rc.C}-range-f{rc.f0}", str(rc.C), part, emu, exact)


@pytest.mark.parametrize("rc", [r for r in R.RANGES if r.C == 64], ids=lambda r: f"64-plain-f{r.f0}")
def test_a_frame_range_of_the_fp16_block_is_the_whole_signals_run_inside_its_margins(rc):
    """the same for the fp16 form of the 64-channel block (plain=True), bitwise only: the whole signal by the sweep form, the range by the
    tiled FIRST form"""
    _range_against_the_whole(rc, True)
