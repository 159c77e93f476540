"""Every launch form of csrc/oscillator.hip against the CPU phase arithmetic: pieces (Q = 8) and whole frames (Q = 1), the switch
between them at N * Lf = 64 / 65, fewer than 64 harmonics, segment lengths and sample rates other than 320 / 16000, crop0 and
phi_col anywhere in the window, the frame-range entry on its own, the workspace size the library reports, the argument checks.

The reference (`reference` below) is oracle/alive_oracle.py::harmonic_oscillator from the amplitudes on, in fp32 on the CPU -- not a
float64 phase: the defined behaviour is the fp32-rounded prefix of an fp64 running sum, and a better phase would disagree with a
correct kernel.  `assert_prefixes_order_free` proves for each case's inputs that no rounded prefix depends on how the fp64 sum is
associated (sequentially, per frame, per eighth of a frame), so the kernel's theta is bit for bit the reference's and what is left
is sin_phase (< 2 ulp) against the CPU sinf, times the amplitude, averaged over H: one bar for every case, 1e-5 (that of
test_gpu_ops.py::test_oscillator_long_window_phase_exact, same amplitude draw).  phi_out: rtol 1e-4 / atol 2e-5 (test_oscillator_golden)
where the reference's |phi| < 1.45 (the fold guard of test_gpu_streaming.py), on at least 80 % of the (n, h) entries.

Measured maxima on the MI355X (every case prints its own, `pytest -s`):

    case                                         wave max abs   phi_out max abs (guarded)
    1 pieces, N=3 H=64 Lf=19 (4 crop0 x 3 cols)  1.8e-7         3.6e-7
    2 whole frames, N=4 H=64 Lf=19               2.4e-7         3.6e-7      rows 0-2 bitwise those of case 1
    3 switch, N*Lf = 64 (1x64, 8x8)              2.4e-7         2.4e-7
    3 switch, N*Lf = 65 / 72                     1.8e-7 / 2.4e-7  3.6e-7 / 2.4e-7
    4 H = 1 / 8 / 37, pieces                     2.4e-7 / 1.2e-7 / 1.8e-7   1.2e-7 / 1.2e-7 / 2.4e-7
    4 H = 1 / 8 / 37, whole frames               2.4e-7 / 1.2e-7 / 1.8e-7   1.2e-7 / 1.2e-7 / 2.4e-7
    5 seg 200 at 22050 / seg 63 at 48000         1.5e-7 / 1.2e-7  2.4e-7 / 2.4e-7
    5 seg 512 / seg 8 at 16000                   1.8e-7 / 7.5e-8  2.4e-7 / 3.6e-7
    6 ranges [5,17) [0,7) [17,24) [9,10) of 24   1.2e-7 / 2.1e-7 / 1.8e-7 / 3.0e-8   1.8e-7 / 1.8e-7 / 2.4e-7 / 1.8e-7
    6 range [11,29) of 40, N=3                   2.7e-7         2.4e-7
No case came near the bars, so no sample had to be located: the kernel's dt is the reference's everywhere.
"""
import functools
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alive_oracle as O
from module import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
WAVE_BAR = 1e-5
PHI_GUARD, PHI_RTOL, PHI_ATOL, PHI_MIN_FRACTION = 1.45, 1e-4, 2e-5, 0.8
_MAXIMA = {}


def g(name, shape, seed=7, scale=1.0):
    return synthetic.gaussian(name, seed, shape, scale)


def record(case, wave_err, phi_err=None):
    m = _MAXIMA.setdefault(case, {"wave_max_abs": 0.0, "phi_max_abs": 0.0})
    m["wave_max_abs"] = max(m["wave_max_abs"], float(wave_err))
    if phi_err is not None:
        m["phi_max_abs"] = max(m["phi_max_abs"], float(phi_err))
    print("oscillator forms:", case, json.dumps(m))                     # the running maximum of the case (pytest -s shows it)


# ---- inputs: drawn per row, so that a row is the same whatever batch it sits in --------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(tag, n, h, lf):
    f0 = torch.empty(n, 1, lf)
    for r in range(n):
        f0[r, 0] = torch.from_numpy(60.0 + 1000.0 * synthetic.uniform01(f"osc.f0.{tag}.{r}", 5, lf)).float()
    f0[:, :, lf // 3: lf // 3 + 3] = 0.0                                 # voiced / unvoiced transitions
    if n >= 2:
        f0[1] = 0.0                                                      # no voiced frame: dt == 0, wave = mean(sin(phi) * amps)
    if n >= 3:
        f0[2, 0, 1:] = 0.0                                               # voiced in frame 0 only
    amps = torch.cat([torch.exp(g(f"osc.amp.{tag}.{r}", (1, h, lf), scale=0.5)) for r in range(n)])
    phi = torch.cat([torch.from_numpy((synthetic.uniform01(f"osc.phi.{tag}.{r}", 5, h) - 0.5) * np.pi).float().view(1, h)
                     for r in range(n)])
    return f0, amps, phi


def inputs(tag, n, h, lf):
    return tuple(t.clone() for t in _inputs(tag, n, h, lf))


# ---- the reference: oracle/alive_oracle.py::harmonic_oscillator line for line, from amps instead of to_amps weights ---------
def reference(amps, f0, phi=0, crop0=0, segment=320, sample_rate=16000):
    n, nh, lf = amps.shape
    lw = lf * segment
    mul = (torch.arange(nh) + 1).view(1, nh, 1).expand(n, nh, lf)
    formants = f0 * mul
    formants = F.interpolate(formants, lw, mode="linear")
    amps = F.interpolate(amps, lw, mode="linear")
    dt = torch.cumsum(formants / sample_rate, dim=2)
    dt = dt - dt[:, :, crop0].unsqueeze(2)
    theta = O.TWO_PI * dt + phi
    harmonics = torch.sin(theta)
    phi_out = torch.asin(harmonics)
    wave = (harmonics * amps).mean(dim=1, keepdim=True)
    return wave, phi_out


def assert_prefixes_order_free(f0, nh, segment, sample_rate):
    """torch.cumsum on fp32 == fp32(sequential fp64 sum) at every sample, and so is the kernel's re-association: fp64 sums of
    pieces of `sub` samples, their exclusive scan, then the running sum inside the piece -- for whole frames and for eighths."""
    n, _, lf = f0.shape
    mul = (torch.arange(nh) + 1).view(1, nh, 1).expand(n, nh, lf)
    q = F.interpolate(f0 * mul, lf * segment, mode="linear") / sample_rate
    want = torch.cumsum(q, dim=2)
    assert torch.equal(want, torch.cumsum(q.double(), dim=2).float()), "cumsum is not the rounded sequential fp64 sum: change the draw"
    for sub in {segment, segment // 8 if segment % 8 == 0 else segment}:
        qd = q.double().view(n, nh, -1, sub)
        s = torch.cumsum(qd, dim=3)[..., -1]
        start = torch.cat([torch.zeros_like(s[..., :1]), torch.cumsum(s, dim=2)[..., :-1]], dim=2)      # exclusive scan: 0, s0, s0 + s1
        got = torch.cumsum(torch.cat([start.unsqueeze(3), qd], dim=3), dim=3)[..., 1:].reshape(n, nh, -1).float()
        bad = int((got != want).sum())
        assert bad == 0, f"{bad} of {want.numel()} rounded prefixes depend on the summation order (pieces of {sub}): change the draw"


@functools.lru_cache(maxsize=None)
def _case_reference(tag, n, h, lf, crop0, segment, sample_rate):
    """(wave, phi_out[N, H, Lw]) of a case, computed once (the pre-check of its inputs included) and left unchanged"""
    f0, amps, phi = _inputs(tag, n, h, lf)
    assert_prefixes_order_free(f0, h, segment, sample_rate)
    return reference(amps, f0, phi.view(n, h, 1), crop0, segment, sample_rate)


def check_phi(case, got, ref_col):
    ok = ref_col.abs() < PHI_GUARD
    frac = ok.float().mean().item()
    assert frac >= PHI_MIN_FRACTION, f"{case}: only {frac:.2f} of the (n, h) entries are away from the fold"
    err = (got - ref_col).abs()[ok].max().item()
    torch.testing.assert_close(got[ok], ref_col[ok], rtol=PHI_RTOL, atol=PHI_ATOL)
    return err


def run_case(case, tag, n, h, lf, crop0, phi_cols, segment=320, sample_rate=16000):
    """one window through ops.oscillator (once per phi_col) against the reference over the whole wave; returns the device wave"""
    from module import ops
    ow, ophi = _case_reference(tag, n, h, lf, crop0, segment, sample_rate)
    f0, amps, phi = inputs(tag, n, h, lf)
    first = None
    for col in phi_cols:
        wave, phi_out = ops.oscillator(amps.to(DEV), f0.to(DEV), phi=phi.to(DEV), crop0=crop0, phi_col=col, seg=segment,
                                       sample_rate=float(sample_rate))
        wave, phi_out = wave.cpu(), phi_out.cpu()
        assert wave.shape == ow.shape
        err = (wave - ow).abs().max().item()
        perr = check_phi(case, phi_out, ophi[:, :, col])
        record(case, err, perr)
        assert err < WAVE_BAR, (case, col, err)
        if first is None:
            first = wave
        else:
            assert torch.equal(wave, first), "the wave depends on phi_col"
    return first


def test_reference_helper_is_the_oracle(golden_dir):
    """the test-local reference cannot drift: bitwise O.harmonic_oscillator on the blk_oscillator fixture"""
    z = np.load(os.path.join(golden_dir, "blk_oscillator.npz"))
    sd = {"n." + k[3:]: torch.from_numpy(z[k]) for k in z.files if k.startswith("w::")}
    x, f0 = torch.from_numpy(z["x"]), torch.from_numpy(z["f0"])
    amps = torch.exp(F.conv1d(x, sd["n.to_amps.weight"], sd["n.to_amps.bias"]))
    for phi, crop0 in ((0, 0), (g("osc.helper.phi", (2, 8, 1)), 1613)):
        ow, oph = O.harmonic_oscillator(sd, "n", x, f0, phi=phi, crop0=crop0)
        w, ph = reference(amps, f0, phi, crop0)
        assert torch.equal(w, ow) and torch.equal(ph, oph)


# ---- 1 / 2: pieces at full width, and the same rows as whole frames ---------------------------------------------------------
LW19 = 19 * 320
CROPS = [0, 795, 1613, LW19 - 1]          # 795: realtime_geometry(160, 16, 24000); neither 795 nor 1613 is a multiple of the piece (40)
PHI_COLS = (0, 901, LW19 - 1)


@pytest.mark.parametrize("crop0", CROPS)
def test_pieces_at_full_width(crop0):
    """N = 3, H = 64, Lf = 19: N * Lf = 57 <= 64, eight pieces per frame (the streaming form) at the product's harmonic count"""
    run_case("1 pieces H=64", "rows", 3, 64, 19, crop0, PHI_COLS)


@pytest.mark.parametrize("crop0", CROPS)
def test_whole_frames_same_rows(crop0):
    """the same three rows plus a fourth: N * Lf = 76, a wave per frame.  Against the reference, and rows 0-2 bitwise those of the
    piece form (no rounded prefix depends on the association: assert_prefixes_order_free) -- a session sounds the same alone and
    in a batch of nine"""
    from module import ops
    w4 = run_case("2 whole frames H=64", "rows", 4, 64, 19, crop0, PHI_COLS)
    f0, amps, phi = inputs("rows", 3, 64, 19)
    for a, b in zip(inputs("rows", 4, 64, 19), (f0, amps, phi)):
        assert torch.equal(a[:3], b)
    w3, p3 = ops.oscillator(amps.to(DEV), f0.to(DEV), phi=phi.to(DEV), crop0=crop0, phi_col=901)
    f0, amps, phi = inputs("rows", 4, 64, 19)
    _, p4 = ops.oscillator(amps.to(DEV), f0.to(DEV), phi=phi.to(DEV), crop0=crop0, phi_col=901)
    assert torch.equal(w4[:3], w3.cpu()), "rows differ between the piece form and the whole-frame form"
    assert torch.equal(p4[:3].cpu(), p3.cpu())


# ---- 3: the switch ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lf", [(1, 64), (8, 8), (5, 13), (9, 8)])
def test_switch_between_the_forms(n, lf):
    """N * Lf = 64, 64 (pieces), 65, 72 (whole frames): eight streaming sessions take one form and nine the other"""
    from module import _native as nat
    assert nat.lib().alive_oscillator_workspace_bytes(n, 64, lf) >= n * 64 * lf * (8 if n * lf <= 64 else 1) * 8 + n * 64 * 4
    lw = lf * 320
    run_case(f"3 switch N*Lf={n * lf}", f"sw{n}x{lf}", n, 64, lf, 1200, (lw - 123,))


# ---- 4: fewer than 64 harmonics ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lf", [(2, 12), (3, 30)])
@pytest.mark.parametrize("h", [1, 8, 37])
def test_fewer_harmonics(h, n, lf):
    """lanes with h >= H are idle, on both forms (N * Lf = 24: pieces; 90: whole frames)"""
    run_case(f"4 H={h} {'pieces' if n * lf <= 64 else 'whole frames'}", f"h{h}", n, h, lf, 795, (901,))


# ---- 5: other segment lengths and sample rates ----------------------------------------------------------------------------------
@pytest.mark.parametrize("seg,rate,n,h,lf,crop0", [
    (200, 22050, 2, 37, 12, 1013),       # pieces of 25: a batch tail of 9, the (i0, i1) pair changes inside a batch; __fdiv_rn
    (63, 48000, 2, 8, 10, 200),          # odd seg: whole frames at few frames (batches 16, 16, 16, 15); __fdiv_rn
    (512, 16000, 1, 64, 6, 1000),        # MAX_SEG, pieces of 64
    (8, 16000, 2, 64, 20, 77),           # one-sample pieces (every crop0 is a multiple of seg / 8 = 1 here: one that is none of seg)
])
def test_other_segment_lengths_and_rates(seg, rate, n, h, lf, crop0):
    assert crop0 % seg != 0 and (seg == 8 or seg % 8 != 0 or crop0 % (seg // 8) != 0)
    lw = lf * seg
    run_case(f"5 seg={seg} rate={rate}", f"seg{seg}", n, h, lf, crop0, (crop0 // 2 + 3, lw - 1), segment=seg, sample_rate=rate)


# ---- 6: the frame range on its own ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,lf,begin,end", [(2, 24, 5, 17), (2, 24, 0, 7), (2, 24, 17, 24), (2, 24, 9, 10), (3, 40, 11, 29)])
def test_frame_range(n, lf, begin, end):
    """alive_oscillator_range is given the range's amps only and clamps neighbour frames into the range, so it computes the window
    whose amps are the range's with the first and last frame replicated outward: the WHOLE range, edges included, must match that
    reference (N * Lf = 48: pieces; 120: whole frames).  Where the range touches the window's own edge, the samples on that side
    (up to half a frame short of the inner edge, where interpolation starts to see the frame beyond) are bitwise the full call's."""
    from module import ops
    seg, h, crop0 = 320, 64, 795
    tag = f"rng{n}x{lf}"
    f0, amps, phi = inputs(tag, n, h, lf)
    assert_prefixes_order_free(f0, h, seg, 16000)
    col = begin * seg + 77
    cols = (torch.arange(lf) - begin).clamp(0, end - begin - 1) + begin
    ow, ophi = reference(amps[:, :, cols], f0, phi.view(n, h, 1), crop0)
    ow = ow[:, :, begin * seg: end * seg]
    wave, phi_out = ops.oscillator(amps[:, :, begin:end].contiguous().to(DEV), f0.to(DEV), phi=phi.to(DEV), crop0=crop0, phi_col=col,
                                   f_begin=begin, n_frames=end - begin)
    wave = wave.cpu()
    assert wave.shape == ow.shape
    err = (wave - ow).abs().max().item()
    case = f"6 range [{begin},{end}) of {lf} N={n}"
    perr = check_phi(case, phi_out.cpu(), ophi[:, :, col])
    record(case, err, perr)
    assert err < WAVE_BAR, (case, err)
    full, _ = ops.oscillator(amps.to(DEV), f0.to(DEV), phi=phi.to(DEV), crop0=crop0)
    full = full.cpu()[:, :, begin * seg: end * seg]
    if begin == 0:
        k = (end - begin) * seg - seg // 2
        assert torch.equal(wave[:, :, :k], full[:, :, :k]), "the range differs from the full window at the window's left edge"
    if end == lf:
        assert torch.equal(wave[:, :, seg // 2:], full[:, :, seg // 2:]), "the range differs from the full window at the window's right edge"
    if 0 < begin and end < lf and end - begin > 1:
        assert torch.equal(wave[:, :, seg // 2: -(seg // 2)], full[:, :, seg // 2: -(seg // 2)])


# ---- 7: the workspace the library reports is the workspace it uses --------------------------------------------------------------
def banded(nbytes, dtype=torch.uint8):
    """nbytes of payload between two 4 KB bands of 0x5A: (whole buffer as bytes, payload view)"""
    raw = torch.zeros(nbytes + 8192, dtype=torch.uint8, device=DEV)
    raw[:4096] = 0x5A
    raw[4096 + nbytes:] = 0x5A
    return raw, raw[4096:4096 + nbytes].view(dtype)


@pytest.mark.parametrize("n,lf,begin,end", [(3, 19, 0, 19), (4, 19, 0, 19), (2, 24, 5, 17)])
def test_workspace_is_what_the_library_reports(n, lf, begin, end):
    """the C entry with a workspace of exactly alive_oscillator_workspace_bytes(N, H, Lf) bytes, wave and phi_out each between guard
    bands: pieces, whole frames, a range.  Every band intact, the outputs bitwise those of the ops call"""
    from module import _native as nat
    from module import ops
    L = nat.lib()
    h, seg, crop0, nf = 64, 320, 795, end - begin
    col = begin * seg + 901
    f0, amps, phi = (t.to(DEV) for t in inputs("rows" if lf == 19 else f"rng{n}x{lf}", n, h, lf))
    amps = amps[:, :, begin:end].contiguous()
    ranged = nf != lf
    want_w, want_p = ops.oscillator(amps, f0, phi=phi, crop0=crop0, phi_col=col, **(dict(f_begin=begin, n_frames=nf) if ranged else {}))
    ws_bytes = L.alive_oscillator_workspace_bytes(n, h, lf)
    ws_raw, ws = banded(ws_bytes)
    w_raw, wave = banded(n * nf * seg * 4, torch.float32)
    p_raw, phi_out = banded(n * h * 4, torch.float32)
    assert ws.data_ptr() % 256 == 0
    if ranged:
        rc = L.alive_oscillator_range(nat.ptr(amps), nat.ptr(f0), nat.ptr(phi), n, h, lf, seg, 16000.0, crop0, col, begin, nf,
                                      nat.ptr(wave), nat.ptr(phi_out), nat.ptr(ws), nat.stream())
    else:
        rc = L.alive_oscillator(nat.ptr(amps), nat.ptr(f0), nat.ptr(phi), n, h, lf, seg, 16000.0, crop0, col,
                                nat.ptr(wave), nat.ptr(phi_out), nat.ptr(ws), nat.stream())
    nat.check(rc, "alive_oscillator")
    torch.cuda.synchronize()
    for name, raw in (("workspace", ws_raw), ("wave", w_raw), ("phi_out", p_raw)):
        assert bool((raw[:4096] == 0x5A).all() and (raw[raw.numel() - 4096:] == 0x5A).all()), f"the oscillator wrote outside its {name}"
    assert torch.equal(wave.view(n, 1, nf * seg), want_w) and torch.equal(phi_out.view(n, h), want_p)


# ---- 8: refusals ------------------------------------------------------------------------------------------------------------
def test_argument_checks():
    """host-side argument checks: a negative code, alive_last_error() names the entry, nothing is launched (every output keeps
    its fill)"""
    from module import _native as nat
    L = nat.lib()
    n, h, lf, seg = 2, 8, 6, 320
    lw = lf * seg
    amps = torch.ones(n, 64, lf, device=DEV)
    f0 = torch.full((n, 1, lf), 100.0, device=DEV)
    wave = torch.full((n, 1, lw), 7.0, device=DEV)
    phi_out = torch.full((n, 65), 7.0, device=DEV)
    ws = torch.zeros(L.alive_oscillator_workspace_bytes(n, 65, lf), dtype=torch.uint8, device=DEV)
    A, F0, W, P, S = (nat.ptr(t) for t in (amps, f0, wave, phi_out, ws))

    def full(amps=A, f0=F0, n=n, h=h, lf=lf, seg=seg, crop0=0, phi_col=0, wave=W, phi_out=P, ws=S):
        return L.alive_oscillator(amps, f0, None, n, h, lf, seg, 16000.0, crop0, phi_col, wave, phi_out, ws, nat.stream())

    def ranged(begin, nf, phi_col=0, phi_out=None):
        return L.alive_oscillator_range(A, F0, None, n, h, lf, seg, 16000.0, 0, phi_col, begin, nf, W, phi_out, S, nat.stream())

    refusals = {
        "H = 65": lambda: full(h=65),
        "seg = 513": lambda: full(seg=513),
        "seg = 0": lambda: full(seg=0),
        "crop0 = Lw": lambda: full(crop0=lw),
        "crop0 < 0": lambda: full(crop0=-1),
        "phi_col = Lw with a phi_out": lambda: full(phi_col=lw),
        "Lf = 65536": lambda: full(lf=65536),
        "N = 0": lambda: full(n=0),
        "range past the window": lambda: ranged(3, 4),
        "range before the window": lambda: ranged(-1, 3),
        "n_frames = 0": lambda: ranged(2, 0),
        "phi_col before the range, with a phi_out": lambda: ranged(2, 3, phi_col=2 * seg - 1, phi_out=P),
        "phi_col past the range, with a phi_out": lambda: ranged(2, 3, phi_col=5 * seg, phi_out=P),
        "null amps": lambda: full(amps=None),
        "null f0": lambda: full(f0=None),
        "null wave": lambda: full(wave=None),
        "null workspace": lambda: full(ws=None),
    }
    for what, call in refusals.items():
        # the message is not cleared by a good call: put another entry's refusal there, so that the one read below is this call's
        assert L.alive_argmax_channels(None, 0, 0, 0, None, nat.stream()) < 0 and b"alive_oscillator" not in L.alive_last_error()
        rc = call()
        msg = L.alive_last_error().decode()
        assert rc < 0, f"{what}: accepted"
        assert "alive_oscillator" in msg, (what, msg)
        torch.cuda.synchronize()
        assert bool((wave == 7.0).all() and (phi_out == 7.0).all()), f"{what}: refused, but something was written"
    # the same calls are accepted once the argument is in range
    assert full(phi_col=lw - 1) == 0 and full(crop0=lw - 1, phi_out=None) == 0 and full(h=64, phi_out=None) == 0
    assert ranged(2, 3, phi_col=2 * seg, phi_out=P) == 0 and ranged(2, 3, phi_col=5 * seg - 1, phi_out=P) == 0
    assert ranged(2, 3, phi_col=0) == 0                                  # no phi_out: phi_col is not looked at
    torch.cuda.synchronize()
