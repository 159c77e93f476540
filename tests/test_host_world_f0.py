"""The float64 restatement of WORLD's DIO + StoneMask (tools/world_ref.py), the CPU reference of csrc/world_f0.hip: known f0
recovered, silence and noise left unvoiced, the shape quirks of the reference pinned, and the fixtures of tools/gen_world_golden.py
(the reference's own compute_f0 glue around the restatement) reproduced from the restatement + O.resample + torch's interpolation."""
import glob
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alive_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import world_ref as W   # noqa: E402

FS = 8000


def harmonic_tone(f0, seconds=1.5, fs=FS, harmonics=6, seed=0):
    rs = np.random.RandomState(seed)
    t = np.arange(int(seconds * fs)) / fs
    x = sum(0.3 / k * np.sin(2 * np.pi * k * f0 * t + rs.uniform(0, 6.28)) for k in range(1, harmonics + 1) if k * f0 < fs / 2)
    return x.astype(np.float32)


@pytest.mark.parametrize("f0", [80.0, 123.4, 200.0, 310.0, 450.0, 600.0])
def test_recovers_harmonic_tones_within_one_percent(f0):
    out = W.dio_stonemask_rows(harmonic_tone(f0)[None], FS)[0]
    inner = out[30:-30]                                    # frames at least 150 ms from either edge
    assert np.all(inner > 0)
    assert np.max(np.abs(inner / f0 - 1.0)) < 0.01


def test_silence_is_all_unvoiced():
    assert not np.any(W.dio_stonemask_rows(np.zeros((2, 12000), np.float32), FS))


def test_white_noise_is_mostly_unvoiced():
    x = (0.1 * np.random.RandomState(3).randn(2, 16000)).astype(np.float32)
    out = W.dio_stonemask_rows(x, FS)
    assert np.mean(out > 0) < 0.3


def test_fix_f0_contour_zeroes_the_21_frame_edges():
    """FixF0Contour at f0_floor 20 / 5 ms: voice range 21 frames; steps 1-2 zero the first and last 21 frames (and the 10 next
    to any gap); steps 3-4 only re-extend a section where some band's candidate continues it within 10 %"""
    F_ = 200
    best = np.full(F_, 150.0)
    none = [np.zeros(F_) for _ in range(16)]
    out = W.fix_f0_contour(best, none, 5.0, 20.0, 0.1)
    assert not np.any(out[:21]) and not np.any(out[-21:])
    assert np.all(out[32:F_ - 31] == 150.0) and not np.any(out[:32]) and not np.any(out[F_ - 31:])
    # with a band that tracks the contour everywhere, step 3 extends the section to the last frame and step 4 back to frame 1
    track = none[:1] + [np.full(F_, 150.0)] + none[2:]
    out = W.fix_f0_contour(best, track, 5.0, 20.0, 0.1)
    assert out[0] == 0.0 and np.all(out[1:] == 150.0)
    # no more frames than the voice range: untouched zeros
    assert not np.any(W.fix_f0_contour(np.full(21, 150.0), track, 5.0, 20.0, 0.1))


def test_stonemask_limits_40_hz_and_fs_over_12():
    x = harmonic_tone(200.0).astype(np.float64)
    t = 0.5
    assert W._refined(x, FS, t, 40.0) == 0.0 and W._refined(x, FS, t, 39.0) == 0.0
    assert W._refined(x, FS, t, 40.5) > 0.0
    assert W._refined(x, FS, t, FS / 12.0) > 0.0 and W._refined(x, FS, t, FS / 12.0 + 0.01) == 0.0


def test_short_ring_is_all_unvoiced():
    """-c 160 -b 16: a ring of 2560 samples at 16 kHz is 33 DIO frames at 8 kHz, all inside the zeroed edges"""
    ring = torch.from_numpy(harmonic_tone(150.0, seconds=0.16, fs=16000))[None]
    x8 = O.resample(ring, 16000, 8000).numpy()
    assert x8.shape[1] == 1280 and W.n_frames(1280, FS) == 33
    assert not np.any(W.dio_stonemask_rows(x8, FS))


def restated_compute_f0(wf16, x8=None):
    """reference compute_f0 composed from the restatement: resample, per-row DIO + StoneMask, two linear interpolations"""
    l = wf16.shape[1]
    if x8 is None:
        x8 = O.resample(torch.from_numpy(wf16), 16000, 8000).numpy()
    f0 = torch.from_numpy(W.dio_stonemask_rows(x8, FS))[:, None]
    f0 = F.interpolate(f0, x8.shape[1] // 256, mode="linear")
    return F.interpolate(f0, l // 320, mode="linear").numpy()


def test_fixtures_are_reproduced_from_the_restatement(golden_dir):
    files = sorted(glob.glob(os.path.join(golden_dir, "world_f0_*.npz")))
    assert len(files) == 4
    for path in files:
        z = np.load(path)
        got = restated_compute_f0(z["wf"])
        assert got.shape == z["f0"].shape == (z["wf"].shape[0], 1, z["wf"].shape[1] // 320), path
        assert np.array_equal(got, z["f0"]), path


def test_fixture_shapes_follow_the_reference_sizes(golden_dir):
    z = np.load(os.path.join(golden_dir, "world_f0_window.npz"))
    assert z["wf"].shape == (2, 144000) and z["f0"].shape == (2, 1, 450)
    assert W.n_frames(72000, FS) == 1801 and 72000 // 256 == 281
    z = np.load(os.path.join(golden_dir, "world_f0_ring.npz"))
    assert z["wf"].shape[1] == 7680 and z["f0"].shape[2] == 24 and W.n_frames(3840, FS) == 97 and 3840 // 256 == 15
    z = np.load(os.path.join(golden_dir, "world_f0_ring_short.npz"))
    assert not np.any(z["f0"])
    assert len(W.bands(20.0, 4096.0)) == 16
