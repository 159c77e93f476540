"""CPU tests of per-session sample rates in multi-session streaming: the argument checks of alive_resample_rows_multi (bad
arguments return -1 with a message and launch nothing), the session geometry arithmetic, and the converter / CLI refusals that
happen before anything touches a device."""
import json

import pytest

from module import _native as nat
from module import multistream as MS


def _call(**over):
    a = dict(x=1, B=4, ld_in=7056, len_in=1, pair=1, table=1, n_pairs=2, filt=1, filt_len=100, lds_bytes=0, pre=1, post=1, y=1,
             ld_out=7056, len_out=1, stream=None)
    a.update(over)
    return nat.lib().alive_resample_rows_multi(*a.values())


def test_multi_rate_resampler_refuses_bad_arguments():
    """null pointers, B outside [1, 1024], an empty pair table, non-positive strides, a bad filter buffer or LDS size: -1"""
    L = nat.lib()
    for name in ("x", "len_in", "pair", "table", "pre", "post", "y", "len_out"):
        assert _call(**{name: None}) == -1, name
        assert b"null" in L.alive_last_error(), name
    for b in (0, -1, 1025):
        assert _call(B=b) == -1 and b"B=%d" % b in L.alive_last_error()
    assert _call(n_pairs=0) == -1 and b"empty pair table" in L.alive_last_error()
    assert _call(ld_in=0) == -1 and b"ld_in=0" in L.alive_last_error()
    assert _call(ld_out=0) == -1 and b"ld_out=0" in L.alive_last_error()
    assert _call(ld_in=-5) == -1 and _call(ld_out=-5) == -1
    assert _call(filt=None) == -1 and b"null filter" in L.alive_last_error()
    assert _call(filt_len=-1) == -1
    assert _call(lds_bytes=16 * 1024 + 4) == -1 and b"lds_bytes" in L.alive_last_error()
    assert _call(lds_bytes=-4) == -1


def test_session_geometry_accepts_and_refuses_rates():
    """a session's chunk is chunk * rate / sr and must be whole; its 16 kHz geometry is then the converter's"""
    for r, c in ((8000, 80), (16000, 160), (24000, 240), (44100, 441), (48000, 480), (32000, 320), (96000, 960)):
        assert MS.session_geometry(160, 16, 16000, r) == c
    assert MS.session_geometry(960, 8, 16000, 22050) == 1323
    assert MS.session_geometry(960, 8, 16000, 44100) == 2646
    assert MS.session_geometry(480, 12, 24000, 8000) == 160
    with pytest.raises(ValueError, match="220.5 samples"):
        MS.session_geometry(160, 16, 16000, 22050)
    with pytest.raises(ValueError, match="not a whole number"):
        MS.session_geometry(960, 8, 16000, 11025)
    with pytest.raises(ValueError, match="> 0"):
        MS.session_geometry(160, 16, 16000, 0)
    # the three quantities, each from its own formula (realtime_inference.py:122-126 at the session's rate)
    for r in (8000, 44100, 48000):
        c = MS.session_geometry(160, 16, 16000, r)
        assert MS._geometry(c, 16, r) == MS._geometry(160, 16, 16000) == (2560, 8, 160)


def test_rates_need_equal_input_and_output_rates():
    with pytest.raises(ValueError, match="input_sr == output_sr"):
        MS.MultiStreamConverter(None, None, None, None, 4, chunk=160, buffersize=16, input_sr=16000, output_sr=24000,
                                rates=[16000, 48000])
    with pytest.raises(ValueError, match="220.5"):
        MS.MultiStreamConverter(None, None, None, None, 4, chunk=160, buffersize=16, rates=[22050])


def test_sessions_file_takes_a_rate(tmp_path):
    import multistream_inference as msi
    p = tmp_path / "s.json"
    json.dump([{"input": "a.wav", "lib": "l.pt", "sr": 48000}, {"input": "b.wav", "lib": "l.pt"}], open(p, "w"))
    a, b = msi.load_sessions(str(p))
    assert a["sr"] == 48000 and b["sr"] is None
    json.dump([{"input": "a.wav", "lib": "l.pt", "sr": 0}], open(p, "w"))
    with pytest.raises(ValueError, match="sample rate"):
        msi.load_sessions(str(p))
    json.dump([{"input": "a.wav", "lib": "l.pt", "sr": 48000}], open(p, "w"))
    with pytest.raises(SystemExit, match="-isr == -osr"):
        msi.main(["-isr", "16000", "-osr", "24000", str(p)])
