"""The voicing decision without a GPU: the NumPy restatement (tools/voicing_ref.py) on the signals it is meant to separate, every branch
of the per-row decision on hand-built sequences, the option checks of module.common.voicing_options, the flags of the four CLIs with
their refusals (a bad value, -vd together with -wpe), and the jobs and sessions file readers with and without the new keys."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import voicing_ref as VR                                             # noqa: E402
from module import common, synthetic                                 # noqa: E402

T = 100


def _noise(n, seed=0):
    return (0.1 * np.random.default_rng(seed).standard_normal(n)).astype(np.float32)


def test_the_defaults_of_the_restatement_and_of_the_options_are_the_same():
    o = common.voicing_options(True)
    assert {k: o[k] for k in common.VOICING_KEYS} == VR.DEFAULTS
    assert (o["lag_lo"], o["lag_hi"]) == VR.lags() == (32, 320) and o["W"] == VR.window() == 640
    assert o["floor_e"] == VR.floor_e() == common.voicing_floor_e(-60.0) == 10.0 ** -6.0 * 320 * 2.0 ** 30
    assert (common.VOICING_MAX_WINDOW, common.VOICING_MAX_LAG) == (VR.MAX_WINDOW, VR.MAX_LAG)
    header = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    assert f"#define ALIVE_VOICING_MAX_WINDOW {VR.MAX_WINDOW}\n" in header and f"#define ALIVE_VOICING_MAX_LAG {VR.MAX_LAG}\n" in header
    assert common.voicing_options(None) is None and common.voicing_options(False) is None


def test_voiced_speech_is_voiced_noise_and_silence_are_not():
    x = synthetic.make_voiced(32000, 3)[0][0].numpy()
    r, lag, silent = VR.scores(x, T)
    assert r.min() > 0.69 and not silent.any() and VR.decide(r, silent).all()
    assert np.all((lag >= 32) & (lag <= 320))
    r, lag, silent = VR.scores(synthetic.make_waveform(32000, 2)[0].numpy(), T)
    assert r.min() > 0.7 and VR.decide(r, silent).all()
    r, lag, silent = VR.scores(_noise(32000), T)
    assert r.max() < 0.2 and not silent.any() and not VR.decide(r, silent).any()
    r, lag, silent = VR.scores(np.zeros(32000, np.float32), T)       # the 0 / 0 guard
    assert np.all(r == 0.0) and np.all(lag == 32) and silent.all() and not VR.decide(r, silent).any()
    out = VR.voicing_rows(np.stack([x, _noise(32000)]), np.full((2, T), 120.0, np.float32))
    assert np.all(out["f0"][0] == 120.0) and np.all(out["f0"][1] == 0.0) and out["changed"].tolist() == [0, T]
    assert np.all(np.signbit(out["f0"][1]) == False)                 # noqa: E712  (+0.0)


def test_the_voiced_runs_of_an_alternating_signal_lie_within_a_frame_of_the_segment_edges():
    n = 32000                                                        # 200 ms = 10 frames of voiced speech, then of noise, in turn
    x = np.where((np.arange(n) // 3200) % 2 == 0, synthetic.make_voiced(n, 3)[0][0].numpy(), _noise(n, 3)).astype(np.float32)
    r, lag, silent = VR.scores(x, T)
    v = VR.decide(r, silent)
    starts = np.flatnonzero(np.diff(np.concatenate([[0], v.astype(int)])) == 1)
    ends = np.flatnonzero(np.diff(np.concatenate([v.astype(int), [0]])) == -1) + 1
    assert len(starts) == 5 == len(ends)
    for k, (a, b) in enumerate(zip(starts, ends)):
        assert abs(a - 20 * k) <= 1 and abs(b - (20 * k + 10)) <= 1, (k, a, b)


def test_quantisation_clamps_zero_extends_and_maps_nan_to_zero():
    x = np.array([1.5, -1.5, np.nan, np.inf, -np.inf, 0.5 / 32768, 1.5 / 32768, 2.5 / 32768, 1.0, -1.0, 0.25], dtype=np.float32)
    assert VR.quantise(x).tolist() == [32767, -32768, 0, 32767, -32768, 0, 2, 2, 32767, -32768, 8192]       # (ties to even)
    assert VR.quantise(x, 3).tolist() == [32767, -32768] + [0] * 9
    # frames may reach past the row: a row of 100 samples, shorter than W, scores as its zero extension
    short = synthetic.make_voiced(100, 3)[0][0].numpy()
    a = VR.scores(short, 2)
    b = VR.scores(np.concatenate([short, np.zeros(2000, np.float32)]), 2)
    assert all(np.array_equal(p, q) for p, q in zip(a, b))
    c = VR.scores(synthetic.make_voiced(2100, 3)[0][0].numpy(), 2, length=100)
    assert all(np.array_equal(p, q) for p, q in zip(a, c))


def test_the_largest_sums_stay_exact():
    """a full-scale square wave at the longest window: Sxx = 4096 * 2^30 = 2^42, and r of a period is exactly 1 or a hair under it"""
    x = np.where((np.arange(12000) // 40) % 2 == 0, 1.0, -1.0).astype(np.float32)
    r, lag, silent = VR.scores(x, 20, W=4096, lag_lo=20, lag_hi=700)
    assert np.all(lag[7:] == 80) and np.all(r[7:] > 0.9999) and np.all(r <= 1.0)


def _decide(r, silent=None, **kw):
    r = np.asarray(r, dtype=np.float64)
    silent = np.zeros(len(r), bool) if silent is None else np.asarray(silent, bool)
    return VR.decide(r, silent, **kw).astype(int).tolist()


def test_every_branch_of_the_row_decision():
    hi, mid, lo = 0.9, 0.5, 0.1                                      # over `on`, between the two, under `off`
    # hysteresis: the band between off and on keeps the state, whichever it is
    assert _decide([lo, mid, hi, mid, mid, lo, mid], bridge=0, min_run=0) == [0, 0, 1, 1, 1, 0, 0]
    assert _decide([0.6, 0.45, 0.4499], bridge=0, min_run=0) == [1, 1, 0]                  # >= on turns on, < off turns off
    # a silent frame clears the state whatever r is, and the band after it stays unvoiced
    assert _decide([hi, hi, mid, mid], [0, 1, 0, 0], bridge=0, min_run=0) == [1, 0, 0, 0]
    # a one-frame dip is bridged; a silent one is not; two frames are too long for bridge = 1 and fit bridge = 2
    assert _decide([hi, hi, lo, hi, hi]) == [1, 1, 1, 1, 1]
    assert _decide([hi, hi, hi, hi, hi], [0, 0, 1, 0, 0]) == [1, 1, 0, 1, 1]
    assert _decide([hi, hi, lo, lo, hi, hi]) == [1, 1, 0, 0, 1, 1]
    assert _decide([hi, hi, lo, lo, hi, hi], bridge=2) == [1, 1, 1, 1, 1, 1]
    assert _decide([hi, hi, lo, lo, hi, hi], [0, 0, 0, 1, 0, 0], bridge=2) == [1, 1, 0, 0, 1, 1]
    # an unvoiced run at either end of the row has no voiced frame on one side: not bridged
    assert _decide([lo, hi, hi, hi, lo]) == [0, 1, 1, 1, 0]
    # a one-frame blip inside the row is removed; at either end of the row it stays
    assert _decide([lo, lo, hi, lo, lo]) == [0, 0, 0, 0, 0]
    assert _decide([hi, lo, lo, lo, hi]) == [1, 0, 0, 0, 1]
    assert _decide([lo, lo, hi, hi, lo, lo]) == [0, 0, 1, 1, 0, 0]                         # min_run frames are enough
    assert _decide([lo, lo, hi, hi, lo, lo], min_run=3) == [0, 0, 0, 0, 0, 0]
    # the bridge runs first: two blips around a dip form a run of three, which stays
    assert _decide([lo, hi, lo, hi, lo, lo]) == [0, 1, 1, 1, 0, 0]
    # ... and runs are taken before any of them changes: removing a blip does not make the gaps around it one gap
    assert _decide([hi, hi, lo, lo, hi, lo, lo, hi, hi], bridge=1, min_run=2) == [1, 1, 0, 0, 0, 0, 0, 1, 1]
    assert _decide([]) == [] and _decide([hi]) == [1] and _decide([mid]) == [0]


@pytest.mark.parametrize("bad,names", [
    (dict(on=0.3), ("off 0.45", "on 0.3")), (dict(off=0.0), ("off 0.0",)), (dict(on=1.5), ("on 1.5",)), (dict(off=-0.1), ("off -0.1",)),
    (dict(lo=0), ("lo 0",)), (dict(lo=600), ("lo 600", "hi 500")), (dict(hi=4001), ("hi 4001",)), (dict(lo=5), ("lo 5 Hz", "1600")),
    (dict(lo=3999.5, hi=3999.9), ("lo 3999.5", "hi 3999.9")), (dict(window_ms=300), ("window_ms 300", "4800", "4096")),
    (dict(window_ms=0), ("window_ms 0",)), (dict(bridge=-1), ("bridge", "-1")), (dict(min_run=1.5), ("min_run", "1.5")),
    (dict(on=float("nan")), ("on", "nan")), (dict(floor_db="x"), ("floor_db", "'x'")), (dict(on=True), ("on", "True")),
    (dict(band=2), ("unknown keys", "band")), ("yes", ("'yes'",)), (3, ("got 3",))])
def test_voicing_options_refuses_a_bad_value_and_names_it(bad, names):
    with pytest.raises(ValueError) as e:
        common.voicing_options(bad, "utterance 2")
    assert str(e.value).startswith("utterance 2: voicing") and all(n in str(e.value) for n in names), str(e.value)


def test_voicing_options_fills_in_and_derives_the_kernels_integers():
    o = common.voicing_options(dict(lo=62.5, hi=400, window_ms=25, on=0.8, off=0.8, floor_db=-50, bridge=0, min_run=0))
    assert (o["lag_lo"], o["lag_hi"], o["W"]) == (40, 256, 400) and o["floor_e"] == VR.floor_e(-50)
    assert common.voicing_options(dict(lo=3999, hi=4000))["lag_lo"] == 4 == common.voicing_options(dict(lo=3999, hi=4000))["lag_hi"]
    assert common.voicing_options(dict(lo=10))["lag_hi"] == 1600 and common.voicing_options(dict(window_ms=256))["W"] == 4096


def test_inference_parser_takes_the_flags_and_leaves_the_defaults_alone():
    import inference as INF
    a = INF.build_parser().parse_args([])
    assert a.voicing is False and common.voicing_arguments(a) is None
    assert (a.voicing_on, a.voicing_off, a.voicing_floor, a.voicing_lo, a.voicing_hi) == (0.6, 0.45, -60.0, 50, 500)
    a = INF.build_parser().parse_args(["-vd", "--voicing-on", "0.7", "--voicing-off", "0.5", "--voicing-floor", "-50", "--voicing-lo", "60",
                                       "--voicing-hi", "400"])
    o = common.voicing_arguments(a)
    assert (o["on"], o["off"], o["floor_db"], o["lo"], o["hi"], o["lag_lo"], o["lag_hi"]) == (0.7, 0.5, -50.0, 60.0, 400.0, 40, 266)
    with pytest.raises(ValueError, match="-vd: voicing: needs 0 < off <= on <= 1"):      # a bad value is refused even without -vd
        common.voicing_arguments(INF.build_parser().parse_args(["--voicing-off", "0.9"]))
    for argv, msg in ((["-vd", "-wpe", "True"], "-vd cannot be combined with -wpe"), (["-vd", "--voicing-lo", "900"], "lo 900.0, hi 500"),
                      (["--voicing-on", "0.2"], "needs 0 < off <= on <= 1, got off 0.45, on 0.2")):
        with pytest.raises(SystemExit, match=msg):
            INF.main(argv)


def _write(tmp_path, name, entries):
    import json
    for f in ("in.wav", "lib.pt"):
        (tmp_path / f).write_bytes(b"")
    (tmp_path / name).write_text(json.dumps(entries))
    return str(tmp_path / name)


def test_the_jobs_file_reader_takes_the_key_and_a_file_without_it_loads_to_what_it_did(tmp_path):
    import batch_inference as BI
    job = dict(input="in.wav", lib="lib.pt")
    plain = BI.load_jobs(_write(tmp_path, "plain.json", [job, dict(job, pitch=2.0)]))
    assert all("voicing" not in j for j in plain)
    assert set(plain[0]) == {"input", "target", "lib", "output", "pitch", "intonation", "f0_rate", "alpha", "gain", "normalize",
                             "world_pitch", "blend", "k", "auto_pitch", "register_hz"}
    path = _write(tmp_path, "jobs.json", [job, dict(job, voicing=True), dict(job, voicing={"on": 0.8, "floor_db": -40}),
                                          dict(job, voicing=False)])
    jobs = BI.load_jobs(path)
    assert [j.get("voicing") for j in jobs] == [None, dict(on=0.6, off=0.45, floor_db=-60.0), dict(on=0.8, off=0.45, floor_db=-40.0), None]
    assert {k: v for k, v in jobs[1].items() if k != "voicing"} == plain[0]
    jobs = BI.load_jobs(path, voicing=True, voicing_on=0.7, voicing_off=0.5, voicing_floor_db=-50.0)     # -vd and its defaults
    assert [j.get("voicing") for j in jobs] == [dict(on=0.7, off=0.5, floor_db=-50.0)] * 2 + [dict(on=0.8, off=0.5, floor_db=-40.0), None]
    for bad, msg in ((dict(job, voicing=1), "job 0: \"voicing\" must be true, false or an object"),
                     (dict(job, voicing={"lo": 60}), "job 0: \"voicing\": unknown keys \\['lo'\\]"),
                     (dict(job, voicing={"on": 0.2}), "job 0: voicing: needs 0 < off <= on <= 1, got off 0.45, on 0.2"),
                     (dict(job, voicing=True, world_pitch=True), "job 0: \"voicing\" cannot be combined with \"world_pitch\"")):
        with pytest.raises(ValueError, match=msg):
            BI.load_jobs(_write(tmp_path, "bad.json", [bad]))
    with pytest.raises(ValueError, match="-vd / --voicing-on / --voicing-off / --voicing-floor: voicing: needs 0 < off <= on <= 1"):
        BI.load_jobs(path, voicing_off=0.9)
    a = BI.build_parser().parse_args([path, "-vd", "--voicing-lo", "60"])
    assert a.voicing is True and a.voicing_lo == 60.0 and BI.build_parser().parse_args([path]).voicing is False


def test_the_sessions_file_reader_takes_the_keys_and_a_file_without_them_loads_to_what_it_did(tmp_path):
    import multistream_inference as msi
    sess = dict(input="in.wav", lib="lib.pt")
    plain = msi.load_sessions(_write(tmp_path, "plain.json", [sess]))
    assert not set(plain[0]) & set(msi.VOICING_KEYS)
    assert set(plain[0]) == {"input", "target", "lib", "output", "pitch", "f0_rate", "alpha", "gain", "input_gain", "start", "sr",
                             "world_pitch", "blend", "k", "auto_pitch", "register_hz"}
    path = _write(tmp_path, "sessions.json", [sess, dict(sess, voicing=True, voicing_on=0.8), dict(sess, voicing=False, voicing_on=0.9)])
    ss = msi.load_sessions(path)
    assert [tuple(s.get(k) for k in msi.VOICING_KEYS) for s in ss] == [(None,) * 4, (True, 0.8, 0.45, -60.0), (None,) * 4]
    assert {k: v for k, v in ss[1].items() if k not in msi.VOICING_KEYS} == plain[0]
    ss = msi.load_sessions(path, voicing=True, voicing_off=0.5, voicing_floor_db=-50.0)                 # -vd and its defaults
    assert [tuple(s.get(k) for k in msi.VOICING_KEYS) for s in ss] == [(True, 0.6, 0.5, -50.0), (True, 0.8, 0.5, -50.0), (None,) * 4]
    for bad, msg in ((dict(sess, voicing=1), "session 0: \"voicing\" must be true or false"),
                     (dict(sess, voicing_on=0.2), "session 0: voicing: needs 0 < off <= on <= 1"),
                     (dict(sess, voicing_lo=60), "session 0: unknown keys"),
                     (dict(sess, voicing=True, world_pitch=True), "session 0: \"voicing\" cannot be combined with \"world_pitch\"")):
        with pytest.raises(ValueError, match=msg):
            msi.load_sessions(_write(tmp_path, "bad.json", [bad]))
    a = msi.build_parser().parse_args([path, "-vd", "--voicing-hi", "400"])
    assert a.voicing is True and a.voicing_hi == 400.0 and msi.build_parser().parse_args([path]).voicing is False


def test_realtime_parser_takes_the_flags():
    import realtime_inference as RT
    a = RT.build_parser().parse_args(["-vd", "--voicing-floor", "-45"])
    assert a.voicing is True and common.voicing_arguments(a)["floor_db"] == -45.0
    assert common.voicing_arguments(RT.build_parser().parse_args([])) is None
    # refused before the device is looked for: together with -wpe, and a bad value even without -vd
    for argv, msg in ((["-vd", "-wpe", "True"], "-vd cannot be combined with -wpe: WORLD makes its own voicing decision"),
                      (["-vd", "--voicing-on", "0.2"], "-vd: voicing: needs 0 < off <= on <= 1, got off 0.45, on 0.2"),
                      (["--voicing-hi", "30"], "needs 0 < lo < hi <= 4000")):
        with pytest.raises(SystemExit, match=msg):
            RT.main(argv)
