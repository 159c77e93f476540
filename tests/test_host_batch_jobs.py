"""CPU tests of the many-to-many batch surface: batch_inference.py's jobs file (parsing, defaults, every validation error, before
anything runs on a device) and the pool search's C ABI (workspace query monotone in every dimension, out-of-range arguments refused
with a message, nothing launched)."""
import json
import os
import sys

import pytest

from module import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alive-vc_amd"))
import batch_inference as BI                                         # noqa: E402


@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "b.wav", "spk.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, jobs):
    p = d / "jobs.json"
    p.write_text(json.dumps(jobs))
    return str(p)


def test_jobs_file_defaults_and_relative_paths(files):
    jobs = BI.load_jobs(write(files, [{"input": "a.wav", "lib": "voice_library.pt"},
                                      {"input": "b.wav", "target": "spk.wav", "lib": "voice_library.pt", "pitch": 2, "intonation": 0.5,
                                       "f0_rate": 0.75, "alpha": 0.2, "gain": 3, "normalize": True, "output": "o.wav"}]))
    a, b = jobs
    assert a["input"] == str(files / "a.wav") and a["target"] is None and a["lib"] == str(files / "voice_library.pt")
    assert (a["pitch"], a["intonation"], a["f0_rate"], a["alpha"], a["gain"], a["normalize"], a["output"]) == (0.0, 1.0, 1.0, 0.0, 1.0, False, None)
    assert (b["pitch"], b["intonation"], b["f0_rate"], b["alpha"], b["gain"], b["normalize"]) == (2.0, 0.5, 0.75, 0.2, 3.0, True)
    assert b["output"] == str(files / "o.wav")
    assert BI.voice_key(a) != BI.voice_key(b)
    assert BI.voice_key(a) == BI.voice_key(BI.load_jobs(write(files, [{"input": "b.wav", "lib": "voice_library.pt"}]))[0])


@pytest.mark.parametrize("jobs,msg", [
    ([], "non-empty"),
    ({"input": "a.wav"}, "non-empty"),
    ([{"target": "spk.wav"}], "\"input\""),
    ([{"input": "a.wav", "lib": "voice_library.pt", "pitchh": 1}], "unknown keys"),
    ([{"input": "a.wav"}], "needs a \"target\""),
    ([{"input": "missing.wav", "lib": "voice_library.pt"}], "does not exist"),
    ([{"input": "a.wav", "target": "nobody.wav"}], "does not exist"),
])
def test_jobs_file_errors(files, jobs, msg):
    with pytest.raises(ValueError, match=msg):
        BI.load_jobs(write(files, jobs))


def test_jobs_k_and_short_voices(files):
    path = write(files, [{"input": "a.wav", "lib": "voice_library.pt"}])
    with pytest.raises(ValueError, match="k=9"):
        BI.load_jobs(path, k=9)
    BI.check_voice_sizes({("t", None): 4}, 4)
    with pytest.raises(ValueError, match="fewer than k=4"):
        BI.check_voice_sizes({("t", None): 3, (None, "l"): 900}, 4)


def test_pool_workspace_query_is_monotone_and_refuses_out_of_range():
    L = nat.lib()
    ws = L.alive_knn_pool_workspace_bytes
    base = ws(64, 450, 4, 8, 400_000, 50_000)
    assert base > 64 * 450 * 768 * 6
    assert ws(128, 450, 4, 8, 400_000, 50_000) > base
    assert ws(64, 451, 4, 8, 400_000, 50_000) >= base
    assert ws(64, 450, 8, 8, 400_000, 50_000) >= base                 # more partial lists per frame at larger k
    assert ws(64, 450, 4, 64, 400_000, 50_000) >= base                # more voices: more partial frame blocks
    assert ws(4096, 256, 4, 300, 2 ** 31 - 1, 200_000) > 0            # the documented limits
    for args in [(0, 450, 4, 8, 1000, 100), (4097, 1, 4, 8, 1000, 100), (1024, 1025, 4, 8, 1000, 100), (64, 450, 0, 8, 1000, 100),
                 (64, 450, 9, 8, 1000, 100), (64, 450, 4, 0, 1000, 100), (64, 450, 4, 8, 2 ** 31, 100), (64, 450, 4, 8, 1000, 1001),
                 (64, 450, 4, 8, 1000, 0)]:
        assert ws(*args) == 0, args


def test_pool_search_abi_refuses_bad_arguments():
    L = nat.lib()
    ok = dict(src=1, N=4, T=8, images=1, img_off=1, rows=1, norms=1, bounds=1, P=1000, lo=1, ln=1, V=2, max_len=600, voice=1, k=4,
              val=1, idx=1, ws=1)

    def call(**kw):
        a = dict(ok, **kw)
        return L.alive_knn_search_pool(a["src"], a["N"], a["T"], a["images"], a["img_off"], a["rows"], a["norms"], a["bounds"], a["P"],
                                       a["lo"], a["ln"], a["V"], a["max_len"], a["voice"], a["k"], a["val"], a["idx"], a["ws"], None)
    for kw, msg in [(dict(src=None), b"null"), (dict(voice=None), b"null"), (dict(bounds=None), b"null"), (dict(k=9), b"k=9"),
                    (dict(k=0), b"k=0"), (dict(N=0), b"N=0"), (dict(N=4097), b"N=4097"), (dict(T=1 << 19), b"N*T"),
                    (dict(V=0), b"V=0"), (dict(P=2 ** 31), b"pool of"), (dict(max_len=1001), b"longest voice")]:
        assert call(**kw) == -1, kw
        assert msg in L.alive_last_error(), (kw, L.alive_last_error())


def test_pool_image_bytes_host_query():
    import numpy as np
    L = nat.lib()
    ln = np.array([5, 128, 129], dtype=np.int32)
    off = np.zeros(3, dtype=np.int64)
    assert L.alive_pool_image_bytes(ln.ctypes.data, 3, off.ctypes.data) == (128 + 128 + 256) * 768 * 2
    assert off.tolist() == [0, 128, 256]
    bad = np.array([5, 0], dtype=np.int32)
    assert L.alive_pool_image_bytes(bad.ctypes.data, 2, None) == 0
