"""CPU tests of voice blending: the blend spec (normalisation and every refusal), the converter's row limit, the "blend" key of
the jobs and sessions files, and the argument checks of alive_knn_blend_gather_rows (-1 with a message, nothing launched)."""
import json
import math
import os
import re
import sys

import numpy as np
import pytest

from module import _native as nat
from module import multistream as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alive-vc_amd"))
import batch_inference as BI                                         # noqa: E402
import multistream_inference as msi                                  # noqa: E402


class _Pool:
    """VoicePool's segment() over a name -> size table (no device)"""

    def __init__(self, sizes):
        self.sizes = sizes

    def segment(self, name):
        if name not in self.sizes:
            raise ValueError(f"unknown voice {name!r}")
        return 0, self.sizes[name]


POOL = _Pool({"a": 100, "b": 50, "c": 8, "d": 3000, "e": 10, "tiny": 3})


def test_blend_spec_normalises_in_the_callers_order():
    assert MS.blend_spec("a", POOL, 4) == (("a",), (1.0,))
    assert MS.blend_spec({"a": 3.7}, POOL, 4) == (("a",), (1.0,))                    # one voice: exactly 1.0
    names, w = MS.blend_spec({"b": 2, "a": 1}, POOL, 4)
    assert names == ("b", "a") and w == (2 / 3, 1 / 3)
    names, w = MS.blend_spec([("a", 0.1), ("b", 0.2), ("c", 0.3), ("d", 0.4)], POOL, 4)
    total = ((0.1 + 0.2) + 0.3) + 0.4                                                 # float64, left to right
    assert names == ("a", "b", "c", "d") and w == (0.1 / total, 0.2 / total, 0.3 / total, 0.4 / total)
    assert MS.blend_spec((("a", np.float32(2.0)), ("b", np.int64(2))), POOL, 4)[1] == (0.5, 0.5)
    assert MS.blend_spec([("x", 1), ("y", 3)])[1] == (0.25, 0.75)                      # without a pool: the weights alone


@pytest.mark.parametrize("voice,kw,msg", [
    ({}, {}, "at least one voice"),
    ([], {}, "at least one voice"),
    ({"a": 1, "b": 1}, dict(limit=1), "at most 1"),
    ({"a": 1, "b": 1, "c": 1}, dict(limit=2), "at most 2"),
    ([("a", 1), ("b", 1), ("c", 1), ("d", 1), ("e", 1)], {}, "at most 4"),
    ([("a", 1), ("b", 1), ("c", 1), ("d", 1), ("e", 1)], dict(limit=8), "at most 4"),
    ([("a", 1), ("a", 2)], {}, "twice"),
    ({"nobody": 1}, {}, "unknown voice"),
    ({"a": 1, "tiny": 1}, {}, "fewer than k=4"),
    ("tiny", {}, "fewer than k=4"),
    ({"a": 0}, {}, "> 0"),
    ({"a": -1.0}, {}, "> 0"),
    ({"a": 1, "b": float("nan")}, {}, "finite"),
    ({"a": float("inf")}, {}, "finite"),
    ({"a": True}, {}, "number"),
    ({"a": np.bool_(True)}, {}, "number"),
    ({"a": "1"}, {}, "number"),
    ([("a", 1, 2)], {}, "pair"),
    (["a"], {}, "pair"),
    (3, {}, "a name"),
])
def test_blend_spec_refusals(voice, kw, msg):
    with pytest.raises(ValueError, match=re.escape(msg)):
        MS.blend_spec(voice, POOL, 4, **kw)


def test_converter_refuses_more_list_rows_than_the_grouped_search_takes():
    for slots, blend in ((257, 4), (342, 3), (513, 2)):
        with pytest.raises(ValueError, match="slots \\* blend"):
            MS.MultiStreamConverter(None, None, None, None, slots, blend=blend)        # (before any allocation: no device)
    for bad in (0, 5, True, 2.0):
        with pytest.raises(ValueError, match="blend="):
            MS.MultiStreamConverter(None, None, None, None, 4, blend=bad)


def test_blend_gather_abi_refuses_bad_arguments():
    L = nat.lib()

    def call(**kw):
        a = dict(val=1, idx=1, k=4, first=1, weight=1, alpha=1, rows=1, src=1, N=2, T=8, out=1)
        a.update(kw)
        return L.alive_knn_blend_gather_rows(a["val"], a["idx"], a["k"], a["first"], a["weight"], a["alpha"], a["rows"], a["src"],
                                             a["N"], a["T"], a["out"], None)
    for kw, msg in [(dict(val=None), b"null"), (dict(first=None), b"null"), (dict(weight=None), b"null"), (dict(alpha=None), b"null"),
                    (dict(out=None), b"null"), (dict(k=0), b"k=0"), (dict(k=9), b"k=9"), (dict(N=0), b"N=0"), (dict(T=0), b"T=0")]:
        assert call(**kw) == -1, kw
        assert msg in L.alive_last_error(), (kw, L.alive_last_error())


def test_header_and_prototypes_agree():
    hdr = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    assert "#define ALIVE_MAX_BLEND 4" in hdr and MS.MAX_BLEND == 4
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(alive_[a-z0-9_]+)\s*\(", hdr))
    assert "alive_knn_blend_gather_rows" in declared
    assert declared == set(nat.PROTOTYPES), declared ^ set(nat.PROTOTYPES)
    decl = re.search(r"int alive_knn_blend_gather_rows\((.*?)\);", hdr, flags=re.S).group(1)
    assert len(decl.split(",")) == len(nat.PROTOTYPES["alive_knn_blend_gather_rows"][1]) == 12


# ---------------------------------------------------------------------------------------------------- jobs and sessions files
@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "b.wav", "spk.wav", "spk2.wav", "voice_library.pt", "lib2.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def _write(d, entries, name="f.json"):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_jobs_file_blend_paths_and_shared_voices(files):
    jobs = BI.load_jobs(_write(files, [
        {"input": "a.wav", "blend": [{"target": "spk.wav", "weight": 2}, {"lib": "voice_library.pt", "weight": 1},
                                     {"target": "spk2.wav", "lib": str(files / "lib2.pt"), "weight": 0.5}]},
        {"input": "b.wav", "lib": "voice_library.pt"},
        {"input": "b.wav", "target": "spk.wav"}]))
    a, b, c = jobs
    assert a["target"] is None and a["lib"] is None
    assert a["blend"] == [(str(files / "spk.wav"), None, 2), (None, str(files / "voice_library.pt"), 1),
                          (str(files / "spk2.wav"), str(files / "lib2.pt"), 0.5)]
    assert b["blend"] is None
    # the components and the plain jobs with the same sources share one voice of the pool
    keys = BI.voice_keys(a)
    assert keys[0] == BI.voice_key(c) and keys[1] == BI.voice_key(b) and len(set(keys)) == 3
    names = {k: f"voice{i}" for i, k in enumerate(dict.fromkeys(k for j in jobs for k in BI.voice_keys(j)))}
    assert len(names) == 3
    assert BI.job_voice(a, names) == [("voice0", 2), ("voice1", 1), ("voice2", 0.5)]
    assert BI.job_voice(b, names) == "voice1" and BI.job_voice(c, names) == "voice0"


@pytest.mark.parametrize("job,msg", [
    ({"input": "a.wav", "target": "spk.wav", "blend": [{"lib": "voice_library.pt", "weight": 1}]}, "excludes"),
    ({"input": "a.wav", "lib": "voice_library.pt", "blend": [{"target": "spk.wav", "weight": 1}]}, "excludes"),
    ({"input": "a.wav", "blend": [{"target": "spk.wav"}]}, "no \"weight\""),
    ({"input": "a.wav", "blend": [{"weight": 1}]}, "needs a \"target\""),
    ({"input": "a.wav", "blend": []}, "non-empty list"),
    ({"input": "a.wav", "blend": {"target": "spk.wav", "weight": 1}}, "non-empty list"),
    ({"input": "a.wav", "blend": ["spk.wav"]}, "must be an object"),
    ({"input": "a.wav", "blend": [{"target": "spk.wav", "weight": 1, "k": 3}]}, "unknown keys"),
    ({"input": "a.wav", "blend": [{"target": "spk.wav", "weight": 0}]}, "> 0"),
    ({"input": "a.wav", "blend": [{"target": "spk.wav", "weight": True}]}, "number"),
    ({"input": "a.wav", "blend": [{"target": "spk.wav", "weight": 1}, {"target": "spk.wav", "weight": 2}]}, "twice"),
    ({"input": "a.wav", "blend": [{"target": "s{}.wav".format(i), "weight": 1} for i in range(5)]}, "at most 4"),
    ({"input": "a.wav", "blend": [{"target": "missing.wav", "weight": 1}]}, "does not exist"),
])
def test_jobs_file_blend_errors(files, job, msg):
    with pytest.raises(ValueError, match=re.escape(msg)):
        BI.load_jobs(_write(files, [job]))


def test_sessions_file_blend(files):
    ss = msi.load_sessions(_write(files, [
        {"input": "a.wav", "blend": [{"target": "spk.wav", "weight": 3}, {"lib": "/abs/l.pt", "weight": 1}], "alpha": 0.3},
        {"input": "b.wav", "target": "spk.wav"}]))
    a, b = ss
    assert a["blend"] == [(str(files / "spk.wav"), None, 3), (None, "/abs/l.pt", 1)] and a["alpha"] == 0.3
    assert b["blend"] is None
    assert msi.session_voice(a) == [(msi.voice_name(str(files / "spk.wav"), None), 3), (msi.voice_name(None, "/abs/l.pt"), 1)]
    assert msi.session_voice(b) == msi.voice_name(str(files / "spk.wav"), None) == msi.session_voice(a)[0][0]
    assert msi.blend_size(ss) == 2 and msi.blend_size([b]) == 1
    for bad, msg in (({"input": "a.wav", "lib": "l.pt", "blend": [{"target": "t.wav", "weight": 1}]}, "excludes"),
                     ({"input": "a.wav", "blend": [{"target": "t.wav"}]}, "no \"weight\""),
                     ({"input": "a.wav", "blend": [{"weight": 2}]}, "needs a \"target\""),
                     ({"input": "a.wav", "blend": [{"lib": "l.pt", "weight": math.inf}]}, "finite"),
                     ({"input": "a.wav"}, "target")):
        with pytest.raises(ValueError, match=re.escape(msg)):
            msi.load_sessions(_write(files, [bad], "bad.json"))
