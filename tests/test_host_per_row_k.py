"""CPU tests of the per-session / per-utterance k of the batched paths: the per-row-k entry points are exported, declared and
refuse bad arguments before they launch anything; the jobs and sessions files take "k" as an integer in 1..8; the converter's
open / set rules (k needs k_max, k <= k_max, every voice at least as long as the session's own k); the multistream CLI's k_max."""
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

from module import _native as nat
from module import multistream as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alive-vc_amd"))
import batch_inference as BI                                         # noqa: E402
import multistream_inference as MSI                                  # noqa: E402

NEW = {"alive_knn_grouped_k_workspace_bytes": 3, "alive_knn_search_grouped_k": 14, "alive_knn_merge_gather_rows_k": 12,
       "alive_knn_blend_gather_rows_k": 13, "alive_knn_pool_k_workspace_bytes": 6, "alive_knn_search_pool_k": 20}


# ---------------------------------------------------------------------------------------------------- the C ABI
def test_library_exports_and_header_declares_every_new_entry_point():
    L = nat.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    for name, nargs in NEW.items():
        assert hasattr(L, name), name
        assert name in nat.PROTOTYPES and len(nat.PROTOTYPES[name][1]) == nargs, name
        decl = re.search(r"\b%s\((.*?)\);" % name, hdr, flags=re.S)
        assert decl is not None, f"{name} is not declared in alive_vc.h"
        assert len(decl.group(1).split(",")) == nargs, name
        assert "k_max" in decl.group(1), name


def test_workspace_queries_follow_k_max_alone():
    L = nat.lib()
    # the grouped form: the workspace of the uniform search at k = k_max (sized from N, T and k_max alone)
    for n, t, k in ((1, 1, 1), (16, 8, 4), (1024, 5, 8), (64, 450, 3)):
        assert L.alive_knn_grouped_k_workspace_bytes(n, t, k) == L.alive_knn_grouped_workspace_bytes(n, t, k) > 0
    for bad in ((0, 8, 4), (1025, 8, 4), (16, 8, 0), (16, 8, 9), (1024, 1025, 4)):
        assert L.alive_knn_grouped_k_workspace_bytes(*bad) == 0, bad
    # the pool form: room for one group per (voice, k), so never less than the uniform search's and monotone in k_max
    args = lambda k: (256, 50, k, 5, 20000, 9000)                     # noqa: E731
    sizes = [L.alive_knn_pool_k_workspace_bytes(*args(k)) for k in range(1, 9)]
    assert all(s > 0 for s in sizes) and sizes == sorted(sizes)
    assert sizes[0] == L.alive_knn_pool_workspace_bytes(*args(1))
    assert all(s >= L.alive_knn_pool_workspace_bytes(*args(k)) for k, s in zip(range(1, 9), sizes))
    for k in (0, 9):
        assert L.alive_knn_pool_k_workspace_bytes(*args(k)) == 0


def test_per_row_k_entry_points_refuse_bad_arguments_before_launching():
    L = nat.lib()

    def grouped(**kw):
        a = dict(src=1, N=4, T=8, rows=1, norms=1, P=100, lo=1, ln=1, k_row=1, k_max=4, val=1, idx=1, ws=1)
        a.update(kw)
        return L.alive_knn_search_grouped_k(a["src"], a["N"], a["T"], a["rows"], a["norms"], a["P"], a["lo"], a["ln"], a["k_row"],
                                            a["k_max"], a["val"], a["idx"], a["ws"], None)

    def pool(**kw):
        a = dict(src=1, N=4, T=8, img=1, off=1, rows=1, norms=1, bounds=1, P=100, lo=1, ln=1, V=2, max_len=60, voice=1, k_row=1,
                 k_max=4, val=1, idx=1, ws=1)
        a.update(kw)
        return L.alive_knn_search_pool_k(a["src"], a["N"], a["T"], a["img"], a["off"], a["rows"], a["norms"], a["bounds"], a["P"],
                                         a["lo"], a["ln"], a["V"], a["max_len"], a["voice"], a["k_row"], a["k_max"], a["val"],
                                         a["idx"], a["ws"], None)

    def merge(**kw):
        a = dict(val=1, idx=1, k_row=1, k_max=4, alpha=1, rows=1, src=1, N=2, T=8, out=1)
        a.update(kw)
        return L.alive_knn_merge_gather_rows_k(a["val"], a["idx"], a["k_row"], a["k_max"], a["alpha"], a["rows"], a["src"], a["N"],
                                               a["T"], a["out"], None, None)

    def blend(**kw):
        a = dict(val=1, idx=1, k_row=1, k_max=4, first=1, weight=1, alpha=1, rows=1, src=1, N=2, T=8, out=1)
        a.update(kw)
        return L.alive_knn_blend_gather_rows_k(a["val"], a["idx"], a["k_row"], a["k_max"], a["first"], a["weight"], a["alpha"],
                                               a["rows"], a["src"], a["N"], a["T"], a["out"], None)
    cases = [(grouped, "alive_knn_search_grouped_k", [(dict(k_row=None), b"null"), (dict(src=None), b"null"), (dict(k_max=0), b"k=0"),
                                                      (dict(k_max=9), b"k=9"), (dict(N=0), b"N=0"), (dict(N=1025), b"N=1025"),
                                                      (dict(T=0), b"T=0"), (dict(P=0), b"pool of 0 rows")]),
             (pool, "alive_knn_search_pool_k", [(dict(k_row=None), b"null"), (dict(voice=None), b"null"), (dict(k_max=0), b"k=0"),
                                                (dict(k_max=9), b"k=9"), (dict(N=4097), b"N=4097"), (dict(V=0), b"V=0"),
                                                (dict(max_len=0), b"longest voice 0")]),
             (merge, "alive_knn_merge_gather_rows_k", [(dict(k_row=None), b"null"), (dict(alpha=None), b"null"), (dict(k_max=0), b"k=0"),
                                                       (dict(k_max=9), b"k=9"), (dict(N=0), b"empty")]),
             (blend, "alive_knn_blend_gather_rows_k", [(dict(k_row=None), b"null"), (dict(first=None), b"null"), (dict(k_max=0), b"k=0"),
                                                       (dict(k_max=9), b"k=9"), (dict(T=0), b"T=0")])]
    for fn, name, bad in cases:
        for kw, msg in bad:
            assert fn(**kw) == -1, (name, kw)
            err = L.alive_last_error()
            assert err.startswith(name.encode() + b":") and msg in err, (name, kw, err)


def test_wrappers_refuse_a_malformed_k_row_before_device_work(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("allocated before the arguments were checked")
    monkeypatch.setattr(MS._ws, "get", boom)
    src = torch.zeros(3, 768, 5)
    t32 = torch.zeros(3, dtype=torch.int32)
    with pytest.raises(ValueError, match="k_max=9"):
        MS.knn_search_grouped_k(src, None, None, t32, t32, t32, 9)
    with pytest.raises(ValueError, match="k_row must be int32"):
        MS.knn_search_grouped_k(src, None, None, t32, t32, torch.zeros(3, dtype=torch.int64), 4)
    with pytest.raises(ValueError, match="k_row must be int32"):
        MS.knn_search_grouped_k(src, None, None, t32, t32, torch.zeros(2, dtype=torch.int32), 4)


def test_check_k():
    assert MS.check_k(1) == 1 and MS.check_k(8) == 8 and MS.check_k(np.int64(3)) == 3
    for bad in (True, False, 0, 9, -1, "4", 4.0, None, [4]):
        with pytest.raises(ValueError, match=r"integer in \[1, 8\]"):
            MS.check_k(bad)
    with pytest.raises(ValueError, match=r"integer in \[1, 4\]"):
        MS.check_k(5, hi=4)
    assert "k" in MS._PARAMS


# ---------------------------------------------------------------------------------------------------- jobs and sessions files
@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "b.wav", "spk.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, entries, name="f.json"):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_jobs_file_takes_k_per_job(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = BI.load_jobs(write(files, [job, dict(job, k=1), dict(job, k=8)]))
    assert (a["k"], b["k"], c["k"]) == (4, 1, 8)
    a, b = BI.load_jobs(write(files, [job, dict(job, k=7)]), k=2)          # the default is -k
    assert (a["k"], b["k"]) == (2, 7)
    for bad in (True, False, 0, 9, "4", 4.5, None):
        with pytest.raises(ValueError, match=r"job 1: \"k\""):
            BI.load_jobs(write(files, [job, dict(job, k=bad)]))
    # a file without "k": today's dicts plus the default
    plain = BI.load_jobs(write(files, [job, dict(job, input="b.wav", target="spk.wav", pitch=2)]), k=3)
    for e in plain:
        assert set(e) == set(BI.JOB_KEYS) and e["k"] == 3
    assert BI.jobs_k(plain, 3) == 3                                          # ... and the uniform path
    mixed = BI.load_jobs(write(files, [job, dict(job, k=2)]))
    assert BI.jobs_k(mixed, 4) == [4, 2]
    assert BI.jobs_k(BI.load_jobs(write(files, [dict(job, k=4), dict(job, k=4)])), 4) == 4


def test_jobs_voice_sizes_are_checked_against_each_jobs_own_k(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    blend = {"input": "a.wav", "blend": [{"lib": "voice_library.pt", "weight": 1}, {"target": "spk.wav", "weight": 1}]}
    lib, spk = (None, str(files / "voice_library.pt")), (str(files / "spk.wav"), None)
    sizes = {lib: 300, spk: 3}
    BI.check_job_voice_sizes(BI.load_jobs(write(files, [dict(job, k=8), dict(blend, k=3)])), sizes)
    with pytest.raises(ValueError, match="3 vectors, fewer than k=4"):
        BI.check_job_voice_sizes(BI.load_jobs(write(files, [dict(job, k=8), blend])), sizes)
    BI.check_job_voice_sizes(BI.load_jobs(write(files, [dict(job, k=8), blend]), k=2), sizes)


def test_sessions_file_takes_k_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, k=1, start=2), dict(sess, k=8)]))
    assert (a["k"], b["k"], c["k"], b["start"]) == (4, 1, 8, 2)
    a, b = MSI.load_sessions(write(files, [sess, dict(sess, k=5)]), k=2)
    assert (a["k"], b["k"]) == (2, 5)
    for bad in (True, False, 0, 9, "4", 4.5, None):
        with pytest.raises(ValueError, match=r"session 0: \"k\""):
            MSI.load_sessions(write(files, [dict(sess, k=bad)]))
    with pytest.raises(ValueError, match="-k=9"):
        MSI.load_sessions(write(files, [sess]), k=9)
    plain = MSI.load_sessions(write(files, [sess, dict(sess, pitch=3)]), k=6)
    for e in plain:
        assert set(e) == set(MSI.SESSION_KEYS) and e["k"] == 6


def test_multistream_cli_derives_k_max():
    f = MSI.converter_k_max
    assert f([dict(k=4), dict(k=4)], 4) is None                              # nobody differs: the uniform converter
    assert f([dict(), dict()], 4) is None
    assert f([dict(k=4), dict(k=2)], 4) == 4                                 # the default stays in range
    assert f([dict(k=1), dict(k=2)], 4) == 4
    assert f([dict(k=4), dict(k=8), dict(k=1)], 4) == 8
    assert f([dict(k=3), dict(k=3)], 2) == 3
    assert f([dict(k=2)], 2) is None


# ---------------------------------------------------------------------------------------------------- open / set
class _Pool:
    """VoicePool's segment() over a name -> size table (no device)"""

    def __init__(self, sizes):
        self.sizes = sizes

    def segment(self, name):
        if name not in self.sizes:
            raise ValueError(f"unknown voice {name!r}")
        return 7, self.sizes[name]


def _converter(B=3, k=4, k_max=None, blend=1):
    """a MultiStreamConverter's session state on host tensors: what open / set / close read and write, without networks"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.pool = _Pool({"big": 500, "six": 6, "two": 2})
    c.B, c.S, c.k, c.k_max = B, blend, k, k_max
    c.device = torch.device("cpu")
    c._reserved, c._names, c.world_pitch, c._rt = False, [()] * B, False, None
    c.input_sr, c.rates, c.chunk, c.buffersize = 16000, (16000,), 160, 4
    c.is_open, c.params, c.count, c.rate, c.slot_chunk = [False] * B, [None] * B, [0] * B, [16000] * B, [160] * B
    c.ring = np.zeros((B, 640), dtype=np.int16)
    c.seg_lo, c.seg_len = torch.zeros(B * blend, dtype=torch.int32), torch.zeros(B * blend, dtype=torch.int32)
    if blend > 1:
        c.weight = torch.zeros(B * blend, dtype=torch.float64)
    if k_max is not None:
        c.k_rows = torch.full((B,), k, dtype=torch.int32)
        c.k_lists = c.k_rows if blend == 1 else torch.full((B * blend,), k, dtype=torch.int32)
    c.alpha = torch.zeros(B, dtype=torch.float64)
    c.f0_rate, c.pitch = torch.ones(B), torch.zeros(B)
    c.in_post, c.out_pre = torch.ones(B), torch.ones(B)
    c.phi = torch.zeros(B, 64)
    return c


def test_constructor_checks_k_max_before_any_device_work():
    for bad in (0, 9, True, 4.0, "8"):
        with pytest.raises(ValueError, match="k_max"):
            MS.MultiStreamConverter(None, None, None, None, 4, k=4, k_max=bad)
    with pytest.raises(ValueError, match="k_max=3 is below the converter's k=4"):
        MS.MultiStreamConverter(None, None, None, None, 4, k=4, k_max=3)


def test_a_session_k_needs_k_max():
    c = _converter(k=4, k_max=None)
    c.open(0, "big")                                                          # as before
    c.open(1, "big", k=4)                                                     # the converter's own k is accepted
    assert c.params[0]["k"] is None and c.params[1]["k"] == 4 and not hasattr(c, "k_rows")
    with pytest.raises(ValueError, match="k_max"):
        c.open(2, "big", k=2)
    assert not c.is_open[2]
    with pytest.raises(ValueError, match="k_max"):
        c.set(0, k=8)
    with pytest.raises(ValueError, match="k_max"):
        c.set(0, k=True)
    assert c.params[0]["k"] is None


def test_open_and_set_with_k_max():
    c = _converter(k=4, k_max=6)
    c.open(0, "big")                                                          # default: the converter's k
    c.open(1, "big", k=1)
    c.open(2, "six", k=6)
    assert c.k_rows.tolist() == [4, 1, 6] and c.seg_len.tolist() == [500, 500, 6] and c.seg_lo.tolist() == [7, 7, 7]
    with pytest.raises(ValueError, match="above the converter's k_max=6"):
        c.set(0, k=7)
    for bad in (0, 9, True, "2", 2.0):
        with pytest.raises(ValueError, match=r"slot 0: k"):
            c.set(0, k=bad)
    assert c.k_rows.tolist() == [4, 1, 6] and c.params[0]["k"] is None        # a refused set changes nothing
    c.set(0, k=2).set(1, k=6, alpha=0.5)
    assert c.k_rows.tolist() == [2, 6, 6] and c.params[1]["k"] == 6 and c.alpha[1] == 0.5
    c.set(0, pitch=2.0)                                                       # the session keeps its k
    assert c.k_rows.tolist() == [2, 6, 6]
    c.set(0, k=None)                                                          # back to the converter's
    assert c.k_rows.tolist() == [4, 6, 6]
    c.close(1)
    assert c.k_rows.tolist() == [4, 4, 6] and c.seg_len.tolist() == [500, 0, 6]     # a closed slot stays inactive


def test_a_voice_shorter_than_the_sessions_k_is_refused_but_taken_at_a_smaller_k():
    c = _converter(k=4, k_max=8)
    with pytest.raises(ValueError, match="'two' has 2 vectors, fewer than k=4"):
        c.open(0, "two")                                                      # the converter's default k
    c.open(0, "two", k=2)                                                     # shorter than k_max and than k, not than its own k
    c.open(1, "six", k=6)
    with pytest.raises(ValueError, match="'six' has 6 vectors, fewer than k=7"):
        c.set(1, k=7)
    with pytest.raises(ValueError, match="'two' has 2 vectors, fewer than k=3"):
        c.set(0, k=3)
    assert c.k_rows.tolist() == [2, 6, 4]
    c.set(0, voice="big", k=8)
    with pytest.raises(ValueError, match="fewer than k=8"):
        c.set(0, voice="six")                                                 # the session's own k is what counts
    assert c.seg_len.tolist()[0] == 500


def test_a_blend_is_checked_against_its_sessions_k_and_k_is_repeated_on_its_list_rows():
    c = _converter(B=2, k=4, k_max=8, blend=3)
    c.open(0, {"big": 1, "six": 1}, k=6)
    assert c.k_rows.tolist() == [6, 4] and c.k_lists.tolist() == [6, 6, 6, 4, 4, 4]
    assert c.seg_len.tolist() == [500, 6, 0, 0, 0, 0]
    with pytest.raises(ValueError, match="'six' has 6 vectors, fewer than k=7"):
        c.set(0, k=7)
    with pytest.raises(ValueError, match="'two' has 2 vectors"):
        c.open(1, [("big", 1), ("two", 2)], k=3)
    c.open(1, [("big", 1), ("two", 2), ("six", 1)], k=2)
    assert c.k_lists.tolist() == [6, 6, 6, 2, 2, 2] and c.seg_len.tolist() == [500, 6, 0, 500, 2, 6]
    c.close(0)
    assert c.k_lists.tolist() == [4, 4, 4, 2, 2, 2] and c.seg_len.tolist()[:3] == [0, 0, 0]


def test_convert_many_checks_a_k_list_before_device_work():
    from module.pipeline import Converter
    conv = Converter.__new__(Converter)
    pool = _Pool({"big": 500, "two": 2})
    u = [torch.zeros(1, 100)] * 2
    with pytest.raises(ValueError, match="k: 3 values for 2 utterances"):
        conv.convert_many(u, pool, ["big", "big"], k=[4, 4, 4])
    for bad in (0, 9, True, "4", 2.5):
        with pytest.raises(ValueError, match=r"convert_many: k\[1\]"):
            conv.convert_many(u, pool, ["big", "big"], k=[4, bad])
    with pytest.raises(ValueError, match="'two' has 2 vectors, fewer than k=3"):
        conv.convert_many(u, pool, ["big", "two"], k=[8, 3])
