"""CPU tests of the multi-session streaming surface: argument checks of its C ABI entry points (null or invalid arguments
return -1 with a message, nothing is launched), of MultiStreamConverter / VoicePool, and of the multistream CLI's sessions file."""
import json

import pytest

from module import _native as nat
from module import multistream as MS


def test_grouped_search_abi_refuses_bad_arguments():
    L = nat.lib()
    assert L.alive_knn_grouped_workspace_bytes(4, 8, 9) == 0                # k > 8
    assert L.alive_knn_grouped_workspace_bytes(0, 8, 4) == 0
    assert L.alive_knn_grouped_workspace_bytes(2000, 8, 4) == 0             # more rows than one call takes
    assert L.alive_knn_grouped_workspace_bytes(16, 8, 4) > 16 * 8 * 768 * 6
    rc = L.alive_knn_search_grouped(1, 4, 8, 1, 1, 1000, 1, 1, 9, 1, 1, 1, None)
    assert rc == -1 and b"k=9" in L.alive_last_error()
    rc = L.alive_knn_search_grouped(None, 4, 8, 1, 1, 1000, 1, 1, 4, 1, 1, 1, None)
    assert rc == -1 and b"null" in L.alive_last_error()
    rc = L.alive_knn_search_grouped(1, 4, 8, 1, 1, 1000, None, 1, 4, 1, 1, 1, None)          # no segment table
    assert rc == -1 and b"null" in L.alive_last_error()
    rc = L.alive_knn_search_grouped(1, 4, 8, 1, 1, 3, 1, 1, 4, 1, 1, 1, None)                # pool shorter than k
    assert rc == -1 and b"pool of 3 rows" in L.alive_last_error()
    rc = L.alive_knn_search_grouped(1, 0, 8, 1, 1, 1000, 1, 1, 4, 1, 1, 1, None)
    assert rc == -1


def test_grouped_workspace_size_refuses_more_frames_than_the_search_takes():
    """N * T <= 2^20 is the search's limit: one frame more and the size is 0 ("out of range"), not a huge positive size"""
    L = nat.lib()
    for k in (1, 4, 8):
        assert L.alive_knn_grouped_workspace_bytes(1024, 1024, k) > 1024 * 1024 * 768 * 6
        assert L.alive_knn_grouped_workspace_bytes(1024, 1025, k) == 0
        assert L.alive_knn_grouped_workspace_bytes(1, 1 << 20, k) > 0
        assert L.alive_knn_grouped_workspace_bytes(1, (1 << 20) + 1, k) == 0
        assert L.alive_knn_grouped_workspace_bytes(1024, 4096, k) == 0
    assert L.alive_knn_grouped_workspace_bytes(1024, 1025, 4) == 0


def test_grouped_search_refuses_too_many_frames_before_allocating(monkeypatch):
    import torch
    src = torch.empty(1024, 768, 1025, device="meta")                      # (no storage)

    def boom(*a, **kw):
        raise AssertionError("allocated for a shape the search refuses")
    monkeypatch.setattr(MS._ws, "get", boom)
    monkeypatch.setattr(MS.torch, "empty", boom)
    with pytest.raises(ValueError, match="1024 rows x 1025 frames"):
        MS.knn_search_grouped(src, None, None, None, None, 4)


def test_per_row_edge_abi_refuses_bad_arguments():
    L = nat.lib()
    assert L.alive_library_pack_rows(None, 10, 768, 1, 1, None) == -1 and b"null" in L.alive_last_error()
    assert L.alive_library_pack_rows(1, 10, 512, 1, 1, None) == -1 and b"feature dim" in L.alive_last_error()
    assert L.alive_knn_merge_gather_rows(1, 1, 4, None, 1, 1, 2, 8, 1, None, None) == -1 and b"null" in L.alive_last_error()
    assert L.alive_knn_merge_gather_rows(1, 1, 9, 1, 1, 1, 2, 8, 1, None, None) == -1 and b"k=9" in L.alive_last_error()
    assert L.alive_pitch_transform_rows(1, 2, 8, 1, None, 1, 1, None) == -1 and b"null" in L.alive_last_error()
    assert L.alive_pitch_transform_rows(1, 2, 8, 3, 1, 1, 1, None) == -1
    assert L.alive_resample_rows(1, 2, 100, 3, 2, 1, None, 1, 1, 67, None) == -1
    assert L.alive_resample_rows(1, 2, 100, 1, 1, None, 1, 1, 1, 99, None) == -1 and b"Lout == L" in L.alive_last_error()
    assert L.alive_resample_rows(1, 2, 100, 3, 2, None, 1, 1, 1, 67, None) == -1 and b"filter" in L.alive_last_error()


def test_converter_and_pool_argument_errors():
    with pytest.raises(ValueError, match="k=9"):
        MS.MultiStreamConverter(None, None, None, None, 4, k=9)
    with pytest.raises(ValueError, match="slots"):
        MS.MultiStreamConverter(None, None, None, None, 0)
    with pytest.raises(ValueError, match="unknown voice"):
        MS.VoicePool(device="cpu").segment("nobody")
    import torch
    with pytest.raises(ValueError, match=r"\[768, M\]"):
        MS.VoicePool(device="cpu").add("bad", torch.zeros(512, 10))


def test_sessions_file_is_checked(tmp_path):
    import multistream_inference as msi
    p = tmp_path / "s.json"
    for bad, msg in (([], "non-empty"), ([{"target": "t.wav"}], "input"), ([{"input": "a.wav"}], "target"),
                     ([{"input": "a.wav", "lib": "l.pt", "speed": 2}], "unknown keys"),
                     ([{"input": "a.wav", "lib": "l.pt", "start": -1}], "start tick")):
        json.dump(bad, open(p, "w"))
        with pytest.raises(ValueError, match=msg):
            msi.load_sessions(str(p))
    json.dump([{"input": "a.wav", "lib": "/abs/l.pt", "pitch": 3}], open(p, "w"))
    s = msi.load_sessions(str(p))[0]
    assert s["input"] == str(tmp_path / "a.wav") and s["lib"] == "/abs/l.pt" and s["pitch"] == 3.0 and s["start"] == 0
    # the flags shared with realtime_inference.py keep its spelling
    a = msi.build_parser().parse_args(["-c", "160", "-b", "16", "-k", "8", "-isr", "24000", "-osr", "48000", "--no-graph", "s.json"])
    assert (a.chunk, a.buffersize, a.k, a.input_sr, a.output_sr, a.no_graph) == (160, 16, 8, 24000, 48000, True)
