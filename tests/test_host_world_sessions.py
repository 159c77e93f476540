"""CPU tests of WORLD pitch on the batched paths: alive_world_f0_rows refuses bad arguments before it launches anything, the
Python wrappers refuse a malformed mask before any device work, and the jobs / sessions files take "world_pitch" as a JSON bool
only."""
import json
import os
import sys

import pytest

from module import _native as nat
from module import multistream as MS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alive-vc_amd"))
import batch_inference as BI                                         # noqa: E402
import multistream_inference as MSI                                  # noqa: E402


def test_masked_world_abi_refuses_bad_arguments():
    L = nat.lib()
    need = L.alive_world_f0_workspace_bytes(4, 3840, 8000, 20.0, 4096.0, 5.0)
    assert need > 0
    args = lambda n, l8, mask, nb: (1, n, l8, 8000, 20.0, 4096.0, 5.0, 1, mask, 1, 1, nb, None)      # noqa: E731
    assert L.alive_world_f0_rows(*args(4, 3840, None, need)) == -1
    assert b"null row mask" in L.alive_last_error()
    for n, l8 in ((0, 3840), (-1, 3840), (4, 0)):
        assert L.alive_world_f0_rows(*args(n, l8, 1, need)) == -1, (n, l8)
        assert L.alive_last_error().startswith(b"alive_world_f0_rows: bad args")
    assert L.alive_world_f0_rows(*args(4, 3840, 1, need - 1)) == -1
    assert b"workspace" in L.alive_last_error() and L.alive_last_error().startswith(b"alive_world_f0_rows")
    assert L.alive_world_f0_rows(None, 4, 3840, 8000, 20.0, 4096.0, 5.0, 1, 1, 1, 1, need, None) == -1
    assert b"null pointer" in L.alive_last_error()
    assert L.alive_world_f0_rows(1, 4, 3840, 48000, 20.0, 4096.0, 5.0, 1, 1, 1, 1, need, None) == -1     # fs > 16000


def test_masked_world_wrapper_refuses_a_bad_mask_before_device_work():
    import torch
    from module.common import world_f0_rows
    x = torch.zeros(3, 4000)
    with pytest.raises(ValueError, match="int32"):
        world_f0_rows(x, torch.ones(3, dtype=torch.int64))
    with pytest.raises(ValueError, match="int32"):
        world_f0_rows(x, torch.ones(2, dtype=torch.int32))
    with pytest.raises(ValueError, match=r"\[N, L\]"):
        world_f0_rows(torch.zeros(4000), torch.ones(1, dtype=torch.int32))


def test_world_pitch_is_a_session_setting():
    assert "world_pitch" in MS._PARAMS


@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, entries, name):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_jobs_file_takes_world_pitch_as_a_bool(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b, c = BI.load_jobs(write(files, [job, dict(job, world_pitch=True), dict(job, world_pitch=False)], "jobs.json"))
    assert (a["world_pitch"], b["world_pitch"], c["world_pitch"]) == (False, True, False)
    for bad in (1, 0, "true", None, [True]):
        with pytest.raises(ValueError, match=r"job 1: \"world_pitch\" must be true or false"):
            BI.load_jobs(write(files, [job, dict(job, world_pitch=bad)], "jobs.json"))
    with pytest.raises(ValueError, match="unknown keys"):
        BI.load_jobs(write(files, [dict(job, world_pitch=True, wpe=True)], "jobs.json"))


def test_sessions_file_takes_world_pitch_as_a_bool(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    a, b = MSI.load_sessions(write(files, [sess, dict(sess, world_pitch=True, start=2)], "s.json"))
    assert (a["world_pitch"], b["world_pitch"], b["start"]) == (False, True, 2)
    for bad in (1, "yes", None, {"on": True}):
        with pytest.raises(ValueError, match=r"session 0: \"world_pitch\" must be true or false"):
            MSI.load_sessions(write(files, [dict(sess, world_pitch=bad)], "s.json"))
    with pytest.raises(ValueError, match="unknown keys"):
        MSI.load_sessions(write(files, [dict(sess, world_pitch=True, wpe=True)], "s.json"))
