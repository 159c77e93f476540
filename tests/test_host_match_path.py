"""CPU tests of the match path: the NumPy restatement tools/match_path_ref.py (weight 0, the worked case on unit rows, the path against
the top-1 path and against every path of a small case), the C ABI (symbols, prototypes, SRCS, the layout, the refusals that need no
device), the options and flags, every refusal of the converters' host logic and the jobs files."""
import ctypes
import itertools
import json
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import batch_inference as BI                                         # noqa: E402
import match_path_ref as MP                                          # noqa: E402
from module import _native as nat                                    # noqa: E402
from module import common, ops                                       # noqa: E402

P = 64


@pytest.fixture(scope="module")
def pool():
    rows = np.random.default_rng(0).standard_normal((P, MP.DIM)).astype(np.float32)
    norms = np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    return rows, norms, MP.cosine_table(rows, norms)


def lists(T, K, seed, repeat=0.35):
    rng = np.random.default_rng(seed)
    val = -np.sort(-rng.uniform(0.6, 0.9, (T, K)).astype(np.float32), axis=1)
    idx = rng.integers(0, P, (T, K)).astype(np.int32)
    for t in range(1, T):
        idx[t] = np.where(rng.random(K) < repeat, idx[t - 1][rng.permutation(K)], idx[t])
    return val, idx


# ------------------------------------------------------------------------------------------------ the restatement
def test_weight_zero_is_the_top_1_match(pool):
    rows, norms, table = pool
    for K in (1, 2, 8):
        val, idx = lists(40, K, K)
        val[7, 1:] = val[7, 0]                                        # a frame of equal cosines: the lowest entry
        J = MP.join(idx, K, rows, norms, table)[0]
        p, score = MP.path(val, idx, K, rows, norms, 0.0, J)
        assert p.tolist() == [0] * 40 and score == 0.0
        ov, oi, moved, _ = MP.path_rows(val[None], idx[None], K, 1, 0.0, rows, norms, table)
        assert np.array_equal(oi[0, :, 0], idx[:, 0]) and np.array_equal(ov[0, :, 0], val[:, 0]) and moved.tolist() == [0]
        assert np.all(oi[0, :, 1:] == -1) and np.all(np.isneginf(ov[0, :, 1:]))


def test_the_worked_case():
    T = 12
    val, idx, rows, norms = MP.exact_case(T)
    J, written = MP.join(idx, 2, rows, norms)
    assert set(np.unique(J[written])) == {0.0, 1.0} and written[1:].all() and not written[0].any()
    assert MP.path(val, idx, 2, rows, norms, 0.0625)[0].tolist() == [0] * T
    p, score = MP.path(val, idx, 2, rows, norms, 0.25)
    assert p.tolist() == [1] * T and score == -0.125 * 12 + 0.25 * 11
    ov, oi, moved, _ = MP.path_rows(val[None], idx[None], 2, 1, 0.25, rows, norms)
    assert moved.tolist() == [12] and np.all(oi[0, :, 0] == 0) and np.all(ov[0, :, 0] == np.float32(0.625))
    val, idx, rows, norms = MP.exact_case(T, gap=5)
    p, score = MP.path(val, idx, 2, rows, norms, 0.25)
    assert p.tolist() == [1] * 5 + [-1] + [1] * 6 and score == (-0.125 * 5 + 0.25 * 4) + (-0.125 * 6 + 0.25 * 5)
    ov, oi, moved, _ = MP.path_rows(val[None], idx[None], 2, 1, 0.25, rows, norms)
    assert moved.tolist() == [11] and np.all(oi[0, 5] == -1) and np.all(np.isneginf(ov[0, 5]))


def test_the_path_scores_at_least_the_top_1_path_and_is_the_best_of_all_paths(pool):
    rows, norms, table = pool
    for seed, (T, K, w) in enumerate([(40, 8, 1.0), (40, 4, 0.25), (33, 2, 8.0), (17, 8, 8.0)]):
        val, idx = lists(T, K, 10 + seed)
        idx[T // 2], val[T // 2] = -1, -np.inf                        # two segments
        J = MP.join(idx, K, rows, norms, table)[0]
        p, score = MP.path(val, idx, K, rows, norms, w, J)
        top1 = np.where(p >= 0, 0, -1)
        assert score == MP.path_score(p, val, idx, K, rows, norms, w, J)
        assert score >= MP.path_score(top1, val, idx, K, rows, norms, w, J)
    val, idx = lists(5, 3, 99, repeat=0.6)                            # 3^5 paths, all enumerated
    idx[3, 2], val[3, 2] = -1, -np.inf                                # a state that does not exist
    J = MP.join(idx, 3, rows, norms, table)[0]
    p, score = MP.path(val, idx, 3, rows, norms, 1.0, J)
    every = [MP.path_score(np.array(q), val, idx, 3, rows, norms, 1.0, J) for q in itertools.product(range(3), repeat=5) if q[3] != 2]
    assert score == max(every) and p[3] != 2


def test_rows_that_are_off_and_frames_beyond_the_table(pool):
    rows, norms, table = pool
    val, idx = lists(9, 4, 5)
    v3, i3 = np.stack([val] * 3), np.stack([idx] * 3)
    i3[2, 4, 1] = P                                                   # beyond the table: its frame is inactive
    ov, oi, moved, paths = MP.path_rows(v3, i3, [4, 5, 4], [0, 1, 1], 1.0, rows, norms, table)
    assert paths[0] is None and paths[1] is None and moved[:2].tolist() == [0, 0]
    assert np.array_equal(oi[:2], i3[:2]) and np.array_equal(ov[:2], v3[:2])
    assert paths[2][4] == -1 and np.all(oi[2, 4] == -1) and (paths[2][[0, 1, 2, 3, 5, 6, 7, 8]] >= 0).all()


# ------------------------------------------------------------------------------------------------ the C ABI
def test_the_symbols_are_exported_and_the_prototypes_agree_with_the_header():
    L = ctypes.CDLL(nat.LIB_PATH)
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    for name, res, nargs in (("alive_knn_path_rows", ctypes.c_int, 16), ("alive_knn_path_layout", ctypes.c_int, 4),
                             ("alive_knn_path_workspace_bytes", ctypes.c_size_t, 3)):
        assert hasattr(L, name)
        decl = re.search(r"\b(?:int|size_t)\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl is not None, f"{name} is not declared in alive_vc.h"
        args = decl.group(1).split(",")
        assert len(args) == nargs == len(nat.PROTOTYPES[name][1]) and nat.PROTOTYPES[name][0] is res
        want = [ctypes.c_void_p if "*" in a else (ctypes.c_int64 if "int64_t" in a else ctypes.c_int) for a in args]
        assert want == nat.PROTOTYPES[name][1], name
    assert re.search(r"#define\s+ALIVE_KNN_PATH_MAX_K\s+8\b", hdr) and re.search(r"#define\s+ALIVE_KNN_PATH_MAX_FRAMES\s+1048576\b", hdr)
    assert (common.PATH_MAX_K, common.PATH_MAX_FRAMES) == (ops.PATH_MAX_K, ops.PATH_MAX_FRAMES) == (MP.MAX_K, MP.MAX_FRAMES) == (8, 1 << 20)
    mk = open(os.path.join(ROOT, "alive-vc_amd", "csrc", "Makefile")).read()
    assert "match_path.hip" in [w for ln in mk.splitlines() if ln.startswith("SRCS") for w in ln.split()]
    assert "-ffp-contract=off" in mk and "-fno-fast-math" in mk


def test_the_layout_agrees_with_the_workspace():
    L = nat.lib()
    for R, T, k in ((1, 1, 1), (3, 33, 8), (3, 5, 3), (128, 24, 4), (384, 450, 8), (1, 1 << 20, 8), (1 << 20, 1, 1)):
        off = (ctypes.c_int64 * 2)(-1, -1)
        assert L.alive_knn_path_layout(R, T, k, off) == 0
        total = L.alive_knn_path_workspace_bytes(R, T, k)
        assert off[0] == 0 and off[1] % 256 == 0 and off[1] >= off[0] + 8 * k * k * R * T and off[1] + R * T * k <= total < off[1] + R * T * k + 256
    for bad in ((0, 5, 4), (3, 0, 4), (3, 5, 0), (3, 5, 9), (1025, 1024, 4)):
        off = (ctypes.c_int64 * 2)(-1, -1)
        assert L.alive_knn_path_workspace_bytes(*bad) == 0
        assert L.alive_knn_path_layout(*bad, off) == -1 and b"alive_knn_path_layout" in L.alive_last_error() and list(off) == [-1, -1]
    assert L.alive_knn_path_layout(3, 5, 4, None) == -1


def test_the_abi_refuses_bad_arguments_without_a_device():
    L = nat.lib()
    #     val   idx   k_row  k_max on     weight rows   norms   P   R  T  out_val out_idx moved   ws       stream
    ok = [4096, 8192, 12288, 4,    16384, 20480, 24576, 28672, 64, 3, 5, 32768,  36864,  40960, 1 << 20, None]
    for change, msg in (({0: None}, b"null lists"), ({1: None}, b"null lists"), ({11: None}, b"null lists"), ({12: None}, b"null lists"),
                        ({2: None}, b"null per-row"), ({4: None}, b"null per-row"), ({5: None}, b"null per-row"), ({13: None}, b"null per-row"),
                        ({6: None}, b"null pointer"), ({7: None}, b"null pointer"), ({14: None}, b"null pointer"),
                        ({3: 0}, b"k_max 0 outside [1, 8]"), ({3: 9}, b"k_max 9 outside [1, 8]"), ({9: 0}, b"empty lists"),
                        ({10: 0}, b"empty lists"), ({9: 1025, 10: 1024}, b"exceeds 2^20 frames"), ({8: 0}, b"P outside"),
                        ({8: -5}, b"P outside"), ({11: 4096}, b"must not be the input lists")):
        a = list(ok)
        for i, v in change.items():
            a[i] = v
        assert L.alive_knn_path_rows(*a) == -1 and msg in L.alive_last_error(), change


# ------------------------------------------------------------------------------------------------ options and flags
def test_path_options_and_the_wrapper_check_their_arguments():
    assert common.path_options(None) is None and common.path_options(False) is None
    assert common.path_options(True) == dict(weight=1.0) == dict(weight=common.PATH_WEIGHT)
    o = common.path_options({"weight": 3})
    assert o == dict(weight=3.0) and isinstance(o["weight"], float) and common.path_options({}) == dict(weight=1.0)
    assert common.path_options({"weight": 0}) == dict(weight=0.0)
    for bad in (-1, float("nan"), float("inf"), "1", True, None):
        with pytest.raises(ValueError, match="match path: weight must be a finite number >= 0"):
            common.path_options({"weight": bad})
    for bad, msg in ((1, "expected None, a bool or a dict"), ("on", "expected None, a bool or a dict"), ({"jump": 2}, r"unknown keys \['jump'\]")):
        with pytest.raises(ValueError, match="match_path: " + msg):
            common.path_options(bad)
    with pytest.raises(ValueError, match=r"convert_many: match_path\[2\]: unknown keys"):
        common.path_options({"w": 1}, "convert_many: match_path[2]")
    val, idx = torch.zeros(10, 4), torch.zeros(10, 4, dtype=torch.int32)
    i32, f64 = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float64)
    rows, norms = torch.zeros(64, 768), torch.zeros(64)
    for args, msg in (((val, idx, i32, 8, i32, f64, rows, norms), r"lists must be fp32 / int32 \[R \* T, 8\]"),
                      ((val, idx.long(), i32, 4, i32, f64, rows, norms), "lists must be"),
                      ((val, idx, torch.zeros(3, dtype=torch.int32), 4, i32, f64, rows, norms), "10 list frames do not divide into 3 rows"),
                      ((val, idx, i32, 4, i32.long(), f64, rows, norms), "on must be a contiguous torch.int32"),
                      ((val, idx, i32, 4, i32, f64.float(), rows, norms), "weight must be a contiguous torch.float64"),
                      ((val, idx, i32, 4, i32, f64, rows[:, :512], norms), "rows must be fp32"),
                      ((val, idx, i32, 4, i32, f64, rows, norms[:5]), "rows must be fp32")):
        with pytest.raises(ValueError, match="match path: " + msg):
            ops.knn_path_rows(*args)
    with pytest.raises(RuntimeError):                                # host tensors: no CPU fall-back
        ops.knn_path_rows(val, idx, i32, 4, i32, f64, rows, norms)


def test_the_clis_take_the_path_flags():
    import inference as INF
    for mod, argv in ((INF, []), (BI, ["j.json"])):
        args = mod.build_parser().parse_args(argv)
        assert (args.match_path, args.path_weight) == (False, 1.0) and common.path_arguments(args) is None
        args = mod.build_parser().parse_args(argv + ["-mp", "--path-weight", "0.5"])
        assert args.match_path is True and common.path_arguments(args) == dict(weight=0.5)
        assert common.path_arguments(mod.build_parser().parse_args(argv + ["--match-path"])) == dict(weight=1.0)
        for bad in ("-1", "nan", "inf"):
            with pytest.raises(ValueError, match="--path-weight must be a finite number >= 0"):
                common.path_arguments(mod.build_parser().parse_args(argv + ["--path-weight", bad]))


# ------------------------------------------------------------------------------------------------ the converters' host logic
def test_the_offline_converter_checks_the_option_before_any_launch():
    from module.pipeline import Converter
    from module.sharded import ShardedConverter
    conv = Converter.__new__(Converter)
    conv.device = torch.device("cpu")
    win = torch.zeros(2, 9600)
    for bad, msg in (({"weight": -1}, "weight must be"), ({"jump": 1}, "unknown keys"), ("on", "expected None, a bool or a dict")):
        with pytest.raises(ValueError, match=msg):
            conv._convert_windows(win, match_path=bad)
    utts = [torch.zeros(1, 4000)] * 3
    with pytest.raises(ValueError, match="match_path: 2 values for 3 utterances"):
        conv.convert_many(utts, None, ["a", "b", "c"], match_path=[True, False])
    with pytest.raises(ValueError, match=r"convert_many: match_path\[2\]: unknown keys"):
        conv.convert_many(utts, None, ["a", "b", "c"], match_path=[True, False, {"width": 1}])
    sh = ShardedConverter.__new__(ShardedConverter)
    sh.device = torch.device("cpu")
    for on in (True, {"weight": 0.5}):
        with pytest.raises(ValueError, match="match_path is not available with a sharded library"):
            sh._convert_windows(win, match_path=on)
    assert sh._path_options(None) is None and sh._path_options(False) is None


# ------------------------------------------------------------------------------------------------ the files
@pytest.fixture
def files(tmp_path):
    for name in ("a.wav", "spk.wav", "voice_library.pt"):
        (tmp_path / name).write_bytes(b"x")
    return tmp_path


def write(d, entries, name="f.json"):
    p = d / name
    p.write_text(json.dumps(entries))
    return str(p)


def test_jobs_file_takes_the_path_per_job(files):
    job = {"input": "a.wav", "lib": "voice_library.pt"}
    assert BI.PATH_KEYS == ("match_path",)
    a, b, c, d = BI.load_jobs(write(files, [job, dict(job, match_path=True), dict(job, match_path=False), dict(job, match_path={"weight": 3})]))
    assert set(a) == set(BI.JOB_KEYS) == set(c) and set(b) == set(BI.JOB_KEYS + BI.PATH_KEYS) == set(d)    # a file without the key: as before
    assert b["match_path"] == dict(weight=1.0) and d["match_path"] == dict(weight=3.0)
    a, b, c = BI.load_jobs(write(files, [job, dict(job, match_path=False), dict(job, match_path={})]), match_path=True, path_weight=0.5)
    assert a["match_path"] == dict(weight=0.5) == c["match_path"] and "match_path" not in b
    a, = BI.load_jobs(write(files, [dict(job, match_path={"weight": 2})]), match_path=False, path_weight=0.5)
    assert a["match_path"] == dict(weight=2.0)
    for bad in (1, "true", None, [True], {"jump": 1}, {"weight": -1}, {"weight": "1"}):
        with pytest.raises(ValueError, match=r"job 1: "):
            BI.load_jobs(write(files, [job, dict(job, match_path=bad)]))
    with pytest.raises(ValueError, match=r"job 0: unknown keys \['path_weight'\]"):
        BI.load_jobs(write(files, [dict(job, path_weight=2)]))
    with pytest.raises(ValueError, match=r"-mp / --path-weight: match path: weight must be"):
        BI.load_jobs(write(files, [job]), path_weight=float("nan"))


# ------------------------------------------------------------------------------------------------ the streaming converters' host logic
import multistream_inference as MSI                                  # noqa: E402
from module import multistream as MS                                 # noqa: E402


def _host_converter(match_path):
    """the part of a converter the path's validation reads, without a device"""
    c = MS.MultiStreamConverter.__new__(MS.MultiStreamConverter)
    c.match_path = match_path
    return c


def test_session_settings_are_checked_against_the_converter():
    assert {"match_path", "path_weight"} <= set(MS._PARAMS) and MS.knn_path_rows is ops.knn_path_rows
    on, off = _host_converter(True), _host_converter(False)
    assert on._session_path(0, dict(match_path=True, path_weight=2)) == (1, 2.0)
    assert on._session_path(0, {}) == (0, 1.0) == off._session_path(0, dict(match_path=False))
    with pytest.raises(ValueError, match=r"slot 2: match_path=True needs a converter built with MultiStreamConverter\(..., match_path=True\)"):
        off._session_path(2, dict(match_path=True))
    for bad in (1, "yes", None):
        with pytest.raises(ValueError, match="slot 1: match_path must be a bool"):
            on._session_path(1, dict(match_path=bad))
    for bad in (-1, float("nan"), float("inf"), "1", True):
        for conv in (on, off):
            with pytest.raises(ValueError, match="slot 1: match path: path_weight must be a finite number >= 0"):
                conv._session_path(1, dict(path_weight=bad))
    with pytest.raises(ValueError, match="match_path must be a bool"):
        MS.MultiStreamConverter(None, None, None, None, 1, match_path=1)
    with pytest.raises(ValueError, match=r"path_moved needs a converter built with MultiStreamConverter\(..., match_path=True\)"):
        off.path_moved()
    assert MS.MultiStreamConverter.match_path is False


def test_realtime_converter_checks_the_option_before_anything_is_built():
    from module.realtime import RealtimeConverter
    for bad, msg in ((1, "expected None, a bool or a dict"), ({"weight": -1}, "weight must be"), ({"x": 1}, "unknown keys")):
        with pytest.raises(ValueError, match="RealtimeConverter: match_path: " + msg if "weight must" not in msg else msg):
            RealtimeConverter(None, None, None, None, match_path=bad)
    with pytest.raises(ValueError, match="interior reuse cannot be combined with match_path"):
        RealtimeConverter(None, None, None, None, match_path=True, reuse_interior=True)
    rt = RealtimeConverter.__new__(RealtimeConverter)
    assert rt.match_path is False
    with pytest.raises(ValueError, match="path_moved needs a converter built with"):
        rt.path_moved()


def test_sessions_file_takes_the_path_per_session(files):
    sess = {"input": "a.wav", "lib": "voice_library.pt"}
    assert MSI.PATH_KEYS == ("match_path", "path_weight")
    a, b, c, d = MSI.load_sessions(write(files, [sess, dict(sess, match_path=True), dict(sess, match_path=False, path_weight=3),
                                                 dict(sess, match_path=True, path_weight=0)]))
    assert set(a) == set(MSI.SESSION_KEYS) == set(c)                 # a file without the keys parses to what it did
    assert set(b) == set(MSI.SESSION_KEYS) | set(MSI.PATH_KEYS) == set(d)
    assert (b["match_path"], b["path_weight"]) == (True, 1.0) and d["path_weight"] == 0.0 and isinstance(d["path_weight"], float)
    # -mp and its weight are the defaults; a session's false switches it off, its own weight wins
    a, b, c = MSI.load_sessions(write(files, [sess, dict(sess, match_path=False), dict(sess, path_weight=2)]), match_path=True, path_weight=0.5)
    assert a["path_weight"] == 0.5 and "match_path" not in b and c["path_weight"] == 2.0 and c["match_path"] is True
    for bad in (1, "true", None, [True], {"weight": 1}):
        with pytest.raises(ValueError, match=r"session 1: \"match_path\" must be true or false"):
            MSI.load_sessions(write(files, [sess, dict(sess, match_path=bad)]))
    for bad in (-1, "1", True):
        with pytest.raises(ValueError, match=r"session 1: match path: \"path_weight\" must be"):
            MSI.load_sessions(write(files, [sess, dict(sess, path_weight=bad)]))
    with pytest.raises(ValueError, match=r"session 0: unknown keys \['path_jump'\]"):
        MSI.load_sessions(write(files, [dict(sess, path_jump=2)]))
    with pytest.raises(ValueError, match=r"-mp / --path-weight: match path: \"path_weight\" must be"):
        MSI.load_sessions(write(files, [sess]), path_weight=-3)


def test_the_streaming_clis_and_the_bench_tool_take_the_flags():
    import realtime_inference as RI
    for mod, argv in ((RI, []), (MSI, ["s.json"])):
        args = mod.build_parser().parse_args(argv)
        assert (args.match_path, args.path_weight) == (False, 1.0) and common.path_arguments(args) is None
        assert common.path_arguments(mod.build_parser().parse_args(argv + ["-mp", "--path-weight", "2"])) == dict(weight=2.0)
    src = open(os.path.join(ROOT, "tools", "bench_multistream.py")).read()
    assert '"--match-path"' in src and '"--match-path-offline"' in src
