"""Half-precision voice pool, host side: the argument refusals of every _f16 entry point (-1 with a message, nothing launched), their
declarations in include/alive_vc.h and module/_native.py, VoicePool's dtype argument, the refusals of the offline paths on a half
pool and the --pool-dtype flag of the streaming CLI.  No device is needed: a refused call launches nothing, and an empty reserved
pool is two host tensors."""
import os
import re
import sys

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from module import _native as nat                                    # noqa: E402
from module import multistream as MS                                 # noqa: E402
from module import ops                                               # noqa: E402

TWINS = ["alive_pool_append", "alive_pool_move_rows", "alive_knn_search_grouped", "alive_knn_search_grouped_k",
         "alive_knn_merge_gather_rows", "alive_knn_merge_gather_rows_k", "alive_knn_blend_gather_rows", "alive_knn_blend_gather_rows_k",
         "alive_knn_path_rows"]


# ------------------------------------------------------------------------------------------------ declarations
def test_every_f16_entry_point_is_declared_like_its_fp32_twin():
    hdr = open(os.path.join(ROOT, "include", "alive_vc.h")).read()
    L = nat.lib()
    for twin in TWINS:
        name = twin + "_f16"
        assert name in nat.PROTOTYPES and hasattr(L, name), name
        res, args = nat.PROTOTYPES[name]
        assert (res, args) == nat.PROTOTYPES[twin], name              # the same signature: only the table's element type differs
        decl = re.search(r"\bint " + name + r"\((.*?)\);", hdr, flags=re.S)
        assert decl is not None, name
        twin_decl = re.search(r"\bint " + twin + r"\((.*?)\);", hdr, flags=re.S).group(1)
        assert len(decl.group(1).split(",")) == len(twin_decl.split(",")) == len(args), name
        assert "rows_f16" in decl.group(1) and "rows_f32" not in decl.group(1), name


# ------------------------------------------------------------------------------------------------ the C ABI's refusals
def _refused(rc, *needles):
    msg = nat.lib().alive_last_error()
    return rc == -1 and all(n in msg for n in needles)


def test_pool_append_f16_and_move_rows_f16_refuse_bad_arguments():
    L = nat.lib()
    ok = dict(tokens=16, rs=10, cs=1, M=10, D=768, rows=16, norms=16, cap=100, at=0, report=16)

    def append(**kw):
        a = dict(ok, **kw)
        return L.alive_pool_append_f16(a["tokens"], a["rs"], a["cs"], a["M"], a["D"], a["rows"], a["norms"], a["cap"], a["at"],
                                       a["report"], None)
    for null in ("tokens", "rows", "norms", "report"):
        assert _refused(append(**{null: None}), b"alive_pool_append_f16", b"null"), null
    assert _refused(append(D=512), b"alive_pool_append_f16: feature dim 512")
    assert _refused(append(D=384), b"feature dim 384")                       # (half the width is not a half table)
    assert _refused(append(at=91), b"[91, +10) outside the table of 100 rows")
    assert _refused(append(at=-1), b"outside the table") and _refused(append(M=101), b"outside the table")
    assert append(M=0) == -1
    assert _refused(append(at=2 ** 40), b"outside the table")
    assert _refused(append(cap=0), b"capacity") and _refused(append(cap=2 ** 31), b"capacity")
    assert _refused(append(cs=-1), b"stride") and _refused(append(rs=-1), b"stride")

    def move(rows=16, norms=16, cap=100, src=0, dst=50, n=10):
        return L.alive_pool_move_rows_f16(rows, norms, cap, src, dst, n, None)
    assert _refused(move(rows=None), b"alive_pool_move_rows_f16", b"null") and _refused(move(norms=None), b"null")
    for misaligned in (2, 8, 24):                                            # fp16-aligned, not quad-aligned
        assert _refused(move(rows=misaligned), b"alive_pool_move_rows_f16", b"16-byte aligned"), misaligned
    assert _refused(move(src=91), b"10 rows from 91 to 50 outside the table of 100 rows")
    assert _refused(move(dst=91), b"outside the table")
    assert move(src=-1) == -1 and move(dst=-1) == -1 and move(n=0) == -1 and move(n=101) == -1
    assert _refused(move(cap=2 ** 31), b"capacity")
    assert move(src=20, dst=20) == 0                                         # nothing to move: nothing launched


def test_grouped_search_f16_refuses_bad_arguments():
    L = nat.lib()
    ok = dict(src=1, N=4, T=8, rows=1, norms=1, P=1000, lo=1, ln=1, k=4, val=1, idx=1, ws=1)

    def plain(**kw):
        a = dict(ok, **kw)
        return L.alive_knn_search_grouped_f16(a["src"], a["N"], a["T"], a["rows"], a["norms"], a["P"], a["lo"], a["ln"], a["k"], a["val"],
                                              a["idx"], a["ws"], None)

    def per_row(**kw):
        a = dict(dict(ok, k_row=1), **kw)
        return L.alive_knn_search_grouped_k_f16(a["src"], a["N"], a["T"], a["rows"], a["norms"], a["P"], a["lo"], a["ln"], a["k_row"],
                                                a["k"], a["val"], a["idx"], a["ws"], None)
    for fn, who in ((plain, b"alive_knn_search_grouped_f16"), (per_row, b"alive_knn_search_grouped_k_f16")):
        for null in ("src", "rows", "norms", "lo", "ln", "val", "idx", "ws"):
            assert _refused(fn(**{null: None}), who, b"null"), (who, null)
        assert _refused(fn(k=0), who, b"k=0") and _refused(fn(k=9), who, b"k=9")
        assert _refused(fn(N=0), who, b"N=0") and _refused(fn(N=1025), who, b"N=1025")
        assert _refused(fn(T=0), who, b"T=0") and _refused(fn(N=1024, T=1025), who, b"out of range")
        assert _refused(fn(P=0), who, b"pool of 0 rows") and _refused(fn(P=2 ** 31), who, b"pool of")
    assert _refused(plain(P=3), b"pool of 3 rows (k=4)")                     # a pool shorter than k
    assert _refused(per_row(k_row=None), b"alive_knn_search_grouped_k_f16", b"null")


def test_gathers_f16_refuse_bad_arguments():
    L = nat.lib()
    ok = dict(val=1, idx=1, k_row=1, k=4, first=1, weight=1, alpha=1, rows=1, src=1, N=2, T=8, out=1)

    def merge(**kw):
        a = dict(ok, **kw)
        return L.alive_knn_merge_gather_rows_f16(a["val"], a["idx"], a["k"], a["alpha"], a["rows"], a["src"], a["N"], a["T"], a["out"],
                                                 None, None)

    def merge_k(**kw):
        a = dict(ok, **kw)
        return L.alive_knn_merge_gather_rows_k_f16(a["val"], a["idx"], a["k_row"], a["k"], a["alpha"], a["rows"], a["src"], a["N"],
                                                   a["T"], a["out"], None, None)

    def blend(**kw):
        a = dict(ok, **kw)
        return L.alive_knn_blend_gather_rows_f16(a["val"], a["idx"], a["k"], a["first"], a["weight"], a["alpha"], a["rows"], a["src"],
                                                 a["N"], a["T"], a["out"], None)

    def blend_k(**kw):
        a = dict(ok, **kw)
        return L.alive_knn_blend_gather_rows_k_f16(a["val"], a["idx"], a["k_row"], a["k"], a["first"], a["weight"], a["alpha"], a["rows"],
                                                   a["src"], a["N"], a["T"], a["out"], None)
    for fn, who, nulls in ((merge, b"alive_knn_merge_gather_rows_f16", ("val", "idx", "alpha", "rows", "src", "out")),
                           (merge_k, b"alive_knn_merge_gather_rows_k_f16", ("val", "idx", "k_row", "alpha", "rows", "src", "out")),
                           (blend, b"alive_knn_blend_gather_rows_f16", ("val", "idx", "first", "weight", "alpha", "rows", "src", "out")),
                           (blend_k, b"alive_knn_blend_gather_rows_k_f16",
                            ("val", "idx", "k_row", "first", "weight", "alpha", "rows", "src", "out"))):
        for null in nulls:
            assert _refused(fn(**{null: None}), who, b"null"), (who, null)
        assert _refused(fn(k=0), who, b"k=0") and _refused(fn(k=9), who, b"k=9")
        assert _refused(fn(N=0), who, b"empty source") and _refused(fn(T=0), who, b"empty source")


def test_path_rows_f16_refuses_bad_arguments():
    L = nat.lib()
    ok = dict(val=8, idx=16, k_row=1, k_max=4, on=1, weight=1, rows=1, norms=1, P=64, R=2, T=5, out_val=24, out_idx=32, moved=1, ws=1)

    def path(**kw):
        a = dict(ok, **kw)
        return L.alive_knn_path_rows_f16(a["val"], a["idx"], a["k_row"], a["k_max"], a["on"], a["weight"], a["rows"], a["norms"], a["P"],
                                         a["R"], a["T"], a["out_val"], a["out_idx"], a["moved"], a["ws"], None)
    who = b"alive_knn_path_rows_f16"
    for null in ("val", "idx", "out_val", "out_idx"):
        assert _refused(path(**{null: None}), who, b"null lists"), null
    for null in ("k_row", "on", "weight", "moved"):
        assert _refused(path(**{null: None}), who, b"null per-row array"), null
    for null in ("rows", "norms", "ws"):
        assert _refused(path(**{null: None}), who, b"null pointer"), null
    assert _refused(path(k_max=0), who, b"k_max 0 outside [1, 8]") and _refused(path(k_max=9), who, b"k_max 9")
    assert _refused(path(R=0), who, b"empty lists") and _refused(path(T=0), who, b"empty lists")
    assert _refused(path(R=1024, T=1025), who, b"exceeds 2^20 frames")
    assert _refused(path(P=0), who, b"P outside") and _refused(path(P=2 ** 31), who, b"P outside")
    assert _refused(path(out_val=8), who, b"must not be the input lists") and _refused(path(out_idx=16), who, b"must not be")


# ------------------------------------------------------------------------------------------------ VoicePool(dtype=)
def test_voice_pool_takes_fp32_or_fp16_and_nothing_else():
    for bad in (torch.bfloat16, torch.float64, torch.int16, "bf16", None):
        with pytest.raises(ValueError, match="torch.float32 or torch.float16"):
            MS.VoicePool(device="cpu", capacity=8, dtype=bad)
    with pytest.raises(ValueError, match="bfloat16"):                        # the message names what it got
        MS.VoicePool(device="cpu", dtype=torch.bfloat16)
    full = MS.VoicePool(device="cpu", capacity=8)
    half = MS.VoicePool(device="cpu", capacity=8, dtype=torch.float16)
    assert full.dtype == torch.float32 and full.rows.dtype == torch.float32 and full.row_bytes == 3072
    assert half.dtype == torch.float16 and half.rows.dtype == torch.float16 and half.row_bytes == 1536
    assert half.rows.shape == full.rows.shape == (8, 768) and half.norms.dtype == full.norms.dtype == torch.float32
    assert 2 * half.rows.numel() * half.rows.element_size() == full.rows.numel() * full.rows.element_size()
    assert half.rows.data_ptr() % 16 == 0
    assert MS.VoicePool(device="cpu", dtype=torch.float16).row_bytes == 1536 and MS.VoicePool(device="cpu").row_bytes == 3072
    assert MS.VoicePool(device="cpu", capacity=8, dtype="fp16").dtype == torch.float16


def test_wrappers_refuse_a_row_table_of_another_dtype():
    rows = torch.zeros(64, 768, dtype=torch.bfloat16)
    norms, src = torch.zeros(64), torch.zeros(2, 768, 5)
    i32, f64 = torch.zeros(2, dtype=torch.int32), torch.zeros(2, dtype=torch.float64)
    val, idx = torch.zeros(10, 4), torch.zeros(10, 4, dtype=torch.int32)
    first = torch.zeros(3, dtype=torch.int32)
    for call in (lambda: MS.knn_search_grouped(src, rows, norms, i32, i32, 4),
                 lambda: MS.knn_search_grouped_k(src, rows, norms, i32, i32, i32, 4),
                 lambda: MS.merge_gather_rows(val, idx, 4, f64, rows, src),
                 lambda: MS.merge_gather_rows_k(val, idx, i32, 4, f64, rows, src),
                 lambda: MS.blend_gather_rows(val, idx, 4, first, f64, f64, rows, src),
                 lambda: MS.blend_gather_rows_k(val, idx, i32, 4, first, f64, f64, rows, src),
                 lambda: ops.knn_path_rows(val, idx, i32, 4, i32, f64, rows, norms)):
        with pytest.raises(ValueError, match="torch.float32 or torch.float16, got torch.bfloat16"):
            call()


def test_offline_paths_refuse_a_half_pool_and_name_its_dtype():
    from module.pipeline import Converter
    from module.sharded import ShardedConverter
    half = MS.VoicePool(device="cpu", capacity=8, dtype=torch.float16)
    with pytest.raises(ValueError, match=r"VoicePool\.search_images needs an fp32 voice pool.*torch\.float16"):
        half.search_images()
    with pytest.raises(ValueError, match=r"VoicePool\.voice_ids needs an fp32 voice pool.*torch\.float16"):
        half.voice_ids(["a"])
    with pytest.raises(ValueError, match=r"Converter\.convert_many needs an fp32 voice pool.*torch\.float16"):
        Converter.convert_many(object.__new__(Converter), [torch.zeros(16000)], half, ["a"])
    with pytest.raises(ValueError, match=r"ShardedConverter\.convert_many needs an fp32 voice pool.*torch\.float16"):
        ShardedConverter.convert_many(object.__new__(ShardedConverter), [torch.zeros(16000)], half, ["a"])
    with pytest.raises(ValueError, match="torch.float16"):
        MS.knn_pool_workspace_bytes(2, 8, 4, half)
    full = MS.VoicePool(device="cpu", capacity=8)                            # an fp32 pool is asked what it always was
    with pytest.raises(ValueError, match="the voice pool is empty"):
        full.search_images()


# ------------------------------------------------------------------------------------------------ the CLI's flag
def test_pool_dtype_flag_parses_and_defaults_to_fp32():
    import multistream_inference as cli
    p = cli.build_parser()
    assert p.parse_args(["s.json"]).pool_dtype == "fp32"
    assert p.parse_args(["s.json", "--pool-dtype", "fp16"]).pool_dtype == "fp16"
    with pytest.raises(SystemExit):
        p.parse_args(["s.json", "--pool-dtype", "bf16"])
    for extra, dtype, capacity in (([], torch.float32, None), (["--pool-rows", "16"], torch.float32, 16),
                                   (["--pool-dtype", "fp32", "--pool-rows", "16"], torch.float32, 16),
                                   (["--pool-dtype", "fp16"], torch.float16, None),
                                   (["--pool-dtype", "fp16", "--pool-rows", "16"], torch.float16, 16)):
        pool = cli.make_pool(p.parse_args(["s.json"] + extra), "cpu")
        assert pool.dtype == dtype and pool.capacity == capacity, extra
        if capacity is not None:
            assert pool.rows.dtype == dtype and pool.rows.shape == (16, 768)
    assert "--pool-dtype fp16" in cli.__doc__
