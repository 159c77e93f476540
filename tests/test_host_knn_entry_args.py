"""CPU tests: the argument-check contract of every kNN search entry of the C ABI.  Each case hands an entry ONE thing it must refuse --
a required pointer null, k = 0 or one above the entry's limit, fewer rows than k, a frame count at the limit, a form's own operand
missing -- and expects ALIVE_ERR_ARG with the message body of that check under the name of the entry that was called.  Pointers are
fake (small integers, as in test_host_logic.py::test_argument_errors_are_reported_without_a_gpu): every case fails a check before
anything is dereferenced or launched, and no case is a call that would pass the checks."""
import ctypes as C

import pytest

from module import _native as nat

PTR = 8                    # a fake non-null pointer
MAX_K, KH = 64, 8          # ALIVE_MAX_K (include/alive_vc.h); the tiered / grouped / pool searches' and the rescoring kernel's k limit
FRAMES = (1 << 31) - 384   # the first N * T the tiered searches refuse
ERR_ARG = -1


def _p(*names):
    return [(n, PTR) for n in names]


_SHAPE = [("N", 2), ("T", 100)]
_TAIL = [("M", 1000), ("idx_base", 0), ("k", 4)] + _p("out_val", "out_idx", "ws") + [("stream", None)]
_EV = [("ev_start", None), ("ev_stop", None)]
_BF16 = _p("src") + _SHAPE + _p("lib_bf16", "rows_f32", "norms") + _TAIL
_STAGE = _p("src") + _SHAPE + _p("lib_stage", "lib_bf16", "rows_f32", "norms") + _TAIL

# entry -> (arguments in call order with a good value each, {optional pointer or own message: body})
NAMED = {
    "alive_knn_search": (_BF16, {}),
    "alive_knn_search_timed": (_BF16 + _EV, {}),
    "alive_knn_search_strict": (_p("src") + _SHAPE + _p("lib_bf16", "lib_lo", "rows_f32", "norms", "bound") + _TAIL + _EV,
                                {"lib_lo": None, "bound": "null bound (alive_library_rounding_bound)"}),
    "alive_knn_search_fp8": (_STAGE, {}),
    "alive_knn_search_fp8_timed": (_STAGE + _EV, {}),
    "alive_knn_search_fp6": (_STAGE, {}),
    "alive_knn_search_fp6_timed": (_STAGE + _EV, {}),
    "alive_knn_search_fp8_rot_timed": (_p("src", "y_rot") + [("c0", 0.5)] + _SHAPE + _p("lib_stage", "lib_bf16", "rows_f32", "norms") + _TAIL + _EV,
                                       {"y_rot": "null rotated frames"}),
    "alive_knn_search_fp6_sub_timed": (_p("src", "y_sub") + _SHAPE + _p("lib_sub", "rho", "lib_stage", "lib_bf16", "rows_f32", "norms") + _TAIL + _EV,
                                       dict.fromkeys(("y_sub", "lib_sub", "rho"), "null subspace operand")),
}

_GROUPED = _p("src") + [("N", 3), ("T", 20)] + _p("rows", "norms") + [("P", 1000)] + _p("seg_lo", "seg_len")
_OUT = _p("out_val", "out_idx", "ws") + [("stream", None)]
GROUPED = {name: _GROUPED + (_p("k_row") if "grouped_k" in name else []) + [("k", 4)] + _OUT
           for name in ("alive_knn_search_grouped", "alive_knn_search_grouped_k", "alive_knn_search_grouped_f16", "alive_knn_search_grouped_k_f16")}

_POOL = (_p("src") + [("N", 3), ("T", 20)] + _p("images", "img_off", "rows", "norms", "bounds") + [("P", 1000)] + _p("seg_lo", "seg_len") +
         [("V", 2), ("max_len", 600)] + _p("voice"))
POOL = {name: _POOL + (_p("k_row") if name.endswith("_k") else []) + [("k", 4)] + _OUT for name in ("alive_knn_search_pool", "alive_knn_search_pool_k")}

GATHER = {}
for _f16 in ("", "_f16"):
    for _k in ("", "_k"):
        _head = _p("cand_val", "cand_idx") + (_p("k_row") if _k else []) + [("k", 4)]
        _src = _p("rows", "src") + [("N", 3), ("T", 20)] + _p("out")
        GATHER["alive_knn_merge_gather_rows" + _k + _f16] = _head + _p("alpha") + _src + [("final_idx", None), ("stream", None)]
        GATHER["alive_knn_blend_gather_rows" + _k + _f16] = _head + _p("first", "weight", "alpha") + _src + [("stream", None)]


def _refused(entry, call, body):
    rc = call()
    msg = nat.lib().alive_last_error().decode()
    assert rc == ERR_ARG, (entry, rc, msg)
    assert body in msg, (entry, body, msg)
    assert msg.startswith(entry + ":"), (entry, msg)           # the message names the entry that was called


def _positional(entry, spec, **change):
    return lambda: getattr(nat.lib(), entry)(*[change.get(n, v) for n, v in spec])


def _pointer_cases(spec, own):
    for n, v in spec:
        if v == PTR and own.get(n, "null pointer") is not None:
            yield n, {n: None}, own.get(n, "null pointer")


def _cases():
    for entry, (spec, own) in NAMED.items():
        extra = [("k=0", {"k": 0}, f"k=0 outside [1,{MAX_K}]"), ("k above", {"k": MAX_K + 1}, f"k={MAX_K + 1} outside [1,{MAX_K}]"),
                 ("M < k", {"M": 3}, "library shard has 3 vectors, fewer than k=4"),
                 ("frames", {"N": 1, "T": FRAMES}, f"{FRAMES} frames in one call")]
        for label, change, body in list(_pointer_cases(spec, own)) + extra:
            yield pytest.param(entry, _positional(entry, spec, **change), body, id=f"{entry}-{label}")
    for entry, spec in GROUPED.items():
        few = ({"P": 0}, "pool of 0 rows (k=4)") if "grouped_k" in entry else ({"P": 3}, "pool of 3 rows (k=4)")
        extra = [("k=0", {"k": 0}, f"k=0 outside [1,{KH}]"), ("k above", {"k": KH + 1}, f"k={KH + 1} outside [1,{KH}]"), ("M < k",) + few,
                 ("frames", {"N": 1, "T": (1 << 20) + 1}, f"T={(1 << 20) + 1} out of range")]
        for label, change, body in list(_pointer_cases(spec, {})) + extra:
            yield pytest.param(entry, _positional(entry, spec, **change), body, id=f"{entry}-{label}")
    for entry, spec in POOL.items():
        extra = [("k=0", {"k": 0}, f"k=0 outside [1,{KH}]"), ("k above", {"k": KH + 1}, f"k={KH + 1} outside [1,{KH}]"),
                 ("M < k", {"P": 0}, "V=2 voices, pool of 0 rows"),
                 ("frames", {"N": 1, "T": (1 << 20) + 1}, f"N*T={(1 << 20) + 1} outside [1,{1 << 20}]")]
        for label, change, body in list(_pointer_cases(spec, {})) + extra:
            yield pytest.param(entry, _positional(entry, spec, **change), body, id=f"{entry}-{label}")
    for entry, spec in GATHER.items():
        extra = [("k=0", {"k": 0}, "k=0 outside [1,8]"), ("k above", {"k": 9}, "k=9 outside [1,8]")]
        for label, change, body in list(_pointer_cases(spec, {})) + extra:
            yield pytest.param(entry, _positional(entry, spec, **change), body, id=f"{entry}-{label}")


@pytest.mark.parametrize("entry,call,body", list(_cases()))
def test_positional_entry_refuses(entry, call, body):
    _refused(entry, call, body)


# ---- alive_knn_search_unit: one record, six forms ----
_UNIT = dict(N=2, T=100, k=4, src=PTR, lib_stage=PTR, lib_bf16=PTR, lib_lo=None, rows_f32=PTR, norms=PTR, rows_hat=PTR, bound=PTR, y=PTR,
             lib_sub=PTR, rho=PTR, sub_w=None, rot_c0=0.5, M=1000, idx_base=0, out_val=PTR, out_idx=PTR, ws=PTR, ev_start=None, ev_stop=None)
_UNIT_PTRS = ("src", "lib_bf16", "rows_f32", "norms", "out_val", "out_idx", "ws")
_UNIT_OWN = {nat.KNN_STRICT: {"bound": "strict form without a bound (alive_library_rounding_bound)"},
             nat.KNN_FP8_ROT: {"y": "rotated form without the rotated frames"},
             nat.KNN_FP6_SUB: dict.fromkeys(("y", "lib_sub", "rho"), "null subspace operand")}     # (y null: sub_w is null too)


def _unit(form, **change):
    def call():
        a = nat.AliveKnnSearch(form=form, **{**_UNIT, **change})
        return nat.lib().alive_knn_search_unit(C.byref(a), None)
    return call


def _unit_cases():
    for form in range(6):
        stage = ("lib_stage",) if form >= nat.KNN_FP8 else ()
        cases = [(n, {n: None}, "null pointer") for n in _UNIT_PTRS + stage]
        cases += [(n, {n: None}, body) for n, body in _UNIT_OWN.get(form, {}).items()]
        cases += [("k=0", {"k": 0}, f"k=0 outside [1,{MAX_K}]"), ("k above", {"k": MAX_K + 1}, f"k={MAX_K + 1} outside [1,{MAX_K}]"),
                  ("M < k", {"M": 3}, "library shard has 3 vectors, fewer than k=4"),
                  ("frames", {"N": 1, "T": FRAMES}, f"{FRAMES} frames in one call")]
        for label, change, body in cases:
            yield pytest.param(_unit(form, **change), body, id=f"form{form}-{label}")
    yield pytest.param(_unit(6), "form 6", id="form6")
    yield pytest.param(lambda: nat.lib().alive_knn_search_unit(None, None), "null arguments", id="no-record")


@pytest.mark.parametrize("call,body", list(_unit_cases()))
def test_unit_entry_refuses(call, body):
    _refused("alive_knn_search_unit", call, body)


# ---- the rescoring kernel's debug entries ----
_RESCORE = dict(cand_val=PTR, cand_idx=PTR, P=2, kp=16, s_f32=PTR, rows=PTR, norms=PTR, M=1000, frames=64, Tt=64, idx_base=0, k=4, out_val=PTR,
                out_idx=PTR, frame_list=PTR, gate_cnt=None, gate_lo=0, gate_hi=64, flag_list=PTR, flag_cnt=PTR, zsig=7.0, list_len=8,
                pre_scale=1.0, sd_prior=1e-4, det_q=None, det_lib=None, thr_list=None, collect=0, overflow_slack=0.0, force_fail=None)
_RESCORE_PTRS = ("cand_val", "cand_idx", "s_f32", "rows", "norms", "out_val", "out_idx")
_PLAN = dict(slot_grp=PTR, grp=PTR, gfail=PTR, fb=PTR)


def _rescore(pool, plan=None, **change):
    def call():
        a = nat.AliveRescoreArgs(**{**_RESCORE, **change})
        if not pool:
            return nat.lib().alive_debug_knn_rescore(C.byref(a), None)
        q = {**_PLAN, **(plan or {})}
        return nat.lib().alive_debug_knn_rescore_pool(C.byref(a), q["slot_grp"], q["grp"], q["gfail"], q["fb"], 1, None)
    return call


def _rescore_cases():
    for pool, entry in ((False, "alive_debug_knn_rescore"), (True, "alive_debug_knn_rescore_pool")):
        cases = [(n, {n: None}, "null pointer") for n in _RESCORE_PTRS]
        cases += [("k=0", {"k": 0}, f"k=0 outside [1,{KH}]"), ("k above", {"k": KH + 1}, f"k={KH + 1} outside [1,{KH}]"),
                  ("frames", {"Tt": 1 << 31, "frames": 1 << 31}, f"Tt={1 << 31}")]
        for label, change, body in cases:
            yield pytest.param(entry, _rescore(pool, **change), body, id=f"{entry}-{label}")
    for n in _PLAN:            # the pool form's own operands, behind a record that passes the shared checks
        yield pytest.param("alive_debug_knn_rescore_pool", _rescore(True, plan={n: None}), "null pointer or no group", id=f"pool-plan-{n}")


@pytest.mark.parametrize("entry,call,body", list(_rescore_cases()))
def test_rescore_entry_refuses(entry, call, body):
    _refused(entry, call, body)
