"""CPU proofs of what tests/knn_cert_cases.py promises, so that the zero tolerance of tests/test_gpu_knn_cert.py rests on checked
facts: the operands make every sum exact, the parameters are production's, the matrix reaches every form and edge the issue of the
rescoring kernel names, the boundary triples sit at their bounds, the selection pairs at their cuts -- and the model itself gives the
hand-computed answer on a frame small enough to work out on paper."""
import copy
import ctypes
import os
import re

import numpy as np
import pytest

import knn_cert_cases as K

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = K.all_cases()
BY_NAME = {c.name: c for c in CASES}


def is_f32(x):
    x = np.asarray(x, np.float64)
    with np.errstate(over="ignore"):
        return bool(np.all(x.astype(F32).astype(np.float64) == x))


def ran(c):
    return K.expected(c)["frames"]


# ---- operands ------------------------------------------------------------------------------------------------------------------------
def test_norms_are_powers_of_two_and_not_all_one():
    for c in CASES:
        m, _ = np.frexp(c.norms.astype(np.float64))
        assert bool(np.all(m == 0.5)) and bool(np.any(c.norms != 1.0)), c.name
        assert float(c.norms.min()) >= 2.0 ** -2 and float(c.norms.max()) <= 2.0 ** 24


def test_every_score_a_launch_can_compute_is_exact_in_any_order():
    """for every (frame, row) pair a case lists -- candidates and, in collect mode, the joined rows: row / norm is an fp32 number, the 768
    products are multiples of one unit with sum |s| |row / norm| below 2^24 units, the float64 sum is an fp32 number and not zero (a zero
    has two encodings)"""
    for c in CASES:
        for slot in range(c.Tt):
            ft = int(c.frame_list[slot]) if c.frame_list is not None else slot
            if ft < 0:
                continue
            ids = set(int(i) for i in c.cand_idx[slot] if i >= 0)
            if c.collect:
                ids |= set(int(g) - c.idx_base for g in c.out_idx0[ft] if g >= 0)
            ids = sorted(ids)
            if not ids:
                continue
            q = c.rows[ids].astype(np.float64) / c.norms[ids].astype(np.float64)[:, None]
            assert is_f32(q), (c.name, slot)
            terms = q * c.s[ft].astype(np.float64)[None, :]
            sums = terms.sum(axis=1)
            assert is_f32(sums) and bool(np.all(sums != 0)), (c.name, slot)
            nz = np.count_nonzero(terms, axis=1)
            for j in np.nonzero(nz > 1)[0]:                       # (a one-hot frame leaves one term: nothing to add up)
                assert K.sum_units(terms[j]) < 2.0 ** 24, (c.name, slot, ids[j])


def test_ramp_rows_hold_768_different_elements_and_frames_are_not_one_hot():
    ramps = [c for c in CASES if c.name.startswith("ramp")]
    assert len(ramps) >= 2 and {c.list_len for c in ramps} == {8, 16}
    for c in ramps:
        assert all(len(set(r.tolist())) == K.D for r in c.rows)
        assert all(np.count_nonzero(s) >= K.D - 4 for s in c.s)
        assert any(r["chosen"] for r in ran(c))


def test_stage_scores_errors_and_their_sums_are_exact():
    """certify mode, over the candidates the rule rescores: pre * pre_scale, e = pre * pre_scale - score and e^2 are fp32 numbers, the e
    and the e^2 add up exactly in any order (units below 2^24), at most 64 are rescored"""
    seen = 0
    for c in CASES:
        if not c.certify or c.collect:
            continue
        ps = np.float64(c.pre_scale)
        m, _ = np.frexp(ps)
        assert m == 0.5 and F32(c.pre_scale) in (K.PS1, K.PS6, K.PS8)
        for r in ran(c):
            assert len(r["chosen"]) <= 64
            if not r["chosen"]:
                continue
            pre = np.array([np.float64(c.cand_val[r["slot"]][list(c.cand_idx[r["slot"]]).index(i)]) for i, _ in r["chosen"]])
            sc = np.array([np.float64(s) for _, s in r["chosen"]])
            e = pre * ps - sc
            assert is_f32(pre * ps) and is_f32(e) and is_f32(e * e), (c.name, r["slot"])
            assert K.sum_units(e) < 2.0 ** 24 and K.sum_units(e * e) < 2.0 ** 24, (c.name, r["slot"])
            assert float(np.max(np.abs(e))) <= 2.0 ** -5, (c.name, r["slot"])
            seen += 1
    assert seen > 150


def test_only_production_parameters():
    for c in CASES:
        assert float(c.zsig) == 7.0 and F32(c.sd_prior) in (K.SD16, K.SD8, K.SD6, K.SD8R) and F32(c.slack) in (F32(0.0), K.SLACK), c.name
        if c.collect:
            assert 4 <= c.kp <= 64, c.name
        else:
            assert (c.list_len, c.kp) in ((8, 16), (16, 32)) and c.R % c.list_len == 0, c.name
        assert not (c.force_fail is not None and c.thr), c.name
        assert c.det_q is None or c.list_len == 8, c.name
        assert c.M <= 2048 and c.R <= 1024


def test_check_indices_refuses_what_would_fault():
    c = BY_NAME["triples_det"]
    for field, at, value in [("cand_idx", (0, 3), c.M), ("cand_idx", (1, 0), -3)]:
        d = copy.copy(c)
        setattr(d, field, getattr(c, field).copy())
        getattr(d, field)[at] = value
        with pytest.raises(AssertionError):
            K.check_indices(d)
    d = copy.copy(BY_NAME["gate_list_count_3_of_5"])
    d.frame_list = d.frame_list.copy()
    d.frame_list[2] = d.frames
    with pytest.raises(AssertionError):
        K.check_indices(d)
    d = copy.copy(BY_NAME["collect_R64_cap64"])
    d.out_idx0 = d.out_idx0.copy()
    d.out_idx0[0, 0] = d.M
    with pytest.raises(AssertionError):
        K.check_indices(d)


# ---- the matrix ------------------------------------------------------------------------------------------------------------------------
def test_matrix_reaches_every_form_and_edge():
    cert = [c for c in CASES if c.certify and not c.collect]
    shapes = {(c.R, c.list_len) for c in cert}
    for R, L in [(16, 8), (64, 8), (80, 8), (192, 8), (208, 8), (256, 8), (288, 16), (512, 16), (544, 16), (1024, 16), (64, 16), (192, 16)]:
        assert (R, L) in shapes, (R, L)
    assert {c.Tt for c in cert} >= {1, 3, 4, 5, 9}
    assert {c.k for c in cert} >= {1, 2, 3, 4, 8}
    assert any(c.idx_base == 0 for c in cert) and any(c.idx_base > 0 for c in cert)
    assert any(c.flag_cnt0 > 0 for c in cert)
    assert {F32(c.slack) for c in cert if c.thr} == {F32(0.0), K.SLACK}
    frames = [(c, r) for c in cert for r in ran(c)]
    assert any(0 < len(r["chosen"]) < r["k"] for _, r in frames)                          # fewer than k candidates
    assert any(not r["chosen"] and r["c_cut"] == K.NINF and not r["flagged"] for _, r in frames)     # none, no floor: stands
    assert any(not r["chosen"] and r["c_cut"] > K.NINF and r["flagged"] for _, r in frames)          # none, but a seeded list
    assert any(r["why"] == "forced" for _, r in frames) and any(r["why"] == "certificate" for _, r in frames)
    assert any(c.force_fail is not None and c.force_fail[r["frame"]] and r["c_cut"] == K.NINF for c, r in frames)   # forced without a floor
    assert any(r["ranked"] for c, r in frames if c.list_len == 8) and any(r["ranked"] for c, r in frames if c.list_len == 16)
    seeded = [c for c in cert if np.any((c.cand_idx == -1) & np.isfinite(c.cand_val))]
    assert len(seeded) >= 6
    pins = [(c, r) for c, r in frames if c.pins.get(r["slot"])]
    for where in K.WHERE:
        got = [(c, r) for c, r in pins if c.pins[r["slot"]] == where]
        assert len(got) >= 25, where
        assert all(r["flagged"] == (where != "above") or r["why"] == "forced" for _, r in got)
        assert {c.R <= 64 for c, _ in got} == {True, False}
    # pinned frames whose c_cut is a candidate the cut left behind, not a floor
    assert sum(1 for c, r in pins if r["n_left"] > 0 and r["c_cut"] > max(
        [F32(min(c.cand_val[r["slot"]][l:l + c.list_len])) for l in range(0, c.R, c.list_len)])) >= 5
    assert any(c.det_q is not None for c in cert) and any(not c.certify for c in CASES)


def test_pinned_frames_sit_on_their_bounds():
    n = 0
    for c in CASES:
        for r in ran(c):
            where = c.pins.get(r["slot"])
            if where:
                want = {"at": r["bound"], "above": np.nextafter(r["bound"], F32(np.inf)), "below": np.nextafter(r["bound"], K.NINF)}[where]
                assert r["vk"].view(np.uint32) == want.view(np.uint32), (c.name, r["slot"])
                n += 1
    assert n >= 100


def test_boundary_triples_share_everything_but_the_kth_score():
    forms = set()
    for c in CASES:
        if not c.name.startswith("triples"):
            continue
        rs = ran(c)
        assert len(rs) == 3 * len(c.forms)
        for t, form in enumerate(c.forms):
            a, b, d = rs[3 * t:3 * t + 3]
            assert a["bound"].view(np.uint32) == b["bound"].view(np.uint32) == d["bound"].view(np.uint32)
            for key in ("c_cut", "err_mu", "err_sd", "err_max"):
                assert a[key] == b[key] == d[key]
            assert a["vk"] == a["bound"] and b["vk"] == np.nextafter(a["bound"], F32(np.inf)) and d["vk"] == np.nextafter(a["bound"], K.NINF)
            assert (a["flagged"], b["flagged"], d["flagged"]) == (True, False, True)
            assert [i for i, _ in a["chosen"]] == [i for i, _ in b["chosen"]] == [i for i, _ in d["chosen"]]
            diff = np.nonzero(c.cand_val[3 * t] != c.cand_val[3 * t + 1])[0]
            assert len(diff) == 1 and bool(np.all(c.cand_idx[3 * t] == c.cand_idx[3 * t + 1]))          # one stage score differs: the k-th's
            zs, mx2 = F32(K.ZSIG * a["err_sd"]), F32(F32(2.0) * a["err_max"])
            if c.det_q is not None:
                assert a["bound"] == F32(F32(a["c_cut"] * c.pre_scale) + a["det_bound"])
                forms.add("det")
                continue
            mean = sum(np.float64(c.cand_val[3 * t][list(c.cand_idx[3 * t]).index(i)]) * np.float64(c.pre_scale) - np.float64(s) for i, s in a["chosen"])
            if form == "tiny":
                assert a["err_sd"] == F32(c.sd_prior) and zs > mx2
            elif form == "rms":
                assert a["err_sd"] > F32(c.sd_prior) and zs > mx2
            elif form == "max":
                assert mx2 > zs
            elif form == "neg":
                assert a["err_mu"] < 0 and a["bound"] > F32(F32(a["c_cut"] * c.pre_scale) + max(zs, mx2))
            elif form == "pos":
                assert mean > 0 and a["err_mu"] == 0 and a["bound"] == F32(F32(a["c_cut"] * c.pre_scale) + max(zs, mx2))
            forms.add(form)
    assert forms == {"tiny", "rms", "max", "neg", "pos", "det"}


def test_selection_pairs_sit_at_the_cut():
    n = 0
    for c in CASES:
        if not c.name.startswith("selection"):
            continue
        for r in ran(c):
            idx, x, n_above = c.sel[r["slot"]]
            e = list(c.cand_idx[r["slot"]]).index(idx)
            stage = c.cand_val[r["slot"]][e]
            lim = F32(r["sk"] - r["prune"])
            assert stage == (lim if x == "at" else np.nextafter(lim, K.NINF))
            selected = idx in [i for i, _ in r["chosen"]]
            assert selected == (x == "at" or n_above == 15), (c.name, r["slot"])          # 15 within the prune: it is the 16th, kept anyway
            if selected:
                assert r["out_idx"][0] == idx + c.idx_base                                # its exact score is the best of the frame
            else:
                assert idx + c.idx_base not in r["out_idx"].tolist() and r["c_cut"] == stage
            n += 1
    assert n == 16


def test_ranking_cases_switch_paths_at_65():
    for c in CASES:
        if not c.name.startswith("ranking"):
            continue
        for r, (n, where) in zip(ran(c), c.variants):
            stages = sorted((float(v) for v, i in zip(c.cand_val[r["slot"]], c.cand_idx[r["slot"]]) if i >= 0), reverse=True)
            if n == 64:
                assert not r["ranked"] and len(r["chosen"]) == 64
            elif n == 65:
                assert r["ranked"] and len(r["chosen"]) == 64 and float(r["c_cut"]) == stages[64]     # the one entry left behind
                assert len(set(stages[:66])) == 66
            else:
                tied = sorted(int(i) for v, i in zip(c.cand_val[r["slot"]], c.cand_idx[r["slot"]]) if i >= 0 and v == F32(0.625 / float(c.pre_scale)))
                assert r["ranked"] and len(r["chosen"]) == 16 and len(tied) == 52
                assert [i for i, _ in r["chosen"] if i in tied] == [tied[0]] and float(r["c_cut"]) == 0.625 / float(c.pre_scale)
                lanes = [e % 64 for e, (v, i) in enumerate(zip(c.cand_val[r["slot"]], c.cand_idx[r["slot"]])) if i in tied]
                assert len(set(lanes)) == 52


def test_collect_cases_overflow_exactly_where_the_lanes_run_out():
    seen = set()
    for c in CASES:
        if not c.collect:
            continue
        for r, (n, marker, present, new, _) in zip(ran(c), c.slots):
            over = marker or n > 64 or new > 64 - min(n, 64)
            assert r["flagged"] == over and (r["why"] == "overflow") == over, (c.name, r["slot"])
            seen.add(("marker", marker and c.R <= 64) if marker else ("rows", n) if n > 64 else ("exact", new) if new and new == 64 - n else ("short", 1) if new == 65 - n else
                     ("present", present == c.k) if new == 0 and n <= 64 else ("rows", n))
            if not over:
                joined = [i for i, _ in r["chosen"]]
                assert len(joined) == len(set(joined)) == n + new
    assert {("marker", True), ("short", 1), ("rows", 65), ("present", True)} <= seen
    assert {("exact", j) for j in (1, 2, 3, 4, 7, 8)} <= seen


def test_tie_cases_hold_equal_scores_across_the_kth_place():
    n = 0
    for c in CASES:
        if not c.name.startswith("ties"):
            continue
        for r in ran(c):
            tied = c.tied[r["slot"]]
            scores = {i: s for i, s in r["chosen"]}
            assert len(tied) == 5 and all(scores[i] == F32(0.75) for i in tied)
            assert r["out_idx"][-2:].tolist() == [c.idx_base + tied[0], c.idx_base + tied[1]] and r["runner_up"] == F32(0.75)
            pos = [list(c.cand_idx[r["slot"]]).index(i) for i in tied]
            n += pos != sorted(pos)                               # index order is not list order
    assert n >= 6


def test_gate_cases_run_what_the_gate_rule_says():
    want = {"count_closed_at_lo": 0, "count_open_above_lo": 5, "count_open_at_hi": 5, "count_closed_above_hi": 0, "bool_closed": 0,
            "bool_open": 5, "bool_open_negative": 5, "list_count_3_of_5": 3, "list_count_closed_at_lo": 0, "list_count_open_at_hi": 5,
            "list_count_closed_above_hi": 0, "zero_count_mode_gate": 5, "one_count_mode_gate": 0}
    for name, n in want.items():
        c = BY_NAME["gate_" + name]
        ex = K.expected(c)
        assert len(ex["frames"]) == n
        if c.frame_list is not None:
            assert [r["frame"] for r in ex["frames"]] == c.frame_list[:n].tolist() and len(set(c.frame_list.tolist())) == 5 < c.frames
        if n == 0:
            assert bool(np.all(ex["out_val"].view(np.uint32) == K.SENT)) and ex["flag_cnt"] == c.flag_cnt0


def test_pool_cases_fail_one_whole_group_and_none_of_the_other():
    for c in CASES:
        if not c.pool:
            continue
        ex = K.expected(c)
        g0 = [s for s in range(c.Tt) if c.pool["slot_grp"][s] == 0 and c.frame_list[s] >= 0]
        assert sorted(ex["fails"][0]) == g0 and ex["fails"][1] == [] and ex["flag_cnt"] == len(g0)
        assert [g["k"] for g in c.pool["groups"]] == [2, 8] and c.k == 8 and len(set(c.det_lib.tolist())) == 2
        assert -1 in c.frame_list[5:8].tolist()
        for r in ex["frames"]:
            assert len(r["out_val"]) == r["k"]
            assert bool(np.all(ex["out_val"][r["frame"], r["k"]:].view(np.uint32) == K.SENT))


# ---- the model on a frame worked out by hand ---------------------------------------------------------------------------------------------
def test_model_on_a_hand_computed_frame():
    """R = 16 (two lists of 8), k = 2, pre_scale 1, sd_prior 1.5e-3.  List 0 is full: stage scores 0.75, 0.5, 0.625 and five at 0.5625; list
    1 holds one entry at 0.25.  Errors: +2^-8 on the first, -2^-8 on the second, 0 elsewhere.  Nine candidates < 16, so all are rescored;
    the floor is list 0's minimum 0.5; mean e = 0, mean e^2 = 2 * 2^-16 / 9."""
    b = K.Board(1, 64, 1)
    fb = K.FrameBuilder(b, 0, 16, 8, 1.0)
    stages = [0.75, 0.5, 0.625] + [0.5625] * 5
    errs = [2.0 ** -8, -(2.0 ** -8)] + [0.0] * 6
    ids = [fb.put(e, st - er, er, idx=10 + e) for e, (st, er) in enumerate(zip(stages, errs))]
    fb.put(9, 0.25, 0.0, idx=3)
    s, rows, norms = b.arrays()
    c = K.Case("hand", P=1, kp=16, list_len=8, k=2, Tt=1, frames=1, M=64, pre_scale=K.PS1, sd_prior=K.SD8, s=s, rows=rows, norms=norms,
               cand_val=fb.cv[None], cand_idx=fb.ci[None], out_idx0=np.full((1, 2), K.SENT, np.int32), thr=True, idx_base=100)
    r = K.model_frame(c, 0, 0, 2, 0, c.out_idx0[0])
    assert r["c_cut"] == F32(0.5) and len(r["chosen"]) == 9 and r["err_mu"] == 0 and r["err_max"] == F32(2.0 ** -8)
    sd = F32(np.sqrt(F32(F32(2.0 ** -15) / F32(9.0))))
    assert r["err_sd"] == sd and sd > K.SD8
    bound = F32(F32(0.5) + F32(F32(7.0) * sd))                       # 7 sd = 0.0129 > 2 max = 0.0078
    assert r["bound"] == bound
    # exact scores: 0.75 - 2^-8 = 0.74609375 (row 10), 0.625 (row 12), 0.5625 (rows 13 ..), 0.5 + 2^-8 (row 11)
    assert r["out_val"].tolist() == [0.74609375, 0.625] and r["out_idx"].tolist() == [110, 112]
    assert not r["flagged"] and r["vk"] > bound
    c.k = 8                                                           # the eighth best is 0.50390625 < bound: flagged, ties by index
    r = K.model_frame(c, 0, 0, 8, 0, np.full(8, K.SENT, np.int32))
    assert r["out_idx"].tolist() == [110, 112, 113, 114, 115, 116, 117, 111] and r["flagged"] and r["why"] == "certificate"
    assert r["thr"] == F32(F32(F32(0.50390625) - F32(bound - F32(0.5))) / F32(1.0))


def test_realistic_seed_stays_within_the_cap():
    c = K.realistic()
    K.check_indices(c)
    ex = K.expected(c)
    inside = [r["frame"] for r in ex["frames"] if abs(float(r["vk"]) - float(r["bound"])) <= K.real_margin(r, c.pre_scale)]
    assert len(inside) <= K.REAL_CAP * c.Tt, inside
    assert 0 < len(ex["flagged"]) and all(len(r["chosen"]) >= 16 for r in ex["frames"])
    # the lists are what a stage leaves: every row of a quarter that is not listed scores at or below the list's floor
    assert c.cand_idx.min() >= 0 and all(len(set(row.tolist())) == c.R for row in c.cand_idx)


# ---- the entries ---------------------------------------------------------------------------------------------------------------------
def test_entries_are_declared_bound_and_laid_out_alike():
    from module import _native as nat
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    body = re.search(r"typedef struct AliveRescoreArgs \{(.*?)\} AliveRescoreArgs;", hdr, re.S).group(1)
    fields = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        kind = ctypes.c_void_p if "*" in decl else ctypes.c_int64 if decl.startswith("int64_t") else ctypes.c_float if decl.startswith("float") else ctypes.c_int
        for name in decl.replace("*", " ").split(None, 2 if decl.startswith(("const", "unsigned")) else 1)[-1].replace("char", "").split(","):
            fields.append((name.strip(), kind))
    assert fields == list(nat.AliveRescoreArgs._fields_)
    for name, nargs in (("alive_debug_knn_rescore", 2), ("alive_debug_knn_rescore_pool", 7), ("alive_debug_knn_pool_fields", 2)):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl is not None and len(decl.group(1).split(",")) == nargs == len(nat.PROTOTYPES[name][1]), name
    src = open(os.path.join(ROOT, "alive-vc_amd", "module", "_native.py")).read()
    for name in ("alive_debug_knn_rescore", "alive_debug_knn_rescore_pool", "alive_debug_knn_pool_fields"):
        assert re.search(r'"' + name + r'":.*# test only', src), name
