"""knn_rescore_kernel (csrc/knn.hip) -- the kernel every kNN search ends in -- against the rule as tests/knn_cert_cases.py states it,
bit for bit: the cases run through alive_debug_knn_rescore / alive_debug_knn_rescore_pool, which launch the searches' own dispatchers
(rescore_launch / pool_rescore_launch) on the buffers given here, so the register form (PER 0 / 3 / 4 / 8 / 16) is production's choice.
Every operand is exact (knn_cert_cases' docstring; tests/test_host_knn_cert.py proves it), so the tolerance is zero: out_val bits,
out_idx, the set of flagged frames with the bits of their thresholds, flag_cnt, the pool form's gfail / fb.  Every output buffer lies
between two guard bands and is filled with a sentinel: entries the rule does not write, rows of frames that did not run and the bands
must keep it.  Before a launch check_indices (knn_cert_cases) verifies every index array of the case; nothing is launched otherwise.
The one realistic case (Gaussian data, fp8-like stage scores) has the tolerances derived in knn_cert_cases.  Needs an MI355X."""
import ctypes as C

import numpy as np
import pytest
import torch

import knn_cert_cases as K
from module import _native as nat

pytestmark = pytest.mark.gpu
DEV = "cuda"
BAND = 1024               # words per guard band
GUARD = K.SENT
CASES = K.all_cases()


class Guarded:
    """a device buffer of 32-bit words between two guard bands, everything filled with the sentinel (or with `init`)"""

    def __init__(self, words, init=None):
        self.n = int(words)
        self.buf = torch.full((2 * BAND + self.n,), GUARD, dtype=torch.int32, device=DEV)
        if init is not None:
            self.buf[BAND:BAND + self.n] = torch.from_numpy(np.ascontiguousarray(init).view(np.int32).ravel()).to(DEV)

    def ptr(self):
        return self.buf.data_ptr() + 4 * BAND

    def body(self):
        return self.buf[BAND:BAND + self.n].cpu().numpy()

    def bands_intact(self):
        return bool((self.buf[:BAND] == GUARD).all()) and bool((self.buf[BAND + self.n:] == GUARD).all())


def dev(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def pool_fields():
    w = (C.c_int32 * 4)()
    nat.check(nat.lib().alive_debug_knn_pool_fields(w, 4), "alive_debug_knn_pool_fields")
    return dict(fields=w[0], voice=w[1], blk0=w[2], k=w[3])


def launch(c):
    """run the case; returns the output buffers (Guarded) by name"""
    K.check_indices(c)                                   # refuses to launch on an index outside its array
    ins = dict(cv=dev(c.cand_val), ci=dev(c.cand_idx), s=dev(c.s), rows=dev(c.rows), norms=dev(c.norms), fl=dev(c.frame_list),
               dq=dev(c.det_q), dl=dev(c.det_lib), ff=dev(c.force_fail),
               gate=dev(np.array([c.gate[1]], np.int32)) if c.gate else None)
    certify_or_collect = c.certify or c.collect
    out = dict(out_val=Guarded(c.frames * c.k), out_idx=Guarded(c.frames * c.k, c.out_idx0))
    if certify_or_collect:
        out["flag_list"] = Guarded(c.flag_cnt0 + c.Tt)
        out["flag_cnt"] = Guarded(1, np.array([c.flag_cnt0], np.int32))
    if c.thr:
        out["thr_list"] = Guarded(c.flag_cnt0 + c.Tt)
    a = nat.AliveRescoreArgs()
    a.cand_val, a.cand_idx, a.P, a.kp = nat.ptr(ins["cv"]), nat.ptr(ins["ci"]), c.P, c.kp
    a.s_f32, a.rows, a.norms = nat.ptr(ins["s"]), nat.ptr(ins["rows"]), nat.ptr(ins["norms"])
    a.M, a.frames, a.Tt, a.idx_base, a.k = c.M, c.frames, c.Tt, c.idx_base, c.k
    a.out_val, a.out_idx = out["out_val"].ptr(), out["out_idx"].ptr()
    a.frame_list, a.gate_cnt = nat.ptr(ins["fl"]), nat.ptr(ins["gate"])
    a.gate_lo, a.gate_hi = (c.gate[2], c.gate[3]) if c.gate else (0, 0)
    a.flag_list = out["flag_list"].ptr() if certify_or_collect else None
    a.flag_cnt = out["flag_cnt"].ptr() if certify_or_collect else None
    a.zsig, a.list_len, a.pre_scale, a.sd_prior = float(c.zsig), c.list_len, float(c.pre_scale), float(c.sd_prior)
    a.det_q, a.det_lib = nat.ptr(ins["dq"]), nat.ptr(ins["dl"])
    a.thr_list = out["thr_list"].ptr() if c.thr else None
    a.collect, a.overflow_slack, a.force_fail = c.collect, float(c.slack), nat.ptr(ins["ff"])
    if c.pool:
        f = pool_fields()
        grp = np.full((len(c.pool["groups"]), f["fields"]), -77, np.int32)
        for g, rec in enumerate(c.pool["groups"]):
            grp[g, f["voice"]], grp[g, f["blk0"]], grp[g, f["k"]] = rec["voice"], rec["blk0"], rec["k"]
        ins["sg"], ins["grp"] = dev(c.pool["slot_grp"]), dev(grp)
        out["gfail"] = Guarded(len(c.pool["groups"]), np.zeros(len(c.pool["groups"]), np.int32))
        out["fb"] = Guarded(256 * c.pool["fb_blocks"])
        nat.check(nat.lib().alive_debug_knn_rescore_pool(C.byref(a), nat.ptr(ins["sg"]), nat.ptr(ins["grp"]), out["gfail"].ptr(),
                                                         out["fb"].ptr(), len(c.pool["groups"]), nat.stream()), c.name)
    else:
        nat.check(nat.lib().alive_debug_knn_rescore(C.byref(a), nat.stream()), c.name)
    torch.cuda.synchronize()
    return out


def frame_note(c, r):
    return (f"case {c.name}, slot {r['slot']}, frame {r['frame']}: model c_cut {r['c_cut']!r}, bound {r['bound']!r}, vk {r['vk']!r}, "
            f"err_mu {r['err_mu']!r}, err_sd {r['err_sd']!r}, err_max {r['err_max']!r}, {len(r['chosen'])} rescored, pin {c.pins.get(r['slot'])}")


@pytest.mark.parametrize("c", CASES, ids=[c.name for c in CASES])
def test_rescore_matches_the_rule_bit_for_bit(c):
    ex = K.expected(c)
    out = launch(c)
    for name, g in out.items():
        assert g.bands_intact(), f"case {c.name}: a guard band of {name} was written"
    notes = {r["frame"]: frame_note(c, r) for r in ex["frames"]}
    got_val = out["out_val"].body().view(np.uint32).reshape(c.frames, c.k)
    got_idx = out["out_idx"].body().reshape(c.frames, c.k)
    want_val, want_idx = ex["out_val"].view(np.uint32), ex["out_idx"]
    for ft in range(c.frames):
        note = notes.get(ft, f"case {c.name}, frame {ft} (did not run: its rows must keep what they held)")
        assert got_val[ft].tolist() == want_val[ft].tolist(), f"out_val bits {got_val[ft].view(np.float32)} != {want_val[ft].view(np.float32)}; {note}"
        assert got_idx[ft].tolist() == want_idx[ft].tolist(), f"out_idx {got_idx[ft]} != {want_idx[ft]}; {note}"
    if "flag_cnt" not in out:
        return
    cnt = int(out["flag_cnt"].body()[0])
    why = {r["frame"]: r["why"] for r in ex["frames"] if r["flagged"]}
    if c.pool:
        gfail, fb = out["gfail"].body(), out["fb"].body()
        for g, rec in enumerate(c.pool["groups"]):
            lo = rec["blk0"] * 256
            want = sorted(ex["fails"][g])
            assert int(gfail[g]) == len(want), f"case {c.name}: group {g} counts {gfail[g]} failing frames, the rule {want}; " + \
                "; ".join(notes[int(c.frame_list[s])] for s in range(c.Tt) if c.pool["slot_grp"][s] == g and c.frame_list[s] >= 0)
            assert sorted(fb[lo:lo + len(want)].tolist()) == want, f"case {c.name}: group {g} lists {fb[lo:lo + len(want)]}, the rule {want}"
            fb[lo:lo + len(want)] = np.int32(GUARD)
        assert bool(np.all(fb == np.int32(GUARD))), f"case {c.name}: fb written outside the groups' ranges"
        assert bool(np.all(out["flag_list"].body() == np.int32(GUARD))), f"case {c.name}: the pool form wrote flag_list"
        assert cnt == ex["flag_cnt"], f"case {c.name}: flag_cnt {cnt} != {ex['flag_cnt']}"
        return
    fl = out["flag_list"].body()
    n0, n1 = c.flag_cnt0, min(max(cnt, c.flag_cnt0), c.flag_cnt0 + c.Tt)
    thr = out["thr_list"].body().view(np.uint32) if c.thr else None
    got = sorted(((int(fl[p]), int(thr[p]) if c.thr else None) for p in range(n0, n1)), key=lambda x: (x[0], x[1] or 0))
    want = ex["flagged"]
    if got != want:
        diff = sorted({f for f, _ in got} ^ {f for f, _ in want}) or sorted(f for (f, t), (_, u) in zip(got, want) if t != u)
        show = lambda lst: [(f, None if t is None else float(np.uint32(t).view(np.float32))) for f, t in lst]
        raise AssertionError(f"case {c.name}: flagged (frame, threshold) {show(got)} != the rule's {show(want)} ({why}); "
                             + "; ".join(notes.get(f, f"frame {f} did not run") for f in diff))
    assert cnt == ex["flag_cnt"], f"case {c.name}: flag_cnt {cnt} != {ex['flag_cnt']}"
    assert bool(np.all(fl[:n0] == np.int32(GUARD))) and bool(np.all(fl[n1:] == np.int32(GUARD))), f"case {c.name}: flag_list written outside [{n0}, {n1})"
    if c.thr:
        assert bool(np.all(thr[:n0] == GUARD)) and bool(np.all(thr[n1:] == GUARD)), f"case {c.name}: thr_list written outside [{n0}, {n1})"


def test_entries_refuse_bad_arguments_before_launching():
    c = next(x for x in CASES if x.name.startswith("triples_tiny"))
    a = nat.AliveRescoreArgs()
    bufs = [dev(c.cand_val), dev(c.cand_idx), dev(c.s), dev(c.rows), dev(c.norms)]
    outs = [Guarded(c.frames * c.k), Guarded(c.frames * c.k), Guarded(c.Tt), Guarded(1, np.zeros(1, np.int32))]

    def fresh():
        a.cand_val, a.cand_idx, a.s_f32, a.rows, a.norms = [nat.ptr(b) for b in bufs]
        a.out_val, a.out_idx, a.flag_list, a.flag_cnt = [g.ptr() for g in outs]
        a.P, a.kp, a.M, a.frames, a.Tt, a.idx_base, a.k = c.P, c.kp, c.M, c.frames, c.Tt, 0, c.k
        a.frame_list = a.gate_cnt = a.det_q = a.det_lib = a.thr_list = a.force_fail = None
        a.gate_lo = a.gate_hi = a.collect = 0
        a.zsig, a.list_len, a.pre_scale, a.sd_prior, a.overflow_slack = 7.0, c.list_len, 1.0, 8.0e-5, 0.0
    bad = [("k", 0), ("k", 9), ("P", 65), ("list_len", 12), ("list_len", 16), ("gate_lo", K.GATE_BOOL), ("gate_lo", 3), ("Tt", c.frames + 1),
           ("cand_idx", None), ("flag_cnt", None), ("det_q", 1)]
    for field, value in bad:
        fresh()
        if field == "list_len" and value == 16:
            a.P, a.kp = 3, 8                                  # 24 candidates are not whole lists of 16
        if field == "det_q":
            value = nat.ptr(bufs[4])                          # det_q without det_lib
        setattr(a, field, value)
        assert nat.lib().alive_debug_knn_rescore(C.byref(a), nat.stream()) != 0, (field, value)
    fresh()
    assert nat.lib().alive_debug_knn_rescore_pool(C.byref(a), None, None, None, None, 1, nat.stream()) != 0      # no frame_list, no plan
    torch.cuda.synchronize()
    for g in outs[:3]:
        assert bool(np.all(g.body() == np.int32(GUARD))) and g.bands_intact()


def test_realistic_case_within_its_derived_tolerances():
    """Gaussian data: values within 2e-6, the verdict wherever |vk - bound| exceeds the margin (knn_cert_cases' docstring)"""
    c = K.realistic()
    ex = K.expected(c)
    out = launch(c)
    for name, g in out.items():
        assert g.bands_intact(), name
    got_val = out["out_val"].body().view(np.float32).reshape(c.frames, c.k)
    got_idx = out["out_idx"].body().reshape(c.frames, c.k)
    cnt = int(out["flag_cnt"].body()[0])
    flagged = set(out["flag_list"].body()[:cnt].tolist())
    assert len(flagged) == cnt <= c.Tt
    inside = 0
    for r in ex["frames"]:
        ft = r["frame"]
        err = float(np.max(np.abs(got_val[ft].astype(np.float64) - r["out_val"].astype(np.float64))))
        margin, gap = K.real_margin(r, c.pre_scale), abs(float(r["vk"]) - float(r["bound"]))
        print(f"frame {ft}: value error {err:.3e}, |vk - bound| {gap:.3e}, margin {margin:.3e}, model flagged {r['flagged']}, kernel {ft in flagged}")
        assert err <= K.COS_TOL, f"frame {ft}: values {got_val[ft]} against {r['out_val']}"
        clear = np.diff(np.concatenate([r["out_val"].astype(np.float64), [float(r["runner_up"])]])) < -2 * K.COS_TOL
        for j in range(c.k):                                  # a place whose neighbours are clearly apart holds the model's row
            if (j == 0 or clear[j - 1]) and clear[j]:
                assert got_idx[ft, j] == r["out_idx"][j], f"frame {ft}, place {j}: row {got_idx[ft, j]} != {r['out_idx'][j]}"
        if gap > margin:
            assert (ft in flagged) == r["flagged"], f"frame {ft}: verdict {ft in flagged}; {frame_note(c, r)}"
        else:
            inside += 1
    assert inside <= K.REAL_CAP * c.Tt
