"""The candidate stages of the kNN search (csrc/knn.hip: knn_score_kernel, knn_score8_kernel, knn_score6_kernel, knn_sub6_kernel)
against exact arithmetic on their own operand codes.

The search returns exact lists whatever its first stage does -- a frame with a bad candidate set fails its certificate and is searched
again -- so no comparison of the returned lists can see a stage that is subtly wrong.  Here the stage's buffers are read back from the
search workspace (alive_debug_knn_stage_view gives their offsets and the plans from ws_layout / make_plan themselves): the operand
images are checked against a NumPy codec (tests/knn_codes.py), and the candidate lists against ONE float64 matmul of the decoded
operands.  For fp6 that reference is exact and order-independent: codes are multiples of 1/8 below 8, products multiples of 2^-6, a
768-term sum a multiple of 2^-6 below 2^16, so every partial sum is an fp32 number; the fold then overwrites the 4 low mantissa bits
(zero in the exact value for |score| < 2^14) with the lane's register index, which the row index predicts.

Why cv / ci still hold the MAIN pass's lists after the search returns: every later tier writes elsewhere (bf16_tiers_launch: tiers 1a /
1 into cv1 / ci1; collect_tier_launch: c2v / c2i) except tier 2 of the bf16 re-search, which is launched only when
p16.Tt_pad > fcap = min(p16.Tt_pad, FCAP = 16384) -- never at these sizes; and below PROBE_MIN_T = 16384 frames no probe runs (its lists
are cvp / cip anyway).  In the subspace search both fp6 kernels are launched on cv / ci and the gate word lets exactly one of them run;
the test asserts stage_form == "subspace".

All cases are far below SEED_MIN_FB6 = 300 / SEED_MIN_FB = 512 frame blocks: admission is unseeded and the lists are deterministic.  The
seeded regime needs >= 115 200 frames, whose reference is too heavy for a test of seconds; it stays with the audit tests of
test_gpu_knn.py.  The rotated fp8 form is out of scope too (its codes have their own test).

Tolerances are derived, not measured:
  fp6       0: bits(value) & ~15 == bits(float32(reference)).
  fp8       products of two e4m3 numbers are exact in fp32, the sums are not: 768 * 2^-24 * sum_i |a_i b_i| from the codes, plus
            2^-19 |reference| for the 4 index bits.
  bf16      the same sum bound; knn_score_kernel's fold stores the accumulator as it is (the row comes from the register number, not
            from bits of the score), so there is no index term.
  subspace  integer part exact; g_f 2^10 is exact, the fold is one fma and the index bits: 2^-18 (|integer part| + |2^10 g rho|).
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_codes as kc  # noqa: E402

from module import _native as nat  # noqa: E402
from module.common import PackedLibrary  # noqa: E402

pytestmark = pytest.mark.gpu

D = 768
F6_SCALE, F8_SCALE = 32.0, 256.0
# scaled values planted in the first frames of the 3 x 130 batch, on both sides of the fp6 clip threshold 7.75 (bf16 keeps 8 significant
# bits: 7.76 / 32 is stored as 7.75 / 32, 7.8 / 32 as 7.8125 / 32):
# (element, scaled value, value the bf16 image holds x 32, value its e2m3 code holds, clips)
PLANTED = [(5, 7.5, 7.5, 7.5, False), (767, 7.75, 7.75, 7.5, False), (31, 7.76, 7.75, 7.5, False), (32, 7.8, 7.8125, 7.5, True),
           (400, -7.75, -7.75, -7.5, False), (63, -7.8, -7.8125, -7.5, True), (0, 7.25, 7.25, 7.0, False), (700, 20.0, 20.0, 7.5, True)]


def _frames(n, t, m):
    g = torch.Generator().manual_seed(1000 * n + t)
    x = torch.randn(n, D, t, generator=g, dtype=torch.float64)
    x /= x.norm(dim=1, keepdim=True)
    if (n, t) == (3, 130):
        for f, (el, scaled, _, _, _) in enumerate(PLANTED):
            a = scaled / F6_SCALE
            rest = x[0, :, f].clone()
            rest[el] = 0.0
            rest *= (1.0 - a * a) ** 0.5 / rest.norm()
            rest[el] = a
            x[0, :, f] = rest
    return x.float().cuda().contiguous()


def _encoder_frames(t):
    from module.content_encoder import ContentEncoder
    ce = ContentEncoder(seed=2).to("cuda")
    g = torch.Generator(device="cuda").manual_seed(2)
    feat = ce(torch.rand(1, 641, t, device="cuda", generator=g))
    return feat.contiguous(), ce._sd["output_layer.weight"], ce._sd["output_layer.bias"]


@functools.lru_cache(maxsize=None)
def _library(m):
    tok = torch.randn(D, m, generator=torch.Generator().manual_seed(77 + m)).cuda()
    lib = PackedLibrary(tok, prefilter="fp6", strict=False)
    assert lib.prefilter == "fp6" and lib.rot is None and lib.M == m
    return lib


def _scores(A, B):
    """the reference: ONE float64 matmul of the decoded operands"""
    return A @ B.T


def _np(t):
    return t.detach().cpu().numpy()


def _bf16_words(t):
    return _np(t.view(torch.int16)).view(np.uint16)


@functools.lru_cache(maxsize=None)
def _case(stage, n, t, m):
    """one search; the stage's operands and lists read back; the float64 reference of its scores.  Built once per case and read only."""
    base = _library(m)
    sub = stage == "fp6-subspace"
    if sub:
        src, w, b = _encoder_frames(t)
        lib = base.with_prefilter("fp6")
        lib.set_subspace(w, b)
        assert lib.sub is not None
    else:
        src = _frames(n, t, m)
        lib = base if stage == "fp6" else base.with_prefilter(stage)
    assert lib.prefilter == stage.split("-")[0] and lib.rot is None
    Tt = n * t
    assert Tt * kc.K > 64 and Tt <= 16384
    lib.search(src, kc.K)
    st = lib.search_stats()
    if sub:
        assert st["stage_form"] == "subspace", st
    elif stage != "bf16":
        assert not st["probe_chose_bf16_first"] and st["fp8_blocks_seeded"] == 0, st
    ws = lib._last[3]
    v = kc.stage_view(nat.lib(), Tt, m, kc.K, sub)
    assert ws.numel() >= v["bytes"]
    plan = v["p16" if stage == "bf16" else ("p8" if stage == "fp8" else "p6")]
    C = v["KP"] if stage == "bf16" else v["KP8"]
    P = plan["P"]

    def read(off, nbytes):
        return _np(ws[off:off + nbytes])

    cv = read(v["cv"], Tt * P * C * 4).view(np.float32).reshape(Tt, P, C)
    ci = read(v["ci"], Tt * P * C * 4).view(np.int32).reshape(Tt, P, C)
    s_bf16 = read(v["s_bf16"], v["p16"]["Tt_pad"] * D * 2).view(np.uint16).reshape(-1, D)
    c = dict(stage=stage, Tt=Tt, M=m, view=v, plan=plan, C=C, P=P, H=C // 2, cv=cv, ci=ci, s_bf16=s_bf16, src=_np(src))
    m_pad = nat.lib().alive_library_padded_rows(m)
    if stage == "bf16":
        A = kc.bf16_decode(s_bf16[:Tt]).astype(np.float64)
        B = kc.bf16_decode(_bf16_words(lib.lib_bf16)[:m]).astype(np.float64)
        ref = _scores(A, B)
        tol = D * 2.0 ** -24 * (np.abs(A) @ np.abs(B).T)
    elif stage == "fp8":
        c["s_f8"] = read(v["s_f8"], plan["Tt_pad"] * D).reshape(-1, D)
        c["lib_img"] = _np(lib.lib_f8).reshape(m_pad, D)
        A, B = kc.e4m3_decode(c["s_f8"][:Tt]), kc.e4m3_decode(c["lib_img"][:m])
        ref = _scores(A, B)
        tol = D * 2.0 ** -24 * (np.abs(A) @ np.abs(B).T) + 2.0 ** -19 * np.abs(ref)
    elif stage == "fp6":
        c["s_f8"] = read(v["s_f8"], plan["Tt_pad"] * D).reshape(-1, D)
        c["clip6"] = read(v["clip6"], plan["Tt_pad"])
        c["lib_img"] = _np(lib.lib_f8).reshape(m_pad, D)
        A, B = kc.fp6_image_decode(c["s_f8"][:Tt]), kc.fp6_image_decode(c["lib_img"][:m])
        ref = _scores(A, B)
        tol = None
        assert float(np.abs(ref).max()) < 2.0 ** 14                 # the 4 low mantissa bits of every exact score are zero
    else:
        A = kc.fp6_image_decode(read(v["sub_f6"], Tt * 512).reshape(Tt, 512))
        B = kc.fp6_image_decode(_np(lib.sub["lib"]).reshape(m_pad, 512)[:m])
        g = read(v["sub_g"], Tt * 4).view(np.float32)
        rho = _np(lib.sub["rho"])[:m]
        gs = g * np.float32(F6_SCALE * F6_SCALE)                    # exact: a power of two
        whole = _scores(A, B)
        gr = gs.astype(np.float64)[:, None] * rho.astype(np.float64)[None, :]
        ref = whole + gr
        tol = 2.0 ** -18 * (np.abs(whole) + np.abs(gr))
        assert float(np.abs(gr).max()) > 0.0                        # the rho term is live
    c.update(ref=ref, tol=tol, real=ci >= 0)
    for a in (cv, ci, ref):
        a.setflags(write=False)
    return c


STAGES = ["fp6", "fp6-subspace", "fp8", "bf16"]
CASES = [(s, n, t, m) for s in STAGES for n, t, m in (kc.SUB_SHAPES if s == "fp6-subspace" else kc.SHAPES)]
_ids = lambda c: f"{c[0]}-{c[1]}x{c[2]}-M{c[3]}"  # noqa: E731


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_entries_are_fillers_or_distinct_library_rows(case):
    """property 1: every one of a real frame's P * KP entries is the filler (-inf, -1) or a row in [0, M); no row twice; no padding row"""
    c = _case(*case)
    cv, ci, real = c["cv"], c["ci"], c["real"]
    assert c["P"] * c["plan"]["tiles_per_split"] >= c["plan"]["tiles_total"]
    assert np.all(ci[~real] == -1) and np.all(np.isneginf(cv[~real]))
    assert np.all(ci[real] < c["M"]) and np.all(np.isfinite(cv[real]))
    flat = np.sort(ci.reshape(c["Tt"], -1), axis=1)
    dup = (flat[:, 1:] == flat[:, :-1]) & (flat[:, 1:] >= 0)
    assert not dup.any(), np.argwhere(dup)[:5]
    assert real.reshape(c["Tt"], -1).sum(1).min() >= min(c["H"], c["M"])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_candidate_values_are_the_scores_of_their_rows(case):
    """property 2: |value - reference[frame, row]| <= tol; for fp6 the value IS the reference under the 4 index bits"""
    c = _case(*case)
    f, s, e = np.nonzero(c["real"])
    val, idx = c["cv"][f, s, e], c["ci"][f, s, e]
    want = c["ref"][f, idx]
    if c["tol"] is None:
        got = val.view(np.uint32) & ~np.uint32(15)
        bad = got != want.astype(np.float32).view(np.uint32)
        assert np.array_equal(want.astype(np.float32).astype(np.float64), want)
    else:
        bad = np.abs(val.astype(np.float64) - want) > c["tol"][f, idx]
    assert not bad.any(), (int(bad.sum()), [(int(f[i]), int(s[i]), int(e[i]), int(idx[i]), float(val[i]), float(want[i])) for i in np.nonzero(bad)[0][:5]])


def _present(c):
    f, s, e = np.nonzero(c["real"])
    here = np.zeros((c["Tt"], c["M"]), dtype=bool)
    here[f, c["ci"][f, s, e]] = True
    return here


def _kth_best(x, k):
    """k-th largest of every row of x [frames, rows]; -inf with fewer than k rows"""
    if x.shape[1] < k:
        return np.full(x.shape[0], -np.inf)
    return np.partition(x, x.shape[1] - k, axis=1)[:, x.shape[1] - k]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_every_clearly_best_row_is_a_candidate(case):
    """property 3: a row whose reference score exceeds the frame's H-th best by more than 2 tol is among the frame's candidates
    (H = half-list depth: 16 block-scaled, 8 bf16 -- a row in the frame's top H is in the top H of its own half-list's rows)"""
    c = _case(*case)
    ref, here = c["ref"], _present(c)
    kth = _kth_best(ref, c["H"])
    need = ref > kth[:, None] + (0.0 if c["tol"] is None else 2.0 * c["tol"])
    assert need.any(1).all()                                  # (the property is not vacuous: every frame has such rows)
    missing = need & ~here
    assert not missing.any(), np.argwhere(missing)[:5]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_half_lists_hold_the_best_of_their_rows(case):
    """knn_score8_body: entries 16 h .. 16 h + 15 of cand[frame][split] are half-wave h's list over
    R(split, h) = rows < M of the split's tiles with ((row % 8) >= 4) == h
    (knn_score_kernel, beyond what the stage's contract needs: the same with 8 entries per half-wave and no index bits)"""
    c = _case(*case)
    cv, ci, real, ref, M, Tt, P = c["cv"], c["ci"], c["real"], c["ref"], c["M"], c["Tt"], c["P"]
    LT, tps, H = c["view"]["LT"], c["plan"]["tiles_per_split"], c["H"]
    assert (H, c["C"]) == ((8, 16) if c["stage"] == "bf16" else (16, 32))
    rows = np.arange(M)
    row_split, row_half = (rows // LT) // tps, (rows % 8 >= 4).astype(np.int64)
    assert row_split.max() < P
    here = _present(c)
    f, s, e = np.nonzero(real)
    idx = ci[f, s, e]
    r32 = idx % 32
    if c["stage"] != "bf16":
        # the index bits of a stored score: the lane's accumulator register of the row
        bits = cv[f, s, e].view(np.uint32) & 15
        assert np.array_equal(r32 & 3, bits & 3) and np.array_equal(r32 >> 3, (bits >> 2) & 3)
    assert np.array_equal((r32 >> 2) & 1, e // H)
    # every entry comes from its own list's rows
    assert np.array_equal(row_split[idx], s) and np.array_equal(row_half[idx], e // H)
    counts = real.reshape(Tt, P, 2, H).sum(-1)
    for sp in range(P):
        for h in range(2):
            R = rows[(row_split == sp) & (row_half == h)]
            assert np.all(counts[:, sp, h] == min(H, len(R))), (sp, h, len(R), counts[:, sp, h].min(), counts[:, sp, h].max())
            if len(R) == 0:
                continue
            sub = ref[:, R]
            tol2 = 0.0 if c["tol"] is None else 2.0 * c["tol"][:, R]
            kth = _kth_best(sub, H)[:, None]
            inside = here[:, R]
            missing = (sub > kth + tol2) & ~inside
            assert not missing.any(), (sp, h, [(int(a), int(R[b])) for a, b in np.argwhere(missing)[:5]])
            intruder = (sub < kth - tol2) & inside
            assert not intruder.any(), (sp, h, [(int(a), int(R[b])) for a, b in np.argwhere(intruder)[:5]])


# ---- operand images -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("m", sorted({m for _, _, m in kc.SHAPES}))
def test_library_images_are_the_codes_of_the_bf16_rows(m):
    """alive_library_pack_fp6 / _fp8: the whole image is encode(bf16 row x 2^5 / x 2^8), byte for byte; padding rows and slot tails zero"""
    lib = _library(m)
    m_pad = nat.lib().alive_library_padded_rows(m)
    rows = kc.bf16_decode(_bf16_words(lib.lib_bf16)).astype(np.float64).reshape(m_pad, D)
    assert not rows[m:].any() and float(np.abs(rows).max()) * F6_SCALE <= 7.75
    img6 = _np(lib.lib_f8).reshape(m_pad, D)
    assert np.array_equal(img6, kc.fp6_image(rows * F6_SCALE))
    assert not img6.reshape(m_pad, D // 32, 32)[:, :, 24:].any()
    assert not img6[m:].any()
    img8 = _np(lib.with_prefilter("fp8").lib_f8).reshape(m_pad, D)
    assert np.array_equal(img8, kc.e4m3_encode(rows * F8_SCALE))
    assert not img8[m:].any()


@pytest.mark.parametrize("shape", kc.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-M{s[2]}")
def test_frame_images_are_the_codes_of_the_bf16_frames(shape):
    """after a search: s_bf16 holds frame n T + t = bf16(unit(src[n, :, t])); the fp6 / fp8 codes are its encoding, zero beyond the bf16
    image's padded end; clip6[f] == any(|bf16 x 32| > 7.75)"""
    n, t, m = shape
    for stage in ("fp6", "fp8"):
        c = _case(stage, n, t, m)
        v, Tt = c["view"], c["Tt"]
        bf = kc.bf16_decode(c["s_bf16"]).astype(np.float64)
        unit = c["src"].astype(np.float64).transpose(0, 2, 1).reshape(Tt, D)
        unit /= np.linalg.norm(unit, axis=1, keepdims=True)
        assert np.all(np.abs(bf[:Tt] - unit) <= 2.0 ** -8 * np.abs(unit) + 1e-30)       # bf16 rounding + the fp32 normalisation
        assert not bf[Tt:].any()
        pad16, pad = v["p16"]["Tt_pad"], c["plan"]["Tt_pad"]
        lim = min(pad16, pad)
        if stage == "fp8":
            assert pad == pad16
            assert np.array_equal(c["s_f8"], kc.e4m3_encode(bf * F8_SCALE))
            continue
        assert np.array_equal(c["s_f8"][:lim], kc.fp6_image(bf[:lim] * F6_SCALE))
        assert not c["s_f8"][lim:].any()
        clip = np.zeros(pad, dtype=np.uint8)
        clip[:lim] = (np.abs(bf[:lim] * F6_SCALE) > 7.75).any(1)
        assert np.array_equal(c["clip6"], clip)
        if (n, t) == (3, 130):
            for f, (el, _, held, coded, clips) in enumerate(PLANTED):
                assert bf[f, el] * F6_SCALE == held and bool(c["clip6"][f]) == clips, (f, el, bf[f, el] * F6_SCALE)
                assert kc.fp6_image_decode(c["s_f8"][f:f + 1])[0, el] == coded, (f, el)
            assert c["clip6"][len(PLANTED):].sum() == 0
