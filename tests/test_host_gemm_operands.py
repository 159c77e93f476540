"""What tests/test_gpu_gemm_exact.py relies on, proved on the CPU for every case of its matrix (tests/gemm_cases.py): the matrix reaches
every form alive_gemm_planes dispatches to at the required depths, edges and epilogues, with the thresholds read from
csrc/gemm_planes.hip; the operands decode to the designed planes under the host codec and the packers; no partial sum can leave the
exact range; and leaving a kept plane pair out of the reference (or adding a dropped one) changes the expected bits in every tile."""
import os
import re
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gemm_cases as gc  # noqa: E402

from module import _pack  # noqa: E402

CASES = gc.all_cases()
SRC = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "alive-vc_amd", "csrc", "gemm_planes.hip")).read()


def _nct(P, n, ch, t):
    """plane image [planes][c_pad / 32][cols_pad][32] (values) -> [planes][n][ch][t]; the padding must be zero"""
    pl, kb, cols_pad, _ = P.shape
    a = P.permute(0, 2, 1, 3).reshape(pl, cols_pad, kb * 32)
    assert not a[:, n * t:].any() and not a[:, :, ch:].any()
    return a[:, :n * t, :ch].reshape(pl, n, t, ch).permute(0, 1, 3, 2)


def test_dispatch_thresholds_are_the_source_s():
    g = lambda pat: tuple(int(v) for v in re.search(pat, SRC).groups())
    assert g(r"constexpr int GM = (\d+), GN = (\d+), GK = (\d+);") == (gc.GM, gc.GN, gc.GK)
    assert g(r"can_persist = ntiles >= (\d+) && variant != 1") == (gc.PERSIST_TILES,)
    assert g(r"if \(can_persist && nsteps >= (\d+)\) return launch_gemm_lw<3, (\d+)>") == (gc.PERSIST_STEPS, gc.RING["np3lw"])
    assert g(r"if \(\(pad32\(d->Ci\) & (\d+)\) == 0 && pad32\(d->Ci\) >= (\d+)\) \{") == (63, gc.KB2_MIN)
    assert "const int nsteps = kpad / (KB2 ? 2 * GK : GK);" in SRC
    # <planes of the slot, ring depth, ...> of every instantiation
    assert g(r"return launch_gemm<1, (\d+), 2>\(\*d") == (gc.RING["np1"],)
    assert g(r"return launch_gemm<2, (\d+), 2>\(\*d") == (gc.RING["np2"],)
    assert g(r"return launch_gemm<3, (\d+), 1>\(\*d") == (gc.RING["np3"],)
    for act in range(3):
        assert g(rf"return launch_gemm_act<2, (\d+), 2, {act}, true>\(\*d") == (gc.RING["kb2"],)
    for act in range(4):
        assert g(rf"return launch_gemm_act<2, (\d+), 2, {act}, false, true>\(\*d") == (gc.RING["f16s"],)
    assert 'static const int variant = getenv("ALIVE_GEMM_VARIANT")' in SRC
    # every launch with Pout hands the epilogue one of its two LDS stages (the direct store path is gone)
    assert SRC.count("p.Pout != nullptr && stage != nullptr") == 2 and SRC.count("p.Pout != nullptr && stage_small != nullptr") == 1
    assert "stage = smem + w * (NP * 8192);" in SRC and "p.Pout != nullptr ? smem + NS * SLOT + w * 2048 : nullptr" in SRC


def test_the_matrix_is_well_formed():
    ids = [c.id for c in CASES]
    assert len(set(ids)) == len(ids), [i for i in ids if ids.count(i) > 1]
    for c in CASES:
        assert gc.dispatch_case(c) == c.form, (c.id, gc.dispatch_case(c))
        assert (c.act == "argmax") == (c.out == "a") and (c.act != "argmax" or set(c.ep) <= {"bias"}), c.id
        assert c.act != "argmax" or c.form in ("f16s", "np3", "np3lw"), c.id
        assert not c.alias or ("residual" in c.ep and c.out in ("y", "yp")), c.id
        assert c.regime == "I" or c.act is None or c.form == "f16s" or c.act == "argmax", c.id
        assert (c.regime[0] == "F") <= (c.form == "f16s") and (c.regime[0] == "H") <= (c.planes == 1), c.id
        assert c.regime[:2] != "II" or c.form in ("np2", "np3", "np3lw"), c.id
        assert c.regime[:3] != "III" or (c.planes == 3 and set(c.ep) <= {"bias"}), c.id
        assert c.act is None or c.act == "argmax" or c.out in ("y", "yp") or c.tag == "pw1", c.id     # (pw1: against its own yp launch)
        assert int(c.n) * c.co * c.t < 2 ** 30
    by = lambda form: [c for c in CASES if c.form == form]
    steps = lambda form: {c.nsteps for c in by(form)}
    assert set(gc.RING) == {c.form for c in CASES}
    assert steps("np1") >= {1, 2, 3, 5} and {gc.pad32(c.ci) for c in by("np1")} >= {32, 64, 96, 160}
    assert {gc.pad32(c.ci) for c in by("kb2")} >= {128, 192, 256}
    for st in (2, 3, 4):
        assert {c.act for c in by("kb2") if c.nsteps == st} >= {None, "gelu", "exp"}, st
    assert steps("np2") >= {1, 2, 3, 5} and steps("np3") >= {1, 2, 3, 4}
    assert {c.act for c in by("f16s")} == {None, "gelu", "exp", "argmax"}
    assert any(c.act == "gelu" and c.out == "p" for c in by("f16s"))                                    # pw1: GELU, planes times pout_scale
    assert any(c.alias and "ch_scale" in c.ep and c.act is None for c in by("f16s"))                     # pw2: ch_scale, Y is the residual
    assert any(c.act == "argmax" and c.co == 4096 for c in by("f16s"))                                   # the classifier
    assert any(c.act == "argmax" for c in by("np3"))
    for form in gc.RING:                                           # fewer steps than the ring, as many, more
        s, ring = steps(form), gc.RING[form]
        # (no K gives the 32-deep one-plane kernel 4 steps: a padded K of 128 takes the 64-deep form; it has ring - 1 and ring + 1)
        assert (ring in s or form == "np1") and any(v > ring for v in s) and (form in ("np3lw", "kb2") or any(v < ring for v in s)), (form, s)
    lw = by("np3lw")
    assert {c.nsteps for c in lw} == {3, 4, 5} and all(31 < gc.cdiv(c.co, 128) < 34 and 15 < gc.cdiv(c.cols, 128) < 18 for c in lw)
    assert {gc.pad32(c.ci) for c in lw} == {96, 128, 160}
    assert any(c.ntiles & 7 for c in lw) and any(c.co % 128 and c.co % 32 for c in lw) and any(c.cols % 128 for c in lw)
    assert any(c.out in ("p", "yp") and c.co % 32 for c in lw) and any(c.act == "argmax" for c in lw)
    assert any(c.regime == "IIIw" for c in lw) and any(c.regime == "IIIx" for c in lw)
    assert any(c.regime == "III11" for c in CASES) and any(c.regime == "III21" for c in CASES)
    # the edges, over all forms
    assert {c.co for c in CASES} >= set(gc.CO_EDGES) and {c.ci for c in CASES} >= set(gc.CI_EDGES)
    one = [c for c in CASES if c.form != "np3lw"]
    assert any(c.t == 1 for c in one) and any((c.n, c.t) == (3, 37) for c in one)
    assert {c.cols for c in one} >= {127, 128, 129} and any(c.cols > 128 and c.t > 128 and c.n > 1 for c in one)
    for form in gc.RING:
        if form != "np3lw":
            assert {c.out for c in by(form)} >= {"y", "p", "yp"}, form
            assert any(c.co % 128 and c.co > 128 for c in by(form)) and any(c.alias for c in by(form)), form
    assert {c.ep for c in one} >= set(gc.EP_SUBSETS)
    for k in gc.EP[1:]:
        assert {c.form for c in CASES if k in c.ep} >= set(gc.RING), k
    assert {c.form for c in CASES if c.ep == gc.EP and c.act == "gelu"} >= {"np1", "np2", "f16s", "np3"}


@pytest.mark.parametrize("chunk", range(8))
def test_operands_decode_to_the_designed_planes_and_sums_stay_exact(chunk):
    for c in CASES[chunk::8]:
        o = gc.make(c)
        for k in ("x", "w", "bias", "post_add", "ch_scale", "residual"):
            if o.get(k) is not None:
                assert torch.equal(o[k].float().double(), o[k]), (c.id, k)                          # every operand is an fp32 number
        # ---- the activation operand under the host codec ----
        if c.f16s:
            X = _nct(gc.planes_as_float(gc.host_planes(o["x"], "f16s", gc.F16S_ACT_SCALE), c), c.n, c.ci, c.t)
            assert torch.equal(X[0], o["xp"][0] * 256.0) and torch.equal(X[1], o["xp"][1] * 256.0) and not o["xp"][2].any(), c.id
            nz = X[X != 0]
            assert float(nz.abs().min()) >= 2.0 ** -14 and float(nz.abs().max()) <= 65504.0, c.id    # normal fp16 numbers
        elif c.planes == 1:
            X = _nct(gc.planes_as_float(gc.host_planes(o["x"], 1), c), c.n, c.ci, c.t)
            assert torch.equal(X[0], o["x"]) and not o["xp"][1].any() and not o["xp"][2].any(), c.id
        else:
            X = _nct(gc.host_planes(o["x"], 3).view(torch.bfloat16).double(), c.n, c.ci, c.t)
            assert all(torch.equal(X[i], o["xp"][i]) for i in range(3)), c.id
            assert c.planes == 3 or not o["xp"][2].any(), c.id
            assert torch.equal(gc.host_planes(o["x"], 3)[:c.planes], gc.host_planes(o["x"], c.planes)), c.id
            for i, s in enumerate(_pack.split_bf16(o["x"].float(), 3)):                              # the packers' own split
                assert torch.equal(s.double(), o["xp"][i]), c.id
        # ---- the weight under the packers ----
        w3 = o["w"].float().unsqueeze(2)
        want = torch.zeros(3, (c.co + 15) // 16 * 16, gc.pad32(c.ci), dtype=torch.float64)
        for i in range(3):
            want[i, :c.co, :c.ci] = o["wp"][i]
        if c.f16s:
            W5, ws = _pack.pack_conv_split_f16s(w3)
            s = 1.0 / float(ws)
            assert s == 2.0 ** round(__import__("math").log2(s)) and ("w" not in c.regime or s == 4096.0), (c.id, s)
            H = _pack.unpack_conv_split(W5[3:]).contiguous().view(torch.float16).double()
            assert torch.equal(H[0], want[0] * s) and torch.equal(H[1], want[1] * s) and not want[2].any(), c.id
            nz = H[H != 0]
            assert float(nz.abs().min()) >= 2.0 ** -14 and float(nz.abs().max()) <= 65504.0, c.id
        elif c.planes == 1:
            H = _pack.unpack_conv_split(_pack.pack_conv_split_h(w3))[2].contiguous().view(torch.float16).double()
            assert torch.equal(H, want[0]) and not want[1].any() and not want[2].any(), c.id
        else:
            P = _pack.unpack_conv_split(_pack.pack_conv_split(w3, 3)).double()
            assert torch.equal(P, want), c.id
            assert torch.equal(_pack.pack_conv_split(w3, c.planes), _pack.pack_conv_split(w3, 3)[:c.planes]), c.id
            assert c.planes == 3 or not want[2].any(), c.id
        # ---- the exactness budget ----
        bound = gc.unit_sum_bound(c, o)
        assert bound < 2 ** 24, (c.id, bound)
        ref = gc.reference(c, o)
        q = ref["v"] / o["unit"]
        assert torch.equal(q, q.round()), c.id                                                        # v: a multiple of the unit
        if c.act in (None, "argmax"):
            assert not ref["yerr"].any() and torch.equal(ref["y"].float().double(), ref["y"]), c.id   # the expected output is an fp32 number
        else:
            assert float(ref["v"].abs().max()) < 24.0 and float(ref["v"].std()) > 0.25, (c.id, float(ref["v"].abs().max()), float(ref["v"].std()))
        if "p" in c.out and (c.f16s or c.planes == 1):                                                # an fp16 plane output stays in range
            top = float((ref["y"].abs() + ref["yerr"]).max()) * (gc.F16S_ACT_SCALE if c.f16s else 1.0)
            assert top < 65504.0 * 0.999, (c.id, top)
        if c.act == "argmax":
            _, _, first, ties = gc.argmax_reference(c, ref["v"])
            assert ties >= 0.1, (c.id, ties)                       # ties of the maximum between rows of different 64-row blocks
            assert c.tag == "narrow" or first.max() >= gc.twin_offset(c.co), c.id                    # ... and maxima in the upper rows too


SPLIT = [c for c in CASES if c.regime in gc.SPLIT_REGIMES]


@pytest.mark.parametrize("chunk", range(4))
def test_every_kept_pair_is_seen_in_every_tile_and_k_block_and_every_dropped_pair_would_be(chunk):
    """the CPU side of "the GPU test fails on a missing or an extra product": without the contribution of one kept plane pair in one
    k-block the expected fp32 bits change in every 128 x 128 tile; with a dropped pair added they change in every complete tile too"""
    for c in SPLIT[chunk::4]:
        o = gc.make(c)
        v = gc.value(c, o)
        live = lambda i, j: bool(o["wp"][i].any()) and bool(o["xp"][j].any())
        kept = [p for p in gc.kept_pairs(c) if live(*p)]
        assert (0, 0) in kept and len(kept) >= 2, (c.id, kept)                                        # a real lo plane
        if c.regime == "III11":
            assert (1, 1) in kept, c.id
        if c.regime in ("IIIw", "III21"):
            assert (2, 0) in kept, c.id
        if c.regime == "IIIx":
            assert (0, 2) in kept, c.id
        for i, j in kept:
            for kb in range(gc.cdiv(c.ci, gc.GK)):
                d = gc.lin(o["wp"][i], o["xp"][j], slice(kb * gc.GK, min(c.ci, (kb + 1) * gc.GK)))
                seen = gc.tiles_any(c, (v - d).float() != v.float())
                assert bool(seen.all()), (c.id, (i, j), kb, (~seen).nonzero().tolist())
        dropped = [p for p in gc.dropped_pairs(c) if live(*p)]
        if c.regime == "IIwx" and c.planes == 2:
            assert dropped == [(1, 1)], c.id
        if c.regime == "III21":
            assert dropped == [(2, 1)], c.id
        for i, j in dropped:
            d = gc.lin(o["wp"][i], o["xp"][j])
            # (an extra product shows only where |v| is small enough for its fp32 grid to resolve it: asked of every complete tile)
            seen = gc.tiles_any(c, (v + d).float() != v.float())
            full = seen[:c.co // gc.GM, :c.cols // gc.GN]
            assert bool(seen.any()) and bool(full.all()), (c.id, "dropped", (i, j), (~seen).nonzero().tolist())


def test_host_codec_writes_the_k_blocked_layout():
    """element (plane, column, k) of host_planes sits at ((plane * K / 32 + k / 32) * cols_pad + column) * 32 + k % 32 (planes_layout.h)"""
    x = torch.arange(2 * 40 * 70, dtype=torch.float32).view(2, 40, 70) % 251.0
    P = gc.host_planes(x, 1).view(torch.float16).reshape(-1)
    for n, ch, t in ((0, 0, 0), (1, 39, 69), (1, 33, 5), (0, 31, 69)):
        col = n * 70 + t
        assert float(P[((ch // 32) * 256 + col) * 32 + ch % 32]) == float(x[n, ch, t])
    assert P.numel() == 64 * 256
