"""The WORLD pitch kernels (csrc/world_f0.hip) stage by stage, bit for bit.

The final f0 shows one winning band per frame and hides the rest of the band sweep, so here the call is stopped after each of its
five launches (alive_world_f0_stages, the production launcher with a stage count) and the workspace is read back where
alive_world_f0_layout says the buffers are: the mean, the low-cut signal at every lag, every stream's interval count and interp1
values (losing bands included), every band's candidate, the best band and FixF0Contour's steps are the restatement's
(tools/world_ref.py dio_stages) BITWISE; StoneMask's f0 is zero exactly where the restatement's is and within 1e-6 elsewhere
(tests/test_host_world_stages.py shows on the restatement alone that no decision of any voiced frame lies that close to a branch).

The workspace is exactly the planned size, filled with 0xFF (a NaN as a double, -1 as an int) between two guard bands, and so is the
f0 output: a stage must leave the buffers of later stages, the padding between buffers and the guards as they were.  Cases:
tests/world_cases.py (rates, ranges and frame periods the library accepts; lengths at the sweep's tile seam, the low cut's block
seam, the voice range; rows with 0 .. 3 intervals per stream, an event every other sample, tiles without events)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import world_cases as wc  # noqa: E402
from world_cases import W  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096
GUARD_BYTE, FILL_BYTE = 0xA5, 0xFF


class Guarded:
    """nbytes of device memory filled with 0xFF between two 4-KB bands of 0xA5"""

    def __init__(self, nbytes):
        self.n = nbytes
        self.buf = torch.full((GUARD + nbytes + GUARD,), GUARD_BYTE, dtype=torch.uint8, device=DEV)
        self.inner = self.buf[GUARD:GUARD + nbytes]
        self.inner.fill_(FILL_BYTE)

    def read(self):
        """the inner bytes, after checking both guard bands"""
        host = self.buf.cpu().numpy()
        assert (host[:GUARD] == GUARD_BYTE).all(), "the guard band below was written"
        assert (host[GUARD + self.n:] == GUARD_BYTE).all(), "the guard band above was written"
        return host[GUARD:GUARD + self.n].copy()


def launch(case, stages=None, mask=None):
    """one call on fresh guarded buffers -> (workspace bytes, f0 bytes); stages None: alive_world_f0 (alive_world_f0_rows with a mask)"""
    from module import _native as nat
    from module.common import _world_taps_for
    L = nat.lib()
    cfg = wc.CONFIGS[case[0]]
    x = torch.from_numpy(np.array(wc.case_rows(case))).to(DEV)
    N, L8 = x.shape
    v = wc.layout(L, N, L8, cfg)
    taps = _world_taps_for(cfg[0], cfg[1], cfg[2], x.device)
    ws, out = Guarded(v["total"]), Guarded(4 * N * v["F"])
    head = (nat.ptr(x), N, L8, cfg[0], cfg[1], cfg[2], cfg[3], nat.ptr(taps))
    tail = (nat.ptr(out.inner), nat.ptr(ws.inner), v["total"])
    if stages is not None:
        nat.check(L.alive_world_f0_stages(*head, *tail, stages, nat.stream()), "alive_world_f0_stages")
    elif mask is not None:
        on = torch.tensor(mask, dtype=torch.int32, device=DEV)
        nat.check(L.alive_world_f0_rows(*head, nat.ptr(on), *tail, nat.stream()), "alive_world_f0_rows")
    else:
        nat.check(L.alive_world_f0(*head, *tail, nat.stream()), "alive_world_f0")
    torch.cuda.synchronize()
    return ws.read(), out.read()


class Run:
    def __init__(self, case):
        from module import _native as nat
        self.case, self.cfg = case, wc.CONFIGS[case[0]]
        self.X = wc.case_rows(case)
        self.N, self.L = self.X.shape
        self.v = wc.layout(nat.lib(), self.N, self.L, self.cfg)
        self.F, self.nb = self.v["F"], self.v["nb"]
        self.ref, self.t = wc.case_stages(case)
        self.vr = W.voice_range(self.cfg[3], self.cfg[1])
        self.ws, self.f0 = {}, {}
        for k in (1, 2, 3, 4, 5):
            self.ws[k], self.f0[k] = launch(case, stages=k)
        self.ws["full"], self.f0["full"] = launch(case)
        self.mask = [1 - (r % 2) for r in range(self.N)]
        self.ws["rows"], self.f0["rows"] = launch(case, mask=self.mask)
        N, F, nb = self.N, self.F, self.nb
        self.shapes = dict(mean=(np.float64, (N,)), yl=(np.float64, (N, self.v["yl_ld"])), iv=(np.float64, (N, nb, 4, F)),
                           ni=(np.int32, (N, nb, 4)), best=(np.float64, (N, F)), s1=(np.float64, (N, F)), s2=(np.float64, (N, F)),
                           s3=(np.float64, (N, F)), pos=(np.int32, (N, F)), neg=(np.int32, (N, F)))

    def extent(self, name):
        dt, shape = self.shapes[name]
        o = self.v["off"][name]
        return o, o + np.dtype(dt).itemsize * int(np.prod(shape))

    def bits(self, key, name):
        """the buffer after run `key` as integers of its word size (a double's bits as int64: the fill reads -1 everywhere)"""
        dt, shape = self.shapes[name]
        lo, hi = self.extent(name)
        return self.ws[key][lo:hi].view(np.int64 if dt == np.float64 else np.int32).reshape(shape)

    def padding(self, key):
        """the workspace bytes that belong to no buffer"""
        own = np.zeros(self.v["total"], dtype=bool)
        for name in wc.OFFSETS:
            lo, hi = self.extent(name)
            own[lo:hi] = True
        return self.ws[key][~own]


def b64(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module", params=wc.cases(), ids=wc.case_id)
def run(request):
    return Run(request.param)


def untouched_from(run, key, name):
    """every workspace byte from buffer `name` on still holds the fill, and so does the f0 output"""
    assert (run.ws[key][run.v["off"][name]:] == FILL_BYTE).all(), f"stage {key} wrote at or past '{name}'"
    assert (run.f0[key] == FILL_BYTE).all(), f"stage {key} wrote the f0 output"


def test_stage_1_mean(run):
    want = np.array([row["mean"] for row in run.ref])
    assert np.array_equal(run.bits(1, "mean"), b64(want))
    untouched_from(run, 1, "yl")
    assert (run.padding(1) == FILL_BYTE).all()


def test_stage_2_low_cut(run):
    want = np.stack([row["yl"] for row in run.ref])
    assert want.shape == (run.N, run.v["yl_ld"])
    got = run.bits(2, "yl")
    bad = np.argwhere(got != b64(want))
    assert len(bad) == 0, f"{len(bad)} lags differ, the first (row, lag + c) {bad[0]}"
    assert np.array_equal(run.ws[2][:run.v["off"]["yl"]], run.ws[1][:run.v["off"]["yl"]])
    untouched_from(run, 2, "iv")
    assert (run.padding(2) == FILL_BYTE).all()


def test_stage_3_band_sweep(run):
    """every stream of every band, winners and losers: the interval count, and from two intervals on the F interp1 values"""
    ni, iv = run.bits(3, "ni"), run.bits(3, "iv")
    want_ni = np.stack([row["ni"] for row in run.ref])
    bad = np.argwhere(ni != want_ni)
    assert len(bad) == 0, f"interval counts differ, the first (row, band, stream) {bad[0]}: {ni[tuple(bad[0])]} != {want_ni[tuple(bad[0])]}"
    for r, row in enumerate(run.ref):
        for b in range(run.nb):
            for st in range(4):
                if row["ni"][b, st] >= 2:
                    d = np.nonzero(iv[r, b, st] != b64(row["iv"][b][st]))[0]
                    assert len(d) == 0, f"row {r} band {b} stream {st} ({row['ni'][b, st]} intervals): {len(d)} frames differ, first {d[0]}"
                else:
                    assert (iv[r, b, st] == -1).all(), f"row {r} band {b} stream {st}: written with {row['ni'][b, st]} intervals"
    assert np.array_equal(run.ws[3][:run.v["off"]["iv"]], run.ws[2][:run.v["off"]["iv"]])
    untouched_from(run, 3, "best")
    assert (run.padding(3) == FILL_BYTE).all()


def test_stage_4_select_and_contour(run):
    iv3, iv4 = run.bits(3, "iv"), run.bits(4, "iv")
    assert np.array_equal(iv4[:, :, 1:], iv3[:, :, 1:]), "select changed the streams 1-3"
    assert np.array_equal(run.bits(4, "ni"), run.bits(3, "ni"))
    assert np.array_equal(run.ws[4][:run.v["off"]["iv"]], run.ws[3][:run.v["off"]["iv"]])
    for r, row in enumerate(run.ref):
        d = np.argwhere(iv4[r, :, 0] != b64(row["cand"]))
        assert len(d) == 0, f"row {r}: {len(d)} candidates differ, the first (band, frame) {d[0]}"
        assert np.array_equal(run.bits(4, "best")[r], b64(row["best"])), f"row {r}: best band"
        assert np.array_equal(run.bits(4, "s3")[r], b64(row["f0"])), f"row {r}: contour"
        pos, neg = run.bits(4, "pos")[r], run.bits(4, "neg")[r]
        if run.F <= run.vr:
            assert not row["f0"].any() and row["s1"] is None
            for name in ("s1", "s2", "pos", "neg"):
                assert (run.bits(4, name)[r] == -1).all(), f"row {r}: '{name}' written with no more frames than the voice range"
            continue
        assert np.array_equal(run.bits(4, "s1")[r], b64(row["s1"])), f"row {r}: step 1"
        assert np.array_equal(run.bits(4, "s2")[r], b64(row["s2"])), f"row {r}: step 2"
        s2 = row["s2"]
        ends = [i - 1 for i in range(1, run.F) if s2[i] == 0 and s2[i - 1] != 0]
        starts = [i for i in range(1, run.F) if s2[i - 1] == 0 and s2[i] != 0]
        assert neg[:len(ends)].tolist() == ends and (neg[len(ends):] == -1).all(), f"row {r}: section ends"
        assert pos[:len(starts)].tolist() == starts and (pos[len(starts):] == -1).all(), f"row {r}: section starts"
    assert (run.f0[4] == FILL_BYTE).all()
    assert (run.padding(4) == FILL_BYTE).all()


def test_stage_5_stonemask(run):
    assert np.array_equal(run.ws[5], run.ws[4]), "StoneMask wrote the workspace"
    got = run.f0[5].view(np.float32).reshape(run.N, run.F)
    X = run.X.astype(np.float64)
    want = np.stack([W.stonemask(X[r], row["f0"], run.t, run.cfg[0]) for r, row in enumerate(run.ref)]).astype(np.float32)
    assert np.array_equal(got == 0, want == 0), "voiced / unvoiced decisions differ"
    assert (got.view(np.int32)[want == 0] == 0).all()           # +0.0f
    voiced = want != 0
    if voiced.any():
        rel = np.abs(got[voiced].astype(np.float64) / want[voiced] - 1.0)
        print(f"{wc.case_id(run.case)}: {int(voiced.sum())} voiced frames, largest relative error {rel.max():.3e}")
        assert rel.max() <= 1e-6, rel.max()


def test_five_stages_are_the_production_call(run):
    assert np.array_equal(run.ws["full"], run.ws[5])
    assert np.array_equal(run.f0["full"], run.f0[5])


def test_row_mask_leaves_on_rows_bitwise_and_off_rows_at_the_fill(run):
    for name in wc.OFFSETS:
        got, want = run.bits("rows", name), run.bits("full", name)
        for r, on in enumerate(run.mask):
            if on:
                assert np.array_equal(got[r], want[r]), f"'{name}' of row {r} (on)"
            else:
                assert (got[r] == -1).all(), f"'{name}' of row {r} (off) was written"
    assert (run.padding("rows") == FILL_BYTE).all()
    got = run.f0["rows"].view(np.int32).reshape(run.N, run.F)
    want = run.f0["full"].view(np.int32).reshape(run.N, run.F)
    for r, on in enumerate(run.mask):
        assert np.array_equal(got[r], want[r]) if on else (got[r] == 0).all(), f"f0 of row {r}"


def test_stage_count_is_checked():
    from module import _native as nat
    from module.common import _world_taps_for
    L = nat.lib()
    x = torch.zeros(2, 400, device=DEV)
    out = torch.zeros(2, 11, device=DEV)
    taps = _world_taps_for(8000, 20.0, 4096.0, x.device)
    need = L.alive_world_f0_workspace_bytes(2, 400, 8000, 20.0, 4096.0, 5.0)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    for stages in (0, 6, -1):
        assert L.alive_world_f0_stages(nat.ptr(x), 2, 400, 8000, 20.0, 4096.0, 5.0, nat.ptr(taps), nat.ptr(out), nat.ptr(ws), need,
                                       stages, nat.stream()) < 0
        assert L.alive_last_error().startswith(b"alive_world_f0_stages")
    torch.cuda.synchronize()
