"""The match path on the device (csrc/match_path.hip) and through the converters, against the NumPy restatement
tools/match_path_ref.py.  Every comparison is bitwise.

1. alive_knn_path_rows alone on a pool of 64 rows: R = 3 list rows, T in {1, 2, 5, 33}, k_max in {1, 2, 4, 8} with mixed k_row, the
   weights 0, 0.25, 1 and 8, lists that repeat indices across consecutive frames, frames without a match at the start, in the middle
   and at the end, entries missing behind a frame's last valid one, a row that is off and rows whose k_row is out of range; the
   workspace and the outputs between guard bands and pre-filled with 0xFF: J at its layout offset is the restatement where it is
   written and fill elsewhere.  The worked case on unit basis rows; a row of 450 frames; a captured call replayed with other per-row
   arrays; an index beyond the table.
2. Converter.match / convert(match_path=) on a strict library: weight 0 is convert(k=1), weight 1 the gather of the restatement on the
   search's lists, the same samples with and without context trimming; convert_many with a mixed list, per-utterance k and a blend;
   a batch_inference.py job against inference.py --knn-strict -mp.
3. MultiStreamConverter(match_path=True), three slots with one on a 2-voice blend, under enable_graph: a slot off is the plain k_max
   converter's, a slot at weight 0 the slot at k = 1, toggling and retuning never re-capture, path_moved() is the restatement on the
   tick's lists, a sparse converter's stalled slot keeps its stream and its count.
4. RealtimeConverter(match_path=...): bitwise a one-slot MultiStreamConverter."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import match_path_ref as MP                                          # noqa: E402
from module import _native as nat                                    # noqa: E402
from module import ops, synthetic                                    # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 256                                                            # guard band, bytes on each side
P = 64


class Guarded:
    """a device array between two guard bands, everything pre-filled with 0xFF"""

    def __init__(self, shape, dtype, nbytes=None):
        self.n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size() if nbytes is None else int(nbytes)
        self.buf = torch.full((self.n + 2 * PAD,), 0xFF, dtype=torch.uint8, device=DEV)
        self.bytes = self.buf[PAD:PAD + self.n]
        self.view = self.bytes.view(dtype).view(*shape) if nbytes is None else self.bytes

    def intact(self):
        return bool((self.buf[:PAD] == 0xFF).all()) and bool((self.buf[-PAD:] == 0xFF).all())


def _dev(a, dtype):
    return torch.as_tensor(np.array(a), dtype=dtype).to(DEV)


@functools.lru_cache(maxsize=None)
def _pool():
    """(rows [64, 768] N(0, 1), norms, the table of all their cosines) -- computed once"""
    rows = np.random.default_rng(11).standard_normal((P, MP.DIM)).astype(np.float32)
    norms = np.sqrt((rows.astype(np.float64) ** 2).sum(axis=1)).astype(np.float32)
    table = MP.cosine_table(rows, norms)
    for a in (rows, norms, table):
        a.setflags(write=False)
    return rows, norms, table


def _lists(R, T, k_max, seed, holes=True):
    """val / idx [R, T, k_max]: descending cosines and indices in [0, 64); about a third of the entries repeat an index of the frame
    before; frames without a match at the start of row 0, in the middle of row 1 and at the end of row 2 (and two in a row where T
    allows); some frames end in -1 entries"""
    rng = np.random.default_rng(seed)
    val = -np.sort(-rng.uniform(0.6, 0.9, (R, T, k_max)).astype(np.float32), axis=2)
    idx = rng.integers(0, P, (R, T, k_max)).astype(np.int32)
    for t in range(1, T):
        again = rng.random((R, k_max)) < 0.35
        idx[:, t] = np.where(again, idx[:, t - 1][:, rng.permutation(k_max)], idx[:, t])
    if holes:
        for r in range(R):
            for t in range(T):
                if k_max > 1 and rng.random() < 0.25:               # entries missing behind the frame's last valid one
                    cut = int(rng.integers(1, k_max))
                    idx[r, t, cut:], val[r, t, cut:] = -1, -np.inf
        gone = {0: [0], 1: [T // 2] + ([T // 2 + 1] if T >= 33 else []), 2: [T - 1]}
        for r, ts in gone.items():
            if r < R and (T > 1 or r == 1):
                idx[r, ts], val[r, ts] = -1, -np.inf
    return val, idx


def _call(val, idx, k_row, k_max, on, weight, rows, norms, R, T, out_val, out_idx, moved, ws):
    return nat.lib().alive_knn_path_rows(val.data_ptr(), idx.data_ptr(), k_row.data_ptr(), k_max, on.data_ptr(), weight.data_ptr(),
                                         rows.data_ptr(), norms.data_ptr(), rows.shape[0], R, T, out_val.data_ptr(),
                                         out_idx.data_ptr(), moved.data_ptr(), ws.data_ptr(), nat.stream())


def _layout(R, T, k_max):
    off = (nat.C.c_int64 * 2)()
    assert nat.lib().alive_knn_path_layout(R, T, k_max, off) == 0
    return int(off[0]), int(off[1]), int(nat.lib().alive_knn_path_workspace_bytes(R, T, k_max))


def _run_and_check(val, idx, k_row, on, weight, rows, norms, table):
    """one guarded call on host lists [R, T, k_max]; J, the lists and `moved` against the restatement -> the restatement's paths"""
    R, T, k_max = idx.shape
    off_j, off_b, nbytes = _layout(R, T, k_max)
    ws = Guarded(None, None, nbytes)
    ov, oi, mv = Guarded((R * T, k_max), torch.float32), Guarded((R * T, k_max), torch.int32), Guarded((R,), torch.int32)
    dv, di = _dev(val.reshape(R * T, k_max), torch.float32), _dev(idx.reshape(R * T, k_max), torch.int32)
    assert _call(dv, di, _dev(k_row, torch.int32), k_max, _dev(on, torch.int32), _dev(weight, torch.float64), _dev(rows, torch.float32),
                 _dev(norms, torch.float32), R, T, ov.view, oi.view, mv.view, ws.view) == 0
    torch.cuda.synchronize()
    assert ws.intact() and ov.intact() and oi.intact() and mv.intact()
    assert np.array_equal(dv.cpu().numpy().view(np.int32), val.reshape(R * T, k_max).view(np.int32))
    assert np.array_equal(di.cpu().numpy(), idx.reshape(R * T, k_max))
    # J: the restatement where a pair of states exists, fill everywhere else, up to the back pointers
    got_j = ws.view[off_j:off_j + R * T * k_max * k_max * 8].cpu().numpy().view(np.int64).reshape(R, T, k_max, k_max)
    for r in range(R):
        live = bool(on[r]) and 1 <= k_row[r] <= k_max
        J, written = MP.join(idx[r], int(k_row[r]) if live else 0, rows, norms, table)
        assert np.array_equal(got_j[r][written], J.view(np.int64)[written]), r
        assert np.all(got_j[r][~written] == -1), r
    assert bool((ws.view[off_j + R * T * k_max * k_max * 8:off_b] == 0xFF).all())
    assert bool((ws.view[off_b + R * T * k_max:] == 0xFF).all())
    want_v, want_i, want_m, paths = MP.path_rows(val, idx, k_row, on, weight, rows, norms, table)
    got_v, got_i = ov.view.cpu().numpy().reshape(R, T, k_max), oi.view.cpu().numpy().reshape(R, T, k_max)
    print("moved", mv.view.cpu().tolist(), "restatement", want_m.tolist())
    assert np.array_equal(got_i, want_i)
    assert np.array_equal(got_v.view(np.int32), want_v.view(np.int32))
    assert np.array_equal(mv.view.cpu().numpy(), want_m)
    return paths, got_v, got_i


# ---------------------------------------------------------------------------------------------------- 1. the kernels alone
@pytest.mark.parametrize("T", [1, 2, 5, 33])
@pytest.mark.parametrize("k_max", [1, 2, 4, 8])
def test_the_kernels_against_the_restatement(k_max, T):
    rows, norms, table = _pool()
    mid = max(1, k_max // 2)
    val, idx = _lists(3, T, k_max, 1000 * k_max + T)
    # every row on with mixed k_row; the middle row off and the last one's k_row beyond k_max, row 0 at weight 0; k_row 0
    for k_row, on, weight in (([k_max, 1, mid], [1, 1, 1], [1.0, 8.0, 0.25]), ([k_max, k_max, k_max + 1], [1, 0, 1], [0.0, 1.0, 1.0]),
                              ([mid, k_max, 0], [1, 1, 1], [8.0, 0.25, 1.0])):
        paths, got_v, got_i = _run_and_check(val, idx, k_row, on, weight, rows, norms, table)
        for r in range(3):
            if paths[r] is None:                                     # a row that is off: a byte copy
                assert np.array_equal(got_i[r], idx[r]) and np.array_equal(got_v[r].view(np.int32), val[r].view(np.int32))
            elif weight[r] == 0.0:                                   # weight 0: the input's entry 0 on every frame
                assert np.all(paths[r] <= 0)
                assert np.array_equal(got_i[r][:, 0], idx[r][:, 0]) and np.array_equal(got_v[r][:, 0].view(np.int32), val[r][:, 0].view(np.int32))


def test_the_worked_case_on_unit_rows():
    T = 12
    val, idx, rows, norms = MP.exact_case(T)
    gv, gi, _, _ = MP.exact_case(T, gap=5)
    val3, idx3 = np.stack([val, val, gv]), np.stack([idx, idx, gi])
    paths, got_v, got_i = _run_and_check(val3, idx3, [2, 2, 2], [1, 1, 1], [0.0625, 0.25, 0.25], rows, norms, MP.cosine_table(rows, norms))
    assert paths[0].tolist() == [0] * T and paths[1].tolist() == [1] * T
    assert paths[2].tolist() == [1] * 5 + [-1] + [1] * 6
    assert got_i[0][:, 0].tolist() == list(range(1, T + 1)) and np.all(got_v[0][:, 0] == np.float32(0.75))
    assert got_i[1][:, 0].tolist() == [0] * T and np.all(got_v[1][:, 0] == np.float32(0.625))
    assert got_i[2][:, 0].tolist() == [0] * 5 + [-1] + [0] * 6 and np.all(got_i[:, :, 1] == -1)


def test_one_long_row():
    rows, norms, table = _pool()
    val, idx = _lists(1, 450, 8, 77)
    paths, _, _ = _run_and_check(val, idx, [8], [1], [1.0], rows, norms, table)
    assert (paths[0] > 0).sum() > 50                                 # (the path does move on such lists)


def test_a_captured_call_follows_its_per_row_arrays():
    rows, norms, table = _pool()
    R, T, k_max = 3, 33, 8
    val, idx = _lists(R, T, k_max, 5)
    dv, di = _dev(val.reshape(R * T, k_max), torch.float32), _dev(idx.reshape(R * T, k_max), torch.int32)
    dr, dn = _dev(rows, torch.float32), _dev(norms, torch.float32)
    k_row, on, weight = _dev([8, 8, 8], torch.int32), _dev([1, 1, 1], torch.int32), _dev([1.0, 1.0, 1.0], torch.float64)
    ov, oi = torch.empty_like(dv), torch.empty_like(di)
    mv = torch.empty(R, dtype=torch.int32, device=DEV)
    ws = torch.empty(_layout(R, T, k_max)[2], dtype=torch.uint8, device=DEV)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        assert _call(dv, di, k_row, k_max, on, weight, dr, dn, R, T, ov, oi, mv, ws) == 0
    for kr, o, w in (([8, 8, 8], [1, 1, 1], [1.0, 1.0, 1.0]), ([4, 8, 1], [1, 0, 1], [8.0, 1.0, 0.25]), ([8, 9, 2], [1, 1, 1], [0.0, 1.0, 8.0])):
        k_row.copy_(_dev(kr, torch.int32)), on.copy_(_dev(o, torch.int32)), weight.copy_(_dev(w, torch.float64))
        ov.fill_(7.0), oi.fill_(-7), mv.fill_(-7)
        g.replay()
        fv, fi, fm = ops.knn_path_rows(dv, di, k_row, k_max, on, weight, dr, dn)                    # a fresh call
        torch.cuda.synchronize()
        assert torch.equal(ov.view(torch.int32), fv.view(torch.int32)) and torch.equal(oi, fi) and torch.equal(mv, fm)
        want_v, want_i, want_m, _ = MP.path_rows(val, idx, kr, o, w, rows, norms, table)
        assert np.array_equal(oi.cpu().numpy().reshape(R, T, k_max), want_i) and np.array_equal(mv.cpu().numpy(), want_m)
        assert np.array_equal(ov.cpu().numpy().reshape(R, T, k_max).view(np.int32), want_v.view(np.int32))


def test_an_index_beyond_the_table_makes_its_frame_inactive():
    """the refusal case: one entry of one frame points past the table (P, and 2^31 - 1).  The frame is treated as a frame without a
    match -- the rows table is never read at that index -- and every other frame is what it is on lists whose frame is all -1"""
    rows, norms, table = _pool()
    val, idx = _lists(3, 33, 4, 9, holes=False)
    bad, clean = idx.copy(), idx.copy()
    bad[0, 7, 2], bad[1, 20, 0], bad[2, 32, 2] = P, 2 ** 31 - 1, P + 5
    for r, t in ((0, 7), (1, 20), (2, 32)):
        clean[r, t] = -1
    bad[2, 3, 3] = P                                                 # beyond k_row = 3: not a state, the frame stays active
    paths, got_v, got_i = _run_and_check(val, bad, [4, 4, 3], [1, 1, 1], [1.0, 1.0, 1.0], rows, norms, table)
    ref_v, ref_i, _, ref_paths = MP.path_rows(val, clean, [4, 4, 3], [1, 1, 1], [1.0, 1.0, 1.0], rows, norms, table)
    for r, t in ((0, 7), (1, 20), (2, 32)):
        assert paths[r][t] == -1 and np.all(got_i[r, t] == -1) and np.all(np.isneginf(got_v[r, t]))
    assert all(np.array_equal(a, b) for a, b in zip(paths, ref_paths)) and np.array_equal(got_i, ref_i)
    assert paths[2][3] >= 0


# ---------------------------------------------------------------------------------------------------- 2. the offline converter
import json                                                          # noqa: E402

from module import audio_io                                          # noqa: E402
from module import multistream as MS                                 # noqa: E402

OFF_CHUNK = 9600                                                     # windows of 28800 samples: 90 frames each


def _nets():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    return ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2)


def _pcm(n, seed, scale=12000):
    return (synthetic.make_waveform(n, seed)[0].numpy() * scale).astype(np.int16)


class Tap:
    """records every call of a module's knn_path_rows (host copies of its lists, per-row arrays and results) while it is in place"""

    def __init__(self, module):
        self.module, self.calls = module, []

    def __enter__(self):
        self.fn = self.module.knn_path_rows

        def tapped(val, idx, k_row, k_max, on, weight, rows, norms, moved=None):
            out = self.fn(val, idx, k_row, k_max, on, weight, rows, norms, moved)
            self.calls.append(dict(val=val.cpu().numpy(), idx=idx.cpu().numpy(), k_row=k_row.cpu().numpy(), k_max=k_max,
                                   on=on.cpu().numpy(), weight=weight.cpu().numpy(), out_val=out[0].cpu().numpy(),
                                   out_idx=out[1].cpu().numpy(), moved=out[2].cpu().numpy()))
            return out
        self.module.knn_path_rows = tapped
        return self

    def __exit__(self, *exc):
        self.module.knn_path_rows = self.fn


def _restated(call, rows, norms):
    """the restatement on a tapped call's lists -> (out_val, out_idx, moved) shaped as the call's"""
    R = len(call["k_row"])
    shape = (R, -1, call["k_max"])
    v, i, m, _ = MP.path_rows(call["val"].reshape(shape), call["idx"].reshape(shape), call["k_row"], call["on"], call["weight"], rows, norms)
    return v.reshape(call["val"].shape), i.reshape(call["idx"].shape), m


def _check_call(call, rows, norms):
    v, i, m = _restated(call, rows, norms)
    assert np.array_equal(call["out_idx"], i) and np.array_equal(call["out_val"].view(np.int32), v.view(np.int32))
    assert np.array_equal(call["moved"], m)
    return m


@pytest.fixture(scope="module")
def offline():
    from module.common import PackedLibrary
    from module.pipeline import Converter
    lib = PackedLibrary(synthetic.make_library(512, 5)[0].to(DEV), strict=True)
    return Converter(*_nets(), DEV).set_library(lib), lib


def test_convert_with_the_path_at_weight_zero_is_the_k_1_match_and_at_weight_one_the_restatement(offline):
    conv, lib = offline
    rows, norms = lib.rows.cpu().numpy(), lib.norms.cpu().numpy()
    wf = synthetic.make_waveform(4000, 91).to(DEV)                   # three windows: the fewest the windowing makes
    kw = dict(chunk=OFF_CHUNK, pitch_shift=1.0)
    plain = conv.convert(wf, k=4, **kw)
    assert torch.equal(conv.convert(wf, k=4, match_path=None, **kw), plain) and torch.equal(conv.convert(wf, k=4, match_path=False, **kw), plain)
    one = conv.convert(wf, k=1, **kw)
    assert torch.equal(conv.convert(wf, k=4, match_path=dict(weight=0), **kw), one) and not torch.equal(one, plain)
    with Tap(ops) as tap:
        full = conv.convert(wf, k=4, match_path=True, **kw)
        trimmed = conv.convert(wf, k=4, match_path=dict(weight=1.0), trim_context=True, share_overlap="auto", **kw)
    assert torch.equal(full, trimmed) and not torch.equal(full, one) and not torch.equal(full, plain)
    assert len(tap.calls) == 2 and tap.calls[0]["val"].shape == (3 * 90, 4) == tap.calls[1]["val"].shape      # the whole windows, both times
    moved = _check_call(tap.calls[0], rows, norms)
    assert np.array_equal(tap.calls[1]["out_idx"], tap.calls[0]["out_idx"]) and moved.max() > 0
    print("frames moved per window:", moved.tolist(), "; read back:", conv.last_path_moved.tolist())
    assert conv.last_path_moved.tolist() == moved.tolist()
    # match(path=): the gather of the restatement's rows
    feat = torch.randn(2, 768, 33, generator=torch.Generator().manual_seed(3)).to(DEV)
    with Tap(ops) as tap:
        got = conv.match(feat, 4, 0.0, path=dict(weight=1.0))
    _, want_i, _ = _restated(tap.calls[0], rows, norms)
    chosen = torch.from_numpy(want_i[:, 0].astype(np.int64)).to(DEV)
    assert torch.equal(got, lib.rows[chosen].view(2, 33, 768).permute(0, 2, 1))
    assert torch.equal(conv.match(feat, 4, 0.3), conv.match(feat, 4, 0.3, path=None))


def test_convert_many_with_a_mixed_list_converts_each_utterance_as_alone(offline):
    from module.common import PackedLibrary
    conv, lib = offline
    g = torch.Generator().manual_seed(5)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 260))}
    vpool = MS.VoicePool(voices)
    utts = [synthetic.make_waveform(n, 40 + i).to(DEV) for i, n in enumerate((4000, OFF_CHUNK + 777, 5000))]      # 3, 4 and 3 windows
    paths = [True, False, {"weight": 0.25}]
    names = ["v0", "v1", "v0"]
    try:
        for kw in (dict(chunk=OFF_CHUNK, k=4, trim_context=True), dict(chunk=OFF_CHUNK, k=[4, 2, 3], trim_context=False)):
            outs = conv.convert_many(utts, vpool, names, pitch_shift=[0.0, 1.0, -1.0], match_path=paths, window_batch=4, **kw)
            plain = conv.convert_many(utts, vpool, names, pitch_shift=[0.0, 1.0, -1.0], window_batch=4, **kw)
            for i, (u, t, n, p) in enumerate(zip(utts, paths, names, (0.0, 1.0, -1.0))):
                conv.set_library(PackedLibrary(voices[n], strict=True))
                k = kw["k"][i] if isinstance(kw["k"], list) else kw["k"]
                alone = conv.convert(u, pitch_shift=p, **dict(kw, k=k), **(dict(match_path=t) if t else {}))
                assert torch.equal(outs[i], alone), i
                assert torch.equal(outs[i], plain[i]) == (not t), i
        # a blend: every list of a window takes its own path; an utterance converts the same alone and inside the corpus
        kw = dict(chunk=OFF_CHUNK, k=4, trim_context=True)
        mix = [{"v0": 2.0, "v1": 1.0}, "v1"]
        both = conv.convert_many(utts[:2], vpool, mix, match_path=[True, False], **kw)
        assert torch.equal(both[0], conv.convert_many(utts[:1], vpool, mix[:1], match_path=True, **kw)[0])
        assert torch.equal(both[1], conv.convert_many(utts[1:2], vpool, mix[1:], **kw)[0])
        assert not torch.equal(both[0], conv.convert_many(utts[:1], vpool, mix[:1], **kw)[0])
        zero = conv.convert_many(utts[:1], vpool, mix[:1], match_path={"weight": 0}, **kw)[0]
        assert torch.equal(zero, conv.convert_many(utts[:1], vpool, mix[:1], **dict(kw, k=1))[0])
    finally:
        conv.set_library(lib)


def _save_nets(d):
    for name, net in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _nets()):
        torch.save(net.state_dict(), d / name)
    return ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt")]


def test_a_batch_job_with_the_path_writes_the_file_of_inference_with_mp(tmp_path, monkeypatch):
    import batch_inference as BI
    import inference as INF
    monkeypatch.setenv("ALIVE_KNN_STRICT", "0")                       # (inference.py --knn-strict sets it; restored after the test)
    d = tmp_path
    nets = _save_nets(d)
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    os.makedirs(d / "inputs")
    audio_io.save(str(d / "inputs" / "utt.wav"), synthetic.make_waveform(36000, 91) * 0.5, 24000)      # 1.5 s mono at 24 kHz
    base = ["-i", str(d / "inputs"), "-lib", str(d / "voice_library.pt"), "-d", "cuda", "-c", "9600", "--knn-strict"] + nets
    INF.main(base + ["-o", str(d / "out_mp"), "-mp", "--path-weight", "0.5"])
    INF.main(base + ["-o", str(d / "out_plain")])
    want, plain = audio_io.load(str(d / "out_mp" / "0_utt.wav"))[0], audio_io.load(str(d / "out_plain" / "0_utt.wav"))[0]
    assert not torch.equal(want, plain)
    job = dict(input="inputs/utt.wav", lib="voice_library.pt")
    (d / "jobs.json").write_text(json.dumps([dict(job, output="b_plain.wav"), dict(job, match_path={"weight": 0.5}, output="b_mp.wav")]))
    BI.main([str(d / "jobs.json"), "-c", "9600"] + nets)
    assert torch.equal(audio_io.load(str(d / "b_mp.wav"))[0], want) and torch.equal(audio_io.load(str(d / "b_plain.wav"))[0], plain)
    (d / "jobs2.json").write_text(json.dumps([dict(job, match_path=False, output="c_plain.wav"), dict(job, output="c_mp.wav")]))
    BI.main([str(d / "jobs2.json"), "-c", "9600", "-mp", "--path-weight", "0.5"] + nets)
    assert torch.equal(audio_io.load(str(d / "c_mp.wav"))[0], want) and torch.equal(audio_io.load(str(d / "c_plain.wav"))[0], plain)


# ---------------------------------------------------------------------------------------------------- 3. MultiStreamConverter
CHUNK, BS, TICKS = 160, 16, 16 + 8                                   # -c 160 -b 16: rings of 2560 samples, 8 frames
GRAPH_AT, SET_AT = BS + 2, BS + 5
MIX = {"v1": 2.0, "v2": 1.0}


@pytest.fixture(scope="module")
def pool():
    g = torch.Generator().manual_seed(31)
    voices = {f"v{i}": torch.randn(768, m, generator=g).to(DEV) for i, m in enumerate((300, 200, 150))}
    return MS.VoicePool(voices)


def _conv(pool, slots=3, **kw):
    return MS.MultiStreamConverter(*_nets(), pool, slots, chunk=CHUNK, buffersize=BS, k=4, **kw)


def _drive(conv, sess, pcm, ticks, actions=None, after=None):
    outs = [[] for _ in sess]
    for s, p in enumerate(sess):
        conv.open(s, **p)
    for tick in range(ticks):
        for a in (actions or {}).get(tick, []):
            a(conv)
        res = conv.step({s: pcm[s][tick * CHUNK:(tick + 1) * CHUNK] for s in range(len(sess))})
        for s in range(len(sess)):
            outs[s].append(res[s])
        if after is not None and any(r is not None for r in res.values()):
            after(conv, tick)
    return outs


def _same(a, b):
    return len(a) == len(b) and all((x is None and y is None) or (x is not None and y is not None and np.array_equal(x, y))
                                    for x, y in zip(a, b))


def test_slots_with_the_path_off_or_at_weight_zero_are_the_plain_converters_and_toggling_never_recaptures(pool):
    pcm = [_pcm(CHUNK * TICKS, 70 + s) for s in range(3)]
    plain = _conv(pool, blend=2, k_max=4)
    assert plain.match_path is False and not hasattr(plain, "path_on")
    plain.enable_graph()
    twin = _drive(plain, [dict(voice="v0", pitch=2.0), dict(voice=MIX, alpha=0.3, k=1), dict(voice="v2", f0_rate=0.9, k=1)], pcm, TICKS)
    with pytest.raises(ValueError, match=r"slot 0: match_path=True needs a converter built with MultiStreamConverter\(..., match_path=True\)"):
        plain.set(0, match_path=True)
    with pytest.raises(ValueError, match="path_moved needs a converter built with"):
        plain.path_moved()
    conv = _conv(pool, blend=2, match_path=True)
    assert conv.k_max == 4 and conv.match_path is True
    captures = []
    actions = {GRAPH_AT: [lambda c: c.enable_graph()],
               SET_AT: [lambda c: c.set(2, path_weight=0.0), lambda c: c.set(0, match_path=True, path_weight=8.0)],
               SET_AT + 1: [lambda c: c.set(0, match_path=False)]}
    sess = [dict(voice="v0", pitch=2.0), dict(voice=MIX, alpha=0.3, match_path=True, path_weight=0.0),
            dict(voice="v2", f0_rate=0.9, match_path=True, path_weight=1.0)]
    outs = _drive(conv, sess, pcm, TICKS, actions=actions, after=lambda c, tick: captures.append((c.captures, c.path_moved())))
    # slot 0 (off, but for one tick); slot 1 (a blend at weight 0: the blend at k = 1); slot 2 (weight 1, then 0: the slot at k = 1)
    assert _same(outs[0][:SET_AT], twin[0][:SET_AT]) and _same(outs[0][SET_AT + 1:], twin[0][SET_AT + 1:])
    assert not np.array_equal(outs[0][SET_AT], twin[0][SET_AT])
    assert _same(outs[1], twin[1])
    assert _same(outs[2][SET_AT:], twin[2][SET_AT:]) and not _same(outs[2][BS:SET_AT], twin[2][BS:SET_AT])
    assert [c for c, _ in captures] == [0] * (GRAPH_AT - BS) + [1] * (TICKS - GRAPH_AT) and conv.captures == 1
    for i, (_, moved) in enumerate(captures):
        tick = BS + i
        assert moved[1] == 0 and (moved[0] > 0) == (tick == SET_AT) and (moved[2] == 0 or tick < SET_AT), (tick, moved)
    assert any(m[2] > 0 for _, m in captures[:SET_AT - BS])
    assert conv.gather_k.tolist() == [4, 1, 1] and conv.path_on.tolist() == [0, 0, 1, 1, 1, 1]
    before = {a: getattr(conv, a).clone() for a in ("path_on", "path_weight", "gather_k", "pitch")}
    for bad in (dict(match_path=1), dict(path_weight=-1.0), dict(path_weight=float("nan"), pitch=3.0), dict(path_weight="x")):
        with pytest.raises(ValueError, match="slot 1: "):
            conv.set(1, **bad)
    assert all(torch.equal(getattr(conv, a), v) for a, v in before.items())
    conv.close(2)
    assert conv.gather_k.tolist() == [4, 1, 4] and conv.path_on.tolist() == [0, 0, 1, 1, 0, 0] and conv.path_moved()[2] == 0


def test_path_moved_is_the_restatement_on_the_ticks_lists(pool):
    pcm = [_pcm(CHUNK * TICKS, 70 + s) for s in range(3)]
    conv = _conv(pool, blend=2, match_path=True)
    rows, norms = pool.rows.cpu().numpy(), pool.norms.cpu().numpy()
    moved = []
    sess = [dict(voice="v0", k=2), dict(voice=MIX, alpha=0.3, match_path=True, path_weight=0.5), dict(voice="v2", match_path=True)]
    with Tap(MS) as tap:
        _drive(conv, sess, pcm, BS + 4, after=lambda c, tick: moved.append(c.path_moved()))
    assert len(tap.calls) == 4 == len(moved)
    for call, got in zip(tap.calls, moved):
        assert call["k_row"].tolist() == [2, 2, 4, 4, 4, 4] and call["on"].tolist() == [0, 0, 1, 1, 1, 1]
        assert call["weight"].tolist()[2:] == [0.5, 0.5, 1.0, 1.0] and call["val"].shape == (6 * 8, 4)
        m = _check_call(call, rows, norms)
        assert np.all(call["idx"].reshape(6, 8, 4)[[1, 5]] == -1)       # the list rows no voice stands behind: no match, no path
        assert got == [0, int(m[2] + m[3]), int(m[4] + m[5])]
    print("frames moved per tick:", moved)
    assert any(g[1] > 0 for g in moved) and any(g[2] > 0 for g in moved)


def test_a_sparse_converter_with_a_stalled_tick_emits_the_same_stream_and_keeps_moved(pool):
    """slot 1 sits one tick out: its ring stands still, so do its lists and what the path makes of them"""
    ticks, stall = BS + 5, BS + 2
    pcm = [_pcm(CHUNK * ticks, 50 + s) for s in range(2)]

    def run(stalled):
        conv = _conv(pool, 2, sparse=True, match_path=True)
        conv.open(0, "v0", match_path=True)
        conv.open(1, "v1", match_path=True, path_weight=2.0)
        outs, at, moved, held = [[], []], [0, 0], [], []
        for tick in range(ticks + (1 if stalled else 0)):
            feed = {}
            for s in range(2):
                if at[s] < ticks and not (stalled and s == 1 and tick == stall):
                    feed[s] = pcm[s][at[s] * CHUNK:(at[s] + 1) * CHUNK]
                    at[s] += 1
            res = conv.step(feed)
            for s, o in res.items():
                if o is not None:
                    outs[s].append(o)
            if 1 in feed and res[1] is not None:
                moved.append(conv.path_moved()[1])
            elif stalled and tick == stall:
                held.append((moved[-1], conv.path_moved()[1]))
        return outs, moved, held
    a, moved_a, _ = run(False)
    b, moved_b, held = run(True)
    assert len(a[1]) == ticks - BS == len(b[1]) and all(np.array_equal(p, q) for p, q in zip(a[1], b[1]))
    assert len(a[0]) == len(b[0]) and all(np.array_equal(p, q) for p, q in zip(a[0], b[0]))
    assert moved_a == moved_b and any(moved_a) and held and held[0][0] == held[0][1]


# ---------------------------------------------------------------------------------------------------- 4. RealtimeConverter
@pytest.mark.parametrize("graph", [False, True])
def test_a_realtime_converter_with_the_path_is_bitwise_a_one_slot_multistream(graph):
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(400, 1)
    kw = dict(chunk=CHUNK, buffersize=BS)
    rt = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, input_gain=-3.0, match_path=dict(weight=0.5), **kw)
    ms = MS.MultiStreamConverter(*_nets(), MS.VoicePool({"lib": lib}), 1, k=4, match_path=True, **kw)
    ms.open(0, "lib", pitch=1.5, alpha=0.2, input_gain=-3.0, match_path=True, path_weight=0.5)
    plain = RealtimeConverter(*_nets(), lib, "cuda", pitch=1.5, alpha=0.2, k=4, input_gain=-3.0, reuse_interior=False, **kw)
    assert rt.match_path is True and rt.reuse is False and plain.match_path is False and not hasattr(plain, "_path_on")
    with pytest.raises(ValueError, match="interior reuse cannot be combined with match_path"):
        RealtimeConverter(*_nets(), lib, "cuda", reuse_interior=True, match_path=True, chunk=960, buffersize=26)
    with pytest.raises(ValueError, match="path_moved needs a converter built with"):
        plain.path_moved()
    if graph:
        rt.enable_graph()
        ms.enable_graph()
    ticks, differ, moved = BS + 6, 0, 0
    pcm = _pcm(CHUNK * ticks, 70)
    for t in range(ticks):
        c = pcm[t * CHUNK:(t + 1) * CHUNK]
        a, b, p = rt.step(c), ms.step({0: c})[0], plain.step(c)
        assert (a is None) == (b is None) == (t < BS)
        if a is not None:
            assert np.array_equal(a, b), t
            assert rt.path_moved() == ms.path_moved()[0]
            moved += rt.path_moved()
            differ += not np.array_equal(a, p)
    assert differ == ticks - BS and moved > 0
