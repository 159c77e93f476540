"""Voice codebooks on the device (csrc/codebook.hip, module/codebook.py) against the float64 NumPy restatement tools/codebook_ref.py.

1. The inverted index is a stable torch.sort (module/codebook.py inverted_index): checked against np.argsort(kind=
   "stable") and np.bincount, twice, on the shapes the update is tested on.
2. alive_codebook_update: bitwise the restatement on rows spread over 2^-24 .. 2^24, list lengths 0 .. 40 000, empty clusters keep a
   sentinel row, a second launch is bitwise the first, guard bands around the centroids and the workspace.
3. alive_codebook_stats: `moved` exact, `objective` bitwise the restatement's order and within 1e-12 of math.fsum.
4. One assignment step (the strict search against a library of the centroids) against a float64 brute force on a dense bank.
5. Planted clusters end to end through build_codebook: two iterations, the planted partition, bitwise the restatement's means.
6. The seeded default init on the dense bank: reproducible, seed-dependent, empty clusters counted, objective rises, packable.
7. Through the pool: enrol_voice(codebook=) against add(build_codebook(.)), the sessions' PCM, and codebook=None as before.
8. generate_voice_library.py --codebook and multistream_inference.py "codebook"."""
import json
import math
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "alive-vc_amd"), os.path.join(ROOT, "tools")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import codebook_ref as CR                                            # noqa: E402
from module import _native as nat                                    # noqa: E402
from module import audio_io, synthetic                               # noqa: E402
from module import codebook as CB                                    # noqa: E402
from module import multistream as MS                                 # noqa: E402

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
PAD = 16                                                             # guard band, elements on each side of every output
SENTINEL = 7.25
BIG_M, BIG_C, BIG_LIST = 70001, 300, 40000
LENGTHS = [0, 1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025]


class Guarded:
    """a device array between two guard bands filled with a sentinel"""

    def __init__(self, shape, dtype, sentinel, band=PAD):
        n = int(np.prod(shape))
        self.band = band
        self.buf = torch.full((n + 2 * band,), sentinel, dtype=dtype, device=DEV)
        self.view = self.buf[band:band + n].view(*shape)
        self.sentinel = sentinel

    def intact(self):
        s = torch.full((self.band,), self.sentinel, dtype=self.buf.dtype, device=DEV)
        return torch.equal(self.buf[:self.band], s) and torch.equal(self.buf[-self.band:], s)


def _nets():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    return ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2)


def _spread_rows(m, seed):
    """random rows, each multiplied by 2^e with e drawn from -24 .. 24"""
    rng = np.random.RandomState(seed)
    return (rng.randn(m, 768).astype(np.float32) * np.exp2(rng.randint(-24, 25, size=(m, 1))).astype(np.float32))


def _small_assign():
    """M = 3840 rows in 12 lists of the lengths LENGTHS (list 0 empty) plus an empty last list, interleaved at random"""
    a = np.concatenate([np.full(n, c, dtype=np.int32) for c, n in enumerate(LENGTHS)])
    np.random.RandomState(11).shuffle(a)
    return a, len(LENGTHS) + 1


def _big_assign():
    """M = 70 001, C = 300: list 0 holds 40 000 rows including row 0 and row M - 1; lists 7 and 299 are empty"""
    rng = np.random.RandomState(12)
    a = np.zeros(BIG_M, dtype=np.int32)
    others = rng.permutation(np.arange(1, BIG_M - 1))[:BIG_M - BIG_LIST]
    free = np.array([c for c in range(1, BIG_C) if c not in (7, 299)])
    a[others] = free[rng.randint(0, len(free), size=len(others))]
    assert (a == 0).sum() == BIG_LIST and a[0] == 0 and a[-1] == 0
    return a, BIG_C


@pytest.fixture(scope="module")
def big_rows():
    rows = _spread_rows(BIG_M, 21)
    return rows, torch.from_numpy(rows).to(DEV)


@pytest.fixture(scope="module")
def dense_bank():
    """M = 20 000 rows with a shared component (randn + 1.0 * one fixed randn direction), C = 300 centroids taken from the rows, and
    the float64 brute-force assignment with its best-to-second gaps"""
    rng = np.random.RandomState(31)
    rows = (rng.randn(20000, 768) + 1.0 * rng.randn(768)[None]).astype(np.float32)
    init = sorted(rng.permutation(20000)[:300].tolist())
    a, best, gap = CR.assign_rows(rows, rows[init], with_gap=True)
    return dict(rows=rows, tokens=torch.from_numpy(np.ascontiguousarray(rows.T)).to(DEV), init=init, assign=a, best=best, gap=gap)


# ---------------------------------------------------------------------------------------------------- 1. the index
@pytest.mark.parametrize("case", ["one", "seven", "big"])
def test_inverted_index_is_the_stable_sort(case):
    if case == "one":
        a, c = np.zeros(1, dtype=np.int32), 1
    elif case == "seven":
        a, c = np.random.RandomState(1).choice([0, 1, 3, 4, 6], size=1000).astype(np.int32), 7           # lists 2 and 5 are empty
    else:
        a, c = _big_assign()
    runs = [CB.inverted_index(torch.from_numpy(a).to(DEV), c) for _ in range(2)]
    order, seg_off, counts = (t.cpu().numpy() for t in runs[0])
    assert order.dtype == np.int32 and seg_off.dtype == np.int32
    assert np.array_equal(order, np.argsort(a, kind="stable"))
    assert np.array_equal(counts, np.bincount(a, minlength=c)) and np.array_equal(seg_off, np.concatenate([[0], np.cumsum(counts)]))
    for x, y in zip(runs[0], runs[1]):
        assert torch.equal(x, y)


# ---------------------------------------------------------------------------------------------------- 2. the update
def _update_call(rows_dev, assign, c):
    """alive_codebook_update on sentinel centroids between guard bands, with a guarded workspace of exactly the queried size"""
    L = nat.lib()
    m = rows_dev.shape[0]
    order, seg_off, _ = CB.inverted_index(torch.from_numpy(assign).to(DEV), c)
    cent = Guarded((c, 768), torch.float32, SENTINEL)
    nbytes = int(L.alive_codebook_workspace_bytes(m, c))
    assert nbytes > 0 and nbytes % 256 == 0
    ws = Guarded((nbytes,), torch.uint8, 0xA5, band=256)
    assert cent.view.data_ptr() % 16 == 0 and ws.view.data_ptr() % 256 == 0
    nat.check(L.alive_codebook_update(nat.ptr(rows_dev), m, 768, nat.ptr(order), nat.ptr(seg_off), c, cent.view.data_ptr(),
                                      ws.view.data_ptr(), nat.stream()), "alive_codebook_update")
    torch.cuda.synchronize()
    assert cent.intact() and ws.intact()
    return cent.view.cpu().numpy()


@pytest.mark.parametrize("case", ["small", "big"])
def test_update_is_bitwise_the_restatement(case, big_rows):
    if case == "small":
        assign, c = _small_assign()
        rows = _spread_rows(len(assign), 20)
        rows_dev = torch.from_numpy(rows).to(DEV)
    else:
        assign, c = _big_assign()
        rows, rows_dev = big_rows
    got = _update_call(rows_dev, assign, c)
    want = CR.update(rows, assign, np.full((c, 768), SENTINEL, dtype=np.float32))
    counts = np.bincount(assign, minlength=c)
    assert (counts == 0).sum() == 2
    assert sorted(counts.tolist()) == sorted(LENGTHS + [0]) if case == "small" else counts[0] == BIG_LIST
    empty = counts == 0
    assert np.array_equal(got[empty].view(np.uint32), np.full((int(empty.sum()), 768), SENTINEL, dtype=np.float32).view(np.uint32))
    bad = [int(i) for i in np.nonzero((got.view(np.uint32) != want.view(np.uint32)).any(axis=1))[0]]
    assert not bad, f"lists {bad[:8]} (lengths {[int(counts[i]) for i in bad[:8]]}) differ from the restatement"
    assert np.isfinite(got).all()
    again = _update_call(rows_dev, assign, c)
    assert np.array_equal(got.view(np.uint32), again.view(np.uint32))


# ---------------------------------------------------------------------------------------------------- 3. the stats
def _stats_call(assign, prev, val):
    obj, mov = Guarded((1,), torch.float64, -3.0), Guarded((1,), torch.int64, -77)
    a = torch.from_numpy(assign).to(DEV)
    p = None if prev is None else torch.from_numpy(prev).to(DEV)
    v = torch.from_numpy(val).to(DEV)
    nat.check(nat.lib().alive_codebook_stats(nat.ptr(a), nat.ptr(p), nat.ptr(v), len(assign), obj.view.data_ptr(), mov.view.data_ptr(),
                                             nat.stream()), "alive_codebook_stats")
    torch.cuda.synchronize()
    assert obj.intact() and mov.intact()
    return float(obj.view.cpu()[0]), int(mov.view.cpu()[0])


@pytest.mark.parametrize("m", [1, 1023, 1025, BIG_M])
def test_stats_moved_is_exact_and_objective_is_the_fixed_order_sum(m):
    rng = np.random.RandomState(40 + m % 97)
    assign = rng.randint(0, 300, size=m).astype(np.int32)
    prev = assign.copy()
    flip = rng.rand(m) < 0.3
    prev[flip] = (prev[flip] + 1 + rng.randint(0, 298, size=int(flip.sum()))) % 300
    val = (rng.rand(m) * 2 - 0.5).astype(np.float32)
    want = CR.stats_sum(val)
    exact = math.fsum(float(x) for x in val)
    for p, moved in ((prev, int(flip.sum())), (None, m), (assign.copy(), 0)):
        obj, mov = _stats_call(assign, p, val)
        assert mov == moved == CR.moved(assign, p)
        assert np.float64(obj).view(np.uint64) == np.float64(want).view(np.uint64)
        assert abs(obj - exact) <= 1e-12 * abs(exact)


# ---------------------------------------------------------------------------------------------------- 4. one assignment step
def test_assignment_step_matches_the_float64_brute_force(dense_bank):
    d = dense_bank
    t = d["tokens"]
    rows = t.t().contiguous()
    cent = rows[torch.tensor(d["init"], device=DEV)].contiguous()
    assign = torch.full((20000,), -1, dtype=torch.int32, device=DEV)
    val = torch.full((20000,), -9.0, dtype=torch.float32, device=DEV)
    CB.assign_rows(t, cent, assign, val)
    got, v = assign.cpu().numpy(), val.cpu().numpy()
    sure = d["gap"] >= 1e-5                                           # the project's kNN bar: nearer ties may go either way
    left_out = int((~sure).sum())
    print(f"assignment step: {left_out} of 20000 rows have a float64 best-to-second gap below 1e-5")
    assert left_out <= 100                                            # at most 0.5 % of the rows
    assert np.array_equal(got[sure], d["assign"][sure])
    assert got.min() >= 0 and got.max() < 300
    assert np.abs(v[sure] - d["best"][sure]).max() < 1e-5             # the value is that centroid's cosine, in float32 arithmetic
    assert all(got[i] == c for c, i in enumerate(d["init"]))           # a centroid's own row


# ---------------------------------------------------------------------------------------------------- 5. planted clusters
def _planted():
    rng = np.random.RandomState(50)
    sizes = [1, 2, 63, 64, 65, 511, 512, 513, 1024, 1025, 1500] + rng.randint(3, 401, size=26).tolist()
    dirs = rng.randn(len(sizes), 768)
    dirs *= 8.0 / np.linalg.norm(dirs, axis=1, keepdims=True)
    label = rng.permutation(np.concatenate([np.full(n, c) for c, n in enumerate(sizes)]))
    m = len(label)
    rows = ((dirs[label] + 0.05 * rng.randn(m, 768)) * np.exp2(rng.randint(-3, 4, size=(m, 1)))).astype(np.float32)
    init = [int(np.nonzero(label == c)[0][0]) for c in range(len(sizes))]
    return rows, label, init


def test_planted_clusters_end_to_end():
    rows, label, init = _planted()
    m, c = rows.shape[0], len(init)
    assert c == 37 and 9000 < m < 13000
    gap = CR.assign_rows(rows, rows[init], with_gap=True)[2]
    assert gap.min() > 0.5                                            # no near-tie can interfere
    tokens = torch.from_numpy(np.ascontiguousarray(rows.T)).to(DEV)
    st = {}
    book = CB.build_codebook(tokens, c, init=init, stats=st)
    assert book.shape == (768, c) and book.dtype == torch.float32 and book.is_cuda and book.is_contiguous()
    assert st["moved"] == [m, 0] and st["iterations"] == 2 and st["converged"] is True and st["empty_clusters"] == 0
    assert (st["list_min"], st["list_max"]) == (1, 1500) and len(st["objective"]) == 2
    assert all(st[k] >= 0 for k in ("search_s", "index_s", "update_s"))
    means = CR.update(rows, label, rows[init])
    got = book.cpu().numpy().T
    assert np.array_equal(got.view(np.uint32), means.view(np.uint32))
    rst = {}
    ref = CR.build_codebook(rows.T, c, init=init, stats=rst)
    assert np.array_equal(got.view(np.uint32), ref.T.view(np.uint32)) and rst["moved"] == st["moved"]
    assert np.allclose(st["objective"], rst["objective"], rtol=1e-6)
    # the [1, 768, M] form, no stats, a 3-D result never: the same codebook
    assert torch.equal(CB.build_codebook(tokens[None], c, init=init), book)
    # size >= M: the tokens unchanged
    assert CB.build_codebook(tokens, m) is tokens and torch.equal(CB.build_codebook(tokens[None], m + 5), tokens)
    with pytest.raises(ValueError, match="twice"):
        CB.build_codebook(tokens, 3, init=[0, 1, 1])
    with pytest.raises(ValueError, match="outside"):
        CB.build_codebook(tokens, 3, init=[0, 1, m])


# ---------------------------------------------------------------------------------------------------- 6. the seeded default init
def test_seeded_default_init_on_the_dense_bank(dense_bank):
    t, rows = dense_bank["tokens"], dense_bank["rows"]
    st = {}
    a = CB.build_codebook(t, 300, iters=4, stats=st)
    b = CB.build_codebook(t, 300, iters=4)
    assert torch.equal(a, b)
    assert not torch.equal(a, CB.build_codebook(t, 300, iters=4, seed=1))
    assert st["iterations"] == 4 and not st["converged"] and st["moved"][0] == 20000 and len(st["objective"]) == 4
    # the last assignment was made against the centroids of three iterations: recompute it in float64
    before = CB.build_codebook(t, 300, iters=3).cpu().numpy().T
    last = CR.assign_rows(rows, before)[0]
    assert st["empty_clusters"] == int((np.bincount(last, minlength=300) == 0).sum())
    print(f"dense bank, C = 300: mean best cosine {st['objective'][0] / 20000:.4f} -> {st['objective'][-1] / 20000:.4f}, "
          f"moved {st['moved']}, empty clusters {st['empty_clusters']}")
    assert st["objective"][-1] > st["objective"][0]
    norms = a.norm(dim=0)
    assert bool(torch.isfinite(norms).all()) and float(norms.min()) > 0
    from module.common import PackedLibrary
    PackedLibrary(a, strict=True)                                     # the result packs


# ---------------------------------------------------------------------------------------------------- 7. through the pool
CHUNK, BS = 160, 16


def _session_pcm(pool, name, nets, ticks):
    conv = MS.MultiStreamConverter(*nets, pool, 1, chunk=CHUNK, buffersize=BS, k=2)
    conv.open(0, name)
    pcm = (synthetic.make_waveform(ticks * CHUNK, 77)[0].numpy() * 12000).astype(np.int16)
    outs = [conv.step({0: pcm[i * CHUNK:(i + 1) * CHUNK]})[0] for i in range(ticks)]
    return [o for o in outs if o is not None]


def test_enrol_voice_with_a_codebook_is_add_of_build_codebook():
    nets = tuple(n.to(DEV) for n in _nets())
    tokens = synthetic.make_library(2000, 9)[0].to(DEV)
    book = CB.build_codebook(tokens, 64)
    assert book.shape == (768, 64)
    a, b = MS.VoicePool(device=DEV, capacity=256), MS.VoicePool(device=DEV, capacity=256)
    assert MS.enrol_voice(a, "v", nets[0], None, None, lib=tokens, codebook=64) == 64
    b.add("v", book)
    assert a.segment("v") == b.segment("v") == (0, 64)
    assert torch.equal(a.rows[:64], b.rows[:64]) and torch.equal(a.norms[:64], b.norms[:64])
    assert torch.equal(a.rows[:64], book.t())
    # in pieces: the centroids go in as any voice does
    c = MS.VoicePool(device=DEV, capacity=256)
    assert MS.enrol_voice(c, "v", nets[0], None, None, lib=tokens, codebook=64, max_frames=24) == 64
    assert torch.equal(c.rows[:64], b.rows[:64]) and torch.equal(c.norms[:64], b.norms[:64])
    # 16 filling ticks, then 12 that emit
    pa, pb = _session_pcm(a, "v", nets, BS + 12), _session_pcm(b, "v", nets, BS + 12)
    assert len(pa) == len(pb) == 12 and all(x.any() for x in pa)
    assert all(np.array_equal(x, y) for x, y in zip(pa, pb))
    with pytest.raises(ValueError, match="codebook"):
        MS.enrol_voice(MS.VoicePool(device=DEV, capacity=256), "v", nets[0], None, None, lib=tokens, codebook=0)


def test_enrol_voice_without_a_codebook_is_todays_call():
    nets = tuple(n.to(DEV) for n in _nets())
    wav, lib = synthetic.make_waveform(16000, 5), synthetic.make_library(300, 9)
    a, b = MS.VoicePool(device=DEV, capacity=1024), MS.VoicePool(device=DEV, capacity=1024)
    n = MS.enrol_voice(a, "v", nets[0], wav, 16000, lib=lib, codebook=None)
    parts = MS.voice_parts(nets[0], wav, 16000, lib, device=DEV)
    b.add("v", parts)
    assert n == sum(int(p.shape[1]) for p in parts) > 300 and a.segment("v") == b.segment("v")
    assert torch.equal(a.rows[:n], b.rows[:n]) and torch.equal(a.norms[:n], b.norms[:n])
    # and with one: the wav's frames and the library's tokens are condensed together, once
    c = MS.VoicePool(device=DEV, capacity=1024)
    assert MS.enrol_voice(c, "v", nets[0], wav, 16000, lib=lib, codebook=32, codebook_seed=3) == 32
    whole = torch.cat([p.to(DEV) for p in parts], dim=1)
    assert torch.equal(c.rows[:32], CB.build_codebook(whole, 32, seed=3).t())
    # a voice no larger than the size stays as it is
    d = MS.VoicePool(device=DEV, capacity=1024)
    assert MS.enrol_voice(d, "v", nets[0], wav, 16000, lib=lib, codebook=n) == n and torch.equal(d.rows[:n], b.rows[:n])


# ---------------------------------------------------------------------------------------------------- 8. the CLIs
def test_generate_voice_library_codebook(tmp_path):
    import generate_voice_library as gvl
    from module.voice_library import VoiceLibrary
    d = tmp_path
    torch.save(_nets()[0].state_dict(), d / "content_encoder.pt")
    os.makedirs(d / "wavs")
    for i in range(3):                                                # 3 x 84 clips of 7680 samples: 252 clips >= 2000 / 8
        audio_io.save(str(d / "wavs" / f"w{i}.wav"), synthetic.make_waveform(84 * 7680, 60 + i), 16000)
    common = [str(d / "wavs"), "-cep", str(d / "content_encoder.pt"), "--num-tokens", "2000", "--frames-per-clip", "8", "--seed", "1"]
    gvl.main(common + ["-lib", str(d / "plain.pt")])
    gvl.main(common + ["-lib", str(d / "book.pt"), "--codebook", "512"])
    plain, book = torch.load(d / "plain.pt"), torch.load(d / "book.pt")
    assert plain["tokens"].shape == (1, 768, 2000) and book["tokens"].shape == (1, 768, 512) and book["tokens"].dtype == torch.float32
    VL = VoiceLibrary()                                               # the reference's fixed 512 slots
    assert VL.tokens.shape == (1, 768, 512)
    VL.load_state_dict(book)
    assert torch.equal(VL.tokens, book["tokens"])
    assert torch.equal(book["tokens"][0], CB.build_codebook(plain["tokens"][0].to(DEV), 512, seed=1).cpu())


def test_multistream_cli_codebook_session_is_a_session_on_the_codebook_file(tmp_path):
    import multistream_inference as msi
    d = tmp_path
    for name, net in zip(("content_encoder.pt", "f0_estimator.pt", "decoder.pt"), _nets()):
        torch.save(net.state_dict(), d / name)
    nets = ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt")]
    lib = synthetic.make_library(2000, 5)
    torch.save({"tokens": lib}, d / "voice_library.pt")
    torch.save({"tokens": CB.build_codebook(lib.to(DEV), 64).cpu()[None].contiguous()}, d / "book.pt")
    audio_io.save(str(d / "in0.wav"), synthetic.make_waveform((BS + 12) * CHUNK, 8) * 0.3, 16000)
    json.dump([dict(input="in0.wav", lib="voice_library.pt", codebook=64, k=2)], open(d / "a.json", "w"))
    json.dump([dict(input="in0.wav", lib="book.pt", k=2)], open(d / "b.json", "w"))
    json.dump([dict(input="in0.wav", lib="voice_library.pt", k=2)], open(d / "c.json", "w"))
    outs = {}
    for tag, extra in (("a", []), ("b", []), ("c", []), ("c_flag", ["--codebook", "64"])):
        out = d / f"out_{tag}"
        msi.main(nets + extra + ["-c", str(CHUNK), "-b", str(BS), "-o", str(out), str(d / f"{tag.split('_')[0]}.json")])
        outs[tag] = open(out / "0_in0.wav", "rb").read()
    assert len(outs["a"]) > 44 + 2 * 12 * CHUNK - 1
    assert outs["a"] == outs["b"] == outs["c_flag"]
    assert outs["a"] != outs["c"]                                     # the full voice sounds different: the key did something
