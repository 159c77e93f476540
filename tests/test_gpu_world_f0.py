"""WORLD pitch estimation on the MI355X (csrc/world_f0.hip, module/common.py compute_f0, `-wpe` of both pipelines and CLIs):
the device DIO + StoneMask against the float64 restatement (tools/world_ref.py) on the same device-resampled input, batch
independence, determinism, graph capture, argument checks, the resize against torch, the reference-glue fixtures, and the
offline / streaming paths against O.* compositions with the restatement's f0."""
import glob
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import alive_oracle as O
from module import audio_io, schema, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import world_ref as W   # noqa: E402

DEV = "cuda"


def voices16(n, L, seed):
    """n rows at 16 kHz: harmonic voices with vibrato at random pitch, two-voice sums, noise, silence and zero-padded tails"""
    rs = np.random.RandomState(seed)
    t = np.arange(L) / 16000.0
    rows = []
    for i in range(n):
        kind = i % 5
        if kind == 3:
            rows.append(0.1 * rs.randn(L))
            continue
        x = np.zeros(L)
        for _ in range(2 if kind == 1 else 1):
            f0 = rs.uniform(70, 400)
            f = f0 * (1 + 0.04 * np.sin(2 * np.pi * rs.uniform(3, 7) * t))
            ph = 2 * np.pi * np.cumsum(f) / 16000.0
            x += sum(0.3 / k * np.sin(k * ph + rs.uniform(0, 6.28)) for k in range(1, 9))
        if kind == 2:
            x[rs.randint(L // 4, 3 * L // 4):] = 0.0
        if kind == 4:
            x *= np.abs(np.sin(2 * np.pi * 1.3 * t))          # voiced / silent alternation
        rows.append(x)
    return torch.from_numpy(np.stack(rows).astype(np.float32))


def device_8k(n, L16, seed):
    return audio_io.resample(voices16(n, L16, seed).to(DEV), 16000, 8000).contiguous()


def check_against_restatement(x8, got, rows):
    want = W.dio_stonemask_rows(x8[rows].cpu().numpy(), 8000)
    got = got[rows].cpu().numpy()
    assert got.shape == want.shape
    assert np.array_equal(got > 0, want > 0), "voiced / unvoiced decisions differ"
    both = want > 0
    if both.any():
        rel = np.abs(got[both].astype(np.float64) / want[both] - 1.0)
        assert rel.max() <= 1e-6, rel.max()
    return int(both.sum())


@pytest.mark.parametrize("n,L16,rows", [(1, 144000, None), (3, 144000, None), (64, 144000, slice(0, 64, 9)),
                                        (384, 144000, slice(5, 384, 47)), (5, 7680, None), (3, 2560, None)])
def test_device_dio_stonemask_matches_the_restatement(n, L16, rows):
    from module.common import world_f0
    x8 = device_8k(n, L16, seed=n + L16)
    got = world_f0(x8)
    torch.cuda.synchronize()
    assert got.shape == (n, W.n_frames(x8.shape[1], 8000))
    voiced = check_against_restatement(x8, got, slice(None) if rows is None else rows)
    if L16 == 2560:
        assert voiced == 0 and not got.any()                   # -c 160 -b 16: the whole ring inside the zeroed edges
    elif L16 == 144000:
        assert voiced > 0


def test_rows_are_independent_and_runs_bitwise_equal():
    from module.common import world_f0
    x8 = device_8k(64, 144000, seed=7)
    a, b, c = world_f0(x8), world_f0(x8), world_f0(x8)
    assert torch.equal(a, b) and torch.equal(b, c)
    for r in (0, 17, 63):
        assert torch.equal(world_f0(x8[r:r + 1].contiguous())[0], a[r])
    three = world_f0(x8[10:13].contiguous())
    assert torch.equal(three, a[10:13])


def test_linear_resize_is_bitwise_torch_cpu():
    from module.common import linear_resize
    rs = np.random.RandomState(0)
    for lin, lout in ((1801, 281), (281, 450), (97, 15), (15, 24), (3, 7), (450, 450), (5, 1), (1, 9)):
        x = torch.from_numpy((rs.rand(6, 1, lin) * 500).astype(np.float32))
        x[:, :, ::4] = 0
        want = F.interpolate(x, lout, mode="linear")
        got = linear_resize(x.to(DEV), lout).cpu()
        assert torch.equal(got, want), (lin, lout)


def test_compute_f0_matches_the_reference_fixtures(golden_dir):
    """the reference's compute_f0 glue (tools/gen_world_golden.py: its own code around the restated WORLD, O.resample as the
    resampler): shapes exact; values to the resampler's rounding (the device resampler is not bitwise O.resample)"""
    from module.common import compute_f0
    files = sorted(glob.glob(os.path.join(golden_dir, "world_f0_*.npz")))
    assert len(files) == 4
    for path in files:
        z = np.load(path)
        got = compute_f0(torch.from_numpy(z["wf"]).to(DEV)).cpu().numpy()
        want = z["f0"]
        assert got.shape == want.shape, path
        close = np.abs(got - want) <= 1e-3 * np.maximum(np.abs(want), 1.0)
        assert close.mean() >= 0.99, (path, close.mean())
        assert np.array_equal(got > 0, want > 0) or np.mean((got > 0) != (want > 0)) <= 0.01, path


def test_compute_f0_dio_shapes():
    from module.common import compute_f0_dio
    x8 = device_8k(2, 7680, seed=1)
    assert compute_f0_dio(x8[0]).shape == (1, 15)
    assert compute_f0_dio(x8).shape == (2, 1, 15)


def test_bad_arguments_and_short_workspace_are_refused():
    from module import _native as nat
    from module.common import _world_taps_for
    L = nat.lib()
    x8 = torch.zeros(2, 4000, device=DEV)
    out = torch.zeros(2, 101, device=DEV)
    taps = _world_taps_for(8000, 20.0, 4096.0, x8.device)
    need = L.alive_world_f0_workspace_bytes(2, 4000, 8000, 20.0, 4096.0, 5.0)
    ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
    args = lambda n, l, fs, lo, hi, nb: (nat.ptr(x8), n, l, fs, lo, hi, 5.0, nat.ptr(taps), nat.ptr(out), nat.ptr(ws), nb,
                                         nat.stream())
    assert L.alive_world_f0(*args(2, 4000, 8000, 20.0, 4096.0, need)) == 0
    assert L.alive_world_f0(*args(2, 4000, 8000, 20.0, 4096.0, need - 1)) < 0
    assert b"workspace" in L.alive_last_error()
    for bad in ((0, 4000, 8000, 20.0, 4096.0), (2, 0, 8000, 20.0, 4096.0), (2, 4000, 48000, 20.0, 4096.0),
                (2, 4000, 8000, 5.0, 4096.0), (2, 4000, 8000, 100.0, 50.0)):
        assert L.alive_world_f0(*args(*bad, need)) < 0, bad
        assert L.alive_last_error().startswith(b"alive_world_f0")
    assert L.alive_world_f0_workspace_bytes(2, 4000, 8000, 5.0, 4096.0, 5.0) == 0
    assert L.alive_linear_resize(nat.ptr(x8), 2, 0, nat.ptr(out), 10, nat.stream()) < 0
    assert b"alive_linear_resize" in L.alive_last_error()
    with pytest.raises(ValueError):
        from module.common import world_f0
        world_f0(torch.zeros(1, 4000, device=DEV), 48000)
    torch.cuda.synchronize()


def test_graph_capture_replays_bitwise():
    from module.common import compute_f0
    wf = voices16(3, 7680, seed=5).to(DEV)
    eager = compute_f0(wf).clone()
    static = wf.clone()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        compute_f0(static)
    torch.cuda.current_stream().wait_stream(s)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = compute_f0(static)
    for seed in (5, 6, 5):
        static.copy_(voices16(3, 7680, seed=seed).to(DEV))
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out, compute_f0(static))
    assert torch.equal(out, eager)


# ---------------------------------------------------------------------------------------------------------------- end to end
def restated_f0(wf16_dev):
    """compute_f0 with the restatement's DIO + StoneMask on the device-resampled signal, torch's CPU interpolation"""
    l = wf16_dev.shape[1]
    x8 = audio_io.resample(wf16_dev, 16000, 8000).cpu().numpy()
    f0 = torch.from_numpy(W.dio_stonemask_rows(x8, 8000))[:, None]
    return F.interpolate(F.interpolate(f0, x8.shape[1] // 256, mode="linear"), l // 320, mode="linear")


def sds():
    return [synthetic.make_state_dict(s, 2, p) for s, p in ((schema.content_encoder_schema(), "ce."),
                                                            (schema.f0_estimator_schema(), "pe."),
                                                            (schema.decoder_schema(), "dec."))]


def oracle_convert_world(ce, dec, wf, lib, chunk, pitch_shift=0.0, intonation=1.0, f0_rate=1.0, k=4, alpha=0.0):
    windows, total = O.make_windows(wf, chunk)
    f0s = restated_f0(windows.contiguous().to(DEV))
    out = []
    for i, w in enumerate(windows):
        w = w[None]
        spec = O.spectrogram(w)
        f0 = O.pitch_transform_offline(f0s[i:i + 1].clone(), pitch_shift, intonation, f0_rate)
        feat = O.match_features(O.content_encoder(ce, spec), lib, k=k, alpha=alpha)
        wav, _ = O.decoder(dec, feat, f0)
        out.append(wav[:, chunk:-chunk])
    return torch.cat(out, dim=1)[:, :total]


def voiced_utterance(L, seed):
    return voices16(1, L, seed)[:, :L] * 0.8


@pytest.mark.parametrize("trim", [False, True])
def test_converter_world_pitch_matches_oracle(trim):
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    from module.pipeline import Converter
    ce, _, dec = sds()
    lib = synthetic.make_library(512, 5)
    wf = voiced_utterance(40000, seed=11)
    conv = Converter(ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2), DEV).set_library(lib.to(DEV))
    got = conv.convert(wf.to(DEV), chunk=4800, world_pitch=True, pitch_shift=2.0, intonation=0.8, f0_rate=0.5, alpha=0.1,
                       trim_context=trim, share_overlap="auto").cpu()
    want = oracle_convert_world(ce, dec, wf, lib, 4800, pitch_shift=2.0, intonation=0.8, f0_rate=0.5, alpha=0.1)
    assert got.shape == want.shape
    err = (got - want).pow(2).mean().sqrt().item()
    assert err < 1e-3 * max(1.0, want.pow(2).mean().sqrt().item()), err


@pytest.fixture(scope="module")
def cli_dir(tmp_path_factory):
    d = tmp_path_factory.mktemp("wpe")
    names = ("content_encoder.pt", "f0_estimator.pt", "decoder.pt")
    for name, sd in zip(names, sds()):
        torch.save(sd, d / name)
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    os.makedirs(d / "inputs")
    audio_io.save(str(d / "inputs" / "utt.wav"), voiced_utterance(32000, seed=12), 16000)
    return d


def test_inference_cli_wpe_writes_the_world_pitch_conversion(cli_dir):
    import inference
    d = cli_dir
    inference.main(["-i", str(d / "inputs"), "-o", str(d / "outputs"), "-dep", str(d / "decoder.pt"),
                    "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt"),
                    "-lib", str(d / "voice_library.pt"), "-d", "cuda", "-c", "4800", "-p", "1", "-wpe", "True"])
    out, sr = audio_io.load(str(d / "outputs" / "0_utt.wav"))
    wf, _ = audio_io.load(str(d / "inputs" / "utt.wav"))
    wf = wf / wf.abs().max()
    ce, _, dec = sds()
    want = O.gain(oracle_convert_world(ce, dec, wf, synthetic.make_library(512, 5), 4800, pitch_shift=1.0), 1.0)  # -g 1 dB
    assert sr == 16000 and out.shape == want.shape
    assert (out - want).pow(2).mean().sqrt().item() < 1e-3


def realtime_world(graph, chunk=960, bs=8, steps=50, pitch=1.5, f0_rate=0.5, pcm=None):
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    from module.realtime import RealtimeConverter
    lib = synthetic.make_library(1000, 1)
    rt = RealtimeConverter(ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2), lib, DEV, chunk=chunk, buffersize=bs,
                           f0_rate=f0_rate, pitch=pitch, world_pitch=True)
    assert not rt.reuse
    if graph:
        rt.enable_graph()
    if pcm is None:
        pcm = (voiced_utterance(chunk * (bs + steps), seed=21)[0].numpy() * 20000).astype(np.int16)
    outs = []
    for s in range(len(pcm) // chunk):
        o = rt.step(pcm[s * chunk:(s + 1) * chunk])
        if s >= bs:
            outs.append(o)
    return pcm, lib, outs


def test_realtime_world_pitch_graph_equals_eager_and_matches_oracle():
    pcm, lib, eager = realtime_world(False)
    _, _, replay = realtime_world(True)
    assert all(np.array_equal(a, b) for a, b in zip(eager, replay))
    ce, _, dec = sds()
    chunk, bs = 960, 8
    begin, end = O.realtime_geometry(chunk, bs)
    phi, refs = 0, []
    for s in range(bs, bs + 50):
        ring = torch.from_numpy(pcm[(s - bs + 1) * chunk:(s + 1) * chunk].astype(np.float32) / 32768)[None]
        f0 = O.pitch_transform_realtime(restated_f0(ring.to(DEV)), 1.5)      # -f0 is not applied to WORLD's f0
        content = O.match_features(O.content_encoder(ce, O.spectrogram(ring)), lib, k=4, alpha=0.0)
        wave, phi_out = O.decoder(dec, content, f0, phi=phi, crop0=begin)
        phi = phi_out[:, :, end].unsqueeze(2)
        ref = (wave[0].numpy() * 32768).astype(np.int16)
        c = bs * chunk // 2
        refs.append(ref[c - chunk // 2: c + chunk // 2])
    got, want = np.concatenate(eager).astype(np.float64), np.concatenate(refs).astype(np.float64)
    assert got.shape == want.shape == (50 * chunk,)
    assert np.sqrt(np.mean((got - want) ** 2)) / 32768 < 1e-3


def test_realtime_cli_wpe_matches_the_converter(tmp_path):
    import realtime_inference as rti
    names = ("content_encoder.pt", "f0_estimator.pt", "decoder.pt")
    for name, sd in zip(names, sds()):
        torch.save(sd, tmp_path / name)
    torch.save({"tokens": synthetic.make_library(1000, 1)}, tmp_path / "voice_library.pt")
    src = (voiced_utterance(960 * 58, seed=21)[0].numpy() * 20000).astype(np.int16)
    audio_io.save(str(tmp_path / "in.wav"), torch.from_numpy(src.astype(np.float32) / 32768)[None], 16000, encoding="pcm16")
    wf, _ = audio_io.load(str(tmp_path / "in.wav"))
    pcm = (wf[0].numpy() * 32767).astype(np.int16)              # what the CLI feeds its converter
    _, _, outs = realtime_world(False, pitch=0.0, f0_rate=1.0, pcm=pcm)      # (-f0 0.5 below: not applied to WORLD's f0)
    rti.main(["-dep", str(tmp_path / "decoder.pt"), "-cep", str(tmp_path / "content_encoder.pt"),
              "-f0ep", str(tmp_path / "f0_estimator.pt"), "-lib", str(tmp_path / "voice_library.pt"), "-d", "cuda",
              "-c", "960", "-b", "8", "-f0", "0.5", "-wpe", "True",
              "--input-wav", str(tmp_path / "in.wav"), "--output-wav", str(tmp_path / "out.wav")])
    got, sr = audio_io.load(str(tmp_path / "out.wav"))
    want = np.concatenate(outs)                                  # int16 samples of the converter
    n = min(got.shape[1], want.shape[0])
    assert sr == 16000 and n == 50 * 960
    assert np.array_equal(np.round(got[0, :n].numpy() * 32768), want[:n].astype(np.float64))


def test_realtime_reuse_with_world_pitch_raises():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    from module.realtime import RealtimeConverter
    with pytest.raises(ValueError, match="world_pitch"):
        RealtimeConverter(ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2), synthetic.make_library(1000, 1), DEV,
                          chunk=320, buffersize=100, reuse_interior=True, world_pitch=True)
