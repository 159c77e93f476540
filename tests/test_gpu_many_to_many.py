"""Many-to-many batch conversion (Converter.convert_many): six utterances of 1 to 12 s over three voices of a pool -- one shared
by three utterances, one 512-vector voice_library.pt, one encoded from a target wav -- each utterance with its own pitch,
intonation, f0 rate and alpha.  Every output is bitwise a Converter with PackedLibrary(voice, strict=True) converting that
utterance alone, with context trimming on and off, on one and on three side streams, with window batches that span utterances;
one utterance against the CPU oracle."""
import pytest
import torch

import alive_oracle as O
from module import ops, schema, synthetic
from module.common import PackedLibrary
from module.multistream import VoicePool

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda")
SECONDS = [1.0, 12.0, 3.5, 7.0, 2.0, 10.25]
VOICE_OF = ["shared", "lib512", "shared", "target", "shared", "lib512"]
PITCH = [0.0, 2.0, -3.0, 5.5, 1.0, -1.0]
INTON = [1.0, 0.8, 1.2, 1.0, 0.5, 1.1]
RATE = [1.0, 0.5, 1.0, 2.0, 1.0, 0.75]
ALPHA = [0.0, 0.1, 0.3, 0.0, 0.5, 0.2]


@pytest.fixture(scope="module")
def rig():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    from module.pipeline import Converter
    from module.spectrogram import spectrogram
    conv = Converter(ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2), DEV)
    g = torch.Generator(device=DEV).manual_seed(41)
    target_wav = synthetic.make_waveform(16000 * 4, 77).to(DEV)
    target_wav = target_wav / target_wav.abs().max()
    tokens = {"shared": torch.randn(1, 768, 3000, device=DEV, generator=g),
              "lib512": synthetic.make_library(512, 5).to(DEV),
              "target": conv.ce(spectrogram(target_wav))}
    pool = VoicePool(tokens, device=DEV)
    utts = [synthetic.make_waveform(int(s * 16000), 300 + i).to(DEV) for i, s in enumerate(SECONDS)]
    utts = [u / u.abs().max() for u in utts]
    return conv, pool, tokens, utts


def single(conv, tokens, u, i, trim, window_batch):
    conv.set_library(PackedLibrary(tokens[VOICE_OF[i]][0], strict=True))
    return conv.convert(u, chunk=48000, k=4, alpha=ALPHA[i], pitch_shift=PITCH[i], intonation=INTON[i], f0_rate=RATE[i],
                        window_batch=window_batch, trim_context=trim)


@pytest.mark.parametrize("trim", [True, False])
@pytest.mark.parametrize("streams", ["1", "3"])
def test_convert_many_is_bitwise_each_utterance_alone(rig, monkeypatch, trim, streams):
    conv, pool, tokens, utts = rig
    monkeypatch.setenv("ALIVE_STREAMS", streams)
    before = ops.Fp16Guard.fallbacks
    outs = conv.convert_many(utts, pool, VOICE_OF, pitch_shift=PITCH, intonation=INTON, f0_rate=RATE, alpha=ALPHA, chunk=48000,
                             k=4, window_batch=5, trim_context=trim)          # 5-window batches: most of them span utterances
    assert ops.Fp16Guard.fallbacks == before, "the fp16 guard repeated the batch: batch composition could matter"
    assert len(outs) == len(utts)
    for i, u in enumerate(utts):
        ref = single(conv, tokens, u, i, trim, 64)
        assert outs[i].shape == ref.shape == (1, u.shape[1])
        assert torch.equal(outs[i], ref), f"utterance {i} differs from its single conversion"


def test_convert_many_scalar_settings_and_errors(rig):
    conv, pool, tokens, utts = rig
    outs = conv.convert_many(utts[:2], pool, ["target", "shared"], alpha=0.1, k=2, window_batch=3)
    for i, name in enumerate(["target", "shared"]):
        conv.set_library(PackedLibrary(tokens[name][0], strict=True))
        assert torch.equal(outs[i], conv.convert(utts[i], k=2, alpha=0.1))
    with pytest.raises(ValueError):
        conv.convert_many(utts[:2], pool, ["target"])
    with pytest.raises(ValueError):
        conv.convert_many(utts[:2], pool, ["target", "nobody"])
    with pytest.raises(ValueError):
        conv.convert_many(utts[:2], pool, ["target", "shared"], pitch_shift=[1.0])


def test_convert_many_against_the_oracle():
    from module.content_encoder import ContentEncoder
    from module.decoder import Decoder
    from module.f0_estimator import F0Estimator
    from module.pipeline import Converter
    conv = Converter(ContentEncoder(seed=2), F0Estimator(seed=2), Decoder(seed=2), DEV)
    lib = synthetic.make_library(512, 5)
    other = synthetic.make_library(700, 9)
    pool = VoicePool({"a": other.to(DEV), "b": lib.to(DEV)}, device=DEV)
    wf = synthetic.make_waveform(16000, 91)
    wf = wf / wf.abs().max()
    outs = conv.convert_many([wf.to(DEV), wf.to(DEV)], pool, ["a", "b"], pitch_shift=[0.0, 2.0], f0_rate=[1.0, 0.5],
                             alpha=[0.0, 0.1], chunk=4800, k=4)
    cpu = [synthetic.make_state_dict(s, 2, p) for s, p in ((schema.content_encoder_schema(), "ce."),
                                                          (schema.f0_estimator_schema(), "pe."),
                                                          (schema.decoder_schema(), "dec."))]
    ref = O.convert_utterance(cpu[0], cpu[1], cpu[2], wf, lib, chunk=4800, k=4, alpha=0.1, pitch_shift=2.0, f0_rate=0.5)
    err = (outs[1].cpu() - ref).pow(2).mean().sqrt().item()
    assert err < 1e-3, err
