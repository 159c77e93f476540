"""batch_inference.py: 3 jobs over 2 voices (inputs at 16 and 24 kHz); every output file bitwise the file
`inference.py --knn-strict` writes for that job's input, voice and settings."""
import json
import os
import shutil
import sys

import pytest
import torch

from module import audio_io, schema, synthetic

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "alive-vc_amd"))


def test_batch_cli_matches_inference_strict(tmp_path, monkeypatch):
    import batch_inference
    import inference
    d = tmp_path
    for name, (sch, pre) in {"content_encoder.pt": (schema.content_encoder_schema(), "ce."),
                             "f0_estimator.pt": (schema.f0_estimator_schema(), "pe."),
                             "decoder.pt": (schema.decoder_schema(), "dec.")}.items():
        torch.save(synthetic.make_state_dict(sch, 2, pre), d / name)
    torch.save({"tokens": synthetic.make_library(512, 5)}, d / "voice_library.pt")
    audio_io.save(str(d / "target.wav"), synthetic.make_waveform(16000 * 3, 7) * 0.4, 16000)
    audio_io.save(str(d / "a.wav"), synthetic.make_waveform(24000 * 2, 91) * 0.5, 24000)
    audio_io.save(str(d / "b.wav"), synthetic.make_waveform(16000 * 5, 92) * 0.3, 16000)
    audio_io.save(str(d / "c.wav"), synthetic.make_waveform(24000 * 1, 93) * 0.5, 24000)
    jobs = [dict(input="a.wav", lib="voice_library.pt", pitch=2.0, alpha=0.1, output="out/a.wav"),
            dict(input="b.wav", target="target.wav", f0_rate=0.5, intonation=0.8, gain=3.0, output="out/b.wav"),
            dict(input="c.wav", lib="voice_library.pt", pitch=-1.0, normalize=True, output="out/c.wav")]
    os.makedirs(d / "out")
    (d / "jobs.json").write_text(json.dumps(jobs))
    nets = ["-dep", str(d / "decoder.pt"), "-cep", str(d / "content_encoder.pt"), "-f0ep", str(d / "f0_estimator.pt"), "-d", "cuda",
            "-c", "16000"]
    batch_inference.main([str(d / "jobs.json")] + nets)
    monkeypatch.setenv("ALIVE_KNN_STRICT", "0")          # (inference.py --knn-strict sets it; restored after the test)
    for j, job in enumerate(jobs):
        ind = d / f"in{j}"
        os.makedirs(ind)
        shutil.copy(d / job["input"], ind / job["input"])
        voice = ["-lib", str(d / job["lib"])] if "lib" in job else ["-t", str(d / job["target"])]
        flags = ["-p", str(job.get("pitch", 0.0)), "-a", str(job.get("alpha", 0.0)), "-f0", str(job.get("f0_rate", 1.0)),
                 "-int", str(job.get("intonation", 1.0)), "-g", str(job.get("gain", 1.0))]
        if job.get("normalize"):
            flags += ["-norm", "1"]
        inference.main(["-i", str(ind), "-o", str(d / f"ref{j}"), "--knn-strict"] + voice + flags + nets)
        ref, sr_ref = audio_io.load(str(d / f"ref{j}" / f"0_{os.path.splitext(job['input'])[0]}.wav"))
        got, sr = audio_io.load(str(d / job["output"]))
        assert sr == sr_ref and got.shape == ref.shape
        assert torch.equal(got, ref), f"job {j} differs from inference.py --knn-strict"
