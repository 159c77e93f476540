"""Writes tests/golden/world_f0_*.npz: the reference's own compute_f0 (module/common.py:113-137) on seeded inputs.

Runs only where the reference checkout exists (like oracle/gen_golden.py).  It imports the reference's module/common.py with two
stubs: pyworld.dio / pyworld.stonemask backed by the float64 restatement tools/world_ref.py, and torchaudio.functional.resample
backed by oracle/alive_oracle.py's resample.  What the fixtures pin is therefore the reference's glue -- the resample call, the
per-row loop, both linear interpolations and the shapes -- around the restated WORLD.  Inputs and outputs only.

  python tools/gen_world_golden.py <reference checkout>
"""
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
sys.path[:0] = [os.path.join(ROOT, "tools"), os.path.join(ROOT, "oracle")]
import world_ref as W            # noqa: E402
import alive_oracle as O         # noqa: E402


def _reference_common(ref):
    ta = types.ModuleType("torchaudio")
    taf = types.ModuleType("torchaudio.functional")
    taf.resample = O.resample
    ta.functional = taf
    pw = types.ModuleType("pyworld")
    pw.dio = lambda x, fs, f0_floor=50.0, f0_ceil=800.0, **kw: W.dio(x, fs, f0_floor, f0_ceil)
    pw.stonemask = lambda x, f0, t, fs: W.stonemask(x, f0, t, fs)
    sys.modules.update({"torchaudio": ta, "torchaudio.functional": taf, "pyworld": pw})
    sys.path.insert(0, ref)
    import module.common as rc
    return rc


def inputs():
    """name -> float32 [N, L] at 16 kHz (seeded)"""
    rs = np.random.RandomState(1234)

    def voice(L, f0, vib_hz, vib_depth, amp=0.3, harmonics=8):
        t = np.arange(L) / 16000.0
        f = f0 * (1.0 + vib_depth * np.sin(2 * np.pi * vib_hz * t))
        ph = 2 * np.pi * np.cumsum(f) / 16000.0
        return sum(amp / k * np.sin(k * ph + rs.uniform(0, 6.28)) for k in range(1, harmonics + 1))

    W_, R = 144000, 7680
    tail = voice(W_, 140.0, 5.0, 0.03)
    tail[60000:] = 0.0                                             # the last offline window: zero-padded past the utterance
    return {
        "world_f0_window": np.stack([voice(W_, 120.0, 5.5, 0.04),
                                     voice(W_, 110.0, 4.0, 0.03) + voice(W_, 230.0, 6.0, 0.05, amp=0.2)]),   # N > 1
        "world_f0_window_tail": tail[None],                                                                  # N = 1
        "world_f0_ring": np.stack([voice(R, 200.0, 5.0, 0.05), 0.1 * rs.randn(R),
                                   voice(R, 95.0, 3.0, 0.02) + voice(R, 310.0, 5.0, 0.03, amp=0.15)]),
        "world_f0_ring_short": np.stack([voice(2560, 150.0, 5.0, 0.02)]),                                    # -c 160 -b 16
    }


def main():
    if len(sys.argv) != 2:
        raise SystemExit(__doc__)
    ref = sys.argv[1]
    rc = _reference_common(ref)
    os.makedirs(GOLD, exist_ok=True)
    for name, x in inputs().items():
        x = x.astype(np.float32)
        f0 = rc.compute_f0(torch.from_numpy(x)).numpy()
        np.savez_compressed(os.path.join(GOLD, name + ".npz"), wf=x, f0=f0)
        print("wrote", name, x.shape, f0.shape, "voiced", int((f0 > 0).sum()))


if __name__ == "__main__":
    main()
