"""dw conv + (Adaptive)ChannelNorm straight to planes (alive_dwconv_norm_planes*), per launch, in the three forms a headline step
launches (128 windows x 450 frames; csrc/networks.hip::convnext_layer):
  decoder          C = 512, adaptive (scale / shift rows of the 4096-row FiLM tensor), one fp16 plane
  ContentEncoder   C = 512, plain affine, fp16 split (hi, lo) of 256 x value
  F0Estimator      C = 256, plain affine, fp16 split
Each form is timed through the product entry point (the register-resident kernel) and through alive_dwconv_norm_planes_ref (the
LDS-resident kernel, the fallback of other widths), alternated, ROUNDS times; the planes of the two are compared bitwise.
  python tools/bench_dwnorm.py [--json out.json] [--rounds 5]
ALIVE_VC_LIB selects the library, as everywhere."""
import argparse, json, os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alive-vc_amd"))
from module import _native as nat

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
a = ap.parse_args()
dev = "cuda"; N, T = 128, 450
L_ = nat.lib(); st = torch.cuda.current_stream().cuda_stream
FORMS = (("decoder", 512, 1, 0.0, True), ("content_encoder", 512, 2, 256.0, False), ("f0_estimator", 256, 2, 256.0, False))


def timeit(fn, reps):
    for _ in range(5): fn()
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    for _ in range(reps): fn()
    e.record(); torch.cuda.synchronize()
    return b.elapsed_time(e) / reps


out = {"windows": N, "frames": T, "reps": a.reps, "lib": nat.LIB_PATH, "forms": {}}
for name, C, planes, scale, adaptive in FORMS:
    g = torch.Generator(device=dev).manual_seed(C + planes)
    r = lambda *s: torch.randn(*s, device=dev, generator=g)
    x, w, b, gain, off = r(N, C, T), r(C, 7) * 0.3, r(C) * 0.1, r(C) * 0.5 + 1.0, r(C) * 0.2
    cond = r(N, 4096, T) if adaptive else None
    rows = (4096, 1024, 1536) if adaptive else (0, 0, 0)
    P = [torch.zeros(L_.alive_planes_bytes(N * T, C, planes), dtype=torch.uint8, device=dev) for _ in range(2)]
    head = (x.data_ptr(), N, C, T, w.data_ptr(), b.data_ptr(), 1 if adaptive else 0, None if adaptive else gain.data_ptr(),
            None if adaptive else off.data_ptr(), cond.data_ptr() if adaptive else None, *rows, 1e-4)
    if scale:
        new = lambda: nat.check(L_.alive_dwconv_norm_planes_f16s(*head, scale, P[0].data_ptr(), st))
    else:
        new = lambda: nat.check(L_.alive_dwconv_norm_planes(*head, planes, P[0].data_ptr(), st))
    ref = lambda: nat.check(L_.alive_dwconv_norm_planes_ref(*head, planes, P[1].data_ptr(), st, scale))
    tn, tr = [], []
    for _ in range(a.rounds):
        tr.append(timeit(ref, a.reps)); tn.append(timeit(new, a.reps))
    same = bool(torch.equal(P[0], P[1]))
    mb = (x.numel() * 4 + (2 * C * N * T * 4 if adaptive else 0) + planes * C * N * T * 2) / 1e6
    out["forms"][name] = {"C": C, "planes": planes, "f16_scale": scale, "adaptive": adaptive, "MB": mb, "ms": tn, "ref_ms": tr, "bitwise_equal": same}
    med = lambda v: sorted(v)[len(v) // 2]
    print(f"{name:16s} C {C} planes {planes}: {med(tn):.4f} ms ({mb / med(tn) / 1e3:.2f} TB/s)   LDS-resident kernel {med(tr):.4f} ms   "
          f"all pairs faster: {all(n_ < r_ for n_, r_ in zip(tn, tr))}   bitwise equal: {same}")
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
