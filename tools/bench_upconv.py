"""The decoder's two coarse transposed convs (csrc/networks.hip: ups[0] composed with input_conv, ups[1]) per launch, at the 192 windows
of a headline batch, on two-plane split bf16:
  ups0   256 -> 256 x 10 (GEMM rows 2560), 450 columns per window
  ups1   256 ->  64 x  8 (GEMM rows  512), 4500 columns per window
Each is timed through alive_conv1d (the stationary-input kernel of csrc/conv_up.hip) and through alive_conv1d_tiled (conv_split.hip's
tiled kernel, which it replaces), alternated in one process: median of ROUNDS rounds of REPS launches between two HIP events.  The
outputs of the two are compared bitwise.  GB/s = (fp32 input + fp32 output bytes) / time.
  python tools/bench_upconv.py [--json out.json] [--rounds 5] [--reps 50] [--windows 192]
ALIVE_VC_LIB selects the library, as everywhere."""
import argparse, ctypes as C, json, os, sys, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alive-vc_amd"))
from module import _native as nat
from module._pack import pack_convT_split

ap = argparse.ArgumentParser()
ap.add_argument("--json", default=None)
ap.add_argument("--rounds", type=int, default=5)
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--windows", type=int, default=192)
a = ap.parse_args()
dev = "cuda"; N = a.windows
L_ = nat.lib(); st = torch.cuda.current_stream().cuda_stream
SHAPES = (("ups0", 256, 256, 10, 450), ("ups1", 256, 64, 8, 4500))


def timeit(fn, reps):
    for _ in range(5): fn()
    b, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    b.record()
    for _ in range(reps): fn()
    e.record(); torch.cuda.synchronize()
    return b.elapsed_time(e) / reps


med = lambda v: sorted(v)[len(v) // 2]
out = {"windows": N, "reps": a.reps, "rounds": a.rounds, "lib": nat.LIB_PATH, "shapes": {}}
for name, ci, co, up, tin in SHAPES:
    g = torch.Generator(device=dev).manual_seed(ci + co * up)
    x = torch.randn(N, ci, tin, device=dev, generator=g)
    w = torch.randn(ci, co, up, device=dev, generator=g) * ci ** -0.5
    W, b = pack_convT_split(w, torch.randn(co, device=dev, generator=g))
    Y = [torch.zeros(N, co, tin * up, device=dev) for _ in range(2)]
    d = []
    for y in Y:
        q = nat.AliveConv()
        q.W, q.bias, q.X, q.Y = W.data_ptr(), b.data_ptr(), x.data_ptr(), y.data_ptr()
        q.N, q.Ci, q.Tin, q.Co, q.K_pad, q.precision, q.Ci_pad = N, ci, tin, co * up, ci, 1, ci
        q.KW, q.stride, q.dil, q.Tout, q.up = 1, 1, 1, tin, up
        d.append(q)
    new = lambda: nat.check(L_.alive_conv1d(C.byref(d[0]), st))
    old = lambda: nat.check(L_.alive_conv1d_tiled(C.byref(d[1]), st))
    L_.alive_conv_up_launches(1)
    new(); took_new = L_.alive_conv_up_launches(1)
    old(); took_old = L_.alive_conv_up_launches(1)
    tn, to = [], []
    for _ in range(a.rounds):
        to.append(timeit(old, a.reps)); tn.append(timeit(new, a.reps))
    same = bool(torch.equal(Y[0].view(torch.int32), Y[1].view(torch.int32)))
    gb = (x.numel() + Y[0].numel()) * 4 / 1e9
    out["shapes"][name] = {"Ci": ci, "rows": co * up, "up": up, "columns": tin, "GB": gb, "ms": tn, "tiled_ms": to,
                           "new_form_ran": [took_new, took_old], "bitwise_equal": same}
    print(f"{name}: {ci} -> {co} x {up}, {tin} columns: {med(tn):.4f} ms ({gb / med(tn):.2f} TB/s)   tiled kernel {med(to):.4f} ms "
          f"({gb / med(to):.2f} TB/s)   all pairs faster: {all(n_ < o_ for n_, o_ in zip(tn, to))}   new form ran: {took_new == 1 and took_old == 0}"
          f"   bitwise equal: {same}")
if a.json:
    with open(a.json, "w") as f:
        json.dump(out, f, indent=1)
