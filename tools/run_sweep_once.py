"""one seeded launch of the fused fp16 FilterBlock of csrc/filter_big.hip in a sweep regime (several tiles per block), digest of the
output: python tools/run_sweep_once.py C L N LF
C = 256: alive_filter_block256_fp16; C = 64: alive_filter_block64s_fp16 and, for L >= 512, alive_filter_block64s_fp16_up (a second digest).
The wave arrangement is chosen by ALIVE_FB256_WAVES (4: one wave of 64 channels per SIMD; else two of 32), read once per process:
equal digests across the two = equal bits."""
import hashlib, sys, os, torch
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "alive-vc_amd"))
from module import ops
c, l, n, lf = (int(a) for a in sys.argv[1:5])
torch.manual_seed(c * 1000 + l)
x = torch.randn(n, c, l).cuda(); skip = torch.randn(n, c, l).cuda()
film = torch.randn(n, 6 * 2 * c + 5, lf) * 0.1
film[:, 5:].view(n, 6, 2, c, lf)[:, :, 0] += 1.0          # scale rows around 1, shift rows around 0
film = film.cuda()
sd = {}
for j in range(3):
    for cc in ("c1", "c2"):
        p = f"n.blocks.{j}.{cc}"
        sd[p + ".conv.conv.weight"] = (torch.randn(c, c, 5) * (0.5 / c ** 0.5)).cuda()
        sd[p + ".conv.conv.bias"] = (torch.randn(c) * 0.1).cuda()
up = (torch.randn(64, 16, 2) * 0.12).cuda(), (torch.randn(16) * 0.1).cuda()
ops.f16_saturations(reset=True)
outs = [ops.filter_block256(x, sd, "n", film, 5, skip=skip)]
if c == 64 and l >= 512:
    outs.append(ops.filter_block256(x, sd, "n", film, 5, skip=skip, up=up))
torch.cuda.synchronize()
assert all(torch.isfinite(o).all() for o in outs) and ops.f16_saturations(reset=True) == 0
print("digest " + " ".join(hashlib.sha256(o.cpu().numpy().tobytes()).hexdigest()[:16] for o in outs))
