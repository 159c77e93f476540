"""The fused fp16 FilterBlocks of csrc/filter_big.hip (alive_filter_block256_fp16, alive_filter_block64s_fp16, ..._fp16_up) in the regime
the product runs them in, and per column.  Needs an MI355X; tests/test_host_filter_big.py is the host twin.

A. Sweep regimes: several tiles per block, runs that start inside a window (behind a warm-up tile) and cross window boundaries (a
   reflected `first` tile in the middle of a run), a short last block -- bitwise against calls of so few windows that every tile is its
   own block.  The batch is derived from the device's CU count through tools/filter_big_ref.py::sweep_plan.
B. The one-wave-per-SIMD form (ALIVE_FB256_WAVES=4, RG = 2) gives the bits of the default form.
C. The noise profile against the exact float64 block: rms error per column and per channel, kernel over emulation, inside the bars
   derived from the null band of two emulations (tools/filter_big_ref.py::BARS) -- at both ends: a result more accurate than one fp16
   plane is not this kernel.
D. The launcher's refusals, none of which launches.
"""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import alive_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import filter_big_ref as R                                           # noqa: E402


def relerr(a, b):
    a, b = a.double().cpu(), b.double().cpu()
    return ((a - b).pow(2).mean().sqrt() / (b.pow(2).mean().sqrt() + 1e-30)).item()


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _device_film(cnd, fw):
    from module import ops
    film, _ = ops.conv1d(cnd.to(DEV), fw[0].to(DEV), fw[1].to(DEV), post_add=fw[2].to(DEV))
    return film


# ---- A ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.SWEEPS, ids=lambda s: s.name)
def test_sweep_regimes_are_bitwise_the_one_tile_per_block_calls(case):
    """every window of the batched call -- per_block tiles per block, contexts handed from tile to tile and across window starts --
    equals, bit for bit, the call of at most cus // tiles windows that computes it with a block per tile behind a warm-up tile; no
    saturations in either; with one planted 1e6 both count the same non-zero number and still agree"""
    from module import ops
    cus = _cus()
    n = R.windows_for(case, cus)
    p = R.check_plan(case, R.sweep_plan(n, case.L, case.C, cus))
    group = cus // p.tiles
    assert group >= 1 and all(R.sweep_plan(min(group, n - s), case.L, case.C, cus).per_block == 1 for s in range(0, n, group))
    print(f"{case.name}: {n} windows x {p.tiles} tiles on {cus} CUs: per_block {p.per_block}, {p.blocks} blocks, {p.warm_runs} runs start "
          f"inside a window, {p.crossing_runs} cross a window boundary (at most {p.most_window_starts} window starts per run), last block "
          f"{p.runs[-1].g1 - p.runs[-1].g0} tiles; {cdiv(n, group)} calls of <= {group} windows")
    sd, fw = R.block_weights(case.C)
    sd = {k: v.to(DEV) for k, v in sd.items()}
    gen = torch.Generator(device=DEV).manual_seed(11)
    x = torch.randn(n, case.C, case.L, device=DEV, generator=gen)
    skip = torch.randn(n, case.C, case.L, device=DEV, generator=gen) if case.skip else None
    film = _device_film(torch.randn(n, R.COND, case.lf, device=DEV, generator=gen), fw)
    up = tuple(t.to(DEV) for t in R.up_weights()) if case.up else None
    kw = {} if case.rng is None else dict(t0=case.rng[0], f0=case.rng[1], frames=case.rng[2])

    def run(s0, s1):
        return ops.filter_block256(x[s0:s1], sd, "n", film[s0:s1], R.PAD_ROWS, skip=None if skip is None else skip[s0:s1], up=up, **kw)

    def both():
        ops.f16_saturations(reset=True)
        whole = run(0, n)
        sat_whole = ops.f16_saturations(reset=True)
        assert whole.shape == ((n, 16, 2 * case.L) if case.up else (n, case.C, case.L)) and bool(torch.isfinite(whole).all())
        differ = [s for s in range(0, n, group) if not torch.equal(run(s, min(s + group, n)), whole[s:s + group])]
        return whole, sat_whole, ops.f16_saturations(reset=True), differ

    whole, sat_whole, sat_parts, differ = both()
    assert not differ, f"windows {differ[0]} .. differ from their small-group call ({len(differ)} of {cdiv(n, group)} groups)"
    assert sat_whole == 0 and sat_parts == 0
    # one value that leaves fp16's range, in the last columns of the first tile of a window that starts in the middle of a run (its
    # saturated context is handed to the next tile)
    r = next(r for r in p.runs if r.crossings)
    w = next(g for g in r.firsts if g > r.g0) // p.tiles
    x[w, 3, min(p.BL, case.L) - 3] = 1e6
    planted, sat_whole, sat_parts, differ = both()
    assert not differ
    assert sat_whole > 0 and sat_whole == sat_parts, (sat_whole, sat_parts)
    others = [i for i in range(n) if i != w]
    assert torch.equal(planted[others], whole[others]) and not torch.equal(planted[w], whole[w])


def cdiv(a, b):
    return (a + b - 1) // b


# ---- B ---------------------------------------------------------------------------------------------------------------------
def _digest_of(cmd, env):
    e = dict(os.environ)
    e.update(env)
    out = subprocess.run([sys.executable] + cmd, env=e, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return [ln for ln in out.stdout.splitlines() if ln.startswith("digest")][-1]


@pytest.mark.parametrize("name", ["256-l520", "64-l1300"])
def test_one_wave_per_simd_gives_the_bits_of_two(name):
    """RG = 2 (ALIVE_FB256_WAVES=4: four waves of 64 channels x 128 columns) against the default RG = 1 (eight of 32 x 128) in a sweep
    regime, C = 64 with and without ups[2] in the store phase: the same A fragments per channel, the same k order per accumulator, the
    same epilogue per value -- the kernel's comments claim the same bits.  (The switch is read once per process: subprocesses.)"""
    case = next(s for s in R.SWEEPS if s.name == name)
    n = R.windows_for(case, _cus())
    R.check_plan(case, R.sweep_plan(n, case.L, case.C, _cus()))
    tool = os.path.join(ROOT, "tools", "run_sweep_once.py")
    ds = [_digest_of([tool, str(case.C), str(case.L), str(n), str(case.lf)], {"ALIVE_FB256_WAVES": f}) for f in ("8", "4")]
    assert len(ds[0].split()) == (2 if case.C == 256 else 3)
    assert ds[0] == ds[1], ds


# ---- C ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c,l,lf,n,up", R.ACCURACY)
def test_noise_profile_against_the_exact_block(c, l, lf, n, up):
    """rms error against the exact float64 block per column (pooled over windows and channels) and per channel (pooled over windows and
    columns): kernel over the "f32" emulation of its roundings on the same fp32 FiLM table, inside the bars at every column and channel;
    the total likewise; no saturations; the global figure of test_fused_filter_block_256 against the fp32 oracle"""
    from module import ops
    assert R.ratio_admitted(c, l, lf)
    sd, fw = R.block_weights(c)
    x, cnd, skip = R.accuracy_inputs(c, l, lf, n)
    upw = R.up_weights() if up else None
    film = _device_film(cnd, fw)
    ops.f16_saturations(reset=True)
    out = ops.filter_block256(x.to(DEV), {k: v.to(DEV) for k, v in sd.items()}, "n", film, R.PAD_ROWS, skip=skip.to(DEV),
                              up=None if upw is None else tuple(t.to(DEV) for t in upw)).cpu()
    assert ops.f16_saturations(reset=True) == 0
    film = film.cpu()
    exact = R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", skip=skip, up=upw, rounding=False)
    emu = R.filter_block_fp16(x, film, R.PAD_ROWS, sd, "n", skip=skip, up=upw, flavour="f32")
    col, ch, tot = R.profile_ratios(out, emu, exact)
    oracle = O.filter_block(sd, "n", x, cnd) + skip
    if up:
        oracle = F.conv_transpose1d(oracle, upw[0], upw[1], stride=2)
    e = relerr(out, oracle)
    bars = R.BARS[R.bars_key(c, up)]
    print(f"C {c} l {l} lf {lf} n {n}{' up' if up else ''}: column ratio {col.min():.3f} .. {col.max():.3f} (bars {bars['column'][0]:.3f} .. "
          f"{bars['column'][1]:.3f}), channel ratio {ch.min():.3f} .. {ch.max():.3f} ({bars['channel'][0]:.3f} .. {bars['channel'][1]:.3f}), "
          f"total {tot:.4f} ({bars['total'][0]:.3f} .. {bars['total'][1]:.3f}), global {e:.3e}")
    assert out.shape == exact.shape
    assert bars["column"][0] <= col.min() and col.max() <= bars["column"][1], (int(col.argmin()), col.min().item(), int(col.argmax()), col.max().item())
    assert bars["channel"][0] <= ch.min() and ch.max() <= bars["channel"][1], (int(ch.argmin()), ch.min().item(), int(ch.argmax()), ch.max().item())
    assert bars["total"][0] <= tot <= bars["total"][1], tot
    assert e < 6e-4, e


# ---- D ---------------------------------------------------------------------------------------------------------------------
def _launch_args(c, n, l, lf, up=False):
    from module import _native as nat
    L_ = nat.lib()
    t = dict(x=torch.zeros(n, c, l, device=DEV), film=torch.zeros(n, 12 * c, lf, device=DEV),
             out=torch.full((n * (32 * l + 2) if up else n * c * l,), 7.0, device=DEV),
             ws=[torch.zeros(c * 5 * c, dtype=torch.float16, device=DEV) for _ in range(6)], bs=[torch.zeros(c, device=DEV) for _ in range(6)],
             upW=torch.zeros(32, 64, device=DEV), upb=torch.zeros(32, device=DEV))
    query = L_.alive_filter_block256_workspace_bytes if c == 256 else L_.alive_filter_block64s_workspace_bytes
    t["nbytes"] = query(n, l)
    t["wsp"] = torch.zeros(t["nbytes"], dtype=torch.uint8, device=DEV)
    return t


def _refused(entry_name, t, c, n, l_, lf_, **over):
    """calls the entry point with `over` replacing arguments; -> the error text.  Nothing may have run: the output keeps its fill"""
    from module import _native as nat
    L_ = nat.lib()
    a = dict(U=t["x"].data_ptr(), W=(ctypes.c_void_p * 6)(*[w.data_ptr() for w in t["ws"]]), B=(ctypes.c_void_p * 6)(*[b.data_ptr() for b in t["bs"]]),
             film=t["film"].data_ptr(), out=t["out"].data_ptr(), ws=t["wsp"].data_ptr(), nbytes=t["nbytes"], l=l_, lf=lf_)
    a.update(over)
    head = (a["U"], n, a["l"], a["W"], a["B"], a["film"], 12 * c, a["lf"], 0, 0, 0, a["lf"], None)
    tail = (a["out"], a["ws"], a["nbytes"], torch.cuda.current_stream().cuda_stream)
    if entry_name.endswith("_up"):
        rc = L_.alive_filter_block64s_fp16_up(*head, t["upW"].data_ptr(), t["upb"].data_ptr(), *tail)
    else:
        rc = getattr(L_, entry_name)(*head, *tail)
    assert rc != 0, f"{entry_name} accepted {over}"
    with pytest.raises(ValueError) as err:
        nat.check(rc)
    torch.cuda.synchronize()
    assert bool((t["out"] == 7.0).all()), "a refused call wrote its output"
    assert entry_name in str(err.value), str(err.value)
    return str(err.value)


@pytest.mark.parametrize("entry_name,c", [("alive_filter_block256_fp16", 256), ("alive_filter_block64s_fp16", 64), ("alive_filter_block64s_fp16_up", 64)])
def test_the_launcher_refuses_what_it_cannot_run(entry_name, c):
    """fb_launch's argument checks, each with an error text that names the entry point, none of which launches: in place; L = 32 (the
    reflection needs columns 1 .. 16 behind a 16-column context); more frames under 128 columns than a wave's table holds; a workspace
    one byte short of the query; a null weight pointer; and for the form with ups[2] an output that is not 8-byte aligned"""
    n, l, lf = 2, 1280, 16
    up = entry_name.endswith("_up")
    t = _launch_args(c, n, l, lf, up)
    assert "in-place" in _refused(entry_name, t, c, n, l, lf, out=t["x"].data_ptr())
    # (the form with ups[2] is a batch form that starts at one tile of 512 columns: its own check answers first)
    assert ("at least one tile" if up else "L must exceed 32") in _refused(entry_name, t, c, n, l, lf, l=32, lf=1)
    most = (R.table_frames(c) - 3) * l // 128                         # 130 / 50 frames under 1280 columns are admitted
    assert R.ratio_admitted(c, l, most) and not R.ratio_admitted(c, l, most + 1)
    big = torch.zeros(n, 12 * c, most + 1, device=DEV)
    assert "frames" in _refused(entry_name, t, c, n, l, lf, film=big.data_ptr(), lf=most + 1)
    assert "workspace too small" in _refused(entry_name, t, c, n, l, lf, nbytes=t["nbytes"] - 1)
    assert "workspace too small" in _refused(entry_name, t, c, n, l, lf, ws=None)
    W = (ctypes.c_void_p * 6)(*[w.data_ptr() for w in t["ws"]])
    W[3] = None
    assert "null weights" in _refused(entry_name, t, c, n, l, lf, W=W)
    assert "null pointer" in _refused(entry_name, t, c, n, l, lf, film=None)
    if up:
        assert "8-byte aligned" in _refused(entry_name, t, c, n, l, lf, out=t["out"].data_ptr() + 4)
    # the same arguments untouched are taken (zeros in, the bias-free block of zeros out)
    from module import _native as nat
    L_ = nat.lib()
    W = (ctypes.c_void_p * 6)(*[w.data_ptr() for w in t["ws"]])
    B = (ctypes.c_void_p * 6)(*[b.data_ptr() for b in t["bs"]])
    head = (t["x"].data_ptr(), n, l, W, B, t["film"].data_ptr(), 12 * c, lf, 0, 0, 0, lf, None)
    tail = (t["out"].data_ptr(), t["wsp"].data_ptr(), t["nbytes"], torch.cuda.current_stream().cuda_stream)
    nat.check(L_.alive_filter_block64s_fp16_up(*head, t["upW"].data_ptr(), t["upb"].data_ptr(), *tail) if up else getattr(L_, entry_name)(*head, *tail))
    torch.cuda.synchronize()
    wrote = n * 16 * 2 * l if up else n * c * l
    assert bool((t["out"][:wrote] == 0.0).all()) and bool((t["out"][wrote:] == 7.0).all())
