"""The decoder's three finest FilterBlocks with the small conv behind each folded into the block's store phase (csrc/filter_small.hip,
TAIL_UP / TAIL_WAVE; csrc/filter_big.hip, UP): `alive_filter_block_small_up_range` = FilterBlock(16) + skip -> ups[3],
`alive_filter_block_small_wave_range` = FilterBlock(8) -> source_out, `alive_filter_block64s_fp16_up` = FilterBlock(64) + skip -> ups[2].
Everything here is bitwise (torch.equal): the fused entry points against the sequence of launches they
replace, and the whole decoder with the fused route on and off.  Needs an MI355X."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from module import synthetic

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COND = 24
PAD_ROWS = 5                                         # the block's FiLM rows start inside a larger table, as in the decoder


def g(name, shape, seed=11, scale=1.0):
    return synthetic.gaussian(name, seed, shape, scale)


def block_weights(c):
    """reference-layout weights of a FilterBlock and the weights / biases of the 1x1 convs that make its FiLM table"""
    sd = {"n.input_conv.weight": g(f"fs.iw{c}", (c, c, 1), scale=0.4), "n.input_conv.bias": g(f"fs.ib{c}", (c,), scale=0.1)}
    ws, bs, post = [torch.zeros(PAD_ROWS, COND, 1)], [torch.zeros(PAD_ROWS)], [torch.zeros(PAD_ROWS)]
    for j in range(3):
        for cc in ("c1", "c2"):
            p = f"n.blocks.{j}.{cc}"
            sd[p + ".conv.conv.weight"] = g(p + f"w{c}", (c, c, 5), scale=0.5 / np.sqrt(c))
            sd[p + ".conv.conv.bias"] = g(p + f"b{c}", (c,), scale=0.1)
            ws += [g(p + f"sw{c}", (c, COND, 1), scale=0.1), g(p + f"hw{c}", (c, COND, 1), scale=0.1)]
            bs += [g(p + f"sb{c}", (c,), scale=0.1), g(p + f"hb{c}", (c,), scale=0.1)]
            post += [torch.ones(c), torch.zeros(c)]
    return {k: v.to(DEV) for k, v in sd.items()}, (torch.cat(ws, 0).to(DEV), torch.cat(bs, 0).to(DEV), torch.cat(post).to(DEV))


def film_of(fw, n, lf, tag):
    from module import ops
    film, _ = ops.conv1d(g(f"fs.cnd{tag}", (n, COND, lf)).to(DEV), fw[0], fw[1], post_add=fw[2])
    return film


UP_W = lambda: g("fs.upw", (16, 8, 2), scale=0.25).to(DEV)          # ConvTranspose1d(16, 8, 2, 2).weight [Ci, Co, r]
UP_B = lambda: g("fs.upb", (8,), scale=0.1).to(DEV)
OUT_W = lambda: g("fs.ow", (1, 8, 7), scale=0.2).to(DEV)            # source_out = Conv1d(8, 1, 7, padding 3)
OUT_B = lambda: g("fs.ob", (1,), scale=0.1).to(DEV)


def up_pair(n, l, lf, with_skip, rng=None):
    """(fused, block -> alive_conv1d(up = 2)) on the same inputs; rng = (t0, f0, frames of the whole window)"""
    from module import ops
    sd, fw = block_weights(16)
    x = g(f"fs.x16.{n}.{l}", (n, 16, l)).to(DEV)
    skip = g(f"fs.s16.{n}.{l}", (n, 16, l)).to(DEV) if with_skip else None
    film = film_of(fw, n, lf, f"16.{n}.{lf}")
    kw = {} if rng is None else dict(t0=rng[0], f0=rng[1], frames=rng[2])
    fused = ops.filter_block_small_up(x, sd, "n", film, PAD_ROWS, UP_W(), UP_B(), skip=skip, **kw)
    h = ops.filter_block_small_range(x, sd, "n", film, PAD_ROWS, skip=skip, **kw)
    ref, _ = ops.conv1d(h, UP_W(), UP_B(), transposed=True)
    return fused, ref


UP2_W = lambda: g("fs.up2w", (64, 16, 2), scale=0.12).to(DEV)      # ConvTranspose1d(64, 16, 2, 2).weight
UP2_B = lambda: g("fs.up2b", (16,), scale=0.1).to(DEV)


def up64_pair(n, l, lf, with_skip, rng=None):
    """(fused, alive_filter_block64s_fp16 -> alive_conv1d(up = 2)) on the same inputs"""
    from module import ops
    sd, fw = block_weights(64)
    x = g(f"fs.x64.{n}.{l}", (n, 64, l)).to(DEV)
    skip = g(f"fs.s64.{n}.{l}", (n, 64, l)).to(DEV) if with_skip else None
    film = film_of(fw, n, lf, f"64.{n}.{lf}")
    kw = {} if rng is None else dict(t0=rng[0], f0=rng[1], frames=rng[2])
    fused = ops.filter_block256(x, sd, "n", film, PAD_ROWS, skip=skip, up=(UP2_W(), UP2_B()), **kw)
    h = ops.filter_block256(x, sd, "n", film, PAD_ROWS, skip=skip, **kw)
    ref, _ = ops.conv1d(h, UP2_W(), UP2_B(), transposed=True)
    return fused, ref


def wave_pair(n, l, lf, rng=None):
    """(fused, block -> alive_filter_source_out) on the same inputs"""
    from module import ops
    sd, fw = block_weights(8)
    x = g(f"fs.x8.{n}.{l}", (n, 8, l)).to(DEV)
    film = film_of(fw, n, lf, f"8.{n}.{lf}")
    kw = {} if rng is None else dict(t0=rng[0], f0=rng[1], frames=rng[2])
    fused = ops.filter_block_small_wave(x, sd, "n", film, PAD_ROWS, OUT_W(), OUT_B(), **kw)
    h = ops.filter_block_small_range(x, sd, "n", film, PAD_ROWS, **kw)
    ref = ops.filter_source_out(h, OUT_W(), OUT_B())
    return fused, ref


# the bench shape; lengths that are no multiple of the tile (456 columns); one column more than a tile; the shortest signal a
# one-frame FiLM table allows (a 512-column tile may span 7 frames: 512 / L <= 7); N = 3
@pytest.mark.parametrize("n,l,lf", [(2, 72000, 450), (2, 5004, 32), (2, 460, 3), (1, 456, 3), (2, 76, 1), (3, 2400, 15)])
@pytest.mark.parametrize("with_skip", [True, False])
def test_block16_with_ups3_in_its_store_phase_is_the_two_launches(n, l, lf, with_skip):
    fused, ref = up_pair(n, l, lf, with_skip)
    assert fused.shape == ref.shape == (n, 8, 2 * l)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    assert torch.equal(fused, ref)


# the bench shape; lengths that are no multiple of the tile (512 columns); the shortest signal the entry point takes (one tile: below
# it the decoder keeps the separate launch); N = 3
@pytest.mark.parametrize("n,l,lf", [(2, 36000, 450), (2, 5004, 62), (2, 516, 6), (2, 512, 6), (3, 1200, 15)])
@pytest.mark.parametrize("with_skip", [True, False])
def test_block64_with_ups2_in_its_store_phase_is_the_two_launches(n, l, lf, with_skip):
    from module import ops
    fused, ref = up64_pair(n, l, lf, with_skip)
    assert fused.shape == ref.shape == (n, 16, 2 * l)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    assert torch.equal(fused, ref)
    assert ops.f16_saturations() == 0


# the bench shape (150 tiles of 960 exactly: the last tile emits the window's last three samples itself); ragged lengths; a last tile
# that holds four columns; the shortest signal with a one-frame table (1024 / L <= 7); N = 3
@pytest.mark.parametrize("n,l,lf", [(2, 144000, 450), (2, 10004, 32), (2, 1924, 6), (1, 960, 3), (2, 964, 3), (2, 148, 1), (3, 4800, 15)])
def test_block8_with_source_out_in_its_store_phase_is_the_two_launches(n, l, lf):
    fused, ref = wave_pair(n, l, lf)
    assert fused.shape == ref.shape == (n, 1, l)
    assert torch.isfinite(ref).all() and ref.abs().max() > 0
    # the reflect-left start and the zero-padded end are where a change of the tile grid would show: on their own first
    assert torch.equal(fused[:, :, :8], ref[:, :, :8]), (fused[:, :, :8], ref[:, :, :8])
    assert torch.equal(fused[:, :, -8:], ref[:, :, -8:]), (fused[:, :, -8:], ref[:, :, -8:])
    assert torch.equal(fused, ref)


def test_fused_blocks_in_a_frame_range():
    """range mode (t0 / f0 / film_ld as test_fused_filter_block_256_in_a_frame_range uses them): frames 40 .. 89 of a 128-frame window
    with the FiLM rows of those frames only -- the fused form is the two launches on the same range, every sample of it"""
    lf, f0, nf = 128, 40, 50
    for up, pair in ((80, lambda l, r: up64_pair(1, l, nf, True, r)), (160, lambda l, r: up_pair(1, l, nf, True, r)),
                     (320, lambda l, r: wave_pair(1, l, nf, r))):
        fused, ref = pair(up * nf, (up * f0, f0, lf))
        whole_f, whole_r = pair(up * nf, None)                       # (the same samples as a window of their own: other coordinates)
        assert torch.equal(fused, ref) and torch.equal(whole_f, whole_r)


def test_fused_blocks_refuse_what_they_do_not_run():
    from module import ops
    sd16, fw16 = block_weights(16)
    sd8, fw8 = block_weights(8)
    for l, lf in ((16, 1), (72, 1)):                                  # the reflect pad of the last convs; a tile over more than 7 frames
        with pytest.raises(ValueError, match="alive_filter_block_small"):
            ops.filter_block_small_up(torch.zeros(1, 16, l, device=DEV), sd16, "n", film_of(fw16, 1, lf, "r16"), PAD_ROWS, UP_W(), UP_B())
    for l, lf in ((16, 1), (144, 1)):
        with pytest.raises(ValueError, match="alive_filter_block_small"):
            ops.filter_block_small_wave(torch.zeros(1, 8, l, device=DEV), sd8, "n", film_of(fw8, 1, lf, "r8"), PAD_ROWS, OUT_W(), OUT_B())
    sd64, fw64 = block_weights(64)
    with pytest.raises(ValueError, match="at least one tile of 512"):
        ops.filter_block256(torch.zeros(2, 64, 508, device=DEV), sd64, "n", film_of(fw64, 2, 6, "r64"), PAD_ROWS, up=(UP2_W(), UP2_B()))
    with pytest.raises(ValueError, match="multiple of 4"):
        ops.filter_block_small_wave(torch.zeros(1, 8, 1002, device=DEV), sd8, "n", film_of(fw8, 1, 4, "r8b"), PAD_ROWS, OUT_W(), OUT_B())


@pytest.mark.parametrize("c,l", [(64, 36000), (16, 72000), (8, 144000)])
def test_fused_blocks_are_deterministic_at_batch_scale(c, l):
    """128 windows (the bench's window batch), 30 launches on the same inputs: one digest"""
    from module import _native as nat
    N, lf = 128, 450
    L_ = nat.lib()
    gen = torch.Generator(device=DEV).manual_seed(5)
    film = torch.randn(N, 4128, lf, device=DEV, generator=gen)
    x = torch.randn(N, c, l, device=DEV, generator=gen)
    skip = torch.randn(N, c, l, device=DEV, generator=gen)
    st = torch.cuda.current_stream().cuda_stream
    if c == 64:
        import ctypes
        w6 = [(torch.randn(5 * 64 // 32, 64, 32, device=DEV, generator=gen) * 0.05).to(torch.float16) for _ in range(6)]      # fp16 slabs [K / 32][64][32]
        b6 = [torch.randn(64, device=DEV, generator=gen) * 0.1 for _ in range(6)]
        tw, tb = torch.randn(32, 64, device=DEV, generator=gen) * 0.12, torch.randn(32, device=DEV, generator=gen) * 0.1
        out = torch.empty(N, 16, 2 * l, device=DEV)
        nbytes = L_.alive_filter_block64s_workspace_bytes(N, l)
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        wp, bp = (ctypes.c_void_p * 6)(*[t.data_ptr() for t in w6]), (ctypes.c_void_p * 6)(*[t.data_ptr() for t in b6])

        def run():
            nat.check(L_.alive_filter_block64s_fp16_up(x.data_ptr(), N, l, wp, bp, film.data_ptr(), 4128, lf, 100, 0, 0, lf, skip.data_ptr(),
                                                       tw.data_ptr(), tb.data_ptr(), out.data_ptr(), ws.data_ptr(), nbytes, st))
    else:
        nw = L_.alive_filter_block_small_weights(c)
        w = (torch.cat([torch.randn(224, device=DEV, generator=gen) * 0.1,    # fp32 biases [7][32], then bf16 weight pairs in fp32 words
                        (torch.randn(2 * (nw - 224), device=DEV, generator=gen) * 0.1).to(torch.bfloat16).view(torch.int16).view(torch.float32)]).contiguous())
    if c == 64:
        pass
    elif c == 16:
        tw, tb = torch.randn(16, 16, device=DEV, generator=gen) * 0.25, torch.randn(16, device=DEV, generator=gen) * 0.1
        out = torch.empty(N, 8, 2 * l, device=DEV)

        def run():
            nat.check(L_.alive_filter_block_small_up_range(x.data_ptr(), N, l, w.data_ptr(), film.data_ptr(), 4128, lf, 100, 0, 0, lf,
                                                           skip.data_ptr(), tw.data_ptr(), tb.data_ptr(), out.data_ptr(), st))
    else:
        tw, tb = torch.randn(8, 7, device=DEV, generator=gen) * 0.2, torch.randn(1, device=DEV, generator=gen) * 0.1
        out = torch.empty(N, 1, l, device=DEV)

        def run():
            nat.check(L_.alive_filter_block_small_wave_range(x.data_ptr(), N, l, w.data_ptr(), film.data_ptr(), 4128, lf, 100, 0, 0, lf,
                                                             tw.data_ptr(), tb.data_ptr(), out.data_ptr(), st))
    digests = set()
    for _ in range(30):
        out.fill_(float("nan"))                                        # (every sample is written by every launch)
        run()
        assert torch.isfinite(out).all()
        digests.add(hashlib.sha256(out.cpu().numpy().tobytes()).hexdigest())
    assert len(digests) == 1, digests


CHILD = r"""
import os, sys, json, hashlib
import torch
sys.path.insert(0, os.path.join(%(root)r, "alive-vc_amd"))
from module import schema, synthetic
from module.decoder import Decoder
dec = Decoder(); dec.load_state_dict(synthetic.make_state_dict(schema.decoder_schema(), 2, "dec.")); dec = dec.to("cuda")
dg = lambda t: hashlib.sha256(t.contiguous().cpu().numpy().tobytes()).hexdigest()
out = {}
for n, lf, a, b in ((3, 450, 118, 316), (2, 97, 10, 80)):
    x = synthetic.gaussian(f"fsd.x{lf}", 61, (n, 768, lf)).cuda()
    f0 = (90.0 + 60.0 * torch.from_numpy(synthetic.uniform01(f"fsd.f0{lf}", 62, n * lf)).float()).view(n, 1, lf).cuda()
    wave, phi = dec(x, f0=f0)
    part = dec.forward_range(x[:, :, a:b].contiguous(), f0, a)
    assert torch.isfinite(wave).all() and torch.isfinite(part).all() and float(wave.abs().max()) > 0
    out[f"{n}x{lf}"] = {"wave": dg(wave), "phi": dg(phi.values), "range": dg(part), "first8": wave[0, :8].tolist(), "last8": wave[-1, -8:].tolist()}
print("RESULT " + json.dumps(out))
"""


def test_decoder_with_the_fused_route_on_and_off():
    """alive_decoder_forward and alive_decoder_forward_range on the synthetic checkpoint (seed 2) at 3 x 450 and 2 x 97 frames: the same
    waveforms and phase outputs with the fused store phases (default), with ALIVE_FINE_FUSE=1 (ups[2] a launch of its own) and with
    ALIVE_FINE_FUSE=0, which puts all three small convs back as launches (the switch is read once per process: one subprocess each)"""
    res = {}
    for name, env in (("fused", {}), ("fine_only", {"ALIVE_FINE_FUSE": "1"}), ("unfused", {"ALIVE_FINE_FUSE": "0"})):
        clean = {k: v for k, v in os.environ.items() if k != "ALIVE_FINE_FUSE"}
        r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT}], env=dict(clean, **env), capture_output=True, text=True, timeout=900)
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        assert line, (r.stdout[-1500:], r.stderr[-1500:])
        res[name] = json.loads(line[0][7:])
    assert res["fused"] == res["unfused"] and res["fine_only"] == res["unfused"], res
