"""Host twin of tests/test_gpu_gemm_walks.py: the operand buffers of the custom row walks of alive_gemm_planes are proved large enough,
aligned and in the kernel's K order on the CPU, before anything is launched.

In those forms only the column index is clamped; every other term of the DMA address is taken as given, and a buffer that is one row
short faults the device instead of failing a test.  tools/gemm_walks_ref.py restates make_walk / StepWalk::advance (with the two
walks of the KB2 kernel); for every case the GPU file runs, this file asserts that the largest address + 32 lies inside the buffer the
GPU test allocates, that every address is a multiple of 8 elements (16 B: the DMA's granule), and that gathering the buffer through the
addresses gives the unfolded operand the standard walk is fed -- element for element, so the harness's unfold has the kernel's K order.
"""
import ctypes
import os
import sys

import pytest
import torch
import torch.nn.functional as F

from module import _native as nat
from module._pack import pack_conv_split, unpack_conv_split

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "tools"),):
    if _p not in sys.path:
        sys.path.insert(0, _p)
import gemm_walks_ref as GW                                          # noqa: E402

FRAME_CASES = [(cid, pl) for cid, c in GW.FRAMES.items() for pl in c[5]]


def _check_walk(buf, g, x_unf):
    idx = GW.operand_indices(g)
    assert int(idx.min()) >= 0 and GW.operand_extent(g) <= buf.numel(), (GW.operand_extent(g), buf.numel())
    assert not bool((idx % 8).any())
    assert idx.shape == (g.planes, g.cols, GW.pad32(g.Ci) // 32)
    assert torch.equal(GW.gather(buf, g), GW.unfolded_bits(x_unf, g.planes))


@pytest.mark.parametrize("cid,planes", FRAME_CASES)
def test_overlapping_rows_stay_inside_their_buffer_and_unfold_to_the_frames(cid, planes):
    c = GW.frames_case(cid, planes)
    g = c["geo"]
    assert c["buf"].numel() == planes * g.b_plane
    _check_walk(c["buf"], g, c["x_unf"])
    assert GW.kernel_instance(g) == GW.FRAMES_KERNEL.get((cid, planes), "one-tile")
    # the buffer is exactly as long as the walk needs, up to the rounding of a row to 8 elements
    assert c["buf"].numel() - GW.operand_extent(g) < 8


@pytest.mark.parametrize("cid", list(GW.CONVS))
def test_strided_rows_stay_inside_the_plane_image_and_unfold_to_the_patches(cid):
    c = GW.conv_case(cid)
    g = c["geo"]
    img = GW.planes_image(c["x"], g.planes)
    assert img.numel() == g.planes * g.b_plane and g.b_blk * (g.Ci // 32 // (g.b_row // 32)) == g.b_plane
    _check_walk(img, g, c["x_unf"])
    assert GW.kernel_instance(g) == GW.CONVS_KERNEL.get(cid, "one-tile")
    assert GW.is_kb2(g) == (GW.CONVS_KERNEL.get(cid) == "KB2")


@pytest.mark.parametrize("cid", ["chpad", "ncb3", "h-ncb3"])
def test_the_unfolded_patches_times_the_packed_weight_are_the_strided_conv(cid):
    """the harness against itself: patches in tap-major K order x the rows of pack_conv_split = F.conv1d(stride = r), in float64"""
    c = GW.conv_case(cid)
    co = c["w"].shape[0]
    rows = unpack_conv_split(pack_conv_split(c["w"], 3)).double().sum(0)[:co]               # [Co][K], three planes: fp32 exactly
    got = torch.einsum("ok,nkt->not", rows, c["x_unf"].double())
    want = F.conv1d(c["x"].double(), c["w"].double(), stride=c["r"])
    assert got.shape == want.shape and (got - want).abs().max().item() < 1e-12


def test_the_standard_walk_is_the_k_blocked_image():
    """b_row = 0: make_walk's k-block stride over planes_at is the layout alive_to_planes writes (2 and 3 planes, one fp16 plane with
    32- and 64-deep steps)"""
    x = GW.gauss("gw.std", (3, 40, 50))
    for planes in (1, 2, 3):
        _check_walk(GW.planes_image(x, planes), GW.Geo(3, 50, 40, 8, planes), F.pad(x, (0, 0, 0, 24)))
    x = GW.gauss("gw.std2", (1, 128, 70))
    _check_walk(GW.planes_image(x, 1), GW.Geo(1, 70, 128, 8, 1), x)


def test_an_odd_block_count_makes_a_kb2_step_straddle_a_tap():
    """ncb = 3, two taps: the second 64-deep step takes block 2 of tap 0 and block 0 of tap 1"""
    g = GW.conv_geo(2, 96, 260, 2, 128, 1)
    assert GW.is_kb2(g) and GW.make_walk(g)[2] == 3
    assert GW.piece_offsets(g) == [0, g.b_blk, 2 * g.b_blk, 32, 32 + g.b_blk, 32 + 2 * g.b_blk]


def test_a_buffer_one_row_short_is_noticed():
    """the extent is tight: it is what keeps the GPU twin from launching on a short buffer"""
    c = GW.frames_case("1a", 3)
    g = c["geo"]
    assert GW.operand_extent(g) == 2 * g.b_plane + (g.T - 1) * g.b_row + g.Ci
    g2 = GW.conv_geo(1, 32, 300, 2, 40, 2)
    assert GW.operand_extent(g2) == g2.b_plane + (300 - 1) * 32 + 32


@pytest.mark.parametrize("co,ys,ci,n,t,planes", [c[:5] + (pl,) for c in GW.SPLITS for pl in c[5]])
def test_split_output_cases_reach_the_kernel_they_are_meant_for(co, ys, ci, n, t, planes):
    assert ys % 128 == 0 and 0 < ys < co
    want = "persistent" if (co, planes) == (2120, 3) else "one-tile"
    assert GW.kernel_instance(GW.Geo(n, t, ci, co, planes)) == want


def test_magnitude_and_plane_output_cases_reach_the_kernel_they_are_meant_for():
    assert [GW.kernel_instance(GW.Geo(n, t, ci, co, 3)) for co, ci, n, t in GW.MAGS] == ["one-tile", "persistent"]
    assert all(GW.kernel_instance(GW.Geo(n, t, ci, co, 3)) == "persistent" for co, ci, n, t in GW.POUTS)
    hop, ci, n, t, co, _ = GW.FRAMES["1c"]
    assert co % 2 == 0 and GW.kernel_instance(GW.frames_case("1c", 3)["geo"]) == "one-tile"


@pytest.mark.parametrize("case", GW.REFUSALS, ids=lambda c: c.name)
def test_refusals_are_decided_on_the_host(case):
    """alive_gemm_planes turns these descriptors down before it touches the device or a pointer (any 16-byte aligned address will do)"""
    room = ctypes.create_string_buffer(64)
    addr = (ctypes.addressof(room) + 15) & ~15
    d = GW.refusal_descriptor(nat.AliveGemm, case, lambda name: addr)
    with pytest.raises(ValueError) as e:
        nat.check(nat.lib().alive_gemm_planes(ctypes.byref(d), None), "alive_gemm_planes")
    assert case.message in str(e.value), str(e.value)
