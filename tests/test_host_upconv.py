"""csrc/conv_up.hip on the CPU: its gfx950 listing under the accumulation-chain rule (DESIGN.md 3.2b', common.h ALIVE_CHAIN_GAP), its
registers, and the agreement of the header, the binding table and the exports on its test-only entry points."""
import ctypes
import os
import re
import subprocess
import sys

import pytest

from module import _native as nat

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"


def test_listing_reads_a_row_tile_before_the_next_chain_starts(tmp_path):
    """A wave walks row tiles one behind the other: each tile's accumulators must be read completely (by the stores) before the
    first MFMA of the next tile, so the scan must find NO chain switch beside an unread accumulator at all -- in every store form and
    in both forms of the channel-block loop.  Two waves per SIMD (two blocks of 64 KB of LDS per CU) need at most 256 registers and
    no scratch."""
    if not os.path.exists(HIPCC):
        pytest.skip("no hipcc")
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_scan as hz
    out = str(tmp_path / "conv_up.s")
    subprocess.run([HIPCC, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                    "--cuda-device-only", "-S", os.path.join(ROOT, "alive-vc_amd", "csrc", "conv_up.hip"), "-o", out],
                   check=True, capture_output=True, timeout=900)
    r = hz.chain_gap_scan(out)
    assert r["kernels"] == 6 and r["mfma"] >= 6 * 18, r            # <ST 0..2> x <NCB 8, 0>; one and two column tiles each
    assert r["switches"] == [], r["switches"][:3]
    txt = open(out).read()
    bodies = re.findall(r"^(_Z\w*conv_up_kernel\w*):[^\n]*\n(.*?)\.end_amdhsa_kernel", txt, re.S | re.M)
    assert len(bodies) == 6
    for name, body in bodies:
        assert body.count("scratch_") == 0, name
        assert int(re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", body).group(1)) <= 256, name
        assert int(re.search(r"\.amdhsa_group_segment_fixed_size\s+(\d+)", body).group(1)) == 65536, name
        assert "v_cvt_pk_bf16_f32" in body, name                  # the split of conv_split.hip's store_X


def test_test_only_entry_points_are_declared_bound_and_exported():
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "alive_vc.h")).read(), flags=re.S)
    L = nat.lib()
    for name, args in (("alive_conv1d_tiled", [ctypes.POINTER(nat.AliveConv), ctypes.c_void_p]), ("alive_conv_up_launches", [ctypes.c_int]),
                       ("alive_conv_up_min_blocks", [ctypes.c_int])):
        decl = re.search(r"\bint\s+" + name + r"\s*\(([^)]*)\)\s*;", hdr)
        assert decl is not None, f"{name} is not declared in alive_vc.h"
        assert len(decl.group(1).split(",")) == len(args) and nat.PROTOTYPES[name] == (ctypes.c_int, args)
        assert hasattr(L, name)
    # the threshold hook: query, set, restore (no GPU needed); the counter starts at rest
    assert L.alive_conv_up_min_blocks(0) == 512
    assert L.alive_conv_up_min_blocks(3) == 3 and L.alive_conv_up_min_blocks(0) == 3
    assert L.alive_conv_up_min_blocks(-1) == 512
    assert L.alive_conv_up_launches(1) >= 0 and L.alive_conv_up_launches(0) == 0
