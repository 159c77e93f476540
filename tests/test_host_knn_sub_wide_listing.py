"""The wide subspace fp6 scoring kernel (csrc/knn.hip knn_sub6w_kernel, K = 512, 128 stationary frames per wave) on its gfx950 listing:
32 MFMAs per tile body over three tile bodies on six-register e2m3 operands, two accumulator sets of four tuples that nothing writes
between the MFMAs of the loop, its asm fragment reads waited for, no spills and no scratch."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KERNEL = "knn_sub6w_kernel"


def test_wide_subspace_scoring_kernel_listing(tmp_path):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path / "knn.s"
    src = os.path.join(ROOT, "alive-vc_amd", "csrc", "knn.hip")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                    "--cuda-device-only", "-S", src, "-o", str(out)], check=True, capture_output=True, timeout=600)
    ls = out.read_text().split("\n")
    start = [i for i, l in enumerate(ls) if KERNEL in l and l.startswith("_ZN") and ":" in l][0]
    end = [i for i, l in enumerate(ls) if i > start and ".amdhsa_kernel" in l][0]
    body = ls[start:end]
    mf = [i for i, l in enumerate(body) if "v_mfma_scale_f32_32x32x64_f8f6f4" in l]
    assert len(mf) == 96, len(mf)
    assert all("cbsz:2 blgp:2" in body[i] for i in mf)
    # destination tuple, A operand, B operand (either register file: half of the stationary fragments live in AGPRs)
    ops = [re.search(r"f8f6f4 (a\[\d+:\d+\]), ([av]\[(\d+):(\d+)\]), ([av]\[(\d+):(\d+)\])", body[i]) for i in mf]
    assert all(o and int(o.group(4)) - int(o.group(3)) == 5 and int(o.group(7)) - int(o.group(6)) == 5 for o in ops)
    # the two bodies of the loop: 2 x 32 MFMAs into two accumulator sets of four tuples, and nothing but MFMAs writes an AGPR there
    # (no zeroing, no copy at the tile boundary: the first MFMA of a chain takes C = 0, the fold reads the previous set in place)
    assert len({o.group(1) for o in ops[:64]}) == 8
    code = [l.strip() for l in body]
    assert not [code[i] for i in range(mf[0], mf[63]) if code[i].startswith("v_accvgpr_write")]
    # rho rides one tile ahead: inside the tile bodies the only vmcnt(0) is the barrier's
    for i in range(mf[0], mf[-1]):
        if code[i].startswith("s_waitcnt") and "vmcnt(0)" in code[i]:
            nxt = next(c for c in code[i + 1:] if c and not c.startswith(";"))
            assert nxt.startswith("s_barrier"), (i, code[i], nxt)
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    import mfma_hazard_scan as hz
    n_asm, unwaited = hz.asm_lds_reads_are_waited_for(str(out), KERNEL)
    assert n_asm == 24 and unwaited == 0, (n_asm, unwaited)
    r = hz.chain_gap_scan(str(out))
    assert not [s for s in r["switches"] if s[4] < hz.CHAIN_GAP_MIN]
    meta = "\n".join(ls)
    m = re.search(r"\.name:\s+\S*" + KERNEL + r"\S*\n(.*?)\.wavefront_size", meta, re.S).group(1)
    assert re.search(r"\.vgpr_spill_count:\s+0\b", m) and re.search(r"\.private_segment_fixed_size:\s+0\b", m), m
