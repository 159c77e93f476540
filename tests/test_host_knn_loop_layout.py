"""Block placement in the main loops of the scoring kernels built from knn_score8_body (csrc/knn.hip), on the gfx950 listing.

A block runs one wave per SIMD, so nothing else issues while that wave's fetch is redirected: the tile loop has to run straight through.
For each kernel the main loop is the backward branch whose span holds the most MFMAs (two tile bodies); every forward conditional branch
inside that span must leave it -- the admission path (fold_rare / fold_loop) and anything else that is rare sit behind the loop, and in
the common case the back edge is the only branch taken.  This test looks at branch targets and nothing else; the MFMA counts, waited-for
asm reads, chain gaps and registers of the bodies are the other listing tests'."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MFMA = "v_mfma_scale_f32_32x32x64_f8f6f4"
# kernel -> MFMAs of the loop: two tile bodies of NK k-steps x NCT8 column tiles
LOOPS = {"knn_score8_kernel": 2 * 12 * 2, "knn_score6_kernel": 2 * 12 * 3, "knn_sub6_kernel": 2 * 8 * 3, "knn_sub6w_kernel": 2 * 8 * 4}


@pytest.fixture(scope="module")
def listing(tmp_path_factory):
    hipcc = "/opt/rocm/bin/hipcc"
    if not os.path.exists(hipcc):
        pytest.skip("no hipcc")
    out = tmp_path_factory.mktemp("knn_loop_layout") / "knn.s"
    src = os.path.join(ROOT, "alive-vc_amd", "csrc", "knn.hip")
    subprocess.run([hipcc, "-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "-Wno-unused-function",
                    "--cuda-device-only", "-S", src, "-o", str(out)], check=True, capture_output=True, timeout=600)
    return out.read_text().split("\n")


def main_loop(body):
    """-> (first line, last line, MFMAs) of the backward branch of `body` whose span holds the most MFMAs, and every branch of the body
    as (line, conditional, target line)"""
    label = {}
    for i, l in enumerate(body):
        m = re.match(r"(\.LBB\d+_\d+):", l)
        if m:
            label[m.group(1)] = i
    branches = []
    for i, l in enumerate(body):
        m = re.match(r"\s+s_(c?)branch\S*\s+(\.LBB\d+_\d+)", l)
        if m:
            branches.append((i, m.group(1) == "c", label[m.group(2)]))
    mfma_at = [i for i, l in enumerate(body) if MFMA in l]
    best = None
    for i, _, t in branches:
        if t < i:
            n = sum(1 for j in mfma_at if t < j < i)
            if best is None or n > best[2]:
                best = (t, i, n)
    return best, branches


@pytest.mark.parametrize("kernel", sorted(LOOPS))
def test_every_forward_branch_of_the_tile_loop_leaves_it(listing, kernel):
    ls = listing
    start = [i for i, l in enumerate(ls) if kernel in l and l.startswith("_ZN") and ":" in l][0]
    end = [i for i, l in enumerate(ls) if i > start and ".amdhsa_kernel" in l][0]
    body = ls[start:end]
    loop, branches = main_loop(body)
    assert loop is not None
    lo, hi, n_mfma = loop
    assert n_mfma == LOOPS[kernel], (n_mfma, lo, hi)
    inside = [(i, t) for i, cond, t in branches if cond and lo < i < hi and t > i and t <= hi]
    assert not inside, [(body[i].strip(), body[t].strip()) for i, t in inside]
    # and no unconditional jump over a block inside the span either: the loop is one straight run of code
    assert not [(i, t) for i, cond, t in branches if not cond and lo < i < hi and i < t <= hi]
    m = re.search(r"\.name:\s+\S*" + kernel + r"\S*\n(.*?)\.wavefront_size", "\n".join(ls), re.S).group(1)
    assert re.search(r"\.vgpr_spill_count:\s+0\b", m) and re.search(r"\.private_segment_fixed_size:\s+0\b", m), m
