"""The subspace form of the fp6 candidate stage (csrc/knn.hip knn_sub6_kernel, PackedLibrary.set_subspace): on content-encoder
frames it returns the lists of the plain fp6 and the strict searches bitwise; frames outside the encoder's output subspace fall back
(per frame, or the whole batch) and still get exact lists."""
import pytest
import torch

from module.common import PackedLibrary
from module.content_encoder import ContentEncoder

pytestmark = pytest.mark.gpu


def _encoder_frames(seed, scale=1.0, n=4, t=450):
    ce = ContentEncoder(seed=seed).to("cuda")
    if scale != 1.0:
        ce.load_state_dict({k: v * scale if k.startswith("output_layer") else v for k, v in ce.state_dict().items()})
    g = torch.Generator(device="cuda").manual_seed(seed)
    spec = torch.rand(n, 641, t, device="cuda", generator=g)
    feat = ce(spec)
    sd = ce._sd
    return feat.contiguous(), sd["output_layer.weight"], sd["output_layer.bias"]


def _libs(M=20000, seed=11):
    tok = torch.randn(768, M, device="cuda", generator=torch.Generator(device="cuda").manual_seed(seed))
    plain = PackedLibrary(tok, prefilter="fp6", strict=False)
    return plain, tok


def _check_against_plain_and_strict(feat, w, b):
    plain, tok = _libs()
    assert plain.prefilter == "fp6"
    sub = plain.with_prefilter("fp6")
    sub.set_subspace(w, b)
    assert sub.sub is not None
    strict = plain.with_strict()
    v0, i0 = plain.search(feat, 4)
    st0 = plain.search_stats()
    v1, i1 = sub.search(feat, 4)
    st = sub.search_stats()
    v2, i2 = strict.search(feat, 4)
    torch.cuda.synchronize()
    assert st["stage_form"] == "subspace" and st["frames_left_subspace"] == 0, st
    assert torch.equal(i1, i0) and torch.equal(v1, v0)
    assert torch.equal(i1, i2) and torch.equal(v1, v2)
    # the lists are exact whatever the stage does (the tiers behind it catch a bad candidate set): the stage must also certify about
    # as many frames as the plain one, or it did not do the scoring
    f0, f1 = st0["frames_failed_fp8_certificate"], st["frames_failed_fp8_certificate"]
    assert f1 <= 2 * f0 + 16, (f0, f1, st)
    return st


@pytest.mark.parametrize("seed,scale", [(2, 1.0), (3, 1.0), (5, 1.0), (2, 4.0)])
def test_subspace_search_matches_plain_and_strict(seed, scale):
    feat, w, b = _encoder_frames(seed, scale)
    _check_against_plain_and_strict(feat, w, b)


def test_large_out_of_span_bias_needs_the_g_rho_term():
    """the encoders above have g ~ 0.005, so g rho ~ 1e-4 hides under the fp6 error: with a bias that has a large part outside span(W)
    (g ~ 0.3, g rho ~ 1e-2) a missing or misplaced rho term would fail most frames' certificates"""
    ce = ContentEncoder(seed=2).to("cuda")
    sd = ce.state_dict()
    W = sd["output_layer.weight"].reshape(768, 512).double()
    U = torch.linalg.qr(W.cpu())[0].cuda()
    v = torch.randn(768, dtype=torch.float64, device="cuda", generator=torch.Generator(device="cuda").manual_seed(9))
    v -= U @ (U.t() @ v)
    v /= v.norm()
    feat0, _, _ = _encoder_frames(2)
    m = float(feat0.norm(dim=1).mean())
    sd["output_layer.bias"] = (sd["output_layer.bias"].double() + 0.35 * m * v).float()
    ce.load_state_dict(sd)
    g = torch.Generator(device="cuda").manual_seed(2)
    feat = ce(torch.rand(4, 641, 450, device="cuda", generator=g)).contiguous()
    w, b = ce._sd["output_layer.weight"], ce._sd["output_layer.bias"]
    bp = b.double() - U @ (U.t() @ b.double())
    u = bp / bp.norm()
    gf = torch.einsum("d,ndt->nt", u, feat.double()) / feat.double().norm(dim=1)
    assert float(gf.abs().mean()) > 0.2, float(gf.abs().mean())
    _check_against_plain_and_strict(feat, w, b)


def test_random_and_perturbed_frames_fall_back_exactly():
    feat, w, b = _encoder_frames(2)
    plain, tok = _libs()
    sub = plain.with_prefilter("fp6")
    sub.set_subspace(w, b)
    strict = plain.with_strict()
    g = torch.Generator(device="cuda").manual_seed(5)
    rnd = torch.randn(feat.shape, device="cuda", generator=g)
    v1, i1 = sub.search(rnd, 4)
    st = sub.search_stats()
    v2, i2 = strict.search(rnd, 4)
    assert st["stage_form"] == "plain" and st["frames_left_subspace"] > 64, st
    assert torch.equal(i1, i2) and torch.equal(v1, v2)
    # a few perturbed frames: flagged one by one, the rest of the batch stays on the subspace kernel
    pert = feat.clone()
    pert[0, :, :10] += 0.2 * feat[0, :, :10].norm(dim=0) * torch.randn(768, 10, device="cuda", generator=g) / 768 ** 0.5
    v1, i1 = sub.search(pert, 4)
    st = sub.search_stats()
    v2, i2 = strict.search(pert, 4)
    assert st["stage_form"] == "subspace" and 10 <= st["frames_left_subspace"] <= 64, st
    assert torch.equal(i1, i2) and torch.equal(v1, v2)


def test_clipped_frames_are_forwarded():
    feat, w, b = _encoder_frames(3)
    plain, tok = _libs()
    sub = plain.with_prefilter("fp6")
    sub.set_subspace(w, b)
    strict = plain.with_strict()
    # frames along one basis direction of the subspace: a coordinate of 1 (x 32 = 32) clips e2m3
    U = torch.linalg.qr(w.reshape(768, 512).double().cpu())[0].float().cuda()
    clip = feat.clone()
    clip[1, :, :5] = U[:, :5]
    v1, i1 = sub.search(clip, 4)
    st = sub.search_stats()
    v2, i2 = strict.search(clip, 4)
    assert st["stage_form"] == "subspace" and st["frames_clipped"] >= 5, st
    assert torch.equal(i1, i2) and torch.equal(v1, v2)


def test_graph_captured_subspace_search():
    feat, w, b = _encoder_frames(5, n=2)
    plain, tok = _libs()
    sub = plain.with_prefilter("fp6")
    sub.set_subspace(w, b)
    ref_v, ref_i = sub.search(feat, 4)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        sub.search(feat, 4)
    torch.cuda.current_stream().wait_stream(s)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out_v, out_i = sub.search(feat, 4)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out_i, ref_i) and torch.equal(out_v, ref_v)
