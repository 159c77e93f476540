"""Drop-in for the inference-time surface of the reference's module/common.py.

  match_features(source, reference, k=4, alpha=0.0)   <- /root/reference/module/common.py:96-109
  compute_f0_dio(wf, sample_rate=8000, ...)           <- module/common.py:113-130 (pyworld.dio + stonemask, `-wpe`)
  compute_f0(wf, sample_rate=16000, segment_size=320) <- module/common.py:133-137
  compute_f0_rows(wf, row_on)                         compute_f0 of the rows a device mask switches on (the batched paths)
  pitch_track(lo=50, hi=1100, band=2.0, device=)      the tables of the pitch tracker (F0Estimator.estimate(track=); no counterpart)
  voicing_options(v, where="")                        the checked settings of the voicing decision (ops.voicing_rows_; no counterpart)
  path_options(v, what="match_path")                  the checked settings of the match path (ops.knn_path_rows; no counterpart)

runs on the MI355X through libalive_vc.so: fp6- (or fp8- / bf16-) MFMA candidate scoring with
LDS-staged top-k' lists, exact fp32 rescoring, gather-mean-blend.  The library
is packed (normalised fp6 / fp8 / bf16 rows + fp32 rows + norms) once per reference tensor
and cached, so the per-window calls of inference.py:129 only pay for the search.
"""
import ctypes
import os
import weakref

import torch

from . import _native as nat

DIM = 768
# Candidate stage of the search: "fp6" (block-scaled e2m3 MFMA at twice the fp8 rate, 96 stationary frames per wave; round 5),
# "fp8" (block-scaled e4m3 MFMA) -- both 32 candidates per frame and library split -- or "bf16" (16 candidates); all of them
# feed the same exact fp32 rescoring and the same per-frame certificate.  env ALIVE_KNN_PREFILTER overrides.
DEFAULT_PREFILTER = "fp6"
_STAGES = ("bf16", "fp8", "fp6")


def _prefilter():
    return os.environ.get("ALIVE_KNN_PREFILTER", DEFAULT_PREFILTER)


def _rotate_allowed():
    """ALIVE_KNN_ROTATE=0 switches the rotated form of the fp8 stage off (dense banks then go through the bf16 stage as in round 5)"""
    return os.environ.get("ALIVE_KNN_ROTATE", "1") not in ("0", "false", "False")


# A bank is searched on ROTATED fp8 operands (csrc/knn.hip rot_codes_kernel, include/alive_vc.h) when it is DENSE -- its rows share a
# common component: the leading eigenvalue of the unit rows' second moment carries at least ROT_MIN_LEAD of the trace -- and lives in a
# subspace of at most 571 dimensions (the reference's ContentEncoder ends in Conv1d(512 -> 768): every bank it produces does).
ROT_MIN_LEAD = 0.10
ROT_MAX_TAIL = 1.0e-9


def _strict():
    """ALIVE_KNN_STRICT=1: every search through the bf16 stage with the DETERMINISTIC certificate (no statistical
    assumption; include/alive_vc.h: alive_knn_search_strict).  The default certificates are statistical (7 sigma of the
    measured stage error; audited in profiles/r03_knn_audit.json)."""
    return os.environ.get("ALIVE_KNN_STRICT", "0") not in ("0", "", "false", "False")


class PackedLibrary:
    """Device-resident search form of a voice library tokens[768, M] (one shard).

    lib_bf16[M_pad,768] normalised rows (MFMA operand), rows[M,768] fp32 raw rows,
    norms[M], rows_hat[M,768] = rows / norms (the rescoring passes read the quotients instead of
    forming them on every call; 3 KB per row).  `idx_base` is the global index of row 0 when the library is sharded."""

    def __init__(self, tokens_DxM: torch.Tensor, idx_base: int = 0, prefilter: str = None, strict: bool = None):
        self.strict = _strict() if strict is None else bool(strict)
        self.prefilter = "bf16" if self.strict else (prefilter or _prefilter())
        if self.prefilter not in _STAGES:
            raise ValueError(f"prefilter must be one of {_STAGES}, got {self.prefilter!r}")
        if tokens_DxM.dim() != 2 or tokens_DxM.shape[0] != DIM:
            raise ValueError(f"library must be [768, M], got {tuple(tokens_DxM.shape)}")
        t = tokens_DxM.contiguous().float()
        L = nat.lib()
        self.M = int(t.shape[1])
        self.idx_base = int(idx_base)
        m_pad = L.alive_library_padded_rows(self.M)
        dev = t.device
        self.lib_bf16 = torch.empty(m_pad, DIM, dtype=torch.bfloat16, device=dev)
        self.rows = torch.empty(self.M, DIM, dtype=torch.float32, device=dev)
        self.norms = torch.empty(self.M, dtype=torch.float32, device=dev)
        nat.check(L.alive_library_pack(nat.ptr(t), self.M, DIM, nat.ptr(self.lib_bf16), nat.ptr(self.rows),
                                       nat.ptr(self.norms), nat.stream()), "alive_library_pack")
        # A zero-norm (or non-finite) row: the reference divides it by its norm (common.py:103) and the NaN cosines that
        # follow rank first in every frame's top-k, i.e. the row silently joins every match.  Here it is an error of the
        # library (one reduction + sync per pack, which happens once per bank).
        bad = ~(torch.isfinite(self.norms) & (self.norms > 0))
        if bool(bad.any()):
            first = int(torch.nonzero(bad)[0])
            raise ValueError(f"voice library row {first + self.idx_base} has zero or non-finite norm ({int(bad.sum())} such rows): "
                             f"remove them (the reference would match every frame to them through NaN cosines)")
        # unit rows, once per library (the copies of with_prefilter / with_strict share them); `rows` stays: merge_gather returns the
        # original rows, and fl(fl(x / n) n) != x
        self.rows_hat = torch.empty_like(self.rows)
        nat.check(L.alive_library_pack_unit_rows(nat.ptr(self.rows), nat.ptr(self.norms), self.M, nat.ptr(self.rows_hat), nat.stream()),
                  "alive_library_pack_unit_rows")
        self.lib_f8 = None                 # the fp8 OR the fp6 image of the rows (same size and tile layout), per self.prefilter
        self.fp6_declined = False
        self.rot = None                    # rotated fp8 stage: {"W": packed 1x1 conv weights of the basis, "spectrum": ...}
        if self.prefilter in ("fp6", "fp8") and self.M >= 4096 and _rotate_allowed():
            self._try_rotated()            # a dense bank: the fp8 stage on rotated operands (sets self.rot, self.lib_f8, prefilter "fp8")
        if self.rot is None and self.prefilter == "fp6" and self.M > 0:
            # e2m3 x 2^5 ends at 7.5 / 32 = 0.234: a row of a unit-norm library with a larger element (a few dominant coordinates:
            # "spiky" banks, never a dense content-encoder bank, whose elements are ~0.036 +- a few sigma) would be CLIPPED, and a clipped
            # row's score is low by more than any per-frame error statistic shows -- such a library is searched through the fp8 stage
            # (e4m3 x 2^8 reaches 1.75).  One reduction + sync per pack.  (A frame that clips is caught per search: knn.hip force_fail.)
            if self._fp6_would_clip():
                self.prefilter, self.fp6_declined = "fp8", True
        if self.rot is None and self.prefilter in ("fp8", "fp6"):
            self.lib_f8 = self._pack_stage(self.prefilter)
        self.sub = None                    # subspace fp6 stage (set_subspace): {"W": packed 1x1 conv weights, "lib": codes, "rho": ...}
        self.sub_forms = []                # forms built for recent encoders: (weight, its version, bias, its version, form or None)
        self.bound = None
        self.lib_lo = None
        if self.strict:
            self._make_bound()
        self._ws = nat.Workspace()

    def _fp6_would_clip(self):
        if self.M == 0:
            return False
        lo, hi = torch.aminmax(self.lib_bf16[:self.M])        # (no |x| temporary: the image is 1.5 GB at 1 M rows)
        return max(-float(lo), float(hi)) > 7.75 / 32.0

    def _pack_stage(self, prefilter):
        L = nat.lib()
        buf = torch.empty(L.alive_library_fp8_bytes(self.M), dtype=torch.uint8, device=self.rows.device)
        fn = L.alive_library_pack_fp6 if prefilter == "fp6" else L.alive_library_pack_fp8
        nat.check(fn(nat.ptr(self.lib_bf16), self.M, nat.ptr(buf), nat.stream()), "alive_library_pack_" + prefilter)
        return buf

    def _try_rotated(self, chunk=131072):
        """Decide whether this bank is searched on rotated fp8 operands and, if so, build the basis and the rows' codes (once per bank:
        torch is used for the 768 x 768 second moment, its eigen-decomposition and the rows' change of basis -- pack-time plumbing; the
        codes, the frames' change of basis (alive_conv1d) and the search are the library's own kernels)."""
        from ._pack import pack_conv_split
        L = nat.lib()
        rc, ra, rm = L.alive_knn_rot_coordinates(), L.alive_knn_rot_leading(), L.alive_knn_rot_mixed()
        used = ra + rm                                          # 571 directions carry the bank; the 5 coordinates behind them are not read
        dev = self.rows.device
        C = torch.zeros(DIM, DIM, dtype=torch.float64, device=dev)
        mean = torch.zeros(DIM, dtype=torch.float64, device=dev)
        for s0 in range(0, self.M, chunk):
            ln = self.rows[s0:s0 + chunk] / self.norms[s0:s0 + chunk, None]
            C += (ln.t() @ ln).double()
            mean += ln.double().sum(0)
        evals, evecs = torch.linalg.eigh((C / self.M).cpu())
        order = torch.argsort(evals, descending=True)
        evals, U = evals[order].clamp(min=0.0), evecs[:, order]
        total = float(evals.sum())
        lead, tail = float(evals[0]) / total, float(evals[used:].sum()) / total
        self.rot_spectrum = {"leading_eigenvalue_share": lead, "energy_beyond_571_directions": tail}
        if not (lead >= ROT_MIN_LEAD and tail <= ROT_MAX_TAIL):
            return
        a0 = float((mean.cpu() / self.M) @ U[:, 0])             # mean of the rows' leading coordinate: make it positive
        if a0 < 0:
            U[:, 0], a0 = -U[:, 0], -a0
        c0 = float((torch.tensor([a0 * 256.0]).to(torch.float8_e4m3fn).float() / 256.0)[0])      # e4m3-exact centring constant
        g = torch.Generator().manual_seed(20261004)
        R = torch.linalg.qr(torch.randn(rm, rm, generator=g, dtype=torch.float64))[0]
        W = torch.zeros(DIM, rc, dtype=torch.float64)
        W[:, :ra] = U[:, :ra]
        W[:, ra:used] = U[:, ra:used] @ R
        W = W.float().to(dev)                                   # [768, 576]: 571 orthonormal columns, 5 zero ones
        buf = torch.empty(L.alive_library_fp8_bytes(self.M), dtype=torch.uint8, device=dev)
        for s0 in range(0, self.M, chunk):                                                    # (chunk is a multiple of 32)
            ln = self.rows[s0:s0 + chunk] / self.norms[s0:s0 + chunk, None]
            y = (ln @ W).contiguous()
            nat.check(L.alive_library_pack_fp8_rot(nat.ptr(y), s0, y.shape[0], self.M, c0, nat.ptr(buf), nat.stream()), "alive_library_pack_fp8_rot")
        self.lib_f8 = buf
        self.prefilter = "fp8"
        # the frames' change of basis is a 1x1 conv 768 -> 576 on two bf16 planes (2^-16: far below the stage's 8-bit digits)
        self.rot = {"W": pack_conv_split(W.t().contiguous().unsqueeze(2), 2), "co": rc, "basis": W, "c0": c0}

    def use_subspace(self, weight, bias):
        """set_subspace for the encoder output layer (weight, bias) unless this library already holds its form: the last few forms are
        kept by the tensors themselves (strong references, so an identity cannot be reused) and their versions, so converters with
        different encoders that share a library do not repack it on every search"""
        for f in self.sub_forms:
            if f[0] is weight and f[1] == weight._version and f[2] is bias and f[3] == bias._version:
                self.sub = f[4]
                return self
        self.set_subspace(weight, bias)
        self.sub_forms = [(weight, weight._version, bias, bias._version, self.sub)] + self.sub_forms[:3]
        return self

    def set_subspace(self, weight, bias, chunk=131072):
        """Search through the subspace form of the fp6 stage (csrc/knn.hip knn_sub6_kernel): frames of the form q = weight h + bias
        (the content encoder's output_layer, weight [768, 512(, 1)]) are scored on their 512 coordinates in an orthonormal basis U of
        span(weight) plus g rho along u, the unit part of bias outside span(weight).  A frame that is not of that form is caught on the
        device and goes to the next tier (or, many of them, the whole batch to the plain fp6 stage): a wrong basis costs time, never
        results.  Only a plain fp6 library takes the form; the basis is built in float64, the rows' codes by alive_library_pack_fp6_sub.
        """
        from ._pack import pack_conv_split
        if self.prefilter != "fp6" or self.strict or self.rot is not None or self.lib_f8 is None or self.M == 0:
            self.sub = None
            return self
        L = nat.lib()
        dev = self.rows.device
        Wt = weight.detach().reshape(DIM, -1).to("cpu", torch.float64)
        b = bias.detach().reshape(DIM).to("cpu", torch.float64)
        U = torch.linalg.qr(Wt)[0]                               # [768, 512] orthonormal basis of span(W)
        bp = b - U @ (U.t() @ b)
        nb = float(bp.norm())
        u = bp / nb if nb > 1e-9 * max(1.0, float(b.norm())) else torch.zeros_like(bp)
        co = L.alive_knn_sub_coordinates()
        B = torch.zeros(DIM, co, dtype=torch.float64)
        B[:, :U.shape[1]] = U
        B[:, 512] = u
        B = B.float().to(dev)
        lib = torch.empty(L.alive_library_fp6_sub_bytes(self.M), dtype=torch.uint8, device=dev)
        rho = torch.empty(L.alive_library_padded_rows(self.M), dtype=torch.float32, device=dev)
        clip = torch.zeros(1, dtype=torch.int32, device=dev)
        for s0 in range(0, self.M, chunk):                                                    # (chunk is a multiple of 32)
            y = ((self.rows[s0:s0 + chunk] / self.norms[s0:s0 + chunk, None]) @ B).contiguous()
            nat.check(L.alive_library_pack_fp6_sub(nat.ptr(y), s0, y.shape[0], self.M, nat.ptr(lib), nat.ptr(rho), nat.ptr(clip),
                                                   nat.stream()), "alive_library_pack_fp6_sub")
        if int(clip.item()) != 0:                  # a row coordinate beyond e2m3's range: keep the plain stage (as _fp6_would_clip)
            self.sub = None
            return self
        # "W": [U | u]^T as two k-blocked bf16 planes -- the weight operand of alive_gemm_planes and of alive_conv1d's split form alike
        self.sub = {"W": pack_conv_split(B.t().contiguous().unsqueeze(2), 2), "co": co, "lib": lib, "rho": rho, "basis": B}
        return self

    def _rotate_frames(self, source, form=None):
        """source [n, 768, t] -> W^T source [n, co, t] through alive_conv1d (split bf16): the rotated fp8 stage's basis, or form["W"]"""
        import ctypes as C
        form = self.rot if form is None else form
        n, d, t = source.shape
        y = torch.empty(n, form["co"], t, device=source.device)
        W = form["W"]
        dsc = nat.AliveConv()
        dsc.W, dsc.bias, dsc.X = nat.ptr(W), None, nat.ptr(source)
        dsc.N, dsc.Ci, dsc.Tin, dsc.Co, dsc.K_pad = n, d, t, form["co"], W.shape[1] * 32
        dsc.precision, dsc.Ci_pad = 1, d
        dsc.KW, dsc.stride, dsc.dil, dsc.pad_left, dsc.pad_mode = 1, 1, 1, 0, 0
        dsc.Tout, dsc.up, dsc.act = t, 1, 0
        dsc.Y = nat.ptr(y)
        nat.check(nat.lib().alive_conv1d(C.byref(dsc), nat.stream()), "alive_conv1d (frames -> the bank's basis)")
        return y

    def _make_bound(self):
        """max_R || r^ - bf16(r^) ||: the library's share of the strict certificate's deterministic bound -- and the library's lo
        plane bf16(r^ - bf16(r^)) for the split-bf16 collect tier behind it (ALIVE_KNN_STRICT_SPLIT=0: without, the round-3 form)"""
        self.bound = torch.zeros(1, dtype=torch.float32, device=self.rows.device)
        nat.check(nat.lib().alive_library_rounding_bound(nat.ptr(self.lib_bf16), nat.ptr(self.rows), nat.ptr(self.norms), self.M,
                                                         nat.ptr(self.bound), nat.stream()), "alive_library_rounding_bound")
        self.lib_lo = None
        if os.environ.get("ALIVE_KNN_STRICT_SPLIT", "1") not in ("0", "false", "False"):
            self.lib_lo = torch.empty_like(self.lib_bf16)
            nat.check(nat.lib().alive_library_pack_lo(nat.ptr(self.lib_bf16), nat.ptr(self.rows), nat.ptr(self.norms), self.M,
                                                      nat.ptr(self.lib_lo), nat.stream()), "alive_library_pack_lo")

    def search(self, source, k, events=None):
        """exact top-k of this shard: (val[Tt,k] fp32 desc, idx[Tt,k] int32 global).
        events = (start, stop): torch.cuda.Event pair recorded around the first-stage scoring kernel (measurement)."""
        n, d, t = source.shape
        L = nat.lib()
        val = torch.empty(n * t, k, dtype=torch.float32, device=source.device)
        idx = torch.empty(n * t, k, dtype=torch.int32, device=source.device)
        split = self.strict and self.lib_lo is not None          # the split-bf16 collect tier needs the frames' two planes as well
        sub = self.sub is not None and self.prefilter == "fp6" and not self.strict and self.rot is None
        wsb = L.alive_knn_workspace_bytes_strict if split else (L.alive_knn_workspace_bytes_sub if sub else L.alive_knn_workspace_bytes_fast)
        ws = self._ws.get(wsb(n * t, self.M), source.device)
        a = nat.AliveKnnSearch()
        a.N, a.T, a.k, a.M, a.idx_base = n, t, k, self.M, self.idx_base
        a.src, a.lib_bf16, a.rows_f32, a.norms = nat.ptr(source), nat.ptr(self.lib_bf16), nat.ptr(self.rows), nat.ptr(self.norms)
        a.rows_hat = nat.ptr(getattr(self, "rows_hat", None))
        a.out_val, a.out_idx, a.ws = nat.ptr(val), nat.ptr(idx), nat.ptr(ws)
        if events is not None:
            a.ev_start, a.ev_stop = events[0].cuda_event, events[1].cuda_event
        if self.strict:
            a.form, what = nat.KNN_STRICT, "alive_knn_search_strict"
            a.lib_lo, a.bound = nat.ptr(self.lib_lo), nat.ptr(self.bound)
        elif self.rot is not None:
            y = self._rotate_frames(source)
            a.form, what = nat.KNN_FP8_ROT, "alive_knn_search_fp8_rot"
            a.lib_stage, a.y, a.rot_c0 = nat.ptr(self.lib_f8), nat.ptr(y), self.rot["c0"]
        elif sub:
            a.form, what = nat.KNN_FP6_SUB, "alive_knn_search_fp6_sub"
            a.lib_stage, a.lib_sub, a.rho = nat.ptr(self.lib_f8), nat.ptr(self.sub["lib"]), nat.ptr(self.sub["rho"])
            if n * t * self.sub["co"] < 1 << 30:       # the search rotates the frames itself (plane GEMM on the form's two-plane weights)
                a.sub_w = nat.ptr(self.sub["W"])
            else:                                      # beyond the plane GEMM's 32-bit offsets: the conv, as the rotated fp8 stage
                y = self._rotate_frames(source, self.sub)
                a.y = nat.ptr(y)
        elif self.lib_f8 is not None:
            a.form, what = (nat.KNN_FP6 if self.prefilter == "fp6" else nat.KNN_FP8), "alive_knn_search_" + self.prefilter
            a.lib_stage = nat.ptr(self.lib_f8)
        else:
            a.form, what = nat.KNN_BF16, "alive_knn_search"
        nat.check(L.alive_knn_search_unit(ctypes.byref(a), nat.stream()), what)
        self._last = (n, t, k, ws, sub)
        return val, idx


    def with_prefilter(self, prefilter, rotated=False):
        """the same resident library searched through the other candidate stage (shares every tensor); the PLAIN form of that stage
        unless rotated=True and this library has a rotated fp8 image"""
        import copy
        if prefilter not in _STAGES:
            raise ValueError(prefilter)
        other = copy.copy(self)
        other.__dict__.pop("search", None)             # an instrumented search (bench.py) stays with the original
        if rotated and self.rot is not None and prefilter == "fp8":
            other._ws, other._last = nat.Workspace(), None
            other.strict, other.bound, other.lib_lo, other.sub, other.sub_forms = False, None, None, None, []
            return other
        was_rot, other.rot = self.rot is not None, None
        other.sub = self.sub if prefilter == "fp6" else None
        other.sub_forms = self.sub_forms if prefilter == "fp6" else []
        other.fp6_declined = prefilter == "fp6" and self._fp6_would_clip()
        if other.fp6_declined:
            prefilter = "fp8"
        other.prefilter = prefilter
        other.strict, other.bound, other.lib_lo = False, None, None
        other._ws = nat.Workspace()
        other._last = None
        if prefilter == "bf16":
            other.lib_f8 = None
        elif self.lib_f8 is None or self.prefilter != prefilter or was_rot:
            other.lib_f8 = self._pack_stage(prefilter)
        return other

    def with_strict(self):
        """the same resident library searched with the deterministic certificate (shares every tensor)"""
        other = self.with_prefilter("bf16")
        other.strict = True
        other._make_bound()
        return other

    def search_stats(self):
        """what the tiers of the last search on the current stream did (syncs; tests / bench)"""
        last = getattr(self, "_last", None)
        if last is None:
            return None
        n, t, k, ws, sub = last
        torch.cuda.synchronize()
        st = {"prefilter": self.prefilter, "certificate": "deterministic" if self.strict else "statistical"}
        if getattr(self, "rot", None) is not None:
            st["rotated_operands"] = True          # dense bank: the fp8 stage on the bank's own basis (csrc/knn.hip rot_codes_kernel)
        off = nat.lib().alive_knn_search_stats(n, t, self.M, nat.ptr(ws)) - ws.data_ptr()
        c = ws[off:off + 128].view(torch.int32).tolist()      # int[32]: knn.hip ST_*
        tier = c[7]                                     # written by the C side on every path (knn.hip: ST_TIER)
        if sub and tier == 5:                           # subspace form (knn.hip ST_SUB_*): which kernel scored, frames flagged / clipped
            st.update(stage_form={1: "subspace", 2: "plain"}.get(c[21], "none"), frames_left_subspace=c[14] - c[15], frames_clipped=c[15],
                      stage_frames=c[22])         # frames per block of the subspace kernel launched: 384 / 512 (alive_knn_sub_frames)
        if tier == 1:
            return dict(st, tier="exact scan of every row (streaming)")
        if tier == 2:
            return dict(st, tier="exact scan of every row (k > 8)")
        if tier not in (3, 4, 5):
            raise RuntimeError(f"alive_knn_search_stats: no search has run on this workspace (tier word {tier})")
        few = 0
        if tier in (4, 5):              # fp8 / fp6 stage first (the counters keep their fp8 names: "the first, low-precision stage")
            # [0] frames that failed the fp8 certificate: up to [11] of them go straight to the exact scan (knn.hip RESEARCH_MIN)
            few = c[0] if c[0] <= c[11] else 0
            st.update(frames_failed_fp8_certificate=c[0], frames_researched_on_bf16=0 if few else c[0], probe_sample=c[2],
                      probe_failed_fp8_certificate=c[3], probe_chose_bf16_first=bool(c[4]), fp8_blocks_seeded=c[9],
                      probe_skipped_on_history=bool(c[13]))      # knn.hip ST_PROBE_SKIPPED: the workspace's last searches all went one way
        # [1] frames that failed the bf16 certificate: up to [12] of them go straight to the exact scan (knn.hip COLLECT_MIN),
        # more go through the collect tier and only its overflow ([8]) is scanned exactly
        direct = c[1] <= c[12]
        split = self.strict and getattr(self, "lib_lo", None) is not None       # the collect tier is the split-bf16 pass then
        st.update(bf16_blocks_seeded=c[10], frames_failed_bf16_certificate=c[1],
                  frames_collected_on_bf16=0 if direct or split else c[1],
                  frames_searched_exactly=few + (c[1] if direct else c[8]), frames=n * t)
        if split:
            st.update(frames_collected_on_split_bf16=0 if direct else c[1])
        return st

    def fallback_frames(self):
        """frames the last fp8 search had to search again, on bf16 or exactly (syncs; tests / bench)"""
        st = self.search_stats()
        return 0 if st is None else int(st.get("frames_failed_fp8_certificate") or 0)


def merge_gather(cand_val, cand_idx, n_shards, k, alpha, rows_full, source, return_indices=False):
    """merge [S, Tt, k] exact lists, gather rows, mean over k, alpha-blend (common.py:107-109)."""
    n, d, t = source.shape
    out = torch.empty_like(source)
    fin = torch.empty(n * t, k, dtype=torch.int32, device=source.device) if return_indices else None
    nat.check(nat.lib().alive_knn_merge_gather(nat.ptr(cand_val), nat.ptr(cand_idx), n_shards, k, float(alpha),
                                               nat.ptr(rows_full), nat.ptr(source), n, t, nat.ptr(out), nat.ptr(fin),
                                               nat.stream()), "alive_knn_merge_gather")
    return (out, fin) if return_indices else out


_cache = {}          # key -> (PackedLibrary, weakref to the tensor that owns the storage)


def _packed_for(reference_DxM):
    """Packed form of a library tensor, cached per source tensor.  The key alone (address, shape, version) cannot tell
    a library from a later one of the same shape that the caching allocator put at the same address, so an entry also
    holds a weak reference to the tensor that owns the storage: it is valid only while that very tensor is alive and
    is dropped the moment it dies.  (Writes that bypass autograd's version counter -- ctypes kernels, `.data` views --
    are invisible to it: call `forget_packed()` after such a write.)"""
    owner = reference_DxM._base if reference_DxM._base is not None else reference_DxM
    key = (reference_DxM.data_ptr(), tuple(reference_DxM.shape), tuple(reference_DxM.stride()), reference_DxM._version,
           str(reference_DxM.device), _prefilter(), _strict())
    hit = _cache.get(key)
    if hit is not None and hit[1]() is owner:
        return hit[0]
    if len(_cache) >= 4:
        _cache.pop(next(iter(_cache)))
    packed = PackedLibrary(reference_DxM)
    _cache[key] = (packed, weakref.ref(owner, lambda _r, key=key: _cache.pop(key, None)))
    return packed


def forget_packed():
    """drop every cached packed library (after writing into a library tensor behind torch's back)"""
    _cache.clear()


def match_features(source, reference, k=4, alpha=0.0, return_indices=False):
    """source [N,768,T], reference [N or 1,768,M] -> [N,768,T].  Same contract as the reference function;
    shape errors surface as ValueError (the reference raises RuntimeError from torch.bmm / topk)."""
    if source.dim() != 3 or reference.dim() != 3 or source.shape[1] != DIM or reference.shape[1] != DIM:
        raise ValueError("match_features expects source [N,768,T] and reference [N,768,M]")
    if reference.shape[0] not in (1, source.shape[0]):
        raise ValueError("match_features: batch of reference must be 1 or equal to the batch of source")
    if reference.shape[2] < k:
        raise ValueError(f"match_features: library has {reference.shape[2]} vectors, fewer than k={k}")
    source = source.contiguous().float()
    if reference.shape[0] == 1:
        lib = _packed_for(reference[0])
        val, idx = lib.search(source, k)
        return merge_gather(val, idx, 1, k, alpha, lib.rows, source, return_indices)
    outs, idxs = [], []
    for n in range(source.shape[0]):
        lib = _packed_for(reference[n])
        s = source[n:n + 1].contiguous()
        val, idx = lib.search(s, k)
        r = merge_gather(val, idx, 1, k, alpha, lib.rows, s, return_indices)
        outs.append(r[0] if return_indices else r)
        if return_indices:
            idxs.append(r[1])
    out = torch.cat(outs, 0)
    return (out, torch.cat(idxs, 0)) if return_indices else out


# ---- WORLD pitch estimation (`-wpe`): DIO + StoneMask in fp64 on the device (csrc/world_f0.hip, DESIGN.md "WORLD pitch") ----------
_world_taps = {}
_world_ws = nat.Workspace()


def _world_taps_for(fs, f0_min, f0_max, device):
    """DIO's filter taps (built on the host by the library, uploaded once per device and rate)"""
    key = (int(fs), float(f0_min), float(f0_max), str(device))
    taps = _world_taps.get(key)
    if taps is None:
        L = nat.lib()
        n = L.alive_world_f0_taps_count(int(fs), float(f0_min), float(f0_max))
        if n <= 0:
            raise ValueError(f"WORLD f0: unsupported rate {fs} / f0 range [{f0_min}, {f0_max}]")
        host = torch.empty(n, dtype=torch.float64)
        nat.check(L.alive_world_f0_taps(int(fs), float(f0_min), float(f0_max), host.data_ptr()), "alive_world_f0_taps")
        taps = host.to(device)
        torch.cuda.current_stream(device).synchronize()         # once per rate: other streams will read it
        _world_taps[key] = taps
    return taps


def world_f0(x, sample_rate=8000, f0_min=20.0, f0_max=4096.0, frame_period=5.0):
    """pyworld.stonemask(x, *pyworld.dio(x, sample_rate, f0_floor=f0_min, f0_ceil=f0_max, frame_period=frame_period)) of every
    row of x [N, L] (float32 on the device), in float64 -> float32 [N, F], F = int(1000 L / sample_rate / frame_period) + 1"""
    if x.dim() != 2:
        raise ValueError(f"world_f0 expects [N, L] rows, got {tuple(x.shape)}")
    x = x.contiguous().float()
    N, L8 = x.shape
    lib = nat.lib()
    args = (int(sample_rate), float(f0_min), float(f0_max), float(frame_period))
    nbytes = lib.alive_world_f0_workspace_bytes(N, L8, *args)
    if nbytes == 0:
        raise ValueError(f"world_f0: unsupported arguments (rows {N}, length {L8}, rate {sample_rate}, f0 [{f0_min}, {f0_max}])")
    taps = _world_taps_for(sample_rate, f0_min, f0_max, x.device)
    out = torch.empty(N, lib.alive_world_f0_frames(L8, int(sample_rate), float(frame_period)), device=x.device)
    ws = _world_ws.get(nbytes, x.device)
    nat.check(lib.alive_world_f0(nat.ptr(x), N, L8, *args, nat.ptr(taps), nat.ptr(out), nat.ptr(ws), ws.numel(), nat.stream()),
              "alive_world_f0")
    return out


def world_f0_rows(x, row_on, sample_rate=8000, f0_min=20.0, f0_max=4096.0, frame_period=5.0):
    """world_f0 of the rows of x [N, L] whose row_on[r] (device int32 [N]) is nonzero, bitwise; the other rows come back 0
    (unvoiced) and cost a block that returns at once.  The mask is read on the device: a captured call serves any mask"""
    if x.dim() != 2:
        raise ValueError(f"world_f0_rows expects [N, L] rows, got {tuple(x.shape)}")
    if row_on.dtype != torch.int32 or row_on.numel() != x.shape[0] or not row_on.is_contiguous():
        raise ValueError(f"world_f0_rows: row_on must be a contiguous int32 [{x.shape[0]}] mask")
    x = x.contiguous().float()
    N, L8 = x.shape
    lib = nat.lib()
    args = (int(sample_rate), float(f0_min), float(f0_max), float(frame_period))
    nbytes = lib.alive_world_f0_workspace_bytes(N, L8, *args)
    if nbytes == 0:
        raise ValueError(f"world_f0_rows: unsupported arguments (rows {N}, length {L8}, rate {sample_rate}, f0 [{f0_min}, {f0_max}])")
    taps = _world_taps_for(sample_rate, f0_min, f0_max, x.device)
    out = torch.empty(N, lib.alive_world_f0_frames(L8, int(sample_rate), float(frame_period)), device=x.device)
    ws = _world_ws.get(nbytes, x.device)
    nat.check(lib.alive_world_f0_rows(nat.ptr(x), N, L8, *args, nat.ptr(taps), nat.ptr(row_on), nat.ptr(out), nat.ptr(ws),
                                      ws.numel(), nat.stream()), "alive_world_f0_rows")
    return out


# ---- pitch tracking: a Viterbi path over the f0 estimator's class scores (csrc/f0_track.hip, DESIGN.md "Pitch tracking") -----------
TRACK_LO, TRACK_HI, TRACK_BAND, TRACK_WEIGHT, TRACK_JUMP = 50, 1100, 2.0, 1.0, 12.0
TRACK_MAX_STATES = 4000                         # ALIVE_F0_TRACK_MAX_STATES: two fp64 score columns in 64 KB of LDS
_track_ws = nat.Workspace()


def pitch_track_tables(lo=TRACK_LO, hi=TRACK_HI, band=TRACK_BAND):
    """(semis float64 [S], band_lo int32 [S], band_hi int32 [S]) in NumPy: semis[i] = 12 log2(lo + i); band_lo / band_hi the first /
    last state j with |semis[i] - semis[j]| <= band.  The device reads these very bits (no log2 runs there)."""
    import numpy as np
    if isinstance(lo, bool) or isinstance(hi, bool) or int(lo) != lo or int(hi) != hi:
        raise ValueError(f"pitch track: lo and hi must be integers (classes in Hz), got {lo!r}, {hi!r}")
    lo, hi = int(lo), int(hi)
    if not 1 <= lo <= hi <= 4095:
        raise ValueError(f"pitch track: needs 1 <= lo <= hi <= 4095 (class 0 is not a state), got lo {lo}, hi {hi}")
    if hi - lo + 1 > TRACK_MAX_STATES:
        raise ValueError(f"pitch track: {hi - lo + 1} states, at most {TRACK_MAX_STATES} (two fp64 score columns in 64 KB of LDS)")
    if isinstance(band, bool) or not isinstance(band, (int, float)) or not (band >= 0.0 and band < float("inf")):
        raise ValueError(f"pitch track: band must be a finite number of semitones >= 0, got {band!r}")
    s = 12.0 * np.log2(np.arange(lo, hi + 1, dtype=np.float64))
    n = s.size
    blo, bhi = np.empty(n, dtype=np.int32), np.empty(n, dtype=np.int32)
    for i0 in range(0, n, 256):                 # (semis ascends, so a band is one run of states)
        near = np.abs(s[i0:i0 + 256, None] - s[None, :]) <= float(band)
        blo[i0:i0 + 256] = near.argmax(axis=1)
        bhi[i0:i0 + 256] = n - 1 - near[:, ::-1].argmax(axis=1)
    return s, blo, bhi


def track_param(name, v):
    """a tracker weight / jump from the host: a finite float >= 0"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v >= 0.0 and v < float("inf")):
        raise ValueError(f"pitch track: {name} must be a finite number >= 0 (in the units of the class scores), got {v!r}")
    return float(v)


def track_options(value, what="pitch_track"):
    """pitch_track=None | False | True | dict(weight=, jump=, lo=, hi=, band=) -> None, or the dict with every key filled in and checked"""
    if value is None or value is False:
        return None
    if value is True:
        value = {}
    if not isinstance(value, dict):
        raise ValueError(f"{what}: expected None, a bool or a dict of weight / jump / lo / hi / band, got {value!r}")
    unknown = set(value) - {"weight", "jump", "lo", "hi", "band"}
    if unknown:
        raise ValueError(f"{what}: unknown keys {sorted(unknown)} (weight, jump, lo, hi, band)")
    o = dict(weight=TRACK_WEIGHT, jump=TRACK_JUMP, lo=TRACK_LO, hi=TRACK_HI, band=TRACK_BAND)
    o.update(value)
    o["weight"], o["jump"] = track_param("weight", o["weight"]), track_param("jump", o["jump"])
    return o


class PitchTrack:
    """the pitch tracker's converter-wide constants: the state classes lo .. hi, the band in semitones and their tables on `device`"""

    def __init__(self, lo=TRACK_LO, hi=TRACK_HI, band=TRACK_BAND, device="cuda"):
        s, blo, bhi = pitch_track_tables(lo, hi, band)          # (refuses before it touches the device)
        self.lo, self.hi, self.band, self.states = int(lo), int(hi), float(band), int(s.size)
        self.device = torch.device(device)
        self.semis = torch.from_numpy(s).to(self.device)
        self.band_lo, self.band_hi = torch.from_numpy(blo).to(self.device), torch.from_numpy(bhi).to(self.device)
        if self.device.type == "cuda":
            torch.cuda.current_stream(self.device).synchronize()    # once: other streams will read the tables

    def rows(self, logits, f0, on=None, weight=TRACK_WEIGHT, jump=TRACK_JUMP, changed=None):
        """alive_f0_track_rows: logits [N, C, T] fp32 -> the tracked classes over f0 [N, 1, T] (or [N, T]) in place, for the rows whose
        on[r] (device int32 [N]; None: every row) is nonzero.  weight / jump: host scalars, or device float64 [N]; changed: a device
        int32 [N] that receives, per row that is on, the number of frames that differ from what f0 held on entry.  No host
        synchronisation and, with device arrays, no allocation once the stream's workspace exists: capturable"""
        if logits.dim() != 3 or logits.dtype != torch.float32 or not logits.is_contiguous():
            raise ValueError(f"pitch track: logits must be a contiguous fp32 [N, C, T] tensor, got {tuple(logits.shape)}")
        n, c, t = logits.shape
        if f0.dtype != torch.float32 or not f0.is_contiguous() or f0.numel() != n * t or f0.shape[0] != n or f0.shape[-1] != t:
            raise ValueError(f"pitch track: f0 must be a contiguous fp32 [{n}, 1, {t}] tensor, got {tuple(f0.shape)}")
        if self.hi >= c:
            raise ValueError(f"pitch track: classes [{self.lo}, {self.hi}] outside the {c} class scores")
        per_row = []
        for name, v in (("weight", weight), ("jump", jump)):
            if not torch.is_tensor(v):
                v = torch.full((n,), track_param(name, v), dtype=torch.float64, device=logits.device)
            elif v.dtype != torch.float64 or v.numel() != n or not v.is_contiguous():
                raise ValueError(f"pitch track: {name} must be a contiguous float64 [{n}] device array")
            per_row.append(v)
        for name, v in (("on", on), ("changed", changed)):
            if v is not None and (v.dtype != torch.int32 or v.numel() != n or not v.is_contiguous()):
                raise ValueError(f"pitch track: {name} must be a contiguous int32 [{n}] device array")
        L = nat.lib()
        ws = _track_ws.get(L.alive_f0_track_workspace_bytes(n, t, self.states), logits.device)
        nat.check(L.alive_f0_track_rows(nat.ptr(logits), n, c, t, self.lo, self.states, nat.ptr(self.semis), nat.ptr(self.band_lo),
                                        nat.ptr(self.band_hi), nat.ptr(on), nat.ptr(per_row[0]), nat.ptr(per_row[1]), nat.ptr(f0),
                                        nat.ptr(changed), nat.ptr(ws), nat.stream()), "alive_f0_track_rows")
        return f0


def pitch_track(lo=TRACK_LO, hi=TRACK_HI, band=TRACK_BAND, device="cuda"):
    """the tracker object F0Estimator.estimate(track=) takes: state classes lo .. hi (Hz), band in semitones, tables on `device`"""
    return PitchTrack(lo, hi, band, device)


def add_track_arguments(parser):
    """the pitch tracker's flags, the same in every CLI: -pt and --track-weight / --track-jump / --track-lo / --track-hi / --track-band"""
    parser.add_argument('-pt', '--pitch-track', action='store_true',
                        help="pitch tracking: f0 is the Viterbi path over the f0 estimator's class scores instead of their per-frame "
                             "argmax (octave outliers of single frames are smoothed away; default: off; not with -wpe; this build only)")
    parser.add_argument('--track-weight', default=TRACK_WEIGHT, type=float, metavar="W",
                        help="pitch tracking: cost per semitone moved between two frames inside --track-band, in the units of the "
                             f"class scores (default {TRACK_WEIGHT})")
    parser.add_argument('--track-jump', default=TRACK_JUMP, type=float, metavar="J",
                        help=f"pitch tracking: flat cost of any other move (default {TRACK_JUMP})")
    parser.add_argument('--track-lo', default=TRACK_LO, type=int, metavar="HZ", help=f"pitch tracking: the lowest class (default {TRACK_LO})")
    parser.add_argument('--track-hi', default=TRACK_HI, type=int, metavar="HZ",
                        help=f"pitch tracking: the highest class, at most {TRACK_MAX_STATES} classes in all (default {TRACK_HI})")
    parser.add_argument('--track-band', default=TRACK_BAND, type=float, metavar="SEMITONES",
                        help=f"pitch tracking: the moves that cost by the semitone (default {TRACK_BAND})")


def track_arguments(args):
    """the parsed flags -> (weight, jump, lo, hi, band), checked before anything is loaded"""
    pitch_track_tables(args.track_lo, args.track_hi, args.track_band)
    return (track_param("--track-weight", args.track_weight), track_param("--track-jump", args.track_jump), int(args.track_lo),
            int(args.track_hi), float(args.track_band))


# ---- voicing: f0 = 0 on aperiodic frames, by a correlation detector on the 16 kHz source (csrc/voicing.hip, DESIGN.md "Voicing") ----
VOICING_ON, VOICING_OFF, VOICING_FLOOR_DB = 0.6, 0.45, -60.0
VOICING_LO, VOICING_HI, VOICING_WINDOW_MS, VOICING_BRIDGE, VOICING_MIN_RUN = 50, 500, 40, 1, 2
VOICING_MAX_WINDOW, VOICING_MAX_LAG = 4096, 1600      # ALIVE_VOICING_MAX_WINDOW, ALIVE_VOICING_MAX_LAG: a frame's samples fit 64 KB of LDS
VOICING_KEYS = ("on", "off", "floor_db", "lo", "hi", "window_ms", "bridge", "min_run")


def voicing_floor_e(floor_db, hop=320):
    """the silence floor as the energy of one frame of int16-grid samples: 10^(dB / 10) * hop * 2^30 in float64"""
    return 10.0 ** (float(floor_db) / 10.0) * float(hop) * float(2 ** 30)


def voicing_options(v, where=""):
    """voicing=None | False | True | dict(on=, off=, floor_db=, lo=, hi=, window_ms=, bridge=, min_run=) -> None, or the dict with
    every key filled in and checked, plus what the kernel takes: lag_lo = ceil(16000 / hi), lag_hi = floor(16000 / lo),
    W = round(16 window_ms) and floor_e = voicing_floor_e(floor_db)"""
    import math
    what = f"{where}: voicing" if where else "voicing"
    if v is None or v is False:
        return None
    if v is True:
        v = {}
    if not isinstance(v, dict):
        raise ValueError(f"{what}: expected None, a bool or a dict of {' / '.join(VOICING_KEYS)}, got {v!r}")
    unknown = set(v) - set(VOICING_KEYS)
    if unknown:
        raise ValueError(f"{what}: unknown keys {sorted(unknown)} ({', '.join(VOICING_KEYS)})")
    o = dict(on=VOICING_ON, off=VOICING_OFF, floor_db=VOICING_FLOOR_DB, lo=VOICING_LO, hi=VOICING_HI, window_ms=VOICING_WINDOW_MS,
             bridge=VOICING_BRIDGE, min_run=VOICING_MIN_RUN)
    o.update(v)
    for key in ("on", "off", "floor_db", "lo", "hi", "window_ms"):
        x = o[key]
        if isinstance(x, bool) or not isinstance(x, (int, float)) or not math.isfinite(x):
            raise ValueError(f"{what}: {key} must be a finite number, got {x!r}")
    for key in ("bridge", "min_run"):
        x = o[key]
        if isinstance(x, bool) or not isinstance(x, int) or x < 0:
            raise ValueError(f"{what}: {key} must be an integer number of frames >= 0, got {x!r}")
    if not 0.0 < o["off"] <= o["on"] <= 1.0:
        raise ValueError(f"{what}: needs 0 < off <= on <= 1, got off {o['off']!r}, on {o['on']!r}")
    if not 0.0 < o["lo"] < o["hi"] <= 4000.0:
        raise ValueError(f"{what}: needs 0 < lo < hi <= 4000 (Hz), got lo {o['lo']!r}, hi {o['hi']!r}")
    lag_lo, lag_hi = int(math.ceil(16000.0 / o["hi"])), int(math.floor(16000.0 / o["lo"]))
    if lag_lo > lag_hi:
        raise ValueError(f"{what}: no whole lag of the 16 kHz signal lies between lo {o['lo']!r} and hi {o['hi']!r} Hz")
    if lag_hi > VOICING_MAX_LAG:
        raise ValueError(f"{what}: lo {o['lo']!r} Hz is a lag of {lag_hi} samples, at most {VOICING_MAX_LAG} (lo >= 10 Hz)")
    W = int(round(16.0 * o["window_ms"]))
    if not 1 <= W <= VOICING_MAX_WINDOW:
        raise ValueError(f"{what}: window_ms {o['window_ms']!r} is {W} samples, needs 1 <= W <= {VOICING_MAX_WINDOW}")
    o.update(on=float(o["on"]), off=float(o["off"]), floor_db=float(o["floor_db"]), lag_lo=lag_lo, lag_hi=lag_hi, W=W,
             floor_e=voicing_floor_e(o["floor_db"]))
    return o


def add_voicing_arguments(parser):
    """the voicing decision's flags, the same in every CLI that takes them: -vd and --voicing-on / -off / -floor / -lo / -hi"""
    parser.add_argument('-vd', '--voicing', action='store_true',
                        help="voicing decision: f0 = 0 on the frames whose 16 kHz source is not periodic (breath, fricatives, pauses), "
                             "by a correlation detector of its own, after the f0 estimator or -pt and before the pitch transform "
                             "(default: off; not with -wpe, which decides for itself; this build only)")
    parser.add_argument('--voicing-on', default=VOICING_ON, type=float, metavar="R",
                        help=f"voicing decision: a frame whose best normalised correlation reaches this turns voiced (default {VOICING_ON})")
    parser.add_argument('--voicing-off', default=VOICING_OFF, type=float, metavar="R",
                        help=f"voicing decision: a frame under this turns unvoiced; between the two the state stays (default {VOICING_OFF})")
    parser.add_argument('--voicing-floor', default=VOICING_FLOOR_DB, type=float, metavar="DB",
                        help=f"voicing decision: a 20 ms frame whose level is under this is unvoiced (dBFS, default {VOICING_FLOOR_DB})")
    parser.add_argument('--voicing-lo', default=VOICING_LO, type=float, metavar="HZ",
                        help=f"voicing decision: the lowest pitch whose period is tried (default {VOICING_LO})")
    parser.add_argument('--voicing-hi', default=VOICING_HI, type=float, metavar="HZ",
                        help=f"voicing decision: the highest pitch whose period is tried (default {VOICING_HI})")


def voicing_arguments(args):
    """the parsed flags -> the checked options (voicing_options) when -vd is set, else None; refuses before anything is loaded"""
    o = voicing_options(dict(on=args.voicing_on, off=args.voicing_off, floor_db=args.voicing_floor, lo=args.voicing_lo,
                             hi=args.voicing_hi), "-vd")
    return o if args.voicing else None


# ---- match path: one library row per frame by a Viterbi path over the top-k lists (csrc/match_path.hip, DESIGN.md "Match path") -----
PATH_WEIGHT = 1.0                               # in cosine units, like the target cost: a design choice, not tuned
PATH_MAX_K = 8                                  # ALIVE_KNN_PATH_MAX_K
PATH_MAX_FRAMES = 1 << 20                       # ALIVE_KNN_PATH_MAX_FRAMES: list rows x frames of one call
PATH_CHUNK_BYTES = 256 << 20                    # Converter.match: the most workspace one call may take


def path_param(v, name="weight"):
    """the path's join weight from the host: a finite float >= 0"""
    if isinstance(v, bool) or not isinstance(v, (int, float)) or not (v >= 0.0 and v < float("inf")):
        raise ValueError(f"match path: {name} must be a finite number >= 0 (in cosine units), got {v!r}")
    return float(v)


def path_options(v, what="match_path"):
    """match_path=None | False | True | dict(weight=) -> None, or dict(weight=) filled in and checked"""
    if v is None or v is False:
        return None
    if v is True:
        v = {}
    if not isinstance(v, dict):
        raise ValueError(f"{what}: expected None, a bool or a dict of weight, got {v!r}")
    unknown = set(v) - {"weight"}
    if unknown:
        raise ValueError(f"{what}: unknown keys {sorted(unknown)} (weight)")
    return dict(weight=path_param(v.get("weight", PATH_WEIGHT)))


def add_path_arguments(parser):
    """the match path's flags, the same in every CLI that takes them: -mp and --path-weight"""
    parser.add_argument('-mp', '--match-path', action='store_true',
                        help="match path: one library row per frame, chosen out of the frame's k nearest by a Viterbi path that keeps "
                             "consecutive rows close in the library's own feature space, instead of their mean (default: off; this "
                             "build only)")
    parser.add_argument('--path-weight', default=PATH_WEIGHT, type=float, metavar="W",
                        help="match path: weight of the cosine between consecutive chosen rows against a candidate's cosine below the "
                             f"frame's best one; 0 is the k = 1 match (default {PATH_WEIGHT})")


def path_arguments(args):
    """the parsed flags -> the checked options (path_options) when -mp is set, else None; refuses before anything is loaded"""
    o = dict(weight=path_param(args.path_weight, "--path-weight"))
    return o if args.match_path else None


def knn_path_chunks(val, idx, k_row, k_max, on, weight, rows, norms):
    """ops.knn_path_rows over any number of list rows: the call goes in chunks of rows whose workspace stays under PATH_CHUNK_BYTES
    and whose frames stay within the call's limit (rows are independent: the chunking does not show) -> (val, idx, moved)"""
    from . import ops
    r = int(k_row.numel())
    t = val.shape[0] // r
    per = max(1, min(PATH_CHUNK_BYTES // (t * (8 * k_max * k_max + k_max) + 512), PATH_MAX_FRAMES // t))
    if per >= r:
        return ops.knn_path_rows(val, idx, k_row, k_max, on, weight, rows, norms)
    parts = [ops.knn_path_rows(val[a * t:(a + per) * t], idx[a * t:(a + per) * t], k_row[a:a + per], k_max, on[a:a + per],
                               weight[a:a + per], rows, norms) for a in range(0, r, per)]
    return tuple(torch.cat([p[i] for p in parts]) for i in range(3))


def match_path(val, idx, n, k, weight, rows, norms):
    """the path over the lists [n * T, k] of one search, every one of the n rows on at one weight -> (val, idx) [n * T, 1], the lists
    of a k = 1 match, and moved [n]"""
    dev = val.device
    val, idx, moved = knn_path_chunks(val, idx, torch.full((n,), k, dtype=torch.int32, device=dev), k,
                                      torch.ones(n, dtype=torch.int32, device=dev),
                                      torch.full((n,), weight, dtype=torch.float64, device=dev), rows, norms)
    return val[:, :1].contiguous(), idx[:, :1].contiguous(), moved


def linear_resize(x, size):
    """F.interpolate(x, size, mode='linear') (align_corners=False) of x [..., Lin] on the device, rounded as torch's CPU kernel"""
    if size <= 0:
        raise ValueError(f"linear_resize: output size {size} must be positive")
    shape = x.shape
    xr = x.reshape(-1, shape[-1]).contiguous().float()
    y = torch.empty(xr.shape[0], int(size), device=x.device)
    nat.check(nat.lib().alive_linear_resize(nat.ptr(xr), xr.shape[0], xr.shape[1], nat.ptr(y), int(size), nat.stream()),
              "alive_linear_resize")
    return y.reshape(shape[:-1] + (int(size),))


def compute_f0_dio(wf, sample_rate=8000, segment_size=256, f0_min=20, f0_max=4096):
    """reference module/common.py:113-130: wf [L] -> [1, L // segment_size]; wf [N, L] -> [N, 1, L // segment_size]"""
    if wf.dim() not in (1, 2):
        raise ValueError(f"compute_f0_dio expects [L] or [N, L], got {tuple(wf.shape)}")
    rows = wf[None] if wf.dim() == 1 else wf
    f0 = linear_resize(world_f0(rows, sample_rate, f0_min, f0_max), rows.shape[1] // segment_size)
    return f0 if wf.dim() == 1 else f0[:, None]


def compute_f0(wf, sample_rate=16000, segment_size=320):
    """reference module/common.py:133-137: wf [N, L] at sample_rate -> f0 [N, 1, L // segment_size] (8-kHz DIO + StoneMask)"""
    from . import audio_io
    l = wf.shape[1]
    wf8 = audio_io.resample(wf, sample_rate, 8000)
    return linear_resize(compute_f0_dio(wf8, 8000), l // segment_size)


def compute_f0_rows(wf, row_on, sample_rate=16000, segment_size=320):
    """compute_f0 of the rows of wf [N, L] whose row_on[r] (device int32 [N]) is nonzero, bitwise; the other rows are 0.  The
    16 -> 8 kHz resample and the two resizes run over every row (cheap); DIO + StoneMask only over the rows that are on.  No host
    synchronisation: capturable once warm (taps, resampling filter and the stream's workspace exist after the first call)"""
    from . import audio_io
    l = wf.shape[1]
    wf8 = audio_io.resample(wf, sample_rate, 8000).contiguous()
    f0 = linear_resize(world_f0_rows(wf8, row_on, 8000), wf8.shape[1] // 256)
    return linear_resize(f0[:, None], l // segment_size)
