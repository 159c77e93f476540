"""The conversion loop of the reference's inference.py:94-135 as a batched device pipeline.

The reference walks the overlapping windows of one utterance serially (N = 1, two host syncs per
window).  Windows are independent units (each has its own mean pitch, oscillator phase origin
and reflect pads), so here all windows of all utterances go through the networks as one batch
[n_windows, ...]; results are identical to per-window calls.
"""
import os

import numpy as np
import torch
import torch.nn.functional as F

from . import ops
from . import common
from .common import PackedLibrary, compute_f0, merge_gather
from .content_encoder import ContentEncoder
from .decoder import Decoder
from .f0_estimator import F0Estimator
from .spectrogram import spectrogram


def make_windows(wf, chunk=48000):
    """inference.py:94-101: wf [1, L] -> windows [n, 3*chunk] (hop = chunk), total length."""
    total = wf.shape[1]
    wf = torch.cat([wf, torch.zeros(1, chunk * 3, device=wf.device, dtype=wf.dtype)], dim=1)
    wf = F.pad(wf, (chunk, chunk))
    n = (wf.shape[1] - 3 * chunk) // chunk + 1
    return wf.unfold(1, 3 * chunk, chunk)[0, :n].contiguous(), total


def stitch(window_out, total, chunk=48000):
    """inference.py:132-135: keep the centre third of every window, concatenate, trim."""
    return window_out[:, chunk:2 * chunk].reshape(1, -1)[:, :total]


# Frames of the matched features that can reach an output frame t through the decoder (module/decoder.py of the
# reference): the FeatureExtractor is four k7 depthwise convs (+-12 frames); the Filter is causal -- mid conv 4 frames,
# the 256 / 64 / 16 / 8-channel blocks 56 columns each at 32 / 4 / 2 / 1 samples (6.7 frames together) -- and reads FiLM
# / amplitudes interpolated from the neighbouring frames (+-1); source_in / source_out add 3 samples either side.
# => features [t - 24, t + 13].  The margins below leave slack and are checked bitwise by the tests.
TRIM_LEFT, TRIM_RIGHT = 32, 16
CE_MARGIN = 16          # ContentEncoder: four k7 depthwise convs (+-12 frames) between the spectrogram and its output


# Overlap sharing.  Consecutive windows of one utterance overlap by two chunks, and a content / f0 frame at least EDGE frames
# from both edges of its window depends on nothing but the samples around it (spectrogram frame +-640 samples, four k7
# depthwise convs +-12 frames): it has the same value in every window that contains it, and so has its kNN match.  With
# `share_overlap` the front end (spectrogram, f0 estimator, content encoder, match) therefore runs ONCE per utterance on the
# padded signal plus, per window, on its two edge blocks; every window's matched features and raw f0 are then assembled by
# copies.  The pitch transform (per-window mean pitch) and the whole decoder still run per window.  Results are bitwise those
# of the per-window front end (tests/test_gpu_batch.py); at the reference's 3-chunk windows it launches ~51 % of the frames.
EDGE = 14            # 12 frames of ConvNeXt context + 2 of STFT reflect padding (module/realtime.py uses the same numbers)
NET_MARGIN = 16
SPEC_MARGIN = 2


def _edge_chunks(n, size):
    """[i0, i1) bounds of the edge-block launches over n windows, `size` windows at a time.  An edge block is EDGE + NET_MARGIN = 30
    frame columns per window, and below 96 columns the library switches to its fp32 streaming kernels, which round differently from
    the plane GEMMs every other window's edge blocks run on: a tail of fewer than 4 windows is folded into the chunk before it, so
    that the stitched output stays bitwise that of the per-window path for every window count."""
    need = -(-96 // (EDGE + NET_MARGIN))
    bounds = [(i, min(n, i + size)) for i in range(0, n, size)]
    if len(bounds) > 1 and bounds[-1][1] - bounds[-1][0] < need:
        last = bounds.pop()
        bounds[-1] = (bounds[-1][0], last[1])
    return bounds


def _signals(windows, group):
    """the padded signal [m, (group + 2) c] of every `group` consecutive windows (make_windows order, chunk c = a third of the
    window): the first chunk of each window, then the last two chunks of the last one"""
    n, L = windows.shape
    m, c = n // group, L // 3
    w3 = windows.view(m, group, L)
    return torch.cat([w3[:, :, :c].reshape(m, group * c), w3[:, -1, c:]], dim=1).contiguous()


def _edge_specs(windows):
    """spectrograms of the two edge blocks of every window, EDGE + NET_MARGIN frames each: frames [0, nl) and [lf - nl, lf),
    each from a slice of the window with SPEC_MARGIN frames more (those are spoiled by the slice's own reflect padding)"""
    L = windows.shape[1]
    nl = EDGE + NET_MARGIN
    sl = spectrogram(windows[:, :(nl + SPEC_MARGIN) * 320].contiguous())[:, :, :nl].contiguous()
    sr = spectrogram(windows[:, L - (nl + SPEC_MARGIN) * 320:].contiguous())[:, :, SPEC_MARGIN:].contiguous()
    return sl, sr


def _decoded_range(keep_frames, lf):
    """the frames [lo, hi) that can reach the kept frames keep_frames of a window of lf frames through the decoder (None: all)"""
    return None if keep_frames is None else (max(0, keep_frames[0] - TRIM_LEFT), min(lf, keep_frames[1] + TRIM_RIGHT))


def prepare_networks(content_encoder, f0_estimator, decoder, device):
    """the three networks on `device` with their weight tables packed and the decoder's precision mode calibrated for this
    checkpoint (module/decoder.py) -- now, on the caller's stream: never lazily inside a window batch on a side stream or
    inside a hipGraph capture"""
    nets = content_encoder.to(device), f0_estimator.to(device), decoder.to(device)
    for net in nets:
        net.table()
    if torch.device(device).type == "cuda":
        nets[2]._split_for_this_checkpoint()
    return nets


class Converter:
    def __init__(self, content_encoder: ContentEncoder, f0_estimator: F0Estimator, decoder: Decoder, device="cuda"):
        self.device = torch.device(device)
        self.ce, self.pe, self.dec = prepare_networks(content_encoder, f0_estimator, decoder, device)
        self.library = None

    def set_library(self, tokens):
        """tokens [1, 768, M] (voice_library.pt layout) or an already packed PackedLibrary.  A plain fp6 library gets the subspace form
        of its candidate stage from the content encoder's output layer (PackedLibrary.set_subspace)."""
        self.library = tokens if isinstance(tokens, PackedLibrary) else PackedLibrary(tokens[0].to(self.device))
        self._subspace()
        return self

    def _subspace(self):
        """(re)build the library's subspace basis when the encoder's output layer is not the one it was built from (load_state_dict
        replaces the tensors)"""
        lib = self.library
        if not isinstance(lib, PackedLibrary) or getattr(self.ce, "generic", False):
            return
        sd = self.ce._sd
        w, b = sd.get("output_layer.weight"), sd.get("output_layer.bias")
        if w is None or b is None or w.shape[0] != 768 or w.shape[1] != 512:
            return
        lib.use_subspace(w, b)

    def _pitch_track(self, lo, hi, band):
        """the tracker tables of (lo, hi, band) on this converter's device, built once"""
        cache = self.__dict__.setdefault("_pitch_tracks", {})
        key = (int(lo), int(hi), float(band))
        if key not in cache:
            cache[key] = common.pitch_track(lo, hi, band, self.device)
        return cache[key]

    def features(self, windows, pitch_shift=0.0, intonation=1.0, f0_rate=1.0, frames=None, out=None, world_pitch=False,
                 pitch_track=None, voicing=None):
        """spectrogram -> f0 (+ per-window pitch transform) and content features   (inference.py:112-128).
        frames = (lo, hi): content features are only needed on [lo, hi) (context trimming): the encoder runs on that range
        plus its own receptive field; the other frames come back as zeros.  f0 always covers the whole window (the pitch
        transform uses the window's mean pitch, the oscillator accumulates phase from the first frame).
        world_pitch: f0 is WORLD's DIO + StoneMask of each whole window (common.compute_f0, reference inference.py:113-114) and the
        f0 estimator does not run.
        pitch_track (common.track_options): the f0 of each whole window is the Viterbi path over the estimator's class scores
        (F0Estimator.estimate(track=), csrc/f0_track.hip) instead of their per-frame argmax, before the pitch transform.
        voicing (common.voicing_options): the f0 of the frames of each whole window that the correlation detector finds unvoiced
        becomes 0 (ops.voicing_rows_, csrc/voicing.hip), after the estimator or the tracker and before the pitch transform, whose
        window mean is then taken over the voiced frames alone."""
        if voicing is not None and world_pitch:
            raise ValueError("voicing cannot be combined with world_pitch: WORLD makes its own voicing decision")
        voice = (lambda f0: f0) if voicing is None else (lambda f0: ops.voicing_rows_(f0, windows, voicing))
        if pitch_track is not None:
            if world_pitch:
                raise ValueError("pitch_track cannot be combined with world_pitch: the tracker decodes the estimator's class scores")
            o = pitch_track
            spec = spectrogram(windows)
            f0 = self.pe.estimate(spec, out=None if out is None else out[1], track=self._pitch_track(o["lo"], o["hi"], o["band"]),
                                  track_weight=o["weight"], track_jump=o["jump"])
            f0 = ops.pitch_transform_(voice(f0), 0, f0_rate=f0_rate, pitch_shift=pitch_shift, intonation=intonation)
            feat = self._encode(spec, frames)
            if out is not None:
                out[0].copy_(feat)
            return feat, f0
        if world_pitch:
            f0 = ops.pitch_transform_(compute_f0(windows), 0, f0_rate=f0_rate, pitch_shift=pitch_shift, intonation=intonation)
            feat = self._encode(spectrogram(windows), frames)
            if out is not None:
                out[0].copy_(feat)
                out[1].copy_(f0)
            return feat, f0
        if frames is None:                 # the whole window: one fused call, no fp32 spectrogram (ops.front_end)
            feat, f0 = ops.front_end(windows, self.ce, self.pe, out=out)     # out = (feat, f0) batch slices to write into
            return feat, ops.pitch_transform_(voice(f0), 0, f0_rate=f0_rate, pitch_shift=pitch_shift, intonation=intonation)
        spec = spectrogram(windows)
        f0 = self.pe.estimate(spec, out=None if out is None else out[1])
        f0 = ops.pitch_transform_(voice(f0), 0, f0_rate=f0_rate, pitch_shift=pitch_shift, intonation=intonation)
        return self._encode(spec, frames), f0

    def _encode(self, spec, frames=None):
        """content features of spectrograms [n, 513, lf].  frames = (lo, hi): the encoder runs on [lo - CE_MARGIN, hi + CE_MARGIN)
        only (its receptive field around the frames that are needed); the frames outside come back as zeros"""
        if frames is None:
            return self.ce(spec)
        lf = spec.shape[2]
        a, b = max(0, frames[0] - CE_MARGIN), min(lf, frames[1] + CE_MARGIN)
        feat = torch.zeros(spec.shape[0], 768, lf, device=spec.device)
        feat[:, :, a:b] = self.ce(spec[:, :, a:b].contiguous())
        return feat

    def features_shared(self, windows, group, k=4, alpha=0.0, utt_batch=32, frames=None):
        """(matched content features [n, 768, lf], raw f0 [n, 1, lf]) of n = m * group windows, every `group` consecutive ones
        being the windows of one signal at hop = a third of the window (make_windows): the front end runs once per signal.
        frames = (r0, r1) with EDGE <= r0 < r1 <= lf - EDGE (context trimming on top of sharing): only the matched features of
        frames [r0, r1) of every window are needed -> [n, 768, r1 - r0].  They are all interior frames of the signal, so the
        edge blocks carry the f0 estimator alone (f0 still covers the whole window) and the match runs on the union of the
        windows' ranges, frames [r0, (group - 1) cf + r1) of each signal."""
        n, L = windows.shape
        c = L // 3
        lf, cf = L // 320, c // 320
        if n % group or c % 320 or lf < 2 * (EDGE + NET_MARGIN + SPEC_MARGIN):
            raise ValueError(f"share_overlap needs groups of {group} windows of 3 chunks, chunk a multiple of 320 and >= "
                             f"{2 * (EDGE + NET_MARGIN + SPEC_MARGIN)} frames per window")
        if frames is not None:
            return self._features_shared_range(windows, group, k, alpha, utt_batch, frames)
        m = n // group
        sig = _signals(windows, group)                         # [m, (group + 2) c]
        dev = windows.device
        feat = torch.empty(n, 768, lf, device=dev)
        f0 = torch.empty(n, 1, lf, device=dev)
        fu = torch.empty(m, 768, (group + 2) * cf, device=dev)
        pu = torch.empty(m, 1, (group + 2) * cf, device=dev)
        for i in range(0, m, utt_batch):                       # interior frames: one pass over each signal
            ops.front_end(sig[i:i + utt_batch], self.ce, self.pe, out=(fu[i:i + utt_batch], pu[i:i + utt_batch]))
        fe = torch.empty(n, 768, 2 * EDGE, device=dev)         # edge frames of every window: [0, EDGE) and [lf - EDGE, lf)
        pe_ = torch.empty(n, 1, 2 * EDGE, device=dev)
        for i, j in _edge_chunks(n, 8 * utt_batch):
            sl, sr = _edge_specs(windows[i:j])
            fe[i:j, :, :EDGE] = self.ce(sl)[:, :, :EDGE]
            fe[i:j, :, EDGE:] = self.ce(sr)[:, :, NET_MARGIN:]
            pe_[i:j, :, :EDGE] = self.pe.estimate(sl)[:, :, :EDGE]
            pe_[i:j, :, EDGE:] = self.pe.estimate(sr)[:, :, NET_MARGIN:]
        # the match: once per distinct frame, and ONE search for the signals' frames and the windows' edge frames together
        # (a search of its own for the 28 edge frames per window would run the scoring kernel at a fraction of its rate)
        tu = fu.shape[2]
        src = torch.cat([fu.permute(1, 0, 2).reshape(768, m * tu), fe.permute(1, 0, 2).reshape(768, n * 2 * EDGE)], dim=1)
        matched = self.match(src.unsqueeze(0).contiguous(), k, alpha)[0]
        fu = matched[:, :m * tu].view(768, m, tu).permute(1, 0, 2)
        fe = matched[:, m * tu:].view(768, n, 2 * EDGE).permute(1, 0, 2)
        f4, p4 = feat.view(m, group, 768, lf), f0.view(m, group, 1, lf)
        for g in range(group):                                 # window g of a signal = frames [g cf, g cf + lf) of it
            f4[:, g, :, EDGE:lf - EDGE] = fu[:, :, g * cf + EDGE:g * cf + lf - EDGE]
            p4[:, g, :, EDGE:lf - EDGE] = pu[:, :, g * cf + EDGE:g * cf + lf - EDGE]
        feat[:, :, :EDGE], feat[:, :, lf - EDGE:] = fe[:, :, :EDGE], fe[:, :, EDGE:]
        f0[:, :, :EDGE], f0[:, :, lf - EDGE:] = pe_[:, :, :EDGE], pe_[:, :, EDGE:]
        self.last_front_end_frames = m * (group + 2) * cf + n * 2 * EDGE           # frames that went through the match
        return feat, f0

    def _features_shared_range(self, windows, group, k, alpha, utt_batch, frames):
        n, L = windows.shape
        c = L // 3
        lf, cf = L // 320, c // 320
        r0, r1 = frames
        if not (EDGE <= r0 < r1 <= lf - EDGE):
            raise ValueError(f"shared front end with a frame range needs {EDGE} <= r0 < r1 <= {lf - EDGE}, got {frames}")
        m = n // group
        nr = r1 - r0
        sig = _signals(windows, group)                         # [m, (group + 2) c]
        dev = windows.device
        tu = (group + 2) * cf
        u0, u1 = r0, (group - 1) * cf + r1                      # frames of a signal that some window's range holds
        a, b = max(0, u0 - CE_MARGIN), min(tu, u1 + CE_MARGIN)  # ... plus the content encoder's own receptive field
        pu = torch.empty(m, 1, tu, device=dev)
        fu = torch.empty(m, 768, u1 - u0, device=dev)
        for i in range(0, m, utt_batch):
            spec = spectrogram(sig[i:i + utt_batch])
            pu[i:i + utt_batch] = self.pe.estimate(spec)
            fu[i:i + utt_batch] = self.ce(spec[:, :, a:b].contiguous())[:, :, u0 - a:u1 - a]
        f0 = torch.empty(n, 1, lf, device=dev)
        for i, j in _edge_chunks(n, 8 * utt_batch):            # f0 of the edge frames of every window
            sl, sr = _edge_specs(windows[i:j])
            f0[i:j, :, :EDGE] = self.pe.estimate(sl)[:, :, :EDGE]
            f0[i:j, :, lf - EDGE:] = self.pe.estimate(sr)[:, :, NET_MARGIN:]
        nu = u1 - u0
        matched = self.match(fu.permute(1, 0, 2).reshape(1, 768, m * nu).contiguous(), k, alpha)[0].view(768, m, nu).permute(1, 0, 2)
        feat = torch.empty(n, 768, nr, device=dev)
        f4, p4 = feat.view(m, group, 768, nr), f0.view(m, group, 1, lf)
        for g in range(group):                                 # window g of a signal = frames [g cf, g cf + lf) of it
            f4[:, g] = matched[:, :, g * cf:g * cf + nr]
            p4[:, g, :, EDGE:lf - EDGE] = pu[:, :, g * cf + EDGE:g * cf + lf - EDGE]
        self.last_front_end_frames = m * nu                     # frames that went through the match
        return feat, f0

    def match(self, feat, k=4, alpha=0.0, path=None):
        """path (common.path_options): instead of the mean of each frame's k nearest rows, ONE of them per frame, chosen by a Viterbi
        path over every window's lists (common.match_path, csrc/match_path.hip), gathered as a k = 1 match"""
        self._subspace()
        val, idx = self.library.search(feat, k)
        if path is None:
            return merge_gather(val, idx, 1, k, alpha, self.library.rows, feat)
        val, idx, self.last_path_moved = common.match_path(val, idx, feat.shape[0], k, path["weight"], self.library.rows, self.library.norms)
        return merge_gather(val, idx, 1, 1, alpha, self.library.rows, feat)

    def convert_windows(self, windows, *a, **kw):
        """`_convert_windows` (below: same arguments) under the fp16 range guard (ops.Fp16Guard): the saturation counters of the fp16
        forms are cleared in stream order when the batch starts and read when it ends (one device synchronisation per call); a batch
        that drove an activation out of fp16's range is REPEATED on bf16 planes instead of being returned saturated -- every public
        batch entry point (this one, `convert`, `generate_voice_library.py`, `RealtimeConverter` above 96 columns) is covered."""
        return ops.Fp16Guard(self._agree_on_saturations()).run(lambda: self._convert_windows(windows, *a, **kw))

    def _agree_on_saturations(self):
        return None                       # one process, one decision (ShardedConverter: max over the ranks)

    def _path_options(self, match_path):
        """the checked match_path option of a call (ShardedConverter refuses it)"""
        return common.path_options(match_path)

    def _convert_windows(self, windows, k=4, alpha=0.0, pitch_shift=0.0, intonation=1.0, f0_rate=1.0, window_batch=64,
                         keep_frames=None, share_overlap=None, world_pitch=False, pitch_track=None, voicing=None, match_path=None):
        """windows [n, L] on the device -> waveforms [n, L]; L a multiple of 320.
        Networks run in batches of `window_batch` windows (bounded scratch); the kNN match runs ONCE over the frames
        of all windows, so every library tile streamed from L2 is used by as many frames as possible.
        keep_frames = (a, b): the caller keeps only the output of frames [a, b) of every window (inference.py keeps the
        centre third).  The match is then restricted to the frames that can reach them through the decoder; the kept
        samples are bitwise the same as without it (the other frames of the window decode from unmatched features).
        world_pitch=True: f0 is WORLD's (DIO + StoneMask) of every whole window instead of the f0 estimator's, as `-wpe` does
        (reference inference.py:113-114); WORLD is not local (mean removal and contour fixing span the window), so overlap
        sharing is not used with it (the per-window path gives the same samples) and trimming applies to the content only.
        pitch_track=True | dict(weight=, jump=, lo=, hi=, band=): the f0 of every whole window is the Viterbi path over the
        estimator's class scores (features); it rides where world_pitch does -- per-window front end, no overlap sharing, f0
        over the whole window also with keep_frames -- and cannot be combined with it.
        voicing=True | dict(on=, off=, floor_db=, lo=, hi=, window_ms=, bridge=, min_run=): the f0 of the frames of every whole window
        that are not periodic becomes 0 (features); it rides where pitch_track does and cannot be combined with world_pitch.
        match_path=True | dict(weight=): the matched feature of a frame is ONE of its k nearest library rows, chosen by a Viterbi path
        over the window (match(path=)) -- per-window front end, no overlap sharing.  The path depends on every frame of its window, so
        with keep_frames the match still covers the whole window and trimming applies to the decoder alone: the kept samples are
        bitwise the same with and without it."""
        match_path = self._path_options(match_path)
        voicing = common.voicing_options(voicing)
        if voicing is not None and world_pitch:
            raise ValueError("voicing cannot be combined with world_pitch: WORLD makes its own voicing decision")
        pitch_track = common.track_options(pitch_track)
        if pitch_track is not None and world_pitch:
            raise ValueError("pitch_track cannot be combined with world_pitch: the tracker decodes the estimator's class scores")
        if pitch_track is not None:
            self._pitch_track(pitch_track["lo"], pitch_track["hi"], pitch_track["band"])        # (refuses a bad range before any launch)
        n, L = windows.shape
        lf = L // 320
        # (the edge blocks of all windows form one launch of n x 30 frame columns: below 96 columns the library would switch
        # to its streaming kernels, which round differently from the plane GEMMs the windows themselves run on -- then the
        # per-window front end is used, so that the result never depends on the flag)
        rng = _decoded_range(keep_frames, lf)
        # sharing and trimming together need the trimmed range to consist of interior frames of the signal (it does for the
        # centre third of a 3-chunk window from 46 frames per chunk on); otherwise trimming alone is used -- same samples
        share_ok = (bool(share_overlap) and n * (EDGE + NET_MARGIN) >= 96 and not world_pitch and pitch_track is None and voicing is None
                    and match_path is None)
        if share_ok and (rng is None or (EDGE <= rng[0] and rng[1] <= lf - EDGE and rng[1] - rng[0] >= 5)):
            # share_overlap = windows per signal (make_windows order): front end once per signal, decoder per window
            feat, f0 = self.features_shared(windows, int(share_overlap), k, alpha, frames=rng)
            f0 = ops.pitch_transform_(f0, 0, f0_rate=f0_rate, pitch_shift=pitch_shift, intonation=intonation)
            return self._decode(windows, feat, f0, rng, window_batch)

        def encode(i, feat, f0):                            # the pitch transform included (features)
            b = slice(i, i + window_batch)
            if rng is None or match_path is not None:       # the networks write straight into the batch's slices
                self.features(windows[b], pitch_shift, intonation, f0_rate, out=(feat[b], f0[b]), world_pitch=world_pitch,
                              pitch_track=pitch_track, voicing=voicing)
            else:
                feat[b], f0[b] = self.features(windows[b], pitch_shift, intonation, f0_rate, frames=rng, world_pitch=world_pitch,
                                               pitch_track=pitch_track, voicing=voicing)

        def match(feat):                                    # (ShardedConverter overrides self.match)
            if match_path is not None:                      # the path runs over the whole window; the decoder takes its range of it
                out = self.match(feat, k, alpha, path=match_path)
                return out if rng is None else out[:, :, rng[0]:rng[1]]
            if rng is None:
                return self.match(feat, k, alpha)
            feat[:, :, rng[0]:rng[1]] = self.match(feat[:, :, rng[0]:rng[1]].contiguous(), k, alpha)
            return feat[:, :, rng[0]:rng[1]]
        return self._convert_per_window(windows, rng, window_batch, encode, match)

    def _convert_per_window(self, windows, rng, window_batch, encode, match, transform=None):
        """The per-window front end of `convert_windows` and `convert_many`: encode(i, feat, f0) writes the content features and
        the f0 of the window batch that starts at i into feat [n, 768, lf] / f0 [n, 1, lf]; transform(f0) then applies the
        pitch transform to every window at once (None: encode did); match(feat) returns the matched features of the frames
        rng = [lo, hi) of every window (of all frames: rng None), ONE match over all windows; the decoder runs per batch."""
        n, L = windows.shape
        feat = torch.empty(n, 768, L // 320, device=windows.device)
        f0 = torch.empty(n, 1, L // 320, device=windows.device)
        self._window_batches(n, window_batch, windows.device, lambda i: encode(i, feat, f0))
        if transform is not None:
            transform(f0)
        return self._decode(windows, match(feat), f0, rng, window_batch)

    def _decode(self, windows, feat, f0, rng, window_batch):
        """matched features and transformed f0 of the windows -> output windows [n, L], decoded per window batch.  With a range
        rng = (lo, hi) feat holds frames [lo, hi) only and only they are decoded (the oscillator still accumulates phase over
        the whole window); samples outside them are not kept by the caller and stay zero."""
        out = torch.empty_like(windows) if rng is None else torch.zeros_like(windows)

        def dec(i):
            b = slice(i, i + window_batch)
            if rng is None:
                self.dec(feat[b], f0[b], out=out[b])
            else:
                out[b, rng[0] * 320:rng[1] * 320] = self.dec.forward_range(feat[b].contiguous(), f0[b], rng[0])
        self._window_batches(windows.shape[0], window_batch, windows.device, dec)
        return out

    def _window_batches(self, n, window_batch, device, fn):
        """fn(i) for the window batches [i, i + window_batch) of n windows.  Window batches are independent before and after the
        match: they go round-robin onto side streams (scratch is per stream, module/_native.py::Workspace), so that the tail of
        one batch's kernels overlaps the next batch's -- the kernels of a batch differ widely in what bounds them.  Same kernels
        on the same data: results are unchanged.  The caller's stream then waits for all of them."""
        cur = torch.cuda.current_stream()
        side = self._side_streams(device)
        for j, i in enumerate(range(0, n, window_batch)):
            if not side:
                fn(i)
                continue
            st = side[j % len(side)]
            st.wait_stream(cur)
            with torch.cuda.stream(st):
                fn(i)
        for st in side:
            cur.wait_stream(st)

    def _side_streams(self, device):
        """side streams of the window batches (ALIVE_STREAMS, default 3; 1 = everything on the caller's stream)"""
        want = int(os.environ.get("ALIVE_STREAMS", "3"))
        if want <= 1:
            return []
        pool = getattr(self, "_streams", None)
        if pool is None or len(pool) != want:
            pool = self._streams = [torch.cuda.Stream(device=device) for _ in range(want)]
        return pool

    def convert(self, wf, chunk=48000, trim_context=False, **kw):
        """one utterance: wf [1, L] at 16 kHz (already normalised / mono) -> [1, L].
        trim_context: match and decode only the frames that can reach the kept centre third (same samples, ~44 % of the kNN
        and decoder work); share_overlap=True / "auto": the front end once per utterance.  The two combine (the CLI's default):
        the stitched output is bitwise that of the plain per-window path."""
        windows, total = make_windows(wf.to(self.device), chunk)
        keep = (chunk // 320, 2 * chunk // 320) if trim_context else None
        share = kw.get("share_overlap")
        if share is True or share == "auto":                      # one utterance: all of its windows form one group
            n = windows.shape[0]
            ok = chunk % 320 == 0 and 3 * chunk // 320 >= 2 * (EDGE + NET_MARGIN + SPEC_MARGIN)
            # "auto": sharing adds ~2.5 ms of small launches (one more encoder pass, edge blocks, copies) and saves about half
            # of the front end, most of it in the kNN match -- measured break-even: 43 windows at a 50 k-vector library, 18 at 1 M
            if share == "auto" and self.library is not None:
                ok = ok and n * (1.0 + self.library.M / 5e5) >= 45.0
            kw["share_overlap"] = n if ok else None
        return stitch(self.convert_windows(windows, keep_frames=keep, **kw), total, chunk)       # (the guard sits in convert_windows)

    def convert_many(self, utterances, pool, voices, pitch_shift=0.0, intonation=1.0, f0_rate=1.0, alpha=0.0, chunk=48000, k=4,
                     window_batch=64, trim_context=False, world_pitch=False, auto_pitch=False, auto_range=False,
                     pitch_range_max=2.0, pitch_track=None, voicing=None, match_path=None):
        """Many-to-many batch conversion: utterance i (16 kHz, [L] or [1, L], any length) to voice voices[i] of `pool`
        (module/multistream.py: VoicePool), with per-utterance pitch_shift / intonation / f0_rate / alpha / world_pitch (a scalar
        applies to every utterance; world_pitch: WORLD's f0 of each whole window, as convert(world_pitch=True)).  Returns one [1, L_i] waveform per utterance.  The windows of ALL utterances form one batch (a network
        batch may span utterances), and the match is ONE pool search over every window's frames, each window against its own
        voice (csrc/knn.hip: alive_knn_search_pool).  Utterance i comes out bitwise as `convert` with
        PackedLibrary(voice, strict=True) makes it alone -- unless the fp16 range guard repeats the batch on bf16 planes: that
        repeat covers the whole batch, so its composition then matters (ops.Fp16Guard).
        voices[i] may also be a blend ({name: weight} or (name, weight) pairs, multistream.blend_spec): then every window of the
        corpus gets one list row per voice of its utterance's blend, the pool search runs over those rows (in pieces within its
        limits, bitwise one call) and the blend gather mixes each window's lists (alive_knn_blend_gather_rows).  A corpus without a
        blend of two or more voices launches the plain path.
        k may be a list with one value per utterance (1 <= k_i <= 8; every voice of utterance i needs at least k_i vectors): the
        match then runs the per-row-k entry points at k_max = max(k) (alive_knn_search_pool_k, alive_knn_merge_gather_rows_k /
        alive_knn_blend_gather_rows_k; the pool search groups its rows by voice and k), and utterance i is bitwise `convert` alone
        at k_i.  A scalar k launches the uniform path.
        auto_pitch (a bool, or one per utterance): utterance i's shift follows its target voice's register (VoicePool.register; a
        blend: the weighted mean of its voices'; ValueError for a voice without one): its source register is the mean voiced pitch
        of the raw f0 (the estimator's or WORLD's, before intonation and rate) over the centre third of each of its windows --
        frames [chunk // 320, 2 * chunk // 320), every original frame once -- from ONE alive_pitch_stats_groups call with a group
        per utterance, and its shift is pitch_shift[i] + (target - that mean) (alive_pitch_shift_groups), pitch_shift[i] alone if
        nothing is voiced.  A group's sums depend on its own rows only and are added in a fixed order, so an utterance converts
        bitwise the same alone and inside any corpus.  A corpus without an auto utterance launches the present path.
        auto_range (a bool, or one per utterance): utterance i's pitch excursions are scaled so that its own standard deviation meets
        its target voice's (VoicePool.pitch_range; a blend: the weighted mean; ValueError for a voice without one).  ONE
        alive_pitch_stats2_groups call over the same centre thirds gives each utterance's mean m and variance v; its intonation
        becomes intonation[i] * clamp(target sd / sqrt(v), 1 / pitch_range_max, pitch_range_max) (alive_pitch_range_groups) and its
        frames are scaled around m -- its OWN mean over all its windows, not each window's -- by
        alive_pitch_transform_rows_centred; the shift stays what it is.  Utterances with the flag off keep the per-window
        arithmetic in the same launch, bitwise; a corpus without an auto-range utterance launches the present path.
        pitch_track (None / a bool / dict(weight=, jump=), or one per utterance): utterance i's f0 is the Viterbi path over the
        estimator's class scores of each of its whole windows, as convert(pitch_track=...) of it alone (lo, hi and band are call-wide:
        the tracked utterances must agree on them; not together with world_pitch).  Per window batch, the class scores of the tracked
        windows are stored (F0Estimator.logits) and alive_f0_track_rows overwrites their f0 rows, each with its utterance's weight
        and jump, before the transform -- auto pitch and auto range measure the tracked contour.  A row's path depends on its own
        scores only; a corpus without a tracked utterance launches the present path.
        voicing (None / a bool / dict(on=, off=, floor_db=), or one per utterance): the f0 of utterance i's frames that are not
        periodic becomes 0, as convert(voicing=...) of it alone (lo, hi, window_ms, bridge and min_run are call-wide: the deciding
        utterances must agree on them; not together with world_pitch).  One alive_voicing_rows call per window batch over the rows
        that are on, each with its utterance's thresholds, after the tracker and before the transform -- auto pitch and auto range
        measure the voiced contour.  A row's decision depends on its own window only; a corpus without a deciding utterance launches
        the present path.
        match_path (None / a bool / dict(weight=), or one per utterance): the matched feature of utterance i's frames is ONE of their
        k_i nearest rows, chosen by a Viterbi path over each of its whole windows, as convert(match_path=...) of it alone.  The pool
        search runs as it does; ONE path call (alive_knn_path_rows) then takes every list row with its utterance's switch and weight
        (a blend: every list of a window its own path), and the per-row-k gathers run at a gather-k of 1 on the path's rows.  With
        trim_context the match covers the whole windows and trimming applies to the decoder alone.  A row's path depends on its own
        lists only; a corpus without such an utterance launches the present path."""
        from . import multistream as MS
        if getattr(pool, "dtype", torch.float32) != torch.float32:         # (a half pool: the pool search rescans fp32 rows)
            pool._need_f32(f"{type(self).__name__}.convert_many")
        m = len(utterances)
        voices = list(voices)
        if len(voices) != m:
            raise ValueError(f"{m} utterances but {len(voices)} voices")
        ks = None                           # per-utterance k: a list; a scalar takes the uniform entry points
        if isinstance(k, (list, tuple)):
            if len(k) != m:
                raise ValueError(f"k: {len(k)} values for {m} utterances")
            ks = [MS.check_k(v, f"convert_many: k[{i}]") for i, v in enumerate(k)]
            k = max(ks)                     # k_max: the stride of the lists
        elif not 1 <= k <= MS.MAX_K:
            raise ValueError(f"convert_many: k={k} outside [1, {MS.MAX_K}]")

        def per(x, what):
            xs = list(x) if isinstance(x, (list, tuple)) else [x] * m
            if len(xs) != m:
                raise ValueError(f"{what}: {len(xs)} values for {m} utterances")
            return [float(v) for v in xs]
        shifts, inton, rates, alphas = (per(pitch_shift, "pitch_shift"), per(intonation, "intonation"), per(f0_rate, "f0_rate"),
                                        per(alpha, "alpha"))
        worlds = list(world_pitch) if isinstance(world_pitch, (list, tuple)) else [world_pitch] * m
        if len(worlds) != m:
            raise ValueError(f"world_pitch: {len(worlds)} values for {m} utterances")
        if not all(isinstance(w, (bool, np.bool_)) for w in worlds):
            raise ValueError(f"world_pitch: expected bools, got {worlds}")
        tracks = list(pitch_track) if isinstance(pitch_track, (list, tuple)) else [pitch_track] * m
        if len(tracks) != m:
            raise ValueError(f"pitch_track: {len(tracks)} values for {m} utterances")
        tracks = [common.track_options(t, f"convert_many: pitch_track[{i}]") for i, t in enumerate(tracks)]
        if any(t is not None and w for t, w in zip(tracks, worlds)):
            raise ValueError("pitch_track cannot be combined with world_pitch on the same utterance")
        tracker = None
        if any(t is not None for t in tracks):
            wide = {(t["lo"], t["hi"], t["band"]) for t in tracks if t is not None}
            if len(wide) != 1:
                raise ValueError(f"pitch_track: lo, hi and band are call-wide, the tracked utterances ask for {sorted(wide)}")
            tracker = self._pitch_track(*wide.pop())
        voicings = list(voicing) if isinstance(voicing, (list, tuple)) else [voicing] * m
        if len(voicings) != m:
            raise ValueError(f"voicing: {len(voicings)} values for {m} utterances")
        voicings = [common.voicing_options(v, f"convert_many: utterance {i}") for i, v in enumerate(voicings)]
        if any(v is not None and w for v, w in zip(voicings, worlds)):
            raise ValueError("voicing cannot be combined with world_pitch on the same utterance")
        voicing_wide = None
        if any(v is not None for v in voicings):
            wide = {tuple(v[key] for key in ("lo", "hi", "window_ms", "bridge", "min_run")) for v in voicings if v is not None}
            if len(wide) != 1:
                raise ValueError("voicing: lo, hi, window_ms, bridge and min_run are call-wide, the deciding utterances ask for "
                                 f"{sorted(wide)}")
            voicing_wide = next(v for v in voicings if v is not None)
        paths = list(match_path) if isinstance(match_path, (list, tuple)) else [match_path] * m
        if len(paths) != m:
            raise ValueError(f"match_path: {len(paths)} values for {m} utterances")
        paths = [common.path_options(v, f"convert_many: match_path[{i}]") for i, v in enumerate(paths)]
        pathed = any(v is not None for v in paths)
        autos = list(auto_pitch) if isinstance(auto_pitch, (list, tuple)) else [auto_pitch] * m
        if len(autos) != m:
            raise ValueError(f"auto_pitch: {len(autos)} values for {m} utterances")
        if not all(isinstance(a, (bool, np.bool_)) for a in autos):
            raise ValueError(f"auto_pitch: expected bools, got {autos}")
        ranged = list(auto_range) if isinstance(auto_range, (list, tuple)) else [auto_range] * m
        if len(ranged) != m:
            raise ValueError(f"auto_range: {len(ranged)} values for {m} utterances")
        if not all(isinstance(a, (bool, np.bool_)) for a in ranged):
            raise ValueError(f"auto_range: expected bools, got {ranged}")
        pitch_range_max = MS.check_range_max(pitch_range_max, "convert_many: pitch_range_max")
        specs = [MS.blend_spec(v, pool, k if ks is None else ks[i]) for i, v in enumerate(voices)]
        targets = [pool.blend_register(*spec) if a else 0.0 for spec, a in zip(specs, autos)]      # (raises: a voice without one)
        target_sds = [pool.blend_range(*spec) if a else 0.0 for spec, a in zip(specs, ranged)]     # (likewise)
        blended = any(len(names) > 1 for names, _ in specs)
        wins, totals, counts = [], [], []
        for u in utterances:
            u = u.reshape(1, -1).to(self.device, torch.float32)
            w, total = make_windows(u, chunk)
            wins.append(w)
            totals.append(total)
            counts.append(w.shape[0])
        windows = torch.cat(wins).contiguous()
        rep = torch.tensor(counts, device=self.device)

        def rows(vals, dtype):
            return torch.repeat_interleave(torch.tensor(vals, dtype=dtype, device=self.device), rep).contiguous()
        params = dict(alpha=rows(alphas, torch.float64), shift=rows(shifts, torch.float32), inton=rows(inton, torch.float32),
                      rate=rows(rates, torch.float32))
        if ks is not None:                  # each window's k; the blended search repeats it on the window's list rows (below)
            params["k"] = rows(ks, torch.int32)
        if any(autos) or any(ranged):       # one group per utterance: its windows' rows, its offset, whether it is on, its target
            first = [0]
            for c in counts:
                first.append(first[-1] + c)
            params["auto"] = dict(first=torch.tensor(first, dtype=torch.int32, device=self.device),
                                  offset=torch.tensor(shifts, dtype=torch.float32, device=self.device),
                                  on=torch.tensor([int(bool(a)) for a in autos], dtype=torch.int32, device=self.device),
                                  target=torch.tensor(targets, dtype=torch.float32, device=self.device))
        if any(ranged):                     # the same groups: each utterance's own intonation, whether it is on, its target range
            params["range"] = dict(inton=torch.tensor(inton, dtype=torch.float32, device=self.device),
                                   on=torch.tensor([int(bool(a)) for a in ranged], dtype=torch.int32, device=self.device),
                                   sd=torch.tensor(target_sds, dtype=torch.float64, device=self.device))
        if not blended:                     # (one-voice blends are their voice: weight 1.0)
            params["ids"] = torch.repeat_interleave(pool.voice_ids([names[0] for names, _ in specs]), rep).contiguous()
        else:                               # compact list rows: window w of utterance i owns S_i of them, in blend order
            owner, lnames, lweights, first = [], [], [], [0]
            w = 0
            for (names, weights), c in zip(specs, counts):
                for _ in range(c):
                    owner += [w] * len(names)
                    lnames += names
                    lweights += weights
                    first.append(first[-1] + len(names))
                    w += 1
            params.update(owner=torch.tensor(owner, dtype=torch.int64, device=self.device), ids=pool.voice_ids(lnames),
                          first=torch.tensor(first, dtype=torch.int32, device=self.device),
                          weight=torch.tensor(lweights, dtype=torch.float64, device=self.device))
            if ks is not None:
                params["k_lists"] = params["k"].index_select(0, params["owner"]).contiguous()
        if pathed:                          # per window: its search k, whether its lists take a path and at what weight, its gather k
            ku = [k] * m if ks is None else ks
            k_win = rows(ku, torch.int32)
            on_win = rows([int(v is not None) for v in paths], torch.int32)
            w_win = rows([v["weight"] if v is not None else 0.0 for v in paths], torch.float64)
            params["path"] = dict(k=k_win, on=on_win, weight=w_win,
                                  gather_k=rows([1 if v is not None else kk for v, kk in zip(paths, ku)], torch.int32))
            if blended:                     # every list row of a window: its owner's
                params["path"].update({key: params["path"][key].index_select(0, params["owner"]).contiguous()
                                       for key in ("k", "on", "weight")})
        # the WORLD windows of every window batch (batch-local row indices, on the device before the batches start)
        on = [bool(w) for w, c in zip(worlds, counts) for _ in range(c)]
        params["world"] = {i: torch.tensor([j - i for j in range(i, min(i + window_batch, len(on))) if on[j]], dtype=torch.int64,
                                           device=self.device) for i in range(0, len(on), window_batch) if any(on[i:i + window_batch])}
        # the tracked windows of every window batch, with their rows' weight and jump.  The class scores of the selected windows are
        # stored: when they are fewer than the 96 frame columns of the plane path, the whole batch is selected and the mask picks
        # the rows (the scores then come from the same kernels as the f0 of the batch)
        params["track"] = {}
        if tracker is not None:
            per_win = [t for t, c in zip(tracks, counts) for _ in range(c)]
            lf_ = windows.shape[1] // 320
            for i in range(0, len(per_win), window_batch):
                part = per_win[i:i + window_batch]
                sel = [j for j, t in enumerate(part) if t is not None]
                if not sel:
                    continue
                if len(sel) * lf_ < 96:
                    sel = list(range(len(part)))
                params["track"][i] = dict(
                    sel=torch.tensor(sel, dtype=torch.int64, device=self.device),
                    on=torch.tensor([int(part[j] is not None) for j in sel], dtype=torch.int32, device=self.device),
                    weight=torch.tensor([part[j]["weight"] if part[j] else 0.0 for j in sel], dtype=torch.float64, device=self.device),
                    jump=torch.tensor([part[j]["jump"] if part[j] else 0.0 for j in sel], dtype=torch.float64, device=self.device))
        # the deciding windows of every window batch: the mask and their rows' thresholds
        params["voicing"] = {}
        if voicing_wide is not None:
            per_win = [v for v, c in zip(voicings, counts) for _ in range(c)]
            f64 = dict(dtype=torch.float64, device=self.device)
            for i in range(0, len(per_win), window_batch):
                part = per_win[i:i + window_batch]
                if any(v is not None for v in part):
                    params["voicing"][i] = dict(
                        mask=torch.tensor([int(v is not None) for v in part], dtype=torch.int32, device=self.device),
                        thr_on=torch.tensor([v["on"] if v else voicing_wide["on"] for v in part], **f64),
                        thr_off=torch.tensor([v["off"] if v else voicing_wide["off"] for v in part], **f64),
                        floor_e=torch.tensor([v["floor_e"] if v else voicing_wide["floor_e"] for v in part], **f64))
        rng = _decoded_range((chunk // 320, 2 * chunk // 320) if trim_context else None, windows.shape[1] // 320)

        def encode(i, feat, f0):
            b = slice(i, i + window_batch)
            if rng is None or pathed:       # (a path runs over the whole window: every frame's features)
                ops.front_end(windows[b], self.ce, self.pe, out=(feat[b], f0[b]))
            else:
                spec = spectrogram(windows[b])
                f0[b] = self.pe.estimate(spec)
                feat[b] = self._encode(spec, rng)
            w = params["world"].get(i)
            if w is not None:               # WORLD's f0 of the whole windows replaces the estimator's (same stream: after it)
                f0[b].index_copy_(0, w, compute_f0(windows[b].index_select(0, w)))
            tr = params["track"].get(i)
            if tr is not None:              # the tracked windows' paths replace the argmax (same stream: after it)
                sub = f0[b].index_select(0, tr["sel"])
                tracker.rows(self.pe.logits(spectrogram(windows[b].index_select(0, tr["sel"]))), sub, tr["on"], tr["weight"], tr["jump"])
                f0[b].index_copy_(0, tr["sel"], sub)
            vo = params["voicing"].get(i)
            if vo is not None:              # the deciding windows' unvoiced frames become 0 (same stream: after the tracker)
                ops.voicing_rows_(f0[b], windows[b], voicing_wide, vo["mask"], vo["thr_on"], vo["thr_off"], vo["floor_e"])

        def transform(f0):                  # each utterance's pitch, intonation and f0 rate (features(world_pitch=True))
            shift, au, rg = params["shift"], params.get("auto"), params.get("range")
            if rg is not None:              # three sums in one call; its first two columns are the auto-pitch call's, bit for bit
                stats3 = MS.pitch_stats2_groups(f0, au["first"], chunk // 320, 2 * chunk // 320)
                if any(autos):
                    shift = MS.pitch_shift_groups(stats3[:, :2].contiguous(), au["first"], f0.shape[0], au["offset"], au["on"],
                                                  au["target"])
                it, centre, centre_on = MS.pitch_range_groups(stats3, au["first"], f0.shape[0], rg["inton"], rg["on"], rg["sd"],
                                                              pitch_range_max)
                MS.pitch_transform_rows_centred_(f0, 0, params["rate"], shift, it, centre, centre_on)
                return
            if au is not None:              # the auto utterances' shifts from the raw f0 of their windows' centre thirds
                stats = MS.pitch_stats_groups(f0, au["first"], chunk // 320, 2 * chunk // 320)
                shift = MS.pitch_shift_groups(stats, au["first"], f0.shape[0], au["offset"], au["on"], au["target"])
            MS.pitch_transform_rows_(f0, 0, params["rate"], shift, params["inton"])

        def search(src):                    # every window's lists, at stride k (a blend: one list row per voice of the window)
            if not blended:
                if ks is None:
                    return MS.knn_search_pool(src, pool, params["ids"], k)
                return MS.knn_search_pool_k(src, pool, params["ids"], params["k"], k)
            src_v = src.index_select(0, params["owner"])
            R, _, t = src_v.shape
            step = max(1, min(MS.POOL_PIECE_ROWS, MS.POOL_PIECE_FRAMES // t))
            if ks is None:
                pieces = [MS.knn_search_pool(src_v[a:a + step], pool, params["ids"][a:a + step], k) for a in range(0, R, step)]
            else:
                pieces = [MS.knn_search_pool_k(src_v[a:a + step], pool, params["ids"][a:a + step],
                                               params["k_lists"][a:a + step].contiguous(), k) for a in range(0, R, step)]
            if len(pieces) == 1:
                return pieces[0]
            return torch.cat([p[0] for p in pieces]), torch.cat([p[1] for p in pieces])

        def match(feat):
            if pathed:                      # over the whole windows: the path call on the lists, the per-row-k gathers at the gather k
                pa = params["path"]
                val, idx = search(feat)
                val, idx, _ = common.knn_path_chunks(val, idx, pa["k"], k, pa["on"], pa["weight"], pool.rows, pool.norms)
                if not blended:
                    out = MS.merge_gather_rows_k(val, idx, pa["gather_k"], k, params["alpha"], pool.rows, feat)
                else:
                    out = MS.blend_gather_rows_k(val, idx, pa["gather_k"], k, params["first"], params["weight"], params["alpha"],
                                                 pool.rows, feat)
                return out if rng is None else out[:, :, rng[0]:rng[1]]
            src = feat if rng is None else feat[:, :, rng[0]:rng[1]].contiguous()
            val, idx = search(src)
            if not blended:
                if ks is None:
                    return MS.merge_gather_rows(val, idx, k, params["alpha"], pool.rows, src)
                return MS.merge_gather_rows_k(val, idx, params["k"], k, params["alpha"], pool.rows, src)
            if ks is None:
                return MS.blend_gather_rows(val, idx, k, params["first"], params["weight"], params["alpha"], pool.rows, src)
            return MS.blend_gather_rows_k(val, idx, params["k"], k, params["first"], params["weight"], params["alpha"], pool.rows,
                                          src)
        out = ops.Fp16Guard(self._agree_on_saturations()).run(
            lambda: self._convert_per_window(windows, rng, window_batch, encode, match, transform))
        res, i = [], 0
        for c, total in zip(counts, totals):
            res.append(stitch(out[i:i + c], total, chunk))
            i += c
        return res

    @staticmethod
    def check_fp16_range():
        """For callers of the LOW-LEVEL ops (ContentEncoder / Decoder objects called directly): raises when a value left fp16's range
        since the counters were last cleared, and clears them.  `convert_windows` / `convert` do not need it: they run under
        ops.Fp16Guard, which repeats a saturated batch on bf16 planes.  Synchronises the device."""
        from . import ops
        n = ops.f16_saturations(reset=True)
        if n > 0:
            raise RuntimeError(f"{n} activation value(s) left fp16's range and were saturated in the fp16 forms of the encoder / decoder GEMMs: "
                               "this checkpoint (or input scale) needs ALIVE_ENCODER_PRECISION=2 and ALIVE_DECODER_PRECISION=2 "
                               "(module.ops.encoder_precision(2), decoder_precision(2)): bf16 planes keep fp32's range")
