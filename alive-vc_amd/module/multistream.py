"""Multi-session streaming: B live voices converted in one batched step per tick (realtime_inference.py:130-183 per slot).

A `MultiStreamConverter` holds B session slots that share the chunk, the ring (buffersize), the sample rates and k.  Each slot has
its own target voice (a segment of a `VoicePool`), pitch shift, f0 rate, alpha, input / output gain, ring and oscillator phase.
One tick runs the whole device pipeline once over [B, ring]: the networks see a batch of B rings, the kNN match is the grouped
exact search (csrc/knn.hip: alive_knn_search_grouped -- row n searches its own pool segment), and the per-user edges read
per-row device arrays (alive_pitch_transform_rows, alive_knn_merge_gather_rows, alive_resample_rows).  Every per-session
value lives in those device arrays, so opening, closing or re-configuring a slot never re-captures the step's hipGraph; the
launch sizes depend on B alone.  Adding a voice to the pool re-packs the pool: the next tick re-captures.

Per slot, as RealtimeConverter.step: the ring fills chunk by chunk, the slot emits None until its ring has held more than
`buffersize` chunks, and the phase is carried through phi[:, :, end_of_output] -- 0 while the slot fills, reset by `open`.
Slots that are closed run on silence with an empty segment.  Interior reuse (RealtimeConverter's reuse_interior) is not
available here.
"""
import numpy as np
import torch

from . import _native as nat
from . import audio_io, ops
from .common import DIM
from .realtime import PLANES_MIN_COLS
from .spectrogram import spectrogram

MAX_K = 8          # the grouped search keeps one register pair per lane and frame (csrc/knn.hip)
_ws = nat.Workspace()


def _tokens_2d(tokens):
    t = tokens
    if t.dim() == 3:
        if t.shape[0] != 1:
            raise ValueError(f"a voice must be [768, M] or [1, 768, M], got {tuple(t.shape)}")
        t = t[0]
    if t.dim() != 2 or t.shape[0] != DIM:
        raise ValueError(f"a voice must be [768, M] or [1, 768, M], got {tuple(tokens.shape)}")
    return t


class VoicePool:
    """Named voices tokens[768, M] packed into one fp32 row table rows[P, 768] with norms[P] (the norms bitwise those of
    PackedLibrary) and a name -> (seg_lo, M) map.  `add` re-packs the pool (a new row table): allowed between ticks, and a
    MultiStreamConverter that replays a captured step re-captures on its next tick."""

    def __init__(self, voices=None, device="cuda"):
        self.device = torch.device(device)
        self._tokens = {}
        self.segments = {}
        self.version = 0
        self.rows = self.norms = None
        self.P = 0
        if voices:
            for name, tok in voices.items():
                self._tokens[str(name)] = _tokens_2d(tok).to(self.device, torch.float32).contiguous()
            self._pack()

    def add(self, name, tokens):
        self._tokens[str(name)] = _tokens_2d(tokens).to(self.device, torch.float32).contiguous()
        self._pack()
        return self

    def segment(self, name):
        if name not in self.segments:
            raise ValueError(f"unknown voice {name!r} (the pool holds {sorted(self.segments)})")
        return self.segments[name]

    def _pack(self):
        L = nat.lib()
        P = sum(int(t.shape[1]) for t in self._tokens.values())
        rows = torch.empty(P, DIM, dtype=torch.float32, device=self.device)
        norms = torch.empty(P, dtype=torch.float32, device=self.device)
        segs, lo = {}, 0
        for name, t in self._tokens.items():
            m = int(t.shape[1])
            if m < 1:
                raise ValueError(f"voice {name!r} is empty")
            nat.check(L.alive_library_pack_rows(nat.ptr(t), m, DIM, rows[lo].data_ptr(), norms[lo].data_ptr(), nat.stream()),
                      "alive_library_pack_rows")
            segs[name] = (lo, m)
            lo += m
        if P >= 2 ** 31:
            raise ValueError(f"a voice pool holds fewer than 2^31 rows (got {P})")
        bad = ~(torch.isfinite(norms) & (norms > 0))          # as PackedLibrary: a zero-norm row would match every frame
        if bool(bad.any()):
            raise ValueError(f"voice pool row {int(torch.nonzero(bad)[0])} has zero or non-finite norm: remove it")
        self.rows, self.norms, self.P, self.segments = rows, norms, P, segs
        self.version += 1


def knn_search_grouped(source, rows, norms, seg_lo, seg_len, k):
    """source [N, 768, T], pool rows / norms, device int32 seg_lo / seg_len [N] -> (val [N*T, k], idx [N*T, k] pool indices)"""
    n, d, t = source.shape
    L = nat.lib()
    if not 1 <= k <= MAX_K:
        raise ValueError(f"grouped search: k={k} outside [1, {MAX_K}]")
    nbytes = L.alive_knn_grouped_workspace_bytes(n, t, k)
    if nbytes == 0:                                         # (before anything is allocated)
        raise ValueError(f"grouped search: {n} rows x {t} frames (k={k}) out of range")
    val = torch.empty(n * t, k, dtype=torch.float32, device=source.device)
    idx = torch.empty(n * t, k, dtype=torch.int32, device=source.device)
    ws = _ws.get(nbytes, source.device)
    nat.check(L.alive_knn_search_grouped(nat.ptr(source), n, t, nat.ptr(rows), nat.ptr(norms), rows.shape[0], nat.ptr(seg_lo),
                                         nat.ptr(seg_len), k, nat.ptr(val), nat.ptr(idx), nat.ptr(ws), nat.stream()),
              "alive_knn_search_grouped")
    return val, idx


def merge_gather_rows(val, idx, k, alpha, rows, source):
    """merge_gather with one shard and a per-window alpha (device float64 [N])"""
    n, d, t = source.shape
    out = torch.empty_like(source)
    nat.check(nat.lib().alive_knn_merge_gather_rows(nat.ptr(val), nat.ptr(idx), k, nat.ptr(alpha), nat.ptr(rows), nat.ptr(source),
                                                    n, t, nat.ptr(out), None, nat.stream()), "alive_knn_merge_gather_rows")
    return out


def pitch_transform_rows_(f0, mode, f0_rate, pitch_shift, intonation):
    """in place on f0 [N, 1, T] with device float32 [N] parameters (ops.pitch_transform_ row by row)"""
    n, _, t = f0.shape
    nat.check(nat.lib().alive_pitch_transform_rows(nat.ptr(f0), n, t, mode, nat.ptr(f0_rate), nat.ptr(pitch_shift),
                                                   nat.ptr(intonation), nat.stream()), "alive_pitch_transform_rows")
    return f0


def resample_rows(x, orig_freq, new_freq, pre_scale, post_scale):
    """x [B, L] -> [B, L'] at new_freq with per-row linear gains (device float32 [B]): audio_io.resample row by row, the gains
    as 10^(dB/20); at equal rates the gains alone"""
    orig, new = audio_io._reduced(orig_freq, new_freq)
    L_ = nat.lib()
    x = x.contiguous()
    b, l = x.shape
    if orig == new:
        filt, lout = None, l
    else:
        key = (orig, new, str(x.device))
        if key not in audio_io._filters:                           # the rate pair's filter bank, shared with audio_io.resample
            f = torch.empty(new * L_.alive_resample_taps(orig, new), device=x.device)
            nat.check(L_.alive_resample_filter(orig, new, nat.ptr(f), nat.stream()), "alive_resample_filter")
            torch.cuda.current_stream(x.device).synchronize()
            audio_io._filters[key] = f
        filt = audio_io._filters[key]
        lout = int(L_.alive_resample_length(l, orig, new))
    y = torch.empty(b, lout, device=x.device)
    nat.check(L_.alive_resample_rows(nat.ptr(x), b, l, orig, new, nat.ptr(filt), nat.ptr(pre_scale), nat.ptr(post_scale),
                                     nat.ptr(y), lout, nat.stream()), "alive_resample_rows")
    return y


def db_scale(db):
    """torchaudio.functional.gain's factor as audio_io.resample forms it (1.0 exactly at 0 dB)"""
    return float(10 ** (db / 20)) if db != 0 else 1.0


_PARAMS = ("voice", "pitch", "f0_rate", "alpha", "gain", "input_gain")


class MultiStreamConverter:
    def __init__(self, content_encoder, f0_estimator, decoder, pool, slots, chunk=960, buffersize=8, input_sr=16000,
                 output_sr=16000, k=4, device="cuda"):
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"MultiStreamConverter: k={k} outside [1, {MAX_K}] (the grouped search keeps k <= 8)")
        if int(slots) < 1 or int(slots) > 1024:
            raise ValueError(f"MultiStreamConverter: slots={slots} outside [1, 1024]")
        self.device = torch.device(device)
        self.ce, self.pe, self.dec = content_encoder.to(device), f0_estimator.to(device), decoder.to(device)
        for net in (self.ce, self.pe, self.dec):
            net.table()
        self.dec._split_for_this_checkpoint()
        self.pool = pool
        self.B, self.k = int(slots), int(k)
        self.chunk, self.buffersize = int(chunk), int(buffersize)
        self.input_sr, self.output_sr = input_sr, output_sr
        internal_chunk = int(chunk * (16000 / output_sr))                  # realtime_inference.py:122-126
        center = int(internal_chunk * buffersize) // 2
        self.end_of_output = center + internal_chunk // 2
        self.begin_of_output = center - internal_chunk // 2
        self.frames = (chunk * buffersize * 16000 // input_sr) // 320
        if self.frames < 5:
            raise ValueError(f"ring of {buffersize} x {chunk} samples is {self.frames} frames; the decoder needs >= 5")
        B, dev = self.B, self.device
        self.n = self.chunk * self.buffersize
        # per-slot state: host side
        self.is_open = [False] * B
        self.params = [None] * B
        self.count = [0] * B
        self.ring = np.zeros((B, self.n), dtype=np.int16)
        # per-slot state: device arrays the (captured) step reads
        self.seg_lo = torch.zeros(B, dtype=torch.int32, device=dev)
        self.seg_len = torch.zeros(B, dtype=torch.int32, device=dev)
        self.alpha = torch.zeros(B, dtype=torch.float64, device=dev)
        self.f0_rate = torch.ones(B, dtype=torch.float32, device=dev)
        self.pitch = torch.zeros(B, dtype=torch.float32, device=dev)
        self.intonation = torch.ones(B, dtype=torch.float32, device=dev)
        self.in_pre = torch.ones(B, dtype=torch.float32, device=dev)
        self.in_post = torch.ones(B, dtype=torch.float32, device=dev)       # input gain: after the resampler (:146-147)
        self.out_pre = torch.ones(B, dtype=torch.float32, device=dev)       # output gain: before the resampler (:173-175)
        self.out_post = torch.ones(B, dtype=torch.float32, device=dev)
        self.emit = torch.zeros(B, 1, dtype=torch.bool, device=dev)          # the slots whose phase advances this tick
        self.phi = torch.zeros(B, 64, device=dev)
        self._in = torch.zeros(B, self.n, device=dev)
        self._graph = None
        self._graph_pool_version = None
        self.captures = 0
        self._side = None
        self._f0_bufs = {}
        self.last_f0 = None
        if self._fp16_guarded():
            ops.f16_clear()

    # ------------------------------------------------------------------ sessions
    def _slot(self, slot):
        if not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < self.B:
            raise ValueError(f"slot {slot!r} out of range [0, {self.B})")
        return int(slot)

    def _apply(self, slot, p):
        lo, m = self.pool.segment(p["voice"])
        if m < self.k:
            raise ValueError(f"voice {p['voice']!r} has {m} vectors, fewer than k={self.k}")
        self.seg_lo[slot] = lo
        self.seg_len[slot] = m
        self.alpha[slot] = float(p["alpha"])
        self.f0_rate[slot] = float(p["f0_rate"])
        self.pitch[slot] = float(p["pitch"])
        self.in_post[slot] = db_scale(p["input_gain"])
        self.out_pre[slot] = db_scale(p["gain"])

    def open(self, slot, voice, pitch=0.0, f0_rate=1.0, alpha=0.0, gain=0.0, input_gain=0.0):
        """start a session in `slot`: empty ring, phase 0"""
        slot = self._slot(slot)
        p = dict(voice=voice, pitch=pitch, f0_rate=f0_rate, alpha=alpha, gain=gain, input_gain=input_gain)
        self._apply(slot, p)                                  # (validates the voice before anything changes)
        self.params[slot] = p
        self.is_open[slot] = True
        self.count[slot] = 0
        self.ring[slot] = 0
        self.phi[slot] = 0.0
        return self

    def set(self, slot, **params):
        """change a session's settings between ticks (voice, pitch, f0_rate, alpha, gain, input_gain)"""
        slot = self._slot(slot)
        if not self.is_open[slot]:
            raise ValueError(f"slot {slot} is not open")
        unknown = set(params) - set(_PARAMS)
        if unknown:
            raise ValueError(f"unknown session settings {sorted(unknown)} (known: {_PARAMS})")
        p = dict(self.params[slot], **params)
        self._apply(slot, p)
        self.params[slot] = p
        return self

    def close(self, slot):
        slot = self._slot(slot)
        self.is_open[slot] = False
        self.params[slot] = None
        self.count[slot] = 0
        self.ring[slot] = 0
        self.seg_len[slot] = 0
        self.phi[slot] = 0.0
        return self

    # ------------------------------------------------------------------ device step
    def _f0_on_side_stream(self, spec):
        """RealtimeConverter._f0_on_side_stream with the per-row pitch transform"""
        cur = torch.cuda.current_stream(spec.device)
        if self._side is None:
            self._side = torch.cuda.Stream(device=spec.device)
        key = (spec.shape[0], spec.shape[2])
        buf = self._f0_bufs.get(key)
        if buf is None:
            buf = self._f0_bufs[key] = torch.empty(spec.shape[0], 1, spec.shape[2], device=spec.device)
        side = self._side
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            f0 = self.pe.estimate(spec, out=buf)
            f0 = pitch_transform_rows_(f0, 1, self.f0_rate, self.pitch, self.intonation)
        return f0, (lambda: cur.wait_stream(side))

    def _device_step(self, data, phi):
        """data float32 [B, ring] on the device, phi [B, 64] -> (wave [B, L] at output_sr, phi_next [B, 64])"""
        data = resample_rows(data, self.input_sr, 16000, self.in_pre, self.in_post)
        spec = spectrogram(data)
        f0, join = self._f0_on_side_stream(spec)
        content = self.ce(spec)
        val, idx = knn_search_grouped(content, self.pool.rows, self.pool.norms, self.seg_lo, self.seg_len, self.k)
        content = merge_gather_rows(val, idx, self.k, self.alpha, self.pool.rows, content)
        join()
        wave, phi_out = self.dec(content, f0=f0, phi=phi, crop=(self.begin_of_output, self.end_of_output))
        self.last_f0 = f0
        wave = resample_rows(wave, 16000, self.output_sr, self.out_pre, self.out_post)
        phi_next = torch.where(self.emit, phi_out[:, :, self.end_of_output], torch.zeros_like(phi))
        return wave, phi_next

    def enable_graph(self):
        """capture the per-tick device pipeline over [B, ring] once; replays read the per-slot device arrays"""
        side = torch.cuda.Stream(device=self.device)
        side.wait_stream(torch.cuda.current_stream())
        saved = self.phi.clone()
        with torch.cuda.stream(side):
            for _ in range(2):
                self._device_step(self._in, self.phi)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        self._graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self._graph):
            wave, phi_next = self._device_step(self._in, self.phi)
            self.phi.copy_(phi_next)
            self._g_out = wave
        self.phi.copy_(saved)
        self._graph_pool_version = self.pool.version
        self.captures += 1
        return self

    def _run(self):
        if self._graph is not None:
            if self._graph_pool_version != self.pool.version:        # the pool was re-packed: its rows moved
                self.enable_graph()
            self._graph.replay()
            return self._g_out
        wave, phi_next = self._device_step(self._in, self.phi)
        self.phi.copy_(phi_next)
        return wave

    def _fp16_guarded(self):
        """as RealtimeConverter: B x frames >= 96 columns select the plane kernels and with them the fp16 forms"""
        return self.B * self.frames >= PLANES_MIN_COLS and (ops.encoder_precision(0) != 2 or ops.decoder_precision(0) != 2)

    def _repeat_on_bf16(self, saved_phi):
        """RealtimeConverter._repeat_on_bf16 for the whole tick: modes 2, every slot's phase restored, the tick again"""
        import warnings
        warnings.warn("an activation left fp16's range in the multi-session streaming step: switching to ALIVE_ENCODER_PRECISION=2 / "
                      "ALIVE_DECODER_PRECISION=2 (bf16 planes) and converting the tick again", RuntimeWarning)
        ops.Fp16Guard.fallbacks += 1
        ops.encoder_precision(2)
        ops.decoder_precision(2)
        self.phi.copy_(saved_phi)
        if self._graph is not None:
            self.enable_graph()
        return audio_io.float_to_pcm16(self._run()).cpu().numpy()

    def step(self, chunks):
        """{slot: int16 chunk} for EVERY open slot -> {slot: converted centre chunk (int16) or None while its ring fills}"""
        for s in chunks:
            self._slot(s)
            if not self.is_open[s]:
                raise ValueError(f"a chunk for slot {s}, which is not open")
        missing = [s for s in range(self.B) if self.is_open[s] and s not in chunks]
        if missing:
            raise ValueError(f"open slots {missing} supplied no chunk this tick")
        emit = [False] * self.B
        for s, c in chunks.items():
            c = np.asarray(c, dtype=np.int16).reshape(-1)
            if c.shape[0] != self.chunk:
                raise ValueError(f"slot {s}: chunk of {c.shape[0]} samples, expected {self.chunk}")
            self.ring[s, :-self.chunk] = self.ring[s, self.chunk:]
            self.ring[s, -self.chunk:] = c
            self.count[s] += 1
            emit[s] = self.count[s] > self.buffersize
        out = {s: None for s in chunks}
        if not any(emit):
            return out
        self.emit.copy_(torch.tensor(emit, device=self.device).view(self.B, 1))
        pcm = torch.from_numpy(self.ring).to(self.device)
        self._in.copy_(audio_io.pcm16_to_float(pcm))
        guarded = self._fp16_guarded()
        if guarded:
            saved_phi = self.phi.clone()
        o = audio_io.float_to_pcm16(self._run()).cpu().numpy()
        if guarded and ops.f16_saturations(reset=True) > 0:
            o = self._repeat_on_bf16(saved_phi)
        center = self.buffersize * self.chunk // 2
        for s in chunks:
            if emit[s]:
                out[s] = o[s, center - self.chunk // 2: center + self.chunk // 2].copy()
        return out
