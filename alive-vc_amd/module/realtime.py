"""Streaming conversion step of the reference's realtime_inference.py:122-191 as a reusable class.

int16 chunk in -> ring of `buffersize` chunks -> spectrogram / content encoder / f0 / kNN /
decoder over the whole ring (exactly what the reference recomputes per step) -> centre chunk out
as int16, with the oscillator phase carried through phi[:, :, end_of_output].

Input gate (`-thr`): RealtimeConverter(gate_db=DB, gate_hold=S) runs the two gate kernels of the multi-session path (csrc/gate.hip,
module/multistream.py "Input gate") at N = 1: alive_gate_rows on the 16 kHz ring after the input gain, alive_gate_apply_rows on the
final wave.  It mutes only: the single-library search has no row mask and runs on.  The gate's state lives beside the phase: `reset`
and `enable_graph` zero it, the bf16 repeat restores it.  Without gate_db the converter launches what it did.

Seam crossfade (`-xf`): RealtimeConverter(crossfade_ms=MS) runs alive_seam_rows (csrc/seam.hip, module/multistream.py "Seam
crossfade") at one row between the output resample and the gate's edge: the head of every chunk is faded in from the previous step's
continuation of itself.  It needs input_sr == output_sr.  The saved tail lives beside the phase: `reset`, `enable_graph` and a
`step_device(continues=False)` drop it (the ring is then unrelated to the previous one), the bf16 repeat restores it.  Without
crossfade_ms the converter launches what it did.

Output limiter (`-lim`): RealtimeConverter(limit_db=DB, limit_lookahead_ms=MS, limit_hold_ms=MS) runs alive_limit_rows (csrc/limit.hip,
module/multistream.py "Limiter") at one row, last, on the emitted span of the final wave: no emitted sample exceeds the ceiling, so the
int16 edge never wraps.  It works on both step forms and with input_sr != output_sr.  The history of required gains lives beside the
phase: `reset`, `enable_graph` and a `step_device(continues=False)` set it to 1.0, the bf16 repeat restores it.  Without limit_db the
converter launches what it did.

Envelope follow (`-env`): RealtimeConverter(envelope=A, envelope_floor_db=, envelope_range_db=, envelope_radius=) runs
alive_envelope_waves (csrc/envelope.hip, module/multistream.py "Envelope follow") at one row right after the decoder, on both step forms:
the decoder's 16 kHz wave takes on the loudness contour of the 16 kHz ring the gate also sees, by the amount A in (0, 1].  It is a
stateless function of the step's ring and wave: nothing is kept between steps.  Without it (A = 0) the converter launches what it did.

Post filter (`-pf`): RealtimeConverter(post_filter=A, post_filter_ratio=, post_filter_tilt=, post_filter_order=, post_filter_window_ms=)
runs alive_postfilter_waves (csrc/postfilter.hip, module/multistream.py "Post filter") at one row right after the decoder and before the
envelope follow, on both step forms: the adaptive formant post filter at alpha A in (0, 0.85] on the decoder's 16 kHz wave.  Stateless
likewise; without it (A = 0) the converter launches what it did.
"""
import numpy as np
import torch

from . import audio_io, common, ops
from .common import PackedLibrary, compute_f0, merge_gather
from .pipeline import prepare_networks
from .spectrogram import spectrogram


# Interior reuse.  A content / f0 frame t of the ring depends on spectrogram frames [t - 12, t + 12] (four k7
# depthwise convs in ContentEncoder and F0Estimator) and those on samples [320 t - 640, 320 t + 640): frames at least EDGE from
# both ring edges do not see the reflect padding, so when the ring advances by a whole number of frames they are the SAME
# values one step later, s frames further left -- and so are their matched features (the kNN is per frame).  What cannot be
# carried over: the oscillator (its phase is a running sum from the ring's first sample, re-anchored every step) and with it
# the whole Filter, i.e. the decoder always runs on the full ring.
# One more condition makes the reuse EXACT rather than merely close: the library picks its kernels by problem size (below 96
# frame COLUMNS -- batch x frames -- the fp32-activation streaming kernels, from 96 the plane-packed split-bf16 GEMMs; the norm
# kernel has a per-frame form for T <= 32), and the two families round differently (1e-5).  A recomputed edge block must
# therefore go through the same kernels as the full ring would.  Blocks are 33 frames (more than 32: the norm kernel's batch
# form either way); under a ring of 96 frames or more the block is run as a BATCH OF THREE identical rows (>= 99 columns: the
# plane-packed family, whose results do not depend on the row), under a shorter ring as it is (its 33 + shift frames must stay
# below 96).  Round 2 used 96-frame blocks for long rings and had to refuse rings of 96 .. 195 frames.
EDGE = 14            # 12 frames of ConvNeXt context + 2 of STFT reflect padding
SPEC_MARGIN = 2      # STFT frames spoiled by the reflect padding of a slice
PLANES_MIN_COLS = 96  # csrc/networks.hip: use_planes()
NORM_SMALL_MAX_T = 32  # csrc/blocks.hip: alive_dwconv_norm's per-frame kernel


def reuse_block(frames, shift):
    """frames of a recomputed edge block (EDGE new frames + margin) under a ring of `frames`, or None where the ring is too
    short for two edge blocks (or, below 96 frames, where a block with the shift would reach the plane-packed family)"""
    blk = NORM_SMALL_MAX_T + 1
    ok = frames >= PLANES_MIN_COLS or blk + shift < PLANES_MIN_COLS
    return blk if ok and frames >= 2 * (blk + SPEC_MARGIN) + shift else None


def reuse_rows(frames):
    """batch rows an edge block is run with: enough identical rows to reach the kernel family of the full ring"""
    blk = NORM_SMALL_MAX_T + 1
    return 1 if frames < PLANES_MIN_COLS else -(-PLANES_MIN_COLS // blk)


def ring_geometry(chunk, buffersize, input_sr, output_sr):
    """realtime_inference.py:122-126: (begin_of_output, end_of_output, frames) of a ring of `buffersize` chunks of `chunk`
    samples at input_sr, converted to output_sr"""
    internal_chunk = int(chunk * (16000 / output_sr))
    center = int(internal_chunk * buffersize) // 2
    frames = (chunk * buffersize * 16000 // input_sr) // 320
    if frames < 5:
        raise ValueError(f"ring of {buffersize} x {chunk} samples is {frames} frames; the decoder needs >= 5 "
                         "(reflection pad 4 on the bottleneck: module/decoder.py:165 of the reference)")
    return center - internal_chunk // 2, center + internal_chunk // 2, frames


def fp16_guarded(cols):
    """Steps of 96 frame columns or more (rings x frames) run the batch kernels and with them the fp16 forms of the encoder /
    decoder GEMMs (modes 1): `step()` then reads the saturation counters after every chunk (it has just synchronised for the PCM
    copy).  Shorter steps -- the reference's defaults -- run the fp32-activation streaming kernels, which write no fp16 plane:
    nothing to guard."""
    return cols >= PLANES_MIN_COLS and (ops.encoder_precision(0) != 2 or ops.decoder_precision(0) != 2)


def f0_on_side_stream(conv, spec, body):
    """The f0 estimator (+ the pitch transform) needs nothing but the spectrogram and feeds nothing before the decoder: its ~35
    dependent launches run on a side stream beside the content encoder and the match (a step is a chain of ~150 small kernels,
    bound by their latencies, not by the chip).  body(buf) computes the transformed f0 [N, 1, F] of `spec` [N, 513, F] into
    `buf` on that stream.  Returns (f0, join): the f0 tensor -- `buf` is a persistent buffer per shape (at most four shapes are
    kept: a converter has one ring geometry and two slice geometries), so that the steady-state step allocates nothing on the
    side stream (the estimator's scratch is sized by the eager warm-up steps that precede hipGraph capture: capture_step) -- and
    the call that makes the current stream wait for it.  The buffer is overwritten by the next call with the same shape: a
    `last_f0` that aliases it is valid until the next step.  Same kernels, same results; captured into the step's hipGraph as
    a parallel branch.  The side stream and the buffers are the converter's `_side` and `_f0_bufs`."""
    cur = torch.cuda.current_stream(spec.device)
    if conv._side is None:
        conv._side = torch.cuda.Stream(device=spec.device)
    key = (spec.shape[0], spec.shape[2])
    buf = conv._f0_bufs.get(key)
    if buf is None:
        if len(conv._f0_bufs) >= 4:
            conv._f0_bufs.pop(next(iter(conv._f0_bufs)))
        buf = conv._f0_bufs[key] = torch.empty(spec.shape[0], 1, spec.shape[2], device=spec.device)
    side = conv._side
    side.wait_stream(cur)                                   # the spectrogram is complete
    with torch.cuda.stream(side):
        f0 = body(buf)
    return f0, (lambda: cur.wait_stream(side))


def track_logits_buf(conv, spec, pe):
    """the buffer that takes the class scores [N, classes, F] of `spec` [N, 513, F] in a tracking converter: allocated once per shape
    (the converter's `_track_bufs`; at most four shapes are kept, as for the f0 buffers), by the eager steps that precede a capture"""
    key = (spec.shape[0], spec.shape[2])
    buf = conv._track_bufs.get(key)
    if buf is None:
        if len(conv._track_bufs) >= 4:
            conv._track_bufs.pop(next(iter(conv._track_bufs)))
        buf = conv._track_bufs[key] = torch.empty(spec.shape[0], pe.sizes[3], spec.shape[2], device=spec.device)
    return buf


def capture_step(device, step, phi):
    """Capture one streaming step into a hipGraph: step() -> (wave, phi_next) runs twice eagerly on a side stream first, so that
    every scratch buffer reaches its steady-state size (the C ABI never allocates or synchronises inside the capture), then once
    under capture with phi_next copied into `phi`.  Returns (graph, the captured step's wave)."""
    side = torch.cuda.Stream(device=device)
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(2):
            step()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        wave, phi_next = step()
        phi.copy_(phi_next)
    return graph, wave


class RealtimeConverter:
    limiter = False                    # (set per converter in __init__: whether the step carries the limiter kernel)
    envelope = False                   # (likewise: whether the step carries the envelope kernel)
    post_filter = False                # (likewise: whether the step carries the post filter kernel)
    pitch_range = False                # (likewise: whether the f0 branch runs the pitch-range follower and the centred transform)
    pitch_track = False                # (likewise: whether the f0 branch stores the class scores and runs the tracker kernel)
    voicing = False                    # (likewise: whether the f0 branch runs the voicing kernels; voicing_state() is the read-back)
    match_path = False                 # (likewise: whether the path call sits between the search and the gather; path_moved() reads back)

    def __init__(self, content_encoder, f0_estimator, decoder, library_tokens, device="cuda", chunk=960, buffersize=8,
                 input_sr=16000, output_sr=16000, f0_rate=1.0, pitch=0.0, k=4, alpha=0.0, gain=0.0, input_gain=0.0,
                 reuse_interior="auto", world_pitch=False, gate_db=None, gate_hold=0.2, gate_lookahead=None,
                 crossfade_ms=None, limit_db=None, limit_lookahead_ms=5.0, limit_hold_ms=20.0, limit_history=0.05,
                 envelope=0.0, envelope_floor_db=-60.0, envelope_range_db=12.0, envelope_radius=1, intonation=1.0,
                 intonation_half_life=10.0, intonation_prior=0.5, pitch_track=None, voicing=None, match_path=None,
                 post_filter=0.0, post_filter_ratio=0.625, post_filter_tilt=0.5, post_filter_order=16, post_filter_window_ms=40.0):
        self.device = torch.device(device)
        path = common.path_options(match_path, "RealtimeConverter: match_path")
        self.match_path = path is not None                  # (checked before anything is built)
        if self.match_path and reuse_interior is True:
            raise ValueError("interior reuse cannot be combined with match_path: a frame's chosen row depends on the whole ring")
        voicing = common.voicing_options(voicing, "RealtimeConverter")
        self.voicing = voicing is not None                  # (checked before anything is built)
        if self.voicing:
            if world_pitch:
                raise ValueError("RealtimeConverter: voicing cannot be combined with world_pitch: WORLD makes its own voicing decision")
            if reuse_interior is True:
                raise ValueError("interior reuse cannot be combined with voicing: a frame's decision depends on the frames around it")
        track = common.track_options(pitch_track, "RealtimeConverter: pitch_track")
        self.pitch_track = track is not None                # (checked before anything is built)
        if self.pitch_track:
            if world_pitch:
                raise ValueError("RealtimeConverter: pitch_track cannot be combined with world_pitch: the tracker decodes the "
                                 "estimator's class scores")
            if reuse_interior is True:
                raise ValueError("interior reuse cannot be combined with pitch_track: a frame's tracked class depends on the whole ring")
            common.pitch_track_tables(track["lo"], track["hi"], track["band"])
        from .multistream import check_intonation
        self.intonation = check_intonation(1.0 if intonation is None else intonation, "RealtimeConverter: intonation")
        self.pitch_range = self.intonation != 1.0           # (checked before anything is built)
        if self.pitch_range:
            if intonation_half_life is not None and not (np.isfinite(intonation_half_life) and intonation_half_life > 0):
                raise ValueError(f"RealtimeConverter: intonation_half_life={intonation_half_life!r} must be > 0 seconds, or None")
            if not (np.isfinite(intonation_prior) and intonation_prior >= 0):
                raise ValueError(f"RealtimeConverter: intonation_prior={intonation_prior!r} must be >= 0 seconds")
        from .multistream import check_envelope
        env = check_envelope(0.0 if envelope is None else envelope, envelope_floor_db, envelope_range_db, envelope_radius)
        self.envelope = env[0] > 0         # (checked before anything is built)
        from .multistream import check_post_filter
        pf = check_post_filter(0.0 if post_filter is None else post_filter, post_filter_ratio, post_filter_tilt, post_filter_order,
                               post_filter_window_ms)
        self.post_filter = pf[0] > 0       # (checked before anything is built)
        self.limiter = limit_db is not None
        if self.limiter:                   # (checked before anything is built)
            from .multistream import check_limit, limit_history_width
            check_limit(limit_db, limit_lookahead_ms, limit_hold_ms)
            limit_width = limit_history_width(limit_history, output_sr)
        self.crossfade = crossfade_ms is not None
        if self.crossfade:                 # (checked before anything is built)
            from .multistream import check_crossfade_ms
            check_crossfade_ms(crossfade_ms)
            if input_sr != output_sr:
                raise ValueError(f"RealtimeConverter: crossfade_ms needs input_sr == output_sr (got {input_sr} and {output_sr}): "
                                 "the ring's advance per step is otherwise not a whole number of output samples")
        self.gate = gate_db is not None
        if self.gate:                      # (checked before anything is built)
            from .multistream import gate_hold_ticks, gate_thr_ms
            thr, ticks = gate_thr_ms(gate_db), gate_hold_ticks(gate_hold, chunk / input_sr)
            if gate_lookahead is not None and not (np.isfinite(gate_lookahead) and gate_lookahead >= 0):
                raise ValueError(f"RealtimeConverter: gate_lookahead={gate_lookahead!r} must be >= 0 seconds, or None (one chunk)")
        self.ce, self.pe, self.dec = prepare_networks(content_encoder, f0_estimator, decoder, device)
        self.lib = library_tokens if isinstance(library_tokens, PackedLibrary) else PackedLibrary(library_tokens[0].to(device))
        self.chunk, self.buffersize = chunk, buffersize
        self.input_sr, self.output_sr = input_sr, output_sr
        self.f0_rate, self.pitch, self.k, self.alpha, self.gain, self.input_gain = f0_rate, pitch, k, alpha, gain, input_gain
        self.begin_of_output, self.end_of_output, frames = ring_geometry(chunk, buffersize, input_sr, output_sr)
        self.ring = []
        self.phi = 0
        self._graph = None
        self.last_f0 = None
        if self.gate:
            # the multi-session gate at one row: an always-emitting session with one (unused) list row; _gate_state = (hold_left,
            # was_open) is the stream's, like the phase
            dev, i32 = self.device, dict(dtype=torch.int32, device=self.device)
            self.gate_db, self.gate_hold = float(gate_db), float(gate_hold)
            self._gate_look16 = int(round((chunk / input_sr if gate_lookahead is None else float(gate_lookahead)) * 16000))
            self._gate_on = torch.ones(1, **i32)
            self._gate_thr = torch.tensor([thr], dtype=torch.float64, device=dev)
            self._gate_hold = torch.tensor([ticks], **i32)
            self._gate_emit = torch.ones(1, dtype=torch.bool, device=dev)
            self._gate_seg = torch.zeros(1, **i32)
            self._gate_seg_eff = torch.zeros(1, **i32)
            self._gate_follow = torch.zeros(1, dtype=torch.bool, device=dev)
            self._gate_state = torch.zeros(1, 2, **i32)
            self._g0 = torch.ones(1, device=dev)
            self._g1 = torch.ones(1, device=dev)
            self._span_lo = torch.tensor([buffersize * chunk // 2 - chunk // 2], **i32)
            self._span_len = torch.tensor([2 * (chunk // 2)], **i32)
        if self.crossfade:
            # the multi-session crossfade at one row: an always-emitting session; _seam_tail / _seam_stored are the stream's, like
            # the phase
            from .multistream import seam_geometry, wave_length
            dev, i32 = self.device, dict(dtype=torch.int32, device=self.device)
            self.crossfade_ms = float(crossfade_ms)
            self._row_len = wave_length(frames, output_sr)
            lo, shift, x = seam_geometry(chunk, buffersize, output_sr, crossfade_ms, self._row_len)
            self._seam_lo = torch.tensor([lo], **i32)
            self._seam_shift = torch.tensor([shift], **i32)
            self._seam_x = torch.tensor([x], **i32)
            self._seam_emit = torch.ones(1, dtype=torch.bool, device=dev)
            self._seam_tail = torch.zeros(1, 2 * (chunk // 2), device=dev)
            self._seam_stored = torch.zeros(1, **i32)
            self._seam_stats = torch.zeros(1, 2, dtype=torch.float64, device=dev)
        if self.limiter:
            # the multi-session limiter at one row: an always-emitting session; _limit_hist is the stream's, like the phase
            from .multistream import limit_geometry, wave_length
            dev, i32 = self.device, dict(dtype=torch.int32, device=self.device)
            self.limit_db_, self.limit_lookahead_ms, self.limit_hold_ms = float(limit_db), float(limit_lookahead_ms), float(limit_hold_ms)
            self._limit_len = wave_length(frames, output_sr)
            shift = chunk if input_sr == output_sr else max(chunk, int(round(chunk * output_sr / input_sr)))
            lo, shift, look, hold, c = limit_geometry(chunk, buffersize, output_sr, limit_db, limit_lookahead_ms, limit_hold_ms,
                                                      self._limit_len, limit_width, shift)
            self._limit_lo = torch.tensor([lo], **i32)
            self._limit_span = torch.tensor([2 * (chunk // 2)], **i32)
            self._limit_shift = torch.tensor([shift], **i32)
            self._limit_look = torch.tensor([look], **i32)
            self._limit_hold = torch.tensor([hold], **i32)
            self._limit_ceil = torch.tensor([c], dtype=torch.float32, device=dev)
            self._limit_emit = torch.ones(1, dtype=torch.bool, device=dev)
            self._limit_hist = torch.ones(1, limit_width, device=dev)
            self._limit_gmin = torch.ones(1, device=dev)
        if self.envelope:
            # the multi-session envelope follow at one row; no state: a function of the step's ring and wave.  _env_out is allocated
            # once, by the first step
            self._env = env[1:]                # (floor_ms, g_lo, g_hi, radius)
            self._env_amount = torch.tensor([env[0]], dtype=torch.float32, device=self.device)
            self._env_out = None
        if self.post_filter:
            # the multi-session post filter at one row; no state: a function of the step's wave.  _pf_out is allocated once, by the
            # first step
            from .multistream import postfilter_tables
            self._pf = pf[1:]                  # (ratio, tilt, order, window, floor_ms, g_lo, g_hi)
            self._pf_win, self._pf_lag = postfilter_tables(pf[4], pf[3], self.device)
            self._pf_alpha = torch.tensor([pf[0]], dtype=torch.float32, device=self.device)
            self._pf_out = None
        if self.pitch_range:
            # the multi-session pitch range at one row: an always-emitting session without auto pitch or auto range (there is no
            # pool); _reg_state = (S, W, Q) is the stream's, like the phase
            from .multistream import auto_constants
            dev, i32, f32 = self.device, dict(dtype=torch.int32, device=self.device), dict(dtype=torch.float32, device=self.device)
            self._range_decay, self._range_prior = auto_constants(chunk / input_sr, buffersize, intonation_half_life,
                                                                  intonation_prior)
            self._reg_state = torch.zeros(1, 3, dtype=torch.float64, device=dev)
            self._range_rate = torch.tensor([1.0 if world_pitch else f0_rate], **f32)
            self._range_pitch = torch.tensor([pitch], **f32)
            self._range_inton = torch.tensor([self.intonation], **f32)
            self._range_off = torch.zeros(1, **i32)            # (auto_on and range_on: both off)
            self._range_zero = torch.zeros(1, **f32)
            self._range_sd = torch.zeros(1, dtype=torch.float64, device=dev)
            self._range_emit = torch.ones(1, dtype=torch.bool, device=dev)
            self._shift_eff, self._inton_eff = torch.zeros(1, **f32), torch.ones(1, **f32)
            self._centre, self._centre_on = torch.zeros(1, **f32), torch.zeros(1, **i32)
        if self.pitch_track:
            # the multi-session tracker at one row; no state: the whole ring is decoded again every step.  The logits buffer is
            # allocated once per shape, by the first step
            dev = self.device
            self._track = common.pitch_track(track["lo"], track["hi"], track["band"], dev)
            self.track_weight, self.track_jump = track["weight"], track["jump"]
            self._track_on = torch.ones(1, dtype=torch.int32, device=dev)
            self._track_weight = torch.tensor([track["weight"]], dtype=torch.float64, device=dev)
            self._track_jump = torch.tensor([track["jump"]], dtype=torch.float64, device=dev)
            self._track_changed = torch.zeros(1, dtype=torch.int32, device=dev)
            self._track_bufs = {}
        if self.match_path:
            # the multi-session path call at one row, between the search and the gather; no state: the whole ring's path every step
            dev = self.device
            self.path_weight = path["weight"]
            self._path_k = torch.full((1,), int(k), dtype=torch.int32, device=dev)
            self._path_on = torch.ones(1, dtype=torch.int32, device=dev)
            self._path_weight = torch.tensor([path["weight"]], dtype=torch.float64, device=dev)
            self._path_moved = torch.zeros(1, dtype=torch.int32, device=dev)
        if self.voicing:
            # the multi-session detector at one row; no state: it looks at the whole ring again every step
            dev = self.device
            self._voicing = voicing
            self._voicing_rows = [torch.tensor([voicing[key]], dtype=torch.float64, device=dev) for key in ("on", "off", "floor_e")]
            self._voicing_out = dict(r=torch.zeros(1, frames, dtype=torch.float64, device=dev),
                                     voiced=torch.zeros(1, frames, dtype=torch.int32, device=dev),
                                     changed=torch.zeros(1, dtype=torch.int32, device=dev))
        self._side = None                  # side stream of the f0 estimator (see _f0_on_side_stream)
        self._f0_bufs = {}
        # interior reuse: only where it is exact -- no resampling in front (the ring IS the 16 kHz signal), a shift of whole
        # frames, and a ring long enough that the two recomputed edge blocks do not meet.  "auto": on when that holds.
        self.frames, self.shift = frames, chunk // 320
        self._blk = reuse_block(frames, self.shift) if (input_sr == 16000 and chunk % 320 == 0 and
                                                        (chunk * buffersize) % 320 == 0) else None
        fits = self._blk is not None
        # world_pitch (`-wpe`): f0 is WORLD's DIO + StoneMask of the whole ring (module/common.py compute_f0), whose mean removal
        # and contour fixing span the ring -- no frame of it can be kept from the previous step, so interior reuse is off
        self.world_pitch = bool(world_pitch)
        if reuse_interior is True and self.world_pitch:
            raise ValueError("interior reuse cannot be combined with world_pitch: WORLD's f0 of a ring depends on the whole ring")
        if self.world_pitch:
            fits = False
        # intonation: every frame is scaled around the running mean of the step that transforms it, so a carried frame would keep an
        # earlier step's centre -- interior reuse is off
        if reuse_interior is True and self.pitch_range:
            raise ValueError("interior reuse cannot be combined with intonation: the carried f0 frames were transformed around an "
                             "earlier step's centre")
        if self.pitch_range:
            fits = False
        # pitch_track: a frame's tracked class depends on the whole ring (the path is decoded again every step) -- interior reuse is off
        if self.pitch_track:
            fits = False
        # voicing: hysteresis, bridge and minimum run make a frame's decision depend on the ring around it -- interior reuse is off
        if self.voicing:
            fits = False
        # match_path: a frame's chosen row depends on the whole ring (the path is decoded again every step) -- interior reuse is off
        if self.match_path:
            fits = False
        if reuse_interior is True and not fits:
            raise ValueError("interior reuse needs input_sr 16000, chunk a multiple of 320 and a ring of at least 70 + chunk / 320 "
                             f"frames (below 96 frames: 33 + chunk / 320 < 96); got {frames} frames: see module/realtime.py")
        self.reuse = bool(fits and reuse_interior in (True, "auto"))
        self._rows = reuse_rows(frames)
        self._cache_valid = False
        if fp16_guarded(frames):
            ops.f16_clear()                # stale counts of earlier work in this process are not this stream's
        if self.reuse:
            self._c_feat = torch.zeros(1, 768, frames, device=self.device)      # matched features of the ring's frames
            self._c_f0 = torch.zeros(1, 1, frames, device=self.device)          # transformed f0

    # ------------------------------------------------------------------ device part of one step
    def _device_step(self, data, phi):
        """data float32 [1, ring samples at input_sr] on the device, phi [1, 64] -> (wave at output_sr [L], phi_next [1, 64])"""
        if self.reuse:
            return self._device_step_reuse(data, phi)
        data = audio_io.resample(data, self.input_sr, 16000, post_gain_db=self.input_gain)     # resample, then gain (:146-147)
        self._gate_decide(data)
        content, f0 = self._front_end(spectrogram(data), data)
        wave, phi_out = self.dec(content, f0=f0, phi=phi, crop=(self.begin_of_output, self.end_of_output))
        self.last_f0 = f0                  # (a view of the per-shape side-stream buffer: valid until the next step)
        wave = self._follow(self._postfilter(wave), data)
        wave = self._limit(self._gate_edge(self._seam(audio_io.resample(wave, 16000, self.output_sr, pre_gain_db=self.gain))))[0]   # gain, then resample
        return wave, phi_out[:, :, self.end_of_output]

    def _gate_decide(self, data):
        """gate on: this step's decision from the 16 kHz ring `data` [1, L] (alive_gate_rows at one row) into _g0 / _g1"""
        if self.gate:
            from .multistream import gate_rows, gate_window
            data = data.contiguous()
            w_lo, w_hi = gate_window(self.begin_of_output, self.end_of_output, data.shape[1], self._gate_look16)
            gate_rows(data, w_lo, w_hi, self._gate_on, self._gate_thr, self._gate_hold, self._gate_emit, None, 1, self._gate_seg,
                      self._gate_state, self._g0, self._g1, self._gate_seg_eff, self._gate_follow, None)

    def _gate_edge(self, wave):
        """gate on: the fade (or the mute) on the emitted span of the final wave [1, L], in place"""
        if self.gate:
            from .multistream import gate_apply_rows_
            wave = gate_apply_rows_(wave.contiguous(), self._span_lo, self._span_len, self._g0, self._g1)
        return wave

    def _seam(self, wave):
        """crossfade on: the head of the emitted span of the final wave [1, L] faded in from the previous step's continuation, in
        place, and this step's continuation saved (alive_seam_rows at one row; before the gate's edge, with its gains)"""
        if self.crossfade:
            from .multistream import seam_rows_
            if wave.shape[1] != self._row_len:
                raise RuntimeError(f"final wave of {wave.shape[1]} samples, the crossfade expects {self._row_len}")
            wave = seam_rows_(wave.contiguous(), self._seam_lo, self._seam_shift, self._seam_x, self._seam_emit, self._seam_tail,
                              self._seam_stored, self._g0 if self.gate else None, self._g1 if self.gate else None,
                              self._seam_stats)
        return wave

    def _postfilter(self, wave):
        """post filter on: the decoder's 16 kHz wave [1, L] through alive_postfilter_waves at one row, into the buffer allocated once
        (right after the decoder, before the envelope follow)"""
        if self.post_filter:
            from .multistream import POSTFILTER_HOP, postfilter_waves_
            wave = wave.contiguous()
            if self._pf_out is None or self._pf_out.shape != wave.shape:
                self._pf_out = torch.empty_like(wave)
            ratio, tilt, order, window, floor_ms, g_lo, g_hi = self._pf
            wave = postfilter_waves_(self._pf_out, wave, None, self._pf_alpha, POSTFILTER_HOP, window, order, self._pf_win,
                                     self._pf_lag, ratio, tilt, floor_ms, g_lo, g_hi)
        return wave

    def _follow(self, wave, data):
        """envelope on: the decoder's 16 kHz wave [1, L] at the loudness contour of the 16 kHz ring `data` [1, L16], into the buffer
        allocated once (alive_envelope_waves at one row; right after the decoder, before the output resample)"""
        if self.envelope:
            from .multistream import ENVELOPE_HOP, envelope_waves_
            wave, data = wave.contiguous(), data.contiguous()
            if self._env_out is None or self._env_out.shape != wave.shape:
                self._env_out = torch.empty_like(wave)
            floor_ms, g_lo, g_hi, radius = self._env
            wave = envelope_waves_(self._env_out, wave, data, None, self._env_amount, ENVELOPE_HOP, radius, floor_ms, g_lo, g_hi)
        return wave

    def _limit(self, wave):
        """limiter on: the emitted span of the final wave [1, L] limited to the ceiling, in place, its lookahead taken one chunk on
        (alive_limit_rows at one row; last, after the gate's edge)"""
        if self.limiter:
            from .multistream import limit_rows_
            if wave.shape[1] != self._limit_len:
                raise RuntimeError(f"final wave of {wave.shape[1]} samples, the limiter expects {self._limit_len}")
            wave = limit_rows_(wave.contiguous(), self._limit_lo, self._limit_span, self._limit_shift, self._limit_look,
                               self._limit_hold, self._limit_ceil, self._limit_emit, self._limit_hist, self._limit_gmin)
        return wave

    def _limit_reset(self):
        if self.limiter:
            self._limit_hist.fill_(1.0)
            self._limit_gmin.fill_(1.0)

    def limit_db(self):
        """how far the limiter turned the latest step down: 20 log10 of the smallest gain of its emitted span; 0.0: untouched (one
        host read)"""
        if not self.limiter:
            raise ValueError("limit_db needs a converter built with RealtimeConverter(..., limit_db=DB)")
        from .multistream import gmin_db
        return gmin_db(self._limit_gmin.tolist())[0]

    def pitch_track_changed(self):
        """how many frames of the ring the tracker moved off the per-frame argmax in the latest step (one host read)"""
        if not self.pitch_track:
            raise ValueError("pitch_track_changed needs a converter built with RealtimeConverter(..., pitch_track=True)")
        return int(self._track_changed.tolist()[0])

    def path_moved(self):
        """how many frames of the ring the match path moved off the frame's nearest row in the latest step (one host read)"""
        if not self.match_path:
            raise ValueError("path_moved needs a converter built with RealtimeConverter(..., match_path=True)")
        return int(self._path_moved.tolist()[0])

    def voicing_state(self):
        """the voicing decision of the latest step: (voiced frames of the ring, frames whose f0 was set to 0, r of the centre frame of
        the emitted span), read back from the device"""
        if not self.voicing:
            raise ValueError("voicing_state needs a converter built with RealtimeConverter(..., voicing=True)")
        o = self._voicing_out
        centre = min((self.begin_of_output + self.end_of_output) // 2 // 320, self.frames - 1)      # (the span is in 16 kHz samples)
        return int(o["voiced"].sum()), int(o["changed"][0]), float(o["r"][0, centre])

    def _f0_on_side_stream(self, spec, data=None):
        """f0_on_side_stream with the estimator's f0 and the pitch transform.  With world_pitch the branch is WORLD's f0 of the
        16-kHz ring `data` instead, and the pitch transform leaves out f0_rate: the reference multiplies only the estimator's f0
        by it (realtime_inference.py:153-156)."""
        def ranged(f0):                    # the multi-session follower and centred transform at one row
            from .multistream import pitch_follow2_rows_, pitch_transform_rows_centred_
            emit = self._gate_follow if self.gate else self._range_emit     # (a gated stream's state learns from open ticks only)
            pitch_follow2_rows_(f0, self._range_rate, self._range_pitch, self._range_off, self._range_zero, self._range_inton,
                                self._range_off, self._range_sd, emit, self._range_decay, self._range_prior, 1.0,
                                self._reg_state, self._shift_eff, self._inton_eff, self._centre, self._centre_on)
            return pitch_transform_rows_centred_(f0, 1, self._range_rate, self._shift_eff, self._inton_eff, self._centre,
                                                 self._centre_on)

        def body(buf):
            if self.world_pitch:
                buf.copy_(compute_f0(data))
                if self.pitch_range:
                    return ranged(buf)
                return ops.pitch_transform_(buf, 1, f0_rate=1.0, pitch_shift=self.pitch)
            if self.pitch_track:               # the class scores stored, their argmax, then the Viterbi path over it
                f0 = self.pe.estimate(spec, out=buf, track=self._track, track_on=self._track_on, track_weight=self._track_weight,
                                      track_jump=self._track_jump, logits_out=track_logits_buf(self, spec, self.pe),
                                      changed=self._track_changed)
            else:
                f0 = self.pe.estimate(spec, out=buf)
            if self.voicing:                   # f0 = 0 where the ring is not periodic, before the follower and the transform
                ops.voicing_rows_(f0, data.contiguous(), self._voicing, None, *self._voicing_rows, self._voicing_out)
            if self.pitch_range:
                return ranged(f0)
            return ops.pitch_transform_(f0, 1, f0_rate=self.f0_rate, pitch_shift=self.pitch)
        return f0_on_side_stream(self, spec, body)

    def _front_end(self, spec, data=None):
        """spectrogram [R, 513, F] (of the 16 kHz ring `data`) -> (matched content [R, 768, F], transformed f0 [R, 1, F])"""
        f0, join = self._f0_on_side_stream(spec, data)
        content = self.ce(spec)
        val, idx = self.lib.search(content, self.k)
        if self.match_path:                # one row per frame, chosen by the path over the ring's lists, gathered as a k = 1 match
            val, idx, _ = ops.knn_path_rows(val, idx, self._path_k, self.k, self._path_on, self._path_weight, self.lib.rows,
                                            self.lib.norms, moved=self._path_moved)
            out = merge_gather(val[:, :1].contiguous(), idx[:, :1].contiguous(), 1, 1, self.alpha, self.lib.rows, content)
        else:
            out = merge_gather(val, idx, 1, self.k, self.alpha, self.lib.rows, content)
        join()
        return out, f0

    def _device_step_reuse(self, data, phi):
        """the same step with the front end computed for the two edge blocks only; interior frames come from the previous
        step's ring, `shift` frames further right.  Bitwise the full computation (tests/test_gpu_cli.py)."""
        F_, s = self.frames, self.shift
        data = data if self.input_gain == 0 else audio_io.gain(data, self.input_gain)
        self._gate_decide(data)
        if not self._cache_valid:
            feat, f0 = self._front_end(spectrogram(data))
            self._c_feat.copy_(feat)
            self._c_f0.copy_(f0)
            self._cache_valid = True
        else:
            keep_f, keep_p = self._c_feat[:, :, s:].clone(), self._c_f0[:, :, s:].clone()
            self._c_feat[:, :, :F_ - s].copy_(keep_f)
            self._c_f0[:, :, :F_ - s].copy_(keep_p)
            nl = self._blk                                            # left block: frames [0, EDGE) from a slice of nl frames
            margin = nl - EDGE                                        # >= 19 > the 12 frames of context
            feat, f0 = self._front_end_slice(data[:, :(nl + SPEC_MARGIN) * 320], 0, nl)
            self._c_feat[:, :, :EDGE].copy_(feat[:, :, :EDGE])
            self._c_f0[:, :, :EDGE].copy_(f0[:, :, :EDGE])
            a = F_ - EDGE - s                                         # right block: frames [a, F)
            lo = a - margin
            feat, f0 = self._front_end_slice(data[:, (lo - SPEC_MARGIN) * 320:], SPEC_MARGIN, SPEC_MARGIN + F_ - lo)
            self._c_feat[:, :, a:].copy_(feat[:, :, margin:])
            self._c_f0[:, :, a:].copy_(f0[:, :, margin:])
        wave, phi_out = self.dec(self._c_feat, f0=self._c_f0, phi=phi, crop=(self.begin_of_output, self.end_of_output))
        self.last_f0 = self._c_f0
        wave = self._follow(self._postfilter(wave), data)
        wave = self._limit(self._gate_edge(self._seam(audio_io.resample(wave, 16000, self.output_sr, pre_gain_db=self.gain))))[0]
        return wave, phi_out[:, :, self.end_of_output]

    def _front_end_slice(self, samples, f_lo, f_hi):
        """front end on a slice of the ring: spectrogram of `samples`, frames [f_lo, f_hi) of it through the networks and the
        match (the frames outside are spoiled by the slice's own reflect padding)"""
        samples = samples.contiguous()
        if self._rows > 1:                                  # identical rows: same kernels as the full ring (see the header)
            samples = samples.expand(self._rows, -1).contiguous()
        out, f0 = self._front_end(spectrogram(samples)[:, :, f_lo:f_hi].contiguous())
        return out[:1], f0[:1].clone()                   # (f0 lives in a per-shape buffer the next slice overwrites)

    def enable_graph(self):
        """Capture the whole per-step device pipeline (~150 launches) into one hipGraph: the C ABI never allocates or
        synchronises, and every scratch buffer reaches its steady-state size during the warm-up steps below."""
        n = self.chunk * self.buffersize
        self._g_in = torch.zeros(1, n, device=self.device)
        self._g_phi = torch.zeros(1, 64, device=self.device)
        self._graph, self._g_out = capture_step(self.device, lambda: self._device_step(self._g_in, self._g_phi), self._g_phi)
        self._g_phi.zero_()
        if self.gate:
            self._gate_state.zero_()       # (capture_step ran the step three times)
        if self.pitch_range:
            self._reg_state.zero_()
        if self.crossfade:
            self._seam_stored.zero_()
        self._limit_reset()
        self._cache_valid = False          # interior reuse: the captured step is the incremental one; the first real step runs in full
        return self

    def reset(self):
        """start a new stream on this converter: empty ring, phase 0, and the interior-reuse caches invalid (the next step runs
        the full front end).  Call it whenever the chunk sequence restarts or a chunk was dropped / duplicated."""
        self.ring = []
        self.phi = 0
        self._cache_valid = False
        if getattr(self, "_graph", None) is not None:
            self._g_phi.zero_()
        if self.gate:
            self._gate_state.zero_()
        if self.pitch_range:
            self._reg_state.zero_()
        if self.crossfade:
            self._seam_stored.zero_()
        self._limit_reset()
        return self

    def seam_db(self):
        """the seam statistic of the latest step: 10 log10(sum (c - t)^2 / sum c^2) over the faded head, c the step's own decode and
        t the previous step's continuation; nan if the step did not fade (one host read)"""
        if not self.crossfade:
            raise ValueError("seam_db needs a converter built with RealtimeConverter(..., crossfade_ms=MS)")
        from .multistream import stats_db
        return stats_db(self._seam_stats.tolist())[0]

    def gate_open(self):
        """whether the gate was open at the end of the latest step (one host read)"""
        if not self.gate:
            raise ValueError("gate_open needs a converter built with RealtimeConverter(..., gate_db=DB)")
        return bool(self._gate_state[0, 1].item())

    def step_device(self, ring_f32, continues=False):
        """ring float32 [1, buffersize*chunk] already on the device -> wave [L] (device); phase carried internally.

        Contract of interior reuse (on when the ring geometry allows, see `reuse_block`): the matched features and f0 of the
        ring's interior frames are carried over from the previous call, which is only right when `ring_f32` IS the previous
        ring advanced by exactly one chunk.  The caller says so with `continues=True` (`step()` does: it owns the ring);
        the default treats the ring as unrelated to the previous one and recomputes the whole front end -- and, with a crossfade,
        drops the saved tail: the previous wave's continuation says nothing about an unrelated ring."""
        if not continues:
            self._cache_valid = False
            if self.crossfade:
                self._seam_stored.zero_()
            self._limit_reset()
        return self._step_device(ring_f32)

    def _step_device(self, ring_f32):
        if getattr(self, "_graph", None) is not None:
            if self.reuse and not self._cache_valid:             # fills the frame caches the captured (incremental) step reads
                wave, phi_next = self._device_step(ring_f32, self._g_phi)
                self._g_phi.copy_(phi_next)
                return wave
            self._g_in.copy_(ring_f32)
            self._graph.replay()
            return self._g_out
        phi = self.phi if isinstance(self.phi, torch.Tensor) else torch.zeros(1, 64, device=self.device)
        wave, phi_next = self._device_step(ring_f32, phi)
        self.phi = phi_next
        return wave

    def _repeat_on_bf16(self, data, saved_phi, saved_gate=None, saved_seam=None, saved_limit=None, saved_reg=None):
        """a chunk drove an activation out of fp16's range: switch the process to bf16 planes (ops.switch_to_bf16), restore the
        phase (and the gate state, and the crossfade's tail) the chunk started from, drop the frame caches, re-capture the step if it
        was a hipGraph, and convert the chunk again -- the whole front end, but crossfaded as the first attempt would have been"""
        ops.switch_to_bf16("streaming step", "chunk")
        self._cache_valid = False
        if getattr(self, "_graph", None) is not None:
            self.enable_graph()
            self._g_phi.copy_(saved_phi)
        else:
            self.phi = saved_phi
        if saved_gate is not None:
            self._gate_state.copy_(saved_gate)
        if saved_reg is not None:          # (after enable_graph, which zeroes it)
            self._reg_state.copy_(saved_reg)
        if saved_seam is not None:
            self._seam_tail.copy_(saved_seam[0])
            self._seam_stored.copy_(saved_seam[1])
        if saved_limit is not None:
            self._limit_hist.copy_(saved_limit[0])
            self._limit_gmin.copy_(saved_limit[1])
        wave = self._step_device(data)                  # (not step_device(continues=False), which would drop the restored tail)
        return audio_io.float_to_pcm16(wave).cpu().numpy()

    def step(self, data_int16: np.ndarray):
        """one chunk of int16 samples -> converted centre chunk (int16), or None while the ring fills
        (the reference's loop emits nothing until it holds more than `buffersize` chunks: :133-137)."""
        self.ring.append(np.asarray(data_int16, dtype=np.int16))
        if len(self.ring) > self.buffersize:
            del self.ring[0]
        else:
            return None
        data = torch.from_numpy(np.concatenate(self.ring, 0)).to(self.device)
        data = audio_io.pcm16_to_float(data).unsqueeze(0)            # / 32768 on the device (:139-140)
        guarded = fp16_guarded(self.frames)
        if guarded:
            saved_phi = self._g_phi.clone() if getattr(self, "_graph", None) is not None else self.phi
            saved_gate = self._gate_state.clone() if self.gate else None
            saved_seam = (self._seam_tail.clone(), self._seam_stored.clone()) if self.crossfade else None
            saved_limit = (self._limit_hist.clone(), self._limit_gmin.clone()) if self.limiter else None
            saved_reg = self._reg_state.clone() if self.pitch_range else None
        wave = self.step_device(data, continues=True)                # this ring is the previous one advanced by one chunk
        out = audio_io.float_to_pcm16(wave).cpu().numpy()            # C cast of numpy's astype, no clipping (:180-183)
        if guarded and ops.f16_saturations(reset=True) > 0:          # (the copy above has synchronised: six 4-byte reads)
            out = self._repeat_on_bf16(data, saved_phi, saved_gate, saved_seam, saved_limit, saved_reg)
        center = self.buffersize * self.chunk // 2
        return out[center - self.chunk // 2: center + self.chunk // 2]
