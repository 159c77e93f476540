"""Multi-session streaming: B live voices converted in one batched step per tick (realtime_inference.py:130-183 per slot).

A `MultiStreamConverter` holds B session slots that share the chunk duration and the ring (buffersize).  Each slot has its own
target voice (a segment of a `VoicePool`), pitch shift, f0 rate, alpha, input / output gain, ring and oscillator phase, -- in a
converter built with k_max= -- its own k (see "Per-session k" below), and -- with
`rates=` declared up front and input_sr == output_sr -- its own sample rate: a session at rate r sends and receives
chunk * r / input_sr samples per tick, and its ring at 16 kHz has the converter's geometry (session_geometry), so only the two
resampling edges differ per row (alive_resample_rows_multi: one launch, every row at its own rate pair).
One tick runs the whole device pipeline once over [B, ring]: the networks see a batch of B rings, the kNN match is the grouped
exact search (csrc/knn.hip: alive_knn_search_grouped -- row n searches its own pool segment), and the per-user edges read
per-row device arrays (alive_pitch_transform_rows, alive_knn_merge_gather_rows, alive_resample_rows).  Every per-session
value lives in those device arrays, so opening, closing or re-configuring a slot never re-captures the step's hipGraph; the
launch sizes depend on B alone.  Adding a voice to a default pool re-packs the pool: the next tick re-captures.  On a reserved
pool (VoicePool(capacity=ROWS): one table for the pool's life) voices are enrolled, grown, removed and compacted between ticks
without a re-capture: the slots hold their voices, and a tick that finds pool.layout changed rewrites its segment arrays first.

Per slot, as RealtimeConverter.step: the ring fills chunk by chunk, the slot emits None until its ring has held more than
`buffersize` chunks, and the phase is carried through phi[:, :, end_of_output] -- 0 while the slot fills, reset by `open`.
Slots that are closed run on silence with an empty segment.  Interior reuse (RealtimeConverter's reuse_interior) is not
available here.

WORLD pitch (`-wpe` per session): a converter built with world_pitch=True adds one masked WORLD branch over all B rings
(common.compute_f0_rows: alive_world_f0_rows) on the f0 side stream, after the estimator; a session opened or set with
world_pitch=True takes that f0 instead of the estimator's, as RealtimeConverter(world_pitch=True) does: WORLD's f0 of its 16-kHz
ring (after the input resample and gain), the mode-1 transform with its pitch shift, and NOT its f0_rate (the reference
multiplies only the estimator's f0 by it).  The mask and the per-row choice are device arrays: switching costs no re-capture.
WORLD needs the whole ring: rings shorter than about 230 ms (-c 160 -b 16 is 160 ms) come out unvoiced.

Voice blending: a session's voice may be a weighted mix of up to `blend` voices (blend_spec: the one rule set, shared with
Converter.convert_many and both CLIs).  A converter built with blend=S > 1 gives slot b the S list rows b*S .. b*S+S-1: the content
[B, 768, T] is replicated to [B*S, 768, T], the grouped search runs over the list rows' segments (unused rows at seg_len 0) and
alive_knn_blend_gather_rows replaces merge_gather_rows, mixing each slot's list means with the device weights.  Blends, single
voices and weights switch between ticks without a re-capture; blend=1 launches exactly the plain tick.

Per-session k: a converter built with k_max=K (k <= K <= 8) keeps a device array k_rows [B] (a closed slot: the converter's k) and
runs the per-row-k entry points (alive_knn_search_grouped_k, alive_knn_merge_gather_rows_k / alive_knn_blend_gather_rows_k, lists
at stride K): open(..., k=) and set(slot, k=) write one word, so a change of k between ticks never re-captures, and a session at k
comes out bitwise as in a converter whose uniform k is that k.  k is part of the search's group key: sessions on one voice at
different k take one pass over the voice per k.  With blend=S the slot's k is repeated onto its S list rows for the search.
k_max=None (the default) is the uniform converter, launch for launch.

Auto pitch: a converter built with auto_pitch=True keeps, per slot, the target voice's register (`target`, from the pool's voice
registers: VoicePool.register, a blend's weighted mean) and a running estimate of the SOURCE's register, reg_state [B, 2] = (S, W) in
fp64 on the device: on every emitting tick alive_pitch_follow_rows, between the f0 and the transform on the f0 side stream, adds the
ring's voiced pitch (after f0_rate, what the mode-1 transform forms) to S and the voiced count to W, both forgotten at `decay` per tick,
and writes shift_eff = pitch + W / (W + prior) * (target - S / W) for the sessions opened or set with auto_pitch=True, `pitch` bit for
bit for the others; the transform reads shift_eff.  `pitch` thus becomes an offset on top of the automatic shift, which grows smoothly
from 0 as voiced speech arrives (no threshold, no jump).  decay = 2^(-tick / auto_pitch_half_life) (None: never forget) and prior =
auto_pitch_prior seconds of voiced speech * 50 frames/s * buffersize (a frame stays in the ring for buffersize ticks and is counted
every time); the defaults, 10 s and 0.5 s, are design choices, not tuned on data.  The state belongs to the session like phi: open and
close zero it, set(voice=) rewrites the target only (the source has not changed), enable_graph and the bf16 repeat save and restore it.
Everything is device arrays: toggling never re-captures, and a converter built without auto_pitch launches exactly what it did.

Pitch range: a converter built with pitch_range=True carries the second moment too.  reg_state is [B, 3] = (S, W, Q), Q the decayed sum
of squared pitch; alive_pitch_follow2_rows stands where alive_pitch_follow_rows stood and alive_pitch_transform_rows_centred where
alive_pitch_transform_rows stood, captured once.  A session follows when it is on auto_pitch, on auto_range, or at an intonation other
than 1.  With m = S / W, v = Q / W - m^2 and a = W / (W + prior), its frames become p' = m + (p - m) * I_eff + shift_eff, where I_eff =
1 + a * (intonation * r - 1) and r = clamp(target_sd / sqrt(v), 1 / pitch_range_max, pitch_range_max) on an auto_range session (target_sd
from VoicePool.blend_range), 1 otherwise: with auto_pitch beside it, the mean-variance transform of log-f0, grown from the identity with
the evidence.  Half-life and prior are auto pitch's.  A session at intonation=1, auto_range=False is bitwise the session of a plain
converter, an auto_pitch-only session bitwise that of an auto_pitch=True converter, and a converter built without pitch_range launches
exactly what it did.  pitch_range_state() reads the running mean, standard deviation and effective intonation back.

Input gate: a converter built with gate=True decides on the device, every tick, which sessions hear something (csrc/gate.hip).  Right
after the input resample, alive_gate_rows takes the mean square of every 16 kHz ring over the detection window [begin_of_output,
min(ring, end_of_output + gate_lookahead)) -- the chunk about to be emitted plus a lookahead, one chunk's duration by default, a
converter constant because it is baked into the captured launch -- and runs, for the sessions opened or set with gate_db=, a hold state
machine against the session's threshold: gate_state [B, 2] = (hold_left, was_open), like phi the session's own (open and close zero it,
so a gated session's first chunk fades in; enable_graph and the bf16 repeat save and restore it).  Its outputs steer the rest of the
tick: g0 / g1, the gains at the two ends of the emitted chunk, which alive_gate_apply_rows turns into a linear fade (or +0.0, or nothing)
on the final waves; seg_len_eff, the search's segment lengths with a row closed at BOTH ends at 0 -- the grouped search does no work for
it and the merge passes it through; a fading chunk is still searched, so what fades is the converted voice, never the source --;
world_eff, WORLD's row mask without the skipped rows; and follow, which replaces emit for the auto-pitch follower, so a session's
register learns from open ticks only.  The encoders and the decoder still run over all B rows.  gate_db is dBFS of the 16 kHz ring after
the input gain (thr = 10^(dB/10) as a mean square, float64 on the host), gate_hold seconds rounded up to ticks.  Everything is device
arrays: toggling and retuning never re-capture, and a converter built without gate launches exactly what it did.  gate_open() reads
the per-slot open flags of the last tick back; seg_len_eff stays an attribute.

Seam crossfade: every tick re-decodes the whole ring and emits its centre span, so successive chunks are cut from two independent
decodes and butted together.  A converter built with crossfade=True (csrc/seam.hip) blends the head of each emitted chunk with the
previous tick's own continuation: that tick's wave went on for 3.5 chunks beyond what it emitted, and its samples [span_lo + shift,
span_lo + shift + X) are its prediction of what this tick emits as [span_lo, span_lo + X), from the same carried phase (the oscillator
refers theta to begin_of_output).  alive_seam_rows keeps those X samples per session (`tail` [B, widest span], `stored` [B]: how many
are valid) and fades from them into the current decode: no future input is waited for, so no latency is added.  shift is the ring's
advance per tick in the session's own samples, its chunk -- NOT the span length: at 44.1 kHz under 160-sample ticks the chunk is 441
and the span 440, so the time-aligned tail starts at span_lo + 441.  The call sits after the output resample and BEFORE the gate's
edge: the tail is always saved from the un-gated converted wave, and the gate's ramp applies on top of the crossfaded head; a tick
whose search the gate skipped (g0 = g1 = 0) decoded the passed-through source, so it leaves stored = 0 and the chunk on which the gate
reopens is not faded from it.  crossfade_ms is per session (open / set; X = round(ms * rate / 1000) in xlen [B], at most the session's
span); tail and stored are the session's, like phi: open and close zero stored, enable_graph and the bf16 repeat save and restore
both.  It needs input_sr == output_sr (otherwise the ring's advance is not a whole number of output samples).  Everything is device
arrays: toggling and retuning never re-capture, and a converter built without crossfade launches exactly what it did.  seam_db() reads
the latest tick's 10 log10(sum (c - t)^2 / sum c^2) per slot back: how far the two decodes disagree, not how it sounds.

Limiter: every path ends in alive_float_to_pcm16, which keeps the low 16 bits: a sample outside [-1, 1) wraps to the other end of the
scale.  A converter built with limiter=True (csrc/limit.hip) runs alive_limit_rows LAST in the tick, after the seam and the gate's edge,
on what is emitted: for the sessions opened or set with limit_db= (dBFS <= 0; c = min(10^(dB / 20), 32767 / 32768)) the span is
multiplied by g[i], the fp64 mean over k = i - L + 1 .. i of m[k] = min over [k - H, k + L - 1] of the required gains a[j] = c /
max(|y[j]|, c), and clamped to +-c.  Every window that enters g[i] contains i, so no emitted sample exceeds c whatever the neighbours
are; the gain ramps down over L = limit_lookahead_ms, holds for H = limit_hold_ms and ramps back over L.  The lookahead is taken from the
tick's own wave one chunk on (limit_shift: where the next tick's span will come from -- 441 against 440 samples at 44.1 kHz), so no
latency is added; the next tick's decode differs a little from that prediction, so the gain may step a little at a seam -- the bound
does not depend on it.  limit_hist [B, round(limit_history * fastest rate)] holds the required gains of each session's latest emitted
samples (L - 1 + H must fit: limit_geometry names the largest value that does); it is the session's, like phi: open and close set it to
1.0, set keeps it, a tick on which the session's limiter is off sets it to 1.0, enable_graph and the bf16 repeat save and restore it
(with _seam_state).  The seam's saved tail lies beyond the span and stays un-limited; the gate's zeros ask for nothing (the lookahead
lies beyond the span, where the gate's edge does not reach: a muted chunk stays zeros, though limit_db() may report a reduction).  Unlike the
seam it works with input_sr != output_sr (the lookahead is then one tick's advance at output_sr on, never less than the span).
Everything is device arrays: toggling and retuning never re-capture, and a converter built without limiter launches exactly what it
did.  limit_db() reads the latest tick's 20 log10(smallest gain) per slot back (0.0: untouched).  limit_waves is the offline form
(alive_limit_waves), bitwise the streaming one run tick by tick over the same signal.  The defaults (-1 dBFS when asked for, 5 ms,
20 ms) are design choices: with no trained weights, how they sound is unmeasured.

Sparse ticks: a dense converter wants a chunk from every open slot on every tick (step raises otherwise) and keeps the rings on the
host: it uploads every whole ring and downloads every whole wave per tick.  A converter built with sparse=True (csrc/ring.hip) gives
every session its own clock.  step(chunks) takes the chunks of ANY subset of the open slots; an open slot without one is absent this
tick and nothing of it moves: its ring and count, phi, reg_state, gate_state, tail and stored, limit_hist and limit_gmin.  It is not a
key of the result and costs no search (its list rows run at segment length 0, as rows the gate skipped; it is off in WORLD's row mask);
the encoders and the decoder still run over all B rows, and what they compute for an absent row is discarded.  The contract: a
session's emitted stream depends only on the sequence of chunks it supplied, bit for bit -- not on the ticks they arrived in, nor on
what the other sessions did.  An absent tick is a STALL of the session: its latency to the wall clock grows by one tick, no audio is
lost or repeated (no concealment audio is made up for it; a chunk that was LOST and should advance the session's clock is named in step(...,
lost=): see "Lost chunks" below).  step({}), or a tick on which no present slot emits, does no network work; present filling slots still have their chunk pushed.
The rings live on the device, int16 [B, ld_in] in time order (ring_dev; `ring` is None, rings() reads them back): the chunks go up
through one pinned staging buffer [B, longest chunk] in one copy, present and emit in a second small one, and alive_ring_push_rows --
once per tick, OUTSIDE the captured step and outside what the bf16 repeat runs again, so a repeated tick starts from the input it
started from and the ring is pushed once -- advances the present rows in place, rewrites their rows of the float input _in (bitwise
alive_pcm16_to_float of the ring a dense converter would hold) and forms the tick's masked row arrays seg_len_tick / world_tick (seg_len
/ world_on on present rows, 0 on absent ones; after _follow_pool has brought seg_len up to date), which the tick reads where a dense one
reads seg_len / world_on -- with a gate they are alive_gate_rows' inputs, whose emit == 0 branch passes the zeros on.  emit[b] is
"present and past filling", so the kernels that leave a row's state alone at emit == 0 (alive_pitch_follow_rows, alive_gate_rows,
alive_seam_rows, alive_limit_rows) do so for an absent row, and phi_next keeps phi where emit is 0 (a filling slot's phi is 0 anyway).
After the step alive_emit_rows cuts the emitting rows' spans (_span of the slot's chunk: 440 of 441 at 44.1 kHz) into one int16
[B, widest span] array, the only thing copied back.  open and close zero the slot's device ring and its row of _in.  With every session
present every tick a sparse converter emits what the dense one emits, byte for byte; a converter built without sparse launches exactly
what it did, `ring`, _in and the ValueError for a missing slot included.

Envelope follow: the decoder sets the level of every frame from the matched features and f0; nothing carries the speaker's own loudness
across.  A converter built with envelope=True (csrc/envelope.hip) runs alive_envelope_waves right after the decoder, before the output
resample: for the sessions opened or set with envelope=A (the amount, 0 < A <= 1) the decoder's 16 kHz wave y is multiplied by a gain
that moves its smoothed frame level towards that of the 16 kHz ring x the gate also sees, which lies beside it sample for sample:
per 320-sample frame the mean squares of x and y over 2 R + 1 frames, rc = sqrt((Px / Cn + e) / (Py / Cn + e)) kept inside
+-envelope_range_db, G = 1 + A (rc - 1), interpolated linearly between the frame centres -- all in fp64 in a fixed order
(tools/envelope_ref.py restates it bit for bit).  The tick re-decodes the whole ring, so the envelope is a stateless function of two
rows: nothing is carried across ticks, the bf16 repeat or a capture, and a row that sat a tick out is recomputed from its unchanged
ring.  The result goes to a buffer allocated once (the captured graph replays into the same memory); the seam, the gate's edge and the
limiter sit downstream and see the enveloped wave.  The amounts are a device array: toggling and retuning never re-capture, a converter
built without envelope launches exactly what it did, and one whose sessions are all at 0 emits byte-identical streams.  The frame grid
is ring-relative, as the decoder's own frames are: with chunks that are no multiple of 320 samples at 16 kHz it moves against the signal
from tick to tick, so two successive decodes get slightly different gains at a seam -- smoothed over 2 R + 1 frames, interpolated, and
faded by crossfade.  The gain can lift a sample above 1.0: use the limiter beside it.  envelope_db() reads the latest tick's smallest
and largest frame gain per slot back.  follow_envelope is the offline form (the same call over whole utterances).  The defaults (R = 1:
60 ms, floor -60 dB, range 12 dB) are design choices: with no trained weights, how they sound is unmeasured.

Post filter: every stage behind the decoder shapes the level of the converted wave; none shapes its spectrum, and a kNN match that
averages k library rows flattens formants.  A converter built with post_filter=True (csrc/postfilter.hip) runs alive_postfilter_waves
right after the decoder and before the envelope follow, which so sets the level of the filtered wave: for the sessions opened or set
with post_filter=A (0 < A <= 0.85; 0.8 is the classic setting) each 320-sample frame of the decoder's 16 kHz wave gets an LPC analysis
(40 ms Hamming window on the int16 grid, order 16, Levinson-Durbin in fp64), the filter A(z / (A ratio)) / A(z / A) with a first-order
tilt compensation as a 128-tap response, and a frame gain that restores the frame's level; between the frame centres the output moves
linearly from one frame's filtered wave to the next's (tools/postfilter_ref.py restates it bit for bit).  Like the envelope follow it
is a stateless function of the tick's wave: nothing is carried across ticks, the bf16 repeat or a capture, the result goes to a buffer
allocated once, the alphas are a device array (toggling and retuning never re-capture), a converter built without it launches exactly
what it did and one whose sessions are all at 0 emits byte-identical streams.  Its frame grid is ring-relative too, exactly as the
envelope follow's: with chunks that are no multiple of 320 samples two successive decodes analyse slightly different frames at a seam.
post_filter_db() reads the latest tick's smallest and largest frame gain per slot back; post_filter is the offline form.  With no trained
weights, what the filter does to perceived quality is unmeasured.

Lost chunks: a stall costs nothing, but a server meets another event more often: a chunk that never arrives while the session's clock
must go on.  Pushing zeros for it puts 10 ms of digital silence with two hard edges into voiced speech, and the hole is re-encoded on
every one of the buffersize ticks it spends in the ring.  A sparse converter built with conceal=True (csrc/conceal.hip) fills the hole
at the input edge instead, by waveform substitution in the style of G.711 Appendix I: step(chunks, lost=[slots]) names the open slots
whose chunk did not arrive; their clock advances exactly as if a chunk had been supplied (count, ring, phase, emission; they are keys of
the result).  alive_conceal_rows, launched in front of alive_ring_push_rows on the same stream -- outside the captured step and outside
what the bf16 repeat runs again -- writes the made-up chunk into the uploaded chunk buffer and the push moves it into the ring: at the
first lost chunk of a run it finds the pitch period P in the ring's newest samples (lags of 60 - 400 Hz, normalised correlation over
20 ms in exact integer sums, the lowest lag on a tie) and keeps the last period as the run's template, its last quarter faded into the
period before; every lost chunk repeats the template at full level for conceal_hold_ms and then fades it to exact zeros over
conceal_fade_ms (the ring, which by then holds made-up samples, is never searched again during the run); the first chunk that arrives
again has its first conceal_recover_ms faded in from the continuation.  The state is the session's: _conceal_state [B, 2] = (samples
made up so far in this run, P) and conceal_tmpl; open and close clear it, an absent tick leaves it standing.  The networks see a
plausible continuation and nothing after the push changes.  A session opened or set with conceal=False that loses a chunk gets zeros.
The host mirrors which slots are in a run: a tick with no lost and no recovering slot launches exactly what it did, and a converter
built without conceal allocates nothing new, launches exactly what it did and refuses lost=.  A session needs a ring of at least max(W +
Lmax, 2 Lmax) samples (587 at 16 kHz: -c 160 -b 4 just fits).  Everything is device arrays: toggling never re-captures.
conceal_state() reads the per-slot (run samples, period) back.  tools/conceal_ref.py restates the arithmetic bit for bit.  The defaults
(10 ms, 50 ms, 5 ms) are design choices: with no trained weights, what this does to perceived quality is unmeasured.  Concealment audio
for a STALL, concealing in feature space, jitter buffers and a voicing decision (the best lag is always used) are not part of it.

Pitch tracking: the estimator's f0 is an independent argmax per frame, so one frame whose octave partner scores a little higher sends
the oscillator up an octave for 20 ms.  A converter built with pitch_track=True (csrc/f0_track.hip) has the f0 branch store the
estimator's class scores (F0Estimator.logits, into a buffer allocated once per shape), take their argmax as before and, for the sessions
opened or set with pitch_track=True, overwrite the row with the Viterbi path over its scores: states are the classes track_lo ..
track_hi, a move costs track_weight per semitone inside track_band semitones and track_jump flat otherwise, in fp64 in the units of the
scores (tools/pitch_track_ref.py restates it bit for bit).  It runs before the WORLD select, the followers and the transform: auto pitch
and pitch range learn from the tracked contour.  The ring is decoded again every tick and the emitted chunk lies 3.5 chunks inside it,
so the tracker is a stateless fixed-lag smoother: nothing is carried across ticks, the bf16 repeat or a capture, and a row that sat a
tick out is decoded again from its unchanged ring.  on, weight and jump are device arrays: toggling and retuning never re-capture, a
converter built without pitch_track allocates nothing, launches exactly what it did and refuses pitch_track=True; not together with
world_pitch on one session.  Class 0 is not a state: a tracked row never emits f0 = 0.  pitch_track_changed() reads back how many
frames of each ring the tracker moved.  The defaults (1.0, 12.0, 2.0 semitones, 50 .. 1100 Hz) are design choices in logit units: with
no trained weights, what tracking does to perceived quality is unmeasured.

Voicing: the estimator's argmax never says "unvoiced" (class 0 is not trained), so the oscillator drives its harmonics through every
breath, fricative and pause, and the followers learn a register from them.  A converter built with voicing=True (csrc/voicing.hip)
has the f0 branch run a periodicity detector of its own on the 16 kHz ring, after the estimator or the tracker and before the WORLD
select, the followers and the transform: per frame the best normalised cross-correlation r over the lags of voicing_lo .. voicing_hi Hz
in a window of voicing_window_ms, on samples quantised to the int16 grid so that every sum is an exact integer (tools/voicing_ref.py
restates it bit for bit); per row a hysteresis between the session's voicing_on and voicing_off, a silence floor voicing_floor_db,
gaps of at most voicing_bridge frames bridged and runs under voicing_min_run frames dropped; the f0 of every other frame becomes 0,
which everything downstream already reads as unvoiced.  Sessions opened or set with voicing=True decide; toggling and retuning never
re-capture.  The detector is stateless over the ring, like the tracker: nothing is carried across ticks, the bf16 repeat or a capture.
A converter built without voicing allocates nothing, launches exactly what it did and refuses voicing=True; not together with
world_pitch on one session (WORLD decides for itself).  voicing_state() reads back, per slot, the voiced frames of the ring, the
frames set to 0 and r of the emitted centre frame.  The defaults (0.6, 0.45, -60 dB, 50 .. 500 Hz, 40 ms, 1, 2) are design choices:
with no trained weights, what the decision does to perceived quality is unmeasured.

Match path: every frame is matched on its own, and the mean of its k nearest rows is all the continuity the match has -- none at the
k = 1 or 2 that a small voice or a codebook wants.  A converter built with match_path=True (csrc/match_path.hip) always runs the
per-row-k entry points (k_max defaults to k) and puts ONE call between the grouped search and the gather: for the sessions opened or
set with match_path=True it chooses, out of each frame's k candidates, one row per frame by a Viterbi path over the ring's frames --
a candidate costs its cosine below the frame's best one, a step earns path_weight times the cosine between the two chosen rows, in
fp64 (tools/match_path_ref.py restates it bit for bit) -- and the gather reads gather_k, 1 on those slots and the slot's k on the
others, beside k_rows.  A blend's lists each take their own path.  path_weight = 0 is the k = 1 match.  The call is stateless over
the ring, like the tracker: nothing is carried across ticks, the bf16 repeat or a capture; a gated row has no match and passes
through, and a sparse converter's row that sits a tick out keeps its count.  on and weight are device arrays: toggling and retuning
never re-capture; a converter built without match_path allocates nothing, launches exactly what it did and refuses match_path=True.
path_moved() reads back how many frames of each ring the path moved off the nearest row.  The default weight (1.0, in cosine units)
is a design choice: with no trained weights, what the path does to perceived quality is unmeasured.

Loudness: every path leaves the converted voice at the level of the library rows it selected.  measure_loudness / normalize_loudness
(csrc/loudness.hip) are the integrated loudness of ITU-R BS.1770-4 / EBU R 128 for one channel -- K-weighting, 400-ms blocks every 100
ms, the absolute gate at -70 LUFS and the relative one 10 LU below the gated mean -- and the one gain per row that brings it to a
target, within +-max_gain_db; rows at mixed rates go through one call.  The K-weighting recurrence runs in tiles of one 100-ms
sub-block, every tile an independent lane run twice, with one short serial carry per row in between (include/alive_vc.h).  A converter
built with loudness=True runs alive_loudness_rows in the tick AFTER the gate's edge and BEFORE the limiter, on what is emitted: for the
sessions opened or set with lufs=L the span goes through the session's K-weighting filter at its own output rate into a running
loudness -- per completed 400-ms block z, S = S d + z and W = W d + 1 with d = 2^(-0.1 / loudness_half_life), for the blocks above the
absolute gate and, once the mean is trusted (W >= P = 10 loudness_prior), above S / W - 10 LU: a talker who drops by more than 10 LU is
taken for a pause until W has decayed below the prior, then believed -- and is multiplied by a gain that ramps linearly over the span
from the previous tick's to G = 1 + min(W / P, 1) (r - 1), r = sqrt(z_t W / S) within +-loudness_max_db, moved by at most
loudness_slew_db dB per second.  The state (loud_state [B, 16]: the filter's, the open sub-block, the last three sub-blocks, S, W and
the gain) is the session's, like phi: open and close start it over, set keeps it, a tick on which the session's lufs is off starts it
over, a row that does not emit (filling, stalled) leaves it standing, enable_graph and the bf16 repeat save and restore it (with
_seam_state).  Everything is device arrays: toggling and retuning never re-capture; a converter built without loudness allocates
nothing, launches exactly what it did and refuses lufs=.  It works with input_sr != output_sr and with per-session rates (the filter
and the sub-block are the session's own rate's).  loudness() reads the running loudness and the gain per slot back.  The gain can lift
a sample above full scale: use the limiter beside it.  tools/loudness_ref.py restates everything bit for bit.  The defaults (half-life
3 s, prior 1 s, gate -70 LUFS, +-12 dB, 6 dB/s) are design choices, not tuned: with no trained weights, how they sound is unmeasured.
"""
import functools
import math

import numpy as np
import torch

from . import _native as nat
from . import audio_io, common, ops
from .common import DIM, compute_f0_rows
from .pipeline import prepare_networks
from .realtime import capture_step, f0_on_side_stream, fp16_guarded, ring_geometry, track_logits_buf
from .spectrogram import spectrogram

MAX_K = 8          # the grouped search keeps one register pair per lane and frame (csrc/knn.hip)
MAX_BLEND = 4      # voices one blend may mix: lists per output row of alive_knn_blend_gather_rows (ALIVE_MAX_BLEND)
MAX_ROWS = 1024    # rows of one grouped search (streaming: slots * blend)
# the pool search's limits (alive_knn_search_pool: N <= 4096, N * T <= 2^20): convert_many searches the list rows of a blended
# corpus in consecutive pieces within them -- the results are per frame, so the pieces are bitwise one call
POOL_PIECE_ROWS, POOL_PIECE_FRAMES = 4096, 1 << 20
_ws = nat.Workspace()


def blend_spec(voice, pool=None, k=None, limit=MAX_BLEND):
    """A voice or a blend -> (names, weights): the ONE place that checks and normalises a blend (both conversion paths and both
    CLIs call it).  `voice` is a name (the blend {name: 1.0}), a {name: weight} dict or a sequence of (name, weight) pairs: 1 to
    `limit` (<= MAX_BLEND) distinct names, weights finite, > 0 and not bool, normalised in float64 as w_s / sum(w) in the caller's
    order (a single voice gets exactly 1.0).  With a pool, every name must be one of its voices with at least k vectors."""
    if isinstance(voice, str):
        items = [(voice, 1.0)]
    elif isinstance(voice, dict):
        items = list(voice.items())
    elif isinstance(voice, (list, tuple)):
        items = []
        for c in voice:
            if not isinstance(c, (list, tuple)) or len(c) != 2:
                raise ValueError(f"a blend component is a (voice, weight) pair, got {c!r}")
            items.append(tuple(c))
    else:
        raise ValueError(f"a voice is a name, a {{name: weight}} dict or (name, weight) pairs, got {voice!r}")
    limit = min(int(limit), MAX_BLEND)
    if not items:
        raise ValueError("a blend needs at least one voice")
    if len(items) > limit:
        raise ValueError(f"a blend of {len(items)} voices: at most {limit} (MAX_BLEND = {MAX_BLEND})")
    names, weights = [], []
    for name, w in items:
        if name in names:
            raise ValueError(f"voice {name!r} appears twice in one blend")
        if isinstance(w, (bool, np.bool_)) or not isinstance(w, (int, float, np.integer, np.floating)):
            raise ValueError(f"blend weight of {name!r} must be a number, got {w!r}")
        w = float(w)
        if not np.isfinite(w) or w <= 0:
            raise ValueError(f"blend weight of {name!r} must be finite and > 0, got {w!r}")
        if pool is not None:
            m = pool.segment(name)[1]
            if k is not None and m < k:
                raise ValueError(f"voice {name!r} has {m} vectors, fewer than k={k}")
        names.append(name)
        weights.append(w)
    total = 0.0
    for w in weights:
        total += w
    return tuple(names), tuple(w / total for w in weights)


def blend_sources(entry, where, rel):
    """the "blend" key of a jobs / sessions file entry -> [(target, lib, weight), ...]: each component is a voice source like an
    entry's own "target" / "lib" (paths through `rel`) with a "weight", checked by blend_spec (the sources are the names);
    ValueError on a malformed blend, before any device work"""
    if entry.get("target") is not None or entry.get("lib") is not None:
        raise ValueError(f"{where}: \"blend\" excludes a top-level \"target\" / \"lib\"")
    comps = entry["blend"]
    if not isinstance(comps, list) or not comps:
        raise ValueError(f"{where}: \"blend\" must be a non-empty list of {{\"target\" / \"lib\", \"weight\"}} objects")
    out = []
    for i, c in enumerate(comps):
        if not isinstance(c, dict):
            raise ValueError(f"{where}: blend component {i} must be an object, got {c!r}")
        unknown = set(c) - {"target", "lib", "weight"}
        if unknown:
            raise ValueError(f"{where}: blend component {i}: unknown keys {sorted(unknown)} (known: target, lib, weight)")
        if c.get("target") is None and c.get("lib") is None:
            raise ValueError(f"{where}: blend component {i} needs a \"target\" wav and / or a \"lib\" voice library")
        if "weight" not in c:
            raise ValueError(f"{where}: blend component {i} has no \"weight\"")
        out.append((rel(c.get("target")), rel(c.get("lib")), c["weight"]))
    try:
        blend_spec([((t, lb), w) for t, lb, w in out])
    except ValueError as e:
        raise ValueError(f"{where}: {e}") from None
    return out


def pitch_hz(hz):
    """the pitch 12 log2(hz / 440) - 9 of a frequency as the kernels form it (the quotient in float32, log2 in float64 rounded once to
    float32, the rest in float32), as a host float"""
    x = np.float32(hz) / np.float32(440.0)
    return float(np.float32(12.0) * np.float32(np.log2(np.float64(x))) - np.float32(9.0))


def _tokens_2d(tokens):
    t = tokens
    if t.dim() == 3:
        if t.shape[0] != 1:
            raise ValueError(f"a voice must be [768, M] or [1, 768, M], got {tuple(t.shape)}")
        t = t[0]
    if t.dim() != 2 or t.shape[0] != DIM:
        raise ValueError(f"a voice must be [768, M] or [1, 768, M], got {tuple(tokens.shape)}")
    return t


class RowAllocator:
    """The host side of a reserved pool: named segments [lo, lo + n) of `capacity` rows.  Plain Python, no device.

    The only state is the segment map; holes are derived from it (the gaps between the segments in address order, the space after
    the highest one last), so a freed segment is coalesced with its neighbours by construction and there is no free list to keep
    in step.  Placement is first-fit in address order.  Every method either succeeds or raises and leaves the map as it was.

    `layout` counts the operations that changed some EXISTING segment's (lo, n): extend (in place or moved) and a compact that moved
    something; add and remove do not.  `hold` / `release` count the users of a segment by label; a held segment cannot be removed."""

    def __init__(self, capacity):
        if isinstance(capacity, bool) or not isinstance(capacity, (int, np.integer)) or not 1 <= capacity < 2 ** 31:
            raise ValueError(f"a reserved pool holds 1 <= capacity < 2^31 rows (got {capacity!r})")
        self.capacity = int(capacity)
        self.segments = {}
        self.layout = 0
        self.holds = {}

    def holes(self):
        """the free ranges [(lo, n), ...] in address order"""
        out, at = [], 0
        for lo, n in sorted(self.segments.values()):
            if lo > at:
                out.append((at, lo - at))
            at = lo + n
        if at < self.capacity:
            out.append((at, self.capacity - at))
        return out

    @property
    def free_rows(self):
        return self.capacity - sum(n for _, n in self.segments.values())

    @property
    def largest_hole(self):
        return max([n for _, n in self.holes()] or [0])

    def _fit(self, n, what):
        for lo, size in self.holes():
            if size >= n:
                return lo
        raise ValueError(f"{what}: needs {n} rows, the pool of {self.capacity} has {self.free_rows} free and its largest hole is "
                         f"{self.largest_hole}" + (": compact() would make room" if n <= self.free_rows else ": the pool is too small"))

    def add(self, name, n):
        """place a new segment of n rows in the first hole that fits -> its first row"""
        if name in self.segments:
            raise ValueError(f"voice {name!r} is already in the pool")
        if n < 1:
            raise ValueError(f"voice {name!r} is empty")
        lo = self._fit(n, f"voice {name!r}")
        self.segments[name] = (lo, n)
        return lo

    def remove(self, name):
        if name not in self.segments:
            raise ValueError(f"unknown voice {name!r} (the pool holds {sorted(self.segments)})")
        users = self.holds.get(name)
        if users:
            raise ValueError(f"voice {name!r} is in use by {', '.join(f'{w} ({c} hold(s))' for w, c in users.items())}: close or "
                             "re-voice those sessions first")
        return self.segments.pop(name)

    def hold(self, name, who):
        """count `who` (a label: a converter) as a user of the segment"""
        if name not in self.segments:
            raise ValueError(f"unknown voice {name!r} (the pool holds {sorted(self.segments)})")
        users = self.holds.setdefault(name, {})
        users[who] = users.get(who, 0) + 1

    def release(self, name, who):
        users = self.holds.get(name, {})
        if users.get(who, 0) < 1:
            raise ValueError(f"{who} holds no voice {name!r}")
        users[who] -= 1
        if users[who] == 0:
            del users[who]
        if not users:
            del self.holds[name]

    def extend(self, name, extra):
        """grow a segment by `extra` rows -> (old_lo, old_n, new_lo): in place (new_lo == old_lo) when the hole behind it is large
        enough, else in the first hole that takes the old and the new rows together (the old segment is freed; the caller copies
        its rows from old_lo to new_lo, two disjoint ranges)"""
        if name not in self.segments:
            raise ValueError(f"unknown voice {name!r} (the pool holds {sorted(self.segments)})")
        if extra < 1:
            raise ValueError(f"voice {name!r}: nothing to append")
        lo, n = self.segments[name]
        end = lo + n
        behind = min([l for l, _ in self.segments.values() if l >= end] or [self.capacity]) - end
        new_lo = lo if behind >= extra else self._fit(n + extra, f"voice {name!r} (growing from {n} rows by {extra})")
        self.segments[name] = (new_lo, n + extra)
        self.layout += 1
        return lo, n, new_lo

    def undo_extend(self, name, lo, n):
        """take back the latest extend of `name` (its new rows were refused)"""
        self.segments[name] = (lo, n)
        self.layout -= 1

    def compact(self):
        """slide every segment down, in address order, until no hole remains between segments -> the moves [(name, src, dst, n),
        ...] in the order in which they must be made (each destination is free or part of its own source by then; src - dst < n
        means the two ranges overlap)"""
        moves, at = [], 0
        for name, (lo, n) in sorted(self.segments.items(), key=lambda kv: kv[1]):
            if lo != at:
                moves.append((name, lo, at, n))
                self.segments[name] = (at, n)
            at += n
        self.layout += bool(moves)
        return moves


def _token_parts(tokens):
    """a voice's tokens -> the list of its [768, m] parts (a tensor, or a sequence of tensors appended in order)"""
    parts = [_tokens_2d(t) for t in (tokens if isinstance(tokens, (list, tuple)) else [tokens])]
    parts = [t for t in parts if t.shape[1] > 0]
    return parts, sum(int(t.shape[1]) for t in parts)


class Register(tuple):
    """a measured register (sum of voiced pitch, voiced frames) that also carries the sum of squared pitch as `.sumsq`: it compares
    and unpacks as the 2-tuple it always was, and VoicePool.add / extend / set_register read the third sum from it"""
    def __new__(cls, s, c, sumsq):
        self = super().__new__(cls, (s, c))
        self.sumsq = sumsq
        return self

    def __getnewargs__(self):              # (pickle and copy rebuild it through __new__)
        return self[0], self[1], self.sumsq


POOL_DTYPES = {"fp32": torch.float32, "fp16": torch.float16}     # (the names of --pool-dtype)


def pool_dtype(dtype):
    """the element type of a pool's row table: torch.float32 or torch.float16 (or their names "fp32" / "fp16"); ValueError otherwise"""
    dtype = POOL_DTYPES.get(dtype, dtype) if isinstance(dtype, str) else dtype
    if dtype not in (torch.float32, torch.float16):
        raise ValueError(f"a voice pool stores torch.float32 or torch.float16 rows, got dtype={dtype!r}")
    return dtype


def _rows_call(name, rows):
    """the entry point `name` for a row table of rows.dtype: itself for fp32, its _f16 twin for fp16; ValueError for any other dtype"""
    if rows.dtype == torch.float32:
        return getattr(nat.lib(), name), name
    if rows.dtype == torch.float16:
        return getattr(nat.lib(), name + "_f16"), name + "_f16"
    raise ValueError(f"{name}: the row table must be torch.float32 or torch.float16, got {rows.dtype}")


class VoicePool:
    """Named voices tokens[768, M] packed into one fp32 row table rows[P, 768] with norms[P] (the norms bitwise those of
    PackedLibrary) and a name -> (seg_lo, M) map.

    Default pool (capacity=None): `add` re-packs the pool (a new row table): allowed between ticks, and a MultiStreamConverter
    that replays a captured step re-captures on its next tick.

    Reserved pool (capacity=ROWS): rows[ROWS, 768] and norms[ROWS] are allocated once and never replaced (P == ROWS, `version`
    stays put), so a captured tick keeps serving while voices are enrolled (`add`), grow (`extend`), go (`remove`) and are packed
    together (`compact`).  Where each voice lies is decided by a RowAllocator; the device work is alive_pool_append (the new rows
    only, with their norms checked on the device: the host reads two words, never the norms) and alive_pool_move_rows.  `tokens`
    may be strided (a slice or an every-4th-frame view of an encoder output goes in without a copy) and, for `add` and `extend`, a
    sequence of such parts.  `layout` counts the operations that changed some EXISTING voice's (seg_lo, seg_len): a converter
    rewrites its segment arrays when it moved on.  `hold` / `release` count the users of a voice; a held voice cannot be removed.

    Stream order: every operation runs on the CURRENT stream of the calling thread (torch.cuda.current_stream()) and records an
    event there; neither allocates table-sized memory nor waits for the device, except that `add` / `extend` read the two-word
    report back.  MultiStreamConverter makes the stream it replays the tick on wait for that event, so an operation issued between
    two ticks is ordered before the next tick whatever stream it ran on; `step` returns after its tick has completed (it copies
    the PCM to the host), so an operation issued between two ticks never overtakes the tick before it either.

    Registers (auto pitch): a voice may carry the register of its speaker as host floats (sum of voiced pitch, voiced frames) in the
    unit of pitch_stats_groups; `register(name)` is their quotient, the mean pitch.  `add` sets it, `extend` merges by adding sums
    and counts, `set_register` declares one (a voice without audio, such as a voice library); it goes with its voice -- `remove`
    drops it with the voice, and no operation on the pool (re-packing, moves, compact, another voice's removal) loses or changes
    the register of a voice that stays.

    Ranges (pitch range): beside its register a voice may carry the sum of its squared voiced pitch (`ranges`), from which
    `pitch_range(name)` is the standard deviation in semitones.  A register given as (sum, count, sumsq) -- or as the Register that
    measure_register returns -- carries it, a 2-tuple does not; a voice keeps a range only while every piece merged into its
    register brought one.  It travels and goes with the register.

    Half pool (dtype=torch.float16, either kind): `rows` is fp16 [P, 768] -- 1536 bytes per row (`row_bytes`) instead of 3072 -- and
    `norms` stays fp32.  Every token element is rounded to fp16 on the way in (alive_pool_append_f16: round to nearest even; a row
    with an element beyond fp16's range, or one that rounds to all zeros, is refused like any row without a usable norm), and the
    norms are those of the rounded rows.  fp16 -> fp32 is exact and the kernels widen in registers, so the streaming search, the
    gathers and the match path on a half pool are bitwise what they are on an fp32 pool of `tokens.half().float()`.  `tokens(name)`
    returns the rounded tokens as fp32.  The offline pool search (`search_images`, `voice_ids`: Converter.convert_many) rescans fp32
    rows and refuses a half pool."""

    def __init__(self, voices=None, device="cuda", capacity=None, registers=None, dtype=torch.float32):
        self.device = torch.device(device)
        self.dtype = pool_dtype(dtype)
        self.segments = {}
        self.registers = {}                    # name -> (sum of voiced pitch, voiced frames), host floats
        self.ranges = {}                       # name -> sum of squared voiced pitch, for the voices that carry a second moment
        self.version = 0
        self.capacity = None
        self._images = None
        if capacity is not None:
            self._alloc = RowAllocator(capacity)
            self.capacity = self.P = self._alloc.capacity
            self.segments = self._alloc.segments
            self.rows = torch.empty(self.P, DIM, dtype=self.dtype, device=self.device)
            self.norms = torch.empty(self.P, dtype=torch.float32, device=self.device)
            self._report = torch.zeros(2, dtype=torch.int32, device=self.device)
            self.mutations = 0                 # every operation; `order` is the event recorded after the latest one
            self.order = None
            for name, tok in (voices or {}).items():
                self.add(str(name), tok, (registers or {}).get(name))
            return
        self._tokens = {}
        self.rows = self.norms = None
        self.P = 0
        if self.dtype == torch.float16:                        # (a default half pool packs through the half append)
            self._report = torch.zeros(2, dtype=torch.int32, device=self.device)
        if voices:
            for name, tok in voices.items():
                self._tokens[str(name)] = _tokens_2d(tok).to(self.device, torch.float32).contiguous()
            self._pack()
            for name, reg in (registers or {}).items():
                self.set_register(str(name), register=reg)

    @property
    def row_bytes(self):
        """bytes one row of the table takes: 3072 (fp32) or 1536 (fp16)"""
        return DIM * self.rows.element_size() if self.rows is not None else DIM * torch.empty(0, dtype=self.dtype).element_size()

    def _need_f32(self, what):
        if self.dtype != torch.float32:
            raise ValueError(f"{what} needs an fp32 voice pool and this one stores {self.dtype} rows: the offline pool search rescans "
                             "fp32 rows (a half pool serves MultiStreamConverter)")

    # ------------------------------------------------------------------ registers (auto pitch)
    @staticmethod
    def _check_register(name, register):
        """-> (sum, count) or (sum, count, sumsq) as floats"""
        try:
            vals = tuple(float(v) for v in register)
            if isinstance(register, Register):
                vals += (float(register.sumsq),)
            if len(vals) not in (2, 3):
                raise ValueError
        except (TypeError, ValueError):
            raise ValueError(f"voice {name!r}: a register is (sum of voiced pitch, voiced frames), got {register!r}") from None
        s, c = vals[:2]
        if not (np.isfinite(s) and np.isfinite(c) and c >= 0):
            raise ValueError(f"voice {name!r}: a register needs a finite sum and a finite count >= 0, got {register!r}")
        if len(vals) == 3 and not (np.isfinite(vals[2]) and vals[2] >= 0):
            raise ValueError(f"voice {name!r}: a register's sum of squares must be finite and >= 0, got {register!r}")
        return vals

    def _merge_register(self, name, register):
        """add a checked (sum, count[, sumsq]) to the voice's register (None: nothing).  The voice carries a range afterwards only
        if the piece brought a sum of squares and what the voice had before (if anything) did too"""
        if register is not None:
            s0, c0 = self.registers.get(name, (0.0, 0.0))
            had = name in self.registers
            self.registers[name] = (s0 + register[0], c0 + register[1])
            if len(register) == 3 and (not had or name in self.ranges):
                self.ranges[name] = self.ranges.get(name, 0.0) + register[2]
            else:
                self.ranges.pop(name, None)

    def set_register(self, name, hz=None, register=None, range_st=None):
        """declare the voice's register: its mean f0 in Hz (stored as one voiced frame at pitch_hz(hz)), or a measured
        (sum of voiced pitch, voiced frames) as pitch_stats_groups returns it -- or (sum, count, sumsq) as pitch_stats2_groups does;
        both None: the voice has none any more.  range_st (with hz=, or alone on a voice that has a register): the standard
        deviation of its pitch in semitones, stored as the sum of squares count * (mean^2 + range_st^2)"""
        self.segment(name)
        if hz is not None and register is not None:
            raise ValueError(f"voice {name!r}: set_register takes hz= or register=, not both")
        if range_st is not None:
            if isinstance(range_st, (bool, np.bool_)) or not isinstance(range_st, (int, float, np.integer, np.floating)) or not (
                    np.isfinite(range_st) and range_st > 0):
                raise ValueError(f"voice {name!r}: range_st={range_st!r} must be a finite number of semitones > 0")
            if register is not None:
                raise ValueError(f"voice {name!r}: set_register takes range_st= with hz= or alone, not with register=")
            if hz is None:
                if self.register(name) is None:
                    raise ValueError(f"voice {name!r}: range_st= needs hz= or a voice that has a register")
                s, c = self.registers[name]
                self.ranges[name] = c * ((s / c) * (s / c) + float(range_st) * float(range_st))
                return self
        if hz is not None:
            if isinstance(hz, (bool, np.bool_)) or not isinstance(hz, (int, float, np.integer, np.floating)) or not (
                    np.isfinite(hz) and hz > 0):
                raise ValueError(f"voice {name!r}: register hz={hz!r} must be a finite number > 0")
            register = (pitch_hz(hz), 1.0)
            if range_st is not None:
                register += (register[0] * register[0] + float(range_st) * float(range_st),)
        if register is not None:
            register = self._check_register(name, register)   # (raises before the voice's own is touched)
        self.registers.pop(name, None)
        self.ranges.pop(name, None)
        self._merge_register(name, register)
        return self

    def register(self, name):
        """the voice's mean pitch (12 log2(f0 / 440) - 9 averaged over its voiced frames, a float), or None if it carries none"""
        self.segment(name)
        s, c = self.registers.get(name, (0.0, 0.0))
        return s / c if c > 0 else None

    def blend_register(self, names, weights):
        """the target register of a voice or blend (blend_spec's names and float64-normalised weights, in the caller's order): the
        weighted mean of the voices' registers; ValueError naming the first voice that has none"""
        total = 0.0
        for n, w in zip(names, weights):
            r = self.register(n)
            if r is None:
                raise ValueError(f"auto pitch: voice {n!r} has no register: enrol it with f0_estimator=, pass register= to add / "
                                 "extend, or declare one with set_register")
            total += w * r
        return total

    def pitch_range(self, name):
        """the standard deviation of the voice's pitch in semitones (a float; 0.0 when its second moment leaves no variance), or
        None if it carries no second moment"""
        self.segment(name)
        s, c = self.registers.get(name, (0.0, 0.0))
        if not c > 0 or name not in self.ranges:
            return None
        m = s / c
        v = self.ranges[name] / c - m * m
        return float(np.sqrt(v)) if v > 0 else 0.0

    def blend_range(self, names, weights):
        """the target range of a voice or blend (blend_spec's names and weights): the weighted mean of the voices' standard
        deviations; ValueError naming the first voice that has none"""
        total = 0.0
        for n, w in zip(names, weights):
            r = self.pitch_range(n)
            if r is None:
                raise ValueError(f"auto range: voice {n!r} has no pitch range: enrol it with f0_estimator=, pass register=(sum, count, "
                                 "sumsq) to add / extend, or declare one with set_register(..., range_st=)")
            total += w * r
        return total

    def add(self, name, tokens, register=None):
        if register is not None:
            register = self._check_register(name, register)
        if self.capacity is not None:
            parts, m = _token_parts(tokens)
            lo = self._alloc.add(str(name), m)                # first fit; raises (rows needed, free rows, largest hole) if none
            try:
                self._append(lo, parts)
            except Exception:
                self._alloc.remove(str(name))
                raise
            self._merge_register(str(name), register)
            self._changed()
            return self
        self._tokens[str(name)] = _tokens_2d(tokens).to(self.device, torch.float32).contiguous()
        self._pack()
        self.registers.pop(str(name), None)                   # (a voice added again under its name: the new speaker's)
        self.ranges.pop(str(name), None)
        self._merge_register(str(name), register)
        return self

    # ------------------------------------------------------------------ reserved pool
    def _reserved(self, what):
        if self.capacity is None:
            raise ValueError(f"VoicePool.{what} needs a reserved pool: VoicePool(..., capacity=ROWS)")

    def _changed(self):
        self.mutations += 1
        self._images = None
        self.order = torch.cuda.Event()
        self.order.record(torch.cuda.current_stream(self.device))

    def _append(self, at, parts):
        """pack the parts at consecutive rows from `at` (the rows are the caller's to write); ValueError if a new row's norm is zero
        or not finite -- read from the device's two-word report, not from the norms"""
        for t in parts:
            m = int(t.shape[1])
            self._append_into(self.rows, self.norms, self.P, at, t)
            at += m

    def _append_into(self, rows, norms, P, at, t):
        """one part t [768, m] packed at rows [at, at + m) of a table of this pool's dtype (alive_pool_append / _f16)"""
        if t.device != self.device or t.dtype != torch.float32:
            t = t.to(self.device, torch.float32)
        half = self.dtype == torch.float16
        name = "alive_pool_append_f16" if half else "alive_pool_append"
        nat.check(getattr(nat.lib(), name)(t.data_ptr(), t.stride(0), t.stride(1), int(t.shape[1]), DIM, nat.ptr(rows), nat.ptr(norms),
                                           P, at, nat.ptr(self._report), nat.stream()), name)
        bad, first = self._report.tolist()
        if bad:
            raise ValueError(f"voice pool row {first} has zero or non-finite norm ({bad} such row(s) among the new ones): "
                             "remove it" + (" (as fp16: an element beyond 65504 is inf, a tiny row rounds to zero)" if half else ""))

    def _move(self, src, dst, n):
        name = "alive_pool_move_rows_f16" if self.dtype == torch.float16 else "alive_pool_move_rows"
        nat.check(getattr(nat.lib(), name)(nat.ptr(self.rows), nat.ptr(self.norms), self.P, src, dst, n, nat.stream()), name)

    def extend(self, name, tokens, register=None):
        """append rows to a live voice (old rows first): in place when the hole behind it is large enough, else the voice moves to
        the first hole that takes the old and the new rows together.  register: the new audio's (sum, count), added to the voice's"""
        self._reserved("extend")
        if register is not None:
            register = self._check_register(name, register)
        parts, extra = _token_parts(tokens)
        lo, n, new_lo = self._alloc.extend(name, extra)
        try:
            self._append(new_lo + n, parts)                   # the new rows first: refused rows leave the voice as it was
        except Exception:
            self._alloc.undo_extend(name, lo, n)
            raise
        if new_lo != lo:
            self._move(lo, new_lo, n)                         # (two disjoint ranges: the new hole was free)
        self._merge_register(name, register)
        self._changed()
        return self

    def remove(self, name):
        self._reserved("remove")
        self._alloc.remove(name)                              # raises while a converter holds the voice
        self.registers.pop(name, None)
        self.ranges.pop(name, None)
        self._changed()
        return self

    def compact(self):
        """slide every voice down until no hole remains between voices.  A voice may move by less than its own length, so a move's
        source and destination may overlap: alive_pool_move_rows copies chain by chain (the elements one shift apart), each chain
        in the direction in which an element is read before it is overwritten (csrc/knn.hip: pool_move_kernel)"""
        self._reserved("compact")
        moves = self._alloc.compact()
        for _, src, dst, n in moves:                          # address order: each destination is free, or its own source, by now
            self._move(src, dst, n)
        if moves:
            self._changed()
        return self

    def hold(self, name, who):
        """count `who` (a label: a converter) as a user of the voice; `remove` raises while any is left"""
        self._reserved("hold")
        self._alloc.hold(name, who)

    def release(self, name, who):
        self._reserved("release")
        self._alloc.release(name, who)

    @property
    def layout(self):
        self._reserved("layout")
        return self._alloc.layout

    def holes(self):
        """the free ranges [(first row, rows), ...] in address order"""
        self._reserved("holes")
        return self._alloc.holes()

    @property
    def free_rows(self):
        self._reserved("free_rows")
        return self._alloc.free_rows

    @property
    def largest_hole(self):
        self._reserved("largest_hole")
        return self._alloc.largest_hole

    def tokens(self, name):
        """the voice's tokens [768, M], bitwise those that went in (a reserved pool keeps no copy: rebuilt from its rows); of a half
        pool the rounded tokens, widened to fp32: what was stored"""
        lo, m = self.segment(name)
        if self.dtype != torch.float32:
            return self.rows[lo:lo + m].float().t().contiguous()
        if self.capacity is None:
            return self._tokens[name]
        return self.rows[lo:lo + m].t().contiguous()

    def segment(self, name):
        if name not in self.segments:
            raise ValueError(f"unknown voice {name!r} (the pool holds {sorted(self.segments)})")
        return self.segments[name]

    def _pack(self):
        L = nat.lib()
        P = sum(int(t.shape[1]) for t in self._tokens.values())
        rows = torch.empty(P, DIM, dtype=self.dtype, device=self.device)
        norms = torch.empty(P, dtype=torch.float32, device=self.device)
        if P >= 2 ** 31:
            raise ValueError(f"a voice pool holds fewer than 2^31 rows (got {P})")
        segs, lo = {}, 0
        for name, t in self._tokens.items():
            m = int(t.shape[1])
            if m < 1:
                raise ValueError(f"voice {name!r} is empty")
            if self.dtype == torch.float16:                   # the half append: the bits a reserved half pool holds
                self._append_into(rows, norms, P, lo, t)
            else:
                nat.check(L.alive_library_pack_rows(nat.ptr(t), m, DIM, rows[lo].data_ptr(), norms[lo].data_ptr(), nat.stream()),
                          "alive_library_pack_rows")
            segs[name] = (lo, m)
            lo += m
        bad = ~(torch.isfinite(norms) & (norms > 0))          # as PackedLibrary: a zero-norm row would match every frame
        if bool(bad.any()):
            raise ValueError(f"voice pool row {int(torch.nonzero(bad)[0])} has zero or non-finite norm: remove it")
        self.rows, self.norms, self.P, self.segments = rows, norms, P, segs
        self.version += 1
        self._images = None

    def search_images(self):
        """The pool search's tables, built on first use after the pool changed (the streaming path never asks; a reserved pool
        passes its live voices only, with P its capacity):
        a dict of the bf16 image buffer, device int64 img_off [V], int32 seg_lo / seg_len [V], float32 bounds [V] (the
        deterministic certificate's per-voice rounding bound), the voice names in table order, and the longest voice."""
        self._need_f32("VoicePool.search_images")
        if self._images is not None:
            return self._images
        L = nat.lib()
        names = list(self.segments)
        V = len(names)
        if V == 0:
            raise ValueError("the voice pool is empty")
        lo = np.array([self.segments[n][0] for n in names], dtype=np.int32)
        ln = np.array([self.segments[n][1] for n in names], dtype=np.int32)
        off = np.zeros(V, dtype=np.int64)
        nbytes = L.alive_pool_image_bytes(ln.ctypes.data, V, off.ctypes.data)
        if nbytes == 0:
            raise ValueError("voice pool: bad segment table")
        images = torch.empty(nbytes // 2, dtype=torch.int16, device=self.device)
        bounds = torch.empty(V, dtype=torch.float32, device=self.device)
        nat.check(L.alive_pool_pack_images(nat.ptr(self.rows), nat.ptr(self.norms), self.P, lo.ctypes.data, ln.ctypes.data, V,
                                           nat.ptr(images), nat.ptr(bounds), nat.stream()), "alive_pool_pack_images")
        dev = self.device
        self._images = dict(images=images, img_off=torch.from_numpy(off).to(dev), seg_lo=torch.from_numpy(lo).to(dev),
                            seg_len=torch.from_numpy(ln).to(dev), bounds=bounds, names=names, index={n: i for i, n in enumerate(names)},
                            max_len=int(ln.max()))
        return self._images

    def voice_ids(self, names):
        """voice names (None: an inactive row) -> device int32 [N] indices of the pool search's table"""
        self._need_f32("VoicePool.voice_ids")
        index = self.search_images()["index"]
        ids = []
        for n in names:
            if n is not None and n not in index:
                raise ValueError(f"unknown voice {n!r} (the pool holds {sorted(index)})")
            ids.append(-1 if n is None else index[n])
        return torch.tensor(ids, dtype=torch.int32, device=self.device)


def _track_call(pitch_track, world_pitch, device):
    """enrolment's pitch_track= -> the keywords of F0Estimator.estimate ({} without it); not together with world_pitch"""
    o = common.track_options(pitch_track)
    if o is None:
        return {}
    if world_pitch:
        raise ValueError("pitch_track cannot be combined with world_pitch: the tracker decodes the estimator's class scores")
    return dict(track=common.pitch_track(o["lo"], o["hi"], o["band"], device), track_weight=o["weight"], track_jump=o["jump"])


def measure_register(f0_estimator, wf16, world_pitch=False, pitch_track=None, voicing=None):
    """the register (sum of voiced pitch, voiced frames) of 16 kHz audio wf16 [1, L] on the device, as host floats: the f0 estimator's
    f0 of its spectrogram (world_pitch: WORLD's f0 of the audio) through alive_pitch_stats2_groups, one group, every frame: a
    Register, the 2-tuple it always was (bitwise alive_pitch_stats_groups') with the sum of squares as `.sumsq`.  One host read: for
    enrolment, never inside a tick.  pitch_track (True, or dict(weight=, jump=, lo=, hi=, band=)): the register and the range are measured
    on the tracked contour (F0Estimator.estimate(track=)), as a session with pitch_track hears its source.  voicing (True, or a dict
    of common.voicing_options' keys): on the frames the voicing decision finds voiced (ops.voicing_rows_), as a session with voicing
    hears its source; not together with world_pitch."""
    track = _track_call(pitch_track, world_pitch, wf16.device)
    voicing = common.voicing_options(voicing)
    if voicing is not None and world_pitch:
        raise ValueError("voicing cannot be combined with world_pitch: WORLD makes its own voicing decision")

    def f0():
        if world_pitch:
            return compute_f0(wf16)
        f = f0_estimator.estimate(spectrogram(wf16), **track)
        return f if voicing is None else ops.voicing_rows_(f, wf16.contiguous(), voicing)
    f = ops.Fp16Guard().run(f0)
    first = torch.tensor([0, f.shape[0]], dtype=torch.int32, device=f.device)
    s, c, q = pitch_stats2_groups(f, first)[0].tolist()
    return Register(s, c, q)


def voice_parts(content_encoder, wav=None, sr=None, lib=None, every=4, device="cuda", f0_estimator=None, world_pitch=False,
                codebook=None, codebook_iters=10, codebook_seed=0, pitch_track=None, voicing=None):
    """A voice's tokens as realtime_inference.py builds its library, as strided [768, m] parts and without a copy: the target
    utterance `wav` [channels, samples] at `sr` Hz -- resampled to 16 kHz, peak-normalised, first channel, content_encoder(
    spectrogram(.)), every `every`-th frame (a column-strided view of the encoder's output) -- then the tokens of `lib` (a voice
    library file, or its tokens [1, 768, M] / [768, M]).  The encoder runs under ops.Fp16Guard, as generate_voice_library.py's.
    f0_estimator= (auto pitch): returns (parts, register) instead, the register measured on the same 16 kHz audio the encoder saw
    (measure_register; world_pitch: with WORLD's f0; pitch_track: on the tracked contour; voicing: on the voiced frames), None without a target wav.  Without it
    the call is what it was.
    codebook=SIZE: the parts are condensed together, once, to one part of SIZE centroid rows (module/codebook.py build_codebook with
    codebook_iters and codebook_seed; a voice of SIZE rows or fewer stays as it is); the register is measured on the audio as before."""
    from .voice_library import VoiceLibrary
    parts, register = [], None
    if wav is not None:
        wf = audio_io.resample(wav.to(device), sr, 16000)
        wf = wf / wf.abs().max()
        feats = ops.Fp16Guard().run(lambda: content_encoder(spectrogram(wf[:1])))
        parts.append(feats[0][:, ::every])
        if f0_estimator is not None:
            register = measure_register(f0_estimator, wf[:1].contiguous(), world_pitch, pitch_track, voicing)
    if lib is not None:
        if isinstance(lib, (str, bytes)) or hasattr(lib, "__fspath__"):
            VL = VoiceLibrary().to(device)
            VL.load_state_dict(torch.load(lib, map_location=device))
            lib = VL.tokens
        parts.append(_tokens_2d(lib))
    if not parts:
        raise ValueError("a voice needs a target wav and / or a voice library")
    if codebook is not None:
        from .codebook import build_codebook, check_size
        check_size(codebook)
        if sum(int(t.shape[1]) for t in parts) > codebook:
            whole = torch.cat([t.to(device, torch.float32) for t in parts], dim=1)
            parts = [build_codebook(whole, codebook, iters=codebook_iters, seed=codebook_seed)]
    return parts if f0_estimator is None else (parts, register)


def enrol_steps(pool, name, content_encoder, wav, sr, lib=None, every=4, max_frames=None, compact=False, f0_estimator=None,
                world_pitch=False, codebook=None, codebook_iters=10, codebook_seed=0, pitch_track=None, voicing=None):
    """enrol_voice as a generator: the utterance is encoded once, then each next() appends one piece -- `add` for the first, `extend`
    for the rest -- and yields the voice's row count so far, so that a server can put a tick between the pieces.  If a piece is
    refused the voice is removed again (when no session holds it yet) and the error propagates.  f0_estimator=: the utterance's
    register is measured too (voice_parts) and stored with the first piece.  codebook=SIZE: the voice is condensed to SIZE centroids
    first (voice_parts), and the centroids are appended in pieces."""
    if pool.capacity is None:
        raise ValueError("enrol_voice needs a reserved pool: VoicePool(..., capacity=ROWS)")
    if max_frames is not None and int(max_frames) < 1:
        raise ValueError(f"max_frames={max_frames!r} must be >= 1")
    register = None
    cb = {} if codebook is None else dict(codebook=codebook, codebook_iters=codebook_iters, codebook_seed=codebook_seed)
    if f0_estimator is None:
        parts = voice_parts(content_encoder, wav, sr, lib, every, pool.device, **cb)
    else:
        parts, register = voice_parts(content_encoder, wav, sr, lib, every, pool.device, f0_estimator, world_pitch,
                                      pitch_track=pitch_track, voicing=voicing, **cb)
    total = sum(int(t.shape[1]) for t in parts)
    step = total if max_frames is None else int(max_frames)
    if compact and pool.largest_hole < min(step, total) <= pool.free_rows:
        pool.compact()
    # pieces of at most `step` tokens of the parts laid end to end; a piece that spans two parts is a list of two views
    pieces, cur, room = [], [], step
    for t in parts:
        at, m = 0, int(t.shape[1])
        while at < m:
            n = min(room, m - at)
            cur.append(t[:, at:at + n])
            at, room = at + n, room - n
            if room == 0:
                pieces.append(cur)
                cur, room = [], step
    if cur:
        pieces.append(cur)
    done = 0
    try:
        for i, piece in enumerate(pieces):
            if i == 0:
                pool.add(name, piece) if register is None else pool.add(name, piece, register)
            else:
                pool.extend(name, piece)
            done += sum(int(t.shape[1]) for t in piece)
            yield done
    except ValueError:
        if done and name in pool.segments:
            try:
                pool.remove(name)
            except ValueError:                                 # a session opened on the part that is there: it stays
                pass
        raise


def enrol_voice(pool, name, content_encoder, wav, sr, lib=None, every=4, max_frames=None, compact=False, f0_estimator=None,
                world_pitch=False, codebook=None, codebook_iters=10, codebook_seed=0, pitch_track=None, voicing=None):
    """Enrol a voice into a reserved pool from audio, while sessions run on the pool's other voices: the recipe of voice_parts
    (multistream_inference.voice_tokens', under ops.Fp16Guard), appended through the strided alive_pool_append -- the encoder's
    output is never copied or concatenated.  The voice's rows are bitwise those of voice_tokens followed by `add`.

    max_frames: the tokens go in pieces of at most that many, `add` then `extend`s (enrol_steps yields between them).  The content
    encoder's receptive field spans the whole utterance, so no cut of the AUDIO gives bitwise the frames of one call: the utterance
    is encoded once and its tokens are appended piece by piece, which is bitwise one call for any max_frames (a row and its norm
    depend on the row's own token alone).  compact=True: compact the pool first when the first piece fits its free rows but none
    of its holes.  f0_estimator= (auto pitch): the voice also gets its register, measured on the same audio (voice_parts; with
    pitch_track= on the tracked contour, with voicing= on the voiced frames).
    codebook=SIZE (with codebook_iters, codebook_seed): the voice goes in as its SIZE-row codebook (module/codebook.py), bitwise
    `add(name, build_codebook(tokens, SIZE))`; `compact=` is about the pool's holes and has nothing to do with it.
    Returns the voice's row count."""
    rows = 0
    for rows in enrol_steps(pool, name, content_encoder, wav, sr, lib, every, max_frames, compact, f0_estimator, world_pitch,
                            codebook, codebook_iters, codebook_seed, pitch_track, voicing):
        pass
    return rows


def knn_search_grouped(source, rows, norms, seg_lo, seg_len, k):
    """source [N, 768, T], pool rows (fp32, or the fp16 rows of a half pool: alive_knn_search_grouped_f16) / norms, device int32
    seg_lo / seg_len [N] -> (val [N*T, k], idx [N*T, k] pool indices)"""
    n, d, t = source.shape
    L = nat.lib()
    if not 1 <= k <= MAX_K:
        raise ValueError(f"grouped search: k={k} outside [1, {MAX_K}]")
    nbytes = L.alive_knn_grouped_workspace_bytes(n, t, k)
    if nbytes == 0:                                         # (before anything is allocated)
        raise ValueError(f"grouped search: {n} rows x {t} frames (k={k}) out of range")
    fn, name = _rows_call("alive_knn_search_grouped", rows)
    val = torch.empty(n * t, k, dtype=torch.float32, device=source.device)
    idx = torch.empty(n * t, k, dtype=torch.int32, device=source.device)
    ws = _ws.get(nbytes, source.device)
    nat.check(fn(nat.ptr(source), n, t, nat.ptr(rows), nat.ptr(norms), rows.shape[0], nat.ptr(seg_lo), nat.ptr(seg_len), k, nat.ptr(val),
                 nat.ptr(idx), nat.ptr(ws), nat.stream()), name)
    return val, idx


def knn_search_grouped_k(source, rows, norms, seg_lo, seg_len, k_row, k_max):
    """knn_search_grouped with a k per row: device int32 k_row [N], 1 <= k_row[n] <= k_max -> (val, idx) [N*T, k_max]; row n's
    first k_row[n] entries per frame are bitwise knn_search_grouped at that k, the rest -inf / -1 (alive_knn_search_grouped_k)"""
    n, d, t = source.shape
    L = nat.lib()
    if not 1 <= k_max <= MAX_K:
        raise ValueError(f"grouped search: k_max={k_max} outside [1, {MAX_K}]")
    if k_row.dtype != torch.int32 or k_row.numel() != n:
        raise ValueError("grouped search: k_row must be int32 [N]")
    nbytes = L.alive_knn_grouped_k_workspace_bytes(n, t, k_max)
    if nbytes == 0:                                         # (before anything is allocated)
        raise ValueError(f"grouped search: {n} rows x {t} frames (k_max={k_max}) out of range")
    fn, name = _rows_call("alive_knn_search_grouped_k", rows)
    val = torch.empty(n * t, k_max, dtype=torch.float32, device=source.device)
    idx = torch.empty(n * t, k_max, dtype=torch.int32, device=source.device)
    ws = _ws.get(nbytes, source.device)
    nat.check(fn(nat.ptr(source), n, t, nat.ptr(rows), nat.ptr(norms), rows.shape[0], nat.ptr(seg_lo), nat.ptr(seg_len), nat.ptr(k_row),
                 k_max, nat.ptr(val), nat.ptr(idx), nat.ptr(ws), nat.stream()), name)
    return val, idx


def knn_pool_workspace_bytes(n, t, k, pool):
    im = pool.search_images()
    return nat.lib().alive_knn_pool_workspace_bytes(n, t, k, len(im["names"]), pool.P, im["max_len"])


def knn_search_pool(source, pool, voice_ids, k, stats=False):
    """source [N, 768, T], a VoicePool, device int32 voice_ids [N] (-1: inactive) -> (val [N*T, k], idx [N*T, k] pool indices):
    the strict search of every row against its own voice in one call (csrc/knn.hip: alive_knn_search_pool).  stats=True also
    returns the call's counters (a host copy: a sync)."""
    n, d, t = source.shape
    L = nat.lib()
    if not 1 <= k <= MAX_K:
        raise ValueError(f"pool search: k={k} outside [1, {MAX_K}]")
    im = pool.search_images()
    nbytes = knn_pool_workspace_bytes(n, t, k, pool)
    if nbytes == 0:                                         # (before anything is allocated)
        raise ValueError(f"pool search: {n} rows x {t} frames (k={k}) out of range")
    if voice_ids.dtype != torch.int32 or voice_ids.numel() != n:
        raise ValueError("pool search: voice_ids must be int32 [N]")
    source = source.contiguous()
    val = torch.empty(n * t, k, dtype=torch.float32, device=source.device)
    idx = torch.empty(n * t, k, dtype=torch.int32, device=source.device)
    ws = _ws.get(nbytes, source.device)
    nat.check(L.alive_knn_search_pool(nat.ptr(source), n, t, nat.ptr(im["images"]), nat.ptr(im["img_off"]), nat.ptr(pool.rows),
                                      nat.ptr(pool.norms), nat.ptr(im["bounds"]), pool.P, nat.ptr(im["seg_lo"]), nat.ptr(im["seg_len"]),
                                      len(im["names"]), im["max_len"], nat.ptr(voice_ids), k, nat.ptr(val), nat.ptr(idx), nat.ptr(ws),
                                      nat.stream()), "alive_knn_search_pool")
    if stats:                                               # knn.hip alive_knn_pool_stats: int[ALIVE_POOL_STATS] at the front of ws
        c = ws[:32].view(torch.int32).tolist()
        return val, idx, dict(frames_failed_certificate=c[0], frames_searched_exactly=c[1], voice_groups=c[2], frame_blocks=c[3])
    return val, idx


def knn_search_pool_k(source, pool, voice_ids, k_row, k_max):
    """knn_search_pool with a k per row: device int32 k_row [N], 1 <= k_row[n] <= k_max -> (val, idx) [N*T, k_max]; row n's first
    k_row[n] entries per frame are bitwise knn_search_pool at that k, the rest -inf / -1 (alive_knn_search_pool_k)"""
    n, d, t = source.shape
    L = nat.lib()
    if not 1 <= k_max <= MAX_K:
        raise ValueError(f"pool search: k_max={k_max} outside [1, {MAX_K}]")
    im = pool.search_images()
    nbytes = L.alive_knn_pool_k_workspace_bytes(n, t, k_max, len(im["names"]), pool.P, im["max_len"])
    if nbytes == 0:                                         # (before anything is allocated)
        raise ValueError(f"pool search: {n} rows x {t} frames (k_max={k_max}) out of range")
    if voice_ids.dtype != torch.int32 or voice_ids.numel() != n:
        raise ValueError("pool search: voice_ids must be int32 [N]")
    if k_row.dtype != torch.int32 or k_row.numel() != n:
        raise ValueError("pool search: k_row must be int32 [N]")
    source = source.contiguous()
    val = torch.empty(n * t, k_max, dtype=torch.float32, device=source.device)
    idx = torch.empty(n * t, k_max, dtype=torch.int32, device=source.device)
    ws = _ws.get(nbytes, source.device)
    nat.check(L.alive_knn_search_pool_k(nat.ptr(source), n, t, nat.ptr(im["images"]), nat.ptr(im["img_off"]), nat.ptr(pool.rows),
                                        nat.ptr(pool.norms), nat.ptr(im["bounds"]), pool.P, nat.ptr(im["seg_lo"]),
                                        nat.ptr(im["seg_len"]), len(im["names"]), im["max_len"], nat.ptr(voice_ids), nat.ptr(k_row),
                                        k_max, nat.ptr(val), nat.ptr(idx), nat.ptr(ws), nat.stream()), "alive_knn_search_pool_k")
    return val, idx


def merge_gather_rows_k(val, idx, k_row, k_max, alpha, rows, source):
    """merge_gather_rows with a k per row (device int32 k_row [N]); val / idx [N*T, k_max] from a per-row-k search"""
    n, d, t = source.shape
    fn, name = _rows_call("alive_knn_merge_gather_rows_k", rows)
    out = torch.empty_like(source)
    nat.check(fn(nat.ptr(val), nat.ptr(idx), nat.ptr(k_row), k_max, nat.ptr(alpha), nat.ptr(rows), nat.ptr(source), n, t, nat.ptr(out),
                 None, nat.stream()), name)
    return out


def blend_gather_rows_k(val, idx, k_row, k_max, first, weight, alpha, rows, source):
    """blend_gather_rows with a k per OUTPUT row (device int32 k_row [N]): every list of a blend uses its owner's k; val / idx
    [first[N] * T, k_max] from a per-row-k search whose k_row repeats the owner's k on each of its list rows"""
    n, d, t = source.shape
    fn, name = _rows_call("alive_knn_blend_gather_rows_k", rows)
    out = torch.empty_like(source)
    nat.check(fn(nat.ptr(val), nat.ptr(idx), nat.ptr(k_row), k_max, nat.ptr(first), nat.ptr(weight), nat.ptr(alpha), nat.ptr(rows),
                 nat.ptr(source), n, t, nat.ptr(out), nat.stream()), name)
    return out


knn_path_rows = ops.knn_path_rows       # the path between a per-row-k search and its gather (csrc/match_path.hip)


def check_k(k, what="k", hi=MAX_K):
    """a k of the batched paths: an int (not a bool) in [1, hi] -> int; ValueError otherwise"""
    if isinstance(k, (bool, np.bool_)) or not isinstance(k, (int, np.integer)) or not 1 <= int(k) <= hi:
        raise ValueError(f"{what}={k!r}: expected an integer in [1, {hi}]")
    return int(k)


def merge_gather_rows(val, idx, k, alpha, rows, source):
    """merge_gather with one shard and a per-window alpha (device float64 [N])"""
    n, d, t = source.shape
    fn, name = _rows_call("alive_knn_merge_gather_rows", rows)
    out = torch.empty_like(source)
    nat.check(fn(nat.ptr(val), nat.ptr(idx), k, nat.ptr(alpha), nat.ptr(rows), nat.ptr(source), n, t, nat.ptr(out), None, nat.stream()),
              name)
    return out


def blend_gather_rows(val, idx, k, first, weight, alpha, rows, source):
    """the blend of output row n: the weighted sum of the means of its list rows first[n] .. first[n+1]-1 (device int32 [N+1];
    weight: device float64 [first[N]]; val / idx: [first[N] * T, k] from a grouped or pool search of the list rows), then the
    per-row alpha (device float64 [N]) as merge_gather_rows (csrc/knn.hip: alive_knn_blend_gather_rows)"""
    n, d, t = source.shape
    fn, name = _rows_call("alive_knn_blend_gather_rows", rows)
    out = torch.empty_like(source)
    nat.check(fn(nat.ptr(val), nat.ptr(idx), k, nat.ptr(first), nat.ptr(weight), nat.ptr(alpha), nat.ptr(rows), nat.ptr(source), n, t,
                 nat.ptr(out), nat.stream()), name)
    return out


def pitch_transform_rows_(f0, mode, f0_rate, pitch_shift, intonation):
    """in place on f0 [N, 1, T] with device float32 [N] parameters (ops.pitch_transform_ row by row)"""
    n, _, t = f0.shape
    nat.check(nat.lib().alive_pitch_transform_rows(nat.ptr(f0), n, t, mode, nat.ptr(f0_rate), nat.ptr(pitch_shift),
                                                   nat.ptr(intonation), nat.stream()), "alive_pitch_transform_rows")
    return f0


def pitch_stats_groups(f0, first, t_lo=0, t_hi=None, out=None):
    """f0 [N, 1, T] or [N, T], device int32 first [G + 1] -> device float64 [G, 2]: (sum of voiced pitch, voiced frames) over
    frames [t_lo, t_hi) (default: all) of rows first[g] .. first[g + 1] - 1, in fp64 in a fixed order (alive_pitch_stats_groups)"""
    if f0.dtype != torch.float32 or not f0.is_contiguous():
        raise ValueError("pitch_stats_groups: f0 must be contiguous float32")
    if first.dtype != torch.int32 or first.dim() != 1 or first.numel() < 2:
        raise ValueError("pitch_stats_groups: first must be int32 [G + 1]")
    n, t = f0.shape[0], f0.shape[-1]
    g = first.numel() - 1
    stats = torch.empty(g, 2, dtype=torch.float64, device=f0.device) if out is None else out
    nat.check(nat.lib().alive_pitch_stats_groups(nat.ptr(f0), n, t, int(t_lo), int(t if t_hi is None else t_hi), nat.ptr(first), g,
                                                 nat.ptr(stats), nat.stream()), "alive_pitch_stats_groups")
    return stats


def pitch_shift_groups(stats, first, n, offset, auto_on, target):
    """the offline shift of every row, device float32 [n]: group g's offset[g], plus target[g] - (float)(sum / count) on an auto
    group with voiced frames (alive_pitch_shift_groups); offset / target: device float32 [G], auto_on: device int32 [G]"""
    g = first.numel() - 1
    out = torch.empty(n, dtype=torch.float32, device=stats.device)
    nat.check(nat.lib().alive_pitch_shift_groups(nat.ptr(stats), nat.ptr(first), g, n, nat.ptr(offset), nat.ptr(auto_on),
                                                 nat.ptr(target), nat.ptr(out), nat.stream()), "alive_pitch_shift_groups")
    return out


def pitch_follow_rows_(f0, f0_rate, offset, auto_on, target, emit, decay, prior, state, shift_out):
    """the streaming register update of every row of f0 [N, 1, T], in place on state (float64 [N, 2]) and shift_out (float32 [N]):
    alive_pitch_follow_rows.  emit: device bool / uint8 [N] (or [N, 1])"""
    n, t = f0.shape[0], f0.shape[-1]
    nat.check(nat.lib().alive_pitch_follow_rows(nat.ptr(f0), n, t, nat.ptr(f0_rate), nat.ptr(offset), nat.ptr(auto_on),
                                                nat.ptr(target), nat.ptr(emit), float(decay), float(prior), nat.ptr(state),
                                                nat.ptr(shift_out), nat.stream()), "alive_pitch_follow_rows")
    return shift_out


def pitch_stats2_groups(f0, first, t_lo=0, t_hi=None, out=None):
    """pitch_stats_groups with the sum of squares: device float64 [G, 3] = (sum, count, sum of squares), the first two bitwise
    pitch_stats_groups' (alive_pitch_stats2_groups)"""
    if f0.dtype != torch.float32 or not f0.is_contiguous():
        raise ValueError("pitch_stats2_groups: f0 must be contiguous float32")
    if first.dtype != torch.int32 or first.dim() != 1 or first.numel() < 2:
        raise ValueError("pitch_stats2_groups: first must be int32 [G + 1]")
    n, t = f0.shape[0], f0.shape[-1]
    g = first.numel() - 1
    stats = torch.empty(g, 3, dtype=torch.float64, device=f0.device) if out is None else out
    nat.check(nat.lib().alive_pitch_stats2_groups(nat.ptr(f0), n, t, int(t_lo), int(t if t_hi is None else t_hi), nat.ptr(first), g,
                                                  nat.ptr(stats), nat.stream()), "alive_pitch_stats2_groups")
    return stats


def pitch_range_groups(stats3, first, n, inton, range_on, target_sd, range_max=2.0):
    """the offline intonation, centre and centre switch of every row, device (float32 [n], float32 [n], int32 [n]): a group with
    range_on and voiced frames gets inton * clamp(target_sd / its own sd) around its own mean, every other group its inton and no
    centre (alive_pitch_range_groups); inton: device float32 [G], target_sd: device float64 [G], range_on: device int32 [G]"""
    g = first.numel() - 1
    dev = stats3.device
    i_out = torch.empty(n, dtype=torch.float32, device=dev)
    c_out = torch.empty(n, dtype=torch.float32, device=dev)
    on_out = torch.empty(n, dtype=torch.int32, device=dev)
    nat.check(nat.lib().alive_pitch_range_groups(nat.ptr(stats3), nat.ptr(first), g, n, nat.ptr(inton), nat.ptr(range_on),
                                                 nat.ptr(target_sd), float(range_max), nat.ptr(i_out), nat.ptr(c_out),
                                                 nat.ptr(on_out), nat.stream()), "alive_pitch_range_groups")
    return i_out, c_out, on_out


def pitch_follow2_rows_(f0, f0_rate, offset, auto_on, target, inton, range_on, target_sd, emit, decay, prior, range_max, state3,
                        shift_out, inton_out, centre_out, centre_on_out):
    """pitch_follow_rows_ on state3 (float64 [N, 3] = (S, W, Q)), in place on it and on the four outputs (float32 [N] x 3, int32
    [N]): alive_pitch_follow2_rows"""
    n, t = f0.shape[0], f0.shape[-1]
    nat.check(nat.lib().alive_pitch_follow2_rows(nat.ptr(f0), n, t, nat.ptr(f0_rate), nat.ptr(offset), nat.ptr(auto_on),
                                                 nat.ptr(target), nat.ptr(inton), nat.ptr(range_on), nat.ptr(target_sd),
                                                 nat.ptr(emit), float(decay), float(prior), float(range_max), nat.ptr(state3),
                                                 nat.ptr(shift_out), nat.ptr(inton_out), nat.ptr(centre_out),
                                                 nat.ptr(centre_on_out), nat.stream()), "alive_pitch_follow2_rows")
    return shift_out, inton_out, centre_out, centre_on_out


def pitch_transform_rows_centred_(f0, mode, f0_rate, pitch_shift, intonation, centre, centre_on):
    """pitch_transform_rows_ with a centre per row (device float32 [N]) where centre_on (device int32 [N]) is set; a row with
    centre_on == 0 is bitwise pitch_transform_rows_ (alive_pitch_transform_rows_centred)"""
    n, t = f0.shape[0], f0.shape[-1]
    nat.check(nat.lib().alive_pitch_transform_rows_centred(nat.ptr(f0), n, t, mode, nat.ptr(f0_rate), nat.ptr(pitch_shift),
                                                           nat.ptr(intonation), nat.ptr(centre), nat.ptr(centre_on), nat.stream()),
              "alive_pitch_transform_rows_centred")
    return f0


def check_range_max(range_max, what="pitch_range_max"):
    if isinstance(range_max, (bool, np.bool_)) or not isinstance(range_max, (int, float, np.integer, np.floating)) or not (
            np.isfinite(range_max) and range_max >= 1):
        raise ValueError(f"{what}={range_max!r} must be a finite number >= 1")
    return float(range_max)


def check_intonation(intonation, what="intonation"):
    if isinstance(intonation, (bool, np.bool_)) or not isinstance(intonation, (int, float, np.integer, np.floating)) or not (
            np.isfinite(intonation) and intonation >= 0):
        raise ValueError(f"{what}={intonation!r} must be a finite number >= 0")
    return float(intonation)


def gate_thr_ms(gate_db):
    """a gate threshold in dBFS -> the mean square alive_gate_rows compares with: 10^(dB / 10) in float64.  ValueError unless it is
    a finite number (not a bool)"""
    if isinstance(gate_db, (bool, np.bool_)) or not isinstance(gate_db, (int, float, np.integer, np.floating)) or not np.isfinite(
            gate_db):
        raise ValueError(f"gate_db={gate_db!r} must be a finite number of dBFS, or None for no gate")
    return 10.0 ** (float(gate_db) / 10.0)


def gate_hold_ticks(gate_hold, tick_seconds):
    """a gate's hold in seconds -> ticks: ceil(hold / tick).  ValueError unless it is a finite number >= 0 (not a bool)"""
    if isinstance(gate_hold, (bool, np.bool_)) or not isinstance(gate_hold, (int, float, np.integer, np.floating)) or not (
            np.isfinite(gate_hold) and gate_hold >= 0):
        raise ValueError(f"gate_hold={gate_hold!r} must be a finite number of seconds >= 0")
    ticks = int(np.ceil(float(gate_hold) / float(tick_seconds)))
    if ticks >= 2 ** 31:
        raise ValueError(f"gate_hold={gate_hold!r} is {ticks} ticks: too long")
    return ticks


def gate_window(begin_of_output, end_of_output, ring16, lookahead):
    """the detection window of a ring of ring16 samples at 16 kHz: [begin_of_output, min(ring16, end_of_output + lookahead))"""
    return int(begin_of_output), min(int(ring16), int(end_of_output) + int(lookahead))


def gate_rows(x, w_lo, w_hi, gate_on, thr_ms, hold_ticks, emit, world_on, S, seg_len, state, g0, g1, seg_len_eff, follow,
              world_eff, ms_out=None):
    """alive_gate_rows on x [N, ld] (the 16 kHz rings): this tick's decision of every row into g0, g1, seg_len_eff, follow,
    world_eff (world_on / world_eff: both None without a WORLD branch), state updated in place.  ms_out: float64 [N] or None"""
    n, ld = x.shape
    if x.dtype != torch.float32 or not x.is_contiguous():
        raise ValueError("gate_rows: x must be contiguous float32 [N, ld]")
    nat.check(nat.lib().alive_gate_rows(nat.ptr(x), n, ld, int(w_lo), int(w_hi), nat.ptr(gate_on), nat.ptr(thr_ms),
                                        nat.ptr(hold_ticks), nat.ptr(emit), nat.ptr(world_on), int(S), nat.ptr(seg_len),
                                        nat.ptr(state), nat.ptr(g0), nat.ptr(g1), nat.ptr(seg_len_eff), nat.ptr(follow),
                                        nat.ptr(world_eff), nat.ptr(ms_out), nat.stream()), "alive_gate_rows")


def gate_apply_rows_(y, span_lo, span_len, g0, g1):
    """alive_gate_apply_rows in place on y [N, ld]: every row's span times its ramp from g0 to g1"""
    n, ld = y.shape
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("gate_apply_rows_: y must be contiguous float32 [N, ld]")
    nat.check(nat.lib().alive_gate_apply_rows(nat.ptr(y), n, ld, nat.ptr(span_lo), nat.ptr(span_len), nat.ptr(g0), nat.ptr(g1),
                                              nat.stream()), "alive_gate_apply_rows")
    return y


def ring_push_rows_(ring, chunks, chunk_len, ring_len, present, x, seg_len=None, seg_len_tick=None, S=1, world_on=None,
                    world_tick=None):
    """alive_ring_push_rows in place: the rows with present != 0 have their int16 ring [N, ld] (time order) advanced by their chunk
    (chunks int16 [N, ld_chunk], chunk_len / ring_len int32 [N]) and their row of x float32 [N, ld_x] rewritten from it; the others
    are not touched.  seg_len -> seg_len_tick (int32 [N * S]) and world_on -> world_tick (int32 [N]): the tick's masked row arrays,
    zero on an absent row (each pair both given or both None)"""
    if ring.dim() != 2 or ring.dtype != torch.int16 or not ring.is_contiguous():
        raise ValueError("ring_push_rows_: ring must be contiguous int16 [N, ld]")
    n, ld = ring.shape
    if chunks.dtype != torch.int16 or chunks.dim() != 2 or chunks.shape[0] != n or not chunks.is_contiguous():
        raise ValueError("ring_push_rows_: chunks must be contiguous int16 [N, ld_chunk]")
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[0] != n or not x.is_contiguous():
        raise ValueError("ring_push_rows_: x must be contiguous float32 [N, ld_x]")
    if present.numel() != n or present.element_size() != 1:
        raise ValueError("ring_push_rows_: present must be [N] bytes")
    for name, t, size in (("chunk_len", chunk_len, n), ("ring_len", ring_len, n), ("seg_len", seg_len, n * int(S)),
                          ("seg_len_tick", seg_len_tick, n * int(S)), ("world_on", world_on, n), ("world_tick", world_tick, n)):
        if t is not None and (t.dtype != torch.int32 or t.numel() != size):
            raise ValueError(f"ring_push_rows_: {name} must be int32 [{size}]")
    if (seg_len is None) != (seg_len_tick is None) or (world_on is None) != (world_tick is None):
        raise ValueError("ring_push_rows_: seg_len / seg_len_tick and world_on / world_tick are given in pairs")
    nat.check(nat.lib().alive_ring_push_rows(nat.ptr(ring), n, ld, nat.ptr(chunks), chunks.shape[1], nat.ptr(chunk_len),
                                             nat.ptr(ring_len), nat.ptr(present), nat.ptr(x), x.shape[1], int(S), nat.ptr(seg_len),
                                             nat.ptr(seg_len_tick), nat.ptr(world_on), nat.ptr(world_tick), nat.stream()),
              "alive_ring_push_rows")
    return ring


CONCEAL_MAX_SPAN, CONCEAL_QMAX = 4096, 1 << 30      # ALIVE_CONCEAL_MAX_SPAN, ALIVE_CONCEAL_QMAX (include/alive_vc.h)


def conceal_rows_(ring, ring_len, chunks, chunk_len, present, lost, on, consts, state, tmpl):
    """alive_conceal_rows in place on chunks int16 [N, ld_chunk]: the rows with lost != 0 get their made-up chunk, the present rows in
    a run (state[n, 0] > 0) have the head of their chunk faded in from the continuation; ring int16 [N, ld] is read only.  present /
    lost / on: [N] bytes; consts int32 [6, N]: lag_lo, lag_hi, window, hold, fade, recover per row; state int32 [N, 2] and tmpl int16
    [N, ld_tmpl] are the rows' state"""
    if ring.dim() != 2 or ring.dtype != torch.int16 or not ring.is_contiguous():
        raise ValueError("conceal_rows_: ring must be contiguous int16 [N, ld]")
    n, ld = ring.shape
    if chunks.dtype != torch.int16 or chunks.dim() != 2 or chunks.shape[0] != n or not chunks.is_contiguous():
        raise ValueError("conceal_rows_: chunks must be contiguous int16 [N, ld_chunk]")
    if tmpl.dtype != torch.int16 or tmpl.dim() != 2 or tmpl.shape[0] != n or not tmpl.is_contiguous():
        raise ValueError("conceal_rows_: tmpl must be contiguous int16 [N, ld_tmpl]")
    for name, t in (("present", present), ("lost", lost), ("on", on)):
        if t.numel() != n or t.element_size() != 1:
            raise ValueError(f"conceal_rows_: {name} must be [N] bytes")
    for name, t, shape in (("chunk_len", chunk_len, (n,)), ("ring_len", ring_len, (n,)), ("consts", consts, (6, n)),
                           ("state", state, (n, 2))):
        if t.dtype != torch.int32 or tuple(t.shape) != shape or not t.is_contiguous():
            raise ValueError(f"conceal_rows_: {name} must be contiguous int32 {list(shape)}")
    c = [consts[i].data_ptr() for i in range(6)]
    nat.check(nat.lib().alive_conceal_rows(nat.ptr(ring), n, ld, nat.ptr(ring_len), nat.ptr(chunks), chunks.shape[1], nat.ptr(chunk_len),
                                           nat.ptr(present), nat.ptr(lost), nat.ptr(on), c[0], c[1], c[2], c[3], c[4], c[5],
                                           nat.ptr(state), nat.ptr(tmpl), tmpl.shape[1], nat.stream()), "alive_conceal_rows")
    return chunks


def check_conceal_ms(hold_ms=10.0, fade_ms=50.0, recover_ms=5.0):
    """the concealment's three durations as floats.  ValueError unless each is a finite number of milliseconds >= 0 (not a bool)"""
    out = []
    for name, v in (("conceal_hold_ms", hold_ms), ("conceal_fade_ms", fade_ms), ("conceal_recover_ms", recover_ms)):
        if not _number(v) or not (np.isfinite(v) and v >= 0):
            raise ValueError(f"{name}={v!r} must be a finite number of milliseconds >= 0")
        out.append(float(v))
    return tuple(out)


def conceal_geometry(rate, chunk_len, ring_len, hold_ms=10.0, fade_ms=50.0, recover_ms=5.0, check=True):
    """a session's concealment constants in its own samples -> (lag_lo, lag_hi, window, hold, fade, recover), the rows of
    alive_conceal_rows' consts: lags of 60 - 400 Hz (rate // 400 .. ceil(rate / 60)), a 20 ms window (rate // 50), hold =
    round(hold_ms rate / 1000), fade = max(1, round(fade_ms rate / 1000)), recover = min(round(recover_ms rate / 1000), chunk_len).
    check: ValueError (naming both numbers) unless the ring holds need = max(window + lag_hi, 2 lag_hi) samples and need fits the
    kernel's CONCEAL_MAX_SPAN"""
    hold_ms, fade_ms, recover_ms = check_conceal_ms(hold_ms, fade_ms, recover_ms)
    r, cl, rl = int(rate), int(chunk_len), int(ring_len)
    lo, hi, w = r // 400, -(-r // 60), r // 50
    hold, fade = int(round(hold_ms * r / 1000.0)), max(1, int(round(fade_ms * r / 1000.0)))
    rec = min(int(round(recover_ms * r / 1000.0)), cl)
    if max(hold, fade) > CONCEAL_QMAX:
        raise ValueError(f"conceal_hold_ms={hold_ms!r} / conceal_fade_ms={fade_ms!r} are {hold} / {fade} samples at {r} Hz: at most "
                         f"{CONCEAL_QMAX}")
    need = max(w + hi, 2 * hi)
    if check and (lo < 1 or need > CONCEAL_MAX_SPAN):
        raise ValueError(f"concealment at {r} Hz would search {need} samples (lags {lo} .. {hi}): the kernel takes lags >= 1 and at "
                         f"most {CONCEAL_MAX_SPAN} samples")
    if check and rl < need:
        raise ValueError(f"concealment at {r} Hz needs a ring of at least {need} samples (a 20 ms window of {w} and the longest lag of "
                         f"{hi}); the session's ring holds {rl} ({cl}-sample chunks): use a larger buffersize, or conceal=False")
    return lo, hi, w, hold, fade, rec


def emit_rows_(wave, span_lo, span_len, take, out):
    """alive_emit_rows: out int16 [N, ld_out] <- the spans [span_lo, span_lo + span_len) of the taken rows (take: [N] bytes) of wave
    float32 [N, ld] as alive_float_to_pcm16 forms them, zeros everywhere else"""
    n, ld = wave.shape
    if wave.dtype != torch.float32 or not wave.is_contiguous():
        raise ValueError("emit_rows_: wave must be contiguous float32 [N, ld]")
    if out.dtype != torch.int16 or out.dim() != 2 or out.shape[0] != n or take.numel() != n or take.element_size() != 1:
        raise ValueError("emit_rows_: out must be int16 [N, ld_out], take [N] bytes")
    nat.check(nat.lib().alive_emit_rows(nat.ptr(wave), n, ld, nat.ptr(span_lo), nat.ptr(span_len), nat.ptr(take), nat.ptr(out),
                                        out.shape[1], nat.stream()), "alive_emit_rows")
    return out


def seam_rows_(y, span_lo, shift, xlen, emit, tail, stored, g0=None, g1=None, stats=None):
    """alive_seam_rows in place on y [N, ld]: every emitting row's head faded from its tail, the tail of the next tick saved.
    tail float32 [N, ld_tail] and stored int32 [N] are the rows' state; g0 / g1: the gate's gains, or both None; stats: float64
    [N, 2] or None"""
    n, ld = y.shape
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("seam_rows_: y must be contiguous float32 [N, ld]")
    if tail.dtype != torch.float32 or not tail.is_contiguous() or tail.dim() != 2 or tail.shape[0] != n:
        raise ValueError("seam_rows_: tail must be contiguous float32 [N, ld_tail]")
    nat.check(nat.lib().alive_seam_rows(nat.ptr(y), n, ld, nat.ptr(span_lo), nat.ptr(shift), nat.ptr(xlen), nat.ptr(emit),
                                        nat.ptr(g0), nat.ptr(g1), nat.ptr(tail), tail.shape[1], nat.ptr(stored), nat.ptr(stats),
                                        nat.stream()), "alive_seam_rows")
    return y


def limit_rows_(y, span_lo, span_len, shift, look, hold, ceil, emit, hist, gmin=None):
    """alive_limit_rows in place on y [N, ld]: every emitting row's span limited to its ceiling with its lookahead taken one chunk on,
    hist float32 [N, ld_hist] (the rows' state: the required gains of the latest emitted samples) moved on.  gmin: float32 [N] or
    None"""
    n, ld = y.shape
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("limit_rows_: y must be contiguous float32 [N, ld]")
    if hist.dtype != torch.float32 or not hist.is_contiguous() or hist.dim() != 2 or hist.shape[0] != n:
        raise ValueError("limit_rows_: hist must be contiguous float32 [N, ld_hist]")
    nat.check(nat.lib().alive_limit_rows(nat.ptr(y), n, ld, nat.ptr(span_lo), nat.ptr(span_len), nat.ptr(shift), nat.ptr(look),
                                         nat.ptr(hold), nat.ptr(ceil), nat.ptr(emit), nat.ptr(hist), hist.shape[1], nat.ptr(gmin),
                                         nat.stream()), "alive_limit_rows")
    return y


def limit_waves_rows(y, lens, look, hold, ceil, gmin=None):
    """alive_limit_waves: y float32 [N, ld], device int32 lens [N], one look / hold in samples, device float32 ceil [N] -> a new
    tensor, row n's first lens[n] samples limited as one signal, the rest copied.  gmin: float32 [N] or None"""
    if y.dtype != torch.float32 or not y.is_contiguous() or y.dim() != 2:
        raise ValueError("limit_waves_rows: y must be contiguous float32 [N, ld]")
    n, ld = y.shape
    out = torch.empty_like(y)
    nat.check(nat.lib().alive_limit_waves(nat.ptr(out), nat.ptr(y), n, ld, nat.ptr(lens), int(look), int(hold), nat.ptr(ceil),
                                          nat.ptr(gmin), nat.stream()), "alive_limit_waves")
    return out


LIMIT_TILE, LIMIT_MAX_HIST = 1024, 3072        # ALIVE_LIMIT_TILE, ALIVE_LIMIT_MAX_HIST (include/alive_vc.h)
LIMIT_CEIL_MAX = 32767.0 / 32768.0             # the largest float sample that alive_float_to_pcm16 does not wrap


def _number(v):
    return isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, (bool, np.bool_))


def check_limit(limit_db, lookahead_ms=5.0, hold_ms=20.0):
    """a limiter's settings -> (ceiling, lookahead_ms, hold_ms) as floats, None for limit_db None (off; the two times are still
    checked).  ValueError unless limit_db is None or a finite number <= 0 (not a bool), limit_lookahead_ms a finite number > 0 and
    limit_hold_ms a finite number >= 0.  The ceiling is min(10^(dB / 20), 32767 / 32768): 0 dB still never wraps"""
    if not _number(lookahead_ms) or not (np.isfinite(lookahead_ms) and lookahead_ms > 0):
        raise ValueError(f"limit_lookahead_ms={lookahead_ms!r} must be a finite number of milliseconds > 0")
    if not _number(hold_ms) or not (np.isfinite(hold_ms) and hold_ms >= 0):
        raise ValueError(f"limit_hold_ms={hold_ms!r} must be a finite number of milliseconds >= 0")
    if limit_db is None:
        return None
    if not _number(limit_db) or not (np.isfinite(limit_db) and limit_db <= 0):
        raise ValueError(f"limit_db={limit_db!r} must be a finite number of dBFS <= 0, or None for no limiter")
    return min(10.0 ** (float(limit_db) / 20.0), LIMIT_CEIL_MAX), float(lookahead_ms), float(hold_ms)


def limit_samples(lookahead_ms, hold_ms, rate):
    """(L, H) in samples at `rate`: L = max(1, round(lookahead_ms * rate / 1000)), H = round(hold_ms * rate / 1000)"""
    return max(1, int(round(float(lookahead_ms) * rate / 1000.0))), int(round(float(hold_ms) * rate / 1000.0))


def limit_geometry(chunk_r, buffersize, rate, limit_db, lookahead_ms, hold_ms, row_len, ld_hist, shift=None):
    """a session's limiter -> (span_lo, shift, L, H, c) of alive_limit_rows: span_lo the first sample step() emits of its wave of
    row_len samples, shift the ring's advance per tick in the session's samples (default chunk_r), L and H as limit_samples forms
    them, c the ceiling; L = H = 0 and c = 1 for limit_db None (off).  ValueError (check_limit's, or one that names the largest value
    that fits) unless L <= chunk_r, span_lo + shift + L - 1 <= row_len and L - 1 + H <= ld_hist, the width of the history"""
    chunk_r, buffersize, rate, row_len, ld_hist = int(chunk_r), int(buffersize), int(rate), int(row_len), int(ld_hist)
    shift = chunk_r if shift is None else int(shift)
    lo = buffersize * chunk_r // 2 - chunk_r // 2
    checked = check_limit(limit_db, lookahead_ms, hold_ms)
    if checked is None:
        return lo, shift, 0, 0, 1.0
    c, look_ms, hold_ms_ = checked
    L, H = limit_samples(look_ms, hold_ms_, rate)
    l_max = min(chunk_r, row_len - lo - shift + 1, ld_hist + 1)
    if L > l_max:
        ms_max = max(l_max, 0) * 1000.0 / rate
        raise ValueError(f"limit_lookahead_ms={lookahead_ms!r} is {L} samples at {rate} Hz; a session with {chunk_r}-sample chunks in "
                         f"a wave of {row_len} and a history of {ld_hist} takes 1 to {max(l_max, 0)} (the largest "
                         f"limit_lookahead_ms that fits is {ms_max:g})")
    h_max = ld_hist - (L - 1)
    if H > h_max:
        raise ValueError(f"limit_hold_ms={hold_ms!r} is {H} samples at {rate} Hz; beside a lookahead of {L} a history of {ld_hist} "
                         f"takes 0 to {h_max} (the largest limit_hold_ms that fits is {h_max * 1000.0 / rate:g})")
    return lo, shift, L, H, c


def limit_history_width(limit_history, rate):
    """the width of the limiter's history, round(limit_history * rate) samples at the fastest declared rate.  ValueError unless it is
    a finite number of seconds > 0 (not a bool) and the width lies in [1, LIMIT_MAX_HIST]"""
    if not _number(limit_history) or not (np.isfinite(limit_history) and limit_history > 0):
        raise ValueError(f"limit_history={limit_history!r} must be a finite number of seconds > 0")
    width = int(round(float(limit_history) * int(rate)))
    if not 1 <= width <= LIMIT_MAX_HIST:
        raise ValueError(f"limit_history={limit_history!r} is {width} samples at {int(rate)} Hz; the limiter keeps 1 to "
                         f"{LIMIT_MAX_HIST} (the largest limit_history that fits is {LIMIT_MAX_HIST / int(rate):g})")
    return width


def gmin_db(gmin):
    """alive_limit_rows' smallest gains -> 20 log10(g) each: 0.0 for an untouched row, -inf for a gain of 0"""
    with np.errstate(divide="ignore"):
        return [float(20.0 * np.log10(np.float64(g))) if g != 1.0 else 0.0 for g in gmin]


def limit_waves(wave, lens=None, limit_db=-1.0, lookahead_ms=5.0, hold_ms=20.0, rate=16000, return_gain=False):
    """The offline limiter: wave float32 [N, ld] (or [ld]) on the device at `rate` Hz -> a new tensor of its shape, row n's first
    lens[n] samples (default: the whole row) limited as one signal to limit_db (a number, or one per row; None: the row is copied),
    the rest copied (alive_limit_waves; bitwise what a streaming session's limiter makes of the same signal).  ValueError as
    check_limit, and unless L - 1 + H <= LIMIT_MAX_HIST.  return_gain=True: also the smallest gain per row as dB (one host read)"""
    one = wave.dim() == 1
    y = (wave[None] if one else wave).contiguous()
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError(f"limit_waves: wave must be float32 [N, ld] or [ld], got {tuple(wave.shape)} {wave.dtype}")
    n, ld = y.shape
    dbs = list(limit_db) if isinstance(limit_db, (list, tuple)) else [limit_db] * n
    if len(dbs) != n:
        raise ValueError(f"limit_waves: {len(dbs)} limit_db for {n} rows")
    ceils = [check_limit(db, lookahead_ms, hold_ms) for db in dbs]
    L, H = limit_samples(lookahead_ms, hold_ms, rate)
    if L - 1 + H > LIMIT_MAX_HIST:
        raise ValueError(f"limit_waves: a lookahead of {L} and a hold of {H} samples at {rate} Hz: L - 1 + H is at most "
                         f"{LIMIT_MAX_HIST} (the largest limit_hold_ms that fits is {(LIMIT_MAX_HIST - L + 1) * 1000.0 / rate:g})")
    lens = [ld] * n if lens is None else [int(v) for v in lens]
    if len(lens) != n:
        raise ValueError(f"limit_waves: {len(lens)} lens for {n} rows")
    dev = y.device
    ceil = torch.tensor([0.0 if c is None else c[0] for c in ceils], dtype=torch.float32, device=dev)     # (0: the row is copied)
    gmin = torch.empty(n, dtype=torch.float32, device=dev) if return_gain else None
    out = limit_waves_rows(y, torch.tensor(lens, dtype=torch.int32, device=dev), L, H, ceil, gmin)
    out = out[0] if one else out
    return (out, gmin_db(gmin.tolist())) if return_gain else out


LOUDNESS_STATE, LOUDNESS_PARAMS = 16, 6         # ALIVE_LOUDNESS_STATE, ALIVE_LOUDNESS_PARAMS (include/alive_vc.h)
LOUDNESS_GATE_LUFS = -70.0                      # the standard's absolute gate
_loudness_ws = nat.Workspace()


def loudness_hop(rate):
    """the samples of a 100-ms sub-block at `rate` Hz: (rate + 5) // 10"""
    return (int(rate) + 5) // 10


def _loudness_biquad(f0, Q, fs, Vh=None):
    K = math.tan(math.pi * f0 / fs)
    a0 = 1.0 + K / Q + K * K
    a1, a2 = 2.0 * (K * K - 1.0) / a0, (1.0 - K / Q + K * K) / a0
    if Vh is None:
        return 1.0, -2.0, 1.0, a1, a2
    Vb = Vh ** 0.4996667741545416
    return (Vh + Vb * K / Q + K * K) / a0, 2.0 * (K * K - Vh) / a0, (Vh - Vb * K / Q + K * K) / a0, a1, a2


@functools.lru_cache(maxsize=None)
def loudness_filter(rate):
    """the K-weighting at `rate` Hz as the kernels take it: (coef, ap), coef = (b0, b1, b2, a1, a2) of the shelf then of the
    high-pass (the usual re-derivation of the standard's 48-kHz filter, in Python floats), ap the 16 entries of AP row by row: column k
    of AP is the state left after loudness_hop(rate) zero samples from unit state k, by the kernels' own recurrence"""
    fs = float(int(rate))
    coef = (_loudness_biquad(1681.974450955533, 0.7071752369554196, fs, 10.0 ** (3.999843853973347 / 20.0))
            + _loudness_biquad(38.13547087602444, 0.5003270373238773, fs))
    b0, b1, b2, a1, a2, d0, d1, d2, e1, e2 = coef
    cols = []
    for k in range(4):
        z = [1.0 if i == k else 0.0 for i in range(4)]
        for _ in range(loudness_hop(rate)):                   # (v = 0.0: the products stay in, as the kernels keep them)
            o1 = b0 * 0.0 + z[0]
            z[0] = (b1 * 0.0 - a1 * o1) + z[1]
            z[1] = b2 * 0.0 - a2 * o1
            o2 = d0 * o1 + z[2]
            z[2] = (d1 * o1 - e1 * o2) + z[3]
            z[3] = d2 * o1 - e2 * o2
        cols.append(z)
    return coef, tuple(cols[k][r] for r in range(4) for k in range(4))


def loudness_z(level):
    """the mean square of a loudness in LUFS: 10^((L + 0.691) / 10)"""
    return 10.0 ** ((float(level) + 0.691) / 10.0)


def loudness_lufs(z):
    """-0.691 + 10 log10(z) on the host; -inf for 0"""
    return -0.691 + 10.0 * math.log10(z) if z > 0 else -math.inf


def check_loudness(target_lufs, max_gain_db=12.0):
    """a loudness target -> (z_t, gmax) as floats, None for target_lufs None (off; max_gain_db is still checked).  ValueError unless
    target_lufs is None or a finite number (not a bool) with -70 < target_lufs <= 0, and max_gain_db a finite number >= 0: the gain
    stays within +-max_gain_db"""
    if not _number(max_gain_db) or not (np.isfinite(max_gain_db) and max_gain_db >= 0):
        raise ValueError(f"loudness max gain {max_gain_db!r} must be a finite number of dB >= 0")
    if target_lufs is None:
        return None
    if not _number(target_lufs) or not (np.isfinite(target_lufs) and LOUDNESS_GATE_LUFS < target_lufs <= 0):
        raise ValueError(f"lufs={target_lufs!r} must be a finite number of LUFS in (-70, 0], or None for no loudness normalisation")
    return loudness_z(target_lufs), 10.0 ** (float(max_gain_db) / 20.0)


def check_loudness_stream(half_life=3.0, prior=1.0, gate_lufs=LOUDNESS_GATE_LUFS, max_db=12.0, slew_db=6.0):
    """a converter's loudness settings -> (d, P, z_abs, gmax, slew_db) as floats: d = 2^(-0.1 / half_life) per 100-ms sub-block, P = 10
    * prior blocks.  ValueError unless half_life is a finite number of seconds > 0, prior one >= 0, gate_lufs finite and <= -20,
    max_db finite >= 0 and slew_db finite > 0 dB per second (none of them a bool)"""
    if not _number(half_life) or not (np.isfinite(half_life) and half_life > 0):
        raise ValueError(f"loudness_half_life={half_life!r} must be a finite number of seconds > 0")
    if not _number(prior) or not (np.isfinite(prior) and prior >= 0):
        raise ValueError(f"loudness_prior={prior!r} must be a finite number of seconds >= 0")
    if not _number(gate_lufs) or not (np.isfinite(gate_lufs) and gate_lufs <= -20):
        raise ValueError(f"loudness_gate_lufs={gate_lufs!r} must be a finite number of LUFS <= -20")
    if not _number(max_db) or not (np.isfinite(max_db) and max_db >= 0):
        raise ValueError(f"loudness_max_db={max_db!r} must be a finite number of dB >= 0")
    if not _number(slew_db) or not (np.isfinite(slew_db) and slew_db > 0):
        raise ValueError(f"loudness_slew_db={slew_db!r} must be a finite number of dB per second > 0")
    return (2.0 ** (-0.1 / float(half_life)), 10.0 * float(prior), loudness_z(gate_lufs), 10.0 ** (float(max_db) / 20.0),
            float(slew_db))


def loudness_slew(slew_db, n, rate):
    """the factor a session's gain may move by in one tick that emits n samples at `rate` Hz: 10^(slew_db (n / rate) / 20)"""
    return 10.0 ** (float(slew_db) * (int(n) / float(rate)) / 20.0)


def loudness_rows_(y, span_lo, span_len, emit, on, hop, coef, par, state):
    """alive_loudness_rows in place on y [N, ld]: every emitting row whose `on` is set has its span K-weighted into its running
    loudness and multiplied by the slewed gain towards its target; state float64 [N, LOUDNESS_STATE] moved on.  coef float64 [N, 10],
    par float64 [N, LOUDNESS_PARAMS], hop int32 [N], emit / on one byte per row"""
    n, ld = y.shape
    if y.dtype != torch.float32 or not y.is_contiguous():
        raise ValueError("loudness_rows_: y must be contiguous float32 [N, ld]")
    for name, t, w in (("coef", coef, 10), ("par", par, LOUDNESS_PARAMS), ("state", state, LOUDNESS_STATE)):
        if t.dtype != torch.float64 or not t.is_contiguous() or tuple(t.shape) != (n, w):
            raise ValueError(f"loudness_rows_: {name} must be contiguous float64 [N, {w}]")
    for name, t in (("emit", emit), ("on", on)):
        if t.element_size() != 1 or t.numel() != n:
            raise ValueError(f"loudness_rows_: {name} must hold one byte per row")
    nat.check(nat.lib().alive_loudness_rows(nat.ptr(y), n, ld, nat.ptr(span_lo), nat.ptr(span_len), nat.ptr(emit), nat.ptr(on),
                                            nat.ptr(hop), nat.ptr(coef), nat.ptr(par), nat.ptr(state), nat.stream()),
              "alive_loudness_rows")
    return y


def measure_loudness_rows(y, lens, hop, coef, ap, z_abs, max_tiles):
    """alive_loudness_measure_waves: y float32 [N, ld], device int32 lens / hop [N], float64 coef [N, 10] and ap [N, 16] -> device
    (zI float64 [N], c1 int32 [N], c2 int32 [N]); max_tiles: the most sub-blocks a row has (a row with more is not measured)"""
    if y.dtype != torch.float32 or not y.is_contiguous() or y.dim() != 2:
        raise ValueError("measure_loudness_rows: y must be contiguous float32 [N, ld]")
    n, ld = y.shape
    dev = y.device
    max_tiles = max(int(max_tiles), 1)
    L = nat.lib()
    nbytes = L.alive_loudness_workspace_bytes(n, max_tiles)
    ws = _loudness_ws.get(max(nbytes, 8), dev)
    zI = torch.empty(n, dtype=torch.float64, device=dev)
    c1, c2 = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
    nat.check(L.alive_loudness_measure_waves(nat.ptr(y), n, ld, nat.ptr(lens), nat.ptr(hop), nat.ptr(coef), nat.ptr(ap), float(z_abs),
                                             max_tiles, nat.ptr(zI), nat.ptr(c1), nat.ptr(c2), nat.ptr(ws), ws.numel(), nat.stream()),
              "alive_loudness_measure_waves")
    return zI, c1, c2


def apply_loudness_rows(y, lens, zI, c2, z_t, gmax, gain=None):
    """alive_loudness_apply_waves: a new tensor, row n's first lens[n] samples times min(max(sqrt(z_t[n] / zI[n]), 1 / gmax), gmax)
    (1 where c2[n] == 0), the rest copied; a row whose z_t is a NaN is copied bit for bit.  gain: float64 [N] or None"""
    if y.dtype != torch.float32 or not y.is_contiguous() or y.dim() != 2:
        raise ValueError("apply_loudness_rows: y must be contiguous float32 [N, ld]")
    n, ld = y.shape
    out = torch.empty_like(y)
    nat.check(nat.lib().alive_loudness_apply_waves(nat.ptr(out), nat.ptr(y), n, ld, nat.ptr(lens), nat.ptr(zI), nat.ptr(c2),
                                                   nat.ptr(z_t), float(gmax), nat.ptr(gain), nat.stream()),
              "alive_loudness_apply_waves")
    return out


def _loudness_inputs(what, wave, lens, rate):
    """the shared front of measure_loudness / normalize_loudness: (one, y, lens list, device lens, hop, coef, ap, max_tiles)"""
    one = wave.dim() == 1
    y = (wave[None] if one else wave).contiguous()
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError(f"{what}: wave must be float32 [N, ld] or [ld], got {tuple(wave.shape)} {wave.dtype}")
    n, ld = y.shape
    lens = [ld] * n if lens is None else [int(v) for v in lens]
    if len(lens) != n:
        raise ValueError(f"{what}: {len(lens)} lens for {n} rows")
    rates = list(rate) if isinstance(rate, (list, tuple)) else [rate] * n
    if len(rates) != n:
        raise ValueError(f"{what}: {len(rates)} rates for {n} rows")
    for r in rates:
        if not isinstance(r, (int, np.integer)) or isinstance(r, (bool, np.bool_)) or not 1000 <= int(r) <= 768000:
            raise ValueError(f"{what}: rate={r!r} must be a whole number of Hz in [1000, 768000]")
    dev = y.device
    filt = [loudness_filter(int(r)) for r in rates]
    hops = [loudness_hop(r) for r in rates]
    tiles = max([min(max(v, 0), ld) // h for v, h in zip(lens, hops)] + [1])
    return (one, y, lens, torch.tensor(lens, dtype=torch.int32, device=dev), torch.tensor(hops, dtype=torch.int32, device=dev),
            torch.tensor([f[0] for f in filt], dtype=torch.float64, device=dev),
            torch.tensor([f[1] for f in filt], dtype=torch.float64, device=dev), tiles)


def measure_loudness(wave, lens=None, rate=16000):
    """The integrated loudness of ITU-R BS.1770-4 (one channel, two-pass gating) of wave float32 [N, ld] (or [ld]) on the device: row
    n's first lens[n] samples (default: the whole row) at `rate` Hz (a number, or one per row) -> (LUFS per row, -inf where nothing
    passed the gates -- fewer than 400 ms, or silence --, the blocks above the absolute gate per row, the blocks above both gates
    per row), three lists (a float and two ints for a 1-d wave).  One host read"""
    one, y, _, lens_d, hop, coef, ap, tiles = _loudness_inputs("measure_loudness", wave, lens, rate)
    zI, c1, c2 = measure_loudness_rows(y, lens_d, hop, coef, ap, loudness_z(LOUDNESS_GATE_LUFS), tiles)
    zI, c1, c2 = zI.tolist(), c1.tolist(), c2.tolist()
    out = [loudness_lufs(z) if c else -math.inf for z, c in zip(zI, c2)]
    return (out[0], c1[0], c2[0]) if one else (out, c1, c2)


def normalize_loudness(wave, lens, target_lufs, rate, max_gain_db=12.0, return_gain=False):
    """Loudness normalisation: wave float32 [N, ld] (or [ld]) on the device -> a new tensor of its shape, row n's first lens[n] samples
    (None: the whole row) at `rate` Hz (a number, or one per row) times the one gain that brings their integrated loudness to
    target_lufs (a number, or one per row; None: the row is copied bit for bit), within +-max_gain_db; the rest of the row is copied.
    A row nothing of which passes the gates keeps its level (gain 1).  The gain can lift a sample above full scale: limit_waves
    belongs behind it.  ValueError as check_loudness.  return_gain=True: also the gain per row in dB (one host read; no host read
    otherwise)"""
    one, y, _, lens_d, hop, coef, ap, tiles = _loudness_inputs("normalize_loudness", wave, lens, rate)
    n = y.shape[0]
    targets = list(target_lufs) if isinstance(target_lufs, (list, tuple)) else [target_lufs] * n
    if len(targets) != n:
        raise ValueError(f"normalize_loudness: {len(targets)} target_lufs for {n} rows")
    checked = [check_loudness(t, max_gain_db) for t in targets]
    gmax = 10.0 ** (float(max_gain_db) / 20.0)
    dev = y.device
    zI, _, c2 = measure_loudness_rows(y, lens_d, hop, coef, ap, loudness_z(LOUDNESS_GATE_LUFS), tiles)
    z_t = torch.tensor([math.nan if c is None else c[0] for c in checked], dtype=torch.float64, device=dev)
    gain = torch.empty(n, dtype=torch.float64, device=dev) if return_gain else None
    out = apply_loudness_rows(y, lens_d, zI, c2, z_t, gmax, gain)
    out = out[0] if one else out
    if not return_gain:
        return out
    db = [20.0 * math.log10(g) for g in gain.tolist()]
    return out, (db[0] if one else db)


ENVELOPE_TILE, ENVELOPE_MAX_RADIUS = 16, 4      # ALIVE_ENVELOPE_TILE, ALIVE_ENVELOPE_MAX_RADIUS (include/alive_vc.h)
ENVELOPE_HOP = 320                              # the decoder's frame at 16 kHz


def envelope_waves_(out, y, x, lens, amount, hop, radius, floor_ms, g_lo, g_hi, gain_minmax=None):
    """alive_envelope_waves into out [N, ld_y]: y float32 [N, ld_y] times the gain that moves its frame levels towards those of x
    float32 [N, ld_x], row n over its first lens[n] samples (device int32 [N], or None: the whole row) at amount[n] (device float32
    [N]; a row whose amount is not in (0, 1] is copied).  gain_minmax: float32 [N, 2] or None.  out must not overlap y or x"""
    for name, t in (("out", out), ("y", y), ("x", x)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2:
            raise ValueError(f"envelope_waves_: {name} must be contiguous float32 [N, ld]")
    n, ld_y = y.shape
    if out.shape != y.shape or x.shape[0] != n:
        raise ValueError(f"envelope_waves_: out {tuple(out.shape)}, y {tuple(y.shape)} and x {tuple(x.shape)} do not belong together")
    nat.check(nat.lib().alive_envelope_waves(nat.ptr(out), nat.ptr(y), ld_y, nat.ptr(x), x.shape[1], n, nat.ptr(lens),
                                             nat.ptr(amount), int(hop), int(radius), float(floor_ms), float(g_lo), float(g_hi),
                                             nat.ptr(gain_minmax), nat.stream()), "alive_envelope_waves")
    return out


def check_envelope(amount, floor_db=-60.0, range_db=12.0, radius=1):
    """an envelope follower's settings -> (amount, floor_ms, g_lo, g_hi, radius): the amount as a float, the floor as a mean square
    10^(floor_db / 10) and the range 10^(-+range_db / 20) in float64.  ValueError unless amount is a finite number in [0, 1] (not a
    bool; 0: off), floor_db a finite number in [-3000, 3000], range_db a finite number in [0, 6000] (so that the floor is above 0 and
    the range finite in float64), and radius
    an integer in [0, ENVELOPE_MAX_RADIUS]"""
    if not _number(amount) or not (np.isfinite(amount) and 0 <= amount <= 1):
        raise ValueError(f"envelope={amount!r} must be a finite number in [0, 1] (0: the converted level as it is)")
    if not _number(floor_db) or not (np.isfinite(floor_db) and -3000 <= floor_db <= 3000):
        raise ValueError(f"envelope_floor_db={floor_db!r} must be a finite number of dB in [-3000, 3000] (its mean square is above 0)")
    if not _number(range_db) or not (np.isfinite(range_db) and 0 <= range_db <= 6000):
        raise ValueError(f"envelope_range_db={range_db!r} must be a finite number of dB >= 0 (at most 6000)")
    if isinstance(radius, (bool, np.bool_)) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= ENVELOPE_MAX_RADIUS:
        raise ValueError(f"envelope_radius={radius!r} must be an integer in [0, {ENVELOPE_MAX_RADIUS}] (frames on each side)")
    return (float(amount), float(10.0 ** (float(floor_db) / 10.0)), float(10.0 ** (-float(range_db) / 20.0)),
            float(10.0 ** (float(range_db) / 20.0)), int(radius))


def minmax_db(minmax):
    """alive_envelope_waves' smallest and largest frame gains -> (20 log10 min, 20 log10 max) per row: (0.0, 0.0) for a row that
    does not follow"""
    return [(float(20.0 * np.log10(np.float64(lo))) if lo != 1.0 else 0.0, float(20.0 * np.log10(np.float64(hi))) if hi != 1.0 else 0.0)
            for lo, hi in minmax]


def follow_envelope(wave, source, lens=None, amount=1.0, floor_db=-60.0, range_db=12.0, radius=1):
    """The offline envelope follow: wave float32 [N, ld] (or [ld]) on the device, the conversion of `source` float32 [N, ld_x] (or
    [ld_x]) that lies beside it sample for sample at 16 kHz -> a new tensor of wave's shape, row n's first lens[n] samples (default:
    as many as both rows hold) at the source's loudness contour, the rest copied (alive_envelope_waves).  amount: a number in [0, 1],
    or one per row (0: the row is copied).  ValueError as check_envelope"""
    one = wave.dim() == 1
    y = (wave[None] if one else wave).contiguous()
    x = (source[None] if source.dim() == 1 else source).contiguous()
    if y.dim() != 2 or y.dtype != torch.float32 or x.dim() != 2 or x.dtype != torch.float32 or x.shape[0] != y.shape[0]:
        raise ValueError(f"follow_envelope: wave and source must be float32 [N, ld] or [ld] with the same N, got "
                         f"{tuple(wave.shape)} {wave.dtype} and {tuple(source.shape)} {source.dtype}")
    if x.device != y.device:
        raise ValueError(f"follow_envelope: wave on {y.device}, source on {x.device}")
    n, ld = y.shape
    amounts = list(amount) if isinstance(amount, (list, tuple)) else [amount] * n
    if len(amounts) != n:
        raise ValueError(f"follow_envelope: {len(amounts)} amounts for {n} rows")
    checked = [check_envelope(a, floor_db, range_db, radius) for a in amounts]
    _, floor_ms, g_lo, g_hi, radius = checked[0]
    cap = min(ld, x.shape[1])
    lens = [cap] * n if lens is None else [int(v) for v in lens]
    if len(lens) != n:
        raise ValueError(f"follow_envelope: {len(lens)} lens for {n} rows")
    dev = y.device
    out = envelope_waves_(torch.empty_like(y), y, x, torch.tensor(lens, dtype=torch.int32, device=dev),
                          torch.tensor([c[0] for c in checked], dtype=torch.float32, device=dev), ENVELOPE_HOP, radius, floor_ms,
                          g_lo, g_hi)
    return out[0] if one else out


POSTFILTER_TAPS, POSTFILTER_MAX_ORDER, POSTFILTER_TILE = 128, 32, 16     # ALIVE_POSTFILTER_* (include/alive_vc.h)
POSTFILTER_HOP = 320                            # the decoder's frame at 16 kHz
POSTFILTER_MAX_ALPHA = 0.85                     # the poles lie inside radius alpha: beyond it 128 taps are no longer the whole response


def postfilter_window(window):
    """the analysis window alive_postfilter_waves takes, int16 [window] on the host: a Hamming window on the half-sample grid in
    units of 1/64 (tools/postfilter_ref.py window_table)"""
    i = np.arange(int(window), dtype=np.float64)
    return np.rint(64.0 * (0.54 - 0.46 * np.cos(2.0 * np.pi * (i + 0.5) / float(window)))).astype(np.int16)


def postfilter_lag(order):
    """the lag window alive_postfilter_waves takes, float64 [order + 1] on the host: a 60 Hz Gaussian at 16 kHz
    (tools/postfilter_ref.py lag_table)"""
    k = np.arange(int(order) + 1, dtype=np.float64)
    return np.exp(-0.5 * (2.0 * np.pi * 60.0 * k / 16000.0) ** 2)


def postfilter_tables(window, order, device):
    """(win int16 [window], lag float64 [order + 1]) on the device"""
    return (torch.from_numpy(postfilter_window(window)).to(device), torch.from_numpy(postfilter_lag(order)).to(device))


def postfilter_waves_(out, y, lens, alpha, hop, window, order, win, lag, ratio, tilt, floor_ms, g_lo, g_hi, gain_minmax=None):
    """alive_postfilter_waves into out [N, ld]: y float32 [N, ld] through the adaptive formant post filter, row n over its first lens[n]
    samples (device int32 [N], or None: the whole row) at alpha[n] (device float32 [N]; a row whose alpha is not in (0, 0.85] is
    copied).  win int16 [window] and lag float64 [order + 1]: postfilter_tables.  gain_minmax: float32 [N, 2] or None.  out must not
    overlap y"""
    for name, t in (("out", out), ("y", y)):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.dim() != 2:
            raise ValueError(f"postfilter_waves_: {name} must be contiguous float32 [N, ld]")
    if out.shape != y.shape:
        raise ValueError(f"postfilter_waves_: out {tuple(out.shape)} and y {tuple(y.shape)} do not belong together")
    if win.dtype != torch.int16 or win.numel() != int(window) or lag.dtype != torch.float64 or lag.numel() != int(order) + 1:
        raise ValueError(f"postfilter_waves_: win must be int16 [{window}] and lag float64 [{int(order) + 1}]")
    n, ld = y.shape
    nat.check(nat.lib().alive_postfilter_waves(nat.ptr(out), nat.ptr(y), ld, n, nat.ptr(lens), nat.ptr(alpha), int(hop), int(window),
                                               int(order), nat.ptr(win), nat.ptr(lag), float(ratio), float(tilt), float(floor_ms),
                                               float(g_lo), float(g_hi), nat.ptr(gain_minmax), nat.stream()), "alive_postfilter_waves")
    return out


def check_post_filter(alpha, ratio=0.625, tilt=0.5, order=16, window_ms=40.0, floor_db=-100.0, range_db=12.0):
    """a post filter's settings -> (alpha, ratio, tilt, order, window, floor_ms, g_lo, g_hi): alpha, ratio and tilt as floats, the
    window in samples at 16 kHz, the floor as a mean square 10^(floor_db / 10) and the range 10^(-+range_db / 20) in float64.
    ValueError unless alpha is a finite number in [0, 0.85] (not a bool; 0: off), ratio and tilt finite numbers in [0, 1], order an
    integer in [1, POSTFILTER_MAX_ORDER], window_ms a number whose 16 samples per millisecond are a whole even number in [320, 1024]
    (the frame of 320 plus an even excess), floor_db a finite number in [-3000, 3000] and range_db one in [0, 6000]"""
    if not _number(alpha) or not (np.isfinite(alpha) and 0 <= alpha <= POSTFILTER_MAX_ALPHA):
        raise ValueError(f"post_filter={alpha!r} must be a finite number in [0, {POSTFILTER_MAX_ALPHA}] (0: the converted wave as it is)")
    if not _number(ratio) or not (np.isfinite(ratio) and 0 <= ratio <= 1):
        raise ValueError(f"post_filter_ratio={ratio!r} must be a finite number in [0, 1] (the numerator's alpha over the denominator's)")
    if not _number(tilt) or not (np.isfinite(tilt) and 0 <= tilt <= 1):
        raise ValueError(f"post_filter_tilt={tilt!r} must be a finite number in [0, 1] (the share of the tilt taken out)")
    if isinstance(order, (bool, np.bool_)) or not isinstance(order, (int, np.integer)) or not 1 <= order <= POSTFILTER_MAX_ORDER:
        raise ValueError(f"post_filter_order={order!r} must be an integer in [1, {POSTFILTER_MAX_ORDER}]")
    window = float(window_ms) * 16.0 if _number(window_ms) and np.isfinite(window_ms) else -1.0
    if window != int(window) or not POSTFILTER_HOP <= window <= 1024 or int(window) % 2:
        raise ValueError(f"post_filter_window_ms={window_ms!r} must be a number of milliseconds in [20, 64] that is a whole even number "
                         "of samples at 16 kHz")
    if not _number(floor_db) or not (np.isfinite(floor_db) and -3000 <= floor_db <= 3000):
        raise ValueError(f"post_filter_floor_db={floor_db!r} must be a finite number of dB in [-3000, 3000] (its mean square is above 0)")
    if not _number(range_db) or not (np.isfinite(range_db) and 0 <= range_db <= 6000):
        raise ValueError(f"post_filter_range_db={range_db!r} must be a finite number of dB >= 0 (at most 6000)")
    return (float(alpha), float(ratio), float(tilt), int(order), int(window), float(10.0 ** (float(floor_db) / 10.0)),
            float(10.0 ** (-float(range_db) / 20.0)), float(10.0 ** (float(range_db) / 20.0)))


def post_filter(wave, lens=None, alpha=0.8, ratio=0.625, tilt=0.5, order=16, window_ms=40.0, floor_db=-100.0, range_db=12.0):
    """The offline post filter: wave float32 [N, ld] (or [ld]) on the device at 16 kHz -> a new tensor of wave's shape, row n's first
    lens[n] samples (default: the whole row) through the adaptive formant post filter, the rest copied (alive_postfilter_waves).
    alpha: a number in [0, 0.85], or one per row (0: the row is copied).  ValueError as check_post_filter"""
    one = wave.dim() == 1
    y = (wave[None] if one else wave).contiguous()
    if y.dim() != 2 or y.dtype != torch.float32:
        raise ValueError(f"post_filter: wave must be float32 [N, ld] or [ld], got {tuple(wave.shape)} {wave.dtype}")
    n, ld = y.shape
    alphas = list(alpha) if isinstance(alpha, (list, tuple)) else [alpha] * n
    if len(alphas) != n:
        raise ValueError(f"post_filter: {len(alphas)} alphas for {n} rows")
    checked = [check_post_filter(a, ratio, tilt, order, window_ms, floor_db, range_db) for a in alphas]
    _, ratio, tilt, order, window, floor_ms, g_lo, g_hi = checked[0]
    lens = [ld] * n if lens is None else [int(v) for v in lens]
    if len(lens) != n:
        raise ValueError(f"post_filter: {len(lens)} lens for {n} rows")
    dev = y.device
    win, lag = postfilter_tables(window, order, dev)
    out = postfilter_waves_(torch.empty_like(y), y, torch.tensor(lens, dtype=torch.int32, device=dev),
                            torch.tensor([c[0] for c in checked], dtype=torch.float32, device=dev), POSTFILTER_HOP, window, order, win,
                            lag, ratio, tilt, floor_ms, g_lo, g_hi)
    return out[0] if one else out


def wave_length(frames, rate):
    """the samples of a converter's final wave: the decoder's 320 per frame at 16 kHz, resampled to `rate`"""
    orig, new = audio_io._reduced(16000, rate)
    return 320 * int(frames) if orig == new else int(nat.lib().alive_resample_length(320 * int(frames), orig, new))


def stats_db(stats):
    """alive_seam_rows' (d2, e2) pairs -> 10 log10(d2 / e2) each; nan for a row that did not fade (or whose head was all zero)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        return [float(10.0 * np.log10(np.float64(d2) / np.float64(e2))) if e2 > 0 else float("nan") for d2, e2 in stats]


def check_crossfade_ms(crossfade_ms):
    """a crossfade in milliseconds as a float, None for off.  ValueError unless it is None or a finite number > 0 (not a bool)"""
    if crossfade_ms is None:
        return None
    if isinstance(crossfade_ms, (bool, np.bool_)) or not isinstance(crossfade_ms, (int, float, np.integer, np.floating)) or not (
            np.isfinite(crossfade_ms) and crossfade_ms > 0):
        raise ValueError(f"crossfade_ms={crossfade_ms!r} must be a finite number of milliseconds > 0, or None for no crossfade")
    return float(crossfade_ms)


def seam_geometry(chunk_r, buffersize, rate, crossfade_ms, row_len):
    """a session's crossfade -> (span_lo, shift, X) of alive_seam_rows: span_lo the first sample step() emits of its wave of
    row_len samples, shift = chunk_r (the ring's advance per tick in the session's samples -- not the span length, 2 * (chunk_r //
    2)), X = round(crossfade_ms * rate / 1000), 0 for crossfade_ms None (off).  ValueError unless crossfade_ms is a finite number
    > 0 (not a bool) with 1 <= X <= the span length and span_lo + shift + X <= row_len"""
    chunk_r, buffersize, rate, row_len = int(chunk_r), int(buffersize), int(rate), int(row_len)
    lo, span = buffersize * chunk_r // 2 - chunk_r // 2, 2 * (chunk_r // 2)
    if check_crossfade_ms(crossfade_ms) is None:
        return lo, chunk_r, 0
    x = int(round(float(crossfade_ms) * rate / 1000.0))
    x_max = min(span, row_len - lo - chunk_r)
    if not 1 <= x <= x_max:
        ms_max = max(x_max, 0) * 1000.0 / rate
        raise ValueError(f"crossfade_ms={crossfade_ms!r} is {x} samples at {rate} Hz; a session with {chunk_r}-sample chunks in a "
                         f"wave of {row_len} takes 1 to {max(x_max, 0)} (the largest crossfade_ms that fits is {ms_max:g})")
    return lo, chunk_r, x


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


class RateTable:
    """rate pairs (orig_freq, new_freq) -> the device pair table of alive_resample_rows_multi: int32 [n][4] entries
    {orig, new, width, offset} (the rates divided by their gcd) and one concatenated filter buffer holding every pair's bank at its
    offset, each filled by alive_resample_filter (bitwise the bank audio_io.resample and resample_rows use).  lds_bytes is the
    largest bank of at most 16 KB: the rows at those pairs stage their bank in LDS."""

    def __init__(self, pairs, device="cuda"):
        L_ = nat.lib()
        self.device = torch.device(device)
        self.index, entries, off, lds = {}, [], 0, 0
        for o, n in pairs:
            key = audio_io._reduced(o, n)
            if key in self.index:
                continue
            orig, new = key
            if orig == new:
                entries.append((1, 1, 0, 0))
            else:
                taps = int(L_.alive_resample_taps(orig, new))
                entries.append((orig, new, (taps - orig) // 2, off))
                bank = new * taps
                if bank * 4 <= 16 * 1024:
                    lds = max(lds, bank * 4)
                off += bank
            self.index[key] = len(entries) - 1
        if not entries:
            raise ValueError("RateTable: no rate pairs")
        self.entries = entries
        self.filt = torch.empty(max(off, 1), dtype=torch.float32, device=self.device)
        for orig, new, _, o in entries:
            if orig != new:
                nat.check(L_.alive_resample_filter(orig, new, self.filt[o].data_ptr(), nat.stream()), "alive_resample_filter")
        self.filt_len = off
        self.lds_bytes = lds
        self.table = torch.tensor(entries, dtype=torch.int32, device=self.device).contiguous()
        torch.cuda.current_stream(self.device).synchronize()

    def pair(self, orig_freq, new_freq):
        """the table index of a rate pair"""
        return self.index[audio_io._reduced(orig_freq, new_freq)]


def resample_rows_multi(x, lens_in, pairs, table, lens_out, ld_out, pre, post):
    """x [B, ld_in], row b resampled at its own pair -> y [B, ld_out]: row b is resample_rows of x[b, :lens_in[b]] at the RateTable
    pair pairs[b], cut to lens_out[b] samples, and zero after them.  lens_in, pairs, lens_out: device int32 [B]; pre / post: device
    float32 [B] linear gains.  The caller keeps lens_in[b] <= ld_in and lens_out[b] <= min(ld_out, the pair's resampled length)."""
    x = x.contiguous()
    b, ld_in = x.shape
    y = torch.empty(b, int(ld_out), device=x.device)
    nat.check(nat.lib().alive_resample_rows_multi(nat.ptr(x), b, ld_in, nat.ptr(lens_in), nat.ptr(pairs), nat.ptr(table.table),
                                                  len(table.entries), nat.ptr(table.filt), table.filt_len, table.lds_bytes,
                                                  nat.ptr(pre), nat.ptr(post), nat.ptr(y), int(ld_out), nat.ptr(lens_out), nat.stream()),
              "alive_resample_rows_multi")
    return y


def _geometry(chunk, buffersize, sr):
    """realtime_inference.py:122-126 at one rate: (ring length at 16 kHz, frames, internal chunk)"""
    return -(-16000 * chunk * buffersize // sr), ring_geometry(chunk, buffersize, sr, sr)[2], int(chunk * (16000 / sr))


def session_geometry(chunk, buffersize, sr, rate):
    """a session at `rate` in a converter of `chunk` samples at `sr`: its chunk, chunk * rate / sr samples.  ValueError unless
    that is a whole number of samples and the session's 16 kHz geometry -- the resampled ring length ceil(16000 * ring / rate),
    the frame count and int(chunk_r * (16000 / rate)) -- is the converter's, each checked on its own."""
    chunk, buffersize, sr, rate = int(chunk), int(buffersize), int(sr), int(rate)
    if rate <= 0:
        raise ValueError(f"sample rate {rate} must be > 0")
    if (chunk * rate) % sr:
        raise ValueError(f"a session at {rate} Hz would take chunks of {chunk} * {rate} / {sr} = {chunk * rate / sr:g} samples: "
                         "not a whole number")
    c = chunk * rate // sr
    mine, want = _geometry(c, buffersize, rate), _geometry(chunk, buffersize, sr)
    for what, a, w in zip(("16 kHz ring length", "frame count", "internal chunk"), mine, want):
        if a != w:
            raise ValueError(f"a session at {rate} Hz ({c}-sample chunks) has a {what} of {a}, the converter's is {w}: its "
                             "geometry must be the converter's")
    return c


def auto_constants(tick_seconds, buffersize, half_life=10.0, prior_seconds=0.5):
    """(decay, prior) of alive_pitch_follow_rows for a converter whose tick lasts tick_seconds: decay = 2^(-tick / half_life), 1 for
    half_life None (never forget); prior = prior_seconds of voiced speech * 50 frames/s * buffersize, because every frame stays in
    the ring for buffersize ticks and is counted each time.  The defaults are design choices, not measurements."""
    decay = 1.0 if half_life is None else float(2.0 ** (-float(tick_seconds) / float(half_life)))
    return decay, float(prior_seconds) * 50.0 * int(buffersize)


def db_scale(db):
    """torchaudio.functional.gain's factor as audio_io.resample forms it (1.0 exactly at 0 dB)"""
    return float(10 ** (db / 20)) if db != 0 else 1.0


_PARAMS = ("voice", "pitch", "f0_rate", "alpha", "gain", "input_gain", "world_pitch", "k", "auto_pitch", "gate_db", "gate_hold",
           "crossfade_ms", "limit_db", "limit_lookahead_ms", "limit_hold_ms", "envelope", "conceal", "intonation", "auto_range",
           "pitch_track", "track_weight", "track_jump", "lufs", "voicing", "voicing_on", "voicing_off", "voicing_floor_db",
           "match_path", "path_weight", "post_filter")


class MultiStreamConverter:
    auto_pitch = False                 # (set per converter in __init__: whether the tick carries the auto-pitch kernel)
    pitch_range = False                # (likewise: whether that kernel is the three-moment follower and the transform the centred one)
    gate = False                       # (likewise: whether the tick carries the two gate kernels)
    crossfade = False                  # (likewise: whether the tick carries the seam kernel)
    limiter = False                    # (likewise: whether the tick carries the limiter kernel)
    sparse = False                     # (likewise: whether the rings live on the device and sessions may sit ticks out)
    envelope = False                   # (likewise: whether the tick carries the envelope kernel)
    conceal = False                    # (likewise: whether lost chunks are concealed in front of the ring push; needs sparse)
    pitch_track = False                # (likewise: whether the f0 branch stores the class scores and carries the tracker kernel)
    loud = False                       # (likewise: whether the tick carries the loudness kernel; loudness() is the read-back)
    voicing = False                    # (likewise: whether the f0 branch carries the voicing kernels; voicing_state() is the read-back)
    match_path = False                 # (likewise: whether the path call sits between the search and the gather; path_moved() reads back)
    post_filter = False                # (likewise: whether the tick carries the post filter kernel; post_filter_db() is the read-back)

    def __init__(self, content_encoder, f0_estimator, decoder, pool, slots, chunk=960, buffersize=8, input_sr=16000,
                 output_sr=16000, k=4, device="cuda", rates=None, world_pitch=False, blend=1, k_max=None, auto_pitch=False,
                 auto_pitch_half_life=10.0, auto_pitch_prior=0.5, gate=False, gate_lookahead=None, crossfade=False,
                 limiter=False, limit_history=0.05, sparse=False, envelope=False, envelope_floor_db=-60.0,
                 envelope_range_db=12.0, envelope_radius=1, conceal=False, conceal_hold_ms=10.0, conceal_fade_ms=50.0,
                 conceal_recover_ms=5.0, pitch_range=False, pitch_range_max=2.0, pitch_track=False, track_lo=50, track_hi=1100,
                 track_band=2.0, loudness=False, loudness_half_life=3.0, loudness_prior=1.0, loudness_gate_lufs=LOUDNESS_GATE_LUFS,
                 loudness_max_db=12.0, loudness_slew_db=6.0, voicing=False, voicing_lo=common.VOICING_LO, voicing_hi=common.VOICING_HI,
                 voicing_window_ms=common.VOICING_WINDOW_MS, voicing_bridge=common.VOICING_BRIDGE,
                 voicing_min_run=common.VOICING_MIN_RUN, match_path=False, post_filter=False, post_filter_ratio=0.625,
                 post_filter_tilt=0.5, post_filter_order=16, post_filter_window_ms=40.0):
        if not isinstance(post_filter, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: post_filter must be a bool, got {post_filter!r}")
        if post_filter:                    # (checked before anything is built)
            try:
                pf = check_post_filter(0.0, post_filter_ratio, post_filter_tilt, post_filter_order, post_filter_window_ms)
            except ValueError as e:
                raise ValueError(f"MultiStreamConverter: {e}") from None
        if not isinstance(match_path, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: match_path must be a bool, got {match_path!r}")
        if not isinstance(voicing, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: voicing must be a bool, got {voicing!r}")
        if voicing:                        # (checked before anything is built)
            voicing_opts = common.voicing_options(dict(lo=voicing_lo, hi=voicing_hi, window_ms=voicing_window_ms, bridge=voicing_bridge,
                                                       min_run=voicing_min_run), "MultiStreamConverter")
        if not isinstance(loudness, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: loudness must be a bool, got {loudness!r}")
        if loudness:                       # (checked before anything is built)
            try:
                loud = check_loudness_stream(loudness_half_life, loudness_prior, loudness_gate_lufs, loudness_max_db,
                                             loudness_slew_db)
            except ValueError as e:
                raise ValueError(f"MultiStreamConverter: {e}") from None
        if not isinstance(pitch_track, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: pitch_track must be a bool, got {pitch_track!r}")
        if pitch_track:                    # (checked before anything is built)
            try:
                common.pitch_track_tables(track_lo, track_hi, track_band)
            except ValueError as e:
                raise ValueError(f"MultiStreamConverter: {e}") from None
        if not isinstance(pitch_range, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: pitch_range must be a bool, got {pitch_range!r}")
        try:
            pitch_range_max = check_range_max(pitch_range_max)
        except ValueError as e:
            raise ValueError(f"MultiStreamConverter: {e}") from None
        if not isinstance(conceal, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: conceal must be a bool, got {conceal!r}")
        if conceal:                        # (checked before anything is built)
            if not (isinstance(sparse, (bool, np.bool_)) and sparse):
                raise ValueError("MultiStreamConverter: conceal=True needs sparse=True: lost chunks are concealed in the device rings "
                                 "of a sparse converter")
            try:
                conceal_ms = check_conceal_ms(conceal_hold_ms, conceal_fade_ms, conceal_recover_ms)
            except ValueError as e:
                raise ValueError(f"MultiStreamConverter: {e}") from None
        if not isinstance(envelope, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: envelope must be a bool, got {envelope!r}")
        if envelope:                       # (checked before anything is built)
            try:
                env = check_envelope(0.0, envelope_floor_db, envelope_range_db, envelope_radius)
            except ValueError as e:
                raise ValueError(f"MultiStreamConverter: {e}") from None
        if not isinstance(sparse, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: sparse must be a bool, got {sparse!r}")
        if not isinstance(limiter, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: limiter must be a bool, got {limiter!r}")
        if limiter:                        # (checked before anything is built)
            try:
                ld_hist = limit_history_width(limit_history, max([int(r) for r in (rates or ())] + [int(output_sr)]))
            except ValueError as e:
                raise ValueError(f"MultiStreamConverter: {e}") from None
        if not isinstance(crossfade, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: crossfade must be a bool, got {crossfade!r}")
        if crossfade and input_sr != output_sr:
            raise ValueError(f"MultiStreamConverter: crossfade=True needs input_sr == output_sr (got {input_sr} and {output_sr}): "
                             "the ring's advance per tick is otherwise not a whole number of output samples")
        if not isinstance(gate, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: gate must be a bool, got {gate!r}")
        if gate_lookahead is not None and (isinstance(gate_lookahead, (bool, np.bool_)) or not isinstance(
                gate_lookahead, (int, float, np.integer, np.floating)) or not (np.isfinite(gate_lookahead) and gate_lookahead >= 0)):
            raise ValueError(f"MultiStreamConverter: gate_lookahead={gate_lookahead!r} must be >= 0 seconds, or None (one chunk)")
        if not isinstance(auto_pitch, (bool, np.bool_)):
            raise ValueError(f"MultiStreamConverter: auto_pitch must be a bool, got {auto_pitch!r}")
        if auto_pitch_half_life is not None and not (np.isfinite(auto_pitch_half_life) and auto_pitch_half_life > 0):
            raise ValueError(f"MultiStreamConverter: auto_pitch_half_life={auto_pitch_half_life!r} must be > 0 seconds, or None")
        if not (np.isfinite(auto_pitch_prior) and auto_pitch_prior >= 0):
            raise ValueError(f"MultiStreamConverter: auto_pitch_prior={auto_pitch_prior!r} must be >= 0 seconds")
        if not 1 <= int(k) <= MAX_K:
            raise ValueError(f"MultiStreamConverter: k={k} outside [1, {MAX_K}] (the grouped search keeps k <= 8)")
        if match_path and k_max is None:   # the path call reads and the gathers after it take a k per row: the per-row-k entry points
            k_max = int(k)
        if k_max is not None:
            k_max = check_k(k_max, "MultiStreamConverter: k_max")
            if k_max < int(k):
                raise ValueError(f"MultiStreamConverter: k_max={k_max} is below the converter's k={int(k)}")
        if int(slots) < 1 or int(slots) > MAX_ROWS:
            raise ValueError(f"MultiStreamConverter: slots={slots} outside [1, {MAX_ROWS}]")
        if isinstance(blend, (bool, np.bool_)) or not isinstance(blend, (int, np.integer)) or not 1 <= blend <= MAX_BLEND:
            raise ValueError(f"MultiStreamConverter: blend={blend!r} outside [1, {MAX_BLEND}]")
        if int(slots) * int(blend) > MAX_ROWS:
            raise ValueError(f"MultiStreamConverter: slots * blend = {int(slots) * int(blend)} list rows, the grouped search takes "
                             f"at most {MAX_ROWS}")
        rates = sorted({int(r) for r in (rates or ())} | {int(input_sr)})
        if len(rates) > 1:
            if input_sr != output_sr:
                raise ValueError(f"MultiStreamConverter: per-session rates {rates} need input_sr == output_sr (got {input_sr} and "
                                 f"{output_sr}): a session's chunk could not then last as long as the converter's on both sides, so "
                                 "its internal chunk and its frame count could not both be the converter's")
            chunks = {r: session_geometry(chunk, buffersize, input_sr, r) for r in rates}
        self.device = torch.device(device)
        self.ce, self.pe, self.dec = prepare_networks(content_encoder, f0_estimator, decoder, device)
        self.pool = pool
        self.B, self.k = int(slots), int(k)
        self.k_max = k_max                 # None: every session at k (the uniform entry points); K: sessions at their own k <= K
        # a reserved pool (VoicePool(capacity=...)): the slots hold their voices, and the tick follows the pool's layout
        self._reserved = getattr(pool, "capacity", None) is not None
        self._label = f"MultiStreamConverter(slots={self.B}) at {id(self):#x}"
        self._names = [()] * self.B
        self._seen_layout = pool.layout if self._reserved else None
        self._seen_mutations = 0
        self.chunk, self.buffersize = int(chunk), int(buffersize)
        self.input_sr, self.output_sr = input_sr, output_sr
        self.begin_of_output, self.end_of_output, self.frames = ring_geometry(chunk, buffersize, input_sr, output_sr)
        B, dev = self.B, self.device
        self.n = self.chunk * self.buffersize
        self.rates = tuple(rates)
        # per-slot state: host side
        self.is_open = [False] * B
        self.params = [None] * B
        self.count = [0] * B
        self.rate = [int(input_sr)] * B
        self.slot_chunk = [self.chunk] * B
        self._rt = None
        ld_in = self.n
        if len(rates) > 1:
            # the multi-rate edges (alive_resample_rows_multi): every rate's pair into and out of 16 kHz in one table, rings padded
            # to the longest session ring; row b's lengths and pairs are device arrays written by open / close
            self._chunks = chunks
            self._rt = RateTable([(r, 16000) for r in rates] + [(16000, r) for r in rates], dev)
            self._len16 = _geometry(self.chunk, self.buffersize, input_sr)[0]          # the ring at 16 kHz, every session's
            self._lw = 320 * (self._len16 // 320)                                     # the decoder's wave: 320 per frame
            L_ = nat.lib()
            self._lout = {r: int(L_.alive_resample_length(self._lw, *audio_io._reduced(16000, r))) for r in rates}
            ld_in = max(c * self.buffersize for c in chunks.values())
            self._ld_out = max(self._lout.values())
            i32 = dict(dtype=torch.int32, device=dev)
            self.len_in = torch.full((B,), self.n, **i32)
            self.pair_in = torch.full((B,), self._rt.pair(input_sr, 16000), **i32)
            self.pair_out = torch.full((B,), self._rt.pair(16000, input_sr), **i32)
            self.len_out = torch.full((B,), self._lout[int(input_sr)], **i32)
            self._len16_rows = torch.full((B,), self._len16, **i32)
            self._lw_rows = torch.full((B,), self._lw, **i32)
        self.ld_in = ld_in
        self.ring = np.zeros((B, ld_in), dtype=np.int16)
        # per-slot state: device arrays the (captured) step reads.  blend = S > 1: slot b owns the S list rows b*S .. b*S+S-1 of
        # the grouped search (unused ones at seg_len 0) with their weights; first = [0, S, 2S, ...] is fixed
        self.S = int(blend)
        self.seg_lo = torch.zeros(B * self.S, dtype=torch.int32, device=dev)
        self.seg_len = torch.zeros(B * self.S, dtype=torch.int32, device=dev)
        if self.S > 1:
            self.first = torch.arange(0, B * self.S + 1, self.S, dtype=torch.int32, device=dev)
            self.weight = torch.zeros(B * self.S, dtype=torch.float64, device=dev)
        if self.k_max is not None:         # the slot's k, and (blend) the same on each of its list rows for the search
            self.k_rows = torch.full((B,), self.k, dtype=torch.int32, device=dev)
            self.k_lists = self.k_rows if self.S == 1 else torch.full((B * self.S,), self.k, dtype=torch.int32, device=dev)
        # match_path: the path call (csrc/match_path.hip) sits between the search and the gather and is part of the tick (captured
        # once); per list row, path_on selects ONE of the frame's k_rows candidates per frame by a Viterbi path over the ring's frames,
        # at the session's weight, and gather_k -- 1 where the path is on, the slot's k otherwise -- is what the gather reads beside
        # k_rows.  No state: the call is a function of the tick's lists.
        self.match_path = bool(match_path)
        if self.match_path:
            self.gather_k = torch.full((B,), self.k, dtype=torch.int32, device=dev)
            self.path_on = torch.zeros(B * self.S, dtype=torch.int32, device=dev)
            self.path_weight = torch.full((B * self.S,), common.PATH_WEIGHT, dtype=torch.float64, device=dev)
            self.path_moved_rows = torch.zeros(B * self.S, dtype=torch.int32, device=dev)
            self._path_moved_tick = torch.zeros(B * self.S, dtype=torch.int32, device=dev)      # (a sparse converter's: the call's own)
        self.alpha = torch.zeros(B, dtype=torch.float64, device=dev)
        self.f0_rate = torch.ones(B, dtype=torch.float32, device=dev)
        self.pitch = torch.zeros(B, dtype=torch.float32, device=dev)
        self.intonation = torch.ones(B, dtype=torch.float32, device=dev)
        self.in_pre = torch.ones(B, dtype=torch.float32, device=dev)
        self.in_post = torch.ones(B, dtype=torch.float32, device=dev)       # input gain: after the resampler (:146-147)
        self.out_pre = torch.ones(B, dtype=torch.float32, device=dev)       # output gain: before the resampler (:173-175)
        self.out_post = torch.ones(B, dtype=torch.float32, device=dev)
        if not sparse:                     # the slots whose phase advances this tick (sparse: a row of the flags array, below)
            self.emit = torch.zeros(B, 1, dtype=torch.bool, device=dev)
        # world_pitch: the masked WORLD branch is part of the tick (captured once); per row, world_on selects WORLD's f0 and the
        # transform's rate is f0_rate_eff: the session's f0_rate, 1.0 on a WORLD row (its f0_rate stays in its params)
        self.world_pitch = bool(world_pitch)
        if self.world_pitch:
            self.world_on = torch.zeros(B, dtype=torch.int32, device=dev)
            self._world_sel = torch.zeros(B, 1, 1, dtype=torch.bool, device=dev)
            self.f0_rate_eff = torch.ones(B, dtype=torch.float32, device=dev)
        # auto_pitch: the follow kernel is part of the tick (captured once); per row, auto_on selects pitch + the automatic shift
        # towards `target`, and the transform reads shift_eff.  reg_state is the session's running source register, like phi
        # pitch_range: the follower is alive_pitch_follow2_rows on reg_state [B, 3] = (S, W, Q) and the transform the centred one;
        # per row, `intonation` scales the excursions around the running mean and range_on maps the running standard deviation onto
        # target_sd.  Such a converter serves auto_pitch sessions too: everything that carries reg_state carries its third column
        self.pitch_range = bool(pitch_range)
        self.auto_pitch = bool(auto_pitch) or self.pitch_range
        if self.auto_pitch:
            self.auto_decay, self.auto_prior = auto_constants(self.chunk / input_sr, self.buffersize, auto_pitch_half_life,
                                                              auto_pitch_prior)
            self.auto_on = torch.zeros(B, dtype=torch.int32, device=dev)
            self.target = torch.zeros(B, dtype=torch.float32, device=dev)
            self.reg_state = torch.zeros(B, 3 if self.pitch_range else 2, dtype=torch.float64, device=dev)
            self.shift_eff = torch.zeros(B, dtype=torch.float32, device=dev)
        if self.pitch_range:
            self.range_max = pitch_range_max
            self.range_on = torch.zeros(B, dtype=torch.int32, device=dev)
            self.target_sd = torch.zeros(B, dtype=torch.float64, device=dev)
            self.inton_eff = torch.ones(B, dtype=torch.float32, device=dev)
            self.centre = torch.zeros(B, dtype=torch.float32, device=dev)
            self.centre_on = torch.zeros(B, dtype=torch.int32, device=dev)
        # pitch_track: the f0 branch stores the class scores and the tracker kernel is part of the tick (captured once); per row,
        # track_on selects the Viterbi path over the scores instead of their argmax, at the session's weight and jump.  No state: the
        # whole ring is decoded again every tick.  The logits buffer is allocated once per shape, by the first tick
        self.pitch_track = bool(pitch_track)
        if self.pitch_track:
            self._track = common.pitch_track(track_lo, track_hi, track_band, dev)
            self.track_on = torch.zeros(B, dtype=torch.int32, device=dev)
            self.track_weight = torch.full((B,), common.TRACK_WEIGHT, dtype=torch.float64, device=dev)
            self.track_jump = torch.full((B,), common.TRACK_JUMP, dtype=torch.float64, device=dev)
            self.track_changed = torch.zeros(B, dtype=torch.int32, device=dev)
            self._track_bufs = {}
        # voicing: the two voicing kernels are part of the f0 branch (captured once); per row, voicing_on switches the decision and
        # the thresholds are the session's.  No state: the detector looks at the whole ring again every tick
        self.voicing = bool(voicing)
        if self.voicing:
            self._voicing = voicing_opts
            f64 = dict(dtype=torch.float64, device=dev)
            self.voicing_on = torch.zeros(B, dtype=torch.int32, device=dev)
            self.voicing_thr_on = torch.full((B,), common.VOICING_ON, **f64)
            self.voicing_thr_off = torch.full((B,), common.VOICING_OFF, **f64)
            self.voicing_floor_e = torch.full((B,), common.voicing_floor_e(common.VOICING_FLOOR_DB), **f64)
            self._voicing_out = dict(r=torch.zeros(B, self.frames, **f64),
                                     voiced=torch.zeros(B, self.frames, dtype=torch.int32, device=dev),
                                     changed=torch.zeros(B, dtype=torch.int32, device=dev))
        # gate: the two gate kernels are part of the tick (captured once); per row, gate_on switches the session's gate, and the tick
        # reads seg_len_eff / world_eff / follow where it read seg_len / world_on / emit.  gate_state is the session's, like phi
        self.gate = bool(gate)
        if self.gate:
            self.tick_seconds = self.chunk / input_sr
            self.gate_lookahead = self.tick_seconds if gate_lookahead is None else float(gate_lookahead)
            self._gate_look16 = int(round(self.gate_lookahead * 16000))
            i32 = dict(dtype=torch.int32, device=dev)
            self.gate_on = torch.zeros(B, **i32)
            self.thr_ms = torch.zeros(B, dtype=torch.float64, device=dev)
            self.hold_ticks = torch.zeros(B, **i32)
            self.gate_state = torch.zeros(B, 2, **i32)
            self.g0 = torch.ones(B, dtype=torch.float32, device=dev)
            self.g1 = torch.ones(B, dtype=torch.float32, device=dev)
            self.seg_len_eff = torch.zeros(B * self.S, **i32)
            self.follow = torch.zeros(B, 1, dtype=torch.bool, device=dev)
            self.world_eff = torch.zeros(B, **i32) if self.world_pitch else None
            lo, ln = self._span(self.chunk)                # the emitted centre span of step(), per session rate (_set_rate)
            self.span_lo = torch.full((B,), lo, **i32)
            self.span_len = torch.full((B,), ln, **i32)
        # crossfade: the seam kernel is part of the tick (captured once); per row, xlen is the session's crossfade in samples (0:
        # off) and shift its chunk.  tail / stored are the session's, like phi
        self.crossfade = bool(crossfade)
        if self.crossfade:
            self._row_len = {r: self._wave_len(r) for r in rates}      # the samples of a session's final wave, per rate
            i32 = dict(dtype=torch.int32, device=dev)
            spans = [self._span(self._chunk_at(r)) for r in rates]
            self.xlen = torch.zeros(B, **i32)
            self.shift = torch.full((B,), self.chunk, **i32)
            self.stored = torch.zeros(B, **i32)
            self.tail = torch.zeros(B, max(ln for _, ln in spans), dtype=torch.float32, device=dev)
            self.seam_stats = torch.zeros(B, 2, dtype=torch.float64, device=dev)
            if not self.gate:
                lo, ln = self._span(self.chunk)
                self.span_lo = torch.full((B,), lo, **i32)
                self.span_len = torch.full((B,), ln, **i32)
        # limiter: the limiter kernel is part of the tick (captured once), last, on what is emitted; per row, look is the session's
        # lookahead in samples (0: off), hold its hold, ceil its ceiling.  limit_hist is the session's, like phi
        self.limiter = bool(limiter)
        if self.limiter:
            i32 = dict(dtype=torch.int32, device=dev)
            self._limit_len = {r: self._wave_len(r) for r in rates}    # the samples of a session's final wave, per rate
            self.look = torch.zeros(B, **i32)
            self.hold = torch.zeros(B, **i32)
            self.ceil = torch.ones(B, dtype=torch.float32, device=dev)
            self.limit_hist = torch.ones(B, ld_hist, dtype=torch.float32, device=dev)
            self.limit_gmin = torch.ones(B, dtype=torch.float32, device=dev)
            self.limit_shift = torch.full((B,), self._limit_shift(self.chunk), **i32)
            if not (self.gate or self.crossfade):
                lo, ln = self._span(self.chunk)
                self.span_lo = torch.full((B,), lo, **i32)
                self.span_len = torch.full((B,), ln, **i32)
        # envelope: the envelope kernel is part of the tick (captured once), right after the decoder; per row, env_amount is the
        # session's amount (0: copied).  No state: the kernel is a function of the tick's ring and wave.  _env_out is allocated once,
        # by the first tick
        self.envelope = bool(envelope)
        if self.envelope:
            self._env = env[1:]                                # (floor_ms, g_lo, g_hi, radius)
            self.env_amount = torch.zeros(B, dtype=torch.float32, device=dev)
            self.env_minmax = torch.ones(B, 2, dtype=torch.float32, device=dev)
            self._env_out = None
        # post filter: the post filter kernel is part of the tick (captured once), right after the decoder and before the envelope
        # follow; per row, pf_alpha is the session's amount (0: copied).  No state: a function of the tick's wave.  _pf_out is
        # allocated once, by the first tick
        self.post_filter = bool(post_filter)
        if self.post_filter:
            self._pf = pf[1:]                                  # (ratio, tilt, order, window, floor_ms, g_lo, g_hi)
            self._pf_win, self._pf_lag = postfilter_tables(pf[4], pf[3], dev)
            self.pf_alpha = torch.zeros(B, dtype=torch.float32, device=dev)
            self.pf_minmax = torch.ones(B, 2, dtype=torch.float32, device=dev)
            self._pf_out = None
        self.phi = torch.zeros(B, 64, device=dev)
        self._in = torch.zeros(B, ld_in, device=dev)
        # sparse: the rings live on the device in time order (ring_dev; `ring` is gone, rings() reads them back), one push per tick
        # moves the present rows on and writes _in and the tick's masked row arrays, which the tick reads where it read seg_len /
        # world_on; the emitted spans are cut on the device into _pcm.  present and emit are the two rows of one flags array: one copy
        self.sparse = bool(sparse)
        if self.sparse:
            i32 = dict(dtype=torch.int32, device=dev)
            cs = [self._chunk_at(r) for r in rates]
            up8 = lambda v: -(-int(v) // 8) * 8                                       # noqa: E731  (strides of whole 16-byte groups)
            self.ring = None
            self.ring_dev = torch.zeros(B, up8(ld_in), dtype=torch.int16, device=dev)
            self._stage = torch.zeros(B, up8(max(cs)), dtype=torch.int16).pin_memory()
            self._chunks_dev = torch.zeros(B, up8(max(cs)), dtype=torch.int16, device=dev)
            rows = 3 if conceal else 2                     # (conceal: `lost`, a third row of the same copy)
            self._flags_host = torch.zeros(rows, B, dtype=torch.bool).pin_memory()
            self._flags = torch.zeros(rows, B, dtype=torch.bool, device=dev)
            self.present, self.emit = self._flags[0], self._flags[1].view(B, 1)
            self._staged = None                            # the event after the latest upload from the two pinned buffers
            self.chunk_len = torch.full((B,), self.chunk, **i32)
            self.ring_len = torch.full((B,), self.n, **i32)
            self.seg_len_tick = torch.zeros(B * self.S, **i32)
            self.world_tick = torch.zeros(B, **i32) if self.world_pitch else None
            if not (self.gate or self.crossfade or self.limiter):
                lo, ln = self._span(self.chunk)
                self.span_lo = torch.full((B,), lo, **i32)
                self.span_len = torch.full((B,), ln, **i32)
            self._pcm = torch.zeros(B, up8(max(self._span(c)[1] for c in cs)), dtype=torch.int16, device=dev)
            self._pcm_host = torch.zeros(self._pcm.shape, dtype=torch.int16).pin_memory()
            self.pushes = 0                                # (how many ticks pushed the rings: one per step with a chunk)
        # conceal: alive_conceal_rows runs in front of the push on the ticks that have a lost or a recovering slot (the host mirrors
        # which slots are in a run: _conceal_run); per row, conceal_on switches the session's concealment and _conceal_consts holds
        # its lags, window and durations in its own samples.  _conceal_state / conceal_tmpl are the session's, like phi
        self.conceal = bool(conceal)
        if self.conceal:
            self._conceal_ms = conceal_ms
            self.lost = self._flags[2]
            geo = {r: conceal_geometry(r, self._chunk_at(r), self._chunk_at(r) * self.buffersize, *conceal_ms, check=False)
                   for r in rates}
            self._conceal_closed = torch.tensor(geo[int(input_sr)], dtype=torch.int32)
            self.conceal_on = torch.zeros(B, dtype=torch.bool, device=dev)
            self._conceal_consts = self._conceal_closed.view(6, 1).repeat(1, B).to(dev).contiguous()
            self._conceal_state = torch.zeros(B, 2, dtype=torch.int32, device=dev)
            self.conceal_tmpl = torch.zeros(B, -(-max(g[1] for g in geo.values()) // 8) * 8, dtype=torch.int16, device=dev)
            self._conceal_run = [False] * B
            self._conceal_host = [False] * B               # (the sessions' switches, for the mirror)
            self.conceals = 0                              # (how many ticks launched alive_conceal_rows)
        # loudness: the loudness kernel is part of the tick (captured once), after the gate's edge and before the limiter; per row,
        # loud_on switches the session's normalisation, loud_hop / loud_coef are its rate's sub-block and K-weighting and loud_par its
        # (z_abs, z_t, d, P, gmax, qs).  loud_state is the session's, like phi
        self.loud = bool(loudness)
        if self.loud:
            self._loud = loud                                  # (d, P, z_abs, gmax, slew_db)
            i32 = dict(dtype=torch.int32, device=dev)
            self.loud_on = torch.zeros(B, dtype=torch.bool, device=dev)
            self.loud_hop = torch.full((B,), loudness_hop(self._out_rate(int(input_sr))), **i32)
            self.loud_coef = torch.zeros(B, 10, dtype=torch.float64, device=dev)
            self.loud_par = torch.zeros(B, LOUDNESS_PARAMS, dtype=torch.float64, device=dev)
            self.loud_state = torch.zeros(B, LOUDNESS_STATE, dtype=torch.float64, device=dev)
            self.loud_state[:, 12] = 1.0
            if not (self.gate or self.crossfade or self.limiter or self.sparse):
                lo, ln = self._span(self.chunk)
                self.span_lo = torch.full((B,), lo, **i32)
                self.span_len = torch.full((B,), ln, **i32)
        self._graph = None
        self._graph_pool_version = None
        self.captures = 0
        self._side = None
        self._f0_bufs = {}
        self.last_f0 = None
        if fp16_guarded(self.B * self.frames):
            ops.f16_clear()

    # ------------------------------------------------------------------ sessions
    def _slot(self, slot):
        if not isinstance(slot, (int, np.integer)) or not 0 <= int(slot) < self.B:
            raise ValueError(f"slot {slot!r} out of range [0, {self.B})")
        return int(slot)

    def _session_k(self, slot, k):
        """a session's k (None: the converter's) against the converter's k_max"""
        if k is None:
            return self.k
        if self.k_max is None:
            if isinstance(k, (int, np.integer)) and not isinstance(k, (bool, np.bool_)) and int(k) == self.k:
                return self.k
            raise ValueError(f"slot {slot}: k={k!r} differs from the converter's k={self.k}: a per-session k needs a converter built "
                             "with MultiStreamConverter(..., k_max=K), k <= K <= 8")
        k = check_k(k, f"slot {slot}: k")
        if k > self.k_max:
            raise ValueError(f"slot {slot}: k={k} is above the converter's k_max={self.k_max}")
        return k

    def _span(self, cs):
        """the span of a session's output wave that step() emits, for chunks of cs samples: (first sample, length)"""
        return self.buffersize * cs // 2 - cs // 2, 2 * (cs // 2)

    def _chunk_at(self, rate):
        """the chunk of a session at a declared rate"""
        return self.chunk if self._rt is None else self._chunks[int(rate)]

    def _wave_len(self, rate):
        """the samples of the final wave of a session at a declared rate: 320 per frame at 16 kHz, resampled to the rate"""
        if self._rt is not None:
            return self._lout[int(rate)]
        return wave_length(self.frames, self.output_sr)

    def _session_seam(self, slot, p, rate=None):
        """a session's crossfade -> X in samples at its rate (0: off), checked against the converter"""
        ms = p.get("crossfade_ms")
        try:
            if check_crossfade_ms(ms) is None:
                return 0
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if not self.crossfade:
            raise ValueError(f"slot {slot}: crossfade_ms={ms!r} needs a converter built with MultiStreamConverter(..., "
                             "crossfade=True)")
        rate = int(self.rate[slot] if rate is None else rate)
        try:
            return seam_geometry(self._chunk_at(rate), self.buffersize, rate, ms, self._row_len[rate])[2]
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None

    def _limit_shift(self, cs):
        """the ring's advance per tick in samples of a session's final wave, for chunks of cs samples: cs where input_sr ==
        output_sr; otherwise the advance at output_sr, but never less than the span (step() cuts cs samples whatever output_sr is)"""
        if self.input_sr == self.output_sr:
            return cs
        return max(cs, int(round(cs * self.output_sr / self.input_sr)))

    def _session_limit(self, slot, p, rate=None):
        """a session's limiter -> (L, H, c) at its rate ((0, 0, 1.0): off), checked against the converter"""
        db, look, hold = p.get("limit_db"), p.get("limit_lookahead_ms", 5.0), p.get("limit_hold_ms", 20.0)
        try:
            if check_limit(db, look, hold) is None:
                return 0, 0, 1.0
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if not self.limiter:
            raise ValueError(f"slot {slot}: limit_db={db!r} needs a converter built with MultiStreamConverter(..., limiter=True)")
        rate = int(self.rate[slot] if rate is None else rate)
        cs = self._chunk_at(rate)
        out_rate = rate if self._rt is not None else int(self.output_sr)
        try:
            return limit_geometry(cs, self.buffersize, out_rate, db, look, hold, self._limit_len[rate], self.limit_hist.shape[1],
                                  self._limit_shift(cs))[2:]
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None

    def _out_rate(self, rate):
        """the rate of the final wave of a session at a declared rate: its own with per-session rates, else output_sr"""
        return int(rate) if self._rt is not None else int(self.output_sr)

    def _session_loudness(self, slot, p, rate=None):
        """a session's loudness target -> (on, hop, coef, par) at its rate (on False: off), checked against the converter"""
        target = p.get("lufs")
        try:
            checked = check_loudness(target)
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if checked is None:
            return False, 0, None, None
        if not self.loud:
            raise ValueError(f"slot {slot}: lufs={target!r} needs a converter built with MultiStreamConverter(..., loudness=True)")
        rate = int(self.rate[slot] if rate is None else rate)
        fs = self._out_rate(rate)
        d, P, z_abs, gmax, slew = self._loud
        n = self._span(self._chunk_at(rate))[1]
        return True, loudness_hop(fs), loudness_filter(fs)[0], (z_abs, checked[0], d, P, gmax, loudness_slew(slew, n, fs))

    def _loud_reset(self, slot):
        self.loud_state[slot] = 0.0
        self.loud_state[slot, 12] = 1.0

    def loudness(self):
        """the sessions' running loudness after the latest tick, a list of B pairs (LUFS, gain in dB): the running loudness S / W of
        what the session emitted BEFORE the gain (-inf before its first counted block) and the gain the latest tick ended at; (-inf,
        0.0) for a slot that does not normalise (or is closed).  One host read"""
        if not self.loud:
            raise ValueError("loudness needs a converter built with MultiStreamConverter(..., loudness=True)")
        out = []
        for b, st in enumerate(self.loud_state.tolist()):
            if not (self.is_open[b] and self.params[b].get("lufs") is not None):
                out.append((-math.inf, 0.0))
                continue
            out.append((loudness_lufs(st[10] / st[11]) if st[11] > 0 else -math.inf, 20.0 * math.log10(st[12]) if st[12] > 0 else 0.0))
        return out

    def _session_envelope(self, slot, p):
        """a session's envelope amount (None: 0), checked against the converter"""
        a = p.get("envelope", 0.0)
        try:
            a = check_envelope(0.0 if a is None else a)[0]
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if a > 0 and not self.envelope:
            raise ValueError(f"slot {slot}: envelope={a!r} needs a converter built with MultiStreamConverter(..., envelope=True)")
        return a

    def _session_post_filter(self, slot, p):
        """a session's post filter amount (None: 0), checked against the converter"""
        a = p.get("post_filter", 0.0)
        try:
            a = check_post_filter(0.0 if a is None else a)[0]
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if a > 0 and not self.post_filter:
            raise ValueError(f"slot {slot}: post_filter={a!r} needs a converter built with MultiStreamConverter(..., post_filter=True)")
        return a

    def _session_conceal(self, slot, p, rate=None):
        """a session's concealment -> (on, consts) at its rate, None in a converter without conceal; checked against the converter.
        conceal None: the converter's (on in a conceal=True converter)"""
        v = p.get("conceal")
        if v is not None and not isinstance(v, (bool, np.bool_)):
            raise ValueError(f"slot {slot}: conceal must be a bool or None, got {v!r}")
        if not self.conceal:
            if v:
                raise ValueError(f"slot {slot}: conceal=True needs a converter built with MultiStreamConverter(..., sparse=True, "
                                 "conceal=True)")
            return None
        on = True if v is None else bool(v)
        rate = int(self.rate[slot] if rate is None else rate)
        cs = self._chunk_at(rate)
        try:
            return on, conceal_geometry(rate, cs, cs * self.buffersize, *self._conceal_ms, check=on)
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None

    def _conceal_clear(self, slot):
        """the slot is in no run any more: the device state and the host's mirror"""
        if self.conceal:
            self._conceal_state[slot] = 0
            self._conceal_run[slot] = False

    def conceal_state(self):
        """the concealment runs after the latest tick, a list of B pairs (samples made up so far in the run, its period in samples);
        (0, 0) for a slot that is in no run, or closed.  One host read"""
        if not self.conceal:
            raise ValueError("conceal_state needs a converter built with MultiStreamConverter(..., sparse=True, conceal=True)")
        return [(q, P) if self.is_open[b] and q > 0 else (0, 0) for b, (q, P) in enumerate(self._conceal_state.tolist())]

    def _session_track(self, slot, p):
        """a session's tracker settings -> (on, weight, jump), checked against the converter"""
        on = p.get("pitch_track", False)
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"slot {slot}: pitch_track must be a bool, got {on!r}")
        try:
            w, j = (common.track_param("track_weight", p.get("track_weight", common.TRACK_WEIGHT)),
                    common.track_param("track_jump", p.get("track_jump", common.TRACK_JUMP)))
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if on and not self.pitch_track:
            raise ValueError(f"slot {slot}: pitch_track=True needs a converter built with MultiStreamConverter(..., pitch_track=True)")
        if on and p.get("world_pitch", False):
            raise ValueError(f"slot {slot}: pitch_track cannot be combined with world_pitch: the tracker decodes the estimator's "
                             "class scores")
        return int(bool(on)), w, j

    def _session_path(self, slot, p):
        """a session's match path settings -> (on, weight), checked against the converter"""
        on = p.get("match_path", False)
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"slot {slot}: match_path must be a bool, got {on!r}")
        try:
            w = common.path_param(p.get("path_weight", common.PATH_WEIGHT), "path_weight")
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if on and not self.match_path:
            raise ValueError(f"slot {slot}: match_path=True needs a converter built with MultiStreamConverter(..., match_path=True)")
        return int(bool(on)), w

    def path_moved(self):
        """how many frames of each slot's ring the path moved off the frame's nearest row in the latest tick (a blend: over all its
        lists), a list of B ints; 0 for a slot without the path (or closed).  One host read"""
        if not self.match_path:
            raise ValueError("path_moved needs a converter built with MultiStreamConverter(..., match_path=True)")
        moved = self.path_moved_rows.view(self.B, self.S).sum(dim=1).tolist()
        return [moved[b] if self.is_open[b] and self.params[b].get("match_path", False) else 0 for b in range(self.B)]

    def _set_path(self, slot, on, weight, k):
        rows = slice(slot * self.S, (slot + 1) * self.S)
        self.path_on[rows], self.path_weight[rows] = on, weight
        self.gather_k[slot] = 1 if on else k
        if not on:
            self.path_moved_rows[rows] = 0

    def _session_voicing(self, slot, p):
        """a session's voicing settings -> (on, thr_on, thr_off, floor_e), checked against the converter"""
        on = p.get("voicing", False)
        if not isinstance(on, (bool, np.bool_)):
            raise ValueError(f"slot {slot}: voicing must be a bool, got {on!r}")
        o = common.voicing_options(dict(on=p.get("voicing_on", common.VOICING_ON), off=p.get("voicing_off", common.VOICING_OFF),
                                        floor_db=p.get("voicing_floor_db", common.VOICING_FLOOR_DB)), f"slot {slot}")
        if on and not self.voicing:
            raise ValueError(f"slot {slot}: voicing=True needs a converter built with MultiStreamConverter(..., voicing=True)")
        if on and p.get("world_pitch", False):
            raise ValueError(f"slot {slot}: voicing cannot be combined with world_pitch: WORLD makes its own voicing decision")
        return int(bool(on)), o["on"], o["off"], o["floor_e"]

    def voicing_state(self):
        """the voicing decision of the latest tick, a list of B triples (voiced frames of the ring, frames whose f0 was set to 0, r of
        the centre frame of the emitted span); (0, 0, 0.0) for a slot that does not decide (or is closed).  One host read"""
        if not self.voicing:
            raise ValueError("voicing_state needs a converter built with MultiStreamConverter(..., voicing=True)")
        o = self._voicing_out
        centre = min((self.begin_of_output + self.end_of_output) // 2 // 320, self.frames - 1)      # (the span is in 16 kHz samples)
        rows = torch.stack([o["voiced"].sum(dim=1).double(), o["changed"].double(), o["r"][:, centre]], dim=1).tolist()
        return [(int(v), int(c), r) if self.is_open[b] and self.params[b].get("voicing", False) else (0, 0, 0.0)
                for b, (v, c, r) in enumerate(rows)]

    def pitch_track_changed(self):
        """how many frames of each slot's ring the tracker moved off the per-frame argmax in the latest tick, a list of B ints; 0 for
        a slot that does not track (or is closed).  One host read"""
        if not self.pitch_track:
            raise ValueError("pitch_track_changed needs a converter built with MultiStreamConverter(..., pitch_track=True)")
        moved = self.track_changed.tolist()
        return [moved[b] if self.is_open[b] and self.params[b].get("pitch_track", False) else 0 for b in range(self.B)]

    def _session_gate(self, slot, p):
        """a session's gate settings -> (on, thr_ms, hold_ticks), checked against the converter"""
        db, hold = p.get("gate_db"), p.get("gate_hold", 0.2)
        try:
            ticks = gate_hold_ticks(hold, self.chunk / self.input_sr)
            if db is None:
                return 0, 0.0, 0
            thr = gate_thr_ms(db)
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if not self.gate:
            raise ValueError(f"slot {slot}: gate_db={db!r} needs a converter built with MultiStreamConverter(..., gate=True)")
        return 1, thr, ticks

    def _apply(self, slot, p, rate=None):
        k = self._session_k(slot, p["k"])
        gate = self._session_gate(slot, p)
        xlen = self._session_seam(slot, p, rate)
        limit = self._session_limit(slot, p, rate)
        env = self._session_envelope(slot, p)
        pfa = self._session_post_filter(slot, p)
        con = self._session_conceal(slot, p, rate)
        track = self._session_track(slot, p)
        voicing = self._session_voicing(slot, p)
        path = self._session_path(slot, p)
        loud = self._session_loudness(slot, p, rate)
        names, weights = blend_spec(p["voice"], self.pool, k, self.S)
        world = p["world_pitch"]
        if not isinstance(world, (bool, np.bool_)):
            raise ValueError(f"slot {slot}: world_pitch must be a bool, got {world!r}")
        if world and not self.world_pitch:
            raise ValueError(f"slot {slot}: world_pitch=True needs a converter built with MultiStreamConverter(..., world_pitch=True)")
        auto = p.get("auto_pitch", False)
        if not isinstance(auto, (bool, np.bool_)):
            raise ValueError(f"slot {slot}: auto_pitch must be a bool, got {auto!r}")
        if auto and not self.auto_pitch:
            raise ValueError(f"slot {slot}: auto_pitch=True needs a converter built with MultiStreamConverter(..., auto_pitch=True)")
        if auto:                                              # (raises for a voice without a register, before anything changes)
            try:
                target = self.pool.blend_register(names, weights)
            except ValueError as e:
                raise ValueError(f"slot {slot}: {e}") from None
        inton, ranged = p.get("intonation", 1.0), p.get("auto_range", False)
        try:
            inton = check_intonation(inton)
        except ValueError as e:
            raise ValueError(f"slot {slot}: {e}") from None
        if not isinstance(ranged, (bool, np.bool_)):
            raise ValueError(f"slot {slot}: auto_range must be a bool, got {ranged!r}")
        if (inton != 1.0 or ranged) and not self.pitch_range:
            raise ValueError(f"slot {slot}: intonation={inton!r} / auto_range={bool(ranged)!r} need a converter built with "
                             "MultiStreamConverter(..., pitch_range=True)")
        if ranged:                                            # (raises for a voice without a range, before anything changes)
            try:
                target_sd = self.pool.blend_range(names, weights)
            except ValueError as e:
                raise ValueError(f"slot {slot}: {e}") from None
        self._write_segments(slot, names)
        if self.S > 1:
            rows = slice(slot * self.S, (slot + 1) * self.S)
            self.weight[rows] = torch.tensor(list(weights) + [0.0] * (self.S - len(names)), dtype=torch.float64)
        self._hold(slot, names)
        if self.k_max is not None:
            self.k_rows[slot] = k
            if self.S > 1:
                self.k_lists[slot * self.S:(slot + 1) * self.S] = k
        if self.match_path:
            self._set_path(slot, path[0], path[1], k)
        self.alpha[slot] = float(p["alpha"])
        self.f0_rate[slot] = float(p["f0_rate"])
        self.pitch[slot] = float(p["pitch"])
        self.in_post[slot] = db_scale(p["input_gain"])
        self.out_pre[slot] = db_scale(p["gain"])
        if self.world_pitch:
            self._set_world(slot, bool(world), float(p["f0_rate"]))
        if self.pitch_track:
            self.track_on[slot], self.track_weight[slot], self.track_jump[slot] = track
            if not track[0]:
                self.track_changed[slot] = 0
        if self.voicing:
            self.voicing_on[slot], self.voicing_thr_on[slot], self.voicing_thr_off[slot], self.voicing_floor_e[slot] = voicing
            if not voicing[0]:
                self._voicing_clear(slot)
        if self.auto_pitch:
            self.auto_on[slot] = int(bool(auto))
            self.target[slot] = target if auto else 0.0
        if self.pitch_range:
            self.intonation[slot] = inton
            self.range_on[slot] = int(bool(ranged))
            self.target_sd[slot] = target_sd if ranged else 0.0
        if self.gate:
            self.gate_on[slot], self.thr_ms[slot], self.hold_ticks[slot] = gate
        if self.crossfade:
            self.xlen[slot] = xlen
        if self.limiter:
            self.look[slot], self.hold[slot], self.ceil[slot] = limit
        if self.envelope:
            self.env_amount[slot] = env
        if self.post_filter:
            self.pf_alpha[slot] = pfa
        if self.loud:
            self.loud_on[slot] = loud[0]
            if loud[0]:
                self.loud_hop[slot] = loud[1]
                self.loud_coef[slot] = torch.tensor(loud[2], dtype=torch.float64)
                self.loud_par[slot] = torch.tensor(loud[3], dtype=torch.float64)
        if self.conceal:
            self.conceal_on[slot], self._conceal_host[slot] = con[0], con[0]
            self._conceal_consts[:, slot] = torch.tensor(con[1], dtype=torch.int32)

    def _voicing_clear(self, slot):
        """the read-back rows of a slot that does not decide (the kernels leave the rows of such a slot untouched)"""
        o = self._voicing_out
        o["r"][slot], o["voiced"][slot], o["changed"][slot] = 0.0, 0, 0

    def _write_segments(self, slot, names):
        """the slot's rows of seg_lo / seg_len from where its voices lie in the pool now"""
        segs = [self.pool.segment(n) for n in names]
        if self.S == 1:
            self.seg_lo[slot], self.seg_len[slot] = segs[0]
        else:                                                 # the slot's S list rows, unused ones inactive, in one write each
            pad = self.S - len(segs)
            rows = slice(slot * self.S, (slot + 1) * self.S)
            self.seg_lo[rows] = torch.tensor([lo for lo, _ in segs] + [0] * pad, dtype=torch.int32)
            self.seg_len[rows] = torch.tensor([m for _, m in segs] + [0] * pad, dtype=torch.int32)

    def _hold(self, slot, names):
        """the slot now uses `names` (blend components included): on a reserved pool, take a hold on each and release the holds
        of the voices it used before, so that pool.remove refuses a voice some session still searches"""
        if self._reserved:
            for n in names:
                self.pool.hold(n, self._label)
            for n in self._names[slot]:
                self.pool.release(n, self._label)
        self._names[slot] = tuple(names)

    def _follow_pool(self):
        """before a tick on a reserved pool: order the tick after the pool's latest operation, whatever stream that ran on, and if
        some voice moved or grew since the last look (pool.layout) rewrite every open slot's segment rows from its stored voice --
        device arrays the captured tick reads, so nothing is re-captured"""
        pool = self.pool
        if pool.mutations != self._seen_mutations:
            torch.cuda.current_stream(self.device).wait_event(pool.order)
            self._seen_mutations = pool.mutations
        if pool.layout != self._seen_layout:                  # every list row in one write each (closed slots stay inactive)
            lo, ln = [0] * (self.B * self.S), [0] * (self.B * self.S)
            for slot in range(self.B):
                if self.is_open[slot]:
                    for j, n in enumerate(self._names[slot]):
                        lo[slot * self.S + j], ln[slot * self.S + j] = pool.segment(n)
            self.seg_lo.copy_(torch.tensor(lo, dtype=torch.int32))
            self.seg_len.copy_(torch.tensor(ln, dtype=torch.int32))
            self._seen_layout = pool.layout

    def _set_world(self, slot, on, f0_rate):
        self.world_on[slot] = int(on)
        self._world_sel[slot] = on
        self.f0_rate_eff[slot] = 1.0 if on else f0_rate

    def _set_rate(self, slot, rate):
        self.rate[slot] = rate
        if self._rt is None:
            return
        c = self._chunks[rate]
        if self.gate or self.crossfade or self.limiter or self.sparse or self.loud:
            self.span_lo[slot], self.span_len[slot] = self._span(c)
        if self.sparse:
            self.chunk_len[slot], self.ring_len[slot] = c, c * self.buffersize
        if self.crossfade:
            self.shift[slot] = c
        if self.limiter:
            self.limit_shift[slot] = self._limit_shift(c)
        self.slot_chunk[slot] = c
        self.len_in[slot] = c * self.buffersize
        self.pair_in[slot] = self._rt.pair(rate, 16000)
        self.pair_out[slot] = self._rt.pair(16000, rate)
        self.len_out[slot] = self._lout[rate]

    def open(self, slot, voice, pitch=0.0, f0_rate=1.0, alpha=0.0, gain=0.0, input_gain=0.0, rate=None, world_pitch=False, k=None,
             auto_pitch=False, gate_db=None, gate_hold=0.2, crossfade_ms=None, limit_db=None, limit_lookahead_ms=5.0,
             limit_hold_ms=20.0, envelope=0.0, conceal=None, intonation=1.0, auto_range=False, pitch_track=False, track_weight=1.0,
             track_jump=12.0, lufs=None, voicing=False, voicing_on=common.VOICING_ON, voicing_off=common.VOICING_OFF,
             voicing_floor_db=common.VOICING_FLOOR_DB, match_path=False, path_weight=common.PATH_WEIGHT, post_filter=0.0):
        """start a session in `slot`: empty ring, phase 0.  k (default: the converter's): the session's own k, 1 <= k <= k_max, in
        a converter built with k_max= (every voice of the session needs at least k vectors); without k_max only the converter's k.  `rate` (default: the converter's input_sr) is one of the declared
        `rates`: the session sends and receives chunk * rate / input_sr samples per tick, for its whole life.  world_pitch=True:
        WORLD's f0 of the session's ring instead of the estimator's, f0_rate not applied (needs a world_pitch=True converter).
        auto_pitch=True (needs an auto_pitch=True converter and a register on every voice of the session): the pitch shift follows
        the target voice's register, and `pitch` is an offset on top of it.  gate_db (needs a gate=True converter): the session's
        input gate, a threshold in dBFS on its 16 kHz ring after the input gain (None: no gate); gate_hold: the seconds (>= 0) it
        stays open after the last loud tick.  A gated session starts closed: its first chunk fades in.  crossfade_ms (needs a
        crossfade=True converter): the milliseconds over which the head of every chunk is faded in from the previous tick's
        continuation (None: a hard cut), at most the session's emitted span; the first chunk has nothing to fade from.  limit_db
        (needs a limiter=True converter): the session's output limiter, a ceiling in dBFS <= 0 that no emitted sample exceeds (None:
        no limiter, the int16 edge wraps); limit_lookahead_ms: how long before a peak the gain starts to fall (and after the hold,
        how long it takes to come back), at most the session's chunk; limit_hold_ms: how long the gain stays down after a peak.
        envelope (above 0: needs an envelope=True converter): how far the converted wave follows the loudness contour of the session's
        input, from 0 (the decoder's own level) to 1 (the source's smoothed frame level, within the converter's range).
        conceal (None: the converter's, on in a conceal=True converter; True needs one): whether the session's lost chunks (step(...,
        lost=)) are concealed by waveform substitution; False: they are chunks of zeros.  The session's ring must hold the search:
        ValueError otherwise.
        intonation (other than 1: needs a pitch_range=True converter): a finite factor >= 0 on the session's pitch excursions around
        its running mean pitch, growing from 1 with the evidence as the automatic shift does.  auto_range=True (needs such a converter
        and a range on every voice of the session): the factor is multiplied by target sd / running source sd, within [1 /
        pitch_range_max, pitch_range_max] -- with auto_pitch, the mean-variance transform of log-f0.
        pitch_track=True (needs a pitch_track=True converter; not together with world_pitch): the session's f0 is the Viterbi path over
        the estimator's class scores of its ring instead of their per-frame argmax, at track_weight per semitone moved inside the
        converter's band and track_jump for any other move (both >= 0, in the units of the scores); the followers and the transform see
        the tracked contour.
        voicing=True (needs a voicing=True converter; not together with world_pitch): the f0 of the frames of the session's ring that
        are not periodic becomes 0, after the estimator or the tracker and before the followers and the transform: a frame turns voiced
        when its best normalised correlation reaches voicing_on and unvoiced under voicing_off (0 < off <= on <= 1), and a frame under
        voicing_floor_db dBFS is unvoiced whatever its correlation.
        lufs (needs a loudness=True converter): the session's loudness target in LUFS, -70 < lufs <= 0 (None: the session's level is
        left alone): what the session emits is brought to it by a running BS.1770 loudness and a slewed gain, ahead of the limiter.
        match_path=True (needs a match_path=True converter): each frame's matched feature is ONE of its k nearest rows, chosen by a
        Viterbi path over the ring's frames that weighs the cosine between consecutive chosen rows by path_weight (>= 0; 0 is the
        k = 1 match) against a candidate's cosine below the frame's best one; a blend: every voice's list takes its own path.
        post_filter (above 0: needs a post_filter=True converter): the alpha of the session's adaptive formant post filter, at most
        0.85 (0.8 is the classic setting): the valleys between the formants of the converted wave are deepened, its level kept"""
        slot = self._slot(slot)
        rate = int(self.input_sr if rate is None else rate)
        if rate not in self.rates:
            raise ValueError(f"slot {slot}: rate {rate} Hz was not declared (rates={list(self.rates)}): pass it in "
                             "MultiStreamConverter(..., rates=...)")
        p = dict(voice=voice, pitch=pitch, f0_rate=f0_rate, alpha=alpha, gain=gain, input_gain=input_gain, world_pitch=world_pitch,
                 k=k, auto_pitch=auto_pitch, gate_db=gate_db, gate_hold=gate_hold, crossfade_ms=crossfade_ms, limit_db=limit_db,
                 limit_lookahead_ms=limit_lookahead_ms, limit_hold_ms=limit_hold_ms, envelope=envelope, conceal=conceal,
                 intonation=intonation, auto_range=auto_range, pitch_track=pitch_track, track_weight=track_weight,
                 track_jump=track_jump, lufs=lufs, voicing=voicing, voicing_on=voicing_on, voicing_off=voicing_off,
                 voicing_floor_db=voicing_floor_db, match_path=match_path, path_weight=path_weight, post_filter=post_filter)
        self._apply(slot, p, rate)                            # (validates the voice before anything changes)
        self._set_rate(slot, rate)
        self.params[slot] = p
        self.is_open[slot] = True
        self.count[slot] = 0
        self._zero_ring(slot)
        self.phi[slot] = 0.0
        if self.auto_pitch:
            self.reg_state[slot] = 0.0                        # a new source: nothing heard yet
        if self.gate:
            self.gate_state[slot] = 0                         # closed, no hold: the first emitted chunk fades in
        if self.crossfade:
            self.stored[slot] = 0                             # never fade from another session's tail
        if self.limiter:
            self._limit_reset(slot)                           # a new stream: no peak behind it
        if self.loud:
            self._loud_reset(slot)                            # a new stream: nothing heard yet, the gain at 1
        self._conceal_clear(slot)                             # a new stream: no run behind it
        return self

    def set(self, slot, **params):
        """change a session's settings between ticks (voice, pitch, f0_rate, alpha, gain, input_gain, world_pitch, k, auto_pitch,
        intonation, auto_range, pitch_track, track_weight, track_jump, voicing, voicing_on, voicing_off, voicing_floor_db, match_path, path_weight, gate_db, gate_hold, crossfade_ms, limit_db, limit_lookahead_ms,
        limit_hold_ms, envelope, post_filter, conceal, lufs; the gate's state, the saved tail, the running loudness with its gain and the
        limiter's history are kept: a longer crossfade fades over what the tail holds this tick and in full from the next, and a
        limiter switched on or retuned sees the required gains of the samples already emitted).
        The running source register is kept: a new voice changes the target only, and auto_pitch=True after False resumes from
        what the session had heard while it was on (nothing, if it never was)"""
        slot = self._slot(slot)
        if not self.is_open[slot]:
            raise ValueError(f"slot {slot} is not open")
        if "rate" in params:
            raise ValueError(f"slot {slot}: a session's rate is fixed for its life: close the slot and open it at the new rate")
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
        self._zero_ring(slot)
        self.seg_len[slot * self.S:(slot + 1) * self.S] = 0
        if self.k_max is not None:                           # (the slot stays inactive: its segments are empty)
            self.k_rows[slot] = self.k
            if self.S > 1:
                self.k_lists[slot * self.S:(slot + 1) * self.S] = self.k
        if self.match_path:
            self._set_path(slot, 0, common.PATH_WEIGHT, self.k)
        self._hold(slot, ())
        self.phi[slot] = 0.0
        if self.world_pitch:
            self._set_world(slot, False, 1.0)
        if self.pitch_track:
            self.track_on[slot], self.track_changed[slot] = 0, 0
            self.track_weight[slot], self.track_jump[slot] = common.TRACK_WEIGHT, common.TRACK_JUMP
        if self.voicing:
            self.voicing_on[slot] = 0
            self.voicing_thr_on[slot], self.voicing_thr_off[slot] = common.VOICING_ON, common.VOICING_OFF
            self.voicing_floor_e[slot] = common.voicing_floor_e(common.VOICING_FLOOR_DB)
            self._voicing_clear(slot)
        if self.auto_pitch:
            self.auto_on[slot] = 0
            self.target[slot] = 0.0
            self.reg_state[slot] = 0.0
        if self.pitch_range:
            self.intonation[slot] = 1.0
            self.range_on[slot] = 0
            self.target_sd[slot] = 0.0
        if self.gate:
            self.gate_on[slot] = 0
            self.thr_ms[slot] = 0.0
            self.hold_ticks[slot] = 0
            self.gate_state[slot] = 0
        if self.crossfade:
            self.xlen[slot] = 0
            self.stored[slot] = 0
        if self.limiter:
            self.look[slot] = 0
            self.hold[slot] = 0
            self.ceil[slot] = 1.0
            self._limit_reset(slot)
        if self.envelope:
            self.env_amount[slot] = 0.0
            self.env_minmax[slot] = 1.0
        if self.post_filter:
            self.pf_alpha[slot] = 0.0
            self.pf_minmax[slot] = 1.0
        if self.loud:
            self.loud_on[slot] = False
            self._loud_reset(slot)
        if self.conceal:
            self.conceal_on[slot], self._conceal_host[slot] = False, False
            self._conceal_consts[:, slot] = self._conceal_closed
            self._conceal_clear(slot)
        self._set_rate(slot, int(self.input_sr))             # a closed slot: the converter's own rate, silence
        return self

    def _zero_ring(self, slot):
        if self.sparse:                                       # the device ring and the slot's row of the float input
            self.ring_dev[slot] = 0
            self._in[slot] = 0.0
        else:
            self.ring[slot] = 0

    def rings(self):
        """a sparse converter's rings, int16 [B, ld_in] in time order (what `ring` holds in a dense one).  One host read"""
        if not self.sparse:
            raise ValueError("rings needs a converter built with MultiStreamConverter(..., sparse=True): a dense one has `ring`")
        return self.ring_dev[:, :self.ld_in].cpu().numpy()

    def gate_open(self):
        """the per-slot open flags after the latest tick, a list of B bools: a gated session's gate (False before its first emitting
        tick), True for an open session without a gate, False for a closed slot.  One host read"""
        if not self.gate:
            raise ValueError("gate_open needs a converter built with MultiStreamConverter(..., gate=True)")
        on, was = self.gate_on.tolist(), self.gate_state[:, 1].tolist()
        return [bool(self.is_open[b] and (was[b] if on[b] else True)) for b in range(self.B)]

    def _limit_reset(self, slot):
        self.limit_hist[slot] = 1.0
        self.limit_gmin[slot] = 1.0

    def limit_db(self):
        """how far the limiter turned each slot down in the latest tick, a list of B floats: 20 log10 of the smallest gain of the
        slot's emitted span; 0.0 for a slot that was not touched (or does not limit, or did not emit yet).  One host read"""
        if not self.limiter:
            raise ValueError("limit_db needs a converter built with MultiStreamConverter(..., limiter=True)")
        return gmin_db(self.limit_gmin.tolist())

    def envelope_db(self):
        """how far the envelope moved each slot in the latest tick, a list of B pairs: 20 log10 of the smallest and of the largest
        frame gain over the slot's whole ring; (0.0, 0.0) for a slot that does not follow.  One host read"""
        if not self.envelope:
            raise ValueError("envelope_db needs a converter built with MultiStreamConverter(..., envelope=True)")
        return minmax_db(self.env_minmax.tolist())

    def _follow(self, wave, data):
        """the decoder's 16 kHz waves [B, L] at the loudness contour of the 16 kHz rings `data`, row by row at the sessions' amounts,
        into the buffer allocated once"""
        wave, data = wave.contiguous(), data.contiguous()
        if self._env_out is None or self._env_out.shape != wave.shape:
            self._env_out = torch.empty_like(wave)
        floor_ms, g_lo, g_hi, radius = self._env
        return envelope_waves_(self._env_out, wave, data, None, self.env_amount, ENVELOPE_HOP, radius, floor_ms, g_lo, g_hi,
                               self.env_minmax)

    def post_filter_db(self):
        """the level correction of the post filter in the latest tick, a list of B pairs: 20 log10 of the smallest and of the largest
        frame gain over the slot's whole wave; (0.0, 0.0) for a slot that is not filtered.  One host read"""
        if not self.post_filter:
            raise ValueError("post_filter_db needs a converter built with MultiStreamConverter(..., post_filter=True)")
        return minmax_db(self.pf_minmax.tolist())

    def _postfilter(self, wave):
        """the decoder's 16 kHz waves [B, L] through the post filter, row by row at the sessions' alphas, into the buffer allocated
        once"""
        wave = wave.contiguous()
        if self._pf_out is None or self._pf_out.shape != wave.shape:
            self._pf_out = torch.empty_like(wave)
        ratio, tilt, order, window, floor_ms, g_lo, g_hi = self._pf
        return postfilter_waves_(self._pf_out, wave, None, self.pf_alpha, POSTFILTER_HOP, window, order, self._pf_win, self._pf_lag,
                                 ratio, tilt, floor_ms, g_lo, g_hi, self.pf_minmax)

    def seam_db(self):
        """the seam statistic of the latest tick, a list of B floats: 10 log10(sum (c - t)^2 / sum c^2) over the faded head of each
        slot, c the tick's own decode and t the previous tick's continuation; nan for a slot that did not fade.  One host read"""
        if not self.crossfade:
            raise ValueError("seam_db needs a converter built with MultiStreamConverter(..., crossfade=True)")
        return stats_db(self.seam_stats.tolist())

    def pitch_range_state(self):
        """per slot, (mean, sd, intonation): the running mean pitch and standard deviation (semitones) of the session's source as
        its (S, W, Q) give them -- None, None before any voiced frame or on a session that does not follow -- and the effective
        intonation of the latest tick (1.0 where the transform ran uncentred).  One host read"""
        if not self.pitch_range:
            raise ValueError("pitch_range_state needs a converter built with MultiStreamConverter(..., pitch_range=True)")
        out = []
        for (S, W, Q), i in zip(self.reg_state.tolist(), self.inton_eff.tolist()):
            if W == 0:
                out.append((None, None, i))
                continue
            m = S / W
            v = Q / W - m * m
            out.append((m, float(np.sqrt(v)) if v > 0 else 0.0, i))
        return out

    # ------------------------------------------------------------------ device step
    def _f0_on_side_stream(self, spec, data):
        """realtime.f0_on_side_stream with the per-row pitch transform.  world_pitch: after the estimator, the masked WORLD f0 of
        the 16-kHz rings `data` (rows off: no work), selected per row, then the transform at the effective rates.  pitch_track: the
        estimator stores its class scores, their argmax goes to the buffer as without it, and the tracker overwrites the rows that are
        on -- before the WORLD select, the followers and the transform.  voicing: after the estimator or the tracker, the f0 of the
        unvoiced frames of the rows that are on becomes 0, again before the WORLD select, the followers and the transform"""
        def body(buf):
            if self.pitch_track:
                f0 = self.pe.estimate(spec, out=buf, track=self._track, track_on=self.track_on, track_weight=self.track_weight,
                                      track_jump=self.track_jump, logits_out=track_logits_buf(self, spec, self.pe),
                                      changed=self.track_changed)
            else:
                f0 = self.pe.estimate(spec, out=buf)
            if self.voicing:                                  # the rows that are on: f0 = 0 where their ring is not periodic
                ops.voicing_rows_(f0, data, self._voicing, self.voicing_on, self.voicing_thr_on, self.voicing_thr_off,
                                  self.voicing_floor_e, self._voicing_out)
            rate = self.f0_rate
            if self.world_pitch:
                world_on = self.world_eff if self.gate else (self.world_tick if self.sparse else self.world_on)
                buf.copy_(torch.where(self._world_sel, compute_f0_rows(data, world_on), buf))
                f0, rate = buf, self.f0_rate_eff
            shift = self.pitch
            if self.pitch_range:                              # running (S, W, Q) -> this tick's shifts, intonations and centres
                emit = self.follow if self.gate else self.emit
                pitch_follow2_rows_(f0, rate, self.pitch, self.auto_on, self.target, self.intonation, self.range_on, self.target_sd,
                                    emit, self.auto_decay, self.auto_prior, self.range_max, self.reg_state, self.shift_eff,
                                    self.inton_eff, self.centre, self.centre_on)
                return pitch_transform_rows_centred_(f0, 1, rate, self.shift_eff, self.inton_eff, self.centre, self.centre_on)
            if self.auto_pitch:                               # the sessions' running registers -> this tick's shifts
                emit = self.follow if self.gate else self.emit      # (a gated session's register learns from open ticks only)
                shift = pitch_follow_rows_(f0, rate, self.pitch, self.auto_on, self.target, emit, self.auto_decay,
                                           self.auto_prior, self.reg_state, self.shift_eff)
            return pitch_transform_rows_(f0, 1, rate, shift, self.intonation)
        return f0_on_side_stream(self, spec, body)

    def _device_step(self, data, phi):
        """data float32 [B, ring] on the device, phi [B, 64] -> (wave [B, L] at output_sr, phi_next [B, 64])"""
        if self._rt is None:
            data = resample_rows(data, self.input_sr, 16000, self.in_pre, self.in_post)
        else:
            data = resample_rows_multi(data, self.len_in, self.pair_in, self._rt, self._len16_rows, self._len16, self.in_pre,
                                       self.in_post)
        # (sparse: the push's masked arrays, zero on the rows that sent nothing this tick, stand in for seg_len / world_on)
        seg_len = self.seg_len_tick if self.sparse else self.seg_len
        if self.gate:                                         # this tick's live rows, before the f0 side stream forks off
            w_lo, w_hi = gate_window(self.begin_of_output, self.end_of_output, data.shape[1], self._gate_look16)
            world_on = (self.world_tick if self.sparse else self.world_on) if self.world_pitch else None
            gate_rows(data, w_lo, w_hi, self.gate_on, self.thr_ms, self.hold_ticks, self.emit,
                      world_on, self.S, seg_len, self.gate_state, self.g0, self.g1,
                      self.seg_len_eff, self.follow, self.world_eff)
            seg_len = self.seg_len_eff
        spec = spectrogram(data)
        f0, join = self._f0_on_side_stream(spec, data)
        content = self.ce(spec)
        if self.pitch_track:
            # the f0 branch ends before the search is launched: the grouped scan fills the chip exactly once, and tracker blocks that
            # are resident while it is placed put part of its blocks out of step with the rest (measured: 38.2 -> 41 - 45 ms at B = 128,
            # -c 960 -b 8, for a tracker call of 0.6 ms; DESIGN.md 5.4 "Pitch tracking")
            join()
        K = self.k_max
        if self.match_path:                                   # the per-row-k search, the path over its lists, the gather at gather_k
            b, d, t = content.shape
            rep = content if self.S == 1 else content.unsqueeze(1).expand(b, self.S, d, t).reshape(b * self.S, d, t).contiguous()
            val, idx = knn_search_grouped_k(rep, self.pool.rows, self.pool.norms, self.seg_lo, seg_len, self.k_lists, K)
            # (a sparse converter's rows that do not emit this tick -- filling, stalled -- search nothing: their count stands)
            val, idx, moved = knn_path_rows(val, idx, self.k_lists, K, self.path_on, self.path_weight, self.pool.rows, self.pool.norms,
                                            moved=self._path_moved_tick if self.sparse else self.path_moved_rows)
            if self.sparse:
                emit = self.emit.expand(b, self.S).reshape(b * self.S)
                self.path_moved_rows.copy_(torch.where(emit, moved, self.path_moved_rows))
            if self.S == 1:
                content = merge_gather_rows_k(val, idx, self.gather_k, K, self.alpha, self.pool.rows, content)
            else:
                content = blend_gather_rows_k(val, idx, self.gather_k, K, self.first, self.weight, self.alpha, self.pool.rows, content)
        elif self.S == 1:
            if K is None:
                val, idx = knn_search_grouped(content, self.pool.rows, self.pool.norms, self.seg_lo, seg_len, self.k)
                content = merge_gather_rows(val, idx, self.k, self.alpha, self.pool.rows, content)
            else:                                             # every session at its own k (device array k_rows)
                val, idx = knn_search_grouped_k(content, self.pool.rows, self.pool.norms, self.seg_lo, seg_len, self.k_rows, K)
                content = merge_gather_rows_k(val, idx, self.k_rows, K, self.alpha, self.pool.rows, content)
        else:                                                 # every slot's content once per list row, then the blend
            b, d, t = content.shape
            rep = content.unsqueeze(1).expand(b, self.S, d, t).reshape(b * self.S, d, t).contiguous()     # (B = 1: a view)
            if K is None:
                val, idx = knn_search_grouped(rep, self.pool.rows, self.pool.norms, self.seg_lo, seg_len, self.k)
                content = blend_gather_rows(val, idx, self.k, self.first, self.weight, self.alpha, self.pool.rows, content)
            else:
                val, idx = knn_search_grouped_k(rep, self.pool.rows, self.pool.norms, self.seg_lo, seg_len, self.k_lists, K)
                content = blend_gather_rows_k(val, idx, self.k_rows, K, self.first, self.weight, self.alpha, self.pool.rows,
                                              content)
        join()
        wave, phi_out = self.dec(content, f0=f0, phi=phi, crop=(self.begin_of_output, self.end_of_output))
        self.last_f0 = f0
        if self.post_filter:                                  # the decoder's spectrum first: the envelope sets the level of the filtered wave
            wave = self._postfilter(wave)
        if self.envelope:                                     # the decoder's level -> the source's contour, before all downstream
            wave = self._follow(wave, data)
        if self._rt is None:
            wave = resample_rows(wave, 16000, self.output_sr, self.out_pre, self.out_post)
        else:
            if wave.shape[1] != self._lw:
                raise RuntimeError(f"decoder wave of {wave.shape[1]} samples, the multi-rate edge expects {self._lw}")
            wave = resample_rows_multi(wave, self._lw_rows, self.pair_out, self._rt, self.len_out, self._ld_out, self.out_pre,
                                       self.out_post)
        if self.crossfade:                                    # before the gate's edge: the tail is the un-gated converted wave
            if wave.shape[1] != max(self._row_len.values()):
                raise RuntimeError(f"final wave of {wave.shape[1]} samples, the crossfade expects {max(self._row_len.values())}")
            seam_rows_(wave, self.span_lo, self.shift, self.xlen, self.emit, self.tail, self.stored,
                       self.g0 if self.gate else None, self.g1 if self.gate else None, self.seam_stats)
        if self.gate:
            gate_apply_rows_(wave, self.span_lo, self.span_len, self.g0, self.g1)
        if self.loud:                                         # the long-term level: behind the gate's edge, ahead of the limiter
            loudness_rows_(wave, self.span_lo, self.span_len, self.emit, self.loud_on, self.loud_hop, self.loud_coef, self.loud_par,
                           self.loud_state)
        if self.limiter:                                      # last: the limiter sees what is emitted (the seam's tail stays un-limited)
            if wave.shape[1] != max(self._limit_len.values()):
                raise RuntimeError(f"final wave of {wave.shape[1]} samples, the limiter expects {max(self._limit_len.values())}")
            limit_rows_(wave, self.span_lo, self.span_len, self.limit_shift, self.look, self.hold, self.ceil, self.emit,
                        self.limit_hist, self.limit_gmin)
        # a row that does not emit: 0 -- a filling slot's phase is 0 anyway -- and in a sparse converter its own phase, which is that
        # same 0 while it fills and stands still on a tick it sat out
        phi_next = torch.where(self.emit, phi_out[:, :, self.end_of_output], phi if self.sparse else torch.zeros_like(phi))
        return wave, phi_next

    def enable_graph(self):
        """capture the per-tick device pipeline over [B, ring] once; replays read the per-slot device arrays"""
        saved = self.phi.clone()
        saved_reg = self.reg_state.clone() if self.auto_pitch else None      # (capture_step runs the step three times)
        saved_gate = self.gate_state.clone() if self.gate else None
        saved_seam = self._seam_state()
        # (the follower's outputs too: pitch_range_state() reads inton_eff, and they are the latest tick's until the next one)
        saved_outs = [(a, a.clone()) for a in (self.shift_eff, self.inton_eff, self.centre, self.centre_on)] if self.pitch_range else []
        self._graph, self._g_out = capture_step(self.device, lambda: self._device_step(self._in, self.phi), self.phi)
        self.phi.copy_(saved)
        for a, v in saved_outs:
            a.copy_(v)
        self._seam_restore(saved_seam)
        if saved_reg is not None:
            self.reg_state.copy_(saved_reg)
        if saved_gate is not None:
            self.gate_state.copy_(saved_gate)
        self._graph_pool_version = self.pool.version
        self.captures += 1
        return self

    def _seam_state(self):
        """a copy of the sessions' tails and how much of them is valid (None without crossfade) -- and, in a limiter converter, of
        the limiter's histories and latest gains, and in a loudness converter of the loudness states: (tail, stored, limit_hist,
        limit_gmin, loud_state), the absent parts None"""
        if not (self.crossfade or self.limiter or self.loud):
            return None
        seam = (self.tail.clone(), self.stored.clone()) if self.crossfade else (None, None)
        seam = seam + ((self.limit_hist.clone(), self.limit_gmin.clone()) if self.limiter else (None, None))
        return seam + (self.loud_state.clone() if self.loud else None,)

    def _seam_restore(self, saved):
        if saved is not None:
            if saved[0] is not None:
                self.tail.copy_(saved[0])
                self.stored.copy_(saved[1])
            if len(saved) > 2 and saved[2] is not None:
                self.limit_hist.copy_(saved[2])
                self.limit_gmin.copy_(saved[3])
            if len(saved) > 4 and saved[4] is not None:
                self.loud_state.copy_(saved[4])

    def _run(self):
        if self._reserved:
            self._follow_pool()
        if self._graph is not None:
            if self._graph_pool_version != self.pool.version:        # the pool was re-packed: its rows moved
                self.enable_graph()
            self._graph.replay()
            return self._g_out
        wave, phi_next = self._device_step(self._in, self.phi)
        self.phi.copy_(phi_next)
        return wave

    def _repeat_on_bf16(self, saved_phi, saved_reg=None, saved_gate=None, saved_seam=None):
        """RealtimeConverter._repeat_on_bf16 for the whole tick: modes 2, every slot's phase (and running register, gate state and
        crossfade tail) restored, the tick again"""
        return audio_io.float_to_pcm16(self._repeat_wave(saved_phi, saved_reg, saved_gate, saved_seam)).cpu().numpy()

    def _repeat_wave(self, saved_phi, saved_reg=None, saved_gate=None, saved_seam=None):
        """the repeated tick's waves on the device.  The tick reads _in, which the repeat leaves as it is: a sparse converter's rings
        were pushed before the first attempt and are not pushed again"""
        ops.switch_to_bf16("multi-session streaming step", "tick")
        self.phi.copy_(saved_phi)
        if saved_reg is not None:
            self.reg_state.copy_(saved_reg)
        if saved_gate is not None:
            self.gate_state.copy_(saved_gate)
        self._seam_restore(saved_seam)
        if self._graph is not None:
            self.enable_graph()
        return self._run()

    def _chunk_of(self, s, c):
        """a slot's chunk as a flat int16 array of the slot's chunk length (ValueError otherwise)"""
        c = np.asarray(c, dtype=np.int16).reshape(-1)
        cs = self.slot_chunk[s]
        if c.shape[0] != cs:
            raise ValueError(f"slot {s}: chunk of {c.shape[0]} samples, expected {cs} (the session runs at {self.rate[s]} Hz)")
        return c

    def _emit_spans(self, wave):
        """the emitting rows' spans of the tick's waves as int16, cut on the device: one [B, widest span] copy to the host"""
        emit_rows_(wave, self.span_lo, self.span_len, self.emit, self._pcm)
        self._pcm_host.copy_(self._pcm, non_blocking=True)
        torch.cuda.current_stream(self.device).synchronize()
        return self._pcm_host.numpy()

    def _lost_slots(self, chunks, lost):
        """step()'s `lost` -> the sorted list of its slots: open slots whose chunk did not arrive, none of them a key of `chunks`;
        ValueError otherwise, and for any lost slot in a converter built without conceal.  Host only"""
        lost = list(lost) if lost is not None else []
        if not lost:
            return []
        if not self.conceal:
            raise ValueError("step(..., lost=) needs a converter built with MultiStreamConverter(..., sparse=True, conceal=True): "
                             "without one a lost chunk is a chunk of zeros")
        out = set()
        for s in lost:
            s = self._slot(s)
            if not self.is_open[s]:
                raise ValueError(f"a lost chunk for slot {s}, which is not open")
            if s in chunks:
                raise ValueError(f"slot {s} is named in both chunks and lost: its chunk arrived or it did not")
            out.add(s)
        return sorted(out)

    def _step_sparse(self, chunks, lost=()):
        """step() of a sparse converter: any subset of the open slots"""
        taken = {}
        for s, c in chunks.items():
            self._slot(s)
            if not self.is_open[s]:
                raise ValueError(f"a chunk for slot {s}, which is not open")
            taken[int(s)] = self._chunk_of(s, c)
        lost = self._lost_slots(taken, lost)
        out = {s: None for s in list(chunks) + lost}
        if not taken and not lost:                            # nobody sent anything: nothing moves
            return out
        if self._staged is not None:
            self._staged.synchronize()                        # (the pinned buffers are free again: the latest upload has been made)
        stage, flags = self._stage.numpy(), self._flags_host.numpy()
        flags[:] = False
        for s, c in taken.items():
            stage[s, :c.shape[0]] = c
            self.count[s] += 1
            flags[0, s] = True
            flags[1, s] = self.count[s] > self.buffersize
        conceal = bool(lost)                                  # does this tick have a lost or a recovering slot?
        for s in taken:
            if self.conceal and self._conceal_run[s]:         # the first chunk after a run: faded in on the device
                conceal, self._conceal_run[s] = True, False
        for s in lost:                                        # the clock goes on as if a chunk had come: the device makes one up
            stage[s, :self.slot_chunk[s]] = 0                 # (zeros if the session does not conceal)
            self.count[s] += 1
            flags[0, s] = flags[2, s] = True
            flags[1, s] = self.count[s] > self.buffersize
            self._conceal_run[s] = self._conceal_host[s]
        emit = flags[1].copy()
        if self._reserved:
            self._follow_pool()                               # seg_len as the pool lies now, before the push masks it
        self._chunks_dev.copy_(self._stage, non_blocking=True)
        self._flags.copy_(self._flags_host, non_blocking=True)
        self._staged = torch.cuda.Event()
        self._staged.record(torch.cuda.current_stream(self.device))
        # once per tick, outside the captured step and outside what the bf16 repeat runs again
        if conceal:                                           # the lost rows' chunks are made up, the recovering rows' heads faded in
            conceal_rows_(self.ring_dev, self.ring_len, self._chunks_dev, self.chunk_len, self.present, self.lost, self.conceal_on,
                          self._conceal_consts, self._conceal_state, self.conceal_tmpl)
            self.conceals += 1
        ring_push_rows_(self.ring_dev, self._chunks_dev, self.chunk_len, self.ring_len, self.present, self._in, self.seg_len,
                        self.seg_len_tick, self.S, self.world_on if self.world_pitch else None, self.world_tick)
        self.pushes += 1
        if not emit.any():                                    # the present rings moved on; no network work
            return out
        guarded = fp16_guarded(self.B * self.frames)
        if guarded:
            saved_phi = self.phi.clone()
            saved_reg = self.reg_state.clone() if self.auto_pitch else None
            saved_gate = self.gate_state.clone() if self.gate else None
            saved_seam = self._seam_state()
        o = self._emit_spans(self._run())
        if guarded and ops.f16_saturations(reset=True) > 0:
            o = self._emit_spans(self._repeat_wave(saved_phi, saved_reg, saved_gate, saved_seam))
        for s in list(taken) + lost:
            if emit[s]:
                out[s] = o[s, :2 * (self.slot_chunk[s] // 2)].copy()
        return out

    def step(self, chunks, lost=()):
        """{slot: int16 chunk} for EVERY open slot -> {slot: converted centre chunk (int16) or None while its ring fills}.
        A session at rate r sends and receives chunks of chunk_r = chunk * r / input_sr samples; its output is cut at its own
        centre, buffersize * chunk_r // 2 +- chunk_r // 2 (realtime_inference.py at that rate), so an odd chunk_r (441 at 44.1 kHz
        with 160-sample chunks at 16 kHz) returns chunk_r - 1 samples per tick, as the reference does.
        A sparse converter takes the chunks of ANY subset of its open slots: a slot without one sits the tick out (nothing of it
        moves, it is not a key of the result), see "Sparse ticks" in the module docstring.
        lost (a sparse converter built with conceal=True): open slots whose chunk did not arrive while their clock must go on; they
        advance exactly as if a chunk had been supplied and are keys of the result, see "Lost chunks" there."""
        if self.sparse:
            return self._step_sparse(chunks, lost)
        self._lost_slots(chunks, lost)                        # (a dense converter has no conceal: any lost slot is refused)
        for s in chunks:
            self._slot(s)
            if not self.is_open[s]:
                raise ValueError(f"a chunk for slot {s}, which is not open")
        missing = [s for s in range(self.B) if self.is_open[s] and s not in chunks]
        if missing:
            raise ValueError(f"open slots {missing} supplied no chunk this tick")
        emit = [False] * self.B
        for s, c in chunks.items():
            c = self._chunk_of(s, c)
            cs = self.slot_chunk[s]
            n = cs * self.buffersize
            self.ring[s, :n - cs] = self.ring[s, cs:n]
            self.ring[s, n - cs:n] = c
            self.count[s] += 1
            emit[s] = self.count[s] > self.buffersize
        out = {s: None for s in chunks}
        if not any(emit):
            return out
        self.emit.copy_(torch.tensor(emit, device=self.device).view(self.B, 1))
        pcm = torch.from_numpy(self.ring).to(self.device)
        self._in.copy_(audio_io.pcm16_to_float(pcm))
        guarded = fp16_guarded(self.B * self.frames)
        if guarded:
            saved_phi = self.phi.clone()
            saved_reg = self.reg_state.clone() if self.auto_pitch else None
            saved_gate = self.gate_state.clone() if self.gate else None
            saved_seam = self._seam_state()
        o = audio_io.float_to_pcm16(self._run()).cpu().numpy()
        if guarded and ops.f16_saturations(reset=True) > 0:
            o = self._repeat_on_bf16(saved_phi, saved_reg, saved_gate, saved_seam)
        for s in chunks:
            if emit[s]:
                cs = self.slot_chunk[s]
                center = self.buffersize * cs // 2
                out[s] = o[s, center - cs // 2: center + cs // 2].copy()
        return out
