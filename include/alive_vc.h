/*
 * alive_vc.h -- C ABI of libalive_vc.so (MI355X / gfx950 voice-conversion hot path).
 *
 * The reference (uthree/ALiVE-VC) is pure PyTorch and has no FFI of its own;
 * its boundary is the Python call surface of its module package.  This header is the
 * native surface that the alive-vc_amd/module package binds with ctypes to implement
 * that Python surface.  Each entry point names the reference function it
 * replaces.
 *
 * Conventions (all entry points):
 *   - every pointer is a DEVICE pointer (tensor.data_ptr()); fp32 unless noted
 *   - activations are [N][C][T], T contiguous (the reference's layout)
 *   - `stream` is a hipStream_t passed as void*
 *   - no allocation, no synchronisation, no host<->device copy inside: any
 *     call sequence can be captured into a hipGraph.  Scratch comes from the
 *     caller via the *_workspace_bytes queries.
 *   - return 0 on success, negative on error; alive_last_error() gives a
 *     thread-local message.
 */
#ifndef ALIVE_VC_H
#define ALIVE_VC_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ALIVE_OK 0
#define ALIVE_ERR_ARG (-1)
#define ALIVE_ERR_LAUNCH (-2)

#define ALIVE_DIM 768          /* content feature width (voice_library.py:7) */
#define ALIVE_KPRIME 16        /* candidates kept per frame and library split by the bf16 stage (the fp8 stage keeps 32) */
#define ALIVE_MAX_K 64         /* largest k accepted by the kNN entry points (the reference takes any k <= M, inference.py:34 /
                                * common.py:105).  k <= 8 runs through the MFMA candidate stages (a half-list of the bf16
                                * stage is 8 deep, and all k true neighbours may fall into one of them); 8 < k <= 64 runs the
                                * exact fp32 scan for every frame                                              */

const char* alive_last_error(void);
int alive_version(void);

/* ---------------------------------------------------------------- kNN ----
 * Replaces match_features (module/common.py:96-109) and VoiceLibrary.match
 * (module/voice_library.py:15-33).
 *
 * alive_library_pack: tokens[D][M] (the on-disk layout of voice_library.pt,
 *   generate_voice_library.py:42, batch dim dropped) ->
 *     lib_bf16[M_pad][D]  L2-normalised rows, bf16 (MFMA scoring operand;
 *                         M_pad = alive_library_padded_rows(M), pad rows zero)
 *     rows_f32[M][D]      raw rows, fp32 (exact rescoring + gather)
 *     norms[M]            fp32 L2 norm of each row
 */
int64_t alive_library_padded_rows(int64_t M);
int alive_library_pack(const float* tokens_DxM, int64_t M, int D,
                       void* lib_bf16, float* rows_f32, float* norms, void* stream);

/* alive_knn_search: exact top-k of one library shard, bf16 MFMA candidate stage first.
 *   src[N][D][T] fp32 source frames; frames are flattened to Tt = N*T.
 *   bf16 MFMA cosine scoring with lane-private top-k' lists in LDS, then exact fp32 rescoring (normalise-then-dot, as
 *   the reference) of every candidate.  Every frame is then CERTIFIED: a row outside its rescored set has a candidate
 *   score <= c (the floor of the partial list it failed to enter, or the best candidate the selection of 64 dropped),
 *   hence an exact cosine <= c - min(mu, 0) + max(7 sigma, 2 max|e|), with mu / sigma / max|e| the mean, the RMS about zero
 *   (floored by the stage's typical error) and the largest magnitude of the candidate-score error measured on that frame's
 *   own rescored candidates; the frame passes if its k-th exact cosine clears that.  This certificate is STATISTICAL: it is
 *   wrong for a frame only if the stage error of one of its k true neighbours lies beyond those 7 sigma (audited:
 *   tools/knn_audit.py, profiles/r03_knn_audit.json; alive_knn_search_strict is the form without any such assumption).
 *   Frames that do not pass go through the COLLECT tier: the same bf16 scoring pass with a fixed per-frame threshold (the
 *   frame's k-th exact cosine so far minus the slack it was tested with) that keeps EVERY row at or above it for exact
 *   rescoring -- final unless more such rows exist than its lists hold (clusters of near-copies), and only those frames are searched
 *   again by the exact tier inside the same call: a brute-force fp32 scan of the whole shard with the rescoring
 *   arithmetic (launched up front, sized on the device, no sync).  k > 8: the exact scan for every frame.
 *   out_val[Tt][k] fp32 cosine, descending; out_idx[Tt][k] = idx_base + row.
 *   ws: alive_knn_workspace_bytes(Tt, M) bytes -- the bound that is sufficient for EVERY search entry point of this header, the strict
 *   search with a lo-plane library included (that entry point takes no size argument, so the general query must cover it).
 */
size_t alive_knn_workspace_bytes(int64_t Tt, int64_t M);
/* the same bound under its explicit name: alive_knn_search_strict with lib_lo != NULL keeps both bf16 planes of the frames
 * (2 x 1.5 KB per frame) for its split-bf16 collect tier */
size_t alive_knn_workspace_bytes_strict(int64_t Tt, int64_t M);
/* the smaller workspace of every search WITHOUT a lo-plane library (alive_knn_search, _fp8, _fp6, alive_knn_search_strict with
 * lib_lo == NULL): 3 KB per frame less.  Never hand a buffer of this size to alive_knn_search_strict with lib_lo != NULL. */
size_t alive_knn_workspace_bytes_fast(int64_t Tt, int64_t M);
int alive_knn_search(const float* src, int N, int T,
                     const void* lib_bf16, const float* rows_f32, const float* norms,
                     int64_t M, int64_t idx_base, int k,
                     float* out_val, int32_t* out_idx, void* ws, void* stream);

/* Strict form of alive_knn_search: the same bf16 candidate stage, but the certificate is DETERMINISTIC -- a row outside a
 * frame's rescored set has an exact cosine <= c + || q^ - bf16(q^) || + 1.004 max_R || r^ - bf16(r^) || + 1.0e-4
 * (Cauchy-Schwarz on the two rounding-error vectors; the last term bounds the fp32 accumulation of the stage and the
 * rounding of the rescoring arithmetic).  Frames that do not clear it go through the exact fp32 scan, so the returned
 * lists are the exact top-k of the rescoring arithmetic for EVERY input, adversarial ones included.
 *   bound: device float[1] = max_R || r^ - bf16(r^) ||, filled by alive_library_rounding_bound from a packed library.
 *   lib_lo: NULL, or the library's lo plane (alive_library_pack_lo: bf16(r^ - lib_bf16), 2 * 768 * alive_library_padded_rows(M)
 *           bytes).  With it the frames that fail the certificate (more than 256 of them) go through an MFMA COLLECT pass on BOTH
 *           planes of both operands (three bf16 products per product) whose deterministic bound is 3.0e-4 (two-plane rounding
 *           3 x 2^-18 + the fp32 accumulation of 3 x 768 products, priced for a truncating adder) instead of the single-plane collect tier, whose band is the
 *           certificate's own 1.8e-3: every row at or above v_k - 3.0e-4 is rescored exactly, and only frames with more such rows
 *           than the lists hold reach the exact scan.  ws must then hold alive_knn_workspace_bytes_strict(Tt, M) bytes.
 *   ev_start / ev_stop: as in the *_timed forms below (NULL: none).  Counters: alive_knn_search_stats [1], [7], [8]. */
int alive_library_rounding_bound(const void* lib_bf16, const float* rows_f32, const float* norms, int64_t M,
                                 float* bound, void* stream);
int alive_library_pack_lo(const void* lib_bf16, const float* rows_f32, const float* norms, int64_t M, void* lib_lo, void* stream);
int alive_knn_search_strict(const float* src, int N, int T,
                            const void* lib_bf16, const void* lib_lo, const float* rows_f32, const float* norms, const float* bound,
                            int64_t M, int64_t idx_base, int k,
                            float* out_val, int32_t* out_idx, void* ws, void* stream, void* ev_start, void* ev_stop);

/* The same search with the first candidate stage on the block-scaled fp8 MFMA (v_mfma_scale_f32_32x32x64_f8f6f4, OCP e4m3
 * operands = normalised rows x 2^8, scales 2^0): about twice the scoring rate at ~20x the score error of bf16, so the
 * lists hold twice as many candidates (32 per frame and library split) in front of the same exact fp32 rescoring.
 *   lib_f8[M_pad][D]: alive_library_fp8_bytes(M) bytes, made from lib_bf16 by alive_library_pack_fp8.
 *   Same workspace, same outputs and the same contract as alive_knn_search.
 * Tiers, all launched up front and decided on the device (no sync, graph-capturable):
 *   probe  batches of >= 16384 frames: the fp8 stage and its certificate on a sample of 1024 frames; when more than 55 %
 *          of the sample fail (a library whose best cosines lie closer together than the fp8 error) the fp8 pass over
 *          the batch is skipped and every frame starts at the bf16 stage;
 *   fp8    candidates, exact rescoring, certificate (fp8 error statistics).  Batches of >= 512 x 256 frames: the blocks of
 *          library split s start their candidate lists at the seeds split s - 1 left for their frames (k-th best fp8 score seen so
 *          far minus 0.02: rows below it are never admitted, and the certificate counts the seed as the bound on them);
 *   bf16   the frames that failed (up to 64 of them: straight to the exact scan), compacted, through the bf16 stage:
 *          candidates, rescoring, certificate (bf16 statistics);
 *   collect the frames that failed again: bf16 scoring pass with a fixed threshold, every row above it rescored exactly;
 *   exact  the frames whose collected rows overflowed: brute-force fp32 scan.
 * alive_knn_search_stats: device pointer (inside ws) to int[16] counters of the last search on that workspace:
 *   [0] frames that failed the fp8 certificate (<= 64: exact scan; more: the bf16 stage)
 *   [1] frames that failed the bf16 certificate (<= 256: exact scan; more: the collect tier)  [8] frames the collect tier
 *   sent on to the exact scan  [2] probe sample size  [3] probe failures  [9] / [10] fp8 / bf16 blocks that started from seeds
 *   [11] / [12] the two limits just named (64, 256), written with the counters
 *   [4] 1 = the probe chose bf16 first  [7] the path taken: 1 streaming scan, 2 exact scan of every frame (k > 8),
 *   3 bf16 first, 4 fp8 first, 5 fp6 first.  (alive_knn_search fills [1] and [7] only.)  The counters sit at the start of ws. */
size_t alive_library_fp8_bytes(int64_t M);
int alive_library_pack_fp8(const void* lib_bf16, int64_t M, void* lib_f8, void* stream);
int alive_knn_search_fp8(const float* src, int N, int T,
                         const void* lib_f8, const void* lib_bf16, const float* rows_f32, const float* norms,
                         int64_t M, int64_t idx_base, int k,
                         float* out_val, int32_t* out_idx, void* ws, void* stream);
const int* alive_knn_search_stats(int N, int T, int64_t M, void* ws);
/* Debug (the candidate-stage tests): where the first stage's buffers sit in the workspace of a search of Tt frames against M rows at
 * this k (sub != 0: the workspace of alive_knn_search_fp6_sub_timed) and the plans of its three stages; host arithmetic only.
 *   out[0 .. 6]   byte offsets from the workspace base: frames as bf16 [Tt_pad][768], the frames' fp8 / fp6 codes, the per-frame fp6
 *                 clip flags, the subspace codes [.][512] and g (-1 without sub), candidate values, candidate indices;  out[7] bytes
 *   out[8 .. 19]  Tt_pad, tiles_total, tiles_per_split, P (library splits) of the bf16, the fp8 and the fp6 / subspace stage
 *   out[20 .. 24] candidates per frame and split (bf16 stage, block-scaled stages), frames per block (256-frame kernels, fp6
 *                 kernels), library rows per tile.  Candidates are [frame][P][candidates per split].  n_out >= 25.
 *   out[25 .. 26] (n_out >= 27; -1 without sub) byte offsets of alive_knn_search_unit's change of basis: the frames' two k-blocked bf16
 *                 planes [2][24][cols_pad][32] and y_sub [N][576][T] fp32.
 *   out[27 .. 31] (n_out >= 32) Tt_pad, tiles_total, tiles_per_split, P of the wide subspace kernel's plan and its frames per block (512). */
int alive_debug_knn_stage_view(int64_t Tt, int64_t M, int k, int sub, int64_t* out, int n_out);
/* Debug (tests/test_gpu_knn_sub_wide.py): the subspace candidate stage alone, the library cut into `split` ranges of the caller's choosing.
 * s_sub [Tt_pad][512] frame codes and g [Tt_pad] (Tt_pad a multiple of 1536), lib_sub / rho from alive_library_pack_fp6_sub, cand_val /
 * cand_idx [Tt_pad][split][32].  The kernel is chosen as in the search (alive_knn_sub_frames, at most 65 535 tiles per split for the
 * 512-frame kernel; mode 0 counts as 512); *frames_out (host) receives its frames per block, 384 or 512.  Unseeded. */
int alive_debug_knn_sub_stage(const void* s_sub, const float* g, int64_t Tt_pad, const void* lib_sub, const float* rho, int64_t M, int split,
                              float* cand_val, int32_t* cand_idx, int* frames_out, void* stream);

/* TEST ONLY (tests/test_gpu_knn_cert.py): the rescoring kernel that ends every search, launched by the searches' own dispatcher on
 * the caller's device buffers -- every argument the searches forward, under the names of knn_rescore_kernel (csrc/knn.hip), plus the
 * sizes the entry validates against.  The grid covers Tt slots, four per block.  Certify mode: flag_list != NULL and collect == 0.
 * Checked before the launch: 1 <= k <= 8, P * kp <= 1024, list_len 8 or 16, in certify mode P * kp a multiple of list_len,
 * gate_lo == -2 (on / off word) only with a gate_cnt, otherwise gate_lo <= gate_hi, a frame_list or Tt <= frames, det_q and det_lib
 * together, collect and thr_list only with a flag_list, a flag_cnt with every flag_list.  Host memory is not read by the kernels and
 * device memory is not read by the entries: what the index arrays hold is the caller's to check. */
typedef struct AliveRescoreArgs {
    const float* cand_val;       /* [Tt][P][kp] stage scores, in units of 1 / pre_scale */
    const int32_t* cand_idx;     /* [Tt][P][kp] library rows; -1 empty, -2 an overflowed collect list */
    int P, kp;
    const float* s_f32;          /* [frames][768] */
    const float* rows;           /* [M][768] */
    const float* norms;          /* [M] */
    int64_t M, frames, Tt, idx_base;
    int k;                       /* entries per frame of out_val / out_idx */
    float* out_val;              /* [frames][k] */
    int32_t* out_idx;
    const int32_t* frame_list;   /* [Tt] slot -> frame, or NULL: slot = frame */
    const int32_t* gate_cnt;
    int gate_lo, gate_hi;
    int32_t* flag_list;          /* [Tt] */
    int32_t* flag_cnt;
    float zsig;
    int list_len;
    float pre_scale, sd_prior;
    const float* det_q;          /* [frames] or NULL */
    const float* det_lib;        /* [1], pool form [voices] */
    float* thr_list;             /* [Tt] or NULL */
    int collect;
    float overflow_slack;
    const unsigned char* force_fail;   /* [frames] or NULL; not used by the pool form */
} AliveRescoreArgs;
int alive_debug_knn_rescore(const AliveRescoreArgs* a, void* stream);
/* the pool search's form (certify mode only, a frame_list required): slots of a plan, frame_list its slot -> frame map (-1: padding), group g's failing
 * slots listed at fb[grp[g][blk0] * 256 + 0 .. gfail[g] - 1], flag_cnt counts them all, flag_list only switches the certificate on. */
int alive_debug_knn_rescore_pool(const AliveRescoreArgs* a, const int32_t* slot_grp, const int32_t* grp, int32_t* gfail, int32_t* fb,
                                 int groups, void* stream);
/* layout of a grp record: out[0 .. 3] = words per group, index of the voice, of the first 256-slot block, of the group's k */
int alive_debug_knn_pool_fields(int32_t* out, int n_out);

/* Measurement forms (bench.py): the same searches; ev_start / ev_stop are hipEvent_t handles (or NULL) recorded on `stream`
 * immediately before / after the first-stage scoring kernel of the whole batch -- the dominant kernel of the path. */
int alive_knn_search_timed(const float* src, int N, int T,
                           const void* lib_bf16, const float* rows_f32, const float* norms,
                           int64_t M, int64_t idx_base, int k,
                           float* out_val, int32_t* out_idx, void* ws, void* stream, void* ev_start, void* ev_stop);
int alive_knn_search_fp8_timed(const float* src, int N, int T,
                               const void* lib_f8, const void* lib_bf16, const float* rows_f32, const float* norms,
                               int64_t M, int64_t idx_base, int k,
                               float* out_val, int32_t* out_idx, void* ws, void* stream, void* ev_start, void* ev_stop);

/* Round 6: the fp8 search on ROTATED operands, for DENSE banks (a single speaker: every row shares a large common component, thousands
 * of rows lie inside an 8-bit stage's error of a frame's k-th neighbour and the plain fp6 / fp8 stages certify next to nothing).  The
 * unit vectors are expressed in a basis of the bank's own subspace -- 64 leading principal directions, carried as two e4m3 digits each,
 * and 512 further coordinates mixed by a fixed rotation; /root/reference/module/content_encoder.py ends in Conv1d(512 -> 768), so a bank
 * has rank <= 513 and nothing is lost -- and laid out so that the unchanged scoring kernel's dot product of the two 768-code vectors is
 * the cosine at a stage error of 2.4e-4 instead of 1.6e-3 (profiles/r06_knn_pca_probe.json; csrc/knn.hip rot_codes_kernel).  The
 * caller owns the basis (module/common.py::PackedLibrary builds it when a bank is packed and rotates the frames with alive_conv1d):
 *   alive_knn_rot_coordinates() = 576 coordinates per vector are passed: the first alive_knn_rot_leading() = 64 the leading directions,
 *       the next alive_knn_rot_mixed() = 507 the mixed ones, the last 5 unread;
 *   c0: the bank's centring constant of the leading coordinate (an e4m3-exact value near the mean of the rows' first coordinate: that
 *       coordinate is ~0.65 for every vector of a dense bank and is carried as c0 + two digits of the difference);
 *   alive_library_pack_fp8_rot: y_rows[count][576] = coordinates of the UNIT rows m0 .. m0 + count - 1 -> their codes in lib_f8
 *       (alive_library_fp8_bytes(M) bytes; chunks in ascending order, m0 a multiple of 32, the last chunk ends at M);
 *   alive_knn_search_fp8_rot_timed: alive_knn_search_fp8_timed with y_rot[N][576][T] = W^T src (not normalised) beside src.
 * Results are those of every other search: exact fp32 rescoring on the original rows, the same certificates (stage prior 2.5e-4),
 * the bf16 tiers on lib_bf16 behind them. */
int alive_knn_rot_coordinates(void);
int alive_knn_rot_leading(void);
int alive_knn_rot_mixed(void);
int alive_library_pack_fp8_rot(const float* y_rows, int64_t m0, int64_t count, int64_t M, float c0, void* lib_f8, void* stream);
int alive_knn_search_fp8_rot_timed(const float* src, const float* y_rot, float c0, int N, int T,
                                   const void* lib_f8_rot, const void* lib_bf16, const float* rows_f32, const float* norms,
                                   int64_t M, int64_t idx_base, int k,
                                   float* out_val, int32_t* out_idx, void* ws, void* stream, void* ev_start, void* ev_stop);

/* Round 5: the same tiered search with the first candidate stage on the fp6 form of that MFMA (OCP e2m3 operands on both sides =
 * normalised rows x 2^5, scales 2^0; /root/reference/module/common.py:100-105 is still what comes out).  The matrix pipe runs e2m3
 * at twice the e4m3 rate, and for unit vectors a 1/8 grid is as accurate as three mantissa bits (score error 1.8e-3 in cosine
 * against 1.35e-3): the per-frame certificate is the fp8 stage's with a prior of 2.0e-3, the lists are as deep (32 candidates per
 * frame and library split), frames that fail go to the bf16 stage exactly as above.  A wave keeps 96 frames stationary (216
 * registers) and a block 384, so one 32-byte LDS fragment feeds three MFMAs.
 *   lib_f6[M_pad][D]: alive_library_fp8_bytes(M) bytes from alive_library_pack_fp6 -- every group of 32 features keeps its 32-byte
 *   slot: 32 six-bit codes as a little-endian bit stream in the first 24 bytes, 8 bytes of zeros.
 *   Workspace, outputs, counters (alive_knn_search_stats; [7] = 5: fp6 first) as for alive_knn_search_fp8. */
int alive_library_pack_fp6(const void* lib_bf16, int64_t M, void* lib_f6, void* stream);
int alive_knn_search_fp6(const float* src, int N, int T,
                         const void* lib_f6, const void* lib_bf16, const float* rows_f32, const float* norms,
                         int64_t M, int64_t idx_base, int k,
                         float* out_val, int32_t* out_idx, void* ws, void* stream);
int alive_knn_search_fp6_timed(const float* src, int N, int T,
                               const void* lib_f6, const void* lib_bf16, const float* rows_f32, const float* norms,
                               int64_t M, int64_t idx_base, int k,
                               float* out_val, int32_t* out_idx, void* ws, void* stream, void* ev_start, void* ev_stop);

/* The subspace form of the fp6 stage (knn.hip knn_sub6_kernel): the content encoder's frames are q = W h + b with W 768 x 512, so
 * q^ . r^ = x_f . y_r + g_f rho_r with x = U^T q^, y = U^T r^ (U an orthonormal basis of span(W)), g = u . q^, rho = u . r^ (u the unit
 * part of b outside span(W)).  The candidate stage scores the 512 coordinates on the fp6 MFMA and adds g_f rho_r in fp32; rescoring,
 * certificate and the tiers behind it are the plain fp6 search's, on the original rows.
 *   alive_library_pack_fp6_sub: y_rows [count][alive_knn_sub_coordinates()] fp32 = [U | u]^T r^ of unit rows m0 .. m0 + count - 1
 *     (m0 a multiple of 32) -> lib_sub (alive_library_fp6_sub_bytes(M)) and rho [M_pad]; *clip (device int, zeroed by the caller) is
 *     set when a code clipped (the caller keeps the plain stage then).
 *   alive_knn_search_fp6_sub_timed: y_sub = [U | u]^T src as [N][alive_knn_sub_coordinates()][T] (unnormalised); lib_f6 is the plain
 *     fp6 image: frames that leave the subspace (or clip) are forced into the next tier, and when more than 64 of a batch do, the
 *     batch is scored by the plain fp6 kernel instead -- decided on the device, no host sync.  ev_start / ev_stop bracket the
 *     scoring launches.  Counters (alive_knn_search_stats): [14] frames flagged, [15] of them clipped, [21] which kernel scored
 *     (1 subspace, 2 plain fp6, 0 neither: the probe chose bf16 first). */
int alive_knn_sub_coordinates(void);
/* Which kernel scores the subspace stage (process-wide; not to be changed while a search is in flight):
 *   mode 384: knn_sub6_kernel, 96 stationary frames per wave, 384-frame blocks;
 *   mode 512: knn_sub6w_kernel, 128 stationary frames per wave, 512-frame blocks, whenever a library split has at most 65 535 tiles
 *             (its lists hold 16-bit tile offsets; beyond that the 384-frame kernel runs);
 *   mode < 0: back to the rule: the 512-frame kernel when the batch fills at least 300 of its frame blocks (seeded admission on) and a
 *             split has at most 65 535 tiles.  The rule reads the frame count and M only.  The initial state, unless
 *             ALIVE_KNN_SUB_FRAMES is 384 or 512;
 *   mode 0:   query.  Returns the mode in force: 384, 512, or 0 for the rule.
 * Either kernel leaves the same candidate layout; the search's results are the exact top-k in both.  Counter [22] of
 * alive_knn_search_stats tells which one the last subspace search launched (384 / 512). */
int alive_knn_sub_frames(int mode);
size_t alive_knn_workspace_bytes_sub(int64_t Tt, int64_t M);      /* the workspace of alive_knn_search_fp6_sub_timed */
size_t alive_library_fp6_sub_bytes(int64_t M);
int alive_library_pack_fp6_sub(const float* y_rows, int64_t m0, int64_t count, int64_t M, void* lib_sub, float* rho, int* clip,
                               void* stream);
int alive_knn_search_fp6_sub_timed(const float* src, const float* y_sub, int N, int T, const void* lib_sub, const float* rho,
                                   const void* lib_f6, const void* lib_bf16, const float* rows_f32, const float* norms, int64_t M,
                                   int64_t idx_base, int k, float* out_val, int32_t* out_idx, void* ws, void* stream,
                                   void* ev_start, void* ev_stop);

/* Unit rows, packed once per library: rows_hat[M][768] = fl(rows_f32[r][d] / norms[r]), the quotient every exact tier forms on every
 * call (IEEE fp32 division).  alive_knn_search_unit is every tiered search above behind one entry -- `form` names the entry it stands
 * for, the members are that entry's arguments under their names there -- whose rescoring passes read rows_hat instead of dividing:
 * (val, idx) are bitwise the named entry's.  rows_f32 and norms are still needed (exact scan tiers; the gather returns the original
 * rows).  rows_hat NULL: the named entry's own arithmetic.  In the ALIVE_KNN_FP6_SUB form the frames' plain fp6 image is built only
 * when it is read (a due probe, or the device-side gate sending the batch to the plain stage): frames whose plain image clips while
 * their subspace image does not are no longer forced to the bf16 tier.  Workspace and counters as for the named entry.
 *   lib_stage: lib_f8 / lib_f6 / lib_f8_rot of the form (unused by BF16 and STRICT); y: y_rot (FP8_ROT) or y_sub (FP6_SUB);
 *   sub_w (FP6_SUB, with y NULL): [U | u]^T as two-plane weights [2][768 / 32][576][32] (module/_pack.py::pack_conv_split of the
 *   1x1 conv) -- the search forms y_sub itself: alive_to_planes of src and alive_gemm_planes (2 planes) into the subspace workspace;
 *   bound / lib_lo: STRICT only; ev_start / ev_stop may be NULL. */
enum { ALIVE_KNN_BF16 = 0, ALIVE_KNN_STRICT = 1, ALIVE_KNN_FP8 = 2, ALIVE_KNN_FP6 = 3, ALIVE_KNN_FP8_ROT = 4, ALIVE_KNN_FP6_SUB = 5 };
typedef struct AliveKnnSearch {
    int form;
    int N, T, k;
    const float* src;
    const void* lib_stage;
    const void* lib_bf16;
    const void* lib_lo;
    const float* rows_f32;
    const float* norms;
    const float* rows_hat;
    const float* bound;
    const float* y;
    const void* lib_sub;
    const float* rho;
    const void* sub_w;
    float rot_c0;
    int64_t M, idx_base;
    float* out_val;
    int32_t* out_idx;
    void* ws;
    void* ev_start;
    void* ev_stop;
} AliveKnnSearch;
int alive_library_pack_unit_rows(const float* rows_f32, const float* norms, int64_t M, float* rows_hat, void* stream);
int alive_knn_search_unit(const AliveKnnSearch* a, void* stream);

/* alive_knn_merge_gather: merge n_shards exact top-k lists ([S][Tt][k], e.g.
 * after an RCCL all-gather), pick the global top-k, gather those rows from the
 * full fp32 row table, mean over k, alpha-blend with the source.  n_shards * k <= 512.
 *   out[N][D][T];  final_idx[Tt][k] (may be NULL).
 */
int alive_knn_merge_gather(const float* cand_val, const int32_t* cand_idx, int n_shards, int k,
                           double alpha, const float* rows_f32_full, const float* src,
                           int N, int T, float* out, int32_t* final_idx, void* stream);

/* ---------------------------------------------- grouped search (multi-session streaming) ----
 * alive_library_pack_rows: the fp32 rows and norms of alive_library_pack alone (bitwise the same norms), for a VOICE POOL:
 *   every voice's tokens[768][M] packed at its own offset of one rows_f32[P][768] / norms[P] table.
 * alive_knn_search_grouped: exact top-k (k <= 8) of every frame of src[N][768][T] against the pool segment of its row:
 *   row n searches rows [seg_lo[n], seg_lo[n] + seg_len[n]) of the pool (seg_lo / seg_len: DEVICE int32[N]); seg_len[n] == 0
 *   marks an inactive row (its frames get val -inf, idx -1), as does a segment outside the pool or shorter than k.
 *   out_val / out_idx [N*T][k]: val and idx - seg_lo[n] are bitwise what alive_knn_search_strict returns for the frame against
 *   the segment packed alone (ties to the lower row); idx is a POOL index, ready for alive_knn_merge_gather(_rows) on rows_f32.
 *   Every launch is sized from N, T and k: the segment table may change between replays of a captured hipGraph.  Rows that
 *   search the same segment share one pass over it.  N <= 1024, N * T <= 2^20.
 *   ws: alive_knn_grouped_workspace_bytes(N, T, k) bytes (0: arguments out of range). */
int alive_library_pack_rows(const float* tokens, int64_t M, int Dd, float* rows_f32, float* norms, void* stream);
size_t alive_knn_grouped_workspace_bytes(int N, int T, int k);
int alive_knn_search_grouped(const float* src, int N, int T, const float* rows_f32, const float* norms, int64_t P,
                             const int32_t* seg_lo, const int32_t* seg_len, int k, float* out_val, int32_t* out_idx,
                             void* ws, void* stream);
/* alive_knn_merge_gather with one shard and a per-window alpha: alpha[N] is a DEVICE double array (the scalar form's type;
 * 1 - alpha is formed the same way), bitwise the scalar form with n_shards = 1 row by row.  A frame whose list starts with
 * idx -1 (an inactive row of the grouped search) is passed through: out = src.  k <= 8. */
int alive_knn_merge_gather_rows(const float* cand_val, const int32_t* cand_idx, int k, const double* alpha,
                                const float* rows_f32_full, const float* src, int N, int T, float* out,
                                int32_t* final_idx, void* stream);
/* alive_knn_blend_gather_rows: voice blending.  Output row n (of src / out [N][768][T]) owns the LIST ROWS first[n] ..
 * first[n+1]-1, at most ALIVE_MAX_BLEND of them (a longer run is cut at ALIVE_MAX_BLEND, a negative one is empty); list row r
 * is one top-k list per frame, cand_val / cand_idx [first[N] * T][k] as alive_knn_search_grouped or alive_knn_search_pool
 * return them for the list rows, with weight[r] (normalised by the caller).  Per frame t of row n, in float32 with every
 * product and sum rounded on its own:
 *   m_s = (r_0 + ... + r_(k-1)) / k          the mean of list s's rows (alive_knn_merge_gather_rows' mean, bitwise)
 *   b   = w_0 m_0 + w_1 m_1 + ...            over the ACTIVE lists (first idx >= 0), in list order, left to right
 *   out = b (1 - alpha[n]) + src alpha[n]    as alive_knn_merge_gather_rows; a frame with no active list: out = src.
 * One list at weight 1.0 is therefore bitwise alive_knn_merge_gather_rows.  first (int32[N+1]), weight (double[first[N]]),
 * alpha (double[N]) are DEVICE arrays: the call neither allocates nor synchronises, and a captured hipGraph may replay it
 * after they change.  k <= 8. */
#define ALIVE_MAX_BLEND 4
int alive_knn_blend_gather_rows(const float* cand_val, const int32_t* cand_idx, int k, const int32_t* first,
                                const double* weight, const double* alpha, const float* rows_f32_full, const float* src,
                                int N, int T, float* out, void* stream);

/* ---------------------------------------------- per-row k (a k per session / utterance in the batched paths) ----
 * The four calls above with a k per row: k_row (DEVICE int32[N], read when the kernels run) in place of the scalar, 1 <= k_row[n]
 * <= k_max <= 8.  Every grid and the workspace are sized from N, T and k_max alone, so a captured hipGraph may replay them after
 * k_row changed.  Lists are [N*T][k_max] (read and written at stride k_max).
 * alive_knn_search_grouped_k: for row n the first k_row[n] entries of each frame are bitwise what alive_knn_search_grouped returns
 *   for that row at k = k_row[n], whatever the other rows use; the rest are val -inf, idx -1.  A row is inactive (every entry
 *   -inf / -1) when k_row[n] lies outside [1, k_max], or under alive_knn_search_grouped's rules with the row's own k: a segment
 *   shorter than k_row[n] (one shorter than k_max but not than k_row[n] is searched).  k is part of the group key: rows that search
 *   the same segment AT THE SAME k share one pass over it, so two rows on one segment at different k take two passes.  With
 *   k_row[n] == k_max for every n the call is bitwise alive_knn_search_grouped at k = k_max.  N <= 1024, N * T <= 2^20.
 *   ws: alive_knn_grouped_k_workspace_bytes(N, T, k_max) bytes (0: arguments out of range).
 * alive_knn_merge_gather_rows_k: alive_knn_merge_gather_rows with the mean (r_0 + ... + r_(k-1)) / (float)k over k = k_row[n] of
 *   row n (same order, bitwise the scalar form at that k); final_idx [N*T][k_max] (may be NULL), -1 behind a row's k.  A row
 *   whose k_row[n] lies outside [1, k_max] is passed through (out = src), like a frame whose list starts with idx -1.
 * alive_knn_blend_gather_rows_k: alive_knn_blend_gather_rows with k_row per OUTPUT row (int32[N]): every list of a blend uses
 *   its owner's k, so the search's k_row repeats it on each of the row's list rows. */
size_t alive_knn_grouped_k_workspace_bytes(int N, int T, int k_max);
int alive_knn_search_grouped_k(const float* src, int N, int T, const float* rows_f32, const float* norms, int64_t P,
                               const int32_t* seg_lo, const int32_t* seg_len, const int32_t* k_row, int k_max, float* out_val,
                               int32_t* out_idx, void* ws, void* stream);
int alive_knn_merge_gather_rows_k(const float* cand_val, const int32_t* cand_idx, const int32_t* k_row, int k_max,
                                  const double* alpha, const float* rows_f32_full, const float* src, int N, int T, float* out,
                                  int32_t* final_idx, void* stream);
int alive_knn_blend_gather_rows_k(const float* cand_val, const int32_t* cand_idx, const int32_t* k_row, int k_max,
                                  const int32_t* first, const double* weight, const double* alpha, const float* rows_f32_full,
                                  const float* src, int N, int T, float* out, void* stream);

/* ---------------------------------------------- reserved voice pool (live enrolment) ----
 * A table rows_f32[capacity][768] / norms[capacity] that is allocated once and never replaced, so that a captured hipGraph whose
 * launches hold its two pointers and its row count keeps serving while voices come, grow, move and go.  Both calls run on
 * `stream`, neither allocates nor synchronises, and both refuse bad arguments (-1, a message, nothing launched).
 * alive_pool_append: packs M tokens into rows [at, at + M) of the table; feature d of token m is tokens[d * row_stride +
 *   m * col_stride] (strides in elements, >= 0: a contiguous [768][M] matrix is row_stride = M, col_stride = 1; a column slice or
 *   an every-4th-frame view of an encoder output goes in as it is).  Rows and norms are bitwise those of alive_library_pack_rows
 *   on the same tokens: the same four partial sums per row, fmaf order and sqrtf.  Nothing outside [at, at + M) is written;
 *   at + M > capacity is refused.  Every new norm is checked on the device: report (DEVICE int32[2], reset by the call) receives
 *   the number of rows whose norm is zero or not finite and the lowest such TABLE row (INT32_MAX: none).
 * alive_pool_move_rows: moves n rows and their norms from row src to row dst of the table; the ranges may overlap in either
 *   direction (the bytes are copied, never recomputed).  With shift = |src - dst|, the elements at one residue modulo shift form a
 *   chain that no other chain reads or writes; one thread walks a chain in the direction in which every element is read before it
 *   is overwritten.  One launch for the rows (float4 elements) and one for the norms, no scratch. */
int alive_pool_append(const float* tokens, int64_t row_stride, int64_t col_stride, int64_t M, int Dd, float* rows_f32,
                      float* norms, int64_t capacity, int64_t at, int32_t* report, void* stream);
int alive_pool_move_rows(float* rows_f32, float* norms, int64_t capacity, int64_t src, int64_t dst, int64_t n, void* stream);

/* ---------------------------------------------- half-precision voice pool (fp16 rows) ----
 * The row table of a voice pool stored as IEEE fp16, rows_f16[P][768] (1536 bytes per row); the norms stay fp32.  Every call is its
 * fp32 twin above with `_f16` appended: the same arguments (the table pointer is to fp16), the same checks and grids, and kernels
 * that widen each element in registers and then run the twin's arithmetic in the twin's order.  fp16 -> fp32 is exact, so on a
 * table H every call returns BITWISE what its twin returns on the fp32 table of H's widened values (same norms).
 * alive_pool_append_f16: rounds each token element to fp16 (round to nearest even, subnormals kept, beyond fp16's range -> inf) and
 *   takes the norm over the rounded values widened again: rows are the fp16 rounding of the tokens, norms bitwise those of
 *   alive_pool_append on the rounded tokens.  The report therefore counts a row that overflowed fp16 (its norm is inf) and a row
 *   that rounded to all zeros, besides the rows alive_pool_append counts.
 * alive_pool_move_rows_f16: the same mover on rows of 96 sixteen-byte quads; the table must be 16-byte aligned. */
int alive_pool_append_f16(const float* tokens, int64_t row_stride, int64_t col_stride, int64_t M, int Dd, void* rows_f16,
                          float* norms, int64_t capacity, int64_t at, int32_t* report, void* stream);
int alive_pool_move_rows_f16(void* rows_f16, float* norms, int64_t capacity, int64_t src, int64_t dst, int64_t n, void* stream);
int alive_knn_search_grouped_f16(const float* src, int N, int T, const void* rows_f16, const float* norms, int64_t P,
                                 const int32_t* seg_lo, const int32_t* seg_len, int k, float* out_val, int32_t* out_idx,
                                 void* ws, void* stream);
int alive_knn_search_grouped_k_f16(const float* src, int N, int T, const void* rows_f16, const float* norms, int64_t P,
                                   const int32_t* seg_lo, const int32_t* seg_len, const int32_t* k_row, int k_max, float* out_val,
                                   int32_t* out_idx, void* ws, void* stream);
int alive_knn_merge_gather_rows_f16(const float* cand_val, const int32_t* cand_idx, int k, const double* alpha,
                                    const void* rows_f16_full, const float* src, int N, int T, float* out,
                                    int32_t* final_idx, void* stream);
int alive_knn_merge_gather_rows_k_f16(const float* cand_val, const int32_t* cand_idx, const int32_t* k_row, int k_max,
                                      const double* alpha, const void* rows_f16_full, const float* src, int N, int T, float* out,
                                      int32_t* final_idx, void* stream);
int alive_knn_blend_gather_rows_f16(const float* cand_val, const int32_t* cand_idx, int k, const int32_t* first,
                                    const double* weight, const double* alpha, const void* rows_f16_full, const float* src,
                                    int N, int T, float* out, void* stream);
int alive_knn_blend_gather_rows_k_f16(const float* cand_val, const int32_t* cand_idx, const int32_t* k_row, int k_max,
                                      const int32_t* first, const double* weight, const double* alpha, const void* rows_f16_full,
                                      const float* src, int N, int T, float* out, void* stream);

/* ---------------------------------------------- pool search (many-to-many batch conversion) ----
 * A pool of V voices: fp32 rows_f32[P][768] / norms[P] from alive_library_pack_rows (voice v = rows [seg_lo[v], seg_lo[v] +
 * seg_len[v])), plus one bf16 IMAGE per voice in the layout of alive_library_pack (padded to alive_library_padded_rows rows),
 * the images at consecutive tile-aligned offsets of one buffer, and a rounding bound per voice.
 * alive_pool_image_bytes: bytes of the image buffer for HOST seg_len[V] (0 on a bad table); img_off (HOST int64[V], may be NULL)
 *   receives each image's first row.
 * alive_pool_pack_images: fills the images and bounds (DEVICE float[V]: alive_library_rounding_bound of each voice alone), from the
 *   pool's rows and norms; seg_lo / seg_len are HOST int32[V].  One small launch pair per voice (packing is not on the hot path).
 * alive_knn_search_pool: exact top-k (1 <= k <= 8) of every frame of src[N][768][T] against the voice of its row: voice[n]
 *   (DEVICE int32[N]) indexes the DEVICE tables img_off[V] (int64, image rows), seg_lo[V], seg_len[V] and bounds[V].
 *   out_val / out_idx [N*T][k]: val and idx - seg_lo[voice[n]] are bitwise alive_knn_search_strict on the voice packed alone, and
 *   so bitwise alive_knn_search_grouped on the same segments (ties to the lower row); idx is a POOL index.  A row whose voice is
 *   -1, outside the table, or shorter than k gets val -inf, idx -1.  The strict search's stages with a plan built on the device
 *   (no host sync, one launch per stage whatever V): bf16 candidate stage per (256-frame block of one voice, library split),
 *   exact rescoring with the deterministic certificate (the frame's own voice's bound), exact fp32 scan of the frames that fail.
 *   Limits: N <= 4096, N * T <= 2^20, P < 2^31; max_len = the longest voice (sizes the library splits).
 *   ws: alive_knn_pool_workspace_bytes(N, T, k, V, P, max_len) bytes (0: arguments out of range).
 * alive_knn_pool_stats: device int[ALIVE_POOL_STATS] inside ws, the last call's counters: [0] frames that failed the certificate,
 *   [1] frames that ended in the exact scan, [2] voice groups, [3] 256-frame blocks of the candidate stage. */
#define ALIVE_POOL_STATS 8
size_t alive_pool_image_bytes(const int32_t* seg_len, int V, int64_t* img_off);
int alive_pool_pack_images(const float* rows_f32, const float* norms, int64_t P, const int32_t* seg_lo, const int32_t* seg_len,
                           int V, void* images, float* bounds, void* stream);
size_t alive_knn_pool_workspace_bytes(int N, int T, int k, int V, int64_t P, int64_t max_len);
int alive_knn_search_pool(const float* src, int N, int T, const void* images, const int64_t* img_off, const float* rows_f32,
                          const float* norms, const float* bounds, int64_t P, const int32_t* seg_lo, const int32_t* seg_len,
                          int V, int64_t max_len, const int32_t* voice, int k, float* out_val, int32_t* out_idx, void* ws,
                          void* stream);
/* alive_knn_search_pool_k: alive_knn_search_pool with a k per row (k_row: DEVICE int32[N], 1 <= k_row[n] <= k_max <= 8, read when
 *   the kernels run).  out_val / out_idx [N*T][k_max]: the first k_row[n] entries of each frame of row n are bitwise
 *   alive_knn_search_pool at k = k_row[n], the rest val -inf, idx -1; a row is inactive when k_row[n] lies outside [1, k_max] or its
 *   voice is -1, outside the table or shorter than k_row[n] (a voice shorter than k_max but not than the row's k is searched).  The
 *   plan sorts the rows by (voice, k): every 256-frame block has one voice and one k, the candidate stage does not depend on k, and
 *   the rescoring, the certificate (the k-th exact cosine) and the exact scan take the block's k -- a voice searched at two values of
 *   k forms two groups of blocks.  Grids and workspace from N, T, k_max and the pool's dimensions.  With k_row[n] == k_max for every
 *   n the call is bitwise alive_knn_search_pool at k = k_max.
 *   ws: alive_knn_pool_k_workspace_bytes(N, T, k_max, V, P, max_len) bytes (room for min(N, k_max V) groups; 0: out of range). */
size_t alive_knn_pool_k_workspace_bytes(int N, int T, int k_max, int V, int64_t P, int64_t max_len);
int alive_knn_search_pool_k(const float* src, int N, int T, const void* images, const int64_t* img_off, const float* rows_f32,
                            const float* norms, const float* bounds, int64_t P, const int32_t* seg_lo, const int32_t* seg_len,
                            int V, int64_t max_len, const int32_t* voice, const int32_t* k_row, int k_max, float* out_val,
                            int32_t* out_idx, void* ws, void* stream);
const int* alive_knn_pool_stats(void* ws);

/* alive_dedup_pass: one pass of the greedy de-duplication of a library (generate_voice_library.py of this build, --dedup):
 * frame i is dropped iff a KEPT earlier frame among its k nearest (val / idx[M][k] = alive_knn_search of the library
 * against itself) has cosine > threshold.  state[M]: 0 undecided, 1 kept, 2 dropped (zero it before the first pass);
 * *undecided (zero it before each pass) counts the frames still waiting for an earlier neighbour; repeat until it is 0. */
int alive_dedup_pass(const float* val, const int32_t* idx, int64_t M, int k, double threshold, int32_t* state,
                     int32_t* undecided, void* stream);

/* ----------------------------------------------------------- operators ----
 * Building blocks, exported so that every kernel has its own parity test.
 *
 * alive_conv1d: Conv1d / ConvTranspose1d(k == stride) as an f32-MFMA implicit
 * GEMM with fused epilogue.  Replaces every nn.Conv1d / nn.ConvTranspose1d on
 * the path (common.py:48-51,88-92; decoder.py:16-17,41,61,108-110,141,164-182).
 */
typedef struct AliveConv {
    const float* W;        /* packed [Co_pad][K_pad], K = Ci*KW (k-major within ci), zero padded to x16 */
    const float* bias;     /* [rows] or NULL (rows = Co, or Co*up for transposed) */
    const float* X;        /* [N][Ci][Tin] */
    int N, Ci, Tin;
    int Co;                /* GEMM rows (Co, or Co*up for transposed convs) */
    int K_pad;             /* padded K (multiple of 16) */
    int KW, stride, dil;   /* input index = t*stride + j*dil - pad_left */
    int pad_left;
    int pad_mode;          /* 0 zero; 1 reflect left, zero right; 2 reflect both (STFT centre pad) */
    int Tout;              /* GEMM columns per batch item */
    int up;                /* 1, or r for ConvTranspose1d(k=r, stride=r): row -> (co=row/r, j=row%r), t -> t*r+j */
    int act;               /* 0 none, 1 gelu(erf), 2 exp, 3 sin */
    const float* post_add; /* [rows] added after act (FiLM "+1"), or NULL */
    const float* ch_scale; /* [rows] multiplied after act (ConvNeXt layer scale), or NULL */
    const float* residual; /* [N][Co][Tout] added after ch_scale, or NULL */
    const float* skip;     /* [N][Co][Tout] added after residual, or NULL */
    float* Y;              /* raw output [N][Co_out][Tout*up], or NULL */
    /* optional second output: Z = gelu(v) * interp(film[fs]) + interp(film[fh])  (decoder.py:112-117,130-132) */
    float* Z;
    const float* film;     /* [N][film_rows][Lf] */
    int film_rows, Lf, film_scale_row, film_shift_row;
    /* arithmetic: 0 = exact fp32 (f32-input MFMA), W as above;
     *             1 = 2-term split bf16 ("bf16x3": hi*hi + hi*lo + lo*hi on the bf16 MFMA, ~2^-16 per product),
     *                 W = bf16, 2 planes (hi, lo) of Co_pad rows x K = KW*Ci_pad, tap-major k = j*Ci_pad + ci, stored K-BLOCKED
     *                 like the activation planes below: [2][K/32][Co_pad][32] (module/_pack.py::pack_conv_split);
     *                 Ci_pad a multiple of 32; stride must be 1;
     *             2 = 3-term split bf16 ("bf16x6", six MFMAs per product, fp32-grade): W as for 1 with 3 planes;
     *             3 = plain fp16 (round 5): ONE MFMA per product (v_mfma_f32_32x32x16_f16), operands rounded to nearest even and saturated
     *                 at +-65504, fp32 accumulate -- W = ONE fp16 plane [K/32][Co_pad][32] (module/_pack.py::pack_conv_split_h stores it
     *                 as the third slab behind the two bf16 planes), Xp / Zp carry ONE fp16 plane.  2^-12 per operand: for layers whose
     *                 contribution to the output has been measured (alive_decoder_precision).  With at most 96 columns (the streaming
     *                 kernels) it is not available: those callers use precision 1. */
    int precision, Ci_pad;
    /* FiLM of a frame RANGE of a longer window (alive_decoder_forward_range): this conv's columns start at sample
     * film_t0 of the window (at its own rate) and `film` holds the frames [film_f0, film_f0 + film_ld) only, row pitch
     * film_ld; Lf stays the window's frame count, so the interpolation coordinates are those of the whole window.
     * film_ld == 0: film covers the whole window (film_t0 = film_f0 = 0, pitch Lf; anything else is refused).  Split kernel only. */
    int film_t0, film_f0, film_ld;
    /* Plane-packed operands of the split kernel (precision 1, Co > 64; round 3).  Format = "plane-packed activations" below:
     * P[plane][C_pad/32][cols_pad][32] bf16 (row = n * T + t), 2 planes, plane stride = cols_pad * C_pad, cols_pad = N * T
     * rounded up to 128.
     *   Xp  input instead of X (X is ignored): Ci a multiple of 32, pad_mode 1 (or no padding); staged by LDS-DMA.
     *   Zp  the second output (gelu + FiLM) in that format instead of / beside Z: Co a multiple of 64, Tout a multiple of 4.
     * The decoder's 256-channel FilterBlock chains its convs through these (networks.hip). */
    const void* Xp;
    void* Zp;
    /* Round 5: Y ALSO as k-blocked bf16 planes (2 planes, [2][pad32(Co) / 32][cols_pad][32], cols = N * Tout), written by the exact
     * fp32 kernel (precision 0) beside Y for a plain conv (no activation / post_add / ch_scale / residual / skip / Z, up 1,
     * 16 < Co <= 64, Co % 4 == 0): the plane image of the Filter's 64-channel skip tensor comes from the conv that produces it
     * (decoder.py:186-188) instead of an alive_to_planes pass over it.  Same bits as alive_to_planes(Y). */
    void* Yp;
    int yp_planes;         /* 0 / 2: two bf16 planes (the bits of alive_to_planes(Y, 2)); 1: ONE fp16 plane (alive_to_planes(Y, 1)) */
} AliveConv;
int alive_conv1d(const AliveConv* desc, void* stream);
/* TEST ONLY.  A transposed conv on split bf16 (precision 1, KW 1, stride 1, up > 1, no padding) with Ci a multiple of 32 up to 256
 * and only a bias takes a kernel that stages the input tile once per (window, 64 columns) and walks all rows under it
 * (csrc/conv_up.hip) when N * ceil(Tout / 64) >= 512; its output is bitwise that of the tiled kernel.  alive_conv1d_tiled is
 * alive_conv1d without that form; alive_conv_up_launches returns how many launches took it so far (reset != 0: and clears the count);
 * alive_conv_up_min_blocks(b) sets that threshold of 512 blocks for the process (b > 0: to b, so that a test reaches the kernel with
 * a small shape; b < 0: back to 512; b == 0: query) and returns the value in force.  The product never calls it. */
int alive_conv1d_tiled(const AliveConv* desc, void* stream);
int alive_conv_up_launches(int reset);
int alive_conv_up_min_blocks(int blocks);

/* ---- plane-packed activations: the frame-rate GEMMs of the ConvNeXt stacks --------------------------
 * The 1x1 convs of ContentEncoder / F0Estimator / FeatureExtractor (content_encoder.py:22-25,
 * f0_estimator.py:23-27, decoder.py:43-48, common.py:57-61,77-81) run as plain GEMMs whose activation operand is
 * already split into bf16 planes and stored K-BLOCKED, so that BOTH operands go global -> LDS by LDS-DMA in contiguous
 * runs of whole cache lines and the inner loop is MFMAs only (csrc/planes_layout.h):
 *   P[plane][C_pad/32][cols_pad][32] bf16 -- element (plane, col, c) at ((plane * C_pad/32 + c/32) * cols_pad + col) * 32 + c % 32,
 *   col = n*T + t, plane 0 = bf16(v), plane 1 = bf16(v - p0), plane 2 = bf16(v - p0 - p1);
 *   C_pad a multiple of 32 (zero filled), plane stride = cols_pad * C_pad with cols_pad a multiple of 128.
 *   (Rounds 2 - 3 stored the planes row-major, [plane][col][C_pad]: a 16-row DMA piece then touched 16 half lines whose other
 *   halves the next K-step fetched again; the k-blocked form took 5 - 12 % off every kernel that reads them.)
 * alive_to_planes converts an fp32 [N][C][T] tensor; alive_gemm_planes writes fp32 [N][Co][T] (same epilogue
 * options as alive_conv1d) and / or plane-packed output (act applied first) for the next GEMM. */
size_t alive_planes_bytes(int64_t cols, int C, int planes);        /* bytes of a plane-packed buffer */
int alive_to_planes(const float* X, int N, int C, int T, int planes, void* P, void* stream);
typedef struct AliveGemm {
    const void* W;         /* bf16 [planes][Ci_pad/32][Co_pad][32], k-blocked like P (module/_pack.py::pack_conv_split of a k=1 conv) */
    const float* bias;     /* [Co] or NULL */
    const void* P;         /* input planes [planes][Ci_pad/32][cols_pad][32] */
    int N, T;              /* cols = N*T; fp32 outputs are [N][Co][T] */
    int Ci, Co;
    int planes;            /* 2: bf16x3, 3: bf16x6 (both operands); 1 (round 5): plain fp16, one MFMA per product -- W, P and Pout are
                            * single fp16 planes in the same k-blocked layout; act 0 - 2 only */
    int act;               /* 0 none, 1 gelu, 2 exp, 3 argmax over Co (3 planes only): no Y / Pout, see arg_val; 4: see the end of the struct */
    const float* post_add; /* [Co] or NULL */
    const float* ch_scale; /* [Co] or NULL */
    const float* residual; /* [N][Co][T] or NULL */
    float* Y;              /* fp32 output [N][Co][T] or NULL */
    void* Pout;            /* plane-packed output [planes][Co_pad32/32][cols_pad][32] or NULL (Co_pad32 = Co rounded up to 32) */
    /* custom placement of the input rows (all 0: the packed form above).  Row (n, t) of plane pl starts at element
     * pl*b_plane + n*b_win + t*b_row: overlapping rows (b_row < Ci) make the GEMM a strided convolution over a signal
     * stored once -- the STFT runs this way (b_row = hop 320, Ci = 1280).  Multiples of 8 elements. */
    int64_t b_plane, b_win;
    int b_row;
    /* b_cblk = 0: such a row is k-contiguous in memory (the STFT's signal).  b_cblk > 0: the rows live in a k-blocked plane buffer
     * (alive_to_planes / Pout) of b_cblk k-blocks, and the K vector of an output column is Ci / (32 b_cblk) consecutive rows of it:
     * k = (tap * b_cblk + block) * 32 + i is element i of row + tap in block `block`, b_blk elements per block (the padded rows of
     * that buffer * 32) -- the Filter's strided down convs (k == stride) run this way on the output planes of the layer before. */
    int b_cblk;
    int64_t b_blk;
    /* act == 3: the [Co][cols] product is never stored.  Each 64-row block of the GEMM leaves, per column, its largest
     * value (bias included) and the row it sits in -- arg_val / arg_idx [ceil(Co/64)][N*T], the rule of
     * alive_argmax_channels below -- and alive_argmax_merge reduces the blocks: F0Estimator.estimate
     * (f0_estimator.py:30-34) without the 4096-class logits tensor. */
    float* arg_val;
    int32_t* arg_idx;
    /* Round 5 (the front end without an fp32 spectrogram).  Fields appended: a zeroed struct of the old size means "off".
     * y_split > 0: ONE GEMM for two consumers of the same input -- rows [0, y_split) go to Y as [N][y_split][T], rows [y_split, Co) to
     *   Y2 as [N][Co - y_split][T] (y_split a multiple of 128; no residual).  The ContentEncoder / F0Estimator input layers
     *   (content_encoder.py:22, f0_estimator.py:23) run as one 641 -> 512 + 256 GEMM this way.
     * act == 4: the rows are (re, im) PAIRS of a DFT (row 2f = cos, 2f + 1 = -sin: alive_dft_basis's interleaved image); the epilogue
     *   takes |re + i im| (hypotf, spectrogram.py:8) of each pair and leaves the Co / 2 magnitudes as plane-packed channels in Pout
     *   ([planes][pad32(Co / 2) / 32][cols_pad][32]) -- the magnitude spectrogram never exists in fp32.  No Y, bias or other term. */
    float* Y2;
    int y_split;
    /* Round 5: fp16 split planes (planes == 2 only; fields appended, all 0 = the bf16 planes above).  f16s != 0: both operands are TWO
     * fp16 planes of a power-of-two multiple of the values -- hi = fp16(s v), lo = fp16(s v - hi), round to nearest even, saturated at
     * +-65504 -- in the same k-blocked layout, multiplied as hi*hi + hi*lo + lo*hi on v_mfma_f32_32x32x16_f16: 22 significand bits per
     * operand (the two bf16 planes carry 16) for elements above 2^-11 / s, an absolute error below 2^-25 / s for smaller ones -- fp32-grade
     * at three MFMAs per product instead of the six of the three-plane bf16 form.  The accumulator is multiplied by *wscale * in_unscale
     * before the bias (wscale: device pointer to 1 / s_W of this weight tensor, module/_pack.py::pack_conv_split_f16s; in_unscale =
     * 1 / s_P, the scale the producer of P used); Pout, if set, is written in the same format with the scale pout_scale.
     * Used by the ConvNeXt pointwise convs of both encoders (alive_encoder_precision). */
    int f16s;
    const float* wscale;
    float in_unscale, pout_scale;
} AliveGemm;
int alive_gemm_planes(const AliveGemm* desc, void* stream);
/* out[col] = (float) row of the largest value over the nblk per-block candidates of column col (smallest row on ties) */
int alive_argmax_merge(const float* arg_val, const int32_t* arg_idx, int nblk, int64_t cols, float* out, void* stream);

/* FilterBlock.forward (decoder.py:137-150) for C = 8 or 16 fused into one kernel (filter_small.hip): input_conv 1x1 + three
 * FilterResBlocks (six GELU -> FiLM -> reflect-left causal k5 convs, dilations 1,1,2,2,4,4), optional U-Net skip
 * added to the result.  U[N][C][L] -> out[N][C][L] (not in place).
 *   wpack: alive_filter_block_small_weights(C) floats, 16-byte aligned = fp32 biases [7][32] (input conv first, rows >= C zero), then
 *          bf16 pairs in fp32 words: input conv [2 planes][32 rows][16] (k = ci) and per conv q = 0..5 [2 planes][32 rows][KP],
 *          k = tap * C + ci, KP = 80 (C = 16) / 48 (C = 8), zero padded; planes hi = bf16(w), lo = bf16(w - hi)
 *          (module/_pack.py::pack_filter_small).  Since round 4 the block computes on the split-bf16 product of the 32x32x16 MFMA
 *          (~2^-16 per product, like the 64- and 256-channel scales), not on the exact f32 MFMA
 *   film[N][film_rows][Lf]; conv q reads its scale rows at film_off + q*2C and shift rows at film_off + q*2C + C. */
int alive_filter_block_small_weights(int C);
int alive_filter_block_small(const float* U, int N, int C, int L, const float* wpack, const float* film,
                             int film_rows, int Lf, int film_off, const float* skip, float* out, void* stream);
/* the same on a frame range of a longer window (see AliveConv.film_t0): L samples starting at sample t0 of the window's
 * tensor at this rate, film[N][film_rows][film_ld] holding the frames from f0 on, Lf = frames of the whole window */
int alive_filter_block_small_range(const float* U, int N, int C, int L, const float* wpack, const float* film,
                                   int film_rows, int Lf, int film_off, int t0, int f0, int film_ld, const float* skip,
                                   float* out, void* stream);
/* The two finest blocks with the small conv that follows them folded into the store phase (the decoder's batch route; the tensor in
 * between is never written, the results are those of the two launches bit for bit):
 *   alive_filter_block_small_up_range  : C = 16, then ConvTranspose1d(16, 8, 2, 2) (ups[3]) on block + skip:
 *        U[N][16][L] -> out[N][8][2 L];  upW[16 rows (co, j)][16], upb[16] as module/_pack.py::pack_convT packs them for alive_conv1d;
 *   alive_filter_block_small_wave_range: C = 8 (no skip), then source_out Conv1d(8, 1, 7, pad 3, zeros outside [0, L)):
 *        U[N][8][L] -> wave[N][L];  oW[8][7], ob[1] as alive_filter_source_out takes them.
 * Other arguments as alive_filter_block_small_range (whole window: t0 = f0 = 0, film_ld = Lf); L > 16 and a multiple of 4.
 * alive_decoder_forward[_range] take this route on the batch path unless the environment has ALIVE_FINE_FUSE=0 (read once), which
 * puts the launches of the small convs back -- a switch for A/B runs and the equality tests, it selects nothing else. */
int alive_filter_block_small_up_range(const float* U, int N, int L, const float* wpack, const float* film, int film_rows, int Lf,
                                      int film_off, int t0, int f0, int film_ld, const float* skip, const float* upW, const float* upb,
                                      float* out, void* stream);
int alive_filter_block_small_wave_range(const float* U, int N, int L, const float* wpack, const float* film, int film_rows, int Lf,
                                        int film_off, int t0, int f0, int film_ld, const float* oW, const float* ob, float* wave,
                                        void* stream);

/* FilterBlock.forward (decoder.py:137-150) for C = 64 fused into one kernel on the split-bf16 MFMA (filter_mid.hip):
 * activations stay in LDS as two bf16 planes through the input conv and the six modulated k5 convs.
 *   W16: bf16, alive_filter_block64_weights() elements = input conv [2 planes][64][64], then per conv q = 0..5
 *        [2 planes][64][k = j*64 + ci]  (module/_pack.py::pack_filter_mid)
 *   biases: fp32 [7][64], input conv first;  film / film_off / skip / out as alive_filter_block_small;
 *   L a multiple of 4, out and skip 16-byte aligned, not in place. */
int64_t alive_filter_block64_weights(void);
int alive_filter_block64(const float* U, int N, int L, const void* W16, const float* biases, const float* film,
                         int film_rows, int Lf, int film_off, const float* skip, float* out, void* stream);
int alive_filter_block64_range(const float* U, int N, int L, const void* W16, const float* biases, const float* film,
                               int film_rows, int Lf, int film_off, int t0, int f0, int film_ld, const float* skip,
                               float* out, void* stream);
/* the same with the six k5 convs on ONE fp16 plane per operand (one MFMA per product, v_mfma_f32_32x32x16_f16; the 1x1 input conv keeps
 * split bf16): W16 = the pack of alive_filter_block64_weights() elements, whose last 6 x 64 x 320 hold the k5 weights as fp16
 * (module/_pack.py::pack_filter_mid).  Part of alive_decoder_precision mode 1. */
int alive_filter_block64_range_fp16(const float* U, int N, int L, const void* W16, const float* biases, const float* film,
                               int film_rows, int Lf, int film_off, int t0, int f0, int film_ld, const float* skip,
                               float* out, void* stream);

/* FilterBlock.forward (decoder.py:137-150) for C = 256 fused into one kernel on plain fp16 operands (filter_big.hip; decoder precision
 * mode 1, batch path): a block sweeps a segment of a window in tiles of 128 columns, the six modulated k5 convs' inputs stay in LDS as one
 * fp16 plane, the residual stream in registers.  The 1x1 input conv is part of the transposed conv that produces U (module/_pack.py).
 *   w16[q], bias[q], q = 0..5: blocks[q / 2].c1 / .c2 -- the fp16 slab [K / 32][256][32] (K = 5 x 256, tap-major) of
 *        module/_pack.py::pack_conv_split_h (third slab of the pack) and the fp32 bias [256];  w16 and bias are HOST arrays of device pointers.
 *   film / film_off / t0 / f0 / film_ld / skip / out as alive_filter_block64_range;  L > 32;  not in place;
 *   ws: alive_filter_block256_workspace_bytes(N, L) bytes of device scratch (the convs' causal contexts between a block's tiles). */
int64_t alive_filter_block256_workspace_bytes(int N, int L);
int alive_filter_block256_fp16(const float* U, int N, int L, const void* const* w16, const float* const* bias, const float* film,
                               int film_rows, int Lf, int film_off, int t0, int f0, int film_ld, const float* skip, float* out,
                               void* ws, int64_t ws_bytes, void* stream);

/* the same kernel for C = 64 (decoder scale 1; round 6): tiles of 512 columns, four column groups of waves, FiLM at <= 1 frame per 25
 * columns.  Like the 256-channel form it takes the block's residual stream -- the decoder composes blocks[1].input_conv into ups[1]
 * (module/_pack.py "flt.up1.Wc") -- and six fp16 slabs [K / 32][64][32], K = 5 x 64.  alive_filter_block64_range_fp16 (input conv inside,
 * one bf16-typed pack) stays for the split-bf16 mode and for short signals. */
int64_t alive_filter_block64s_workspace_bytes(int N, int L);
int alive_filter_block64s_fp16(const float* U, int N, int L, const void* const* w16, const float* const* bias, const float* film,
                               int film_rows, int Lf, int film_off, int t0, int f0, int film_ld, const float* skip, float* out,
                               void* ws, int64_t ws_bytes, void* stream);
/* the same with the ConvTranspose1d(64, 16, 2, 2) behind the block (ups[2]) in its store phase: U[N][64][L] -> out[N][16][2 L], bit for
 * bit alive_conv1d(up = 2) on the block's output, which is never written.  upW[32 rows (co, j)][64], upb[32] as
 * module/_pack.py::pack_convT packs them.  Part of the decoder's batch route like the two entry points in filter_small.hip above
 * (ALIVE_FINE_FUSE=1 keeps those two and puts this conv back as a launch of its own). */
int alive_filter_block64s_fp16_up(const float* U, int N, int L, const void* const* w16, const float* const* bias, const float* film,
                                  int film_rows, int Lf, int film_off, int t0, int f0, int film_ld, const float* skip, const float* upW,
                                  const float* upb, float* out, void* ws, int64_t ws_bytes, void* stream);

/* The waveform-rate edges of Filter.forward (decoder.py:164,182,186-188,194) as streaming kernels:
 *   alive_filter_source_in : downs[0](source_in(src)):  src[N][Lw] -> d0[N][16][Lw/2]
 *                            Win[8][7], bin[8] = source_in (pad 3); Wd[16][8][2], bd[16] = downs[0] (stride 2); fp32,
 *                            reference layouts.  The 8-channel intermediate is not a skip and is never stored.
 *   alive_filter_source_out: source_out(H):  H[N][8][Lw] -> wave[N][Lw];  W[8][7] (= weight[0]), b[1] */
int alive_filter_source_in(const float* src, int N, int Lw, const float* Win, const float* bin, const float* Wd,
                           const float* bd, float* d0, void* stream);
int alive_filter_source_out(const float* H, int N, int Lw, const float* W, const float* b, float* wave, void* stream);

/* depthwise k7 conv + (Adaptive)ChannelNorm (common.py:20-26,35-41,55-56,75-76)
 *   affine_mode 0: gain[C], offset[C];  1: per-sample scale/shift rows in cond[N][cond_rows][T] */
int alive_dwconv_norm(const float* X, int N, int C, int T, const float* dw_w, const float* dw_b,
                      int affine_mode, const float* gain, const float* offset,
                      const float* cond, int cond_rows, int scale_row, int shift_row,
                      float eps, float* Y, void* stream);
/* the same with plane-packed output for alive_gemm_planes (dw_w == dw_b == NULL: the norm alone); one pass over memory:
 * a block's [C][32 or 64 columns] tile stays on chip between the conv, the statistics, the affine and the split.  C a multiple of 32. */
int alive_dwconv_norm_planes(const float* X, int N, int C, int T, const float* dw_w, const float* dw_b,
                             int affine_mode, const float* gain, const float* offset,
                             const float* cond, int cond_rows, int scale_row, int shift_row,
                             float eps, int planes, void* P, void* stream);
/* the same with fp16 split planes: TWO planes hi = fp16(s y), lo = fp16(s y - hi) with s = scale (a power of two), saturated at
 * +-65504 -- the input format of alive_gemm_planes with f16s (AliveGemm.in_unscale = 1 / scale) */
int alive_dwconv_norm_planes_f16s(const float* X, int N, int C, int T, const float* dw_w, const float* dw_b,
                                  int affine_mode, const float* gain, const float* offset,
                                  const float* cond, int cond_rows, int scale_row, int shift_row,
                                  float eps, float scale, void* P, void* stream);
/* TEST ONLY: the two entry points above always through the kernel that keeps the tile in LDS from the conv on.  The widths the networks
 * run (C = 64, 128, 256, 512) otherwise take a kernel that holds each thread's channels in registers; its planes are bitwise the same.
 * f16_scale != 0 (planes = 2): the fp16 split form with that scale. */
int alive_dwconv_norm_planes_ref(const float* X, int N, int C, int T, const float* dw_w, const float* dw_b,
                                 int affine_mode, const float* gain, const float* offset,
                                 const float* cond, int cond_rows, int scale_row, int shift_row,
                                 float eps, int planes, void* P, void* stream, float f16_scale);
/* z = gelu(h) * interp(film[scale_row + c]) + interp(film[shift_row + c])  (decoder.py:112-117,130-132: F.gelu, then the FiLM of a
 * ModulatedCausalConv1d with F.interpolate(mode='linear')), the arithmetic of alive_conv1d's second output.  H [N][C][L];
 * film [N][film_rows][film_ld] holds the frames from f0 on of a window of Lf frames, t0 = first sample of H in the window at this
 * rate (whole window: t0 = f0 = 0, film_ld = Lf).  Exactly one of Z (fp32 [N][C][L]) and Zp (2 k-blocked bf16 planes, C % 32 == 0). */
int alive_gelu_film(const float* H, int N, int C, int L, const float* film, int film_rows, int Lf, int scale_row,
                    int shift_row, int t0, int f0, int film_ld, float* Z, void* Zp, void* stream);
/* ChannelNorm alone (f0_estimator.py:25) */
int alive_channel_norm(const float* X, int N, int C, int T, const float* gain, const float* offset,
                       float eps, float* Y, void* stream);
/* argmax over channels -> float (f0_estimator.py:33), torch.argmax's answer on every column: a NaN is the maximum; among equal values,
 * and among NaNs, the lowest channel wins; a column of -inf gives 0.  The act == 3 GEMM with alive_argmax_merge follows the same rule. */
int alive_argmax_channels(const float* X, int N, int C, int T, float* out, void* stream);

/* HarmonicOscillator.forward after to_amps/exp (decoder.py:79-100).
 *   amps[N][H][Lf] (already exp'd), f0[N][Lf], phi_in[N][H] or NULL, crop0,
 *   wave[N][Lf*seg], phi_out[N][H] = asin(sin(theta)) at column phi_col (or NULL).
 *   ws: alive_oscillator_workspace_bytes(N, H, Lf). */
size_t alive_oscillator_workspace_bytes(int N, int H, int Lf);
int alive_oscillator(const float* amps, const float* f0, const float* phi_in, int N, int H, int Lf,
                     int seg, float sample_rate, int crop0, int phi_col,
                     float* wave, float* phi_out, void* ws, void* stream);
/* the frames [f_begin, f_begin + n_frames) of the window only: amps[N][H][n_frames], wave[N][n_frames*seg]; f0 and the
 * phase accumulation cover the whole window, so the samples are bitwise those of alive_oscillator.  crop0 and phi_col are
 * columns of the window; with a phi_out, phi_col must lie inside the range's samples [f_begin*seg, (f_begin+n_frames)*seg) */
int alive_oscillator_range(const float* amps, const float* f0, const float* phi_in, int N, int H, int Lf,
                           int seg, float sample_rate, int crop0, int phi_col, int f_begin, int n_frames,
                           float* wave, float* phi_out, void* ws, void* stream);

/* magnitude STFT 1280/320, rect window, reflect centre pad, last frame dropped
 * (module/spectrogram.py:5-10): wav[N][L] -> spec[N][641][L/320], as a DFT GEMM on the
 * f32 MFMA.  basis: [1296][1280] fp32 filled once by alive_dft_basis (rows 0..640 cos,
 * 641..1281 -sin, rest zero); ws: alive_spectrogram_workspace_bytes(N, L). */
size_t alive_dft_basis_bytes(void);
int alive_dft_basis(float* basis, void* stream);
size_t alive_spectrogram_workspace_bytes(int N, int L);
int alive_spectrogram(const float* basis, const float* wav, int N, int L, float* spec, void* ws, void* stream);

/* Decoder.forward on the frames [f_begin, f_begin + n_frames) of windows of Lf frames (context trimming: inference.py
 * keeps the centre third of a window).  x[N][768][n_frames] are the matched features of that range, f0[N][Lf] covers the
 * whole window (phase accumulation), wave[N][320*n_frames].  Frames further than the decoder's receptive field from the
 * range edges (12 + 12 to the left, 13 to the right) are bitwise those of alive_decoder_forward on the whole window.
 * ws: alive_decoder_workspace_bytes(N, n_frames) + alive_decoder_workspace_bytes(N, Lf) is enough. */
int alive_decoder_forward_range(const float* const* w, const float* x, const float* f0, int N, int Lf, int f_begin,
                                int n_frames, float* wave, void* ws, void* stream);

/* ------------------------------------------------------- audio edges (f2) ----
 * torchaudio.functional.resample (sinc_interp_hann, lowpass_filter_width 6, rolloff 0.99) as a polyphase filter bank,
 * torchaudio.functional.gain folded in as a pre / post factor, and the int16 conversions of the streaming loop
 * (inference.py:88-94,135-142; realtime_inference.py:139-147,173-183).  orig / new are the rates divided by their gcd.
 *   filt: [new][alive_resample_taps(orig, new)] floats filled once by alive_resample_filter;
 *   y[b][o] = post_scale * sum_j filt[o % new][j] * (pre_scale * x[b][(o / new) * orig + j - width]), zero outside x;
 *   Lout <= alive_resample_length(L, orig, new) = ceil(new * L / orig).
 *   alive_float_to_pcm16 truncates toward zero and keeps the low 16 bits (numpy astype, no clipping). */
int alive_resample_taps(int orig, int new_rate);
int64_t alive_resample_length(int64_t L, int orig, int new_rate);
int alive_resample_filter(int orig, int new_rate, float* filt, void* stream);
int alive_resample(const float* x, int B, int L, int orig, int new_rate, const float* filt, float pre_scale,
                   float post_scale, float* y, int Lout, void* stream);
/* alive_resample with per-row factors: pre_scale / post_scale are DEVICE float[B] (row b: bitwise alive_resample with
 * pre_scale[b], post_scale[b]).  orig == new: the gains alone, y = (x * pre) * post (torchaudio.functional.gain twice), Lout == L,
 * filt not read. */
int alive_resample_rows(const float* x, int B, int L, int orig, int new_rate, const float* filt, const float* pre_scale,
                        const float* post_scale, float* y, int Lout, void* stream);
/* alive_resample_rows with a rate pair per row, for a batch of sessions at different rates in one launch (one captured graph).
 *   x[B][ld_in]: row b holds len_in[b] valid samples.  y[B][ld_out]: row b receives len_out[b] samples; the rest of the row up to
 *   ld_out is written 0.0f.
 *   table: DEVICE int32[n_pairs][4], 16-byte aligned, entry {orig, new, width, offset} -- the rates divided by their gcd,
 *   width = (alive_resample_taps(orig, new) - orig) / 2, and the offset (in floats) of the pair's bank, filled by
 *   alive_resample_filter(orig, new, filt + offset), in the concatenated buffer filt[filt_len].  An equal-rate entry is {1, 1, 0, 0}
 *   and reads no bank (filt may be NULL when every entry is equal-rate and filt_len is 0).
 *   pair, len_in, len_out: DEVICE int32[B]; pre_scale / post_scale: DEVICE float[B].
 *   Row b is bitwise alive_resample_rows of that row alone at table[pair[b]] with pre_scale[b], post_scale[b] and Lout = len_out[b]
 *   (at orig == new: the gains alone, (x * pre) * post).  A resampling row whose bank is at most lds_bytes stages it in LDS; pass
 *   the largest bank of at most 16 KB in the table (any value in [0, 16384] is safe and gives the same result).
 *   The grid depends on B and ld_out only: one captured launch serves any mix of pairs and lengths written between replays.
 *   The per-row arrays are device data the host does not read: the caller guarantees len_in[b] <= ld_in and
 *   len_out[b] <= min(ld_out, alive_resample_length(len_in[b], orig, new)).  Out-of-range device data never leads to an access
 *   outside x, filt or y: lengths are clamped to the strides, and a row whose pair index or table entry is invalid is written 0.
 *   B in [1, 1024], n_pairs >= 1, ld_in, ld_out > 0. */
int alive_resample_rows_multi(const float* x, int B, int ld_in, const int* len_in, const int* pair, const int* table, int n_pairs,
                              const float* filt, int64_t filt_len, int lds_bytes, const float* pre_scale, const float* post_scale,
                              float* y, int ld_out, const int* len_out, void* stream);
int alive_pcm16_to_float(const int16_t* in, int64_t n, float* out, void* stream);
int alive_float_to_pcm16(const float* in, int64_t n, int16_t* out, void* stream);

/* ------------------------------------------------------------ networks ----
 * Weight tables are arrays of device pointers in the order given by
 * alive_weight_name(model, i), i < alive_weight_count(model); tensors are the
 * packed forms produced by module/_pack.py from a reference state_dict.
 * model: 0 content encoder, 1 f0 estimator, 2 decoder.
 */
int alive_weight_count(int model);
const char* alive_weight_name(int model, int index);

/* ContentEncoder.forward (content_encoder.py:21-25): spec[N][641][T] -> out[N][768][T] */
/* Fused front end (round 5): wav[N][L] at 16 kHz -> content features feat[N][768][L / 320] and f0 classes
 * f0[N][1][L / 320] (the argmax of F0Estimator.estimate, before the class -> Hz map is applied by the caller exactly as after
 * alive_f0_estimate), i.e. spectrogram.py:5-10 + content_encoder.py:21-25 + f0_estimator.py:22-34 in one call and without an
 * fp32 spectrogram: bitwise alive_spectrogram + alive_f0_estimate + alive_content_encoder.  Batch path only (N * (L / 320) >= 96,
 * L % 8 == 0).  w_in: the two input layers' plane-packed weights concatenated along the rows (CE's 512, then PE's 256:
 * [3][672 / 32][768][32] bf16), b_in: their biases [768].  ws: alive_front_end_workspace_bytes(N, L). */
size_t alive_front_end_workspace_bytes(int N, int L);
int alive_front_end(const float* basis, const float* const* ce_weights, const float* const* pe_weights, const void* w_in,
                    const float* b_in, const float* wav, int N, int L, float* feat, float* f0, void* ws, void* stream);
size_t alive_content_encoder_workspace_bytes(int N, int T);
int alive_content_encoder(const float* const* w, const float* spec, int N, int T,
                          float* out, void* ws, void* stream);

/* F0Estimator.estimate (f0_estimator.py:29-34): spec -> f0[N][T] (class index as float) */
size_t alive_f0_estimate_workspace_bytes(int N, int T);
int alive_f0_estimate(const float* const* w, const float* spec, int N, int T,
                      float* f0, void* ws, void* stream);

/* F0Estimator.forward through the fused kernels: spec -> the class scores logits[N][4096][T] that alive_f0_estimate reduces in its
 * classifier's epilogue, stored instead.  Same operands per branch (fp32 below 96 frame columns, fp16 split planes or three bf16
 * planes above), so alive_argmax_channels(logits) is bitwise alive_f0_estimate.  ws: alive_f0_estimate_workspace_bytes(N, T). */
int alive_f0_logits(const float* const* w, const float* spec, int N, int T, float* logits, void* ws, void* stream);

/* Pitch tracking: a Viterbi path over class scores instead of the per-frame argmax (tools/pitch_track_ref.py is the NumPy
 * restatement, bit for bit).  States i = 0 .. S - 1 stand for the classes lo + i (1 <= lo, lo + S <= C, S <= ALIVE_F0_TRACK_MAX_STATES:
 * two fp64 score columns in 64 KB of LDS).  HOST tables, uploaded once: semis[i] = 12 log2(lo + i) and band_lo[i] / band_hi[i], the
 * first / last state j with |semis[i] - semis[j]| <= band.  Per row: weight >= 0 (cost per semitone moved inside the band) and
 * jump >= 0 (flat cost of any other move), in the units of the scores (raw logits serve: the path is invariant to a per-frame
 * constant).  With x[t][i] = (double) logits[n][lo + i][t] (NaN -> -FLT_MAX, else clamped to +-FLT_MAX), e[t][i] = x[t][i] -
 * max_j x[t][j] (the frame's scores below its best one, so that an all-NaN or all-equal frame is e = 0 and the path passes through
 * it instead of -FLT_MAX rounding every earlier score away) and D[0] = e[0]:
 *   g = max_j D[t-1][j] - jump;  a = max_{j in band of i} (D[t-1][j] - weight |semis[i] - semis[j]|);  D[t][i] = e[t][i] + max(a, g)
 * (a wins a tie with g; every max keeps its lowest index); the path is traced back from the lowest argmax of D[T-1] and
 * f0[n][t] = (float)(lo + p[t]).  fp64 + - * abs and compares only.
 *   on       DEVICE int32 [N] or NULL (every row): a row with on[n] == 0 does nothing and its f0 row is untouched
 *   changed  DEVICE int32 [N] or NULL: the number of frames whose tracked class differs from what f0 held on entry
 *   ws       alive_f0_track_workspace_bytes(N, T, S) bytes (back pointers, uint16 per row, frame and state; 0: bad args)
 * One block per row, sequential over the frames; no host synchronisation, no allocation, no floating-point atomics. */
#define ALIVE_F0_TRACK_MAX_STATES 4000
size_t alive_f0_track_workspace_bytes(int N, int T, int S);
int alive_f0_track_rows(const float* logits, int N, int C, int T, int lo, int S, const double* semis, const int32_t* band_lo,
                        const int32_t* band_hi, const int32_t* on, const double* weight, const double* jump, float* f0,
                        int32_t* changed, void* ws, void* stream);

/* Voicing: f0 = 0 on the frames of a row whose source is not periodic (tools/voicing_ref.py is the NumPy restatement, bit for bit).
 * The detector is a normalised cross-correlation of the 16 kHz signal x[N][ld] (valid length L <= ld, zero beyond it) and does not
 * look at the f0 estimator.  q[i] = clamp(rintf(x[i] * 32768.0f), -32768, 32767) as an integer (NaN -> 0; 0 outside [0, L)), so every
 * sum below is an exact integer (int64) and no summation order can matter.  Per frame t of `hop` samples and lag tau in
 * [lag_lo, lag_hi], with c = hop t + hop / 2 and s = c - floor((W + tau) / 2):
 *   Sxy = sum q[i] q[i + tau], Sxx = sum q[i]^2, Syy = sum q[i + tau]^2 over i in [s, s + W)
 *   rho(tau) = (double)Sxy / sqrt((double)Sxx * (double)Syy) when all three sums are > 0, else 0.0 (each operation rounded on its own)
 *   r[t] = max over tau of rho, lag[t] the lowest tau attaining it (lag_lo when r[t] == 0)
 *   silent[t] = (double)(sum of q[i]^2 over [hop t, hop t + hop)) < floor_e[n]     (host: floor_e = 10^(dB / 10) * hop * 2^30)
 * then per row, in frame order: (a) hysteresis from s = 0: silent -> 0; else r >= thr_on[n] -> 1; else r < thr_off[n] -> 0; else s
 * stays; (b) an unvoiced run of at most `bridge` frames with a voiced frame on both sides and no silent frame in it becomes voiced;
 * (c) a voiced run shorter than `min_run` frames that touches neither end of the row becomes unvoiced.  f0[n][t] (row stride ld_f0)
 * keeps its value on a voiced frame and becomes +0.0f on every other one.
 *   on          DEVICE int32 [N] or NULL (every row): a row with on[n] == 0 does nothing; its f0 row and outputs are untouched
 *   thr_on, thr_off, floor_e   DEVICE double [N], read when the kernels run
 *   r_out (double [N][T]), lag_out, voiced_out (int32 [N][T]), changed (int32 [N]: the frames that were not 0 and were set to 0):
 *               DEVICE or NULL
 *   ws          alive_voicing_workspace_bytes(N, T) bytes (0: bad args)
 * Limits: W <= ALIVE_VOICING_MAX_WINDOW, lag_hi <= ALIVE_VOICING_MAX_LAG (a frame's samples and the int64 prefix sum of their squares
 * lie in 64 KB of LDS).  Two launches whose grids depend on N, T, hop, W and lag_hi alone; no host synchronisation, no allocation,
 * no atomics. */
#define ALIVE_VOICING_MAX_WINDOW 4096
#define ALIVE_VOICING_MAX_LAG 1600
size_t alive_voicing_workspace_bytes(int N, int T);
int alive_voicing_rows(const float* x, int N, int ld, int L, int hop, int T, int lag_lo, int lag_hi, int W, int min_run, int bridge,
                       const int32_t* on, const double* thr_on, const double* thr_off, const double* floor_e, float* f0, int ld_f0,
                       double* r_out, int32_t* lag_out, int32_t* voiced_out, int32_t* changed, void* ws, void* stream);

/* Match path: out of each frame's candidates of a top-k list, ONE library row per frame by a Viterbi path, between a search and its
 * gather (tools/match_path_ref.py is the NumPy restatement, bit for bit).  R list rows of T frames: val / idx [R][T][k_max] as every
 * search form writes them (best first, -1 behind the last valid entry), k_row[r] entries of a frame in use; rows_f32 [P][768] and
 * norms [P] are the table the indices point into.  A frame is active when idx[t][0] >= 0 and no idx[t][i], i < k_row, is >= P (such an
 * index is never dereferenced); state i of an active frame exists when i < k_row and idx[t][i] >= 0.  In fp64, every operation rounded
 * on its own:
 *   e[t][i] = val[t][i] - val[t][0];   c[t][i][j] = dot(a, b) / (norms[a] * norms[b]) with a = idx[t][i], b = idx[t-1][j]
 *   D[t][i] = e[t][i] at t = 0 and after an inactive frame, else e[t][i] + max_j (D[t-1][j] + weight * c[t][i][j])   (lowest j on ties)
 * dot in one fixed order (lane l of 64: products l + 64 q, q ascending from 0.0; then p[l] += p[l + o], o = 32 .. 1).  Each segment of
 * consecutive active frames is traced back from the lowest argmax of D at its end.  Output lists [R][T][k_max]: entry 0 of frame t is
 * the chosen (val, idx), every other entry and every entry of an inactive frame (-inf, -1), so that every gather serves at k = 1; they
 * must not overlap the input lists.  weight = 0 chooses entry 0 everywhere.
 *   k_row, on   DEVICE int32 [R]: a row with on[r] == 0 or k_row[r] outside [1, k_max] is off: its lists are copied, moved[r] = 0
 *   weight      DEVICE double [R], >= 0, in cosine units (the units of e)
 *   moved       DEVICE int32 [R]: the frames whose chosen entry is not entry 0
 *   ws          alive_knn_path_workspace_bytes(R, T, k_max) bytes (0: bad sizes); alive_knn_path_layout: off[0] the byte offset of
 *               J = c as double [R][T][k_max][k_max] (written for existing states of consecutive active frames only), off[1] that of
 *               the back pointers, uint8 [R][T][k_max]
 * Limits: k_max <= ALIVE_KNN_PATH_MAX_K, R * T <= ALIVE_KNN_PATH_MAX_FRAMES.  Two launches (one when T = 1) whose grids depend on R, T
 * and k_max alone; every per-row array is read when the kernels run; no host synchronisation, no allocation, no atomics. */
#define ALIVE_KNN_PATH_MAX_K 8
#define ALIVE_KNN_PATH_MAX_FRAMES 1048576
size_t alive_knn_path_workspace_bytes(int R, int T, int k_max);
int alive_knn_path_layout(int R, int T, int k_max, int64_t* off);
int alive_knn_path_rows(const float* val, const int32_t* idx, const int32_t* k_row, int k_max, const int32_t* on, const double* weight,
                        const float* rows_f32, const float* norms, int64_t P, int R, int T, float* out_val, int32_t* out_idx,
                        int32_t* moved, void* ws, void* stream);
/* the same on a half pool's table rows_f16 [P][768] (see "half-precision voice pool"): the join cost's dot over the widened values in
 * the same order, bitwise alive_knn_path_rows on the fp32 table of the widened values */
int alive_knn_path_rows_f16(const float* val, const int32_t* idx, const int32_t* k_row, int k_max, const int32_t* on,
                            const double* weight, const void* rows_f16, const float* norms, int64_t P, int R, int T, float* out_val,
                            int32_t* out_idx, int32_t* moved, void* ws, void* stream);

/* Arithmetic of the decoder's two largest groups of GEMMs on the batch path (more than 96 columns; the streaming kernels are not
 * affected): (a) the six k = 5 convs of the 256-channel FilterBlock (decoder.py:128-134 at the Filter's coarsest scale), (b) the two
 * pointwise convs of the feature extractor's four AdaptiveConvNeXt1d layers (common.py:74-82), (c) the norm-FiLM projection, the two
 * coarse down convs and the mid conv, (e) the six k = 5 convs of the fused 64-channel FilterBlock.
 *   mode 1 (default since round 5, or ALIVE_DECODER_PRECISION=1): plain fp16 operands, one MFMA per product (AliveConv.precision 3,
 *          AliveGemm.planes 1), fp32 accumulate, fp32 residual streams;
 *   mode 2 (ALIVE_DECODER_PRECISION=2): two-plane split bf16 like the decoder's other GEMMs (rounds 1 - 4);
 *   mode 0: query.  Returns the mode in force.  Process-wide; not to be changed while a decoder call is in flight.
 * Measured on the reference's 450-frame fixture (tests/test_gpu_models.py::test_decoder_precision_modes): decoder waveform RMS error
 * 5.0e-6 in mode 2, 2.90e-5 in mode 1, whole conversion of a 450-frame window 1.22e-4 in both; the bar of the path is 1e-3.  Everything else in the
 * decoder (FiLM projections, input layer, to_amps, strided / transposed convs, the fused 16 / 8-channel FilterBlocks) keeps
 * split bf16 or exact fp32 in both modes, and so do both encoders (top-k / argmax downstream). */
int alive_decoder_precision(int mode);
/* Arithmetic of the pointwise convs of the ConvNeXt layers of ContentEncoder / F0Estimator on the batch path (common.py:54-62):
 *   mode 1 (default since round 5, or ALIVE_ENCODER_PRECISION=1): fp16 split planes, three MFMAs per product (AliveGemm.f16s; 22
 *          significand bits per operand);
 *   mode 2 (ALIVE_ENCODER_PRECISION=2): three bf16 planes, six MFMAs per product (24 bits; rounds 1 - 4);
 *   mode 0: query.  Both are fp32-grade: content features agree with the reference fixture to < 1e-5 of their RMS in either mode and
 * the f0 classes outside the 1e-4 margin are identical (tests/test_gpu_models.py).  In mode 1 the F0Estimator's classifier runs on
 * fp16 split planes too (its input is what last_norm leaves); the DFT and the input / output layers of both encoders stay on three
 * bf16 planes in either mode (their inputs are not range-limited by a normalisation). */
int alive_encoder_precision(int mode);
/* Values that left fp16's range (|scaled value| > 65504) while an fp16 plane was written by any kernel of modes 1 above since the last
 * clear -- they were saturated, not turned into infinities, but the result is then not the reference's.  0 on every tested checkpoint
 * and input.  SYNCHRONISES THE DEVICE (hipDeviceSynchronize, then a 4-byte read per kernel file of the CURRENT device's counters: the
 * caller's streams may be non-blocking, so the null stream alone orders nothing); reset != 0 clears the counters after the read.
 * Returns -1 when a runtime call fails -- callers must treat that as an error, not as "no saturation".
 * module/pipeline.py::Converter.convert_windows clears the counters when a batch starts (alive_f16_saturations_clear), reads them when
 * it ends and repeats the batch in modes 2 when they are not zero. */
int alive_f16_saturations(int reset);
/* Zeroes the counters asynchronously, in the order of `stream` (five 4-byte memsets; no synchronisation, graph-capturable). */
int alive_f16_saturations_clear(void* stream);

/* Decoder.forward (decoder.py:205-210) at harmonics_scale == 1:
 *   x[N][768][Lf], f0[N][Lf], phi_in[N][64] or NULL (phi = 0), crop0,
 *   wave[N][320*Lf], phi_out[N][64] at column phi_col, or NULL. */
size_t alive_decoder_workspace_bytes(int N, int Lf);
int alive_decoder_forward(const float* const* w, const float* x, const float* f0,
                          const float* phi_in, int crop0, int phi_col, int N, int Lf,
                          float* wave, float* phi_out, void* ws, void* stream);

/* pitch transform of inference.py:119-126,130 (mode 0, per-window mean pitch)
 * and realtime_inference.py:156-163 (mode 1); in place on f0[N][T]. */
int alive_pitch_transform(float* f0, int N, int T, int mode, float f0_rate, float pitch_shift,
                          float intonation, void* stream);
/* the same with per-row parameters: f0_rate / pitch_shift / intonation are DEVICE float[N]; row n is bitwise
 * alive_pitch_transform with that row's values */
int alive_pitch_transform_rows(float* f0, int N, int T, int mode, const float* f0_rate, const float* pitch_shift,
                               const float* intonation, void* stream);

/* Auto pitch (csrc/pitch_auto.hip): the source's register measured on the device and turned into a shift towards the target voice's.
 * "pitch" is 12*log2(f0/440) - 9 as alive_pitch_transform forms it (log2 in fp64, rounded once to float32); a frame is voiced when that
 * value is finite (0, NaN and inf are unvoiced, inference.py:121).  All pointers are DEVICE pointers; no call allocates, synchronises
 * or reads anything on the host (graph-capturable).  Sums are fp64 in a fixed order (per row: alive_pitch_transform's tree; then the
 * rows of a group in index order), no floating-point atomics: bitwise reproducible, and a group's result does not depend on the other
 * groups of the call.
 *   alive_pitch_stats_groups   stats[g] = (sum of voiced pitch, voiced count as a double) over frames [t_lo, t_hi) of rows
 *                              first[g] .. first[g+1]-1 of f0[N][T] (first: int32 [G+1]); empty and all-unvoiced groups give (0, 0)
 *   alive_pitch_shift_groups   shift_out[r] for the rows r of group g: offset[g], plus on a group with auto_on[g] != 0 and a voiced
 *                              count > 0 the float32 (target[g] - (float)(sum / count)); offset / target: float [G], auto_on: int32 [G].
 *                              shift_out [N] then feeds alive_pitch_transform_rows (mode 0)
 *   alive_pitch_follow_rows    the streaming update, row n of f0[N][T] (f0_rate, offset, target: float [N]; auto_on: int32 [N]; emit:
 *                              bytes [N]; state: double [N][2] = (S, W)):
 *                                auto_on[n] == 0: shift_out[n] = offset[n] bit for bit, state[n] untouched;
 *                                else, if emit[n] != 0, with p_t = pitch(f0[n][t] * f0_rate[n]) (what mode 1 forms before the shift):
 *                                  S <- decay * S + sum of voiced p_t,  W <- decay * W + voiced count   (emit[n] == 0: state stays)
 *                                then shift_out[n] = offset[n] + (float)(W / (W + prior) * (target[n] - S / W)), the automatic part
 *                                exactly 0 when W == 0.  0 <= decay <= 1, prior >= 0 (a pseudo-count of voiced frames).
 *                              alive_pitch_transform_rows(mode 1, f0_rate, shift_out, ...) then runs unchanged */
int alive_pitch_stats_groups(const float* f0, int N, int T, int t_lo, int t_hi, const int* first, int G, double* stats, void* stream);
int alive_pitch_shift_groups(const double* stats, const int* first, int G, int N, const float* offset, const int* auto_on,
                             const float* target, float* shift_out, void* stream);
int alive_pitch_follow_rows(const float* f0, int N, int T, const float* f0_rate, const float* offset, const int* auto_on,
                            const float* target, const unsigned char* emit, double decay, double prior, double* state,
                            float* shift_out, void* stream);

/* Pitch range (csrc/pitch_auto.hip): the second moment of the same pitch.  The conventions of "Auto pitch" hold: DEVICE pointers, no
 * allocation or host read (graph-capturable), fp64 sums in the same fixed order.  Every fp64 operation is one of + - * / sqrt, rounded on
 * its own, so a host restatement in the same order (tools/pitch_range_ref.py) agrees bit for bit.  The range factor of a group or row is
 *   r = clamp(target_sd / sqrt(v), 1 / range_max, range_max),  r = 1 when v <= 0, target_sd <= 0 or either is not finite,
 * with v the variance of the voiced pitch; range_max is finite and >= 1.
 *   alive_pitch_stats2_groups  stats3[g] = (sum, count, sum of squares); components 0 and 1 are bitwise alive_pitch_stats_groups'
 *   alive_pitch_range_groups   the offline counterpart of alive_pitch_shift_groups (inton: float [G]; target_sd: double [G]; range_on: int32 [G]):
 *                              a group with range_on[g] != 0 and count > 0 has m = sum / count, v = sumsq / count - m * m, and its rows
 *                              get inton_out = (float)((double)inton[g] * r), centre_out = (float)m, centre_on_out = 1; every other
 *                              group's rows get inton_out = inton[g] bit for bit, centre_out = 0, centre_on_out = 0
 *   alive_pitch_follow2_rows   alive_pitch_follow_rows on state3: double [N][3] = (S, W, Q) (inton: float [N]; target_sd: double [N]; range_on:
 *                              int32 [N]).  Row n follows when auto_on[n], or range_on[n], or inton[n] != 1; a row that does not writes
 *                              shift_out = offset[n] bit for bit, inton_out = 1, centre_out = 0, centre_on_out = 0 and leaves its state.
 *                              A following row with emit[n] != 0 updates S and W as alive_pitch_follow_rows does (bitwise) and
 *                              Q <- decay * Q + sum of voiced p_t^2.  Then, when W != 0: a = W / (W + prior), m = S / W,
 *                              v = Q / W - m * m, r as above (1 when range_on[n] == 0), I = (double)inton[n] * r,
 *                              inton_out = (float)(1 + a * (I - 1)), centre_out = (float)m, centre_on_out = (inton_out != 1), and on an
 *                              auto_on row shift_out = offset[n] + (float)(a * (target[n] - m)) (alive_pitch_follow_rows' expression);
 *                              any other row, and every row at W == 0, gives shift_out = offset[n]; W == 0 also gives inton_out = 1,
 *                              centre_on_out = 0: the automatic parts grow from exactly 0
 *   alive_pitch_transform_rows_centred   in place on f0[N][T]; centre: float [N], centre_on: int32 [N].  A row with centre_on[n] == 0 is
 *                              bitwise that row of alive_pitch_transform_rows in the same mode; a row with centre_on[n] != 0 gets
 *                              p = c + (p - c) * inton + shift in float32, each operation rounded, in either mode (f0_rate before in
 *                              mode 1, after in mode 0; NaN and inf -> 0) */
int alive_pitch_stats2_groups(const float* f0, int N, int T, int t_lo, int t_hi, const int* first, int G, double* stats3, void* stream);
int alive_pitch_range_groups(const double* stats3, const int* first, int G, int N, const float* inton, const int* range_on,
                             const double* target_sd, double range_max, float* inton_out, float* centre_out, int* centre_on_out,
                             void* stream);
int alive_pitch_follow2_rows(const float* f0, int N, int T, const float* f0_rate, const float* offset, const int* auto_on,
                             const float* target, const float* inton, const int* range_on, const double* target_sd,
                             const unsigned char* emit, double decay, double prior, double range_max, double* state3, float* shift_out,
                             float* inton_out, float* centre_out, int* centre_on_out, void* stream);
int alive_pitch_transform_rows_centred(float* f0, int N, int T, int mode, const float* f0_rate, const float* shift, const float* inton,
                                       const float* centre, const int* centre_on, void* stream);

/* Input gate of the streaming paths (csrc/gate.hip): which rows are live this tick, decided on the device, and the output edge.
 * All pointers are DEVICE pointers; no call allocates, synchronises or reads anything on the host; the grids depend on N and the
 * strides alone (graph-capturable: a captured call serves any settings).  No floating-point atomics.
 *   alive_gate_rows         one block per row n of x[N][ld] (the 16 kHz rings after the input resample and gain).  Per row: gate_on
 *                           int32, thr_ms double (the threshold as a mean square), hold_ticks int32, emit bytes, world_on int32 (may
 *                           be NULL, then world_eff must be NULL too); S list rows per row with seg_len int32 [N*S]; state int32
 *                           [N][2] = (hold_left, was_open).  ms = (sum of x[n][t]^2, t in [w_lo, w_hi)) / (w_hi - w_lo) in fp64 in a
 *                           fixed order (thread tid: t = w_lo + tid, + 256, ...; then a pairwise tree over the 256 partial sums):
 *                           bitwise reproducible, and the same for a row alone and in any batch.
 *                             gate_on[n] == 0 or emit[n] == 0: g0 = g1 = 1, seg_len_eff = seg_len, follow = emit, world_eff =
 *                               world_on, state[n] untouched (ms_out[n] = 0);
 *                             else loud = ms >= thr_ms[n].  loud: left = hold_ticks[n], open = 1.  Not loud: open = left > 0, then
 *                               left = max(left - 1, 0) -- the gate stays open for exactly hold_ticks ticks after the last loud one.
 *                               g0 = was_open, g1 = open, was_open <- open; skip = g0 == 0 && g1 == 0 (closed at both ends of the
 *                               chunk); seg_len_eff[n*S + s] = skip ? 0 : seg_len[n*S + s]; world_eff = world_on && !skip; follow =
 *                               open (emit is nonzero here).
 *                           Outputs: g0, g1 float [N]; seg_len_eff int32 [N*S]; follow bytes [N]; world_eff int32 [N] or NULL; ms_out
 *                           double [N] or NULL (the level, for tests and meters).  0 <= w_lo < w_hi <= ld.
 *   alive_gate_apply_rows   in place on y[N][ld] (the final waves): for i in [0, span_len[n]) with 0 <= span_lo[n] + i < ld,
 *                           y[n][span_lo[n] + i] *= g0[n] + (g1[n] - g0[n]) * ((float)(i + 1) / (float)span_len[n]) in float32, every
 *                           operation rounded on its own.  A row with g0 == g1 == 1 is not touched (no load, no store); a row with
 *                           g0 == g1 == 0 gets +0.0f stored over its span without a load (a NaN there does not leak); samples outside
 *                           the span are never written.  N <= 65535. */
int alive_gate_rows(const float* x, int N, int ld, int w_lo, int w_hi, const int* gate_on, const double* thr_ms,
                    const int* hold_ticks, const unsigned char* emit, const int* world_on, int S, const int* seg_len, int* state,
                    float* g0, float* g1, int* seg_len_eff, unsigned char* follow, int* world_eff, double* ms_out, void* stream);
int alive_gate_apply_rows(float* y, int N, int ld, const int* span_lo, const int* span_len, const float* g0, const float* g1,
                          void* stream);

/* Seam crossfade of the streaming paths (csrc/seam.hip): the head of every emitted chunk blended with the previous tick's continuation.
 * All pointers are DEVICE pointers; the call does not allocate, synchronise or read anything on the host; the grid depends on N alone
 * (graph-capturable: a captured call serves any settings).  No floating-point atomics.
 *   alive_seam_rows   one block per row n of y[N][ld] (the final waves, after the output resample, before alive_gate_apply_rows), in
 *                     place.  Per row: span_lo int32 (the first emitted sample), shift int32 (the ring's advance per tick in samples
 *                     of y: the session's chunk, NOT the span length -- 441 against 440 at 44.1 kHz with 160-sample ticks), xlen int32
 *                     (X, the crossfade in samples; 0: off), emit bytes; the row's state tail[N][ld_tail] float and stored[N] int32
 *                     (how many samples of the tail are valid).  g0 / g1: both NULL, or the two gains of alive_gate_rows.
 *                       emit[n] == 0: y, tail, stored untouched, stats[n] = {0, 0};
 *                       X == 0: y untouched, stored[n] = 0, stats[n] = {0, 0};
 *                       a row whose regions do not fit (span_lo < 0, X < 0, X > ld_tail, X > shift, span_lo + shift + X > ld): the
 *                         same; nothing outside [0, ld) or [0, ld_tail) is ever read or written;
 *                       else Xe = min(X, max(stored[n], 0)) and, for i < Xe with t = tail[n][i], c = y[n][span_lo + i]:
 *                         y[n][span_lo + i] = t + (c - t) * ((float)(i + 1) / (float)(Xe + 1)) in float32, every operation rounded on
 *                         its own (the weight never reaches 0 or 1); then tail[n][i] = y[n][span_lo + shift + i] for i < X, and
 *                         stored[n] = X -- or 0 where g0 and g1 are given and both 0 for the row: the gate skipped that tick's
 *                         search, so what it decoded is the passed-through source and must not be faded from.
 *                     stats double [N][2] or NULL: {sum over i < Xe of ((double)c - (double)t)^2, sum of (double)c^2} of the UNFADED
 *                     head, in fp64 in a fixed order (thread tid: i = tid, tid + 256, ...; then a pairwise tree over the 256 partial
 *                     sums): bitwise reproducible, and the same for a row alone and in any batch.  N, ld, ld_tail > 0. */
int alive_seam_rows(float* y, int N, int ld, const int* span_lo, const int* shift, const int* xlen, const unsigned char* emit,
                    const float* g0, const float* g1, float* tail, int ld_tail, int* stored, double* stats, void* stream);

/* Limiter (csrc/limit.hip): a lookahead peak limiter in front of the int16 edge (alive_float_to_pcm16 wraps whatever leaves [-1, 1)).
 * All pointers are DEVICE pointers; no call allocates, synchronises or reads anything on the host; the grids depend on N and ld alone
 * (graph-capturable: a captured call serves any settings).  No floating-point atomics; every store is a plain vector store.
 * With ceiling c (0 < c <= 1), lookahead L >= 1 and hold H >= 0 samples, P = L - 1 + H, for stream index i of the emitted signal y:
 *     a[j]   = c / fmaxf(|y[j]|, c)                   the required gain: exactly 1.0f where |y[j]| <= c, 1 for a NaN, 0 for an inf
 *     m[k]   = min a[k - H .. k + L - 1]
 *     g[i]   = (float)(sum over k = i - L + 1 .. i, ascending, in double from 0.0, of (double)m[k] / (double)L)
 *     out[i] = fminf(fmaxf(y[i] * g[i], -c), c)       float32, every operation rounded on its own
 * Every window that enters g[i] contains i: g[i] <= a[i] and |out[i]| <= c whatever the neighbours are.  A NaN or infinite sample comes
 * out as -c (inf * 0 is a NaN, and fminf(fmaxf(NaN, -c), c) = -c); no other sample becomes non-finite.  Bitwise tools/limit_ref.py.
 *   alive_limit_rows    streaming, in place, one block per row n of y[N][ld] (the final waves, after alive_seam_rows and
 *                       alive_gate_apply_rows).  Per row: span_lo, span_len int32 (the emitted span), shift int32 (the ring's advance
 *                       per tick in samples of y: the session's chunk, NOT the span length), look int32 (L; 0: off), hold int32 (H),
 *                       ceil float (c), emit bytes; the row's state hist[N][ld_hist] float: the required gains of its last ld_hist
 *                       emitted samples, the latest last (a new stream starts from 1.0f).  For i in [0, span_len) the past comes from
 *                       hist, the present is y[n][span_lo + i] and the future, stream index span_len + j, is y[n][span_lo + shift + j],
 *                       j < L - 1: where the next tick's span will come from.
 *                         emit[n] == 0: y, hist and gmin[n] untouched;
 *                         look == 0, a ceiling outside (0, 1], or a row whose regions do not fit (look < 0, hold < 0, span_lo < 0,
 *                           span_len < 0, span_len > shift, L > shift, span_lo + shift + L - 1 > ld, P > ld_hist): y untouched, hist
 *                           row = 1.0f, gmin[n] = 1.0f; nothing outside [0, ld) or [0, ld_hist) is ever read or written;
 *                         else only [span_lo, span_lo + span_len) of y is written, and hist becomes the last ld_hist values of (hist,
 *                           a[0 .. span_len)).
 *                       gmin float [N] or NULL: the smallest g of the row's span this tick (1.0f: nothing was reduced).
 *                       N, ld > 0; 0 < ld_hist <= ALIVE_LIMIT_MAX_HIST.
 *   alive_limit_waves   offline, stateless, OUT OF PLACE: out[N][ld] from y[N][ld]; row n's first len[n] samples (int32, clamped to
 *                       [0, ld]) are limited as one signal with a = 1 outside it, the rest of the row is copied; one look / hold for
 *                       the call, ceil float [N] (a row whose ceiling is outside (0, 1] is copied whole).  The grid is tiles of
 *                       ALIVE_LIMIT_TILE samples x rows; a tile's halo is another tile's output range, so an `out` that overlaps `y` is
 *                       refused.  gmin float [N] or NULL: the smallest g of the row (1.0f first, then an integer atomic min on the
 *                       float's bits: every g is >= +0, so the order of the bits is the order of the values and the result does not
 *                       depend on the order).  0 < N <= 65535, ld > 0, look >= 1, hold >= 0, look - 1 + hold <= ALIVE_LIMIT_MAX_HIST.
 *                       Bitwise alive_limit_rows run tick by tick over the same signal. */
#define ALIVE_LIMIT_TILE 1024
#define ALIVE_LIMIT_MAX_HIST 3072
int alive_limit_rows(float* y, int N, int ld, const int* span_lo, const int* span_len, const int* shift, const int* look,
                     const int* hold, const float* ceil, const unsigned char* emit, float* hist, int ld_hist, float* gmin, void* stream);
int alive_limit_waves(float* out, const float* y, int N, int ld, const int* len, int look, int hold, const float* ceil, float* gmin,
                      void* stream);

/* Loudness (csrc/loudness.hip): programme loudness after ITU-R BS.1770-4 / EBU R 128 for one channel, measured and normalised per file
 * (offline) and per session (streaming, between alive_gate_apply_rows and alive_limit_rows).  All pointers are DEVICE pointers; no call
 * allocates, synchronises or reads anything on the host; the grids depend on N, ld and max_tiles alone (graph-capturable: a captured
 * call serves any settings).  No atomics; every store is a plain vector store.  Everything is fp64 with every operation rounded on its
 * own; the device uses only + - * / sqrt and compares, and every 10^x, 2^x and tan is the host's: bitwise tools/loudness_ref.py.
 * K-weighting at rate fs, coef = (b0, b1, b2, a1, a2) of the shelf then of the high-pass, 10 doubles per row, the usual re-derivation of
 * the standard's 48-kHz filter:
 *     shelf      f0 = 1681.974450955533, G = 3.999843853973347, Q = 0.7071752369554196; K = tan(pi f0 / fs), Vh = 10^(G / 20),
 *                Vb = Vh^0.4996667741545416, a0 = 1 + K / Q + K^2; b0 = (Vh + Vb K / Q + K^2) / a0, b1 = 2 (K^2 - Vh) / a0,
 *                b2 = (Vh - Vb K / Q + K^2) / a0, a1 = 2 (K^2 - 1) / a0, a2 = (1 - K / Q + K^2) / a0
 *     high-pass  f0 = 38.13547087602444, Q = 0.5003270373238773; b = (1, -2, 1), a1 and a2 as above
 * Both run in transposed direct form II, the high-pass fed the shelf's o; a non-finite input sample counts as 0.0:
 *     o = b0 v + z1;   z1 = (b1 v - a1 o) + z2;   z2 = b2 v - a2 o
 * With H = hop = (fs + 5) / 10 samples per 100-ms sub-block, q[j] is the sum of the squared filter output p over sub-block j (acc = acc
 * + p p in sample order from 0.0) and block b is z[b] = (((q[b] + q[b + 1]) + q[b + 2]) + q[b + 3]) / (double)(4 H); samples past the
 * last whole sub-block are not measured.  z_abs = 10^((gate + 0.691) / 10), z_t = 10^((target + 0.691) / 10).
 *   alive_loudness_workspace_bytes   scratch of alive_loudness_measure_waves for N rows of at most max_tiles sub-blocks: 9 doubles
 *                       per tile (0: arguments out of range).
 *   alive_loudness_measure_waves   offline, stateless.  y float [N][ld]; per row len (int32, clamped to [0, ld]), hop (int32), coef
 *                       double [N][10] and ap double [N][16]: mixed rates are allowed in one call.  THE FILTER RUNS IN TILES: a tile
 *                       is a sub-block (hop samples), every tile is one lane.  e[j] is the 4-state left by the recurrence over tile j
 *                       from zero state; ap[r * 4 + k] = AP[r][k], column k of AP the state left after hop zero samples from unit
 *                       state k (the host's, by the same recurrence); s[0] = 0 and
 *                           s[j + 1][r] = (((AP[r][0] s[j][0] + AP[r][1] s[j][1]) + AP[r][2] s[j][2]) + AP[r][3] s[j][3]) + e[j][r];
 *                       q[j] comes from the recurrence over tile j started from s[j].  Then, with nb = len / hop and all sums
 *                       ascending from 0.0: pass 1 sums z[b] over the blocks with z[b] > z_abs and counts them, c1; rel = 0.1 (sum1 /
 *                       c1); pass 2 sums over the blocks with z[b] > z_abs and z[b] > rel and counts them, c2; zI = sum2 / c2, or 0.0
 *                       where c2 == 0 (fewer than four sub-blocks, or silence).  A row with hop < 1 or nb > max_tiles is not
 *                       measured (c1 = c2 = 0).  0 < N <= 65535; ld, max_tiles > 0; 0 < z_abs, finite; workspace_bytes at least
 *                       alive_loudness_workspace_bytes(N, max_tiles).
 *   alive_loudness_apply_waves   offline, OUT OF PLACE (an `out` that overlaps y is refused): g = min(max(sqrt(z_t[n] / zI[n]), 1 /
 *                       gmax), gmax), g = 1 where c2[n] == 0; out[i] = (float)((double)y[i] g) for i < len[n], the rest of the row is
 *                       copied.  A row whose z_t is a NaN is copied bit for bit.  gain double [N] or NULL: g per row (1 for a copied
 *                       row).  0 < N <= 65535, ld > 0, 1 <= gmax, finite.
 *   alive_loudness_rows   streaming, in place, one block per row n of y[N][ld].  Per row: span_lo, span_len int32 (the emitted span, n =
 *                       span_len), emit and on bytes, hop int32, coef double [10], par double [ALIVE_LOUDNESS_PARAMS] = (z_abs, z_t, d,
 *                       P, gmax, qs) with d = 2^(-0.1 / half life), P = 10 * the prior in seconds (blocks) and qs = 10^(slew (n / fs) /
 *                       20); the row's state double [ALIVE_LOUDNESS_STATE] = (the four filter states, acc, cnt, the last three q oldest
 *                       first, nsub, S, W, g, 0, 0, 0), a new stream starting from zeros with g = 1.
 *                         emit[n] == 0: y and the state untouched;
 *                         on[n] == 0, or a row whose regions do not fit (hop < 1, span_lo < 0, span_len < 1, span_lo + span_len > ld):
 *                           y untouched, the state back to its start; nothing outside [0, ld) is ever read or written;
 *                         else, for i ascending over the span: filter, acc = acc + p p, cnt = cnt + 1, and when cnt >= hop:
 *                           nsub = min(nsub + 1, 4); z = (((q0 + q1) + q2) + acc) / (double)(4 H); S = S d, W = W d; if nsub == 4 and z
 *                           > z_abs and (W < P or z W > 0.1 S): S = S + z, W = W + 1; (q0, q1, q2) = (q1, q2, acc), acc = cnt = 0.
 *                           Then G = 1 if W == 0, else r = min(max(sqrt(z_t / (S / W)), 1 / gmax), gmax), a = min(W / P, 1), G = 1 + a
 *                           (r - 1); G = min(max(G, g / qs), g qs); y[span_lo + i] = (float)((double)y[span_lo + i] (g + (G - g)
 *                           ((double)(i + 1) / (double)n))); g = G.
 *                       The relative gate is tested against the running mean only while that mean is trusted (W >= P).  N, ld > 0. */
#define ALIVE_LOUDNESS_STATE 16
#define ALIVE_LOUDNESS_PARAMS 6
size_t alive_loudness_workspace_bytes(int N, int max_tiles);
int alive_loudness_measure_waves(const float* y, int N, int ld, const int* len, const int* hop, const double* coef, const double* ap,
                                 double z_abs, int max_tiles, double* zI, int* c1, int* c2, void* workspace, size_t workspace_bytes,
                                 void* stream);
int alive_loudness_apply_waves(float* out, const float* y, int N, int ld, const int* len, const double* zI, const int* c2,
                               const double* z_t, double gmax, double* gain, void* stream);
int alive_loudness_rows(float* y, int N, int ld, const int* span_lo, const int* span_len, const unsigned char* emit,
                        const unsigned char* on, const int* hop, const double* coef, const double* par, double* state, void* stream);

/* The device edge of a sparse multi-session converter (csrc/ring.hip): the sessions' int16 rings kept on the device, and the emitted
 * spans cut there.  All pointers are DEVICE pointers; no call allocates, synchronises or reads anything on the host; the grids depend
 * on N and the strides alone (graph-capturable: a captured call serves any lengths and masks).  No atomics.
 *   alive_ring_push_rows   one block per row n.  ring int16 [N][ld] holds each row's last ring_len[n] samples in TIME ORDER; chunks int16
 *                          [N][ld_chunk] holds this tick's chunk_len[n] new samples of the rows with present[n] != 0 (bytes).  Such a
 *                          row's ring becomes ring[n][cl:rl] ++ chunks[n][0:cl], advanced in place (tile by tile, every tile read
 *                          before it is written), and x[n][j] = (float)ring[n][j] / 32768.0f for j < rl -- bitwise
 *                          alive_pcm16_to_float of the new ring -- with x[n][rl:ld_x] = 0.0f.  A row with present[n] == 0, or whose
 *                          lengths do not fit (cl < 0, cl > rl, cl > ld_chunk, rl > ld, rl > ld_x), is ABSENT: its ring and its row of x
 *                          are neither read nor written.  The same launch writes the tick's masked row arrays: seg_len_tick[n*S + s]
 *                          = seg_len[n*S + s] on a row that takes part and 0 on an absent one (int32 [N*S]; both NULL or neither), and
 *                          world_tick[n] from world_on[n] likewise (int32 [N]; both NULL or neither).  16-byte accesses on rows whose
 *                          cl and rl are multiples of 8 when ring, chunks and x are 16-byte aligned and ld, ld_chunk and ld_x multiples
 *                          of 8; scalar ones otherwise, with the same result.  N, ld, ld_chunk, ld_x, S > 0, N * S < 2^31.
 *   alive_emit_rows        out[n][i] = (short)(int)(wave[n][span_lo[n] + i] * 32768.0f) for i < span_len[n] on the rows with take[n]
 *                          != 0 (bytes) -- bitwise alive_float_to_pcm16 of those samples; the rest of every row of out int16
 *                          [N][ld_out], and every row not taken, is 0.  The spans are device data the host does not read: a row whose
 *                          span does not fit (span_lo < 0, span_len < 0, span_lo + span_len > ld, span_len > ld_out) is written as
 *                          zeros, and nothing outside [0, ld) or [0, ld_out) is ever read or written.  wave float [N][ld].
 *                          0 < N <= 65535, ld > 0, 0 < ld_out < 2^30. */
int alive_ring_push_rows(int16_t* ring, int N, int ld, const int16_t* chunks, int ld_chunk, const int* chunk_len, const int* ring_len,
                         const unsigned char* present, float* x, int ld_x, int S, const int* seg_len, int* seg_len_tick,
                         const int* world_on, int* world_tick, void* stream);
int alive_emit_rows(const float* wave, int N, int ld, const int* span_lo, const int* span_len, const unsigned char* take, int16_t* out,
                    int ld_out, void* stream);

/* Lost-chunk concealment at the input edge of a sparse multi-session converter (csrc/conceal.hip): waveform substitution in the style
 * of G.711 Appendix I on the sessions' int16 rings.  Called in FRONT of alive_ring_push_rows, on the same stream, on a tick that has a
 * lost or a recovering row.  All pointers are DEVICE pointers; the call allocates nothing, synchronises nothing and reads nothing on
 * the host; the grid depends on N alone (graph-capturable: a captured call serves any flags, lengths and constants).  No atomics;
 * every store is a plain vector-memory store.  Bitwise tools/conceal_ref.py.
 *   alive_conceal_rows   one block per row n.  ring int16 [N][ld] (READ ONLY) holds each row's last ring_len[n] samples in time order;
 *                        chunks int16 [N][ld_chunk] is the uploaded chunk buffer, rewritten IN PLACE over chunk_len[n] samples;
 *                        present / lost / on are bytes [N]; lag_lo, lag_hi, window, hold, fade, recover int32 [N] are the row's
 *                        constants in its own samples; state int32 [N][2] = (q: samples made up so far in this run, P: the run's
 *                        period), tmpl int16 [N][ld_tmpl] the run's template.  With cl = chunk_len[n], rl = ring_len[n], W = window[n]:
 *                          present[n] == 0                 absent (a stall): nothing of the row is read or written
 *                          lost[n] == 0 and q == 0         neither lost nor recovering: nothing is read or written
 *                          lost[n] != 0, on[n] == 0        chunk[0:cl] = 0, state = (0, 0)
 *                          lost[n] != 0, on[n] != 0        if q == 0, the period and the template are taken, ONCE per run: for every lag
 *                              l in [lag_lo, lag_hi], C(l) = sum_i a[i] ring[rl - W + i - l] and E(l) = sum_i ring[rl - W + i - l]^2 over
 *                              i < W with a[i] = ring[rl - W + i], exact in int64; score = (double)C * (double)C / (double)E if C > 0 and
 *                              E > 0, else 0; P = the lag of the largest score, the lowest lag on a tie (a silent ring: lag_lo);
 *                              t[j] = ring[rl - P + j] for j < P, and over its last V = P / 4 samples, m = 1 .. V, j = P - V + m - 1:
 *                              t[j] = rint(a + (double)((b - a) m) / (double)(V + 1)), a = ring[rl - P + j], b = ring[rl - 2 P + j];
 *                              t -> tmpl[n][0:P].  If q > 0 the template is read back from tmpl and the ring is not read at all.
 *                              Then chunk[i] = (int16)rint((double)t[(q + i) mod P] * att(q + i)) for i < cl, with att(k) = 0 if d <= 0,
 *                              1 if d >= fade, else (double)d / (double)fade, d = hold + fade - k; state = (min(q + cl, QMAX), P)
 *                          lost[n] == 0, q > 0             recovering: for i < rec = min(recover[n], cl), s = (double)t[(q + i) mod P] *
 *                              att(q + i) and chunk[i] = rint(s + (((double)chunk[i] - s) * (double)(i + 1)) / (double)(rec + 1)),
 *                              clamped to int16; the rest of the chunk is untouched; state = (0, 0)
 *                        every fp64 operation rounded on its own.  A row whose lengths do not fit (cl < 1, cl > ld_chunk, cl > rl, rl >
 *                        ld), whose constants are out of range (lag_lo < 1, lag_hi < lag_lo, lag_hi > ld_tmpl, W < 1, fade < 1, hold <
 *                        0, recover < 0, hold or fade > QMAX), whose ring is shorter than need = max(W + lag_hi, 2 lag_hi), whose need
 *                        exceeds ALIVE_CONCEAL_MAX_SPAN (the samples staged in LDS), or whose state no run leaves behind (q < 0; q > 0
 *                        with P outside [1, lag_hi]) is LEFT ALONE; device data never leads outside a row.  16-byte stores on rows
 *                        whose cl is a multiple of 8 when chunks is 16-byte aligned and ld_chunk a multiple of 8; scalar ones
 *                        otherwise, with the same result.  N, ld, ld_tmpl > 0, 0 < ld_chunk < 2^30. */
#define ALIVE_CONCEAL_MAX_SPAN 4096
#define ALIVE_CONCEAL_QMAX (1 << 30)
int alive_conceal_rows(const int16_t* ring, int N, int ld, const int* ring_len, int16_t* chunks, int ld_chunk, const int* chunk_len,
                       const unsigned char* present, const unsigned char* lost, const unsigned char* on, const int* lag_lo,
                       const int* lag_hi, const int* window, const int* hold, const int* fade, const int* recover, int* state,
                       int16_t* tmpl, int ld_tmpl, void* stream);

/* Envelope follow (csrc/envelope.hip): the converted wave y takes on the loudness contour of the source x that lies beside it sample
 * for sample (both at 16 kHz: the streaming ring and the decoder's wave of a tick; an utterance and its conversion).  Stateless and OUT
 * OF PLACE: out[N][ld_y] from y[N][ld_y] and x[N][ld_x].  All pointers are DEVICE pointers; the call allocates nothing, synchronises
 * nothing and reads nothing on the host; the grid depends on N, ld_y and hop alone (graph-capturable: a captured call serves any amounts
 * and lengths).  No floating-point atomics; every store is a plain vector store.
 * Per row, with n = len[row] clamped to [0, min(ld_y, ld_x)] (len NULL: ld_y, clamped likewise), frames of `hop` samples,
 * F = ceil(n / hop), R = radius, m = amount[row], e = floor_ms (a mean square) and the range [g_lo, g_hi], everything in fp64 with
 * every operation rounded on its own:
 *     Sx[f], Sy[f]  sums of squares over [f hop, min((f + 1) hop, n)) in one fixed order: 256 accumulators, accumulator a adds
 *                   v[f hop + a + 256 j]^2 for ascending j from 0.0 (a missing sample adds +0.0); s[l] = (acc[4l] + acc[4l + 1]) +
 *                   (acc[4l + 2] + acc[4l + 3]) for l < 64; then s[l] = s[l] + s[l + o] for l < o, o = 32, 16, .., 1; the sum is s[0]
 *     Px, Py        sums of Sx[t] / Sy[t] over t = a .. b ascending from 0.0, a = max(f - R, 0), b = min(f + R, F - 1)
 *     Cn            (double)(min((b + 1) hop, n) - a hop)
 *     q             (Px / Cn + e) / (Py / Cn + e);   rc = min(max(sqrt(q), g_lo), g_hi) if q is finite, else 1.0
 *     G[f]          1.0 + (double)m * (rc - 1.0)
 *     g[i]          G[0] for i < hop / 2; G[F - 1] for i >= hop / 2 + (F - 1) hop; otherwise G[f] + (G[f + 1] - G[f]) * w with
 *                   f = (i - hop / 2) / hop and w = (double)((i - hop / 2) - f hop) / (double)hop
 *     out[i]        (float)((double)y[i] * g[i]) for i < n; y[i] for i >= n
 * A row whose amount is not in (0, 1] (0, a NaN, 1.5) or whose n is 0 is copied bit for bit.  A NaN in either signal, or an inf in x,
 * makes q non-finite in the frames within R of it: those stay at G = 1 and no other frame changes (an inf in y alone gives q = 0, so
 * g_lo, and the sample stays infinite).  A row's result does not depend on N, on the other rows or on the tiling.  Bitwise
 * tools/envelope_ref.py.
 *   The grid is tiles of ALIVE_ENVELOPE_TILE frames x rows, 256 threads; a tile recomputes the frame sums of radius + 1 frames on each
 *   side, so an `out` that overlaps y or x is refused (a tile's halo is another tile's output).
 *   gain_minmax float [N][2] or NULL: the row's smallest and largest G[f] over f < F as floats, (1, 1) for a copied row (filled with
 *   (+inf, 0) first, then integer atomic min / max on the floats' bits: every G is > 0, so the order of the bits is the order of the
 *   values and the result does not depend on the order).
 *   0 < N <= 65535; ld_y, ld_x > 0; hop even in [2, 1024]; 0 <= radius <= ALIVE_ENVELOPE_MAX_RADIUS; floor_ms > 0;
 *   0 < g_lo <= 1 <= g_hi; all three finite. */
#define ALIVE_ENVELOPE_TILE 16
#define ALIVE_ENVELOPE_MAX_RADIUS 4
int alive_envelope_waves(float* out, const float* y, int ld_y, const float* x, int ld_x, int N, const int* len, const float* amount,
                         int hop, int radius, double floor_ms, double g_lo, double g_hi, float* gain_minmax, void* stream);

/* Post filter (csrc/postfilter.hip): an adaptive formant post filter (Chen and Gersho 1995; G.729 4.2) on the converted 16 kHz wave:
 * per frame an LPC analysis gives A(z), the frame's filter is A(z / b) / A(z / a) with a tilt compensation, and a frame gain restores
 * the level.  Stateless and OUT OF PLACE: out[N][ld] from y[N][ld].  All pointers are DEVICE pointers; the call allocates nothing,
 * synchronises nothing and reads nothing on the host; the grid depends on N, ld and hop alone (graph-capturable: a captured call serves
 * any alphas and lengths).  No floating-point atomics; every store is a plain vector store.
 * Per row, n = len[row] clamped to [0, ld] (len NULL: ld), frames of `hop` samples, F = ceil(n / hop), a = (double)alpha[row],
 * b = a * ratio, e = floor_ms (a mean square).  Per frame f:
 *     q[i]      the int16 grid: clamp(rintf(32768 y[i]), +-32767), a NaN 0, 0 outside [0, n)
 *     s[i]      q[f hop - (window - hop) / 2 + i] * win[i] for i < window          (win: `window` integers, 64 = unity)
 *     R[k]      sum_i s[i] s[i + k] for k = 0 .. order: exact integers (below 2^53 for win <= 64), so their order cannot show
 *     r[k]      (double)R[k] * lag[k]; r[0] = r[0] * 1.0001                         (lag: order + 1 doubles)
 *     Levinson-Durbin in fp64, err = r[0], for m = 1 .. order: acc = r[m], acc = acc + A[j] * r[m - j] for j = 1 .. m - 1 ascending;
 *               k = -acc / err; A'[j] = A[j] + k * A[m - j] for j < m, A'[m] = k; err = err * (1 - k * k)
 *     den[j]    A[j] * a^j, num[j] = A[j] * b^j, A[0] = 1, the powers by repeated multiplication
 *     h0[k]     (k <= order ? num[k] : 0) - acc for k < ALIVE_POSTFILTER_TAPS, acc = 0.0, acc = acc + den[j] * h0[k - j] for
 *               j = 1 .. min(k, order) ascending
 *     t         tilt * (c1 / c0), c0 = sum_k h0[k]^2 and c1 = sum_k h0[k] h0[k + 1], both ascending from 0.0
 *     h[k]      h0[k] - t * h0[k - 1], h[0] = h0[0]
 *     U(f, i)   sum_k h[k] * (double)y[i - k] for k ascending from 0.0, y = 0 before the row's start
 *     g[f]      min(max(sqrt(q), g_lo), g_hi) if q = (Ein + e c) / (Eout + e c) and its denominator are finite (an infinite Eout
 *               would give q = 0), else 1: Ein = sum y[i]^2 and Eout = sum U(f, i)^2 over the frame's own c samples, both in the
 *               order of the envelope follow's frame sums
 * A frame is the identity (h = delta, so g = 1) when R[0] <= 0, when a k is not finite or |k| >= 1, or when err stops being > 0.
 *     out[i]    (float)(g[0] U(0, i)) for i < hop / 2; (float)(g[F - 1] U(F - 1, i)) for i >= hop / 2 + (F - 1) hop; otherwise
 *               (float)(Z0 + (Z1 - Z0) * w) with f = (i - hop / 2) / hop, w = (double)((i - hop / 2) - f hop) / (double)hop,
 *               Z0 = g[f] U(f, i) and Z1 = g[f + 1] U(f + 1, i);  y[i] for i >= n
 * A row whose alpha (the float) is not in (0, 0.85] -- 0, a NaN, 0.9 -- or whose n is 0 is copied bit for bit: the poles lie inside
 * radius a, and at 0.85 the 128 taps leave less than 1e-9 of full scale.  A NaN or an infinite sample makes up to 127 samples behind it
 * non-finite and leaves the gains of the frames those lie in at 1.  A row's result does not depend on N, on the other rows or on the
 * tiling.  Everything after R is fp64 with only + - * / and sqrt, each rounded on its own: bitwise tools/postfilter_ref.py.
 *   The grid is tiles of ALIVE_POSTFILTER_TILE centre-to-centre units x rows, 256 threads; a tile recomputes the filters and gains of
 *   the frames it shares with its neighbours and reads the samples around its own, so an `out` that overlaps y is refused.
 *   gain_minmax float [N][2] or NULL: the row's smallest and largest g[f] as floats, (1, 1) for a copied row (filled with (+inf, 0)
 *   first, then integer atomic min / max on the floats' bits: every g is > 0).
 *   0 < N <= 65535; ld > 0; hop even in [2, 1024]; hop <= window <= 1024 with window - hop even; 1 <= order <=
 *   ALIVE_POSTFILTER_MAX_ORDER and < window; ratio and tilt finite in [0, 1]; floor_ms > 0; 0 < g_lo <= 1 <= g_hi; all finite. */
#define ALIVE_POSTFILTER_TAPS 128
#define ALIVE_POSTFILTER_MAX_ORDER 32
#define ALIVE_POSTFILTER_TILE 16
int alive_postfilter_waves(float* out, const float* y, int ld, int N, const int* len, const float* alpha, int hop, int window,
                           int order, const int16_t* win, const double* lag, double ratio, double tilt, double floor_ms, double g_lo,
                           double g_hi, float* gain_minmax, void* stream);

/* Voice codebooks (csrc/codebook.hip; module/codebook.py build_codebook): the device passes of one k-means iteration over a voice's
 * rows that are not the search.  The assignment of a row is the strict search's top-1 against the centroids (alive_knn_search_strict)
 * and the inverted index a stable sort of the assignment; both are the caller's.  All pointers are DEVICE pointers; no call allocates,
 * copies or synchronises; argument errors return -1 with a message and launch nothing.  No floating-point atomics: every result is
 * bitwise the same run to run, and bitwise tools/codebook_ref.py's.  1 <= C <= M < 2^31, 768 columns.
 *   alive_codebook_workspace_bytes   scratch of alive_codebook_update for M rows and C lists (0: arguments out of range): the plan of
 *                                    the launch plus the chunk sums of split lists, at most about 2 M / 512 slots of 768 doubles.
 *   alive_codebook_update            centroids[c][:] <- the mean of rows[order[i]][:], i in [seg_off[c], seg_off[c + 1]), for every list
 *                                    that is not empty; an empty list's centroid is not written.  order int32 [M]: the rows of list 0,
 *                                    then of list 1, ..., each list in ascending row index; seg_off int32 [C + 1].  Per column, in fp64:
 *                                    a list is cut into chunks of 512 rows, each chunk summed from +0.0 in list order, the chunk sums
 *                                    added from +0.0 in chunk order, the total divided by the count and rounded to fp32 once.  A wave
 *                                    takes one chunk (a lane 12 columns as three 16-byte loads); a list of one chunk is finished by its
 *                                    wave, the others by a second launch.  rows and centroids 16-byte aligned; Dd must be 768.  A list
 *                                    whose boundaries fall or leave [0, M] counts as empty, a row index outside [0, M) is skipped.
 *   alive_codebook_stats             *objective <- the fp64 sum of val[M] (thread t of 1024 adds val[t], val[t + 1024], ... in turn from
 *                                    +0.0, then acc[i] += acc[i + o] for o = 512, ..., 1); *moved <- the number of m with assign[m] !=
 *                                    prev[m], or M when prev is NULL.  One block. */
size_t alive_codebook_workspace_bytes(int64_t M, int64_t C);
int alive_codebook_update(const float* rows, int64_t M, int Dd, const int32_t* order, const int32_t* seg_off, int64_t C,
                          float* centroids, void* ws, void* stream);
int alive_codebook_stats(const int32_t* assign, const int32_t* prev, const float* val, int64_t M, double* objective, int64_t* moved,
                         void* stream);

/* WORLD pitch estimation (`-wpe`): DIO + StoneMask on N rows of L8 samples at fs, in fp64   (reference module/common.py:113-137,
 * pyworld.dio(x, fs, f0_floor, f0_ceil, channels_in_octave=2, frame_period, speed=1, allowed_range=0.1) then pyworld.stonemask).
 * Restated from the published algorithm (tools/world_ref.py is the NumPy restatement; parity with pyworld is unpinned).
 *   alive_world_f0_frames      F = int(1000 L8 / fs / frame_period) + 1 frames per row
 *   alive_world_f0_taps        HOST call: fills host_taps[alive_world_f0_taps_count(...)] doubles with DIO's filter taps (low cut,
 *                              then one Nuttall low-pass per band), cosines from the C library; upload once, pass as `taps`
 *   alive_world_f0             x8 [N][L8] fp32 -> f0_out [N][F] fp32 (0 = unvoiced); workspace of
 *                              alive_world_f0_workspace_bytes(N, L8, fs, f0_floor, f0_ceil, frame_period) bytes (0: bad args).
 *                              fs <= 16000; the lowest band's low-pass may have at most 1024 taps (fs / f0_floor <= ~724)
 *   alive_world_f0_rows        alive_world_f0 over the rows whose row_on[r] (DEVICE int32 [N]) is nonzero, bitwise; the other
 *                              rows get 0 (unvoiced) at every frame and do no other work.  Same plan, workspace and taps; the
 *                              mask is read on the device, so one captured call serves any mix of rows (a null mask is refused)
 *   alive_linear_resize        y [rows][Lout] = torch F.interpolate(x [rows][Lin], Lout, mode='linear', align_corners=False) as
 *                              torch's CPU kernel rounds it (float32, fused multiply-adds where it fuses)                      */
int alive_world_f0_frames(int L8, int fs, double frame_period);
int alive_world_f0_taps_count(int fs, double f0_floor, double f0_ceil);
int alive_world_f0_taps(int fs, double f0_floor, double f0_ceil, double* host_taps);
size_t alive_world_f0_workspace_bytes(int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period);
int alive_world_f0(const float* x8, int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period,
                   const double* taps, float* f0_out, void* ws, size_t ws_bytes, void* stream);
int alive_world_f0_rows(const float* x8, int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period,
                        const double* taps, const int32_t* row_on, float* f0_out, void* ws, size_t ws_bytes, void* stream);
int alive_linear_resize(const float* x, int rows, int Lin, float* y, int Lout, void* stream);
/* TEST ONLY.  alive_world_f0_stages is alive_world_f0 (the same launcher) stopped after the first `stages` (1 .. 5) of its five
 * launches: mean, low cut, bands, select + FixF0Contour, StoneMask; buffers of later stages, and f0_out below 5, are not touched.
 * alive_world_f0_layout is host arithmetic on the same plan: it writes 16 + 3 nb int64 words and returns that count (a negative
 * code where the plan refuses the arguments, -10 for a missing or short `out`; at most 16 + 3 * 32 words):
 *   out[0 .. 5]    F, nb (bands), c (low-cut half width), Ly = L8 + 1, yl_ld = Ly + 2c, total (= alive_world_f0_workspace_bytes)
 *   out[6 .. 15]   byte offsets in the workspace: mean f64 [N], yl f64 [N][yl_ld] (lag n at n + c), iv f64 [N][nb][4][F] (the
 *                  streams' interp1 values; select overwrites stream 0 with the band's candidate), ni i32 [N][nb][4] (interval
 *                  counts), best / s1 / s2 / s3 f64 [N][F] (best band, FixF0Contour steps 1, 2 and 3-4), pos / neg i32 [N][F]
 *   out[16 ..]     h[nb] (band half delay; 4h taps), woff[nb] (offset of the band's taps in the table), bound[nb] (bits of the f64) */
int alive_world_f0_stages(const float* x8, int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period,
                          const double* taps, float* f0_out, void* ws, size_t ws_bytes, int stages, void* stream);
int alive_world_f0_layout(int N, int L8, int fs, double f0_floor, double f0_ceil, double frame_period, int64_t* out, int n_out);

#ifdef __cplusplus
}
#endif
#endif /* ALIVE_VC_H */
