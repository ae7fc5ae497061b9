/* mfa_hip.h — C ABI of libmfa_hip.so: the MI355X (gfx950) alignment hot path.
 *
 * Drop-in boundary: the reference (Cathoven-AI/Montreal-Forced-Aligner) reaches all arithmetic on
 * this path through the kalpy Python objects; each entry point below names the kalpy call it stands behind.  The
 * Python host module (montreal_forced_aligner_amd/) mirrors those objects and binds these symbols with ctypes —
 * INTEGRATION.md shows the binding a maintainer would add.
 *
 * Conventions
 *  - Every function returns 0 on success, <0 on error; mfa_last_error(ctx) gives the message.  No exceptions cross
 *    the ABI.  A per-utterance alignment failure is NOT an error: it is reported in status[] (the reference counts
 *    failures and raises only if none succeed — MFA/alignment/mixins.py:305-324).
 *  - Pointers named d_* are DEVICE pointers owned by the caller (torch tensors or mfa_device_alloc); h_* are host
 *    pointers.  The library never frees caller memory.  All work is enqueued on the ctx stream (mfa_set_stream);
 *    nothing synchronises unless the name says so.
 *  - Ragged batches use CSR offsets: frame_off[u]..frame_off[u+1] are the rows of utterance u.
 *  - One ctx per (process, GPU); calls on a ctx are serialised by the caller.
 */
#ifndef MFA_HIP_H_
#define MFA_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MFA_API __attribute__((visibility("default")))

typedef struct mfa_ctx mfa_ctx;

/* ---- context ------------------------------------------------------------------------------------------------ */
MFA_API mfa_ctx *mfa_create(int device_id);
MFA_API void mfa_destroy(mfa_ctx *ctx);
MFA_API const char *mfa_last_error(mfa_ctx *ctx);
MFA_API int mfa_version(void);
/* Enqueue on the caller's hipStream_t (e.g. torch.cuda.current_stream().cuda_stream; NULL is HIP's default stream, which
 * is what torch uses unless told otherwise).  use_own != 0 switches back to the ctx's private non-blocking stream. */
MFA_API int mfa_set_stream(mfa_ctx *ctx, void *hip_stream, int use_own);
MFA_API int mfa_synchronize(mfa_ctx *ctx);
/* Device-memory helpers for callers without torch. */
MFA_API void *mfa_device_alloc(mfa_ctx *ctx, size_t bytes);
MFA_API int mfa_device_free(mfa_ctx *ctx, void *d_ptr);
MFA_API int mfa_memcpy_h2d(mfa_ctx *ctx, void *d_dst, const void *h_src, size_t bytes);
MFA_API int mfa_memcpy_d2h(mfa_ctx *ctx, void *h_dst, const void *d_src, size_t bytes);
/* HIP-event timing of everything enqueued between begin and end on the ctx stream (bench.py's roofline leg). */
MFA_API int mfa_timer_begin(mfa_ctx *ctx);
MFA_API int mfa_timer_end_ms(mfa_ctx *ctx, float *h_ms);
/* Per-kernel accumulated HIP-event times since the last reset.  which: 0 mfcc, 1 cmvn, 2 feats, 3 gmm, 4 viterbi,
 * 5 resample, 6 pitch, 7 feature codec, 8-11 GMM statistics (lookup, ordering, sums, reduction), 12 equal alignment,
 * 13-16 LDA statistics (lookup, second moment, ordering + class sums, reductions), 17-20 MLLT statistics (lookup,
 * ordering, sums, reductions), 21-23 tree statistics (keys, ordering, sums), 24 speech activity (each entry point's launches),
 * 25-28 diagonal UBM (selection, posteriors, sums, reductions), 29-34 i-vector extractor (pruning, utterance statistics,
 * scatter, products, solve, accumulators), 35-38 PLDA (transform, prepare, sweep, merge), 39-42 clustering (symmetrise, degree, rounds, labels),
 * 43-44 silhouette (offsets, sweep).
 * Enabled with mfa_kernel_timing(ctx, 1) (adds an event pair around each launch). */
MFA_API int mfa_kernel_timing(mfa_ctx *ctx, int enable);
MFA_API int mfa_kernel_time_ms(mfa_ctx *ctx, int which, float *h_ms, int *h_launches);
MFA_API int mfa_kernel_time_reset(mfa_ctx *ctx);

/* ---- MFCC: replaces kalpy.feat.mfcc.MfccComputer(**mfcc_options).compute_mfccs[_for_export]
 *      (MFA/corpus/features.py:193-251, :235; MFA/online/alignment.py:83; options MFA/corpus/features.py:780-820). */
typedef struct {
  float sample_frequency;   /* 16000 */
  float frame_length_ms;    /* 25 */
  float frame_shift_ms;     /* 10 */
  float preemphasis;        /* 0.97 */
  float low_frequency;      /* 20 */
  float high_frequency;     /* 7800 (<=0: relative to Nyquist) */
  float cepstral_lifter;    /* 22 */
  float energy_floor;       /* 0 */
  int32_t num_mel_bins;     /* 23 */
  int32_t num_coefficients; /* 13 */
  int32_t snip_edges;       /* MFA default 0 */
  int32_t remove_dc_offset; /* 1 */
  int32_t use_energy;       /* 0; 1: C0 := the frame's log energy (floored at log(energy_floor) when that is > 0) */
  int32_t raw_energy;       /* 1: energy before pre-emphasis and window; 0: after */
} mfa_mfcc_opts;

MFA_API int mfa_mfcc_configure(mfa_ctx *ctx, const mfa_mfcc_opts *opts);
/* Frames Kaldi extracts from num_samples samples under the configured options (host arithmetic). */
MFA_API int32_t mfa_mfcc_num_frames(mfa_ctx *ctx, int64_t num_samples);
/* d_pcm: int16 samples of all utterances back to back; d_sample_off[n_utt+1]; d_frame_off[n_utt+1] (host computes
 * them with mfa_mfcc_num_frames); d_mfcc: float32 [total_frames][num_coefficients].  max_frames = longest utterance. */
MFA_API int mfa_mfcc_batch(mfa_ctx *ctx, const int16_t *d_pcm, const int64_t *d_sample_off, const int64_t *d_frame_off,
                           int32_t n_utt, int32_t max_frames, float *d_mfcc);
/* Which kernel tail the next mfa_mfcc_batch launches under the configured options: 1 the specialised one (compile-time
 * trip counts; every filterbank plan whose bins have at most 8 pieces), 2 the generic one (any other plan, or
 * MFA_MFCC_GENERIC=1 in the environment, read at every call; the bit reference), 0 before mfa_mfcc_configure. */
MFA_API int mfa_mfcc_path(mfa_ctx *ctx);

/* Host helper for the call above: utterance u's samples h_src[u][0 .. h_sample_off[u+1] - h_sample_off[u]) copied to
 * h_dst + h_sample_off[u] by n_threads host threads (<= 0: hardware concurrency).  h_dst is the caller's staging buffer
 * (pinned memory, followed by ONE asynchronous host-to-device copy): the reference hands kalpy one Segment per utterance
 * (MFA/corpus/features.py:223-235); a batch of 4 096 ten-second utterances is 1.3 GB of samples. */
MFA_API int mfa_gather_pcm(int32_t n_utt, const int16_t *const *h_src, const int64_t *h_sample_off, int16_t *h_dst,
                           int32_t n_threads);

/* ---- Sample-rate conversion ahead of the MFCC: what OfflineFeatureTpl::ComputeFeatures does with a wave whose rate is
 *      not sample_frequency when allow_downsample / allow_upsample are set (MFA passes both as True,
 *      MFA/corpus/features.py:605-607) — Kaldi's LinearResample: a Hann-windowed sinc low-pass at 0.99 x the lower Nyquist
 *      frequency, 6 zero crossings a side, one filter per output phase of a unit of 1/gcd(in_hz, out_hz) seconds.
 * The plan is computed in double precision and each weight is rounded once to float32; the device sums
 * acc = fmaf(w, (float)x, acc) over a phase's taps in ascending order from 0.0f (taps outside the utterance dropped) and
 * stores acc rounded to nearest-even and clamped to int16 — so the MFCC that follows sees exactly what it would see had
 * the file been converted to 16-bit PCM at the model's rate beforehand.  Rates: 1 000 - 384 000 Hz. */
/* Output samples for n input samples (Kaldi GetNumOutputSamples with flush): host arithmetic, < 0 on bad arguments. */
MFA_API int64_t mfa_resample_num_samples(int32_t in_hz, int32_t out_hz, int64_t n);
/* The filter bank the kernel uses, on the host (no context): phases = out_hz/gcd, in_per_unit = in_hz/gcd, and per phase i
 * h_first[i] (first input of output i of a unit, relative to the unit's first input; may be negative), h_taps[i] and the
 * row h_weights[i][0 .. max_taps) (zero beyond h_taps[i]).  Output k = u*phases + i is
 * sum_j h_weights[i][j] * x[h_first[i] + u*in_per_unit + j].  Any of the pointers may be NULL: call once with NULL arrays
 * for the sizes.  < 0: rates outside the limits, or equal. */
MFA_API int mfa_resample_plan(int32_t in_hz, int32_t out_hz, int32_t *phases, int32_t *in_per_unit, int32_t *max_taps,
                              int32_t *h_first, int32_t *h_taps, float *h_weights);
/* The same bank with the low-pass cutoff (Hz; 0 < 2 * cutoff_hz < both rates) and the zero crossings kept on each side (1 - 64)
 * chosen by the caller, and equal rates allowed (one phase: a plain low-pass): Kaldi's LinearResample(in, out, cutoff, zeros).
 * mfa_resample_plan is this with (0.99 x the lower Nyquist frequency, 6), bit for bit; the pitch tracker's down-sampler
 * (mfa_pitch_batch) is (sample_frequency -> resample_frequency, lowpass_cutoff, lowpass_filter_width). */
MFA_API int mfa_resample_plan_general(int32_t in_hz, int32_t out_hz, double cutoff_hz, int32_t zeros, int32_t *phases,
                                      int32_t *in_per_unit, int32_t *max_taps, int32_t *h_first, int32_t *h_taps,
                                      float *h_weights);
/* Consecutive output samples one workgroup of the kernel produces (tests place utterance lengths around it). */
MFA_API int32_t mfa_resample_block_outputs(void);
/* Resamples the n_sel utterances d_utt[0 .. n_sel) — all recorded at in_hz — of a ragged batch: utterance u's samples are
 * d_in[d_in_off[u] .. d_in_off[u+1]) and its output goes to d_out[d_out_off[u] .. d_out_off[u+1]), whose length the caller
 * computed with mfa_resample_num_samples.  Both offset arrays span the whole batch (which may hold several rates: one call
 * per distinct rate, all writing the same d_out); max_out = longest output among the selected utterances.  The plan of a
 * pair of rates is built on first use and kept in the context.  Errors: rates outside the limits, in_hz == out_hz, more
 * than 65 535 selected utterances. */
MFA_API int mfa_resample_batch(mfa_ctx *ctx, int32_t in_hz, int32_t out_hz, const int16_t *d_in, const int64_t *d_in_off,
                               int16_t *d_out, const int64_t *d_out_off, const int32_t *d_utt, int32_t n_sel, int64_t max_out);

/* ---- Pitch and voicing: replaces kalpy.feat.pitch.PitchComputer(**pitch_options).compute_pitch[_for_export]
 *      (MFA/corpus/features.py:687-688, :340-355; pasted after CMVN, MFA/alignment/multiprocessing.py:1290-1294; options
 *      MFA/models.py:551-576) = Kaldi ComputeKaldiPitch (offline, whole utterance) followed by ProcessPitch.
 * Kaldi's source is not among this project's references: the algorithm is RESTATED ("Pitch"; tests/pitch_ref.py)
 * and pinned by what a pitch tracker has to do, not by parity with Kaldi's arithmetic.
 *  1. down-sample: LinearResample(sample_frequency -> resample_frequency, lowpass_cutoff, lowpass_filter_width) to float32
 *     (acc = fmaf(w, (float)x, acc) over a phase's taps in ascending order from 0.0f, no rounding to int16);
 *  2. per frame a window of N + last_lag resampled samples (zeros outside the utterance), minus the mean of its first N;
 *     per measured integer lag l: inner = sum_k w[k] w[k+l], norm = (sum_k w[k]^2)(sum_k w[k+l]^2) (fmaf chains over
 *     ascending k < N from 0.0f) and two NCCFs inner / sqrtf(norm + ballast) (0 where the denominator is 0): ballast
 *     (mean_square * N)^2 * nccf_ballast for the pitch NCCF, 0 for the voicing (POV) NCCF;
 *  3. both NCCFs up-sampled onto the state lags lag_i = (1 + delta_pitch)^i / max_f0 <= 1 / min_f0 by a Hann-windowed sinc
 *     (cutoff resample_frequency / 2, upsample_filter_width zero crossings; fmaf over ascending taps from 0.0f);
 *  4. Viterbi over the states: local_i = fmaf(soft_min_f0 * lag_i, n_i, 1 - n_i), fwd_t[i] = min_j (fwd_{t-1}[j] +
 *     c * (i-j)^2) + local_i with c = delta_pitch^2 * penalty_factor, the frame's minimum subtracted after every frame;
 *     ties take the SMALLEST j and the final state is the smallest argmin (Kaldi's tie order is not reproduced);
 *     raw output per frame: (POV NCCF at the state, 1 / lag_state Hz);
 *  5. ProcessPitch: POV feature, normalised log-pitch (POV-weighted mean over +-normalization_context frames), raw log-pitch.
 * Stages 1-4 are exact float32 contracts (a float32 numpy restatement is bit-identical); stage 5 uses the device's logf /
 * expf / powf and is checked under a tolerance. */
typedef struct {
  float sample_frequency;        /* 16000 */
  float frame_length_ms;         /* 25 */
  float frame_shift_ms;          /* 10 */
  float min_f0;                  /* 50 */
  float max_f0;                  /* MFA: 800 (Kaldi: 400) */
  float soft_min_f0;             /* 10 */
  float penalty_factor;          /* 0.1 */
  float lowpass_cutoff;          /* 1000 */
  float resample_frequency;      /* 4000 */
  float delta_pitch;             /* 0.005 */
  float nccf_ballast;            /* 7000 */
  float preemphasis;             /* 0 (anything else is refused) */
  float pov_scale;               /* 2 */
  float pov_offset;              /* 0 */
  float pitch_scale;             /* 2 */
  int32_t lowpass_filter_width;  /* 1 */
  int32_t upsample_filter_width; /* 5 */
  int32_t snip_edges;            /* MFA's model default 1 */
  int32_t normalization_context; /* 75 frames on each side */
  int32_t add_pov_feature;       /* use_voicing */
  int32_t add_normalized_log_pitch; /* use_pitch and normalize_pitch */
  int32_t add_raw_log_pitch;     /* use_pitch and not normalize_pitch */
  int32_t add_delta_pitch;       /* refused: Kaldi adds Gaussian noise to it, so like dither it has no parity domain */
} mfa_pitch_opts;

/* Refused with a message, the context keeping its previous options and staying usable: add_delta_pitch, preemphasis != 0,
 * min_f0 >= max_f0 or min_f0 <= 0, max_f0 >= resample_frequency / 2 - 100 Hz (no room for the up-sampling filter below the
 * Nyquist lag: one measured lag at least must lie under 1 / max_f0), 2 * lowpass_cutoff >= either rate, non-integer rates,
 * more than 2 048 states, 1 024 measured lags or 2 048 window samples (what a workgroup's LDS holds), no column asked for. */
MFA_API int mfa_pitch_configure(mfa_ctx *ctx, const mfa_pitch_opts *opts);
/* Frames the tracker gives for num_samples samples (host arithmetic): with n the resampled length
 * (mfa_resample_num_samples) and N, shift the window and shift in resampled samples, 0 when n < N; otherwise
 * (n - N) / shift + 1 with snip_edges, (int)(n / shift + 0.5) without.  The MFCC's count may differ by one: a caller pastes
 * min(mfcc, pitch) frames when they differ by at most 1 (paste-feats, length tolerance 1) and refuses the utterance otherwise. */
MFA_API int32_t mfa_pitch_num_frames(mfa_ctx *ctx, int64_t num_samples);
MFA_API int32_t mfa_pitch_num_states(mfa_ctx *ctx);
/* Columns mfa_pitch_process_batch writes under the configured options (1 - 3). */
MFA_API int32_t mfa_pitch_num_columns(mfa_ctx *ctx);
/* Device workspace mfa_pitch_batch will hold for a batch of this shape: back-pointers uint16 [frames][states], the POV NCCF
 * [frames][lags] and the resampled signal, for as many utterances as fit the workspace budget at a time — 2 GiB, or
 * environment MFA_PITCH_WORKSPACE_MB (read at every call) — and never less than the largest single utterance needs
 * (max_samples, max_frames).  The utterances of a batch are tracked in sub-launches that fit it. */
MFA_API size_t mfa_pitch_workspace_bytes(mfa_ctx *ctx, int32_t n_utt, int64_t total_samples, int64_t total_frames,
                                         int64_t max_samples, int32_t max_frames);
/* d_pcm / d_sample_off as for mfa_mfcc_batch (samples at sample_frequency); d_frame_off[n_utt+1]: rows of every utterance
 * in d_raw, float32 [total_frames][2] = (POV NCCF, pitch in Hz), exactly mfa_pitch_num_frames rows each (the trace-back
 * starts at the utterance's last frame: a row the paste rule drops is dropped afterwards, as paste-feats does).  h_sample_off / h_frame_off: host copies of the two
 * offset arrays (workspace sizing and sub-launches without a synchronisation on device data). */
MFA_API int mfa_pitch_batch(mfa_ctx *ctx, const int16_t *d_pcm, const int64_t *d_sample_off, const int64_t *d_frame_off,
                            const int64_t *h_sample_off, const int64_t *h_frame_off, int32_t n_utt, int32_t max_frames,
                            float *d_raw);
/* ProcessPitch on the raw output: the configured columns of frame r go to d_out[r * out_stride + out_col0 ...] (float32; a
 * wider base-feature matrix whose first columns hold the MFCCs, or a matrix of its own with out_stride = columns). */
MFA_API int mfa_pitch_process_batch(mfa_ctx *ctx, const float *d_raw, const int64_t *d_frame_off, int32_t n_utt,
                                    int32_t max_frames, float *d_out, int32_t out_stride, int32_t out_col0);
/* Test aid.  Host tables, no device: with ctx NULL the tables of *opts (otherwise of the configured options).  h_sizes[8] =
 * {states, first measured lag, last measured lag, up-sampler max taps, N, shift, down-sampler phases, down-sampler max
 * taps}; h_lags / h_soft_min_lag / h_penalty [states]; h_up_first / h_up_taps [states], h_up_weights [states][max taps].
 * Every array pointer may be NULL (call once for the sizes).  Device stages (ctx and d_pcm non-NULL): tracks the batch as
 * mfa_pitch_batch does, in ONE sub-launch whatever the budget, and copies out what the caller gave room for: d_resampled
 * (float32, utterance u at d_rs_off[u], length mfa_resample_num_samples), d_nccf_pitch / d_nccf_pov [total_frames][states]
 * (the up-sampled NCCFs), d_path [total_frames] (state per frame), d_raw [total_frames][2].  Returns 0, < 0 on refusal
 * (ctx NULL: no message is kept). */
MFA_API int mfa_debug_pitch_stages(mfa_ctx *ctx, const mfa_pitch_opts *opts, int32_t *h_sizes, float *h_lags,
                                   float *h_soft_min_lag, float *h_penalty, int32_t *h_up_first, int32_t *h_up_taps,
                                   float *h_up_weights, const int16_t *d_pcm, const int64_t *d_sample_off,
                                   const int64_t *d_frame_off, const int64_t *h_sample_off, const int64_t *h_frame_off,
                                   int32_t n_utt, int32_t max_frames, float *d_resampled, const int64_t *d_rs_off,
                                   float *d_nccf_pitch, float *d_nccf_pov, int32_t *d_path, float *d_raw);

/* ---- CMVN statistics: replaces CmvnComputer().compute_cmvn_from_features / export_cmvn
 *      (MFA/corpus/acoustic_corpus.py:1315-1367; MFA/online/alignment.py:86-88).
 * d_spk_utt_off[n_spk+1] / d_spk_utt[…]: utterances of each speaker; d_stats: float64 [n_spk][2][dim+1]
 * (row 0: sums + count, row 1: sums of squares — Kaldi's layout).  Deterministic summation order. */
MFA_API int mfa_cmvn_stats(mfa_ctx *ctx, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt, int32_t dim,
                           const int32_t *d_spk_utt_off, const int32_t *d_spk_utt, int32_t n_spk, double *d_stats);

/* ---- Final features: replaces FeatureArchive(..., cmvn, deltas | lda_mat, transform) iteration / the explicit chain at
 *      MFA/alignment/multiprocessing.py:1287-1304: ApplyCmvn → compute_deltas | splice_frames+LDA → fMLLR.
 * mode 0: CMVN + Δ+ΔΔ (order 2, window 2): out dim = 3*dim; with d_fmllr non-NULL the per-speaker transform follows the
 *         deltas in the same launch: d_fmllr[n_spk][3*dim][3*dim+1], out[t][o] = Σ_d W[o][d]·y[t][d] + W[o][3*dim] with
 *         y the Δ+ΔΔ vector (fmaf over ascending d, offset last).  d_lda / lda_rows / lda_cols are not read.
 * mode 1: CMVN + splice(±ctx) + LDA d_lda[lda_rows][lda_cols] (+ fMLLR d_fmllr[n_spk][lda_rows][lda_rows+1] if non-NULL).
 * d_utt2spk[n_utt] indexes d_cmvn and d_fmllr (NULL: every utterance takes row 0 of d_fmllr; d_cmvn then must be NULL);
 * d_cmvn may be NULL (no CMVN).  The caller vouches for n_spk: the rows are indexed by d_utt2spk alone. */
MFA_API int mfa_feats_batch(mfa_ctx *ctx, const float *d_mfcc, const int64_t *d_frame_off, int32_t n_utt, int32_t max_frames,
                            int32_t dim, const int32_t *d_utt2spk, const double *d_cmvn, int32_t mode, int32_t splice_ctx,
                            const float *d_lda, int32_t lda_rows, int32_t lda_cols, const float *d_fmllr, float *d_out);

/* ---- Feature codec: Kaldi CompressedMatrix, method kOneByteWithColHeaders ("CM") — what compute_mfccs_for_export /
 *      compute_pitch_for_export (compress=True) and FinalFeatureFunction store (MFA/corpus/features.py:235, :356-365).
 * d_feats: float32 [total_frames][stride]; for every utterance with rows, columns [c0, c1) of its rows are one table.
 * Bit-identical to kaldi_io.write_compressed_matrix / _read_compressed (the specification):
 *   d_global  float  [n_utt][2]            min, range of the table                                   (or NULL)
 *   d_colhdr  uint16 [n_utt][c1-c0][4]     the columns' 0/25/75/100-th percentile codes             (or NULL)
 *   d_bytes   uint8, utterance k at d_frame_off[k]*(c1-c0), column-major [c1-c0][rows]               (or NULL)
 *   d_out     float32 [total_frames][stride]: what a reader makes of those headers and bytes; only columns [c0, c1) are
 *             written (or NULL).  It may not be d_feats.
 * d_cmvn float64 [n_spk][2][cmvn_dim+1] with d_utt2spk [n_utt] (both or neither): the speaker's mean
 * (float)(sum[c] / count) is subtracted in float32 before the table is compressed (ApplyCmvn without variance
 * normalisation, then the second trip); cmvn_dim >= c1.  An utterance without rows has no table: nothing of it is written.
 * Any number of rows (a table of at most mfa_compress_resident_values() values is held in LDS, a longer one is read
 * from memory by the same passes) and of utterances.  Non-finite input has no defined result.  Asynchronous on the
 * context's stream. */
MFA_API int32_t mfa_compress_resident_values(void);
MFA_API int mfa_compress_batch(mfa_ctx *ctx, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt, int32_t stride,
                               int32_t c0, int32_t c1, const double *d_cmvn, const int32_t *d_utt2spk, int32_t cmvn_dim,
                               float *d_out, float *d_global, uint16_t *d_colhdr, uint8_t *d_bytes);
/* Debug/test: the codec's arithmetic (the functions the kernel runs, compiled for the host) on one host table
 * h_table [rows][cols], order statistics by a sort: h_global [2], h_colhdr [cols][4], h_bytes [cols][rows],
 * h_out [rows][cols], each or NULL.  No context, no device.  < 0: an empty table. */
MFA_API int mfa_debug_compress_host(const float *h_table, int32_t rows, int32_t cols, float *h_global, uint16_t *h_colhdr,
                                    uint8_t *h_bytes, float *h_out);

/* ---- Speech activity: Kaldi's energy VAD (compute-vad, kalpy VadComputer), apply-cmvn-sliding, select-voiced-frames +
 *      subsample-feats, and the runs of voiced frames the reference's segmenter walks frame by frame
 *      (MFA/vad/multiprocessing.py:324-406, MFA/vad/models.py:44-130, MFA/corpus/features.py:284-342).
 * All of them take a ragged batch with d_frame_off[0] = 0 and total_frames = d_frame_off[n_utt] < 2^31, given by the caller
 * (the grids are sized from it), and are parallel over the frames inside an utterance.  The arithmetic lives in
 * csrc/vad_math.hpp, host and device; the mfa_debug_*_host twins (csrc/vad_host.cpp: no context, no device) run the same
 * operations in the same order, and every result below has the same bits on either side, whatever else is in the batch, in
 * whatever order, and whatever the grid.
 *
 * The integer scan all of them rest on: d_scan[f] = Σ d_values[g] over the frames g < f of f's own utterance (an exclusive
 * scan that starts again at every d_frame_off boundary), d_totals[u] = the utterance's sum (either may be NULL).  Built
 * reduce-then-scan: sums of blocks of mfa_vad_scan_block_frames() consecutive frames, an exclusive scan of the block sums
 * by one workgroup (a thread walks more than one block sum once there are more than mfa_vad_scan_totals_threads() of
 * them), then the scan inside every block.  No workgroup waits for another.  Sums must stay below 2^31. */
MFA_API int32_t mfa_vad_scan_block_frames(void);
MFA_API int32_t mfa_vad_scan_totals_threads(void);
MFA_API int mfa_vad_scan_batch(mfa_ctx *ctx, const int32_t *d_values, const int64_t *d_frame_off, int32_t n_utt,
                               int64_t total_frames, int32_t *d_scan, int32_t *d_totals);
MFA_API int mfa_debug_vad_scan_host(const int32_t *h_values, const int64_t *h_frame_off, int32_t n_utt, int32_t *h_scan,
                                    int32_t *h_totals);

/* Energy VAD (Kaldi ComputeVadEnergy) on column 0 of d_feats float32 [total_frames][stride], e(t) = that column:
 *   thr(u)     = (float)((double)energy_threshold + (double)energy_mean_scale · (sum / T)) for energy_mean_scale != 0 and
 *                T > 0, else energy_threshold.  sum is float64 in this order: the utterance is cut into chunks of
 *                mfa_vad_sum_chunk_frames() frames from its first frame; inside a chunk, lane l of 256 adds frames l, l + 256, …
 *                in that order from 0.0; the 256 lane sums are folded by halving (lane l += lane l + 128, then + 64, … + 1);
 *                the chunk sums are added in chunk order from 0.0.
 *   voiced(t)  iff (float)num >= (float)den · proportion_threshold (one float32 product), den = frames of [t − ctx, t + ctx]
 *                inside the utterance, num = those of them with e > thr, from the scan above — exact for any
 *                frames_context >= 0.
 * d_vad float32 [total_frames] 1.0 / 0.0 (what compute-vad writes), d_thr float32 [n_utt], d_voiced int32 [n_utt] (NULL:
 * not wanted).  The reference's adaptive mode (threshold = the mean of c0, mean scale 0) is energy_threshold 0,
 * energy_mean_scale 1 here; numpy's float32 pairwise mean and this float64 mean can differ in the last bit. */
typedef struct {
  float energy_threshold;      /* Kaldi 5.0; the reference passes 5.5 */
  float energy_mean_scale;     /* 0.5 */
  float proportion_threshold;  /* 0.6 */
  int32_t frames_context;      /* 0 */
} mfa_vad_opts;
MFA_API int32_t mfa_vad_sum_chunk_frames(void);
MFA_API int mfa_vad_batch(mfa_ctx *ctx, const float *d_feats, int32_t stride, const int64_t *d_frame_off, int32_t n_utt,
                          int64_t total_frames, int32_t max_frames, const mfa_vad_opts *opts, float *d_vad, float *d_thr,
                          int32_t *d_voiced);
MFA_API int mfa_debug_vad_host(const float *h_feats, int32_t stride, const int64_t *h_frame_off, int32_t n_utt,
                               const mfa_vad_opts *opts, float *h_vad, float *h_thr, int32_t *h_voiced);

/* Sliding-window CMVN (Kaldi SlidingWindowCmn) of columns [0, dim) of d_feats [total_frames][stride] into d_out of the
 * same shape (not d_feats itself); columns [dim, stride) are copied.  The window of frame t of T:
 *   center: start = t − cmn_window / 2, end = start + cmn_window; else start = t − cmn_window, end = t + 1;
 *   start < 0: end −= start, start = 0;  not center and end > t: end = max(t + 1, min_window);
 *   end > T: start −= end − T, end = T, start = max(start, 0).
 * out = (float)((x − sum / n) · f) in float64, rounded once; f = 1 without norm_vars or with n = 1, else
 * 1 / sqrt(max(sumsq / n − (sum / n)², 1e-10)).  sum and sumsq are float64 running sums with this order: the utterance is
 * cut into tiles of mfa_sliding_cmvn_tile_frames() frames from its first frame; a tile's first frame adds its window's
 * frames in frame order from 0.0; every next frame first takes off the frames that left the window, in frame order, then
 * adds the ones that entered, in frame order (a window that does not continue the previous one is summed from 0.0 again). */
typedef struct {
  int32_t cmn_window;          /* Kaldi 600; the reference's archive 300 */
  int32_t min_window;          /* 100 */
  int32_t center;              /* 0 */
  int32_t norm_vars;           /* 0 */
} mfa_sliding_cmvn_opts;
MFA_API int32_t mfa_sliding_cmvn_tile_frames(void);
MFA_API int mfa_sliding_cmvn_batch(mfa_ctx *ctx, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt,
                                   int32_t max_frames, int32_t dim, int32_t stride, const mfa_sliding_cmvn_opts *opts,
                                   float *d_out);
MFA_API int mfa_debug_sliding_cmvn_host(const float *h_feats, const int64_t *h_frame_off, int32_t n_utt, int32_t dim,
                                        int32_t stride, const mfa_sliding_cmvn_opts *opts, float *h_out);

/* Frame selection: select-voiced-frames (rows with d_vad[f] != 0; NULL: all rows) followed by subsample-feats n >= 1 (rows
 * 0, n, 2n, … of what remains: ceil(T' / n) rows; Kaldi's negative offset form is refused).  Two steps, as the caller sizes
 * the output: mfa_select_frames_count writes d_out_off int64 [n_utt + 1] (the new frame offsets) and d_src int32
 * [total_frames], whose first d_out_off[n_utt] entries name the source row of every output row; mfa_select_frames_batch
 * is the gather of n_out rows of dim columns (strides in floats) by that map. */
MFA_API int mfa_select_frames_count(mfa_ctx *ctx, const float *d_vad, const int64_t *d_frame_off, int32_t n_utt,
                                    int64_t total_frames, int32_t n, int32_t *d_src, int64_t *d_out_off);
MFA_API int mfa_select_frames_batch(mfa_ctx *ctx, const float *d_feats, int32_t stride, int32_t dim, const int32_t *d_src,
                                    int64_t n_out, float *d_out, int32_t out_stride);
MFA_API int mfa_debug_select_frames_host(const float *h_vad, const int64_t *h_frame_off, int32_t n_utt, int32_t n,
                                         int32_t *h_src, int64_t *h_out_off);

/* Runs of voiced frames: every maximal run of frames with d_vad != 0 inside an utterance, in order, as (first frame, last
 * frame + 1) relative to the utterance's first frame; d_run_off int64 [n_utt + 1]: run_off[u] .. run_off[u + 1] are the
 * runs of utterance u.  d_run_begin / d_run_end int32 [capacity]: runs beyond capacity are counted, not written — the
 * caller reads d_run_off[n_utt] and calls again with room for all when it is larger. */
MFA_API int mfa_vad_runs_batch(mfa_ctx *ctx, const float *d_vad, const int64_t *d_frame_off, int32_t n_utt,
                               int64_t total_frames, int64_t capacity, int32_t *d_run_begin, int32_t *d_run_end,
                               int64_t *d_run_off);
MFA_API int mfa_debug_vad_runs_host(const float *h_vad, const int64_t *h_frame_off, int32_t n_utt, int64_t capacity,
                                    int32_t *h_run_begin, int32_t *h_run_end, int64_t *h_run_off);

/* ---- Acoustic model: replaces GmmAligner.__init__'s model load (+ .boost_silence, applied by the host to gconsts)
 *      (MFA/alignment/multiprocessing.py:814-815).  Host arrays, SoA over all Gaussians:
 * gconsts[G], means_invvars[G][dim], inv_vars[G][dim], pdf_offsets[num_pdfs+1].  Packs them for the MFMA kernel. */
MFA_API int mfa_load_gmm(mfa_ctx *ctx, int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                         const float *h_means_invvars, const float *h_inv_vars);
/* Slot class of a pdf in the packed model (rows it occupies in an MFMA block: 1, 4, 8, 16 or 32); the host must order
 * each utterance's pdf list by descending slot class (mfa_gmm_sort_pdf_list does it). */
MFA_API int32_t mfa_gmm_slot(mfa_ctx *ctx, int32_t pdf);
/* Sort h_pdfs[n] in place into the order the scoring kernels require; h_class_counts[6] receives how many pdfs fall in
 * the classes {32 rows single block, 32 rows multi-block (>32 Gaussians), 16, 8, 4, 1}. */
MFA_API int mfa_gmm_sort_pdf_list(mfa_ctx *ctx, int32_t *h_pdfs, int32_t n, int32_t *h_class_counts);
/* Same, with a per-pdf key (h_first_frame[n], permuted along): inside each class the pdfs are ordered by ascending key.
 * With key = first frame at which the decoder can ask for the pdf (mfa_fst_first_frames + a min over the arcs that emit
 * it), the pdfs a given frame range needs form a PREFIX of every class, which is what mfa_gmm_score_batch's
 * d_pdf_first_frame argument relies on. */
MFA_API int mfa_gmm_sort_pdf_list_keyed(mfa_ctx *ctx, int32_t *h_pdfs, int32_t *h_first_frame, int32_t n,
                                        int32_t *h_class_counts);
/* Host helper: h_depth[s] = the smallest number of arcs on a path from `start` to state s of an epsilon-free graph in
 * CSR form (arc_off[n_states+1], arc_next[n_arcs]); INT32_MAX for unreachable states.  A decoder token can sit on s at
 * frame t only if h_depth[s] <= t (FasterDecoder consumes one frame per arc; kaldi decoder/faster-decoder.cc
 * ProcessEmitting), so an arc leaving s is never scored before frame h_depth[s]. */
MFA_API int mfa_fst_first_frames(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next, int32_t start,
                                 int32_t *h_depth);

/* ---- Acoustic scoring: replaces DecodableAmDiagGmmScaled::LogLikelihood inside GmmAligner.align_utterance and
 *      gmm_compute_likes (MFA/alignment/multiprocessing.py:846-853, :1415).
 * Per utterance u: pdf list d_pdf_list[pdf_off[u]..pdf_off[u+1]) (sorted as above) with d_class_counts[u][6];
 * output d_loglikes + ll_off[u]: float32 [T_u][P_u] row-major (UNSCALED log-likelihoods).
 * A list is a list of score COLUMNS: it may hold a pdf more than once (mfa_build_score_plan gives a pdf that recurs in a
 * transcript one column per cluster of occurrences), so P_u may exceed the model's number of pdfs; every entry gets its
 * column, on every kernel. */
/* d_pdf_first_frame (may be NULL): int32 parallel to d_pdf_list, ascending inside every class of every utterance
 * (mfa_gmm_sort_pdf_list_keyed).  When given, cell (t, j) is only guaranteed to be written if
 * d_pdf_first_frame[j] <= t rounded up to the end of its 64-frame tile: Kaldi's decodable is evaluated lazily, for the
 * arcs leaving live tokens only, and no token can ask for pdf j before that frame — the skipped cells are never read by
 * mfa_align_batch.  NULL scores every cell (what gmm_compute_likes-style callers want). */
/* Numerics: single-Gaussian pdfs are scored on the float32 matrix pipe as one k-ordered fmaf chain (bit-identical to the
 * oracle's chain, bit-exact end to end).  Pdfs of 2 or more Gaussians go, by default, through the 16-bit matrix pipe with
 * every float32 product formed from split operands (accumulation order differs from the chain):
 *   - two f16 pieces per operand, power-of-two column scales fixed at mfa_load_gmm (3 * 2^-22 per term worst case;
 *     measured <= 1e-6 x max|score of the frame|); a 256-frame tile whose scaled features leave the f16 range is scored
 *     with three bf16 pieces instead.  MFA_GMM_F16=0: bf16 for all.
 *   - pdfs of more than 32 Gaussians are runs of 32-row blocks merged with an online log-sum-exp (same operand splits).
 * Both against a tolerance of 1e-3 on log-likelihoods.  Environment MFA_GMM_BF16=0 keeps every pdf on the float32 pipe. */
MFA_API int mfa_gmm_score_batch(mfa_ctx *ctx, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt,
                                int32_t max_frames, const int32_t *d_pdf_list, const int64_t *d_pdf_off,
                                const int32_t *d_class_counts, const int32_t *d_pdf_first_frame, const int64_t *d_ll_off,
                                float *d_loglikes);

/* Debug/profiling aid: when d_trace is non-NULL the scoring kernel records, for every (utterance u, 64-frame sub-tile r)
 * it scores, four uint64 words {start, end (100 MHz wall clock), hardware id (HW_ID | XCC_ID << 32), 32-row blocks
 * walked} at d_trace[((u * tiles) * 4 + r) * 4], tiles = ceil(max_frames / 256).  NULL turns it off. */
MFA_API int mfa_debug_gmm_trace(mfa_ctx *ctx, void *d_trace);
/* Test aid, no context and no device: packs a model as mfa_load_gmm does and copies out what it would upload.  h_info[13] =
 * {kpad, rows, blocks, split tables present, has_slot_class[5] (32, 16, 8, 4, 1 rows), has_single32, has_multi_block,
 * max_nblk, all_pdfs_32row}; *h_acc_scale = S.  Every array pointer may be NULL (call once for the sizes): h_row0
 * [num_pdfs + 1], h_nblk / h_slot [num_pdfs], h_w [blocks * 32 * kpad], h_gc / h_gch [blocks * 32], h_wb [blocks * 32 *
 * kpad * 3] bf16 bits, h_wh [blocks * 32 * kpad * 2] f16 bits, h_fscale [kpad]; h_wb, h_wh and h_gch are written only when
 * the split tables are present (kpad 80 or 96).  h_sort_pdfs[n_sort] (may be NULL) is sorted in place as by
 * mfa_gmm_sort_pdf_list_keyed with the keys h_sort_keys[n_sort] — or, h_sort_keys NULL, as by mfa_gmm_sort_pdf_list — and
 * h_sort_counts[6] receives the class counts.  Returns 0, -1 for a model without pdfs or with an empty pdf, -2 for a pdf id
 * out of range in h_sort_pdfs. */
MFA_API int mfa_debug_gmm_pack(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                               const float *h_means_invvars, const float *h_inv_vars, int32_t *h_info, float *h_acc_scale,
                               int32_t *h_row0, int32_t *h_nblk, int32_t *h_slot, float *h_w, float *h_gc, uint16_t *h_wb,
                               uint16_t *h_wh, float *h_gch, float *h_fscale, int32_t *h_sort_pdfs, int32_t *h_sort_keys,
                               int32_t n_sort, int32_t *h_sort_counts);
/* Profiling aid, effective only in a library built with -DVIT_STAMPS (tools/viterbi_phases.py): the first-beam decoder
 * launch leaves, per utterance, twelve uint64 shader-clock totals (one per phase of its frame loop) at d_stamps[u * 12]. */
MFA_API int mfa_debug_viterbi_stamps(mfa_ctx *ctx, void *d_stamps);

/* ---- Alignment: replaces GmmAligner.align_utterance(fst, feats) / .export_alignments
 *      (MFA/alignment/multiprocessing.py:846-853, :1311-1315; MFA/online/alignment.py:107) = Kaldi AddTransitionProbs
 *      (done by the host on the arc weights) + AlignUtteranceWrapper + FasterDecoder (beam, min_active 20,
 *      beam_delta 0.5, hash_ratio 2.0) with exactly Kaldi's pruning and tie-breaking order.
 * Graph u (epsilon-free, or with d_state_nemit: see mfa_graph_batch): states state_off[u]..state_off[u+1]; d_arc_off[global_state] .. [global_state+1] index the
 * arc arrays RELATIVE to arc_base[u]; start state d_start[u]; d_final[global_state] (+inf = non-final).
 * Arcs (SoA): d_arc_next (local state), d_arc_weight (graph cost incl. transition probs), d_arc_col (column of the
 * utterance's log-likelihood matrix = position of pdf(tid) in its pdf list), d_arc_ilabel (transition-id),
 * d_arc_olabel (word id). */
typedef struct {
  int32_t n_utt;
  const int64_t *d_state_off; /* [n_utt+1] */
  const int64_t *d_arc_base;  /* [n_utt+1] */
  const int32_t *d_start;     /* [n_utt] */
  const int32_t *d_arc_off;   /* [total_states + n_utt] : per utterance S_u+1 entries, at state_off[u]+u */
  const float *d_final;       /* [total_states] */
  const int32_t *d_arc_next;
  const float *d_arc_weight;
  const int32_t *d_arc_col;
  const int32_t *d_arc_ilabel;
  const int32_t *d_arc_olabel;
  /* Graphs with EPSILON INPUT ARCS (ilabel 0; training graphs compiled by kalpy / Kaldi can hold them) on the wavefront-
   * parallel decoder: NULL for epsilon-free batches; otherwise [total_states] = emitting arcs of every state, whose arcs
   * must then be stored [emitting arcs | epsilon arcs], each kind in its original relative order (FasterDecoder's
   * ProcessEmitting walks the emitting arcs of a state in order and skips the others, ProcessNonemitting the other way round:
   * the interleaving never matters).  d_arc_col of an epsilon arc is ignored.  Requirement (the host checks it and routes
   * anything else to mfa_align_general_batch): at most 64 emitting and at most 64 epsilon arcs per state.  The closure pops
   * its stack one token at a time exactly as Kaldi's does, so neither ties nor negative epsilon weights change its result. */
  const int32_t *d_state_nemit;
} mfa_graph_batch;

typedef struct {
  float beam;            /* 10 */
  float retry_beam;      /* 40; 0 = no retry */
  float acoustic_scale;  /* 0.1 */
  int32_t max_tokens;    /* live-token capacity per utterance (LDS-resident tables), e.g. 1024 */
  int32_t bp_tokens_per_frame; /* back-pointer capacity per utterance = T_u * this, e.g. 512 */
} mfa_align_opts;

/* d_utt_list: which utterances to decode (NULL = all n_utt); outputs (device):
 *   d_ali [total_frames] transition-ids (at frame_off), d_words [total_frames] word ids packed at frame_off[u] with
 *   d_n_words[u] valid entries, d_like[u] = -(graph+acoustic cost)/acoustic_scale, d_frame_like [total_frames] or NULL,
 *   d_status[u]: 0 ok, 1 ok after retry, 2 no final token (failed), 3 token-capacity overflow, 4 back-pointer overflow,
 *                5 unsupported graph (a state with more than 64 arcs), 6 internal consistency check failed,
 *                7 the best path carries more word labels than the utterance has frames — possible only when epsilon input arcs
 *                  carry output labels; d_words holds one entry per frame, so the word sequence cannot be returned (the utterance's
 *                  other outputs are undefined).  Graphs compiled from a lexicon never do this: every word consumes a frame.
 * total_frames = frame_off[n_utt], total_arcs = arc_base[n_utt] (host copies, so the call never synchronises); max_states / max_arcs = largest S_u / A_u
 * in the batch (they bound the token and candidate tables). */
MFA_API int mfa_align_batch(mfa_ctx *ctx, const mfa_graph_batch *graphs, const float *d_loglikes, const int64_t *d_ll_off,
                            const int32_t *d_ll_cols, const int64_t *d_frame_off, int64_t total_frames,
                            int64_t total_arcs, int32_t max_states, int32_t max_arcs, const mfa_align_opts *opts, int32_t *d_ali, int32_t *d_words, int32_t *d_n_words,
                            float *d_like, float *d_frame_like, int32_t *d_status);
/* ---- The same alignment for graphs the wavefront-parallel decoder does not take: EPSILON INPUT ARCS (ilabel 0; training
 * graphs compiled by kalpy / Kaldi can hold them — FstArchive handed to export_alignments,
 * MFA/alignment/multiprocessing.py:846-853) and states with more than 64 arcs.  FasterDecoder exactly as Kaldi runs it,
 * ProcessNonemitting included (LIFO queue, hash-list insertion order), one GPU thread per utterance with every structure in a
 * per-utterance HBM workspace: a correctness path (tens of milliseconds per 10 s utterance, thousands in parallel), results
 * bit-identical to the oracle's.  Graph layout as for mfa_align_batch; d_arc_col of an epsilon arc is ignored.
 * h_frame_off: host copy of d_frame_off (workspace sizing without a synchronisation on device data). */
MFA_API int mfa_align_general_batch(mfa_ctx *ctx, const mfa_graph_batch *graphs, const float *d_loglikes,
                                    const int64_t *d_ll_off, const int32_t *d_ll_cols, const int64_t *d_frame_off,
                                    const int64_t *h_frame_off, int32_t max_states, int32_t max_arcs,
                                    const mfa_align_opts *opts, int32_t *d_ali, int32_t *d_words, int32_t *d_n_words,
                                    float *d_like, float *d_frame_like, int32_t *d_status);
/* Bytes of device workspace mfa_align_batch will hold for a batch shape (so callers can budget HBM). */
MFA_API size_t mfa_align_workspace_bytes(mfa_ctx *ctx, int32_t n_utt, int64_t total_frames, const mfa_align_opts *opts);
/* Host query, no device work: the launches mfa_align_batch (lazy = 0) or mfa_align_features_batch (lazy = 1) makes for a
 * batch whose largest graph has max_states states and max_arcs arcs, eps != 0 when a graph of the batch has epsilon input
 * arcs — the same plan the decoder itself consumes (csrc/viterbi_plan.hpp).  One row of seven int32 per launch, in launch
 * order, into h_out (room for `cap` rows; further rows are not written):
 *   {pass (0 beam, 1 retry beam), code (0: every utterance; -2: those the first tier gave up; -1: those still pending),
 *    N (live-token capacity), C (candidate capacity), dynamic LDS bytes, token lists in LDS (1) or in HBM (0),
 *    log2 of the hashed state-to-slot table's size (0: one entry per graph state)}.
 * N below the capacity asked for means that the tables did not fit in 160 KiB and the capacity was halved until they did:
 * a token overflow (status 3) is then possible even with one token per graph state.  With lazy = 1 the first of two pass-0
 * launches is the small first-tier kernel, whose LDS layout is its own; its row holds the general kernel's figures.
 * Returns the number of launches, -1 if the decoder would refuse the batch (tables beyond 160 KiB at 64 tokens), -2 for
 * bad arguments. */
MFA_API int mfa_debug_viterbi_plan(const mfa_align_opts *opts, int32_t max_states, int32_t max_arcs, int32_t eps, int32_t lazy,
                                   int32_t *h_out, int32_t cap);

/* ---- Alignment from features, acoustic scores evaluated LAZILY: the same replacement as mfa_align_batch, but it takes the
 *      features GmmAligner.align_utterance(fst, feats) takes (MFA/alignment/multiprocessing.py:846-853;
 *      MFA/online/alignment.py:107) and scores only what Kaldi's lazy decodable would be asked for — a superset of it:
 *      the utterance is decoded in windows of `window` frames; before a window is decoded, the pdfs that arcs within
 *      `window` arcs of the live tokens can emit are scored for the window's frames (split-operand MFMA kernels as in
 *      mfa_gmm_score_batch); everything else in the score matrix is left untouched and never read.  Results are those of
 *      mfa_gmm_score_batch + mfa_align_batch bit for bit (same kernels' arithmetic per cell, same decoder).
 * plan: the utterances' pdf lists as for mfa_gmm_score_batch plus two depth keys per pdf and per graph state
 *   d_pdf_first_frame[j] = smallest BFS depth of a source state of the column's arcs
 *   d_pdf_last_depth[j]  = running max, inside the column's class in list order, of the largest such depth
 *   d_state_depth[global state][2] = {BFS depth, smallest BFS depth reachable from the state}
 * — all three come out of mfa_build_score_plan (one call per utterance).
 * d_loglikes [sum T_u * P_u] is caller-provided scratch for the scores (d_ll_off, d_ll_cols as for mfa_align_batch). */
typedef struct {
  const int32_t *d_pdf_list;
  const int64_t *d_pdf_off;
  const int32_t *d_class_counts;
  const int32_t *d_pdf_first_frame;
  const int32_t *d_pdf_last_depth;
  const int32_t *d_state_depth;
  int32_t max_cols;                 /* largest column count of an utterance of the batch (host value) */
  int32_t groups;                   /* 0 or 1: class 0 in one run ordered by first depth; G > 1 (mfa_build_score_plan_grouped):
                                       G runs (pdf id mod G), each ordered by first depth */
  const int32_t *d_group_counts;    /* [n_utt][groups] class-0 columns per run (NULL when groups <= 1) */
} mfa_score_plan;

MFA_API int mfa_align_features_batch(mfa_ctx *ctx, const mfa_graph_batch *graphs, const mfa_score_plan *plan,
                                     const float *d_feats, const int64_t *d_frame_off, int32_t max_frames,
                                     int64_t total_frames, int64_t total_arcs, int32_t max_states, int32_t max_arcs,
                                     const mfa_align_opts *opts, int32_t window, float *d_loglikes, const int64_t *d_ll_off,
                                     const int32_t *d_ll_cols, int32_t *d_ali, int32_t *d_words, int32_t *d_n_words,
                                     float *d_like, float *d_frame_like, int32_t *d_status);
/* Host helper: h_depth[s] = the smallest BFS depth (h_bfs_depth, from mfa_fst_first_frames) among the states reachable
 * from s, s included — computed on the graph's condensation, so self-loops and the small cycles of an ergodic silence
 * topology are fine.  It never decreases along an arc, and it is <= the BFS depth of everything reachable from s: a state
 * whose BFS depth is below h_depth[l] of every live token l can never be visited again.  Returns 0 for a graph that is
 * acyclic apart from self-loops, 1 if larger components were contracted, <0 if malformed. */
MFA_API int mfa_fst_last_depths(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next, int32_t start,
                                const int32_t *h_bfs_depth, int32_t *h_depth);
/* Host helper: the score columns of ONE utterance's graph, in the order the scoring kernels require.
 * In: the graph in CSR form with the pdf id of every arc (h_arc_pdf = pdf of the arc's transition-id) and the slot class
 * of every pdf of the model, h_pdf_class[num_pdfs] in 0..5 = {32 rows single block, 32 rows multi-block, 16, 8, 4, 1}
 * (from mfa_gmm_slot and the pdf's Gaussian count).  Returns 0, -1 for a malformed graph, -2 for a pdf id out of range.
 * A column is a pdf restricted to a cluster of its occurrences: arcs emitting the pdf whose source states' BFS depths lie
 * within cluster_span of the cluster's first (cluster_span <= 0: one column per pdf).  The same phone in two words thus gets
 * two columns, and the lazy-scoring band — a range of graph depths — need not keep it alive in between.
 * Out: h_state_depth[n_states][2] = {BFS depth, mfa_fst_last_depths value}; h_arc_col[n_arcs] = column of every arc;
 * per column (capacity n_arcs each): h_col_pdf, h_col_first = smallest BFS depth of a source, h_col_last = running max
 * (inside the column's slot class, in list order) of the largest BFS depth of a source; h_class_counts[6]; *h_n_cols.
 * Band rule (mfa_align_features_batch): with lo = min over live tokens of h_state_depth[.][1] and hi = max over live
 * tokens of h_state_depth[.][0] + window - 1, the columns a window can ask for are, in every class, the index range
 * [count(h_col_last < lo), count(h_col_first <= hi)). */
MFA_API int mfa_build_score_plan(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next,
                                 const int32_t *h_arc_pdf, int32_t start, int32_t num_pdfs, const int32_t *h_pdf_class,
                                 int32_t cluster_span, int32_t *h_state_depth, int32_t *h_arc_col, int32_t *h_col_pdf,
                                 int32_t *h_col_first, int32_t *h_col_last, int32_t *h_class_counts, int32_t *h_n_cols);
/* The same with the class-0 columns (one 32-row model block per pdf — the bulk of a context-dependent model) laid out in
 * `groups` runs, run g holding the pdfs with id mod groups == g, each run in ascending first depth with its own running
 * max in h_col_last; h_group_counts[groups] = columns per run.  With groups = 8 the lazy scoring kernel gives run g of every
 * utterance to workgroups of one XCD, whose 4 MiB L2 then only ever sees an eighth of the model (MI355X: 8 XCDs; a
 * 5k-pdf model is 51 MB of operands, re-read from the Infinity Cache otherwise); with groups = 16 an XCD serves runs x and
 * x + 8 one after the other (first and second half of the launch).  The band rule holds per run.
 * groups = 1 is mfa_build_score_plan.  Returns -3 for groups outside 1..MFA_PLAN_MAX_GROUPS. */
#define MFA_PLAN_MAX_GROUPS 16
MFA_API int mfa_build_score_plan_grouped(int32_t n_states, const int32_t *h_arc_off, const int32_t *h_arc_next,
                                         const int32_t *h_arc_pdf, int32_t start, int32_t num_pdfs, const int32_t *h_pdf_class,
                                         int32_t cluster_span, int32_t groups, int32_t *h_state_depth, int32_t *h_arc_col,
                                         int32_t *h_col_pdf, int32_t *h_col_first, int32_t *h_col_last, int32_t *h_class_counts,
                                         int32_t *h_group_counts, int32_t *h_n_cols);

/* The score plans of a whole batch, utterances spread over n_threads host threads (the per-utterance call above costs more
 * in its Python caller than in itself once graphs arrive at 20 k per second).  Graphs concatenated as the device layout
 * has them: h_state_off / h_arc_base [n_utt + 1] prefix sums; utterance u's arc offsets (S_u + 1 values, relative to its
 * first arc) at h_arc_off[h_state_off[u] + u]; h_arc_next / h_arc_pdf [total arcs]; h_start [n_utt].  Outputs as above,
 * concatenated: h_state_depth [total states][2], h_arc_col [total arcs]; utterance u's columns at h_col_*[h_arc_base[u] ..
 * + h_n_cols[u]) (capacity = its arcs); h_class_counts [n_utt][6]; h_group_counts [n_utt][groups] (groups > 1);
 * h_n_cols [n_utt].  Returns 0, or the first failing utterance's code with its index in *h_bad_utt. */
MFA_API int mfa_build_score_plans_batch(int32_t n_utt, const int64_t *h_state_off, const int64_t *h_arc_base,
                                        const int32_t *h_arc_off, const int32_t *h_arc_next, const int32_t *h_arc_pdf,
                                        const int32_t *h_start, int32_t num_pdfs, const int32_t *h_pdf_class,
                                        int32_t cluster_span, int32_t groups, int32_t n_threads, int32_t *h_state_depth,
                                        int32_t *h_arc_col, int32_t *h_col_pdf, int32_t *h_col_first, int32_t *h_col_last,
                                        int32_t *h_class_counts, int32_t *h_group_counts, int32_t *h_n_cols,
                                        int32_t *h_bad_utt);

/* ---- fMLLR statistics: replaces the accumulation of CalcFmllrFunction / kalpy FmllrComputer
 *      (MFA/corpus/features.py:506-527; Kaldi FmllrDiagGmmAccs) between the two alignment passes
 *      (MFA/alignment/base.py:510-539).  d_feats [total_frames][dim]: the features the transform will be applied to;
 * d_ali_pdf [total_frames]: pdf-id of the first-pass alignment per frame (<0 = skip); d_weight [total_frames]: frame
 * weights (0 for silence frames: silence_weight 0.0, MFA/corpus/features.py:759-766).  Outputs per speaker, float64,
 * deterministic: d_beta[n_spk], d_K[n_spk][dim][dim+1], d_G[n_spk][dim][dim+1][dim+1].  The per-speaker solve
 * (Kaldi ComputeFmllrMatrixDiagGmmFull) is host-side: montreal_forced_aligner_amd/fmllr.py.
 * Limits (refused with a message, the context stays usable): dim <= 41 — a block of the speaker kernel holds the
 * (dim+1)^2 <= 7*256 entries of a G_d in registers — and at most 128 Gaussians in a pdf.  n_utt, n_spk or total_frames of
 * 0 is no error: nothing is written.  A speaker without a weighted frame gets beta, K and G exactly 0.  A speaker's sums
 * depend on its own utterances in d_spk_utt order only: never on the other speakers of the batch. */
MFA_API int mfa_fmllr_acc_batch(mfa_ctx *ctx, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt,
                                int64_t total_frames, const int32_t *d_ali_pdf, const float *d_weight,
                                const int32_t *d_spk_utt_off, const int32_t *d_spk_utt, int32_t n_spk, double *d_beta,
                                double *d_K, double *d_G);

/* The same from the alignment itself: d_ali [total_frames] transition-ids (0 = no alignment for the frame), d_tid2pdf /
 * d_tid_weight [n_tids] host-built tables (pdf of a transition-id; frame weight by its phone: silence_weight for silence
 * phones, 1 otherwise); d_pdf_scratch / d_weight_scratch [total_frames] caller scratch. */
MFA_API int mfa_fmllr_acc_ali_batch(mfa_ctx *ctx, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt,
                                    int64_t total_frames, const int32_t *d_ali, const int32_t *d_tid2pdf,
                                    const float *d_tid_weight, int32_t n_tids, int32_t *d_pdf_scratch, float *d_weight_scratch,
                                    const int32_t *d_spk_utt_off, const int32_t *d_spk_utt, int32_t n_spk, double *d_beta,
                                    double *d_K, double *d_G);
/* Two-model form of the same accumulation — what the reference runs whenever the acoustic model ships final.alimdl
 * (MFA/corpus/features.py:503-511: FmllrComputer(ali_model_path, model_path, ...); MFA/alignment/mixins.py:404-410):
 * the Gaussian posteriors come from the model loaded with mfa_load_gmm (the ALIGNMENT model, evaluated on the
 * speaker-independent features), the statistics are formed with the means and variances given here (the FINAL model;
 * Kaldi gmm-post-to-gpost + FmllrDiagGmmAccs::AccumulateFromPosteriors).  Both models must have the same number of
 * Gaussians in every pdf.  Stays in force until the next mfa_load_gmm, or until called with NULL arrays. */
MFA_API int mfa_fmllr_stats_model(mfa_ctx *ctx, int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets,
                                  const float *h_means_invvars, const float *h_inv_vars);

/* ---- GMM statistics: replaces the accumulation of AccStatsFunction / kalpy GmmStatsAccumulator.accumulate_stats
 *      (MFA/alignment/adapting.py, MFA/alignment/multiprocessing.py:40; Kaldi gmm-acc-stats-ali =
 *      AccumAmDiagGmm::AccumulateForGmm, restated here from the algorithm's description — Kaldi's source is not among this
 *      project's references: parity unpinned).  The E-step of `mfa adapt` and of every training stage.
 *
 * Arithmetic contract.  A frame t takes no part when its transition-id d_ali[t] is outside the table (< 0 or >= n_tids), is
 * 0, or has weight 0 (or names a pdf the loaded model does not have).  Otherwise p = d_tid2pdf[d_ali[t]],
 * w = d_tid_weight[d_ali[t]], and for every Gaussian g of pdf p, in model order:
 *   log-likelihood   ll_g: the float32 fmaf chain of the fMLLR statistics — from gconst_g, then means_invvars_g[k] * x[k]
 *                    over ascending k, then (-0.5f * inv_vars_g[k]) * (x[k] * x[k]) over ascending k;
 *   softmax          m = max ll, e_g = expf(ll_g - m), s = sum of e_g, gamma_g = e_g * (1 / s) * w, all float32; the frame's
 *                    log-likelihood is m + logf(s);
 *   sums (double, explicit fma)
 *                    occ[g] += gamma_g;  mean[g][k] = fma(gamma_g, x_k, mean[g][k]);
 *                    var[g][k] = fma(gamma_g, x_k * x_k, var[g][k]) with the square formed in double;
 *                    tot[0] = fma(w, loglike, tot[0]);  tot[1] += w;
 *   counts           tid_count[d_ali[t]] += 1 (int64).
 * The accumulators are indexed by MODEL Gaussian (pdf_offsets of mfa_load_gmm, not packed rows): d_occ [G], d_mean / d_var
 * [G][dim], d_tot [2], d_tid_count [n_tids] (may be NULL).  They are added to, never overwritten.
 * Order of the double sums on the device: the frames of a pdf in ascending frame index, cut into chunks of
 * mfa_gmm_acc_chunk_frames() consecutive frames of that pdf; a chunk is summed from zero in frame order, the chunks are
 * added in order onto the caller's value; tot sums the chunks' totals in (pdf, chunk) order.  The result is therefore a
 * function of the input alone: two calls on the same input give the same bits.  No floating-point atomics.
 * mfa_debug_gmm_acc_host is the same contract on host arrays, frames in ascending index, expf / logf from libm: the
 * log-likelihood bits are the device's by construction (both run csrc/gmm_acc_math.hpp); only expf / logf, the order in
 * which the e_g are added and the order of the double sums may differ.
 * Runs on the model loaded with mfa_load_gmm, asynchronously on the ctx stream.  Limits (refused with a message, the
 * context stays usable): no model loaded; a pdf of more than 128 Gaussians; dim > mfa_gmm_acc_max_dim() = 48 (a thread of
 * the sum kernel owns 3 of 48 columns); 2^31 frames or more in one call.  total_frames == 0 is no error and writes nothing. */
MFA_API int32_t mfa_gmm_acc_chunk_frames(void);
MFA_API int32_t mfa_gmm_acc_max_dim(void);
MFA_API int mfa_gmm_acc_batch(mfa_ctx *ctx, const float *d_feats, int64_t total_frames, const int32_t *d_ali,
                              const int32_t *d_tid2pdf, const float *d_tid_weight, int32_t n_tids, double *d_occ, double *d_mean,
                              double *d_var, double *d_tot, int64_t *d_tid_count);
/* Host twin, no context and no device.  The model as mfa_load_gmm takes it; h_feats [total_frames][dim]; per frame
 * h_pdf (< 0 or >= num_pdfs: the frame takes no part) and h_weight (0: no part); h_tid [total_frames] with n_tids (both
 * optional: NULL / 0) feed h_tid_count (may be NULL).  h_post (may be NULL): [total_frames][post_stride] receives every
 * frame's gamma (0 beyond the pdf's Gaussians and for frames that take no part); post_stride >= the largest pdf.
 * Returns 0, -1 for bad arguments or an empty pdf, -2 for a pdf of more than 128 Gaussians. */
MFA_API int mfa_debug_gmm_acc_host(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                                   const float *h_means_invvars, const float *h_inv_vars, const float *h_feats,
                                   int64_t total_frames, const int32_t *h_pdf, const float *h_weight, const int32_t *h_tid,
                                   int32_t n_tids, double *h_occ, double *h_mean, double *h_var, double *h_tot,
                                   int64_t *h_tid_count, float *h_post, int32_t post_stride);

/* GMM statistics from two feature matrices of the same frames: replaces Kaldi gmm-acc-stats-twofeats, which the reference's
 * SatTrainer.create_align_model runs to build final.alimdl (MFA/acoustic_modeling/sat.py: posteriors from the
 * speaker-adapted features, sufficient statistics from the unadapted ones; restated from its description as above).
 * The contract is mfa_gmm_acc_batch's, word for word, with two differences:
 *   the log-likelihood chain, the softmax, gamma_g and the frame's log-likelihood (so tot[0]) use row t of d_feats_post;
 *   the x_k of mean[g][k] = fma(gamma_g, x_k, mean[g][k]) and var[g][k] = fma(gamma_g, x_k * x_k, var[g][k]) are row t of
 *   d_feats_sum.
 * Both matrices are [total_frames][dim] of the loaded model's dim.  Frames that take no part, the ordering by pdf (the stable
 * sort), the chunks of mfa_gmm_acc_chunk_frames(), the chunk-order reduction, the absence of floating-point atomics, the
 * limits and refusals, total_frames == 0 and the four timing slots are mfa_gmm_acc_batch's; a NULL d_feats_sum with frames is
 * refused too.  A consequence: with d_feats_sum holding the values of d_feats_post the result has the bits of mfa_gmm_acc_batch on
 * that input. */
MFA_API int mfa_gmm_acc_twofeats_batch(mfa_ctx *ctx, const float *d_feats_post, const float *d_feats_sum, int64_t total_frames,
                                       const int32_t *d_ali, const int32_t *d_tid2pdf, const float *d_tid_weight, int32_t n_tids,
                                       double *d_occ, double *d_mean, double *d_var, double *d_tot, int64_t *d_tid_count);
/* Its host twin: mfa_debug_gmm_acc_host with h_feats_sum [total_frames][dim] after h_feats; the same loop, the x of the sums
 * from h_feats_sum.  Returns as mfa_debug_gmm_acc_host; -1 also for a NULL h_feats_sum with frames. */
MFA_API int mfa_debug_gmm_acc_twofeats_host(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                                            const float *h_means_invvars, const float *h_inv_vars, const float *h_feats,
                                            const float *h_feats_sum, int64_t total_frames, const int32_t *h_pdf,
                                            const float *h_weight, const int32_t *h_tid, int32_t n_tids, double *h_occ,
                                            double *h_mean, double *h_var, double *h_tot, int64_t *h_tid_count, float *h_post,
                                            int32_t post_stride);

/* ---- Equal alignment: replaces kalpy gmm_align_equal (MFA/acoustic_modeling/monophone.py:108; Kaldi align-equal =
 *      EqualAlign, restated here from its description — Kaldi's source is not among this project's references, and its
 *      random numbers are not reproducible here: parity unpinned by construction).  The first alignment of
 *      flat-start training: a random path through the utterance's graph with its T_u frames spread evenly over the path's
 *      self-loops.  No features, no model.
 *
 * Graphs: mfa_graph_batch as for mfa_align_batch; read are d_state_off, d_arc_base, d_start, d_arc_off, d_final,
 * d_arc_next and d_arc_ilabel, in the arc order they are stored in.  d_frame_off [n_utt + 1]; d_utt_key [n_utt]: one
 * uint32 per utterance, which the host derives from the utterance's position in the CORPUS, not in the batch.
 * Outputs: d_ali [total_frames] transition-ids at frame_off, d_status [n_utt]: 0 ok, 2 failed.
 *
 * Random numbers are counter-based.  With fmix(h): h ^= h >> 16; h *= 0x85EBCA6B; h ^= h >> 13; h *= 0xC2B2AE35;
 * h ^= h >> 16 (uint32 arithmetic), draw d of an utterance is
 *   u = fmix(fmix(fmix(seed ^ 0x9E3779B9) + key * 0x85EBCA6B + 0x165667B1) ^ (d * 0xC2B2AE35 + 0x27D4EB2F))
 * and picks among m candidates by multiply-high, (u * m) >> 32 in 64 bits.  No state is shared between utterances: an
 * utterance's result is the same bits alone, in any batch, at any position, on the device and in the host twin (both run
 * csrc/align_equal_math.hpp; everything is integer arithmetic).
 * One attempt: from the start state, while the state is not final (d_final = +inf), choose uniformly among its arcs that
 *   are not self-loops (next != state), in arc order; append the arc; count it if its ilabel != 0.  Stop at the FIRST final
 *   state.  The attempt fails as soon as the counted ilabels exceed T_u (they only grow: Kaldi's check made early, and it
 *   bounds the walk), when the steps exceed 2 (T_u + S_u) (epsilon cycles), or at a non-final state without a non-self-loop
 *   arc.  Up to 10 attempts, the draws numbered on across attempts; after that status 2 and the utterance's frames set to 0.
 *   A malformed graph (a start state, an arc range or a next state outside it) is status 2 as well.
 * Spreading: a path state is loopable when it has a self-loop arc with ilabel != 0; the first such arc in arc order is
 *   the loop's transition-id.  With extra = T_u - ilabels and L loopable path states (a state the path visits twice counts
 *   twice): L == 0 and extra > 0 is status 2; otherwise every loopable state gets extra / L loops, the first extra % L of
 *   them in path order one more.  Output per path state, in path order: its loops, then its outgoing path arc's ilabel if
 *   != 0; the last state's loops go last.  T_u == 0: ok iff the walk reaches a final state with 0 ilabels; nothing is written.
 * total_frames = frame_off[n_utt] with frame_off[0] = 0 and total_states = state_off[n_utt] - state_off[0] are host copies
 * (the call never synchronises): they size the path workspace, 2 (2 (total_frames + total_states) + n_utt) int32 laid over
 * the context's shared workspace; an utterance whose device offsets do not fit them fails (status 2) without a write.
 * Asynchronous on the ctx stream.  Refused with a message, the context usable afterwards: NULL graph arrays (or offsets,
 * keys, outputs) with n_utt > 0; 2^31 frames or more.  n_utt == 0 is no error. */
MFA_API int mfa_align_equal_batch(mfa_ctx *ctx, const mfa_graph_batch *graphs, const int64_t *d_frame_off, int64_t total_frames,
                                  int64_t total_states, const uint32_t *d_utt_key, uint32_t seed, int32_t *d_ali,
                                  int32_t *d_status);
/* Host twin, no context and no device: the same contract on host arrays (the graph batch's arrays by name).  Returns 0,
 * -1 for bad arguments (a NULL array that would be read or written), -2 for 2^31 frames or more. */
MFA_API int mfa_debug_align_equal_host(int32_t n_utt, const int64_t *h_state_off, const int64_t *h_arc_base,
                                       const int32_t *h_start, const int32_t *h_arc_off, const float *h_final,
                                       const int32_t *h_arc_next, const int32_t *h_arc_ilabel, const int64_t *h_frame_off,
                                       const uint32_t *h_utt_key, uint32_t seed, int32_t *h_ali, int32_t *h_status);

/* ---- LDA statistics: replaces the accumulation of LdaAccStatsFunction / kalpy LdaStatsAccumulator.accumulate_stats
 *      (MFA/acoustic_modeling/lda.py:54-119; Kaldi acc-lda = LdaEstimate::Accumulate with weight-silence-post and
 *      RandPrune, restated here from the algorithm's description — Kaldi's source is not among this project's references,
 *      and its random numbers are not reproducible here: parity unpinned).  Class-labelled scatter sums in the
 *      SPLICED feature space, S = (2 * splice_ctx + 1) * dim; the spliced matrix is never materialised.
 *
 * Inputs.  d_mfcc [total_frames][dim], d_frame_off [n_utt + 1], d_utt2spk [n_utt], d_cmvn float64 [n_spk][2][dim + 1] (may
 * be NULL: no CMVN; the caller vouches for n_spk) and splice_ctx are what mfa_feats_batch mode 1 takes; total_frames =
 * frame_off[n_utt] is the host's copy (the call never synchronises).  d_ali [total_frames] transition-ids, d_tid2class /
 * d_tid_weight [n_tids], n_classes = C.  rand_prune (0: off), d_utt_key [n_utt] (uint32, from the utterance's position in
 * the CORPUS; may be NULL when rand_prune == 0), seed.
 * Accumulators, float64, added to and never overwritten: d_zero [C], d_first [C][S], d_second [S][S] (the full square, both
 * triangles written and bit-equal; the caller's value is read from the lower triangle), optional int64 d_tid_count [n_tids].
 *
 * Arithmetic contract.
 *   spliced vector   x_t of frame t of utterance u is what mfa_feats_batch mode 1 multiplies by the LDA matrix: for o in
 *                    -ctx..ctx the CMVN-applied row of frame clamp(t + o, first, last of u); a column is
 *                    x - (float)(sum / count) in float32 (pitch columns are zero-padded in the statistics and stay
 *                    untouched); offsets ascend, columns within an offset.
 *   taking part      a frame takes no part when its transition-id is outside the table or 0, its weight is 0, or its class
 *                    is outside [0, C).  Otherwise c = tid2class[ali[t]], w = tid_weight[ali[t]].
 *   random prune     with rand_prune = theta > 0 and |w| < theta: r = |w| / theta (float32), u = draw (t - first frame of
 *                    the utterance) of the utterance's stream — the fmix construction of the equal alignment above, keyed
 *                    by seed and d_utt_key[utt]; if (float)(u >> 8) * 2^-24 < r then w = copysign(theta, w), otherwise the
 *                    frame takes no part.  Kaldi's RandPrune on a generator whose draws are a function of (seed, corpus
 *                    position, frame): the kept set does not depend on how batches are cut.
 *   sums (double)    zero[c] += w;  first[c][i] = fma(w, x_i, first[c][i]);  second[i][j] += (w * x_i) * x_j, where the
 *                    product (double)w * (double)x_i is exact and the second product and the addition are rounded once (an
 *                    fma on the f64 matrix pipe: the device) or twice (multiply, add: the host twin);
 *   counts           tid_count[ali[t]] += 1 for the frames that take part.
 * Order on the device.  second: the batch's frames in slabs of mfa_lda_acc_slab_frames() consecutive frames; a slab is
 * summed from zero (4 frames per step of the matrix instruction, in frame order), the slabs are added in order onto the
 * caller's value.  zero / first: the frames of a class in ascending frame index (stable sort by class), cut into chunks of
 * mfa_lda_acc_chunk_frames() entries; a chunk is summed from zero in frame order, the chunks are added in order onto the
 * caller's value.  The result is a function of the input alone: two calls give the same bits.  No floating-point atomics.
 * mfa_debug_lda_acc_host is the same contract on host arrays, frames in ascending index: spliced vectors, weights and
 * prune decisions have the device's bits by construction (both run csrc/lda_acc_math.hpp); only the order of the double
 * sums and the rounding of a second-moment term may differ.
 * Asynchronous on the ctx stream.  Limits (refused with a message, the context stays usable): S > mfa_lda_acc_max_dim() =
 * 128; dim <= 0 or splice_ctx < 0; n_classes <= 0; a NULL array that would be read or written (CMVN without utt2spk,
 * pruning without keys among them); 2^31 frames or more.  total_frames == 0 is no error and writes nothing. */
MFA_API int32_t mfa_lda_acc_slab_frames(void);
MFA_API int32_t mfa_lda_acc_chunk_frames(void);
MFA_API int32_t mfa_lda_acc_max_dim(void);
MFA_API int mfa_lda_acc_batch(mfa_ctx *ctx, const float *d_mfcc, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames,
                              int32_t dim, const int32_t *d_utt2spk, const double *d_cmvn, int32_t splice_ctx,
                              const int32_t *d_ali, const int32_t *d_tid2class, const float *d_tid_weight, int32_t n_tids,
                              int32_t n_classes, float rand_prune, const uint32_t *d_utt_key, uint32_t seed, double *d_zero,
                              double *d_first, double *d_second, int64_t *d_tid_count);
/* Host twin, no context and no device: the same contract on host arrays (total_frames is h_frame_off[n_utt]).  Returns 0,
 * -1 for bad arguments (a NULL array that would be read or written, offsets that do not ascend), -2 for S > 128, -3 for
 * 2^31 frames or more. */
MFA_API int mfa_debug_lda_acc_host(const float *h_mfcc, const int64_t *h_frame_off, int32_t n_utt, int32_t dim,
                                   const int32_t *h_utt2spk, const double *h_cmvn, int32_t splice_ctx, const int32_t *h_ali,
                                   const int32_t *h_tid2class, const float *h_tid_weight, int32_t n_tids, int32_t n_classes,
                                   float rand_prune, const uint32_t *h_utt_key, uint32_t seed, double *h_zero, double *h_first,
                                   double *h_second, int64_t *h_tid_count);

/* ---- MLLT statistics: replaces the accumulation of MlltAccStatsFunction / kalpy MlltStatsAccumulator.accumulate_stats
 *      (MFA/acoustic_modeling/lda.py:122-180; Kaldi gmm-acc-mllt = MlltAccs::AccumulateFromPosteriors, restated here from
 *      the algorithm's description — Kaldi's source is not among this project's references: parity unpinned).
 *      Kaldi keeps, per output dimension j, G_j = sum over (t, g) of gamma_tg * inv_var_g[j] * d_tg d_tg^T with
 *      d = x - mean_g.  The same G_j is sum over g of inv_var_g[j] * F_g with the per-Gaussian full second moment
 *      F_g = sum over t of gamma_tg d_tg d_tg^T: this call forms occ and F_g, the contraction is the host's (mllt.py).
 *
 * Arithmetic contract.  A frame takes part, and gets its weight w, by the GMM statistics' rule (above).  The posteriors
 * gamma_g of the frame's pdf are the GMM statistics' bits: the same float32 chain and the same softmax
 * (csrc/gmm_acc_math.hpp, shared and not restated).  d_means float32 [G][dim], model Gaussian order, comes from the caller
 * (means_invvars / inv_vars, formed once in float32 and handed to the device and to the twin alike).  For every Gaussian g
 * of the pdf, in model order:
 *   d_k = x_k - means[g][k]                         float32, one rounding;
 *   occ[g] += gamma_g                               double;
 *   full[g][i][j] = fma((double)gamma_g * (double)d_i, (double)d_j, full[g][i][j])   for j <= i; the first product is
 *                                                   exact in double (24 + 24 bits);
 *   the upper triangle of full[g] is a copy of the lower (the caller's value is read from the lower triangle);
 *   tot[0] = fma(w, loglike, tot[0]);  tot[1] += w  as in the GMM statistics.
 * Accumulators, float64, indexed by MODEL Gaussian: d_occ [G], d_full [G][dim][dim], d_tot [2].  They are added to, never
 * overwritten; the Gaussians of a pdf without a frame keep the caller's bits, both triangles.
 * Order of the double sums on the device: the frames of a pdf in ascending frame index (the GMM statistics' ordering).  full:
 * cut into chunks of mfa_mllt_acc_chunk_frames() consecutive frames of that pdf; a chunk is summed from zero in frame order
 * (4 frames per step of the f64 matrix instruction), the chunks are added in order onto the caller's value.  occ and tot:
 * the same with chunks of mfa_gmm_acc_chunk_frames() — every chunk of full is a whole number of those —, so that occ and
 * tot are bit-equal to mfa_gmm_acc_batch's on the same input.  The result is a function of the input alone: two calls on
 * the same input give the same bits.  No floating-point atomics.
 * mfa_debug_mllt_acc_host is the same contract on host arrays, frames in ascending index, plain loops, expf / logf from
 * libm: only expf / logf, the order in which a frame's exponentials are added and the order of the double sums may differ.
 * Runs on the model loaded with mfa_load_gmm, asynchronously on the ctx stream; the partials lie in the context's shared
 * workspace: (frames / chunk + 1) * largest pdf + G rows of dim * (dim + 1) / 2 doubles at the most.  Limits (refused with
 * a message, the context stays usable): no model loaded; dim > mfa_mllt_acc_max_dim() = 48 (three 16-wide blocks of the
 * matrix tiles); a pdf of more than 128 Gaussians; 2^31 frames or more in one call; a NULL array.  total_frames == 0 is no
 * error and writes nothing. */
MFA_API int32_t mfa_mllt_acc_chunk_frames(void);
MFA_API int32_t mfa_mllt_acc_max_dim(void);
MFA_API int mfa_mllt_acc_batch(mfa_ctx *ctx, const float *d_feats, int64_t total_frames, const int32_t *d_ali,
                               const int32_t *d_tid2pdf, const float *d_tid_weight, int32_t n_tids, const float *d_means,
                               double *d_occ, double *d_full, double *d_tot);
/* Host twin, no context and no device.  The model as mfa_load_gmm takes it plus h_means [G][dim]; h_feats
 * [total_frames][dim]; per frame h_pdf (< 0 or >= num_pdfs: the frame takes no part) and h_weight (0: no part).  h_post
 * (may be NULL) as in mfa_debug_gmm_acc_host.  Returns 0, -1 for bad arguments or an empty pdf, -2 for a pdf of more than
 * 128 Gaussians, -3 for dim > 48. */
MFA_API int mfa_debug_mllt_acc_host(int32_t dim, int32_t num_pdfs, const int32_t *h_pdf_offsets, const float *h_gconsts,
                                    const float *h_means_invvars, const float *h_inv_vars, const float *h_means,
                                    const float *h_feats, int64_t total_frames, const int32_t *h_pdf, const float *h_weight,
                                    double *h_occ, double *h_full, double *h_tot, float *h_post, int32_t post_stride);

/* ---- Tree statistics: replaces the accumulation of TreeStatsFunction / kalpy TreeStatsAccumulator.accumulate_stats
 *      (MFA/acoustic_modeling/triphone.py; Kaldi acc-tree-stats, restated here from the algorithm's description — Kaldi's
 *      source is not among this project's references: parity unpinned).  Per event (left phone, centre phone,
 *      right phone, pdf-class) a count, the sum and the sum of squares of the features.  Context width 3, central position 1.
 *
 * Inputs.  d_feats float32 [total_frames][dim], the stage's final features; d_frame_off int64 [n_utt + 1]; total_frames =
 * frame_off[n_utt] is the host's copy (the call never synchronises).  d_ali [total_frames] transition-ids.  Per
 * transition-id, int32 [n_tids] each: d_tid_phone, d_tid_class (the pdf-class of the arc: the state's self-loop pdf-class for
 * a self-loop, its forward pdf-class otherwise), d_tid_flags (bit 0: the arc is final, it enters the topology entry's final
 * state; bit 1: the arc is a self-loop).  d_phone_ci uint8 [n_phones + 1]: 1 marks a context-independent phone.
 *
 * Taking part.  The alignments are those of this project's graphs, which put a state's self-loops AFTER its forward arc
 * (Kaldi's reorder option; SplitToPhones with reordered = true): a segment is a maximal run of frames that ends at a final
 * transition-id and the self-loops that follow it directly.  An utterance takes part only if every transition-id is in
 * (0, n_tids) with a phone in [1, n_phones] and a pdf-class in [0, 256), its last frame ends a segment, and no frame's phone
 * differs from the phone of the first frame of its segment.  Otherwise none of its frames take part and it is counted in
 * d_skipped.  An utterance of 0 frames is counted nowhere.
 * Event key of frame t in a segment of phone c: l = the previous segment's phone (0 at the utterance's start), r = the next
 * segment's (0 at its end), l = r = 0 if d_phone_ci[c], pc = tid_class[ali[t]];
 *   key = l << 48 | c << 28 | r << 8 | pc   (uint64; all ones for a frame that takes no part).
 * The left phone has 16 bits of the key: n_phones of 2^16 or more is refused.
 *
 * Outputs, fresh per call (never added to).  d_frame_event int32 [total_frames]: the frame's row in the event list, or -1.
 * d_n_events int64 [1]: always the true number of distinct keys.  d_skipped int64 [1].  For e < n_events, only if n_events <=
 * cap: d_ev_key [e] (ascending), d_ev_count int64 [e], d_ev_sum / d_ev_sumsq float64 [e][dim].  If n_events > cap no event
 * row is written: the host repeats the call with cap >= n_events (cap 0: the event arrays may be NULL).
 *
 * Arithmetic.  sum[k] += (double)x_k;  sumsq[k] += (double)x_k * (double)x_k — the product is exact in double, each step
 * rounds once.  Order: the frames of an event in ascending frame index (stable sort by key), cut into chunks of
 * mfa_tree_acc_chunk_frames(); a chunk is summed from zero in frame order, the chunks are added in order.  The result is a
 * function of the input alone: two calls give the same bits.  No floating-point atomics.
 * mfa_debug_tree_acc_host is the same contract on host arrays: keys, participation and event order are the device's by
 * construction (both run csrc/tree_acc_math.hpp); every event is one plain loop in ascending frame index, so only the order
 * of the double additions may differ.
 * Asynchronous on the ctx stream; scratch in the context's shared workspace (some 36 bytes a frame and the sort's own).  Limits (refused with a
 * message, the context stays usable): dim <= 0 or dim > mfa_tree_acc_max_dim() = 48 (the GMM statistics' limit: those run
 * next); n_phones >= 2^16; a NULL array that would be read or written; 2^31 frames or more.  total_frames == 0 is no
 * error: it writes n_events = 0 and skipped = 0. */
MFA_API int32_t mfa_tree_acc_chunk_frames(void);
MFA_API int32_t mfa_tree_acc_max_dim(void);
MFA_API int mfa_tree_acc_batch(mfa_ctx *ctx, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt, int64_t total_frames,
                               int32_t dim, const int32_t *d_ali, const int32_t *d_tid_phone, const int32_t *d_tid_class,
                               const int32_t *d_tid_flags, int32_t n_tids, const uint8_t *d_phone_ci, int32_t n_phones,
                               int64_t cap, int32_t *d_frame_event, int64_t *d_n_events, int64_t *d_skipped, uint64_t *d_ev_key,
                               int64_t *d_ev_count, double *d_ev_sum, double *d_ev_sumsq);
/* Host twin, no context and no device (total_frames is h_frame_off[n_utt]).  Returns 0, -1 for bad arguments (a NULL array
 * that would be read or written, offsets that do not ascend), -2 for dim > 48, -3 for 2^31 frames or more, -4 for n_phones
 * >= 2^16. */
MFA_API int mfa_debug_tree_acc_host(const float *h_feats, const int64_t *h_frame_off, int32_t n_utt, int32_t dim,
                                    const int32_t *h_ali, const int32_t *h_tid_phone, const int32_t *h_tid_class,
                                    const int32_t *h_tid_flags, int32_t n_tids, const uint8_t *h_phone_ci, int32_t n_phones,
                                    int64_t cap, int32_t *h_frame_event, int64_t *h_n_events, int64_t *h_skipped,
                                    uint64_t *h_ev_key, int64_t *h_ev_count, double *h_ev_sum, double *h_ev_sumsq);

/* ---- Diagonal UBM: replaces the per-job work of the reference's DubmTrainer (MFA/ivector/trainer.py:105-388,
 *      MFA/ivector/multiprocessing.py:64-140 and :233-280): Gaussian selection (Kaldi gmm-gselect =
 *      DiagGmm::GaussianSelection) and the global statistics over the selected Gaussians (gmm-global-acc-stats --gselect =
 *      AccumDiagGmm::AccumulateFromDiag), restated here from the algorithms' descriptions — Kaldi's source is not among this
 *      project's references: parity unpinned, DESIGN §2.
 * Both calls take the model — one mixture of G Gaussians — as device arrays with the call: d_gconsts [G], d_means_invvars
 * [G][dim], d_inv_vars [G][dim].  There is no context state and mfa_load_gmm is not involved.
 *
 * Gaussian selection.  Arithmetic contract.  For every frame t and every Gaussian g, ll_g is the GMM statistics' float32 fmaf
 * chain (above).  With n = min(num_gselect, G), d_gselect [total_frames][n] (int32) receives the n Gaussians of largest
 * ll, best first, in the order of (ll, index) pairs sorted descending: at equal ll the larger index comes first (how
 * Kaldi's sort of pairs is remembered: unpinned).  The order is that of the 64-bit keys of csrc/ubm_math.hpp (the
 * order-preserving image of the float's bits, then the index), which is total over every bit pattern: whatever the features
 * are, NaN and infinity included, a frame's indices are distinct and lie in [0, G), and nothing faults.  (The key tells
 * -0 from +0; a NaN sorts above +inf or below -inf by its sign bit.)  d_loglike [total_frames] (may be NULL) receives the
 * frame's log-sum-exp over the SELECTED Gaussians only: m + logf(s), m the best ll, s = sum of expf(ll - m), float32.
 * Order on the device: none that matters for d_gselect — the result is a function of the input alone; the expf(ll - m) of
 * d_loglike are added across a wavefront's lanes.  The [frames][G] log-likelihoods are never written to memory.
 * mfa_debug_ubm_gselect_host is the same contract on host arrays with libm's expf / logf: both run csrc/gmm_acc_math.hpp and
 * csrc/ubm_math.hpp, so the ll bits, and with them the indices and their order, are the device's by construction; only
 * d_loglike may differ (expf / logf themselves and the order in which the exponentials are added).
 * Limits (refused with a message, the context stays usable): dim <= 0 or dim > 48; G <= 0 or G > 2048 (32 rounds of lane =
 * Gaussian); num_gselect <= 0 or min(num_gselect, G) > 64 (a frame's list is one wavefront register); a NULL array that
 * would be read or written; 2^31 frames or more.  total_frames == 0 is no error and writes nothing.  Asynchronous on the ctx
 * stream; timing slot 25.  mfa_ubm_gselect_tile_frames(): the frames a workgroup of the selection stages at a time (tests cut
 * their batches around it). */
MFA_API int32_t mfa_ubm_gselect_tile_frames(void);
MFA_API int mfa_ubm_gselect_batch(mfa_ctx *ctx, const float *d_feats, int64_t total_frames, int32_t dim, int32_t G,
                                  const float *d_gconsts, const float *d_means_invvars, const float *d_inv_vars,
                                  int32_t num_gselect, int32_t *d_gselect, float *d_loglike);
/* Host twin.  Returns 0, -1 for bad arguments (dim <= 0, a NULL array that would be read or written), -2 for dim > 48, -3
 * for G outside [1, 2048], -4 for num_gselect <= 0 or min(num_gselect, G) > 64, -5 for 2^31 frames or more. */
MFA_API int mfa_debug_ubm_gselect_host(const float *h_feats, int64_t total_frames, int32_t dim, int32_t G,
                                       const float *h_gconsts, const float *h_means_invvars, const float *h_inv_vars,
                                       int32_t num_gselect, int32_t *h_gselect, float *h_loglike);

/* Global GMM statistics.  Arithmetic contract.  A frame's Gaussians: with d_gselect ([total_frames][n] int32) its n listed
 * indices, of which one outside [0, G) is skipped; with d_gselect NULL every Gaussian (n is ignored: the init phase's dense
 * E-step).  The frame's weight w is d_frame_weight[t], or 1 when that is NULL.  A frame with no valid index, or with weight
 * 0, takes no part.  Otherwise, over the frame's Gaussians, the GMM statistics' softmax operation for operation: ll_g (the
 * chain), m = max ll, e_g = expf(ll_g - m), s = sum of e_g, gamma_g = e_g * (1 / s) * w, the frame's log-likelihood
 * LL = m + logf(s), all float32; and the GMM statistics' sums (double, explicit fma):
 *   occ[g] += gamma_g;  mean[g][k] = fma(gamma_g, x_k, mean[g][k]);  var[g][k] = fma(gamma_g, x_k * x_k, var[g][k]) with
 *   the square formed in double;  tot[0] = fma(w, LL, tot[0]);  tot[1] += w.
 * d_occ [G], d_mean / d_var [G][dim], d_tot [2] are added to, never overwritten; a Gaussian that no frame selects keeps the
 * caller's bits.  d_post (may be NULL; only with a d_gselect): [total_frames][n] float receives gamma in the list's order, 0
 * for a skipped entry and for a frame that takes no part.  A list's indices are distinct, as the selection writes them; a
 * list that repeats an index is outside the contract (on the device one of the repeated entries counts; nothing faults).
 * Feature rows are finite; a value that is not enters the device's sums as 0 beside the NaN its gamma already is.
 * Order on the device: the batch's frames are cut into slabs of mfa_ubm_acc_slab_frames() consecutive frames; a slab is
 * summed from zero in frame order, 4 frames per step of the f64 matrix instruction (a Gaussian that a frame does not list
 * adds an exact zero there); the slabs are added in order onto the caller's value, tot likewise from the slabs' totals.  The
 * slabs run in passes sized to the context's workspace; the slab order makes the result independent of the passes.  The
 * result is a function of the input alone: two calls on the same input give the same bits.  No floating-point atomics.
 * mfa_debug_ubm_acc_host is the same contract on host arrays, frames in ascending index, a frame's Gaussians in list order,
 * expf / logf from libm: the ll bits are the device's by construction; only expf / logf, the order in which a frame's e_g
 * are added, and the order and rounding of the double sums may differ.
 * Limits (refused with a message, the context stays usable): those of the selection for dim, G and the frames; with a
 * non-NULL d_gselect n <= 0 or n > 64; d_post without d_gselect; a NULL array that would be read or written.
 * total_frames == 0 is no error and writes nothing.  Asynchronous on the ctx stream; timing slots 26-28. */
MFA_API int32_t mfa_ubm_acc_slab_frames(void);
MFA_API int mfa_ubm_acc_batch(mfa_ctx *ctx, const float *d_feats, int64_t total_frames, int32_t dim, int32_t G,
                              const float *d_gconsts, const float *d_means_invvars, const float *d_inv_vars, int32_t n,
                              const int32_t *d_gselect, const float *d_frame_weight, double *d_occ, double *d_mean, double *d_var,
                              double *d_tot, float *d_post);
/* Host twin.  Return codes as mfa_debug_ubm_gselect_host; -4 for n outside [1, 64] with a non-NULL h_gselect; -1 also for
 * h_post without h_gselect. */
MFA_API int mfa_debug_ubm_acc_host(const float *h_feats, int64_t total_frames, int32_t dim, int32_t G, const float *h_gconsts,
                                   const float *h_means_invvars, const float *h_inv_vars, int32_t n, const int32_t *h_gselect,
                                   const float *h_frame_weight, double *h_occ, double *h_mean, double *h_var, double *h_tot,
                                   float *h_post);

/* ---- I-vector extractor: replaces the per-job work of the reference's IvectorTrainer (MFA/ivector/trainer.py:390-632,
 *      MFA/ivector/multiprocessing.py:143-231 and :283-331) and of ExtractIvectorsFunction (MFA/corpus/features.py:956-1015):
 *      gauss-to-post's pruning, the utterance statistics and the E-step of Kaldi's ivector-extractor programs with
 *      use_weights = false, restated here from the algorithm's description — Kaldi's source is not among this project's
 *      references: parity unpinned, DESIGN §2.
 * Notation: G Gaussians, feature dimension D, i-vector dimension R, P = R (R + 1) / 2.  A symmetric matrix is its packed
 * lower triangle, row-major: element (r, c), c <= r, at r (r + 1) / 2 + c.  The model comes with the call as device arrays
 * of double: W [G][D][R] (W_i = SigmaInv_i M_i), U [G][P] (U_i = M_i^T SigmaInv_i M_i) and the scalar prior_offset.  There is
 * no context state.  All three calls are asynchronous on the ctx stream; no floating-point atomics anywhere: each result
 * is a function of the input alone, and two calls on the same input give the same bits.
 *
 * Posterior pruning.  Arithmetic contract (csrc/ivector_math.hpp, ivector_prune_frame), per frame of n float32 entries in
 * list order: an entry survives when it is >= min_post (a NaN never is); when none survives, the first of the largest
 * entries does, if it is positive; the survivors are summed in list order, s; a survivor becomes p / s * scale (two
 * roundings), every other entry 0.  A frame whose survivors do not sum to a positive number (all zeros: a frame that took no
 * part in the statistics that wrote it) becomes all zeros.  d_out may be d_post (in place).  The host twin runs the same
 * function: the bits are the device's by construction.  Limits: n outside [1, 64]; 2^31 frames or more; a NULL array.
 * total_frames == 0 is no error.  Timing slot 29. */
MFA_API int mfa_ivector_prune_post_batch(mfa_ctx *ctx, const float *d_post, int64_t total_frames, int32_t n, float min_post,
                                         float scale, float *d_out);
/* Host twin.  Returns 0, -1 for a NULL array or a negative count, -4 for n outside [1, 64], -5 for 2^31 frames or more. */
MFA_API int mfa_debug_ivector_prune_post_host(const float *h_post, int64_t total_frames, int32_t n, float min_post, float scale,
                                              float *h_out);

/* Utterance statistics.  d_frame_off [n_utt + 1] (int64, ascending from 0 to total_frames) cuts d_feats [total_frames][dim]
 * into utterances; d_gselect / d_post [total_frames][n] are a frame's Gaussians and their (pruned) posteriors: an index
 * outside [0, G) is skipped, a list's indices are distinct (one that repeats an index is outside the contract: on the
 * device one of the entries counts; nothing faults).  Arithmetic contract, in double, p the float posterior made double:
 *   gamma[u][g] = sum over the utterance's frames of p;  X[u][g][k] = sum of p * x_k;
 *   S[g][pk(j, k)] += sum over all frames of p * (x_j * x_k), the product of two floats formed in double (exact).
 * A feature value that is not finite enters the sums as 0.  d_gamma [n_utt][G] and d_X [n_utt][G][dim] are overwritten for
 * every utterance (one without frames gets zeros); d_S [G][dim (dim + 1) / 2] (may be NULL) is added to, never overwritten.
 * max_count > 0 (extraction): an utterance whose sum of gamma over the Gaussians exceeds it has gamma and X multiplied by
 * max_count / that sum; S is not scaled.  max_count <= 0: no scaling.
 * Order on the device: an utterance's frames in order, 4 per step of the f64 matrix instruction, from zero (a Gaussian that
 * a frame does not list adds an exact zero there).  S: the batch's frames cut into slabs of
 * mfa_ivector_scatter_slab_frames() frames, each summed from zero in frame order, the slabs added in order onto the
 * caller's value — frame order is utterance order; the slabs run in passes sized to the workspace (MFA_IVECTOR_PASS_SLABS
 * overrides, for tests), and the slab order makes the result independent of the passes.  Two calls that split a batch at a
 * multiple of the slab add to S what one call adds.  The sum of gamma for max_count: each of 256 threads its Gaussians
 * g = t, t + 256, ... ascending, then a binary tree.
 * mfa_debug_ivector_utt_stats_host is the same contract in plain loops, frames ascending, a frame's entries in list order,
 * separate multiply and add: only the order and the rounding of the double sums may differ.
 * Limits (refused with a message, the context stays usable): dim outside [1, 48]; G outside [1, 2048]; n outside [1, 64];
 * 2^31 frames or more; a NULL array that would be read or written.  n_utt == 0 is no error.  Timing slots 30 (gamma, X and
 * max_count) and 31 (S). */
MFA_API int32_t mfa_ivector_scatter_slab_frames(void);
MFA_API int mfa_ivector_utt_stats_batch(mfa_ctx *ctx, const float *d_feats, const int64_t *d_frame_off, int32_t n_utt,
                                        int64_t total_frames, int32_t dim, int32_t G, int32_t n, const int32_t *d_gselect,
                                        const float *d_post, double max_count, double *d_gamma, double *d_X, double *d_S);
/* Host twin; total_frames is h_frame_off[n_utt].  Returns 0, -1 for a NULL array, a negative count or offsets that do not
 * ascend from 0, -2 dim, -3 G, -4 n, -5 2^31 frames or more. */
MFA_API int mfa_debug_ivector_utt_stats_host(const float *h_feats, const int64_t *h_frame_off, int32_t n_utt, int32_t dim, int32_t G,
                                             int32_t n, const int32_t *h_gselect, const float *h_post, double max_count,
                                             double *h_gamma, double *h_X, double *h_S);

/* E-step.  Arithmetic contract, in double, per utterance u (gamma [n_utt][G], X [n_utt][G][dim] as the statistics write them):
 *   Q = I + sum_g gamma[g] U_g and lin = prior_offset e0 + sum_(g, k) X[g][k] W_g[k][.]: the prior term first, then g (and
 *   k within g) ascending;  Q = L L^T by Cholesky;  Var = Q^-1 = L^-T L^-1;  mu = L^-T (L^-1 lin);  Sc = Var + mu mu^T.
 * d_ivec_mean [n_utt][R] receives mu; d_ivec_var [n_utt][P] (may be NULL) Var; d_aux [n_utt][2] (may be NULL) the two
 * numbers of the objective that need the factorisation: lin . mu and log det Q.  The accumulators are all NULL (extraction)
 * or all set, and are added to, never overwritten: over the utterances that take part, in utterance order,
 *   Gamma[g] += gamma[g];  Y[g][k][r] += X[g][k] mu[r];  Rq[g][.] += gamma[g] Sc;  isum += mu;  iscat += Sc;  n[0] += 1.
 * An utterance takes part when some gamma is not zero and every element of mu is finite.  A Q that is not positive definite
 * cannot arise from gamma >= 0 and a valid U; a non-finite input gives NaN in that utterance's mu, Var and aux only, the
 * utterance takes no part, and nothing faults (no index depends on a value).
 * Order on the device: the utterances run in chunks sized to the context's workspace ([chunk][P] doubles;
 * MFA_IVECTOR_PASS_UTTS=<utterances> overrides, for tests), a chunk being a multiple of 4 utterances, the K of the f64 matrix
 * instruction (an override is rounded up to one).  Per chunk: Q and lin as products [chunk x G][G x P] and
 * [chunk x G dim][G dim x R] on the matrix instruction, k ascending, 4 per step; one workgroup per utterance holds the packed
 * triangle in LDS and runs the twin's operations (left-looking Cholesky, L^-1 in place by columns from the last, every
 * element's sum over k ascending in one thread); Rq and Y as products over the chunk's utterances whose accumulator starts
 * from the caller's value, 4 utterances per step; Gamma, isum, iscat and n one thread per element, utterances in order.
 * Chunks follow one another in utterance order and begin at multiples of 4, so every step holds the same four utterances
 * whatever the chunk size: the result does not depend on the chunking.
 * mfa_debug_ivector_estep_host is the same contract in plain loops, utterances ascending: only the order and rounding of
 * the products' sums (and log) may differ; given the same Q and lin, the factorisation's operations are the same.
 * Limits (refused with a message, the context stays usable): dim outside [1, 48]; G outside [1, 2048]; R outside [1, 192]
 * (the packed triangle, 148 224 B at 192, lives in one workgroup's LDS); some but not all accumulators; a NULL array that
 * would be read or written; 2^31 utterances or more.  n_utt == 0 is no error.  Timing slots 32 (Q, lin), 33 (the solve),
 * 34 (the accumulators). */
MFA_API int mfa_ivector_estep_batch(mfa_ctx *ctx, const double *d_gamma, const double *d_X, int32_t n_utt, int32_t dim, int32_t G,
                                    int32_t R, const double *d_W, const double *d_U, double prior_offset, double *d_ivec_mean,
                                    double *d_ivec_var, double *d_aux, double *d_Gamma, double *d_Y, double *d_Rq, double *d_isum,
                                    double *d_iscat, double *d_n);
/* Host twin.  Returns 0, -1 for a NULL array, a negative count or some but not all accumulators, -2 dim, -3 G, -5 2^31
 * utterances or more, -6 R outside [1, 192]. */
MFA_API int mfa_debug_ivector_estep_host(const double *h_gamma, const double *h_X, int32_t n_utt, int32_t dim, int32_t G, int32_t R,
                                         const double *h_W, const double *h_U, double prior_offset, double *h_ivec_mean,
                                         double *h_ivec_var, double *h_aux, double *h_Gamma, double *h_Y, double *h_Rq,
                                         double *h_isum, double *h_iscat, double *h_n);

/* ---- PLDA: what consumes an i-vector in the reference — the transform of IvectorCorpusMixin.transform_ivectors and
 *      collect_speaker_ivectors (MFA/corpus/ivector_corpus.py:316-452), and the pairwise log-likelihood ratios behind
 *      PldaClassificationFunction, cluster_matrix and calculate_distance_threshold (MFA/diarization/multiprocessing.py), which
 *      the reference asks of Kaldi's Plda one pair at a time.  Restated here from the algorithm's description — Kaldi's source
 *      is not among this project's references: parity unpinned, DESIGN §2.
 * The model comes with the call as device arrays of double: transform [D][D], offset [D] (= -transform mean) and psi [D].
 * There is no context state.  No atomics anywhere: each result is a function of the input alone, and two calls on the same
 * input give the same bits.
 *
 * Transform.  Arithmetic contract, per row x of d_x [n][D]: u = transform x + offset, the accumulator starting from offset
 * and the products added k ascending, 4 per step of the f64 matrix instruction (D zero-padded to a multiple of 4: the
 * padding's +0 products can turn a -0 result into +0, nothing else); then the row is multiplied by its factor:
 *   norm 0: none;  norm 1 (simple): sqrt(D / sum_k u_k^2);  norm 2 (the model's): sqrt(D / sum_k u_k^2 / (psi_k + 1 / n_row)),
 * n_row = d_num_examples[row] (int32; NULL: 1).  Order on the device: the sum is one wavefront's — lane l adds its elements
 * k = l, l + 64, ... ascending, then the 64 sums meet in a butterfly (xor 32, 16, ... 1).  A row whose sum is 0 or not finite,
 * or whose n_row is below 1, gets what the formula gives (NaN or infinities); nothing faults.  d_out [n][D] may not be d_x.
 * mfa_debug_plda_transform_host is the same contract in plain loops, k ascending: only the order and rounding of the sums
 * may differ.  Limits (refused with a message, the context stays usable): D outside [1, 1024]; norm outside [0, 2]; 2^31
 * rows or more; a NULL array that would be read or written (d_psi only with norm 2).  n == 0 is no error.  Asynchronous on
 * the ctx stream; timing slot 35. */
MFA_API int mfa_plda_transform_batch(mfa_ctx *ctx, const double *d_x, int64_t n, int32_t D, const double *d_transform,
                                     const double *d_offset, const double *d_psi, const int32_t *d_num_examples, int32_t norm,
                                     double *d_out);
/* Host twin.  Returns 0, -1 for a NULL array, a negative count or a norm outside [0, 2], -2 for D outside [1, 1024], -5 for
 * 2^31 rows or more. */
MFA_API int mfa_debug_plda_transform_host(const double *h_x, int64_t n, int32_t D, const double *h_transform, const double *h_offset,
                                          const double *h_psi, const int32_t *h_num_examples, int32_t norm, double *h_out);

/* Scoring.  d_test [n_test][D] and d_train [n_train][D] are vectors in the model's space (the transform's output);
 * d_train_n [n_train] (int32; NULL: 1) the number of examples a train vector is the mean of.  Arithmetic contract, in double.
 * Per train column j and element k (csrc/plda_math.hpp), with g = train[j][k], n = train_n[j]:
 *   a = n psi_k / (n psi_k + 1);  v = 1 + psi_k / (n psi_k + 1);
 *   A_jk = -1/2 (1 / v - 1 / (1 + psi_k)), computed as -1/2 psi_k a / (v (1 + psi_k));  B_jk = (a g) / v;
 *   c_j = -1/2 (sum_k log v - sum_k log(1 + psi_k) + sum_k (a g)^2 / v), computed as 1/2 (sum_k log1p(psi_k a / v) -
 *   sum_k (a g)^2 / v), each sum over k ascending (the computed forms take no difference of nearly equal numbers);
 * and score[i][j] = c_j + sum_k p_ik^2 A_jk + sum_k p_ik B_jk, p = test: the log-likelihood ratio of "test i has train j's
 * class" against "it has a class of its own", expanded so that the whole matrix is one product with K = 2 D.  Order on the
 * device: the accumulator starts from c_j; k ascending, 4 per step of the f64 matrix instruction, D zero-padded to a multiple
 * of 4; per step first the four products (p p) A — the square is formed first, a separate rounding — then the four p B.
 * Three outputs, each optional (NULL: off), at least one required:
 *   (a) d_scores [n_test][n_train]: every score, the diagonal included whatever exclude_diagonal says;
 *   (b) d_best_idx [n_test] (int32) and d_best_score [n_test]: a row's best candidate; -1 and -inf when it has none;
 *   (c) d_knn_idx / d_knn_score [n_test][k], 1 <= k <= 64: a row's k best candidates, best first, padded with -1 and -inf.
 * A row's candidates are its columns whose score is finite (a NaN or an infinity is never selected), without column j == i
 * when exclude_diagonal is not 0 (test and train are the same vectors).  The order is one strict order: the larger score
 * first, at equal scores the lower index (+0 and -0 are equal).  (b) and (c) are taken from the very accumulator values that
 * (a) stores: they are exactly the first 1 and k of that order over the matrix row, whatever the tiling.  A NaN in test row i
 * stays in row i of the matrix, one in train column j in column j.
 * On the device a wavefront keeps a row's list across its whole sweep of the columns; for few rows and many columns the
 * columns are cut into passes (MFA_PLDA_PASS_COLS=<columns per pass> overrides, rounded up to a multiple of 64; for tests)
 * whose lists are merged in pass order.  The order being strict, the result does not depend on the passes.
 * mfa_debug_plda_score_host is the same contract in plain loops: A and B are the device's bits (basic operations only), c may
 * differ by log1p; the sums run k ascending in the device's step structure, so only what the matrix instruction does inside a
 * step may differ.  Given the same matrix the selections are the same.
 * Limits (refused with a message, the context stays usable): D outside [1, 1024]; k outside [1, 64] when (c) is asked for;
 * every output NULL, or an index output without its scores; a psi entry that is not positive and finite; a train_n below 1
 * (these two are found on the device by the prepare step, which the call waits for; without train vectors there is no
 * prepare step and psi is not looked at); 2^31 test or train vectors or more; a NULL array
 * that would be read.  n_test == 0 is no error and writes nothing; n_train == 0 writes the empty lists.  Timing slots 36
 * (prepare), 37 (sweep), 38 (merge). */
MFA_API int mfa_plda_score_batch(mfa_ctx *ctx, const double *d_test, int64_t n_test, const double *d_train, int64_t n_train,
                                 int32_t D, const int32_t *d_train_n, const double *d_psi, int32_t exclude_diagonal, int32_t k,
                                 double *d_scores, int32_t *d_best_idx, double *d_best_score, int32_t *d_knn_idx,
                                 double *d_knn_score);
/* Host twin.  Returns 0, -1 for a NULL array, a negative count or an index output without its scores, -2 D, -3 k, -4 a psi
 * entry that is not positive and finite, -5 2^31 vectors or more, -6 a train_n below 1, -7 every output NULL. */
MFA_API int mfa_debug_plda_score_host(const double *h_test, int64_t n_test, const double *h_train, int64_t n_train, int32_t D,
                                      const int32_t *h_train_n, const double *h_psi, int32_t exclude_diagonal, int32_t k,
                                      double *h_scores, int32_t *h_best_idx, double *h_best_score, int32_t *h_knn_idx,
                                      double *h_knn_score);
/* The prepare step alone, on the host: h_A, h_B [n_train][D] and h_c [n_train].  Return codes as the scoring twin's. */
MFA_API int mfa_debug_plda_prepare_host(const double *h_train, int64_t n_train, int32_t D, const int32_t *h_train_n, const double *h_psi,
                                        double *h_A, double *h_B, double *h_c);
/* The sweep alone over the caller's operands A, B [n_train][D] and c [n_train] (tests: operands chosen so that every product
 * and sum is exact), on the device and on the host: the scoring contract from "score[i][j] =" on, the same limits. */
MFA_API int mfa_debug_plda_sweep_batch(mfa_ctx *ctx, const double *d_test, int64_t n_test, int32_t D, const double *d_A,
                                       const double *d_B, const double *d_c, int64_t n_train, int32_t exclude_diagonal, int32_t k,
                                       double *d_scores, int32_t *d_best_idx, double *d_best_score, int32_t *d_knn_idx,
                                       double *d_knn_score);
MFA_API int mfa_debug_plda_sweep_host(const double *h_test, int64_t n_test, int32_t D, const double *h_A, const double *h_B,
                                      const double *h_c, int64_t n_train, int32_t exclude_diagonal, int32_t k, double *h_scores,
                                      int32_t *h_best_idx, double *h_best_score, int32_t *h_knn_idx, double *h_knn_score);

/* Neighbour bits: a fourth consumer of the same sweep, and the sweep for two more metrics.  What the reference's
 * cluster_matrix and calculate_distance_threshold (MFA/diarization/multiprocessing.py) need of the vectors of a corpus.
 *   (d) d_bits [n_test][W] (uint64), W = ceil(n_train / 64): bit j & 63 of word j >> 6 of row i is set iff score[i][j] >=
 *       threshold, a plain comparison on the very accumulator value that (a) stores: never for a NaN score; with threshold =
 *       -inf for every score that is not NaN.  Bits of columns >= n_train are 0.  Column passes own whole words, so nothing
 *       is merged and the words do not depend on MFA_PLDA_PASS_COLS.  Every word of every row is written.
 * metric chooses the prepare step (csrc/plda_math.hpp); the sweep's arithmetic and order are those of the scoring contract:
 *   0 plda: A, B, c as above (d_train_n, d_psi as above);
 *   1 euclidean: A_jk = -1, B_jk = 2 g, c_j = -sum_k g^2 (k ascending): score = -|p - g|^2 in its expanded form;
 *   2 dot: A_jk = 0, B_jk = g, c_j = 0: score = p . g (the cosine of rows the caller made unit length).
 * For metrics 1 and 2 d_train_n and d_psi are not looked at.  The outputs (a), (b), (c) are as in mfa_plda_score_batch, for any
 * metric; at least one of (a) to (d) is required; threshold is only looked at with (d).
 * Limits: those of mfa_plda_score_batch, and a metric outside [0, 2], a threshold that is NaN when (d) is asked for.  The
 * context stays usable.  n_test == 0 is no error and writes nothing.  Timing slots 36 to 38.
 * mfa_debug_neighbor_sweep_batch takes the caller's operands like mfa_debug_plda_sweep_batch; the _host functions are the same
 * contracts in plain loops (return codes as mfa_debug_plda_score_host, -8 an unknown metric, -9 a NaN threshold). */
MFA_API int mfa_neighbor_bits_batch(mfa_ctx *ctx, const double *d_test, int64_t n_test, const double *d_train, int64_t n_train,
                                    int32_t D, int32_t metric, const int32_t *d_train_n, const double *d_psi,
                                    int32_t exclude_diagonal, int32_t k, double threshold, double *d_scores, int32_t *d_best_idx,
                                    double *d_best_score, int32_t *d_knn_idx, double *d_knn_score, uint64_t *d_bits);
MFA_API int mfa_debug_neighbor_bits_host(const double *h_test, int64_t n_test, const double *h_train, int64_t n_train, int32_t D,
                                         int32_t metric, const int32_t *h_train_n, const double *h_psi, int32_t exclude_diagonal,
                                         int32_t k, double threshold, double *h_scores, int32_t *h_best_idx, double *h_best_score,
                                         int32_t *h_knn_idx, double *h_knn_score, uint64_t *h_bits);
MFA_API int mfa_debug_neighbor_sweep_batch(mfa_ctx *ctx, const double *d_test, int64_t n_test, int32_t D, const double *d_A,
                                           const double *d_B, const double *d_c, int64_t n_train, int32_t exclude_diagonal,
                                           int32_t k, double threshold, double *d_scores, int32_t *d_best_idx, double *d_best_score,
                                           int32_t *d_knn_idx, double *d_knn_score, uint64_t *d_bits);
MFA_API int mfa_debug_neighbor_sweep_host(const double *h_test, int64_t n_test, int32_t D, const double *h_A, const double *h_B,
                                          const double *h_c, int64_t n_train, int32_t exclude_diagonal, int32_t k, double threshold,
                                          double *h_scores, int32_t *h_best_idx, double *h_best_score, int32_t *h_knn_idx,
                                          double *h_knn_score, uint64_t *h_bits);

/* ---- Clustering: DBSCAN on the neighbour bit matrix of N points (the square case of (d): test = train), what the
 *      reference's cluster_matrix asks of scikit-learn for ClusterType.dbscan.  Integer work with a unique answer; no atomics;
 *      every output is a function of the input alone.  In order:
 *   symmetrise, in place: bits[i][j] |= bits[j][i] (an edge is a pair that passes in either direction — the expanded score is
 *     not bit-symmetric in i and j), the diagonal is set, bits of columns >= N are cleared;
 *   d_count [N] (int32): the popcount of row i, the point itself included; d_core [N] (int32 0 / 1): count >= min_samples;
 *   components of the core points over the edges between core points; a component's root is its smallest index;
 *   d_labels [N] (int32): clusters are numbered 0, 1, ... in ascending order of their root; a core point takes its cluster's
 *     number, any other point the smallest number among its core neighbours, -1 without one (scikit-learn's result: a cluster
 *     starts at the lowest unvisited core index, and the first cluster to reach a border point keeps it).
 * *h_n_clusters: the number of clusters; *h_rounds: the rounds the component search took (a round: every core point takes the
 * smallest root among its core neighbours and offers it to its old root, then roots follow their roots; the search ends with the first round that changes
 * nothing; the rounds work in place, so their number depends on the order the device ran the wavefronts in — it is a
 * measurement, the one result here that is not a function of the input alone).  The call waits for the device between rounds
 * and before it returns.
 * Limits (refused with a message, the context stays usable): N outside [0, 2^31); min_samples below 1; a NULL array or
 * result.  N == 0 writes nothing but the two results (0).  Timing slots 39 (symmetrise), 40 (degree), 41 (rounds), 42 (labels).
 * The host twin does the same to h_bits by any sequential method.  Returns 0, -1 a NULL array, -2 N, -3 min_samples. */
MFA_API int mfa_dbscan_from_bits(mfa_ctx *ctx, uint64_t *d_bits, int64_t N, int32_t min_samples, int32_t *d_labels, int32_t *d_core,
                                 int32_t *d_count, int32_t *h_n_clusters, int32_t *h_rounds);
MFA_API int mfa_debug_dbscan_from_bits_host(uint64_t *h_bits, int64_t N, int32_t min_samples, int32_t *h_labels, int32_t *h_core,
                                            int32_t *h_count, int32_t *h_n_clusters);

/* ---- HDBSCAN: the part of the reference's ClusterType.hdbscan that costs O(N^2 D) — every point's core distance and the
 *      minimum spanning tree of the mutual-reachability graph — on N points, with no N x N array stored.  The cluster tree
 *      on the N - 1 edges is host work (montreal_forced_aligner_amd/hdbscan.py).  Shared arithmetic: csrc/hdbscan_math.hpp.
 * The pair form: point i gets a row y_i (D doubles) and a scalar q_i, and the score of the unordered pair is
 *   v(i, j) = (q_i + q_j) + w * sum_k y_ik y_jk   (k ascending, the sweep's sum with test = y, A = 0, B = y, c = 0)
 * the same bits for (i, j) and (j, i); larger is nearer.  metric (the codes of mfa_neighbor_bits_batch):
 *   0 plda, one example a vector: y_k = x_k sqrt(b_k), q = c/2 - 1/2 sum a_k x_k^2, w = 1, with a_k, b_k, c the prepare
 *     step's coefficients at n = 1: v is the log-likelihood ratio; 1 euclidean: y = x, q = -sum x^2, w = 2: v = -|x_i - x_j|^2;
 *   2 dot: y = x, q = 0, w = 1.
 * mfa_hdbscan_core_batch: d_y [N][D], d_q [N] from d_x [N][D] (d_psi [D] for metric 0 only), and d_core [N]: the k-th best
 *   v(i, j) over j != i with v finite (k = min_samples - 1: scikit-learn's count includes the point itself), the order of the
 *   k-nearest lists; -inf for a point with fewer than k finite scores; k = 0: +inf.  d_v [N][N] or NULL: every v as the
 *   consumer sees it (tests).  d_x and d_y may be the same array for metrics 1 and 2.
 * mfa_hdbscan_mst_batch: from d_y, d_q, d_core (metric gives w) the spanning forest of the graph whose edges are the pairs
 *   with v finite, weighted m = min(v, core_i, core_j), under the strict order "larger m, then smaller min(i, j), then
 *   smaller max(i, j)": Boruvka rounds, each one sweep; *h_n_edges edges (N - 1 when the graph is connected) in d_edge_lo <
 *   d_edge_hi, d_edge_score [N - 1], in the order the rounds found them; *h_rounds rounds (at most 40: each at least halves
 *   the components that can still be joined).  The edge set is unique: the same bits every run and for every
 *   MFA_PLDA_PASS_COLS.  Vectors that are not finite are not refused: such a point has no finite score and no edge.
 *   The call waits for the device once a round.
 * Limits (refused with a message, the context stays usable): D outside [1, 1024]; k outside [0, 64]; 2^31 points or more; a
 * metric outside [0, 2]; a psi entry that is not positive and finite (metric 0); a NULL array or result.  N == 0 writes
 * nothing.  Timing slots 36 (prepare), 37 (sweeps), 38 (merges), 41 (the rounds' component work).
 * The host twins: the same contracts in plain loops; the tree twin is Kruskal under the same order, on h_v [N][N] when it
 * is given (then h_y, h_q are not looked at), and the core twin reads its scores from h_v_in [N][N] when that is given.
 * Return 0, -1 a NULL array or a negative count, -2 D, -3 k, -4 psi, -5 N, -8 an unknown metric. */
MFA_API int mfa_hdbscan_core_batch(mfa_ctx *ctx, const double *d_x, int64_t N, int32_t D, int32_t metric, const double *d_psi, int32_t k,
                                   double *d_y, double *d_q, double *d_core, double *d_v);
MFA_API int mfa_hdbscan_mst_batch(mfa_ctx *ctx, const double *d_y, const double *d_q, const double *d_core, int64_t N, int32_t D,
                                  int32_t metric, int32_t *d_edge_lo, int32_t *d_edge_hi, double *d_edge_score, int32_t *h_n_edges,
                                  int32_t *h_rounds);
MFA_API int mfa_debug_hdbscan_core_host(const double *h_x, int64_t N, int32_t D, int32_t metric, const double *h_psi, int32_t k,
                                        double *h_y, double *h_q, double *h_core, double *h_v, const double *h_v_in);
MFA_API int mfa_debug_hdbscan_mst_host(const double *h_y, const double *h_q, const double *h_core, const double *h_v, int64_t N, int32_t D,
                                       int32_t metric, int32_t *h_edge_lo, int32_t *h_edge_hi, double *h_edge_score, int32_t *h_n_edges);

/* ---- Silhouette: the last step of the reference's cluster_matrix, metrics.silhouette_score(to_fit, c_labels, metric), as the
 *      coefficient of every point, on N points whose rows are ordered by cluster, with no N x N array stored.  Shared
 *      arithmetic: csrc/silhouette_math.hpp.  The scores are the pair form's v(i, j) of "HDBSCAN" above (the same metric codes,
 *      the same prepare step); the distance is d = -v (0 plda: the signed -LLR as it is), sqrt(max(-v, 0)) (1 euclidean),
 *      1 - v (2 dot: the cosine distance when the rows have unit length).
 * d_off [C + 1] (int32): cluster c is the rows (and columns) off[c] .. off[c + 1] - 1; off[0] = 0, off[C] = N, strictly
 *   ascending (no empty cluster).
 * For row i of cluster own and every cluster c:  S(i, c) = sum of d(i, j) over j in c, j != i (the diagonal never enters).
 *   The order of the sum: column j adds to partial (j & 63) >> 4 of four, each starting from +0 over its columns ascending, and
 *   S = (P0 + P1) + (P2 + P3).
 *   a = S(i, own) / (n_own - 1), 0 when n_own = 1;  b = the least S(i, c) / n_c over c != own, taken in ascending c from +inf
 *   with "if (m < b) { b = m; bj = c; }": ties go to the lower cluster, a NaN mean is never taken; bj = -1 with b = +inf if none was.
 *   s = 0 when n_own = 1 (scikit-learn's rule); otherwise den = max(a, b) (a < b ? b : a), s = 0 when den == 0, else (b - a) / den.
 *   The counts enter as doubles; every quotient is one IEEE division.  For metric 0 s may leave [-1, 1].
 * d_sil [N]; d_a, d_b [N] and d_bj [N] (int32) or NULL; d_v [N][N] or NULL: every v as the consumer sees it (tests).
 * The sweep runs in one column pass whatever MFA_PLDA_PASS_COLS says: a cluster is never split, and two calls give the same bits.
 * Shape check (silhouette_math.hpp sil_check_shape): N >= 0; D in [1, 1024]; N < 2^31; for N > 0, 2 <= C <= N.
 * Limits (refused with a message, the context stays usable): that shape check; a metric outside [0, 2]; a psi entry that is not
 * positive and finite (metric 0); offsets that break the rule above; a NULL d_x, d_off, d_sil (d_psi for metric 0).  N == 0
 * writes nothing.  The call waits for the device once (the flags).  Timing slots 36 (prepare and pack), 43 (offsets), 44 (sweep).
 * The host twin: the same contract in plain loops and the same order of every sum; it reads its scores from h_v_in [N][N] when
 * that is given.  Returns 0, -1 a NULL array or a negative count, -2 D, -4 psi, -5 N, -6 C, -7 the offsets, -8 an unknown metric. */
MFA_API int mfa_silhouette_batch(mfa_ctx *ctx, const double *d_x, int64_t N, int32_t D, int32_t metric, const double *d_psi,
                                 const int32_t *d_off, int32_t C, double *d_sil, double *d_a, double *d_b, int32_t *d_bj, double *d_v);
MFA_API int mfa_debug_silhouette_host(const double *h_x, int64_t N, int32_t D, int32_t metric, const double *h_psi, const int32_t *h_off,
                                      int32_t C, double *h_sil, double *h_a, double *h_b, int32_t *h_bj, double *h_v, const double *h_v_in);

#ifdef __cplusplus
}
#endif
#endif /* MFA_HIP_H_ */
