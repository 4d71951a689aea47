/*
 * uvad.h -- C ABI of libuvad.so: MI355X (gfx950) voice-activity hot path.
 *
 *   16 kHz PCM --fbank--> log-mel (B,T,F) --classify--> per-frame logit / probability
 *
 * The reference (arnavsshah/universal-voice-activity-detection) is pure Python and has no
 * FFI for this path; its boundary is a set of torch.nn.Module / lhotse call contracts.
 * Each entry point below names the reference interface it stands behind (paths relative to
 * the reference root).  The Python host in universal-voice-activity-detection_amd/ binds
 * these with ctypes (see INTEGRATION.md for the stub a reference maintainer would add).
 *
 * Conventions
 *   - return 0 on success, negative on error: UVAD_E_ARG bad argument, UVAD_E_HIP HIP runtime
 *     error (no GPU, launch failure), UVAD_E_STATE wrong call order (not finalized ...),
 *     UVAD_E_WORKSPACE workspace too small, UVAD_E_UNSUPPORTED configuration outside what the
 *     kernels implement.  uvad_last_error() gives the text.
 *   - every pointer named d_* is a DEVICE pointer owned by the caller; the library never
 *     allocates or frees caller tensors.  It owns only the weights / tables inside uvad_ctx.
 *   - compute calls are ASYNCHRONOUS on `stream` (a hipStream_t passed as void*; NULL = the
 *     default stream) and perform no allocation or synchronisation => hipGraph-capturable
 *     (exceptions: uvad_stream_step, uvad_window_step and uvad_window_wav_step, see there).  Every call makes the context's device current
 *     (hipSetDevice) before it enqueues, so a multi-GPU process may interleave contexts freely.
 *   - one ctx per (device, model); a ctx is NOT thread-safe (the reference drives the model
 *     from a single thread: Trainer(devices=1), src/scripts/predict.py:79-85).
 *   - there is NO CPU fallback: on a machine without a gfx950 device uvad_create fails.
 */
#ifndef UVAD_H
#define UVAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UVAD_OK             0
#define UVAD_E_ARG         -1
#define UVAD_E_HIP         -2
#define UVAD_E_STATE       -3
#define UVAD_E_WORKSPACE   -4
#define UVAD_E_UNSUPPORTED -5

#define UVAD_ABI_VERSION 5

typedef struct uvad_ctx uvad_ctx; /* opaque */

/* Feature-stage configuration = lhotse FbankConfig as constructed at
 * src/datasets/ami/utils.py:153 and src/utils/helper.py:120 (all defaults but sampling_rate). */
typedef struct {
    int sample_rate;   /* 16000 */
    int frame_len;     /* samples per frame: 400 (25 ms) */
    int frame_shift;   /* hop: 160 (10 ms) */
    int n_fft;         /* 512 (next power of two of frame_len); only 512 is implemented */
    int n_mels;        /* 80 in the reference (config/config.py:33), 64 in BASELINE cfg 2 */
    float preemph;     /* 0.97 */
    float low_hz;      /* informational (the mel matrix is uploaded by uvad_set_tables) */
    float high_hz;     /* informational */
    float log_floor;   /* FLT_EPSILON */
    int remove_dc;     /* 1 */
    int snip_edges;    /* 0 (reflect-padded, T = (S + shift/2) / shift) */
} uvad_fbank_cfg;

/* Classifier configuration = constructor arguments of PyanNet2,
 * src/models/segmentation/PyanNet2.py:60-90 (LSTM_DEFAULTS / LINEAR_DEFAULTS / encoding_dim). */
typedef struct {
    int in_dim;        /* encoding_dim */
    int hidden;        /* lstm.hidden_size: 128 (and 64) run the register-resident recurrent kernels; any other size with hidden x
                        * directions a multiple of 32 (<= 1024) runs a generic recurrence (correct to the same bound, slow: W_hh is
                        * streamed from L2 every step); other sizes: UVAD_E_UNSUPPORTED */
    int num_layers;    /* lstm.num_layers: 4 */
    int bidirectional; /* lstm.bidirectional: 1 */
    int lin_hidden;    /* linear.hidden_size: 128 */
    int lin_layers;    /* linear.num_layers: 2 */
    float leaky_slope; /* F.leaky_relu default 0.01 (PyanNet2.py:185); any finite value (NaN / inf: UVAD_E_ARG from uvad_create) */
} uvad_model_cfg;

/* ABI version of the loaded library (== UVAD_ABI_VERSION of the header it was built from). */
int uvad_abi_version(void);

/* Replaces: PyanNet2.__init__/build (PyanNet2.py:69-152) + Fbank(FbankConfig(...)) construction
 * (ami/utils.py:153).  Either cfg may be NULL if that stage is not used. */
int uvad_create(int device, const uvad_fbank_cfg *fb, const uvad_model_cfg *model, uvad_ctx **out);

/* Host tables for the feature stage: window[frame_len]; mel[n_mels][n_fft/2+1] row-major
 * (any banded non-negative matrix; the library converts it to per-filter (start,len,weights)).
 * Replaces the window / filterbank buffers lhotse builds inside Fbank (third party). */
int uvad_set_tables(uvad_ctx *, const float *window, const float *mel);

/* One tensor of the PyanNet2 state_dict, by its torch key ("lstm.weight_ih_l0_reverse",
 * "linear.0.weight", "classifier.bias", ...; an optional "model." Lightning prefix is stripped),
 * host pointer, row-major f32.  Replaces nn.Module.load_state_dict / VadModel.load_from_checkpoint
 * (src/scripts/predict.py:77). */
int uvad_set_weight(uvad_ctx *, const char *torch_key, const float *host, const int64_t *shape, int ndim /* 1..3 */);

/* Checks that every tensor is present, repacks into kernel layouts and uploads.  May be called again after
 * further uvad_set_weight calls (weight hot-swap): it waits for the device to go idle, frees the previous
 * upload and replaces it -- so every hipGraph captured from this context earlier (it bakes the old device pointers of the
 * weights into its kernel nodes) is INVALID afterwards and must be captured again. */
int uvad_finalize(uvad_ctx *);
/* Contexts of one process that are finalized with identical tensors, model / SincNet configuration and device SHARE the packed weights on the
 * device (read-only there; repacked and uploaded once: a pipeline of twelve contexts pays the ~45 ms of host-side packing once, not twelve times).
 * Transparent: a context that swaps a weight and finalizes again gets a block of its own, the others keep theirs; a block is freed with its last
 * context.  Returns how many contexts currently use this context's block (1 = not shared; 0 before uvad_finalize; negative on error). */
int uvad_weights_shared_by(const uvad_ctx *);

/* T for S samples (lhotse framing; data/test_data.py:23 pins T = S/160 for 5 s cuts). */
int64_t uvad_num_frames(const uvad_ctx *, int64_t S);

/* Bytes of caller-provided device workspace uvad_classify / uvad_forward need for B sequences of
 * T frames (uvad_forward: pass T = uvad_num_frames(S)). */
size_t uvad_workspace_bytes(const uvad_ctx *, int B, int64_t T);

/* Replaces: Fbank.extract_batch (lhotse; call sites ami/utils.py:157-163, helper.py:122-130).
 * d_pcm [B][S] f32 in [-1,1]  ->  d_feats [B][T][n_mels] f32. */
int uvad_fbank(uvad_ctx *, const float *d_pcm, int B, int64_t S, float *d_feats, void *stream);

/* Same with int16 PCM (wav ingest; halves the HBM read).  Samples are scaled by 1/32768. */
int uvad_fbank_i16(uvad_ctx *, const int16_t *d_pcm, int B, int64_t S, float *d_feats, void *stream);

/* Replaces: PyanNet2.forward (PyanNet2.py:154-187) = VadModel.forward (vad_engine.py:69-80).
 * d_feats [B][T][in_dim] -> d_logits [B][T] (pre-sigmoid, may be NULL) and d_probs [B][T]
 * (what forward returns, viewed as (B,T,1); may be NULL). */
int uvad_classify(uvad_ctx *, const float *d_feats, int B, int T, float *d_logits, float *d_probs,
                  void *d_workspace, size_t ws_bytes, void *stream);

/* uvad_fbank + uvad_classify without returning the features (they stay in the workspace). */
int uvad_forward(uvad_ctx *, const float *d_pcm, int B, int64_t S, float *d_logits, float *d_probs,
                 void *d_workspace, size_t ws_bytes, void *stream);

/* The same from 16-bit PCM as read from a wav file (samples scaled by 1/32768): what the reference's predict flow does per batch
 * (decode audio -> features -> model, src/scripts/predict.py:98 with the offline feature step of ami/utils.py:153-163 folded in). */
int uvad_forward_i16(uvad_ctx *, const int16_t *d_pcm, int B, int64_t S, float *d_logits, float *d_probs,
                     void *d_workspace, size_t ws_bytes, void *stream);

/* Debug / parity taps: copy of the last LSTM layer output [B][T][hidden*dirs] and of the last
 * feed-forward activation [B][T][lin_hidden] from the most recent uvad_classify on this
 * workspace (async on stream).  Either pointer may be NULL.  Where the fused head ran (two 128-unit feed-forward layers, large
 * launch) the feed-forward tap is recomputed from the LSTM output with the per-layer kernels -- the same bits in GEMM modes 1 / 2;
 * in mode 3 (three products) no kernel can reproduce the fused head's activation and d_lin_out != NULL returns UVAD_E_UNSUPPORTED.
 * After a *_lens call the taps of row b are defined at frames t < len_b only: the rows past a length are padding (the forward direction
 * runs on over the zeroed features up to its workgroup's longest row, rows past that are not written); logits and probabilities there are +0. */
int uvad_get_taps(uvad_ctx *, int B, int T, float *d_lstm_out, float *d_lin_out,
                  const void *d_workspace, void *stream);

/* Streaming (BASELINE cfg 5; the reference has no streaming mode): causal model
 * (bidirectional = 0) with carried state, B streams advancing in lockstep.  Semantics: the logits of
 * frame t are EXACTLY those of the offline path (uvad_forward on the whole signal) because features use
 * the same centred framing; a frame is emitted once its last sample (t*shift - (len-shift)/2 + len) has
 * arrived, i.e. with a look-ahead of 280 samples at the reference geometry.  Each call consumes
 * d_pcm_chunk [B][chunk] and writes the newly complete frames to d_logits [B][ld_logits] (row b, columns
 * 0..k-1); the return value is k >= 0 (same for every stream) or a negative error.  d_state is caller-owned
 * device memory of uvad_stream_state_bytes(ctx, B) bytes holding the PCM tail and (h, c) of every layer;
 * uvad_stream_reset (re)starts all B streams.  The right-edge reflection of the offline path needs the end
 * of the signal and is therefore never produced (streams are open-ended).
 * Nothing but row b's columns 0..k-1 is written; ld_logits < k is UVAD_E_ARG and leaves the streams where they were (the
 * step can be repeated with room for its frames).  Feeds never mix: a NaN / Inf sample makes the logits of ITS feed
 * non-finite from the first frame that holds it on (the energy floor keeps NaN, as the reference's clamp; the carried
 * (h, c) stays NaN until uvad_stream_reset) -- and of the frame before it where the two share a transform (frames are
 * transformed in pairs, positions 2i and 2i + 1 of a step) -- and changes no bit of any other feed.
 * uvad_stream_step is asynchronous but NOT replay-safe by itself under hipGraph capture: the number of complete frames, the
 * PCM-tail ping-pong parity and the first-chunk reflection are host-side counters baked into the launch arguments at
 * enqueue time.  Replay is offered explicitly: uvad_stream_peek says what the NEXT step will bake in -- two steps with the
 * same (B, chunk, k, offset, parity, first) and the same buffers enqueue identical work, so a graph captured around one
 * uvad_stream_step can be replayed for the other, followed by uvad_stream_advance, which moves the counters exactly as the
 * step would have and returns its k (VadRuntime.stream_step does this; at the reference geometry a stream group settles
 * into two graphs, one per parity). */
size_t uvad_stream_state_bytes(const uvad_ctx *, int B);
size_t uvad_stream_workspace_bytes(const uvad_ctx *, int B, int chunk);
int uvad_stream_reset(uvad_ctx *, void *d_state, int B, void *stream);
int uvad_stream_step(uvad_ctx *, const float *d_pcm_chunk, int B, int chunk, void *d_state,
                     float *d_logits, int ld_logits, void *d_workspace, size_t ws_bytes, void *stream);
int uvad_stream_peek(const uvad_ctx *, const void *d_state, int chunk, int *k, int64_t *offset, int *parity, int *first);
int uvad_stream_advance(uvad_ctx *, void *d_state, int chunk);

/* Windowed streaming: any model uvad_classify runs -- bidirectional included, which uvad_stream_* refuses -- served live by
 * re-running it from zero state over a sliding window, the reference's inference semantic (5 s windows, each from zero state,
 * src/datasets/ami/utils.py:107,163; the reference itself has no streaming).  B feeds advance in lockstep, `chunk` samples per step;
 * uvad_window_reset configures a window of `window` = W frames and a look-ahead of `lookahead` = L frames (0 <= L < W, and every step
 * needs L + chunk / frame_shift + 1 <= W, else UVAD_E_ARG).
 *   Features: the framing of uvad_stream_step (snip_edges = 0, first chunk reflected on the left).  Frame t is transformed ONCE, when
 *   its last sample arrives, into a per-feed ring of W frames in d_state, so a window's features are slices of the continuous feature
 *   stream: frame t equals uvad_fbank of the whole signal at t to fp32 rounding.  This is the one deliberate difference from the
 *   reference, which frames every cut anew: only the reflected edge frames of a reference cut differ.
 *   Emission: after a step let e be the number of complete frames.  The step emits frames [f0, e - L) (f0 = what earlier steps emitted;
 *   none while e <= L) and returns their number k >= 0.  The logit of each emitted frame t is row t of the model run from zero state
 *   over the window [max(0, e - W), e) (the prefix [0, e) during the warm-up e < W).  Streams are open-ended: the last L frames are
 *   never emitted and there is no right-edge reflection.  For a causal model with L = 0 the warm-up steps equal uvad_stream_step.
 *   Outputs: d_logits / d_probs [B][ld_out] (row b, columns 0 .. k - 1; either may be NULL, not both).
 * A step enqueues the feature stage for the new frames only, one kernel that writes the window from the ring straight into the first
 * projection's operand, the classifier at (B, Tw = min(e, W)) -- with time chunks off (uvad_get_time_chunks() is 1 afterwards) -- and a
 * gather of the emitted rows.  It never allocates, frees or synchronises, warm-up included.  Host-side counters decide the launch
 * arguments (as for uvad_stream_step); once the window is full the ring position and frame count are read from the device, so two
 * steps with the same replay_key (uvad_window_peek; -1 during the warm-up) and the same buffers enqueue identical work: a graph
 * captured around one replays for the other, followed by uvad_window_advance, which moves the counters as the step would and
 * returns its k.  For a chunk that is a multiple of frame_shift a group settles into two keys (the PCM-tail parity); otherwise into
 * a number bounded by the chunk / frame_shift cycle.
 * uvad_window_features (debug tap) copies the current window's features [B][Tw][n_mels] (as the last step classified them) to
 * d_feats and sets *Tw; d_feats = NULL only sets *Tw. */
size_t uvad_window_state_bytes(const uvad_ctx *, int B, int window);
size_t uvad_window_workspace_bytes(const uvad_ctx *, int B, int chunk, int window);
int uvad_window_reset(uvad_ctx *, void *d_state, int B, int window, int lookahead, void *stream);
int uvad_window_step(uvad_ctx *, const float *d_pcm_chunk, int B, int chunk, void *d_state,
                     float *d_logits, float *d_probs, int ld_out, void *d_workspace, size_t ws_bytes, void *stream);
int uvad_window_peek(const uvad_ctx *, const void *d_state, int chunk, int *k, int64_t *replay_key);
int uvad_window_advance(uvad_ctx *, void *d_state, int chunk);
int uvad_window_features(uvad_ctx *, const void *d_state, int B, float *d_feats, int *Tw, void *stream);

/* Variable-length batches (what torch users know as pack_padded_sequence semantics for nn.LSTM).  Row b of a [B][T] batch holds
 * len_b valid frames; for a bidirectional model padding is no substitute (the backward direction would start in the padding and run
 * through it), so these calls carry the lengths down to the recurrence.
 *   - Lengths live in DEVICE memory: int32 [B] frames (d_lens) or int64 [B] samples (d_nsamp).  They are read on the device and clamped
 *     to [0, T] (resp. [0, S]), so a call stays enqueue-only and hipGraph-capturable, and one captured graph serves any lengths <= T.
 *   - Every output of row b at frame t < len_b equals the model run on that row's first len_b frames alone (from zero state in both
 *     directions).  For GEMM modes 0 and 2 and a pinned recurrent tile (uvad_set_recurrent_tile) the bits are those of uvad_classify on
 *     the row alone at T = len_b; modes 1 and 3 pick their projection / head kernels by launch size and agree to rounding.
 *   - Input frames t >= len_b and PCM samples >= S_b are NEVER read: NaN, Inf or 1e30 there changes no output bit, and they cannot trip
 *     the f16 range check of uvad_classify (the padding of the classifier's operand is zero).
 *   - Outputs at t >= len_b are exactly 0.0f, logits and probabilities; labels there are 0 and runs never extend past len_b.
 *   - PCM: row b has T_b = uvad_num_frames(S_b) frames, framed with the right-edge reflection at S_b: frame t < T_b is bit-identical to
 *     uvad_fbank on pcm[b, :S_b] alone.  Outputs are [B][T], T = uvad_num_frames(S).
 *   - A lens call runs with time chunks off (uvad_get_time_chunks() is 1 afterwards).  The recurrence of a workgroup runs as many steps
 *     as its longest sequence; the GEMMs still run over all T rows.
 *   - Workspace: uvad_workspace_bytes(B, T) as for the dense calls.  d_lens / d_nsamp == NULL: UVAD_E_ARG; a missing table or model:
 *     UVAD_E_STATE. */
int uvad_classify_lens(uvad_ctx *, const float *d_feats, int B, int T, const int32_t *d_lens, float *d_logits, float *d_probs,
                       void *d_workspace, size_t ws_bytes, void *stream);
int uvad_forward_lens(uvad_ctx *, const float *d_pcm, int B, int64_t S, const int64_t *d_nsamp, float *d_logits, float *d_probs,
                      void *d_workspace, size_t ws_bytes, void *stream);
int uvad_forward_lens_i16(uvad_ctx *, const int16_t *d_pcm, int B, int64_t S, const int64_t *d_nsamp, float *d_logits, float *d_probs,
                          void *d_workspace, size_t ws_bytes, void *stream);
/* d_feats [B][T][n_mels], T = uvad_num_frames(S); rows past T_b are written as zero */
int uvad_fbank_lens(uvad_ctx *, const float *d_pcm, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *stream);
int uvad_fbank_lens_i16(uvad_ctx *, const int16_t *d_pcm, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *stream);
/* uvad_median_filter / uvad_label_runs on each row's prefix [0, len_b): the median is scipy medfilt of the prefix with zero padding at
 * both of its ends; a run open at the end of the prefix closes at len_b */
int uvad_median_filter_lens(uvad_ctx *, const float *d_probs, int B, int T, const int32_t *d_lens, int kernel, uint8_t *d_labels,
                            void *stream);
int uvad_label_runs_lens(uvad_ctx *, const uint8_t *d_labels, int B, int T, const int32_t *d_lens, int max_runs, int32_t *d_runs,
                         int32_t *d_counts, void *stream);

/* The waveform model (PyanNet: SincNet + classifier) with per-row sample counts, the semantics above applied to waveforms.
 *   - d_nsamp: device int64 [B], clamped to [0, S].  Row b has T_b = uvad_sincnet_num_frames(S_b) frames; at t < T_b its features /
 *     outputs equal uvad_sincnet / uvad_forward_wav on wav[b, :S_b] alone (the waveform norm and the three instance norms are taken over
 *     the row's own samples / positions), at t >= T_b they are exactly +0.  A row with T_b = 0 (S_b < the receptive field, S_b = 0 too)
 *     is all +0.  Samples >= S_b are never read.  Outputs are [B][frames(S)].
 *   - Features: bit-identical to the dense call on the row when both run the same SincNet form.  The form is chosen on the padded S
 *     (the f16 range guard bounds every row by it), so a lens call can run the exact-f32 form where a row alone would run the split-f16
 *     form; uvad_get_sincnet_form says which ran.  The forward is bit-identical to the dense call on the row for GEMM modes 0 and 2 and a
 *     pinned recurrent tile; modes 1 and 3 agree to rounding (launch-size kernel choice, as uvad_forward_lens).
 *   - The SincNet workgroups share the rows' valid tiles only: padding costs no conv work.  The classifier GEMMs still run over all rows.
 *   - Workspace: uvad_sincnet_workspace_bytes(B, S) (+ uvad_workspace_bytes(B, frames(S)) for the forward), as for the dense calls.
 *     The call is refused only when S itself gives no frame.  d_nsamp == NULL: UVAD_E_ARG; no SincNet configuration or tensors:
 *     UVAD_E_STATE; a workspace too small: UVAD_E_WORKSPACE. */
int uvad_sincnet_lens(uvad_ctx *, const float *d_wav, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *d_workspace,
                      size_t ws_bytes, void *stream);
int uvad_sincnet_lens_i16(uvad_ctx *, const int16_t *d_wav, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *d_workspace,
                          size_t ws_bytes, void *stream);
int uvad_forward_wav_lens(uvad_ctx *, const float *d_wav, int B, int64_t S, const int64_t *d_nsamp, float *d_logits, float *d_probs,
                          void *d_workspace, size_t ws_bytes, void *stream);
int uvad_forward_wav_lens_i16(uvad_ctx *, const int16_t *d_wav, int B, int64_t S, const int64_t *d_nsamp, float *d_logits, float *d_probs,
                              void *d_workspace, size_t ws_bytes, void *stream);

/* Replaces: median_filter (src/utils/helper.py:66-97) as used by VadModel.predict_step
 * (vad_engine.py:204-211): threshold 0.5 then odd `kernel`-tap median, zero padded edges.
 * d_probs [B][T] -> d_labels [B][T] uint8 (0/1). */
int uvad_median_filter(uvad_ctx *, const float *d_probs, int B, int T, int kernel, uint8_t *d_labels,
                       void *stream);

/* Replaces: the per-frame run-length walk of get_new_cuts (src/scripts/predict.py:472-490) on 0/1 frame rows
 * (the output of uvad_median_filter): run i of row b is d_runs[b][i] = {first speech frame, first non-speech frame
 * after it (T if the run is open at the end)}, in order; d_counts[b] = number of runs in the row (runs beyond
 * max_runs are counted but not stored; a row of T frames has at most (T+1)/2).  The host turns frames into seconds
 * with the reference's rounding (round(k*shift, 2), drop empty intervals). */
int uvad_label_runs(uvad_ctx *, const uint8_t *d_labels, int B, int T, int max_runs, int32_t *d_runs /*[B][max_runs][2]*/,
                    int32_t *d_counts /*[B]*/, void *stream);

/* Replaces: get_false_alarm / get_missed_detection (src/scripts/predict.py:666-673) on 0/1 frame rows:
 * d_counts [B][2] uint32 = {#(gt == 0 and pred == 1), #(gt == 1 and pred == 0)} per row; the reference's
 * FA / MD / DER are these counts divided by the row length (DER = FA + MD, vad_engine.py:102-105). */
int uvad_der_counts(uvad_ctx *, const uint8_t *d_pred, const uint8_t *d_gt, int B, int T, uint32_t *d_counts,
                    void *stream);

/* ---- SincNet front end (PyanNet) ------------------------------------------------------------
 * Constructor arguments of SincNet (src/models/blocks/sincnet.py:33-70) as PyanNet builds it
 * (src/models/segmentation/PyanNet.py:62, 91-95: stride 10). */
typedef struct {
    int stride;        /* hop of the sinc filter bank: SINCNET_DEFAULTS["stride"] = 10 */
    int n_filters;     /* 80 (40 cos + 40 sin band-pass filters) */
    int kernel_size;   /* 251 */
    int c2, k2;        /* Conv1d(80, 60, 5) */
    int c3, k3;        /* Conv1d(60, 60, 5); c3 must equal the classifier's encoding_dim */
    float leaky_slope; /* F.leaky_relu default 0.01; any finite value (NaN / inf: UVAD_E_ARG).  A slope > 1 runs the exact-f32 stages */
    float eps;         /* InstanceNorm1d eps 1e-5 of all four norms; finite and >= 0 (else UVAD_E_ARG) */
} uvad_sincnet_cfg;

/* Replaces: SincNet.__init__ (sincnet.py:33-70).  Adds the stage to a context created with a model
 * configuration; its tensors go through uvad_set_weight under their state_dict names
 *   sincnet.wav_norm1d.{weight,bias} [1]      sincnet.norm1d.{0,1,2}.{weight,bias} [C]
 *   sincnet.conv1d.{1,2}.weight [Cout][Cin][k]  sincnet.conv1d.{1,2}.bias [Cout]
 * plus the MATERIALISED first-layer filter bank  sincnet.conv1d.0.filters [n_filters][kernel_size]
 * (what asteroid_filterbanks.ParamSincFB.filters() returns from low_hz_ / band_hz_; the host computes it,
 * see universal-voice-activity-detection_amd/sincnet.py), and uvad_finalize packs them. */
int uvad_sincnet_configure(uvad_ctx *, const uvad_sincnet_cfg *);

/* Output frames for S samples: three (conv, MaxPool1d(3)) stages; 80000 -> 293
 * (src/datasets/custom_vad.py:47, src/utils/receptive_field.py:165-193). */
int64_t uvad_sincnet_num_frames(const uvad_ctx *, int64_t S);

/* Device workspace of uvad_sincnet (pooled activations + norm statistics) for B waveforms of S samples;
 * uvad_forward_wav needs this plus uvad_workspace_bytes(ctx, B, frames). */
size_t uvad_sincnet_workspace_bytes(const uvad_ctx *, int B, int64_t S);

/* Replaces: SincNet.forward (sincnet.py:72-103) followed by the rearrange of PyanNet.forward (PyanNet.py:179).
 * d_wav [B][S] f32 (the reference's (batch, 1, samples) tensor) -> d_feats [B][frames][c3]. */
int uvad_sincnet(uvad_ctx *, const float *d_wav, int B, int64_t S, float *d_feats, void *d_workspace,
                 size_t ws_bytes, void *stream);

/* Replaces: PyanNet.forward (PyanNet.py:162-195): uvad_sincnet + uvad_classify; d_logits / d_probs [B][frames]. */
int uvad_forward_wav(uvad_ctx *, const float *d_wav, int B, int64_t S, float *d_logits, float *d_probs,
                     void *d_workspace, size_t ws_bytes, void *stream);

/* uvad_sincnet / uvad_forward_wav from 16-bit PCM as read from a wav file: samples are read as q / 32768 (as uvad_fbank_i16), straight
 * from d_wav by the waveform kernels (no conversion pass, no f32 copy).  Same workspace (uvad_sincnet_workspace_bytes), same form
 * selection (uvad_get_sincnet_form), asynchronous and capturable like the f32 calls; the results are the f32 calls' bits on q / 32768
 * for S < 2^23 samples per row (the waveform statistics are summed exactly, csrc/sincnet.hip). */
int uvad_sincnet_i16(uvad_ctx *, const int16_t *d_wav, int B, int64_t S, float *d_feats, void *d_workspace,
                     size_t ws_bytes, void *stream);
int uvad_forward_wav_i16(uvad_ctx *, const int16_t *d_wav, int B, int64_t S, float *d_logits, float *d_probs,
                         void *d_workspace, size_t ws_bytes, void *stream);

/* Windowed streaming of the waveform model (PyanNet: SincNet + classifier), the uvad_window_* semantic on raw PCM.  SincNet normalises
 * every stage over the whole row, so nothing carries from step to step: each step re-runs uvad_forward_wav over a sliding window,
 * as the reference infers this model on fixed 5 s cuts, each normalised and run from zero state (predict_sincnet.py, custom_vad.py).
 *   Geometry: J = 27 * stride is the frame step and R = kernel_size + stride * (9 * k3 + 3 * k2 + 14) the receptive field, in samples
 *   (J = 270, R = 991 for the reference); frames(S) = S < R ? 0 : (S - R) / J + 1 = uvad_sincnet_num_frames(S).
 *   B feeds advance in lockstep, `chunk` samples per step.  After a step n samples per feed have arrived and e = frames(n) frames are
 *   complete.  The window is the last Tw = min(e, W) frames [e - Tw, e), whose samples are exactly [J (e - Tw), J (e - Tw) + S_w),
 *   S_w = R + J (Tw - 1).  During the warm-up (e < W) it is the prefix; trailing samples of an incomplete frame are never in it.
 *   The model runs on those S_w samples exactly as uvad_forward_wav (_i16) runs a (B, S_w) batch: from zero state, every norm over the
 *   window.  The step emits frames [f0, e - L) (f0 = what earlier steps emitted; none while e <= L); frame t's logit is row t - (e - Tw)
 *   of that run.  Streams are open-ended: the last L frames are never emitted.
 *   W is in frames and a window holds whole frames only: W = 293 spans 79 831 samples, not the 80 000 of a reference 5 s cut (the
 *   reference's last 169 samples complete no frame).  This is the one difference from the reference's cuts.
 * uvad_window_wav_reset: 0 <= L < W (else UVAD_E_ARG); is_i16 fixes the sample type of the state: uvad_window_wav_step reads f32,
 * uvad_window_wav_step_i16 reads int16 as q / 32768 (as uvad_forward_wav_i16), and a step of the other type is UVAD_E_ARG.  A step
 * needs L + ceil(chunk / J) <= W (else UVAD_E_ARG).  Outputs d_logits / d_probs [B][ld_out] (row b, columns 0 .. k - 1; either may be
 * NULL, not both); an ld_out below the step's k is UVAD_E_ARG and nothing is enqueued or counted.  Returns k >= 0.
 * State: a per-feed ring of the latest PCM in the state's sample type, the last window's SincNet output and a device sample counter.
 * A step commits its chunk to the ring and writes the window [B][S_w] contiguously into the workspace (one kernel), then runs the
 * SincNet stages at (B, S_w), the classifier at (B, Tw) -- time chunks off, uvad_get_time_chunks() is 1 afterwards -- and a gather of
 * the emitted rows.  A step that completes no frame only commits its samples and moves the device counter.  Steps never allocate,
 * free or synchronise, warm-up included.  Once the window is full the ring position comes from the device and every launch argument
 * except k is constant, so two steps with the same replay_key (uvad_window_wav_peek: k; -1 during the warm-up) and the same buffers
 * enqueue identical work: a graph captured around one replays for the other, followed by uvad_window_wav_advance, which moves the
 * counters as the step would and returns its k.
 * uvad_window_wav_features (debug tap) copies the SincNet output [B][Tw][c3] of the last window the model ran on to d_feats and sets
 * *Tw; d_feats = NULL only sets *Tw.
 * Every entry needs a context with a model, uvad_sincnet_configure and uvad_finalize done: otherwise UVAD_E_STATE.  The byte counts
 * need the model and SincNet configurations only, and return 0 without them. */
size_t uvad_window_wav_state_bytes(const uvad_ctx *, int B, int window, int is_i16);
size_t uvad_window_wav_workspace_bytes(const uvad_ctx *, int B, int chunk, int window);
int uvad_window_wav_reset(uvad_ctx *, void *d_state, int B, int window, int lookahead, int is_i16, void *stream);
int uvad_window_wav_step(uvad_ctx *, const float *d_pcm_chunk, int B, int chunk, void *d_state,
                         float *d_logits, float *d_probs, int ld_out, void *d_workspace, size_t ws_bytes, void *stream);
int uvad_window_wav_step_i16(uvad_ctx *, const int16_t *d_pcm_chunk, int B, int chunk, void *d_state,
                             float *d_logits, float *d_probs, int ld_out, void *d_workspace, size_t ws_bytes, void *stream);
int uvad_window_wav_peek(const uvad_ctx *, const void *d_state, int chunk, int *k, int64_t *replay_key);
int uvad_window_wav_advance(uvad_ctx *, void *d_state, int chunk);
int uvad_window_wav_features(uvad_ctx *, const void *d_state, int B, float *d_feats, int *Tw, void *stream);

/* Slot pools of both window families: windowed streams where feeds start and end independently.  A pool of B slots advances in lockstep,
 * `chunk` samples per step; each slot holds at most one session (one call of a server) at a time, and a per-step flag byte per slot
 * starts and ends sessions.  The existing window families (uvad_window_*, uvad_window_wav_*) are unchanged.
 *   State: after *_slots_reset every slot is idle.  d_flags is a DEVICE uint8 [B] per step, or NULL for no changes:
 *     UVAD_SLOT_START  the slot drops whatever it held and a new session begins with this step's chunk as its first samples;
 *     UVAD_SLOT_END    the session ends after this chunk: the slot is idle from the next step on.  Both bits: a one-chunk session.
 *   Idle slots: the chunk row of an idle slot is never read (NaN or Inf there changes no output bit anywhere); they emit nothing.
 *   A session's frames are those of a single-feed stream of the family (B = 1 uvad_window_step / uvad_window_wav_step[_i16]) opened at
 *   the session's start and fed the same chunks: for log-mel the uvad_window_step framing (first chunk reflected on the left, a per-feed
 *   ring, windows of the last min(e, W) frames run from zero state); for the waveform model whole frames of J samples with receptive
 *   field R, the window's samples run as uvad_forward_wav runs them.
 *   Emission, per session: with e_prev complete frames before the step and e after it, a step emits frames [max(0, e_prev - L),
 *   max(0, e - L)); the END step emits [max(0, e_prev - L), e) instead, flushing the L held-back frames from the same window run (no
 *   right-edge reflection, as the window families).  Row b of d_logits / d_probs [B][ld_out] (either may be NULL, not both) gets its
 *   n_b frames in columns 0 .. n_b - 1; columns at and past n_b are not written; d_counts (DEVICE int32 [B], required) receives n_b.
 *   ld_out must be at least L + kmax, kmax = chunk / frame_shift + 1 (log-mel) or ceil(chunk / J) (waveform): else UVAD_E_ARG and
 *   nothing is enqueued.
 *   Enqueue only: a step never allocates, frees or synchronises, and reads every per-slot quantity -- samples since the session's start,
 *   frames, the PCM tail and its ring position, first-chunk status -- from the device (emitted frames follow from frames and L).  Two
 *   steps with the same (B, chunk) and buffers enqueue identical work: a graph captured around any one step replays for every later
 *   one, warm-ups and session changes included.  Steps return UVAD_OK, not a count.
 *   Fixed at reset: chunk, W = window and L = lookahead (0 <= L < W), so the workspace and the graph's shape are fixed too.  Both
 *   families need L + kmax <= W; log-mel needs chunk >= (frame_len - frame_shift) / 2, since any step can be a session's first.
 *   Violations: UVAD_E_ARG.  A step with another B or chunk than the reset's, or the other sample type (waveform): UVAD_E_ARG; a state
 *   never reset: UVAD_E_STATE; a missing configuration / tables / weights: UVAD_E_STATE; a workspace too small: UVAD_E_WORKSPACE.
 *   Work per step: every slot's window runs at (B, W) with per-row lengths Tw_b = min(e_b, W) (0 for an idle slot), the semantics of
 *   uvad_classify_lens: in GEMM modes 0 and 2 with a pinned recurrent tile a session's outputs are bit-identical to its B = 1 stream's,
 *   modes 1 and 3 agree to rounding.  The GEMMs run over all W rows of every slot, idle ones included.
 *   Log-mel: one kernel applies the flags and writes an aligned staging row per slot (its first new frame at column 0) and the next
 *   PCM tail; the unchanged feature kernel transforms kmax frames of every row (plain rows, snip_edges = 1; frames past k_b are
 *   discarded); one kernel commits the k_b new frames to the slot's ring and writes its window left-aligned into the first projection's
 *   operand; then the classifier and a gather of the emitted rows that also commits the counters.
 *   Waveform: one kernel applies the flags, commits the chunk to the slot's PCM ring and writes its window of Sw_b = R + J (Tw_b - 1)
 *   samples left-aligned into [B][Sw_max]; SincNet runs in its lens form at S = Sw_max (workgroups walk the valid tiles only), then the
 *   classifier and the gather.  The SincNet form is chosen on the padded S = Sw_max (uvad_sincnet_lens): a slot can run the exact-f32
 *   form where its B = 1 stream runs the split-f16 one; uvad_get_sincnet_form says which ran.  GEMM modes 0 and 2 always run exact-f32.
 *   *_slots_features (debug tap): the window each slot's last step classified -- log-mel features [B][W][n_mels] / SincNet output
 *   [B][W][c3], left-aligned, rows past Tw_b zero -- and d_tw (DEVICE int32 [B]) = Tw_b (0 for a slot idle in that step).
 *   Time chunks are off in every step (uvad_get_time_chunks() is 1 afterwards). */
#define UVAD_SLOT_START 1
#define UVAD_SLOT_END   2
size_t uvad_window_slots_state_bytes(const uvad_ctx *, int B, int window);
size_t uvad_window_slots_workspace_bytes(const uvad_ctx *, int B, int chunk, int window);
int uvad_window_slots_reset(uvad_ctx *, void *d_state, int B, int chunk, int window, int lookahead, void *stream);
int uvad_window_slots_step(uvad_ctx *, const float *d_pcm_chunk, const uint8_t *d_flags, int B, int chunk, void *d_state,
                           float *d_logits, float *d_probs, int ld_out, int32_t *d_counts, void *d_workspace, size_t ws_bytes, void *stream);
int uvad_window_slots_features(uvad_ctx *, const void *d_state, int B, float *d_feats, int32_t *d_tw, void *stream);
/* The causal stream's slot pool: uvad_stream_step for feeds that start and end independently, still ONE launch per step.  The contract
 * is that of the window slot pools above with lookahead 0 -- flags, idle slots, outputs, d_counts, enqueue only -- and the step has
 * uvad_window_slots_step's argument list, so whatever runs behind a window pool (fusion, endpointers, gates) runs behind this one.
 *   Flags: after uvad_stream_slots_reset every slot is idle.  UVAD_SLOT_START drops whatever the slot held and starts a session with this
 *   chunk as its first samples (zero (h, c) in every layer, the first chunk reflected on the left); UVAD_SLOT_END makes the slot idle
 *   from the next step on; both bits: a one-chunk session; END on an idle slot does nothing.  An idle slot's chunk row is never read, its
 *   state is not written, and d_counts[b] = 0.
 *   A session's frames are, bit for bit, those of a B = 1 uvad_stream_step stream reset at the session's start and fed the same chunks;
 *   frame t is emitted in the step in which its last sample arrives.  The END step emits what its chunk completes and nothing more:
 *   streams are open-ended, there is NO right-edge reflection and no flush (as uvad_stream_step; there is no lookahead to flush).
 *   Row b of d_logits / d_probs [B][ld_out] (either may be NULL, not both) gets its n_b frames in columns 0 .. n_b - 1 and d_counts[b]
 *   (DEVICE int32 [B], required) = n_b; nothing else is written.  ld_out < kmax = uvad_stream_slots_kmax(ctx, chunk) = ceil(chunk /
 *   frame_shift) is UVAD_E_ARG and nothing is enqueued.  A NaN / Inf sample poisons its own session only (as uvad_stream_step), until the
 *   slot's next START.
 *   Enqueue only: the step never allocates, frees or synchronises.  Every per-slot quantity -- the active bit, samples since the
 *   session's start (int64), frames, the PCM tail (updated in place), whether this is the first chunk -- is read and written on the
 *   device, so two steps with the same (B, chunk) and buffers enqueue identical work: one captured graph replays for every later step.
 *   There is no peek / advance.  Steps return UVAD_OK, not a count.
 *   Scope, fixed at reset: the pool exists where uvad_stream_step is one launch -- a causal model with hidden_size 128, 64 or 80 features,
 *   1 .. 8 layers, at most 4 feed-forward layers of 128 -> 128 units; kmax <= 4, i.e. chunks up to 4 frame shifts (40 ms at the
 *   reference geometry); the feature stage (4 rows of frame_len + chunk samples, the mel image, the transform scratch) within 120 KiB
 *   of LDS; chunk >= (frame_len - frame_shift) / 2, since any step can be a session's first; snip_edges = 0.  Reset refuses anything
 *   else with UVAD_E_UNSUPPORTED (model, framing) or UVAD_E_ARG (chunk) and a uvad_last_error text that names the limit; there is no
 *   fallback: other models stream in lockstep groups (uvad_stream_step) or behind the window pools.
 *   Other refusals as the window pools': another B or chunk than the reset's: UVAD_E_ARG; a state never reset, or missing tables /
 *   weights: UVAD_E_STATE; a workspace below uvad_stream_slots_workspace_bytes: UVAD_E_WORKSPACE (the step needs no scratch memory; the
 *   size is a token one that keeps the pools' calling convention).  A refused call leaves the state as it was. */
int uvad_stream_slots_kmax(const uvad_ctx *, int chunk);
size_t uvad_stream_slots_state_bytes(const uvad_ctx *, int B);
size_t uvad_stream_slots_workspace_bytes(const uvad_ctx *, int B, int chunk);
int uvad_stream_slots_reset(uvad_ctx *, void *d_state, int B, int chunk, void *stream);
int uvad_stream_slots_step(uvad_ctx *, const float *d_pcm_chunk, const uint8_t *d_flags, int B, int chunk, void *d_state,
                           float *d_logits, float *d_probs, int ld_out, int32_t *d_counts, void *d_workspace, size_t ws_bytes, void *stream);
/* the same for the waveform model; the sample type (f32, or int16 read as q / 32768) is fixed at reset as in uvad_window_wav_reset */
size_t uvad_window_wav_slots_state_bytes(const uvad_ctx *, int B, int window, int is_i16);
size_t uvad_window_wav_slots_workspace_bytes(const uvad_ctx *, int B, int chunk, int window);
int uvad_window_wav_slots_reset(uvad_ctx *, void *d_state, int B, int chunk, int window, int lookahead, int is_i16, void *stream);
int uvad_window_wav_slots_step(uvad_ctx *, const float *d_pcm_chunk, const uint8_t *d_flags, int B, int chunk, void *d_state,
                               float *d_logits, float *d_probs, int ld_out, int32_t *d_counts, void *d_workspace, size_t ws_bytes,
                               void *stream);
int uvad_window_wav_slots_step_i16(uvad_ctx *, const int16_t *d_pcm_chunk, const uint8_t *d_flags, int B, int chunk, void *d_state,
                                   float *d_logits, float *d_probs, int ld_out, int32_t *d_counts, void *d_workspace, size_t ws_bytes,
                                   void *stream);
int uvad_window_wav_slots_features(uvad_ctx *, const void *d_state, int B, float *d_feats, int32_t *d_tw, void *stream);

/* ---- Sliding-window inference over whole recordings, aggregated on the device --------------------------------------------------------
 * The offline counterpart of the window streams: every recording is covered by overlapping windows of the trained length, each run from
 * zero state, and a frame's score is the weighted mean over all windows that cover it.  Replaces the reference's disjoint 5 s cuts
 * (cut_into_windows(duration=5).filter(duration > 3), src/datasets/ami/utils.py:107, rows laid end to end, predict.py:451-458) with two
 * documented differences: features are slices of the recording's CONTINUOUS feature stream (one uvad_fbank_lens pass per recording,
 * right-edge reflection at S_r; the reference frames every cut anew), and no tail is dropped.
 *   uvad_sliding_configure: window W and hop Hf in frames, 1 <= Hf <= W, and a HOST weight table w[W] (NULL: all ones), uploaded here
 *     once; every weight must be finite and > 0 (so the denominator below is never zero where a window covers): else UVAD_E_ARG.
 *     Configuring again with a table of other values waits for the device to go idle first.
 *   Windows of a recording of T_r frames: n_r = uvad_sliding_count(T_r, W, Hf) = 0 if T_r == 0, 1 if T_r <= W, else
 *     ceil((T_r - W) / Hf) + 1.  Window j starts at frame j Hf and holds len_j = min(W, T_r - j Hf) frames; it runs AT ITS OWN LENGTH with
 *     the semantics of uvad_classify_lens (backward direction from len_j - 1) and is never padded.  Every frame t < T_r is covered and the
 *     last window holds more than W - Hf frames whenever T_r > W.
 *   Aggregate: out[r][t] = (sum_j w[t - j Hf] p_j[t - j Hf]) / (sum_j w[t - j Hf]) over the windows j of r with 0 <= t - j Hf < len_j, in
 *     ascending j, in f32 with every product, sum and the quotient rounded once; probabilities (after the sigmoid), not logits;
 *     out[r][t] = +0 for t >= T_r and for any frame no planned window covers.  Columns [T, ld_out) are not written.
 *   Window list: the host owns the launch count, so it passes d_first, DEVICE int32 [R + 1], the exclusive prefix sums of n_r, and
 *     N = first[R]: global window i in [first[r], first[r + 1]) is window j = i - first[r] of r.  Lengths stay on the device (d_lens int32
 *     frames / d_nsamp int64 samples, clamped as in the lens calls) and len_j is derived there as clamp(T_r - j Hf, 0, W): a plan that
 *     disagrees with the device lengths never causes an out-of-row read, only empty windows or uncovered (zero) frames.  The N windows
 *     are classified in groups of at most `group` per classifier launch, so the workspace is bounded by the group and not by N, each
 *     group writing its rows of an [N][W] buffer; one aggregate launch follows the last group: the result does not depend on `group`
 *     (bit for bit in GEMM modes 0 and 2 with a pinned recurrent tile).  The f16 range flag of uvad_sliding_classify is per group: with
 *     a feature outside the f16 range (GEMM modes 1 - 3) the windows that share a group with the flagged one take the exact-f32 first
 *     projection with it and the other groups the split one, so there the bits, not the error bound, depend on `group`.
 *     d_win_probs (debug tap, or NULL): DEVICE f32 [N][W], every
 *     window's probabilities left-aligned, +0 past len_j.  d_frames (or NULL): DEVICE int32 [R] receives T_r.
 *   uvad_sliding_classify: caller features d_feats [R][T][F] with d_lens; rows past a length are never read.  uvad_sliding_forward
 *     [_i16]: PCM [R][S] with d_nsamp; T = uvad_num_frames(S), T_r = uvad_num_frames(S_r).  uvad_sliding_forward_wav[_i16]: the
 *     waveform model on samples: window j of r is samples [J Hf j, J Hf j + R + J (W - 1)) clipped to S_r, run through SincNet in its
 *     lens form with every norm over the window's own samples; its frame i is the recording's frame j Hf + i; T_r =
 *     uvad_sincnet_num_frames(S_r).  A geometry without a single frame step J: UVAD_E_UNSUPPORTED.
 *   uvad_sliding_workspace_bytes(ctx, R, T, N, group) serves uvad_sliding_classify at that T and uvad_sliding_forward[_i16] at
 *     T = uvad_num_frames(S); uvad_sliding_wav_workspace_bytes(ctx, R, S, N, group) the waveform calls.  0: not configured / bad argument.
 *   Enqueue only: the calls never allocate or synchronise; a graph captured around one replays with other device lengths <= S under the
 *   same plan.  Refusals: before uvad_sliding_configure (or without model / tables / weights): UVAD_E_STATE; group < 1, N < 0, NULL
 *   d_first or lengths, ld_out < T: UVAD_E_ARG; a workspace too small: UVAD_E_WORKSPACE, the needed size in the message.  Time chunks
 *   are off in every call (uvad_get_time_chunks() is 1 afterwards). */
int uvad_sliding_configure(uvad_ctx *, int window, int hop, const float *h_weights /* host [window] or NULL */);
int64_t uvad_sliding_count(int64_t frames, int window, int hop);   /* pure; negative: bad argument */
size_t uvad_sliding_workspace_bytes(const uvad_ctx *, int R, int64_t T, int64_t N, int group);
size_t uvad_sliding_wav_workspace_bytes(const uvad_ctx *, int R, int64_t S, int64_t N, int group);
int uvad_sliding_classify(uvad_ctx *, const float *d_feats, int R, int T, const int32_t *d_lens, const int32_t *d_first, int64_t N, int group,
                          float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *d_workspace, size_t ws_bytes,
                          void *stream);
int uvad_sliding_forward(uvad_ctx *, const float *d_pcm, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first, int64_t N,
                         int group, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *d_workspace, size_t ws_bytes,
                         void *stream);
int uvad_sliding_forward_i16(uvad_ctx *, const int16_t *d_pcm, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first, int64_t N,
                             int group, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *d_workspace,
                             size_t ws_bytes, void *stream);
int uvad_sliding_forward_wav(uvad_ctx *, const float *d_wav, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first, int64_t N,
                             int group, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *d_workspace,
                             size_t ws_bytes, void *stream);
int uvad_sliding_forward_wav_i16(uvad_ctx *, const int16_t *d_wav, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first,
                                 int64_t N, int group, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs,
                                 void *d_workspace, size_t ws_bytes, void *stream);

/* ---- Ingest stage: audio as it arrives -> the [rows][samples] f32, 16 kHz layout every entry point above takes ------------------------
 * Replaces: the audio loading of the reference's non-16 kHz recipes, multi_cut.to_mono(mono_downmix=False) and CutSet.resample(16000)
 * (src/datasets/switchboard/utils.py:102-107, fisher_english/utils.py:106-108, callhome_english/utils.py:110-112, eval2000/utils.py:92-94,
 * babel/utils.py:139, santa_barbara/utils.py:90; lhotse / torchaudio, third party), and the G.711 decode a telephone feed needs first.
 * A stage in FRONT of the existing calls: its output is handed to uvad_forward*, uvad_window_*_step, uvad_*_slots_step unchanged.
 *   Source: `encoding` -- UVAD_INGEST_F32, UVAD_INGEST_I16 (read as q / 32768, as the _i16 calls), UVAD_INGEST_ULAW / UVAD_INGEST_ALAW
 *   (G.711, one byte per sample, expanded to the standard 16-bit value, then / 32768); `channels` C in 1 .. 8, interleaved frame by frame
 *   as in a wav file: input [B][S_in][C]; `sample_rate`: 16000 / sample_rate reduced to up / down.
 *   Channels: every channel becomes a row of its own, output row b * C + c (to_mono(mono_downmix=False)); there is no down-mix.
 *   Resampler: a polyphase FIR whose taps the HOST uploads (uvad_ingest_set_taps: taps[up][K] row-major, K = 2 * width + down), as the
 *   window and mel tables are; output o = j * up + p of a row is the f32 fma chain over k = 0 .. K - 1, in that order from +0, of
 *   x[j * down + k - width] * taps[p][k], x read as zero outside the row.  The order is part of the contract: the dense, ragged and
 *   stream forms give the same bits.  Output length: ceil(up * S_in / down) (uvad_ingest_out_len).  A table of more than 8 phases
 *   (up) or more than 64 taps per phase (K) is UVAD_E_UNSUPPORTED (44.1 kHz: 160 x 475).  up / down = 1 / 1 takes no table and is a
 *   pure decode / de-interleave (bit-exact).  The Python host computes the published Hann-windowed sinc design (width 6, rolloff 0.99).
 *   uvad_ingest_configure drops a table uploaded for another ratio.  uvad_ingest_set_taps with the table the context already holds
 *   (same up, down, width and values) does nothing; with another table it waits for the device to go idle first.  The table keeps its
 *   device address, so a graph captured earlier stays valid only if the new table has the SAME width: K, width, the delay and the LDS
 *   size are baked into a captured step, and the stream state's layout depends on the width.  After a uvad_ingest_set_taps with another
 *   width every ingest stream must be reset on a state of the new uvad_ingest_state_bytes and every graph captured again.
 * uvad_ingest: d_in [B][S_in][C] in the source encoding -> d_out [B * C][ceil(up * S_in / down)] f32.  Outputs leave as 16-byte
 *   vector stores when d_out is 16-byte aligned and the output length is a multiple of 4; any other length is correct but stored
 *   4 bytes at a time throughout (every row then starts at 4-byte alignment only): a caller who chooses S_in picks it so.
 * uvad_ingest_lens: d_nsamp DEVICE int64 [B] input frames per row, clamped to [0, S_in]; frames at or past a row's count are read as
 *   zero and NEVER from memory; row b * C + c equals uvad_ingest on d_in[b, :n_b] alone, and is +0 from ceil(up * n_b / down) on.
 *   d_out_nsamp DEVICE int64 [B * C] receives ceil(up * n_b / down), repeated per channel: it is what uvad_forward_lens /
 *   uvad_forward_wav_lens take as d_nsamp.
 * Stream: B feeds x C channels in lockstep, chunk_in input frames per step (a multiple of down), d_out [B * C][chunk_in * up / down].
 *   The stream cannot see the future: its output is the dense output DELAYED by D = ceil((width + down - 1) / down) * up samples (14
 *   samples = 0.875 ms for 8 kHz; 0 for 1 / 1).  The first D samples of a session are +0 and the last D samples of a session are never
 *   produced.  d_state: caller-owned device memory of uvad_ingest_state_bytes(ctx, B) bytes -- per output row the most recent
 *   H = D * down / up + width decoded input samples and a counter -- cleared by uvad_ingest_stream_reset.  d_flags: DEVICE uint8 [B * C],
 *   one per output row with the slot pools' meaning, or NULL: a row with UVAD_SLOT_START has its history and counter zeroed before the
 *   chunk is consumed (a new session); UVAD_SLOT_END needs no action here.  Everything a step depends on is on the device: a step's
 *   launch depends only on (B, C, chunk_in) and the buffers, so one captured graph replays every step.
 * All compute entries are enqueue-only on `stream` and capturable.  Errors: before uvad_ingest_configure, or without a table where
 * the ratio needs one: UVAD_E_STATE; chunk_in not a multiple of down, NULL pointers: UVAD_E_ARG; state_bytes below
 * uvad_ingest_state_bytes: UVAD_E_WORKSPACE.  A context created without feature / model configuration serves these calls. */
#define UVAD_INGEST_F32  0
#define UVAD_INGEST_I16  1
#define UVAD_INGEST_ULAW 2
#define UVAD_INGEST_ALAW 3
#define UVAD_INGEST_MAX_PHASES 8
#define UVAD_INGEST_MAX_TAPS   64
typedef struct {
    int encoding;      /* UVAD_INGEST_* */
    int channels;      /* 1 .. 8, interleaved */
    int sample_rate;   /* of the source, Hz */
} uvad_ingest_cfg;
int uvad_ingest_configure(uvad_ctx *, const uvad_ingest_cfg *);
int uvad_ingest_set_taps(uvad_ctx *, const float *taps /* host [up][2 * width + down] */, int up, int down, int width);
int64_t uvad_ingest_out_len(const uvad_ctx *, int64_t S_in);   /* negative: not configured / bad argument */
size_t uvad_ingest_state_bytes(const uvad_ctx *, int B);       /* 0: not configured, or no table where one is needed */
int uvad_ingest(uvad_ctx *, const void *d_in, int B, int64_t S_in, float *d_out, void *stream);
int uvad_ingest_lens(uvad_ctx *, const void *d_in, int B, int64_t S_in, const int64_t *d_nsamp, float *d_out, int64_t *d_out_nsamp,
                     void *stream);
int uvad_ingest_stream_reset(uvad_ctx *, void *d_state, size_t state_bytes, int B, void *stream);
int uvad_ingest_stream_step(uvad_ctx *, const void *d_in, const uint8_t *d_flags, int B, int chunk_in, void *d_state, size_t state_bytes,
                            float *d_out, void *stream);

/* ---- Live endpointing: per-feed speech start / end events on the device --------------------------------------------------------------
 * The streaming counterpart of uvad_median_filter_lens, uvad_label_runs_lens and merge_intervals_with_buffer in frame units.  Replaces,
 * used live: median_filter (src/utils/helper.py:66-97), the run walk of get_new_cuts (src/scripts/predict.py:472-490) and
 * merge_intervals_with_buffer (predict.py:614-634).  Everything is integer: the outputs equal the offline kernels' on the whole session.
 *   Sessions: the state holds B slots, one session each; after uvad_endpoint_reset every slot holds the empty session (n = 0 frames).
 *     A step hands slot b the next n_b = clamp(d_counts[b], 0, ld_in) probabilities of its session, columns 0 .. n_b - 1 of row b of
 *     d_probs [B][ld_in]: the d_probs and d_counts a slot pool step wrote, consumed as they are.  d_flags is the slot pools' byte, or NULL:
 *     UVAD_SLOT_START  before this step's frames the slot drops whatever session it held -- silently, no closing events -- and begins at 0;
 *     UVAD_SLOT_END    after this step's frames the session is flushed (below) and the slot holds the empty session again.
 *     Both bits: a one-step session.  Columns >= n_b, and whole rows with n_b = 0, are never read (NaN there changes no output byte).
 *   Labels: x[t] = !(p[t] < threshold) (NaN counts as speech, as uvad_median_filter); with the odd kernel K = 2 h + 1, y[t] = 1 iff the sum
 *     of x[u] over u in [t - h, t + h] and [0, n) exceeds h: scipy.signal.medfilt with zero padding, what uvad_median_filter_lens computes
 *     on the prefix n.  y[t] is final once frame t + h has arrived, or at END: with m frames seen, labels are final on [0, max(0, m - h)),
 *     and END finalises up to n.  A session's finalised labels, concatenated over its steps, are byte-identical to
 *     uvad_median_filter_lens on the session's whole row with len = n (threshold 0.5).
 *   Intervals with a pad of P >= 0 frames: the raw runs [s_i, c_i) of y (uvad_label_runs_lens) become [max(s_i - P, 0), min(c_i + P, n)),
 *     and an interval merges into its predecessor when its start <= the predecessor's end.  Streaming: START at frame max(s - P, 0) is
 *     issued when y[s] = 1 becomes final and no interval is open or pending; a run closed at c stays pending until y[c .. c + 2 P] are all
 *     final and zero, then END is issued at c + P; a run that starts at s <= c + 2 P rejoins the pending interval without events; the END
 *     flag closes what is open or pending at min(c + P, n), or at n while still in speech.  A session's events, concatenated, are exactly
 *     START(lo_0), END(hi_0), START(lo_1), ... of the merged interval list of the whole session, however its frames were cut into steps.
 *   Outputs per step, all DEVICE memory; d_ev_counts is required, the others may be NULL:
 *     d_events [B][max_events][2] int32 {kind, frame}: kind 1 = START, 2 = END; frames count from the session's start;
 *     d_ev_counts [B] int32: the true number of events of this step; events beyond max_events are counted but not stored (as
 *       uvad_label_runs treats max_runs); max_events = ld_in + h + 2 always suffices;
 *     d_active [B] uint8: 1 while a merged interval is open or pending after the step -- the gate a downstream recogniser wants;
 *     d_labels [B][ld_lab] uint8: the labels finalised by this step, d_lab_counts [B] int32 their number (at most n_b + h);
 *       ld_lab >= ld_in + h, and d_labels needs d_lab_counts.
 *   Frames are int32 and saturate: a session consumes no frames past 2^31 - 1 (over a year at 20 ms) and an event frame never wraps.
 *   The configuration lives in the state (a header written by reset): a step carries none, is one launch, allocates nothing, never
 *   synchronises and reads every per-slot quantity from the device, so a graph captured around any step -- alone or in the same capture
 *   as the slot pool step that feeds it -- replays for every later one.  ld_in is at most 2^18 frames per step.
 *   A context created without feature / model configuration serves these calls.  Refusals (UVAD_E_ARG, nothing enqueued): kernel even,
 *   < 1 or > 255; pad < 0 or > 2^20; threshold not finite; B < 1; ld_in < 1; NULL d_probs / d_counts / d_ev_counts / d_state; d_events NULL
 *   with max_events > 0; d_labels with ld_lab < ld_in + h or without d_lab_counts; state_bytes below uvad_endpoint_state_bytes.  A state
 *   never reset, or reset with another B: UVAD_E_STATE. */
typedef struct {
    int kernel;        /* odd median taps K, 1 .. 255 (25 at 20 ms frames, 49 at 10 ms) */
    int pad;           /* P frames added to both ends of every run before merging, 0 .. 2^20 */
    float threshold;   /* speech iff !(p < threshold); finite; 0.5 is the offline kernels' */
} uvad_endpoint_cfg;
size_t uvad_endpoint_state_bytes(const uvad_ctx *, int B, const uvad_endpoint_cfg *);   /* 0 on a bad configuration */
int uvad_endpoint_reset(uvad_ctx *, void *d_state, size_t state_bytes, int B, const uvad_endpoint_cfg *, void *stream);
int uvad_endpoint_step(uvad_ctx *, const float *d_probs, int ld_in, const int32_t *d_counts, const uint8_t *d_flags, int B, void *d_state,
                       size_t state_bytes, int32_t *d_events, int max_events, int32_t *d_ev_counts, uint8_t *d_active, uint8_t *d_labels,
                       int ld_lab, int32_t *d_lab_counts, void *stream);

/* ---- Scoring against reference labels: counts, loss, threshold sweep, accumulated on the device ---------------------------------------
 * Replaces: test_step / validation_step of src/engines/vad_engine.py:128-202 (BinaryStatScores at one operating point, the median filter
 * in front of it, binary_cross_entropy of _common_step, :247-278), get_false_alarm / get_missed_detection and get_binary_tensor of
 * src/scripts/other_vad_metrics.py:299-318 and supervisions_feature_mask of src/datasets/custom_vad.py:41-75.  Everything but the loss
 * is integer and exact; the state accumulates over any number of steps, and a step allocates nothing, never synchronises and reads the
 * row lengths from the device, so it can be one more node of a captured graph.
 *
 * uvad_intervals_to_labels: d_iv [B][max_iv][2] int32 {start, end} in frames, d_iv_counts [B] int32 (clamped to [0, max_iv]).  Row b of
 *   d_labels [B][ld] uint8 becomes 1 on the union of [max(s, 0), min(e, len_b)) over its first d_iv_counts[b] intervals and 0 elsewhere
 *   on [0, len_b), len_b = clamp(d_lens[b], 0, T) (T when d_lens is NULL).  Intervals may be unsorted and overlapping; e <= s is ignored.
 *   Columns at or past len_b are not written.  ld >= T; d_iv may be NULL when max_iv is 0.
 *
 * Configuration (uvad_score_configure; a context created without feature / model configuration serves these calls):
 *   n_points 1 .. 8 operating points (threshold[m] finite, kernel[m] odd 1 .. 255); collar 0 .. 1024 frames; bins a power of two 2 .. 1024;
 *   segment: frames one workgroup scores, 1 .. 16384, 0 = the built-in default (2048).  No output depends on it.
 * Semantics of a step for row b with n = clamp(d_lens[b], 0, T) (T when d_lens is NULL), p = d_probs [B][ld_p] f32, gt = d_gt [B][ld_gt]
 * uint8 (non-zero = speech); columns at or past n, and rows with n = 0, are never read in either:
 *   labels at point m   x[t] = !(p[t] < threshold[m]) (NaN counts as speech); with K = 2 h + 1, y[t] = 1 iff the sum of x over
 *                       [t - h, t + h] and [0, n) exceeds h: uvad_median_filter_lens at that threshold; K = 1 is the raw threshold;
 *   collar c            with k over the boundaries 1 <= k <= n - 1 where gt[k - 1] != gt[k], frame t is unscored iff some k has
 *                       k - c <= t <= k + c - 1; row ends are not boundaries; c = 0 scores every valid frame;
 *   counts              tp, fp, tn, fn per point over the scored frames, pooled in the state; for point 0 also per row:
 *                       d_rows [B][4] uint64 {tp, fp, tn, fn} of this step (may be NULL);
 *   sweep               hist[class][bin] over the scored frames, class = (gt != 0), bin = min(bins - 1, floor(p * bins)) (NaN: the last
 *                       bin; p * bins is exact in f32): the sum of hist[0] over bins >= j is the number of false-alarm frames at
 *                       threshold j / bins with K = 1, the sum of hist[1] over bins < j the number of missed frames, both exactly, for
 *                       every j < bins (j = bins stands for a threshold above every probability: p = 1 and NaN sit in the last bin);
 *   loss                the sum of F.binary_cross_entropy's terms -(g max(log p, -100) + (1 - g) max(log(1 - p), -100)) over ALL valid
 *                       frames (no collar), each evaluated in f64 from the f32 probability, summed per (row, segment), then over the
 *                       segments and rows in a fixed order by a second kernel: no floating-point atomics, the same calls give the same
 *                       bits.  A NaN probability (or one outside [0, 1]) in a valid frame makes the loss NaN.
 * Workspace: uvad_score_ws_bytes(ctx, B, T) bytes (0 on a bad argument or before uvad_score_configure).  After a step its first 16 bytes
 *   hold {double loss sum, uint64 valid frames} of THAT step (what test_step returns as the batch loss, without a copy to the host).
 * uvad_score_totals writes UVAD_SCORE_TOTALS_WORDS uint64 words to d_out (device memory, for the host to copy):
 *   [0] n_points  [1] bins  [2] valid frames  [3] the loss sum, the bits of a double  [4] steps  [5 .. 7] 0
 *   [8 + 4 m + k] k = 0 .. 3: tp, fp, tn, fn of point m (m < 8)
 *   [40 + 1024 cls + j] hist[cls][j], j < bins
 * Refusals (nothing enqueued).  UVAD_E_ARG: n_points outside 1 .. 8; kernel even, < 1 or > 255; threshold not finite; collar < 0 or
 *   > 1024; bins not a power of two in 2 .. 1024; segment < 0 or > 16384; NULL d_probs / d_gt / d_state / d_ws / d_out; B < 1; T < 1 or
 *   > 2^30; ld_p < T or ld_gt < T; state_bytes below uvad_score_state_bytes or ws_bytes below uvad_score_ws_bytes.  UVAD_E_STATE: no
 *   uvad_score_configure yet; a state that was never reset, or reset under another n_points / bins. */
#define UVAD_SCORE_MAX_POINTS 8
#define UVAD_SCORE_TOTALS_WORDS 2088
typedef struct {
    int n_points;                            /* 1 .. 8 */
    float threshold[UVAD_SCORE_MAX_POINTS];  /* speech iff !(p < threshold) */
    int kernel[UVAD_SCORE_MAX_POINTS];       /* odd median taps, 1 .. 255 (1: the raw threshold, what validation_step scores) */
    int collar;                              /* frames left unscored on each side of a reference boundary, 0 .. 1024 */
    int bins;                                /* histogram bins, a power of two, 2 .. 1024 */
    int segment;                             /* frames per workgroup, 0 = default */
} uvad_score_cfg;
int uvad_intervals_to_labels(uvad_ctx *, const int32_t *d_iv, const int32_t *d_iv_counts, int B, int max_iv, int T, int ld,
                             const int32_t *d_lens, uint8_t *d_labels, void *stream);
int uvad_score_configure(uvad_ctx *, const uvad_score_cfg *);
size_t uvad_score_state_bytes(const uvad_ctx *);   /* 0 before uvad_score_configure */
size_t uvad_score_ws_bytes(const uvad_ctx *, int B, int T);
int uvad_score_reset(uvad_ctx *, void *d_state, size_t state_bytes, void *stream);
int uvad_score_step(uvad_ctx *, const float *d_probs, int ld_p, const uint8_t *d_gt, int ld_gt, int B, int T, const int32_t *d_lens,
                    void *d_state, size_t state_bytes, uint64_t *d_rows, void *d_ws, size_t ws_bytes, void *stream);
int uvad_score_totals(uvad_ctx *, const void *d_state, size_t state_bytes, uint64_t *d_out, void *stream);

/* ---- Speech cuts: merged, split segments and their audio, on the device ---------------------------------------------------------------
 * The offline counterpart of the endpointer.  Replaces the tail of get_new_cuts (src/scripts/predict.py): the run walk (:472-490),
 * merge_intervals_with_buffer (:614-634) in frames, split_into_windows (:638-647) on integers, and the truncation of the recording to
 * each window -- with no copy to the host in between.  The input is the output of uvad_median_filter(_lens).  Everything is integer;
 * every output is byte-exact against a numpy restatement (tests/cuts_ref.py).
 *
 * Cut semantics for row b with n = clamp(d_lens[b], 0, T) frames and S_b = clamp(d_nsamp[b], 0, S) samples (NULL: T and S):
 *   1 runs      [s_i, c_i) of the labels on [0, n), exactly as uvad_label_runs_lens; any non-zero byte counts as 1;
 *   2 merge     with the pad P: each run becomes [max(s - P, 0), min(c + P, n)), and an interval merges into its predecessor when its
 *               start <= the predecessor's end (what the endpointer reports as START / END events over the whole session);
 *   3 split     a merged interval [lo, hi) of L frames: with W = max_len > 0, q = (L - 1) / W pieces of W frames from lo on and a last
 *               piece of r = L - q W frames, 0 < r <= W; W = 0: q = 0, r = L.  The last piece is kept iff r > m = min_len.  This is
 *               split_into_windows (predict.py:638-647: `while e - s > window` cuts full windows, `if e - s > 0.1` keeps the rest) on
 *               integer frames, its 0.1 s made the parameter m;
 *   4 samples   a piece [f, f + k) covers samples [max(f hop - lead, 0), min((f + k) hop + tail, S_b)), in int64; a piece whose range
 *               is empty is still listed, with n_samples = 0.  With tail = frame_len - hop (240 for log-mel, 721 for SincNet's 991 - 270)
 *               a cut holds every sample any of its frames saw; tail = 0 gives disjoint cuts.
 *   Cuts are ordered by row, then by time.  The reference's split=True, window=10 at 10 ms frames is max_len = 1000, min_len = 10; its
 *   split=False is 0, 0.
 * uvad_cuts_max_per_row: (T + 1) / 2 + (W ? T / W : 0), a bound on one row's cuts; uvad_cuts_max_samples: W ? min(S, W hop + lead + tail)
 *   : S, a bound on n_samples.  Both 0 on a bad configuration (or T outside 1 .. 2^30, S < 0).
 * uvad_cuts_table: d_labels [B][ld] uint8, ld >= T.  d_table [max_cuts] receives the first min(total, max_cuts) cuts (cuts past max_cuts
 *   are counted but not stored, as uvad_label_runs treats max_runs; later entries are not written); d_row_first [B + 1] int32: entry b
 *   the index of row b's first cut, entry B the total; d_total [1] int32: the true number of cuts.  Label columns at or past n, and
 *   whole rows with n = 0, are never read.  Workspace: uvad_cuts_ws_bytes(ctx, B, T) bytes (0 on a bad argument).
 * uvad_cuts_gather: output row i < min(*d_total, max_cuts) of d_out [max_cuts][ld_out] receives units [0, c) of cut i, c = min(n, ld_out),
 *   then zero bytes up to ld_out, and d_out_len[i] = c (int32): truncation shows as d_out_len[i] < n.  Later rows and lengths are not
 *   written; source units outside a cut's range are never read.
 *     UVAD_CUTS_SAMPLES  n = n_samples from first_sample on; d_src [B][row_stride] units of 2 bytes (int16 PCM) or 4 (f32);
 *     UVAD_CUTS_FRAMES   n = n_frames from first_frame on; d_src [B][row_stride] records of unit_bytes, any multiple of 4 up to 4096
 *                        (a feature tensor [B][T][F] f32: unit_bytes = 4 F, row_stride = T): the rows a recogniser with log-mel input wants.
 *   Stores are 16 bytes wide when ld_out x unit_bytes is a multiple of 16 and d_out is 16-byte aligned; any other stride works, slower.
 * Both calls allocate nothing, never synchronise and read every count from the device; their grids depend on B, T, max_cuts and ld_out
 * alone, and workgroups past the total do nothing: a graph captured around table + gather replays for new labels, lengths and audio.
 * A context created without feature / model configuration serves them.
 * Refusals (UVAD_E_ARG, nothing enqueued, uvad_last_error names the word): a NULL cfg; pad outside [0, 2^20]; max_len outside [0, 2^24];
 *   min_len < 0, or >= max_len when max_len > 0; hop < 1; lead < 0; tail < 0; B < 1; T < 1 or > 2^30; ld < T; S < 0; max_cuts < 0; NULL
 *   d_labels / d_row_first / d_total / d_ws; NULL d_table with max_cuts > 0; B x uvad_cuts_max_per_row above 2^31 - 1; ws_bytes below
 *   uvad_cuts_ws_bytes ("need N bytes"); unit_bytes not 2 or 4 (samples) or no multiple of 4 in [4, 4096] (frames); which unknown;
 *   ld_out < 1 or > 2^31 - 1; row_stride < 0; NULL d_src / d_table / d_total / d_out / d_out_len. */
#define UVAD_CUTS_SAMPLES 0
#define UVAD_CUTS_FRAMES 1
typedef struct {
    int pad;       /* P frames added to both ends of every run before merging, 0 .. 2^20 (as uvad_endpoint_cfg.pad) */
    int max_len;   /* W frames: 0 = no splitting, 1 .. 2^24 = no cut longer than W frames */
    int min_len;   /* m frames: a last piece of <= m frames is dropped; 0 drops nothing; < max_len when max_len > 0 */
    int hop;       /* samples per frame, >= 1 (160 log-mel at 10 ms, 270 SincNet) */
    int lead;      /* samples taken before the first frame's first sample, >= 0 */
    int tail;      /* samples taken past the last frame's hop, >= 0 */
} uvad_cuts_cfg;
typedef struct {
    int32_t row, index, first_frame, n_frames;
    int64_t first_sample, n_samples;
} uvad_cut;   /* 32 bytes; index = position within its row */
int uvad_cuts_max_per_row(const uvad_cuts_cfg *, int T);
int64_t uvad_cuts_max_samples(const uvad_cuts_cfg *, int64_t S);
size_t uvad_cuts_ws_bytes(const uvad_ctx *, int B, int T);
int uvad_cuts_table(uvad_ctx *, const uint8_t *d_labels, int ld, int B, int T, const int32_t *d_lens, const int64_t *d_nsamp, int64_t S,
                    const uvad_cuts_cfg *, uvad_cut *d_table, int max_cuts, int32_t *d_row_first, int32_t *d_total, void *d_ws,
                    size_t ws_bytes, void *stream);
int uvad_cuts_gather(uvad_ctx *, const void *d_src, int64_t row_stride, int unit_bytes, int which, const uvad_cut *d_table,
                     const int32_t *d_total, int max_cuts, void *d_out, int64_t ld_out, int32_t *d_out_len, void *stream);

/* ---- The cut-supervision join: which supervisions (or words) belong to which cut, and the audit, on the device -------------------------
 * Replaces the step get_new_cuts exists for (src/scripts/predict.py): cut.truncate(offset, duration, keep_excessive_supervisions=True,
 * _supervisions_index=...) (predict.py:515-520), which gives each new cut the supervisions that overlap it; the exceed test of :541; the
 * transcript of a cut, its supervisions' texts or the alignment's words that lie wholly inside it (:549-572); and the seven counters
 * printed after every run (:597-611, again in other_vad_metrics.py:259-271).  Everything is integer, in frames; every output is
 * byte-exact against a brute-force numpy restatement (tests/join_ref.py).
 *
 * Inputs: d_table, d_row_first [B + 1] and d_total exactly as uvad_cuts_table wrote them; d_iv [B][max_iv][2] int32 {s, e} in frames and
 *   d_iv_counts [B] int32 (clamped to [0, max_iv]), the layout of uvad_intervals_to_labels.  Items may be unsorted, overlapping, negative
 *   or past the row.  With m = min(*d_total, max_cuts), only cuts with global index < m take part (later cuts are not in the table);
 *   row b's cuts are [d_row_first[b], min(d_row_first[b + 1], m)), ascending and disjoint in frames.
 * Semantics: a cut covers [f, f + k), f = first_frame, k = n_frames; an item is [s, e).
 *   UVAD_JOIN_OVERLAP  the item matches the cut iff s < f + k and e > f (the half-open rule of the interval tree behind truncate);
 *   UVAD_JOIN_INSIDE   iff s >= f and e <= f + k (the word rule of predict.py:565-568);
 *   an item with e <= s matches nothing in either mode, and is still counted as an item;
 *   a matched pair EXCEEDS iff f > s or f + k < e (predict.py:541); INSIDE can never exceed.
 * Outputs:
 *   d_pair_first [max_cuts + 1] int32: entry i <= m the index of cut i's first pair, so entry m is the true number of pairs, which may
 *     exceed max_pairs; entries past m are not written;
 *   d_pairs [max_pairs] int32: for each cut in table order the indices, within the row, of its matching items, ascending within a cut;
 *     pairs at or past max_pairs are counted, not stored (as uvad_label_runs treats max_runs);
 *   d_item_cuts [B][max_iv][2] int32 (may be NULL): for each item below its row's count {global index of the first matching cut, number
 *     of matching cuts} -- the matching cuts are contiguous because cuts are disjoint and ordered -- and {-1, 0} when none match;
 *     slots past the count are not written;
 *   d_audit [B + 1][UVAD_JOIN_AUDIT_WORDS] uint64, per row, row B the sum over rows:
 *     [0] items  [1] cuts taking part  [2] pairs  [3] items with at least one cut  [4] items with none (= [0] - [3])
 *     [5] exceeding pairs  [6] repeated pairs (= [2] - [3]; the reference's "in multiple")  [7] cuts with no item
 *     The reference's report: Total = [0], in new cuts = [2], unique = [3], not in = [4], exceeding = [5], in multiple = [6], empty
 *     cuts = [7].  Words 0, 3, 4, 5 are counted from the items' side and 1, 2, 7 from the cuts' side, independently.
 * The call allocates nothing, never synchronises and reads every count from the device; its grids depend on B, max_iv and max_cuts
 * alone, and workgroups past the totals do nothing: a graph captured around uvad_cuts_table + uvad_cuts_join (+ uvad_cuts_gather) replays
 * for new labels, lengths and items.  Never read: table entries at or past m, item slots at or past the row's count, and the item
 * slots of a row with no cuts (such a row still gets its counters; a row with no items gives every one of its cuts an empty pair list).
 * No atomics: the same calls give the same bytes.  Workspace: uvad_cuts_join_ws_bytes(ctx, B, max_iv, max_cuts) bytes (0 on a bad
 * argument).  The cost is cuts x items per row.  A context created without feature / model configuration serves the call.
 * Refusals (UVAD_E_ARG, nothing enqueued, uvad_last_error names the word): B < 1; max_iv < 0; max_cuts < 0; max_pairs < 0; mode unknown;
 *   NULL d_row_first / d_total / d_iv_counts / d_pair_first / d_audit / d_ws; NULL d_table with max_cuts > 0; NULL d_iv with max_iv > 0;
 *   NULL d_pairs with max_pairs > 0; max_cuts x max_iv above 2^31 - 1 (what d_pair_first can count); ws_bytes below
 *   uvad_cuts_join_ws_bytes ("need N bytes"). */
#define UVAD_JOIN_OVERLAP 0
#define UVAD_JOIN_INSIDE  1
#define UVAD_JOIN_AUDIT_WORDS 8
size_t uvad_cuts_join_ws_bytes(const uvad_ctx *, int B, int max_iv, int max_cuts);   /* 0 on a bad argument */
int uvad_cuts_join(uvad_ctx *, const uvad_cut *d_table, const int32_t *d_row_first, const int32_t *d_total, int max_cuts, int B,
                   const int32_t *d_iv, const int32_t *d_iv_counts, int max_iv, int mode,
                   int32_t *d_pair_first, int32_t *d_pairs, int max_pairs, int32_t *d_item_cuts, uint64_t *d_audit,
                   void *d_ws, size_t ws_bytes, void *stream);

/* ---- Channel fusion: one decision per multi-microphone recording, on the device ------------------------------------------------------------
 * The ingest stage makes a row of every channel; this stage puts the rows of one recording back together.  It replaces, for corpora with
 * one set of reference labels over several channels (the `mdm` microphone-array and the two-channel telephone recipes under
 * src/datasets/), the stack / reduce / argmax a caller would do on the host before the per-recording get_binary_tensor / FA / MD block of
 * src/scripts/other_vad_metrics.py:156-213 -- with no copy to the host in between.  Every output is bit-defined and byte-exact against a
 * numpy restatement (tests/fuse_ref.py).
 *
 * uvad_fuse_configure: all arrays are HOST arrays; they are validated, then uploaded into the context (as uvad_sliding_configure's weights
 *   and uvad_ingest_set_taps' table).  Group g is member slots j in [h_group_first[g], h_group_first[g + 1]); slot j reads input row
 *   h_members[j]; N = h_group_first[G].  Rows need not be contiguous and may appear in several groups.  h_weights [N] (NULL: all ones)
 *   weigh MEAN and VOTE.  cfg.threshold is a member's own speech test, !(p < threshold); cfg.decide the same test on the fused value.
 *   One configuration per context; a later configure replaces it (graphs captured before it keep the grid of the old one).
 *   If the upload itself fails (UVAD_E_HIP) the validated configuration is kept, so uvad_fuse_ws_bytes and every argument refusal below
 *   still answer; uvad_fuse and uvad_fuse_pick then return UVAD_E_HIP after their argument checks.
 * uvad_fuse: d_in [B][ld_in] f32, d_lens [B] int32 or NULL, d_flags_in [B] uint8 or NULL.  One call serves dense and ragged batches and a
 *   live step: there d_in, d_lens and d_flags_in are the d_probs, d_counts and flag bytes a slot pool step wrote, and T = ld_in.
 *   With n_r = clamp(d_lens[r], 0, T) (T when d_lens is NULL):
 *   group length  L_g = max n_r over the group's members -> d_glens[g] (int32).  At frame t < L_g the valid members are those with t < n_r.
 *   never read    columns at or past n_r of any row; rows no group names; whole rows with n_r = 0.  Output columns at or past L_g are
 *                 never written.
 *   UVAD_FUSE_MAX   the largest valid member value, NaN ranking above everything: if any valid member is NaN the result is (that) NaN,
 *                   in keeping with "NaN counts as speech" everywhere above;
 *   UVAD_FUSE_MEAN  over the valid members in slot order, in f64: acc += (double)w_j * (double)p_j, W += (double)w_j; the result is
 *                   (float)(acc / W), or 0.0f when W == 0.  A product of two f32 values is exact in f64, so contraction to an fma cannot
 *                   change a bit.  The input may as well be logits: no meaning is attached to the range.  A NaN result (a NaN member,
 *                   inf x 0, inf - inf) is written as the one quiet NaN 0x7fc00000, whatever sign the arithmetic gave it;
 *   UVAD_FUSE_VOTE  the same expression with p_j replaced by 1.0 if !(p_j < threshold) (NaN votes speech) and 0.0 otherwise: the weighted
 *                   share of members that hear speech.  decide = 0.5 is a majority; a decide just above 0 means any member.
 *   d_fused [G][ld_f] f32   the fused value;
 *   d_labels [G][ld_l] u8   !(fused < decide) as 0 / 1: raw labels, in the form uvad_cuts_table reads as it is;
 *   d_best [G][ld_b] u8     the position within the group of the valid member with the largest value: NaN ranks above everything, ties
 *                           go to the lowest position, weights play no part;
 *   d_stats [N][UVAD_FUSE_STATS_WORDS] uint64 per member slot, ADDED to what is there (the caller zeroes it once with a memset; a live
 *                           session or a sweep over batches then accumulates with no copy to the host): [0] valid frames  [1] frames
 *                           with !(p < threshold)  [2] frames whose own decision equals the fused decision  [3] frames where it is best;
 *   d_flags_out [G] u8      the bitwise OR of the members' d_flags_in bytes; written only when both flag pointers are given.
 *   d_labels, d_best, d_stats and the two flag arrays may each be NULL; d_fused and d_glens are required.
 *   The call allocates nothing, never synchronises and reads all lengths from the device; its grid depends on the configuration, B and T
 *   alone: a captured graph replays for new inputs and lengths.  No atomics: ballots and population counts per wave, one partial per
 *   (member slot, frame tile, wave) in d_ws, and a fold in a fixed order that adds into d_stats -- the same calls give the same bytes.
 *   16-byte loads where a row's base is 16-byte aligned and four frames are valid, single loads elsewhere; the output does not depend on
 *   which ran.  Workspace: uvad_fuse_ws_bytes(ctx, B, T) bytes (0 on a bad argument or before uvad_fuse_configure).
 * uvad_fuse_pick: the channel of each cut.  For cut i < min(*d_total, max_cuts) of a table uvad_cuts_table made from the fused labels
 *   (row = group g): among the group's members the position k with the most frames t in [first_frame, first_frame + n_frames) where
 *   d_best[g][t] == k; ties go to the lowest position; a cut of 0 frames gets k = 0.  d_pick[i] = k (int32); d_out_table[i] is the cut
 *   with row replaced by that member's INPUT row index and everything else unchanged, so the unchanged uvad_cuts_gather on the [B] audio
 *   rows fetches each cut from the channel that heard it best.  Later entries are not written.  A cut whose row is not a group index is
 *   skipped: its entry is copied unchanged and its pick is -1.  d_out_table may be d_table itself.
 * A context created without feature / model configuration serves all of these calls.
 * Refusals (UVAD_E_ARG, nothing enqueued, uvad_last_error names the word):
 *   uvad_fuse_configure: NULL cfg / h_group_first / h_members; G < 1; h_group_first[0] != 0 or not non-decreasing; a group with 0 or
 *     more than UVAD_FUSE_MAX_MEMBERS members; a member index < 0; a weight that is not finite or is < 0; a group whose weights sum to 0;
 *     a threshold or decide that is not finite; an unknown mode;
 *   uvad_fuse: NULL d_in / d_fused / d_glens / d_ws; B not above the largest configured member index; T < 1 or > 2^30; any of ld_in,
 *     ld_f, ld_l, ld_b below T where its array is given; ws_bytes below uvad_fuse_ws_bytes ("need N bytes"); exactly one of the two flag
 *     arrays given;
 *   uvad_fuse_pick: NULL d_best / d_total; NULL d_table with max_cuts > 0; both outputs NULL; max_cuts < 0; ld_b < 1.
 *   UVAD_E_STATE: uvad_fuse / uvad_fuse_pick before uvad_fuse_configure. */
#define UVAD_FUSE_MAX  0
#define UVAD_FUSE_MEAN 1
#define UVAD_FUSE_VOTE 2
#define UVAD_FUSE_MAX_MEMBERS 255
#define UVAD_FUSE_STATS_WORDS 4
typedef struct {
    int mode;          /* UVAD_FUSE_MAX, UVAD_FUSE_MEAN or UVAD_FUSE_VOTE */
    float threshold;   /* a member hears speech at !(p < threshold); finite */
    float decide;      /* the fused label is !(fused < decide); finite */
} uvad_fuse_cfg;
int uvad_fuse_configure(uvad_ctx *, const uvad_fuse_cfg *, const int32_t *h_group_first, const int32_t *h_members, const float *h_weights,
                        int G);
size_t uvad_fuse_ws_bytes(const uvad_ctx *, int B, int T);   /* 0 on a bad argument or before uvad_fuse_configure */
int uvad_fuse(uvad_ctx *, const float *d_in, int ld_in, int B, int T, const int32_t *d_lens, const uint8_t *d_flags_in,
              float *d_fused, int ld_f, int32_t *d_glens, uint8_t *d_flags_out, uint8_t *d_labels, int ld_l, uint8_t *d_best, int ld_b,
              uint64_t *d_stats, void *d_ws, size_t ws_bytes, void *stream);
int uvad_fuse_pick(uvad_ctx *, const uint8_t *d_best, int ld_b, const uvad_cut *d_table, const int32_t *d_total, int max_cuts,
                   uvad_cut *d_out_table, int32_t *d_pick, void *stream);

/* ---- Hysteresis decisions with minimum durations, on the device -----------------------------------------------------------------------
 * The other way from probabilities to speech labels, beside the threshold + median of uvad_median_filter (the reference's predict_step):
 * two thresholds, a shortest speech interval, a shortest pause and asymmetric padding -- the parameter set of the pyannote pipeline whose
 * output the reference scores itself against (src/scripts/other_vad_metrics.py reads baseline_vad/pyannote_output).  Offline: dense and
 * ragged batches (live feeds: uvad_endpoint_hyst_* below).  Everything after the two comparisons is integer; every output is byte-exact
 * against a frame-loop restatement (tests/binarize_ref.py).
 *
 * Semantics for row b with n = clamp(d_lens[b], 0, T) (T when d_lens is NULL) and p = d_probs [B][ld_p] f32; columns at or past n, and
 * whole rows with n = 0, are never read:
 *   1 classes   frame t is HI iff !(p[t] < onset) (NaN counts as speech, as uvad_median_filter), LO iff p[t] < offset, MID otherwise;
 *               offset <= onset, so no frame is both;
 *   2 state     s[-1] = 0; s[t] = 1 on HI, 0 on LO, s[t - 1] on MID;
 *   3 runs      [s_i, c_i) of s on [0, n), exactly as uvad_label_runs_lens;
 *   4 pad       each run becomes [max(s_i - pad_on, 0), min(c_i + pad_off, n));
 *   5 fill      left to right, an interval merges into its predecessor iff start - prev_end <= 0 or start - prev_end < min_off (on the
 *               raw runs: s' - c <= pad_on + pad_off + max(min_off - 1, 0));
 *   6 drop      a merged interval [lo, hi) is kept iff hi - lo >= min_on.
 *   The order is pad, fill, drop.  onset = offset and all four integers 0 give the runs of !(p < onset): uvad_median_filter_lens with
 *   kernel 1, then uvad_label_runs_lens.  pad_on = pad_off = P with min_off <= 1 and min_on = 0 is the merge step of uvad_cuts_table.
 * Outputs: d_iv [B][max_iv][2] int32 {lo, hi} in time order and d_iv_counts [B] int32, the TRUE number of kept intervals: intervals past
 *   max_iv are counted but not stored and later entries are not written (as uvad_label_runs treats max_runs; (T + 1) / 2 always
 *   suffices).  The pair is what uvad_intervals_to_labels reads.  d_labels [B][ld] uint8 (may be NULL): 1 on the union of the row's kept
 *   intervals, 0 elsewhere on [0, n); columns at or past n are not written.  The labels come from the row's full interval list, never
 *   from a truncated d_iv.  d_iv may be NULL when max_iv is 0.
 * Workspace: uvad_binarize_ws_bytes(ctx, B, T) bytes (0 on a bad argument), 16-byte aligned; its contents before the call do not matter.
 * The call allocates nothing, never synchronises and reads the lengths on the device; its grids depend on B and T alone, so a graph
 * captured around it replays for new probabilities and lengths.  Rows of d_probs that all start on a 16-byte boundary (d_probs aligned
 * and ld_p a multiple of 4, or B = 1) are read with 16-byte loads; any other layout works, with 4-byte loads.  No atomics.  A context
 * created without feature / model configuration serves it.
 * Refusals (UVAD_E_ARG, nothing enqueued, uvad_last_error names the word): a NULL cfg, d_probs, d_iv_counts or d_ws; NULL d_iv with
 *   max_iv > 0; onset or offset not finite, or offset > onset; min_on, min_off, pad_on or pad_off outside [0, 2^20]; B < 1; T < 1 or
 *   > 2^30; ld_p < T; ld < T with labels; max_iv < 0; d_ws not 16-byte aligned; B x ceil(T / 2048) above 2^31 - 1; ws_bytes below
 *   uvad_binarize_ws_bytes ("need N bytes"). */
typedef struct {
    float onset;    /* a frame with !(p < onset) turns speech on (NaN counts as speech, as uvad_median_filter) */
    float offset;   /* a frame with p < offset turns speech off; finite, offset <= onset */
    int min_on;     /* frames, 0 .. 2^20: a final interval shorter than this is dropped */
    int min_off;    /* frames, 0 .. 2^20: a pause shorter than this between two intervals is filled */
    int pad_on;     /* frames, 0 .. 2^20, added before every run */
    int pad_off;    /* frames, 0 .. 2^20, added after every run */
} uvad_binarize_cfg;   /* 24 bytes */
size_t uvad_binarize_ws_bytes(const uvad_ctx *, int B, int T);
int uvad_binarize(uvad_ctx *, const float *d_probs, int ld_p, int B, int T, const int32_t *d_lens, const uvad_binarize_cfg *,
                  uint8_t *d_labels, int ld, int32_t *d_iv, int max_iv, int32_t *d_iv_counts, void *d_ws, size_t ws_bytes, void *stream);

/* ---- Live hysteresis endpointing: uvad_binarize's decisions as per-feed events ----------------------------------------------------------
 * The streaming counterpart of uvad_binarize, with the contract of uvad_endpoint_*: whatever way a session's frames are cut into steps,
 * its events and labels, concatenated, are byte-identical to uvad_binarize on the session's whole row.  The configuration is
 * uvad_binarize_cfg with uvad_binarize's validity rules; the step's argument list is uvad_endpoint_step's, so the d_probs / d_counts /
 * d_flags a slot pool step wrote are consumed as they are.  Sessions, flags and n_b = clamp(d_counts[b], 0, ld_in) are exactly those of
 * uvad_endpoint_step: UVAD_SLOT_START drops the old session silently, UVAD_SLOT_END flushes after the step's frames, columns >= n_b and
 * rows with n_b = 0 are never read (NaN there changes no output byte).
 *   The hysteresis state is causal -- s[t] is known the moment frame t arrives -- so the slot keeps no frames, and a START costs no frames
 *   of delay when min_on is 0.  Let D = pad_on + pad_off + max(min_off - 1, 0).  Per slot the state is m, the frames seen; the state bit
 *   s; mode, one of IDLE, SPEECH, PENDING; a confirmed bit; lo, c and the label frontier F.  For each new frame t = m, in order:
 *     1 state bit   s becomes 1 on HI (!(p < onset), NaN included), 0 on LO (p < offset), and is unchanged on MID; compared in f32;
 *     2 mode        IDLE and s = 1: lo = max(t - pad_on, 0), mode = SPEECH, unconfirmed.  SPEECH and s = 0: c = t, mode = PENDING.
 *                   PENDING and s = 1: mode = SPEECH, the run rejoins with no event;
 *     3 close       in PENDING with s = 0 and t >= c + D the interval is closed with hi = c + pad_off (with D = 0 in the frame that set
 *                   c).  If it is confirmed END(hi) is issued; otherwise it vanishes without events: it is shorter than min_on.
 *                   mode = IDLE;
 *     4 confirm     m = t + 1.  If the mode is not IDLE and the interval is unconfirmed, let bound = m in SPEECH and min(c + pad_off, m)
 *                   in PENDING; when bound - lo >= min_on, START(lo) is issued and the interval is confirmed (with min_on = 0 that is
 *                   the frame the run begins in);
 *     5 frontier    labels are final on [0, F).  IDLE: F = max(F, m - pad_on), the new labels are 0.  Confirmed SPEECH: F = m, the new
 *                   labels are 1.  Confirmed PENDING: F = max(F, min(c + pad_off, m)), the new labels are 1.  Unconfirmed: F stays at
 *                   lo.  When an interval closes, its frames [lo, hi) are written as 1 if it was kept and as 0 if it was dropped;
 *     6 END flag    after the frames, n = m: an open interval closes at n, a pending one at min(c + pad_off, n); END is issued iff the
 *                   interval is confirmed; F = n, and the slot holds the empty session again.
 *   Hence a session's events, concatenated, are exactly START(lo_0), END(hi_0), START(lo_1), ... of uvad_binarize's kept interval list
 *   on the whole session, and its finalised labels, concatenated, are uvad_binarize's d_labels row.  START is issued once the interval has
 *   min_on frames the session has seen; END comes D - pad_off + 1 frames after hi.
 *   Outputs per step, all DEVICE memory, as uvad_endpoint_step's; d_ev_counts is required, the others may be NULL:
 *     d_events [B][max_events][2] int32 {kind, frame}, kind 1 = START, 2 = END; d_ev_counts [B] int32 the true number of events of this
 *       step: at most n_b + 1 (one per frame, plus the flush), so max_events = ld_in + 1 always suffices; events beyond max_events are
 *       counted but not stored;
 *     d_active [B] uint8: 0 when idle, 1 while a confirmed interval is open or pending, 2 while an unconfirmed candidate is open or
 *       pending -- the early gate a downstream recogniser may want before min_on is met;
 *     d_labels [B][ld_lab] uint8: the labels finalised by this step, d_lab_counts [B] int32 their number: at most n_b + lag with
 *       lag = uvad_endpoint_hyst_lag = min_on + D (attained), so ld_lab >= ld_in + lag, and d_labels needs d_lab_counts.
 *   With onset = offset = thr, pad_on = pad_off = P, min_on = 0 and min_off <= 1 every step's events, event counts and active byte equal
 *   those of uvad_endpoint_step with kernel 1, pad P, threshold thr.
 *   Frames are int32 and saturate: a session consumes no frames past 2^31 - 1; positions such as c + pad_off are formed in 64 bits.
 *   The configuration lives in the state (a header written by reset): a step carries none, is one launch, allocates nothing, never
 *   synchronises and reads every per-slot quantity from the device, so a graph captured around any step -- alone or in the same capture
 *   as the slot pool step that feeds it -- replays for every later one.  ld_in is at most 2^18 frames per step.  The state is 32 bytes
 *   per slot behind a 256-byte header.  A context created without feature / model configuration serves these calls.
 *   Refusals (UVAD_E_ARG, nothing enqueued, uvad_last_error names the word): uvad_binarize's checks on the cfg; B < 1; ld_in < 1 or
 *   > 2^18; NULL d_probs / d_counts / d_ev_counts / d_state; max_events < 0, or d_events NULL with max_events > 0; d_labels with
 *   ld_lab < ld_in + lag or without d_lab_counts; state_bytes below uvad_endpoint_hyst_state_bytes.  A state never reset, or reset with
 *   another B: UVAD_E_STATE. */
int uvad_endpoint_hyst_lag(const uvad_binarize_cfg *);   /* min_on + D; -1 on a bad cfg */
size_t uvad_endpoint_hyst_state_bytes(const uvad_ctx *, int B, const uvad_binarize_cfg *);   /* 0 on a bad configuration */
int uvad_endpoint_hyst_reset(uvad_ctx *, void *d_state, size_t state_bytes, int B, const uvad_binarize_cfg *, void *stream);
int uvad_endpoint_hyst_step(uvad_ctx *, const float *d_probs, int ld_in, const int32_t *d_counts, const uint8_t *d_flags, int B,
                            void *d_state, size_t state_bytes, int32_t *d_events, int max_events, int32_t *d_ev_counts, uint8_t *d_active,
                            uint8_t *d_labels, int ld_lab, int32_t *d_lab_counts, void *stream);

/* ---- Live speech gate: each feed's speech audio per step, on the device ---------------------------------------------------------------------
 * The streaming counterpart of uvad_cuts_table + uvad_cuts_gather(UVAD_CUTS_SAMPLES), with the endpointers' contract: however a session's
 * samples and labels are cut into steps, the fragments a slot emits, concatenated per cut, are byte-identical to the offline pair run on
 * the whole session's labels and PCM with the same uvad_cuts_cfg (n = the session's labels, S_b = its samples).  It stands behind an
 * endpointer step and hands a recogniser the speech audio, and only that, with no copy of events to the host and no PCM history there.
 *   Sessions: the state holds B slots; after uvad_gate_reset every slot is idle.  d_flags is the slot pools' byte, or NULL:
 *     UVAD_SLOT_START  before this step's input the slot drops whatever session it held -- silently, no closing records -- and a new
 *                      session begins with this step's chunk and labels;
 *     UVAD_SLOT_END    after this step's input the session is flushed (below) and the slot is idle again.  Both bits: a one-step session.
 *   Inputs per step: row b of d_chunk [B][chunk] holds the session's next `chunk` samples of unit_bytes each, copied as bytes (int16 or
 *     f32: a slot pool's own input buffer); columns 0 .. clamp(d_lab_counts[b], 0, ld_lab) - 1 of row b of d_labels [B][ld_lab] hold the
 *     session's next finalised labels -- an endpointer step's d_labels / d_lab_counts, consumed as they are; any non-zero byte counts as
 *     1, as in uvad_cuts_table.  The chunk row, the label row and the count of an idle slot, and label columns past the count, are never
 *     read (NaN or junk there changes no output byte).  ld_lab = 0 feeds samples alone.
 *   Cuts: uvad_cuts_cfg in full, with min_len required to be 0 (dropping a short last piece would need a further hold).  Per slot the
 *     state is A, the samples received; F, the labels received; mode, one of IDLE, OPEN (inside a run), PENDING (a run closed at c); and
 *     the current piece: its first frame f, its index, the samples it has delivered.  The step first commits the chunk (A += chunk), then
 *     takes each label v of frame t = F in order:
 *     1 mode     IDLE and v: f = max(t - pad, 0), mode = OPEN.  OPEN and !v: c = t, mode = PENDING.  PENDING and v: the run rejoins;
 *     2 close    F = t + 1.  In PENDING with !v and t >= c + 2 pad (labels c .. c + 2 pad are final and zero: the median endpointer's
 *                rule) the interval ends at hi = c + pad: after step 3 with g = hi the piece [f, hi) closes if hi > f; mode = IDLE;
 *     3 split    otherwise, outside IDLE, the frames known to lie inside the interval end at g = F (OPEN) or min(c + pad, F) (PENDING);
 *                while max_len > 0 and g - f >= max_len the piece [f, f + max_len) closes and f += max_len: a piece closes in the frame
 *                that completes it, and the next one opens with the first frame known to lie behind it;
 *     4 END flag after the labels, n = F: with g as in 3 (OPEN: n, PENDING: min(c + pad, n)) the piece [f, g) closes if g > f.
 *     A piece [f, f + k) that closes covers samples [max(f hop - lead, 0), min((f + k) hop + tail, A)), exactly uvad_cuts_table's range
 *     when the step carries the END flag (A = S_b).  A piece that closes in a step without END while A < (f + k) hop + tail carries
 *     UVAD_GATE_SHORT: it is shorter than its offline cut.  That cannot happen with a pool's own geometry -- log-mel: lead =
 *     (frame_len - shift) / 2, tail = frame_len - shift - lead; waveform: lead 0, tail R - J -- because frame t spans samples
 *     [t hop - lead, (t + 1) hop + tail), a label exists only for a complete frame, and a piece closes with g <= F, so label g - 1 exists
 *     and A >= g hop + tail.
 *   Emission: cuts in table order and each cut's samples in order, nothing deferred.  Every piece that closes in a step gives one record
 *     with the rest of its samples, up to its end; after the labels (without END) the open piece [f, g) gives one record with its samples
 *     up to min(g hop, A), if there are new ones.  So a step emits at most one record per piece, a piece whose sample range is empty still
 *     emits one (FIRST | LAST, n = 0), and the records of a cut are back to back in offset.
 *   History ring: the slot keeps the last `history` samples it received in a ring in the state (its write position runs on across
 *     sessions).  The step commits the chunk, then reads.  Samples a fragment needs that have left the ring -- positions below A - history
 *     -- are written as zero bytes and the record carries UVAD_GATE_LOST.  uvad_gate_history = chunk + (lag_frames + pad + 1) hop + lead is
 *     a size at which this never happens provided that after every step F >= floor(A / hop) - lag_frames (DESIGN.md 3.20 derives it; behind
 *     a pool lag_frames = lookahead + the endpointer's lag + ceil(tail / hop)).
 *   Outputs per step, all DEVICE memory:
 *     d_out [B][ld_out] units: the step's fragments back to back in record order; units behind them are not written;
 *     d_seg [B][max_seg] uvad_gate_seg: index = the cut's position within the session (uvad_cut.index); flags = UVAD_GATE_FIRST (the
 *       cut's first record) | LAST (its last; n_frames is final) | LOST | SHORT; first_frame, n_frames = the piece's first frame and its
 *       frames so far; offset = the fragment's first sample within the cut; n = its true sample count (saturating at 2^31 - 1);
 *       n_stored = what fitted into the rest of the row: truncation shows as n_stored < n, and the rest is skipped, not deferred;
 *     d_seg_counts [B] int32: the TRUE number of records; records past max_seg are counted but neither stored nor copied (as
 *       uvad_label_runs treats max_runs).  An idle slot's count is 0 and nothing else of it is written.
 *   uvad_gate_max_seg: 2 I + 1 + (max_len ? (ld_lab + 2 pad I) / max_len : 0) with I = (ld_lab + 1) / 2 + 1, the intervals a step can
 *     touch: a max_seg that never overflows (saturating at 2^31 - 1).  uvad_gate_max_out: chunk + (ld_lab + 2 pad I) hop + max_seg x
 *     (lead + tail), an ld_out that never truncates; lost samples are written too, so it does not depend on `history`, which is only
 *     checked.  Both, and uvad_gate_history, return -1 on a bad argument.
 *   Positions are int64; frames are int32 and saturate: a session consumes no labels past 2^31 - 1.  The configuration lives in the state
 *   (a header written by reset; 64 bytes per slot and its ring, rounded up to 16 bytes, behind a 256-byte header): a step carries none, is
 *   one launch of one workgroup per slot, allocates nothing, never synchronises and reads every per-slot quantity from the device; its
 *   grid depends on B alone, so a graph captured around any step -- alone or in a pool's capture behind the endpointer -- replays for
 *   every later one.  Copies are 16 bytes per lane where the output row's alignment allows and one unit at the edges; no atomics.  A
 *   context created without feature / model configuration serves these calls.
 *   Refusals (UVAD_E_ARG, nothing enqueued, uvad_last_error names the word): uvad_cuts_table's checks on the cfg; min_len != 0;
 *   unit_bytes not 2 or 4; history < 1, above 2^31 - 1 or (step) below chunk; B < 1; chunk < 1 or > 2^24; ld_lab < 0; ld_out < 0;
 *   max_seg < 0; NULL d_chunk / d_state / d_seg_counts; NULL d_labels or d_lab_counts with ld_lab > 0; d_out NULL with ld_out > 0; d_seg
 *   NULL with max_seg > 0; state_bytes below uvad_gate_state_bytes.  A state never reset, or reset with another B: UVAD_E_STATE. */
#define UVAD_GATE_FIRST 1
#define UVAD_GATE_LAST  2
#define UVAD_GATE_LOST  4
#define UVAD_GATE_SHORT 8
typedef struct {
    int32_t index, flags, first_frame, n_frames;
    int64_t offset;
    int32_t n, n_stored;
} uvad_gate_seg;   /* 32 bytes */
size_t uvad_gate_state_bytes(const uvad_ctx *, int B, const uvad_cuts_cfg *, int unit_bytes, int64_t history);   /* 0 on a bad configuration */
int64_t uvad_gate_history(const uvad_cuts_cfg *, int lag_frames, int chunk);
int64_t uvad_gate_max_out(const uvad_cuts_cfg *, int ld_lab, int chunk, int64_t history);
int uvad_gate_max_seg(const uvad_cuts_cfg *, int ld_lab);
int uvad_gate_reset(uvad_ctx *, void *d_state, size_t state_bytes, int B, const uvad_cuts_cfg *, int unit_bytes, int64_t history,
                    void *stream);
int uvad_gate_step(uvad_ctx *, const void *d_chunk, int chunk, const uint8_t *d_labels, int ld_lab, const int32_t *d_lab_counts,
                   const uint8_t *d_flags, int B, void *d_state, size_t state_bytes, void *d_out, int64_t ld_out, uvad_gate_seg *d_seg,
                   int max_seg, int32_t *d_seg_counts, void *stream);

/* ---- Live speech gate for fused groups: each cut from its best channel, per step, on the device ------------------------------------------------
 * The streaming counterpart of uvad_cuts_table (on the fused labels) + uvad_fuse_pick + uvad_cuts_gather(UVAD_CUTS_SAMPLES), as
 * uvad_gate_step is of the table + gather: it stands behind uvad_fuse and an endpointer over the groups and emits, per group and step, the
 * speech audio of the group's cuts, each cut taken WHOLE from one member channel.  It replaces the host round trip a multi-microphone
 * caller otherwise pays behind a fused pool (copy events and best bytes out, keep a PCM history per channel, slice there), and nothing in
 * the reference (its multi-channel corpora are fused offline: see uvad_fuse).
 *   Groups: those of the context's uvad_fuse_configure: G groups, N member slots; slot j reads row h_members[j] of d_chunk [B][chunk].
 *     Position p of group g is slot h_group_first[g] + p.  Reset writes G, N and decide_frames into the state's header; a step against a
 *     state whose G / N differ from the context's configuration returns UVAD_E_STATE.  As for uvad_fuse, a failed upload keeps the
 *     validated configuration: every argument refusal below still answers, and reset / step then return UVAD_E_HIP.
 *   Inputs per step: d_chunk [B][chunk] units, the pool's input buffer; d_best [G][ld_best] with d_best_counts [G]: this step's uvad_fuse
 *     d_best and d_glens (the first clamp(count, 0, ld_best) bytes of row g are the group's next best bytes); d_labels [G][ld_lab] with
 *     d_lab_counts [G]: the endpointer's finalised labels, as uvad_gate_step takes them; d_gflags [G] (or NULL: no flags): the group's
 *     session flags, uvad_fuse's OR-ed d_flags_out, with UVAD_SLOT_START / UVAD_SLOT_END as in uvad_gate_step; d_rflags [B] (or NULL: no
 *     check): the pool's per-row flag bytes, for the lockstep check below.  The chunk rows, best row, label row and counts of an idle
 *     group, columns past a count and rows no group names are never read (NaN or junk there changes no output byte).
 *   The rule: the mode machine, pad, max_len, the END flush, SHORT, LOST, the record order and the n / n_stored / offset semantics are
 *     uvad_gate_step's, unchanged, on the group's labels; min_len must be 0.  What is new is the channel and when a piece first speaks:
 *     choice    a piece [f, f + k) -- one uvad_cut -- takes its audio from the member position with the most frames t in
 *               [f, f + min(k, D)), D = decide_frames >= 1, at which best[g][t] equals that position; ties go to the lowest position; no
 *               votes: position 0.  This is uvad_fuse_pick's rule on the cut truncated to its first D frames.  A frame at or past the
 *               best bytes received, or one that has left the best ring, votes for nobody (a best byte at or above the group's size too);
 *     deferral  a piece delivers nothing until its choice is final: until the end of the first step after which g - f >= D, with g the
 *               frames known to lie inside the interval (uvad_gate_step's step 3), or the step in which the piece closes.  Its first
 *               record then carries its whole backlog from max(f hop - lead, 0); later records continue it as uvad_gate_step's do.  Each
 *               piece a max_len split makes chooses for itself.
 *     Because the choice reads frames below f + D only, and a record is made only when those are known, the choice -- and with it every
 *     byte -- does not depend on how the session is cut into steps: a session's fragments concatenated per cut are byte-identical to the
 *     cuts of uvad_cuts_table on the fused labels, each gathered from the audio row of the member the truncated pick names.  With
 *     max_len > 0 and D >= max_len no cut is longer than D and that is uvad_cuts_table -> uvad_fuse_pick -> uvad_cuts_gather; with D = 1
 *     nothing is deferred and the records and sample ranges are uvad_gate_step's on the same labels.  (DESIGN.md 3.23 proves all three.)
 *   Preconditions for "no UVAD_GATE_LOST, every frame votes" with the sizes below (both hold behind a fused pool): after every step
 *     F >= floor(A / hop) - lag_frames (uvad_gate_step's), and F <= Fb <= floor(A / hop), with A the samples, F the labels and Fb the best
 *     bytes the session has received.
 *   State: one PCM ring of `history` units per member slot (a row that sits in several groups is kept once per slot) and one best ring of
 *     `best_history` bytes per group, each rounded up to 16 bytes, behind a 256-byte header and 96 bytes per group.
 *     uvad_gate_group_history = chunk + (lag_frames + pad + D) hop + lead (uvad_gate_history at D = 1) and uvad_gate_group_best_history =
 *     ceil(chunk / hop) + lag_frames + pad + D are sizes at which, under the preconditions, no sample is lost and every frame of a choice
 *     window is still in its ring: a piece first delivered in a step has f >= F_before - pad - D + 1.  uvad_gate_group_max_out =
 *     uvad_gate_max_out + D hop (the one deferred piece adds its backlog) is an ld_out that never truncates; uvad_gate_max_seg holds as it
 *     is (deferral only removes records).  The three helpers return -1 on a bad argument, uvad_gate_group_state_bytes 0 (also before
 *     uvad_fuse_configure).
 *   Outputs: d_out [G][ld_out], d_seg [G][max_seg] and d_seg_counts [G] exactly as uvad_gate_step's with B = G.  Bits 8 .. 15 of
 *     uvad_gate_seg.flags hold the chosen member position, UVAD_GATE_CHANNEL(flags), the same on every record of a cut.
 *   Lockstep: a group's members must be stepped together.  With d_rflags, a group whose members' bytes differ in a step is out of
 *     lockstep: from that step until the session's END every record carries UVAD_GATE_UNSYNC.  The gate otherwise acts on d_gflags as given.
 *   One launch of one workgroup per group per step; it allocates nothing, never synchronises and uses no atomics; its grid depends on the
 *   configuration alone, so a graph captured around a step -- alone or in a pool's capture behind the endpointer -- replays for later ones.
 *   Refusals (UVAD_E_ARG, nothing enqueued, uvad_last_error names the word): uvad_gate_reset's checks on the cfg (min_len != 0 among them),
 *   unit_bytes and history; decide_frames outside [1, 2^24] (the largest max_len uvad_cuts_table accepts); best_history < 1 or above
 *   2^31 - 1; chunk < 1 or > 2^24; ld_lab, ld_best, ld_out or max_seg < 0; NULL d_chunk / d_state / d_seg_counts; NULL d_labels or
 *   d_lab_counts with ld_lab > 0; NULL d_best or d_best_counts with ld_best > 0; d_out NULL with ld_out > 0; d_seg NULL with max_seg > 0;
 *   B not above the largest configured member index; history below chunk (step); state_bytes below uvad_gate_group_state_bytes.
 *   UVAD_E_STATE: any call before uvad_fuse_configure; a step on a state never reset, or reset under another G / N. */
#define UVAD_GATE_UNSYNC 16
#define UVAD_GATE_CHANNEL(flags) (((flags) >> 8) & 0xff)
int64_t uvad_gate_group_history(const uvad_cuts_cfg *, int lag_frames, int chunk, int decide_frames);
int uvad_gate_group_best_history(const uvad_cuts_cfg *, int lag_frames, int chunk, int decide_frames);
int64_t uvad_gate_group_max_out(const uvad_cuts_cfg *, int ld_lab, int chunk, int decide_frames);
size_t uvad_gate_group_state_bytes(const uvad_ctx *, const uvad_cuts_cfg *, int unit_bytes, int64_t history, int best_history);
int uvad_gate_group_reset(uvad_ctx *, void *d_state, size_t state_bytes, const uvad_cuts_cfg *, int unit_bytes, int64_t history,
                          int best_history, int decide_frames, void *stream);
int uvad_gate_group_step(uvad_ctx *, const void *d_chunk, int chunk, int B, const uint8_t *d_best, int ld_best, const int32_t *d_best_counts,
                         const uint8_t *d_labels, int ld_lab, const int32_t *d_lab_counts, const uint8_t *d_gflags, const uint8_t *d_rflags,
                         void *d_state, size_t state_bytes, void *d_out, int64_t ld_out, uvad_gate_seg *d_seg, int max_seg,
                         int32_t *d_seg_counts, void *stream);

/* ---- Head fine-tuning on the device: loss gradient, backward pass, Adam ------------------------------------------------------------------
 * The LSTM stack stays frozen; the feed-forward layers and the classifier learn from the last LSTM layer's output x0 [B][T][D0]
 * (D0 = hidden x directions: what uvad_get_taps writes to d_lstm_out, which a caller may cache across epochs).  Replaces, for that
 * slice of the model, VadModel.training_step / _common_step (src/engines/vad_engine.py:247-278: the head expression of
 * PyanNet2.forward, F.leaky_relu(linear(x)) and sigmoid(classifier(x)), F.binary_cross_entropy with the mean over the frames present,
 * src/utils/loss.py:56-89, and autograd's backward pass through them) and configure_optimizers (:280: torch.optim.Adam, no weight decay).
 * Gradient clipping, weight decay, learning-rate schedules and the skip of a non-finite step are uvad_optim_step, below (it replaces the
 * _apply calls); DDP is not here.  Gradients into a SincNet front end are uvad_sincnet_train_*, below (dropout between LSTM layers is a stage of
 * uvad_lstm_train_*, below; the head has none in the reference either); d_grad_x is where the backward pass through
 * the LSTM stack starts (uvad_lstm_train_backward below takes it as d_dy).
 *
 * With s = leaky_slope, a_0 = x0, a_l = leaky_relu(a_{l-1} W_l^T + b_l, s) for l = 1 .. L, z = a_L . w_c + b_c, p = sigmoid(z), a frame
 * (b, t) is valid iff t < len_b = clamp(d_lens[b], 0, T) (T when d_lens is NULL).  A valid frame with label y = (d_gt != 0) and weight w
 * (d_fw, 1 when NULL) adds  w * -(y max(log p, -100) + (1 - y) max(log(1 - p), -100))  (f64, from the f32 p) to the loss sum and has
 *   dz = w * ((p - y) * (q / max(q, 1e-12))),  q = p * (1 - p)
 * every operation one f32 rounding in that order (autograd's gradient of BCE on sigmoid(z), saturation included: 0 where p rounds to 0
 * or 1).  Frames past a length have dz = 0, add nothing, and are never read in d_x, d_gt, d_fw or d_dz.  A non-NULL d_dz [B][ld_dz]
 * replaces the loss-derived dz (the caller's own loss): d_gt and d_fw are then ignored and may be NULL, and no loss is accumulated.
 * The backward pass is d_L = (dz w_c) * leaky'(a_L), dW_l = sum_n d_l[n]^T a_{l-1}[n], db_l = sum_n d_l[n],
 * d_{l-1} = (d_l W_l) * leaky'(a_{l-1}) with leaky' = 1 where the stored activation is > 0 and s elsewhere.
 *
 * uvad_head_train_grad runs the forward pass with the STATE's f32 master weights (not the context's packed ones), and ADDS the
 *   gradients of the summed loss into the state's accumulator, the loss into its f64 sum and the valid frames into its count; any
 *   number of calls (micro-batches) may precede a step.  d_probs [B][ld_p] (may be NULL) receives p at valid frames, columns past a
 *   length are not written; d_grad_x [B][T][D0] (may be NULL) receives dL/dx0 of the summed loss and +0 at frames past a length.
 *   After the call the workspace's first 16 bytes hold {double loss sum, uint64 valid frames} of THAT call.
 *   All products run on the exact f32 matrix instruction (a k-ordered fma chain); the frames are reduced per segment of `segment` frames
 *   (flat index b T + t) and the partials folded in segment order: no floating-point atomics, the same calls give the same bits.
 * uvad_head_train_apply: one Adam step with g = accumulator / count, then the accumulator, loss sum and count are zeroed and t advances.
 *   A zero count does nothing.  The bias corrections c_t = 1 - beta^t are kept in the state as f32 values advanced once per step,
 *   c <- c beta + (1 - beta) from 0, so one captured graph serves every step (tests/head_train_ref.py restates the step operation by
 *   operation).  The complement is kept, not the product beta^t: 1 - (f32 nearest 0.999)^t is 1.3e-5 off at every t.
 * grad and apply allocate nothing, never synchronise and read lengths and counts from the device: any sequence of them can be captured
 *   in one graph and replayed with new data.
 * uvad_head_train_read copies out (device memory): which = UVAD_HEAD_TRAIN_MASTERS / _GRAD / _M / _V: the P floats of the trainable
 *   tensors packed in state_dict order -- linear.0.weight [H][D0], linear.0.bias [H], linear.l.weight [H][H], linear.l.bias [H], ...,
 *   classifier.weight [1][K_L], classifier.bias [1] (K_L = H, or D0 when lin_layers is 0), P = uvad_head_train_param_count;
 *   which = UVAD_HEAD_TRAIN_SCALARS: UVAD_HEAD_TRAIN_SCALAR_WORDS 32-bit words: [0 .. 1] the accumulated loss sum (bits of a double, low
 *   word first), [2 .. 3] the accumulated valid frames (uint64), [4 .. 5] t (uint64), [6] 1 - beta1^t, [7] 1 - beta2^t (f32).
 * uvad_head_train_commit synchronises the device, then feeds the masters through uvad_set_weight + uvad_finalize: from then on
 *   uvad_classify and every stream of THIS context serve the adapted head.  As for uvad_finalize: graphs captured earlier hold the old
 *   weight buffers, which are freed here -- capture them again; contexts that shared the upload block keep the old weights.
 * State: uvad_head_train_state_bytes (0 before configure).  Workspace: uvad_head_train_ws_bytes(ctx, B, T) (0 on a bad argument): the
 *   kept activations lin_layers x B T x lin_hidden floats, two gradient buffers of B T x lin_hidden, ceil(B T / segment) x P partials.
 * Served: D0 any multiple of 32 up to 2048; lin_layers 0 .. 4; lin_hidden a multiple of 32 in 32 .. 256; leaky_slope > 0 (the factor
 *   leaky' is read from the sign of the stored activation).  uvad_head_train_configure returns UVAD_E_UNSUPPORTED for any other head
 *   that uvad_create accepts.  PyanNet2 and PyanNet (SincNet front end) contexts alike.
 * Refusals (nothing enqueued).  UVAD_E_ARG: NULL cfg / d_x / d_state / d_ws / d_out; both d_gt and d_dz NULL; lr not finite or <= 0;
 *   beta1 / beta2 outside [0, 1) or not finite; eps not finite or <= 0; segment not 0 or a multiple of 32 in 32 .. 16384; B < 1; T < 1;
 *   B T > 2^24 or more than 65535 segments; ld_gt / ld_fw / ld_dz / ld_p below T (for the pointers given); state_bytes or ws_bytes below the helpers; which outside
 *   0 .. 4.  UVAD_E_STATE: a context without a model; no uvad_head_train_configure yet; a context that is not finalized (reset,
 *   commit); a state that was never reset, or reset under another head shape.  UVAD_E_UNSUPPORTED: see above. */
#define UVAD_HEAD_TRAIN_MASTERS 0
#define UVAD_HEAD_TRAIN_GRAD 1
#define UVAD_HEAD_TRAIN_M 2
#define UVAD_HEAD_TRAIN_V 3
#define UVAD_HEAD_TRAIN_SCALARS 4
#define UVAD_HEAD_TRAIN_SCALAR_WORDS 8
typedef struct {
    float lr, beta1, beta2, eps;
    int segment;                             /* frames per gradient partial, 0 = default (2048) */
} uvad_head_train_cfg;
int uvad_head_train_configure(uvad_ctx *, const uvad_head_train_cfg *);
int64_t uvad_head_train_param_count(const uvad_ctx *);   /* P; 0 before uvad_head_train_configure */
size_t uvad_head_train_state_bytes(const uvad_ctx *);
size_t uvad_head_train_ws_bytes(const uvad_ctx *, int B, int T);
int uvad_head_train_reset(uvad_ctx *, void *d_state, size_t state_bytes, void *stream);
int uvad_head_train_grad(uvad_ctx *, const float *d_x, int B, int T, const int32_t *d_lens, const uint8_t *d_gt, int ld_gt,
                         const float *d_fw, int ld_fw, const float *d_dz, int ld_dz, float *d_probs, int ld_p, float *d_grad_x,
                         void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);
int uvad_head_train_apply(uvad_ctx *, void *d_state, size_t state_bytes, void *stream);
int uvad_head_train_read(uvad_ctx *, const void *d_state, size_t state_bytes, int which, float *d_out, void *stream);
int uvad_head_train_commit(uvad_ctx *, const void *d_state, size_t state_bytes);

/* ---- LSTM training on the device: forward with kept activations, backpropagation through time, Adam ---------------------------------------
 * Layers first_layer .. num_layers - 1 of the context's LSTM stack learn; the layers below stay frozen and run through the inference
 * kernels as before (their output, or the features themselves when first_layer is 0, is this block's input and may be cached across
 * epochs).  Together with uvad_head_train_* this is VadModel.training_step / configure_optimizers (src/engines/vad_engine.py:247-281)
 * for everything above the front end: nn.LSTM on pack_padded_sequence rows, autograd's backward pass through it, torch.optim.Adam.
 * Clipping, weight decay and schedules are uvad_optim_step, below; DDP is not here; d_grad_in of a PyanNet is what uvad_sincnet_train_backward takes.  Dropout between the trainable layers is
 * (uvad_lstm_train_set_dropout, defined below); the frozen prefix runs in eval mode.
 *
 * d_x_in [B][T][Din] is the dense f32 input of layer first_layer (Din = in_dim when first_layer is 0, else hidden x directions);
 * d_y [B][T][hidden x directions] the top layer's output computed with the STATE's f32 master weights: what uvad_head_train_grad takes as
 * d_x; d_dy the head's d_grad_x (the gradient of the summed loss); d_grad_in [B][T][Din] (may be NULL) dL/dx_in.  len_b =
 * clamp(d_lens[b], 0, T) (T when d_lens is NULL).  d_y and d_grad_in are +0 at frames past a length, and such frames are never read in
 * d_x_in or d_dy.
 * Forward, per layer and direction: nn.LSTM's cell -- gate order i, f, g, o, zero initial state, the backward direction starting at
 *   len_b - 1 -- keeping i, f, g, o after their nonlinearities, c_t and h_{t-1} in the workspace, whose header records B and T.
 * Backward, per step in reverse time for each direction, with dh = dy_t + dh_rec:  do = dh tanh(c_t);
 *   dc = dh o (1 - tanh^2 c_t) + dc_rec;  di = dc g, dg = dc i, df = dc c_{t-1};  dpre = {di i (1 - i), df f (1 - f), dg (1 - g^2),
 *   do o (1 - o)};  dc_rec <- dc f;  dh_rec <- dpre W_hh.  dW_ih = sum dpre^T x, dW_hh = sum dpre^T h_prev (the previous step's h in that
 *   direction's own order, +0 at its first step), db_ih = db_hh = sum dpre (the same bits), d_in = dpre W_ih summed over the directions:
 *   the next lower trainable layer's dy, and at first_layer d_grad_in.  The gradients are ADDED into the state's accumulator and the call's
 *   valid frames into its count, so that uvad_lstm_train_apply divides by the count uvad_head_train_apply divides by.  The kernels check
 *   the workspace header on the device: a backward call whose (B, T) is not that of the forward call that filled the workspace writes nothing.
 *   All time-parallel products run on the head's exact f32 tile kernel, per segment of `segment` frames folded in segment order; the
 *   recurrences sum in a fixed order: no floating-point atomics, the same calls give the same bits.
 * uvad_lstm_train_apply, _read and _commit mean what the head's mean (the same Adam step, restated in tests/head_train_ref.py; `which` is
 *   UVAD_HEAD_TRAIN_MASTERS / _GRAD / _M / _V / _SCALARS).  The P = uvad_lstm_train_param_count floats are packed in state_dict order,
 *   per layer k = first_layer .., forward then _reverse: lstm.weight_ih_l{k} [4 hidden][in], weight_hh_l{k} [4 hidden][hidden],
 *   bias_ih_l{k}, bias_hh_l{k} [4 hidden]; bias_ih and bias_hh are separate Adam tensors.  Commit synchronises the device, then feeds the
 *   masters through uvad_set_weight + uvad_finalize, with the consequences uvad_head_train_commit names.
 *   An LSTM state's scalar record has UVAD_LSTM_TRAIN_SCALAR_WORDS = 10 words: the head's eight, then [8 .. 9] the dropout draw ordinal
 *   (uint64, low word first); d_out must hold ten words for which = UVAD_HEAD_TRAIN_SCALARS.
 * uvad_lstm_train_reset copies the masters from the context's host tensors: it synchronises the stream and is not for graph capture.
 *   forward, backward and apply allocate nothing and never synchronise: forward -> uvad_head_train_grad -> backward -> both applies can
 *   be captured as one graph and replayed with new data.
 * Served: hidden 64 or 128; one or two directions; Din a multiple of 4 up to 2048; up to 8 trainable layers; B T <= 2^24; segment as the
 *   head's.  uvad_lstm_train_configure returns UVAD_E_UNSUPPORTED for anything else.
 * Refusals (nothing enqueued).  UVAD_E_ARG: NULL cfg / d_x_in / d_y / d_dy / d_state / d_ws / d_out; d_state or d_ws not 16-byte aligned
 *   (forward, backward); lr, beta1, beta2, eps, segment as the head's; first_layer outside [0, num_layers); B < 1; T < 1; B T > 2^24 or more than 65535 segments; state_bytes or ws_bytes below
 *   the helpers; which outside 0 .. 4.  UVAD_E_STATE: a context without a model; no uvad_lstm_train_configure yet; a context that is not
 *   finalized (reset, commit); a state that was never reset, or reset under another shape.
 *
 * Dropout between the trainable layers: nn.LSTM(dropout = p) in training mode.  uvad_lstm_train_set_dropout(ctx, p, seed) sets what every
 *   later uvad_lstm_train_forward of the context applies; a new context has p = 0, and uvad_lstm_train_configure leaves the setting
 *   alone.  With p = 0 forward and backward launch the kernels they launched before this stage existed and write nothing into the state.
 *   The mask is a pure function of its coordinates, never stored; forward and backward each regenerate it.
 *   Generator: Philox4x32-10 (Salmon et al., the Random123 definition): multipliers 0xD2511F53, 0xCD9E8D57, Weyl constants 0x9E3779B9,
 *     0xBB67AE85, ten rounds, the key bumped after each round.  counter (0,0,0,0), key (0,0) gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 *   Coordinates, for the output of absolute layer k at frame n = b T + t and column j in [0, hidden x directions):
 *     counter = (n, (k << 16) | (j >> 2), draw_lo, draw_hi), key = (seed_lo, seed_hi); the element uses output word j & 3, so one call
 *     serves four adjacent columns.
 *   Decision: thr = (uint32) floor((double)p 2^32) (p = 0.5: 0x80000000; f32 0.3: 1288490240), scale = 1.0f / (1.0f - p) in IEEE f32;
 *     the element is kept iff word >= thr; a kept value is fl(v scale), one f32 rounding; a dropped value is +0, chosen by a select, so
 *     a NaN or -0 at a dropped position comes out +0.
 *   Where: forward, the input of trainable layer k + 1 is the masked, scaled output of layer k for first_layer <= k < num_layers - 1;
 *     backward, the dy of layer k is the masked, scaled d_in of layer k + 1 with the same mask.  d_y (the top layer's output) and
 *     d_x_in are never dropped.  Frames past a length stay +0.
 *   Draw ordinal: a 64-bit count at byte 56 of the state (zeroed by reset).  A forward call with thr > 0 takes draw = the count and
 *     advances it by one, on the device, in a single thread of its first kernel, and records the call's values in the workspace header:
 *     draw u64 at byte 16, thr u32 at byte 24, scale f32 at byte 28, seed u64 at byte 32.  A forward call with thr == 0 leaves the count
 *     alone and writes only thr = 0 at byte 24.  thr, scale and seed are launch arguments of the forward call, so a captured graph holds
 *     them, and every replay draws a fresh mask.  The backward call takes all four values from the workspace header only: a setting
 *     changed to another p > 0 or seed between forward and backward does not break the pair, and micro-batches within one step get
 *     different masks.  (The host enqueues the backward stage when the context's p is above 0 or its last forward call's was; switching
 *     to p = 0 AND running a p = 0 forward call on another workspace in between is the one order that loses a pending backward's mask.)
 *   uvad_lstm_train_set_dropout refuses with UVAD_E_ARG: NULL context; p not finite, < 0 or >= 1; UVAD_E_STATE: a context without a
 *     model; no uvad_lstm_train_configure yet.  uvad_lstm_train_ws_bytes and _state_bytes do not depend on the setting.
 * uvad_dropout_apply is the same mask function as a stand-alone call without a context: d_out [rows][cols] = keep ? d_x scale : +0, with
 *   frame n = the row and k = layer; in place when d_out == d_x.  For input dropout on cached features, and to pin the mask bit for
 *   bit.  UVAD_E_ARG: a NULL pointer; pointers not 16-byte aligned; cols not a multiple of 4 in [4, 2048]; rows outside [1, 2^24]; layer
 *   outside [0, 65535]; p not finite, < 0 or >= 1. */
typedef struct {
    float lr, beta1, beta2, eps;
    int segment;                             /* frames per gradient partial, 0 = default (2048) */
    int first_layer;                         /* layers first_layer .. num_layers - 1 learn */
} uvad_lstm_train_cfg;
#define UVAD_LSTM_TRAIN_SCALAR_WORDS 10
int uvad_lstm_train_configure(uvad_ctx *, const uvad_lstm_train_cfg *);
int64_t uvad_lstm_train_param_count(const uvad_ctx *);   /* P; 0 before uvad_lstm_train_configure */
size_t uvad_lstm_train_state_bytes(const uvad_ctx *);
size_t uvad_lstm_train_ws_bytes(const uvad_ctx *, int B, int T);
int uvad_lstm_train_reset(uvad_ctx *, void *d_state, size_t state_bytes, void *stream);
int uvad_lstm_train_forward(uvad_ctx *, const float *d_x_in, int B, int T, const int32_t *d_lens, float *d_y, void *d_state,
                            size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);
int uvad_lstm_train_backward(uvad_ctx *, const float *d_x_in, const float *d_dy, int B, int T, const int32_t *d_lens, float *d_grad_in,
                             void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);
int uvad_lstm_train_apply(uvad_ctx *, void *d_state, size_t state_bytes, void *stream);
int uvad_lstm_train_read(uvad_ctx *, const void *d_state, size_t state_bytes, int which, float *d_out, void *stream);
int uvad_lstm_train_commit(uvad_ctx *, const void *d_state, size_t state_bytes);
int uvad_lstm_train_set_dropout(uvad_ctx *, float p, uint64_t seed);
int uvad_dropout_apply(const float *d_x, float *d_out, int64_t rows, int cols, int layer, uint64_t draw, float p, uint64_t seed, void *stream);

/* ---- SincNet training on the device: forward with kept activations, the backward pass, Adam ----------------------------------------------
 * The front end of PyanNet (src/models/blocks/sincnet.py:33-103) learns: with uvad_lstm_train_* and uvad_head_train_* this is
 * VadModel.training_step / configure_optimizers for the waveform model.  d_dfeats is what uvad_lstm_train_backward writes as d_grad_in:
 * the gradient of the SUMMED loss with respect to d_feats.  Dense batches only: B rows of the same S samples, T =
 * uvad_sincnet_num_frames(S); per-row sample counts (uvad_sincnet_lens) are not trained.
 *
 * Stage s = 0, 1, 2 has L_s conv positions and Lp_s = L_s / 3 pooled positions; the 0 .. 2 conv positions past 3 Lp_s take part in nothing.
 * Forward, from the STATE's f32 masters (not the context's packed weights):
 *   the bank F [n_filters][kernel_size] from low_hz_ / band_hz_ as ParamSincFB.filters() defines it (sample rate 16000, min_low_hz =
 *     min_band_hz = 50; low = 50 + |low_hz_|, high = clamp(low + 50 + |band_hz_|, 50, 8000), band = high - low; cos filter c and sin filter
 *     c + n_filters / 2 share parameter c), evaluated in double from the f32 masters and the module's f32 buffers window_ / n_, rounded
 *     once to f32.  It lives in the state behind the Adam block, and commit serves a bank built by this very kernel;
 *   per row the biased variance over the S samples and eps, xn = g xhat + b0 (g, b0 = wav_norm1d.weight, .bias);
 *   u = conv(a_in) (+ bias for s >= 1), for s = 0 u <- |u|;  p[l] = max(u[3 l .. 3 l + 2]), the LOWEST index winning a tie;
 *   mean and rstd = 1 / sqrt(var + eps) per (b, c) over l < Lp_s (biased);  xhat = (p - mean) rstd, z = gamma xhat + beta, a_out = leaky_relu(z).
 *   Kept in the workspace: p; one byte per pooled element (bits 0 .. 1 the winner's index, stage 0 also bits 2 .. 3: 1 the winning conv
 *   output was > 0, 2 it was < 0, 0 it was +-0); mean, rstd; the row statistics.  a_out and xhat are recomputed; the pre-pool conv output is
 *   not kept.  The workspace header records (B, S) and a magic word (xor the high word of S).  d_feats [B][T][c3] is the last a_out.
 * Backward, stages 2 down to first_stage:  dz = d_a_out (z > 0 ? 1 : slope);  d gamma_c = sum_{b,l} dz xhat, d beta_c = sum_{b,l} dz;
 *   dxhat = dz gamma;  dp = rstd (dxhat - mean_l(dxhat) - xhat mean_l(dxhat xhat));  du[3 l + winner] = dp, 0 at the other two positions
 *   and past 3 Lp_s; stage 0 multiplies by the kept sign, sign(+-0) = 0 as torch.abs's gradient.  Stages 1, 2: dbias_co = sum du,
 *   dW[co][ci][k] = sum_{b,t} du[co][t] a_in[ci][t + k], d_a_in[ci][j] = sum_{co,k} du[co][j - k] W[co][ci][k] (the next lower stage's d_a_out).
 *   Stage 0 (no gradient for the waveform):  G[c][k] = sum_{b,t} du[c][t] xhat[b][stride t + k], D[c] = sum_{b,t} du[c][t], then
 *   dF = g G + b0 D, dg = sum_{c,k} F G, db0 = sum_c D[c] sum_k F[c][k], and d low_hz_, d band_hz_ by the chain rule through filters() in
 *   double: torch.abs's sign(0) = 0, torch.clamp passes a gradient only where min <= v <= max.
 *   The weight-gradient contractions run in the PLAIN form: k over the conv positions t < 3 Lp_s of every row (flat b 3 Lp_s + t), du formed
 *   from dp and the winner byte while staging, per segment of `segment` positions folded in segment order.  All contractions are exact f32
 *   on v_mfma_f32_32x32x2_f32; the per-(b, c) sums run in double, lanes folded in a fixed order.  No floating-point atomics: the same calls
 *   give the same bits.  The gradients are ADDED into the state's accumulator and the call's B T frames into its count, the count the head
 *   and the LSTM divide by.  Every backward kernel checks the workspace header on the device: under a (B, S) that is not the forward
 *   call's it writes nothing.
 * Stages first_stage .. 2 learn, in the sense of the LSTM's first_layer.  Stage 0 owns wav_norm1d.*, conv1d.0.filterbank.{low_hz_,
 *   band_hz_} and norm1d.0.*; stage s >= 1 owns conv1d.s.* and norm1d.s.*.  Frozen stages run in the training forward with the state's copy
 *   of their tensors (a frozen stage 0: the same bank from the band edges when the context has them, so d_feats do not depend on
 *   first_stage; else the bank given as sincnet.conv1d.0.filters); they get no gradient and the backward walk stops above.
 *   The P floats are packed in state_dict order restricted to the learning tensors: wav_norm1d.weight, .bias; conv1d.0.filterbank.low_hz_,
 *   band_hz_; conv1d.1.weight, .bias; conv1d.2.weight, .bias; norm1d.0.weight, .bias; norm1d.1.*; norm1d.2.*.  P = 42602 / 42360 / 18180
 *   for first_stage 0 / 1 / 2 on the reference geometry.
 * apply and read are the head's (torch.optim.Adam, no weight decay -- clipping, decay and schedules are uvad_optim_step, below;
 *   tests/head_train_ref.py); which = UVAD_SINCNET_TRAIN_FILTERS reads the
 *   n_filters x kernel_size bank of the last forward call.
 * reset copies the masters from the context's host tensors and synchronises: not for graph capture.  The band edges arrive through
 *   uvad_set_weight as sincnet.conv1d.0.filterbank.low_hz_ / .band_hz_ ([n_filters / 2][1] or [n_filters / 2]); they are optional for
 *   inference, and reset with stage 0 learning and no band edges returns UVAD_E_STATE.  sincnet.conv1d.0.filterbank.window_ / .n_
 *   ([kernel_size / 2], the module's buffers) are taken when given and restated on the host otherwise.
 * commit synchronises, rebuilds the state's bank from the masters as they stand (so the bank served matches the committed band edges, also
 *   right after an apply; the one write a commit makes to the state), feeds the masters through uvad_set_weight and that bank as
 *   sincnet.conv1d.0.filters, then calls uvad_finalize, with the consequences uvad_head_train_commit names.
 * forward, backward and apply allocate nothing and never synchronise: a whole step can be captured as one graph.
 * Served: the geometries uvad_sincnet_configure accepts with leaky_slope <= 1 (stage 0 learning: kernel_size odd); 1 <= B <= 65535; S with
 *   at least one frame; B L_0 <= 2^31 - 1; at most 65535 segments.  Otherwise uvad_sincnet_train_configure returns UVAD_E_UNSUPPORTED.
 * Refusals (nothing enqueued).  UVAD_E_ARG: NULL cfg / d_wav / d_feats / d_dfeats / d_state / d_ws / d_out; d_state or d_ws not 16-byte
 *   aligned (forward, backward); lr, beta1, beta2, eps, segment as the head's; first_stage outside [0, 2]; B or S out of range, S without a
 *   frame; state_bytes or ws_bytes below the helpers; which outside 0 .. 5.  UVAD_E_STATE: a context without a model or without a SincNet
 *   stage; no uvad_sincnet_train_configure yet; a context that is not finalized (reset, commit); a state never reset, or reset under another
 *   shape. */
#define UVAD_SINCNET_TRAIN_FILTERS 5
typedef struct {
    float lr, beta1, beta2, eps;
    int segment;                             /* conv positions per gradient partial, 0 = default (2048) */
    int first_stage;                         /* stages first_stage .. 2 learn */
} uvad_sincnet_train_cfg;
int uvad_sincnet_train_configure(uvad_ctx *, const uvad_sincnet_train_cfg *);
int64_t uvad_sincnet_train_param_count(const uvad_ctx *);   /* P; 0 before uvad_sincnet_train_configure */
size_t uvad_sincnet_train_state_bytes(const uvad_ctx *);
size_t uvad_sincnet_train_ws_bytes(const uvad_ctx *, int B, int64_t S);
int uvad_sincnet_train_reset(uvad_ctx *, void *d_state, size_t state_bytes, void *stream);
int uvad_sincnet_train_forward(uvad_ctx *, const float *d_wav, int B, int64_t S, float *d_feats, void *d_state, size_t state_bytes,
                               void *d_ws, size_t ws_bytes, void *stream);
int uvad_sincnet_train_backward(uvad_ctx *, const float *d_wav, const float *d_dfeats, int B, int64_t S, void *d_state, size_t state_bytes,
                                void *d_ws, size_t ws_bytes, void *stream);
int uvad_sincnet_train_apply(uvad_ctx *, void *d_state, size_t state_bytes, void *stream);
int uvad_sincnet_train_read(uvad_ctx *, const void *d_state, size_t state_bytes, int which, float *d_out, void *stream);
int uvad_sincnet_train_commit(uvad_ctx *, const void *d_state, size_t state_bytes);

/* ---- The joint optimizer step on the device: gradient clipping, weight decay, learning-rate table, skipped steps, resume -----------------
 * uvad_optim_step replaces the _apply calls of the training states it is given (head, LSTM, SincNet; any may be NULL, not all): what
 * torch.nn.utils.clip_grad_norm_ over ALL parameters, torch.optim.Adam(weight_decay=) or AdamW, an lr scheduler stepped once per
 * optimizer step, and Lightning's skipped step (the reference's _common_step returns None on a NaN loss, src/engines/vad_engine.py:275) do
 * around configure_optimizers.  Like grad and apply it allocates nothing and never synchronises, and it reads every count and the step
 * index from the device: forward -> head grad -> backward(s) -> uvad_optim_step is one graph that replays for every step.  DDP is not here.
 *
 * A state TAKES PART iff it is given, its header carries its family's magic word and parameter count, and its frame count is not 0.  A
 *   state that does not take part adds nothing to the norm and nothing in it is written; when no state takes part nothing is written at all.
 * Step, every operation one f32 rounding in this order, no fused multiply-add (tests/optim_ref.py restates it):
 *   g_j = fl(acc_j / (float)frames) per parameter of a state that takes part;
 *   S = sum (double)g_j (double)g_j (each product exact).  Order: the parameters of a state in chunks of 4096; within a chunk lane l of 256
 *     adds elements l, l + 256, ..., l + 3840 in that order from +0, then lane l += lane l + o for o = 128, 64, ..., 1; the chunk sums are
 *     added in chunk order into one running sum, the states in the order head, LSTM, SincNet.  No atomics: the same calls give the same bits.
 *   norm = (float)sqrt(S);  coef = max_norm > 0 ? fminf(1, max_norm / (norm + 1e-6f)) : 1  (clip_grad_norm_'s expression);
 *   lr_t = table[min(t, n_lr - 1)], t the optim state's count of applied steps: any schedule is an uploaded table, the device only indexes
 *     (the idiom of uvad_mix's amplitude table), so it is bit-defined; uvad_optim_set_lr_table rewrites it between steps without re-capture;
 *   skip_nonfinite and S not finite: every participating state's accumulator, loss sum and frame count are zeroed, the optim state's
 *     `skipped` advances, and no master, m, v, t, bc1 or bc2 of any state changes, nor the optim state's t;
 *   otherwise, with lr_k = fl(lr_t lr_scale[k]) for family k:  g = fl(g coef);  weight_decay > 0, L2: g = fl(g + fl(wd w));  AdamW:
 *     w = fl(w fl(1 - fl(lr_k wd)));  then uvad_head_train_apply's update with lr_k and the header update of apply (t, bc1, bc2 advance, the
 *     sums are zeroed), and the optim state's t advances once.  Mixing _apply and uvad_optim_step on one state is well defined.
 *   With max_norm = 0, weight_decay = 0, lr_scale = 1 and a one-entry table holding the family's lr (and its betas and eps) the step leaves
 *   the bytes the three _apply calls leave.
 * uvad_optim_reset uploads the configuration and the table, zeroes t and skipped; it synchronises the stream and is not for graph capture, nor
 *   is uvad_optim_set_lr_table (n_lr at most the reset's).  1 - beta is formed as the families' configure forms it.
 * uvad_optim_read copies UVAD_OPTIM_RECORD_WORDS 32-bit words to d_out (device memory): [0] norm, [1] coef (0 for a skipped step), [2] lr_t
 *   of the last step that had a participant (f32), [3] bit k set: family k (0 head, 1 LSTM, 2 SincNet) took part, [4 .. 5] t, [6 .. 7] skipped
 *   (uint64, low word first).  uvad_optim_write puts such a record (device memory) back.
 * uvad_head_train_write / uvad_lstm_train_write / uvad_sincnet_train_write mirror the _read calls, d_in in device memory: which =
 *   UVAD_HEAD_TRAIN_MASTERS / _M / _V copy P floats in; UVAD_HEAD_TRAIN_SCALARS takes the family's scalar record and restores t, 1 - beta1^t,
 *   1 - beta2^t, and for an LSTM state the draw ordinal (the accumulated loss and frame words are ignored: a write belongs between steps,
 *   and _GRAD is refused).  A state written from what was read is indistinguishable from the one that was read.
 * State: uvad_optim_state_bytes(n_lr) = a 256-byte header | the table, padded to 64 floats (0 for n_lr outside [1, 2^24]).  Workspace:
 *   uvad_optim_ws_bytes(ctx): one double per 4096 parameters of every family the context has configured, padded to 256 bytes.
 * Refusals (nothing enqueued).  UVAD_E_ARG: NULL cfg, table, optim state, workspace, d_in or d_out; n_lr < 1 or above 2^24 or above the
 *   reset's; a table entry not finite or <= 0; beta1 / beta2 outside [0, 1); eps not finite or <= 0; max_norm or weight_decay negative or
 *   not finite; an lr_scale not finite or < 0; all three states NULL; byte counts below the helpers; which outside MASTERS, M, V, SCALARS.
 *   UVAD_E_STATE: a family whose state is given but which is not configured; a family or optim state never reset, or reset under another
 *   shape.  On the device a state or optim state whose magic word or shape does not match makes the kernels write nothing. */
#define UVAD_OPTIM_RECORD_WORDS 8
typedef struct {
    float beta1, beta2, eps;
    float max_norm;                          /* 0 = no clipping */
    float weight_decay;                      /* 0 = none */
    int decoupled;                           /* 0: L2 into the gradient (Adam(weight_decay=)); 1: AdamW */
    int skip_nonfinite;                      /* 1: a step whose squared norm is not finite is skipped */
    float lr_scale[3];                       /* head, LSTM, SincNet: lr_k = fl(lr_t * scale) */
} uvad_optim_cfg;
size_t uvad_optim_state_bytes(int n_lr);
size_t uvad_optim_ws_bytes(const uvad_ctx *);
int uvad_optim_reset(uvad_ctx *, void *d_state, size_t state_bytes, const uvad_optim_cfg *, const float *h_lr_table, int n_lr, void *stream);
int uvad_optim_set_lr_table(uvad_ctx *, void *d_state, size_t state_bytes, const float *h_lr_table, int n_lr, void *stream);
int uvad_optim_step(uvad_ctx *, void *d_head_state, size_t head_bytes, void *d_lstm_state, size_t lstm_bytes, void *d_sincnet_state,
                    size_t sincnet_bytes, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);
int uvad_optim_read(uvad_ctx *, const void *d_state, size_t state_bytes, void *d_out, void *stream);
int uvad_optim_write(uvad_ctx *, void *d_state, size_t state_bytes, const void *d_in, void *stream);
int uvad_head_train_write(uvad_ctx *, void *d_state, size_t state_bytes, int which, const float *d_in, void *stream);
int uvad_lstm_train_write(uvad_ctx *, void *d_state, size_t state_bytes, int which, const float *d_in, void *stream);
int uvad_sincnet_train_write(uvad_ctx *, void *d_state, size_t state_bytes, int which, const float *d_in, void *stream);

/* ---- Noise mixing of training batches on the device -----------------------------------------------------------------------------------------
 * Every training recipe of the reference runs cuts.mix(noise_cuts, snr = (10, 20), mix_prob = 0.5, preserve_id = "left") on its training
 * phase (src/datasets/<corpus>/utils.py, enable_musan), once, on the host, before the features are stored.  Here the mix is a stage in front of uvad_fbank_lens /
 * uvad_sincnet_train_forward and is drawn anew for every batch: the draws come from the generator of the dropout stage above, the draw
 * ordinal lives on the device, so one captured graph draws a fresh mix per replay.  Not here: parity with lhotse itself, random start
 * offsets inside a clip, speed perturbation (reverberation is the block behind this one).
 *
 * Noise bank: one caller-owned device buffer d_bank of f32 samples, n_clips clips back to back; h_clip_first [n_clips + 1] (host, int64)
 *   are the clips' first samples, h_clip_first[0] = 0, every clip at least 1 sample.  The state keeps the pointer: the bank must stay where
 *   it is and unchanged while the state is in use.
 * Configuration: mix_prob in [0, 1]; snr_steps = Q >= 1 and the host table h_amp [Q] of doubles, the noise-to-speech AMPLITUDE ratios (the
 *   caller computes them: 10^(-(lo + (hi - lo) (q + 0.5) / Q) / 20) for Q steps over lo .. hi dB; no transcendental function runs on the
 *   device); max_seg in [1, UVAD_MIX_MAX_SEG]; seed.
 * Batch: d_in [B][S], fmt UVAD_INGEST_F32 or UVAD_INGEST_I16 (read as q / 32768, as uvad_sincnet_i16); len_b = clamp(d_nsamp[b], 0, S) as
 *   uvad_fbank_lens takes it (S when d_nsamp is NULL); d_out [B][S] f32, for f32 input d_out == d_in is allowed (in place).
 *
 * Energy: E(x, n) = (sum_i (double)x_i (double)x_i) / n over the n valid samples, 0 for n = 0; every product is exact in double.  The
 *   ORDER of the sum is a function of (samples, n) alone -- not of B, S, the grid or neighbouring rows: lane t = (i / 4) mod 1024 adds the
 *   squares of its samples in increasing i, starting from +0 (1024 lanes; samples 4 t .. 4 t + 3, then 4096 + 4 t .. and so on); then within
 *   each run of 64 lanes lane t += lane t + o for o = 32, 16, 8, 4, 2, 1; then the 16 run sums w_j += w_{j + o} for o = 8, 4, 2, 1; w_0 is
 *   divided by (double)n, one correctly rounded division.  No floating-point atomics.  A clip's energy is over the WHOLE clip (as lhotse's
 *   AudioMixer takes it before truncation), computed by uvad_mix_reset in the same order.
 * Draws: Philox4x32-10 exactly as the dropout block above defines it, counter = (row b, segment k, draw_lo, draw_hi), key = (seed_lo,
 *   seed_hi); row b is the row's index in the batch (uvad_mix_apply: row0 + b), as a 32-bit word.
 *     segment 0, word 0: the row is mixed iff (uint64)w0 < floor(mix_prob 2^32), a 64-bit compare: 1.0 always mixes, 0.0 never does;
 *     segment 0, word 1: q = (w1 Q) >> 32, one SNR per row, as in lhotse;
 *     segment k, word 2: clip = (w2 n_clips) >> 32;   word 3 is reserved.
 * Plan: segments are laid end to end from sample 0; segment k covers min(clip length, len_b - offset) samples, from the clip's first sample.
 *   Drawing stops when the row is covered or after max_seg segments; what is left stays clean.
 *   gain_k = (float)(amp[q] sqrt(E_row / E_clip)): the division and the square root correctly rounded double operations, the product one
 *   double rounding, then one rounding to f32; +0 when E_clip == 0 or E_row == 0.  A row of length 0, or one not mixed, has no segments.
 * Output: out = fl32(x + fl32(gain noise)) inside a segment: two f32 roundings, no fused multiply-add.  Samples outside every segment, and
 *   whole unmixed rows, are the input's f32 value bit for bit (a NaN passes through).  Samples past a row's length are +0 and are never read.
 * Draw ordinal: a 64-bit count at byte 56 of the state (zeroed by reset).  uvad_mix_step takes draw = the count and advances it by one, on
 *   the device, in a single thread of its first kernel, whatever mix_prob is: a replayed graph draws anew and micro-batches differ.
 * Plan record: d_plan (may be NULL) [B][UVAD_MIX_PLAN_HEAD + UVAD_MIX_SEG_WORDS max_seg] int32: {mixed (0 / 1: the draw's decision), q,
 *   nseg, 0}, then per segment {clip, dst offset, count, gain (the f32's bits)}; slots past nseg are zeros.  For logging and the tests.
 * State (uvad_mix_state_bytes; it does not depend on the bank's size): a 256-byte header {u32 magic, i32 n_clips, Q, max_seg; byte 16 u64
 *   floor(mix_prob 2^32); byte 24 u64 seed; byte 32 i64 samples in the bank; byte 56 u64 draw ordinal} | clip_first [n_clips + 1] int64 |
 *   clip energies [n_clips] f64 | amp [Q] f64, every part padded to 256 bytes.
 * Workspace (uvad_mix_ws_bytes(B, max_seg)): 256-byte header {byte 0 u64 the call's draw, byte 8 i64 row0} | row energies [B] f64 (from
 *   byte 256) | the plan [B][...] as above, every part padded to 256 bytes.
 * uvad_mix_reset uploads the tables, computes every clip's energy on the device and zeroes the draw ordinal; it synchronises the stream and
 *   is not for graph capture.  uvad_mix_step allocates nothing, never synchronises and can be captured.  uvad_mix_apply is the same step
 *   with the draw and the first row's index given and no state update: the same arguments give the same bytes, and row b of a batch equals
 *   a one-row call with row0 = b.  The three share every kernel.
 * Refusals (nothing enqueued).  UVAD_E_ARG: NULL ctx / cfg / h_amp / d_bank / h_clip_first / d_in / d_out / d_state / d_ws; d_state or
 *   d_ws not 16-byte aligned, d_bank / d_in / d_out / d_plan not aligned to their element; mix_prob outside [0, 1] or not finite; Q < 1 or > 2^24; an
 *   amplitude not finite or negative; max_seg outside [1, 64]; n_clips < 1; h_clip_first[0] != 0, an empty clip or a non-monotone table;
 *   B < 1; S < 1 or S > 2^31 - 1; state_bytes / ws_bytes below the helpers; an unknown fmt; int16 input with d_out == d_in.
 *   UVAD_E_STATE: a state that was never reset.  The size helpers return 0 on a bad argument. */
#define UVAD_MIX_MAX_SEG 64
#define UVAD_MIX_PLAN_HEAD 4
#define UVAD_MIX_SEG_WORDS 4
typedef struct {
    float mix_prob;          /* the share of rows that get noise, [0, 1] */
    int snr_steps;           /* Q: entries of h_amp */
    const double *h_amp;     /* host: noise-to-speech amplitude ratio of SNR step q */
    int max_seg;             /* noise clips laid end to end per row, at most */
    uint64_t seed;
} uvad_mix_cfg;
size_t uvad_mix_state_bytes(const uvad_mix_cfg *, int n_clips);
size_t uvad_mix_ws_bytes(int B, int max_seg);
int uvad_mix_reset(uvad_ctx *, void *d_state, size_t state_bytes, const uvad_mix_cfg *, const float *d_bank, const int64_t *h_clip_first,
                   int n_clips, void *stream);
int uvad_mix_step(uvad_ctx *, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan,
                  void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);
int uvad_mix_apply(uvad_ctx *, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan,
                   int64_t row0, uint64_t draw, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);

/* ---- Reverberation of training batches on the device ------------------------------------------------------------------------------------------
 * More than a third of the corpora the reference trains and tests on are far-field or meeting-room audio (CHiME-6 mdm, DiPCo, AMI, DIHARD3,
 * VoxConverse), and additive noise does not model a room.  This stage sits in front of uvad_mix_step (reverb, then noise, then uvad_fbank_lens /
 * uvad_sincnet_train_forward): per batch and per row it either leaves the row alone or convolves it with one room impulse response (RIR) of a
 * device-resident bank, what lhotse's reverb_rir does once on the host.  The draw is fresh per call and the draw ordinal lives on the device,
 * so one captured graph of reverb -> mix -> front end -> train step replays with new draws.  Not here, and UNPINNED: parity with lhotse /
 * torchaudio themselves (neither is available to the tests and the reference holds no fixture: the definition below is the contract);
 * multi-channel responses; reverberating the noise bank; speed perturbation.
 *
 * Bank: one caller-owned device buffer d_rir of f32 taps, n_rirs responses back to back; h_rir_first [n_rirs + 1] (host, int64) are the
 *   responses' first taps, h_rir_first[0] = 0, strictly increasing.  The state keeps the pointer: the bank must stay where it is and
 *   unchanged while the state is in use.  Response r has K_r = its length, or min(length, max_taps) when max_taps > 0: a truncated tail
 *   ("early reflections only" is a small max_taps).  K_r <= UVAD_REVERB_MAX_TAPS = 2^20 taps (65.5 s at 16 kHz); a longer response is
 *   refused unless max_taps cuts it.  Taps and the samples of a drawn row are expected finite: the kernel multiplies the zeros around a row
 *   and around a response like any other operand, so a NaN or Inf spreads further than the sum below says.
 * Delay: uvad_reverb_reset computes, on the device, delay_r = the smallest k < K_r at which |h_r[k]| is largest (the direct path), and keeps
 *   it in the state.  A NaN never wins the comparison (a response of NaNs has delay 0).
 * Batch: d_in [B][S], fmt UVAD_INGEST_F32 or UVAD_INGEST_I16 (read as q / 32768); n_b = clamp(d_nsamp[b], 0, S) (S when d_nsamp is NULL);
 *   d_out [B][S] f32.  d_out == d_in is refused: a row is read while it is written.
 * Draws: Philox4x32-10 exactly as the dropout block above defines it, counter = (row0 + b, 0x52560000, draw_lo, draw_hi), key = (seed_lo,
 *   seed_hi).  Word 1 of the counter differs from every segment index the mix stage uses (at most 63), so a mix state and a reverb state
 *   under one seed stay independent.
 *     word 0: the row is reverberated iff (uint64)w0 < floor(prob 2^32), a 64-bit compare: 1.0 always does, 0.0 never does;
 *     word 1: r = (w1 n_rirs) >> 32;   words 2 and 3 are reserved.
 * Convolution of a drawn row, with d = delay_r when align != 0 and d = 0 otherwise:
 *     z[i] = sum_{k = 0}^{K_r - 1} h_r[k] x[i + d - k]   for 0 <= i < n_b,
 *   x outside [0, n_b) is 0 and is never read.  The output has the row's own length (the tail is dropped, as lhotse does); with align the
 *   direct path stays where it was, so frame labels stay valid.  Products are f32-exact (v_mfma_f32_32x32x2_f32, the arithmetic of the
 *   training kernels; not the split-f16 planes).  Accumulation is in f32: ONE chain per output sample, starting from +0, over the taps in
 *   increasing k (in front of k = 0 and behind k = K_r - 1 the chain holds products with zero taps, which change nothing).  The order is a
 *   function of (K_r, i) alone, not of B, S, the grid or neighbouring rows.  No atomics: the same call gives the same bits.
 *   UVAD_REVERB_TILE (output samples of a workgroup) and UVAD_REVERB_K_CHUNK (input offsets staged at a time) are the kernel's tile
 *   constants, exported for the tests; no result depends on them.
 * Normalisation (normalize != 0; lhotse's normalize_output): E_in = E(x, n_b) and E_out = E(z, n_b) over the f32 values of z, E exactly the
 *   energy of the mix block above (the same double sum in the same order).  g = (float)sqrt(E_in / E_out): the division and the square
 *   root correctly rounded double operations, then one rounding to f32; g = 1.0f when either energy is 0.  out = fl32(z g): one rounding,
 *   no fused operation.  With normalize == 0, out = z.
 * Rows not drawn are the input's f32 value bit for bit (a NaN payload and -0 pass through; int16: q / 32768).  Samples past a row's length
 *   are +0 in d_out, in every row.
 * Draw ordinal: a 64-bit count at byte 56 of the state (zeroed by reset).  uvad_reverb_step takes draw = the count and advances it by one, on
 *   the device, in a single thread of its first kernel, whatever prob is.  uvad_reverb_apply takes draw and row0 as arguments and updates
 *   nothing: row b of a batch equals a one-row apply with row0 = b, byte for byte.
 * Plan record: d_plan (may be NULL) [B][UVAD_REVERB_PLAN_WORDS = 4] int32: {applied (0 / 1), r, d, the bits of g}; a row not drawn reads
 *   {0, 0, 0, the bits of 1.0f}.  For logging and the tests.
 * State (uvad_reverb_state_bytes; it does not depend on the bank's size): a 256-byte header {u32 magic, i32 n_rirs, normalize, align; byte 16
 *   u64 floor(prob 2^32); byte 24 u64 seed; byte 32 i64 taps in the bank; byte 40 i32 max_taps; byte 56 u64 draw ordinal} | rir_first
 *   [n_rirs + 1] int64 | K_r [n_rirs] int32 | delay_r [n_rirs] int32, every part padded to 256 bytes.
 * Workspace (uvad_reverb_ws_bytes(B)): 256-byte header {byte 0 u64 the call's draw, byte 8 i64 row0} | the plan [B][4] as above, padded to
 *   256 bytes.
 * uvad_reverb_reset uploads the tables, computes the delays and zeroes the draw ordinal; it synchronises the stream and is not for graph
 *   capture.  uvad_reverb_step and uvad_reverb_apply allocate nothing, never synchronise, read lengths and the ordinal on the device and can
 *   be captured.  Their argument order is that of uvad_mix_step / uvad_mix_apply; uvad_reverb_ws_bytes has no second argument because the plan
 *   row has a fixed width.
 * Refusals (nothing enqueued).  UVAD_E_ARG: NULL ctx / cfg / d_rir / h_rir_first / d_in / d_out / d_state / d_ws; d_state or d_ws not
 *   16-byte aligned, d_rir / d_in / d_out / d_plan not aligned to their element; prob outside [0, 1] or not finite; max_taps < 0; n_rirs < 1;
 *   h_rir_first[0] != 0, an empty response or a non-monotone table, K_r > 2^20; B < 1; S < 1 or S > 2^31 - 1; B ceil(S / 4096) > 2^31 - 1;
 *   state_bytes / ws_bytes below the helpers; an unknown fmt; d_out == d_in.
 *   UVAD_E_STATE: a state that was never reset.  The size helpers return 0 on a bad argument. */
#define UVAD_REVERB_PLAN_WORDS 4
#define UVAD_REVERB_MAX_TAPS 1048576
#define UVAD_REVERB_TILE 4096
#define UVAD_REVERB_K_CHUNK 256
typedef struct {
    float prob;              /* the share of rows that are reverberated, [0, 1] */
    int normalize;           /* != 0: scale the output to the input's energy */
    int align;               /* != 0: keep the direct path where it was (d = delay_r) */
    int max_taps;            /* > 0: use the first max_taps taps of every response; 0: all */
    uint64_t seed;
} uvad_reverb_cfg;
size_t uvad_reverb_state_bytes(const uvad_reverb_cfg *, int n_rirs);
size_t uvad_reverb_ws_bytes(int B);
int uvad_reverb_reset(uvad_ctx *, void *d_state, size_t state_bytes, const uvad_reverb_cfg *, const float *d_rir, const int64_t *h_rir_first,
                      int n_rirs, void *stream);
int uvad_reverb_step(uvad_ctx *, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan,
                     void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);
int uvad_reverb_apply(uvad_ctx *, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan,
                      int64_t row0, uint64_t draw, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);

/* ---- Training batches drawn on the device ------------------------------------------------------------------------------------------------------
 * The first stage of the chain sampler -> reverb -> mix -> front end -> train step: it cuts a device-resident corpus into windows, walks a
 * shuffled epoch order per dataset, multiplexes the datasets by weight, gathers the batch's samples and rasterises its frame labels.  It is the
 * reference's cut_into_windows(duration).filter(duration > min) ... .pad(duration), SimpleCutSampler(shuffle, drop_last), CutSet.mux(weights)
 * (data_module.py:140-151) and supervisions_feature_mask (custom_vad.py:41-75) as ONE definition that every draw follows; the cursors and the
 * draw ordinal live on the device, so one captured graph replays with a new batch.  No atomics: the same call gives the same bytes.
 * UNPINNED, and not claimed: parity with lhotse's samplers (their order comes from Python's random module; neither lhotse nor a fixture is
 * available to the tests): the definition below is the contract, tests/sampler_ref.py restates it.
 *
 * Corpus (caller-owned; the state keeps the pointer, the buffer must stay where it is and unchanged while the state is in use): d_pcm, the
 *   samples of R recordings back to back, fmt UVAD_INGEST_F32 or UVAD_INGEST_I16 (read as q / 32768); h_rec_first [R + 1] (host, int64) the
 *   recordings' first samples, h_rec_first[0] = 0, every recording 1 .. 2^31 - 1 samples.  Supervisions: h_sup [n_sup][2] (host, int64)
 *   {start, end} in samples of their own recording, h_sup_first [R + 1] (host, int32) each recording's range (h_sup_first[0] = 0, not
 *   decreasing, h_sup_first[R] = n_sup; h_sup may be NULL when n_sup = 0).  Supervisions may be unsorted, overlapping, empty, negative or past
 *   the end.  h_rec_set [R] (host, int32): each recording's dataset in 0 .. D - 1, 1 <= D <= UVAD_SAMPLER_MAX_SETS; h_weight [D] (host,
 *   doubles) finite and > 0.  All host tables are copied by reset.
 * Window table (built by uvad_sampler_reset on the host): recording r gives the windows {r, start = k W, n = min(W, len_r - k W)} for
 *   k = 0, 1, ..; a window is kept iff n > min_keep, a strict comparison (the reference's `> 3`), 0 <= min_keep < W -- so every full window
 *   is kept and only a recording's last, short one can go.  Windows are grouped by dataset, in recording order inside a dataset, in k order
 *   inside a recording: dataset d owns the N_d windows first_d .. first_d + N_d - 1.  A dataset without a window is refused; at most
 *   2^31 - 1 windows in all.  The table is stored per recording (kept windows of a recording are k = 0 .. K_r - 1): the state's size does not
 *   depend on the corpus' length.
 * Epoch order: the permutation is never stored.  perm(N, seed, d, e, p) for 0 <= p < N: 0 when N = 1; else k = max(8, bits(N - 1)) rounded
 *   up to even (bits(v) = the position of v's highest set bit, plus one), half = k / 2, mask = 2^half - 1, and starting from x = p repeat,
 *   until x < N (cycle walking over a bijection of [0, 2^k): the walk ends):
 *     L = x >> half, R = x & mask; four rounds t = 0 .. 3 of (L, R) = (R, L ^ (F & mask)), F = word 0 of Philox4x32-10 (the dropout block's
 *     generator) on counter (R | t << 16, 0x53500000 | d, e_lo, e_hi), key (seed_lo, seed_hi), R being the round's input; x = L << half | R.
 *   shuffle == 0 makes perm the identity (validation).  Counter word 1 differs from the mix stage's segment indices (at most 63), the reverb
 *   stage's 0x52560000 and every dropout layer word (layer << 16 | j >> 2 with layer below 0x5253): one seed serves all of them.  The minimum
 *   k of 8 is part of the definition (smaller domains are visibly biased).
 * A step of B rows.  Row b draws its dataset from Philox counter (row0 + b, 0x53440000, draw_lo, draw_hi), key (seed_lo, seed_hi): the first
 *   d with (uint64)w0 < cum[d], cum[d] = floor(2^32 ((w_0 + .. + w_d) / sum)) in double, the sums taken left to right, sum = w_0 + .. +
 *   w_{D - 1}, cum[D - 1] = 2^32 (D = 1: always 0).  Its position is c = cursor_d + (the rows b' < b of the same dataset); e = c / L_d,
 *   p = c mod L_d, window = first_d + perm(N_d, seed, d, e, p).  L_d = N_d, except that drop_last != 0 needs D = 1 and uses
 *   L = floor(N / batch) batch, batch being the cfg's: the step's B must equal it, N < batch is refused, and the last N - L windows of every
 *   epoch's permutation are skipped (SimpleCutSampler(drop_last=True)).  After planning one thread adds every dataset's row count to its
 *   cursor and 1 to the draw ordinal.  uvad_sampler_apply takes h_cursor [D] (host, int64, >= 0), draw and row0 as arguments and updates
 *   nothing: row b of a batch equals a one-row apply with row0 = b and its own cursor, byte for byte.  The two calls share every kernel.
 * Gather: d_out [B][ld_out >= W] f32: the window's n samples -- f32 bit for bit (a NaN payload and -0 pass through), int16 q / 32768 -- then
 *   +0 up to W; columns [W, ld_out) are untouched.  d_nsamp [B] int64 = len_b = n, or W when pad != 0 (the reference's .pad(duration): the
 *   waveform model's rows share a length).  16-byte stores from the first 16-byte boundary of the output row, 16-byte loads when the source
 *   is aligned with them (the source offset of a window is arbitrary: recordings are packed back to back), element by element before and behind.
 * Labels: d_labels [B][ld_gt >= T] uint8 and d_frames [B] int32, T = frames(W), T_b = frames(len_b), frames = uvad_num_frames for
 *   UVAD_SAMPLER_FBANK and uvad_sincnet_num_frames for UVAD_SAMPLER_SINCNET (the context's configuration at reset).  A supervision {s, e} of
 *   the window's recording is clipped to rs = max(s - start, 0), re = min(e - start, n), skipped when re <= rs, and sets the frames
 *   [st, et) n [0, T_b) to 1:
 *     FBANK    st = rs / hop, et = re / hop (integer division; hop = the context's frame shift in samples);
 *     SINCNET  st = rs > 0 ? max(floordiv(rs - half, step), 0) : 0,  et = re < len_b ? max(floordiv(re - half, step), 0) : T_b
 *              (half, step from the cfg; the reference's 496 and 270; custom_vad.py:41-75 with postprocess.supervision_frames' clamp).
 *   Bytes [T_b, T) are 0, bytes [T, ld_gt) untouched.  The walk over a recording's supervisions is brute force.
 * Plan record: d_plan (may be NULL) [B][UVAD_SAMPLER_PLAN_WORDS = 8] int32: {dataset, epoch (low word), position p, window, recording, start,
 *   n, T_b}.
 * State (uvad_sampler_state_bytes(cfg, R, n_sup, D)): a 256-byte header {u32 magic, i32 R, n_sup, D; byte 16 i64 W; byte 24 u64 seed; byte 32
 *   i64 samples in the corpus; byte 40 i32 fmt, geometry; byte 48 i32 windows in all, batch; byte 56 u64 draw ordinal; byte 64 i32 shuffle,
 *   drop_last, pad, half, step, hop, frame_len, snip_edges; byte 96 i32 the three kernel widths and the stride of the waveform front end; byte
 *   112 i64 min_keep} | 64 dataset entries of 32 bytes {i64 cursor, i64 L_d, u64 cum[d], i32 first_d, i32 N_d} | the recordings in table order
 *   [R] int32 | their first windows [R + 1] int32 | rec_first [R + 1] int64 | sup_first [R + 1] int32 | sup [n_sup][2] int64, every part
 *   padded to 256 bytes.  Workspace (uvad_sampler_ws_bytes(B)): 256-byte header {byte 0 u64 the call's draw, byte 8 i64 row0} | the plan
 *   [B][8] as above, padded to 256 bytes.
 * uvad_sampler_reset builds the table, uploads it and zeroes the cursors and the ordinal; it synchronises the stream and is not for graph
 *   capture.  uvad_sampler_step and uvad_sampler_apply allocate nothing, never synchronise and can be captured.  uvad_sampler_read writes the
 *   record {draw ordinal, cursor_0 .. cursor_{D - 1}} (1 + D int64, device memory) and uvad_sampler_write sets it (a negative cursor is stored as 0; the convention of
 *   uvad_optim_read / uvad_optim_write: device buffers, on the stream, no synchronisation): a resumed run continues to the bytes of an
 *   uninterrupted one.
 * Refusals (nothing enqueued, uvad_last_error names the word).  UVAD_E_ARG: NULL ctx / cfg / d_pcm / h_rec_first / h_sup_first / h_rec_set /
 *   h_weight / d_out / d_nsamp / d_labels / d_frames / d_state / d_ws / h_cursor, NULL h_sup with n_sup > 0; d_state or d_ws not 16-byte aligned,
 *   d_pcm / d_out / d_nsamp / d_frames / d_plan not aligned to their element; an unknown fmt; R < 1, n_sup < 0, D outside [1, 64];
 *   h_rec_first[0] != 0, an empty recording, a non-monotone table or a recording above 2^31 - 1 samples; a bad h_sup_first; a dataset index out
 *   of range, a dataset without windows; a weight not finite or <= 0; W < 1 or > 2^31 - 1; min_keep outside [0, W); drop_last with D > 1, with
 *   batch < 1, with N < batch, or a step with another B; an unknown geometry, step < 1 or half < 0 (SINCNET); a window without a frame; B < 1;
 *   ld_out < W or ld_gt < T; a negative cursor; state_bytes / ws_bytes below the helpers.
 *   UVAD_E_STATE: a state that was never reset; the label geometry's configuration missing from the context (no feature configuration for
 *   FBANK, no uvad_sincnet_configure for SINCNET).  The size helpers return 0 on a bad argument. */
#define UVAD_SAMPLER_FBANK 0
#define UVAD_SAMPLER_SINCNET 1
#define UVAD_SAMPLER_PLAN_WORDS 8
#define UVAD_SAMPLER_MAX_SETS 64
typedef struct {
    int64_t window;          /* W: samples of a window */
    int64_t min_keep;        /* a window is kept iff it has MORE samples than this; [0, W) */
    int geometry;            /* UVAD_SAMPLER_FBANK / UVAD_SAMPLER_SINCNET: which frame grid the labels are on */
    int half, step;          /* SINCNET: the receptive field's half width and the frame step in samples (496, 270) */
    int shuffle;             /* 0: table order (validation) */
    int drop_last;           /* != 0: an epoch is floor(N / batch) batch windows (D = 1 only) */
    int pad;                 /* != 0: d_nsamp = W for every row (short windows count as zero-padded) */
    int batch;               /* the batch size drop_last refers to */
    uint64_t seed;
} uvad_sampler_cfg;
size_t uvad_sampler_state_bytes(const uvad_sampler_cfg *, int R, int n_sup, int D);
size_t uvad_sampler_ws_bytes(int B);
int uvad_sampler_reset(uvad_ctx *, void *d_state, size_t state_bytes, const uvad_sampler_cfg *, const void *d_pcm, int fmt,
                       const int64_t *h_rec_first, int R, const int64_t *h_sup, const int32_t *h_sup_first, int n_sup, const int32_t *h_rec_set,
                       const double *h_weight, int D, void *stream);
int uvad_sampler_step(uvad_ctx *, int B, float *d_out, int64_t ld_out, int64_t *d_nsamp, uint8_t *d_labels, int64_t ld_gt, int32_t *d_frames,
                      int32_t *d_plan, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream);
int uvad_sampler_apply(uvad_ctx *, int B, float *d_out, int64_t ld_out, int64_t *d_nsamp, uint8_t *d_labels, int64_t ld_gt, int32_t *d_frames,
                       int32_t *d_plan, const int64_t *h_cursor, int64_t row0, uint64_t draw, void *d_state, size_t state_bytes, void *d_ws,
                       size_t ws_bytes, void *stream);
int uvad_sampler_read(uvad_ctx *, const void *d_state, size_t state_bytes, int64_t *d_out, void *stream);
int uvad_sampler_write(uvad_ctx *, void *d_state, size_t state_bytes, const int64_t *d_in, void *stream);

/* Which kernel runs the time-parallel contractions (input projections, feed-forward layers):
 *   0  exact f32: v_mfma_f32_32x32x2_f32, a k-ordered fmaf chain, bit-compatible with f32 FMA arithmetic;
 *   1  (default) f32-accurate on the f16 matrix cores: weights scaled by a power of two and split on the host into THREE
 *      f16 planes that reproduce them exactly, activations into two planes (22 bits) by the kernel that produces them;
 *      four v_mfma_f32_32x32x16_f16 products per term set in two f32 accumulator sets (dropped terms <= 2^-22 relative,
 *      below the rounding noise of the f32 accumulation).
 *      Needs operands inside the f16 range (|x| < 65504).  The library guarantees that without the caller's help:
 *      weights (and the bound they put on the feed-forward activations) are checked by uvad_finalize and a context
 *      that fails runs mode 0; features handed to uvad_classify are checked on the device and a batch that fails runs
 *      its first projection in mode 0 (no host synchronisation: both kernels are enqueued, a device flag picks one).
 *   2  the arithmetic of mode 1 with the tile-streaming kernel (gemm_f16p_kernel) for every GEMM: mode 1 runs the input
 *      projections of large launches in a weight-stationary persistent kernel (gemm_f16p_ws_kernel: the weight planes of a
 *      128-column tile stay in registers, only the activation planes stream through LDS) whose output is BIT-IDENTICAL;
 *      mode 2 exists for A/B measurements and as the reference of that identity test.
 *   3  mode 1 with THREE products per term set in the kernels of large launches (the weight-stationary projection, the fused head,
 *      the 16-sequence recurrence): the P2 x a_hi product is dropped, i.e. the weights are rounded to their two leading f16 planes
 *      (22 bits, the precision the activations already have).  The matrix cores then do 25 % less work, and because a step in
 *      flight runs at the socket's power limit that is time: +9 % frames/s at BASELINE cfg 2, recurrence launch
 *      1.85 -> 1.60 ms.  Logit error on contractive networks as in mode 1 (3e-7 at weights x2); on the near-chaotic x4 test
 *      network twice mode 1's distance from the float64 truth (a rounded weight is a slightly different network), which is why
 *      it is not the default.  Small launches (streaming steps) run mode 1's kernels: outputs of different launch sizes then
 *      differ in the last bits.
 * The SincNet front end (uvad_sincnet, uvad_forward_wav) follows the same selector: modes 1 and 3 run its three convolution stages on
 * the f16 matrix cores with the split arithmetic of mode 1 (exact three-plane weights in registers, sincnet_f16p.hip) when the geometry
 * is the reference's (sinc bank of 80 filters x <= 256 taps at stride 10; Conv1d(80 -> <= 64, 5); Conv1d(<= 64 -> <= 64, 5)), the leaky
 * slope is <= 1 and every stage input provably fits the f16 range ((|gamma| * sqrt(length) + |beta|) x max(1, |slope|) < 60000 for the
 * instance norm and leaky_relu in front of it); modes 0 and 2, other geometries, slopes and inputs outside that bound run the exact-f32
 * stages (v_mfma_f32_32x32x2_f32, sincnet.hip).  uvad_get_sincnet_form tells which.
 * All are held to the same 1e-4 logit bound by the tests.  Replaces nothing in the reference (torch picks its GEMM). */
int uvad_set_gemm_mode(uvad_ctx *, int mode);
/* What the most recent uvad_sincnet / uvad_forward_wav call of this context ran: 1 = the split-f16 stages, 0 = the exact-f32 stages
 * (also before the first call); negative on error. */
int uvad_get_sincnet_form(const uvad_ctx *);

/* How many sequences one recurrent workgroup owns (the time loop of nn.LSTM, PyanNet2.py:169-172):
 *   4   latency form (v_mfma_f32_4x4x1): B/4 x directions workgroups, the right one up to a few hundred sequences;
 *   16  throughput form (hidden_size 128 only): W_hh * h as four matrix-core products on the same exact three-plane
 *       split as GEMM mode 1 (three v_mfma_f32_16x16x32_f16; the fourth -- the residue plane, exactly bf8 -- on
 *       v_mfma_scale_f32_16x16x128_f8f6f4: uvad_get_p2_on_fp8); a quarter of the workgroups, each 1.35 x as long: a third of the CU-time per
 *       sequence.  The right one for B >= 1024 and for callers that keep several batches in flight on separate contexts;
 *   0   (default) chosen per call: the form with fewer estimated rounds of workgroups over the CUs (uvad_recurrent_tile_for).
 * uvad_get_recurrent_tile returns what the most recent uvad_classify / uvad_forward* call launched (4 or 16; 0 before
 * the first call).  Results agree to rounding between the two (tests/test_gpu_parity.py). */
int uvad_set_recurrent_tile(uvad_ctx *, int sequences);

/* Time chunks of a layer (the time loop of nn.LSTM and the x_t W_ih^T product in front of it, PyanNet2.py:169-172).  One batch alone
 * on the GPU cannot overlap its layers (layer l + 1 needs the backward pass of layer l to its last step), but inside a layer the
 * forward pass at frame t needs the gate rows up to t only and the backward pass those from t on: with n chunks the projection of
 * chunk i + 1 runs on a stream the library owns, on the CUs the 4-sequence recurrence leaves idle, beside the recurrence of chunk
 * i on the caller's stream (events fork and join the two; the call stays asynchronous and capturable once the stream pair has been
 * used outside a capture).  Same kernels and arithmetic per row: outputs are bit-identical to the unchunked call.
 *   0  (default) automatic: T / 96 chunks, at most 6, of geometrically growing length (only the first one's projection is exposed),
 *      when the 4-sequence recurrence is the form in use, it leaves at least a quarter of the CUs idle, the GEMM mode is 1 or 3 and
 *      a side stream concurrent with the caller's was found;
 *   1  off;   2 .. 64  that many chunks wherever the chunked form can run.
 * uvad_get_time_chunks: what the most recent uvad_classify / uvad_forward* call ran (1 = not chunked).
 * Replaces nothing in the reference (its nn.LSTM is one cuDNN / MIOpen call per layer stack). */
int uvad_set_time_chunks(uvad_ctx *, int chunks);
int uvad_get_time_chunks(const uvad_ctx *);
int uvad_get_recurrent_tile(const uvad_ctx *);
/* How many steps the caller keeps in flight at once, this context's included (one context and stream per step: ForwardPipeline).
 * The large input projections (x_t W_ih^T, PyanNet2.py:169-172) and the fused head run as persistent grids of one workgroup per CU,
 * and such a workgroup and a recurrence workgroup cannot share a CU (registers).  A grid over the whole chip keeps every CU until
 * its last tile is done, so the recurrences that the other steps launch meanwhile wait for it and the steps fall into lockstep.
 * With n > 1 the persistent grids of a call that is not time-chunked leave (n - 1) x rec_cus CUs free, rec_cus being the
 * workgroups of this call's own recurrence launch (ceil(B / 16) x directions in the 16-sequence form, ceil(B / 4) x directions
 * in the 4-sequence form): max(per, (CUs - reserve) / per x per) workgroups, per = 8 x (4 x hidden x directions / 128).  A
 * reserve above half the CUs is not made: so many steps keep every CU taken anyway and smaller grids were measured to lose there
 * (whole-chip grids again).  The tile queue hands every tile out once whatever the grid: outputs are bit-identical for every n.
 *   1  (default) the call runs alone: grids over the whole chip;   n >= 1 accepted.
 * uvad_get_projection_grid: the workgroups of the weight-stationary projection launches of the most recent uvad_classify /
 * uvad_forward* call (0 = it launched none: small launches and the other GEMM modes run the tile-streaming kernels).
 * Replaces nothing in the reference (its inference is one batch at a time, src/scripts/predict.py:98). */
int uvad_set_concurrent_steps(uvad_ctx *, int n);
int uvad_get_concurrent_steps(const uvad_ctx *);
int uvad_get_projection_grid(const uvad_ctx *);
/* 1 if the throughput form runs its fourth product (P2 x h, the residue plane of the exact three-way split of W_hh) on the 8-bit
 * matrix pipe (v_mfma_scale_f32_16x16x128_f8f6f4): decided by uvad_finalize, which checks that EVERY element of every layer's P2 plane is
 * exactly a bf8 (E5M2) number after one power-of-two shift, so the weights stay exact (the residue of two round-to-nearest f16
 * splits of a 24-bit significand always is: at most two significant bits, within bf8's exponent range of the f16 value it replaces);
 * 0 in GEMM mode 2 (the kernel set kept for comparisons reads P2 from its f16 image, as every mode did before round 4), if a check
 * failed, or if the model has no hidden_size-128 layers.  h enters that one product rounded to fp8 (E4M3). */
int uvad_get_p2_on_fp8(const uvad_ctx *);
/* What mode 0 would launch for a batch of B sequences (4 or 16).  A sweep sharded over n GPUs that wants every utterance to
 * get the same bits as the unsharded run pins all ranks to uvad_recurrent_tile_for(ctx, GLOBAL batch) (tools/run_cfg4.py
 * --reproducible); left alone each rank picks the faster form for its own shard and results agree to rounding. */
int uvad_recurrent_tile_for(const uvad_ctx *, int B);

/* Do two HIP streams run concurrently?  HIP maps streams onto a small pool of hardware queues and two streams that share
 * a queue serialise, which silently defeats "two batches in flight" (ForwardPipeline).  The probe enqueues a 3 ms
 * spinning wave on stream_a and an empty kernel on stream_b and reports whether b's retired while a's was still running:
 * 1 = concurrent, 0 = serialised, negative = error.  Synchronises both streams (call it at set-up time, not per batch).
 * Replaces nothing in the reference (its inference is one batch at a time, src/scripts/predict.py:98). */
int uvad_streams_overlap(uvad_ctx *, void *stream_a, void *stream_b);

/* Per-stage device timing of the most recent uvad_forward/uvad_classify made with timing enabled
 * (uvad_set_timing(ctx, 1) inserts hipEvents on the caller's stream; not graph-capturable while
 * enabled).  ms[0..4] = fbank, input projections, recurrences, feed-forward+classifier, total.
 * Synchronises on the recorded events. */
int uvad_set_timing(uvad_ctx *, int enabled);
int uvad_get_timing(uvad_ctx *, float ms[5]);
/* The same timed call layer by layer: ms[2k] = input projection of LSTM layer k (x * W_ih^T, nn.LSTM inside PyanNet2.forward,
 * PyanNet2.py:169-172), ms[2k+1] = its recurrence; n = capacity of ms in floats (>= 2 * num_layers).  Returns the number of
 * floats written.  bench.py reads the K = 256 projection and one recurrent launch from here for its roofline object. */
int uvad_get_layer_timing(uvad_ctx *, float *ms, int n);

const char *uvad_last_error(const uvad_ctx *);
void uvad_destroy(uvad_ctx *);

#ifdef __cplusplus
}
#endif
#endif /* UVAD_H */
