// Internal launcher declarations shared by the translation units of libuvad.so.
// Everything here is gfx950-only HIP; no torch types, no CPU fallbacks.
#pragma once
#include <hip/hip_runtime.h>
#include <type_traits>
#include <stdint.h>
#include "../../include/uvad.h"

namespace uvad {

// Sequences are processed in tiles of SEQ_TILE batch entries: activation rows are ordered
//   m = (tile * T + t) * SEQ_TILE + j,   b = tile * SEQ_TILE + j
// so that the SEQ_TILE rows one recurrent workgroup needs at step t are adjacent in HBM.
constexpr int SEQ_TILE = 4;

// f16 activation planes (the operands of gemm_f16p.hip) are K-BLOCKED: rows in tiles of PLANE_TILE, columns in blocks of 16,
//   element (row, col) of a plane with `width` columns (a multiple of 16) lives at plane_index(row, col, width),
// so the PLANE_TILE x 16 slab one GEMM workgroup needs per k-block is one contiguous 4 KiB run.  A plane of M rows
// occupies plane_rows(M) * width elements.
constexpr int PLANE_TILE = 128;
__host__ __device__ inline size_t plane_index(size_t row, int col, int width) {
    return ((row / PLANE_TILE) * (size_t)(width / 16) + (size_t)(col / 16)) * (PLANE_TILE * 16) + (row % PLANE_TILE) * 16 + (size_t)(col % 16);
}
inline size_t plane_rows(size_t M) { return (M + PLANE_TILE - 1) / PLANE_TILE * PLANE_TILE; }

// The gate pre-activations G (output of the projection GEMMs, input of the recurrent kernels) are TILE-BLOCKED:
// [128-row tile][64-column tile][128][64] f32, so a GEMM workgroup's 128 x 128 output tile (two adjacent tiles) is one contiguous 64 KiB run
// (row-major G made every workgroup write 128 pieces of 256 bytes 4 KiB apart: measured 2.6 TB/s, not overlapped with
// the K loops) and the 4 rows x 64 gate columns (16 units x 4 gates) a recurrent wave reads per step are one contiguous KiB.
// ncols (= 4 * hidden * directions) is a multiple of 64; a G of M rows occupies plane_rows(M) * ncols floats.
__host__ __device__ inline size_t g_index(size_t row, int col, int ncols) {
    return ((row / 128) * (size_t)(ncols / 64) + (size_t)(col / 64)) * (128 * 64) + (row % 128) * 64 + (size_t)(col % 64);
}

// ---- gemm.hip / gemm_f16p.hip -------------------------------------------------------------
// C[M][ldc] (cols [0,N)) = act( A[M][K] * W[N][K]^T + bias[N] ).
//   gemm.hip       exact f32 on v_mfma_f32_32x32x2_f32 (a k-ordered fmaf chain); A and C are f32.
//   gemm_f16p.hip  f32-accurate on the f16 matrix cores; A arrives (and C may leave) as two f16 PLANES
//                  x ~= hi + lo * 2^-11 written by the producing kernel, W as three exact f16 planes (see gemm_f16p.hip).
struct GemmArgs {
    // ---- gemm.hip operands
    const float *A;      // activations
    const float *W;      // [N][ldw] row-major (torch Linear / LSTM weight layout, rows possibly permuted),
                         // each row zero-padded to ldw = gemm_padded_k(K) floats
    // ---- gemm_f16p.hip operands
    const unsigned short *Ah, *Al;    // K-blocked f16 planes of the activations, K columns (columns past the true width zero)
    const unsigned short *Wsplit16;   // w * 2^S as three K-blocked f16 planes (128-row tiles) that add up to it exactly
    float wscale;                     // 2^-S
    unsigned short *Ch, *Cl;          // out_planes: K-blocked f16 planes of the result, ldc columns ([N, ldc) written as zero)
    int out_planes;
    int products;        // gemm_f16p_ws.hip: 4 (0 reads as 4) = all four products above, weights exact; 3 = without P2 x a_hi (weights rounded to 22 bits)
    // ---- common
    int c_blocked;       // C is the tile-blocked gate matrix (g_index, ncols = N) instead of row-major [M][ldc]
    int ldw;
    const float *bias;   // [N] or nullptr
    float *C;
    int M, N, K;         // gemm_f16p.hip: K = the padded width (multiple of 32)
    int lda, ldc;
    // a_mode 0: row m of A is A + m*lda.
    // a_mode 1 (gemm.hip only): A is canonical [B][T][K]; row m = (tile*T + t)*SEQ_TILE + j reads sequence
    //           b = tile*SEQ_TILE + j at frame t (zeros when b >= B).
    //           (rows of padded sequences and rows past the tile's range are clamped, never stored)
    int a_mode, B, T;
    float leaky_slope;   // act: v >= 0 ? v : slope*v when act == 1
    int act;
    // Device-side kernel selection for caller-supplied features (uvad_classify): when `gate` is set the kernel
    // returns at once unless (*gate != 0) == gate_run_if_set.  *gate is written by launch_split_features() earlier on
    // the same stream, so the f16 split never feeds an operand outside the f16 range to the matrix cores and no host
    // sync is needed.
    const int *gate;
    int gate_run_if_set;
    // gemm_f16p_ws.hip, optional (time-chunked projections, uvad_api.hip): instead of every row tile 0 .. ceil(M / 128) - 1, the column
    // tiles of direction d (ws_dirs = 2: d = 0 for columns [0, N / 2), d = 1 for the rest; ws_dirs = 1: d = 0 for all) process the
    // 128-row tiles ws_tiles[ws_off[d] .. ws_off[d] + ws_len[d]) -- device memory, read with scalar loads.  nullptr: all row tiles.
    const int *ws_tiles;
    int ws_off[2], ws_len[2], ws_dirs;
};
hipError_t launch_gemm(const GemmArgs &a, hipStream_t s);
int gemm_padded_k(int K);        // gemm.hip: K rounded up to its K-step (weight row padding)
hipError_t launch_gemm_f16p(const GemmArgs &a, hipStream_t s);
int gemm_f16p_padded_k(int K);   // gemm_f16p.hip: plane row width for a true width K (multiple of 32)
// gemm_f16p_ws.hip: the same contraction for the tile-blocked gate matrix (c_blocked, no activation) as a weight-stationary persistent
// kernel; bit-identical output.  `counters` = gemm_f16p_ws_counter_bytes() of device memory (zeroed by the launcher on the stream).
bool gemm_f16p_ws_supported(const GemmArgs &a, int n_cu);
size_t gemm_f16p_ws_counter_bytes();
// grid_cus: CUs the persistent grid may take (0 = n_cu; rounded down to a multiple of 8 column-tile groups, at least one);
// grid_used: the workgroups launched.
hipError_t launch_gemm_f16p_ws(const GemmArgs &a, unsigned *counters, int n_cu, hipStream_t s, int *grid_used = nullptr, int grid_cus = 0);
size_t weight_plane_elems(int N, int ldw);
bool split_weights_f16x3(const float *w, int N, int ldw, unsigned short *out /*3 * weight_plane_elems*/, float *wscale);   // false: not representable
// canonical f32 features [B][T][F] -> the same with frames t >= clamp(lens[b], 0, T) zero (never read): the operand of a lens classify
hipError_t launch_mask_features(const float *x, int B, int T, int F, const int *lens, float *out, hipStream_t s);
// canonical f32 features [B][T][F] -> tile-major K-blocked f16 planes (tiles*T*4 rows, Fp columns); *flag (optional) = 1 if a value is non-finite or
// outside the f16 range
hipError_t launch_split_features(const float *x, int B, int T, int F, int Fp, int tiles, unsigned short *xh, unsigned short *xl, int *flag,
                                 hipStream_t s);

// ---- lstm.hip -----------------------------------------------------------------------------
// One layer, all directions: grid (tiles, dirs).  G holds x_t*W_ih^T + b_ih + b_hh with column
// dir*4H + u*4 + gate, tile-blocked (g_index with ldg columns); Y gets h_t at column dir*H + u.  Rows as above.
struct LstmArgs {
    const float *G; int ldg;
    const float *Whh_packed;     // per dir: register image, see pack_whh()
    // 16-sequence form (H = 128 only, pack_whh16h): per dir the P0 / P1 register image, the P2 LDS image, and 2^-S
    const unsigned *Whh16h_regs; const unsigned short *Whh16h_p2; const float *whh16h_scale;
    // ... and (optional) the P2 image as bf8 bytes for the 8-bit matrix pipe (pack_whh16h_p2q; nullptr: the f16 image is used) with the
    // E8M0 scale operand that undoes its power-of-two shift
    const unsigned short *Whh16h_p2q; int p2q_scale;
    float *Y; int ldy;           // f32 output (exact-f32 GEMM mode), or
    unsigned short *Yh, *Yl;     // the two K-blocked f16 planes (ldy columns) h ~= hi + lo * 2^-11 the f16p GEMM of the next layer reads (Y == nullptr)
    int products;                // 16-sequence form: 4 (0 reads as 4) or 3 (no P2 plane: see GemmArgs)
    int tiles, T, H, dirs;
    // 4-sequence form, optional: run `steps` time steps only (0 = all T): direction 0 frames t_begin[0] .. t_begin[0] + steps - 1 in
    // ascending order, direction 1 frames t_begin[1] .. t_begin[1] + steps - 1 in descending order, from / to the carried state
    // (h0, c0 -> hN, cN).  Rows are addressed with the whole sequence length T.
    int steps, t_begin[2];
    int tile_mode;               // sequences per workgroup: 0 = by estimated time, 4, 16 (see launch_lstm)
    int n_cu;                    // compute units of the device (0 = 256)
    // optional carried state (streaming): [dirs][tiles*SEQ_TILE][H], nullptr = zeros / discard
    const float *h0, *c0; float *hN, *cN;
    // optional per-row lengths (uvad_classify_lens): device int32 [nB], clamped to [0, T], sequences past nB have length 0; every sequence
    // runs from zero state over its first len frames (no steps / carried state); a workgroup runs max(len) steps of its sequences
    const int *lens; int nB;
};
hipError_t launch_lstm(const LstmArgs &a, hipStream_t s, int *tile_used = nullptr);
int lstm_auto_tile(int tiles, int dirs, int H, int n_cu);   // what tile_mode 0 picks (4 or 16)
// elements of the packed W_hh image for one direction
size_t whh_packed_elems(int H);
int lstm_waves(int H);   // waves per recurrent workgroup (8 at H = 128: two per SIMD)
// host-side packer: torch w_hh [4H][H] (rows i,f,g,o) -> register image
void pack_whh(const float *w_hh, int H, float *out);
size_t whh16h_regs_elems();
size_t whh16h_p2_elems();
bool pack_whh16h(const float *w_hh, unsigned *regs, unsigned short *p2, float *wscale);   // false: a weight is non-finite
size_t whh16h_p2q_elems();
// the P2 image as bf8 (E5M2) bytes, columns in the kernel's k order; false if some element is not exactly representable (the f16 image
// then stays in use); *scale = the E8M0 scale operand (127 - shift)
bool pack_whh16h_p2q(const float *w_hh, unsigned short *p2q, int *scale);

// ---- head.hip -----------------------------------------------------------------------------
// logit = Z[m][:K] . w + b ; prob = sigmoid(logit); written at canonical [b][t] (b < B only).
struct ClsArgs {
    const float *Z; int ldz, K;
    const float *w, *b;
    float *logits, *probs;   // either may be nullptr
    int tiles, T, B;
    int ld_out;              // row stride of logits / probs (>= T)
};
hipError_t launch_classifier(const ClsArgs &a, hipStream_t s);
// rows (tile-major) -> canonical [B][T][W] copy, for the parity taps (src_lo != nullptr: src / src_lo are f16 planes)
hipError_t launch_untile(const void *src, const void *src_lo, int lds_, int W, float *dst, int tiles, int T, int B, hipStream_t s);
// threshold 0.5 + binary median
hipError_t launch_median(const float *probs, int B, int T, int kernel, uint8_t *labels, hipStream_t s);
// 0/1 label rows -> ordered (start frame, first non-speech frame) pairs per row + the number of runs
hipError_t launch_runs(const uint8_t *labels, int B, int T, int max_runs, int *runs, int *counts, hipStream_t s);
// per-row lengths (device int32 [B], clamped to [0, T]): outputs [B][ld] at t >= len_b set to 0; median / runs on each row's prefix
hipError_t launch_lens_fill(float *logits, float *probs, int B, int T, int ld, const int *lens, hipStream_t s);
hipError_t launch_median_lens(const float *probs, int B, int T, int kernel, uint8_t *labels, const int *lens, hipStream_t s);
hipError_t launch_runs_lens(const uint8_t *labels, int B, int T, int max_runs, int *runs, int *counts, const int *lens, hipStream_t s);
// per-row {false alarm, missed detection} frame counts of 0/1 label rows
hipError_t launch_der(const uint8_t *pred, const uint8_t *gt, int B, int T, uint32_t *counts, hipStream_t s);

// zero n words of tile-queue counters with device-scope atomic exchanges: the operations the persistent kernels count with
// (gemm_f16p_ws_kernel, head_fused_kernel), so the reset and the counting meet at the same coherence point.  Used instead of
// hipMemsetAsync, whose blit node in a replayed hipGraph was not always seen by the next kernel's atomics (the head then found its
// queue exhausted and left its logits unwritten)
hipError_t launch_zero_counters(unsigned *p, int n, hipStream_t s);

// one wave that busy-waits `ticks` of the 100 MHz constant clock, then (optionally) stores the waited ticks
hipError_t launch_spin(unsigned long long ticks, unsigned long long *sink, hipStream_t s);

// ---- head_fused.hip: leaky_relu(y W1^T + b1) -> leaky_relu(. W2^T + b2) -> . w + b -> sigmoid in one kernel (two 128-unit layers, split-f16 mode) ----
struct HeadArgs {
    const unsigned short *Yh, *Yl;   // K-blocked f16 planes of the LSTM output (K1 columns), tile-major rows
    long long M; int K1;             // rows (tiles * T * SEQ_TILE), input width (256 or 128)
    const unsigned short *W1, *W2;   // three exact f16 planes each (split_weights_f16x3: N = 128 rows, K1 / 128 columns)
    float w1scale, w2scale;
    const float *b1, *b2, *wc, *bc;  // biases [128], classifier row [128] and bias [1]
    float slope;
    float *logits, *probs;           // canonical [b][t] (b < B only), row stride ld_out; either may be nullptr
    int tiles, T, B, ld_out;
    unsigned *counter;               // one word of device memory (zeroed by the launcher)
    int products;                    // 4 (0 reads as 4) or 3 (no P2 plane: see GemmArgs)
};
bool head_fused_supported(int K1, int lin_hidden, int lin_layers, long long M, int n_cu);
hipError_t launch_head_fused(const HeadArgs &a, int n_cu, hipStream_t s);

// ---- fbank.hip ----------------------------------------------------------------------------
struct FbankTables {            // device pointers owned by the ctx
    const float *window;        // [frame_len]
    const int *mel_start;       // [n_mels] first bin with non-zero weight
    const int *mel_len;         // [n_mels] number of bins
    const float *mel_w;         // [n_mels][mel_stride] weights (zero padded)
    const float *mel_wt;        // the same transposed, the LDS image of the mel stage: [mel_stride][mel_image_ld(n_mels)] (zero padded), x 1/4
    int mel_stride;             // the uniform trip count of the band loop: the longest band rounded up to a multiple of 4 bins
    const float *tw512;         // [512][2] (cos, -sin)(2*pi*j/512): forward FFT twiddles
    int nyquist;                // 1 if any filter weighs bin n_fft / 2 (kaldi-style tables, the reference's, carry a zero column there: the
                                // power of that bin -- a fifth round of the spectrum split for one lane's sake -- is then not computed)
};
// The mel stage's weight image (fbank_pair.h): one row of mel_image_ld floats per bin-in-band, a compile-time row stride in the kernels
// (the weights a lane needs per iteration sit at immediate offsets).
__host__ __device__ inline int mel_image_ld(int n_mels) { return n_mels <= 64 ? 64 : 128; }
__host__ __device__ inline size_t mel_image_floats(int mel_stride, int n_mels) { return (size_t)mel_stride * mel_image_ld(n_mels); }
struct FbankArgs {
    const void *pcm; int pcm_is_i16;
    int B; int64_t S; int64_t T;
    int64_t row_stride;         // elements between rows of pcm (0 = S)
    int frame_len, frame_shift, n_mels;
    float preemph, log_floor; int remove_dc, snip_edges;
    float *feats;               // [B][T][n_mels]
    // Instead of feats (plane_hi != nullptr): the two K-blocked f16 planes of the features (plane_w columns, a multiple of 16, the
    // columns [n_mels, plane_w) written as zero) with rows in the classifier's tile-major order, padding sequences zeroed: the A
    // operand of the first projection GEMM (gemm_f16p.hip), bit-identical to what launch_split_features makes of feats
    unsigned short *plane_hi, *plane_lo; int plane_w;
    // Streaming (uvad_stream_step): instead of pcm the rows are VIRTUAL -- row b = [tail of the previous steps (vs_tail samples; on the
    // first step the reflection of the chunk's head) | this step's chunk], read from vs_offset on -- and the workgroups of the first
    // tile also write the next tail (the last vs_tail samples of that row) to vs_tail_out.  vs_chunk == nullptr: plain pcm rows.
    const float *vs_chunk, *vs_tail_in; float *vs_tail_out;
    int vs_tail, vs_chunk_len, vs_first, vs_n_left, vs_offset;
    FbankTables tab;
    // optional per-row sample counts (uvad_fbank_lens): device int64 [B], clamped to [0, S]; row b is framed as a row of nsamp[b] samples
    // alone (reflection at its end, later samples never read) and its frames past uvad_num_frames(nsamp[b]) are written as zero
    const int64_t *nsamp;
};
hipError_t launch_fbank(const FbankArgs &a, hipStream_t s);
// frames[b] = the frame count of a row of clamp(nsamp[b], 0, S) samples (uvad_num_frames), device int32 [B]
hipError_t launch_frames_of(const int64_t *nsamp, int B, int64_t S, int frame_len, int frame_shift, int snip_edges, int *frames, hipStream_t s);
size_t fbank_lds_bytes(const FbankArgs &a);
// streaming: staging[b] = [tail (frame_len samples, reflection-filled on the first step) | chunk];
// new tail = last `tail` samples of staging
hipError_t launch_stream_stage(const float *chunk_pcm, int B, int chunk, int tail, int n_left, int first_step,
                               const float *tail_in, float *tail_out, float *staging, hipStream_t s);

// ---- window_stream.hip: the feature ring of the windowed stream (uvad_window_step) -------------------------------------------
// The window [e - Tw, e) of every feed, e = *ctr_in + k read on the device, from the ring [B][R][F] (frame t in slot t % R) and the k
// new frames newf [B][k][F] (committed to their slots on the way) -> the f16 planes of the first projection (planes: split_features_kernel's
// layout, Fp columns, tiles * Tw * SEQ_TILE tile-major rows, padding sequences zero) or canonical f32 rows out [B][Tw][F].  ctr_out
// (optional) receives e.  k = 0, ctr_out = nullptr: a read-only copy of the window (the debug tap).
struct WindowArgs {
    const float *newf; float *ring; const long long *ctr_in; long long *ctr_out;
    int B, R, F, k, Tw;
    int planes; unsigned short *xh, *xl; int Fp, tiles;
    float *out;
};
hipError_t launch_window_assemble(const WindowArgs &a, hipStream_t s);
// a step that completes no frame: *ctr_out = *ctr_in (a kernel, not a copy node: see launch_zero_counters)
hipError_t launch_window_carry(const long long *ctr_in, long long *ctr_out, hipStream_t s);
// logits / probs [b][j] (row stride ld_out) = logits_in / probs_in [b][r0 + j] (row stride Tw), j < n; either output may be nullptr
hipError_t launch_window_emit(const float *logits_in, const float *probs_in, int B, int Tw, int r0, int n, float *logits, float *probs,
                              int ld_out, hipStream_t s);

// ---- wav_window_stream.hip: the PCM ring of the waveform model's windowed stream (uvad_window_wav_step) ----------------------------
// n_prev = *ctr_in samples have arrived before the step (read on the device); the chunk [B][chunk] is committed to the ring [B][ring]
// (sample p in slot p % ring) and, when out != nullptr, the window of Tw frames, e = frames(n_prev + chunk) = (n - R) / J + 1, samples
// [J (e - Tw), J (e - Tw) + Sw) is written to out [B][Sw]; *ctr_out = n_prev + chunk.  Samples of the type of the state (f32 or int16).
struct WavWindowArgs {
    const void *chunk; void *ring; const long long *ctr_in; long long *ctr_out;
    int B, chunk_len, J, R, Tw, Sw;
    long long ring_len;
    void *out;
};
hipError_t launch_wav_window_assemble(const WavWindowArgs &a, int is_i16, hipStream_t s);

// ---- window_slots.hip: the slot pools of both window families (uvad_window_slots_*, uvad_window_wav_slots_*) ------------------------
// Per-slot counters in the pool's state, device arrays [B]: samples and frames of the slot's session so far, whether a session is open,
// the window length the last step classified (the features tap); step: the pool's step count (the log-mel tail's ping-pong parity).
struct SlotCounters { long long *n, *e; int *active, *tw_last; long long *step; };
// What one step does to one slot, written by the step's first kernel into the workspace and read by the later ones
struct alignas(16) SlotPlan {
    long long n, e, e_prev;          // samples and frames of the session after the step, frames before it
    int live, end, first, k;         // holds a session this step / it ends now / this is its first chunk / new frames
    int offset, Tw, r0, n_emit;      // (log-mel) first new frame in the virtual [tail | chunk] row; window; emitted rows [r0, r0 + n_emit)
    int pad[2];
};
// log-mel: flags applied, plan[b] written, aligned staging rows [B][row] of the new frames side by side (row = frames * frame_len, frames =
// kmax rounded up to even) and the next tails
struct SlotStageArgs {
    const float *chunk; const uint8_t *flags; SlotCounters ctr;
    float *tails;                    // [2][B][frame_len]: the step reads tails[step & 1], writes tails[(step & 1) ^ 1]
    float *staging; SlotPlan *plan;
    int B, chunk_len, frame_len, shift, n_left, row, W, L;
};
hipError_t launch_slot_stage(const SlotStageArgs &a, hipStream_t s);
// log-mel: the new frames newf [B][kmax][F] (kmax: the staging rows' frames) committed to the ring [B][W][F] (session frame f in slot f % W) and each slot's window of
// Tw_b frames left-aligned into the planes (window_assemble_kernel's layout at T = W) or out [B][W][F], zero past Tw_b; lens[b] = Tw_b.
// plan == nullptr: the read-only tap of the window the last step classified (ctr.e, ctr.tw_last), into out.
struct SlotAssembleArgs {
    const SlotPlan *plan; SlotCounters ctr;
    const float *newf; int kmax; float *ring;
    int B, W, F;
    int planes; unsigned short *xh, *xl; int Fp, tiles;
    float *out; int *lens;
};
hipError_t launch_slot_assemble(const SlotAssembleArgs &a, hipStream_t s);
// waveform: flags applied, plan[b] written, the chunk committed to the PCM ring [B][ring_len] (session sample p in slot p % ring_len),
// each slot's window of Sw_b samples left-aligned into out [B][Sw_max] (zero past Sw_b), nsamp[b] = Sw_b
struct WavSlotArgs {
    const void *chunk; const uint8_t *flags; SlotCounters ctr;
    void *ring; long long ring_len;
    void *out; int Sw_max; long long *nsamp; SlotPlan *plan;
    int B, chunk_len, J, R, W, L;
};
hipError_t launch_wav_slot_assemble(const WavSlotArgs &a, int is_i16, hipStream_t s);
// both: rows [r0_b, r0_b + n_b) of logits_in / probs_in [B][W] -> columns 0 .. n_b - 1 of logits / probs [B][ld_out], counts[b] = n_b,
// the counters committed and the step counted
struct SlotEmitArgs {
    const SlotPlan *plan; SlotCounters ctr;
    const float *logits_in, *probs_in; int B, W;
    float *logits, *probs; int ld_out; int *counts;
};
hipError_t launch_slot_emit(const SlotEmitArgs &a, hipStream_t s);

// ---- sliding.hip: sliding-window inference over whole recordings (uvad_sliding_*) ------------------------------------------------------
// The window list of a batch of nrec recordings: first (device int32 [nrec + 1], the exclusive prefix of the planned window counts, from
// the host), N = first[nrec] as the host passed it, window W and hop Hf in frames.  T_r comes from the device lengths alone: lens (int32
// [nrec] frames, clamped to [0, T]) for log-mel, or nsamp (int64 [nrec] samples, clamped to [0, S]) with the waveform model's closed
// form frames(S) = 0 if S < R0 else (S - R0) / J + 1.  Window j of r holds clamp(T_r - j Hf, 0, W) frames, whatever the plan says.
struct SlidingPlan {
    const int *first; int nrec; long long N; int W, Hf;
    const int *lens; int T;                              // T: frames per row of the recordings' feature / output rows
    const long long *nsamp; long long S; int J, R0;      // waveform model: samples per PCM row, frame step and receptive field
};
// log-mel: windows [i0, i0 + Bg) of the plan out of feats [nrec][T][F] -> the planes (window_assemble_kernel's layout at T = W) and / or
// f32 rows out [Bg][W][F] (planes: optional, the exact projection's operand), zero past each length; lens [Bg] = the lengths; flag
// (planes only, optional, zeroed by the caller): set to 1 if a value is non-finite or outside the f16 range
struct SlidingAssembleArgs {
    SlidingPlan plan; const float *feats; long long i0; int Bg, F;
    int planes; unsigned short *xh, *xl; int Fp, tiles;
    float *out; int *lens; int *flag;
};
hipError_t launch_sliding_assemble(const SlidingAssembleArgs &a, hipStream_t s);
// waveform: the same windows' samples [J Hf j, J Hf j + Sw) of pcm [nrec][S], clipped to S_r, left-aligned into out [Bg][Sw] (zero past
// the clipped length), nsamp_out [Bg] = that length; Sw = R0 + J (W - 1)
struct SlidingWavArgs {
    SlidingPlan plan; const void *pcm; long long i0; int Bg; long long Sw;
    void *out; long long *nsamp_out;
};
hipError_t launch_sliding_wav_gather(const SlidingWavArgs &a, int is_i16, hipStream_t s);
// out [nrec][ld_out] at t < T: the weighted mean over the covering windows of win [N][W] (weights: device [W] or nullptr = ones), +0 at
// t >= T_r and where no planned window covers; frames [nrec] (optional) = T_r
struct SlidingAggregateArgs {
    SlidingPlan plan; const float *win, *weights;
    float *out; int ld_out; int *frames;
};
hipError_t launch_sliding_aggregate(const SlidingAggregateArgs &a, hipStream_t s);

// ---- lstm_stack.hip: every layer of a causal (one-direction, H = 128) stack for T <= LSTM_STACK_TMAX new frames in ONE launch, carried
//      (h, c) updated in place: the streaming step (uvad_stream_step).  Exact f32.
constexpr int LSTM_STACK_TMAX = 4, LSTM_STACK_MAX_LAYERS = 8, LSTM_STACK_MAX_LIN = 4;
struct LstmStackArgs {
    const float *feats; int kin0;                 // canonical [B][T][kin0] f32 features
    const float *wih[LSTM_STACK_MAX_LAYERS];      // register images of W_ih (pack_lstm_image, K = kin0 for layer 0, 128 after)
    const float *whh[LSTM_STACK_MAX_LAYERS];      // register images of W_hh (pack_whh)
    const float *bias[LSTM_STACK_MAX_LAYERS];     // [4H] b_ih + b_hh in (unit, gate) order
    int n_layers;
    float *h, *c; size_t layer_stride;            // carried state [layer][tiles * SEQ_TILE][128] (layer_stride floats apart)
    float *Y; int ldy;                            // last layer's output: f32 rows (tile-major), or
    unsigned short *Yh, *Yl;                      // its two K-blocked f16 planes of ldy columns (Y == nullptr)
    int tiles, T, B;
    // optional head in the same launch (logits != nullptr): n_lin feed-forward layers of 128 units (leaky_relu) as register images
    // (pack_fc_image), the classifier row and bias; logits / probs at canonical [b][t] (b < B), row stride ld_out
    const float *lin_w[LSTM_STACK_MAX_LIN], *lin_b[LSTM_STACK_MAX_LIN]; int n_lin;
    const float *cls_w, *cls_b; float slope;
    float *logits, *probs; int ld_out;
    // optional feature stage in the same launch (fb_on): the step's virtual rows (fb.vs_*: chunk + carried tail) are framed and
    // transformed by the workgroup that consumes them (fbank_pair.h) and `feats` is not read; fb.tab, fb.frame_len, ... as in FbankArgs
    FbankArgs fb; int fb_on;
};
// LDS the feature stage of lstm_stack_kernel needs beside the kernel's static arrays (0 if it cannot run for these arguments)
size_t lstm_stack_fb_lds_bytes(const FbankArgs &fb, int T);
bool lstm_stack_supported(int hidden, int dirs, int in_dim, int T, int n_layers);
hipError_t launch_lstm_stack(const LstmStackArgs &a, hipStream_t s);
// The slot form (uvad_stream_slots_step): the same launch for a pool of B slots with a session each.  st as for a one-launch step with
// the head and the feature stage inside (weights, h / c, head, logits and / or probs, ld_out, tiles, B; fb: the front-end configuration
// and tables only) -- st.T, st.feats, st.Y*, st.fb.vs_* are not read: every slot's T, offset and first-chunk status come from the flag
// bytes and the counters below, on the device.
struct LstmStackSlotsArgs {
    LstmStackArgs st;
    const float *chunk; int chunk_len;            // this step's samples [B][chunk_len]; an idle slot's row is never read
    const uint8_t *flags;                         // [B] UVAD_SLOT_START | UVAD_SLOT_END, or nullptr
    int kmax;                                     // ceil(chunk_len / frame_shift) <= LSTM_STACK_TMAX
    long long *n, *e; int *active;                // per slot: samples and frames since the session's start, whether it holds a session
    float *tail;                                  // [B][frame_len]: the last frame_len samples of each session, updated in place
    int *counts;                                  // [B] frames emitted this step (0 for an idle slot)
};
size_t lstm_stack_slots_lds_bytes(const FbankArgs &fb, int chunk);   // dynamic LDS of the slot form (0 if it cannot run)
hipError_t launch_lstm_stack_slots(const LstmStackSlotsArgs &a, hipStream_t s);
size_t lstm_image_elems(int K);
void pack_lstm_image(const float *w /*[4 * 128][K], torch row order*/, int K, float *out);
size_t fc_image_elems();                                                   // a 128 x 128 feed-forward matrix as a register image
void pack_fc_image(const float *w /*[128][128], torch nn.Linear.weight*/, float *out);

// ---- lens calls of the SincNet stages: the persistent workgroups walk the valid (row, tile) pairs only.  Pair g of the walk is tile
//      g - prefix[b] of the row b with prefix[b] <= g < prefix[b + 1] (prefix: the exclusive prefix of the rows' tile counts, SincGeo); a
//      workgroup finds its first pair with a binary search and steps to the next one, which reads memory only when the row changes.
//      Everything here is wave-uniform (scalar loads).
// The lens conv kernels take their arguments with the rows appended (SincArgsT); the small kernels take the rows as one more argument,
// which is an empty struct in the dense instantiations and adds no kernel-argument bytes.  Either way the dense kernels keep their
// argument layout and code.
struct SincRows { const int *lin, *lpool, *prefix; };   // device int32 [B] Lin_b, [B] Lpool_b, [B + 1] exclusive prefix of the rows' tiles
struct SincNoRows {};
template <class A> struct SincLensArgs : A { SincRows rows; };
template <bool LENS, class A> using SincArgsT = typename std::conditional<LENS, SincLensArgs<A>, A>::type;
template <bool LENS> using SincRowsArg = typename std::conditional<LENS, SincRows, SincNoRows>::type;
template <bool LENS> using SincRowTArg = typename std::conditional<LENS, const int *, SincNoRows>::type;
struct SincRowCursor { int b, tile, end, lin, lpool; };
__device__ __forceinline__ void sinc_cursor_at(const SincRows &r, int b, long long g, SincRowCursor &c) {
    c.b = b; c.tile = (int)(g - r.prefix[b]); c.end = r.prefix[b + 1]; c.lin = r.lin[b]; c.lpool = r.lpool[b];
}
__device__ __forceinline__ SincRowCursor sinc_cursor_seek(const SincRows &r, int B, long long g) {
    int lo = 0, hi = B;   // prefix[lo] <= g < prefix[hi] (prefix[B] = the total > g)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (r.prefix[mid] <= g) lo = mid; else hi = mid;
    }
    SincRowCursor c;
    sinc_cursor_at(r, lo, g, c);
    return c;
}
// c (pair g - 1) -> pair g
__device__ __forceinline__ void sinc_cursor_next(const SincRows &r, long long g, SincRowCursor &c) {
    if (g < c.end) { ++c.tile; return; }
    int b = c.b + 1;
    while (r.prefix[b + 1] <= g) ++b;   // (rows without tiles)
    sinc_cursor_at(r, b, g, c);
}

// ---- sincnet.hip: SincNet front end of PyanNet (conv + |.| + maxpool(3) + instance-norm statistics) ----------
struct SincConvArgs {
    const float *in; long long in_bstride; int Cin, Lin;   // in[b*in_bstride + ci*Lin + x]
    const int16_t *in_i16;                                 // single-channel stage only: the waveform as int16 (read as q / 32768), else null
    const float *in_scale, *in_shift;                      // [B][Cin]: x*scale + shift applied while staging (previous norm)
    int in_lrelu; float slope;                             // then leaky_relu (layers after the first)
    const float *Wt2;                                      // [Kp][NW]: W^T, zero padded (NW = 32*ceil(Cout/32))
    const float *bias;                                     // [NW] zero padded
    int Kw, stride, Ktot, Kp, Cout, do_abs;                // Ktot = Cin*Kw, Kp = Ktot rounded up to a multiple of 8
    int Lconv, Lpool, ntiles;                              // ntiles = ceil(Lpool / plan.pt)
    float *out;                                            // [B][Cout][Lpool] pooled, before the norm
    float *partials;                                       // [B][ntiles][plan.phases][NW][2] (sum, M2 about the group mean) per statistics group
    int B;
    int n_cu;                                              // compute units of the device (persistent grid size); 0 = 256
};
// row_n (lens calls): device int32 [B], row b's statistics over its first row_n[b] samples (0: scale = shift = 0); null = S for every row
hipError_t launch_wav_stats(const float *wav, int B, long long S, long long row_stride, const float *gamma, const float *beta, float eps,
                            float *scale, float *shift, hipStream_t s, const int *row_n = nullptr);
hipError_t launch_wav_stats(const int16_t *wav, int B, long long S, long long row_stride, const float *gamma, const float *beta, float eps,
                            float *scale, float *shift, hipStream_t s, const int *row_n = nullptr);   // int16 samples read as q / 32768
struct SincConvPlan { int waves, pt, phases; };            // waves per workgroup, pooled outputs per tile, statistics groups per tile
SincConvPlan sinc_conv_plan(const SincConvArgs &a);        // needs Cin, Cout, Kw, stride, Kp
hipError_t launch_sinc_conv(const SincConvArgs &a, hipStream_t s, const SincRows *rows = nullptr);   // rows: a lens call (exact-form tiles)
size_t sinc_conv_lds_bytes(const SincConvArgs &a, int NT, int waves);
int sinc_conv_ept(const SincConvArgs &a, int waves);   // window elements per thread held in registers (<= 8 single-channel, <= 48 otherwise)
// rows (lens calls): row b combines its own ntiles_b partials over L_b positions (L_b = 0: scale = shift = 0)
hipError_t launch_norm_finalize(const float *partials, int B, int ntiles, int pt, int phases, int NW, int C, int L, const float *gamma,
                                const float *beta, float eps, float *scale, float *shift, hipStream_t s, const SincRows *rows = nullptr);
// row_T (lens calls): frames t >= row_T[b] are written as +0 (P is not read there)
hipError_t launch_sinc_out(const float *P, const float *scale, const float *shift, int B, int C, int L, float slope, float *feats, int ldf,
                           hipStream_t s, const int *row_T = nullptr);

// Per-row geometry of a lens call (uvad_sincnet_lens): SINC_GEO_ARRAYS int32 arrays of ld = B + 1 entries in the workspace.
//   [0] T_b (frames); stage i: [1 + 6 i] Lin_b, [2 + 6 i] Lpool_b, [3 + 6 i] tiles of the split form (sinc_f16p_ntiles(Lpool_b)),
//   [4 + 6 i] their exclusive prefix over rows (entry B: the total), [5 + 6 i] tiles of the exact form (ceil(Lpool_b / pt_i)), [6 + 6 i] prefix.
// A row with T_b = 0 has 0 in every array: no stage touches it.
constexpr int SINC_GEO_ARRAYS = 19;
struct SincGeoArgs {
    const int64_t *nsamp; int B; long long S;   // lengths clamped to [0, S]
    int kw[3], stride0, pt[3];                  // taps of the stages, the sinc bank's stride, the exact form's pooled outputs per tile
    int *geo;                                   // [SINC_GEO_ARRAYS][B + 1]
};
hipError_t launch_sinc_row_geometry(const SincGeoArgs &g, hipStream_t s);

// ---- sincnet_f16p.hip: the same three stages on the f16 matrix cores (f32-equivalent split arithmetic), channel-minor intermediates ----
struct SincF16Args {
    const float *in; long long in_bstride; int Lin;        // stage 0: in[b * in_bstride + x] (the waveform); stages 1, 2: in[(b * Lin + x) * cst_in + c]
    const int16_t *in_i16;                                 // stage 0 only: the waveform as int16 (read as q / 32768; `in` unused), else null
    const float *in_scale, *in_shift; int n_in;            // [B][n_in]: x * scale + shift applied while staging (n_in = 1, or the real channel count)
    float slope;                                           // leaky_relu of the previous stage (stages 1, 2)
    const unsigned short *Wfrag; float wscale;             // sinc_f16p_pack_weights
    const float *bias;                                     // [cst] zero padded
    int Lpool, ntiles;                                     // ntiles = sinc_f16p_ntiles(Lpool)
    float *out;                                            // [B][Lpool][cst] pooled, before the norm (channels past Cout written as zero)
    float *partials;                                       // [B][ntiles][4 slots][3][cst]: (count, sum, M2 about the set's own mean); slot 0 per tile,
                                                           // stage 0's channels 64 .. 79 one slot per wave
    int B, n_cu;
};
bool sinc_f16p_supported(int n_filters, int kernel_size, int stride, int c2, int k2, int c3, int k3);
int sinc_f16p_ksteps(int stage);       // 32-deep k-steps of the stage's contraction (K = 32 * ksteps: the packed weight row length)
int sinc_f16p_cst(int stage);          // floats per output row (channels padded to whole 16-channel tiles)
int sinc_f16p_ntiles(long long Lpool);
size_t sinc_f16p_partial_floats(int stage, int B, int ntiles);
size_t sinc_f16p_wfrag_elems(int stage);
bool sinc_f16p_pack_weights(int stage, const float *w, int nrows, int ldk, unsigned short *out, float *wscale);
hipError_t launch_sinc_conv_f16p(int stage, const SincF16Args &a, hipStream_t s, const SincRows *rows = nullptr);   // rows: split-form tiles
hipError_t launch_norm_finalize_f16p(int stage, const float *partials, int B, int ntiles, int C, int L, const float *gamma, const float *beta, float eps,
                                     float *scale, float *shift, hipStream_t s, const SincRows *rows = nullptr);
hipError_t launch_sinc_out_f16p(const float *P, const float *scale, const float *shift, int B, int C, int CST, int L, float slope, float *feats, int ldf,
                                hipStream_t s, const int *row_T = nullptr);

// ---- ingest.hip: the ingest stage (uvad_ingest*, include/uvad.h): decode, de-interleave and polyphase resampling to 16 kHz ----
// Output sample o = j up + p of a row is the f32 fma chain, k ascending from +0, over x[j down + k - shift] taps[p][k], k < K = 2 width +
// down; x is the decoded channel, zero outside [0, n), and for a stream step the row's history at negative indices.  shift = width for
// the dense and ragged forms, Dj down + width = H for a stream step (the output delayed by Dj up samples).
constexpr int INGEST_MAX_PHASES = 8, INGEST_MAX_TAPS = 64, INGEST_MAX_CHANNELS = 8;
struct IngestArgs {
    const void *in; int enc, C; long long S_in;      // in[(b S_in + f) C + c] in the source encoding (UVAD_INGEST_*), S_in frames per row
    const long long *nsamp;                          // ragged: device int64 [B] frames per row, clamped to [0, S_in]; null: S_in
    const float *taps; int up, down, width, K;       // taps[up][K] on the device; null: the 1/1 pass (up = down = K = 1, width = 0)
    float *out; long long S_out;                     // out[(b C + c) S_out + o]
    long long *out_nsamp;                            // ragged: [B C] = ceil(up n_b / down), repeated per channel; else null
    float *hist; long long *seen; const uint8_t *flags; int H, Dj;   // stream: hist [B C][H] decoded samples, seen [B C] output groups
                                                                     // since the session's start (saturating at Dj), flags [B C] or null
    int B;
};
hipError_t launch_ingest(const IngestArgs &a, hipStream_t s);

// ---- state_reset.hip: the one reset of the device states that are a 256-byte header followed by slots that start as zeros ------------------
// (EndpointHeader, EndpointHystHeader, GateHeader, GateGroupHeader).  A launcher fills its header struct by field name -- the struct the
// step kernel reads by field name -- and hands it over as 64 words in the kernel's arguments; the kernel writes word i of the header for
// i < 64 and zero for the n_words - 64 words of the slots.  What follows the slots (the gates' rings) is not touched.
struct HeaderWords { unsigned w[64]; };
template <class H> inline HeaderWords header_words(const H &h) {
    static_assert(sizeof(H) == 256 && sizeof(HeaderWords) == 256 && std::is_trivially_copyable<H>::value, "a state header is 256 bytes of plain words");
    HeaderWords o;
    __builtin_memcpy(&o, &h, sizeof(o));
    return o;
}
hipError_t launch_state_reset(void *state, const HeaderWords &h, long long n_words, hipStream_t s);

// ---- endpoint.hip: the live endpointer (uvad_endpoint_*, include/uvad.h): streaming median, runs and the padded merge, one slot per feed ----
// The state is a header (what reset fixed: B and the configuration, so a step carries none) followed by one EndpointSlot per slot.
// hist[0 .. n), n = ceil(2 h / 64), holds the thresholded frames before the slot's frame m as a bit string that ENDS at the top bit of
// word n - 1 (frame m - 1); only its newest 2 h bits are ever read, and a new session starts from all zeros -- the median's zero padding
// on the left.
constexpr int EP_HIST_WORDS = 4;                      // 2 h <= 254 bits
constexpr unsigned EP_MAGIC = 0x55564550u;            // "UVEP"
constexpr int EP_IDLE = 0, EP_SPEECH = 1, EP_PENDING = 2;
constexpr int EP_MAX_LD_IN = 1 << 18;                 // the step keeps the step's bits in LDS: 8 bytes per 64 frames
struct EndpointHeader { unsigned magic; int B, kernel, pad; float threshold; int reserved[59]; };   // 256 bytes
struct EndpointSlot {
    unsigned long long hist[EP_HIST_WORDS];
    int m;        // frames of the session so far (saturates at 2^31 - 1: frames past that are not consumed)
    int st;       // EP_IDLE / EP_SPEECH (inside a run) / EP_PENDING (a run closed at frame c, its padded end not yet decided)
    int c;        // EP_PENDING: the first non-speech frame after the last run
    int reserved;
};
struct EndpointArgs {
    const float *probs; int ld_in; const int *counts; const uint8_t *flags; int B;
    void *state;
    int *events; int max_events; int *ev_counts; uint8_t *active;
    uint8_t *labels; int ld_lab; int *lab_counts;
};
size_t endpoint_state_bytes(int B);
hipError_t launch_endpoint_reset(void *state, int B, int kernel, int pad, float threshold, hipStream_t s);
hipError_t launch_endpoint_step(const EndpointArgs &a, int kernel, hipStream_t s);   // kernel: the reset's, for the LDS size only

// ---- score.hip: scoring against reference labels (uvad_score_*, uvad_intervals_to_labels, include/uvad.h) ---------------------------------
// The state is a 256-byte header followed by the record uvad_score_totals copies out (SC_* word offsets, include/uvad.h).  The workspace
// is a 32-byte head (this step's loss sum and valid frames) followed by one ScorePartial per (row, segment).
constexpr int SC_MAX_POINTS = 8, SC_MAX_BINS = 1024, SC_MAX_COLLAR = 1024, SC_MAX_SEGMENT = 1 << 14, SC_DEFAULT_SEGMENT = 2048;
constexpr int SC_MAX_T = 1 << 30;                     // frame arithmetic stays in int32 with a segment and two halos on top
constexpr unsigned SC_MAGIC = 0x55565343u;            // "UVSC"
constexpr int SC_W_POINTS = 0, SC_W_BINS = 1, SC_W_VALID = 2, SC_W_LOSS = 3, SC_W_STEPS = 4, SC_W_COUNTS = 8, SC_W_HIST = 40;
constexpr int SC_RECORD_WORDS = SC_W_HIST + 2 * SC_MAX_BINS;   // == UVAD_SCORE_TOTALS_WORDS
struct ScoreHeader { unsigned magic; int n_points, bins, reserved[61]; };   // 256 bytes
struct ScoreWsHead { double loss; unsigned long long valid; unsigned long long reserved[2]; };
struct ScorePartial { double loss; unsigned tp, fp, tn, fn; unsigned reserved[2]; };   // point 0's counts and the loss of one (row, segment)
struct ScoreArgs {
    const float *probs; int ld_p; const uint8_t *gt; int ld_gt; int B, T; const int *lens;
    void *state; unsigned long long *rows; void *ws;
    int n_points; float thr[SC_MAX_POINTS]; int half[SC_MAX_POINTS];
    int collar, bins, seg, halo, nseg;
};
constexpr size_t score_state_bytes() { return sizeof(ScoreHeader) + (size_t)SC_RECORD_WORDS * sizeof(unsigned long long); }
constexpr int score_nseg(int T, int seg) { return (T + seg - 1) / seg; }
constexpr size_t score_ws_bytes(int B, int T, int seg) { return sizeof(ScoreWsHead) + (size_t)B * score_nseg(T, seg) * sizeof(ScorePartial); }
hipError_t launch_score_reset(void *state, int n_points, int bins, hipStream_t s);
hipError_t launch_score_step(const ScoreArgs &a, hipStream_t s);
hipError_t launch_score_totals(const void *state, unsigned long long *out, hipStream_t s);
hipError_t launch_intervals_to_labels(const int *iv, const int *iv_counts, int B, int max_iv, int T, int ld, const int *lens, uint8_t *labels,
                                      hipStream_t s);

// ---- cuts.hip: speech cuts (uvad_cuts_*, include/uvad.h): the cut table of a batch of label rows and the gather of the cuts' audio ----------
// The workspace is 2 B int32 {cuts, stored intervals} per row, rounded up to 16 bytes, followed by (T + 1) / 2 CutsInterval per row: the
// row's merged intervals that keep at least one piece, in order, with the index of their first piece within the row.
constexpr int CUTS_MAX_T = 1 << 30;                   // frame arithmetic stays in int32 with a pad and a pass on top
constexpr int CUTS_MAX_PAD = 1 << 20, CUTS_MAX_LEN = 1 << 24;
constexpr int CUTS_SPAN_WORDS = 64;                   // 64-frame words per pass of a row: 4096 frames
constexpr int CUTS_ROWS_THREADS = 320;                // cuts_rows_kernel: wave 0 walks a pass, waves 1 .. 4 load the next
constexpr int CUTS_TILE_BYTES = 65536;                // of an output row per (cut, tile) pair of the gather
constexpr int CUTS_MAX_BLOCKS = 1 << 16;              // grids are capped: the write and gather kernels stride over their items
struct CutsCfgInt { int pad, max_len, min_len, hop, lead, tail; };   // uvad_cuts_cfg, field for field
struct alignas(16) CutsInterval { int lo, hi, base, reserved; };
struct CutRecord { int row, index, first_frame, n_frames; long long first_sample, n_samples; };   // uvad_cut, field for field
struct CutsTableArgs {
    const uint8_t *labels; int ld, B, T; const int *lens; const long long *nsamp; long long S;
    CutsCfgInt q;
    CutRecord *table; int max_cuts; int *row_first, *total;
    int *counts; CutsInterval *iv; int cap;           // the workspace: [B][2], [B][cap], cap = (T + 1) / 2
};
struct CutsGatherArgs {
    const void *src; long long row_stride; int unit_bytes, frames;   // frames: ranges from first_frame / n_frames, records of unit_bytes
    const CutRecord *table; const int *total; int max_cuts;
    void *out; long long ld_out; int *out_len; int tiles;
};
constexpr size_t cuts_counts_bytes(int B) { return ((size_t)B * 2 * sizeof(int) + 15) / 16 * 16; }
constexpr size_t cuts_ws_bytes(int B, int T) { return cuts_counts_bytes(B) + (size_t)B * ((T + 1) / 2) * sizeof(CutsInterval); }
constexpr int cuts_gather_tiles(long long ld_out, int unit_bytes) { return (int)((ld_out * unit_bytes + CUTS_TILE_BYTES - 1) / CUTS_TILE_BYTES); }
int cuts_max_per_row(const CutsCfgInt &q, int T);
hipError_t launch_cuts_table(const CutsTableArgs &a, hipStream_t s);
hipError_t launch_cuts_gather(const CutsGatherArgs &a, hipStream_t s);

// ---- join.hip: the cut-supervision join (uvad_cuts_join, include/uvad.h): which items of its row each cut of a cut table matches -----------
// The workspace is one int32 per cut (its number of pairs), rounded up to 16 bytes, followed by max_cuts + 1 int32: the exclusive prefix
// of the cuts without a pair, from which a row's empty cuts are one subtraction.
constexpr int JOIN_AUDIT_WORDS = 8;                   // UVAD_JOIN_AUDIT_WORDS
struct JoinArgs {
    const CutRecord *table; const int *row_first, *total; int max_cuts, B;
    const int *iv, *iv_counts; int max_iv, inside;    // inside: UVAD_JOIN_INSIDE, else UVAD_JOIN_OVERLAP
    int *pair_first, *pairs; int max_pairs; int *item_cuts; unsigned long long *audit;
    int *counts, *empty_first;                        // the workspace: [max_cuts], [max_cuts + 1]
};
constexpr size_t join_counts_bytes(int max_cuts) { return ((size_t)max_cuts * sizeof(int) + 15) / 16 * 16; }
constexpr size_t join_ws_bytes(int max_cuts) { return join_counts_bytes(max_cuts) + (((size_t)max_cuts + 1) * sizeof(int) + 15) / 16 * 16; }
hipError_t launch_cuts_join(const JoinArgs &a, hipStream_t s);

// ---- fuse.hip: channel fusion (uvad_fuse_*, include/uvad.h): one row per group of input rows, and the channel of each cut ---------------------
// The configuration (group_first [G + 1], members [N], weights [N] or none) lives on the device with the context.  The workspace of
// uvad_fuse is, per member slot, one FusePartial per wave of every frame tile: [N][fuse_tiles(T) * FUSE_WAVES], 16 bytes each.
constexpr int FUSE_MAX_T = 1 << 30;
constexpr int FUSE_MAX_MEMBERS = 255;                 // per group: a position fits d_best's byte
constexpr int FUSE_THREADS = 256, FUSE_WAVES = FUSE_THREADS / 64;
constexpr int FUSE_TILE = FUSE_THREADS * 4;           // frames per workgroup pass: four consecutive frames a lane (one 16-byte load)
constexpr int FUSE_MAX_BLOCKS = 1 << 16;              // grids are capped: workgroups stride over their (group, tile) items
constexpr int FUSE_STATS_WORDS = 4;                   // valid, speech, agree, best
struct FuseCfgInt { int mode; float threshold, decide; };   // uvad_fuse_cfg, field for field
struct FusePartial { unsigned valid, speech, agree, best; };
struct FuseArgs {
    const int *first, *members; const float *weights; int G, N;   // the configuration on the device (weights may be null: all ones)
    FuseCfgInt q;
    const float *in; int ld_in, T; const int *lens; const uint8_t *flags_in;
    float *fused; int ld_f; int *glens; uint8_t *flags_out; uint8_t *labels; int ld_l; uint8_t *best; int ld_b;
    unsigned long long *stats; FusePartial *part; int tiles;
};
struct FusePickArgs {
    const int *first, *members; int G;
    const uint8_t *best; int ld_b; const CutRecord *table; const int *total; int max_cuts; CutRecord *out_table; int *pick;
};
constexpr int fuse_tiles(int T) { return (T + FUSE_TILE - 1) / FUSE_TILE; }
constexpr size_t fuse_ws_bytes(int N, int T) { return (size_t)N * fuse_tiles(T) * FUSE_WAVES * sizeof(FusePartial); }
hipError_t launch_fuse(const FuseArgs &a, hipStream_t s);
hipError_t launch_fuse_pick(const FusePickArgs &a, hipStream_t s);

// ---- binarize.hip: hysteresis decisions with minimum durations (uvad_binarize, include/uvad.h) -------------------------------------------
// The workspace is (T + 63) / 64 word pairs {HI mask, LO mask} per row (16 bytes a pair), followed by (T + 1) / 2 int32 pairs {lo, hi}
// per row: the row's full interval list, which the labels are made from.
constexpr int BIN_MAX_T = 1 << 30;                    // frame arithmetic stays in int32 with two pads, a pause and a pass on top
constexpr int BIN_MAX_FRAMES = 1 << 20;               // min_on, min_off, pad_on, pad_off
constexpr int BIN_SEG = 2048;                         // frames per workgroup of binarize_classify_kernel
constexpr int BIN_SPAN_WORDS = CUTS_SPAN_WORDS;       // 64-frame words per pass of binarize_rows_kernel: 4096 frames
struct BinCfgInt { float onset, offset; int min_on, min_off, pad_on, pad_off; };   // uvad_binarize_cfg, field for field
struct BinarizeArgs {
    const float *probs; int ld_p, B, T; const int *lens;
    BinCfgInt q;
    int *iv; int max_iv; int *iv_counts;
    unsigned long long *words; int *list; int nwt, cap;   // the workspace: [B][nwt][2], [B][cap][2]; nwt = (T + 63) / 64, cap = (T + 1) / 2
};
constexpr int bin_words(int T) { return (T + 63) / 64; }
constexpr size_t bin_words_bytes(int B, int T) { return (size_t)B * bin_words(T) * 16; }
constexpr size_t bin_ws_bytes(int B, int T) { return bin_words_bytes(B, T) + (size_t)B * ((T + 1) / 2) * 2 * sizeof(int); }
hipError_t launch_binarize(const BinarizeArgs &a, uint8_t *labels, int ld, hipStream_t s);   // labels may be NULL

// ---- endpoint_hyst.hip: the live hysteresis endpointer (uvad_endpoint_hyst_*, include/uvad.h): uvad_binarize's decisions as per-feed events ----
// The state is a header (what reset fixed: B and the uvad_binarize_cfg, so a step carries none) followed by one EndpointHystSlot per slot.
// The hysteresis state is causal, so a slot keeps no frames at all: seven integers.  It takes EndpointArgs, as the median endpointer's step.
constexpr unsigned EPH_MAGIC = 0x55564548u;           // "UVEH"
struct EndpointHystHeader { unsigned magic; int B; BinCfgInt q; int reserved[56]; };   // 256 bytes
struct EndpointHystSlot {
    int m;        // frames of the session so far (saturates at 2^31 - 1: frames past that are not consumed)
    int F;        // the label frontier: the session's labels are final on [0, F), F <= m
    int lo;       // SPEECH / PENDING: the interval's first frame, the first run's start less pad_on, clipped at 0
    int c;        // PENDING: the first non-speech frame after the last run
    int mode;     // EP_IDLE / EP_SPEECH (inside a run) / EP_PENDING (a run closed at frame c, the interval's end not yet decided)
    int conf;     // SPEECH / PENDING: 1 once START(lo) has been issued (the interval has min_on frames)
    int s;        // the hysteresis state of frame m - 1 (0 before the first frame)
    int reserved;
};                // 32 bytes
size_t endpoint_hyst_state_bytes(int B);
hipError_t launch_endpoint_hyst_reset(void *state, int B, const BinCfgInt &q, hipStream_t s);
hipError_t launch_endpoint_hyst_step(const EndpointArgs &a, hipStream_t s);

// ---- gate.hip: the live speech gate (uvad_gate_*, include/uvad.h): each feed's speech audio per step, the streaming uvad_cuts_* ------------
// The state is a header (what reset fixed: B, the uvad_cuts_cfg, the unit size and the ring's length, so a step carries none), one GateSlot
// per slot, then one ring of `history` units per slot, each rounded up to 16 bytes so that every ring starts as aligned as the state does.
constexpr unsigned GATE_MAGIC = 0x55564754u;          // "UVGT"
constexpr int GATE_MAX_CHUNK = 1 << 24;
constexpr int GATE_THREADS = 256;                     // one workgroup per slot, and per group of the group gate
constexpr int GATE_LAB_TILE = 1024;                   // labels staged in LDS per round of the walk
struct GateHeader { unsigned magic; int B; CutsCfgInt q; int unit_bytes, history; long long ring_bytes; int reserved[52]; };   // 256 bytes
struct GateSlot {
    long long A;      // samples of the session so far
    long long sent;   // samples of the current piece delivered so far (the next fragment's offset)
    int F;            // labels of the session so far (saturates at 2^31 - 1: labels past that are not consumed)
    int c;            // PENDING: the first non-speech frame after the last run
    int pf;           // the current piece's first frame (OPEN / PENDING)
    int idx;          // the current piece's index within the session
    int mode;         // EP_IDLE / EP_SPEECH (inside a run) / EP_PENDING
    int started;      // 1 once the current piece has a record (the next one carries no FIRST)
    int live;         // 1 from a START step to the END step: an idle slot reads no input and emits nothing
    int wp;           // the ring's write position, 0 .. history - 1; it runs on across sessions
    int reserved[4];
};                    // 64 bytes
struct GateSeg { int index, flags, first_frame, n_frames; long long offset; int n, n_stored; };   // uvad_gate_seg, field for field
struct GateArgs {
    const void *chunk; int chunk_n; const uint8_t *labels; int ld_lab; const int *lab_counts; const uint8_t *flags; int B;
    void *state; void *out; long long ld_out; GateSeg *seg; int max_seg; int *seg_counts;
};
constexpr size_t gate_ring_bytes(int unit_bytes, long long history) { return ((size_t)history * unit_bytes + 15) / 16 * 16; }
constexpr size_t gate_state_bytes(int B, int unit_bytes, long long history) {
    return sizeof(GateHeader) + (size_t)B * (sizeof(GateSlot) + gate_ring_bytes(unit_bytes, history));
}
hipError_t launch_gate_reset(void *state, int B, const CutsCfgInt &q, int unit_bytes, int history, hipStream_t s);
hipError_t launch_gate_step(const GateArgs &a, int unit_bytes, hipStream_t s);   // unit_bytes: the reset's, it picks the copy's granule

// ---- gate_group.hip: the live speech gate for fused groups (uvad_gate_group_*, include/uvad.h): each cut from the channel that heard it best ----
// The state is a header (what reset fixed: G and N of the fusion configuration, the uvad_cuts_cfg, the unit size, the two ring lengths and
// the decision horizon), one GateGroupSlot per group, one ring of `best_history` bytes per group, then one ring of `history` units per
// MEMBER SLOT (a row that sits in several groups is kept once per slot); every ring is rounded up to 16 bytes.  The rings of a group's
// members share the group's write position: its members receive the same chunk count every step.
constexpr unsigned GATE_GROUP_MAGIC = 0x55564747u;    // "UVGG"
constexpr int GATE_GROUP_UNSYNC = 16;                 // UVAD_GATE_UNSYNC
struct GateGroupHeader {
    unsigned magic; int G, N; CutsCfgInt q; int unit_bytes, history, best_history, decide, reserved0;
    long long ring_bytes, best_bytes; int reserved[46];
};                    // 256 bytes
struct GateGroupSlot {
    long long A;      // samples of the session so far (of every member)
    long long sent;   // samples of the current piece delivered so far
    long long Fb;     // `best` bytes of the session so far
    int F, c, pf, idx, mode;   // as GateSlot
    int started;      // 1 once the current piece has a record, which is when its channel was chosen
    int live;
    int wp;           // the PCM rings' write position, 0 .. history - 1; it runs on across sessions
    int bwp;          // the best ring's write position, 0 .. best_history - 1; it runs on across sessions
    int ch;           // started: the member position the current piece takes its audio from
    int unsync;       // 1 from the step in which the members' flag bytes differed to the session's END
    int reserved[7];
};                    // 96 bytes
struct GateGroupArgs {
    const int *first, *members; int G, N;             // the fusion configuration on the device
    const void *chunk; int chunk_n, B;
    const uint8_t *best; int ld_best; const int *best_counts;
    const uint8_t *labels; int ld_lab; const int *lab_counts; const uint8_t *gflags, *rflags;
    void *state; void *out; long long ld_out; GateSeg *seg; int max_seg; int *seg_counts;
};
constexpr size_t gate_group_best_bytes(long long best_history) { return ((size_t)best_history + 15) / 16 * 16; }
constexpr size_t gate_group_state_bytes(int G, int N, int unit_bytes, long long history, long long best_history) {
    return sizeof(GateGroupHeader) + (size_t)G * (sizeof(GateGroupSlot) + gate_group_best_bytes(best_history)) +
           (size_t)N * gate_ring_bytes(unit_bytes, history);
}
hipError_t launch_gate_group_reset(void *state, int G, int N, const CutsCfgInt &q, int unit_bytes, int history, int best_history, int decide,
                                   hipStream_t s);
hipError_t launch_gate_group_step(const GateGroupArgs &a, int unit_bytes, hipStream_t s);

// ---- head_train.hip: fine-tuning of the head (uvad_head_train_*, include/uvad.h): forward with kept activations, loss gradient, backward, Adam ----
// Frames are flat, n = b T + t.  The trainable tensors are packed in state_dict order (linear.l.weight [H][K_l], linear.l.bias [H], ...,
// classifier.weight [K_L], classifier.bias [1]; K_1 = D0, K_l = H after), P floats, padded to Pp = a multiple of 64.
// State: HeadTrainHeader (256 bytes) | masters [Pp] | gradient accumulator [Pp] | m [Pp] | v [Pp].
// Workspace: HeadTrainWsHead (256 bytes) | valid [N] bytes | dz [N] | activations [L][N][H] | two gradient buffers [N][H] (L > 0) |
//            gradient partials [nseg][Pp] | loss partials [ceil(N / 256)] doubles; every part 256-byte aligned.
constexpr int HT_MAX_LAYERS = 4, HT_MAX_HIDDEN = 256, HT_MAX_D0 = 2048;
constexpr int HT_MIN_SEGMENT = 32, HT_MAX_SEGMENT = 1 << 14, HT_DEFAULT_SEGMENT = 2048;
constexpr int HT_MAX_FRAMES = 1 << 24;               // B x T: flat frame arithmetic stays in int32
constexpr int HT_LOSS_BLOCK = 256;                   // frames per loss partial
constexpr unsigned HT_MAGIC = 0x55564854u;           // "UVHT"
constexpr int HT_SCALAR_WORDS = 8;                   // UVAD_HEAD_TRAIN_SCALAR_WORDS
struct HeadTrainShape {
    int D0, H, L, P, Pp;
    int off_w[HT_MAX_LAYERS + 1], off_b[HT_MAX_LAYERS + 1];   // entry L: the classifier
    float slope;
};
struct HeadTrainHeader {
    unsigned magic; int D0, H, L, P, pad0;
    double loss; unsigned long long frames, t;       // accumulated since the last step: loss sum, valid frames; steps taken
    // the bias corrections 1 - beta1^t, 1 - beta2^t, advanced once per step as c <- c beta + (1 - beta) from 0: one captured graph serves
    // every step, and the value keeps f32 relative accuracy.  (The running PRODUCT beta^t of the f32 nearest to 0.999 is 1.3e-8 off per
    // factor, which 1 - beta^t magnifies to 1.3e-5 at every t: the loss of a 20-step run then drifts 1e-3 from torch's, not 1e-6.)
    float bc1, bc2;
    unsigned long long draws;                        // byte 56, LSTM training states only: dropout masks drawn so far (the draw ordinal)
    int reserved[48];
};                                                   // 256 bytes
struct HeadTrainWsHead { double loss; unsigned long long frames; int reserved[60]; };   // of the last uvad_head_train_grad
struct HeadTrainWs { size_t off_valid, off_dz, off_act, off_d[2], off_part, off_loss, total; int N, nseg; };
struct HeadTrainGradArgs {
    const float *x; int B, T; const int *lens;
    const uint8_t *gt; int ld_gt; const float *fw; int ld_fw; const float *dz_in; int ld_dz;
    float *probs; int ld_p; float *grad_x;
    void *state; void *ws; int seg;
};
struct HeadTrainAdam { float lr, b1, b2, eps, omb1, omb2; };
struct HeadTrainInit { const float *w[HT_MAX_LAYERS + 1], *b[HT_MAX_LAYERS + 1]; int ldw[HT_MAX_LAYERS + 1]; };   // the context's device copies
HeadTrainShape head_train_shape(int D0, int H, int L, float slope);
size_t head_train_state_bytes(const HeadTrainShape &q);
HeadTrainWs head_train_ws(const HeadTrainShape &q, long long N, int seg);
hipError_t launch_head_train_reset(const HeadTrainShape &q, const HeadTrainInit &in, void *state, hipStream_t s);
hipError_t launch_head_train_grad(const HeadTrainShape &q, const HeadTrainGradArgs &a, hipStream_t s);
// One training state of any family (head, LSTM, SincNet): the layout above under the family's magic word; state == nullptr: absent.  What works
// on the blocks alone is launched once for all three, from optim.hip:
//   apply  ht_adam_kernel, then the one-workgroup ht_adam_commit_kernel
//   read   which = MASTERS / GRAD / M / V: the block's P floats; SCALARS: the family's scalar record
//   write  MASTERS / M / V: P floats into that block; SCALARS: t, bc1, bc2 from the record's words (an LSTM state: the draw ordinal too)
struct TrainBlock { void *state; unsigned magic; int P, Pp; };
hipError_t launch_train_apply(const TrainBlock &b, const HeadTrainAdam &o, hipStream_t s);
hipError_t launch_train_read(const TrainBlock &b, int which, float *out, hipStream_t s);
hipError_t launch_train_write(const TrainBlock &b, int which, const float *in, hipStream_t s);

// ---- lstm_train.hip: training of the top LSTM layers (uvad_lstm_train_*, include/uvad.h): forward with kept activations, BPTT, Adam ----
// Layers first_layer .. num_layers - 1 learn; nl of them, layer index li = 0 .. nl - 1 from the bottom.  Frames are flat, n = b T + t, N = B T.
// The trainable tensors are packed in state_dict order -- per layer, forward then _reverse: weight_ih [4H][in], weight_hh [4H][H],
// bias_ih [4H], bias_hh [4H] (in = Din for li = 0, H x dirs above) -- P floats, padded to Pp = a multiple of 64.
// State: HeadTrainHeader with LT_MAGIC (256 bytes) | masters [Pp] | gradient accumulator [Pp] | m [Pp] | v [Pp]: the head's layout (TrainBlock).
// Workspace: LstmTrainWsHead (256 bytes: magic, B, T) | HeadTrainWsHead (the fold's record of the last backward) | valid [N] bytes |
//            b_ih + b_hh [nl][dirs][4H] | per layer: gates [dirs][N][4H] (pre-activations, then i f g o, then dpre), c [dirs][N][H],
//            h_prev [dirs][N][H], and below the top layer its output h [N][H dirs] | two gradient buffers [N][H dirs] (nl > 1) |
//            gradient partials [nseg][Pp]; every part 256-byte aligned.
constexpr int LT_MAX_LAYERS = 8, LT_MAX_DIN = 2048;
constexpr unsigned LT_MAGIC = 0x55564C54u;           // "UVLT": the state
constexpr int LT_WS_MAGIC = 0x4C545753;              // "LTWS": a workspace whose kept activations belong to (B, T)
constexpr int LT_SCALAR_WORDS = 10;                  // UVAD_LSTM_TRAIN_SCALAR_WORDS: the head's eight, then the draw ordinal
struct LstmTrainShape {
    int Din, H, dirs, nl, first_layer, P, Pp;
    int in[LT_MAX_LAYERS];                           // input width of layer li
    int off[LT_MAX_LAYERS][2][4];                    // weight_ih, weight_hh, bias_ih, bias_hh of (li, direction)
};
// written by the forward call, checked by every backward kernel.  draw .. seed (bytes 16 .. 39) are the dropout record of that forward
// call: the backward call's masks come from here alone; thr == 0 means that forward call dropped nothing.
struct LstmTrainWsHead {
    int magic, B, T, pad0;
    unsigned long long draw; unsigned thr; float scale; unsigned long long seed;
    int reserved[54];
};
struct LstmTrainWs {
    size_t off_fold, off_valid, off_bsum, off_gates[LT_MAX_LAYERS], off_c[LT_MAX_LAYERS], off_hprev[LT_MAX_LAYERS], off_h[LT_MAX_LAYERS], off_d[2],
        off_part, total;
    int N, nseg;
};
struct LstmTrainArgs {
    const float *x; const float *dy; int B, T; const int *lens;
    float *y; float *grad_in;
    void *state; void *ws; int seg;
    unsigned thr; float scale; unsigned long long seed;   // forward: the dropout setting (thr == 0: off, today's launches)
    bool drop;                                       // backward: launch the dropout stage (it reads the workspace header's record)
};
LstmTrainShape lstm_train_shape(int Din, int H, int dirs, int num_layers, int first_layer);
size_t lstm_train_state_bytes(const LstmTrainShape &q);
LstmTrainWs lstm_train_ws(const LstmTrainShape &q, long long N, int seg);
hipError_t launch_lstm_train_reset(const LstmTrainShape &q, void *state, hipStream_t s);   // masters are copied in by the caller
hipError_t launch_lstm_train_forward(const LstmTrainShape &q, const LstmTrainArgs &a, hipStream_t s);
hipError_t launch_lstm_train_backward(const LstmTrainShape &q, const LstmTrainArgs &a, hipStream_t s);
// the dropout mask of include/uvad.h as a stand-alone pass: out = keep ? x scale : +0 over [rows][cols]; in place when out == x
constexpr int LT_DROP_MAX_COLS = 2048, LT_DROP_MAX_LAYER = 65535;
unsigned lstm_dropout_threshold(float p);            // floor((double)p 2^32)
hipError_t launch_dropout_apply(const float *x, float *out, long long rows, int cols, int layer, unsigned long long draw, unsigned thr, float scale,
                                unsigned long long seed, hipStream_t s);

// ---- sincnet_train.hip: training of the SincNet front end (uvad_sincnet_train_*, include/uvad.h): forward with kept activations, backward, Adam ----
// Stages first_stage .. 2 learn.  The 14 tensors in state_dict order (SNT_T_*): wav_norm1d.weight, .bias, conv1d.0.filterbank.low_hz_, band_hz_
// (stage 0), conv1d.1.weight, .bias (stage 1), conv1d.2.weight, .bias (stage 2), norm1d.s.weight, .bias (stage s); the learning ones packed in
// that order are the P floats of the Adam block, padded to Pp = a multiple of 64.
// State: HeadTrainHeader with SNT_MAGIC (256 bytes) | masters [Pp] | gradient accumulator [Pp] | m [Pp] | v [Pp] (the head's layout: TrainBlock) |
//        the bank [n_filters][kernel_size] the last forward call ran (padded to 64 floats) |
//        all 14 tensors as reset found them, in order (the frozen stages run from here; padded) | window_ [kernel_size / 2] | n_ [kernel_size / 2]
//        (each padded to 64 floats).
// Workspace: SincTrainWsHead (256 bytes: magic ^ high word of S, B, S) | HeadTrainWsHead (the fold's record) | row statistics [B][4] | per stage:
//            pooled values [B][Cout][Lp], winner bytes [B][Cout][Lp], mean / rstd [B][Cout][2], and for a learning stage the gradient buffer
//            [B][Cout][Lp] (d_a_out, then dp in place) | the rows' shares of d gamma / d beta [B][max Cout][2] | gradient partials [nseg][Pp] |
//            stage 0 learning: its partials of G and D [nseg][GS] and their fold [GS], GS = n_filters (kernel_size + 1) padded to 64; every part
//            256-byte aligned.  nseg = ceil(B 3 Lp_first_stage / segment): the segments run over the flat conv positions of the lowest learning stage.
constexpr unsigned SNT_MAGIC = 0x5556534Eu;          // "UVSN": the state
constexpr int SNT_WS_MAGIC = 0x534E5753;             // "SNWS": a workspace whose kept activations belong to (B, S)
constexpr int SNT_TENSORS = 14, SNT_T_WAV = 0, SNT_T_LOW = 2, SNT_T_BAND = 3, SNT_T_CONV = 4, SNT_T_NORM = 8;
constexpr int SNT_MAX_B = 65535;                     // rows are a grid dimension
struct SincTrainShape {
    int first_stage, P, Pp, Pfull, Pfullp;
    int NF, KS, stride;
    int Cin[3], Cout[3], Kw[3];
    int cnt[SNT_TENSORS], stage_of[SNT_TENSORS], off_full[SNT_TENSORS], off_master[SNT_TENSORS];   // off_master: -1 for a frozen tensor
    int bankp, halfp, off_bank, off_fullblock, off_win, off_n;   // in floats behind the header
    float slope, eps;
};
struct SincTrainGeo { long long Lin[3], L[3], Lp[3]; bool ok; };   // ok: at least one frame
struct SincTrainWsHead { int magic, B, S_lo, S_hi; int reserved[60]; };
struct SincTrainWs { size_t off_fold, off_wstat, off_p[3], off_idx[3], off_stat[3], off_g[3], off_nb, off_part, off_partG, off_Gf, total; int nseg, GS; };
struct SincTrainArgs {
    const float *wav; const float *dfeats; int B; long long S;
    float *feats;
    void *state; void *ws; int seg;
};
SincTrainShape sinc_train_shape(int n_filters, int kernel_size, int stride, int c2, int k2, int c3, int k3, float slope, float eps, int first_stage);
size_t sinc_train_state_bytes(const SincTrainShape &q);
SincTrainGeo sinc_train_geo(const SincTrainShape &q, long long S);
SincTrainWs sinc_train_ws(const SincTrainShape &q, const SincTrainGeo &geo, int B, int seg);
hipError_t launch_sinc_train_forward(const SincTrainShape &q, const SincTrainArgs &a, hipStream_t s);
hipError_t launch_sinc_train_backward(const SincTrainShape &q, const SincTrainArgs &a, hipStream_t s);
hipError_t launch_sinc_train_bank(const SincTrainShape &q, void *state, hipStream_t s);   // the bank from the masters as they stand
hipError_t launch_sinc_train_read_bank(const SincTrainShape &q, const void *state, float *out, hipStream_t s);   // _read's which 5: the bank

// ---- optim.hip: the joint optimizer step over the three training states (uvad_optim_*, include/uvad.h); the launch_train_* above live there too ----
// State: OptimHeader (256 bytes) | the learning-rate table [cap] f32, padded to 64 floats.  cap is the n_lr of uvad_optim_reset (the shape the
// kernels check beside the magic word), n <= cap the entries in use.
// Workspace: one double per chunk of OPT_CHUNK parameters, the chunks of the head first, then the LSTM's, then SincNet's; padded to 256 bytes.
constexpr unsigned OPT_MAGIC = 0x55564F50u;          // "UVOP"
constexpr int OPT_CHUNK = 4096;                      // parameters per sum-of-squares partial: 256 lanes x 16 passes
constexpr int OPT_RECORD_WORDS = 8;                  // UVAD_OPTIM_RECORD_WORDS
constexpr int OPT_MAX_LR = 1 << 24;
struct OptimHeader {
    unsigned magic; int cap, n, decoupled, skip_nonfinite;
    float b1, b2, eps, omb1, omb2, max_norm, wd;     // byte 20
    float lr_scale[3];                               // byte 48
    int pad0;
    unsigned long long t, skipped;                   // byte 64, 72: steps applied, steps skipped
    float norm, coef, lr_t; unsigned mask;           // byte 80: the record of the last step; mask bit k: family k took part
    int skip;                                        // byte 96: the step in flight is skipped (written by the fold, read by the update and the commit)
    int reserved[39];
};                                                   // 256 bytes
inline int optim_chunks(int P) { return (P + OPT_CHUNK - 1) / OPT_CHUNK; }
inline size_t optim_state_bytes(int n_lr) { return sizeof(OptimHeader) + (size_t)((n_lr + 63) / 64 * 64) * sizeof(float); }
inline size_t optim_ws_bytes(int chunks) { return ((size_t)chunks * sizeof(double) + 255) / 256 * 256; }
hipError_t launch_optim_step(const TrainBlock fam[3], void *opt, int cap, double *part, hipStream_t s);
hipError_t launch_optim_set_n(void *opt, int cap, int n, hipStream_t s);
hipError_t launch_optim_read(const void *opt, int cap, unsigned *out, hipStream_t s);
hipError_t launch_optim_write(void *opt, int cap, const unsigned *in, hipStream_t s);

// ---- mix.hip: noise mixing for training batches (uvad_mix_*, include/uvad.h): row energies, the plan of every row, the mix pass ----
// State: MixHeader (256 bytes) | clip_first [n_clips + 1] int64 | clip energies [n_clips] f64 | amp [Q] f64; every part 256-byte aligned.
// Workspace: MixWsHead (256 bytes: the call's draw and first row index) | row energies [B] f64 | the plan [B][4 + 4 max_seg] int32; every part
//            256-byte aligned.  The plan row is the record of include/uvad.h; the mix pass reads it from here, d_plan is a copy.
constexpr unsigned MIX_MAGIC = 0x55564D58u;          // "UVMX"
constexpr int MIX_MAX_SEG = 64;                      // UVAD_MIX_MAX_SEG
constexpr int MIX_PLAN_HEAD = 4, MIX_SEG_WORDS = 4;  // words of a plan row: {mixed, q, nseg, 0}, then {clip, dst offset, count, gain bits} per segment
constexpr int MIX_LANES = 1024, MIX_CHUNK = 4 * MIX_LANES;   // the energy order of include/uvad.h: lanes per row, samples per pass of the lanes
constexpr long long MIX_MAX_S = 2147483647LL;        // offsets and counts of the plan are int32
struct MixHeader {
    unsigned magic; int n_clips, Q, max_seg;
    unsigned long long thr;                          // byte 16: floor(mix_prob 2^32), 0 .. 2^32
    unsigned long long seed;                         // byte 24
    long long bank_total;                            // byte 32: samples of the bank = clip_first[n_clips]
    int reserved0[4];
    unsigned long long draws;                        // byte 56: steps drawn so far (the draw ordinal), where the training states keep theirs
    int reserved[48];
};                                                   // 256 bytes
struct MixWsHead { unsigned long long draw; long long row0; int reserved[60]; };   // 256 bytes: what the call's first kernel recorded
struct MixLayout { size_t off_first, off_energy, off_amp, total; };               // the state
struct MixWs { size_t off_energy, off_plan, total; int plan_words; };             // the workspace
struct MixArgs {
    const void *in; int fmt; int B; long long S; const long long *nsamp;
    float *out; int *plan;                           // plan: the caller's copy, may be null
    const float *bank; void *state; void *ws;
    int n_clips, Q, max_seg;
    bool take; unsigned long long draw; long long row0;   // take: the draw is the state's ordinal, which advances; else `draw`
};
MixLayout mix_layout(int n_clips, int Q);
MixWs mix_ws(int B, int max_seg);
hipError_t launch_mix_clip_energies(const float *bank, void *state, int n_clips, int Q, hipStream_t s);
hipError_t launch_mix(const MixArgs &a, hipStream_t s);

// ---- reverb.hip: reverberation of training batches (uvad_reverb_*, include/uvad.h): delays, the plan of every row, the convolution, gains ----
// State: ReverbHeader (256 bytes) | rir_first [n_rirs + 1] int64 | taps K_r [n_rirs] int32 | delay_r [n_rirs] int32; every part 256-byte aligned.
// Workspace: MixWsHead (256 bytes: the call's draw and first row index) | the plan [B][4] int32 (the record of include/uvad.h; d_plan is a copy).
constexpr unsigned REVERB_MAGIC = 0x55565242u;       // "UVRB"
constexpr int REVERB_PLAN_WORDS = 4;                 // UVAD_REVERB_PLAN_WORDS: {applied, r, d, gain bits}
constexpr int REVERB_MAX_TAPS = 1 << 20;             // UVAD_REVERB_MAX_TAPS: K_r at most (65.5 s at 16 kHz)
constexpr int REVERB_TILE = 4096;                    // UVAD_REVERB_TILE: output samples of one workgroup: 4 waves x 32 blocks x 32 phases
constexpr int REVERB_KC = 256;                       // UVAD_REVERB_K_CHUNK: input offsets s staged in LDS at a time
struct ReverbHeader {
    unsigned magic; int n_rirs, normalize, align;
    unsigned long long thr;                          // byte 16: floor(prob 2^32), 0 .. 2^32
    unsigned long long seed;                         // byte 24
    long long bank_total;                            // byte 32: taps in the bank = rir_first[n_rirs]
    int max_taps, reserved0[3];                      // byte 40
    unsigned long long draws;                        // byte 56: steps drawn so far (the draw ordinal), where the mix state keeps its own
    int reserved[48];
};                                                   // 256 bytes
struct ReverbLayout { size_t off_first, off_taps, off_delay, total; };
struct ReverbArgs {
    const void *in; int fmt; int B; long long S; const long long *nsamp;
    float *out; int *plan;                           // plan: the caller's copy, may be null
    const float *bank; void *state; void *ws;
    int n_rirs, normalize;
    bool take; unsigned long long draw; long long row0;   // take: the draw is the state's ordinal, which advances; else `draw`
};
ReverbLayout reverb_layout(int n_rirs);
size_t reverb_ws_bytes(int B);
hipError_t launch_reverb_delays(const float *bank, void *state, int n_rirs, hipStream_t s);
hipError_t launch_reverb(const ReverbArgs &a, hipStream_t s);

// ---- sampler.hip: training batches drawn on the device (uvad_sampler_*, include/uvad.h): the window table, the plan of every row, the gather
//      of the samples, the labels ----
// State: SamplerHeader (256 bytes) | SamplerSet [SAMPLER_MAX_SETS] | slot_rec [R] int32 (the recordings in table order) | win_first [R + 1] int32
//        (the first window of every slot) | rec_first [R + 1] int64 | sup_first [R + 1] int32 | sup [n_sup][2] int64; every part 256-byte aligned.
// Workspace: MixWsHead (256 bytes: the call's draw and first row index) | the plan [B][8] int32 (the record of include/uvad.h; d_plan is a copy).
constexpr unsigned SAMPLER_MAGIC = 0x55565350u;      // "UVSP"
constexpr int SAMPLER_PLAN_WORDS = 8;                // UVAD_SAMPLER_PLAN_WORDS: {dataset, epoch, position, window, recording, start, n, T_b}
constexpr int SAMPLER_MAX_SETS = 64;                 // UVAD_SAMPLER_MAX_SETS
constexpr long long SAMPLER_MAX_LEN = 2147483647LL;  // samples of a recording, of a window, windows in all: plan words are int32
struct SamplerHeader {
    unsigned magic; int R, n_sup, D;
    long long W;                                     // byte 16
    unsigned long long seed;                         // byte 24
    long long total;                                 // byte 32: samples of the corpus = rec_first[R]
    int fmt, geometry;                               // byte 40
    int n_windows, batch;                            // byte 48
    unsigned long long draws;                        // byte 56: steps drawn so far (the draw ordinal), where the mix state keeps its own
    int shuffle, drop_last, pad, half;               // byte 64
    int step, hop, frame_len, snip;                  // byte 80: hop / frame_len / snip_edges: the log-mel front end's framing (FBANK)
    int kw[3], stride0;                              // byte 96: the waveform front end's stages (SINCNET)
    long long min_keep;                              // byte 112
    int reserved[34];
};                                                   // 256 bytes
struct SamplerSet { long long cursor, L; unsigned long long cum; int first, N; };   // 32 bytes per dataset
struct SamplerLayout { size_t off_sets, off_slot, off_win, off_first, off_supf, off_sup, total; };
// frames of a row of n samples on the label grid of the header: uvad_num_frames / uvad_sincnet_num_frames (the floor chains of frames_of_kernel
// and sinc_row_geometry_kernel), for the host and the device
__host__ __device__ inline long long sampler_frames(const SamplerHeader &h, long long n) {
    if (h.geometry == UVAD_SAMPLER_FBANK) return h.snip ? (n < h.frame_len ? 0 : 1 + (n - h.frame_len) / h.hop) : (n + h.hop / 2) / h.hop;
    long long L = n;
    for (int i = 0; i < 3; ++i) {
        const long long lconv = L >= h.kw[i] ? (L - h.kw[i]) / (i == 0 ? h.stride0 : 1) + 1 : 0;
        L = lconv / 3;
    }
    return L;
}
struct SamplerTables {                               // what uvad_sampler_reset is given on the host
    const uvad_sampler_cfg *q; int fmt;
    const int64_t *rec_first; int R; const int64_t *sup; const int32_t *sup_first; int n_sup; const int32_t *rec_set; const double *weight; int D;
};
struct SamplerArgs {
    int B; float *out; long long ld_out; long long *nsamp; unsigned char *labels; long long ld_gt; int *frames; int *plan;   // plan: may be null
    const void *pcm; int fmt; void *state; void *ws;
    int R, n_sup, D; long long W, T;
    bool take; unsigned long long draw; long long row0; long long cursor[SAMPLER_MAX_SETS];   // take: ordinal and cursors are the state's, which advance
};
SamplerLayout sampler_layout(int R, int n_sup);
size_t sampler_ws_bytes(int B);
// Validates the tables and fills `image` (sampler_layout(R, n_sup).total bytes; the header's geometry fields are the caller's, already in
// image).  Returns nullptr, or the sentence uvad_last_error reports.  Host only, no HIP call.
const char *sampler_build(const SamplerTables &t, char *image);
hipError_t launch_sampler(const SamplerArgs &a, hipStream_t s);
hipError_t launch_sampler_read(const void *state, int D, long long *out, hipStream_t s);
hipError_t launch_sampler_write(void *state, int D, const long long *in, hipStream_t s);

}  // namespace uvad
