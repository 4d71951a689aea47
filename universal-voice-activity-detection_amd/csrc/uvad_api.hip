// uvad_api.hip -- C ABI of libuvad.so (see include/uvad.h): context, weight repacking into
// kernel layouts, workspace carving and the launch sequence of the hot path.  Host code only;
// every compute call enqueues kernels on the caller's stream and returns (no allocation, no
// synchronisation), so the whole sequence can be captured into a hipGraph by the caller.
#include "../../include/uvad.h"
#include "uvad_internal.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <memory>
#include <mutex>
#include <set>
#include <tuple>
#include <string>
#include <vector>

using namespace uvad;

struct HostTensor {
    std::vector<float> data;
    std::vector<int64_t> shape;
};

struct LayerDev {
    float *w_ih = nullptr;   // [dirs*4H (permuted: dir, unit, gate)][in]
    unsigned short *w_ih_split16 = nullptr; // the same, scaled by a power of two, as three exact f16 planes (gemm_f16p.hip)
    float w_ih_scale = 1.0f;
    float *bias = nullptr;   // [dirs*4H] b_ih + b_hh, same permutation
    float *w_hh = nullptr;   // [dirs][packed register image]
    float *w_ih_img = nullptr;   // causal H = 128 models: W_ih as a register image (lstm_stack.hip), else nullptr
    unsigned *w_hh16_regs = nullptr;        // 16-sequence kernel (H = 128): [dirs][P0 / P1 register image]
    unsigned short *w_hh16_p2 = nullptr;    // [dirs][P2 LDS image]
    unsigned short *w_hh16_p2q = nullptr;   // [dirs][the same as bf8 bytes] (nullptr: not every element is exactly representable)
    int w_hh16_p2q_scale = 127;
    float *w_hh16_scale = nullptr;          // [dirs] 2^-S
    bool w_hh16_ok = false;
    int in = 0;
};

// Everything uvad_finalize produces from the host tensors: the device buffers (owned here, freed with the last owner) and the values derived
// while packing.  Contexts that are finalized with IDENTICAL host tensors, model / SincNet configuration and device share one of these through a
// process-wide cache (packed_cache): the twelve slots of a ForwardPipeline, or the three of predict_vad, repack and upload the 6 MB of
// weights once instead of once per context (host-side packing is ~45 ms per context: it was 0.18 of the 0.26 s predict_vad spends on a one-hour
// recording).  Read-only on the device, so sharing needs no synchronisation; a weight hot-swap gives the swapping context a block of its own.
// uvad_finalize fills a fresh block and publishes it only when every step has succeeded (a block dropped half-built frees its uploads);
// from then on it is immutable -- contexts hold it as pointer-to-const -- and the launch code reads the weights through it.
struct PackedWeights {
    int device = 0;
    std::vector<void *> allocs;
    std::vector<LayerDev> layers;
    bool f16_ok = true;   // every GEMM operand the weights determine fits the f16 range (gemm mode 1 is usable)
    std::vector<float *> lin_w, lin_b;
    std::vector<float *> lin_w_img;   // 128 x 128 layers as register images (lstm_stack.hip), else nullptr
    std::vector<unsigned short *> lin_w_split16;
    std::vector<float> lin_w_scale;
    float *cls_w = nullptr, *cls_b = nullptr;
    // SincNet front end (sincnet.hip): packed only when its tensors were given (sinc_ready)
    bool sinc_ready = false, sinc_f16 = false;   // sinc_f16: the split-f16 form below is packed and usable
    float *sn_wav_g = nullptr, *sn_wav_b = nullptr;
    float *sn_wt[3] = {nullptr, nullptr, nullptr}, *sn_bias[3] = {nullptr, nullptr, nullptr}, *sn_g[3] = {nullptr, nullptr, nullptr}, *sn_b[3] = {nullptr, nullptr, nullptr};
    // ... and for the split-f16 form of the stages (sincnet_f16p.hip; GEMM modes 1 / 3): B-operand register images, 2^-S, padded biases,
    // and the largest |gamma| / |beta| of the norm in FRONT of each stage (the f16 range guard of sincnet_impl)
    unsigned short *sn_wfrag[3] = {nullptr, nullptr, nullptr};
    float sn_wscale[3] = {1.f, 1.f, 1.f}, *sn_bias16[3] = {nullptr, nullptr, nullptr};
    float sn_in_gmax[3] = {0.f, 0.f, 0.f}, sn_in_bmax[3] = {0.f, 0.f, 0.f};
    ~PackedWeights() {
        if (allocs.empty()) return;
        int cur = -1;
        (void)hipGetDevice(&cur);
        (void)hipSetDevice(device);
        for (void *p : allocs) (void)hipFree(p);
        if (cur >= 0) (void)hipSetDevice(cur);
    }
};

// Row tiles of the tile-major activation matrices (row = (tile * T + t) * 4 + j, 128-row tiles) by the time chunk that needs them first:
// direction 0 walks t upwards, direction 1 downwards.  list[off[d][i] .. + len[d][i]) = the row tiles of chunk i of direction d.
struct ChunkPlan {
    int chunks = 1;
    std::vector<int> bound;   // chunk i = frames [bound[i], bound[i + 1]) of the forward pass, [T - bound[i + 1], T - bound[i]) of the backward pass
    int *d_list = nullptr;
    std::vector<int> off[2], len[2];
    unsigned long long last_use = 0;   // stamp of the context's use counter: the least recently used plan is evicted (MAX_CHUNK_PLANS)
    bool pinned = false;               // handed to a stream capture: a graph may replay launches that read d_list, so it is never evicted
};
constexpr size_t MAX_CHUNK_PLANS = 16;      // distinct (batch, T) shapes whose row-tile lists stay on the device
constexpr int SIDE_RETRY_AFTER = 256;       // calls after which a caller stream that found no concurrent side stream is probed again

struct StreamCounters { int64_t n_samples = 0, n_frames = 0, n_steps = 0; };
struct StreamState { float *h = nullptr, *c = nullptr; size_t layer_stride = 0; };
struct WindowGroup { StreamCounters sc; int B = 0, W = 0, L = 0; };
struct WavWindowGroup { StreamCounters sc; int B = 0, W = 0, L = 0, is_i16 = 0; };
// a slot pool (uvad_window_slots_*, uvad_window_wav_slots_*): only what reset fixes; every per-slot counter lives on the device
struct SlotPool { int B = 0, chunk = 0, W = 0, L = 0, is_i16 = 0; };
// an endpointer state (uvad_endpoint_*): what reset fixed; the device header holds the same and every per-slot quantity
struct EndpointPool { int B = 0, kernel = 0, pad = 0; float threshold = 0.5f; };
// a hysteresis endpointer state (uvad_endpoint_hyst_*): B and the lag of the configuration at its reset
struct EndpointHystPool { int B = 0, lag = 0; };
// a speech gate state (uvad_gate_*): what reset fixed (the device header holds the same)
struct GatePool { int B = 0, unit_bytes = 0, history = 0; };
// a group gate state (uvad_gate_group_*): what reset fixed, G and N of the fusion configuration it was reset under among it
struct GateGroupPool { int G = 0, N = 0, unit_bytes = 0, history = 0, best_history = 0; };
// a scoring state (uvad_score_*): the configuration's n_points and bins at its reset (the device header holds the same)
struct ScoreState { int n_points = 0, bins = 0; };
// a noise-mix state (uvad_mix_*): the caller's bank and what reset fixed (the device header holds the same)
struct MixState { const float *bank = nullptr; int n_clips = 0, Q = 0, max_seg = 0; };
// a reverberation state (uvad_reverb_*): the same for the bank of impulse responses
struct ReverbState { const float *bank = nullptr; int n_rirs = 0, normalize = 0; };
// a sampler state (uvad_sampler_*): the caller's corpus and what reset fixed (the device header holds the same)
struct SamplerState { const void *pcm = nullptr; int fmt = 0, R = 0, n_sup = 0, D = 0, geometry = 0, drop_last = 0, batch = 0; int64_t W = 0, T = 0; };

struct uvad_ctx {
    std::map<void *, StreamCounters> streams;   // host mirror of the lock-step stream groups, keyed by d_state
    std::map<void *, WindowGroup> windows;      // ... and of the windowed stream groups (uvad_window_*)
    std::map<void *, WavWindowGroup> wav_windows;   // ... and of the waveform model's windowed stream groups (uvad_window_wav_*)
    std::map<void *, SlotPool> slot_pools, wav_slot_pools;   // ... and of the slot pools of both window families (uvad_window_*slots_*)
    std::map<void *, SlotPool> stream_slot_pools;   // ... and of the causal stream's slot pools (uvad_stream_slots_*): B and chunk
    std::map<void *, EndpointPool> endpoints;   // ... and of the endpointer states (uvad_endpoint_*)
    std::map<void *, EndpointHystPool> endpoint_hysts;   // ... and of the hysteresis endpointer states (uvad_endpoint_hyst_*)
    std::map<void *, GatePool> gates;           // ... and of the speech gate states (uvad_gate_*)
    std::map<void *, GateGroupPool> gate_groups;   // ... and of the group gate states (uvad_gate_group_*)
    std::map<void *, ScoreState> scores;        // ... and of the scoring states (uvad_score_*)
    bool has_score = false;                     // uvad_score_configure: operating points, collar, bins, segment (0 replaced by the default)
    uvad_score_cfg sq{};
    std::map<void *, int> head_trains;          // ... and of the head fine-tuning states (uvad_head_train_*): the parameter count at reset
    bool has_ht = false;                        // uvad_head_train_configure: the optimiser (segment 0 replaced by the default) and the head's shape
    uvad_head_train_cfg hq{};
    HeadTrainShape hts{};
    std::map<void *, int> lstm_trains;          // ... and of the LSTM training states (uvad_lstm_train_*): the parameter count at reset
    bool has_lt = false;                        // uvad_lstm_train_configure: the optimiser, first_layer and the packed shape of the trainable layers
    uvad_lstm_train_cfg lq{};
    LstmTrainShape lts{};
    unsigned lt_thr = 0; float lt_scale = 1.0f; uint64_t lt_seed = 0;   // uvad_lstm_train_set_dropout: what the forward call launches with (thr == 0: off)
    bool lt_dropped = false;                    // the last forward call of this context ran with thr > 0
    std::map<void *, int> sinc_trains;          // ... and of the SincNet training states (uvad_sincnet_train_*): first_stage at reset, | TRAIN_TAG_FLAG with band edges
    bool has_snt = false;                       // uvad_sincnet_train_configure: the optimiser, first_stage and the packed shape of the front end
    uvad_sincnet_train_cfg snq{};
    SincTrainShape snts{};
    std::map<void *, MixState> mixes;           // ... and of the noise-mix states (uvad_mix_*)
    std::map<void *, ReverbState> reverbs;      // ... and of the reverberation states (uvad_reverb_*)
    std::map<void *, SamplerState> samplers;    // ... and of the sampler states (uvad_sampler_*)
    std::map<void *, int> optims;               // ... and of the optimizer states (uvad_optim_*): n_lr at reset
    int device = 0, n_cu = 256;
    bool has_fb = false, has_model = false, finalized = false, tables_set = false;
    uvad_fbank_cfg fb{};
    uvad_model_cfg mc{};
    std::string err;
    std::map<std::string, HostTensor> host_w;
    // device
    float *d_window = nullptr, *d_mel_w = nullptr, *d_mel_wt = nullptr, *d_tw512 = nullptr;
    int *d_mel_start = nullptr, *d_mel_len = nullptr;
    int mel_stride = 0, mel_nyquist = 1;
    int gemm_mode = 1;    // 0: exact f32 MFMA (gemm.hip); 1: split-f16 x3 (gemm_f16p.hip)
    int rec_tile_mode = 0, rec_tile_used = 0;   // sequences per recurrent workgroup: requested (0 = by batch size) / last launched
    // SincNet front end (sincnet.hip)
    bool has_sinc = false;
    uvad_sincnet_cfg sc{};
    bool sinc_f16_used = false;          // the form the most recent uvad_sincnet ran (1: split-f16)
    std::vector<void *> allocs;          // feature tables, twiddles: live as long as the context
    // the finalized weights, the only thing the context knows about them (possibly shared with other contexts: PackedWeights); set
    // whenever `finalized` is, and kept after uvad_set_weight until the next uvad_finalize
    std::shared_ptr<const PackedWeights> packed;
    // timing
    bool timing = false;
    hipEvent_t ev[5] = {nullptr, nullptr, nullptr, nullptr, nullptr};
    bool ev_valid = false;
    std::vector<hipEvent_t> layer_ev;
    // time-chunked layers (uvad_set_time_chunks): the projection of chunk i + 1 on a side stream beside the recurrence of chunk i
    int chunk_mode = 0;                    // 0 = automatic, 1 = off, n > 1 = n chunks wherever the chunked form can run
    int chunks_used = 0;                   // chunks of the most recent classify / forward (1 = not chunked)
    // steps the caller keeps in flight on other contexts (uvad_set_concurrent_steps): sizes the persistent projection grids
    int concurrent_steps = 1;
    int proj_grid_used = 0;                // workgroups of the most recent call's weight-stationary projections (0 = it launched none)
    hipStream_t side = nullptr;            // the library's own stream for the chunk projections
    hipStream_t side_for = nullptr;        // the caller stream `side` was PROVEN concurrent with (nullptr: not yet probed / not concurrent)
    bool side_probed_for_null = false;     // (a null caller stream is a valid key: remember that it was probed)
    std::map<hipStream_t, int> side_failed;   // caller streams no side stream was found concurrent with -> calls left until the next probe
                                              // (a probe that ran while other contexts kept the GPU busy can read "serialised" falsely)
    unsigned long long plan_clock = 0;
    hipEvent_t ev_fork = nullptr;
    std::vector<hipEvent_t> ev_chunk;
    std::map<std::tuple<int, int, int, int>, ChunkPlan> chunk_plans;   // (tiles, T, dirs, chunks) -> row-tile lists on the device
    // ingest stage (uvad_ingest*, ingest.hip): the source description, the ratio 16000 / sample_rate reduced, and the uploaded taps
    bool has_ingest = false, ig_taps = false;
    uvad_ingest_cfg ig{};
    int ig_up = 1, ig_down = 1, ig_width = 0;
    std::vector<float> ig_taps_host;   // what d_ig_taps holds (an unchanged table is not uploaded again)
    float *d_ig_taps = nullptr;   // [INGEST_MAX_PHASES * INGEST_MAX_TAPS], allocated by the first uvad_ingest_set_taps, lives with the context
    // sliding-window inference (uvad_sliding_*, sliding.hip): window and hop in frames, the weight table as uploaded (empty: all ones)
    bool has_sliding = false;
    int sl_W = 0, sl_Hf = 0;
    std::vector<float> sl_w_host;
    float *d_sl_w = nullptr; int sl_w_cap = 0;   // [sl_w_cap] floats, grown by uvad_sliding_configure, lives with the context
    // channel fusion (uvad_fuse_*, fuse.hip): the validated configuration as given, and its copy on the device: one buffer of
    // fz_cap 4-byte words {group_first [G + 1], members [N], weights [N]}, grown by uvad_fuse_configure, lives with the context
    bool has_fuse = false, fz_on_device = false;
    uvad_fuse_cfg fz{};
    int fz_G = 0, fz_N = 0, fz_max_member = -1;
    bool fz_weighted = false;
    std::vector<int32_t> fz_host;      // what d_fz holds
    int32_t *d_fz = nullptr; size_t fz_cap = 0;
};

namespace {

int fail(uvad_ctx *c, int code, const std::string &msg) {
    if (c) c->err = msg;
    return code;
}
int hip_fail(uvad_ctx *c, hipError_t e, const char *what) {
    (void)hipGetLastError();   // reported here: a failed launch or attribute call must not resurface in the next call's hipGetLastError
    return fail(c, UVAD_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
}
#define HIPCHK(c, call)                                        \
    do {                                                       \
        hipError_t e_ = (call);                                \
        if (e_ != hipSuccess) return hip_fail((c), e_, #call); \
    } while (0)

size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

// The two questions the launch code asks of the finalized weights besides their pointers.  (f16_planes: callers have checked `finalized`.)
// split-f16 GEMMs are on and every operand the weights determine fits the f16 range: activations, and features, travel as f16 planes
bool f16_planes(const uvad_ctx *c) { return c->gemm_mode >= 1 && c->packed->f16_ok; }
// finalized with the SincNet tensors (uvad_sincnet_configure and uvad_set_weight clear `finalized`)
bool sinc_weights_ready(const uvad_ctx *c) { return c->finalized && c->packed->sinc_ready; }

// `owner`: the list the allocation is freed with (the context's tables, or the PackedWeights block a uvad_finalize is filling)
template <typename T>
int dev_upload(uvad_ctx *c, std::vector<void *> &owner, const T *host, size_t n, T **out) {
    void *p = nullptr;
    HIPCHK(c, hipMalloc(&p, n * sizeof(T) ? n * sizeof(T) : sizeof(T)));
    owner.push_back(p);
    if (n) HIPCHK(c, hipMemcpy(p, host, n * sizeof(T), hipMemcpyHostToDevice));
    *out = reinterpret_cast<T *>(p);
    return UVAD_OK;
}

// Workspace carving for B sequences of T frames (all offsets in bytes, 256-B aligned).
struct WsLayout {
    int tiles = 0, D = 0, Wd = 0, Fp = 0, Zw = 0;
    size_t M = 0;
    size_t off_G = 0, off_Y[2] = {0, 0}, off_Z[2] = {0, 0}, off_feats = 0, off_fplanes = 0, off_flag = 0, off_ctr = 0, off_hc = 0, total = 0;
};
// Activation buffers hold EITHER f32 rows OR two f16 planes of the same row width (hi plane, then the lo plane): same bytes.
WsLayout carve(const uvad_ctx *c, int B, int64_t T) {
    WsLayout w;
    const uvad_model_cfg &m = c->mc;
    w.tiles = (B + SEQ_TILE - 1) / SEQ_TILE;
    w.D = m.bidirectional ? 2 : 1;
    w.Wd = m.hidden * w.D;
    w.M = (size_t)w.tiles * SEQ_TILE * (size_t)T;
    w.Fp = gemm_f16p_padded_k(m.in_dim);
    w.Zw = m.lin_layers > 0 ? gemm_f16p_padded_k(m.lin_hidden) : 0;
    size_t o = 0;
    w.off_G = o; o += align_up(plane_rows(w.M) * 4 * m.hidden * w.D * sizeof(float));   // tile-blocked: whole 128-row tiles
    const size_t Mp = plane_rows(w.M);   // K-blocked planes come in whole 128-row tiles
    for (int i = 0; i < 2; ++i) { w.off_Y[i] = o; o += align_up(Mp * w.Wd * sizeof(float)); }
    for (int i = 0; i < 2; ++i) { w.off_Z[i] = o; o += align_up(Mp * (size_t)w.Zw * sizeof(float)); }
    w.off_feats = o; o += align_up((size_t)B * T * (size_t)(c->has_fb && c->fb.n_mels > m.in_dim ? c->fb.n_mels : m.in_dim) * sizeof(float));
    w.off_fplanes = o; o += align_up(Mp * (size_t)w.Fp * sizeof(float));   // f16 planes of the features (split-f16 GEMM mode)
    w.off_flag = o; o += align_up(sizeof(int));   // device-side "features outside the f16 range" flag (uvad_classify)
    w.off_ctr = o; o += align_up(gemm_f16p_ws_counter_bytes());   // tile-queue counters of the weight-stationary projection kernel
    w.off_hc = o; o += 2 * align_up((size_t)w.D * w.tiles * SEQ_TILE * m.hidden * sizeof(float));   // (h, c) carried between the time chunks of a layer
    w.total = o;
    return w;
}

// SincNet stage geometry and workspace for B waveforms of S samples.
struct SincLayout {
    int Cin[3], Cout[3], Kw[3], stride[3], NW[3], pt[3], phases[3];
    int64_t Lin[3], Lconv[3], Lpool[3];
    int ntiles[3];
    bool f16 = false; int cst[3] = {0, 0, 0}, ntiles16[3] = {0, 0, 0};   // split-f16 form (sincnet_f16p.hip): floats per output row, tiles of 64 pooled outputs
    size_t off_s0 = 0, off_P[3] = {0, 0, 0}, off_part[3] = {0, 0, 0}, off_sc[3] = {0, 0, 0}, total = 0;
    size_t off_geo = 0;   // lens calls: the per-row geometry (SincGeoArgs), behind everything else so no other offset moves
    bool ok = false;
};
SincLayout sinc_carve(const uvad_ctx *c, int B, int64_t S) {
    SincLayout l;
    const uvad_sincnet_cfg &q = c->sc;
    const int cin[3] = {1, q.n_filters, q.c2}, cout[3] = {q.n_filters, q.c2, q.c3}, kw[3] = {q.kernel_size, q.k2, q.k3};
    int64_t L = S;
    l.ok = true;
    for (int i = 0; i < 3; ++i) {
        l.Cin[i] = cin[i]; l.Cout[i] = cout[i]; l.Kw[i] = kw[i]; l.stride[i] = i == 0 ? q.stride : 1;
        l.NW[i] = (cout[i] + 31) / 32 * 32;
        l.Lin[i] = L;
        l.Lconv[i] = L >= kw[i] ? (L - kw[i]) / l.stride[i] + 1 : 0;
        l.Lpool[i] = l.Lconv[i] / 3;
        {   // workgroup shape of the stage (sincnet.hip): pooled outputs per tile and statistics groups per tile
            SincConvArgs a{};
            a.Cin = cin[i]; a.Cout = cout[i]; a.Kw = kw[i]; a.stride = l.stride[i]; a.Ktot = cin[i] * kw[i]; a.Kp = (a.Ktot + 7) / 8 * 8;
            const SincConvPlan plan = sinc_conv_plan(a);
            l.pt[i] = plan.pt; l.phases[i] = plan.phases;
        }
        l.ntiles[i] = (int)((l.Lpool[i] + l.pt[i] - 1) / l.pt[i]);
        if (l.Lpool[i] <= 0) l.ok = false;
        L = l.Lpool[i];
    }
    l.f16 = sinc_f16p_supported(q.n_filters, q.kernel_size, q.stride, q.c2, q.k2, q.c3, q.k3);
    size_t o = 0;
    l.off_s0 = o; o += align_up((size_t)2 * B * sizeof(float));
    for (int i = 0; i < 3; ++i) {
        // the buffers are sized for whichever form a call runs (the GEMM mode can change between calls)
        size_t pooled = (size_t)B * l.Cout[i] * (size_t)(l.ok ? l.Lpool[i] : 0);
        size_t part = (size_t)B * (size_t)(l.ok ? l.ntiles[i] : 0) * l.phases[i] * l.NW[i] * 2;
        if (l.f16) {
            l.cst[i] = sinc_f16p_cst(i);
            l.ntiles16[i] = l.ok ? sinc_f16p_ntiles(l.Lpool[i]) : 0;
            pooled = std::max(pooled, (size_t)B * l.cst[i] * (size_t)(l.ok ? l.Lpool[i] : 0));
            part = std::max(part, sinc_f16p_partial_floats(i, B, l.ntiles16[i]));
        }
        l.off_P[i] = o; o += align_up(pooled * sizeof(float));
        l.off_part[i] = o; o += align_up(part * sizeof(float));
        l.off_sc[i] = o; o += align_up((size_t)2 * B * l.Cout[i] * sizeof(float));
    }
    l.off_geo = o; o += align_up((size_t)SINC_GEO_ARRAYS * (B + 1) * sizeof(int));
    l.total = o;
    return l;
}

std::string strip_prefix(const char *key) {
    std::string k(key);
    if (k.rfind("model.", 0) == 0) k = k.substr(6);
    // ModuleList-of-LSTMs variant (monolithic=False, PyanNet2.py:103-118): lstm.{k}.weight_ih_l0[_reverse]
    if (k.rfind("lstm.", 0) == 0 && k.size() > 5 && isdigit((unsigned char)k[5])) {
        size_t dot = k.find('.', 5);
        if (dot != std::string::npos) {
            const std::string layer = k.substr(5, dot - 5);
            std::string rest = k.substr(dot + 1);
            const size_t l0 = rest.find("_l0");
            if (l0 != std::string::npos) {
                rest.replace(l0, 3, "_l" + layer);
                k = "lstm." + rest;
            }
        }
    }
    return k;
}

bool expect_shape(const HostTensor &t, std::initializer_list<int64_t> want) {
    if (t.shape.size() != want.size()) return false;
    size_t i = 0;
    for (int64_t w : want)
        if (t.shape[i++] != w) return false;
    return true;
}

}  // namespace

extern "C" {

int uvad_abi_version(void) { return UVAD_ABI_VERSION; }

int uvad_create(int device, const uvad_fbank_cfg *fb, const uvad_model_cfg *model, uvad_ctx **out) {
    if (!out) return UVAD_E_ARG;
    *out = nullptr;
    uvad_ctx *c = new uvad_ctx();
    *out = c;  // returned even on failure so uvad_last_error() can be read; caller destroys it
    c->device = device;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(c, UVAD_E_HIP, std::string("no HIP device available (libuvad has no CPU fallback): ") +
                                       (e != hipSuccess ? hipGetErrorString(e) : "device count is 0"));
    if (device < 0 || device >= ndev) return fail(c, UVAD_E_ARG, "device index out of range");
    HIPCHK(c, hipSetDevice(device));
    hipDeviceProp_t prop;
    HIPCHK(c, hipGetDeviceProperties(&prop, device));
    c->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(c, UVAD_E_HIP, std::string("libuvad is built for gfx950 only; device is ") + prop.gcnArchName);
    if (fb) {
        c->fb = *fb;
        c->has_fb = true;
        if (fb->n_fft != 512) return fail(c, UVAD_E_UNSUPPORTED, "only n_fft = 512 is implemented");
        if (fb->frame_len < 2 || fb->frame_len > 512 || fb->frame_shift < 1 || fb->n_mels < 1 || fb->n_mels > 128)
            return fail(c, UVAD_E_ARG, "bad fbank configuration");
        // forward-FFT twiddles (cos, -sin)(2 pi j / 512), computed in double
        std::vector<float> tw(2 * 512);
        for (int j = 0; j < 512; ++j) {
            const double a = 2.0 * M_PI * j / 512.0;
            tw[2 * j] = (float)std::cos(a);
            tw[2 * j + 1] = (float)(-std::sin(a));
        }
        int r = dev_upload(c, c->allocs, tw.data(), tw.size(), &c->d_tw512);
        if (r) return r;
    }
    if (model) {
        c->mc = *model;
        c->has_model = true;
        // hidden sizes: 128 and 64 have the register-resident recurrent kernels; any other size whose gate matrix comes in whole
        // 128-column tiles runs the generic recurrence (lstm_rec_any_kernel: correct, slow)
        if (model->hidden < 4 || model->hidden > 1024 || (4 * model->hidden * (model->bidirectional ? 2 : 1)) % 128 != 0)
            return fail(c, UVAD_E_UNSUPPORTED, "lstm hidden_size x directions must be a multiple of 32, hidden_size <= 1024");
        if (model->in_dim < 4 || model->in_dim % 4 != 0)
            return fail(c, UVAD_E_UNSUPPORTED, "encoding_dim must be a positive multiple of 4");
        if (model->num_layers < 1 || model->lin_layers < 0 || (model->lin_layers > 0 && (model->lin_hidden < 4 || model->lin_hidden % 4)))
            return fail(c, UVAD_E_ARG, "bad model configuration");
        if (!std::isfinite(model->leaky_slope)) return fail(c, UVAD_E_ARG, "model leaky_slope must be finite");
    }
    for (auto &ev : c->ev) HIPCHK(c, hipEventCreate(&ev));
    return UVAD_OK;
}

int uvad_set_tables(uvad_ctx *c, const float *window, const float *mel) {
    if (!c || !window || !mel) return UVAD_E_ARG;
    if (!c->has_fb) return fail(c, UVAD_E_STATE, "context was created without a fbank configuration");
    HIPCHK(c, hipSetDevice(c->device));
    const int nb = c->fb.n_fft / 2 + 1, F = c->fb.n_mels;
    std::vector<int> st(F), ln(F);
    int maxlen = 1;
    for (int m = 0; m < F; ++m) {
        int lo = nb, hi = -1;
        for (int k = 0; k < nb; ++k)
            if (mel[(size_t)m * nb + k] != 0.0f) { if (k < lo) lo = k; hi = k; }
        st[m] = hi < 0 ? 0 : lo;
        ln[m] = hi < 0 ? 0 : hi - lo + 1;
        if (ln[m] > maxlen) maxlen = ln[m];
    }
    // LDS bank spreading of the mel stage.  In fbank_pair() lane m walks its band's power values at scratch index st[m] + i with the SAME
    // i in every lane, so two lanes of a 32-lane group whose band starts are equal mod 32 hit one bank on every read (the 64-filter
    // table of the bench: up to 4 lanes per bank in the upper half of the filters -- a third of the kernel's LDS cycles were bank
    // conflicts).  Every lane runs the same trip count (the longest band, rounded up to four bins), so a shorter band has slack: its start
    // may be moved down by up to trip - len bins (zero weights in front) without costing an iteration.  A bipartite matching per
    // 32-lane group (filters -> bank residues, augmenting paths, smallest shift first) picks shifts that make the starts distinct
    // mod 32 wherever the slack allows; filters it cannot place keep their start.  Same sums up to the order of their terms.
    {
        const int trip = 4 * ((maxlen + 3) / 4);
        for (int g0 = 0; g0 < F; g0 += 32) {   // lanes g0 % 64 .. + 31 of filter pass g0 / 64: one LDS lane group
            const int n = std::min(32, F - g0);
            std::vector<int> owner(32, -1), shift_of(n, 0);   // bank residue -> filter of the group; chosen shift per filter
            // residue reached by filter j with shift sh; candidates in order of increasing shift
            auto max_shift = [&](int j) { const int m = g0 + j; return ln[m] > 0 ? std::min(trip - ln[m], st[m]) : 0; };
            std::function<bool(int, std::vector<char> &)> place = [&](int j, std::vector<char> &seen) -> bool {
                const int m = g0 + j;
                for (int sh = 0; sh <= max_shift(j); ++sh) {
                    const int res = ((st[m] - sh) % 32 + 32) % 32;
                    if (seen[res]) continue;
                    seen[res] = 1;
                    if (owner[res] < 0 || place(owner[res], seen)) {
                        owner[res] = j;
                        shift_of[j] = sh;
                        return true;
                    }
                }
                return false;
            };
            std::vector<int> order(n);
            for (int j = 0; j < n; ++j) order[j] = j;
            std::sort(order.begin(), order.end(), [&](int a, int b) { return max_shift(a) < max_shift(b); });   // the constrained ones first
            for (int j : order) {
                std::vector<char> seen(32, 0);
                if (!place(j, seen)) shift_of[j] = 0;   // no free bank within its slack: stays where it is (conflicts with one other lane)
            }
            for (int j = 0; j < n; ++j) {
                const int m = g0 + j;
                st[m] -= shift_of[j];
                ln[m] += ln[m] > 0 ? shift_of[j] : 0;
            }
        }
        // (maxlen is unchanged: every shifted band still fits the trip count)
        for (int m = 0; m < F; ++m)
            if (ln[m] > trip) return fail(c, UVAD_E_STATE, "internal: mel band shift exceeded the trip count");
        maxlen = trip;
    }
    {   // the feature kernel keeps the whole weight image, a PCM tile and the transform scratch in LDS: refuse here, by name, what a launch could not take
        FbankArgs probe{};
        probe.frame_len = c->fb.frame_len; probe.frame_shift = c->fb.frame_shift; probe.n_mels = F;
        probe.tab.mel_stride = maxlen;
        if (fbank_lds_bytes(probe) > 160 * 1024)
            return fail(c, UVAD_E_UNSUPPORTED, "mel matrix: the longest band (" + std::to_string(maxlen) + " bins) makes the feature kernel's weight image (" +
                                               std::to_string(mel_image_floats(maxlen, F) * 4) + " bytes) exceed the 160 KiB of LDS with this frame geometry");
    }
    c->mel_stride = maxlen;
    c->mel_nyquist = 0;
    for (int m = 0; m < F; ++m)
        if (mel[(size_t)m * nb + nb - 1] != 0.0f) c->mel_nyquist = 1;
    std::vector<float> w((size_t)F * maxlen, 0.0f);
    for (int m = 0; m < F; ++m)
        for (int i = 0; i < ln[m]; ++i) w[(size_t)m * maxlen + i] = mel[(size_t)m * nb + st[m] + i];
    int r;
    if ((r = dev_upload(c, c->allocs, window, (size_t)c->fb.frame_len, &c->d_window))) return r;
    if ((r = dev_upload(c, c->allocs, st.data(), st.size(), &c->d_mel_start))) return r;
    if ((r = dev_upload(c, c->allocs, ln.data(), ln.size(), &c->d_mel_len))) return r;
    if ((r = dev_upload(c, c->allocs, w.data(), w.size(), &c->d_mel_w))) return r;
    const int ld_t = mel_image_ld(F);
    std::vector<float> wt(mel_image_floats(maxlen, F), 0.0f);
    for (int m = 0; m < F; ++m)
        for (int i = 0; i < ln[m]; ++i) wt[(size_t)i * ld_t + m] = 0.25f * w[(size_t)m * maxlen + i];   // the spectrum split leaves 4 |X|^2 (fbank_pair.h): exact
    if ((r = dev_upload(c, c->allocs, wt.data(), wt.size(), &c->d_mel_wt))) return r;
    c->tables_set = true;
    return UVAD_OK;
}

int uvad_set_weight(uvad_ctx *c, const char *torch_key, const float *host, const int64_t *shape, int ndim) {
    if (!c || !torch_key || !host || !shape || ndim < 1 || ndim > 3) return UVAD_E_ARG;
    if (!c->has_model) return fail(c, UVAD_E_STATE, "context was created without a model configuration");
    HostTensor t;
    size_t n = 1;
    for (int i = 0; i < ndim; ++i) {
        if (shape[i] <= 0) return fail(c, UVAD_E_ARG, "non-positive dimension");
        t.shape.push_back(shape[i]);
        n *= (size_t)shape[i];
    }
    t.data.assign(host, host + n);
    c->host_w[strip_prefix(torch_key)] = std::move(t);
    c->finalized = false;
    return UVAD_OK;
}

extern "C++" {
namespace {
void free_weights(uvad_ctx *c) {
    for (auto &ev : c->layer_ev)
        if (ev) (void)hipEventDestroy(ev);
    c->layer_ev.clear();
    c->packed.reset();   // the shared block goes with its last owner
    c->finalized = false;
}
}  // namespace
}  // extern "C++"

extern "C++" {
namespace {
// 128-bit digest of everything the packed weights depend on: device, model / SincNet configuration, every host tensor (name, shape, bytes)
struct WeightKey {
    unsigned long long h[2];
    bool operator<(const WeightKey &o) const { return h[0] != o.h[0] ? h[0] < o.h[0] : h[1] < o.h[1]; }
};
inline void mix(WeightKey &k, const void *p, size_t n) {
    const unsigned char *b = reinterpret_cast<const unsigned char *>(p);
    size_t i = 0;
    for (; i + 8 <= n; i += 8) {
        unsigned long long w;
        memcpy(&w, b + i, 8);
        k.h[0] = (k.h[0] ^ w) * 0x9E3779B97F4A7C15ull; k.h[0] ^= k.h[0] >> 29;
        k.h[1] = (k.h[1] + w) * 0xC2B2AE3D27D4EB4Full; k.h[1] ^= k.h[1] >> 31;
    }
    for (; i < n; ++i) {
        k.h[0] = (k.h[0] ^ b[i]) * 0x100000001B3ull;
        k.h[1] = (k.h[1] + b[i]) * 0x9E3779B97F4A7C15ull; k.h[1] ^= k.h[1] >> 27;
    }
}
WeightKey weight_key(const uvad_ctx *c) {
    WeightKey k{{0xcbf29ce484222325ull, 0x84222325cbf29ce4ull}};
    mix(k, &c->device, sizeof c->device);
    mix(k, &c->mc, sizeof c->mc);
    const int hs = c->has_sinc ? 1 : 0;
    mix(k, &hs, sizeof hs);
    if (c->has_sinc) mix(k, &c->sc, sizeof c->sc);
    for (const auto &kv : c->host_w) {   // std::map: key order
        mix(k, kv.first.data(), kv.first.size());
        const size_t nd = kv.second.shape.size();
        mix(k, &nd, sizeof nd);
        mix(k, kv.second.shape.data(), nd * sizeof(int64_t));
        mix(k, kv.second.data.data(), kv.second.data.size() * sizeof(float));
    }
    return k;
}
std::mutex packed_mu;
std::map<WeightKey, std::weak_ptr<const PackedWeights>> packed_cache;
}  // namespace
}  // extern "C++"

int uvad_finalize(uvad_ctx *c) {
    if (!c) return UVAD_E_ARG;
    if (!c->has_model) return fail(c, UVAD_E_STATE, "no model configuration");
    HIPCHK(c, hipSetDevice(c->device));
    // Idempotent: a second call (e.g. after swapping weights with uvad_set_weight) replaces the previous upload.
    // Kernels of earlier calls may still be reading the old buffers.
    // The previous block goes before packing starts, so the peak is one block.
    if (c->packed) HIPCHK(c, hipDeviceSynchronize());
    free_weights(c);
    const uvad_model_cfg &m = c->mc;
    const int H = m.hidden, D = m.bidirectional ? 2 : 1;
    // another context of this process already holds these very weights in kernel layouts on this device: share them
    const WeightKey wkey = weight_key(c);
    {
        std::lock_guard<std::mutex> lk(packed_mu);
        auto it = packed_cache.find(wkey);
        if (it != packed_cache.end()) {
            if (std::shared_ptr<const PackedWeights> hit = it->second.lock()) {
                c->layer_ev.assign((size_t)2 * m.num_layers + 2, nullptr);
                for (auto &ev : c->layer_ev) HIPCHK(c, hipEventCreate(&ev));
                c->packed = hit;
                c->finalized = true;
                return UVAD_OK;
            }
            packed_cache.erase(it);
        }
    }
    auto get = [&](const std::string &k) -> const HostTensor * {
        auto it = c->host_w.find(k);
        return it == c->host_w.end() ? nullptr : &it->second;
    };
    // A block of this call's own: every early return below drops it, and its destructor frees what was uploaded so far.
    const std::shared_ptr<PackedWeights> pw = std::make_shared<PackedWeights>();
    PackedWeights &W = *pw;
    W.device = c->device;
    auto upload = [&](const auto *host, size_t n, auto **out) { return dev_upload(c, W.allocs, host, n, out); };
    W.layers.assign(m.num_layers, LayerDev());
    for (int k = 0; k < m.num_layers; ++k) {
        const int in = k == 0 ? m.in_dim : H * D;
        const int inp = gemm_padded_k(in);   // rows zero-padded to the GEMM's K-step
        std::vector<float> wp((size_t)D * 4 * H * inp, 0.0f), bp((size_t)D * 4 * H), hh((size_t)D * whh_packed_elems(H));
        std::vector<unsigned> hh16r(H == 128 ? (size_t)D * whh16h_regs_elems() : 0, 0u);
        std::vector<unsigned short> hh16p(H == 128 ? (size_t)D * whh16h_p2_elems() : 0, 0);
        std::vector<unsigned short> hh16q(H == 128 ? (size_t)D * whh16h_p2q_elems() : 0, 0);
        bool hh16q_ok = H == 128;
        int hh16q_scale = 127;
        std::vector<float> hh16s(D, 1.0f);
        bool hh16ok = H == 128;
        std::vector<float> ih_img;
        for (int d = 0; d < D; ++d) {
            const std::string suf = "_l" + std::to_string(k) + (d ? "_reverse" : "");
            const HostTensor *wih = get("lstm.weight_ih" + suf), *whh = get("lstm.weight_hh" + suf);
            const HostTensor *bih = get("lstm.bias_ih" + suf), *bhh = get("lstm.bias_hh" + suf);
            if (!wih || !whh || !bih || !bhh) return fail(c, UVAD_E_STATE, "missing LSTM tensor for suffix " + suf);
            if (!expect_shape(*wih, {4 * H, in}) || !expect_shape(*whh, {4 * H, H}) ||
                !expect_shape(*bih, {4 * H}) || !expect_shape(*bhh, {4 * H}))
                return fail(c, UVAD_E_ARG, "LSTM tensor shape mismatch for suffix " + suf);
            // torch rows are gate-major (i,f,g,o blocks of H); kernels want (unit, gate) interleaved
            for (int u = 0; u < H; ++u)
                for (int g = 0; g < 4; ++g) {
                    const size_t dst = (size_t)d * 4 * H + (size_t)u * 4 + g, src = (size_t)g * H + u;
                    std::memcpy(&wp[dst * inp], &wih->data[src * in], sizeof(float) * in);
                    bp[dst] = bih->data[src] + bhh->data[src];
                }
            pack_whh(whh->data.data(), H, &hh[(size_t)d * whh_packed_elems(H)]);
            if (D == 1 && H == 128 && in % 4 == 0) {   // the streaming step's one-launch stack (lstm_stack.hip)
                ih_img.resize(lstm_image_elems(in));
                pack_lstm_image(wih->data.data(), in, ih_img.data());
            }
            if (H == 128 && !pack_whh16h(whh->data.data(), &hh16r[(size_t)d * whh16h_regs_elems()], &hh16p[(size_t)d * whh16h_p2_elems()], &hh16s[d]))
                hh16ok = false;
            if (H == 128 && !pack_whh16h_p2q(whh->data.data(), &hh16q[(size_t)d * whh16h_p2q_elems()], &hh16q_scale)) hh16q_ok = false;
        }
        LayerDev &L = W.layers[k];
        L.in = in;
        int r;
        if ((r = upload(wp.data(), wp.size(), &L.w_ih))) return r;
        {
            std::vector<unsigned short> sp(3 * weight_plane_elems(D * 4 * H, inp));
            if (!split_weights_f16x3(wp.data(), D * 4 * H, inp, sp.data(), &L.w_ih_scale)) W.f16_ok = false;
            if ((r = upload(sp.data(), sp.size(), &L.w_ih_split16))) return r;
        }
        if ((r = upload(bp.data(), bp.size(), &L.bias))) return r;
        if ((r = upload(hh.data(), hh.size(), &L.w_hh))) return r;
        if (!ih_img.empty() && (r = upload(ih_img.data(), ih_img.size(), &L.w_ih_img))) return r;
        if (H == 128) {
            if ((r = upload(hh16r.data(), hh16r.size(), &L.w_hh16_regs))) return r;
            if ((r = upload(hh16p.data(), hh16p.size(), &L.w_hh16_p2))) return r;
            L.w_hh16_p2q = nullptr;
            L.w_hh16_p2q_scale = hh16q_scale;
            if (hh16q_ok && (r = upload(hh16q.data(), hh16q.size(), &L.w_hh16_p2q))) return r;
            if ((r = upload(hh16s.data(), hh16s.size(), &L.w_hh16_scale))) return r;
        }
        L.w_hh16_ok = hh16ok;
    }
    W.lin_w.assign(m.lin_layers, nullptr);
    W.lin_b.assign(m.lin_layers, nullptr);
    W.lin_w_split16.assign(m.lin_layers, nullptr);
    W.lin_w_img.assign(m.lin_layers, nullptr);
    W.lin_w_scale.assign(m.lin_layers, 1.0f);
    int prev = H * D;
    // Static bound on what the feed-forward GEMMs can be fed: |h| < 1 out of the LSTM, so |z_j| <= sum_k |w_jk| * amax + |b_j|
    // (leaky_relu does not grow magnitudes for slopes in [-1, 1]).  If that can leave the f16 range the split-f16 GEMM is not used.
    double amax = 1.0;
    for (int j = 0; j < m.lin_layers; ++j) {
        const HostTensor *w = get("linear." + std::to_string(j) + ".weight"), *b = get("linear." + std::to_string(j) + ".bias");
        if (!w || !b) return fail(c, UVAD_E_STATE, "missing linear." + std::to_string(j));
        if (!expect_shape(*w, {m.lin_hidden, prev}) || !expect_shape(*b, {m.lin_hidden}))
            return fail(c, UVAD_E_ARG, "linear." + std::to_string(j) + " shape mismatch");
        int r;
        const int prevp = gemm_padded_k(prev);
        std::vector<float> wpad((size_t)m.lin_hidden * prevp, 0.0f);
        double zmax = 0.0;
        for (int o = 0; o < m.lin_hidden; ++o) {
            std::memcpy(&wpad[(size_t)o * prevp], &w->data[(size_t)o * prev], sizeof(float) * prev);
            double l1 = 0.0;
            for (int k = 0; k < prev; ++k) l1 += std::fabs((double)w->data[(size_t)o * prev + k]);
            const double z = l1 * amax + std::fabs((double)b->data[o]);
            if (!(z <= zmax)) zmax = z;   // NaN-propagating max
        }
        if ((r = upload(wpad.data(), wpad.size(), &W.lin_w[j]))) return r;
        {
            std::vector<unsigned short> sp(3 * weight_plane_elems(m.lin_hidden, prevp));
            if (!split_weights_f16x3(wpad.data(), m.lin_hidden, prevp, sp.data(), &W.lin_w_scale[j])) W.f16_ok = false;
            if ((r = upload(sp.data(), sp.size(), &W.lin_w_split16[j]))) return r;
        }
        if ((r = upload(b->data.data(), b->data.size(), &W.lin_b[j]))) return r;
        if (m.lin_hidden == 128 && prev == 128) {   // the streaming step's in-launch head (lstm_stack.hip)
            std::vector<float> img(fc_image_elems());
            pack_fc_image(w->data.data(), img.data());
            if ((r = upload(img.data(), img.size(), &W.lin_w_img[j]))) return r;
        }
        amax = zmax * std::fmax(1.0, std::fabs((double)m.leaky_slope));
        if (j + 1 < m.lin_layers && !(amax < 65504.0)) W.f16_ok = false;   // the next feed-forward GEMM would see it
        prev = m.lin_hidden;
    }
    const HostTensor *cw = get("classifier.weight"), *cb = get("classifier.bias");
    if (!cw || !cb) return fail(c, UVAD_E_STATE, "missing classifier tensors");
    if (!expect_shape(*cw, {1, prev}) || !expect_shape(*cb, {1})) return fail(c, UVAD_E_ARG, "classifier shape mismatch");
    int r;
    if ((r = upload(cw->data.data(), cw->data.size(), &W.cls_w))) return r;
    if ((r = upload(cb->data.data(), cb->data.size(), &W.cls_b))) return r;
    if (c->has_sinc && get("sincnet.conv1d.0.filters")) {   // the stage is optional: packed only when its tensors were given
        const uvad_sincnet_cfg &q = c->sc;
        const HostTensor *wg = get("sincnet.wav_norm1d.weight"), *wb = get("sincnet.wav_norm1d.bias");
        if (!wg || !wb || !expect_shape(*wg, {1}) || !expect_shape(*wb, {1})) return fail(c, UVAD_E_STATE, "missing / misshaped sincnet.wav_norm1d tensors");
        if ((r = upload(wg->data.data(), 1, &W.sn_wav_g))) return r;
        if ((r = upload(wb->data.data(), 1, &W.sn_wav_b))) return r;
        const int cin[3] = {1, q.n_filters, q.c2}, cout[3] = {q.n_filters, q.c2, q.c3}, kw[3] = {q.kernel_size, q.k2, q.k3};
        for (int i = 0; i < 3; ++i) {
            const std::string id = std::to_string(i);
            const HostTensor *w = get(i == 0 ? std::string("sincnet.conv1d.0.filters") : "sincnet.conv1d." + id + ".weight");
            const HostTensor *b = i == 0 ? nullptr : get("sincnet.conv1d." + id + ".bias");
            const HostTensor *g = get("sincnet.norm1d." + id + ".weight"), *be = get("sincnet.norm1d." + id + ".bias");
            if (!w || (i > 0 && !b) || !g || !be) return fail(c, UVAD_E_STATE, "missing sincnet tensors of stage " + id);
            const bool wshape = i == 0 ? (expect_shape(*w, {cout[0], kw[0]}) || expect_shape(*w, {cout[0], 1, kw[0]})) : expect_shape(*w, {cout[i], cin[i], kw[i]});
            if (!wshape || (b && !expect_shape(*b, {cout[i]})) || !expect_shape(*g, {cout[i]}) || !expect_shape(*be, {cout[i]}))
                return fail(c, UVAD_E_ARG, "sincnet stage " + id + " tensor shape mismatch");
            // W[n][ci][tap] -> W^T [k = tap*Cin + ci][NW], zero padded in n and k (sincnet.hip B-operand layout)
            const int Ktot = cin[i] * kw[i], Kp = (Ktot + 7) / 8 * 8, NW = (cout[i] + 31) / 32 * 32;
            std::vector<float> wt((size_t)Kp * NW, 0.0f), bias((size_t)NW, 0.0f);
            for (int n = 0; n < cout[i]; ++n) {
                for (int ci = 0; ci < cin[i]; ++ci)
                    for (int t = 0; t < kw[i]; ++t)   // kernel K order: tap-major, channel-minor
                        wt[(size_t)(t * cin[i] + ci) * NW + n] = w->data[((size_t)n * cin[i] + ci) * kw[i] + t];
                if (b) bias[n] = b->data[n];
            }
            if ((r = upload(wt.data(), wt.size(), &W.sn_wt[i]))) return r;
            if ((r = upload(bias.data(), bias.size(), &W.sn_bias[i]))) return r;
            if ((r = upload(g->data.data(), g->data.size(), &W.sn_g[i]))) return r;
            if ((r = upload(be->data.data(), be->data.size(), &W.sn_b[i]))) return r;
            // the norm in FRONT of stage i + 1 (stage 0's is the waveform norm): bounds for the f16 range guard
            if (i < 2) {
                float gm = 0.f, bm = 0.f;
                for (float v : g->data) gm = std::max(gm, std::fabs(v));
                for (float v : be->data) bm = std::max(bm, std::fabs(v));
                W.sn_in_gmax[i + 1] = gm; W.sn_in_bmax[i + 1] = bm;
            }
        }
        W.sn_in_gmax[0] = std::fabs(wg->data[0]); W.sn_in_bmax[0] = std::fabs(wb->data[0]);
        // the split-f16 form of the stages (sincnet_f16p.hip): W[n][k] in the stage's K order -> three exact f16 planes as register images
        W.sinc_f16 = sinc_f16p_supported(q.n_filters, q.kernel_size, q.stride, q.c2, q.k2, q.c3, q.k3);
        for (int i = 0; i < 3 && W.sinc_f16; ++i) {
            const std::string id = std::to_string(i);
            const HostTensor *w = get(i == 0 ? std::string("sincnet.conv1d.0.filters") : "sincnet.conv1d." + id + ".weight");
            const HostTensor *b = i == 0 ? nullptr : get("sincnet.conv1d." + id + ".bias");
            const int ldk = 32 * sinc_f16p_ksteps(i), cst = sinc_f16p_cst(i);
            const int cpad = i == 1 ? cin[1] : 64;            // k = tap * cpad + channel (stage 1: 80 channels per tap, stage 2: 64 with 60 real)
            std::vector<float> wn((size_t)cout[i] * ldk, 0.0f), bias((size_t)cst, 0.0f);
            for (int n = 0; n < cout[i]; ++n) {
                if (i == 0)
                    for (int t = 0; t < kw[0]; ++t) wn[(size_t)n * ldk + t] = w->data[(size_t)n * kw[0] + t];
                else
                    for (int ci = 0; ci < cin[i]; ++ci)
                        for (int t = 0; t < kw[i]; ++t) wn[(size_t)n * ldk + t * cpad + ci] = w->data[((size_t)n * cin[i] + ci) * kw[i] + t];
                if (b) bias[n] = b->data[n];
            }
            std::vector<unsigned short> frag(sinc_f16p_wfrag_elems(i));
            if (!sinc_f16p_pack_weights(i, wn.data(), cout[i], ldk, frag.data(), &W.sn_wscale[i])) { W.sinc_f16 = false; break; }   // a non-finite weight: exact kernels
            if ((r = upload(frag.data(), frag.size(), &W.sn_wfrag[i]))) return r;
            if ((r = upload(bias.data(), bias.size(), &W.sn_bias16[i]))) return r;
        }
        W.sinc_ready = true;
    }
    c->layer_ev.assign((size_t)2 * m.num_layers + 2, nullptr);
    for (auto &ev : c->layer_ev) HIPCHK(c, hipEventCreate(&ev));
    {   // complete: the context's weights from here on, and a block other contexts with the same weights can share
        c->packed = pw;
        std::lock_guard<std::mutex> lk(packed_mu);
        for (auto it = packed_cache.begin(); it != packed_cache.end();)   // (entries whose block is gone: a process that cycles through weight sets)
            it = it->second.expired() ? packed_cache.erase(it) : std::next(it);
        packed_cache[wkey] = pw;
    }
    c->finalized = true;
    return UVAD_OK;
}

int uvad_sincnet_configure(uvad_ctx *c, const uvad_sincnet_cfg *q) {
    if (!c || !q) return UVAD_E_ARG;
    if (!c->has_model) return fail(c, UVAD_E_STATE, "uvad_sincnet_configure: context was created without a model configuration");
    if (q->stride < 1 || q->kernel_size < 3 || q->k2 < 3 || q->k3 < 3 || q->n_filters < 1 || q->c2 < 1 || q->c3 < 1)
        return fail(c, UVAD_E_ARG, "bad SincNet configuration");
    if (!std::isfinite(q->leaky_slope)) return fail(c, UVAD_E_ARG, "SincNet leaky_slope must be finite");
    // eps >= 0 keeps an instance-normalised value within sqrt(L - 1) in magnitude: the bound the split-f16 range guard rests on
    if (!std::isfinite(q->eps) || q->eps < 0.0f) return fail(c, UVAD_E_ARG, "SincNet eps must be finite and >= 0");
    const int cout[3] = {q->n_filters, q->c2, q->c3};
    if ((q->n_filters & 1) || (q->c2 & 1)) return fail(c, UVAD_E_UNSUPPORTED, "SincNet input channel counts of the conv stages must be even");
    for (int i = 0; i < 3; ++i)
        if (cout[i] <= 32 || cout[i] > 96) return fail(c, UVAD_E_UNSUPPORTED, "SincNet channel counts must be in 33..96 (two or three 32-wide MFMA column tiles)");
    if (q->c3 != c->mc.in_dim) return fail(c, UVAD_E_ARG, "SincNet output channels != classifier encoding_dim");
    // LDS budget of the widest stage (filter matrix + staging window), 160 KiB per CU
    const int cin[3] = {1, q->n_filters, q->c2}, kw[3] = {q->kernel_size, q->k2, q->k3};
    for (int i = 0; i < 3; ++i) {
        SincConvArgs a{};
        a.Cin = cin[i]; a.Kw = kw[i]; a.stride = i == 0 ? q->stride : 1; a.Ktot = cin[i] * kw[i]; a.Kp = (a.Ktot + 7) / 8 * 8;
        a.Cout = cout[i];
        if (sinc_conv_lds_bytes(a, (cout[i] + 31) / 32, 3) > (size_t)160 * 1024)
            return fail(c, UVAD_E_UNSUPPORTED, "SincNet stage does not fit the 160 KiB LDS (filter matrix is LDS-resident)");
        if (sinc_conv_ept(a, 3) > (i == 0 ? 8 : 48))
            return fail(c, UVAD_E_UNSUPPORTED, "SincNet stage input window too large for the register-prefetched staging");
    }
    c->sc = *q;
    c->has_sinc = true;
    c->finalized = false;   // (with it, "the SincNet weights are ready": sinc_weights_ready)
    return UVAD_OK;
}

int64_t uvad_sincnet_num_frames(const uvad_ctx *c, int64_t S) {
    if (!c || !c->has_sinc || S < 0) return -1;
    const SincLayout l = sinc_carve(c, 1, S);
    return l.ok ? l.Lpool[2] : 0;
}

size_t uvad_sincnet_workspace_bytes(const uvad_ctx *c, int B, int64_t S) {
    if (!c || !c->has_sinc || B <= 0 || S <= 0) return 0;
    return sinc_carve(c, B, S).total;
}

// d_wav: f32, or int16 read as q / 32768 (is_i16): the waveform kernels (statistics, the first conv stage of either form) read it as
// given -- no conversion pass, no f32 copy -- and everything after the first stage is the same for both sample types.
// nsamp (uvad_sincnet_lens): device int64 [B] sample counts, clamped to [0, S] on the device.  A geometry kernel turns them into each
// row's stage lengths, frame count T_b and the exclusive prefixes of the rows' tile counts; every later kernel runs its lens form, so row b
// gets the bits of a dense call on wav[b, :S_b] at t < T_b and +0 after.  *row_T: where T_b (int32 [B]) lands, for classify_impl.
static int sincnet_impl(uvad_ctx *c, const void *d_wav, int is_i16, int B, int64_t S, float *d_feats, void *ws, size_t ws_bytes, hipStream_t s,
                        const int64_t *nsamp = nullptr, const int **row_T = nullptr) {
    if (!c->has_sinc) return fail(c, UVAD_E_STATE, "uvad_sincnet: uvad_sincnet_configure has not been called");
    if (!sinc_weights_ready(c)) return fail(c, UVAD_E_STATE, "uvad_sincnet: SincNet tensors not set / uvad_finalize not called");
    const PackedWeights &W = *c->packed;
    const SincLayout l = sinc_carve(c, B, S);
    if (!l.ok) return fail(c, UVAD_E_ARG, "uvad_sincnet: waveform too short for one output frame");
    if (l.Lconv[0] > 0x7fffffff / 4) return fail(c, UVAD_E_UNSUPPORTED, "uvad_sincnet: waveform too long");
    if (ws_bytes < l.total) return fail(c, UVAD_E_WORKSPACE, "workspace too small: need " + std::to_string(l.total) + " bytes");
    char *base = reinterpret_cast<char *>(ws);
    const uvad_sincnet_cfg &q = c->sc;
    float *s0 = reinterpret_cast<float *>(base + l.off_s0);
    const int16_t *wav16 = is_i16 ? static_cast<const int16_t *>(d_wav) : nullptr;
    // lens: the rows of each stage in both forms' tiles (geo arrays of SincGeoArgs)
    int *geo = reinterpret_cast<int *>(base + l.off_geo);
    auto garr = [&](int k) { return geo + (size_t)k * (B + 1); };
    SincRows rows16[3], rows32[3];
    const int *T_rows = nullptr;
    if (nsamp) {
        SincGeoArgs g{};
        g.nsamp = nsamp; g.B = B; g.S = S; g.stride0 = q.stride; g.geo = geo;
        for (int i = 0; i < 3; ++i) {
            g.kw[i] = l.Kw[i]; g.pt[i] = l.pt[i];
            rows16[i] = SincRows{garr(1 + 6 * i), garr(2 + 6 * i), garr(4 + 6 * i)};
            rows32[i] = SincRows{garr(1 + 6 * i), garr(2 + 6 * i), garr(6 + 6 * i)};
        }
        HIPCHK(c, launch_sinc_row_geometry(g, s));
        T_rows = garr(0);
        if (row_T) *row_T = T_rows;
    }
    const int *row_n = nsamp ? rows16[0].lin : nullptr;
    if (wav16) HIPCHK(c, launch_wav_stats(wav16, B, S, S, W.sn_wav_g, W.sn_wav_b, q.eps, s0, s0 + B, s, row_n));
    else HIPCHK(c, launch_wav_stats(static_cast<const float *>(d_wav), B, S, S, W.sn_wav_g, W.sn_wav_b, q.eps, s0, s0 + B, s, row_n));
    const float *in = wav16 ? nullptr : static_cast<const float *>(d_wav), *in_scale = s0, *in_shift = s0 + B;
    // Split-f16 form (GEMM modes 1 / 3) when the geometry is the reference's and every stage input provably fits the f16 range: an
    // instance-normalised value is at most sqrt(L - 1) in magnitude, so |gamma| * sqrt(L) + |beta| bounds what the staging converts, and
    // the leaky_relu in front of stages 2 and 3 scales that by at most max(1, |slope|).  The staging of those stages applies leaky_relu
    // as max(e, e * slope), which is leaky_relu only for slope <= 1: a larger slope runs the exact-f32 stages.  A lens call checks the
    // padded S, which bounds every row: it can run the exact form where one of its rows alone would run the split form.
    bool f16 = l.f16 && W.sinc_f16 && (c->gemm_mode == 1 || c->gemm_mode == 3) && q.leaky_slope <= 1.0f;
    const double act = std::fmax(1.0, std::fabs((double)q.leaky_slope));
    for (int i = 0; i < 3 && f16; ++i)
        if (!((W.sn_in_gmax[i] * std::sqrt((double)l.Lin[i]) + W.sn_in_bmax[i]) * (i > 0 ? act : 1.0) < 60000.0)) f16 = false;
    c->sinc_f16_used = f16;
    if (f16) {
        for (int i = 0; i < 3; ++i) {
            float *P = reinterpret_cast<float *>(base + l.off_P[i]);
            float *part = reinterpret_cast<float *>(base + l.off_part[i]);
            float *sc = reinterpret_cast<float *>(base + l.off_sc[i]);
            SincF16Args a{};
            a.in = in; a.in_i16 = i == 0 ? wav16 : nullptr; a.in_bstride = S; a.Lin = (int)l.Lin[i];
            a.in_scale = in_scale; a.in_shift = in_shift; a.n_in = l.Cin[i]; a.slope = q.leaky_slope;
            a.Wfrag = W.sn_wfrag[i]; a.wscale = W.sn_wscale[i]; a.bias = W.sn_bias16[i];
            a.Lpool = (int)l.Lpool[i]; a.ntiles = l.ntiles16[i];
            a.out = P; a.partials = part; a.B = B; a.n_cu = c->n_cu;
            HIPCHK(c, launch_sinc_conv_f16p(i, a, s, nsamp ? &rows16[i] : nullptr));
            HIPCHK(c, launch_norm_finalize_f16p(i, part, B, l.ntiles16[i], l.Cout[i], (int)l.Lpool[i], W.sn_g[i], W.sn_b[i], q.eps, sc,
                                                sc + (size_t)B * l.Cout[i], s, nsamp ? &rows16[i] : nullptr));
            in = P; in_scale = sc; in_shift = sc + (size_t)B * l.Cout[i];
        }
        HIPCHK(c, launch_sinc_out_f16p(in, in_scale, in_shift, B, l.Cout[2], l.cst[2], (int)l.Lpool[2], q.leaky_slope, d_feats, l.Cout[2], s, T_rows));
        return UVAD_OK;
    }
    for (int i = 0; i < 3; ++i) {
        float *P = reinterpret_cast<float *>(base + l.off_P[i]);
        float *part = reinterpret_cast<float *>(base + l.off_part[i]);
        float *sc = reinterpret_cast<float *>(base + l.off_sc[i]);
        SincConvArgs a{};
        a.in = in; a.in_i16 = i == 0 ? wav16 : nullptr; a.in_bstride = (long long)l.Cin[i] * l.Lin[i]; a.Cin = l.Cin[i]; a.Lin = (int)l.Lin[i];
        a.in_scale = in_scale; a.in_shift = in_shift; a.in_lrelu = i > 0; a.slope = q.leaky_slope;
        a.Wt2 = W.sn_wt[i]; a.bias = W.sn_bias[i];
        a.Kw = l.Kw[i]; a.stride = l.stride[i]; a.Ktot = l.Cin[i] * l.Kw[i]; a.Kp = (a.Ktot + 7) / 8 * 8; a.Cout = l.Cout[i]; a.do_abs = i == 0;
        a.Lconv = (int)l.Lconv[i]; a.Lpool = (int)l.Lpool[i]; a.ntiles = l.ntiles[i];
        a.out = P; a.partials = part; a.B = B; a.n_cu = c->n_cu;
        HIPCHK(c, launch_sinc_conv(a, s, nsamp ? &rows32[i] : nullptr));
        HIPCHK(c, launch_norm_finalize(part, B, l.ntiles[i], l.pt[i], l.phases[i], l.NW[i], l.Cout[i], (int)l.Lpool[i], W.sn_g[i], W.sn_b[i], q.eps, sc,
                                       sc + (size_t)B * l.Cout[i], s, nsamp ? &rows32[i] : nullptr));
        in = P; in_scale = sc; in_shift = sc + (size_t)B * l.Cout[i];
    }
    HIPCHK(c, launch_sinc_out(in, in_scale, in_shift, B, l.Cout[2], (int)l.Lpool[2], q.leaky_slope, d_feats, l.Cout[2], s, T_rows));
    return UVAD_OK;
}

static int sincnet_entry(uvad_ctx *c, const void *d_wav, int is_i16, int B, int64_t S, float *d_feats, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_wav || !d_feats || B <= 0 || S <= 0 || !ws) return fail(c, UVAD_E_ARG, "uvad_sincnet: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    return sincnet_impl(c, d_wav, is_i16, B, S, d_feats, ws, ws_bytes, (hipStream_t)stream);
}

int uvad_sincnet(uvad_ctx *c, const float *d_wav, int B, int64_t S, float *d_feats, void *ws, size_t ws_bytes, void *stream) {
    return sincnet_entry(c, d_wav, 0, B, S, d_feats, ws, ws_bytes, stream);
}
int uvad_sincnet_i16(uvad_ctx *c, const int16_t *d_wav, int B, int64_t S, float *d_feats, void *ws, size_t ws_bytes, void *stream) {
    return sincnet_entry(c, d_wav, 1, B, S, d_feats, ws, ws_bytes, stream);
}

static int sincnet_lens_entry(uvad_ctx *c, const void *d_wav, int is_i16, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *ws,
                              size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_nsamp) return fail(c, UVAD_E_ARG, "uvad_sincnet_lens: d_nsamp is NULL");
    if (!d_wav || !d_feats || B <= 0 || S <= 0 || !ws) return fail(c, UVAD_E_ARG, "uvad_sincnet_lens: bad argument");
    HIPCHK(c, hipSetDevice(c->device));
    return sincnet_impl(c, d_wav, is_i16, B, S, d_feats, ws, ws_bytes, (hipStream_t)stream, d_nsamp);
}
int uvad_sincnet_lens(uvad_ctx *c, const float *d_wav, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *ws, size_t ws_bytes,
                      void *stream) {
    return sincnet_lens_entry(c, d_wav, 0, B, S, d_nsamp, d_feats, ws, ws_bytes, stream);
}
int uvad_sincnet_lens_i16(uvad_ctx *c, const int16_t *d_wav, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *ws, size_t ws_bytes,
                          void *stream) {
    return sincnet_lens_entry(c, d_wav, 1, B, S, d_nsamp, d_feats, ws, ws_bytes, stream);
}

int64_t uvad_num_frames(const uvad_ctx *c, int64_t S) {
    if (!c || !c->has_fb || S < 0) return -1;
    if (c->fb.snip_edges) return S < c->fb.frame_len ? 0 : 1 + (S - c->fb.frame_len) / c->fb.frame_shift;
    return (S + c->fb.frame_shift / 2) / c->fb.frame_shift;
}

size_t uvad_workspace_bytes(const uvad_ctx *c, int B, int64_t T) {
    if (!c || !c->has_model || B <= 0 || T <= 0) return 0;
    return carve(c, B, T).total;
}

// What every launch of the feature kernel takes from the context: the front-end configuration and the tables of uvad_set_tables.  The
// callers add what differs: input, geometry, snip_edges, outputs.
static FbankArgs fbank_cfg_args(const uvad_ctx *c) {
    FbankArgs a{};
    a.frame_len = c->fb.frame_len; a.frame_shift = c->fb.frame_shift; a.n_mels = c->fb.n_mels;
    a.preemph = c->fb.preemph; a.log_floor = c->fb.log_floor; a.remove_dc = c->fb.remove_dc;
    a.tab.window = c->d_window; a.tab.mel_start = c->d_mel_start; a.tab.mel_len = c->d_mel_len;
    a.tab.mel_w = c->d_mel_w; a.tab.mel_wt = c->d_mel_wt; a.tab.mel_stride = c->mel_stride; a.tab.tw512 = c->d_tw512; a.tab.nyquist = c->mel_nyquist;
    return a;
}

static int fbank_impl(uvad_ctx *c, const void *d_pcm, int is_i16, int B, int64_t S, float *d_feats, void *stream,
                      unsigned short *plane_hi = nullptr, unsigned short *plane_lo = nullptr, int plane_w = 0, const int64_t *nsamp = nullptr) {
    if (!c || !d_pcm || (!d_feats && !plane_hi) || B <= 0 || S <= 0) return fail(c, UVAD_E_ARG, "uvad_fbank: bad argument");
    if (!c->has_fb || !c->tables_set) return fail(c, UVAD_E_STATE, "uvad_fbank: uvad_set_tables has not been called");
    const int64_t T = uvad_num_frames(c, S);
    if (T <= 0) return fail(c, UVAD_E_ARG, "uvad_fbank: input shorter than one frame");
    HIPCHK(c, hipSetDevice(c->device));
    if (B > 65535) return fail(c, UVAD_E_UNSUPPORTED, "uvad_fbank: B > 65535 (grid.y); split the batch");
    FbankArgs a = fbank_cfg_args(c);
    a.pcm = d_pcm; a.pcm_is_i16 = is_i16; a.B = B; a.S = S; a.T = T; a.snip_edges = c->fb.snip_edges;
    a.feats = d_feats; a.plane_hi = plane_hi; a.plane_lo = plane_lo; a.plane_w = plane_w; a.nsamp = nsamp;
    HIPCHK(c, launch_fbank(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_fbank(uvad_ctx *c, const float *d_pcm, int B, int64_t S, float *d_feats, void *stream) {
    return fbank_impl(c, d_pcm, 0, B, S, d_feats, stream);
}
int uvad_fbank_i16(uvad_ctx *c, const int16_t *d_pcm, int B, int64_t S, float *d_feats, void *stream) {
    return fbank_impl(c, d_pcm, 1, B, S, d_feats, stream);
}
static int fbank_lens_entry(uvad_ctx *c, const void *d_pcm, int is_i16, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_nsamp) return fail(c, UVAD_E_ARG, "uvad_fbank_lens: d_nsamp is NULL");
    return fbank_impl(c, d_pcm, is_i16, B, S, d_feats, stream, nullptr, nullptr, 0, d_nsamp);
}
int uvad_fbank_lens(uvad_ctx *c, const float *d_pcm, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *stream) {
    return fbank_lens_entry(c, d_pcm, 0, B, S, d_nsamp, d_feats, stream);
}
int uvad_fbank_lens_i16(uvad_ctx *c, const int16_t *d_pcm, int B, int64_t S, const int64_t *d_nsamp, float *d_feats, void *stream) {
    return fbank_lens_entry(c, d_pcm, 1, B, S, d_nsamp, d_feats, stream);
}

// The feed-forward layers one GEMM each (leaky_relu epilogue): workspace buffers Y[last] -> Z[0] -> Z[1] ...; the last one f32.
// modes 1 and 3 use the weight-stationary projection and the fused head for large launches; mode 2 keeps the tile-streaming / per-layer
// kernels everywhere (A/B, reference of the tests); mode 3 = mode 1 with three MFMA products per f32-equivalent product in those
// large-launch kernels and in the 16-sequence recurrence (weights rounded to 22 bits: GemmArgs::products)
static bool mode_is_ws(const uvad_ctx *c) { return c->gemm_mode == 1 || c->gemm_mode == 3; }
static bool mode_fuses_head(const uvad_ctx *c) { return mode_is_ws(c); }
static int mode_products(const uvad_ctx *c) { return c->gemm_mode == 3 ? 3 : 4; }
static int feed_forward_layers(uvad_ctx *c, const WsLayout &w, char *base, int B, int T, bool f16, hipStream_t s) {
    const uvad_model_cfg &m = c->mc;
    const PackedWeights &W = *c->packed;
    auto Yf = [&](int i) { return reinterpret_cast<float *>(base + w.off_Y[i]); };
    auto Zf = [&](int i) { return reinterpret_cast<float *>(base + w.off_Z[i]); };
    auto hi_of = [&](size_t off) { return reinterpret_cast<unsigned short *>(base + off); };
    auto lo_of = [&](size_t off, int width) { return reinterpret_cast<unsigned short *>(base + off) + plane_rows(w.M) * (size_t)width; };
    const int last = (m.num_layers - 1) & 1;
    const float *cur = Yf(last);
    int curw = w.Wd;
    for (int j = 0; j < m.lin_layers; ++j) {
        GemmArgs g{};
        g.W = W.lin_w[j]; g.ldw = gemm_padded_k(curw); g.Wsplit16 = W.lin_w_split16[j]; g.wscale = W.lin_w_scale[j]; g.bias = W.lin_b[j];
        g.M = (int)w.M; g.N = m.lin_hidden; g.B = B; g.T = T; g.act = 1; g.leaky_slope = m.leaky_slope;
        if (f16) {
            const size_t in_off = j == 0 ? w.off_Y[last] : w.off_Z[(j - 1) & 1];
            const int in_w = j == 0 ? w.Wd : w.Zw;
            g.Ah = hi_of(in_off); g.Al = lo_of(in_off, in_w); g.lda = in_w; g.K = in_w;
            if (j + 1 < m.lin_layers) { g.out_planes = 1; g.Ch = hi_of(w.off_Z[j & 1]); g.Cl = lo_of(w.off_Z[j & 1], w.Zw); g.ldc = w.Zw; }
            else { g.C = Zf(j & 1); g.ldc = m.lin_hidden; }
            HIPCHK(c, launch_gemm_f16p(g, s));
        } else {
            g.A = cur; g.lda = curw; g.a_mode = 0; g.K = curw; g.C = Zf(j & 1); g.ldc = m.lin_hidden;
            HIPCHK(c, launch_gemm(g, s));
        }
        cur = Zf(j & 1);
        curw = m.lin_hidden;
    }
    return UVAD_OK;
}

// true if a streaming step of T new frames runs the LSTM stack as one launch (lstm_stack.hip)
static bool stream_uses_stack(const uvad_ctx *c, int T) {
    const uvad_model_cfg &m = c->mc;
    if (!lstm_stack_supported(m.hidden, m.bidirectional ? 2 : 1, m.in_dim, T, m.num_layers)) return false;
    for (const LayerDev &L : c->packed->layers)
        if (!L.w_ih_img) return false;
    return true;
}

// ... and its feed-forward layers + classifier inside that launch (every feed-forward layer 128 x 128)
static bool stream_head_in_stack(const uvad_ctx *c) {
    const uvad_model_cfg &m = c->mc;
    if (m.lin_layers > LSTM_STACK_MAX_LIN) return false;
    for (int j = 0; j < m.lin_layers; ++j)
        if (!c->packed->lin_w_img[j]) return false;
    return true;
}

// ---- time-chunked layers ---------------------------------------------------------------------------------------------------
// A batch's recurrence (4-sequence form) occupies tiles x directions CUs and the projection in front of it needs the whole chip for a
// fraction of that time; layer l + 1 cannot start before layer l has finished (its first frame needs the backward pass's LAST
// step), so with one launch per stage the projections sit exposed between the recurrences (cfg 2 alone on the GPU: 1.55 of 7.1 ms).
// Inside ONE layer nothing forces that: the forward pass at frame t needs the gate rows up to t only, the backward pass those from t
// on.  The layer is therefore cut into time chunks: the projection of chunk i + 1 (weight-stationary GEMM over the row tiles that
// chunk needs, GemmArgs::ws_tiles) runs on the library's side stream, on the CUs the recurrence leaves idle, while the recurrence of
// chunk i (LstmArgs::steps, state carried in the workspace) runs on the caller's stream; only the first chunk's projection is exposed.
// Same kernels, same arithmetic per row: bit-identical outputs (tests/test_gpu_scale.py).
static int streams_overlap_probe(hipStream_t a, hipStream_t b) {   // 1: kernels on a and b run concurrently, 0: they serialise, < 0: HIP error
    hipEvent_t ea = nullptr, eb = nullptr;
    if (hipEventCreateWithFlags(&ea, hipEventDisableTiming) != hipSuccess) return -1;
    if (hipEventCreateWithFlags(&eb, hipEventDisableTiming) != hipSuccess) { (void)hipEventDestroy(ea); return -1; }
    int result = -1;
    do {
        if (hipStreamSynchronize(a) != hipSuccess || hipStreamSynchronize(b) != hipSuccess) break;
        // 3 ms of spinning on a, then an empty spin on b: if b's kernel retires while a's is still running the two
        // streams sit on different hardware queues; on one queue b waits behind a.
        if (launch_spin(300000ull, nullptr, a) != hipSuccess || hipEventRecord(ea, a) != hipSuccess) break;
        if (launch_spin(0ull, nullptr, b) != hipSuccess || hipEventRecord(eb, b) != hipSuccess) break;
        if (hipEventSynchronize(eb) != hipSuccess) break;
        const hipError_t q = hipEventQuery(ea);
        if (q != hipSuccess && q != hipErrorNotReady) break;
        result = q == hipErrorNotReady ? 1 : 0;
        if (hipEventSynchronize(ea) != hipSuccess) result = -1;
    } while (0);
    (void)hipEventDestroy(ea);
    (void)hipEventDestroy(eb);
    return result;
}

// The side stream, PROVEN concurrent with the caller's stream s (HIP maps streams onto a few hardware queues and two streams on one
// queue serialise: the chunked schedule would then only add launches).  Probed once per (context, caller stream); never while s is
// being captured into a graph (the probe synchronises): a capture runs chunked only on a stream that has been used before.
static bool side_stream_for(uvad_ctx *c, hipStream_t s) {
    if (c->side && c->side_for == s && (s != nullptr || c->side_probed_for_null)) return true;
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess || cs != hipStreamCaptureStatusNone) return false;
    {
        auto f = c->side_failed.find(s);
        if (f != c->side_failed.end()) {
            if (--f->second > 0) return false;
            c->side_failed.erase(f);   // the verdict has expired: probe again
        }
    }
    // A stream that turns out to share s's hardware queue is kept alive until the search ends: destroyed at once, its queue would be
    // the least loaded one again and the next stream created would land on it too.
    std::vector<hipStream_t> same_queue;
    bool found = false;
    for (int attempt = 0; attempt < 6 && !found; ++attempt) {
        hipStream_t cand = c->side;   // first the one proven beside another caller stream, if any
        c->side = nullptr;
        if (!cand && hipStreamCreateWithFlags(&cand, hipStreamNonBlocking) != hipSuccess) break;
        const int r = streams_overlap_probe(s, cand);
        if (r == 1) {
            c->side = cand;
            c->side_for = s;
            c->side_probed_for_null = s == nullptr;
            found = true;
        } else {
            same_queue.push_back(cand);
            if (r < 0) break;
        }
    }
    for (hipStream_t q : same_queue) (void)hipStreamDestroy(q);
    if (found) return true;
    c->side_failed[s] = SIDE_RETRY_AFTER;
    return false;
}

static const ChunkPlan *chunk_plan(uvad_ctx *c, int tiles, int T, int D, int chunks, hipStream_t s) {
    const auto key = std::make_tuple(tiles, T, D, chunks);
    auto it = c->chunk_plans.find(key);
    hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cs) != hipSuccess) return nullptr;
    if (it != c->chunk_plans.end()) {
        it->second.last_use = ++c->plan_clock;
        if (cs != hipStreamCaptureStatusNone) it->second.pinned = true;
        return &it->second;
    }
    if (cs != hipStreamCaptureStatusNone) return nullptr;   // (a new plan allocates and copies: not inside a capture)
    if (c->chunk_plans.size() >= MAX_CHUNK_PLANS) {   // a caller that walks through many shapes: drop the least recently used list
        auto old = c->chunk_plans.end();
        for (auto j = c->chunk_plans.begin(); j != c->chunk_plans.end(); ++j)
            if (!j->second.pinned && (old == c->chunk_plans.end() || j->second.last_use < old->second.last_use)) old = j;
        if (old != c->chunk_plans.end()) {
            // eager launches that read the list may still be in flight: drain the device before the memory goes back (this path
            // already costs an allocation and a blocking copy); lists a graph captured stay (pinned)
            if (hipDeviceSynchronize() != hipSuccess) return nullptr;
            (void)hipFree(old->second.d_list);
            c->chunk_plans.erase(old);
        }
    }
    ChunkPlan P;
    P.last_use = ++c->plan_clock;
    // Chunk lengths grow geometrically (x 1.3): only chunk 0's projection is exposed, so it is the short one, and projection i + 1 --
    // on the CUs the recurrence leaves free, about half the chip -- still finishes inside recurrence i (per frame a projection on
    // half the chip takes ~2/3 of the recurrence's time: the ratio of consecutive lengths has to stay below ~1.5; 1.0 / 1.15 / 1.3 /
    // 1.4 measured 6.85 / 6.76 / 6.70 / 6.77 ms per cfg-2 step with six chunks, 7.2 unchunked).
    {
        std::vector<double> wgt(chunks);
        double sum = 0.0;
        for (int i = 0; i < chunks; ++i) sum += (wgt[i] = std::pow(1.3, i));
        P.bound.assign(1, 0);
        double acc = 0.0;
        for (int i = 0; i < chunks; ++i) {
            acc += wgt[i];
            const int b = i + 1 == chunks ? T : std::min(T, std::max(P.bound.back() + 1, (int)std::lround(acc / sum * T)));
            if (b > P.bound.back()) P.bound.push_back(b);
        }
        P.bound.back() = T;
        P.chunks = (int)P.bound.size() - 1;
    }
    auto chunk_of = [&](int t) { return (int)(std::upper_bound(P.bound.begin(), P.bound.end(), t) - P.bound.begin()) - 1; };
    const long rows_per_tile = (long)SEQ_TILE * T, M = (long)tiles * rows_per_tile, mt = (M + 127) / 128;
    std::vector<std::vector<int>> lists[2];
    for (int d = 0; d < 2; ++d) lists[d].assign(P.chunks, {});
    for (long r = 0; r < mt; ++r) {
        const long first = 128 * r, last = std::min(128 * r + 127, M - 1);
        int tmin, tmax;
        if (first / rows_per_tile != last / rows_per_tile) { tmin = 0; tmax = T - 1; }   // the tile spans the end of one sequence tile and the start of the next
        else { tmin = (int)((first % rows_per_tile) / SEQ_TILE); tmax = (int)((last % rows_per_tile) / SEQ_TILE); }
        lists[0][chunk_of(tmin)].push_back((int)r);
        lists[1][chunk_of(T - 1 - tmax)].push_back((int)r);
    }
    std::vector<int> flat;
    for (int d = 0; d < D; ++d)
        for (int i = 0; i < P.chunks; ++i) {
            P.off[d].push_back((int)flat.size());
            P.len[d].push_back((int)lists[d][i].size());
            flat.insert(flat.end(), lists[d][i].begin(), lists[d][i].end());
        }
    if (hipMalloc(reinterpret_cast<void **>(&P.d_list), std::max<size_t>(flat.size(), 1) * sizeof(int)) != hipSuccess) return nullptr;
    if (hipMemcpy(P.d_list, flat.data(), flat.size() * sizeof(int), hipMemcpyHostToDevice) != hipSuccess) { (void)hipFree(P.d_list); return nullptr; }
    return &(c->chunk_plans[key] = P);
}

// How many time chunks a layer of T frames is cut into when nothing is forced: none unless the recurrence leaves at least a quarter
// of the CUs to the projections; T / 96 chunks, at most 6 (each recurrence launch re-loads its weight image and costs ~10 us).
static int auto_time_chunks(int T, int tiles, int D, int n_cu) {
    if ((long)tiles * D * 4 > 3L * n_cu || T < 192) return 1;
    return std::min(6, T / 96);   // (lengths grow x 1.3 per chunk: six chunks of T = 1000 are 78 ... 290 frames)
}

// CUs a call's persistent projection grids may take when the caller keeps n steps in flight (uvad_set_concurrent_steps): what is left
// after the other n - 1 steps each hold the CUs of one recurrence launch (rec_cus workgroups, one per CU).  At least 1 (the launcher
// rounds to whole column-tile groups).  A reserve above SLOT_GRID_RESERVE_NUM / _DEN of the chip is not made: so many steps keep every
// CU taken whatever the grids are, and a smaller grid then only makes each projection longer (profiles/slot_grid.json).
constexpr long SLOT_GRID_RESERVE_NUM = 1, SLOT_GRID_RESERVE_DEN = 2;
static int slot_grid_cus(int n_cu, int n, int rec_cus) {
    const long reserve = (long)(n - 1) * rec_cus;
    if (reserve * SLOT_GRID_RESERVE_DEN > (long)n_cu * SLOT_GRID_RESERVE_NUM) return n_cu;
    return (int)std::max(1L, (long)n_cu - reserve);
}

// One run of the classifier (LSTM stack, feed-forward layers, head) on B sequences of T frames.  The options default to what uvad_classify
// asks for; every caller names the ones it sets.
struct ClassifyCall {
    const float *feats = nullptr;   // [B][T][in_dim] f32
    int B = 0, T = 0;
    float *logits = nullptr, *probs = nullptr;
    void *ws = nullptr;
    size_t ws_bytes = 0;
    hipStream_t stream = nullptr;
    bool record_start = true;       // record ev[0] here (false: the caller did, in front of its feature stage)
    // check_range: the features come from the caller (or from a front end with learnable scales) and may lie outside the f16
    // range; the split-f16 layer-0 projection is then replaced by the exact-f32 one ON THE DEVICE (both are enqueued, a flag
    // written by range_flag_kernel lets exactly one of them run), so the call stays asynchronous and capturable.
    bool check_range = true;
    const StreamState *stream_state = nullptr;   // a streaming step: (h, c) carried in the caller's state, updated in place
    int ld_out = 0;                 // row stride of logits / probs (0: T)
    bool feats_in_planes = false;   // the feature stage has written the first projection's f16 operand planes itself
    const FbankArgs *fused_fb = nullptr;   // the feature stage inside the one-launch stack (uvad_stream_step decides)
    // lens (uvad_classify_lens / uvad_forward_lens): device int32 [B] frame counts.  The recurrences run the lens forms (per-workgroup step
    // count, backward reset past each length), time chunks are off, and the outputs at t >= len_b are set to 0 after the head.  Rows past a
    // length carry padding values through the row-independent GEMMs and are never read by a valid row.
    const int *lens = nullptr;
    bool timed = true;                // record the timing events if uvad_set_timing asked for them (the step calls: never)
    bool time_chunks_allowed = true;  // follow uvad_set_time_chunks (false: unchunked whatever it says)
};
// the request of a caller's (B, T) problem on its buffers and stream, every option at its default
static ClassifyCall classify_call(const float *feats, int B, int T, float *logits, float *probs, void *ws, size_t ws_bytes, hipStream_t s) {
    ClassifyCall rq;
    rq.feats = feats; rq.B = B; rq.T = T; rq.logits = logits; rq.probs = probs; rq.ws = ws; rq.ws_bytes = ws_bytes; rq.stream = s;
    return rq;
}
static int classify_impl(uvad_ctx *c, const ClassifyCall &rq) {
    const float *d_feats = rq.feats;
    const int B = rq.B, T = rq.T, ld_out = rq.ld_out;
    float *d_logits = rq.logits, *d_probs = rq.probs;
    hipStream_t s = rq.stream;
    const bool check_range = rq.check_range, feats_in_planes = rq.feats_in_planes;
    const StreamState *ss = rq.stream_state;
    const FbankArgs *fused_fb = rq.fused_fb;
    const int *lens = rq.lens;
    const bool timing = rq.timed && c->timing;
    const int chunk_mode = rq.time_chunks_allowed ? c->chunk_mode : 1;
    const uvad_model_cfg &m = c->mc;
    const PackedWeights &W = *c->packed;
    const WsLayout w = carve(c, B, T);
    if (rq.ws_bytes < w.total) return fail(c, UVAD_E_WORKSPACE, "workspace too small: need " + std::to_string(w.total) + " bytes");
    if (w.M > (size_t)0x7fffffff) return fail(c, UVAD_E_UNSUPPORTED, "B*T exceeds 2^31 rows; split the batch");
    char *base = reinterpret_cast<char *>(rq.ws);
    float *G = reinterpret_cast<float *>(base + w.off_G);
    int *flag = reinterpret_cast<int *>(base + w.off_flag);
    const int H = m.hidden, D = w.D, N4 = 4 * H * D;
    // Activation buffer i as f32 rows, or as the (hi, lo) f16 planes of `width` columns
    auto Yf = [&](int i) { return reinterpret_cast<float *>(base + w.off_Y[i]); };
    auto Zf = [&](int i) { return reinterpret_cast<float *>(base + w.off_Z[i]); };
    auto hi_of = [&](size_t off) { return reinterpret_cast<unsigned short *>(base + off); };
    auto lo_of = [&](size_t off, int width) { return reinterpret_cast<unsigned short *>(base + off) + plane_rows(w.M) * (size_t)width; };
    // the split-f16 GEMM needs operands inside the f16 range: weights were checked by uvad_finalize (f16_ok)
    const bool f16 = f16_planes(c);
    // the last LSTM layer feeds the classifier kernel directly when there are no feed-forward layers: f32 then
    auto y_planes = [&](int k) { return f16 && (k + 1 < m.num_layers || m.lin_layers > 0); };
    if (timing && rq.record_start) HIPCHK(c, hipEventRecord(c->ev[0], s));
    if (timing) HIPCHK(c, hipEventRecord(c->ev[1], s));
    // Streaming steps of a causal model: the whole stack in one launch (lstm_stack.hip; every layer of a sequence depends on that
    // sequence only, so a workgroup takes its 4 sequences through all layers).  Needs the f32 features (uvad_stream_step asks the
    // feature kernel for them when stream_uses_stack() says so).
    const bool use_stack = ss && !feats_in_planes && stream_uses_stack(c, T);
    if (use_stack) {
        LstmStackArgs q{};
        q.feats = d_feats; q.kin0 = m.in_dim; q.n_layers = m.num_layers;
        for (int k = 0; k < m.num_layers; ++k) { q.wih[k] = W.layers[k].w_ih_img; q.whh[k] = W.layers[k].w_hh; q.bias[k] = W.layers[k].bias; }
        q.h = ss->h; q.c = ss->c; q.layer_stride = ss->layer_stride;
        const int lastl = m.num_layers - 1;
        if (y_planes(lastl)) { q.Yh = hi_of(w.off_Y[lastl & 1]); q.Yl = lo_of(w.off_Y[lastl & 1], w.Wd); }
        else q.Y = Yf(lastl & 1);
        q.ldy = w.Wd; q.tiles = w.tiles; q.T = T; q.B = B;
        // the head in the same launch when every feed-forward layer is 128 -> 128 (the default head)
        const bool head_in = d_logits != nullptr && stream_head_in_stack(c);
        if (fused_fb && !head_in) return fail(c, UVAD_E_STATE, "internal: fused feature stage without the in-launch head");
        if (fused_fb) { q.fb = *fused_fb; q.fb_on = 1; }   // the feature stage in the same launch (uvad_stream_step decided)
        if (head_in) {
            for (int j = 0; j < m.lin_layers; ++j) { q.lin_w[j] = W.lin_w_img[j]; q.lin_b[j] = W.lin_b[j]; }
            q.n_lin = m.lin_layers; q.cls_w = W.cls_w; q.cls_b = W.cls_b; q.slope = m.leaky_slope;
            q.logits = d_logits; q.probs = d_probs; q.ld_out = ld_out > 0 ? ld_out : T;
        }
        HIPCHK(c, launch_lstm_stack(q, s));
        c->rec_tile_used = 4;
        if (head_in) {
            if (timing) {
                HIPCHK(c, hipEventRecord(c->layer_ev[2 * m.num_layers], s));
                HIPCHK(c, hipEventRecord(c->ev[2], s));
                HIPCHK(c, hipEventRecord(c->ev[3], s));
                c->ev_valid = true;
            }
            return UVAD_OK;
        }
    }
    // time chunks (see above): only for the 4-sequence recurrence on the weight-stationary split-f16 projections, never for streaming steps
    int NC = 1;
    const ChunkPlan *plan = nullptr;
    if (!ss && !use_stack && !lens && f16 && mode_is_ws(c) && chunk_mode != 1 && (H == 128 || H == 64) &&
        (c->rec_tile_mode ? c->rec_tile_mode : lstm_auto_tile(w.tiles, D, H, c->n_cu)) == 4) {
        int want = chunk_mode > 1 ? std::min(chunk_mode, T) : auto_time_chunks(T, w.tiles, D, c->n_cu);
        const long mt = (long)((w.M + 127) / 128);
        while (want > 1 && (mt / want) * (N4 / 128) < 2L * c->n_cu) --want;   // every chunk must still be a launch the weight-stationary kernel takes
        if (want > 1 && side_stream_for(c, s) && (plan = chunk_plan(c, w.tiles, T, D, want, s)) != nullptr) {
            NC = plan->chunks;
            if (!c->ev_fork) HIPCHK(c, hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
            while ((int)c->ev_chunk.size() < NC) {
                hipEvent_t e = nullptr;
                HIPCHK(c, hipEventCreateWithFlags(&e, hipEventDisableTiming));
                c->ev_chunk.push_back(e);
            }
        }
    }
    c->chunks_used = NC;
    c->proj_grid_used = 0;
    // Steps in flight on other contexts (uvad_set_concurrent_steps(n), n > 1): a projection workgroup and a recurrence workgroup
    // exclude each other on a CU (registers), and a persistent grid over the whole chip holds every CU until its last tile is done, so
    // a recurrence that another step launches meanwhile cannot start one workgroup and the steps fall into lockstep.  The grid
    // therefore leaves the other n - 1 steps the CUs of a recurrence launch like this call's own; the tile queue hands out the same
    // tiles whatever the grid (same bits).  slot_grid_cus says where the cut stops paying.
    int cu_proj = c->n_cu;
    if (c->concurrent_steps > 1 && NC == 1 && !use_stack) {
        const bool tile16 = !ss && H == 128 && W.layers[0].w_hh16_ok &&
                            (c->rec_tile_mode ? c->rec_tile_mode : lstm_auto_tile(w.tiles, D, H, c->n_cu)) == 16;
        cu_proj = slot_grid_cus(c->n_cu, c->concurrent_steps, (tile16 ? (w.tiles + 3) / 4 : w.tiles) * D);
    }
    for (int k = 0; k < (use_stack ? 0 : m.num_layers); ++k) {
        const LayerDev &L = W.layers[k];
        GemmArgs g{};
        g.W = L.w_ih; g.ldw = gemm_padded_k(L.in); g.Wsplit16 = L.w_ih_split16; g.wscale = L.w_ih_scale; g.bias = L.bias; g.C = G;
        g.M = (int)w.M; g.N = N4; g.ldc = N4; g.c_blocked = 1; g.B = B; g.T = T; g.act = 0; g.leaky_slope = 0.f;
        if (timing) HIPCHK(c, hipEventRecord(c->layer_ev[2 * k], s));
        if (f16) {
            if (k == 0) {
                if (!feats_in_planes)   // (uvad_forward: the feature kernel has written the planes itself)
                    HIPCHK(c, launch_split_features(d_feats, B, T, m.in_dim, w.Fp, w.tiles, hi_of(w.off_fplanes), lo_of(w.off_fplanes, w.Fp),
                                                    check_range ? flag : nullptr, s));
                g.Ah = hi_of(w.off_fplanes); g.Al = lo_of(w.off_fplanes, w.Fp); g.lda = w.Fp; g.K = w.Fp;
                if (check_range) { g.gate = flag; g.gate_run_if_set = 0; }
            } else {
                g.Ah = hi_of(w.off_Y[(k - 1) & 1]); g.Al = lo_of(w.off_Y[(k - 1) & 1], w.Wd); g.lda = w.Wd; g.K = w.Wd;
            }
            g.products = mode_products(c);
            if (NC > 1 && !(k == 0 && check_range) && gemm_f16p_ws_supported(g, c->n_cu)) {
                // ---- the layer in NC time chunks: every chunk's projection on the side stream (they follow each other there), the
                //      recurrence of chunk i on s as soon as projection i has finished, state carried through the workspace
                HIPCHK(c, hipEventRecord(c->ev_fork, s));               // layer k - 1 (or the features) complete
                HIPCHK(c, hipStreamWaitEvent(c->side, c->ev_fork, 0));
                unsigned *ctr = reinterpret_cast<unsigned *>(base + w.off_ctr);
                // The projection's persistent grid is sized to the CUs the recurrence leaves free: workgroups beyond that would wait in
                // the dispatcher and take the CUs of a finishing recurrence chunk before the next chunk's workgroups arrive (each holds
                // its CU for a whole projection chunk: measured, the recurrence then ran 20 % longer and the overlap gained nothing).
                const int cu_side = std::max(c->n_cu / 4, c->n_cu - w.tiles * D);
                for (int i = 0; i < NC; ++i) {
                    GemmArgs gi = g;
                    gi.ws_tiles = plan->d_list; gi.ws_dirs = D;
                    for (int d = 0; d < D; ++d) { gi.ws_off[d] = plan->off[d][i]; gi.ws_len[d] = plan->len[d][i]; }
                    HIPCHK(c, launch_gemm_f16p_ws(gi, ctr, cu_side, c->side, &c->proj_grid_used));   // (chunk 0 too: on the whole chip it was 0.1 ms shorter and the layer's recurrences 0.3 ms longer)
                    HIPCHK(c, hipEventRecord(c->ev_chunk[i], c->side));
                }
                float *hst = reinterpret_cast<float *>(base + w.off_hc);
                float *cst = reinterpret_cast<float *>(base + w.off_hc + align_up((size_t)w.D * w.tiles * SEQ_TILE * m.hidden * sizeof(float)));
                for (int i = 0; i < NC; ++i) {
                    HIPCHK(c, hipStreamWaitEvent(s, c->ev_chunk[i], 0));
                    if (i == 0 && timing) HIPCHK(c, hipEventRecord(c->layer_ev[2 * k + 1], s));   // "projection" = what the recurrence had to wait for
                    LstmArgs r{};
                    r.G = G; r.ldg = N4; r.Whh_packed = L.w_hh; r.ldy = w.Wd;
                    if (y_planes(k)) { r.Yh = hi_of(w.off_Y[k & 1]); r.Yl = lo_of(w.off_Y[k & 1], w.Wd); }
                    else r.Y = Yf(k & 1);
                    r.tiles = w.tiles; r.T = T; r.H = H; r.dirs = D; r.tile_mode = 4; r.n_cu = c->n_cu; r.products = 4;
                    r.steps = plan->bound[i + 1] - plan->bound[i];
                    r.t_begin[0] = plan->bound[i];
                    r.t_begin[1] = T - plan->bound[i + 1];
                    r.h0 = i ? hst : nullptr; r.c0 = i ? cst : nullptr; r.hN = hst; r.cN = cst;
                    HIPCHK(c, launch_lstm(r, s, &c->rec_tile_used));
                }
                continue;
            }
            if (mode_is_ws(c) && gemm_f16p_ws_supported(g, c->n_cu))   // large launches: weights stay in registers, bit-identical gates
                HIPCHK(c, launch_gemm_f16p_ws(g, reinterpret_cast<unsigned *>(base + w.off_ctr), c->n_cu, s, &c->proj_grid_used, cu_proj));
            else
                HIPCHK(c, launch_gemm_f16p(g, s));
            if (k == 0 && check_range) {   // the same projection by the exact kernel, run only if the flag is set
                g.A = d_feats; g.lda = m.in_dim; g.a_mode = 1; g.K = L.in; g.gate_run_if_set = 1;
                HIPCHK(c, launch_gemm(g, s));
            }
        } else {
            g.K = L.in;
            if (k == 0) { g.A = d_feats; g.lda = m.in_dim; g.a_mode = 1; }
            else { g.A = Yf((k - 1) & 1); g.lda = w.Wd; g.a_mode = 0; }
            HIPCHK(c, launch_gemm(g, s));
        }
        if (timing) HIPCHK(c, hipEventRecord(c->layer_ev[2 * k + 1], s));
        LstmArgs r{};
        r.G = G; r.ldg = N4; r.Whh_packed = L.w_hh; r.ldy = w.Wd;
        if (L.w_hh16_ok) {
            r.Whh16h_regs = L.w_hh16_regs; r.Whh16h_p2 = L.w_hh16_p2; r.whh16h_scale = L.w_hh16_scale;
            r.Whh16h_p2q = c->gemm_mode == 2 ? nullptr : L.w_hh16_p2q;   // mode 2 = the kernel set kept for comparisons: P2 from its f16 image
            r.p2q_scale = L.w_hh16_p2q_scale;
        }
        if (y_planes(k)) { r.Yh = hi_of(w.off_Y[k & 1]); r.Yl = lo_of(w.off_Y[k & 1], w.Wd); }
        else r.Y = Yf(k & 1);
        r.tiles = w.tiles; r.T = T; r.H = H; r.dirs = D; r.tile_mode = ss ? 4 : c->rec_tile_mode; r.n_cu = c->n_cu;
        r.products = f16 ? mode_products(c) : 4;
        r.lens = lens; r.nB = B;
        if (ss) {   // carried (h, c) of this layer, updated in place
            r.h0 = r.hN = ss->h + (size_t)k * ss->layer_stride;
            r.c0 = r.cN = ss->c + (size_t)k * ss->layer_stride;
        }
        HIPCHK(c, launch_lstm(r, s, &c->rec_tile_used));
    }
    if (timing) HIPCHK(c, hipEventRecord(c->layer_ev[2 * m.num_layers], s));
    if (timing) HIPCHK(c, hipEventRecord(c->ev[2], s));
    const int last = (m.num_layers - 1) & 1;
    // The default head (two 128-unit feed-forward layers) in split-f16 mode, large launches: feed-forward layers, classifier and
    // sigmoid in one kernel (head_fused.hip); the LSTM output planes are read once and nothing but the logits is written.
    // (uvad_get_taps recomputes the feed-forward output from those planes when it is asked for.)
    if (f16 && mode_fuses_head(c) && head_fused_supported(w.Wd, m.lin_hidden, m.lin_layers, (long long)w.M, c->n_cu)) {
        HeadArgs h{};
        h.Yh = hi_of(w.off_Y[last]); h.Yl = lo_of(w.off_Y[last], w.Wd); h.M = (long long)w.M; h.K1 = w.Wd;
        h.W1 = W.lin_w_split16[0]; h.W2 = W.lin_w_split16[1]; h.w1scale = W.lin_w_scale[0]; h.w2scale = W.lin_w_scale[1];
        h.b1 = W.lin_b[0]; h.b2 = W.lin_b[1]; h.wc = W.cls_w; h.bc = W.cls_b; h.slope = m.leaky_slope;
        h.logits = d_logits; h.probs = d_probs; h.tiles = w.tiles; h.T = T; h.B = B; h.ld_out = ld_out > 0 ? ld_out : T;
        h.counter = reinterpret_cast<unsigned *>(base + w.off_ctr);
        h.products = mode_products(c);
        // (its workgroups take a whole CU's registers as the projections' do: the same share of the chip, at least a quarter)
        HIPCHK(c, launch_head_fused(h, std::max(c->n_cu / 4, cu_proj), s));
        if (lens) HIPCHK(c, launch_lens_fill(d_logits, d_probs, B, T, h.ld_out, lens, s));
        if (timing) {
            HIPCHK(c, hipEventRecord(c->ev[3], s));
            c->ev_valid = true;
        }
        return UVAD_OK;
    }
    int r_ff = feed_forward_layers(c, w, base, B, T, f16, s);
    if (r_ff) return r_ff;
    const float *cur = m.lin_layers > 0 ? Zf((m.lin_layers - 1) & 1) : Yf(last);
    const int curw = m.lin_layers > 0 ? m.lin_hidden : w.Wd;
    ClsArgs q{};
    q.Z = cur; q.ldz = curw; q.K = curw; q.w = W.cls_w; q.b = W.cls_b; q.logits = d_logits; q.probs = d_probs;
    q.tiles = w.tiles; q.T = T; q.B = B; q.ld_out = ld_out > 0 ? ld_out : T;
    HIPCHK(c, launch_classifier(q, s));
    if (lens) HIPCHK(c, launch_lens_fill(d_logits, d_probs, B, T, q.ld_out, lens, s));
    if (timing) {
        HIPCHK(c, hipEventRecord(c->ev[3], s));
        c->ev_valid = true;
    }
    return UVAD_OK;
}

int uvad_classify(uvad_ctx *c, const float *d_feats, int B, int T, float *d_logits, float *d_probs,
                  void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_feats || B <= 0 || T <= 0 || !ws) return fail(c, UVAD_E_ARG, "uvad_classify: bad argument");
    if (!c->finalized) return fail(c, UVAD_E_STATE, "uvad_classify: uvad_finalize has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    return classify_impl(c, classify_call(d_feats, B, T, d_logits, d_probs, ws, ws_bytes, (hipStream_t)stream));
}

int uvad_classify_lens(uvad_ctx *c, const float *d_feats, int B, int T, const int32_t *d_lens, float *d_logits, float *d_probs,
                       void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_feats || B <= 0 || T <= 0 || !ws) return fail(c, UVAD_E_ARG, "uvad_classify_lens: bad argument");
    if (!d_lens) return fail(c, UVAD_E_ARG, "uvad_classify_lens: d_lens is NULL");
    if (!c->finalized) return fail(c, UVAD_E_STATE, "uvad_classify_lens: uvad_finalize has not been called");
    const WsLayout w = carve(c, B, T);
    if (ws_bytes < w.total) return fail(c, UVAD_E_WORKSPACE, "workspace too small: need " + std::to_string(w.total) + " bytes");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], s));
    // the caller's padding frames are never read: the classifier runs on a copy whose padding is zero (split, range check and the exact
    // projection all read that copy)
    float *masked = reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + w.off_feats);
    HIPCHK(c, launch_mask_features(d_feats, B, T, c->mc.in_dim, d_lens, masked, s));
    ClassifyCall rq = classify_call(masked, B, T, d_logits, d_probs, ws, ws_bytes, s);
    rq.record_start = false; rq.lens = d_lens;
    return classify_impl(c, rq);
}

static int forward_impl(uvad_ctx *c, const void *d_pcm, int is_i16, int B, int64_t S, float *d_logits, float *d_probs,
                        void *ws, size_t ws_bytes, void *stream, const int64_t *nsamp = nullptr) {
    if (!c) return UVAD_E_ARG;
    if (!d_pcm || B <= 0 || S <= 0 || !ws) return fail(c, UVAD_E_ARG, "uvad_forward: bad argument");
    if (!c->finalized) return fail(c, UVAD_E_STATE, "uvad_forward: uvad_finalize has not been called");
    if (!c->has_fb || !c->tables_set) return fail(c, UVAD_E_STATE, "uvad_forward: uvad_set_tables has not been called");
    if (c->fb.n_mels != c->mc.in_dim) return fail(c, UVAD_E_ARG, "uvad_forward: n_mels != encoding_dim");
    const int64_t T = uvad_num_frames(c, S);
    if (T <= 0 || T > 0x7fffffff) return fail(c, UVAD_E_ARG, "uvad_forward: bad frame count");
    const WsLayout w = carve(c, B, T);
    if (ws_bytes < w.total) return fail(c, UVAD_E_WORKSPACE, "workspace too small: need " + std::to_string(w.total) + " bytes");
    float *feats = reinterpret_cast<float *>(reinterpret_cast<char *>(ws) + w.off_feats);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], s));
    // split-f16 GEMM mode: the feature kernel writes the two f16 planes the first projection reads (K-blocked, tile-major rows) and
    // the f32 feature tensor never exists; exact-f32 mode: f32 features.  (log-mel values are within +-90: no range check.)
    const bool planes = f16_planes(c);
    unsigned short *ph = reinterpret_cast<unsigned short *>(reinterpret_cast<char *>(ws) + w.off_fplanes);
    int r = planes ? fbank_impl(c, d_pcm, is_i16, B, S, nullptr, stream, ph, ph + plane_rows(w.M) * (size_t)w.Fp, w.Fp, nsamp)
                   : fbank_impl(c, d_pcm, is_i16, B, S, feats, stream, nullptr, nullptr, 0, nsamp);
    if (r) return r;
    int *lens = nullptr;
    if (nsamp) {   // frame counts of the rows, in the workspace of the time chunks' carried state (a lens call runs unchunked)
        lens = reinterpret_cast<int *>(reinterpret_cast<char *>(ws) + w.off_hc);
        HIPCHK(c, launch_frames_of(nsamp, B, S, c->fb.frame_len, c->fb.frame_shift, c->fb.snip_edges, lens, s));
    }
    ClassifyCall rq = classify_call(feats, B, (int)T, d_logits, d_probs, ws, ws_bytes, s);
    rq.record_start = false; rq.check_range = false; rq.feats_in_planes = planes; rq.lens = lens;
    return classify_impl(c, rq);
}

int uvad_forward(uvad_ctx *c, const float *d_pcm, int B, int64_t S, float *d_logits, float *d_probs,
                 void *ws, size_t ws_bytes, void *stream) {
    return forward_impl(c, d_pcm, 0, B, S, d_logits, d_probs, ws, ws_bytes, stream);
}

int uvad_forward_i16(uvad_ctx *c, const int16_t *d_pcm, int B, int64_t S, float *d_logits, float *d_probs,
                     void *ws, size_t ws_bytes, void *stream) {
    return forward_impl(c, d_pcm, 1, B, S, d_logits, d_probs, ws, ws_bytes, stream);
}

static int forward_lens_entry(uvad_ctx *c, const void *d_pcm, int is_i16, int B, int64_t S, const int64_t *d_nsamp, float *d_logits,
                              float *d_probs, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_nsamp) return fail(c, UVAD_E_ARG, "uvad_forward_lens: d_nsamp is NULL");
    return forward_impl(c, d_pcm, is_i16, B, S, d_logits, d_probs, ws, ws_bytes, stream, d_nsamp);
}
int uvad_forward_lens(uvad_ctx *c, const float *d_pcm, int B, int64_t S, const int64_t *d_nsamp, float *d_logits, float *d_probs,
                      void *ws, size_t ws_bytes, void *stream) {
    return forward_lens_entry(c, d_pcm, 0, B, S, d_nsamp, d_logits, d_probs, ws, ws_bytes, stream);
}
int uvad_forward_lens_i16(uvad_ctx *c, const int16_t *d_pcm, int B, int64_t S, const int64_t *d_nsamp, float *d_logits, float *d_probs,
                          void *ws, size_t ws_bytes, void *stream) {
    return forward_lens_entry(c, d_pcm, 1, B, S, d_nsamp, d_logits, d_probs, ws, ws_bytes, stream);
}

// nsamp (uvad_forward_wav_lens): the SincNet stage in its lens form, then the classifier with lens = the rows' frame counts T_b (the
// geometry block of the SincNet workspace): time chunks off, outputs at t >= T_b exactly +0.
static int forward_wav_impl(uvad_ctx *c, const void *d_wav, int is_i16, int B, int64_t S, float *d_logits, float *d_probs,
                            void *ws, size_t ws_bytes, void *stream, const int64_t *nsamp = nullptr) {
    if (!c) return UVAD_E_ARG;
    if (!d_wav || B <= 0 || S <= 0 || !ws) return fail(c, UVAD_E_ARG, "uvad_forward_wav: bad argument");
    if (!c->has_sinc) return fail(c, UVAD_E_STATE, "uvad_forward_wav: uvad_sincnet_configure has not been called");
    if (!c->finalized) return fail(c, UVAD_E_STATE, "uvad_forward_wav: uvad_finalize has not been called");
    const int64_t T = uvad_sincnet_num_frames(c, S);
    if (T <= 0 || T > 0x7fffffff) return fail(c, UVAD_E_ARG, "uvad_forward_wav: waveform too short for one output frame");
    const WsLayout w = carve(c, B, T);
    const size_t sn = sinc_carve(c, B, S).total;
    if (ws_bytes < w.total + sn) return fail(c, UVAD_E_WORKSPACE, "workspace too small: need " + std::to_string(w.total + sn) + " bytes");
    char *base = reinterpret_cast<char *>(ws);
    float *feats = reinterpret_cast<float *>(base + w.off_feats);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->timing) HIPCHK(c, hipEventRecord(c->ev[0], s));
    const int *lens = nullptr;
    int r = sincnet_impl(c, d_wav, is_i16, B, S, feats, base + w.total, ws_bytes - w.total, s, nsamp, &lens);
    if (r) return r;
    ClassifyCall rq = classify_call(feats, B, (int)T, d_logits, d_probs, ws, w.total, s);
    rq.record_start = false; rq.lens = lens;
    return classify_impl(c, rq);
}

int uvad_forward_wav(uvad_ctx *c, const float *d_wav, int B, int64_t S, float *d_logits, float *d_probs,
                     void *ws, size_t ws_bytes, void *stream) {
    return forward_wav_impl(c, d_wav, 0, B, S, d_logits, d_probs, ws, ws_bytes, stream);
}
int uvad_forward_wav_i16(uvad_ctx *c, const int16_t *d_wav, int B, int64_t S, float *d_logits, float *d_probs,
                         void *ws, size_t ws_bytes, void *stream) {
    return forward_wav_impl(c, d_wav, 1, B, S, d_logits, d_probs, ws, ws_bytes, stream);
}
static int forward_wav_lens_entry(uvad_ctx *c, const void *d_wav, int is_i16, int B, int64_t S, const int64_t *d_nsamp, float *d_logits,
                                  float *d_probs, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_nsamp) return fail(c, UVAD_E_ARG, "uvad_forward_wav_lens: d_nsamp is NULL");
    return forward_wav_impl(c, d_wav, is_i16, B, S, d_logits, d_probs, ws, ws_bytes, stream, d_nsamp);
}
int uvad_forward_wav_lens(uvad_ctx *c, const float *d_wav, int B, int64_t S, const int64_t *d_nsamp, float *d_logits, float *d_probs,
                          void *ws, size_t ws_bytes, void *stream) {
    return forward_wav_lens_entry(c, d_wav, 0, B, S, d_nsamp, d_logits, d_probs, ws, ws_bytes, stream);
}
int uvad_forward_wav_lens_i16(uvad_ctx *c, const int16_t *d_wav, int B, int64_t S, const int64_t *d_nsamp, float *d_logits, float *d_probs,
                              void *ws, size_t ws_bytes, void *stream) {
    return forward_wav_lens_entry(c, d_wav, 1, B, S, d_nsamp, d_logits, d_probs, ws, ws_bytes, stream);
}

int uvad_get_taps(uvad_ctx *c, int B, int T, float *d_lstm_out, float *d_lin_out, const void *ws, void *stream) {
    if (!c || !ws || B <= 0 || T <= 0) return UVAD_E_ARG;
    if (!c->finalized) return fail(c, UVAD_E_STATE, "not finalized");
    HIPCHK(c, hipSetDevice(c->device));
    const uvad_model_cfg &m = c->mc;
    const WsLayout w = carve(c, B, T);
    const char *base = reinterpret_cast<const char *>(ws);
    if (d_lstm_out) {
        const char *y = base + w.off_Y[(m.num_layers - 1) & 1];
        const bool planes = f16_planes(c) && m.lin_layers > 0;   // what classify_impl made the last layer write
        HIPCHK(c, launch_untile(y, planes ? y + plane_rows(w.M) * (size_t)w.Wd * sizeof(unsigned short) : nullptr, w.Wd, w.Wd, d_lstm_out, w.tiles, T, B,
                                (hipStream_t)stream));
    }
    if (d_lin_out) {
        if (m.lin_layers <= 0) return fail(c, UVAD_E_ARG, "model has no feed-forward layers");
        const bool f16 = f16_planes(c);
        if (f16 && mode_fuses_head(c) && head_fused_supported(w.Wd, m.lin_hidden, m.lin_layers, (long long)w.M, c->n_cu)) {
            // the fused head keeps the feed-forward activations on chip: recompute them from the LSTM output planes of the last call
            // with the per-layer kernels -- four products, exact weights: the bits of the fused head in modes 1 / 2.  In mode 3 the
            // fused head ran THREE products on rounded weights and the per-layer kernels have no such form, so the tap that
            // produced the logits cannot be reproduced: refuse instead of returning a near-miss.
            if (mode_products(c) != 4)
                return fail(c, UVAD_E_UNSUPPORTED, "uvad_get_taps: the feed-forward tap is not available in GEMM mode 3 (fused head, three products); "
                                                   "pass d_lin_out = NULL or use mode 1");
            int r = feed_forward_layers(c, w, const_cast<char *>(base), B, T, true, (hipStream_t)stream);
            if (r) return r;
        }
        const float *z = reinterpret_cast<const float *>(base + w.off_Z[(m.lin_layers - 1) & 1]);
        HIPCHK(c, launch_untile(z, nullptr, m.lin_hidden, m.lin_hidden, d_lin_out, w.tiles, T, B, (hipStream_t)stream));
    }
    return UVAD_OK;
}

// ---- streaming ---------------------------------------------------------------------------------
// state layout (bytes, 256-aligned blocks): tail[2][B][frame_len] f32 (ping-pong) | per layer: h [Bpad][H], c [Bpad][H]
extern "C++" {
namespace {
struct StreamLayout {
    int tail = 0, Bpad = 0;
    size_t off_tail[2] = {0, 0}, off_h = 0, off_c = 0, layer_stride = 0, total = 0;
};
StreamLayout stream_layout(const uvad_ctx *c, int B) {
    StreamLayout L;
    L.tail = c->fb.frame_len;
    L.Bpad = (B + SEQ_TILE - 1) / SEQ_TILE * SEQ_TILE;
    size_t o = 0;
    for (int i = 0; i < 2; ++i) { L.off_tail[i] = o; o += align_up((size_t)B * L.tail * sizeof(float)); }
    L.layer_stride = align_up((size_t)L.Bpad * c->mc.hidden * sizeof(float));
    L.off_h = o; o += L.layer_stride * c->mc.num_layers;
    L.off_c = o; o += L.layer_stride * c->mc.num_layers;
    L.total = o;
    return L;
}
int stream_max_frames(const uvad_ctx *c, int chunk) { return chunk / c->fb.frame_shift + 1; }
// What the next step of a stream group does, from its host-side counters: which tail buffer it reads, whether it is the first
// chunk (left reflection), how many frames it completes and where the first of them starts inside a staging row.
struct StreamPlan { int parity = 0, first = 0, k = 0; int64_t offset = 0, n_after = 0; };
StreamPlan stream_plan(const uvad_ctx *c, const StreamCounters &sc, int chunk) {
    const int L = c->fb.frame_len, sh = c->fb.frame_shift, n_left = (L - sh) / 2;
    StreamPlan p;
    p.parity = (int)(sc.n_steps & 1);
    p.first = sc.n_samples == 0 ? 1 : 0;
    const int64_t n_prev = sc.n_samples, n = n_prev + chunk;
    // frame t spans [t*sh - n_left, t*sh - n_left + L): complete once n >= t*sh - n_left + L
    const int64_t f_hi = n + n_left - L >= 0 ? (n + n_left - L) / sh : -1;
    p.k = (int)(f_hi - (sc.n_frames - 1));
    if (p.k < 0) p.k = 0;
    p.n_after = n;
    p.offset = p.k > 0 ? sc.n_frames * sh - n_left - (n_prev - L) : 0;   // offset of the first new frame inside a staging row (tail = L samples)
    return p;
}
// The feature stage of a step with p.k > 0 frames: VIRTUAL rows [tail (frame_len samples) | chunk] read from p.offset on (FbankArgs::vs_*);
// the kernel also writes the next tail.  Output pointers (feats / planes) are the caller's.
FbankArgs stream_fbank_args(const uvad_ctx *c, const float *d_pcm_chunk, int B, int chunk, const StreamPlan &p, const float *staging,
                            const float *tail_in, float *tail_out) {
    const int L = c->fb.frame_len, sh = c->fb.frame_shift;
    FbankArgs fa = fbank_cfg_args(c);
    fa.pcm = staging + p.offset; fa.pcm_is_i16 = 0; fa.B = B; fa.S = (int64_t)(L + chunk) - p.offset; fa.T = p.k;
    fa.vs_chunk = d_pcm_chunk; fa.vs_tail_in = tail_in; fa.vs_tail_out = tail_out;
    fa.vs_tail = L; fa.vs_chunk_len = chunk; fa.vs_first = p.first; fa.vs_n_left = (L - sh) / 2; fa.vs_offset = (int)p.offset;
    fa.row_stride = L + chunk; fa.snip_edges = 1;
    return fa;
}
}  // namespace
}  // extern "C++"

size_t uvad_stream_state_bytes(const uvad_ctx *c, int B) {
    if (!c || !c->has_fb || !c->has_model || B <= 0) return 0;
    return stream_layout(c, B).total;
}

size_t uvad_stream_workspace_bytes(const uvad_ctx *c, int B, int chunk) {
    if (!c || !c->has_fb || !c->has_model || B <= 0 || chunk <= 0) return 0;
    const size_t staging = align_up((size_t)B * (c->fb.frame_len + chunk) * sizeof(float));
    return staging + carve(c, B, stream_max_frames(c, chunk)).total;
}

int uvad_stream_reset(uvad_ctx *c, void *d_state, int B, void *stream) {
    if (!c || !d_state || B <= 0) return UVAD_E_ARG;
    if (!c->has_fb || !c->has_model) return fail(c, UVAD_E_STATE, "streaming needs both a fbank and a model configuration");
    if (c->mc.bidirectional) return fail(c, UVAD_E_UNSUPPORTED, "streaming needs a causal model (lstm.bidirectional = False)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(d_state, 0, stream_layout(c, B).total, (hipStream_t)stream));
    c->streams[d_state] = StreamCounters();
    return UVAD_OK;
}

int uvad_stream_step(uvad_ctx *c, const float *d_pcm_chunk, int B, int chunk, void *d_state, float *d_logits, int ld_logits,
                     void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_pcm_chunk || !d_state || !d_logits || !ws || B <= 0 || chunk <= 0) return fail(c, UVAD_E_ARG, "uvad_stream_step: bad argument");
    if (!c->finalized || !c->has_fb || !c->tables_set) return fail(c, UVAD_E_STATE, "uvad_stream_step: context not ready (tables / weights)");
    if (c->mc.bidirectional) return fail(c, UVAD_E_UNSUPPORTED, "streaming needs a causal model (lstm.bidirectional = False)");
    if (c->fb.snip_edges) return fail(c, UVAD_E_UNSUPPORTED, "streaming implements the centred (snip_edges = 0) framing only");
    if (c->fb.n_mels != c->mc.in_dim) return fail(c, UVAD_E_ARG, "n_mels != encoding_dim");
    auto it = c->streams.find(d_state);
    if (it == c->streams.end()) return fail(c, UVAD_E_STATE, "uvad_stream_step: call uvad_stream_reset on this state first");
    StreamCounters &sc = it->second;
    const int L = c->fb.frame_len, sh = c->fb.frame_shift, n_left = (L - sh) / 2;
    if (sc.n_samples == 0 && chunk < n_left) return fail(c, UVAD_E_ARG, "first chunk must hold at least (frame_len - shift)/2 samples");
    if (ws_bytes < uvad_stream_workspace_bytes(c, B, chunk)) return fail(c, UVAD_E_WORKSPACE, "stream workspace too small");
    const StreamLayout S = stream_layout(c, B);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    char *st = reinterpret_cast<char *>(d_state);
    char *wsb = reinterpret_cast<char *>(ws);
    float *staging = reinterpret_cast<float *>(wsb);
    const size_t staging_bytes = align_up((size_t)B * (L + chunk) * sizeof(float));
    const StreamPlan plan = stream_plan(c, sc, chunk);
    const int par = plan.parity;
    const int k = plan.k;
    // A step that produces frames reads its rows straight from the chunk and the carried tail inside the feature kernel, which also
    // writes the next tail (FbankArgs::vs_*); only a step without frames (a short first chunk) runs the staging kernel for the tail.
    if (k > ld_logits) return fail(c, UVAD_E_ARG, "ld_logits smaller than the number of new frames");   // (before anything moves: the call can be repeated)
    if (k <= 0)
        HIPCHK(c, launch_stream_stage(d_pcm_chunk, B, chunk, S.tail, n_left, plan.first,
                                      reinterpret_cast<const float *>(st + S.off_tail[par]),
                                      reinterpret_cast<float *>(st + S.off_tail[par ^ 1]), staging, s));
    sc.n_samples = plan.n_after;
    sc.n_steps += 1;
    if (k <= 0) return 0;
    sc.n_frames += k;
    void *cws = wsb + staging_bytes;
    const WsLayout w = carve(c, B, k);
    float *feats = reinterpret_cast<float *>(reinterpret_cast<char *>(cws) + w.off_feats);
    FbankArgs fa = stream_fbank_args(c, d_pcm_chunk, B, chunk, plan, staging, reinterpret_cast<const float *>(st + S.off_tail[par]),
                                     reinterpret_cast<float *>(st + S.off_tail[par ^ 1]));
    fa.feats = feats;
    // as in uvad_forward: features straight into the first projection's operand planes -- unless the one-launch stack runs (f32 features)
    const bool planes = f16_planes(c) && !stream_uses_stack(c, k);
    if (planes) {
        fa.plane_hi = reinterpret_cast<unsigned short *>(reinterpret_cast<char *>(cws) + w.off_fplanes);
        fa.plane_lo = fa.plane_hi + plane_rows(w.M) * (size_t)w.Fp;
        fa.plane_w = w.Fp;
    }
    // One launch for the whole step when the stack kernel also takes the head and the feature stage fits beside it (lstm_stack.hip)
    const bool fuse_fb = !planes && stream_uses_stack(c, k) && stream_head_in_stack(c) && lstm_stack_fb_lds_bytes(fa, k) > 0;
    if (!fuse_fb) HIPCHK(c, launch_fbank(fa, s));
    StreamState ss;
    ss.h = reinterpret_cast<float *>(st + S.off_h); ss.c = reinterpret_cast<float *>(st + S.off_c);
    ss.layer_stride = S.layer_stride / sizeof(float);
    ClassifyCall rq = classify_call(feats, B, k, d_logits, nullptr, cws, ws_bytes - staging_bytes, s);
    rq.timed = false; rq.record_start = false; rq.check_range = false;
    rq.stream_state = &ss; rq.ld_out = ld_logits; rq.feats_in_planes = planes; rq.fused_fb = fuse_fb ? &fa : nullptr;
    const int r = classify_impl(c, rq);
    return r < 0 ? r : k;
}

int uvad_stream_peek(const uvad_ctx *c, const void *d_state, int chunk, int *k, int64_t *offset, int *parity, int *first) {
    if (!c || !d_state || chunk <= 0 || !k || !offset || !parity || !first) return UVAD_E_ARG;
    auto it = c->streams.find(const_cast<void *>(d_state));
    if (it == c->streams.end() || !c->has_fb) return UVAD_E_STATE;
    const StreamPlan p = stream_plan(c, it->second, chunk);
    *k = p.k; *offset = p.offset; *parity = p.parity; *first = p.first;
    return UVAD_OK;
}

int uvad_stream_advance(uvad_ctx *c, void *d_state, int chunk) {
    if (!c || !d_state || chunk <= 0) return UVAD_E_ARG;
    auto it = c->streams.find(d_state);
    if (it == c->streams.end() || !c->has_fb) return fail(c, UVAD_E_STATE, "uvad_stream_advance: call uvad_stream_reset on this state first");
    StreamCounters &sc = it->second;
    const StreamPlan p = stream_plan(c, sc, chunk);
    sc.n_samples = p.n_after;
    sc.n_steps += 1;
    sc.n_frames += p.k;
    return p.k;
}

// ---- windowed streaming ------------------------------------------------------------------------
// state layout (bytes, 256-aligned blocks): tail[2][B][frame_len] f32 (ping-pong, as the stream) | ring [B][W][n_mels] f32 |
// ctr[2] int64 (frames complete: ctr[parity] before a step, ctr[parity ^ 1] after it)
// workspace: staging [B][frame_len + chunk] (steps without frames) | new frames [B][kmax][n_mels] | logits, probs [B][W] | classifier
//            workspace of (B, W) (carve() grows with T, so it holds every warm-up window too)
extern "C++" {
namespace {
struct WindowLayout {
    size_t off_tail[2] = {0, 0}, off_ring = 0, off_ctr = 0, total = 0;
};
WindowLayout window_layout(const uvad_ctx *c, int B, int W) {
    WindowLayout L;
    size_t o = 0;
    for (int i = 0; i < 2; ++i) { L.off_tail[i] = o; o += align_up((size_t)B * c->fb.frame_len * sizeof(float)); }
    L.off_ring = o; o += align_up((size_t)B * W * c->fb.n_mels * sizeof(float));
    L.off_ctr = o; o += align_up(2 * sizeof(long long));
    L.total = o;
    return L;
}
struct WindowWs {
    size_t off_new = 0, off_logits = 0, off_probs = 0, off_cls = 0, total = 0;
};
WindowWs window_ws(const uvad_ctx *c, int B, int chunk, int W) {
    WindowWs w;
    size_t o = align_up((size_t)B * (c->fb.frame_len + chunk) * sizeof(float));
    w.off_new = o; o += align_up((size_t)B * stream_max_frames(c, chunk) * c->fb.n_mels * sizeof(float));
    w.off_logits = o; o += align_up((size_t)B * W * sizeof(float));
    w.off_probs = o; o += align_up((size_t)B * W * sizeof(float));
    w.off_cls = o; o += carve(c, B, W).total;
    w.total = o;
    return w;
}
// What the next step of a window group does: the stream's plan for the feature stage (k new frames), the window [e - Tw, e) it
// classifies and the rows [r0, r0 + n_emit) of that window it emits (frames [max(0, e_prev - L), max(0, e - L))).
struct WindowPlan { StreamPlan fp; int64_t e = 0; int Tw = 0, r0 = 0, n_emit = 0; int64_t key = -1; };
WindowPlan window_plan(const uvad_ctx *c, const WindowGroup &g, int chunk) {
    WindowPlan p;
    p.fp = stream_plan(c, g.sc, chunk);
    const int64_t e_prev = g.sc.n_frames;
    p.e = e_prev + p.fp.k;
    p.Tw = (int)std::min<int64_t>(p.e, g.W);
    const int64_t f0 = std::max<int64_t>(0, e_prev - g.L), f1 = std::max<int64_t>(0, p.e - g.L);
    p.n_emit = (int)(f1 - f0);
    p.r0 = (int)(f0 - (p.e - p.Tw));
    // Once the window is full, everything that moves from step to step is read from the device (ring position, counter); what the launch
    // arguments still carry is k, the staging offset and the parity (Tw = W, r0 = W - L - k, n_emit = k follow from them)
    if (!p.fp.first && p.e >= g.W) p.key = ((int64_t)p.fp.k << 32) | (p.fp.offset << 1) | p.fp.parity;
    return p;
}
void window_advance(WindowGroup &g, const WindowPlan &p) {
    g.sc.n_samples = p.fp.n_after;
    g.sc.n_steps += 1;
    g.sc.n_frames = p.e;
}
int window_check_cfg(uvad_ctx *c, const char *who) {
    if (!c->has_fb || !c->has_model) return fail(c, UVAD_E_STATE, std::string(who) + ": needs both a fbank and a model configuration");
    if (c->fb.snip_edges) return fail(c, UVAD_E_UNSUPPORTED, std::string(who) + ": the centred (snip_edges = 0) framing only");
    if (c->fb.n_mels != c->mc.in_dim) return fail(c, UVAD_E_ARG, std::string(who) + ": n_mels != encoding_dim");
    return UVAD_OK;
}
}  // namespace
}  // extern "C++"

size_t uvad_window_state_bytes(const uvad_ctx *c, int B, int window) {
    if (!c || !c->has_fb || !c->has_model || B <= 0 || window < 1) return 0;
    return window_layout(c, B, window).total;
}

size_t uvad_window_workspace_bytes(const uvad_ctx *c, int B, int chunk, int window) {
    if (!c || !c->has_fb || !c->has_model || B <= 0 || chunk <= 0 || window < 1) return 0;
    return window_ws(c, B, chunk, window).total;
}

int uvad_window_reset(uvad_ctx *c, void *d_state, int B, int window, int lookahead, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || B <= 0) return fail(c, UVAD_E_ARG, "uvad_window_reset: bad argument");
    if (window < 1) return fail(c, UVAD_E_ARG, "uvad_window_reset: window must be >= 1 frame");
    if (lookahead < 0 || lookahead >= window) return fail(c, UVAD_E_ARG, "uvad_window_reset: need 0 <= lookahead < window");
    if (int r = window_check_cfg(c, "uvad_window_reset")) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(d_state, 0, window_layout(c, B, window).total, (hipStream_t)stream));
    WindowGroup g;
    g.B = B; g.W = window; g.L = lookahead;
    c->windows[d_state] = g;
    return UVAD_OK;
}

int uvad_window_step(uvad_ctx *c, const float *d_pcm_chunk, int B, int chunk, void *d_state, float *d_logits, float *d_probs, int ld_out,
                     void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_pcm_chunk || !d_state || (!d_logits && !d_probs) || !ws || B <= 0 || chunk <= 0)
        return fail(c, UVAD_E_ARG, "uvad_window_step: bad argument");
    if (!c->finalized || !c->tables_set) return fail(c, UVAD_E_STATE, "uvad_window_step: context not ready (tables / weights)");
    if (int r = window_check_cfg(c, "uvad_window_step")) return r;
    auto it = c->windows.find(d_state);
    if (it == c->windows.end()) return fail(c, UVAD_E_STATE, "uvad_window_step: call uvad_window_reset on this state first");
    WindowGroup &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, "uvad_window_step: B differs from the one the state was reset with");
    const int L = c->fb.frame_len, sh = c->fb.frame_shift, n_left = (L - sh) / 2, F = c->fb.n_mels;
    const int kmax = stream_max_frames(c, chunk);
    if ((int64_t)g.L + kmax > g.W)
        return fail(c, UVAD_E_ARG, "uvad_window_step: lookahead + chunk / frame_shift + 1 = " + std::to_string(g.L + kmax) + " frames exceeds the window of " +
                                       std::to_string(g.W));
    if (g.sc.n_samples == 0 && chunk < n_left) return fail(c, UVAD_E_ARG, "first chunk must hold at least (frame_len - shift)/2 samples");
    const WindowWs wl = window_ws(c, B, chunk, g.W);
    if (ws_bytes < wl.total) return fail(c, UVAD_E_WORKSPACE, "window workspace too small: need " + std::to_string(wl.total) + " bytes");
    const WindowPlan p = window_plan(c, g, chunk);
    if (p.n_emit > ld_out) return fail(c, UVAD_E_ARG, "uvad_window_step: ld_out smaller than the number of emitted frames");
    const WindowLayout SL = window_layout(c, B, g.W);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    char *st = reinterpret_cast<char *>(d_state);
    char *wsb = reinterpret_cast<char *>(ws);
    float *staging = reinterpret_cast<float *>(wsb);
    const int par = p.fp.parity, k = p.fp.k;
    const float *tail_in = reinterpret_cast<const float *>(st + SL.off_tail[par]);
    float *tail_out = reinterpret_cast<float *>(st + SL.off_tail[par ^ 1]);
    long long *ctr = reinterpret_cast<long long *>(st + SL.off_ctr);
    c->chunks_used = 1;
    if (k <= 0) {   // no frame completes: carry the tail and the frame count over to the other parity
        HIPCHK(c, launch_stream_stage(d_pcm_chunk, B, chunk, L, n_left, p.fp.first, tail_in, tail_out, staging, s));
        HIPCHK(c, launch_window_carry(ctr + par, ctr + (par ^ 1), s));
        window_advance(g, p);
        return 0;
    }
    // the k new frames, computed once
    float *newf = reinterpret_cast<float *>(wsb + wl.off_new);
    FbankArgs fa = stream_fbank_args(c, d_pcm_chunk, B, chunk, p.fp, staging, tail_in, tail_out);
    fa.feats = newf;
    HIPCHK(c, launch_fbank(fa, s));
    // the window into the first projection's operand, as uvad_forward's feature kernel writes it
    char *cws = wsb + wl.off_cls;
    const WsLayout w = carve(c, B, p.Tw);
    const bool planes = f16_planes(c);
    float *feats = reinterpret_cast<float *>(cws + w.off_feats);
    WindowArgs a{};
    a.newf = newf; a.ring = reinterpret_cast<float *>(st + SL.off_ring); a.ctr_in = ctr + par; a.ctr_out = ctr + (par ^ 1);
    a.B = B; a.R = g.W; a.F = F; a.k = k; a.Tw = p.Tw;
    a.planes = planes; a.Fp = w.Fp; a.tiles = w.tiles;
    a.xh = reinterpret_cast<unsigned short *>(cws + w.off_fplanes); a.xl = a.xh + plane_rows(w.M) * (size_t)w.Fp;
    a.out = feats;
    HIPCHK(c, launch_window_assemble(a, s));
    window_advance(g, p);
    if (p.n_emit <= 0) return 0;
    float *lg = reinterpret_cast<float *>(wsb + wl.off_logits), *pr = reinterpret_cast<float *>(wsb + wl.off_probs);
    // the classifier at (B, Tw), time chunks off: a new T every warm-up step would churn the chunk-plan cache, whose eviction synchronises
    ClassifyCall rq = classify_call(feats, B, p.Tw, d_logits ? lg : nullptr, d_probs ? pr : nullptr, cws, wl.total - wl.off_cls, s);
    rq.timed = false; rq.time_chunks_allowed = false; rq.record_start = false; rq.check_range = false; rq.feats_in_planes = planes;
    if (int r = classify_impl(c, rq)) return r;
    HIPCHK(c, launch_window_emit(lg, pr, B, p.Tw, p.r0, p.n_emit, d_logits, d_probs, ld_out, s));
    return p.n_emit;
}

int uvad_window_peek(const uvad_ctx *c, const void *d_state, int chunk, int *k, int64_t *replay_key) {
    if (!c || !d_state || chunk <= 0 || !k || !replay_key) return UVAD_E_ARG;
    auto it = c->windows.find(const_cast<void *>(d_state));
    if (it == c->windows.end() || !c->has_fb) return UVAD_E_STATE;
    const WindowPlan p = window_plan(c, it->second, chunk);
    *k = p.n_emit;
    *replay_key = p.key;
    return UVAD_OK;
}

int uvad_window_advance(uvad_ctx *c, void *d_state, int chunk) {
    if (!c || !d_state || chunk <= 0) return UVAD_E_ARG;
    auto it = c->windows.find(d_state);
    if (it == c->windows.end() || !c->has_fb) return fail(c, UVAD_E_STATE, "uvad_window_advance: call uvad_window_reset on this state first");
    const WindowPlan p = window_plan(c, it->second, chunk);
    window_advance(it->second, p);
    return p.n_emit;
}

int uvad_window_features(uvad_ctx *c, const void *d_state, int B, float *d_feats, int *Tw, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !Tw || B <= 0) return fail(c, UVAD_E_ARG, "uvad_window_features: bad argument");
    auto it = c->windows.find(const_cast<void *>(d_state));
    if (it == c->windows.end()) return fail(c, UVAD_E_STATE, "uvad_window_features: call uvad_window_reset on this state first");
    const WindowGroup &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, "uvad_window_features: B differs from the one the state was reset with");
    *Tw = (int)std::min<int64_t>(g.sc.n_frames, g.W);
    if (!d_feats || *Tw == 0) return UVAD_OK;
    const WindowLayout SL = window_layout(c, B, g.W);
    const char *st = reinterpret_cast<const char *>(d_state);
    HIPCHK(c, hipSetDevice(c->device));
    WindowArgs a{};
    a.ring = reinterpret_cast<float *>(const_cast<char *>(st) + SL.off_ring);
    a.ctr_in = reinterpret_cast<const long long *>(st + SL.off_ctr) + (g.sc.n_steps & 1);
    a.B = B; a.R = g.W; a.F = c->fb.n_mels; a.k = 0; a.Tw = *Tw; a.out = d_feats;
    HIPCHK(c, launch_window_assemble(a, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- windowed streaming of the waveform model (PyanNet) ------------------------------------------------------------------------
// state layout (bytes, 256-aligned blocks): ring [B][R + J W] samples in the state's type (f32 / int16) | feats [B][W][c3] f32 (the SincNet
// output of the window the model last ran on) | ctr[2] int64 (samples received: the step's assembly kernel reads ctr[0] and writes
// ctr[1], a one-thread carry right behind it copies ctr[1] to ctr[0]: every step reads the same slot, so the replay key needs no parity)
// workspace: window [B][Sw_max] samples (sized for f32) | logits, probs [B][W] | classifier workspace of (B, W) | SincNet workspace of
//            (B, Sw_max) (carve() and sinc_carve() grow with T and S, so they hold every warm-up window too)
extern "C++" {
namespace {
struct WavGeom { int64_t J = 0, R = 0; };
// J = 27 stride (three MaxPool1d(3) after the strided first stage); R = the shortest input of one frame, restated from the floor chain
// of sinc_carve: Lpool3 >= f  <=>  S >= stride (3 (3 (3 f + k3 - 1) + k2 - 1) - 1) + kernel_size = J f + R - J
WavGeom wav_geom(const uvad_ctx *c) {
    const uvad_sincnet_cfg &q = c->sc;
    WavGeom g;
    g.J = 27LL * q.stride;
    g.R = (int64_t)q.kernel_size + (int64_t)q.stride * (9LL * q.k3 + 3LL * q.k2 + 14);
    return g;
}
int64_t wav_frames(const WavGeom &g, int64_t S) { return S < g.R ? 0 : (S - g.R) / g.J + 1; }
int64_t wav_span(const WavGeom &g, int64_t Tw) { return Tw > 0 ? g.R + g.J * (Tw - 1) : 0; }
int wav_kmax(const WavGeom &g, int chunk) { return (int)((chunk + g.J - 1) / g.J); }
// n - start < Sw + J for every window (it ends at J (e - 1) + R <= n, less than J before n), and a chunk is at most J (W - L) < Sw_max + J
// samples: a ring of Sw_max + J slots keeps every sample a later window reads, and one launch never writes a slot it reads
int64_t wav_ring_len(const WavGeom &g, int W) { return wav_span(g, W) + g.J; }
struct WavWindowLayout { size_t off_ring = 0, off_feats = 0, off_ctr = 0, total = 0; int64_t ring_len = 0; };
WavWindowLayout wav_window_layout(const uvad_ctx *c, int B, int W, int is_i16) {
    WavWindowLayout L;
    L.ring_len = wav_ring_len(wav_geom(c), W);
    size_t o = 0;
    L.off_ring = o; o += align_up((size_t)B * (size_t)L.ring_len * (is_i16 ? sizeof(int16_t) : sizeof(float)));
    L.off_feats = o; o += align_up((size_t)B * W * c->sc.c3 * sizeof(float));
    L.off_ctr = o; o += align_up(2 * sizeof(long long));
    L.total = o;
    return L;
}
struct WavWindowWs { size_t off_logits = 0, off_probs = 0, off_cls = 0, cls_bytes = 0, off_sinc = 0, sinc_bytes = 0, total = 0; };
WavWindowWs wav_window_ws(const uvad_ctx *c, int B, int W) {
    WavWindowWs w;
    const int64_t sw = wav_span(wav_geom(c), W);
    size_t o = align_up((size_t)B * (size_t)sw * sizeof(float));
    w.off_logits = o; o += align_up((size_t)B * W * sizeof(float));
    w.off_probs = o; o += align_up((size_t)B * W * sizeof(float));
    w.off_cls = o; w.cls_bytes = carve(c, B, W).total; o += w.cls_bytes;
    w.off_sinc = o; w.sinc_bytes = sinc_carve(c, B, sw).total; o += w.sinc_bytes;
    w.total = o;
    return w;
}
// What the next step of a waveform window group does: k new frames, the window [e - Tw, e) of Sw samples the model runs on and the rows
// [r0, r0 + n_emit) of it that it emits (frames [max(0, e_prev - L), max(0, e - L))).  Once the window is full, Tw = W, Sw, r0 = W - L - k
// and n_emit = k follow from k, and the ring position from the device counter: replay key k.
struct WavWindowPlan { int64_t n = 0, e = 0, Sw = 0; int k = 0, Tw = 0, r0 = 0, n_emit = 0; int64_t key = -1; };
WavWindowPlan wav_window_plan(const uvad_ctx *c, const WavWindowGroup &g, int chunk) {
    const WavGeom geo = wav_geom(c);
    WavWindowPlan p;
    p.n = g.sc.n_samples + chunk;
    p.e = wav_frames(geo, p.n);
    p.k = (int)(p.e - g.sc.n_frames);
    p.Tw = (int)std::min<int64_t>(p.e, g.W);
    p.Sw = wav_span(geo, p.Tw);
    const int64_t f0 = std::max<int64_t>(0, g.sc.n_frames - g.L), f1 = std::max<int64_t>(0, p.e - g.L);
    p.n_emit = (int)(f1 - f0);
    p.r0 = (int)(f0 - (p.e - p.Tw));
    if (p.e >= g.W && g.sc.n_frames >= g.L) p.key = p.k;
    return p;
}
void wav_window_advance(WavWindowGroup &g, const WavWindowPlan &p) {
    g.sc.n_samples = p.n;
    g.sc.n_frames = p.e;
    g.sc.n_steps += 1;
}
int wav_window_check_cfg(uvad_ctx *c, const std::string &who) {
    if (!c->has_model || !c->has_sinc)
        return fail(c, UVAD_E_STATE, who + ": needs a model and a SincNet configuration (uvad_sincnet_configure)");
    if (!sinc_weights_ready(c)) return fail(c, UVAD_E_STATE, who + ": SincNet tensors not set / uvad_finalize not called");
    return UVAD_OK;
}
}  // namespace
}  // extern "C++"

size_t uvad_window_wav_state_bytes(const uvad_ctx *c, int B, int window, int is_i16) {
    if (!c || !c->has_model || !c->has_sinc || B <= 0 || window < 1 || (is_i16 != 0 && is_i16 != 1)) return 0;
    return wav_window_layout(c, B, window, is_i16).total;
}

size_t uvad_window_wav_workspace_bytes(const uvad_ctx *c, int B, int chunk, int window) {
    if (!c || !c->has_model || !c->has_sinc || B <= 0 || chunk <= 0 || window < 1) return 0;
    return wav_window_ws(c, B, window).total;
}

int uvad_window_wav_reset(uvad_ctx *c, void *d_state, int B, int window, int lookahead, int is_i16, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || B <= 0 || B > 65535 || (is_i16 != 0 && is_i16 != 1)) return fail(c, UVAD_E_ARG, "uvad_window_wav_reset: bad argument");
    if (window < 1) return fail(c, UVAD_E_ARG, "uvad_window_wav_reset: window must be >= 1 frame");
    if (lookahead < 0 || lookahead >= window) return fail(c, UVAD_E_ARG, "uvad_window_wav_reset: need 0 <= lookahead < window");
    if (int r = wav_window_check_cfg(c, "uvad_window_wav_reset")) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(d_state, 0, wav_window_layout(c, B, window, is_i16).total, (hipStream_t)stream));
    WavWindowGroup g;
    g.B = B; g.W = window; g.L = lookahead; g.is_i16 = is_i16;
    c->wav_windows[d_state] = g;
    return UVAD_OK;
}

static int window_wav_step_impl(uvad_ctx *c, const void *d_pcm_chunk, int is_i16, int B, int chunk, void *d_state, float *d_logits,
                                float *d_probs, int ld_out, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string who = is_i16 ? "uvad_window_wav_step_i16" : "uvad_window_wav_step";
    if (!d_pcm_chunk || !d_state || (!d_logits && !d_probs) || !ws || B <= 0 || chunk <= 0) return fail(c, UVAD_E_ARG, who + ": bad argument");
    if (int r = wav_window_check_cfg(c, who)) return r;
    auto it = c->wav_windows.find(d_state);
    if (it == c->wav_windows.end()) return fail(c, UVAD_E_STATE, who + ": call uvad_window_wav_reset on this state first");
    WavWindowGroup &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, who + ": B differs from the one the state was reset with");
    if (g.is_i16 != is_i16)
        return fail(c, UVAD_E_ARG, who + (g.is_i16 ? ": the state was reset for int16 samples (uvad_window_wav_step_i16)"
                                                   : ": the state was reset for f32 samples (uvad_window_wav_step)"));
    const WavGeom geo = wav_geom(c);
    const int kmax = wav_kmax(geo, chunk);
    if ((int64_t)g.L + kmax > g.W)
        return fail(c, UVAD_E_ARG, who + ": lookahead + ceil(chunk / J) = " + std::to_string((int64_t)g.L + kmax) + " frames exceeds the window of " +
                                       std::to_string(g.W));
    const WavWindowWs wl = wav_window_ws(c, B, g.W);
    if (ws_bytes < wl.total) return fail(c, UVAD_E_WORKSPACE, who + ": window workspace too small: need " + std::to_string(wl.total) + " bytes");
    const WavWindowPlan p = wav_window_plan(c, g, chunk);
    if (p.n_emit > ld_out) return fail(c, UVAD_E_ARG, who + ": ld_out smaller than the number of emitted frames");
    // the closed form the window arithmetic rests on, against the stage-by-stage floor chain
    if (p.e != uvad_sincnet_num_frames(c, p.n) || (p.Tw > 0 && uvad_sincnet_num_frames(c, p.Sw) != p.Tw))
        return fail(c, UVAD_E_STATE, who + ": internal: frames(S) = (S - R) / J + 1 disagrees with uvad_sincnet_num_frames");
    const WavWindowLayout SL = wav_window_layout(c, B, g.W, is_i16);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    char *st = reinterpret_cast<char *>(d_state);
    char *wsb = reinterpret_cast<char *>(ws);
    long long *ctr = reinterpret_cast<long long *>(st + SL.off_ctr);
    c->chunks_used = 1;
    // the chunk into the ring and, if a frame completes, the window into the workspace (a step without one only commits its samples)
    WavWindowArgs a{};
    a.chunk = d_pcm_chunk; a.ring = st + SL.off_ring; a.ctr_in = ctr; a.ctr_out = ctr + 1;
    a.B = B; a.chunk_len = chunk; a.J = (int)geo.J; a.R = (int)geo.R; a.Tw = p.Tw; a.Sw = (int)p.Sw; a.ring_len = SL.ring_len;
    a.out = p.k > 0 ? wsb : nullptr;
    HIPCHK(c, launch_wav_window_assemble(a, is_i16, s));
    HIPCHK(c, launch_window_carry(ctr + 1, ctr, s));
    wav_window_advance(g, p);
    if (p.k <= 0) return 0;
    // the model on the window's Sw samples as uvad_forward_wav runs a (B, Sw) batch: SincNet into the state (the features tap) ...
    float *feats = reinterpret_cast<float *>(st + SL.off_feats);
    if (int r = sincnet_impl(c, wsb, is_i16, B, p.Sw, feats, wsb + wl.off_sinc, wl.sinc_bytes, s)) return r;
    if (p.n_emit <= 0) return 0;
    // ... and the classifier at (B, Tw) with time chunks off (a new T every warm-up step would churn the chunk-plan cache)
    float *lg = reinterpret_cast<float *>(wsb + wl.off_logits), *pr = reinterpret_cast<float *>(wsb + wl.off_probs);
    ClassifyCall rq = classify_call(feats, B, p.Tw, d_logits ? lg : nullptr, d_probs ? pr : nullptr, wsb + wl.off_cls, wl.cls_bytes, s);
    rq.timed = false; rq.time_chunks_allowed = false; rq.record_start = false;
    if (int r = classify_impl(c, rq)) return r;
    HIPCHK(c, launch_window_emit(lg, pr, B, p.Tw, p.r0, p.n_emit, d_logits, d_probs, ld_out, s));
    return p.n_emit;
}

int uvad_window_wav_step(uvad_ctx *c, const float *d_pcm_chunk, int B, int chunk, void *d_state, float *d_logits, float *d_probs, int ld_out,
                         void *ws, size_t ws_bytes, void *stream) {
    return window_wav_step_impl(c, d_pcm_chunk, 0, B, chunk, d_state, d_logits, d_probs, ld_out, ws, ws_bytes, stream);
}
int uvad_window_wav_step_i16(uvad_ctx *c, const int16_t *d_pcm_chunk, int B, int chunk, void *d_state, float *d_logits, float *d_probs,
                             int ld_out, void *ws, size_t ws_bytes, void *stream) {
    return window_wav_step_impl(c, d_pcm_chunk, 1, B, chunk, d_state, d_logits, d_probs, ld_out, ws, ws_bytes, stream);
}

int uvad_window_wav_peek(const uvad_ctx *c, const void *d_state, int chunk, int *k, int64_t *replay_key) {
    if (!c || !d_state || chunk <= 0 || !k || !replay_key) return UVAD_E_ARG;
    auto it = c->wav_windows.find(const_cast<void *>(d_state));
    if (it == c->wav_windows.end() || !c->has_sinc) return UVAD_E_STATE;
    const WavWindowPlan p = wav_window_plan(c, it->second, chunk);
    *k = p.n_emit;
    *replay_key = p.key;
    return UVAD_OK;
}

int uvad_window_wav_advance(uvad_ctx *c, void *d_state, int chunk) {
    if (!c || !d_state || chunk <= 0) return UVAD_E_ARG;
    auto it = c->wav_windows.find(d_state);
    if (it == c->wav_windows.end() || !c->has_sinc)
        return fail(c, UVAD_E_STATE, "uvad_window_wav_advance: call uvad_window_wav_reset on this state first");
    const WavWindowPlan p = wav_window_plan(c, it->second, chunk);
    wav_window_advance(it->second, p);
    return p.n_emit;
}

int uvad_window_wav_features(uvad_ctx *c, const void *d_state, int B, float *d_feats, int *Tw, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !Tw || B <= 0) return fail(c, UVAD_E_ARG, "uvad_window_wav_features: bad argument");
    if (int r = wav_window_check_cfg(c, "uvad_window_wav_features")) return r;
    auto it = c->wav_windows.find(const_cast<void *>(d_state));
    if (it == c->wav_windows.end()) return fail(c, UVAD_E_STATE, "uvad_window_wav_features: call uvad_window_wav_reset on this state first");
    const WavWindowGroup &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, "uvad_window_wav_features: B differs from the one the state was reset with");
    *Tw = (int)std::min<int64_t>(g.sc.n_frames, g.W);
    if (!d_feats || *Tw == 0) return UVAD_OK;
    const WavWindowLayout SL = wav_window_layout(c, B, g.W, g.is_i16);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(d_feats, reinterpret_cast<const char *>(d_state) + SL.off_feats, (size_t)B * *Tw * c->sc.c3 * sizeof(float),
                             hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- slot pools of both window families -------------------------------------------------------------------------------------------
// Every per-slot quantity lives on the device (window_slots.hip): a step's launch arguments depend on (B, chunk) and the buffers alone.
// counters (both families, 256-aligned blocks): n [B] int64 | e [B] int64 | active [B] int32 | tw_last [B] int32 | step int64
// log-mel state:  tails [2][B][frame_len] f32 | ring [B][W][n_mels] f32 | counters
// log-mel workspace: staging [B][nfr frame_len] | new frames [B][nfr][n_mels] | plan [B] | lens [B] int32 |  (nfr = kmax rounded up to even)
//                    logits, probs [B][W] | classifier workspace of (B, W)
// waveform state: ring [B][R + J W] samples (f32 / int16) | feats [B][W][c3] f32 (the last step's SincNet output) | counters
// waveform workspace: window [B][Sw_max] (sized for f32) | nsamp [B] int64 | plan [B] | logits, probs [B][W] | classifier workspace
//                     of (B, W) | SincNet workspace of (B, Sw_max)
extern "C++" {
namespace {
size_t slot_counter_bytes(int B) {
    return 2 * align_up((size_t)B * sizeof(long long)) + 2 * align_up((size_t)B * sizeof(int)) + align_up(sizeof(long long));
}
SlotCounters slot_counters(char *base, int B) {
    SlotCounters k;
    size_t o = 0;
    k.n = reinterpret_cast<long long *>(base + o); o += align_up((size_t)B * sizeof(long long));
    k.e = reinterpret_cast<long long *>(base + o); o += align_up((size_t)B * sizeof(long long));
    k.active = reinterpret_cast<int *>(base + o); o += align_up((size_t)B * sizeof(int));
    k.tw_last = reinterpret_cast<int *>(base + o); o += align_up((size_t)B * sizeof(int));
    k.step = reinterpret_cast<long long *>(base + o);
    return k;
}
struct SlotsLayout { size_t off_tail[2] = {0, 0}, off_ring = 0, off_ctr = 0, total = 0; };
SlotsLayout slots_layout(const uvad_ctx *c, int B, int W) {
    SlotsLayout L;
    size_t o = 0;
    for (int i = 0; i < 2; ++i) { L.off_tail[i] = o; o += align_up((size_t)B * c->fb.frame_len * sizeof(float)); }
    L.off_ring = o; o += align_up((size_t)B * W * c->fb.n_mels * sizeof(float));
    L.off_ctr = o; o += slot_counter_bytes(B);
    L.total = o;
    return L;
}
// the frames of a staging row: kmax, rounded up to even (the feature kernel transforms frames in pairs)
int slots_frames(const uvad_ctx *c, int chunk) { return (stream_max_frames(c, chunk) + 1) / 2 * 2; }
int slots_row(const uvad_ctx *c, int chunk) { return slots_frames(c, chunk) * c->fb.frame_len; }
struct SlotsWs { size_t off_new = 0, off_plan = 0, off_lens = 0, off_logits = 0, off_probs = 0, off_cls = 0, total = 0; };
SlotsWs slots_ws(const uvad_ctx *c, int B, int chunk, int W) {
    SlotsWs w;
    size_t o = align_up((size_t)B * slots_row(c, chunk) * sizeof(float));
    w.off_new = o; o += align_up((size_t)B * slots_frames(c, chunk) * c->fb.n_mels * sizeof(float));
    w.off_plan = o; o += align_up((size_t)B * sizeof(SlotPlan));
    w.off_lens = o; o += align_up((size_t)B * sizeof(int));
    w.off_logits = o; o += align_up((size_t)B * W * sizeof(float));
    w.off_probs = o; o += align_up((size_t)B * W * sizeof(float));
    w.off_cls = o; o += carve(c, B, W).total;
    w.total = o;
    return w;
}
struct WavSlotsLayout { size_t off_ring = 0, off_feats = 0, off_ctr = 0, total = 0; int64_t ring_len = 0; };
WavSlotsLayout wav_slots_layout(const uvad_ctx *c, int B, int W, int is_i16) {
    WavSlotsLayout L;
    L.ring_len = wav_ring_len(wav_geom(c), W);
    size_t o = 0;
    L.off_ring = o; o += align_up((size_t)B * (size_t)L.ring_len * (is_i16 ? sizeof(int16_t) : sizeof(float)));
    L.off_feats = o; o += align_up((size_t)B * W * c->sc.c3 * sizeof(float));
    L.off_ctr = o; o += slot_counter_bytes(B);
    L.total = o;
    return L;
}
struct WavSlotsWs { size_t off_nsamp = 0, off_plan = 0, off_logits = 0, off_probs = 0, off_cls = 0, cls_bytes = 0, off_sinc = 0, sinc_bytes = 0, total = 0; };
WavSlotsWs wav_slots_ws(const uvad_ctx *c, int B, int W) {
    WavSlotsWs w;
    const int64_t sw = wav_span(wav_geom(c), W);
    size_t o = align_up((size_t)B * (size_t)sw * sizeof(float));
    w.off_nsamp = o; o += align_up((size_t)B * sizeof(int64_t));
    w.off_plan = o; o += align_up((size_t)B * sizeof(SlotPlan));
    w.off_logits = o; o += align_up((size_t)B * W * sizeof(float));
    w.off_probs = o; o += align_up((size_t)B * W * sizeof(float));
    w.off_cls = o; w.cls_bytes = carve(c, B, W).total; o += w.cls_bytes;
    w.off_sinc = o; w.sinc_bytes = sinc_carve(c, B, sw).total; o += w.sinc_bytes;
    w.total = o;
    return w;
}
}  // namespace
}  // extern "C++"

size_t uvad_window_slots_state_bytes(const uvad_ctx *c, int B, int window) {
    if (!c || !c->has_fb || !c->has_model || B <= 0 || window < 1) return 0;
    return slots_layout(c, B, window).total;
}

size_t uvad_window_slots_workspace_bytes(const uvad_ctx *c, int B, int chunk, int window) {
    if (!c || !c->has_fb || !c->has_model || B <= 0 || chunk <= 0 || window < 1) return 0;
    return slots_ws(c, B, chunk, window).total;
}

int uvad_window_slots_reset(uvad_ctx *c, void *d_state, int B, int chunk, int window, int lookahead, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || B <= 0 || B > 65535 || chunk <= 0) return fail(c, UVAD_E_ARG, "uvad_window_slots_reset: bad argument");
    if (window < 1) return fail(c, UVAD_E_ARG, "uvad_window_slots_reset: window must be >= 1 frame");
    if (lookahead < 0 || lookahead >= window) return fail(c, UVAD_E_ARG, "uvad_window_slots_reset: need 0 <= lookahead < window");
    if (int r = window_check_cfg(c, "uvad_window_slots_reset")) return r;
    const int n_left = (c->fb.frame_len - c->fb.frame_shift) / 2, kmax = stream_max_frames(c, chunk);
    if (chunk < n_left)
        return fail(c, UVAD_E_ARG, "uvad_window_slots_reset: every step can be a session's first: chunk must hold at least (frame_len - shift) / 2 = " +
                                       std::to_string(n_left) + " samples");
    if ((int64_t)lookahead + kmax > window)
        return fail(c, UVAD_E_ARG, "uvad_window_slots_reset: lookahead + chunk / frame_shift + 1 = " + std::to_string(lookahead + kmax) +
                                       " frames exceeds the window of " + std::to_string(window));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(d_state, 0, slots_layout(c, B, window).total, (hipStream_t)stream));
    SlotPool g;
    g.B = B; g.chunk = chunk; g.W = window; g.L = lookahead;
    c->slot_pools[d_state] = g;
    return UVAD_OK;
}

int uvad_window_slots_step(uvad_ctx *c, const float *d_pcm_chunk, const uint8_t *d_flags, int B, int chunk, void *d_state, float *d_logits,
                           float *d_probs, int ld_out, int32_t *d_counts, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_pcm_chunk || !d_state || (!d_logits && !d_probs) || !d_counts || !ws || B <= 0 || chunk <= 0)
        return fail(c, UVAD_E_ARG, "uvad_window_slots_step: bad argument");
    if (!c->finalized || !c->tables_set) return fail(c, UVAD_E_STATE, "uvad_window_slots_step: context not ready (tables / weights)");
    if (int r = window_check_cfg(c, "uvad_window_slots_step")) return r;
    auto it = c->slot_pools.find(d_state);
    if (it == c->slot_pools.end()) return fail(c, UVAD_E_STATE, "uvad_window_slots_step: call uvad_window_slots_reset on this state first");
    const SlotPool &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, "uvad_window_slots_step: B differs from the one the state was reset with");
    if (chunk != g.chunk) return fail(c, UVAD_E_ARG, "uvad_window_slots_step: chunk differs from the one the state was reset with");
    const int kmax = stream_max_frames(c, chunk), F = c->fb.n_mels;
    if ((int64_t)ld_out < (int64_t)g.L + kmax)
        return fail(c, UVAD_E_ARG, "uvad_window_slots_step: ld_out must be at least lookahead + chunk / frame_shift + 1 = " + std::to_string(g.L + kmax));
    const SlotsWs wl = slots_ws(c, B, chunk, g.W);
    if (ws_bytes < wl.total) return fail(c, UVAD_E_WORKSPACE, "slot pool workspace too small: need " + std::to_string(wl.total) + " bytes");
    const SlotsLayout SL = slots_layout(c, B, g.W);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    char *st = reinterpret_cast<char *>(d_state);
    char *wsb = reinterpret_cast<char *>(ws);
    const SlotCounters ctr = slot_counters(st + SL.off_ctr, B);
    SlotPlan *plan = reinterpret_cast<SlotPlan *>(wsb + wl.off_plan);
    int *lens = reinterpret_cast<int *>(wsb + wl.off_lens);
    float *staging = reinterpret_cast<float *>(wsb), *newf = reinterpret_cast<float *>(wsb + wl.off_new);
    // 1. flags, plans, aligned staging rows and the next tails
    SlotStageArgs sa{};
    sa.chunk = d_pcm_chunk; sa.flags = d_flags; sa.ctr = ctr; sa.tails = reinterpret_cast<float *>(st + SL.off_tail[0]);
    sa.staging = staging; sa.plan = plan;
    sa.B = B; sa.chunk_len = chunk; sa.frame_len = c->fb.frame_len; sa.shift = c->fb.frame_shift; sa.n_left = (c->fb.frame_len - c->fb.frame_shift) / 2;
    sa.row = slots_row(c, chunk); sa.W = g.W; sa.L = g.L;
    HIPCHK(c, launch_slot_stage(sa, s));
    // 2. the unchanged feature kernel on plain rows of side-by-side frames (frame_shift = frame_len): the staging row's frames, those
    //    at t >= k_b discarded by the assembly
    const int nfr = slots_frames(c, chunk);
    FbankArgs fa = fbank_cfg_args(c);
    fa.pcm = staging; fa.pcm_is_i16 = 0; fa.B = B; fa.S = sa.row; fa.T = nfr; fa.row_stride = sa.row;
    fa.frame_shift = c->fb.frame_len; fa.snip_edges = 1;
    fa.feats = newf;
    HIPCHK(c, launch_fbank(fa, s));
    // 3. ring commit and the left-aligned windows into the first projection's operand; lens = Tw_b
    char *cws = wsb + wl.off_cls;
    const WsLayout w = carve(c, B, g.W);
    const bool planes = f16_planes(c);
    float *feats = reinterpret_cast<float *>(cws + w.off_feats);
    SlotAssembleArgs a{};
    a.plan = plan; a.ctr = ctr; a.newf = newf; a.kmax = nfr; a.ring = reinterpret_cast<float *>(st + SL.off_ring);
    a.B = B; a.W = g.W; a.F = F;
    a.planes = planes; a.Fp = w.Fp; a.tiles = w.tiles;
    a.xh = reinterpret_cast<unsigned short *>(cws + w.off_fplanes); a.xl = a.xh + plane_rows(w.M) * (size_t)w.Fp;
    a.out = feats; a.lens = lens;
    HIPCHK(c, launch_slot_assemble(a, s));
    // 4. the classifier at (B, W) with lens
    float *lg = reinterpret_cast<float *>(wsb + wl.off_logits), *pr = reinterpret_cast<float *>(wsb + wl.off_probs);
    ClassifyCall rq = classify_call(feats, B, g.W, d_logits ? lg : nullptr, d_probs ? pr : nullptr, cws, wl.total - wl.off_cls, s);
    rq.timed = false; rq.time_chunks_allowed = false; rq.record_start = false;
    rq.check_range = false; rq.feats_in_planes = planes; rq.lens = lens;
    if (int r = classify_impl(c, rq)) return r;
    // 5. emission, counts and the counters
    SlotEmitArgs ea{};
    ea.plan = plan; ea.ctr = ctr; ea.logits_in = lg; ea.probs_in = pr; ea.B = B; ea.W = g.W;
    ea.logits = d_logits; ea.probs = d_probs; ea.ld_out = ld_out; ea.counts = d_counts;
    HIPCHK(c, launch_slot_emit(ea, s));
    return UVAD_OK;
}

int uvad_window_slots_features(uvad_ctx *c, const void *d_state, int B, float *d_feats, int32_t *d_tw, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !d_feats || !d_tw || B <= 0) return fail(c, UVAD_E_ARG, "uvad_window_slots_features: bad argument");
    if (int r = window_check_cfg(c, "uvad_window_slots_features")) return r;
    auto it = c->slot_pools.find(const_cast<void *>(d_state));
    if (it == c->slot_pools.end()) return fail(c, UVAD_E_STATE, "uvad_window_slots_features: call uvad_window_slots_reset on this state first");
    const SlotPool &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, "uvad_window_slots_features: B differs from the one the state was reset with");
    const SlotsLayout SL = slots_layout(c, B, g.W);
    char *st = reinterpret_cast<char *>(const_cast<void *>(d_state));
    HIPCHK(c, hipSetDevice(c->device));
    SlotAssembleArgs a{};
    a.ctr = slot_counters(st + SL.off_ctr, B); a.ring = reinterpret_cast<float *>(st + SL.off_ring);
    a.B = B; a.W = g.W; a.F = c->fb.n_mels; a.out = d_feats; a.lens = d_tw;
    HIPCHK(c, launch_slot_assemble(a, (hipStream_t)stream));
    return UVAD_OK;
}

size_t uvad_window_wav_slots_state_bytes(const uvad_ctx *c, int B, int window, int is_i16) {
    if (!c || !c->has_model || !c->has_sinc || B <= 0 || window < 1 || (is_i16 != 0 && is_i16 != 1)) return 0;
    return wav_slots_layout(c, B, window, is_i16).total;
}

size_t uvad_window_wav_slots_workspace_bytes(const uvad_ctx *c, int B, int chunk, int window) {
    if (!c || !c->has_model || !c->has_sinc || B <= 0 || chunk <= 0 || window < 1) return 0;
    return wav_slots_ws(c, B, window).total;
}

int uvad_window_wav_slots_reset(uvad_ctx *c, void *d_state, int B, int chunk, int window, int lookahead, int is_i16, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || B <= 0 || B > 65535 || chunk <= 0 || (is_i16 != 0 && is_i16 != 1))
        return fail(c, UVAD_E_ARG, "uvad_window_wav_slots_reset: bad argument");
    if (window < 1) return fail(c, UVAD_E_ARG, "uvad_window_wav_slots_reset: window must be >= 1 frame");
    if (lookahead < 0 || lookahead >= window) return fail(c, UVAD_E_ARG, "uvad_window_wav_slots_reset: need 0 <= lookahead < window");
    if (int r = wav_window_check_cfg(c, "uvad_window_wav_slots_reset")) return r;
    const WavGeom geo = wav_geom(c);
    const int kmax = wav_kmax(geo, chunk);
    if ((int64_t)lookahead + kmax > window)
        return fail(c, UVAD_E_ARG, "uvad_window_wav_slots_reset: lookahead + ceil(chunk / J) = " + std::to_string((int64_t)lookahead + kmax) +
                                       " frames exceeds the window of " + std::to_string(window));
    const int64_t sw = wav_span(geo, window);
    if (sw > 0x7fffffff - chunk) return fail(c, UVAD_E_UNSUPPORTED, "uvad_window_wav_slots_reset: window too long");
    // the closed form the window arithmetic rests on, against the stage-by-stage floor chain
    if (uvad_sincnet_num_frames(c, sw) != window)
        return fail(c, UVAD_E_STATE, "uvad_window_wav_slots_reset: internal: frames(S) = (S - R) / J + 1 disagrees with uvad_sincnet_num_frames");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(d_state, 0, wav_slots_layout(c, B, window, is_i16).total, (hipStream_t)stream));
    SlotPool g;
    g.B = B; g.chunk = chunk; g.W = window; g.L = lookahead; g.is_i16 = is_i16;
    c->wav_slot_pools[d_state] = g;
    return UVAD_OK;
}

static int window_wav_slots_step_impl(uvad_ctx *c, const void *d_pcm_chunk, int is_i16, const uint8_t *d_flags, int B, int chunk, void *d_state,
                                      float *d_logits, float *d_probs, int ld_out, int32_t *d_counts, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string who = is_i16 ? "uvad_window_wav_slots_step_i16" : "uvad_window_wav_slots_step";
    if (!d_pcm_chunk || !d_state || (!d_logits && !d_probs) || !d_counts || !ws || B <= 0 || chunk <= 0)
        return fail(c, UVAD_E_ARG, who + ": bad argument");
    if (int r = wav_window_check_cfg(c, who)) return r;
    auto it = c->wav_slot_pools.find(d_state);
    if (it == c->wav_slot_pools.end()) return fail(c, UVAD_E_STATE, who + ": call uvad_window_wav_slots_reset on this state first");
    const SlotPool &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, who + ": B differs from the one the state was reset with");
    if (chunk != g.chunk) return fail(c, UVAD_E_ARG, who + ": chunk differs from the one the state was reset with");
    if (g.is_i16 != is_i16)
        return fail(c, UVAD_E_ARG, who + (g.is_i16 ? ": the state was reset for int16 samples (uvad_window_wav_slots_step_i16)"
                                                   : ": the state was reset for f32 samples (uvad_window_wav_slots_step)"));
    const WavGeom geo = wav_geom(c);
    const int kmax = wav_kmax(geo, chunk);
    if ((int64_t)ld_out < (int64_t)g.L + kmax)
        return fail(c, UVAD_E_ARG, who + ": ld_out must be at least lookahead + ceil(chunk / J) = " + std::to_string((int64_t)g.L + kmax));
    const WavSlotsWs wl = wav_slots_ws(c, B, g.W);
    if (ws_bytes < wl.total) return fail(c, UVAD_E_WORKSPACE, who + ": slot pool workspace too small: need " + std::to_string(wl.total) + " bytes");
    const WavSlotsLayout SL = wav_slots_layout(c, B, g.W, is_i16);
    const int64_t sw_max = wav_span(geo, g.W);
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    char *st = reinterpret_cast<char *>(d_state);
    char *wsb = reinterpret_cast<char *>(ws);
    const SlotCounters ctr = slot_counters(st + SL.off_ctr, B);
    SlotPlan *plan = reinterpret_cast<SlotPlan *>(wsb + wl.off_plan);
    int64_t *nsamp = reinterpret_cast<int64_t *>(wsb + wl.off_nsamp);
    // 1. flags, plans, the chunk into the ring and each slot's window left-aligned at S = Sw_max
    WavSlotArgs a{};
    a.chunk = d_pcm_chunk; a.flags = d_flags; a.ctr = ctr; a.ring = st + SL.off_ring; a.ring_len = SL.ring_len;
    a.out = wsb; a.Sw_max = (int)sw_max; a.nsamp = reinterpret_cast<long long *>(nsamp); a.plan = plan;
    a.B = B; a.chunk_len = chunk; a.J = (int)geo.J; a.R = (int)geo.R; a.W = g.W; a.L = g.L;
    HIPCHK(c, launch_wav_slot_assemble(a, is_i16, s));
    // 2. SincNet in its lens form (workgroups walk the valid tiles only) into the state (the features tap) ...
    float *feats = reinterpret_cast<float *>(st + SL.off_feats);
    const int *lens = nullptr;
    if (int r = sincnet_impl(c, wsb, is_i16, B, sw_max, feats, wsb + wl.off_sinc, wl.sinc_bytes, s, nsamp, &lens)) return r;
    // 3. ... the classifier at (B, W) with the rows' frame counts ...
    float *lg = reinterpret_cast<float *>(wsb + wl.off_logits), *pr = reinterpret_cast<float *>(wsb + wl.off_probs);
    ClassifyCall rq = classify_call(feats, B, g.W, d_logits ? lg : nullptr, d_probs ? pr : nullptr, wsb + wl.off_cls, wl.cls_bytes, s);
    rq.timed = false; rq.time_chunks_allowed = false; rq.record_start = false; rq.lens = lens;
    if (int r = classify_impl(c, rq)) return r;
    // 4. ... and emission, counts and the counters
    SlotEmitArgs ea{};
    ea.plan = plan; ea.ctr = ctr; ea.logits_in = lg; ea.probs_in = pr; ea.B = B; ea.W = g.W;
    ea.logits = d_logits; ea.probs = d_probs; ea.ld_out = ld_out; ea.counts = d_counts;
    HIPCHK(c, launch_slot_emit(ea, s));
    return UVAD_OK;
}

int uvad_window_wav_slots_step(uvad_ctx *c, const float *d_pcm_chunk, const uint8_t *d_flags, int B, int chunk, void *d_state, float *d_logits,
                               float *d_probs, int ld_out, int32_t *d_counts, void *ws, size_t ws_bytes, void *stream) {
    return window_wav_slots_step_impl(c, d_pcm_chunk, 0, d_flags, B, chunk, d_state, d_logits, d_probs, ld_out, d_counts, ws, ws_bytes, stream);
}
int uvad_window_wav_slots_step_i16(uvad_ctx *c, const int16_t *d_pcm_chunk, const uint8_t *d_flags, int B, int chunk, void *d_state,
                                   float *d_logits, float *d_probs, int ld_out, int32_t *d_counts, void *ws, size_t ws_bytes, void *stream) {
    return window_wav_slots_step_impl(c, d_pcm_chunk, 1, d_flags, B, chunk, d_state, d_logits, d_probs, ld_out, d_counts, ws, ws_bytes, stream);
}

int uvad_window_wav_slots_features(uvad_ctx *c, const void *d_state, int B, float *d_feats, int32_t *d_tw, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !d_feats || !d_tw || B <= 0) return fail(c, UVAD_E_ARG, "uvad_window_wav_slots_features: bad argument");
    if (int r = wav_window_check_cfg(c, "uvad_window_wav_slots_features")) return r;
    auto it = c->wav_slot_pools.find(const_cast<void *>(d_state));
    if (it == c->wav_slot_pools.end())
        return fail(c, UVAD_E_STATE, "uvad_window_wav_slots_features: call uvad_window_wav_slots_reset on this state first");
    const SlotPool &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, "uvad_window_wav_slots_features: B differs from the one the state was reset with");
    const WavSlotsLayout SL = wav_slots_layout(c, B, g.W, g.is_i16);
    char *st = reinterpret_cast<char *>(const_cast<void *>(d_state));
    const SlotCounters ctr = slot_counters(st + SL.off_ctr, B);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(d_feats, st + SL.off_feats, (size_t)B * g.W * c->sc.c3 * sizeof(float), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    HIPCHK(c, hipMemcpyAsync(d_tw, ctr.tw_last, (size_t)B * sizeof(int32_t), hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- the causal stream's slot pool (lstm_stack.hip, the slot form) ------------------------------------------------------------------
// One launch per step, and nothing of a step on the host: the pool exists where the one-launch step of uvad_stream_step exists (feature
// stage, every layer and the head in lstm_stack_kernel), and reset refuses everything else -- the per-layer paths take one T per launch
// from host counters and stay with the lockstep groups.
// state (256-aligned blocks): tail [B][frame_len] f32 (in place) | h [layers][Bpad][128] | c likewise | n [B] int64 | e [B] int64 |
//                             active [B] int32.  The workspace is not used (a token size keeps the calling convention of the pools).
extern "C++" {
namespace {
struct StreamSlotsLayout { size_t off_tail = 0, off_h = 0, off_c = 0, off_n = 0, off_e = 0, off_active = 0, layer_stride = 0, total = 0; };
StreamSlotsLayout stream_slots_layout(const uvad_ctx *c, int B) {
    StreamSlotsLayout L;
    const size_t Bpad = (size_t)(B + SEQ_TILE - 1) / SEQ_TILE * SEQ_TILE;
    size_t o = 0;
    L.off_tail = o; o += align_up((size_t)B * c->fb.frame_len * sizeof(float));
    L.layer_stride = align_up(Bpad * c->mc.hidden * sizeof(float));
    L.off_h = o; o += L.layer_stride * c->mc.num_layers;
    L.off_c = o; o += L.layer_stride * c->mc.num_layers;
    L.off_n = o; o += align_up((size_t)B * sizeof(long long));
    L.off_e = o; o += align_up((size_t)B * sizeof(long long));
    L.off_active = o; o += align_up((size_t)B * sizeof(int));
    L.total = o;
    return L;
}
constexpr size_t STREAM_SLOTS_WS_BYTES = 256;
int stream_slots_kmax(const uvad_ctx *c, int chunk) { return (chunk + c->fb.frame_shift - 1) / c->fb.frame_shift; }
}  // namespace
}  // extern "C++"

int uvad_stream_slots_kmax(const uvad_ctx *c, int chunk) {
    if (!c || !c->has_fb || chunk <= 0) return UVAD_E_ARG;
    return stream_slots_kmax(c, chunk);
}

size_t uvad_stream_slots_state_bytes(const uvad_ctx *c, int B) {
    if (!c || !c->has_fb || !c->has_model || B <= 0) return 0;
    return stream_slots_layout(c, B).total;
}

size_t uvad_stream_slots_workspace_bytes(const uvad_ctx *c, int B, int chunk) {
    if (!c || !c->has_fb || !c->has_model || B <= 0 || chunk <= 0) return 0;
    return STREAM_SLOTS_WS_BYTES;
}

int uvad_stream_slots_reset(uvad_ctx *c, void *d_state, int B, int chunk, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string who = "uvad_stream_slots_reset: ";
    if (!d_state || B <= 0 || chunk <= 0) return fail(c, UVAD_E_ARG, who + "bad argument");
    if (!c->has_fb || !c->has_model) return fail(c, UVAD_E_STATE, who + "needs both a fbank and a model configuration");
    const uvad_model_cfg &m = c->mc;
    if (m.bidirectional) return fail(c, UVAD_E_UNSUPPORTED, who + "needs a causal model (lstm.bidirectional = False)");
    if (c->fb.snip_edges) return fail(c, UVAD_E_UNSUPPORTED, who + "the centred (snip_edges = 0) framing only");
    if (c->fb.n_mels != m.in_dim) return fail(c, UVAD_E_ARG, who + "n_mels != encoding_dim");
    if (m.hidden != 128 || (m.in_dim != 64 && m.in_dim != 80) || m.num_layers < 1 || m.num_layers > LSTM_STACK_MAX_LAYERS)
        return fail(c, UVAD_E_UNSUPPORTED, who + "the one-launch step needs hidden_size 128, 64 or 80 features and 1 .. " +
                                               std::to_string(LSTM_STACK_MAX_LAYERS) + " layers (got " + std::to_string(m.hidden) + ", " +
                                               std::to_string(m.in_dim) + ", " + std::to_string(m.num_layers) +
                                               "); other models stream in lockstep groups (uvad_stream_step)");
    if (m.lin_layers > LSTM_STACK_MAX_LIN || (m.lin_layers > 0 && m.lin_hidden != 128))
        return fail(c, UVAD_E_UNSUPPORTED, who + "the in-launch head needs at most " + std::to_string(LSTM_STACK_MAX_LIN) +
                                               " feed-forward layers, each 128 -> 128 (got " + std::to_string(m.lin_layers) + " of " +
                                               std::to_string(m.lin_hidden) + " units)");
    const int n_left = (c->fb.frame_len - c->fb.frame_shift) / 2, kmax = stream_slots_kmax(c, chunk);
    if (chunk < n_left)
        return fail(c, UVAD_E_ARG, who + "every step can be a session's first: chunk must hold at least (frame_len - shift) / 2 = " +
                                       std::to_string(n_left) + " samples");
    if (kmax > LSTM_STACK_TMAX)
        return fail(c, UVAD_E_ARG, who + "a step completes up to ceil(chunk / frame_shift) = " + std::to_string(kmax) + " frames, the one-launch step takes " +
                                       std::to_string(LSTM_STACK_TMAX) + ": chunk <= " + std::to_string(LSTM_STACK_TMAX * c->fb.frame_shift) + " samples");
    if (!c->finalized || !c->tables_set) return fail(c, UVAD_E_STATE, who + "context not ready (tables / weights)");
    if (!stream_uses_stack(c, kmax) || !stream_head_in_stack(c))
        return fail(c, UVAD_E_UNSUPPORTED, who + "the weights have no one-launch form (lstm_stack.hip)");
    if (!lstm_stack_slots_lds_bytes(fbank_cfg_args(c), chunk))
        return fail(c, UVAD_E_UNSUPPORTED, who + "the feature stage (4 rows of frame_len + chunk samples, the mel image, the transform scratch) "
                                               "exceeds the 120 KiB of LDS beside the stack");
    if ((int64_t)B * std::max(c->fb.frame_len, 128) * m.num_layers >= ((int64_t)1 << 31))
        return fail(c, UVAD_E_ARG, who + "B too large");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(d_state, 0, stream_slots_layout(c, B).total, (hipStream_t)stream));
    SlotPool g;
    g.B = B; g.chunk = chunk;
    c->stream_slot_pools[d_state] = g;
    return UVAD_OK;
}

int uvad_stream_slots_step(uvad_ctx *c, const float *d_pcm_chunk, const uint8_t *d_flags, int B, int chunk, void *d_state, float *d_logits,
                           float *d_probs, int ld_out, int32_t *d_counts, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string who = "uvad_stream_slots_step: ";
    if (!d_pcm_chunk || !d_state || (!d_logits && !d_probs) || !d_counts || !ws || B <= 0 || chunk <= 0) return fail(c, UVAD_E_ARG, who + "bad argument");
    if (!c->finalized || !c->has_fb || !c->tables_set) return fail(c, UVAD_E_STATE, who + "context not ready (tables / weights)");
    auto it = c->stream_slot_pools.find(d_state);
    if (it == c->stream_slot_pools.end()) return fail(c, UVAD_E_STATE, who + "call uvad_stream_slots_reset on this state first");
    const SlotPool &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_ARG, who + "B differs from the one the state was reset with");
    if (chunk != g.chunk) return fail(c, UVAD_E_ARG, who + "chunk differs from the one the state was reset with");
    const int kmax = stream_slots_kmax(c, chunk);
    if (ld_out < kmax) return fail(c, UVAD_E_ARG, who + "ld_out must be at least ceil(chunk / frame_shift) = " + std::to_string(kmax));
    if (ws_bytes < STREAM_SLOTS_WS_BYTES)
        return fail(c, UVAD_E_WORKSPACE, "stream slot pool workspace too small: need " + std::to_string(STREAM_SLOTS_WS_BYTES) + " bytes");
    // (weights loaded since the reset: the scope is checked again, nothing is enqueued outside it)
    if (c->mc.bidirectional || !stream_uses_stack(c, kmax) || !stream_head_in_stack(c))
        return fail(c, UVAD_E_UNSUPPORTED, who + "the model has no one-launch step");
    const uvad_model_cfg &m = c->mc;
    const PackedWeights &W = *c->packed;
    const StreamSlotsLayout S = stream_slots_layout(c, B);
    char *st = reinterpret_cast<char *>(d_state);
    HIPCHK(c, hipSetDevice(c->device));
    LstmStackSlotsArgs q{};
    LstmStackArgs &a = q.st;
    a.kin0 = m.in_dim; a.n_layers = m.num_layers;
    for (int k = 0; k < m.num_layers; ++k) { a.wih[k] = W.layers[k].w_ih_img; a.whh[k] = W.layers[k].w_hh; a.bias[k] = W.layers[k].bias; }
    a.h = reinterpret_cast<float *>(st + S.off_h); a.c = reinterpret_cast<float *>(st + S.off_c); a.layer_stride = S.layer_stride / sizeof(float);
    a.tiles = (B + SEQ_TILE - 1) / SEQ_TILE; a.B = B;
    for (int j = 0; j < m.lin_layers; ++j) { a.lin_w[j] = W.lin_w_img[j]; a.lin_b[j] = W.lin_b[j]; }
    a.n_lin = m.lin_layers; a.cls_w = W.cls_w; a.cls_b = W.cls_b; a.slope = m.leaky_slope;
    a.logits = d_logits; a.probs = d_probs; a.ld_out = ld_out;
    a.fb = fbank_cfg_args(c); a.fb_on = 1;
    q.chunk = d_pcm_chunk; q.chunk_len = chunk; q.flags = d_flags; q.kmax = kmax;
    q.n = reinterpret_cast<long long *>(st + S.off_n); q.e = reinterpret_cast<long long *>(st + S.off_e);
    q.active = reinterpret_cast<int *>(st + S.off_active);
    q.tail = reinterpret_cast<float *>(st + S.off_tail);
    q.counts = d_counts;
    HIPCHK(c, launch_lstm_stack_slots(q, (hipStream_t)stream));
    c->rec_tile_used = 4;
    return UVAD_OK;
}

// ---- sliding-window inference over whole recordings (sliding.hip) -------------------------------------------------------------------
// log-mel workspace: window probabilities [N][W] | lens [group] | frames [R] | features [R][T][F] (uvad_sliding_forward) | classifier
//                    workspace of (group, W)
// waveform workspace: windows [group][Sw] samples (sized for f32) | nsamp [group] int64 | window probabilities [N][W] | SincNet output
//                     [group][W][c3] | classifier workspace of (group, W) | SincNet workspace of (group, Sw)
extern "C++" {
namespace {
struct SlidingWs { size_t off_win = 0, off_lens = 0, off_frames = 0, off_feats = 0, off_cls = 0, cls_bytes = 0, total = 0; };
SlidingWs sliding_ws(const uvad_ctx *c, int R, int64_t T, int64_t N, int group) {
    SlidingWs w;
    size_t o = 0;
    w.off_win = o; o += align_up((size_t)std::max<int64_t>(N, 1) * c->sl_W * sizeof(float));
    w.off_lens = o; o += align_up((size_t)group * sizeof(int));
    w.off_frames = o; o += align_up((size_t)R * sizeof(int));
    w.off_feats = o; o += align_up((size_t)R * (size_t)T * c->mc.in_dim * sizeof(float));
    w.off_cls = o; w.cls_bytes = carve(c, group, c->sl_W).total; o += w.cls_bytes;
    w.total = o;
    return w;
}
struct SlidingWavWs { size_t off_nsamp = 0, off_win = 0, off_feats = 0, off_cls = 0, cls_bytes = 0, off_sinc = 0, sinc_bytes = 0, total = 0; };
SlidingWavWs sliding_wav_ws(const uvad_ctx *c, int64_t N, int group) {
    SlidingWavWs w;
    const int64_t sw = wav_span(wav_geom(c), c->sl_W);
    size_t o = align_up((size_t)group * (size_t)sw * sizeof(float));
    w.off_nsamp = o; o += align_up((size_t)group * sizeof(int64_t));
    w.off_win = o; o += align_up((size_t)std::max<int64_t>(N, 1) * c->sl_W * sizeof(float));
    w.off_feats = o; o += align_up((size_t)group * c->sl_W * c->sc.c3 * sizeof(float));
    w.off_cls = o; w.cls_bytes = carve(c, group, c->sl_W).total; o += w.cls_bytes;
    w.off_sinc = o; w.sinc_bytes = sinc_carve(c, group, sw).total; o += w.sinc_bytes;
    w.total = o;
    return w;
}
// what every sliding call refuses before it enqueues anything
int sliding_check(uvad_ctx *c, const std::string &who, const void *d_in, int R, int64_t len, const void *d_lens, const int32_t *d_first, int64_t N,
                  int group, const float *d_probs, const void *ws) {
    if (!c->has_sliding) return fail(c, UVAD_E_STATE, who + ": uvad_sliding_configure has not been called");
    if (!d_lens) return fail(c, UVAD_E_ARG, who + ": the per-recording lengths are NULL");
    if (!d_first) return fail(c, UVAD_E_ARG, who + ": d_first is NULL");
    if (group < 1) return fail(c, UVAD_E_ARG, who + ": group must be >= 1");
    if (N < 0 || N > 0x7fffffff) return fail(c, UVAD_E_ARG, who + ": N must be in [0, 2^31)");
    if (!d_in || !d_probs || !ws || R <= 0 || R > 65535 || len <= 0) return fail(c, UVAD_E_ARG, who + ": bad argument");
    return UVAD_OK;
}
// the windows [0, N) in groups of at most `group` through assemble + classifier (log-mel), into win [N][W]
int sliding_run_groups(uvad_ctx *c, const SlidingPlan &plan, const float *feats, bool caller_feats, int group, float *win, int *lens,
                       char *cws, size_t cws_bytes, hipStream_t s) {
    const bool planes = f16_planes(c);
    const int W = c->sl_W;
    for (int64_t i0 = 0; i0 < plan.N; i0 += group) {
        const int Bg = (int)std::min<int64_t>(group, plan.N - i0);
        const WsLayout w = carve(c, Bg, W);
        float *rows = reinterpret_cast<float *>(cws + w.off_feats);
        SlidingAssembleArgs a{};
        a.plan = plan; a.feats = feats; a.i0 = i0; a.Bg = Bg; a.F = c->mc.in_dim;
        a.planes = planes; a.Fp = w.Fp; a.tiles = w.tiles;
        a.xh = reinterpret_cast<unsigned short *>(cws + w.off_fplanes); a.xl = a.xh + plane_rows(w.M) * (size_t)w.Fp;
        a.lens = lens;
        // caller-supplied features can lie outside the f16 range: the f32 rows and the device flag beside the planes, as uvad_classify;
        // the feature kernel's log-mel values cannot (uvad_forward): planes alone
        const bool check_range = planes && caller_feats;
        if (!planes || check_range) a.out = rows;
        if (check_range) {
            a.flag = reinterpret_cast<int *>(cws + w.off_flag);
            HIPCHK(c, launch_zero_counters(reinterpret_cast<unsigned *>(a.flag), 1, s));
        }
        HIPCHK(c, launch_sliding_assemble(a, s));
        ClassifyCall rq = classify_call(rows, Bg, W, nullptr, win + (size_t)i0 * W, cws, cws_bytes, s);
        rq.timed = false; rq.time_chunks_allowed = false; rq.record_start = false;
        rq.check_range = check_range; rq.feats_in_planes = planes; rq.lens = lens;
        if (int r = classify_impl(c, rq)) return r;
    }
    return UVAD_OK;
}
int sliding_finish(uvad_ctx *c, const SlidingPlan &plan, const float *win, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs,
                   hipStream_t s) {
    SlidingAggregateArgs g{};
    g.plan = plan; g.win = win; g.weights = c->sl_w_host.empty() ? nullptr : c->d_sl_w;
    g.out = d_probs; g.ld_out = ld_out; g.frames = d_frames;
    HIPCHK(c, launch_sliding_aggregate(g, s));
    if (d_win_probs && plan.N > 0)
        HIPCHK(c, hipMemcpyAsync(d_win_probs, win, (size_t)plan.N * plan.W * sizeof(float), hipMemcpyDeviceToDevice, s));
    c->chunks_used = 1;
    return UVAD_OK;
}
int sliding_logmel_cfg(uvad_ctx *c, const std::string &who, bool from_pcm) {
    if (!c->has_model) return fail(c, UVAD_E_STATE, who + ": needs a model configuration");
    if (!c->finalized) return fail(c, UVAD_E_STATE, who + ": uvad_finalize has not been called");
    if (from_pcm) {
        if (!c->has_fb || !c->tables_set) return fail(c, UVAD_E_STATE, who + ": uvad_set_tables has not been called");
        if (c->fb.n_mels != c->mc.in_dim) return fail(c, UVAD_E_ARG, who + ": n_mels != encoding_dim");
    }
    return UVAD_OK;
}
}  // namespace
}  // extern "C++"

int uvad_sliding_configure(uvad_ctx *c, int window, int hop, const float *h_weights) {
    if (!c) return UVAD_E_ARG;
    if (window < 1) return fail(c, UVAD_E_ARG, "uvad_sliding_configure: window must be >= 1 frame");
    if (hop < 1 || hop > window) return fail(c, UVAD_E_ARG, "uvad_sliding_configure: need 1 <= hop <= window");
    for (int i = 0; h_weights && i < window; ++i)
        if (!std::isfinite(h_weights[i]) || !(h_weights[i] > 0.0f))
            return fail(c, UVAD_E_ARG, "uvad_sliding_configure: every weight must be finite and > 0 (weight " + std::to_string(i) + ")");
    if (h_weights) {
        HIPCHK(c, hipSetDevice(c->device));
        const bool same = c->has_sliding && c->sl_w_host.size() == (size_t)window &&
                          std::memcmp(c->sl_w_host.data(), h_weights, (size_t)window * sizeof(float)) == 0;
        if (!same) {
            if (c->sl_w_cap < window) {   // a larger table: a new buffer (the old one lives with the context: captured graphs may name it)
                void *p = nullptr;
                HIPCHK(c, hipMalloc(&p, (size_t)window * sizeof(float)));
                c->allocs.push_back(p);
                c->d_sl_w = reinterpret_cast<float *>(p);
                c->sl_w_cap = window;
            } else {
                HIPCHK(c, hipDeviceSynchronize());   // kernels of earlier calls may still be reading the table
            }
            HIPCHK(c, hipMemcpy(c->d_sl_w, h_weights, (size_t)window * sizeof(float), hipMemcpyHostToDevice));
            c->sl_w_host.assign(h_weights, h_weights + window);
        }
    } else {
        c->sl_w_host.clear();
    }
    c->sl_W = window; c->sl_Hf = hop;
    c->has_sliding = true;
    return UVAD_OK;
}

int64_t uvad_sliding_count(int64_t frames, int window, int hop) {
    if (frames < 0 || window < 1 || hop < 1 || hop > window) return UVAD_E_ARG;
    if (frames == 0) return 0;
    if (frames <= window) return 1;
    return (frames - window + hop - 1) / hop + 1;
}

size_t uvad_sliding_workspace_bytes(const uvad_ctx *c, int R, int64_t T, int64_t N, int group) {
    if (!c || !c->has_model || !c->has_sliding || R <= 0 || T <= 0 || N < 0 || group < 1) return 0;
    return sliding_ws(c, R, T, N, group).total;
}

size_t uvad_sliding_wav_workspace_bytes(const uvad_ctx *c, int R, int64_t S, int64_t N, int group) {
    if (!c || !c->has_model || !c->has_sinc || !c->has_sliding || R <= 0 || S <= 0 || N < 0 || group < 1) return 0;
    return sliding_wav_ws(c, N, group).total;
}

int uvad_sliding_classify(uvad_ctx *c, const float *d_feats, int R, int T, const int32_t *d_lens, const int32_t *d_first, int64_t N, int group,
                          float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string who = "uvad_sliding_classify";
    if (int r = sliding_check(c, who, d_feats, R, T, d_lens, d_first, N, group, d_probs, ws)) return r;
    if (int r = sliding_logmel_cfg(c, who, false)) return r;
    if (ld_out < T) return fail(c, UVAD_E_ARG, who + ": ld_out must be at least T");
    const SlidingWs wl = sliding_ws(c, R, T, N, group);
    if (ws_bytes < wl.total) return fail(c, UVAD_E_WORKSPACE, who + ": workspace too small: need " + std::to_string(wl.total) + " bytes");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    char *wsb = reinterpret_cast<char *>(ws);
    SlidingPlan plan{};
    plan.first = d_first; plan.nrec = R; plan.N = N; plan.W = c->sl_W; plan.Hf = c->sl_Hf; plan.lens = d_lens; plan.T = T;
    float *win = reinterpret_cast<float *>(wsb + wl.off_win);
    if (int r = sliding_run_groups(c, plan, d_feats, true, group, win, reinterpret_cast<int *>(wsb + wl.off_lens), wsb + wl.off_cls, wl.cls_bytes, s))
        return r;
    return sliding_finish(c, plan, win, d_probs, ld_out, d_frames, d_win_probs, s);
}

static int sliding_forward_impl(uvad_ctx *c, const void *d_pcm, int is_i16, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first,
                                int64_t N, int group, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *ws,
                                size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string who = is_i16 ? "uvad_sliding_forward_i16" : "uvad_sliding_forward";
    if (int r = sliding_check(c, who, d_pcm, R, S, d_nsamp, d_first, N, group, d_probs, ws)) return r;
    if (int r = sliding_logmel_cfg(c, who, true)) return r;
    const int64_t T = uvad_num_frames(c, S);
    if (T <= 0 || T > 0x7fffffff) return fail(c, UVAD_E_ARG, who + ": bad frame count");
    if (ld_out < T) return fail(c, UVAD_E_ARG, who + ": ld_out must be at least uvad_num_frames(S) = " + std::to_string(T));
    const SlidingWs wl = sliding_ws(c, R, T, N, group);
    if (ws_bytes < wl.total) return fail(c, UVAD_E_WORKSPACE, who + ": workspace too small: need " + std::to_string(wl.total) + " bytes");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    char *wsb = reinterpret_cast<char *>(ws);
    // the recordings' continuous feature rows, once, by the unchanged feature kernel in its lens form (right-edge reflection at S_r)
    float *feats = reinterpret_cast<float *>(wsb + wl.off_feats);
    if (int r = fbank_impl(c, d_pcm, is_i16, R, S, feats, stream, nullptr, nullptr, 0, d_nsamp)) return r;
    int *frames = reinterpret_cast<int *>(wsb + wl.off_frames);
    HIPCHK(c, launch_frames_of(d_nsamp, R, S, c->fb.frame_len, c->fb.frame_shift, c->fb.snip_edges, frames, s));
    SlidingPlan plan{};
    plan.first = d_first; plan.nrec = R; plan.N = N; plan.W = c->sl_W; plan.Hf = c->sl_Hf; plan.lens = frames; plan.T = (int)T;
    float *win = reinterpret_cast<float *>(wsb + wl.off_win);
    if (int r = sliding_run_groups(c, plan, feats, false, group, win, reinterpret_cast<int *>(wsb + wl.off_lens), wsb + wl.off_cls, wl.cls_bytes, s))
        return r;
    return sliding_finish(c, plan, win, d_probs, ld_out, d_frames, d_win_probs, s);
}

int uvad_sliding_forward(uvad_ctx *c, const float *d_pcm, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first, int64_t N, int group,
                         float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *ws, size_t ws_bytes, void *stream) {
    return sliding_forward_impl(c, d_pcm, 0, R, S, d_nsamp, d_first, N, group, d_probs, ld_out, d_frames, d_win_probs, ws, ws_bytes, stream);
}
int uvad_sliding_forward_i16(uvad_ctx *c, const int16_t *d_pcm, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first, int64_t N,
                             int group, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *ws, size_t ws_bytes,
                             void *stream) {
    return sliding_forward_impl(c, d_pcm, 1, R, S, d_nsamp, d_first, N, group, d_probs, ld_out, d_frames, d_win_probs, ws, ws_bytes, stream);
}

static int sliding_forward_wav_impl(uvad_ctx *c, const void *d_wav, int is_i16, int R, int64_t S, const int64_t *d_nsamp,
                                    const int32_t *d_first, int64_t N, int group, float *d_probs, int ld_out, int32_t *d_frames,
                                    float *d_win_probs, void *ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string who = is_i16 ? "uvad_sliding_forward_wav_i16" : "uvad_sliding_forward_wav";
    if (int r = sliding_check(c, who, d_wav, R, S, d_nsamp, d_first, N, group, d_probs, ws)) return r;
    if (int r = wav_window_check_cfg(c, who)) return r;
    const WavGeom geo = wav_geom(c);
    const int W = c->sl_W;
    const int64_t sw = wav_span(geo, W);
    if (sw > 0x7fffffff || geo.J * (int64_t)c->sl_Hf > 0x7fffffff) return fail(c, UVAD_E_UNSUPPORTED, who + ": window too long");
    // the closed form the window arithmetic rests on (one constant stride J, receptive field R), against the stage-by-stage floor chain
    if (uvad_sincnet_num_frames(c, sw) != W || uvad_sincnet_num_frames(c, sw + geo.J) != W + 1 || uvad_sincnet_num_frames(c, sw - 1) != W - 1)
        return fail(c, UVAD_E_UNSUPPORTED, who + ": the SincNet geometry has no single frame step: frames(S) = (S - R) / J + 1 does not hold");
    const int64_t T = uvad_sincnet_num_frames(c, S);
    if (T <= 0 || T > 0x7fffffff) return fail(c, UVAD_E_ARG, who + ": rows too short for one output frame");
    if (ld_out < T) return fail(c, UVAD_E_ARG, who + ": ld_out must be at least uvad_sincnet_num_frames(S) = " + std::to_string(T));
    const SlidingWavWs wl = sliding_wav_ws(c, N, group);
    if (ws_bytes < wl.total) return fail(c, UVAD_E_WORKSPACE, who + ": workspace too small: need " + std::to_string(wl.total) + " bytes");
    hipStream_t s = (hipStream_t)stream;
    HIPCHK(c, hipSetDevice(c->device));
    char *wsb = reinterpret_cast<char *>(ws);
    SlidingPlan plan{};
    plan.first = d_first; plan.nrec = R; plan.N = N; plan.W = W; plan.Hf = c->sl_Hf; plan.T = (int)T;
    plan.nsamp = reinterpret_cast<const long long *>(d_nsamp); plan.S = S; plan.J = (int)geo.J; plan.R0 = (int)geo.R;
    float *win = reinterpret_cast<float *>(wsb + wl.off_win);
    float *feats = reinterpret_cast<float *>(wsb + wl.off_feats);
    int64_t *nsamp = reinterpret_cast<int64_t *>(wsb + wl.off_nsamp);
    for (int64_t i0 = 0; i0 < N; i0 += group) {
        const int Bg = (int)std::min<int64_t>(group, N - i0);
        // 1. the group's PCM windows left-aligned at S = Sw, 2. SincNet in its lens form (every norm over the window's own samples),
        // 3. the classifier at (Bg, W) with the windows' frame counts
        SlidingWavArgs a{};
        a.plan = plan; a.pcm = d_wav; a.i0 = i0; a.Bg = Bg; a.Sw = sw; a.out = wsb; a.nsamp_out = reinterpret_cast<long long *>(nsamp);
        HIPCHK(c, launch_sliding_wav_gather(a, is_i16, s));
        const int *lens = nullptr;
        if (int r = sincnet_impl(c, wsb, is_i16, Bg, sw, feats, wsb + wl.off_sinc, wl.sinc_bytes, s, nsamp, &lens)) return r;
        ClassifyCall rq = classify_call(feats, Bg, W, nullptr, win + (size_t)i0 * W, wsb + wl.off_cls, wl.cls_bytes, s);
        rq.timed = false; rq.time_chunks_allowed = false; rq.record_start = false; rq.lens = lens;
        if (int r = classify_impl(c, rq)) return r;
    }
    return sliding_finish(c, plan, win, d_probs, ld_out, d_frames, d_win_probs, s);
}

int uvad_sliding_forward_wav(uvad_ctx *c, const float *d_wav, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first, int64_t N,
                             int group, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *ws, size_t ws_bytes,
                             void *stream) {
    return sliding_forward_wav_impl(c, d_wav, 0, R, S, d_nsamp, d_first, N, group, d_probs, ld_out, d_frames, d_win_probs, ws, ws_bytes, stream);
}
int uvad_sliding_forward_wav_i16(uvad_ctx *c, const int16_t *d_wav, int R, int64_t S, const int64_t *d_nsamp, const int32_t *d_first, int64_t N,
                                 int group, float *d_probs, int ld_out, int32_t *d_frames, float *d_win_probs, void *ws, size_t ws_bytes,
                                 void *stream) {
    return sliding_forward_wav_impl(c, d_wav, 1, R, S, d_nsamp, d_first, N, group, d_probs, ld_out, d_frames, d_win_probs, ws, ws_bytes, stream);
}

// ---- ingest stage (ingest.hip) ---------------------------------------------------------------------------------------------------
extern "C++" {
namespace {
struct IngestGeom { int up, down, width, K, Dj, H; };
IngestGeom ingest_geom(const uvad_ctx *c) {
    IngestGeom g{};
    g.up = c->ig_up; g.down = c->ig_down; g.width = c->ig_width;
    g.K = 2 * g.width + g.down;
    g.Dj = (g.width + g.down - 1 + g.down - 1) / g.down;   // ceil((width + down - 1) / down) output groups of delay
    g.H = g.Dj * g.down + g.width;
    return g;
}
bool ingest_identity(const uvad_ctx *c) { return c->ig_up == 1 && c->ig_down == 1; }
// configured, and a table where the ratio needs one
int ingest_check(uvad_ctx *c, const char *who) {
    if (!c->has_ingest) return fail(c, UVAD_E_STATE, std::string(who) + ": call uvad_ingest_configure first");
    if (!ingest_identity(c) && !c->ig_taps)
        return fail(c, UVAD_E_STATE, std::string(who) + ": no resampler taps for " + std::to_string(c->ig_up) + " / " + std::to_string(c->ig_down) +
                                         " (uvad_ingest_set_taps)");
    return UVAD_OK;
}
struct IngestState { size_t off_seen = 0, total = 0; };
IngestState ingest_state(const uvad_ctx *c, int B) {
    IngestState s;
    const size_t rows = (size_t)B * c->ig.channels;
    s.off_seen = align_up(rows * (size_t)ingest_geom(c).H * sizeof(float));
    s.total = s.off_seen + align_up(rows * sizeof(long long));
    return s;
}
IngestArgs ingest_args(const uvad_ctx *c, const void *d_in, int B, int64_t S_in, float *d_out) {
    const IngestGeom g = ingest_geom(c);
    IngestArgs a{};
    a.in = d_in; a.enc = c->ig.encoding; a.C = c->ig.channels; a.S_in = S_in;
    a.taps = ingest_identity(c) ? nullptr : c->d_ig_taps;
    a.up = g.up; a.down = g.down; a.width = g.width; a.K = g.K;
    a.out = d_out; a.S_out = (S_in * g.up + g.down - 1) / g.down;
    a.B = B;
    return a;
}
}  // namespace
}  // extern "C++"

int uvad_ingest_configure(uvad_ctx *c, const uvad_ingest_cfg *q) {
    if (!c) return UVAD_E_ARG;
    if (!q) return fail(c, UVAD_E_ARG, "uvad_ingest_configure: bad argument");
    if (q->encoding < UVAD_INGEST_F32 || q->encoding > UVAD_INGEST_ALAW)
        return fail(c, UVAD_E_ARG, "uvad_ingest_configure: encoding must be UVAD_INGEST_F32, _I16, _ULAW or _ALAW");
    if (q->channels < 1) return fail(c, UVAD_E_ARG, "uvad_ingest_configure: channels must be >= 1");
    if (q->channels > INGEST_MAX_CHANNELS)
        return fail(c, UVAD_E_UNSUPPORTED, "uvad_ingest_configure: at most " + std::to_string(INGEST_MAX_CHANNELS) + " interleaved channels");
    if (q->sample_rate < 1 || q->sample_rate > 16000 * 4096) return fail(c, UVAD_E_ARG, "uvad_ingest_configure: bad sample_rate");
    int a = 16000, b = q->sample_rate;
    while (b) { const int t = a % b; a = b; b = t; }
    const int up = 16000 / a, down = q->sample_rate / a;
    if (!c->has_ingest || up != c->ig_up || down != c->ig_down) {   // a table for another ratio is dropped
        c->ig_taps = false;
        c->ig_width = 0;
    }
    c->ig = *q; c->ig_up = up; c->ig_down = down;
    c->has_ingest = true;
    return UVAD_OK;
}

int uvad_ingest_set_taps(uvad_ctx *c, const float *taps, int up, int down, int width) {
    if (!c) return UVAD_E_ARG;
    if (!c->has_ingest) return fail(c, UVAD_E_STATE, "uvad_ingest_set_taps: call uvad_ingest_configure first");
    if (!taps || up < 1 || down < 1 || width < 0) return fail(c, UVAD_E_ARG, "uvad_ingest_set_taps: bad argument");
    if (up != c->ig_up || down != c->ig_down)
        return fail(c, UVAD_E_ARG, "uvad_ingest_set_taps: the table is for " + std::to_string(up) + " / " + std::to_string(down) +
                                       ", the configured rate needs " + std::to_string(c->ig_up) + " / " + std::to_string(c->ig_down));
    const long long K = 2LL * width + down;
    if (up > UVAD_INGEST_MAX_PHASES || K > UVAD_INGEST_MAX_TAPS)
        return fail(c, UVAD_E_UNSUPPORTED, "uvad_ingest_set_taps: a table of " + std::to_string(up) + " phases x " + std::to_string(K) +
                                               " taps exceeds the limit of " + std::to_string(UVAD_INGEST_MAX_PHASES) + " phases x " +
                                               std::to_string(UVAD_INGEST_MAX_TAPS) + " taps per phase");
    if (up == 1 && down == 1) return fail(c, UVAD_E_ARG, "uvad_ingest_set_taps: 1 / 1 takes no table (a pure decode / de-interleave)");
    for (long long i = 0; i < up * K; ++i)
        if (!std::isfinite(taps[i])) return fail(c, UVAD_E_ARG, "uvad_ingest_set_taps: taps must be finite");
    // the table the device already holds: nothing to upload, nothing to wait for
    if (c->ig_taps && c->ig_width == width && c->ig_taps_host.size() == (size_t)(up * K) &&
        std::memcmp(c->ig_taps_host.data(), taps, (size_t)(up * K) * sizeof(float)) == 0)
        return UVAD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_ig_taps) {
        void *p = nullptr;
        HIPCHK(c, hipMalloc(&p, (size_t)UVAD_INGEST_MAX_PHASES * UVAD_INGEST_MAX_TAPS * sizeof(float)));
        c->allocs.push_back(p);
        c->d_ig_taps = reinterpret_cast<float *>(p);
    } else {
        HIPCHK(c, hipDeviceSynchronize());   // kernels of earlier calls may still be reading the table
    }
    c->ig_taps = false;
    HIPCHK(c, hipMemcpy(c->d_ig_taps, taps, (size_t)(up * K) * sizeof(float), hipMemcpyHostToDevice));
    c->ig_taps_host.assign(taps, taps + up * K);
    c->ig_width = width;
    c->ig_taps = true;
    return UVAD_OK;
}

int64_t uvad_ingest_out_len(const uvad_ctx *c, int64_t S_in) {
    if (!c || S_in < 0) return UVAD_E_ARG;
    if (!c->has_ingest) return UVAD_E_STATE;
    return (S_in * c->ig_up + c->ig_down - 1) / c->ig_down;
}

size_t uvad_ingest_state_bytes(const uvad_ctx *c, int B) {
    if (!c || !c->has_ingest || B <= 0 || (!ingest_identity(c) && !c->ig_taps)) return 0;
    return ingest_state(c, B).total;
}

int uvad_ingest(uvad_ctx *c, const void *d_in, int B, int64_t S_in, float *d_out, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = ingest_check(c, "uvad_ingest")) return r;
    if (!d_in || B <= 0 || S_in < 0 || (S_in > 0 && !d_out)) return fail(c, UVAD_E_ARG, "uvad_ingest: bad argument");
    if (S_in == 0) return UVAD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_ingest(ingest_args(c, d_in, B, S_in, d_out), (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_ingest_lens(uvad_ctx *c, const void *d_in, int B, int64_t S_in, const int64_t *d_nsamp, float *d_out, int64_t *d_out_nsamp,
                     void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = ingest_check(c, "uvad_ingest_lens")) return r;
    if (!d_in || !d_nsamp || !d_out_nsamp || B <= 0 || S_in < 0 || (S_in > 0 && !d_out)) return fail(c, UVAD_E_ARG, "uvad_ingest_lens: bad argument");
    IngestArgs a = ingest_args(c, d_in, B, S_in, d_out);
    a.nsamp = reinterpret_cast<const long long *>(d_nsamp);
    a.out_nsamp = reinterpret_cast<long long *>(d_out_nsamp);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_ingest(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_ingest_stream_reset(uvad_ctx *c, void *d_state, size_t state_bytes, int B, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = ingest_check(c, "uvad_ingest_stream_reset")) return r;
    if (!d_state || B <= 0) return fail(c, UVAD_E_ARG, "uvad_ingest_stream_reset: bad argument");
    const IngestState st = ingest_state(c, B);
    if (state_bytes < st.total)
        return fail(c, UVAD_E_WORKSPACE, "uvad_ingest_stream_reset: state too small: need " + std::to_string(st.total) + " bytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(d_state, 0, st.total, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_ingest_stream_step(uvad_ctx *c, const void *d_in, const uint8_t *d_flags, int B, int chunk_in, void *d_state, size_t state_bytes,
                            float *d_out, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!c->has_ingest) return fail(c, UVAD_E_STATE, "uvad_ingest_stream_step: call uvad_ingest_configure first");
    if (!d_in || !d_state || !d_out || B <= 0 || chunk_in <= 0) return fail(c, UVAD_E_ARG, "uvad_ingest_stream_step: bad argument");
    if (chunk_in % c->ig_down)
        return fail(c, UVAD_E_ARG, "uvad_ingest_stream_step: chunk_in must be a multiple of down = " + std::to_string(c->ig_down));
    if (int r = ingest_check(c, "uvad_ingest_stream_step")) return r;
    const IngestGeom g = ingest_geom(c);
    const IngestState st = ingest_state(c, B);
    if (state_bytes < st.total)
        return fail(c, UVAD_E_WORKSPACE, "uvad_ingest_stream_step: state too small: need " + std::to_string(st.total) + " bytes");
    IngestArgs a = ingest_args(c, d_in, B, chunk_in, d_out);
    char *base = reinterpret_cast<char *>(d_state);
    a.hist = reinterpret_cast<float *>(base);
    a.seen = reinterpret_cast<long long *>(base + st.off_seen);
    a.flags = d_flags; a.H = g.H; a.Dj = g.Dj;
    a.S_out = (long long)chunk_in / g.down * g.up;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_ingest(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_median_filter(uvad_ctx *c, const float *d_probs, int B, int T, int kernel, uint8_t *d_labels, void *stream) {
    if (!c || !d_probs || !d_labels || B <= 0 || T <= 0) return UVAD_E_ARG;
    if (kernel < 1 || kernel % 2 == 0) return fail(c, UVAD_E_ARG, "median kernel must be odd");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_median(d_probs, B, T, kernel, d_labels, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_der_counts(uvad_ctx *c, const uint8_t *d_pred, const uint8_t *d_gt, int B, int T, uint32_t *d_counts, void *stream) {
    if (!c || !d_pred || !d_gt || !d_counts || B <= 0 || T <= 0) return UVAD_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_der(d_pred, d_gt, B, T, d_counts, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_label_runs(uvad_ctx *c, const uint8_t *d_labels, int B, int T, int max_runs, int32_t *d_runs, int32_t *d_counts, void *stream) {
    if (!c || !d_labels || !d_runs || !d_counts || B <= 0 || T <= 0 || max_runs <= 0) return UVAD_E_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_runs(d_labels, B, T, max_runs, d_runs, d_counts, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_median_filter_lens(uvad_ctx *c, const float *d_probs, int B, int T, const int32_t *d_lens, int kernel, uint8_t *d_labels,
                            void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_probs || !d_labels || B <= 0 || T <= 0) return fail(c, UVAD_E_ARG, "uvad_median_filter_lens: bad argument");
    if (!d_lens) return fail(c, UVAD_E_ARG, "uvad_median_filter_lens: d_lens is NULL");
    if (kernel < 1 || kernel % 2 == 0) return fail(c, UVAD_E_ARG, "median kernel must be odd");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_median_lens(d_probs, B, T, kernel, d_labels, d_lens, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_label_runs_lens(uvad_ctx *c, const uint8_t *d_labels, int B, int T, const int32_t *d_lens, int max_runs, int32_t *d_runs,
                         int32_t *d_counts, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_labels || !d_runs || !d_counts || B <= 0 || T <= 0 || max_runs <= 0) return fail(c, UVAD_E_ARG, "uvad_label_runs_lens: bad argument");
    if (!d_lens) return fail(c, UVAD_E_ARG, "uvad_label_runs_lens: d_lens is NULL");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_runs_lens(d_labels, B, T, max_runs, d_runs, d_counts, d_lens, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- the live endpointer (endpoint.hip) ------------------------------------------------------------------------------------------------
static bool endpoint_cfg_ok(const uvad_endpoint_cfg *q) {
    return q && q->kernel >= 1 && q->kernel <= 255 && q->kernel % 2 == 1 && q->pad >= 0 && q->pad <= (1 << 20) && std::isfinite(q->threshold);
}

size_t uvad_endpoint_state_bytes(const uvad_ctx *c, int B, const uvad_endpoint_cfg *q) {
    if (!c || B < 1 || !endpoint_cfg_ok(q)) return 0;
    return endpoint_state_bytes(B);
}

int uvad_endpoint_reset(uvad_ctx *c, void *d_state, size_t state_bytes, int B, const uvad_endpoint_cfg *q, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || B < 1 || !q) return fail(c, UVAD_E_ARG, "uvad_endpoint_reset: bad argument");
    if (q->kernel < 1 || q->kernel > 255 || q->kernel % 2 == 0) return fail(c, UVAD_E_ARG, "uvad_endpoint_reset: kernel must be odd, 1 .. 255");
    if (q->pad < 0 || q->pad > (1 << 20)) return fail(c, UVAD_E_ARG, "uvad_endpoint_reset: pad must lie in [0, 2^20] frames");
    if (!std::isfinite(q->threshold)) return fail(c, UVAD_E_ARG, "uvad_endpoint_reset: threshold must be finite");
    if (state_bytes < endpoint_state_bytes(B))
        return fail(c, UVAD_E_ARG, "uvad_endpoint_reset: state too small: need " + std::to_string(endpoint_state_bytes(B)) + " bytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_endpoint_reset(d_state, B, q->kernel, q->pad, q->threshold, (hipStream_t)stream));
    EndpointPool g;
    g.B = B; g.kernel = q->kernel; g.pad = q->pad; g.threshold = q->threshold;
    c->endpoints[d_state] = g;
    return UVAD_OK;
}

int uvad_endpoint_step(uvad_ctx *c, const float *d_probs, int ld_in, const int32_t *d_counts, const uint8_t *d_flags, int B, void *d_state,
                       size_t state_bytes, int32_t *d_events, int max_events, int32_t *d_ev_counts, uint8_t *d_active, uint8_t *d_labels,
                       int ld_lab, int32_t *d_lab_counts, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_probs || !d_counts || !d_ev_counts || !d_state || B < 1 || ld_in < 1) return fail(c, UVAD_E_ARG, "uvad_endpoint_step: bad argument");
    if (ld_in > EP_MAX_LD_IN) return fail(c, UVAD_E_ARG, "uvad_endpoint_step: ld_in above " + std::to_string(EP_MAX_LD_IN) + " frames per step");
    if (max_events < 0 || (max_events > 0 && !d_events)) return fail(c, UVAD_E_ARG, "uvad_endpoint_step: d_events is NULL with max_events > 0");
    if (d_labels && !d_lab_counts) return fail(c, UVAD_E_ARG, "uvad_endpoint_step: d_labels needs d_lab_counts");
    auto it = c->endpoints.find(d_state);
    if (it == c->endpoints.end()) return fail(c, UVAD_E_STATE, "uvad_endpoint_step: call uvad_endpoint_reset on this state first");
    const EndpointPool &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_STATE, "uvad_endpoint_step: the state was reset with B = " + std::to_string(g.B));
    if (state_bytes < endpoint_state_bytes(B))
        return fail(c, UVAD_E_ARG, "uvad_endpoint_step: state too small: need " + std::to_string(endpoint_state_bytes(B)) + " bytes");
    if (d_labels && (int64_t)ld_lab < (int64_t)ld_in + g.kernel / 2)
        return fail(c, UVAD_E_ARG, "uvad_endpoint_step: ld_lab must be at least ld_in + kernel / 2 = " + std::to_string(ld_in + g.kernel / 2));
    EndpointArgs a{};
    a.probs = d_probs; a.ld_in = ld_in; a.counts = d_counts; a.flags = d_flags; a.B = B; a.state = d_state;
    a.events = d_events; a.max_events = max_events; a.ev_counts = d_ev_counts; a.active = d_active;
    a.labels = d_labels; a.ld_lab = ld_lab; a.lab_counts = d_lab_counts;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_endpoint_step(a, g.kernel, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- scoring against reference labels (score.hip) --------------------------------------------------------------------------------------
int uvad_intervals_to_labels(uvad_ctx *c, const int32_t *d_iv, const int32_t *d_iv_counts, int B, int max_iv, int T, int ld,
                             const int32_t *d_lens, uint8_t *d_labels, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_iv_counts || !d_labels || B < 1 || T < 1 || T > SC_MAX_T || max_iv < 0 || (max_iv > 0 && !d_iv))
        return fail(c, UVAD_E_ARG, "uvad_intervals_to_labels: bad argument");
    if (ld < T) return fail(c, UVAD_E_ARG, "uvad_intervals_to_labels: ld must be at least T");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_intervals_to_labels(d_iv, d_iv_counts, B, max_iv, T, ld, d_lens, d_labels, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_score_configure(uvad_ctx *c, const uvad_score_cfg *q) {
    if (!c) return UVAD_E_ARG;
    if (!q) return fail(c, UVAD_E_ARG, "uvad_score_configure: bad argument");
    if (q->n_points < 1 || q->n_points > SC_MAX_POINTS) return fail(c, UVAD_E_ARG, "uvad_score_configure: n_points must lie in 1 .. 8");
    for (int m = 0; m < q->n_points; ++m) {
        if (q->kernel[m] < 1 || q->kernel[m] > 255 || q->kernel[m] % 2 == 0)
            return fail(c, UVAD_E_ARG, "uvad_score_configure: kernel must be odd, 1 .. 255");
        if (!std::isfinite(q->threshold[m])) return fail(c, UVAD_E_ARG, "uvad_score_configure: threshold must be finite");
    }
    if (q->collar < 0 || q->collar > SC_MAX_COLLAR) return fail(c, UVAD_E_ARG, "uvad_score_configure: collar must lie in [0, 1024] frames");
    if (q->bins < 2 || q->bins > SC_MAX_BINS || (q->bins & (q->bins - 1)))
        return fail(c, UVAD_E_ARG, "uvad_score_configure: bins must be a power of two, 2 .. 1024");
    if (q->segment < 0 || q->segment > SC_MAX_SEGMENT) return fail(c, UVAD_E_ARG, "uvad_score_configure: segment must lie in [0, 16384] frames");
    c->sq = *q;
    if (c->sq.segment == 0) c->sq.segment = SC_DEFAULT_SEGMENT;
    c->has_score = true;
    return UVAD_OK;
}

size_t uvad_score_state_bytes(const uvad_ctx *c) { return c && c->has_score ? score_state_bytes() : 0; }

size_t uvad_score_ws_bytes(const uvad_ctx *c, int B, int T) {
    if (!c || !c->has_score || B < 1 || T < 1 || T > SC_MAX_T) return 0;
    return score_ws_bytes(B, T, c->sq.segment);
}

int uvad_score_reset(uvad_ctx *c, void *d_state, size_t state_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state) return fail(c, UVAD_E_ARG, "uvad_score_reset: bad argument");
    if (!c->has_score) return fail(c, UVAD_E_STATE, "uvad_score_reset: call uvad_score_configure first");
    if (state_bytes < score_state_bytes())
        return fail(c, UVAD_E_ARG, "uvad_score_reset: state too small: need " + std::to_string(score_state_bytes()) + " bytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_score_reset(d_state, c->sq.n_points, c->sq.bins, (hipStream_t)stream));
    ScoreState g;
    g.n_points = c->sq.n_points; g.bins = c->sq.bins;
    c->scores[d_state] = g;
    return UVAD_OK;
}

int uvad_score_step(uvad_ctx *c, const float *d_probs, int ld_p, const uint8_t *d_gt, int ld_gt, int B, int T, const int32_t *d_lens,
                    void *d_state, size_t state_bytes, uint64_t *d_rows, void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_probs || !d_gt || !d_state || !d_ws || B < 1 || T < 1 || T > SC_MAX_T) return fail(c, UVAD_E_ARG, "uvad_score_step: bad argument");
    if (ld_p < T || ld_gt < T) return fail(c, UVAD_E_ARG, "uvad_score_step: ld_p and ld_gt must be at least T");
    if (!c->has_score) return fail(c, UVAD_E_STATE, "uvad_score_step: call uvad_score_configure first");
    if (state_bytes < score_state_bytes())
        return fail(c, UVAD_E_ARG, "uvad_score_step: state too small: need " + std::to_string(score_state_bytes()) + " bytes");
    const uvad_score_cfg &q = c->sq;
    const size_t need = score_ws_bytes(B, T, q.segment);
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, "uvad_score_step: workspace too small: need " + std::to_string(need) + " bytes");
    if ((long long)B * score_nseg(T, q.segment) > 0x7fffffffll) return fail(c, UVAD_E_ARG, "uvad_score_step: B x segments above 2^31 - 1");
    auto it = c->scores.find(d_state);
    if (it == c->scores.end()) return fail(c, UVAD_E_STATE, "uvad_score_step: call uvad_score_reset on this state first");
    if (it->second.n_points != q.n_points || it->second.bins != q.bins)
        return fail(c, UVAD_E_STATE, "uvad_score_step: the state was reset under another n_points / bins");
    ScoreArgs a{};
    a.probs = d_probs; a.ld_p = ld_p; a.gt = d_gt; a.ld_gt = ld_gt; a.B = B; a.T = T; a.lens = d_lens;
    a.state = d_state; a.rows = reinterpret_cast<unsigned long long *>(d_rows); a.ws = d_ws;
    a.n_points = q.n_points; a.collar = q.collar; a.bins = q.bins; a.seg = q.segment; a.nseg = score_nseg(T, q.segment);
    a.halo = q.collar;
    for (int m = 0; m < q.n_points; ++m) {
        a.thr[m] = q.threshold[m];
        a.half[m] = q.kernel[m] / 2;
        a.halo = std::max(a.halo, a.half[m]);
    }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_score_step(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_score_totals(uvad_ctx *c, const void *d_state, size_t state_bytes, uint64_t *d_out, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !d_out) return fail(c, UVAD_E_ARG, "uvad_score_totals: bad argument");
    if (state_bytes < score_state_bytes())
        return fail(c, UVAD_E_ARG, "uvad_score_totals: state too small: need " + std::to_string(score_state_bytes()) + " bytes");
    if (c->scores.find(const_cast<void *>(d_state)) == c->scores.end())
        return fail(c, UVAD_E_STATE, "uvad_score_totals: call uvad_score_reset on this state first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_score_totals(d_state, reinterpret_cast<unsigned long long *>(d_out), (hipStream_t)stream));
    return UVAD_OK;
}

// ---- head fine-tuning (head_train.hip) ----------------------------------------------------------------------------------------------------
// The optimiser's constants.  1 - beta as torch hands it to lerp_ / addcmul_: the difference taken in f64 from the double the caller wrote
// (0.999, not the f32 next to it, whose complement is 1.3e-5 off) -- the shortest decimal that rounds to the f32 given -- and rounded to f32 once
static HeadTrainAdam adam_of(float lr, float beta1, float beta2, float eps) {
    auto one_minus = [](float b) {
        char buf[32];
        double d = (double)b;
        for (int p = 1; p <= 9; ++p) {
            std::snprintf(buf, sizeof buf, "%.*g", p, (double)b);
            d = std::strtod(buf, nullptr);
            if ((float)d == b) break;
        }
        return (float)(1.0 - d);
    };
    return HeadTrainAdam{lr, beta1, beta2, eps, one_minus(beta1), one_minus(beta2)};
}

// nullptr: in range; else the words uvad_last_error names.  The segment's words end where the caller names the unit (frames, positions).
static const char *adam_cfg_error(float lr, float beta1, float beta2, float eps) {
    if (!std::isfinite(lr) || !(lr > 0.0f)) return "lr must be finite and positive";
    if (!std::isfinite(beta1) || beta1 < 0.0f || !(beta1 < 1.0f)) return "beta1 must lie in [0, 1)";
    if (!std::isfinite(beta2) || beta2 < 0.0f || !(beta2 < 1.0f)) return "beta2 must lie in [0, 1)";
    if (!std::isfinite(eps) || !(eps > 0.0f)) return "eps must be finite and positive";
    return nullptr;
}
static const char *segment_error(int segment) {
    if (segment != 0 && (segment < HT_MIN_SEGMENT || segment > HT_MAX_SEGMENT || segment % 32)) return "segment must be 0 or a multiple of 32 in [32, 16384] ";
    return nullptr;
}

// ---- what the three training families share: one view of a family's configuration on the context, and the calls on a state's blocks ----
constexpr int TRAIN_TAG_FLAG = 1 << 30;   // a bit a family may keep beside the tag in its map of reset states (SincNet: reset found band edges)
struct TrainFamily {
    const char *name;                          // "head", "lstm", "sincnet": the messages name uvad_<name>_train_*
    bool configured;
    size_t state_bytes;
    unsigned magic; int P, Pp;                 // the TrainBlock of a state of this family
    float lr, beta1, beta2, eps;
    const std::map<void *, int> &resets;       // the states this family reset -> the tag then; the maps stay apart, so a state belongs to one family
    int tag;                                   // what "reset under this shape" compares: P (head, LSTM), first_stage (SincNet)
};
static TrainFamily head_family(const uvad_ctx *c) {
    return {"head", c->has_ht, uvad_head_train_state_bytes(c), HT_MAGIC, c->hts.P, c->hts.Pp, c->hq.lr, c->hq.beta1, c->hq.beta2, c->hq.eps,
            c->head_trains, c->hts.P};
}
static TrainFamily lstm_family(const uvad_ctx *c) {
    return {"lstm", c->has_lt, uvad_lstm_train_state_bytes(c), LT_MAGIC, c->lts.P, c->lts.Pp, c->lq.lr, c->lq.beta1, c->lq.beta2, c->lq.eps,
            c->lstm_trains, c->lts.P};
}
static TrainFamily sinc_family(const uvad_ctx *c) {
    return {"sincnet", c->has_snt, uvad_sincnet_train_state_bytes(c), SNT_MAGIC, c->snts.P, c->snts.Pp, c->snq.lr, c->snq.beta1, c->snq.beta2, c->snq.eps,
            c->sinc_trains, c->snts.first_stage};
}

// the checks every call on a state shares, `fn` the public call refused; `reset`: the call that makes the state known
static int train_state_check(uvad_ctx *c, const TrainFamily &v, const std::string &fn, const void *d_state, size_t state_bytes, bool reset) {
    const std::string family = std::string("uvad_") + v.name + "_train_";
    if (!d_state) return fail(c, UVAD_E_ARG, fn + ": bad argument");
    if (!v.configured) return fail(c, UVAD_E_STATE, fn + ": call " + family + "configure first");
    if (state_bytes < v.state_bytes) return fail(c, UVAD_E_ARG, fn + ": state too small: need " + std::to_string(v.state_bytes) + " bytes");
    if (reset) return UVAD_OK;
    auto it = v.resets.find(const_cast<void *>(d_state));
    if (it == v.resets.end()) return fail(c, UVAD_E_STATE, fn + ": call " + family + "reset on this state first");
    if ((it->second & ~TRAIN_TAG_FLAG) != v.tag) return fail(c, UVAD_E_STATE, fn + ": the state was reset under another shape");
    return UVAD_OK;
}

static int train_apply(uvad_ctx *c, const TrainFamily &v, void *d_state, size_t state_bytes, void *stream) {
    if (int r = train_state_check(c, v, std::string("uvad_") + v.name + "_train_apply", d_state, state_bytes, false)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_train_apply(TrainBlock{d_state, v.magic, v.P, v.Pp}, adam_of(v.lr, v.beta1, v.beta2, v.eps), (hipStream_t)stream));
    return UVAD_OK;
}

// which = MASTERS .. SCALARS; SincNet's bank (which 5) is its own entry's case
static int train_read(uvad_ctx *c, const TrainFamily &v, const void *d_state, size_t state_bytes, int which, float *d_out, void *stream) {
    const std::string fn = std::string("uvad_") + v.name + "_train_read";
    if (!d_out || which < 0 || which > UVAD_HEAD_TRAIN_SCALARS) return fail(c, UVAD_E_ARG, fn + ": bad argument");
    if (int r = train_state_check(c, v, fn, d_state, state_bytes, false)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_train_read(TrainBlock{const_cast<void *>(d_state), v.magic, v.P, v.Pp}, which, d_out, (hipStream_t)stream));
    return UVAD_OK;
}

static int train_write(uvad_ctx *c, const TrainFamily &v, void *d_state, size_t state_bytes, int which, const float *d_in, void *stream) {
    const std::string fn = std::string("uvad_") + v.name + "_train_write";
    const bool which_ok = which == UVAD_HEAD_TRAIN_MASTERS || which == UVAD_HEAD_TRAIN_M || which == UVAD_HEAD_TRAIN_V || which == UVAD_HEAD_TRAIN_SCALARS;
    if (!d_in || !which_ok) return fail(c, UVAD_E_ARG, fn + ": bad argument");
    if (int r = train_state_check(c, v, fn, d_state, state_bytes, false)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_train_write(TrainBlock{d_state, v.magic, v.P, v.Pp}, which, d_in, (hipStream_t)stream));
    return UVAD_OK;
}

// the shell of a family's _commit: the checks, every enqueued backward / apply landed, then `words` floats from behind the header on the host.
// before_copy (SincNet: the bank rebuilt from the masters) runs between the two.
static int train_commit_begin(uvad_ctx *c, const TrainFamily &v, const void *d_state, size_t state_bytes, size_t words, std::vector<float> &host,
                              hipError_t (*before_copy)(uvad_ctx *, const void *) = nullptr) {
    const std::string fn = std::string("uvad_") + v.name + "_train_commit";
    if (int r = train_state_check(c, v, fn, d_state, state_bytes, false)) return r;
    if (!c->finalized) return fail(c, UVAD_E_STATE, fn + ": call uvad_finalize first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    if (before_copy) HIPCHK(c, before_copy(c, d_state));
    host.resize(words);
    HIPCHK(c, hipMemcpy(host.data(), reinterpret_cast<const char *>(d_state) + sizeof(HeadTrainHeader), words * sizeof(float), hipMemcpyDeviceToHost));
    return UVAD_OK;
}

int uvad_head_train_configure(uvad_ctx *c, const uvad_head_train_cfg *q) {
    if (!c) return UVAD_E_ARG;
    if (!q) return fail(c, UVAD_E_ARG, "uvad_head_train_configure: bad argument");
    if (const char *e = adam_cfg_error(q->lr, q->beta1, q->beta2, q->eps)) return fail(c, UVAD_E_ARG, std::string("uvad_head_train_configure: ") + e);
    if (const char *e = segment_error(q->segment)) return fail(c, UVAD_E_ARG, std::string("uvad_head_train_configure: ") + e + "frames");
    if (!c->has_model) return fail(c, UVAD_E_STATE, "uvad_head_train_configure: context was created without a model configuration");
    const uvad_model_cfg &m = c->mc;
    const int D0 = m.hidden * (m.bidirectional ? 2 : 1);
    if (D0 % 32 || D0 > HT_MAX_D0) return fail(c, UVAD_E_UNSUPPORTED, "uvad_head_train_configure: hidden x directions must be a multiple of 32, at most 2048");
    if (m.lin_layers > HT_MAX_LAYERS) return fail(c, UVAD_E_UNSUPPORTED, "uvad_head_train_configure: at most 4 feed-forward layers");
    if (m.lin_layers > 0 && (m.lin_hidden < 32 || m.lin_hidden > HT_MAX_HIDDEN || m.lin_hidden % 32))
        return fail(c, UVAD_E_UNSUPPORTED, "uvad_head_train_configure: lin_hidden must be a multiple of 32 in [32, 256]");
    if (m.lin_layers > 0 && !(m.leaky_slope > 0.0f))
        return fail(c, UVAD_E_UNSUPPORTED, "uvad_head_train_configure: leaky_slope must be positive (the backward pass reads leaky' from the activation's sign)");
    c->hq = *q;
    if (c->hq.segment == 0) c->hq.segment = HT_DEFAULT_SEGMENT;
    c->hts = head_train_shape(D0, m.lin_layers > 0 ? m.lin_hidden : 0, m.lin_layers, m.leaky_slope);
    c->has_ht = true;
    return UVAD_OK;
}

int64_t uvad_head_train_param_count(const uvad_ctx *c) { return c && c->has_ht ? (int64_t)c->hts.P : 0; }
size_t uvad_head_train_state_bytes(const uvad_ctx *c) { return c && c->has_ht ? head_train_state_bytes(c->hts) : 0; }

size_t uvad_head_train_ws_bytes(const uvad_ctx *c, int B, int T) {
    if (!c || !c->has_ht || B < 1 || T < 1 || (long long)B * T > HT_MAX_FRAMES) return 0;
    return head_train_ws(c->hts, (long long)B * T, c->hq.segment).total;
}

int uvad_head_train_reset(uvad_ctx *c, void *d_state, size_t state_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = train_state_check(c, head_family(c), "uvad_head_train_reset", d_state, state_bytes, true)) return r;
    if (!c->finalized) return fail(c, UVAD_E_STATE, "uvad_head_train_reset: call uvad_finalize first");
    const HeadTrainShape &q = c->hts;
    const PackedWeights &W = *c->packed;
    HeadTrainInit in{};
    for (int l = 0; l < q.L; ++l) { in.w[l] = W.lin_w[l]; in.b[l] = W.lin_b[l]; in.ldw[l] = gemm_padded_k(l ? q.H : q.D0); }
    in.w[q.L] = W.cls_w; in.b[q.L] = W.cls_b; in.ldw[q.L] = q.L ? q.H : q.D0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_head_train_reset(q, in, d_state, (hipStream_t)stream));
    c->head_trains[d_state] = q.P;
    return UVAD_OK;
}

int uvad_head_train_grad(uvad_ctx *c, const float *d_x, int B, int T, const int32_t *d_lens, const uint8_t *d_gt, int ld_gt,
                         const float *d_fw, int ld_fw, const float *d_dz, int ld_dz, float *d_probs, int ld_p, float *d_grad_x,
                         void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_x || !d_state || !d_ws || B < 1 || T < 1) return fail(c, UVAD_E_ARG, "uvad_head_train_grad: bad argument");
    if ((long long)B * T > HT_MAX_FRAMES) return fail(c, UVAD_E_ARG, "uvad_head_train_grad: B x T above 2^24 frames");
    if (!d_dz && !d_gt) return fail(c, UVAD_E_ARG, "uvad_head_train_grad: labels (d_gt) or a gradient (d_dz) must be given");
    if (c->has_ht && ((long long)B * T + c->hq.segment - 1) / c->hq.segment > 65535)
        return fail(c, UVAD_E_ARG, "uvad_head_train_grad: more than 65535 segments: B x T / segment too large");
    if ((d_dz && ld_dz < T) || (!d_dz && ld_gt < T) || (!d_dz && d_fw && ld_fw < T) || (d_probs && ld_p < T))
        return fail(c, UVAD_E_ARG, "uvad_head_train_grad: ld_gt, ld_fw, ld_dz and ld_p must be at least T");
    if (int r = train_state_check(c, head_family(c), "uvad_head_train_grad", d_state, state_bytes, true)) return r;   // configured, and the state's size
    const size_t need = head_train_ws(c->hts, (long long)B * T, c->hq.segment).total;
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, "uvad_head_train_grad: workspace too small: need " + std::to_string(need) + " bytes");
    if (int r = train_state_check(c, head_family(c), "uvad_head_train_grad", d_state, state_bytes, false)) return r;  // ... and that it was reset
    HeadTrainGradArgs a{};
    a.x = d_x; a.B = B; a.T = T; a.lens = d_lens;
    a.gt = d_dz ? nullptr : d_gt; a.ld_gt = ld_gt; a.fw = d_dz ? nullptr : d_fw; a.ld_fw = ld_fw; a.dz_in = d_dz; a.ld_dz = ld_dz;
    a.probs = d_probs; a.ld_p = ld_p; a.grad_x = d_grad_x;
    a.state = d_state; a.ws = d_ws; a.seg = c->hq.segment;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_head_train_grad(c->hts, a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_head_train_apply(uvad_ctx *c, void *d_state, size_t state_bytes, void *stream) {
    return c ? train_apply(c, head_family(c), d_state, state_bytes, stream) : UVAD_E_ARG;
}

int uvad_head_train_read(uvad_ctx *c, const void *d_state, size_t state_bytes, int which, float *d_out, void *stream) {
    return c ? train_read(c, head_family(c), d_state, state_bytes, which, d_out, stream) : UVAD_E_ARG;
}

int uvad_head_train_commit(uvad_ctx *c, const void *d_state, size_t state_bytes) {
    if (!c) return UVAD_E_ARG;
    const HeadTrainShape &q = c->hts;
    std::vector<float> w;
    if (int r = train_commit_begin(c, head_family(c), d_state, state_bytes, (size_t)q.P, w)) return r;
    for (int l = 0; l <= q.L; ++l) {
        const bool cls = l == q.L;
        const int K = cls ? (q.L ? q.H : q.D0) : (l ? q.H : q.D0), rows = cls ? 1 : q.H;
        const std::string name = cls ? std::string("classifier") : "linear." + std::to_string(l);
        const int64_t wshape[2] = {rows, K}, bshape[1] = {rows};
        int r;
        if ((r = uvad_set_weight(c, (name + ".weight").c_str(), w.data() + q.off_w[l], wshape, 2))) return r;
        if ((r = uvad_set_weight(c, (name + ".bias").c_str(), w.data() + q.off_b[l], bshape, 1))) return r;
    }
    return uvad_finalize(c);
}

// ---- LSTM training (lstm_train.hip) ---------------------------------------------------------------------------------------------------------
int uvad_lstm_train_configure(uvad_ctx *c, const uvad_lstm_train_cfg *q) {
    if (!c) return UVAD_E_ARG;
    if (!q) return fail(c, UVAD_E_ARG, "uvad_lstm_train_configure: bad argument");
    if (const char *e = adam_cfg_error(q->lr, q->beta1, q->beta2, q->eps)) return fail(c, UVAD_E_ARG, std::string("uvad_lstm_train_configure: ") + e);
    if (const char *e = segment_error(q->segment)) return fail(c, UVAD_E_ARG, std::string("uvad_lstm_train_configure: ") + e + "frames");
    if (!c->has_model) return fail(c, UVAD_E_STATE, "uvad_lstm_train_configure: context was created without a model configuration");
    const uvad_model_cfg &m = c->mc;
    if (q->first_layer < 0 || q->first_layer >= m.num_layers)
        return fail(c, UVAD_E_ARG, "uvad_lstm_train_configure: first_layer must lie in [0, num_layers)");
    if (m.hidden != 64 && m.hidden != 128) return fail(c, UVAD_E_UNSUPPORTED, "uvad_lstm_train_configure: hidden must be 64 or 128");
    if (m.num_layers - q->first_layer > LT_MAX_LAYERS) return fail(c, UVAD_E_UNSUPPORTED, "uvad_lstm_train_configure: at most 8 trainable layers");
    const int dirs = m.bidirectional ? 2 : 1;
    const int Din = q->first_layer == 0 ? m.in_dim : m.hidden * dirs;
    if (Din < 4 || Din % 4 || Din > LT_MAX_DIN)
        return fail(c, UVAD_E_UNSUPPORTED, "uvad_lstm_train_configure: the input width of first_layer must be a multiple of 4, at most 2048");
    c->lq = *q;
    if (c->lq.segment == 0) c->lq.segment = HT_DEFAULT_SEGMENT;
    c->lts = lstm_train_shape(Din, m.hidden, dirs, m.num_layers, q->first_layer);
    c->has_lt = true;
    return UVAD_OK;
}

int uvad_lstm_train_set_dropout(uvad_ctx *c, float p, uint64_t seed) {
    if (!c) return UVAD_E_ARG;
    if (!std::isfinite(p) || p < 0.0f || !(p < 1.0f)) return fail(c, UVAD_E_ARG, "uvad_lstm_train_set_dropout: p must lie in [0, 1)");
    if (!c->has_model) return fail(c, UVAD_E_STATE, "uvad_lstm_train_set_dropout: context was created without a model configuration");
    if (!c->has_lt) return fail(c, UVAD_E_STATE, "uvad_lstm_train_set_dropout: call uvad_lstm_train_configure first");
    c->lt_thr = lstm_dropout_threshold(p);
    c->lt_scale = 1.0f / (1.0f - p);
    c->lt_seed = seed;
    return UVAD_OK;
}

int uvad_dropout_apply(const float *d_x, float *d_out, int64_t rows, int cols, int layer, uint64_t draw, float p, uint64_t seed, void *stream) {
    if (!d_x || !d_out || rows < 1 || rows > HT_MAX_FRAMES || cols < 4 || cols % 4 || cols > LT_DROP_MAX_COLS || layer < 0 ||
        layer > LT_DROP_MAX_LAYER || !std::isfinite(p) || p < 0.0f || !(p < 1.0f) || reinterpret_cast<uintptr_t>(d_x) % 16 ||
        reinterpret_cast<uintptr_t>(d_out) % 16)
        return UVAD_E_ARG;
    return launch_dropout_apply(d_x, d_out, rows, cols, layer, draw, lstm_dropout_threshold(p), 1.0f / (1.0f - p), seed, (hipStream_t)stream) ==
                   hipSuccess ? UVAD_OK : UVAD_E_HIP;
}

int64_t uvad_lstm_train_param_count(const uvad_ctx *c) { return c && c->has_lt ? (int64_t)c->lts.P : 0; }
size_t uvad_lstm_train_state_bytes(const uvad_ctx *c) { return c && c->has_lt ? lstm_train_state_bytes(c->lts) : 0; }

size_t uvad_lstm_train_ws_bytes(const uvad_ctx *c, int B, int T) {
    if (!c || !c->has_lt || B < 1 || T < 1 || (long long)B * T > HT_MAX_FRAMES) return 0;
    return lstm_train_ws(c->lts, (long long)B * T, c->lq.segment).total;
}

// the torch key of a trainable tensor: which = 0 .. 3 (weight_ih, weight_hh, bias_ih, bias_hh)
static std::string lstm_train_key(int layer, int dir, int which) {
    const char *const names[4] = {"weight_ih", "weight_hh", "bias_ih", "bias_hh"};
    return std::string("lstm.") + names[which] + "_l" + std::to_string(layer) + (dir ? "_reverse" : "");
}

int uvad_lstm_train_reset(uvad_ctx *c, void *d_state, size_t state_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = train_state_check(c, lstm_family(c), "uvad_lstm_train_reset", d_state, state_bytes, true)) return r;
    if (!c->finalized) return fail(c, UVAD_E_STATE, "uvad_lstm_train_reset: call uvad_finalize first");
    const LstmTrainShape &q = c->lts;
    std::vector<float> w((size_t)q.P);
    for (int li = 0; li < q.nl; ++li)
        for (int d = 0; d < q.dirs; ++d)
            for (int k = 0; k < 4; ++k) {
                const std::string key = lstm_train_key(q.first_layer + li, d, k);
                auto it = c->host_w.find(key);
                const size_t n = (size_t)4 * q.H * (k == 0 ? q.in[li] : k == 1 ? q.H : 1);
                if (it == c->host_w.end() || it->second.data.size() != n) return fail(c, UVAD_E_STATE, "uvad_lstm_train_reset: missing LSTM tensor " + key);
                std::memcpy(w.data() + q.off[li][d][k], it->second.data.data(), n * sizeof(float));
            }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));   // the masters come from the host tensors: a blocking copy, then the rest on the stream
    HIPCHK(c, hipMemcpy(reinterpret_cast<char *>(d_state) + sizeof(HeadTrainHeader), w.data(), w.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, launch_lstm_train_reset(q, d_state, (hipStream_t)stream));
    c->lstm_trains[d_state] = q.P;
    return UVAD_OK;
}

// the checks forward and backward share, in the head's order: arguments, configuration and sizes, then that the state was reset
static int lstm_train_call_check(uvad_ctx *c, const char *fn, const void *d_x, const void *d_other, int B, int T, void *d_state, size_t state_bytes,
                                 void *d_ws, size_t ws_bytes) {
    const std::string f(fn);
    if (!d_x || !d_other || !d_state || !d_ws || B < 1 || T < 1) return fail(c, UVAD_E_ARG, f + ": bad argument");
    if (reinterpret_cast<uintptr_t>(d_state) % 16 || reinterpret_cast<uintptr_t>(d_ws) % 16)
        return fail(c, UVAD_E_ARG, f + ": d_state and d_ws must be 16-byte aligned");
    if ((long long)B * T > HT_MAX_FRAMES) return fail(c, UVAD_E_ARG, f + ": B x T above 2^24 frames");
    if (c->has_lt && ((long long)B * T + c->lq.segment - 1) / c->lq.segment > 65535)
        return fail(c, UVAD_E_ARG, f + ": more than 65535 segments: B x T / segment too large");
    if (int r = train_state_check(c, lstm_family(c), f, d_state, state_bytes, true)) return r;
    const size_t need = lstm_train_ws(c->lts, (long long)B * T, c->lq.segment).total;
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, f + ": workspace too small: need " + std::to_string(need) + " bytes");
    return train_state_check(c, lstm_family(c), f, d_state, state_bytes, false);
}

int uvad_lstm_train_forward(uvad_ctx *c, const float *d_x_in, int B, int T, const int32_t *d_lens, float *d_y, void *d_state, size_t state_bytes,
                            void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = lstm_train_call_check(c, "uvad_lstm_train_forward", d_x_in, d_y, B, T, d_state, state_bytes, d_ws, ws_bytes)) return r;
    LstmTrainArgs a{};
    a.x = d_x_in; a.B = B; a.T = T; a.lens = d_lens; a.y = d_y; a.state = d_state; a.ws = d_ws; a.seg = c->lq.segment;
    a.thr = c->lt_thr; a.scale = c->lt_scale; a.seed = c->lt_seed;
    c->lt_dropped = a.thr > 0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_lstm_train_forward(c->lts, a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_lstm_train_backward(uvad_ctx *c, const float *d_x_in, const float *d_dy, int B, int T, const int32_t *d_lens, float *d_grad_in,
                             void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = lstm_train_call_check(c, "uvad_lstm_train_backward", d_x_in, d_dy, B, T, d_state, state_bytes, d_ws, ws_bytes)) return r;
    LstmTrainArgs a{};
    a.x = d_x_in; a.dy = d_dy; a.B = B; a.T = T; a.lens = d_lens; a.grad_in = d_grad_in; a.state = d_state; a.ws = d_ws; a.seg = c->lq.segment;
    a.drop = c->lt_thr > 0 || c->lt_dropped;   // the masks themselves come from the workspace header; off and never on: today's launches
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_lstm_train_backward(c->lts, a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_lstm_train_apply(uvad_ctx *c, void *d_state, size_t state_bytes, void *stream) {
    return c ? train_apply(c, lstm_family(c), d_state, state_bytes, stream) : UVAD_E_ARG;
}

int uvad_lstm_train_read(uvad_ctx *c, const void *d_state, size_t state_bytes, int which, float *d_out, void *stream) {
    return c ? train_read(c, lstm_family(c), d_state, state_bytes, which, d_out, stream) : UVAD_E_ARG;
}

int uvad_lstm_train_commit(uvad_ctx *c, const void *d_state, size_t state_bytes) {
    if (!c) return UVAD_E_ARG;
    const LstmTrainShape q = c->lts;
    std::vector<float> w;
    if (int r = train_commit_begin(c, lstm_family(c), d_state, state_bytes, (size_t)q.P, w)) return r;
    for (int li = 0; li < q.nl; ++li)
        for (int d = 0; d < q.dirs; ++d)
            for (int k = 0; k < 4; ++k) {
                const int64_t shape[2] = {4 * q.H, k == 0 ? q.in[li] : q.H};
                if (int r = uvad_set_weight(c, lstm_train_key(q.first_layer + li, d, k).c_str(), w.data() + q.off[li][d][k], shape, k < 2 ? 2 : 1)) return r;
            }
    return uvad_finalize(c);
}

// ---- SincNet training (sincnet_train.hip) ----------------------------------------------------------------------------------------------------
int uvad_sincnet_train_configure(uvad_ctx *c, const uvad_sincnet_train_cfg *q) {
    if (!c) return UVAD_E_ARG;
    if (!q) return fail(c, UVAD_E_ARG, "uvad_sincnet_train_configure: bad argument");
    if (const char *e = adam_cfg_error(q->lr, q->beta1, q->beta2, q->eps)) return fail(c, UVAD_E_ARG, std::string("uvad_sincnet_train_configure: ") + e);
    if (const char *e = segment_error(q->segment)) return fail(c, UVAD_E_ARG, std::string("uvad_sincnet_train_configure: ") + e + "positions");
    if (q->first_stage < 0 || q->first_stage > 2) return fail(c, UVAD_E_ARG, "uvad_sincnet_train_configure: first_stage must lie in [0, 2]");
    if (!c->has_model) return fail(c, UVAD_E_STATE, "uvad_sincnet_train_configure: context was created without a model configuration");
    if (!c->has_sinc) return fail(c, UVAD_E_STATE, "uvad_sincnet_train_configure: the context has no SincNet stage (uvad_sincnet_configure)");
    const uvad_sincnet_cfg &sc = c->sc;
    if (!(sc.leaky_slope <= 1.0f)) return fail(c, UVAD_E_UNSUPPORTED, "uvad_sincnet_train_configure: leaky_slope must be <= 1");
    if (q->first_stage == 0 && !(sc.kernel_size & 1))
        return fail(c, UVAD_E_UNSUPPORTED, "uvad_sincnet_train_configure: a learning sinc bank needs an odd kernel_size");
    c->snq = *q;
    if (c->snq.segment == 0) c->snq.segment = HT_DEFAULT_SEGMENT;
    c->snts = sinc_train_shape(sc.n_filters, sc.kernel_size, sc.stride, sc.c2, sc.k2, sc.c3, sc.k3, sc.leaky_slope, sc.eps, q->first_stage);
    c->has_snt = true;
    return UVAD_OK;
}

int64_t uvad_sincnet_train_param_count(const uvad_ctx *c) { return c && c->has_snt ? (int64_t)c->snts.P : 0; }
size_t uvad_sincnet_train_state_bytes(const uvad_ctx *c) { return c && c->has_snt ? sinc_train_state_bytes(c->snts) : 0; }

// nullptr: (B, S) is served; else the word uvad_last_error names
static const char *sinc_train_shape_error(const uvad_ctx *c, int B, int64_t S, SincTrainGeo *geo_out) {
    if (B < 1 || B > SNT_MAX_B) return "B must lie in [1, 65535]";
    if (S < 1) return "S must be >= 1";
    const SincTrainGeo geo = sinc_train_geo(c->snts, S);
    if (!geo.ok) return "S too short for one output frame";
    if ((long long)B * geo.L[0] > 0x7fffffffLL) return "B x L_0 above 2^31 - 1 conv positions";
    if (((long long)B * 3 * geo.Lp[c->snts.first_stage] + c->snq.segment - 1) / c->snq.segment > 65535)
        return "more than 65535 segments: B x 3 Lp / segment too large";
    if (geo_out) *geo_out = geo;
    return nullptr;
}

size_t uvad_sincnet_train_ws_bytes(const uvad_ctx *c, int B, int64_t S) {
    SincTrainGeo geo;
    if (!c || !c->has_snt || sinc_train_shape_error(c, B, S, &geo)) return 0;
    return sinc_train_ws(c->snts, geo, B, c->snq.segment).total;
}

// the torch key and shape of tensor t (SNT_T_* order)
static std::string sinc_train_key(int t) {
    static const char *const names[SNT_TENSORS] = {"wav_norm1d.weight", "wav_norm1d.bias", "conv1d.0.filterbank.low_hz_", "conv1d.0.filterbank.band_hz_",
                                                   "conv1d.1.weight", "conv1d.1.bias", "conv1d.2.weight", "conv1d.2.bias", "norm1d.0.weight",
                                                   "norm1d.0.bias", "norm1d.1.weight", "norm1d.1.bias", "norm1d.2.weight", "norm1d.2.bias"};
    return std::string("sincnet.") + names[t];
}
static int sinc_train_tensor_shape(const SincTrainShape &q, int t, int64_t shape[3]) {
    if (t == SNT_T_LOW || t == SNT_T_BAND) { shape[0] = q.NF / 2; shape[1] = 1; return 2; }
    if (t == SNT_T_CONV || t == SNT_T_CONV + 2) {
        const int s = t == SNT_T_CONV ? 1 : 2;
        shape[0] = q.Cout[s]; shape[1] = q.Cin[s]; shape[2] = q.Kw[s];
        return 3;
    }
    shape[0] = q.cnt[t];
    return 1;
}

int uvad_sincnet_train_reset(uvad_ctx *c, void *d_state, size_t state_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = train_state_check(c, sinc_family(c), "uvad_sincnet_train_reset", d_state, state_bytes, true)) return r;
    if (!c->finalized) return fail(c, UVAD_E_STATE, "uvad_sincnet_train_reset: call uvad_finalize first");
    const SincTrainShape &q = c->snts;
    auto get = [&](const std::string &k) -> const HostTensor * {
        auto it = c->host_w.find(k);
        return it == c->host_w.end() ? nullptr : &it->second;
    };
    const size_t words = (sinc_train_state_bytes(q) - sizeof(HeadTrainHeader)) / sizeof(float);
    std::vector<float> img(words, 0.0f);
    for (int t = 0; t < SNT_TENSORS; ++t) {
        const HostTensor *h = get(sinc_train_key(t));
        const bool edge = t == SNT_T_LOW || t == SNT_T_BAND;
        if (!h && edge && q.first_stage > 0) continue;   // a frozen bank runs from sincnet.conv1d.0.filters
        if (!h || h->data.size() != (size_t)q.cnt[t]) return fail(c, UVAD_E_STATE, "uvad_sincnet_train_reset: missing SincNet tensor " + sinc_train_key(t));
        std::memcpy(img.data() + q.off_fullblock + q.off_full[t], h->data.data(), h->data.size() * sizeof(float));
        if (q.off_master[t] >= 0) std::memcpy(img.data() + q.off_master[t], h->data.data(), h->data.size() * sizeof(float));
    }
    const bool edges = get(sinc_train_key(SNT_T_LOW)) && get(sinc_train_key(SNT_T_BAND)) && (q.KS & 1);
    if (const HostTensor *f = get("sincnet.conv1d.0.filters")) {
        if (f->data.size() != (size_t)q.NF * q.KS) return fail(c, UVAD_E_STATE, "uvad_sincnet_train_reset: misshaped sincnet.conv1d.0.filters");
        std::memcpy(img.data() + q.off_bank, f->data.data(), f->data.size() * sizeof(float));
    } else if (!edges) {
        return fail(c, UVAD_E_STATE, "uvad_sincnet_train_reset: missing SincNet tensor sincnet.conv1d.0.filters");
    }
    const int half = q.KS / 2;
    const HostTensor *hw = get("sincnet.conv1d.0.filterbank.window_"), *hn = get("sincnet.conv1d.0.filterbank.n_");
    for (int i = 0; i < half; ++i) {   // ParamSincFB's buffers: np.hamming(kernel_size)[:half] as f32, 2 pi (i - half) / 16000 in f32
        img[q.off_win + i] = hw && hw->data.size() == (size_t)half ? hw->data[i] : (float)(0.54 - 0.46 * std::cos(2.0 * M_PI * i / (double)(q.KS - 1)));
        img[q.off_n + i] = hn && hn->data.size() == (size_t)half ? hn->data[i] : (float)(2.0 * M_PI) * ((float)(i - half) / 16000.0f);
    }
    HeadTrainHeader h{};
    h.magic = SNT_MAGIC; h.D0 = q.first_stage; h.H = q.NF; h.L = q.KS; h.P = q.P;
    h.pad0 = edges ? 1 : 0;   // the forward call materialises the bank from the band edges
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));   // the state comes from the host tensors: blocking copies
    HIPCHK(c, hipMemcpy(reinterpret_cast<char *>(d_state) + sizeof(HeadTrainHeader), img.data(), img.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, hipMemcpy(d_state, &h, sizeof h, hipMemcpyHostToDevice));
    c->sinc_trains[d_state] = q.first_stage | (edges ? TRAIN_TAG_FLAG : 0);
    return UVAD_OK;
}

// the checks forward and backward share: arguments, configuration, shape and sizes, then that the state was reset
static int sinc_train_call_check(uvad_ctx *c, const char *fn, const void *d_wav, const void *d_other, int B, int64_t S, void *d_state, size_t state_bytes,
                                 void *d_ws, size_t ws_bytes) {
    const std::string f(fn);
    if (!d_wav || !d_other || !d_state || !d_ws || B < 1 || S < 1) return fail(c, UVAD_E_ARG, f + ": bad argument");
    if (reinterpret_cast<uintptr_t>(d_state) % 16 || reinterpret_cast<uintptr_t>(d_ws) % 16)
        return fail(c, UVAD_E_ARG, f + ": d_state and d_ws must be 16-byte aligned");
    if (int r = train_state_check(c, sinc_family(c), f, d_state, state_bytes, true)) return r;
    SincTrainGeo geo;
    if (const char *w = sinc_train_shape_error(c, B, S, &geo)) return fail(c, UVAD_E_ARG, f + ": " + w);
    const size_t need = sinc_train_ws(c->snts, geo, B, c->snq.segment).total;
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, f + ": workspace too small: need " + std::to_string(need) + " bytes");
    return train_state_check(c, sinc_family(c), f, d_state, state_bytes, false);
}

int uvad_sincnet_train_forward(uvad_ctx *c, const float *d_wav, int B, int64_t S, float *d_feats, void *d_state, size_t state_bytes, void *d_ws,
                               size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = sinc_train_call_check(c, "uvad_sincnet_train_forward", d_wav, d_feats, B, S, d_state, state_bytes, d_ws, ws_bytes)) return r;
    SincTrainArgs a{};
    a.wav = d_wav; a.B = B; a.S = S; a.feats = d_feats; a.state = d_state; a.ws = d_ws; a.seg = c->snq.segment;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_sinc_train_forward(c->snts, a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_sincnet_train_backward(uvad_ctx *c, const float *d_wav, const float *d_dfeats, int B, int64_t S, void *d_state, size_t state_bytes,
                                void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (int r = sinc_train_call_check(c, "uvad_sincnet_train_backward", d_wav, d_dfeats, B, S, d_state, state_bytes, d_ws, ws_bytes)) return r;
    SincTrainArgs a{};
    a.wav = d_wav; a.dfeats = d_dfeats; a.B = B; a.S = S; a.state = d_state; a.ws = d_ws; a.seg = c->snq.segment;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_sinc_train_backward(c->snts, a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_sincnet_train_apply(uvad_ctx *c, void *d_state, size_t state_bytes, void *stream) {
    return c ? train_apply(c, sinc_family(c), d_state, state_bytes, stream) : UVAD_E_ARG;
}

int uvad_sincnet_train_read(uvad_ctx *c, const void *d_state, size_t state_bytes, int which, float *d_out, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (which != UVAD_SINCNET_TRAIN_FILTERS) return train_read(c, sinc_family(c), d_state, state_bytes, which, d_out, stream);
    if (!d_out) return fail(c, UVAD_E_ARG, "uvad_sincnet_train_read: bad argument");
    if (int r = train_state_check(c, sinc_family(c), "uvad_sincnet_train_read", d_state, state_bytes, false)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_sinc_train_read_bank(c->snts, d_state, d_out, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_sincnet_train_commit(uvad_ctx *c, const void *d_state, size_t state_bytes) {
    if (!c) return UVAD_E_ARG;
    const SincTrainShape q = c->snts;
    // a state reset with band edges: the bank of the masters as they stand after the last apply, so that what is served matches the committed edges
    auto bank = [](uvad_ctx *x, const void *st) -> hipError_t {
        if (!(x->sinc_trains[const_cast<void *>(st)] & TRAIN_TAG_FLAG)) return hipSuccess;
        const hipError_t e = launch_sinc_train_bank(x->snts, const_cast<void *>(st), nullptr);
        return e != hipSuccess ? e : hipDeviceSynchronize();
    };
    std::vector<float> w;
    if (int r = train_commit_begin(c, sinc_family(c), d_state, state_bytes, (size_t)q.off_bank + q.bankp, w, bank)) return r;
    const bool edges = (c->sinc_trains[const_cast<void *>(d_state)] & TRAIN_TAG_FLAG) != 0;
    for (int t = 0; t < SNT_TENSORS; ++t) {
        if (q.off_master[t] < 0) continue;
        int64_t shape[3];
        const int nd = sinc_train_tensor_shape(q, t, shape);
        if (int r = uvad_set_weight(c, sinc_train_key(t).c_str(), w.data() + q.off_master[t], shape, nd)) return r;
    }
    if (edges) {   // learning or frozen
        const int64_t shape[3] = {q.NF, 1, q.KS};
        if (int r = uvad_set_weight(c, "sincnet.conv1d.0.filters", w.data() + q.off_bank, shape, 3)) return r;
    }
    return uvad_finalize(c);
}

// ---- the joint optimizer step and the _write calls (optim.hip) ------------------------------------------------------------------------------
// nullptr: the configuration and the table are in range; else the word uvad_last_error names
static const char *optim_table_error(const float *h_lr_table, int n_lr) {
    if (!h_lr_table) return "h_lr_table is NULL";
    if (n_lr < 1 || n_lr > OPT_MAX_LR) return "n_lr must lie in [1, 2^24]";
    for (int i = 0; i < n_lr; ++i)
        if (!std::isfinite(h_lr_table[i]) || !(h_lr_table[i] > 0.0f)) return "every lr table entry must be finite and positive";
    return nullptr;
}
static const char *optim_cfg_error(const uvad_optim_cfg *q) {
    if (!q) return "cfg is NULL";
    if (const char *e = adam_cfg_error(1.0f, q->beta1, q->beta2, q->eps)) return e;   // the learning rates are the table's
    if (!std::isfinite(q->max_norm) || q->max_norm < 0.0f) return "max_norm must be finite and >= 0";
    if (!std::isfinite(q->weight_decay) || q->weight_decay < 0.0f) return "weight_decay must be finite and >= 0";
    for (int k = 0; k < 3; ++k)
        if (!std::isfinite(q->lr_scale[k]) || q->lr_scale[k] < 0.0f) return "every lr_scale must be finite and >= 0";
    return nullptr;
}

size_t uvad_optim_state_bytes(int n_lr) { return n_lr < 1 || n_lr > OPT_MAX_LR ? 0 : optim_state_bytes(n_lr); }

size_t uvad_optim_ws_bytes(const uvad_ctx *c) {
    if (!c) return 0;
    int chunks = 0;
    for (const TrainFamily &v : {head_family(c), lstm_family(c), sinc_family(c)}) chunks += v.configured ? optim_chunks(v.P) : 0;
    return chunks ? optim_ws_bytes(chunks) : 0;
}

int uvad_optim_reset(uvad_ctx *c, void *d_state, size_t state_bytes, const uvad_optim_cfg *q, const float *h_lr_table, int n_lr, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state) return fail(c, UVAD_E_ARG, "uvad_optim_reset: bad argument");
    if (const char *e = optim_cfg_error(q)) return fail(c, UVAD_E_ARG, std::string("uvad_optim_reset: ") + e);
    if (const char *e = optim_table_error(h_lr_table, n_lr)) return fail(c, UVAD_E_ARG, std::string("uvad_optim_reset: ") + e);
    if (reinterpret_cast<uintptr_t>(d_state) % 16) return fail(c, UVAD_E_ARG, "uvad_optim_reset: d_state must be 16-byte aligned");
    const size_t need = optim_state_bytes(n_lr);
    if (state_bytes < need) return fail(c, UVAD_E_ARG, "uvad_optim_reset: state too small: need " + std::to_string(need) + " bytes");
    const HeadTrainAdam o = adam_of(1.0f, q->beta1, q->beta2, q->eps);
    std::vector<char> host(need, 0);
    OptimHeader h{};
    h.magic = OPT_MAGIC; h.cap = n_lr; h.n = n_lr; h.decoupled = q->decoupled ? 1 : 0; h.skip_nonfinite = q->skip_nonfinite ? 1 : 0;
    h.b1 = o.b1; h.b2 = o.b2; h.eps = o.eps; h.omb1 = o.omb1; h.omb2 = o.omb2; h.max_norm = q->max_norm; h.wd = q->weight_decay;
    for (int k = 0; k < 3; ++k) h.lr_scale[k] = q->lr_scale[k];
    std::memcpy(host.data(), &h, sizeof h);
    std::memcpy(host.data() + sizeof h, h_lr_table, (size_t)n_lr * sizeof(float));
    c->optims.erase(d_state);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));      // what the stream still does to this state comes first
    HIPCHK(c, hipMemcpy(d_state, host.data(), host.size(), hipMemcpyHostToDevice));
    c->optims[d_state] = n_lr;
    return UVAD_OK;
}

// the checks every call on a reset optim state shares -> its n_lr at reset through *cap
static int optim_state_check(uvad_ctx *c, const char *fn, const void *d_state, size_t state_bytes, int *cap) {
    const std::string f(fn);
    if (!d_state) return fail(c, UVAD_E_ARG, f + ": bad argument");
    auto it = c->optims.find(const_cast<void *>(d_state));
    if (it == c->optims.end()) return fail(c, UVAD_E_STATE, f + ": call uvad_optim_reset on this state first");
    const size_t need = optim_state_bytes(it->second);
    if (state_bytes < need) return fail(c, UVAD_E_ARG, f + ": state too small: need " + std::to_string(need) + " bytes");
    *cap = it->second;
    return UVAD_OK;
}

int uvad_optim_set_lr_table(uvad_ctx *c, void *d_state, size_t state_bytes, const float *h_lr_table, int n_lr, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state) return fail(c, UVAD_E_ARG, "uvad_optim_set_lr_table: bad argument");
    if (const char *e = optim_table_error(h_lr_table, n_lr)) return fail(c, UVAD_E_ARG, std::string("uvad_optim_set_lr_table: ") + e);
    int cap = 0;
    if (int r = optim_state_check(c, "uvad_optim_set_lr_table", d_state, state_bytes, &cap)) return r;
    if (n_lr > cap) return fail(c, UVAD_E_ARG, "uvad_optim_set_lr_table: n_lr above the " + std::to_string(cap) + " entries of uvad_optim_reset");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));      // the steps enqueued so far read the old table
    HIPCHK(c, hipMemcpy(reinterpret_cast<char *>(d_state) + sizeof(OptimHeader), h_lr_table, (size_t)n_lr * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(c, launch_optim_set_n(d_state, cap, n_lr, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_optim_step(uvad_ctx *c, void *d_head_state, size_t head_bytes, void *d_lstm_state, size_t lstm_bytes, void *d_sincnet_state,
                    size_t sincnet_bytes, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !d_ws) return fail(c, UVAD_E_ARG, "uvad_optim_step: bad argument");
    if (!d_head_state && !d_lstm_state && !d_sincnet_state) return fail(c, UVAD_E_ARG, "uvad_optim_step: at least one training state must be given");
    if (reinterpret_cast<uintptr_t>(d_ws) % 8) return fail(c, UVAD_E_ARG, "uvad_optim_step: d_ws must be 8-byte aligned");
    void *const given[3] = {d_head_state, d_lstm_state, d_sincnet_state};
    const size_t bytes[3] = {head_bytes, lstm_bytes, sincnet_bytes};
    const TrainFamily family[3] = {head_family(c), lstm_family(c), sinc_family(c)};
    TrainBlock fam[3] = {};
    int chunks = 0;
    for (int k = 0; k < 3; ++k) {   // a family whose state is given: configured, and the state's size
        if (!given[k]) continue;
        if (int r = train_state_check(c, family[k], "uvad_optim_step", given[k], bytes[k], true)) return r;
        fam[k] = TrainBlock{given[k], family[k].magic, family[k].P, family[k].Pp};
        chunks += optim_chunks(family[k].P);
    }
    int cap = 0;
    if (int r = optim_state_check(c, "uvad_optim_step", d_state, state_bytes, &cap)) return r;
    const size_t need = optim_ws_bytes(chunks);
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, "uvad_optim_step: workspace too small: need " + std::to_string(need) + " bytes");
    for (int k = 0; k < 3; ++k)     // ... and that it was reset
        if (given[k])
            if (int r = train_state_check(c, family[k], "uvad_optim_step", given[k], bytes[k], false)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_optim_step(fam, d_state, cap, reinterpret_cast<double *>(d_ws), (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_optim_read(uvad_ctx *c, const void *d_state, size_t state_bytes, void *d_out, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_out) return fail(c, UVAD_E_ARG, "uvad_optim_read: bad argument");
    int cap = 0;
    if (int r = optim_state_check(c, "uvad_optim_read", d_state, state_bytes, &cap)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_optim_read(d_state, cap, reinterpret_cast<unsigned *>(d_out), (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_optim_write(uvad_ctx *c, void *d_state, size_t state_bytes, const void *d_in, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_in) return fail(c, UVAD_E_ARG, "uvad_optim_write: bad argument");
    int cap = 0;
    if (int r = optim_state_check(c, "uvad_optim_write", d_state, state_bytes, &cap)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_optim_write(d_state, cap, reinterpret_cast<const unsigned *>(d_in), (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_head_train_write(uvad_ctx *c, void *d_state, size_t state_bytes, int which, const float *d_in, void *stream) {
    return c ? train_write(c, head_family(c), d_state, state_bytes, which, d_in, stream) : UVAD_E_ARG;
}
int uvad_lstm_train_write(uvad_ctx *c, void *d_state, size_t state_bytes, int which, const float *d_in, void *stream) {
    return c ? train_write(c, lstm_family(c), d_state, state_bytes, which, d_in, stream) : UVAD_E_ARG;
}
int uvad_sincnet_train_write(uvad_ctx *c, void *d_state, size_t state_bytes, int which, const float *d_in, void *stream) {
    return c ? train_write(c, sinc_family(c), d_state, state_bytes, which, d_in, stream) : UVAD_E_ARG;
}

// ---- noise mixing of training batches (mix.hip) ------------------------------------------------------------------------------------------
// nullptr: the configuration is in range; else the word uvad_last_error names
static const char *mix_cfg_error(const uvad_mix_cfg *q) {
    if (!q) return "cfg is NULL";
    if (!std::isfinite(q->mix_prob) || q->mix_prob < 0.0f || q->mix_prob > 1.0f) return "mix_prob must lie in [0, 1]";
    if (q->snr_steps < 1 || q->snr_steps > (1 << 24)) return "snr_steps must lie in [1, 2^24]";
    if (!q->h_amp) return "h_amp is NULL";
    for (int i = 0; i < q->snr_steps; ++i)
        if (!std::isfinite(q->h_amp[i]) || q->h_amp[i] < 0.0) return "every amplitude must be finite and >= 0";
    if (q->max_seg < 1 || q->max_seg > MIX_MAX_SEG) return "max_seg must lie in [1, 64]";
    return nullptr;
}

size_t uvad_mix_state_bytes(const uvad_mix_cfg *q, int n_clips) {
    if (mix_cfg_error(q) || n_clips < 1) return 0;
    return mix_layout(n_clips, q->snr_steps).total;
}

size_t uvad_mix_ws_bytes(int B, int max_seg) {
    if (B < 1 || max_seg < 1 || max_seg > MIX_MAX_SEG) return 0;
    return mix_ws(B, max_seg).total;
}

int uvad_mix_reset(uvad_ctx *c, void *d_state, size_t state_bytes, const uvad_mix_cfg *q, const float *d_bank, const int64_t *h_clip_first,
                   int n_clips, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !d_bank || !h_clip_first) return fail(c, UVAD_E_ARG, "uvad_mix_reset: bad argument");
    if (const char *e = mix_cfg_error(q)) return fail(c, UVAD_E_ARG, std::string("uvad_mix_reset: ") + e);
    if (n_clips < 1) return fail(c, UVAD_E_ARG, "uvad_mix_reset: n_clips must be at least 1");
    if (reinterpret_cast<uintptr_t>(d_state) % 16) return fail(c, UVAD_E_ARG, "uvad_mix_reset: d_state must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_bank) % 4) return fail(c, UVAD_E_ARG, "uvad_mix_reset: d_bank must be 4-byte aligned");
    if (h_clip_first[0] != 0) return fail(c, UVAD_E_ARG, "uvad_mix_reset: h_clip_first[0] must be 0");
    for (int i = 0; i < n_clips; ++i)
        if (h_clip_first[i + 1] <= h_clip_first[i])
            return fail(c, UVAD_E_ARG, "uvad_mix_reset: h_clip_first must increase: clip " + std::to_string(i) + " is empty");
    const MixLayout l = mix_layout(n_clips, q->snr_steps);
    if (state_bytes < l.total) return fail(c, UVAD_E_ARG, "uvad_mix_reset: state too small: need " + std::to_string(l.total) + " bytes");
    std::vector<char> host(l.total, 0);
    MixHeader h{};
    h.magic = MIX_MAGIC; h.n_clips = n_clips; h.Q = q->snr_steps; h.max_seg = q->max_seg;
    h.thr = (unsigned long long)__builtin_floor((double)q->mix_prob * 4294967296.0);
    h.seed = q->seed; h.bank_total = h_clip_first[n_clips]; h.draws = 0;
    std::memcpy(host.data(), &h, sizeof(h));
    std::memcpy(host.data() + l.off_first, h_clip_first, ((size_t)n_clips + 1) * 8);
    std::memcpy(host.data() + l.off_amp, q->h_amp, (size_t)q->snr_steps * 8);
    c->mixes.erase(d_state);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));      // what the stream still does to this state comes first
    HIPCHK(c, hipMemcpy(d_state, host.data(), host.size(), hipMemcpyHostToDevice));
    HIPCHK(c, launch_mix_clip_energies(d_bank, d_state, n_clips, q->snr_steps, (hipStream_t)stream));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
    MixState g;
    g.bank = d_bank; g.n_clips = n_clips; g.Q = q->snr_steps; g.max_seg = q->max_seg;
    c->mixes[d_state] = g;
    return UVAD_OK;
}

static int mix_call(uvad_ctx *c, const char *fn, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan,
                    bool take, int64_t row0, uint64_t draw, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string f(fn);
    if (!d_in || !d_out || !d_state || !d_ws) return fail(c, UVAD_E_ARG, f + ": bad argument");
    if (fmt != UVAD_INGEST_F32 && fmt != UVAD_INGEST_I16) return fail(c, UVAD_E_ARG, f + ": fmt must be UVAD_INGEST_F32 or UVAD_INGEST_I16");
    if (B < 1) return fail(c, UVAD_E_ARG, f + ": B must be at least 1");
    if (S < 1 || S > MIX_MAX_S) return fail(c, UVAD_E_ARG, f + ": S must lie in [1, 2^31 - 1]");
    if (reinterpret_cast<uintptr_t>(d_state) % 16 || reinterpret_cast<uintptr_t>(d_ws) % 16)
        return fail(c, UVAD_E_ARG, f + ": d_state and d_ws must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_in) % (fmt == UVAD_INGEST_F32 ? 4 : 2) || reinterpret_cast<uintptr_t>(d_out) % 4 ||
        reinterpret_cast<uintptr_t>(d_plan) % 4 || reinterpret_cast<uintptr_t>(d_nsamp) % 8)
        return fail(c, UVAD_E_ARG, f + ": d_in, d_out, d_plan and d_nsamp must be aligned to their element");
    if (fmt == UVAD_INGEST_I16 && d_in == static_cast<const void *>(d_out)) return fail(c, UVAD_E_ARG, f + ": int16 input cannot be mixed in place");
    auto it = c->mixes.find(d_state);
    if (it == c->mixes.end()) return fail(c, UVAD_E_STATE, f + ": call uvad_mix_reset on this state first");
    const MixState &g = it->second;
    const size_t need_state = mix_layout(g.n_clips, g.Q).total, need_ws = mix_ws(B, g.max_seg).total;
    if (state_bytes < need_state) return fail(c, UVAD_E_ARG, f + ": state too small: need " + std::to_string(need_state) + " bytes");
    if (ws_bytes < need_ws) return fail(c, UVAD_E_ARG, f + ": workspace too small: need " + std::to_string(need_ws) + " bytes");
    MixArgs a{};
    a.in = d_in; a.fmt = fmt; a.B = B; a.S = S; a.nsamp = reinterpret_cast<const long long *>(d_nsamp);
    a.out = d_out; a.plan = d_plan; a.bank = g.bank; a.state = d_state; a.ws = d_ws;
    a.n_clips = g.n_clips; a.Q = g.Q; a.max_seg = g.max_seg;
    a.take = take; a.draw = draw; a.row0 = row0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_mix(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_mix_step(uvad_ctx *c, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan, void *d_state,
                  size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    return mix_call(c, "uvad_mix_step", d_in, fmt, B, S, d_nsamp, d_out, d_plan, true, 0, 0, d_state, state_bytes, d_ws, ws_bytes, stream);
}

int uvad_mix_apply(uvad_ctx *c, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan, int64_t row0,
                   uint64_t draw, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    return mix_call(c, "uvad_mix_apply", d_in, fmt, B, S, d_nsamp, d_out, d_plan, false, row0, draw, d_state, state_bytes, d_ws, ws_bytes, stream);
}

// ---- reverberation of training batches (reverb.hip) --------------------------------------------------------------------------------------
// nullptr: the configuration is in range; else the word uvad_last_error names
static const char *reverb_cfg_error(const uvad_reverb_cfg *q) {
    if (!q) return "cfg is NULL";
    if (!std::isfinite(q->prob) || q->prob < 0.0f || q->prob > 1.0f) return "prob must lie in [0, 1]";
    if (q->max_taps < 0) return "max_taps must be >= 0";
    return nullptr;
}

size_t uvad_reverb_state_bytes(const uvad_reverb_cfg *q, int n_rirs) {
    if (reverb_cfg_error(q) || n_rirs < 1) return 0;
    return reverb_layout(n_rirs).total;
}

size_t uvad_reverb_ws_bytes(int B) {
    if (B < 1) return 0;
    return reverb_ws_bytes(B);
}

int uvad_reverb_reset(uvad_ctx *c, void *d_state, size_t state_bytes, const uvad_reverb_cfg *q, const float *d_rir, const int64_t *h_rir_first,
                      int n_rirs, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !d_rir || !h_rir_first) return fail(c, UVAD_E_ARG, "uvad_reverb_reset: bad argument");
    if (const char *e = reverb_cfg_error(q)) return fail(c, UVAD_E_ARG, std::string("uvad_reverb_reset: ") + e);
    if (n_rirs < 1) return fail(c, UVAD_E_ARG, "uvad_reverb_reset: n_rirs must be at least 1");
    if (reinterpret_cast<uintptr_t>(d_state) % 16) return fail(c, UVAD_E_ARG, "uvad_reverb_reset: d_state must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_rir) % 4) return fail(c, UVAD_E_ARG, "uvad_reverb_reset: d_rir must be 4-byte aligned");
    if (h_rir_first[0] != 0) return fail(c, UVAD_E_ARG, "uvad_reverb_reset: h_rir_first[0] must be 0");
    const ReverbLayout l = reverb_layout(n_rirs);
    std::vector<char> host(l.total, 0);
    int *taps = reinterpret_cast<int *>(host.data() + l.off_taps);
    for (int i = 0; i < n_rirs; ++i) {
        int64_t k = h_rir_first[i + 1] - h_rir_first[i];
        if (k <= 0) return fail(c, UVAD_E_ARG, "uvad_reverb_reset: h_rir_first must increase: response " + std::to_string(i) + " is empty");
        if (q->max_taps > 0) k = std::min<int64_t>(k, q->max_taps);
        if (k > REVERB_MAX_TAPS)
            return fail(c, UVAD_E_ARG, "uvad_reverb_reset: response " + std::to_string(i) + " has more than 2^20 taps: set max_taps");
        taps[i] = (int)k;
    }
    if (state_bytes < l.total) return fail(c, UVAD_E_ARG, "uvad_reverb_reset: state too small: need " + std::to_string(l.total) + " bytes");
    ReverbHeader h{};
    h.magic = REVERB_MAGIC; h.n_rirs = n_rirs; h.normalize = q->normalize != 0; h.align = q->align != 0;
    h.thr = (unsigned long long)__builtin_floor((double)q->prob * 4294967296.0);
    h.seed = q->seed; h.bank_total = h_rir_first[n_rirs]; h.max_taps = q->max_taps; h.draws = 0;
    std::memcpy(host.data(), &h, sizeof(h));
    std::memcpy(host.data() + l.off_first, h_rir_first, ((size_t)n_rirs + 1) * 8);
    c->reverbs.erase(d_state);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));      // what the stream still does to this state comes first
    HIPCHK(c, hipMemcpy(d_state, host.data(), host.size(), hipMemcpyHostToDevice));
    HIPCHK(c, launch_reverb_delays(d_rir, d_state, n_rirs, (hipStream_t)stream));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));
    ReverbState g;
    g.bank = d_rir; g.n_rirs = n_rirs; g.normalize = h.normalize;
    c->reverbs[d_state] = g;
    return UVAD_OK;
}

static int reverb_call(uvad_ctx *c, const char *fn, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out,
                       int32_t *d_plan, bool take, int64_t row0, uint64_t draw, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes,
                       void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string f(fn);
    if (!d_in || !d_out || !d_state || !d_ws) return fail(c, UVAD_E_ARG, f + ": bad argument");
    if (fmt != UVAD_INGEST_F32 && fmt != UVAD_INGEST_I16) return fail(c, UVAD_E_ARG, f + ": fmt must be UVAD_INGEST_F32 or UVAD_INGEST_I16");
    if (B < 1) return fail(c, UVAD_E_ARG, f + ": B must be at least 1");
    if (S < 1 || S > MIX_MAX_S) return fail(c, UVAD_E_ARG, f + ": S must lie in [1, 2^31 - 1]");
    if ((int64_t)B * ((S + REVERB_TILE - 1) / REVERB_TILE) > 2147483647LL) return fail(c, UVAD_E_ARG, f + ": B x ceil(S / 4096) must stay below 2^31");
    if (reinterpret_cast<uintptr_t>(d_state) % 16 || reinterpret_cast<uintptr_t>(d_ws) % 16)
        return fail(c, UVAD_E_ARG, f + ": d_state and d_ws must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_in) % (fmt == UVAD_INGEST_F32 ? 4 : 2) || reinterpret_cast<uintptr_t>(d_out) % 4 ||
        reinterpret_cast<uintptr_t>(d_plan) % 4 || reinterpret_cast<uintptr_t>(d_nsamp) % 8)
        return fail(c, UVAD_E_ARG, f + ": d_in, d_out, d_plan and d_nsamp must be aligned to their element");
    if (d_in == static_cast<const void *>(d_out)) return fail(c, UVAD_E_ARG, f + ": d_out == d_in: a row is read while it is written");
    auto it = c->reverbs.find(d_state);
    if (it == c->reverbs.end()) return fail(c, UVAD_E_STATE, f + ": call uvad_reverb_reset on this state first");
    const ReverbState &g = it->second;
    const size_t need_state = reverb_layout(g.n_rirs).total, need_ws = reverb_ws_bytes(B);
    if (state_bytes < need_state) return fail(c, UVAD_E_ARG, f + ": state too small: need " + std::to_string(need_state) + " bytes");
    if (ws_bytes < need_ws) return fail(c, UVAD_E_ARG, f + ": workspace too small: need " + std::to_string(need_ws) + " bytes");
    ReverbArgs a{};
    a.in = d_in; a.fmt = fmt; a.B = B; a.S = S; a.nsamp = reinterpret_cast<const long long *>(d_nsamp);
    a.out = d_out; a.plan = d_plan; a.bank = g.bank; a.state = d_state; a.ws = d_ws;
    a.n_rirs = g.n_rirs; a.normalize = g.normalize;
    a.take = take; a.draw = draw; a.row0 = row0;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_reverb(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_reverb_step(uvad_ctx *c, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan, void *d_state,
                     size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    return reverb_call(c, "uvad_reverb_step", d_in, fmt, B, S, d_nsamp, d_out, d_plan, true, 0, 0, d_state, state_bytes, d_ws, ws_bytes, stream);
}

int uvad_reverb_apply(uvad_ctx *c, const void *d_in, int fmt, int B, int64_t S, const int64_t *d_nsamp, float *d_out, int32_t *d_plan, int64_t row0,
                      uint64_t draw, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    return reverb_call(c, "uvad_reverb_apply", d_in, fmt, B, S, d_nsamp, d_out, d_plan, false, row0, draw, d_state, state_bytes, d_ws, ws_bytes, stream);
}

// ---- training batches drawn on the device (sampler.hip) ----------------------------------------------------------------------------------
// nullptr: the configuration is in range; else the word uvad_last_error names
static const char *sampler_cfg_error(const uvad_sampler_cfg *q, int D) {
    if (!q) return "cfg is NULL";
    if (q->window < 1 || q->window > SAMPLER_MAX_LEN) return "window must lie in [1, 2^31 - 1]";
    if (q->min_keep < 0 || q->min_keep >= q->window) return "min_keep must lie in [0, window)";
    if (q->geometry != UVAD_SAMPLER_FBANK && q->geometry != UVAD_SAMPLER_SINCNET) return "geometry must be UVAD_SAMPLER_FBANK or UVAD_SAMPLER_SINCNET";
    if (q->geometry == UVAD_SAMPLER_SINCNET && q->step < 1) return "step must be at least 1";
    if (q->geometry == UVAD_SAMPLER_SINCNET && q->half < 0) return "half must be >= 0";
    if (D < 1 || D > SAMPLER_MAX_SETS) return "D must lie in [1, 64]";
    if (q->drop_last && D > 1) return "drop_last needs D = 1";
    if (q->drop_last && q->batch < 1) return "drop_last needs batch >= 1";
    return nullptr;
}

size_t uvad_sampler_state_bytes(const uvad_sampler_cfg *q, int R, int n_sup, int D) {
    if (sampler_cfg_error(q, D) || R < 1 || n_sup < 0) return 0;
    return sampler_layout(R, n_sup).total;
}

size_t uvad_sampler_ws_bytes(int B) {
    if (B < 1) return 0;
    return sampler_ws_bytes(B);
}

int uvad_sampler_reset(uvad_ctx *c, void *d_state, size_t state_bytes, const uvad_sampler_cfg *q, const void *d_pcm, int fmt,
                       const int64_t *h_rec_first, int R, const int64_t *h_sup, const int32_t *h_sup_first, int n_sup, const int32_t *h_rec_set,
                       const double *h_weight, int D, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_state || !d_pcm || !h_rec_first || !h_sup_first || !h_rec_set || !h_weight) return fail(c, UVAD_E_ARG, "uvad_sampler_reset: bad argument");
    if (const char *e = sampler_cfg_error(q, D)) return fail(c, UVAD_E_ARG, std::string("uvad_sampler_reset: ") + e);
    if (fmt != UVAD_INGEST_F32 && fmt != UVAD_INGEST_I16) return fail(c, UVAD_E_ARG, "uvad_sampler_reset: fmt must be UVAD_INGEST_F32 or UVAD_INGEST_I16");
    if (R < 1) return fail(c, UVAD_E_ARG, "uvad_sampler_reset: R must be at least 1");
    if (n_sup < 0 || (n_sup > 0 && !h_sup)) return fail(c, UVAD_E_ARG, "uvad_sampler_reset: n_sup must be >= 0 and h_sup given");
    if (reinterpret_cast<uintptr_t>(d_state) % 16) return fail(c, UVAD_E_ARG, "uvad_sampler_reset: d_state must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_pcm) % (fmt == UVAD_INGEST_F32 ? 4 : 2)) return fail(c, UVAD_E_ARG, "uvad_sampler_reset: d_pcm must be aligned to its element");
    const SamplerLayout l = sampler_layout(R, n_sup);
    std::vector<char> host(l.total, 0);
    SamplerTables t{};
    t.q = q; t.fmt = fmt; t.rec_first = h_rec_first; t.R = R; t.sup = h_sup; t.sup_first = h_sup_first; t.n_sup = n_sup; t.rec_set = h_rec_set;
    t.weight = h_weight; t.D = D;
    if (const char *e = sampler_build(t, host.data())) return fail(c, UVAD_E_ARG, std::string("uvad_sampler_reset: ") + e);
    if (state_bytes < l.total) return fail(c, UVAD_E_ARG, "uvad_sampler_reset: state too small: need " + std::to_string(l.total) + " bytes");
    SamplerHeader *h = reinterpret_cast<SamplerHeader *>(host.data());
    int64_t T;
    if (q->geometry == UVAD_SAMPLER_FBANK) {
        if (!c->has_fb) return fail(c, UVAD_E_STATE, "uvad_sampler_reset: UVAD_SAMPLER_FBANK needs a context with a feature configuration");
        h->hop = c->fb.frame_shift; h->frame_len = c->fb.frame_len; h->snip = c->fb.snip_edges != 0;
        T = uvad_num_frames(c, q->window);
    } else {
        if (!c->has_sinc) return fail(c, UVAD_E_STATE, "uvad_sampler_reset: UVAD_SAMPLER_SINCNET needs uvad_sincnet_configure");
        h->kw[0] = c->sc.kernel_size; h->kw[1] = c->sc.k2; h->kw[2] = c->sc.k3; h->stride0 = c->sc.stride;
        T = uvad_sincnet_num_frames(c, q->window);
    }
    if (T != sampler_frames(*h, q->window)) return fail(c, UVAD_E_STATE, "uvad_sampler_reset: internal: the frame count disagrees with the front end's");
    if (T < 1) return fail(c, UVAD_E_ARG, "uvad_sampler_reset: a window of " + std::to_string(q->window) + " samples gives no frame");
    c->samplers.erase(d_state);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize((hipStream_t)stream));      // what the stream still does to this state comes first
    HIPCHK(c, hipMemcpy(d_state, host.data(), host.size(), hipMemcpyHostToDevice));
    SamplerState g;
    g.pcm = d_pcm; g.fmt = fmt; g.R = R; g.n_sup = n_sup; g.D = D; g.geometry = q->geometry; g.drop_last = q->drop_last != 0; g.batch = q->batch;
    g.W = q->window; g.T = T;
    c->samplers[d_state] = g;
    return UVAD_OK;
}

// the checks uvad_sampler_read / _write share with the step: a state that was reset, and large enough
static int sampler_state_check(uvad_ctx *c, const std::string &f, const void *d_state, size_t state_bytes, const SamplerState **out) {
    if (!d_state) return fail(c, UVAD_E_ARG, f + ": bad argument");
    if (reinterpret_cast<uintptr_t>(d_state) % 16) return fail(c, UVAD_E_ARG, f + ": d_state must be 16-byte aligned");
    auto it = c->samplers.find(const_cast<void *>(d_state));
    if (it == c->samplers.end()) return fail(c, UVAD_E_STATE, f + ": call uvad_sampler_reset on this state first");
    const size_t need = sampler_layout(it->second.R, it->second.n_sup).total;
    if (state_bytes < need) return fail(c, UVAD_E_ARG, f + ": state too small: need " + std::to_string(need) + " bytes");
    *out = &it->second;
    return UVAD_OK;
}

static int sampler_call(uvad_ctx *c, const char *fn, int B, float *d_out, int64_t ld_out, int64_t *d_nsamp, uint8_t *d_labels, int64_t ld_gt,
                        int32_t *d_frames, int32_t *d_plan, bool take, const int64_t *h_cursor, int64_t row0, uint64_t draw, void *d_state,
                        size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    const std::string f(fn);
    if (!d_out || !d_nsamp || !d_labels || !d_frames || !d_state || !d_ws || (!take && !h_cursor)) return fail(c, UVAD_E_ARG, f + ": bad argument");
    if (B < 1) return fail(c, UVAD_E_ARG, f + ": B must be at least 1");
    if (reinterpret_cast<uintptr_t>(d_state) % 16 || reinterpret_cast<uintptr_t>(d_ws) % 16)
        return fail(c, UVAD_E_ARG, f + ": d_state and d_ws must be 16-byte aligned");
    if (reinterpret_cast<uintptr_t>(d_out) % 4 || reinterpret_cast<uintptr_t>(d_nsamp) % 8 || reinterpret_cast<uintptr_t>(d_frames) % 4 ||
        reinterpret_cast<uintptr_t>(d_plan) % 4)
        return fail(c, UVAD_E_ARG, f + ": d_out, d_nsamp, d_frames and d_plan must be aligned to their element");
    const SamplerState *gp = nullptr;
    if (int r = sampler_state_check(c, f, d_state, state_bytes, &gp)) return r;
    const SamplerState &g = *gp;
    if (g.geometry == UVAD_SAMPLER_FBANK ? !c->has_fb : !c->has_sinc)
        return fail(c, UVAD_E_STATE, f + ": the label geometry's configuration is missing from the context");
    if (ld_out < g.W) return fail(c, UVAD_E_ARG, f + ": ld_out must be at least the window, " + std::to_string(g.W));
    if (ld_gt < g.T) return fail(c, UVAD_E_ARG, f + ": ld_gt must be at least the window's frames, " + std::to_string(g.T));
    if (g.drop_last && B != g.batch) return fail(c, UVAD_E_ARG, f + ": drop_last: B must be the configuration's batch, " + std::to_string(g.batch));
    if ((int64_t)B * (g.W / 4096 + 1) > 2147483647LL) return fail(c, UVAD_E_ARG, f + ": B x ceil(window / 4096) must stay below 2^31");
    const size_t need_ws = sampler_ws_bytes(B);
    if (ws_bytes < need_ws) return fail(c, UVAD_E_ARG, f + ": workspace too small: need " + std::to_string(need_ws) + " bytes");
    SamplerArgs a{};
    a.B = B; a.out = d_out; a.ld_out = ld_out; a.nsamp = reinterpret_cast<long long *>(d_nsamp); a.labels = d_labels; a.ld_gt = ld_gt;
    a.frames = d_frames; a.plan = d_plan; a.pcm = g.pcm; a.fmt = g.fmt; a.state = d_state; a.ws = d_ws; a.R = g.R; a.n_sup = g.n_sup; a.D = g.D;
    a.W = g.W; a.T = g.T; a.take = take; a.draw = draw; a.row0 = row0;
    if (!take)
        for (int d = 0; d < g.D; ++d) {
            if (h_cursor[d] < 0) return fail(c, UVAD_E_ARG, f + ": a cursor must be >= 0");
            a.cursor[d] = h_cursor[d];
        }
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_sampler(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_sampler_step(uvad_ctx *c, int B, float *d_out, int64_t ld_out, int64_t *d_nsamp, uint8_t *d_labels, int64_t ld_gt, int32_t *d_frames,
                      int32_t *d_plan, void *d_state, size_t state_bytes, void *d_ws, size_t ws_bytes, void *stream) {
    return sampler_call(c, "uvad_sampler_step", B, d_out, ld_out, d_nsamp, d_labels, ld_gt, d_frames, d_plan, true, nullptr, 0, 0, d_state, state_bytes,
                        d_ws, ws_bytes, stream);
}

int uvad_sampler_apply(uvad_ctx *c, int B, float *d_out, int64_t ld_out, int64_t *d_nsamp, uint8_t *d_labels, int64_t ld_gt, int32_t *d_frames,
                       int32_t *d_plan, const int64_t *h_cursor, int64_t row0, uint64_t draw, void *d_state, size_t state_bytes, void *d_ws,
                       size_t ws_bytes, void *stream) {
    return sampler_call(c, "uvad_sampler_apply", B, d_out, ld_out, d_nsamp, d_labels, ld_gt, d_frames, d_plan, false, h_cursor, row0, draw, d_state,
                        state_bytes, d_ws, ws_bytes, stream);
}

int uvad_sampler_read(uvad_ctx *c, const void *d_state, size_t state_bytes, int64_t *d_out, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_out || reinterpret_cast<uintptr_t>(d_out) % 8) return fail(c, UVAD_E_ARG, "uvad_sampler_read: bad argument");
    const SamplerState *g = nullptr;
    if (int r = sampler_state_check(c, "uvad_sampler_read", d_state, state_bytes, &g)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_sampler_read(d_state, g->D, reinterpret_cast<long long *>(d_out), (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_sampler_write(uvad_ctx *c, void *d_state, size_t state_bytes, const int64_t *d_in, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_in || reinterpret_cast<uintptr_t>(d_in) % 8) return fail(c, UVAD_E_ARG, "uvad_sampler_write: bad argument");
    const SamplerState *g = nullptr;
    if (int r = sampler_state_check(c, "uvad_sampler_write", d_state, state_bytes, &g)) return r;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_sampler_write(d_state, g->D, reinterpret_cast<const long long *>(d_in), (hipStream_t)stream));
    return UVAD_OK;
}

// ---- speech cuts (cuts.hip) --------------------------------------------------------------------------------------------------------------
// nullptr: the configuration is in range; else the word uvad_last_error names
static const char *cuts_cfg_error(const uvad_cuts_cfg *q) {
    if (!q) return "cfg is NULL";
    if (q->pad < 0 || q->pad > CUTS_MAX_PAD) return "pad must lie in [0, 2^20] frames";
    if (q->max_len < 0 || q->max_len > CUTS_MAX_LEN) return "max_len must lie in [0, 2^24] frames";
    if (q->min_len < 0 || (q->max_len > 0 && q->min_len >= q->max_len)) return "min_len must be >= 0 and below max_len";
    if (q->hop < 1) return "hop must be >= 1";
    if (q->lead < 0) return "lead must be >= 0";
    if (q->tail < 0) return "tail must be >= 0";
    return nullptr;
}
static CutsCfgInt cuts_cfg_of(const uvad_cuts_cfg *q) { return CutsCfgInt{q->pad, q->max_len, q->min_len, q->hop, q->lead, q->tail}; }

int uvad_cuts_max_per_row(const uvad_cuts_cfg *q, int T) {
    if (cuts_cfg_error(q) || T < 1 || T > CUTS_MAX_T) return 0;
    return cuts_max_per_row(cuts_cfg_of(q), T);
}

int64_t uvad_cuts_max_samples(const uvad_cuts_cfg *q, int64_t S) {
    if (cuts_cfg_error(q) || S < 0) return 0;
    if (q->max_len == 0) return S;
    return std::min<int64_t>(S, (int64_t)q->max_len * q->hop + q->lead + q->tail);
}

size_t uvad_cuts_ws_bytes(const uvad_ctx *c, int B, int T) {
    if (!c || B < 1 || T < 1 || T > CUTS_MAX_T) return 0;
    return cuts_ws_bytes(B, T);
}

int uvad_cuts_table(uvad_ctx *c, const uint8_t *d_labels, int ld, int B, int T, const int32_t *d_lens, const int64_t *d_nsamp, int64_t S,
                    const uvad_cuts_cfg *q, uvad_cut *d_table, int max_cuts, int32_t *d_row_first, int32_t *d_total, void *d_ws,
                    size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (const char *w = cuts_cfg_error(q)) return fail(c, UVAD_E_ARG, std::string("uvad_cuts_table: ") + w);
    if (B < 1) return fail(c, UVAD_E_ARG, "uvad_cuts_table: B must be >= 1");
    if (T < 1 || T > CUTS_MAX_T) return fail(c, UVAD_E_ARG, "uvad_cuts_table: T must lie in [1, 2^30]");
    if (ld < T) return fail(c, UVAD_E_ARG, "uvad_cuts_table: ld must be at least T");
    if (S < 0) return fail(c, UVAD_E_ARG, "uvad_cuts_table: S must be >= 0");
    if (max_cuts < 0) return fail(c, UVAD_E_ARG, "uvad_cuts_table: max_cuts must be >= 0");
    if (!d_labels) return fail(c, UVAD_E_ARG, "uvad_cuts_table: d_labels is NULL");
    if (!d_row_first) return fail(c, UVAD_E_ARG, "uvad_cuts_table: d_row_first is NULL");
    if (!d_total) return fail(c, UVAD_E_ARG, "uvad_cuts_table: d_total is NULL");
    if (!d_ws) return fail(c, UVAD_E_ARG, "uvad_cuts_table: d_ws is NULL");
    if (max_cuts > 0 && !d_table) return fail(c, UVAD_E_ARG, "uvad_cuts_table: d_table is NULL with max_cuts > 0");
    const CutsCfgInt qi = cuts_cfg_of(q);
    if ((long long)B * cuts_max_per_row(qi, T) > 0x7fffffffll) return fail(c, UVAD_E_ARG, "uvad_cuts_table: B x uvad_cuts_max_per_row above 2^31 - 1");
    const size_t need = cuts_ws_bytes(B, T);
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, "uvad_cuts_table: workspace too small: need " + std::to_string(need) + " bytes");
    CutsTableArgs a{};
    a.labels = d_labels; a.ld = ld; a.B = B; a.T = T; a.lens = d_lens; a.nsamp = reinterpret_cast<const long long *>(d_nsamp); a.S = S;
    a.q = qi;
    a.table = reinterpret_cast<CutRecord *>(d_table); a.max_cuts = max_cuts; a.row_first = d_row_first; a.total = d_total;
    a.counts = reinterpret_cast<int *>(d_ws);
    a.iv = reinterpret_cast<CutsInterval *>(reinterpret_cast<char *>(d_ws) + cuts_counts_bytes(B));
    a.cap = (T + 1) / 2;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_cuts_table(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_cuts_gather(uvad_ctx *c, const void *d_src, int64_t row_stride, int unit_bytes, int which, const uvad_cut *d_table,
                     const int32_t *d_total, int max_cuts, void *d_out, int64_t ld_out, int32_t *d_out_len, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (which != UVAD_CUTS_SAMPLES && which != UVAD_CUTS_FRAMES) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: which must be UVAD_CUTS_SAMPLES or UVAD_CUTS_FRAMES");
    if (which == UVAD_CUTS_SAMPLES && unit_bytes != 2 && unit_bytes != 4)
        return fail(c, UVAD_E_ARG, "uvad_cuts_gather: unit_bytes must be 2 (int16) or 4 (f32) for samples");
    if (which == UVAD_CUTS_FRAMES && (unit_bytes < 4 || unit_bytes > 4096 || unit_bytes % 4))
        return fail(c, UVAD_E_ARG, "uvad_cuts_gather: unit_bytes must be a multiple of 4 in [4, 4096] for frames");
    if (ld_out < 1 || ld_out > 0x7fffffffll) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: ld_out must lie in [1, 2^31 - 1]");
    if (row_stride < 0) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: row_stride must be >= 0");
    if (max_cuts < 0) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: max_cuts must be >= 0");
    if (!d_src) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: d_src is NULL");
    if (!d_table) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: d_table is NULL");
    if (!d_total) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: d_total is NULL");
    if (!d_out) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: d_out is NULL");
    if (!d_out_len) return fail(c, UVAD_E_ARG, "uvad_cuts_gather: d_out_len is NULL");
    CutsGatherArgs a{};
    a.src = d_src; a.row_stride = row_stride; a.unit_bytes = unit_bytes; a.frames = which == UVAD_CUTS_FRAMES;
    a.table = reinterpret_cast<const CutRecord *>(d_table); a.total = d_total; a.max_cuts = max_cuts;
    a.out = d_out; a.ld_out = ld_out; a.out_len = d_out_len; a.tiles = cuts_gather_tiles(ld_out, unit_bytes);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_cuts_gather(a, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- the cut-supervision join (join.hip) --------------------------------------------------------------------------------------------------
size_t uvad_cuts_join_ws_bytes(const uvad_ctx *c, int B, int max_iv, int max_cuts) {
    if (!c || B < 1 || max_iv < 0 || max_cuts < 0 || (long long)max_cuts * max_iv > 0x7fffffffll) return 0;
    return join_ws_bytes(max_cuts);
}

int uvad_cuts_join(uvad_ctx *c, const uvad_cut *d_table, const int32_t *d_row_first, const int32_t *d_total, int max_cuts, int B,
                   const int32_t *d_iv, const int32_t *d_iv_counts, int max_iv, int mode, int32_t *d_pair_first, int32_t *d_pairs,
                   int max_pairs, int32_t *d_item_cuts, uint64_t *d_audit, void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (B < 1) return fail(c, UVAD_E_ARG, "uvad_cuts_join: B must be >= 1");
    if (max_iv < 0) return fail(c, UVAD_E_ARG, "uvad_cuts_join: max_iv must be >= 0");
    if (max_cuts < 0) return fail(c, UVAD_E_ARG, "uvad_cuts_join: max_cuts must be >= 0");
    if (max_pairs < 0) return fail(c, UVAD_E_ARG, "uvad_cuts_join: max_pairs must be >= 0");
    if (mode != UVAD_JOIN_OVERLAP && mode != UVAD_JOIN_INSIDE) return fail(c, UVAD_E_ARG, "uvad_cuts_join: mode must be UVAD_JOIN_OVERLAP or UVAD_JOIN_INSIDE");
    if (!d_row_first) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_row_first is NULL");
    if (!d_total) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_total is NULL");
    if (!d_iv_counts) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_iv_counts is NULL");
    if (!d_pair_first) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_pair_first is NULL");
    if (!d_audit) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_audit is NULL");
    if (!d_ws) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_ws is NULL");
    if (max_cuts > 0 && !d_table) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_table is NULL with max_cuts > 0");
    if (max_iv > 0 && !d_iv) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_iv is NULL with max_iv > 0");
    if (max_pairs > 0 && !d_pairs) return fail(c, UVAD_E_ARG, "uvad_cuts_join: d_pairs is NULL with max_pairs > 0");
    if ((long long)max_cuts * max_iv > 0x7fffffffll) return fail(c, UVAD_E_ARG, "uvad_cuts_join: max_cuts x max_iv above 2^31 - 1");
    const size_t need = join_ws_bytes(max_cuts);
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, "uvad_cuts_join: workspace too small: need " + std::to_string(need) + " bytes");
    JoinArgs a{};
    a.table = reinterpret_cast<const CutRecord *>(d_table); a.row_first = d_row_first; a.total = d_total; a.max_cuts = max_cuts; a.B = B;
    a.iv = d_iv; a.iv_counts = d_iv_counts; a.max_iv = max_iv; a.inside = mode == UVAD_JOIN_INSIDE;
    a.pair_first = d_pair_first; a.pairs = d_pairs; a.max_pairs = max_pairs; a.item_cuts = d_item_cuts;
    a.audit = reinterpret_cast<unsigned long long *>(d_audit);
    a.counts = reinterpret_cast<int *>(d_ws);
    a.empty_first = reinterpret_cast<int *>(reinterpret_cast<char *>(d_ws) + join_counts_bytes(max_cuts));
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_cuts_join(a, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- channel fusion (fuse.hip) -----------------------------------------------------------------------------------------------------------
int uvad_fuse_configure(uvad_ctx *c, const uvad_fuse_cfg *q, const int32_t *h_first, const int32_t *h_members, const float *h_weights, int G) {
    if (!c) return UVAD_E_ARG;
    if (!q) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: cfg is NULL");
    if (!h_first) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: h_group_first is NULL");
    if (!h_members) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: h_members is NULL");
    if (G < 1) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: G must be >= 1");
    if (q->mode != UVAD_FUSE_MAX && q->mode != UVAD_FUSE_MEAN && q->mode != UVAD_FUSE_VOTE)
        return fail(c, UVAD_E_ARG, "uvad_fuse_configure: mode must be UVAD_FUSE_MAX, UVAD_FUSE_MEAN or UVAD_FUSE_VOTE");
    if (!std::isfinite(q->threshold)) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: threshold must be finite");
    if (!std::isfinite(q->decide)) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: decide must be finite");
    if (h_first[0] != 0) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: h_group_first[0] must be 0");
    for (int g = 0; g < G; ++g) {
        const long long m = (long long)h_first[g + 1] - h_first[g];
        if (m < 0) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: h_group_first must be non-decreasing (group " + std::to_string(g) + ")");
        if (m < 1 || m > FUSE_MAX_MEMBERS)
            return fail(c, UVAD_E_ARG, "uvad_fuse_configure: a group has 1 .. 255 members (group " + std::to_string(g) + " has " + std::to_string(m) + ")");
    }
    const int N = h_first[G];
    int max_member = -1;
    for (int j = 0; j < N; ++j) {
        if (h_members[j] < 0) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: a member index must be >= 0 (slot " + std::to_string(j) + ")");
        max_member = std::max(max_member, (int)h_members[j]);
    }
    if (h_weights) {
        for (int j = 0; j < N; ++j)
            if (!std::isfinite(h_weights[j]) || h_weights[j] < 0.0f)
                return fail(c, UVAD_E_ARG, "uvad_fuse_configure: every weight must be finite and >= 0 (slot " + std::to_string(j) + ")");
        for (int g = 0; g < G; ++g) {
            double sum = 0.0;
            for (int j = h_first[g]; j < h_first[g + 1]; ++j) sum += (double)h_weights[j];
            if (!(sum > 0.0)) return fail(c, UVAD_E_ARG, "uvad_fuse_configure: the weights of a group must not sum to 0 (group " + std::to_string(g) + ")");
        }
    }
    std::vector<int32_t> host((size_t)G + 1 + 2 * (size_t)N);
    std::memcpy(host.data(), h_first, ((size_t)G + 1) * sizeof(int32_t));
    std::memcpy(host.data() + G + 1, h_members, (size_t)N * sizeof(int32_t));
    if (h_weights) std::memcpy(host.data() + G + 1 + N, h_weights, (size_t)N * sizeof(float));
    const bool same = c->has_fuse && c->fz_on_device && host == c->fz_host;
    c->fz = *q; c->fz_G = G; c->fz_N = N; c->fz_max_member = max_member; c->fz_weighted = h_weights != nullptr;
    c->has_fuse = true;
    if (same) return UVAD_OK;
    c->fz_on_device = false;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->fz_cap < host.size()) {   // a larger configuration: a new buffer (the old one lives with the context: captured graphs may name it)
        void *p = nullptr;
        HIPCHK(c, hipMalloc(&p, host.size() * sizeof(int32_t)));
        c->allocs.push_back(p);
        c->d_fz = reinterpret_cast<int32_t *>(p);
        c->fz_cap = host.size();
    } else {
        HIPCHK(c, hipDeviceSynchronize());   // kernels of earlier calls may still be reading the arrays
    }
    HIPCHK(c, hipMemcpy(c->d_fz, host.data(), host.size() * sizeof(int32_t), hipMemcpyHostToDevice));
    c->fz_host.swap(host);
    c->fz_on_device = true;
    return UVAD_OK;
}

size_t uvad_fuse_ws_bytes(const uvad_ctx *c, int B, int T) {
    if (!c || !c->has_fuse || B <= c->fz_max_member || T < 1 || T > FUSE_MAX_T) return 0;
    return fuse_ws_bytes(c->fz_N, T);
}

int uvad_fuse(uvad_ctx *c, const float *d_in, int ld_in, int B, int T, const int32_t *d_lens, const uint8_t *d_flags_in, float *d_fused,
              int ld_f, int32_t *d_glens, uint8_t *d_flags_out, uint8_t *d_labels, int ld_l, uint8_t *d_best, int ld_b, uint64_t *d_stats,
              void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!c->has_fuse) return fail(c, UVAD_E_STATE, "uvad_fuse: uvad_fuse_configure has not been called");
    if (!d_in) return fail(c, UVAD_E_ARG, "uvad_fuse: d_in is NULL");
    if (!d_fused) return fail(c, UVAD_E_ARG, "uvad_fuse: d_fused is NULL");
    if (!d_glens) return fail(c, UVAD_E_ARG, "uvad_fuse: d_glens is NULL");
    if (!d_ws) return fail(c, UVAD_E_ARG, "uvad_fuse: d_ws is NULL");
    if (B <= c->fz_max_member)
        return fail(c, UVAD_E_ARG, "uvad_fuse: B must be above the largest configured member index (" + std::to_string(c->fz_max_member) + ")");
    if (T < 1 || T > FUSE_MAX_T) return fail(c, UVAD_E_ARG, "uvad_fuse: T must lie in [1, 2^30]");
    if (ld_in < T) return fail(c, UVAD_E_ARG, "uvad_fuse: ld_in must be at least T");
    if (ld_f < T) return fail(c, UVAD_E_ARG, "uvad_fuse: ld_f must be at least T");
    if (d_labels && ld_l < T) return fail(c, UVAD_E_ARG, "uvad_fuse: ld_l must be at least T");
    if (d_best && ld_b < T) return fail(c, UVAD_E_ARG, "uvad_fuse: ld_b must be at least T");
    if ((d_flags_in == nullptr) != (d_flags_out == nullptr))
        return fail(c, UVAD_E_ARG, "uvad_fuse: d_flags_in and d_flags_out go together: give both or neither");
    const size_t need = fuse_ws_bytes(c->fz_N, T);
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, "uvad_fuse: workspace too small: need " + std::to_string(need) + " bytes");
    if (!c->fz_on_device) return fail(c, UVAD_E_HIP, "uvad_fuse: the configuration is not on the device (uvad_fuse_configure's upload failed)");
    FuseArgs a{};
    a.first = c->d_fz; a.members = c->d_fz + c->fz_G + 1; a.G = c->fz_G; a.N = c->fz_N;
    a.weights = c->fz_weighted ? reinterpret_cast<const float *>(c->d_fz + c->fz_G + 1 + c->fz_N) : nullptr;
    a.q = FuseCfgInt{c->fz.mode, c->fz.threshold, c->fz.decide};
    a.in = d_in; a.ld_in = ld_in; a.T = T; a.lens = d_lens; a.flags_in = d_flags_in;
    a.fused = d_fused; a.ld_f = ld_f; a.glens = d_glens; a.flags_out = d_flags_out; a.labels = d_labels; a.ld_l = ld_l;
    a.best = d_best; a.ld_b = ld_b; a.stats = reinterpret_cast<unsigned long long *>(d_stats);
    a.part = reinterpret_cast<FusePartial *>(d_ws); a.tiles = fuse_tiles(T);
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_fuse(a, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_fuse_pick(uvad_ctx *c, const uint8_t *d_best, int ld_b, const uvad_cut *d_table, const int32_t *d_total, int max_cuts,
                   uvad_cut *d_out_table, int32_t *d_pick, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!c->has_fuse) return fail(c, UVAD_E_STATE, "uvad_fuse_pick: uvad_fuse_configure has not been called");
    if (!d_best) return fail(c, UVAD_E_ARG, "uvad_fuse_pick: d_best is NULL");
    if (!d_total) return fail(c, UVAD_E_ARG, "uvad_fuse_pick: d_total is NULL");
    if (max_cuts < 0) return fail(c, UVAD_E_ARG, "uvad_fuse_pick: max_cuts must be >= 0");
    if (max_cuts > 0 && !d_table) return fail(c, UVAD_E_ARG, "uvad_fuse_pick: d_table is NULL with max_cuts > 0");
    if (!d_out_table && !d_pick) return fail(c, UVAD_E_ARG, "uvad_fuse_pick: d_out_table and d_pick are both NULL");
    if (ld_b < 1) return fail(c, UVAD_E_ARG, "uvad_fuse_pick: ld_b must be >= 1");
    if (!c->fz_on_device) return fail(c, UVAD_E_HIP, "uvad_fuse_pick: the configuration is not on the device (uvad_fuse_configure's upload failed)");
    FusePickArgs a{};
    a.first = c->d_fz; a.members = c->d_fz + c->fz_G + 1; a.G = c->fz_G;
    a.best = d_best; a.ld_b = ld_b; a.table = reinterpret_cast<const CutRecord *>(d_table); a.total = d_total; a.max_cuts = max_cuts;
    a.out_table = reinterpret_cast<CutRecord *>(d_out_table); a.pick = d_pick;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_fuse_pick(a, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- hysteresis decisions with minimum durations (binarize.hip) ---------------------------------------------------------------------------
// nullptr: the configuration is in range; else the word uvad_last_error names
static const char *binarize_cfg_error(const uvad_binarize_cfg *q) {
    if (!q) return "cfg is NULL";
    if (!std::isfinite(q->onset)) return "onset must be finite";
    if (!std::isfinite(q->offset)) return "offset must be finite";
    if (q->offset > q->onset) return "offset must be <= onset";
    if (q->min_on < 0 || q->min_on > BIN_MAX_FRAMES) return "min_on must lie in [0, 2^20] frames";
    if (q->min_off < 0 || q->min_off > BIN_MAX_FRAMES) return "min_off must lie in [0, 2^20] frames";
    if (q->pad_on < 0 || q->pad_on > BIN_MAX_FRAMES) return "pad_on must lie in [0, 2^20] frames";
    if (q->pad_off < 0 || q->pad_off > BIN_MAX_FRAMES) return "pad_off must lie in [0, 2^20] frames";
    return nullptr;
}

size_t uvad_binarize_ws_bytes(const uvad_ctx *c, int B, int T) {
    if (!c || B < 1 || T < 1 || T > BIN_MAX_T) return 0;
    return bin_ws_bytes(B, T);
}

int uvad_binarize(uvad_ctx *c, const float *d_probs, int ld_p, int B, int T, const int32_t *d_lens, const uvad_binarize_cfg *q,
                  uint8_t *d_labels, int ld, int32_t *d_iv, int max_iv, int32_t *d_iv_counts, void *d_ws, size_t ws_bytes, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (const char *w = binarize_cfg_error(q)) return fail(c, UVAD_E_ARG, std::string("uvad_binarize: ") + w);
    if (B < 1) return fail(c, UVAD_E_ARG, "uvad_binarize: B must be >= 1");
    if (T < 1 || T > BIN_MAX_T) return fail(c, UVAD_E_ARG, "uvad_binarize: T must lie in [1, 2^30]");
    if (ld_p < T) return fail(c, UVAD_E_ARG, "uvad_binarize: ld_p must be at least T");
    if (d_labels && ld < T) return fail(c, UVAD_E_ARG, "uvad_binarize: ld must be at least T");
    if (max_iv < 0) return fail(c, UVAD_E_ARG, "uvad_binarize: max_iv must be >= 0");
    if (!d_probs) return fail(c, UVAD_E_ARG, "uvad_binarize: d_probs is NULL");
    if (!d_iv_counts) return fail(c, UVAD_E_ARG, "uvad_binarize: d_iv_counts is NULL");
    if (!d_ws) return fail(c, UVAD_E_ARG, "uvad_binarize: d_ws is NULL");
    if (reinterpret_cast<uintptr_t>(d_ws) % 16) return fail(c, UVAD_E_ARG, "uvad_binarize: d_ws must be 16-byte aligned");
    if (max_iv > 0 && !d_iv) return fail(c, UVAD_E_ARG, "uvad_binarize: d_iv is NULL with max_iv > 0");
    if ((long long)B * ((T + BIN_SEG - 1) / BIN_SEG) > 0x7fffffffll) return fail(c, UVAD_E_ARG, "uvad_binarize: B x segments above 2^31 - 1");
    const size_t need = bin_ws_bytes(B, T);
    if (ws_bytes < need) return fail(c, UVAD_E_ARG, "uvad_binarize: workspace too small: need " + std::to_string(need) + " bytes");
    BinarizeArgs a{};
    a.probs = d_probs; a.ld_p = ld_p; a.B = B; a.T = T; a.lens = d_lens;
    a.q = BinCfgInt{q->onset, q->offset, q->min_on, q->min_off, q->pad_on, q->pad_off};
    a.iv = d_iv; a.max_iv = max_iv; a.iv_counts = d_iv_counts;
    a.words = reinterpret_cast<unsigned long long *>(d_ws);
    a.list = reinterpret_cast<int *>(reinterpret_cast<char *>(d_ws) + bin_words_bytes(B, T));
    a.nwt = bin_words(T); a.cap = (T + 1) / 2;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_binarize(a, d_labels, ld, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- the live hysteresis endpointer (endpoint_hyst.hip) --------------------------------------------------------------------------------------
static int endpoint_hyst_lag(const uvad_binarize_cfg *q) {
    return q->min_on + q->pad_on + q->pad_off + (q->min_off > 1 ? q->min_off - 1 : 0);   // at most 4 x 2^20
}

int uvad_endpoint_hyst_lag(const uvad_binarize_cfg *q) { return binarize_cfg_error(q) ? -1 : endpoint_hyst_lag(q); }

size_t uvad_endpoint_hyst_state_bytes(const uvad_ctx *c, int B, const uvad_binarize_cfg *q) {
    if (!c || B < 1 || binarize_cfg_error(q)) return 0;
    return endpoint_hyst_state_bytes(B);
}

int uvad_endpoint_hyst_reset(uvad_ctx *c, void *d_state, size_t state_bytes, int B, const uvad_binarize_cfg *q, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (const char *w = binarize_cfg_error(q)) return fail(c, UVAD_E_ARG, std::string("uvad_endpoint_hyst_reset: ") + w);
    if (!d_state || B < 1) return fail(c, UVAD_E_ARG, "uvad_endpoint_hyst_reset: bad argument");
    if (state_bytes < endpoint_hyst_state_bytes(B))
        return fail(c, UVAD_E_ARG, "uvad_endpoint_hyst_reset: state too small: need " + std::to_string(endpoint_hyst_state_bytes(B)) + " bytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_endpoint_hyst_reset(d_state, B, BinCfgInt{q->onset, q->offset, q->min_on, q->min_off, q->pad_on, q->pad_off},
                                         (hipStream_t)stream));
    EndpointHystPool g;
    g.B = B; g.lag = endpoint_hyst_lag(q);
    c->endpoint_hysts[d_state] = g;
    return UVAD_OK;
}

int uvad_endpoint_hyst_step(uvad_ctx *c, const float *d_probs, int ld_in, const int32_t *d_counts, const uint8_t *d_flags, int B,
                            void *d_state, size_t state_bytes, int32_t *d_events, int max_events, int32_t *d_ev_counts, uint8_t *d_active,
                            uint8_t *d_labels, int ld_lab, int32_t *d_lab_counts, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!d_probs || !d_counts || !d_ev_counts || !d_state || B < 1 || ld_in < 1) return fail(c, UVAD_E_ARG, "uvad_endpoint_hyst_step: bad argument");
    if (ld_in > EP_MAX_LD_IN) return fail(c, UVAD_E_ARG, "uvad_endpoint_hyst_step: ld_in above " + std::to_string(EP_MAX_LD_IN) + " frames per step");
    if (max_events < 0 || (max_events > 0 && !d_events)) return fail(c, UVAD_E_ARG, "uvad_endpoint_hyst_step: d_events is NULL with max_events > 0");
    if (d_labels && !d_lab_counts) return fail(c, UVAD_E_ARG, "uvad_endpoint_hyst_step: d_labels needs d_lab_counts");
    auto it = c->endpoint_hysts.find(d_state);
    if (it == c->endpoint_hysts.end()) return fail(c, UVAD_E_STATE, "uvad_endpoint_hyst_step: call uvad_endpoint_hyst_reset on this state first");
    const EndpointHystPool &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_STATE, "uvad_endpoint_hyst_step: the state was reset with B = " + std::to_string(g.B));
    if (state_bytes < endpoint_hyst_state_bytes(B))
        return fail(c, UVAD_E_ARG, "uvad_endpoint_hyst_step: state too small: need " + std::to_string(endpoint_hyst_state_bytes(B)) + " bytes");
    if (d_labels && (int64_t)ld_lab < (int64_t)ld_in + g.lag)
        return fail(c, UVAD_E_ARG, "uvad_endpoint_hyst_step: ld_lab must be at least ld_in + lag = " + std::to_string((int64_t)ld_in + g.lag));
    EndpointArgs a{};
    a.probs = d_probs; a.ld_in = ld_in; a.counts = d_counts; a.flags = d_flags; a.B = B; a.state = d_state;
    a.events = d_events; a.max_events = max_events; a.ev_counts = d_ev_counts; a.active = d_active;
    a.labels = d_labels; a.ld_lab = ld_lab; a.lab_counts = d_lab_counts;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_endpoint_hyst_step(a, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- the live speech gate (gate.hip) ---------------------------------------------------------------------------------------------------------
// nullptr: a configuration the gate takes; else the word uvad_last_error names
static const char *gate_cfg_error(const uvad_cuts_cfg *q) {
    if (const char *w = cuts_cfg_error(q)) return w;
    if (q->min_len != 0) return "min_len must be 0: the gate drops no short last piece";
    return nullptr;
}
static const char *gate_size_error(int B, int unit_bytes, int64_t history) {
    if (B < 1) return "B must be >= 1";
    if (unit_bytes != 2 && unit_bytes != 4) return "unit_bytes must be 2 (int16) or 4 (f32)";
    if (history < 1 || history > 0x7fffffffll) return "history must lie in [1, 2^31 - 1] samples";
    return nullptr;
}
// the intervals a step of ld_lab labels can touch: the one it found open and one per run that starts in it
static int64_t gate_intervals(int ld_lab) { return ((int64_t)ld_lab + 1) / 2 + 1; }
static int64_t gate_max_seg(const uvad_cuts_cfg *q, int ld_lab) {
    const int64_t I = gate_intervals(ld_lab);
    return 2 * I + 1 + (q->max_len ? ((int64_t)ld_lab + 2 * (int64_t)q->pad * I) / q->max_len : 0);   // below 2^54
}

// the argument checks uvad_gate_step and uvad_gate_group_step share, in the order both report them: the chunk's range, the signs of the
// leading dimensions and of max_seg, then the NULL pairs.  fn: the entry point's name, which every message starts with.  The mono gate has
// no best bytes: it passes ld_best = 0, so that their checks never fire.  -> UVAD_OK, or what fail() returned
static int gate_step_args_error(uvad_ctx *c, const char *fn, int chunk, int ld_lab, int ld_best, int64_t ld_out, int max_seg, const void *d_chunk,
                                const void *d_state, const void *d_seg_counts, const void *d_labels, const void *d_lab_counts, const void *d_best,
                                const void *d_best_counts, const void *d_out, const void *d_seg) {
    const char *w = nullptr;
    if (chunk < 1 || chunk > GATE_MAX_CHUNK) w = "chunk must lie in [1, 2^24] samples";
    else if (ld_lab < 0) w = "ld_lab must be >= 0";
    else if (ld_best < 0) w = "ld_best must be >= 0";
    else if (ld_out < 0) w = "ld_out must be >= 0";
    else if (max_seg < 0) w = "max_seg must be >= 0";
    else if (!d_chunk) w = "d_chunk is NULL";
    else if (!d_state) w = "d_state is NULL";
    else if (!d_seg_counts) w = "d_seg_counts is NULL";
    else if (ld_lab > 0 && !d_labels) w = "d_labels is NULL with ld_lab > 0";
    else if (ld_lab > 0 && !d_lab_counts) w = "d_lab_counts is NULL with ld_lab > 0";
    else if (ld_best > 0 && !d_best) w = "d_best is NULL with ld_best > 0";
    else if (ld_best > 0 && !d_best_counts) w = "d_best_counts is NULL with ld_best > 0";
    else if (ld_out > 0 && !d_out) w = "d_out is NULL with ld_out > 0";
    else if (max_seg > 0 && !d_seg) w = "d_seg is NULL with max_seg > 0";
    return w ? fail(c, UVAD_E_ARG, std::string(fn) + ": " + w) : UVAD_OK;
}

int64_t uvad_gate_history(const uvad_cuts_cfg *q, int lag_frames, int chunk) {
    if (gate_cfg_error(q) || lag_frames < 0 || chunk < 1 || chunk > GATE_MAX_CHUNK) return -1;
    return (int64_t)chunk + ((int64_t)lag_frames + q->pad + 1) * q->hop + q->lead;   // below 2^63: (2^31 + 2^20 + 1) 2^31 + 2^31 + 2^24
}

int uvad_gate_max_seg(const uvad_cuts_cfg *q, int ld_lab) {
    if (gate_cfg_error(q) || ld_lab < 0) return -1;
    return (int)std::min<int64_t>(gate_max_seg(q, ld_lab), 0x7fffffffll);
}

int64_t uvad_gate_max_out(const uvad_cuts_cfg *q, int ld_lab, int chunk, int64_t history) {
    if (gate_cfg_error(q) || ld_lab < 0 || chunk < 1 || chunk > GATE_MAX_CHUNK || history < chunk || history > 0x7fffffffll) return -1;
    const double est = (double)chunk + ((double)ld_lab + 2.0 * q->pad * (double)gate_intervals(ld_lab)) * q->hop +
                       (double)gate_max_seg(q, ld_lab) * ((double)q->lead + q->tail);
    if (est > 9.0e18) return INT64_MAX;                                             // saturates
    return (int64_t)chunk + ((int64_t)ld_lab + 2 * (int64_t)q->pad * gate_intervals(ld_lab)) * q->hop +
           gate_max_seg(q, ld_lab) * ((int64_t)q->lead + q->tail);
}

size_t uvad_gate_state_bytes(const uvad_ctx *c, int B, const uvad_cuts_cfg *q, int unit_bytes, int64_t history) {
    if (!c || gate_cfg_error(q) || gate_size_error(B, unit_bytes, history)) return 0;
    return gate_state_bytes(B, unit_bytes, history);
}

int uvad_gate_reset(uvad_ctx *c, void *d_state, size_t state_bytes, int B, const uvad_cuts_cfg *q, int unit_bytes, int64_t history,
                    void *stream) {
    if (!c) return UVAD_E_ARG;
    if (const char *w = gate_cfg_error(q)) return fail(c, UVAD_E_ARG, std::string("uvad_gate_reset: ") + w);
    if (const char *w = gate_size_error(B, unit_bytes, history)) return fail(c, UVAD_E_ARG, std::string("uvad_gate_reset: ") + w);
    if (!d_state) return fail(c, UVAD_E_ARG, "uvad_gate_reset: d_state is NULL");
    const size_t need = gate_state_bytes(B, unit_bytes, history);
    if (state_bytes < need) return fail(c, UVAD_E_ARG, "uvad_gate_reset: state_bytes too small: need " + std::to_string(need) + " bytes");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_gate_reset(d_state, B, cuts_cfg_of(q), unit_bytes, (int)history, (hipStream_t)stream));
    GatePool g;
    g.B = B; g.unit_bytes = unit_bytes; g.history = (int)history;
    c->gates[d_state] = g;
    return UVAD_OK;
}

int uvad_gate_step(uvad_ctx *c, const void *d_chunk, int chunk, const uint8_t *d_labels, int ld_lab, const int32_t *d_lab_counts,
                   const uint8_t *d_flags, int B, void *d_state, size_t state_bytes, void *d_out, int64_t ld_out, uvad_gate_seg *d_seg,
                   int max_seg, int32_t *d_seg_counts, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (B < 1) return fail(c, UVAD_E_ARG, "uvad_gate_step: B must be >= 1");
    if (const int e = gate_step_args_error(c, "uvad_gate_step", chunk, ld_lab, 0, ld_out, max_seg, d_chunk, d_state, d_seg_counts, d_labels, d_lab_counts,
                                           nullptr, nullptr, d_out, d_seg))
        return e;
    auto it = c->gates.find(d_state);
    if (it == c->gates.end()) return fail(c, UVAD_E_STATE, "uvad_gate_step: call uvad_gate_reset on this state first");
    const GatePool &g = it->second;
    if (B != g.B) return fail(c, UVAD_E_STATE, "uvad_gate_step: the state was reset with B = " + std::to_string(g.B));
    if (g.history < chunk) return fail(c, UVAD_E_ARG, "uvad_gate_step: history " + std::to_string(g.history) + " is below chunk");
    const size_t need = gate_state_bytes(B, g.unit_bytes, g.history);
    if (state_bytes < need) return fail(c, UVAD_E_ARG, "uvad_gate_step: state_bytes too small: need " + std::to_string(need) + " bytes");
    GateArgs a{};
    a.chunk = d_chunk; a.chunk_n = chunk; a.labels = d_labels; a.ld_lab = ld_lab; a.lab_counts = d_lab_counts; a.flags = d_flags; a.B = B;
    a.state = d_state; a.out = d_out; a.ld_out = ld_out; a.seg = reinterpret_cast<GateSeg *>(d_seg); a.max_seg = max_seg;
    a.seg_counts = d_seg_counts;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_gate_step(a, g.unit_bytes, (hipStream_t)stream));
    return UVAD_OK;
}

// ---- the live speech gate for fused groups (gate_group.hip) ------------------------------------------------------------------------------------
static bool gate_group_args_ok(const uvad_cuts_cfg *q, int lag_frames, int chunk, int decide) {
    return !gate_cfg_error(q) && lag_frames >= 0 && chunk >= 1 && chunk <= GATE_MAX_CHUNK && decide >= 1 && decide <= CUTS_MAX_LEN;
}
static const char *gate_group_size_error(int unit_bytes, int64_t history, int64_t best_history) {
    if (const char *w = gate_size_error(1, unit_bytes, history)) return w;
    if (best_history < 1 || best_history > 0x7fffffffll) return "best_history must lie in [1, 2^31 - 1] frames";
    return nullptr;
}

int64_t uvad_gate_group_history(const uvad_cuts_cfg *q, int lag_frames, int chunk, int decide) {
    if (!gate_group_args_ok(q, lag_frames, chunk, decide)) return -1;
    return (int64_t)chunk + ((int64_t)lag_frames + q->pad + decide) * q->hop + q->lead;   // below 2^63, as uvad_gate_history
}

int uvad_gate_group_best_history(const uvad_cuts_cfg *q, int lag_frames, int chunk, int decide) {
    if (!gate_group_args_ok(q, lag_frames, chunk, decide)) return -1;
    const int64_t v = ((int64_t)chunk + q->hop - 1) / q->hop + lag_frames + q->pad + decide;
    return v > 0x7fffffffll ? -1 : (int)v;
}

int64_t uvad_gate_group_max_out(const uvad_cuts_cfg *q, int ld_lab, int chunk, int decide) {
    if (gate_cfg_error(q) || decide < 1 || decide > CUTS_MAX_LEN) return -1;
    const int64_t base = uvad_gate_max_out(q, ld_lab, chunk, chunk);   // it does not depend on the history, which is only checked
    if (base < 0) return -1;
    const int64_t extra = (int64_t)decide * q->hop;                    // below 2^55
    return base > INT64_MAX - extra ? INT64_MAX : base + extra;
}

size_t uvad_gate_group_state_bytes(const uvad_ctx *c, const uvad_cuts_cfg *q, int unit_bytes, int64_t history, int best_history) {
    if (!c || !c->has_fuse || gate_cfg_error(q) || gate_group_size_error(unit_bytes, history, best_history)) return 0;
    return gate_group_state_bytes(c->fz_G, c->fz_N, unit_bytes, history, best_history);
}

int uvad_gate_group_reset(uvad_ctx *c, void *d_state, size_t state_bytes, const uvad_cuts_cfg *q, int unit_bytes, int64_t history,
                          int best_history, int decide, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!c->has_fuse) return fail(c, UVAD_E_STATE, "uvad_gate_group_reset: uvad_fuse_configure has not been called");
    if (const char *w = gate_cfg_error(q)) return fail(c, UVAD_E_ARG, std::string("uvad_gate_group_reset: ") + w);
    if (const char *w = gate_group_size_error(unit_bytes, history, best_history)) return fail(c, UVAD_E_ARG, std::string("uvad_gate_group_reset: ") + w);
    if (decide < 1 || decide > CUTS_MAX_LEN) return fail(c, UVAD_E_ARG, "uvad_gate_group_reset: decide_frames must lie in [1, 2^24] frames");
    if (!d_state) return fail(c, UVAD_E_ARG, "uvad_gate_group_reset: d_state is NULL");
    const size_t need = gate_group_state_bytes(c->fz_G, c->fz_N, unit_bytes, history, best_history);
    if (state_bytes < need) return fail(c, UVAD_E_ARG, "uvad_gate_group_reset: state_bytes too small: need " + std::to_string(need) + " bytes");
    if (!c->fz_on_device)
        return fail(c, UVAD_E_HIP, "uvad_gate_group_reset: the configuration is not on the device (uvad_fuse_configure's upload failed)");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_gate_group_reset(d_state, c->fz_G, c->fz_N, cuts_cfg_of(q), unit_bytes, (int)history, best_history, decide, (hipStream_t)stream));
    GateGroupPool g;
    g.G = c->fz_G; g.N = c->fz_N; g.unit_bytes = unit_bytes; g.history = (int)history; g.best_history = best_history;
    c->gate_groups[d_state] = g;
    return UVAD_OK;
}

int uvad_gate_group_step(uvad_ctx *c, const void *d_chunk, int chunk, int B, const uint8_t *d_best, int ld_best, const int32_t *d_best_counts,
                         const uint8_t *d_labels, int ld_lab, const int32_t *d_lab_counts, const uint8_t *d_gflags, const uint8_t *d_rflags,
                         void *d_state, size_t state_bytes, void *d_out, int64_t ld_out, uvad_gate_seg *d_seg, int max_seg,
                         int32_t *d_seg_counts, void *stream) {
    if (!c) return UVAD_E_ARG;
    if (!c->has_fuse) return fail(c, UVAD_E_STATE, "uvad_gate_group_step: uvad_fuse_configure has not been called");
    if (B <= c->fz_max_member)
        return fail(c, UVAD_E_ARG, "uvad_gate_group_step: B must be above the largest configured member index (" + std::to_string(c->fz_max_member) + ")");
    if (const int e = gate_step_args_error(c, "uvad_gate_group_step", chunk, ld_lab, ld_best, ld_out, max_seg, d_chunk, d_state, d_seg_counts, d_labels,
                                           d_lab_counts, d_best, d_best_counts, d_out, d_seg))
        return e;
    auto it = c->gate_groups.find(d_state);
    if (it == c->gate_groups.end()) return fail(c, UVAD_E_STATE, "uvad_gate_group_step: call uvad_gate_group_reset on this state first");
    const GateGroupPool &g = it->second;
    if (g.G != c->fz_G || g.N != c->fz_N)
        return fail(c, UVAD_E_STATE, "uvad_gate_group_step: the state was reset under a configuration of G = " + std::to_string(g.G) + ", N = " +
                                         std::to_string(g.N));
    if (g.history < chunk) return fail(c, UVAD_E_ARG, "uvad_gate_group_step: history " + std::to_string(g.history) + " is below chunk");
    const size_t need = gate_group_state_bytes(g.G, g.N, g.unit_bytes, g.history, g.best_history);
    if (state_bytes < need) return fail(c, UVAD_E_ARG, "uvad_gate_group_step: state_bytes too small: need " + std::to_string(need) + " bytes");
    if (!c->fz_on_device)
        return fail(c, UVAD_E_HIP, "uvad_gate_group_step: the configuration is not on the device (uvad_fuse_configure's upload failed)");
    GateGroupArgs a{};
    a.first = c->d_fz; a.members = c->d_fz + c->fz_G + 1; a.G = c->fz_G; a.N = c->fz_N;
    a.chunk = d_chunk; a.chunk_n = chunk; a.B = B; a.best = d_best; a.ld_best = ld_best; a.best_counts = d_best_counts;
    a.labels = d_labels; a.ld_lab = ld_lab; a.lab_counts = d_lab_counts; a.gflags = d_gflags; a.rflags = d_rflags;
    a.state = d_state; a.out = d_out; a.ld_out = ld_out; a.seg = reinterpret_cast<GateSeg *>(d_seg); a.max_seg = max_seg;
    a.seg_counts = d_seg_counts;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, launch_gate_group_step(a, g.unit_bytes, (hipStream_t)stream));
    return UVAD_OK;
}

int uvad_set_gemm_mode(uvad_ctx *c, int mode) {
    if (!c) return UVAD_E_ARG;
    if (mode < 0 || mode > 3)
        return fail(c, UVAD_E_ARG, "gemm mode must be 0 (exact f32 MFMA), 1 (split f16, 4 products), 2 (the same, tile-streaming kernels only) or 3 (split f16, 3 products)");
    c->gemm_mode = mode;
    return UVAD_OK;
}

int uvad_set_recurrent_tile(uvad_ctx *c, int sequences) {
    if (!c) return UVAD_E_ARG;
    if (sequences != 0 && sequences != 4 && sequences != 16) return fail(c, UVAD_E_ARG, "recurrent tile must be 0 (by batch size), 4 or 16 sequences per workgroup");
    if (sequences == 16 && c->has_model && c->mc.hidden != 128) return fail(c, UVAD_E_UNSUPPORTED, "the 16-sequence recurrent kernel exists for hidden_size 128 only");
    c->rec_tile_mode = sequences;
    return UVAD_OK;
}

int uvad_get_recurrent_tile(const uvad_ctx *c) { return c ? c->rec_tile_used : UVAD_E_ARG; }
int uvad_weights_shared_by(const uvad_ctx *c) {
    if (!c) return UVAD_E_ARG;
    return c->packed ? (int)c->packed.use_count() : 0;
}

int uvad_get_sincnet_form(const uvad_ctx *c) {
    if (!c) return UVAD_E_ARG;
    return c->sinc_f16_used ? 1 : 0;
}

int uvad_get_p2_on_fp8(const uvad_ctx *c) {
    if (!c) return UVAD_E_ARG;
    if (!c->has_model || !c->finalized || c->mc.hidden != 128 || c->gemm_mode == 2) return 0;
    for (const LayerDev &L : c->packed->layers)
        if (!L.w_hh16_ok || !L.w_hh16_p2q) return 0;
    return 1;
}

int uvad_set_time_chunks(uvad_ctx *c, int chunks) {
    if (!c) return UVAD_E_ARG;
    if (chunks < 0 || chunks > 64) return fail(c, UVAD_E_ARG, "time chunks must be 0 (automatic), 1 (off) or 2 .. 64");
    c->chunk_mode = chunks;
    return UVAD_OK;
}

int uvad_get_time_chunks(const uvad_ctx *c) { return c ? c->chunks_used : UVAD_E_ARG; }

int uvad_set_concurrent_steps(uvad_ctx *c, int n) {
    if (!c) return UVAD_E_ARG;
    if (n < 1) return fail(c, UVAD_E_ARG, "concurrent steps must be 1 (this context's calls run alone) or more");
    c->concurrent_steps = n;
    return UVAD_OK;
}

int uvad_get_concurrent_steps(const uvad_ctx *c) { return c ? c->concurrent_steps : UVAD_E_ARG; }
int uvad_get_projection_grid(const uvad_ctx *c) { return c ? c->proj_grid_used : UVAD_E_ARG; }

int uvad_recurrent_tile_for(const uvad_ctx *c, int B) {
    if (!c || !c->has_model || B <= 0) return UVAD_E_ARG;
    return lstm_auto_tile((B + SEQ_TILE - 1) / SEQ_TILE, c->mc.bidirectional ? 2 : 1, c->mc.hidden, c->n_cu);
}

int uvad_streams_overlap(uvad_ctx *c, void *stream_a, void *stream_b) {
    if (!c) return UVAD_E_ARG;
    if (stream_a == stream_b) return 0;
    HIPCHK(c, hipSetDevice(c->device));
    const int result = streams_overlap_probe((hipStream_t)stream_a, (hipStream_t)stream_b);   // (the probe of the time-chunked layers, above)
    if (result < 0) return fail(c, UVAD_E_HIP, "uvad_streams_overlap: HIP error while probing");
    return result;
}

int uvad_set_timing(uvad_ctx *c, int enabled) {
    if (!c) return UVAD_E_ARG;
    c->timing = enabled != 0;
    c->ev_valid = false;
    return UVAD_OK;
}

int uvad_get_timing(uvad_ctx *c, float ms[5]) {
    if (!c || !ms) return UVAD_E_ARG;
    if (!c->ev_valid) return fail(c, UVAD_E_STATE, "no timed call recorded");
    HIPCHK(c, hipEventSynchronize(c->ev[3]));
    const int L = c->mc.num_layers;
    float fb = 0.f, proj = 0.f, rec = 0.f, head = 0.f, total = 0.f, t = 0.f;
    HIPCHK(c, hipEventElapsedTime(&fb, c->ev[0], c->ev[1]));
    for (int k = 0; k < L; ++k) {
        HIPCHK(c, hipEventElapsedTime(&t, c->layer_ev[2 * k], c->layer_ev[2 * k + 1]));
        proj += t;
        HIPCHK(c, hipEventElapsedTime(&t, c->layer_ev[2 * k + 1], c->layer_ev[2 * k + 2]));
        rec += t;
    }
    HIPCHK(c, hipEventElapsedTime(&head, c->ev[2], c->ev[3]));
    HIPCHK(c, hipEventElapsedTime(&total, c->ev[0], c->ev[3]));
    ms[0] = fb; ms[1] = proj; ms[2] = rec; ms[3] = head; ms[4] = total;
    return UVAD_OK;
}

int uvad_get_layer_timing(uvad_ctx *c, float *ms, int n) {
    if (!c || !ms) return UVAD_E_ARG;
    if (!c->ev_valid) return fail(c, UVAD_E_STATE, "no timed call recorded");
    const int L = c->mc.num_layers;
    if (n < 2 * L) return fail(c, UVAD_E_ARG, "uvad_get_layer_timing: ms holds fewer than 2 * num_layers floats");
    HIPCHK(c, hipEventSynchronize(c->ev[3]));
    for (int k = 0; k < 2 * L; ++k) HIPCHK(c, hipEventElapsedTime(&ms[k], c->layer_ev[k], c->layer_ev[k + 1]));
    return 2 * L;
}

const char *uvad_last_error(const uvad_ctx *c) { return c ? c->err.c_str() : "null context"; }

void uvad_destroy(uvad_ctx *c) {
    if (!c) return;
    if (!c->allocs.empty() || c->packed || c->ev[0]) (void)hipSetDevice(c->device);
    free_weights(c);
    for (void *p : c->allocs) (void)hipFree(p);
    for (auto &ev : c->ev)
        if (ev) (void)hipEventDestroy(ev);
    for (auto &kv : c->chunk_plans)
        if (kv.second.d_list) (void)hipFree(kv.second.d_list);
    for (auto &ev : c->ev_chunk) (void)hipEventDestroy(ev);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->side) (void)hipStreamDestroy(c->side);
    delete c;
}

}  // extern "C"
