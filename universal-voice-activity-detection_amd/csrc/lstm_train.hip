// lstm_train.hip -- training of the top layers of the LSTM stack (uvad_lstm_train_*, include/uvad.h): the backward pass that
// uvad_head_train_grad's d_grad_x starts, through nn.LSTM with pack_padded_sequence rows (gate order i, f, g, o, zero initial state, the
// backward direction starting at len_b - 1), and torch.optim.Adam on its tensors: the recurrent part of VadModel.training_step /
// configure_optimizers of src/engines/vad_engine.py.  Layers below first_layer stay frozen and are not touched here.
//
// Frames are flat (n = b T + t, N = B T).  Per trainable layer, bottom to top in the forward call and top to bottom in the backward call:
//   lt_prep_kernel        valid[n] = t < len_b, b_ih + b_hh of every (layer, direction), and the workspace header (magic, B, T)
//   ht_gemm_kernel<0>     the gate pre-activations x W_ih^T + (b_ih + b_hh) of one direction, [N][4H]         (ht_kernels.h: exact f32 on
//                         v_mfma_f32_32x32x2_f32, shared with head_train.hip; slope 1 makes its epilogue the identity)
//   lt_fwd_kernel<H>      the recurrence with kept activations: 4 sequences of one direction per workgroup, W_hh resident in registers as
//                         the A operand of v_mfma_f32_4x4x1_16B_f32 (block = hidden unit, A rows = its 4 gates, B = h_{t-1} of the 4
//                         sequences), h exchanged through a double-buffered LDS tile, the gates prefetched LT_PD steps ahead, the 1-ulp
//                         sigmoid_f / tanh_f of lstm.hip restated.  It overwrites the pre-activations with i, f, g, o, keeps c_t and
//                         h_{t-1} (in the direction's own order: +0 at its first step) and writes h_t; +0 past a length.
//   lt_bwd_kernel<H>      the backward recurrence of the same 4 sequences, W_hh resident in the OTHER operand order: a wave owns one gate's
//                         H rows of W_hh and 64 output units -- A rows = 4 output units, block = group of 4 units, B = that gate's dpre of
//                         the 4 sequences broadcast from LDS -- so the 4H-deep chain of dh_rec = dpre W_hh is split by gate across the
//                         wave groups and the four partials are summed through LDS in gate order.  The elementwise half (one thread per
//                         (sequence, unit)) forms dh = dy_t + dh_rec, dc, the four dpre, and writes dpre over the kept gates; +0 past a
//                         length and for the steps the workgroup does not run.
//   ht_gemm_kernel<2>     dW_ih = sum dpre^T x and dW_hh = sum dpre^T h_prev per segment of frames; the bias partial rides along in both, which
//                         is how bias_ih and bias_hh receive the same bits
//   ht_gemm_kernel<1>     d_in = dpre W_ih, the second direction added to the first: the next lower layer's dy, or d_grad_in
//   ht_fold_kernel        as the head's; Adam, the read-out and the write are launch_train_apply / _read / _write of optim.hip
// Dropout between the trainable layers (uvad_lstm_train_set_dropout; the mask is defined in include/uvad.h) is a stage of its own:
//   lt_dropout_kernel     out = keep ? x scale : +0, one thread per group of four columns of one frame: one Philox4x32-10 call, one 16-byte
//                         load, one 16-byte store.  In place over h[li] after layer li's forward recurrence and over the gradient buffer
//                         before layer li's backward recurrence, with draw / thr / scale / seed read from the workspace header, where
//                         lt_prep_kernel recorded them when it took the draw ordinal from the state.  With the setting off the host
//                         launches none of it and lt_prep_kernel writes only thr = 0 into that record.
// No floating-point atomics: the same calls give the same bits.  Every backward kernel checks the workspace header on the device and does
// nothing under a mismatch.  Contraction is off (ht_kernels.h and the Makefile's flag); the fused multiply-adds below are explicit.
#include "ht_kernels.h"
#include "philox.h"

namespace uvad {

static_assert(sizeof(LstmTrainWsHead) == 256, "workspace layout");
static_assert(offsetof(HeadTrainHeader, draws) == 56, "the draw ordinal of include/uvad.h");
static_assert(offsetof(LstmTrainWsHead, draw) == 16 && offsetof(LstmTrainWsHead, thr) == 24 && offsetof(LstmTrainWsHead, scale) == 28 &&
              offsetof(LstmTrainWsHead, seed) == 32, "the dropout record of include/uvad.h");

namespace {

using f32x4 = __attribute__((ext_vector_type(4))) float;

constexpr int LT_PD = 4;   // gate prefetch depth of the forward recurrence (steps)
constexpr float LT_L2E = 1.4426950408889634f;

// lstm.hip's gate functions, restated: v_exp_f32 + v_rcp_f32 refined by one Newton step, ~1 ulp at the output scale
__device__ __forceinline__ float lt_rcp_nr(float d) {
    const float r = __builtin_amdgcn_rcpf(d);
    return __builtin_fmaf(__builtin_fmaf(-d, r, 1.0f), r, r);
}
__device__ __forceinline__ float lt_sigmoid(float x) {
    const float e = __builtin_amdgcn_exp2f(__builtin_fminf(-LT_L2E * x, 126.0f));
    return lt_rcp_nr(1.0f + e);
}
__device__ __forceinline__ float lt_tanh(float x) {
    const float e = __builtin_amdgcn_exp2f((-2.0f * LT_L2E) * __builtin_fabsf(x));
    const float n = 1.0f - e, d = 1.0f + e;
    const float r = __builtin_amdgcn_rcpf(d);
    float q = n * r;
    q = __builtin_fmaf(__builtin_fmaf(-d, q, n), r, q);
    return __builtin_copysignf(q, x);
}

struct LtRec {
    const void *state; int P;
    const float *whh[2];        // weight_hh [4H][H] of the two directions, inside the state's masters
    float *gates, *c, *hprev;   // [dirs][N][4H], [dirs][N][H], [dirs][N][H]
    float *y;                   // forward: the layer's output [N][ldy], column dir H + unit
    const float *dy;            // backward: dL/dy [N][ldy]
    int ldy;
    const int *lens; int B, T;
    HtGuard guard;              // backward: the workspace header
};

__device__ __forceinline__ int lt_len(const LtRec &a, int b) { return b < a.B ? ht_row_len(a.lens, b, a.T) : 0; }

__global__ __launch_bounds__(256) void lt_prep_kernel(LstmTrainShape q, void *state, const int *lens, int B, int T, uint8_t *valid, float *bsum,
                                                      LstmTrainWsHead *head, unsigned thr, float scale, unsigned long long seed) {
    if (!ht_state_ok(state, LT_MAGIC, q.P)) return;
    const float *master = reinterpret_cast<const float *>(reinterpret_cast<const HeadTrainHeader *>(state) + 1);
    const int N = B * T, G = 4 * q.H;
    const int gtid = (int)blockIdx.x * 256 + threadIdx.x, gsz = (int)gridDim.x * 256;
    for (int n = gtid; n < N; n += gsz) {
        const int b = n / T;
        valid[n] = (n - b * T) < ht_row_len(lens, b, T) ? 1 : 0;
    }
    for (int j = gtid; j < q.nl * q.dirs * G; j += gsz) {
        const int ld = j / G, r = j - ld * G, li = ld / q.dirs, d = ld - li * q.dirs;
        bsum[j] = master[q.off[li][d][2] + r] + master[q.off[li][d][3] + r];
    }
    if (gtid == 0) {
        head->magic = LT_WS_MAGIC; head->B = B; head->T = T;
        head->thr = thr;                                 // 0: this forward call drops nothing, whatever an earlier one left here
        if (thr > 0) {                                   // take the draw ordinal and advance it: the one writer of the count
            HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(state);
            const unsigned long long draw = hd->draws;
            hd->draws = draw + 1;
            head->draw = draw; head->scale = scale; head->seed = seed;
        }
    }
}

// lt_philox: Philox4x32-10, philox.h (shared with mix.hip)

// head != nullptr: the record of the workspace header (thr == 0 there: nothing to do), under the state's magic and the guard;
// head == nullptr: the stand-alone call, everything in the arguments
struct LtDrop {
    const float *x; float *out; long long groups; int cq, layer;   // groups = rows x cq, cq = cols / 4
    const LstmTrainWsHead *head; const void *state; int P; HtGuard guard;
    unsigned long long draw, seed; unsigned thr; float scale;
};

__global__ __launch_bounds__(256) void lt_dropout_kernel(LtDrop a) {
    unsigned long long draw = a.draw, seed = a.seed;
    unsigned thr = a.thr;
    float scale = a.scale;
    if (a.head) {
        if (!ht_state_ok(a.state, LT_MAGIC, a.P) || !ht_guard_ok(a.guard)) return;
        thr = a.head->thr;
        if (thr == 0) return;
        draw = a.head->draw; scale = a.head->scale; seed = a.head->seed;
    }
    const long long g = (long long)blockIdx.x * 256 + threadIdx.x;
    if (g >= a.groups) return;
    const long long n = g / a.cq;
    const unsigned jq = (unsigned)(g - n * a.cq);
    const uint4 r = lt_philox(make_uint4((unsigned)n, ((unsigned)a.layer << 16) | jq, (unsigned)draw, (unsigned)(draw >> 32)), (unsigned)seed,
                              (unsigned)(seed >> 32));
    const float4 v = reinterpret_cast<const float4 *>(a.x)[g];
    float4 o;   // selects, not products: a NaN or -0 at a dropped position comes out +0
    o.x = r.x >= thr ? v.x * scale : 0.0f;
    o.y = r.y >= thr ? v.y * scale : 0.0f;
    o.z = r.z >= thr ? v.z * scale : 0.0f;
    o.w = r.w >= thr ? v.w * scale : 0.0f;
    reinterpret_cast<float4 *>(a.out)[g] = o;
}

template <int H>
__global__ __launch_bounds__(H * 4) void lt_fwd_kernel(LtRec a) {
    constexpr int HS = H + 4;   // LDS row stride (floats): the 4 sequence rows land on disjoint banks
    constexpr int PD = LT_PD;
    __shared__ __attribute__((aligned(16))) float hbuf[2][4][HS];
    if (!ht_state_ok(a.state, LT_MAGIC, a.P)) return;

    const int tile = blockIdx.x, dir = blockIdx.y;
    const bool reverse = dir == 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int jb = lane & 3;    // sequence within the tile (B / D operand column), gate index of the A operand
    const int blk = lane >> 2;  // MFMA block = hidden unit within the wave's 16
    const int unit = wave * 16 + blk;
    int tmax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) tmax = max(tmax, lt_len(a, tile * 4 + i));
    const int seq = tile * 4 + jb;
    const int len = lt_len(a, seq);                      // 0 past the batch: such a lane stores nothing
    const int seqc = seq < a.B ? seq : a.B - 1;          // ... and prefetches a row that exists

    float w[H];                                          // row (gate jb, unit) of W_hh
    {
        const float4 *wp = reinterpret_cast<const float4 *>(a.whh[dir] + ((size_t)jb * H + unit) * H);
#pragma unroll
        for (int kq = 0; kq < H / 4; ++kq) {
            const float4 v = wp[kq];
            w[4 * kq + 0] = v.x; w[4 * kq + 1] = v.y; w[4 * kq + 2] = v.z; w[4 * kq + 3] = v.w;
        }
    }

    const size_t N = (size_t)a.B * a.T, row0 = (size_t)dir * N + (size_t)seqc * a.T;
    float *gp = a.gates + row0 * (4 * H) + unit;         // + t 4H + gate H
    float *cp = a.c + row0 * H + unit;                   // + t H
    float *hp = a.hprev + row0 * H + unit;
    float *yp = a.y + (size_t)seqc * a.T * a.ldy + (size_t)dir * H + unit;   // + t ldy
    // the frame of step s in this direction's order (the backward direction walks down from tmax - 1 and holds the zero state until its
    // sequence's own last frame); a step past the last one prefetches the last row again, and with no step at all frame 0
    auto t_of = [&](int s) {
        if (tmax == 0) return 0;
        s = s < tmax ? s : tmax - 1;
        return reverse ? tmax - 1 - s : s;
    };
    auto g_load = [&](f32x4 &dst, int t) {
        const float *p = gp + (size_t)t * (4 * H);
        dst[0] = p[0]; dst[1] = p[H]; dst[2] = p[2 * H]; dst[3] = p[3 * H];
    };
    f32x4 gq[PD];
#pragma unroll
    for (int p = 0; p < PD; ++p) g_load(gq[p], t_of(p));

    float c = 0.0f, hcarry = 0.0f;                       // the carried state of (sequence jb, unit)
    hbuf[0][jb][unit] = 0.0f;
    __syncthreads();

    for (int s0 = 0; s0 < tmax; s0 += PD) {
#pragma unroll
        for (int u = 0; u < PD; ++u) {
            const int s = s0 + u;
            if (s >= tmax) break;   // uniform over the workgroup
            const int t = t_of(s);
            const float *hb = &hbuf[s & 1][jb][0];
            // 4 independent accumulation chains (k mod 4), the first one starting from the prefetched pre-activations
            f32x4 a0 = gq[u], a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f}, a3 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kq = 0; kq < H / 4; ++kq) {
                const float4 hq = *reinterpret_cast<const float4 *>(hb + 4 * kq);
                a0 = __builtin_amdgcn_mfma_f32_4x4x1f32(w[4 * kq + 0], hq.x, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_4x4x1f32(w[4 * kq + 1], hq.y, a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_4x4x1f32(w[4 * kq + 2], hq.z, a2, 0, 0, 0);
                a3 = __builtin_amdgcn_mfma_f32_4x4x1f32(w[4 * kq + 3], hq.w, a3, 0, 0, 0);
                if (kq == H / 8) g_load(gq[u], t_of(s + PD));   // refill this ring slot
            }
            const f32x4 pre = (a0 + a1) + (a2 + a3);
            const float ig = lt_sigmoid(pre[0]), fg = lt_sigmoid(pre[1]), gg = lt_tanh(pre[2]), og = lt_sigmoid(pre[3]);
            const float cn = __builtin_fmaf(fg, c, ig * gg);
            const float h = og * lt_tanh(cn);
            const bool valid = t < len;
            if (valid) {
                float *g = gp + (size_t)t * (4 * H);
                g[0] = ig; g[H] = fg; g[2 * H] = gg; g[3 * H] = og;
                cp[(size_t)t * H] = cn;
                hp[(size_t)t * H] = hcarry;
                yp[(size_t)t * a.ldy] = h;
            } else if (seq < a.B) {
                yp[(size_t)t * a.ldy] = 0.0f;
            }
            // a select, not a product: whatever a frame past the length computed from never reaches the carried state
            c = valid ? cn : 0.0f;
            hcarry = valid ? h : 0.0f;
            hbuf[(s + 1) & 1][jb][unit] = hcarry;
            __syncthreads();
        }
    }
    if (seq < a.B)
        for (int t = tmax; t < a.T; ++t) yp[(size_t)t * a.ldy] = 0.0f;
}

struct LtRow { float i, f, g, o, c, dy; bool valid; };

template <int H>
__global__ __launch_bounds__(H * 4) void lt_bwd_kernel(LtRec a) {
    constexpr int DS = 4 * H + 4;   // LDS row stride of one sequence's dpre
    constexpr int PS = H + 4;
    constexpr int UG = H / 64;      // groups of 64 output units: a wave is (gate, unit group)
    __shared__ __attribute__((aligned(16))) float dps[4][DS];
    __shared__ __attribute__((aligned(16))) float part[4][4][PS];   // [gate][sequence][unit]
    if (!ht_state_ok(a.state, LT_MAGIC, a.P) || !ht_guard_ok(a.guard)) return;

    const int tile = blockIdx.x, dir = blockIdx.y;
    const bool reverse = dir == 1;
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the matrix half: wave (gate, ug), A rows = output units ug 64 + 4 blk + (0 .. 3), B / D column = sequence
    const int gate = wave / UG, ug = wave - gate * UG;
    const int col = lane & 3, blk = lane >> 2;
    float wt[H];                                         // column (ug 64 + 4 blk + col) of the gate's H rows of W_hh
    {
        const float *wp = a.whh[dir] + (size_t)gate * H * H + ug * 64 + 4 * blk + col;
#pragma unroll
        for (int j = 0; j < H; ++j) wt[j] = wp[(size_t)j * H];
    }
    // the elementwise half: one thread per (sequence jb, unit u)
    const int jb = (int)threadIdx.x / H, u = (int)threadIdx.x - jb * H;
    int tmax = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) tmax = max(tmax, lt_len(a, tile * 4 + i));
    const int seq = tile * 4 + jb;
    const int len = lt_len(a, seq);
    const int seqc = seq < a.B ? seq : a.B - 1;
    const size_t N = (size_t)a.B * a.T, row0 = (size_t)dir * N + (size_t)seqc * a.T;
    float *gp = a.gates + row0 * (4 * H) + u;
    const float *cp = a.c + row0 * H + u;
    const float *dyp = a.dy + (size_t)seqc * a.T * a.ldy + (size_t)dir * H + u;
    // step s walks the direction's own order backwards: the forward direction from tmax - 1 down, the backward direction from 0 up
    auto t_of = [&](int s) { return reverse ? s : tmax - 1 - s; };
    auto load = [&](int s) {
        LtRow r{0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, false};
        if (s < tmax) {
            const int t = t_of(s);
            r.valid = t < len;
            if (r.valid) {                               // frames past a length are never read
                const float *g = gp + (size_t)t * (4 * H);
                r.i = g[0]; r.f = g[H]; r.g = g[2 * H]; r.o = g[3 * H];
                r.c = cp[(size_t)t * H];
                r.dy = dyp[(size_t)t * a.ldy];
            }
        }
        return r;
    };
    LtRow cur = load(0), nx1 = load(1);
    float dc_rec = 0.0f;
    for (int s = 0; s < tmax; ++s) {
        const LtRow nx2 = load(s + 2);                   // two steps ahead: the next step's c is this step's c_{t-1}
        float dh_rec = 0.0f;
        if (s > 0) dh_rec = ((part[0][jb][u] + part[1][jb][u]) + part[2][jb][u]) + part[3][jb][u];   // the four gates' shares, in gate order
        const float dh = cur.dy + dh_rec;
        const float tc = lt_tanh(cur.c);
        const float d_o = dh * tc;
        const float dc = (dh * cur.o) * (1.0f - tc * tc) + dc_rec;
        const float c_prev = nx1.valid ? nx1.c : 0.0f;   // +0 at the direction's first step
        const float di = dc * cur.g, dg = dc * cur.i, df = dc * c_prev;
        float pi = di * (cur.i * (1.0f - cur.i));
        float pf = df * (cur.f * (1.0f - cur.f));
        float pg = dg * (1.0f - cur.g * cur.g);
        float po = d_o * (cur.o * (1.0f - cur.o));
        float dcn = dc * cur.f;
        if (!cur.valid) { pi = 0.0f; pf = 0.0f; pg = 0.0f; po = 0.0f; dcn = 0.0f; }   // selects: +0 past a length
        dc_rec = dcn;
        if (seq < a.B) {
            float *g = gp + (size_t)t_of(s) * (4 * H);
            g[0] = pi; g[H] = pf; g[2 * H] = pg; g[3 * H] = po;
        }
        dps[jb][u] = pi; dps[jb][H + u] = pf; dps[jb][2 * H + u] = pg; dps[jb][3 * H + u] = po;
        __syncthreads();
        if (s + 1 < tmax) {   // uniform over the workgroup; this gate's share of dh_rec = dpre W_hh for the next step
            const float *db = &dps[col][gate * H];
            f32x4 a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f}, a2 = {0.f, 0.f, 0.f, 0.f}, a3 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int kq = 0; kq < H / 4; ++kq) {
                const float4 dv = *reinterpret_cast<const float4 *>(db + 4 * kq);
                a0 = __builtin_amdgcn_mfma_f32_4x4x1f32(wt[4 * kq + 0], dv.x, a0, 0, 0, 0);
                a1 = __builtin_amdgcn_mfma_f32_4x4x1f32(wt[4 * kq + 1], dv.y, a1, 0, 0, 0);
                a2 = __builtin_amdgcn_mfma_f32_4x4x1f32(wt[4 * kq + 2], dv.z, a2, 0, 0, 0);
                a3 = __builtin_amdgcn_mfma_f32_4x4x1f32(wt[4 * kq + 3], dv.w, a3, 0, 0, 0);
            }
            *reinterpret_cast<f32x4 *>(&part[gate][col][ug * 64 + 4 * blk]) = (a0 + a1) + (a2 + a3);
        }
        __syncthreads();
        cur = nx1;
        nx1 = nx2;
    }
    if (seq < a.B)   // the frames no step of this workgroup ran: dpre is +0 there too, the weight-gradient products read every frame
        for (int t = tmax; t < a.T; ++t) {
            float *g = gp + (size_t)t * (4 * H);
            g[0] = 0.0f; g[H] = 0.0f; g[2 * H] = 0.0f; g[3 * H] = 0.0f;
        }
}

// everything but the masters, which the caller copies in: accumulator, m, v and the padding zeroed, the header written
__global__ __launch_bounds__(256) void lt_reset_kernel(LstmTrainShape q, void *state) {
    HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(state);
    float *w = reinterpret_cast<float *>(hd + 1);
    const int gtid = (int)blockIdx.x * 256 + threadIdx.x, gsz = (int)gridDim.x * 256;
    for (int j = q.P + gtid; j < 4 * q.Pp; j += gsz) w[j] = 0.0f;
    if (gtid == 0) {
        HeadTrainHeader h{};
        h.magic = LT_MAGIC; h.D0 = q.Din; h.H = q.H; h.L = q.nl; h.P = q.P;
        h.loss = 0.0; h.frames = 0ull; h.t = 0ull; h.bc1 = 0.0f; h.bc2 = 0.0f;
        *hd = h;
    }
}

struct LtBufs {
    LstmTrainWsHead *head; HeadTrainWsHead *fold; uint8_t *valid; float *bsum, *dbuf[2], *part;
    float *gates[LT_MAX_LAYERS], *c[LT_MAX_LAYERS], *hprev[LT_MAX_LAYERS], *h[LT_MAX_LAYERS];
};
LtBufs lt_bufs(const LstmTrainShape &q, const LstmTrainWs &w, void *ws) {
    char *base = reinterpret_cast<char *>(ws);
    LtBufs b{};
    b.head = reinterpret_cast<LstmTrainWsHead *>(base);
    b.fold = reinterpret_cast<HeadTrainWsHead *>(base + w.off_fold);
    b.valid = reinterpret_cast<uint8_t *>(base + w.off_valid);
    b.bsum = reinterpret_cast<float *>(base + w.off_bsum);
    for (int i = 0; i < 2; ++i) b.dbuf[i] = reinterpret_cast<float *>(base + w.off_d[i]);
    b.part = reinterpret_cast<float *>(base + w.off_part);
    for (int li = 0; li < q.nl; ++li) {
        b.gates[li] = reinterpret_cast<float *>(base + w.off_gates[li]);
        b.c[li] = reinterpret_cast<float *>(base + w.off_c[li]);
        b.hprev[li] = reinterpret_cast<float *>(base + w.off_hprev[li]);
        b.h[li] = reinterpret_cast<float *>(base + w.off_h[li]);
    }
    return b;
}

bool lt_args_ok(const LstmTrainShape &q, const LstmTrainArgs &a) {
    return a.x && a.state && a.ws && a.B > 0 && a.T > 0 && (long long)a.B * a.T <= HT_MAX_FRAMES && a.seg >= HT_MIN_SEGMENT &&
           a.seg <= HT_MAX_SEGMENT && a.seg % 32 == 0 && (q.H == 64 || q.H == 128) && q.nl >= 1 && q.nl <= LT_MAX_LAYERS;
}
// the in-place stage over the output of trainable layer li, or over the gradient with respect to it: a buffer [N][H dirs]
hipError_t lt_launch_drop(const LstmTrainShape &q, const LstmTrainArgs &a, const LtBufs &b, float *buf, int li, const HtGuard &guard, hipStream_t s) {
    LtDrop d{};
    d.x = buf; d.out = buf; d.cq = q.H * q.dirs / 4; d.groups = (long long)a.B * a.T * d.cq; d.layer = q.first_layer + li;
    d.head = b.head; d.state = a.state; d.P = q.P; d.guard = guard;
    hipLaunchKernelGGL(lt_dropout_kernel, dim3((unsigned)((d.groups + 255) / 256)), dim3(256), 0, s, d);
    return hipGetLastError();
}
unsigned lt_tiles(int M, int Nc) { return (unsigned)(((M + HT_TM - 1) / HT_TM) * ((Nc + HT_TN - 1) / HT_TN)); }

template <typename K>
hipError_t lt_launch_rec(K fwd64, K fwd128, int H, int B, int dirs, const LtRec &r, hipStream_t s) {
    const dim3 grid((unsigned)((B + 3) / 4), (unsigned)dirs);
    if (H == 64) hipLaunchKernelGGL(fwd64, grid, dim3(256), 0, s, r);
    else hipLaunchKernelGGL(fwd128, grid, dim3(512), 0, s, r);
    return hipGetLastError();
}

}  // namespace

LstmTrainShape lstm_train_shape(int Din, int H, int dirs, int num_layers, int first_layer) {
    LstmTrainShape q{};
    q.Din = Din; q.H = H; q.dirs = dirs; q.nl = num_layers - first_layer; q.first_layer = first_layer;
    int off = 0;
    for (int li = 0; li < q.nl && li < LT_MAX_LAYERS; ++li) {
        q.in[li] = li == 0 ? Din : H * dirs;
        for (int d = 0; d < dirs; ++d) {
            q.off[li][d][0] = off; off += 4 * H * q.in[li];
            q.off[li][d][1] = off; off += 4 * H * H;
            q.off[li][d][2] = off; off += 4 * H;
            q.off[li][d][3] = off; off += 4 * H;
        }
    }
    q.P = off;
    q.Pp = (off + 63) / 64 * 64;
    return q;
}

size_t lstm_train_state_bytes(const LstmTrainShape &q) { return sizeof(HeadTrainHeader) + (size_t)4 * q.Pp * sizeof(float); }

LstmTrainWs lstm_train_ws(const LstmTrainShape &q, long long N, int seg) {
    LstmTrainWs w{};
    w.N = (int)N;
    w.nseg = (int)((N + seg - 1) / seg);
    const size_t H = (size_t)q.H, D = (size_t)q.dirs, f = sizeof(float);
    size_t off = sizeof(LstmTrainWsHead);
    w.off_fold = off; off += sizeof(HeadTrainWsHead);
    w.off_valid = off; off = ht_align(off + (size_t)N);
    w.off_bsum = off; off = ht_align(off + (size_t)q.nl * D * 4 * H * f);
    for (int li = 0; li < q.nl; ++li) {
        w.off_gates[li] = off; off = ht_align(off + D * N * 4 * H * f);
        w.off_c[li] = off; off = ht_align(off + D * N * H * f);
        w.off_hprev[li] = off; off = ht_align(off + D * N * H * f);
        w.off_h[li] = off; off = ht_align(off + (li + 1 < q.nl ? (size_t)N * H * D * f : 0));
    }
    for (int i = 0; i < 2; ++i) { w.off_d[i] = off; off = ht_align(off + (q.nl > 1 ? (size_t)N * H * D * f : 0)); }
    w.off_part = off; off = ht_align(off + (size_t)w.nseg * q.Pp * f);
    w.total = off;
    return w;
}

hipError_t launch_lstm_train_reset(const LstmTrainShape &q, void *state, hipStream_t s) {
    if (!state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(lt_reset_kernel, dim3(64), dim3(256), 0, s, q, state);
    return hipGetLastError();
}

#define LT_LAUNCHED() do { e = hipGetLastError(); if (e != hipSuccess) return e; } while (0)

hipError_t launch_lstm_train_forward(const LstmTrainShape &q, const LstmTrainArgs &a, hipStream_t s) {
    if (!lt_args_ok(q, a) || !a.y) return hipErrorInvalidValue;
    const int N = a.B * a.T, H = q.H, D = q.dirs;
    const LstmTrainWs w = lstm_train_ws(q, N, a.seg);
    const LtBufs b = lt_bufs(q, w, a.ws);
    const float *master = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.state) + sizeof(HeadTrainHeader));
    hipError_t e;
    {
        const int work = N > q.nl * D * 4 * H ? N : q.nl * D * 4 * H;
        const unsigned blocks = (unsigned)((work + 255) / 256 < 4096 ? (work + 255) / 256 : 4096);
        hipLaunchKernelGGL(lt_prep_kernel, dim3(blocks), dim3(256), 0, s, q, a.state, a.lens, a.B, a.T, b.valid, b.bsum, b.head, a.thr, a.scale,
                           a.seed);
        LT_LAUNCHED();
    }
    for (int li = 0; li < q.nl; ++li) {
        const float *x = li == 0 ? a.x : b.h[li - 1];
        for (int d = 0; d < D; ++d) {   // the gate pre-activations of direction d
            HtGemm g{};
            g.A = x; g.B = master + q.off[li][d][0]; g.M = N; g.Nc = 4 * H; g.K = q.in[li];
            g.a_valid = li == 0 ? b.valid : nullptr;
            g.bias = b.bsum + (size_t)(li * D + d) * 4 * H; g.slope = 1.0f;
            g.C = b.gates[li] + (size_t)d * N * 4 * H; g.ldc = 4 * H;
            g.state = a.state; g.magic = LT_MAGIC; g.P = q.P;
            hipLaunchKernelGGL(ht_gemm_kernel<0>, dim3(lt_tiles(N, 4 * H)), dim3(256), 0, s, g);
            LT_LAUNCHED();
        }
        LtRec r{};
        r.state = a.state; r.P = q.P;
        for (int d = 0; d < D; ++d) r.whh[d] = master + q.off[li][d][1];
        r.gates = b.gates[li]; r.c = b.c[li]; r.hprev = b.hprev[li];
        r.y = li + 1 == q.nl ? a.y : b.h[li]; r.ldy = H * D;
        r.lens = a.lens; r.B = a.B; r.T = a.T;
        e = lt_launch_rec(lt_fwd_kernel<64>, lt_fwd_kernel<128>, H, a.B, D, r, s);
        if (e != hipSuccess) return e;
        if (a.thr > 0 && li + 1 < q.nl) {   // the next layer's projection and its dW_ih both take the dropped value; h_prev is kept apart
            e = lt_launch_drop(q, a, b, b.h[li], li, HtGuard{}, s);
            if (e != hipSuccess) return e;
        }
    }
    return hipSuccess;
}

hipError_t launch_lstm_train_backward(const LstmTrainShape &q, const LstmTrainArgs &a, hipStream_t s) {
    if (!lt_args_ok(q, a) || !a.dy) return hipErrorInvalidValue;
    const int N = a.B * a.T, H = q.H, D = q.dirs;
    const LstmTrainWs w = lstm_train_ws(q, N, a.seg);
    const LtBufs b = lt_bufs(q, w, a.ws);
    const float *master = reinterpret_cast<const float *>(reinterpret_cast<const char *>(a.state) + sizeof(HeadTrainHeader));
    const HtGuard guard{reinterpret_cast<const int *>(b.head), {LT_WS_MAGIC, a.B, a.T}};
    hipError_t e;
    for (int li = q.nl - 1; li >= 0; --li) {
        const float *x = li == 0 ? a.x : b.h[li - 1];
        LtRec r{};
        r.state = a.state; r.P = q.P;
        for (int d = 0; d < D; ++d) r.whh[d] = master + q.off[li][d][1];
        r.gates = b.gates[li]; r.c = b.c[li]; r.hprev = b.hprev[li];
        r.dy = li + 1 == q.nl ? a.dy : b.dbuf[li & 1]; r.ldy = H * D;
        r.lens = a.lens; r.B = a.B; r.T = a.T; r.guard = guard;
        if (a.drop && li + 1 < q.nl) {   // dy of layer li = the masked, scaled d_in of layer li + 1: the forward call's mask, from the header
            e = lt_launch_drop(q, a, b, b.dbuf[li & 1], li, guard, s);
            if (e != hipSuccess) return e;
        }
        e = lt_launch_rec(lt_bwd_kernel<64>, lt_bwd_kernel<128>, H, a.B, D, r, s);
        if (e != hipSuccess) return e;
        float *d_in = li > 0 ? b.dbuf[(li - 1) & 1] : a.grad_in;
        for (int d = 0; d < D; ++d) {
            const float *dpre = b.gates[li] + (size_t)d * N * 4 * H;
            for (int hh = 0; hh < 2; ++hh) {   // dW_ih = sum dpre^T x, dW_hh = sum dpre^T h_prev; db rides along in both
                HtGemm g{};
                g.A = dpre; g.B = hh ? b.hprev[li] + (size_t)d * N * H : x; g.M = 4 * H; g.Nc = hh ? H : q.in[li]; g.K = N;
                g.b_valid = b.valid;
                g.C = b.part + q.off[li][d][hh]; g.ldc = g.Nc; g.Cb = b.part + q.off[li][d][2 + hh]; g.part_stride = q.Pp; g.seg = a.seg;
                g.state = a.state; g.magic = LT_MAGIC; g.P = q.P; g.guard = guard;
                hipLaunchKernelGGL(ht_gemm_kernel<2>, dim3(lt_tiles(g.M, g.Nc), (unsigned)w.nseg), dim3(256), 0, s, g);
                LT_LAUNCHED();
            }
            if (d_in) {   // d_in = dpre W_ih, the directions added in order
                HtGemm g{};
                g.A = dpre; g.B = master + q.off[li][d][0]; g.M = N; g.Nc = q.in[li]; g.K = 4 * H;
                g.c_valid = b.valid; g.c_add = d;
                g.C = d_in; g.ldc = q.in[li];
                g.state = a.state; g.magic = LT_MAGIC; g.P = q.P; g.guard = guard;
                hipLaunchKernelGGL(ht_gemm_kernel<1>, dim3(lt_tiles(N, q.in[li])), dim3(256), 0, s, g);
                LT_LAUNCHED();
            }
        }
    }
    hipLaunchKernelGGL(ht_fold_kernel, dim3((unsigned)((q.P + 255) / 256)), dim3(256), 0, s, a.state, LT_MAGIC, q.P, q.Pp, b.part, w.nseg,
                       (const double *)nullptr, 0, 0, a.lens, a.B, a.T, b.fold, guard);
    LT_LAUNCHED();
    return hipSuccess;
}
#undef LT_LAUNCHED

unsigned lstm_dropout_threshold(float p) { return (unsigned)__builtin_floor((double)p * 4294967296.0); }

hipError_t launch_dropout_apply(const float *x, float *out, long long rows, int cols, int layer, unsigned long long draw, unsigned thr, float scale,
                                unsigned long long seed, hipStream_t s) {
    if (!x || !out || rows < 1 || rows > HT_MAX_FRAMES || cols < 4 || cols % 4 || cols > LT_DROP_MAX_COLS || layer < 0 || layer > LT_DROP_MAX_LAYER)
        return hipErrorInvalidValue;
    LtDrop d{};
    d.x = x; d.out = out; d.cq = cols / 4; d.groups = rows * d.cq; d.layer = layer;
    d.draw = draw; d.seed = seed; d.thr = thr; d.scale = scale;
    hipLaunchKernelGGL(lt_dropout_kernel, dim3((unsigned)((d.groups + 255) / 256)), dim3(256), 0, s, d);
    return hipGetLastError();
}

}  // namespace uvad
