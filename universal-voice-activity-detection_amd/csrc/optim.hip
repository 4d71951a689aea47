// optim.hip -- the joint optimizer step over the head, LSTM and SincNet training states (uvad_optim_*, include/uvad.h): the global gradient
// norm and its clipping coefficient, weight decay (L2 into the gradient, or decoupled as AdamW), a learning-rate table indexed by the count
// of applied steps, the skip of a step whose norm is not finite, and the Adam update of ht_adam_kernel with those applied.  What
// torch.nn.utils.clip_grad_norm_ + torch.optim.Adam(weight_decay=) / AdamW + an lr scheduler + Lightning's skipped step do around the
// reference's configure_optimizers.  The three states share HeadTrainHeader | masters | accumulator | m | v, so one set of kernels serves them.
//   opt_sumsq_kernel    one workgroup per chunk of OPT_CHUNK parameters of a state that takes part: g = acc / frames, the squares in double
//                       (exact), lane l adds elements l, l + 256, ... of its chunk in order, the 256 lanes fold as a fixed tree: a partial
//   opt_fold_kernel     one workgroup stages the partials through LDS, one thread adds them: the partials in chunk order, the states in
//                       the order head, LSTM, SincNet; norm, coef, lr_t and the skip decision into the optim header
//   opt_adam_kernel     one thread per parameter of a state that takes part: the clipped, decayed gradient and ht_adam_kernel's update;
//                       a skipped step zeroes the accumulator and nothing else
//   opt_commit_kernel   one thread, after every workgroup above has read the headers: ht_adam_commit_kernel's header update per state,
//                       the optim state's counts
// A state takes part iff it is given, its header carries its family's magic word and parameter count, and its frame count is not zero; every
// kernel decides that from the headers alone, which only the commit changes.  No atomics: the same calls give the same bits.
// Contraction is off in the whole file, as in head_train.hip: tests/optim_ref.py restates the step operation by operation.
// The kernels on one state's blocks live here too, once for the three families: ht_adam_kernel + ht_adam_commit_kernel (launch_train_apply:
// a family's own _apply), ht_read_kernel (launch_train_read) and ht_write_kernel (launch_train_write), keyed by a TrainBlock's magic word.
#include "ht_kernels.h"

namespace uvad {

static_assert(sizeof(OptimHeader) == 256 && offsetof(OptimHeader, t) == 64 && offsetof(OptimHeader, norm) == 80, "the optim state's layout");
static_assert(OPT_RECORD_WORDS == UVAD_OPTIM_RECORD_WORDS && LT_SCALAR_WORDS == UVAD_LSTM_TRAIN_SCALAR_WORDS, "the records of include/uvad.h");
static_assert(OPT_CHUNK == 16 * 256, "a chunk is 16 passes of 256 lanes");

namespace {

struct OptFam { void *state; unsigned magic; int P, Pp, chunk0, nchunk, blk0, nblk; };   // chunks of the norm's grid, 256-parameter blocks of the update's
struct OptArgs { OptFam f[3]; void *opt; int cap; double *part; };

__device__ __forceinline__ bool opt_ok(const void *opt, int cap) {
    const OptimHeader *oh = reinterpret_cast<const OptimHeader *>(opt);
    return oh->magic == OPT_MAGIC && oh->cap == cap && oh->n >= 1 && oh->n <= cap;
}
__device__ __forceinline__ bool opt_takes_part(const OptFam &f) {
    return f.state && ht_state_ok(f.state, f.magic, f.P) && reinterpret_cast<const HeadTrainHeader *>(f.state)->frames != 0ull;
}
// the family whose chunks hold global chunk c (-1: none)
__device__ __forceinline__ int opt_family_of(const OptArgs &a, int c) {
    for (int k = 0; k < 3; ++k)
        if (a.f[k].state && c >= a.f[k].chunk0 && c < a.f[k].chunk0 + a.f[k].nchunk) return k;
    return -1;
}

__global__ __launch_bounds__(256) void opt_sumsq_kernel(OptArgs a) {
    __shared__ double sh[256];
    if (!opt_ok(a.opt, a.cap)) return;
    const int c = (int)blockIdx.x, k = opt_family_of(a, c);
    if (k < 0 || !opt_takes_part(a.f[k])) return;
    const OptFam &f = a.f[k];
    const HeadTrainHeader *hd = reinterpret_cast<const HeadTrainHeader *>(f.state);
    const float *acc = reinterpret_cast<const float *>(hd + 1) + f.Pp;
    const float cnt = (float)hd->frames;
    const int tid = threadIdx.x, j0 = (c - f.chunk0) * OPT_CHUNK;
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < OPT_CHUNK / 256; ++i) {
        const int j = j0 + i * 256 + tid;
        if (j < f.P) {
            const float g = acc[j] / cnt;
            s = s + (double)g * (double)g;
        }
    }
    sh[tid] = s;
    __syncthreads();
    for (int o = 128; o >= 1; o >>= 1) {
        if (tid < o) sh[tid] = sh[tid] + sh[tid + o];
        __syncthreads();
    }
    if (tid == 0) a.part[c] = sh[0];
}

__global__ __launch_bounds__(256) void opt_fold_kernel(OptArgs a) {
    __shared__ double sh[256];
    if (!opt_ok(a.opt, a.cap)) return;                           // block-uniform, as every test below: the barriers are reached by all or none
    OptimHeader *oh = reinterpret_cast<OptimHeader *>(a.opt);
    const int tid = threadIdx.x;
    unsigned mask = 0u;
    double S = 0.0;                                              // thread 0's running sum: the partials in chunk order, the states in family order
    for (int k = 0; k < 3; ++k) {
        if (!opt_takes_part(a.f[k])) continue;
        mask |= 1u << k;
        for (int c0 = 0; c0 < a.f[k].nchunk; c0 += 256) {        // 256 partials at a time through LDS: the loads run side by side, the adds in order
            const int n = a.f[k].nchunk - c0 < 256 ? a.f[k].nchunk - c0 : 256;
            if (tid < n) sh[tid] = a.part[a.f[k].chunk0 + c0 + tid];
            __syncthreads();
            if (tid == 0)
                for (int c = 0; c < n; ++c) S = S + sh[c];
            __syncthreads();
        }
    }
    if (tid != 0 || !mask) return;                               // nothing accumulated anywhere: no step, nothing written
    const float norm = (float)sqrt(S);
    const float coef = oh->max_norm > 0.0f ? fminf(1.0f, oh->max_norm / (norm + 1e-6f)) : 1.0f;   // clip_grad_norm_'s expression
    const unsigned long long last = (unsigned long long)(oh->n - 1);
    const float *table = reinterpret_cast<const float *>(oh + 1);
    const int skip = oh->skip_nonfinite && !isfinite(S) ? 1 : 0;
    oh->norm = norm;
    oh->coef = skip ? 0.0f : coef;
    oh->lr_t = table[oh->t < last ? oh->t : last];
    oh->mask = mask;
    oh->skip = skip;
}

__global__ __launch_bounds__(256) void opt_adam_kernel(OptArgs a) {
    if (!opt_ok(a.opt, a.cap)) return;
    const int b = (int)blockIdx.x;
    int k = -1;
    for (int i = 0; i < 3; ++i)
        if (a.f[i].state && b >= a.f[i].blk0 && b < a.f[i].blk0 + a.f[i].nblk) k = i;
    if (k < 0 || !opt_takes_part(a.f[k])) return;
    const OptFam &f = a.f[k];
    const OptimHeader *oh = reinterpret_cast<const OptimHeader *>(a.opt);
    HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(f.state);
    float *w = reinterpret_cast<float *>(hd + 1), *acc = w + f.Pp, *m = acc + f.Pp, *v = m + f.Pp;
    const int j = (b - f.blk0) * 256 + (int)threadIdx.x;
    if (j >= f.P) return;
    if (oh->skip) {                                              // the step is skipped: the gradients go, everything else stays
        acc[j] = 0.0f;
        return;
    }
    const float cnt = (float)hd->frames;
    const float coef = oh->coef, wd = oh->wd;
    const float lr = oh->lr_t * oh->lr_scale[k];                 // lr_k = fl(lr_t * scale)
    const float b1 = oh->b1, b2 = oh->b2, omb1 = oh->omb1, omb2 = oh->omb2, eps = oh->eps;
    const float bc1 = hd->bc1 * b1 + omb1, bc2 = hd->bc2 * b2 + omb2;   // 1 - beta^t, advanced: see HeadTrainHeader
    const float step_size = lr / bc1;
    const float bc2s = sqrtf(bc2);
    float g = acc[j] / cnt;
    g = g * coef;
    float wj = w[j];
    if (wd > 0.0f) {
        if (oh->decoupled) wj = wj * (1.0f - lr * wd);           // AdamW: w <- w (1 - lr wd)
        else g = g + wd * wj;                                    // Adam(weight_decay=): L2 into the gradient
    }
    float mj = m[j], vj = v[j];
    mj = mj + (g - mj) * omb1;                                   // ht_adam_kernel's update from here on
    vj = vj * b2 + (omb2 * g) * g;
    const float denom = sqrtf(vj) / bc2s + eps;
    w[j] = wj - step_size * (mj / denom);
    m[j] = mj;
    v[j] = vj;
    acc[j] = 0.0f;
}

__global__ void opt_commit_kernel(OptArgs a) {
    if (threadIdx.x != 0 || !opt_ok(a.opt, a.cap)) return;
    OptimHeader *oh = reinterpret_cast<OptimHeader *>(a.opt);
    bool any = false;
    for (int k = 0; k < 3; ++k) {
        if (!opt_takes_part(a.f[k])) continue;
        any = true;
        HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(a.f[k].state);
        if (!oh->skip) {                                         // ht_adam_commit_kernel's header update
            hd->bc1 = hd->bc1 * oh->b1 + oh->omb1;
            hd->bc2 = hd->bc2 * oh->b2 + oh->omb2;
            hd->t += 1ull;
        }
        hd->loss = 0.0;
        hd->frames = 0ull;
    }
    if (!any) return;
    if (oh->skip) oh->skipped += 1ull;
    else oh->t += 1ull;
    oh->skip = 0;
}

__global__ void opt_set_n_kernel(void *opt, int cap, int n) {
    OptimHeader *oh = reinterpret_cast<OptimHeader *>(opt);
    if (threadIdx.x != 0 || oh->magic != OPT_MAGIC || oh->cap != cap) return;
    oh->n = n;
}

__global__ void opt_read_kernel(const void *opt, int cap, unsigned *out) {
    const OptimHeader *oh = reinterpret_cast<const OptimHeader *>(opt);
    const int i = threadIdx.x;
    if (i >= OPT_RECORD_WORDS) return;
    const unsigned long long q = i < 6 ? oh->t : oh->skipped;
    const unsigned word = i == 0 ? __float_as_uint(oh->norm) : i == 1 ? __float_as_uint(oh->coef) : i == 2 ? __float_as_uint(oh->lr_t)
                          : i == 3 ? oh->mask : (unsigned)(i & 1 ? q >> 32 : q);
    out[i] = opt_ok(opt, cap) ? word : 0u;
}

__global__ void opt_write_kernel(void *opt, int cap, const unsigned *in) {
    if (threadIdx.x != 0 || !opt_ok(opt, cap)) return;
    OptimHeader *oh = reinterpret_cast<OptimHeader *>(opt);
    oh->norm = __uint_as_float(in[0]);
    oh->coef = __uint_as_float(in[1]);
    oh->lr_t = __uint_as_float(in[2]);
    oh->mask = in[3];
    oh->t = (unsigned long long)in[4] | (unsigned long long)in[5] << 32;
    oh->skipped = (unsigned long long)in[6] | (unsigned long long)in[7] << 32;
    oh->skip = 0;
}

// ---- the kernels on one state's blocks: every family's _apply, _read and _write (launch_train_*) ----
// torch.optim.Adam (no weight decay, no amsgrad) with the running bias corrections 1 - beta^t; every operation one rounding
__global__ __launch_bounds__(256) void ht_adam_kernel(void *state, unsigned magic, int P, int Pp, HeadTrainAdam o) {
    if (!ht_state_ok(state, magic, P)) return;
    HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(state);
    const unsigned long long frames = hd->frames;
    if (frames == 0ull) return;                                  // nothing accumulated: no step
    float *w = reinterpret_cast<float *>(hd + 1), *acc = w + Pp, *m = acc + Pp, *v = m + Pp;
    const float cnt = (float)frames;
    const float bc1 = hd->bc1 * o.b1 + o.omb1, bc2 = hd->bc2 * o.b2 + o.omb2;   // 1 - beta^t, advanced: see HeadTrainHeader
    const float step_size = o.lr / bc1;
    const float bc2s = sqrtf(bc2);
    const int j = (int)blockIdx.x * 256 + threadIdx.x;
    if (j < P) {
        const float g = acc[j] / cnt;
        float mj = m[j], vj = v[j];
        mj = mj + (g - mj) * o.omb1;                             // exp_avg.lerp_(grad, 1 - beta1)
        vj = vj * o.b2 + (o.omb2 * g) * g;                       // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value = 1 - beta2)
        const float denom = sqrtf(vj) / bc2s + o.eps;
        w[j] = w[j] - step_size * (mj / denom);                  // param.addcdiv_(exp_avg, denom, value = -step_size)
        m[j] = mj;
        v[j] = vj;
        acc[j] = 0.0f;
    }
}
// after every workgroup of ht_adam_kernel has read the header: the step counted, the running corrections advanced, the sums zeroed
__global__ void ht_adam_commit_kernel(void *state, unsigned magic, int P, HeadTrainAdam o) {
    if (!ht_state_ok(state, magic, P)) return;
    HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(state);
    if (threadIdx.x != 0 || hd->frames == 0ull) return;
    hd->bc1 = hd->bc1 * o.b1 + o.omb1;
    hd->bc2 = hd->bc2 * o.b2 + o.omb2;
    hd->t += 1ull;
    hd->loss = 0.0;
    hd->frames = 0ull;
}

__global__ __launch_bounds__(256) void ht_read_kernel(const void *state, unsigned magic, int P, int Pp, int which, float *out) {
    const HeadTrainHeader *hd = reinterpret_cast<const HeadTrainHeader *>(state);
    const bool ok = ht_state_ok(state, magic, P);
    if (which == UVAD_HEAD_TRAIN_SCALARS) {
        // an LSTM state's record carries two more words, [8 .. 9]: the dropout draw ordinal (UVAD_LSTM_TRAIN_SCALAR_WORDS)
        if (blockIdx.x == 0 && threadIdx.x < (magic == LT_MAGIC ? LT_SCALAR_WORDS : HT_SCALAR_WORDS)) {
            const int i = threadIdx.x;
            const unsigned long long q = i < 2 ? (unsigned long long)__double_as_longlong(hd->loss) : i < 4 ? hd->frames : i < 8 ? hd->t : hd->draws;
            const unsigned word = i == 6 ? __float_as_uint(hd->bc1) : i == 7 ? __float_as_uint(hd->bc2) : (unsigned)(i & 1 ? q >> 32 : q);
            reinterpret_cast<unsigned *>(out)[i] = ok ? word : 0u;
        }
        return;
    }
    const float *src = reinterpret_cast<const float *>(hd + 1) + (size_t)which * Pp;
    for (int j = (int)blockIdx.x * 256 + threadIdx.x; j < P; j += (int)gridDim.x * 256) out[j] = ok ? src[j] : 0.0f;
}

// what ht_read_kernel copied out, put back: a tensor block, or t, bc1, bc2 (and an LSTM state's draw ordinal) from the scalar record
__global__ __launch_bounds__(256) void ht_write_kernel(void *state, unsigned magic, int P, int Pp, int which, const float *in) {
    if (!ht_state_ok(state, magic, P)) return;
    HeadTrainHeader *hd = reinterpret_cast<HeadTrainHeader *>(state);
    if (which == UVAD_HEAD_TRAIN_SCALARS) {
        if (blockIdx.x != 0 || threadIdx.x != 0) return;
        const unsigned *q = reinterpret_cast<const unsigned *>(in);
        hd->t = (unsigned long long)q[4] | (unsigned long long)q[5] << 32;
        hd->bc1 = __uint_as_float(q[6]);
        hd->bc2 = __uint_as_float(q[7]);
        if (magic == LT_MAGIC) hd->draws = (unsigned long long)q[8] | (unsigned long long)q[9] << 32;
        return;
    }
    float *dst = reinterpret_cast<float *>(hd + 1) + (size_t)which * Pp;
    for (int j = (int)blockIdx.x * 256 + threadIdx.x; j < P; j += (int)gridDim.x * 256) dst[j] = in[j];
}

}  // namespace

hipError_t launch_optim_step(const TrainBlock fam[3], void *opt, int cap, double *part, hipStream_t s) {
    if (!opt || !part || cap < 1) return hipErrorInvalidValue;
    OptArgs a{};
    int chunks = 0, blocks = 0;
    for (int k = 0; k < 3; ++k) {
        a.f[k] = OptFam{fam[k].state, fam[k].magic, fam[k].P, fam[k].Pp, chunks, fam[k].state ? optim_chunks(fam[k].P) : 0,
                        blocks, fam[k].state ? (fam[k].P + 255) / 256 : 0};
        chunks += a.f[k].nchunk;
        blocks += a.f[k].nblk;
    }
    if (chunks < 1) return hipErrorInvalidValue;
    a.opt = opt; a.cap = cap; a.part = part;
    hipError_t e;
    hipLaunchKernelGGL(opt_sumsq_kernel, dim3((unsigned)chunks), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(opt_fold_kernel, dim3(1), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(opt_adam_kernel, dim3((unsigned)blocks), dim3(256), 0, s, a);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    hipLaunchKernelGGL(opt_commit_kernel, dim3(1), dim3(64), 0, s, a);
    return hipGetLastError();
}

hipError_t launch_optim_set_n(void *opt, int cap, int n, hipStream_t s) {
    if (!opt || n < 1 || n > cap) return hipErrorInvalidValue;
    hipLaunchKernelGGL(opt_set_n_kernel, dim3(1), dim3(64), 0, s, opt, cap, n);
    return hipGetLastError();
}

hipError_t launch_optim_read(const void *opt, int cap, unsigned *out, hipStream_t s) {
    if (!opt || !out) return hipErrorInvalidValue;
    hipLaunchKernelGGL(opt_read_kernel, dim3(1), dim3(64), 0, s, opt, cap, out);
    return hipGetLastError();
}

hipError_t launch_optim_write(void *opt, int cap, const unsigned *in, hipStream_t s) {
    if (!opt || !in) return hipErrorInvalidValue;
    hipLaunchKernelGGL(opt_write_kernel, dim3(1), dim3(64), 0, s, opt, cap, in);
    return hipGetLastError();
}

hipError_t launch_train_apply(const TrainBlock &b, const HeadTrainAdam &o, hipStream_t s) {
    if (!b.state) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ht_adam_kernel, dim3((unsigned)((b.P + 255) / 256)), dim3(256), 0, s, b.state, b.magic, b.P, b.Pp, o);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    hipLaunchKernelGGL(ht_adam_commit_kernel, dim3(1), dim3(64), 0, s, b.state, b.magic, b.P, o);
    return hipGetLastError();
}

hipError_t launch_train_read(const TrainBlock &b, int which, float *out, hipStream_t s) {
    if (!b.state || !out || which < 0 || which > UVAD_HEAD_TRAIN_SCALARS) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ht_read_kernel, dim3(which == UVAD_HEAD_TRAIN_SCALARS ? 1u : (unsigned)((b.P + 255) / 256)), dim3(256), 0, s,
                       (const void *)b.state, b.magic, b.P, b.Pp, which, out);
    return hipGetLastError();
}

hipError_t launch_train_write(const TrainBlock &b, int which, const float *in, hipStream_t s) {
    if (!b.state || !in || which < 0 || which > UVAD_HEAD_TRAIN_SCALARS || which == UVAD_HEAD_TRAIN_GRAD) return hipErrorInvalidValue;
    hipLaunchKernelGGL(ht_write_kernel, dim3(which == UVAD_HEAD_TRAIN_SCALARS ? 1u : (unsigned)((b.P + 255) / 256)), dim3(256), 0, s, b.state, b.magic,
                       b.P, b.Pp, which, in);
    return hipGetLastError();
}

}  // namespace uvad
