// One-launch Adam step over a list of fp32 tensors (gfx950) — the optimizer
// of every reference training script (torch.optim.Adam(model.parameters(),
// lr, weight_decay=5e-5), e.g. exp_pretraining.py / exp_molhiv.py:53), with
// the arithmetic of torch's fused Adam (L2 weight decay added to the
// gradient, no amsgrad / maximize):
//   t = step + 1;  g += wd * p;  m = b1 m + (1 - b1) g;  v = b2 v + (1 - b2) g^2
//   p -= (lr / (1 - b1^t)) * m / (sqrt(v) / sqrt(1 - b2^t) + eps);  step = t
//
// torch's fused / foreach paths need 4-5 launches per step for a model of
// ~75 small tensors (step increments + chunked multi-tensor kernels); here
// the tensor table (up to 80 tensors: one launch for the pretraining model)
// travels by value in the kernel arguments (captured with the launch in a
// HIP graph), every workgroup handles one 1024-element chunk
// of one tensor, and the last workgroup to finish advances every tensor's
// step counter (all workgroups read the step before they arrive).
//
// The _dyn entry points read the hyper-parameters from a device block instead
// of the kernel arguments (a learning-rate schedule over a device call
// counter, the clip coefficient of scgib_grad_norm, the skip of a non-finite
// step: DESIGN.md §24), and DEC selects AdamW's decoupled weight decay.
#include "common.h"

namespace scgib {

constexpr int kAdamMax = 80;       // tensors per launch (kernel-argument table, < 4 KB)
constexpr int kAdamChunk = 1024;   // elements per workgroup

// structure of arrays (no per-entry padding): 80 tensors in 3.8 KB of kernel
// arguments, so a whole model's ~75 hot-path tensors take one launch
struct AdamTable {
    float *param[kAdamMax];
    const float *grad[kAdamMax];
    float *exp_avg[kAdamMax];
    float *exp_avg_sq[kAdamMax];
    float *step[kAdamMax];
    int32_t numel[kAdamMax];
    int32_t chunk0[kAdamMax + 1];  // first chunk of tensor i; chunk0[n] = grid
    int32_t n;
};
static_assert(sizeof(AdamTable) <= 4096, "kernel-argument table");

struct AdamRef {
    float *param;
    const float *grad;
    float *exp_avg, *exp_avg_sq;
    int64_t numel;
};

// Where a launch's hyper-parameters come from.  ByValue: the kernel arguments
// (frozen into a captured graph node; scgib_adam_step, the path of every
// reference script).  FromDevice: the optimizer's device blocks, read by
// every workgroup for itself (scgib_adam_step_dyn: a learning-rate schedule,
// the clip coefficient and the skip decision inside a replayed step).  Both
// resolve to one Hyper, and adam_coef / adam_elem take it from there, so the
// arithmetic of the two paths cannot drift.
struct ByValue {
    static constexpr bool kDyn = false;
    double lr, beta1, beta2, eps, wd;
};
struct FromDevice {
    static constexpr bool kDyn = true;
    const scgib_optim_hyper *h;  // this launch's param group
    scgib_optim_state *st;
    double *last_lr;             // this group's read-out
    int32_t flags;               // SCGIB_OPTIM_*
};
struct Hyper {
    double lr, beta1, beta2, eps, wd;
    float coef;     // clip coefficient (1 without a norm launch)
    bool skip;      // non-finite norm under SCGIB_OPTIM_SKIP: change nothing
    int64_t calls;  // the call counter this step read
};

// factor(c) of the schedule, in double (optim.Schedule.factor is its host
// restatement, expression for expression)
__device__ __forceinline__ double sched_factor(const scgib_optim_hyper &h, int64_t c) {
    if (c < h.warmup)
        return h.warmup_start + (1 - h.warmup_start) * static_cast<double>(c) /
                                    static_cast<double>(h.warmup);
    const int64_t span = h.total - h.warmup > 1 ? h.total - h.warmup : 1;
    double u = static_cast<double>(c - h.warmup) / static_cast<double>(span);
    u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    if (h.kind == SCGIB_SCHED_LINEAR) return 1 - (1 - h.min_ratio) * u;
    if (h.kind == SCGIB_SCHED_COSINE)
        return h.min_ratio + (1 - h.min_ratio) * 0.5 * (1 + cos(3.141592653589793 * u));
    return 1.0;
}

__device__ __forceinline__ Hyper resolve(const ByValue &hp) {
    return Hyper{hp.lr, hp.beta1, hp.beta2, hp.eps, hp.wd, 1.f, false, 0};
}
__device__ __forceinline__ Hyper resolve(const FromDevice &hp) {
    const scgib_optim_hyper &h = *hp.h;
    const int64_t c = hp.st->calls;
    const bool normed = (hp.flags & SCGIB_OPTIM_NORM) != 0;
    return Hyper{h.lr * sched_factor(h, c), h.beta1, h.beta2, h.eps, h.weight_decay,
                 normed ? hp.st->coef : 1.f,
                 normed && (hp.flags & SCGIB_OPTIM_SKIP) && hp.st->finite == 0, c};
}

// The last workgroup of a FromDevice launch: this group's read-out, and with
// SCGIB_OPTIM_ADVANCE (the step's last launch) the call counter — read by
// every workgroup of every launch of the step before it arrived — and the
// count of skipped steps.  One thread.
__device__ __forceinline__ void optim_advance(const FromDevice &hp, const Hyper &hy) {
    *hp.last_lr = hy.lr;
    if (hp.flags & SCGIB_OPTIM_ADVANCE) {
        hp.st->calls = hy.calls + 1;
        if (hy.skip) hp.st->skipped += 1;
    }
}
__device__ __forceinline__ void optim_advance(const ByValue &, const Hyper &) {}

// Precision mirrors torch's fused Adam (ATen fused_adam_utils.cuh): the
// hyper-parameters are doubles, so the weight decay, both moment updates and
// eps enter in double and round to fp32 on assignment; the bias corrections
// are computed in double and rounded to fp32; the final update is fp32.
// One element (shared by adam_chunk and the fused reduce + Adam launch, so
// both give the same bits).
// DEC: decoupled weight decay (AdamW), torch's fused ADAMW mode: p -= lr wd p
// in double, rounded to fp32, before the update; nothing is added to g.
template <bool DEC>
__device__ __forceinline__ void adam_elem(float p, float g, float m, float v, float step_size,
                                          float bc2_sqrt, double beta1, double beta2, double eps,
                                          double wd, double lr, float &pp, float &mm, float &vv) {
    float gg = g;
    if (wd != 0.0) {
        if (DEC) p = static_cast<float>(p - lr * wd * p);
        else gg = static_cast<float>(gg + p * wd);
    }
    mm = static_cast<float>(beta1 * m + (1 - beta1) * gg);
    vv = static_cast<float>(beta2 * v + (1 - beta2) * gg * gg);
    const float denom = static_cast<float>(sqrtf(vv) / bc2_sqrt + eps);
    pp = p - step_size * mm / denom;
}

// the tensor's bias corrections at its step t = *step + 1
__device__ __forceinline__ void adam_coef(const float *step, double lr, double beta1,
                                          double beta2, float &step_size, float &bc2_sqrt) {
    const float t = *step + 1.f;
    const float bc1 = static_cast<float>(1 - pow(beta1, static_cast<double>(t)));
    bc2_sqrt = static_cast<float>(sqrt(1 - pow(beta2, static_cast<double>(t))));
    step_size = static_cast<float>(lr / bc1);
}

// DYN: the gradient enters as g * coef (an fp32 multiply, always applied)
template <int NT, int EPT, bool DYN, bool DEC>  // NT threads; a chunk is EPT * NT elements
__device__ __forceinline__ void adam_chunk(const AdamRef &T, int64_t base, float step_size,
                                           float bc2_sqrt, const Hyper &hy) {
    float p[EPT], g[EPT], m[EPT], v[EPT];
    int64_t idx[EPT];
#pragma unroll
    for (int k = 0; k < EPT; ++k) {  // clamped loads (all in flight), masked stores
        const int64_t j = base + threadIdx.x + NT * k;
        idx[k] = j < T.numel ? j : T.numel - 1;
        p[k] = T.param[idx[k]];
        g[k] = T.grad[idx[k]];
        m[k] = T.exp_avg[idx[k]];
        v[k] = T.exp_avg_sq[idx[k]];
    }
#pragma unroll
    for (int k = 0; k < EPT; ++k) {
        float pp, mm, vv;
        adam_elem<DEC>(p[k], DYN ? g[k] * hy.coef : g[k], m[k], v[k], step_size, bc2_sqrt,
                       hy.beta1, hy.beta2, hy.eps, hy.wd, hy.lr, pp, mm, vv);
        if (base + threadIdx.x + NT * k < T.numel) {
            T.param[idx[k]] = pp;
            T.exp_avg[idx[k]] = mm;
            T.exp_avg_sq[idx[k]] = vv;
        }
    }
}

template <class H, bool DEC>
__global__ __launch_bounds__(256) void adam_step_k(const AdamTable tab, const H hp,
                                                   unsigned *__restrict__ counter) {
    const Hyper hy = resolve(hp);
    const int b = blockIdx.x;
    // tensor of this chunk: one parallel compare over the table (lane q holds
    // chunk0[q]) instead of a dependent scalar-load chain
    const int lane = threadIdx.x & 63;
    int i = -1;
#pragma unroll
    for (int r = 0; r < (kAdamMax + 63) / 64; ++r) {
        const int q = 64 * r + lane;
        const bool le = q < tab.n && tab.chunk0[q < tab.n ? q : 0] <= b;
        i += __popcll(__ballot(le));
    }
    const AdamRef T{tab.param[i], tab.grad[i], tab.exp_avg[i], tab.exp_avg_sq[i], tab.numel[i]};
    float step_size, bc2_sqrt;
    adam_coef(tab.step[i], hy.lr, hy.beta1, hy.beta2, step_size, bc2_sqrt);
    const int64_t base = static_cast<int64_t>(b - tab.chunk0[i]) * kAdamChunk;
    if (T.numel > 0 && !hy.skip)
        adam_chunk<256, 4, H::kDyn, DEC>(T, base, step_size, bc2_sqrt, hy);
    __shared__ unsigned s_last;
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                 gridDim.x - 1;
    __syncthreads();
    if (s_last) {  // every workgroup has read its step: advance all of them at once
        if (threadIdx.x < tab.n && !hy.skip) *tab.step[threadIdx.x] += 1.f;
        if (threadIdx.x == 0) {
            *counter = 0u;
            optim_advance(hp, hy);
        }
    }
}

// ---------------------------------------------------------------------------
// The step's last weight-gradient reduce and the Adam step in ONE launch
// (scgib_adam_step_reduce): the reduce's column blocks (slab_reduce_multi_k's
// decomposition and fixed order, so every gradient has the same bits) apply
// Adam to the elements of the tensors whose gradients they produce, right
// where the reduced value is in a register; the other tensors' Adam chunks
// run as the launch's remaining workgroups, beside them.  The replayed
// pretraining step ended with the two launches back to back (the ego chain's
// final reduce after the join, then Adam): one launch boundary and the Adam
// launch's latency leave its tail.
// ---------------------------------------------------------------------------
constexpr int kFuseJobs = 8;
constexpr int kFuseSegs = 16;
// Adam elements per thread in the fused launch: one (a chunk per 1024
// elements, ~96 workgroups for the pretraining model) — with four, QM9
// B = 32 ran 0.2537–0.2552 ms against 0.2519–0.2527 (B = 512 unchanged,
// profiles/r06_noise/fuse_ept_ab.txt).  Build-time A/B hook SCGIB_FUSE_EPT.
#ifndef SCGIB_FUSE_EPT
#define SCGIB_FUSE_EPT 1
#endif
constexpr int kFuseEPT = SCGIB_FUSE_EPT;
constexpr int kFuseChunk = kFuseEPT * 1024;  // Adam elements per 1024-thread workgroup

struct FuseTable {
    scgib_slab_job j[kFuseJobs];
    int32_t blk0[kFuseJobs + 1];  // first column block of job i; blk0[nj] = reduce blocks
    int32_t nj;
    // reduced tensors: table entry t's gradient = elements [o0, o0 + numel) of job's output
    int32_t seg_t[kFuseSegs], seg_job[kFuseSegs], seg_o0[kFuseSegs];
    int32_t ns;
};

template <class H, bool DEC>
__global__ __launch_bounds__(1024) void adam_reduce_k(const AdamTable tab, const FuseTable ft,
                                                      const H hp,
                                                      unsigned *__restrict__ counter) {
    const Hyper hy = resolve(hp);  // (no norm launch precedes a fused reduce: coef 1, no skip)
    const int b = blockIdx.x;
    const int lane = threadIdx.x & 63;
    const int nred = ft.blk0[ft.nj];
    __shared__ float red[16][64];
    if (b < nred) {  // block-uniform: one column block of one reduce job
        const int el = threadIdx.x & 63, sp = threadIdx.x >> 6;
        const bool le = lane < ft.nj && ft.blk0[lane < ft.nj ? lane : 0] <= b;
        const int i = __popcll(__ballot(le)) - 1;
        const scgib_slab_job &J = ft.j[i];
        const int64_t e = static_cast<int64_t>(b - ft.blk0[i]) * 64 + el;
        const int64_t stride = J.stride > 0 ? J.stride : J.width;
        // the Adam tensor of this element's gradient, its bias corrections and
        // operands: independent of the sums, so in flight with the slab loads
        int t = -1;
        int64_t o = 0;
        float step_size = 0.f, bc2_sqrt = 1.f, p0 = 0.f, m0 = 0.f, v0 = 0.f;
        if (sp == 0 && e < J.width) {
            for (int q = 0; q < ft.ns; ++q) {
                const int64_t oq = e - ft.seg_o0[q];
                if (ft.seg_job[q] == i && oq >= 0 && oq < tab.numel[ft.seg_t[q]]) {
                    t = ft.seg_t[q];
                    o = oq;
                }
            }
            if (t >= 0) {
                p0 = tab.param[t][o];
                m0 = tab.exp_avg[t][o];
                v0 = tab.exp_avg_sq[t][o];
                adam_coef(tab.step[t], hy.lr, hy.beta1, hy.beta2, step_size, bc2_sqrt);
            }
        }
        float acc = 0.f;
        if (e < J.width) {
            for (int b0 = sp; b0 < J.n_slabs; b0 += 16 * 8) {
                float v[8];
#pragma unroll
                for (int u = 0; u < 8; ++u)
                    v[u] = ld_ok(J.slab, static_cast<int64_t>(b0 + 16 * u) * stride + e, e,
                                 b0 + 16 * u < J.n_slabs, 0.f);
#pragma unroll
                for (int u = 0; u < 8; ++u) acc += v[u];
            }
        }
        red[sp][el] = acc;
        __syncthreads();
        if (sp == 0 && e < J.width) {
            double sum = 0.0;
#pragma unroll
            for (int k = 0; k < 16; ++k) sum += static_cast<double>(red[k][el]);
            const float g = static_cast<float>(sum);
            J.out[e] = g;
            if (t >= 0) {
                float pp, mm, vv;
                adam_elem<DEC>(p0, g, m0, v0, step_size, bc2_sqrt, hy.beta1, hy.beta2, hy.eps,
                               hy.wd, hy.lr, pp, mm, vv);
                tab.param[t][o] = pp;
                tab.exp_avg[t][o] = mm;
                tab.exp_avg_sq[t][o] = vv;
            }
        }
    } else {  // an Adam chunk of a tensor whose gradient is already complete
        const int c = b - nred;
        int i = -1;
#pragma unroll
        for (int r = 0; r < (kAdamMax + 63) / 64; ++r) {
            const int q = 64 * r + lane;
            const bool le = q < tab.n && tab.chunk0[q < tab.n ? q : 0] <= c;
            i += __popcll(__ballot(le));
        }
        const AdamRef T{tab.param[i], tab.grad[i], tab.exp_avg[i], tab.exp_avg_sq[i], tab.numel[i]};
        float step_size, bc2_sqrt;
        adam_coef(tab.step[i], hy.lr, hy.beta1, hy.beta2, step_size, bc2_sqrt);
        const int64_t base = static_cast<int64_t>(c - tab.chunk0[i]) * kFuseChunk;
        if (T.numel > 0)
            adam_chunk<1024, kFuseEPT, false, DEC>(T, base, step_size, bc2_sqrt, hy);
    }
    __shared__ unsigned s_last;
    __syncthreads();
    if (threadIdx.x == 0)
        s_last = __hip_atomic_fetch_add(counter, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ==
                 gridDim.x - 1;
    __syncthreads();
    if (s_last) {  // every workgroup has read its steps: advance all of them at once
        if (threadIdx.x < tab.n) *tab.step[threadIdx.x] += 1.f;
        if (threadIdx.x == 0) {
            *counter = 0u;
            optim_advance(hp, hy);
        }
    }
}

// A FromDevice step that has no tensor at all still counts as a call.
__global__ void optim_advance_k(const FromDevice hp) {
    if (threadIdx.x == 0) optim_advance(hp, resolve(hp));
}

// ---------------------------------------------------------------------------
// Global gradient norm (scgib_grad_norm): S = sum (double)g (double)g over the
// table's gradients in a FIXED order, so that norm, clip coefficient and the
// skip decision have the same bits on every run, eagerly and replayed.  One
// workgroup per 1024-element chunk (the Adam step's chunk -> tensor scheme):
// thread t adds its elements t, t + 256, t + 512, t + 768 of the chunk in that
// order, a wavefront is summed by a fixed butterfly, the four wavefronts in
// order; the chunk's partial goes to ws[chunk].  The last workgroup to arrive
// adds the partials: thread t takes ws[t], ws[t + 256], ... in order (as many
// rounds as the chunks need), then the same butterfly and wavefront order.
// Which workgroup arrives last changes nothing: it reads every partial,
// its own included, from ws, and only ws[0 .. chunks) is read.  No atomics
// on floating point.  Several launches (more tensors than one table): each
// adds its total to st->sumsq in launch order (`first` starts it), the `last`
// one writes norm, coef and finite.
// ---------------------------------------------------------------------------
__device__ __forceinline__ double wave_sum_d(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// every thread's value -> the workgroup's sum, valid on thread 0
__device__ __forceinline__ double block_sum_d(double v, double *sh) {
    v = wave_sum_d(v);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh[0] + sh[1]) + sh[2]) + sh[3];
}

__global__ __launch_bounds__(256) void grad_norm_k(const AdamTable tab, double *ws,
                                                   unsigned *counter,
                                                   const scgib_optim_hyper *__restrict__ h,
                                                   scgib_optim_state *st, int first, int last) {
    __shared__ double sh[2][4];
    const int b = blockIdx.x, lane = threadIdx.x & 63, G = gridDim.x;
    double a = 0.0;
    if (b < tab.chunk0[tab.n]) {  // (a table without elements is one idle workgroup)
        int i = -1;
#pragma unroll
        for (int r = 0; r < (kAdamMax + 63) / 64; ++r) {
            const int q = 64 * r + lane;
            const bool le = q < tab.n && tab.chunk0[q < tab.n ? q : 0] <= b;
            i += __popcll(__ballot(le));
        }
        const float *g = tab.grad[i];
        const int64_t n = tab.numel[i];  // > 0: the tensor has a chunk
        const int64_t base = static_cast<int64_t>(b - tab.chunk0[i]) * kAdamChunk;
        float v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // clamped loads, masked values
            const int64_t j = base + threadIdx.x + 256 * k;
            v[k] = g[j < n ? j : n - 1];
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const double d = static_cast<double>(v[k]);
            a += base + threadIdx.x + 256 * k < n ? d * d : 0.0;
        }
    }
    const double part = block_sum_d(a, sh[0]);
    if (threadIdx.x == 0) st_agent(ws + b, part);
    if (!block_arrive(counter, G)) return;
    double t = 0.0;
    for (int q = threadIdx.x; q < G; q += 256) t += ld_agent(ws + q);
    const double total = block_sum_d(t, sh[1]);
    if (threadIdx.x == 0) {
        const double S = first ? total : st->sumsq + total;
        st->sumsq = S;
        if (last) {
            const float norm = static_cast<float>(sqrt(S));
            // torch.nn.utils.clip_grad_norm_: max_norm / (norm + 1e-6) clamped at 1,
            // in fp32; a NaN stays a NaN (the comparison is false)
            const float c = static_cast<float>(h->max_grad_norm) / (norm + 1e-6f);
            st->norm = norm;
            st->coef = h->max_grad_norm < 0.0 ? 1.f : (c > 1.f ? 1.f : c);
            st->finite = isfinite(norm) ? 1 : 0;
        }
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// ---------------------------------------------------------------------------
// Gradient bucket for the data-parallel all-reduce (dist.GradAllReducer): all
// gradients packed into one flat buffer in ONE launch (and unpacked, scaled
// by 1 / world, in one more) instead of a copy launch per tensor.  Same
// chunk -> tensor scheme as the Adam step; the table travels by value.
// ---------------------------------------------------------------------------
constexpr int kPackMax = 96;

struct PackTable {
    scgib_grad_slice t[kPackMax];
    int32_t chunk0[kPackMax + 1];
    int32_t n;
};

template <bool UNPACK>
__global__ __launch_bounds__(256) void grad_pack_k(const PackTable tab, float *__restrict__ flat,
                                                   float scale) {
    const int b = blockIdx.x, lane = threadIdx.x & 63;
    // tensor of this chunk: parallel compare over the table (two 64-wide rounds)
    int i = -1;
#pragma unroll
    for (int r = 0; r < (kPackMax + 63) / 64; ++r) {
        const int q = 64 * r + lane;
        const bool le = q < tab.n && tab.chunk0[q < tab.n ? q : 0] <= b;
        i += __popcll(__ballot(le));
    }
    const scgib_grad_slice &T = tab.t[i];
    const int64_t base = static_cast<int64_t>(b - tab.chunk0[i]) * kAdamChunk;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const int64_t j = base + threadIdx.x + 256 * k;
        if (j < T.numel) {
            if (UNPACK) T.data[j] = scale * flat[T.offset + j];
            else flat[T.offset + j] = T.data[j];
        }
    }
}

static int launch_pack(const scgib_grad_slice *tensors, int32_t n, float *flat, float scale,
                       bool unpack, hipStream_t st) {
    if (n < 0 || n > kPackMax) return SCGIB_EINVAL;
    if (n == 0) return SCGIB_OK;
    if (!tensors || !flat) return SCGIB_EINVAL;
    PackTable tab;
    tab.n = n;
    int64_t chunks = 0;
    for (int i = 0; i < n; ++i) {
        const scgib_grad_slice &T = tensors[i];
        if (T.numel < 0 || T.offset < 0 || (T.numel > 0 && !T.data)) return SCGIB_EINVAL;
        tab.t[i] = T;
        tab.chunk0[i] = static_cast<int32_t>(chunks);
        chunks += (T.numel + kAdamChunk - 1) / kAdamChunk;
        if (chunks > 0x7fffffff) return SCGIB_EUNSUPPORTED;
    }
    tab.chunk0[n] = static_cast<int32_t>(chunks);
    for (int i = n; i < kPackMax; ++i) tab.t[i] = scgib_grad_slice{};
    if (chunks == 0) return SCGIB_OK;
    if (unpack)
        grad_pack_k<true><<<dim3(static_cast<unsigned>(chunks)), 256, 0, st>>>(tab, flat, scale);
    else
        grad_pack_k<false><<<dim3(static_cast<unsigned>(chunks)), 256, 0, st>>>(tab, flat, scale);
    return launch_status();
}

// The by-value table of a launch: tensor i's chunks of `chunk` elements start
// at chunk0[i].  `own(i)`: the tensor has chunks of its own (the fused reduce
// updates some tensors from the reduce's workgroups).  Returns a status and
// the number of chunks.
template <class Own>
static int fill_table(const scgib_adam_tensor *tensors, int32_t n, int chunk, Own own,
                      AdamTable &tab, int64_t &chunks) {
    tab.n = n;
    chunks = 0;
    for (int i = 0; i < n; ++i) {
        const scgib_adam_tensor &T = tensors[i];
        if (T.numel < 0 || !T.step || (T.numel > 0 && (!T.param || !T.grad || !T.exp_avg ||
                                                       !T.exp_avg_sq)))
            return SCGIB_EINVAL;
        if (T.numel > 0x7fffffff) return SCGIB_EUNSUPPORTED;
        tab.param[i] = T.param;
        tab.grad[i] = T.grad;
        tab.exp_avg[i] = T.exp_avg;
        tab.exp_avg_sq[i] = T.exp_avg_sq;
        tab.step[i] = T.step;
        tab.numel[i] = static_cast<int32_t>(T.numel);
        tab.chunk0[i] = static_cast<int32_t>(chunks);
        const int rc = own(i);
        if (rc < 0) return rc;
        if (rc > 0) chunks += (T.numel + chunk - 1) / chunk;
        if (chunks > 0x7fffffff) return SCGIB_EUNSUPPORTED;
    }
    tab.chunk0[n] = static_cast<int32_t>(chunks);
    for (int i = n; i < kAdamMax; ++i) {
        tab.param[i] = tab.exp_avg[i] = tab.exp_avg_sq[i] = tab.step[i] = nullptr;
        tab.grad[i] = nullptr;
        tab.numel[i] = 0;
    }
    return SCGIB_OK;
}

static bool dyn_args_ok(const FromDevice &hp) {
    return hp.h && hp.st && hp.last_lr && !(reinterpret_cast<uintptr_t>(hp.h) & 7) &&
           !(reinterpret_cast<uintptr_t>(hp.st) & 7) &&
           !(reinterpret_cast<uintptr_t>(hp.last_lr) & 7) &&
           !(hp.flags & ~(SCGIB_OPTIM_NORM | SCGIB_OPTIM_SKIP | SCGIB_OPTIM_ADVANCE));
}

template <class H>
static int launch_step(const scgib_adam_tensor *tensors, int32_t n_tensors, const H &hp,
                       bool decoupled, uint32_t *counter, hipStream_t st) {
    if (n_tensors < 0 || n_tensors > kAdamMax) return SCGIB_EINVAL;
    if (n_tensors == 0) return SCGIB_OK;
    if (!tensors || !counter) return SCGIB_EINVAL;
    AdamTable tab;
    int64_t chunks;
    if (const int rc = fill_table(tensors, n_tensors, kAdamChunk, [](int) { return 1; }, tab,
                                  chunks))
        return rc;
    if (chunks == 0) {  // only empty tensors: just advance the steps
        tab.chunk0[n_tensors] = 1;
        chunks = 1;
    }
    const dim3 grid(static_cast<unsigned>(chunks));
    if (decoupled) adam_step_k<H, true><<<grid, 256, 0, st>>>(tab, hp, counter);
    else adam_step_k<H, false><<<grid, 256, 0, st>>>(tab, hp, counter);
    return launch_status();
}

template <class H>
static int launch_step_reduce(const scgib_adam_tensor *tensors, int32_t n_tensors,
                              const scgib_slab_job *jobs, int32_t n_jobs, const H &hp,
                              bool decoupled, uint32_t *counter, hipStream_t st) {
    if (n_tensors < 0 || n_tensors > kAdamMax || n_jobs < 0 || n_jobs > kFuseJobs) return SCGIB_EINVAL;
    if (n_jobs == 0) return launch_step(tensors, n_tensors, hp, decoupled, counter, st);
    if (!jobs || !counter || (n_tensors > 0 && !tensors)) return SCGIB_EINVAL;
    FuseTable ft{};
    ft.nj = n_jobs;
    int64_t blocks = 0;
    for (int i = 0; i < n_jobs; ++i) {
        const scgib_slab_job &J = jobs[i];
        if (J.n_slabs <= 0 || J.width <= 0 || !J.slab || !J.out) return SCGIB_EINVAL;
        if (J.stride < 0 || (J.stride > 0 && J.stride < J.width)) return SCGIB_EINVAL;
        ft.j[i] = J;
        ft.blk0[i] = static_cast<int32_t>(blocks);
        blocks += (J.width + 63) / 64;
        if (blocks > 0x3fffffff) return SCGIB_EUNSUPPORTED;
    }
    ft.blk0[n_jobs] = static_cast<int32_t>(blocks);
    AdamTable tab{};
    int64_t chunks;
    // a gradient inside a job's output: Adam in the reduce (no chunks of its own);
    // one that straddles an output's edge is refused
    auto own = [&](int t) -> int {
        const scgib_adam_tensor &T = tensors[t];
        int seg = -1;
        for (int i = 0; i < n_jobs && T.numel > 0; ++i) {
            const float *o0 = jobs[i].out, *o1 = jobs[i].out + jobs[i].width;
            const float *g0 = T.grad, *g1 = T.grad + T.numel;
            if (g0 >= o0 && g1 <= o1) {
                seg = i;
                break;
            }
            if (g0 < o1 && g1 > o0) return SCGIB_EINVAL;
        }
        if (seg < 0) return 1;
        if (ft.ns == kFuseSegs) return SCGIB_EUNSUPPORTED;
        ft.seg_t[ft.ns] = t;
        ft.seg_job[ft.ns] = seg;
        ft.seg_o0[ft.ns] = static_cast<int32_t>(T.grad - jobs[seg].out);
        ++ft.ns;
        return 0;
    };
    if (const int rc = fill_table(tensors, n_tensors, kFuseChunk, own, tab, chunks)) return rc;
    for (int a = 0; a < ft.ns; ++a)  // each reduced element updates one tensor
        for (int c = a + 1; c < ft.ns; ++c)
            if (ft.seg_job[a] == ft.seg_job[c] &&
                ft.seg_o0[a] < ft.seg_o0[c] + tab.numel[ft.seg_t[c]] &&
                ft.seg_o0[c] < ft.seg_o0[a] + tab.numel[ft.seg_t[a]])
                return SCGIB_EINVAL;
    const dim3 grid(static_cast<unsigned>(blocks + chunks));
    if (decoupled) adam_reduce_k<H, true><<<grid, 1024, 0, st>>>(tab, ft, hp, counter);
    else adam_reduce_k<H, false><<<grid, 1024, 0, st>>>(tab, ft, hp, counter);
    return launch_status();
}

}  // namespace scgib

using namespace scgib;

extern "C" int64_t scgib_adam_max_tensors(void) { return kAdamMax; }

extern "C" int scgib_adam_step(const scgib_adam_tensor *tensors, int32_t n_tensors, double lr,
                               double beta1, double beta2, double eps, double weight_decay,
                               uint32_t *counter, scgib_stream_t stream) {
    return launch_step(tensors, n_tensors, ByValue{lr, beta1, beta2, eps, weight_decay}, false,
                       counter, as_stream(stream));
}

extern "C" int scgib_adamw_step(const scgib_adam_tensor *tensors, int32_t n_tensors, double lr,
                                double beta1, double beta2, double eps, double weight_decay,
                                uint32_t *counter, scgib_stream_t stream) {
    return launch_step(tensors, n_tensors, ByValue{lr, beta1, beta2, eps, weight_decay}, true,
                       counter, as_stream(stream));
}

extern "C" int scgib_adam_step_dyn(const scgib_adam_tensor *tensors, int32_t n_tensors,
                                   const scgib_optim_hyper *hyper, scgib_optim_state *state,
                                   double *last_lr, int32_t flags, int32_t decoupled,
                                   uint32_t *counter, scgib_stream_t stream) {
    const FromDevice hp{hyper, state, last_lr, flags};
    if (!dyn_args_ok(hp) || n_tensors < 0 || n_tensors > kAdamMax) return SCGIB_EINVAL;
    if (n_tensors == 0) {  // nothing to step: the call still counts
        if (!(flags & SCGIB_OPTIM_ADVANCE)) return SCGIB_OK;
        optim_advance_k<<<1, 64, 0, as_stream(stream)>>>(hp);
        return launch_status();
    }
    return launch_step(tensors, n_tensors, hp, decoupled != 0, counter, as_stream(stream));
}

extern "C" int64_t scgib_grad_norm_ws_doubles(int64_t n_chunks) {
    return n_chunks > 0 ? n_chunks : 1;
}

extern "C" int64_t scgib_grad_norm_chunks(const scgib_adam_tensor *tensors, int32_t n_tensors) {
    int64_t chunks = 0;
    for (int i = 0; tensors && i < n_tensors; ++i)
        if (tensors[i].numel > 0) chunks += (tensors[i].numel + kAdamChunk - 1) / kAdamChunk;
    return chunks;
}

extern "C" int scgib_grad_norm(const scgib_adam_tensor *tensors, int32_t n_tensors, double *ws,
                               uint32_t *counter, const scgib_optim_hyper *hyper,
                               scgib_optim_state *state, int32_t first, int32_t last,
                               scgib_stream_t stream) {
    if (n_tensors < 0 || n_tensors > kAdamMax || (n_tensors > 0 && !tensors)) return SCGIB_EINVAL;
    if (!ws || !counter || !hyper || !state) return SCGIB_EINVAL;
    if ((reinterpret_cast<uintptr_t>(ws) & 7) || (reinterpret_cast<uintptr_t>(hyper) & 7) ||
        (reinterpret_cast<uintptr_t>(state) & 7))
        return SCGIB_EINVAL;
    AdamTable tab;
    int64_t chunks;
    if (const int rc = fill_table(tensors, n_tensors, kAdamChunk, [](int) { return 1; }, tab,
                                  chunks))
        return rc;
    // (chunk0[n] stays the real count: a table without elements is one idle workgroup)
    grad_norm_k<<<dim3(static_cast<unsigned>(chunks > 0 ? chunks : 1)), 256, 0,
                  as_stream(stream)>>>(tab, ws, counter, hyper, state, first != 0, last != 0);
    return launch_status();
}


extern "C" int64_t scgib_grad_pack_max_tensors(void) { return kPackMax; }

extern "C" int scgib_grad_pack(const scgib_grad_slice *tensors, int32_t n_tensors, float *flat,
                               scgib_stream_t stream) {
    return launch_pack(tensors, n_tensors, flat, 1.f, false, as_stream(stream));
}

extern "C" int scgib_grad_unpack(const scgib_grad_slice *tensors, int32_t n_tensors,
                                 const float *flat, float scale, scgib_stream_t stream) {
    return launch_pack(tensors, n_tensors, const_cast<float *>(flat), scale, true,
                       as_stream(stream));
}

extern "C" int64_t scgib_adam_reduce_max_jobs(void) { return scgib::kFuseJobs; }

extern "C" int scgib_adam_step_reduce(const scgib_adam_tensor *tensors, int32_t n_tensors,
                                      const scgib_slab_job *jobs, int32_t n_jobs, double lr,
                                      double beta1, double beta2, double eps, double weight_decay,
                                      uint32_t *counter, scgib_stream_t stream) {
    return launch_step_reduce(tensors, n_tensors, jobs, n_jobs,
                              ByValue{lr, beta1, beta2, eps, weight_decay}, false, counter,
                              as_stream(stream));
}

extern "C" int scgib_adamw_step_reduce(const scgib_adam_tensor *tensors, int32_t n_tensors,
                                       const scgib_slab_job *jobs, int32_t n_jobs, double lr,
                                       double beta1, double beta2, double eps,
                                       double weight_decay, uint32_t *counter,
                                       scgib_stream_t stream) {
    return launch_step_reduce(tensors, n_tensors, jobs, n_jobs,
                              ByValue{lr, beta1, beta2, eps, weight_decay}, true, counter,
                              as_stream(stream));
}

/* (no norm launch precedes a fused reduce: SCGIB_OPTIM_NORM / _SKIP are refused) */
extern "C" int scgib_adam_step_reduce_dyn(const scgib_adam_tensor *tensors, int32_t n_tensors,
                                          const scgib_slab_job *jobs, int32_t n_jobs,
                                          const scgib_optim_hyper *hyper,
                                          scgib_optim_state *state, double *last_lr,
                                          int32_t flags, int32_t decoupled, uint32_t *counter,
                                          scgib_stream_t stream) {
    const FromDevice hp{hyper, state, last_lr, flags};
    if (!dyn_args_ok(hp) || (flags & (SCGIB_OPTIM_NORM | SCGIB_OPTIM_SKIP))) return SCGIB_EINVAL;
    if (n_jobs == 0)
        return scgib_adam_step_dyn(tensors, n_tensors, hyper, state, last_lr, flags, decoupled,
                                   counter, stream);
    return launch_step_reduce(tensors, n_tensors, jobs, n_jobs, hp, decoupled != 0, counter,
                              as_stream(stream));
}
