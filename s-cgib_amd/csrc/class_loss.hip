// Class-index cross-entropy and TU accuracy: loss_CrossEntropy of
// Mainmodel_finetuning (models.py:527-530, F.cross_entropy on the scores and
// the class column) and accuracy_TU (metrics.py:146-159) of the TU
// graph-classification loops (train_tudataset.py:146, :205), in one launch
// forward and one backward.  Labels are class indices as float32 (what the
// device loaders carry, NaN = no label), int32 or int64 (-100 = torch's
// ignore_index).  A label that is neither masked nor an integer in [0, C) is
// counted as invalid and indexes nothing.  No float atomics: a row is owned by
// one group of W lanes of a wavefront (W = 64 above 32 classes; 32, 8 or 2
// below, so that a wavefront holds 2, 8 or 32 rows of the few-class shapes the
// TU datasets have), a wavefront's rows are summed by a fixed butterfly and
// its sweeps in order, the four wavefronts of a workgroup in order, and the
// last workgroup to arrive adds the per-workgroup partials in workgroup order.
// The real shapes (B 32-2048, C 2-20) are a launch's latency: up to 128 rows
// of two classes are one workgroup, which then finishes without the arrival.
#include "common.h"

namespace scgib {

constexpr int kClassCMax = 1024;  // ops.HEAD_C_MAX
constexpr int kClassWG = 64;      // most workgroups of the forward
constexpr int kClassWaves = 4;    // wavefronts per workgroup (256 threads)
constexpr int kClassBwdWG = 256;  // most workgroups of the backward

enum { kRowMasked = 0, kRowKept = 1, kRowInvalid = 2 };

// The label of row r: kRowKept with its class in *y, kRowMasked, or
// kRowInvalid (*y is then 0: a safe index that nothing uses).
__device__ __forceinline__ int row_label(const void *labels, int ltype, int64_t r, int C, int *y) {
    *y = 0;
    if (ltype == SCGIB_LABEL_F32) {
        const float v = static_cast<const float *>(labels)[r];
        if (v != v) return kRowMasked;
        // +-inf, negatives, fractions and v >= C all fail one of these
        if (!(v >= 0.f && v < static_cast<float>(C) && v == floorf(v))) return kRowInvalid;
        *y = static_cast<int>(v);
        return kRowKept;
    }
    const int64_t v = ltype == SCGIB_LABEL_I32
                          ? static_cast<int64_t>(static_cast<const int32_t *>(labels)[r])
                          : static_cast<const int64_t *>(labels)[r];
    if (v == -100) return kRowMasked;
    if (v < 0 || v >= C) return kRowInvalid;
    *y = static_cast<int>(v);
    return kRowKept;
}

// torch's argmax order: a NaN is above every number, and among equals (or
// among NaNs) the lower index wins.
__device__ __forceinline__ bool arg_before(float av, int ai, float bv, int bi) {
    const bool an = av != av, bn = bv != bv;
    if (an != bn) return an;
    if (!an && av != bv) return av > bv;
    return ai < bi;
}

// The maximum of row s[0..C) and its first index over a group of W lanes
// (lane `sub` of the group holds classes sub, sub + W, ...); every lane of the
// group receives both.  A row that holds a NaN returns NaN and the first
// NaN's index.
template <int W>
__device__ __forceinline__ void row_argmax(const float *__restrict__ s, int C, int sub, float *mv,
                                           int *mi) {
    float bv = -INFINITY;
    int bi = 0x7fffffff;  // a lane without a class loses to every real one
    for (int c = sub; c < C; c += W) {
        const float v = s[c];
        if (arg_before(v, c, bv, bi)) {
            bv = v;
            bi = c;
        }
    }
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) {
        const float ov = __shfl_xor(bv, off, kWave);
        const int oi = __shfl_xor(bi, off, kWave);
        if (arg_before(ov, oi, bv, bi)) {
            bv = ov;
            bi = oi;
        }
    }
    *mv = bv;
    *mi = bi;
}

// sum_c exp(s_c - m): each lane in class order, then the group's fixed butterfly.
template <int W>
__device__ __forceinline__ float row_expsum(const float *__restrict__ s, int C, int sub, float m) {
    float a = 0.f;
    for (int c = sub; c < C; c += W) a += expf(s[c] - m);
#pragma unroll
    for (int off = W / 2; off >= 1; off >>= 1) a += __shfl_xor(a, off, kWave);
    return a;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ int wave_count(bool p) { return __popcll(__ballot(p)); }

// The batch's outputs from its totals, and the epoch's (one thread).
__device__ __forceinline__ void class_finish(double sum, double k, double h, double iv,
                                             float *loss, int32_t *count, int32_t *hits,
                                             int32_t *invalid, double *epoch) {
    const float mean = static_cast<float>(sum / k);  // no kept row: 0 / 0 = NaN
    *loss = mean;
    *count = static_cast<int32_t>(k);
    *hits = static_cast<int32_t>(h);
    *invalid = static_cast<int32_t>(iv);
    if (epoch) {
        if (k > 0.0) {
            epoch[0] += static_cast<double>(mean);
            epoch[1] += 1.0;
            epoch[2] += h;
            epoch[3] += k;
        }
        epoch[4] += iv;
    }
}

// forward: wavefront q of workgroup w owns rows (4 w + q) R .. + R - 1 of
// every sweep of 4 R G rows, R = 64 / W rows at a time, one per lane group.
// The rows' losses are added over the wavefront in fp64 (the group leaders'
// values through a fixed butterfly) and sweep after sweep; thread 0 adds the
// four wavefronts in order.  One workgroup: it writes the outputs.  More: each
// publishes its partials (st_agent) and the last to arrive adds them in
// workgroup order.
// ws: 4 G doubles (loss sum | kept | hits | invalid); counter: one zeroed
// uint32, left zero.  epoch (or NULL): 5 doubles, loss sum | batches | hits |
// labelled | invalid, updated by that one thread.
template <int W>
__global__ __launch_bounds__(256) void class_loss_fwd_k(
    const float *__restrict__ s, const void *__restrict__ labels, int ltype, int64_t B, int C,
    double *ws, unsigned *counter, float *__restrict__ loss, int32_t *__restrict__ count,
    int32_t *__restrict__ hits, int32_t *__restrict__ invalid, double *epoch) {
    constexpr int R = kWave / W, RW = kClassWaves * R;
    __shared__ double shl[kClassWaves];
    __shared__ int shc[kClassWaves][3];
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid >> 6, G = gridDim.x;
    const int grp = lane / W, sub = lane % W;
    double a = 0.0;
    int nk = 0, nh = 0, ni = 0;  // wavefront totals, the same on every lane
    for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * RW + wave * R; r0 < B;
         r0 += static_cast<int64_t>(G) * RW) {  // wave-uniform
        const int64_t r = r0 + grp;
        const bool in = r < B;
        const int64_t rc = in ? r : B - 1;  // lanes past the batch recompute its last row, unused
        int y;
        const int st = row_label(labels, ltype, rc, C, &y);
        const float *row = s + rc * C;
        float m;
        int am;
        row_argmax<W>(row, C, sub, &m, &am);
        const float l = logf(row_expsum<W>(row, C, sub, m)) + m - row[y];
        const bool lead = in && sub == 0, kept = lead && st == kRowKept;
        a += wave_sum_f64(kept ? static_cast<double>(l) : 0.0);
        nk += wave_count(kept);
        nh += wave_count(kept && am == y);
        ni += wave_count(lead && st == kRowInvalid);
    }
    if (lane == 0) {
        shl[wave] = a;
        shc[wave][0] = nk;
        shc[wave][1] = nh;
        shc[wave][2] = ni;
    }
    __syncthreads();
    double sum = 0.0;
    int k = 0, h = 0, iv = 0;
    if (tid == 0) {
        for (int q = 0; q < kClassWaves; ++q) {
            sum += shl[q];
            k += shc[q][0];
            h += shc[q][1];
            iv += shc[q][2];
        }
    }
    if (G == 1) {
        if (tid == 0) class_finish(sum, k, h, iv, loss, count, hits, invalid, epoch);
        return;
    }
    if (tid == 0) {
        st_agent(ws + blockIdx.x, sum);
        st_agent(ws + G + blockIdx.x, static_cast<double>(k));
        st_agent(ws + 2 * G + blockIdx.x, static_cast<double>(h));
        st_agent(ws + 3 * G + blockIdx.x, static_cast<double>(iv));
    }
    if (!block_arrive(counter, G)) return;
    if (tid == 0) {
        double ts = 0.0, tk = 0.0, th = 0.0, ti = 0.0;
        for (int w = 0; w < G; ++w) {
            ts += ld_agent(ws + w);
            tk += ld_agent(ws + G + w);
            th += ld_agent(ws + 2 * G + w);
            ti += ld_agent(ws + 3 * G + w);
        }
        class_finish(ts, tk, th, ti, loss, count, hits, invalid, epoch);
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// backward: d s_rc = g (softmax(s_r)_c - [c = y_r]) / count at kept rows, the
// softmax recomputed from the scores; exactly 0 at masked and invalid rows and
// everywhere when count = 0.  One lane group per row, as the forward.
template <int W>
__global__ __launch_bounds__(256) void class_loss_bwd_k(
    const float *__restrict__ s, const void *__restrict__ labels, int ltype, int64_t B, int C,
    const float *__restrict__ g, const int32_t *__restrict__ count, float *__restrict__ ds) {
    constexpr int R = kWave / W, RW = kClassWaves * R;
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x >> 6;
    const int grp = lane / W, sub = lane % W;
    const int32_t m = *count;
    const float gn = m > 0 ? *g / static_cast<float>(m) : 0.f;
    for (int64_t r0 = static_cast<int64_t>(blockIdx.x) * RW + wave * R; r0 < B;
         r0 += static_cast<int64_t>(gridDim.x) * RW) {  // wave-uniform
        const int64_t r = r0 + grp;
        const bool in = r < B;
        const int64_t rc = in ? r : B - 1;
        int y;
        const bool keep = row_label(labels, ltype, rc, C, &y) == kRowKept && m > 0;
        const float *row = s + rc * C;
        float mx;
        int am;
        row_argmax<W>(row, C, sub, &mx, &am);
        const float inv = 1.f / row_expsum<W>(row, C, sub, mx);
        if (in) {  // (after the group reductions: every lane took part)
            float *out = ds + r * C;
            for (int c = sub; c < C; c += W)
                out[c] = keep ? gn * (expf(row[c] - mx) * inv - (c == y ? 1.f : 0.f)) : 0.f;
        }
    }
}

}  // namespace scgib

using namespace scgib;

static int class_shape(int64_t n_rows, int32_t n_classes, int32_t label_type) {
    if (n_rows < 1 || n_classes < 1 || label_type < SCGIB_LABEL_F32 || label_type > SCGIB_LABEL_I64)
        return SCGIB_EINVAL;
    if (n_classes > kClassCMax || n_rows > (int64_t{1} << 30)) return SCGIB_EUNSUPPORTED;
    return SCGIB_OK;
}

// lanes per row: 64 / W rows share a wavefront
static int class_group(int32_t n_classes) {
    return n_classes <= 2 ? 2 : (n_classes <= 8 ? 8 : (n_classes <= 32 ? 32 : 64));
}

static unsigned class_workgroups(int64_t n_rows, int group, int most) {
    const int64_t per = kClassWaves * (kWave / group);  // rows per workgroup sweep
    const int64_t g = (n_rows + per - 1) / per;
    return static_cast<unsigned>(g > most ? most : g);
}

#define SCGIB_CLASS_DISPATCH(W, CALL) \
    switch (W) {                      \
        case 2: CALL(2); break;       \
        case 8: CALL(8); break;       \
        case 32: CALL(32); break;     \
        default: CALL(64); break;     \
    }

extern "C" int64_t scgib_class_loss_ws_doubles(void) { return 4 * kClassWG; }

extern "C" int scgib_class_loss_fwd(const float *scores, const void *labels, int32_t label_type,
                                    int64_t n_rows, int32_t n_classes, double *ws,
                                    uint32_t *counter, float *loss, int32_t *count, int32_t *hits,
                                    int32_t *invalid, double *epoch, scgib_stream_t stream) {
    if (const int rc = class_shape(n_rows, n_classes, label_type)) return rc;
    if (!scores || !labels || !ws || !counter || !loss || !count || !hits || !invalid)
        return SCGIB_EINVAL;
    if ((reinterpret_cast<uintptr_t>(ws) & 7) || (reinterpret_cast<uintptr_t>(epoch) & 7))
        return SCGIB_EINVAL;
    const int group = class_group(n_classes);
    const unsigned wg = class_workgroups(n_rows, group, kClassWG);
#define SCGIB_CLASS_FWD(W)                                                                   \
    class_loss_fwd_k<W><<<wg, 256, 0, as_stream(stream)>>>(scores, labels, label_type, n_rows, \
                                                           n_classes, ws, counter, loss, count, \
                                                           hits, invalid, epoch)
    SCGIB_CLASS_DISPATCH(group, SCGIB_CLASS_FWD)
#undef SCGIB_CLASS_FWD
    return launch_status();
}

extern "C" int scgib_class_loss_bwd(const float *scores, const void *labels, int32_t label_type,
                                    int64_t n_rows, int32_t n_classes, const float *g_loss,
                                    const int32_t *count, float *d_scores, scgib_stream_t stream) {
    if (const int rc = class_shape(n_rows, n_classes, label_type)) return rc;
    if (!scores || !labels || !g_loss || !count || !d_scores) return SCGIB_EINVAL;
    const int group = class_group(n_classes);
    const unsigned wg = class_workgroups(n_rows, group, kClassBwdWG);
#define SCGIB_CLASS_BWD(W)                                                                   \
    class_loss_bwd_k<W><<<wg, 256, 0, as_stream(stream)>>>(scores, labels, label_type, n_rows, \
                                                           n_classes, g_loss, count, d_scores)
    SCGIB_CLASS_DISPATCH(group, SCGIB_CLASS_BWD)
#undef SCGIB_CLASS_BWD
    return launch_status();
}
