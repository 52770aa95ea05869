// Evaluation metrics on the device (gfx950): a score buffer that a replayed
// step appends to, and per-task ROC-AUC / AP / RMSE / accuracy over it
// (DESIGN.md §13).
//
// Reference: metrics.py:18-87 (eval_rocauc / eval_ap / eval_rmse / eval_acc)
// copies every score and label to the host and calls sklearn per task column;
// the loops concatenate the epoch's scores with torch.cat
// (train_molpcba.py:156-159, evaluate_network :165-207).
//
// eval_append_k: copies a [B][C] batch of scores and labels to the buffer's
//   row cursor (device uint32); the last workgroup to arrive (block_arrive)
//   advances the cursor, so nothing synchronises and the launch replays.
//   Rows that would pass the capacity are not written; the cursor stops at
//   the capacity and the overflow bit is set.
// eval_keys_k, grid (row tiles of 64, task tiles of 64): reads the row-major
//   [n][C] buffers coalesced along the tasks, writes task-major 64-bit keys
//   [Cg][n] coalesced along the rows, through an LDS tile.  key = (~ord(score)
//   << 1) | label, ord the order-preserving uint32 image of the fp32 score
//   (-0.0 taken as +0.0), so an ASCENDING integer sort is the descending score
//   order with the label carried in the low bit; elements without a 0/1 label
//   and rows past the cursor get INT64_MAX.  Per (row tile, task) it leaves
//   the counts of labels equal to 1 / equal to 0 / not NaN / equal to their
//   score and the squared error (fp64) in a slab: every sum is taken in a
//   fixed order, no floating-point atomics.  Error bits are OR-ed into *err.
// eval_scan_k, one workgroup per task: sums the task's slab column (P, N,
//   labelled, matches, squared error), then walks the m = P + N valid sorted
//   keys in chunks of 1024 (4 per thread).  A tie group ends where the next
//   key's score bits differ or at element m - 1.  TP is a block-wide inclusive
//   sum scan of the label bits (FP = position - TP); the (position, TP) pair
//   at the previous group end comes from an exclusive max scan of the pairs
//   masked to the group ends, packed into one uint64 (both are monotone, so
//   the packed maximum is the latest end).  Running TP and the last end are
//   carried across chunks.  With TP', FP' the counts at the previous end:
//     AUC = sum (FP - FP') (TP + TP') / (2 P N)   int64 sum, one fp64 division
//     AP  = sum (TP - TP') TP / (TP + FP) / P     fp64, fixed order
// which are sklearn's trapezoid and step sums restated as counts.
#include "common.h"

namespace scgib {

constexpr int kEvTile = 64;
constexpr int kEvThreads = 256;
constexpr int kEvItems = 4;
constexpr int kEvChunk = kEvThreads * kEvItems;
constexpr uint32_t kEvErrOverflow = 1;  // an append passed the capacity
constexpr uint32_t kEvErrNanScore = 2;  // NaN score on a labelled element
constexpr uint32_t kEvErrLabel = 4;     // a label that is neither 0, 1 nor NaN
constexpr int64_t kEvSentinel = INT64_MAX;

__device__ __forceinline__ uint32_t ev_ld(const uint32_t *p) {
    return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void ev_st(uint32_t *p, uint32_t v) {
    __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}

// state: [0] row cursor, [1] arrival counter (zero between launches), [2] error word
__global__ __launch_bounds__(kEvThreads) void eval_append_k(
    const float *__restrict__ scores, const float *__restrict__ targets, int64_t n_rows,
    int64_t n_tasks, float *__restrict__ buf_scores, float *__restrict__ buf_labels,
    int64_t capacity, uint32_t *state) {
    const int64_t cur = ev_ld(state);
    const int64_t base = cur * n_tasks, lim = capacity * n_tasks, total = n_rows * n_tasks;
    const int64_t step = static_cast<int64_t>(gridDim.x) * kEvThreads;
    for (int64_t e = static_cast<int64_t>(blockIdx.x) * kEvThreads + threadIdx.x; e < total;
         e += step) {
        // lim - base is a whole number of rows: a row is stored whole or not at all
        if (base + e < lim) {
            buf_scores[base + e] = scores[e];
            buf_labels[base + e] = targets[e];
        }
    }
    if (block_arrive(state + 1, gridDim.x) && threadIdx.x == 0) {
        int64_t next = cur + n_rows;
        if (next > capacity) {
            next = capacity;
            atomicOr(state + 2, kEvErrOverflow);
        }
        ev_st(state, static_cast<uint32_t>(next));
        ev_st(state + 1, 0u);
    }
}

__device__ __forceinline__ int64_t ev_key(float s, bool positive) {
    uint32_t u = __float_as_uint(s);
    if ((u << 1) == 0u) u = 0u;  // -0.0 ties with +0.0
    const uint32_t ord = (u & 0x80000000u) ? ~u : (u | 0x80000000u);  // ascending in s
    const uint32_t desc = ~ord;
    return static_cast<int64_t>((static_cast<uint64_t>(desc) << 1) | (positive ? 1u : 0u));
}

__global__ __launch_bounds__(kEvThreads) void eval_keys_k(
    const float *__restrict__ scores, const float *__restrict__ labels, int64_t n, int C,
    int task0, int ng, const uint32_t *__restrict__ rows, int64_t *__restrict__ keys,
    double *__restrict__ sq_slab, int4 *__restrict__ cnt_slab, uint32_t *err) {
    __shared__ int64_t tile[kEvTile][kEvTile + 1];
    __shared__ double s_sq[4][kEvTile];
    __shared__ int4 s_cnt[4][kEvTile];
    const int tid = threadIdx.x, g = tid >> 6, c = tid & 63;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kEvTile;
    const int ct0 = blockIdx.y * kEvTile;
    int64_t live = n;
    if (rows) {
        const int64_t r = rows[0];
        live = r < n ? r : n;
    }
    const bool cok = ct0 + c < ng;
    const int tc = task0 + ct0 + c;

    // read side: lane = task (contiguous in memory), 16 rows per thread
    float sv[16], yv[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int64_t row = row0 + g + 4 * i;
        const bool ok = cok && row < live;
        const int64_t at = row * C + tc;
        sv[i] = ld_ok(scores, at, 0, ok, 0.f);
        yv[i] = ld_ok(labels, at, 0, ok, __builtin_nanf(""));
    }
    double sq = 0.0;
    int pos = 0, neg = 0, lab = 0, mat = 0;
    uint32_t e = 0;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const float s = sv[i], y = yv[i];
        int64_t key = kEvSentinel;
        if (y == y) {  // labelled (a row past the cursor was given a NaN label)
            ++lab;
            if (s != s) e |= kEvErrNanScore;
            const double d = static_cast<double>(y) - static_cast<double>(s);
            sq += d * d;
            mat += (s == y) ? 1 : 0;
            if (y == 1.f) {
                ++pos;
                key = ev_key(s, true);
            } else if (y == 0.f) {
                ++neg;
                key = ev_key(s, false);
            } else {
                e |= kEvErrLabel;
            }
        }
        tile[c][g + 4 * i] = key;
    }
    s_sq[g][c] = sq;
    s_cnt[g][c] = make_int4(pos, neg, lab, mat);
    if (e) atomicOr(err, e);
    __syncthreads();
    if (g == 0 && cok) {
        double t = s_sq[0][c];
        int4 k = s_cnt[0][c];
#pragma unroll
        for (int q = 1; q < 4; ++q) {
            t += s_sq[q][c];
            const int4 v = s_cnt[q][c];
            k.x += v.x; k.y += v.y; k.z += v.z; k.w += v.w;
        }
        const int64_t at = static_cast<int64_t>(blockIdx.x) * C + tc;
        sq_slab[at] = t;
        cnt_slab[at] = k;
    }
    // write side: lane = row (contiguous in the task-major keys)
    const int64_t row = row0 + c;
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        const int cc = g + 4 * i;
        if (ct0 + cc < ng && row < n)
            keys[static_cast<int64_t>(ct0 + cc) * n + row] = tile[cc][c];
    }
}

// Fixed-order block sum (butterfly per wave, then the four waves in order);
// every thread receives the total.  `smem`: 4 values, reused across calls.
template <class T>
__device__ __forceinline__ T ev_block_sum(T v, T *smem) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    __syncthreads();  // earlier readers of smem are done
    if ((threadIdx.x & 63) == 0) smem[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((smem[0] + smem[1]) + smem[2]) + smem[3];
}

__global__ __launch_bounds__(kEvThreads) void eval_scan_k(
    const int64_t *__restrict__ sorted, int64_t n, int C, int task0, int64_t n_tiles,
    const double *__restrict__ sq_slab, const int4 *__restrict__ cnt_slab,
    double *__restrict__ out, int32_t *__restrict__ counts) {
    __shared__ double s_d[4];
    __shared__ long long s_l[4];
    __shared__ uint32_t s_sum[4];
    __shared__ uint64_t s_max[4];
    const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
    const int tc = task0 + blockIdx.x;

    // the task's totals from the key kernel's slab column
    double sq = 0.0;
    long long pos = 0, neg = 0, lab = 0, mat = 0;
    for (int64_t t = tid; t < n_tiles; t += kEvThreads) {
        sq += sq_slab[t * C + tc];
        const int4 v = cnt_slab[t * C + tc];
        pos += v.x; neg += v.y; lab += v.z; mat += v.w;
    }
    sq = ev_block_sum(sq, s_d);
    pos = ev_block_sum(pos, s_l);
    neg = ev_block_sum(neg, s_l);
    lab = ev_block_sum(lab, s_l);
    mat = ev_block_sum(mat, s_l);

    const int64_t m = pos + neg;  // valid keys: a prefix of the sorted row
    const uint64_t *k = reinterpret_cast<const uint64_t *>(sorted) +
                        static_cast<int64_t>(blockIdx.x) * n;
    uint32_t carry_tp = 0;   // positives before this chunk
    uint64_t carry_pk = 0;   // (position << 32 | TP) at the last group end before it
    long long num = 0;
    double ap = 0.0;
    for (int64_t base = 0; base < m; base += kEvChunk) {
        const int64_t i0 = base + static_cast<int64_t>(tid) * kEvItems;
        uint64_t key[kEvItems + 1];
#pragma unroll
        for (int j = 0; j <= kEvItems; ++j)
            key[j] = ld_ok(k, i0 + j, 0, i0 + j < m, static_cast<uint64_t>(0));
        uint32_t tp[kEvItems];
        bool end[kEvItems];
        uint32_t run = 0;
#pragma unroll
        for (int j = 0; j < kEvItems; ++j) {
            const bool valid = i0 + j < m;
            run += valid ? static_cast<uint32_t>(key[j] & 1u) : 0u;
            tp[j] = run;
            end[j] = valid && (i0 + j == m - 1 || (key[j + 1] >> 1) != (key[j] >> 1));
        }
        // block-wide inclusive sum scan of the positives
        uint32_t inc = run;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint32_t v = __shfl_up(inc, off, kWave);
            if (lane >= off) inc += v;
        }
        if (lane == kWave - 1) s_sum[w] = inc;
        __syncthreads();
        uint32_t before = carry_tp + inc - run, total = 0;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint32_t v = s_sum[q];
            if (q < w) before += v;
            total += v;
        }
        // block-wide exclusive max scan of the packed group ends
        uint64_t pk[kEvItems];
        uint64_t last = 0;
#pragma unroll
        for (int j = 0; j < kEvItems; ++j) {
            pk[j] = (static_cast<uint64_t>(i0 + j + 1) << 32) | (before + tp[j]);
            if (end[j]) last = pk[j];
        }
        uint64_t mx = last;
#pragma unroll
        for (int off = 1; off < kWave; off <<= 1) {
            const uint64_t v = __shfl_up(mx, off, kWave);
            if (lane >= off && v > mx) mx = v;
        }
        uint64_t prev = __shfl_up(mx, 1, kWave);
        if (lane == 0) prev = 0;
        if (lane == kWave - 1) s_max[w] = mx;
        __syncthreads();
        uint64_t chunk_last = carry_pk;
        if (carry_pk > prev) prev = carry_pk;
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const uint64_t v = s_max[q];
            if (q < w && v > prev) prev = v;
            if (v > chunk_last) chunk_last = v;
        }
#pragma unroll
        for (int j = 0; j < kEvItems; ++j) {
            if (!end[j]) continue;
            const long long tp1 = static_cast<uint32_t>(pk[j]), at1 = pk[j] >> 32;
            const long long tp0 = static_cast<uint32_t>(prev), at0 = prev >> 32;
            const long long dtp = tp1 - tp0, dfp = (at1 - tp1) - (at0 - tp0);
            num += dfp * (tp1 + tp0);
            if (dtp) ap += static_cast<double>(dtp * tp1) / static_cast<double>(at1);
            prev = pk[j];
        }
        carry_tp += total;
        carry_pk = chunk_last;
    }
    num = ev_block_sum(num, s_l);
    ap = ev_block_sum(ap, s_d);
    if (tid == 0) {
        const double nan = __builtin_nan("");
        const bool both = pos > 0 && neg > 0;
        const int64_t Cc = C;
        out[0 * Cc + tc] = both ? static_cast<double>(num) /
                                      (2.0 * static_cast<double>(pos) * static_cast<double>(neg))
                                : nan;
        out[1 * Cc + tc] = both ? ap / static_cast<double>(pos) : nan;
        out[2 * Cc + tc] = lab > 0 ? sqrt(sq / static_cast<double>(lab)) : nan;
        out[3 * Cc + tc] = lab > 0 ? static_cast<double>(mat) / static_cast<double>(lab) : nan;
        counts[0 * Cc + tc] = static_cast<int32_t>(pos);
        counts[1 * Cc + tc] = static_cast<int32_t>(neg);
        counts[2 * Cc + tc] = static_cast<int32_t>(lab);
    }
}

}  // namespace scgib

using namespace scgib;

extern "C" int64_t scgib_eval_tiles(int64_t n_rows) {
    return n_rows <= 0 ? 0 : (n_rows + kEvTile - 1) / kEvTile;
}

extern "C" int scgib_eval_append(const float *scores, const float *targets, int64_t n_rows,
                                 int32_t n_tasks, float *buf_scores, float *buf_labels,
                                 int64_t capacity, uint32_t *state, scgib_stream_t stream) {
    if (n_rows < 0 || n_tasks <= 0 || capacity <= 0) return SCGIB_EINVAL;
    if (!buf_scores || !buf_labels || !state) return SCGIB_EINVAL;
    if (n_rows == 0) return SCGIB_OK;
    if (!scores || !targets) return SCGIB_EINVAL;
    if (capacity > 0x7fffffff || n_rows > 0x7fffffff) return SCGIB_EUNSUPPORTED;
    const int64_t total = n_rows * n_tasks;
    int64_t grid = (total + kEvThreads - 1) / kEvThreads;
    if (grid > 1024) grid = 1024;
    eval_append_k<<<static_cast<unsigned>(grid), kEvThreads, 0, as_stream(stream)>>>(
        scores, targets, n_rows, n_tasks, buf_scores, buf_labels, capacity, state);
    return launch_status();
}

extern "C" int scgib_eval_keys(const float *scores, const float *labels, int64_t n_rows,
                               int32_t n_tasks, int32_t task0, int32_t n_group,
                               const uint32_t *rows, int64_t *keys, double *sq_slab,
                               int32_t *cnt_slab, uint32_t *err, scgib_stream_t stream) {
    if (n_rows <= 0 || n_tasks <= 0 || task0 < 0 || n_group <= 0 || task0 + n_group > n_tasks)
        return SCGIB_EINVAL;
    if (!scores || !labels || !keys || !sq_slab || !cnt_slab || !err) return SCGIB_EINVAL;
    if (n_rows > 0x7fffffff) return SCGIB_EUNSUPPORTED;
    const dim3 grid(static_cast<unsigned>(scgib_eval_tiles(n_rows)),
                    static_cast<unsigned>((n_group + kEvTile - 1) / kEvTile));
    if (grid.y > 65535) return SCGIB_EUNSUPPORTED;
    eval_keys_k<<<grid, kEvThreads, 0, as_stream(stream)>>>(
        scores, labels, n_rows, n_tasks, task0, n_group, rows, keys, sq_slab,
        reinterpret_cast<int4 *>(cnt_slab), err);
    return launch_status();
}

extern "C" int scgib_eval_scan(const int64_t *sorted, int64_t n_rows, int32_t n_tasks,
                               int32_t task0, int32_t n_group, const double *sq_slab,
                               const int32_t *cnt_slab, double *out, int32_t *counts,
                               scgib_stream_t stream) {
    if (n_rows <= 0 || n_tasks <= 0 || task0 < 0 || n_group <= 0 || task0 + n_group > n_tasks)
        return SCGIB_EINVAL;
    if (!sorted || !sq_slab || !cnt_slab || !out || !counts) return SCGIB_EINVAL;
    if (n_rows > 0x7fffffff) return SCGIB_EUNSUPPORTED;
    eval_scan_k<<<static_cast<unsigned>(n_group), kEvThreads, 0, as_stream(stream)>>>(
        sorted, n_rows, n_tasks, task0, scgib_eval_tiles(n_rows), sq_slab,
        reinterpret_cast<const int4 *>(cnt_slab), out, counts);
    return launch_status();
}
