// Wide fine-tune heads and NaN-masked task losses: the tail of
// Mainmodel_finetuning (models.py:510-543) for the multi-label and regression
// datasets (ogbg-molpcba 128 tasks, ToxCast 617, SIDER 27, Tox21 12,
// Peptides-func 10; QM9 / ESOL / FreeSolv / Lipo regressions),
//   scores = [sigmoid](predict(q*)),  predict = Linear(K, 64) - ReLU - Linear(64, C)
// for 16 < C <= 1024 (head.hip keeps C <= 16), and the losses the train
// scripts take through MetricWrapper(..., "ignore-flatten"): a mean over the
// elements whose target is not NaN.  The wrapper's target[~isnan] is a
// data-dependent shape (a device-host synchronise, so no graph capture); here
// the mask is applied per element inside the reduction and the kept count m
// stays on the device.  No float atomics: every output is owned by one
// thread, or is a per-workgroup slab summed by scgib_slab_reduce_multi, or a
// per-workgroup fp64 partial summed in workgroup order by the last arriver.
#include "common.h"
#include "running_update.h"

namespace scgib {

constexpr int kWideH = 64;       // hidden width (args.dims)
constexpr int kWideKMax = 128;   // input width (2 * hidden: the Set2Set output)
constexpr int kWideCMin = 17;    // below: head.hip
constexpr int kWideCMax = 1024;
constexpr int kWideRows = 16;    // rows per workgroup (forward, backward row role)
constexpr int kWideTile = 64;    // W2 column tile (outputs per LDS tile)
constexpr int kWideColsA = 16;   // backward column role: dW2 rows per workgroup
constexpr int kWideChunkA = 32;  // backward column role: rows per chunk

__device__ __forceinline__ float4 wld4(const float *p) { return *reinterpret_cast<const float4 *>(p); }
__device__ __forceinline__ float4 wzero4() { return make_float4(0.f, 0.f, 0.f, 0.f); }

// forward: workgroup (bx, by) = 16 rows x the W2 column tiles by, by + gridDim.y, ...
// Phase 1 is head_fwd_k's: W1 and the 16 x rows staged in LDS (float4 rows at
// stride K + 4), thread (r = tid >> 4, u = tid & 15) owns hidden units
// u + 16 i of row r (every by computes them; by = 0 stores hid).  Phase 2
// walks W2 in tiles of 64 outputs staged over the W1 image (rows at stride
// 68): the same thread owns outputs c0 + u + 16 i of row r, each a k-ordered
// fmaf chain over the 64 hidden units, so C is bounded by the grid and not by
// LDS.  with_ru: one more workgroup column (bx = gridDim.x - 1, by = 0) runs
// the compressor BatchNorm's running update, as in head_fwd_k.
__global__ __launch_bounds__(256) void head_wide_fwd_k(
    const float *__restrict__ x, int64_t B, int K, const float *__restrict__ w1,
    const float *__restrict__ b1, const float *__restrict__ w2, const float *__restrict__ b2, int C,
    int act, float *__restrict__ hid, float *__restrict__ out, const scgib_running_update ru,
    int with_ru) {
    if (with_ru && blockIdx.x == gridDim.x - 1) {
        if (blockIdx.y == 0) running_update_body<256>(ru);
        return;
    }
    constexpr int LH = kWideH + 4, LH4 = LH / 4;
    __shared__ float4 sW[kWideH * (kWideKMax + 4) / 4];  // W1, then the W2 tiles
    __shared__ float4 sX[kWideRows * (kWideKMax + 4) / 4];
    __shared__ float4 sH[kWideRows * LH / 4];
    const int tid = threadIdx.x, K4 = K >> 2, L4 = K4 + 1;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * kWideRows;
    const int nv = static_cast<int>(B - row0 < kWideRows ? B - row0 : kWideRows);
    {   // W1 (64 K / 4 <= 2048 float4: 8 per thread), x (16 K / 4: 2): loads, then LDS stores
        float4 vw[8], vx[2];
        const int nw = kWideH * K4, nx = kWideRows * K4;
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = tid + 256 * u;
            vw[u] = wld4(w1 + 4 * (i < nw ? i : nw - 1));
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + 256 * u, ic = i < nx ? i : nx - 1, r = ic / K4;
            vx[u] = wld4(x + (row0 + (r < nv ? r : nv - 1)) * K + 4 * (ic - r * K4));
        }
#pragma unroll
        for (int u = 0; u < 8; ++u) {
            const int i = tid + 256 * u, j = i / K4;
            if (i < nw) sW[j * L4 + (i - j * K4)] = vw[u];
        }
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int i = tid + 256 * u, r = i / K4;
            if (i < nx) sX[r * L4 + (i - r * K4)] = vx[u];
        }
    }
    __syncthreads();
    const int r = tid >> 4, u = tid & 15;
    float acc[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[i] = 0.f;
#pragma unroll 4
    for (int k4 = 0; k4 < K4; ++k4) {
        const float4 xv = sX[r * L4 + k4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const float4 w = sW[(u + 16 * i) * L4 + k4];
            acc[i] = fmaf(xv.x, w.x, acc[i]);
            acc[i] = fmaf(xv.y, w.y, acc[i]);
            acc[i] = fmaf(xv.z, w.z, acc[i]);
            acc[i] = fmaf(xv.w, w.w, acc[i]);
        }
    }
    float *sHf = reinterpret_cast<float *>(sH);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int j = u + 16 * i;
        const float h = fmaxf(acc[i] + b1[j], 0.f);
        sHf[r * LH + j] = h;
        if (blockIdx.y == 0 && r < nv) hid[(row0 + r) * kWideH + j] = h;
    }
    const int ntile = (C + kWideTile - 1) / kWideTile;
    for (int t = blockIdx.y; t < ntile; t += gridDim.y) {  // block-uniform
        const int c0 = t * kWideTile;
        const int nc = C - c0 < kWideTile ? C - c0 : kWideTile;
        // the tile's W2 rows [c0, c0 + nc) x 64: nc 16 float4 <= 1024, 4 per thread
        float4 vw[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q, ic = i < nc * 16 ? i : nc * 16 - 1;
            vw[q] = wld4(w2 + static_cast<int64_t>(c0) * kWideH + 4 * ic);
        }
        __syncthreads();  // W1 (first tile) / the previous tile has been read; sH is written
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q;
            sW[(i >> 4) * LH4 + (i & 15)] = i < nc * 16 ? vw[q] : wzero4();
        }
        __syncthreads();
        float o[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) o[i] = 0.f;
#pragma unroll 4
        for (int j4 = 0; j4 < kWideH / 4; ++j4) {
            const float4 h = sH[r * LH4 + j4];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 w = sW[(u + 16 * i) * LH4 + j4];
                o[i] = fmaf(h.x, w.x, o[i]);
                o[i] = fmaf(h.y, w.y, o[i]);
                o[i] = fmaf(h.z, w.z, o[i]);
                o[i] = fmaf(h.w, w.w, o[i]);
            }
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int c = c0 + u + 16 * i;
            if (c < C && r < nv) {
                float v = o[i] + b2[c];
                if (act) v = 1.f / (1.f + expf(-v));
                out[(row0 + r) * C + c] = v;
            }
        }
    }
}

// backward, one launch of nA + nB workgroups (do = ds * (act ? s (1 - s) : 1)):
//   column role, workgroup a < nA: dW2 rows [16 a, 16 a + 16) and their db2,
//     dW2[c][j] = sum_r do[r][c] hid[r][j] over all rows in chunks of 32;
//     thread (cg = tid >> 4, u = tid & 15) owns dW2[16 a + cg][4 u .. 4 u + 3]
//     and sums its terms in row order (threads u = 0 also db2).
//   row role, workgroup b: rows [16 b, 16 b + 16),
//     dh = (do W2) [hid > 0]  over the W2 column tiles of 64 (thread
//       (r = tid >> 4, u = tid & 15) owns dh[r][4 u .. 4 u + 3], c order),
//     dx[r][k] = sum_j dh[r][j] W1[j][k]  (thread (r, kx = tid & 15): k = kx + 16 m),
//     dW1 / db1 partials over the 16 rows (thread (jw = tid >> 4, kw = tid & 15):
//       j = jw + 16 q, k = kw + 16 m) written to row b of pw1 / pb1: the
//       per-workgroup slab that scgib_slab_reduce_multi sums in a fixed order,
//       or dW1 / db1 themselves when there is one row workgroup.
// LDS (row role): one 32 KB image holds the W2 tile (float4 rows of 64), then W1.
__global__ __launch_bounds__(256) void head_wide_bwd_k(
    const float *__restrict__ x, const float *__restrict__ hid, const float *__restrict__ s,
    const float *__restrict__ ds, int64_t B, int K, const float *__restrict__ w1,
    const float *__restrict__ w2, int C, int act, int nA, float *__restrict__ dx,
    float *__restrict__ pw1, float *__restrict__ pb1, int64_t pstride, float *__restrict__ dw2,
    float *__restrict__ db2) {
    __shared__ float4 sBig[kWideH * kWideKMax / 4];     // row role: W2 tile, then W1 [64][K]
    __shared__ float4 sX4[kWideChunkA * kWideH / 4];    // row role: x [16][K]; column role: hid [32][64]
    __shared__ float4 sDo4[kWideRows * kWideTile / 4];  // row role: do [16][64]; column role: do [32][16]
    __shared__ float sDh[kWideRows * kWideH];           // row role: dh [16][64]
    const int tid = threadIdx.x;
    if (static_cast<int>(blockIdx.x) < nA) {
        // ---- column role ----
        const int c0 = blockIdx.x * kWideColsA;
        const int cg = tid >> 4, u = tid & 15, c = c0 + cg;
        float *sDo = reinterpret_cast<float *>(sDo4);
        float4 a = wzero4();
        float ab = 0.f;
        for (int64_t r0 = 0; r0 < B; r0 += kWideChunkA) {
            const int nv = static_cast<int>(B - r0 < kWideChunkA ? B - r0 : kWideChunkA);
            // hid chunk (32 x 16 float4: 2 per thread), do chunk (32 x 16: 2 per thread)
            float4 vh[2];
            float vd[2], vs[2];
            bool ok[2];
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = tid + 256 * q, rr = i >> 4;
                vh[q] = wld4(hid + (r0 + (rr < nv ? rr : nv - 1)) * kWideH + 4 * (i & 15));
                const int cc = c0 + (i & 15);
                ok[q] = rr < nv && cc < C;
                const int64_t at = (r0 + (rr < nv ? rr : nv - 1)) * C + (cc < C ? cc : C - 1);
                vd[q] = ds[at];
                vs[q] = act ? s[at] : 0.f;
            }
            __syncthreads();  // the previous chunk's reads are done
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int i = tid + 256 * q, rr = i >> 4;
                sX4[i] = rr < nv ? vh[q] : wzero4();
                sDo[i] = ok[q] ? (act ? vd[q] * (vs[q] * (1.f - vs[q])) : vd[q]) : 0.f;
            }
            __syncthreads();
#pragma unroll 4
            for (int rr = 0; rr < kWideChunkA; ++rr) {
                const float d = sDo[rr * kWideColsA + cg];
                const float4 h = sX4[rr * 16 + u];
                a.x = fmaf(d, h.x, a.x);
                a.y = fmaf(d, h.y, a.y);
                a.z = fmaf(d, h.z, a.z);
                a.w = fmaf(d, h.w, a.w);
                ab += d;
            }
        }
        if (c < C) {
            *reinterpret_cast<float4 *>(dw2 + static_cast<int64_t>(c) * kWideH + 4 * u) = a;
            if (u == 0) db2[c] = ab;
        }
        return;
    }
    // ---- row role ----
    const int b = blockIdx.x - nA, K4 = K >> 2;
    const int64_t row0 = static_cast<int64_t>(b) * kWideRows;
    const int nv = static_cast<int>(B - row0 < kWideRows ? B - row0 : kWideRows);
    const int r = tid >> 4, u = tid & 15;
    float *sDo = reinterpret_cast<float *>(sDo4), *sX = reinterpret_cast<float *>(sX4);
    float *sW = reinterpret_cast<float *>(sBig);
    {   // x rows (16 K / 4 <= 512 float4: 2 per thread), zero past nv
        const int nx = kWideRows * K4;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const int i = tid + 256 * q, ic = i < nx ? i : nx - 1, rr = ic / K4;
            const float4 v = wld4(x + (row0 + (rr < nv ? rr : nv - 1)) * K + 4 * (ic - rr * K4));
            if (i < nx) sX4[i] = rr < nv ? v : wzero4();
        }
    }
    float4 dh = wzero4();
    const int ntile = (C + kWideTile - 1) / kWideTile;
    for (int t = 0; t < ntile; ++t) {
        const int c0 = t * kWideTile;
        const int nc = C - c0 < kWideTile ? C - c0 : kWideTile;
        // W2 tile rows [c0, c0 + nc) (nc 16 float4: 4 per thread), do [16][64] (4 per thread)
        float4 vw[4];
        float vd[4], vs[4];
        bool ok[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q, ic = i < nc * 16 ? i : nc * 16 - 1;
            vw[q] = wld4(w2 + static_cast<int64_t>(c0) * kWideH + 4 * ic);
            const int rr = i >> 6, cc = i & 63;
            ok[q] = rr < nv && cc < nc;
            const int64_t at = (row0 + (rr < nv ? rr : nv - 1)) * C + c0 + (cc < nc ? cc : nc - 1);
            vd[q] = ds[at];
            vs[q] = act ? s[at] : 0.f;
        }
        __syncthreads();  // the previous tile's reads are done
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int i = tid + 256 * q;
            sBig[i] = i < nc * 16 ? vw[q] : wzero4();
            sDo[i] = ok[q] ? (act ? vd[q] * (vs[q] * (1.f - vs[q])) : vd[q]) : 0.f;
        }
        __syncthreads();
#pragma unroll 4
        for (int c4 = 0; c4 < kWideTile / 4; ++c4) {
            const float4 d = sDo4[r * (kWideTile / 4) + c4];
            const float dv[4] = {d.x, d.y, d.z, d.w};
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const float4 w = sBig[(4 * c4 + e) * 16 + u];
                dh.x = fmaf(dv[e], w.x, dh.x);
                dh.y = fmaf(dv[e], w.y, dh.y);
                dh.z = fmaf(dv[e], w.z, dh.z);
                dh.w = fmaf(dv[e], w.w, dh.w);
            }
        }
    }
    {   // the ReLU mask, dh to LDS; W1 [64][K] over the W2 tile
        const float4 h = wld4(hid + (row0 + (r < nv ? r : nv - 1)) * kWideH + 4 * u);
        float4 vw[8];
        const int nw = kWideH * K4;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = tid + 256 * q;
            vw[q] = wld4(w1 + 4 * (i < nw ? i : nw - 1));
        }
        __syncthreads();  // the last tile's reads are done
        sDh[r * kWideH + 4 * u + 0] = h.x > 0.f ? dh.x : 0.f;
        sDh[r * kWideH + 4 * u + 1] = h.y > 0.f ? dh.y : 0.f;
        sDh[r * kWideH + 4 * u + 2] = h.z > 0.f ? dh.z : 0.f;
        sDh[r * kWideH + 4 * u + 3] = h.w > 0.f ? dh.w : 0.f;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const int i = tid + 256 * q;
            if (i < nw) sBig[i] = vw[q];
        }
        __syncthreads();
    }
    {   // dx[r][k], k = u + 16 m.  Unconditional in k (as head_bwd_k): for
        // K < 128 the reads past column K stay inside the 64 x 128 image
        // (j K + k <= 63 K + 127 < 8192) and are never written out.
        float a[8];
#pragma unroll
        for (int m = 0; m < 8; ++m) a[m] = 0.f;
#pragma unroll 4
        for (int j = 0; j < kWideH; ++j) {
            const float d = sDh[r * kWideH + j];
#pragma unroll
            for (int m = 0; m < 8; ++m) a[m] = fmaf(d, sW[j * K + u + 16 * m], a[m]);
        }
        if (r < nv) {
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int k = u + 16 * m;
                if (k < K) dx[(row0 + r) * K + k] = a[m];
            }
        }
    }
    {   // dW1[j][k] partial: j = r + 16 q, k = u + 16 m over the 16 rows (row
        // order); reads past column K stay inside x's 16 x 128 image
        // (rr K + k <= 15 K + 127 < 2048) and are never written out.
        float a[4][8];
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int m = 0; m < 8; ++m) a[q][m] = 0.f;
#pragma unroll 2
        for (int rr = 0; rr < kWideRows; ++rr) {
            float d[4], xv[8];
#pragma unroll
            for (int q = 0; q < 4; ++q) d[q] = sDh[rr * kWideH + r + 16 * q];
#pragma unroll
            for (int m = 0; m < 8; ++m) xv[m] = sX[rr * K + u + 16 * m];
#pragma unroll
            for (int q = 0; q < 4; ++q)
#pragma unroll
                for (int m = 0; m < 8; ++m) a[q][m] = fmaf(d[q], xv[m], a[q][m]);
        }
        float *ow = pw1 + static_cast<int64_t>(b) * pstride;
#pragma unroll
        for (int q = 0; q < 4; ++q)
#pragma unroll
            for (int m = 0; m < 8; ++m) {
                const int k = u + 16 * m;
                if (k < K) ow[(r + 16 * q) * K + k] = a[q][m];
            }
        if (tid < kWideH) {
            float sb = 0.f;
            for (int rr = 0; rr < kWideRows; ++rr) sb += sDh[rr * kWideH + tid];
            pb1[static_cast<int64_t>(b) * pstride + tid] = sb;
        }
    }
}

// ---- NaN-masked mean losses ------------------------------------------------
// kind: SCGIB_LOSS_BCE / _BCE_LOGITS / _MAE / _RMSE; per kept element (fp32,
// torch's formulas)
//   bce         (t - 1) max(log(1 - s), -100) - t max(log s, -100)
//   bce_logits  max(x, 0) - x t + log1p(exp(-|x|))
//   mae         |s - t|
//   rmse        (s - t)^2                     (loss = sqrt(sum / m))
// An element is kept when its target is not NaN (mask_nan) or always.
constexpr int kLossWG = 64;    // most workgroups of the forward
constexpr int kLossPer = 2048; // elements per workgroup before another one is added

__device__ __forceinline__ float loss_term(int kind, float s, float t) {
    switch (kind) {
        case SCGIB_LOSS_BCE:
            return (t - 1.f) * fmaxf(logf(1.f - s), -100.f) - t * fmaxf(logf(s), -100.f);
        case SCGIB_LOSS_BCE_LOGITS:
            return fmaxf(s, 0.f) - s * t + log1pf(expf(-fabsf(s)));
        case SCGIB_LOSS_MAE:
            return fabsf(s - t);
        default: {
            const float d = s - t;
            return d * d;
        }
    }
}

// forward: workgroup w sums elements w 256 + tid, + G 256, ... (fp64, a fixed
// tree over the 256 threads), publishes its partial sum and count (st_agent),
// and the last workgroup to arrive adds the G partials in workgroup order.
// ws: 2 G doubles; counter: one zeroed uint32, left zero.
__global__ __launch_bounds__(256) void task_loss_fwd_k(const float *__restrict__ s,
                                                       const float *__restrict__ t, int64_t n,
                                                       int kind, int mask_nan, double *ws,
                                                       unsigned *counter, float *__restrict__ loss,
                                                       int32_t *__restrict__ count) {
    __shared__ double sh[256];
    __shared__ int shn[256];
    const int tid = threadIdx.x, G = gridDim.x;
    double a = 0.0;
    int m = 0;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + tid; i < n; i += static_cast<int64_t>(G) * 256) {
        const float tv = t[i], sv = s[i];
        const bool keep = !mask_nan || tv == tv;
        const float l = loss_term(kind, sv, tv);
        a += keep ? static_cast<double>(l) : 0.0;
        m += keep ? 1 : 0;
    }
    sh[tid] = a;
    shn[tid] = m;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if (tid < w) {
            sh[tid] += sh[tid + w];
            shn[tid] += shn[tid + w];
        }
        __syncthreads();
    }
    if (tid == 0) {
        st_agent(ws + blockIdx.x, sh[0]);
        st_agent(ws + G + blockIdx.x, static_cast<double>(shn[0]));
    }
    if (!block_arrive(counter, G)) return;
    if (tid == 0) {
        double sum = 0.0, cnt = 0.0;
        for (int w = 0; w < G; ++w) {
            sum += ld_agent(ws + w);
            cnt += ld_agent(ws + G + w);
        }
        const double mean = sum / cnt;  // m = 0: 0 / 0 = NaN, torch's mean over an empty tensor
        *loss = static_cast<float>(kind == SCGIB_LOSS_RMSE ? sqrt(mean) : mean);
        *count = static_cast<int32_t>(cnt);
        __hip_atomic_store(counter, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

// backward: d scores = g * d loss / d s, exactly 0 at masked elements (and
// everywhere when m = 0):
//   bce         g (s - t) / max((1 - s) s, 1e-12) / m
//   bce_logits  g (sigmoid(x) - t) / m
//   mae         g sign(s - t) / m
//   rmse        g (s - t) / (m loss)
__global__ __launch_bounds__(256) void task_loss_bwd_k(const float *__restrict__ s,
                                                       const float *__restrict__ t, int64_t n,
                                                       int kind, int mask_nan,
                                                       const float *__restrict__ g,
                                                       const float *__restrict__ loss,
                                                       const int32_t *__restrict__ count,
                                                       float *__restrict__ ds) {
    const int32_t m = *count;
    float gn = m > 0 ? *g / static_cast<float>(m) : 0.f;
    if (kind == SCGIB_LOSS_RMSE && m > 0) gn = gn / *loss;
    for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < n;
         i += static_cast<int64_t>(gridDim.x) * 256) {
        const float sv = s[i], tv = t[i];
        const bool keep = m > 0 && (!mask_nan || tv == tv);
        const float df = sv - tv;
        float d;
        switch (kind) {
            case SCGIB_LOSS_BCE: d = gn * df / fmaxf((1.f - sv) * sv, 1e-12f); break;
            case SCGIB_LOSS_BCE_LOGITS: d = gn * (1.f / (1.f + expf(-sv)) - tv); break;
            case SCGIB_LOSS_MAE: d = df > 0.f ? gn : (df < 0.f ? -gn : df * gn); break;  // sign(0) = 0
            default: d = gn * df; break;
        }
        ds[i] = keep ? d : 0.f;
    }
}

}  // namespace scgib

using namespace scgib;

static bool wide_aligned(const void *p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }

static int wide_shape(int64_t n_rows, int32_t k_in, int32_t n_out) {
    if (n_rows < 0 || k_in < 1 || n_out < 1) return SCGIB_EINVAL;
    if (k_in > kWideKMax || k_in % 4 || n_out < kWideCMin || n_out > kWideCMax ||
        n_rows > (int64_t{1} << 30))
        return SCGIB_EUNSUPPORTED;
    return SCGIB_OK;
}

static int64_t wide_row_groups(int64_t n_rows) { return (n_rows + kWideRows - 1) / kWideRows; }

extern "C" int64_t scgib_head_wide_slab_floats(int64_t n_rows, int32_t k_in) {
    const int64_t nb = wide_row_groups(n_rows);
    return nb > 1 ? nb * (static_cast<int64_t>(kWideH) * k_in + kWideH) : 0;
}

extern "C" int scgib_head_wide_fwd(const float *x, int64_t n_rows, int32_t k_in, const float *w1,
                                   const float *b1, const float *w2, const float *b2,
                                   int32_t n_out, int32_t sigmoid, float *hid, float *out,
                                   const scgib_running_update *ru, scgib_stream_t stream) {
    if (const int rc = wide_shape(n_rows, k_in, n_out)) return rc;
    if (n_rows == 0) return SCGIB_OK;
    if (!x || !w1 || !b1 || !w2 || !b2 || !hid || !out) return SCGIB_EINVAL;
    if (!wide_aligned(x) || !wide_aligned(w1) || !wide_aligned(w2)) return SCGIB_EUNSUPPORTED;
    if (ru && (ru->n_graphs < 1 || !ru->stats || !ru->graph_ptr || !ru->running_mean ||
               !ru->running_var))
        return SCGIB_EINVAL;
    const int64_t nb = wide_row_groups(n_rows);
    const int ntile = (n_out + kWideTile - 1) / kWideTile;
    // column tiles spread over workgroups while the grid stays within one wave of the chip
    int64_t gy = 256 / nb;
    gy = gy < 1 ? 1 : (gy > ntile ? ntile : gy);
    const dim3 grid(static_cast<unsigned>(nb + (ru ? 1 : 0)), static_cast<unsigned>(gy));
    head_wide_fwd_k<<<grid, 256, 0, as_stream(stream)>>>(x, n_rows, k_in, w1, b1, w2, b2, n_out,
                                                         sigmoid ? 1 : 0, hid, out,
                                                         ru ? *ru : scgib_running_update{},
                                                         ru ? 1 : 0);
    return launch_status();
}

extern "C" int scgib_head_wide_bwd(const float *x, const float *hid, const float *out,
                                   const float *d_out, int64_t n_rows, int32_t k_in,
                                   const float *w1, const float *w2, int32_t n_out,
                                   int32_t sigmoid, float *dx, float *dw1, float *db1, float *dw2,
                                   float *db2, float *slab, scgib_stream_t stream) {
    if (const int rc = wide_shape(n_rows, k_in, n_out)) return rc;
    if (!dw1 || !db1 || !dw2 || !db2) return SCGIB_EINVAL;
    hipStream_t st = as_stream(stream);
    if (n_rows == 0) {  // an empty batch (the forward accepted it): zero weight gradients
        hipError_t e = hipMemsetAsync(dw1, 0, sizeof(float) * kWideH * k_in, st);
        if (e == hipSuccess) e = hipMemsetAsync(db1, 0, sizeof(float) * kWideH, st);
        if (e == hipSuccess) e = hipMemsetAsync(dw2, 0, sizeof(float) * kWideH * n_out, st);
        if (e == hipSuccess) e = hipMemsetAsync(db2, 0, sizeof(float) * n_out, st);
        return e == hipSuccess ? SCGIB_OK : static_cast<int>(e);
    }
    if (!x || !hid || !out || !d_out || !w1 || !w2 || !dx) return SCGIB_EINVAL;
    if (!wide_aligned(x) || !wide_aligned(w1) || !wide_aligned(w2) || !wide_aligned(hid) ||
        !wide_aligned(dw2))
        return SCGIB_EUNSUPPORTED;
    const int64_t nb = wide_row_groups(n_rows);
    const int nA = (n_out + kWideColsA - 1) / kWideColsA;
    const int64_t width = static_cast<int64_t>(kWideH) * k_in;
    if (nb > 1 && !slab) return SCGIB_EINVAL;
    float *pw1 = nb > 1 ? slab : dw1, *pb1 = nb > 1 ? slab + width : db1;
    head_wide_bwd_k<<<static_cast<unsigned>(nA + nb), 256, 0, st>>>(
        x, hid, out, d_out, n_rows, k_in, w1, w2, n_out, sigmoid ? 1 : 0, nA, dx, pw1, pb1,
        nb > 1 ? width + kWideH : 0, dw2, db2);
    if (const int rc = launch_status()) return rc;
    if (nb == 1) return SCGIB_OK;
    const int32_t stride = static_cast<int32_t>(width + kWideH);
    const scgib_slab_job jobs[2] = {{slab, dw1, width, static_cast<int32_t>(nb), stride},
                                    {slab + width, db1, kWideH, static_cast<int32_t>(nb), stride}};
    return scgib_slab_reduce_multi(jobs, 2, stream);
}

static int loss_shape(int64_t n, int32_t kind) {
    if (n < 1 || kind < SCGIB_LOSS_BCE || kind > SCGIB_LOSS_RMSE) return SCGIB_EINVAL;
    return n > 0x7fffffff ? SCGIB_EUNSUPPORTED : SCGIB_OK;  // count is an int32
}

static unsigned loss_workgroups(int64_t n) {
    const int64_t g = (n + kLossPer - 1) / kLossPer;
    return static_cast<unsigned>(g < 1 ? 1 : (g > kLossWG ? kLossWG : g));
}

extern "C" int64_t scgib_task_loss_ws_doubles(void) { return 2 * kLossWG; }

extern "C" int scgib_task_loss_fwd(const float *scores, const float *targets, int64_t n,
                                   int32_t kind, int32_t mask_nan, double *ws, uint32_t *counter,
                                   float *loss, int32_t *count, scgib_stream_t stream) {
    if (const int rc = loss_shape(n, kind)) return rc;
    if (!scores || !targets || !ws || !counter || !loss || !count) return SCGIB_EINVAL;
    task_loss_fwd_k<<<loss_workgroups(n), 256, 0, as_stream(stream)>>>(
        scores, targets, n, kind, mask_nan ? 1 : 0, ws, counter, loss, count);
    return launch_status();
}

extern "C" int scgib_task_loss_bwd(const float *scores, const float *targets, int64_t n,
                                   int32_t kind, int32_t mask_nan, const float *g_loss,
                                   const float *loss, const int32_t *count, float *d_scores,
                                   scgib_stream_t stream) {
    if (const int rc = loss_shape(n, kind)) return rc;
    if (!scores || !targets || !g_loss || !loss || !count || !d_scores) return SCGIB_EINVAL;
    const int64_t wg = (n + 255) / 256;
    task_loss_bwd_k<<<static_cast<unsigned>(wg < 256 ? wg : 256), 256, 0, as_stream(stream)>>>(
        scores, targets, n, kind, mask_nan ? 1 : 0, g_loss, loss, count, d_scores);
    return launch_status();
}
