// Molecule-resident eval forward (gfx950): with every BatchNorm on its running
// statistics and no loss, the model is a pure function of one molecule, so one
// workgroup carries a molecule from its raw features to its pooled vector
// without a layer output in global memory, and a batch is ONE launch
// (scgib_infer_fwd; ops.infer_forward, infer.Scorer).
//
// Walk of a workgroup (256 threads, 4 waves) for each of its molecules
// g = blockIdx.x, blockIdx.x + gridDim.x, ... (rows [r0, r1) of the batch,
// n = r1 - r0 <= kInfRows):
//   1. Encoder2 over the molecule's ego-nets (the ego batch of
//      graph.egonet_batch: ego-net v <-> atom v, rows ego_ptr[v] .. ego_ptr[v+1])
//      in tiles of WHOLE ego-nets of at most kInfRows rows, taken greedily in
//      atom order (a function of the molecule's ego sizes alone): raw features
//      through the ego -> parent map and transfer_d into LDS, L GIN layers in
//      LDS, then s_v = sum of the ego-net's rows -> bufS[v].
//   2. Encoder1 over the molecule's rows, the same layer routine.
//   3. Interaction in eval mode: y = relu(BN_running(compressor[0] f)),
//      p = compressor[3] y, lam = gate(u_gate, p), per-molecule mean and
//      unbiased std of f, noisy = lam f + (1 - lam) mu + u_feat (1 - lam) sig,
//      a_v = softmax_v(w_hi . s_v) s_v (ATT; else a_v = s_v), z1 = sum noisy,
//      z2 = sum f.
//   4. HEAD: m = MLP([noisy | a]) (128 -> 64 -> 64), Set2Set over the
//      molecule's rows (one-layer LSTM, n_iters rounds, gate order i f g o),
//      pooled[g] = q* [128].
// A GIN layer in LDS: Y = (1 + eps) X + sum of CSR neighbours (local rows),
// X = relu(Y W1^T + b1), Y = relu(a (X W2^T + b2) + c) with the BatchNorm as
// the affine map a = gamma / sqrt(var + eps), c = beta - mean a.  The 64-wide
// products are exact-f32 MFMA (mma_pf of mfma_tile.h, v_mfma_f32_32x32x2_f32),
// 32 x 32 output tiles spread over the four waves; every output element has
// one writer and a fixed k order, every reduction over rows runs in row order
// in one thread, and nothing is atomic: the launch is bitwise reproducible and
// a molecule's outputs depend only on the molecule (its rows, its ego-nets,
// its noise rows) — not on the batch, its position, or the grid.
//
// LDS map (floats; row stride kInfLd = 65, conflict-free column reads):
//   bufA, bufB, bufS  3 x kInfRows x 65   activations (ping / pong) and s_v / a_v
//   sW1, sW2          2 x 64 x 65         the current layer's weights
//   sWt 32 x 16 (transfer_d), sPar 6 x 64 (biases, affine maps, vectors),
//   sRow / sLog kInfRows each, LSTM state (256 + 128 + 64 + 64), the ego
//   pointers and the tile's CSR row pointers (kInfRows + 1 each).
// ~138 KiB: one workgroup per CU (160 KiB).
//
// Capacity mode: the row count comes from dims[0], molecules from graph_ptr;
// a molecule with no rows writes zero rows; rows of lam / logit / im in
// [count, n_rows_cap) are written as zeros.  A molecule above kInfRows rows,
// a graph_ptr range that is no range of the batch's rows, an ego-net above
// kInfRows rows or an index that leaves its molecule / ego tile / capacity
// sets *err (sticky) and gets NaN rows;
// such an index is never dereferenced.
#include "mfma_tile.h"

namespace scgib {

namespace {

constexpr int kInfRows = 128;     // rows of a molecule / of an ego tile held in LDS
constexpr int kInfLd = LDH;       // 65
constexpr int kInfMaxWG = 1024;   // workgroups of a launch (molecules wrap past it)
constexpr int kInfF = 16;         // raw feature columns
constexpr float kInfGateScale = static_cast<float>(0.0001 - (1.0 - 0.0001));
constexpr float kInfGateShift = static_cast<float>(1.0 - 0.0001);

typedef scgib_infer_params InfTab;
static_assert(sizeof(InfTab) <= 4096, "kernel-argument table");

__device__ __forceinline__ float inf_red16(float v) {
    v += __shfl_xor(v, 1, kWave);
    v += __shfl_xor(v, 2, kWave);
    v += __shfl_xor(v, 4, kWave);
    v += __shfl_xor(v, 8, kWave);
    return v;
}

__device__ __forceinline__ float inf_sigmoid(float v) { return 1.f / (1.f + expf(-v)); }

// s[row * 65 + k] = w[row * ldw + c0 + k] for k < kcols, 0 up to 64
__device__ __forceinline__ void inf_stage64(const float *__restrict__ w, int ldw, int c0, int kcols,
                                            float *s) {
    for (int i = threadIdx.x; i < 64 * 64; i += 256) {
        const int row = i >> 6, k = i & 63;
        s[row * kInfLd + k] = k < kcols ? w[row * ldw + c0 + k] : 0.f;
    }
}

// Out[r][c] = act(sc[c] * (sum_k A[r][k] W[c][k] (+ sum_k A2[r][k] W2[c][k]) + bias[c]) + sh[c])
// for the 32-row blocks that hold rows [0, rows); K columns of A, W rows of
// stride ldw; sc NULL: no affine map.  mma_pf: mma_nt's k order, operands
// read one chunk ahead (mfma_tile.h).
template <int K>
__device__ __forceinline__ void inf_mm(const float *A, const float *W, int ldw, const float *A2,
                                       const float *W2, float *Out, int rows, const float *bias,
                                       const float *sc, const float *sh, bool relu) {
    const int w = threadIdx.x >> 6, l = threadIdx.x & 63;
    const int nrb = (rows + 31) >> 5;
    for (int t = w; t < 2 * nrb; t += 4) {
        const int rb = t >> 1, cb = t & 1;
        f32x16 acc = zero16();
        acc = mma_pf<K, false, false>(A + rb * 32 * kInfLd, kInfLd, W + cb * 32 * ldw, ldw, acc);
        if (A2)
            acc = mma_pf<K, false, false>(A2 + rb * 32 * kInfLd, kInfLd, W2 + cb * 32 * ldw, ldw, acc);
        const int c = cb * 32 + (l & 31);
        const float b = bias[c], a = sc ? sc[c] : 1.f, s = sc ? sh[c] : 0.f;
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            float v = acc[reg] + b;
            if (sc) v = fmaf(a, v, s);
            if (relu) v = v < 0.f ? 0.f : v;  // (keeps a NaN, as torch's relu; fmaxf would drop it)
            Out[(rb * 32 + acc_row(reg, l)) * kInfLd + c] = v;
        }
    }
}

// out[i] = <X[i], v> + add for i < rows (16 lanes per row, 16 rows per pass)
__device__ __forceinline__ void inf_rowdot(const float *X, const float *v, float *out, int rows,
                                           float add) {
    const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
    const float v0 = v[4 * c4], v1 = v[4 * c4 + 1], v2 = v[4 * c4 + 2], v3 = v[4 * c4 + 3];
    for (int i0 = 0; i0 < rows; i0 += 16) {
        const int i = i0 + rg, ii = i < rows ? i : 0;
        const float *p = X + ii * kInfLd + 4 * c4;
        float d = p[0] * v0;
        d = fmaf(p[1], v1, d);
        d = fmaf(p[2], v2, d);
        d = fmaf(p[3], v3, d);
        d = inf_red16(d);
        if (i < rows && c4 == 0) out[i] = d + add;
    }
}

// (max, sum of exp(e - max)) over e[0, rows), rows <= 128; every wave computes
// both redundantly, in the same fixed order
__device__ __forceinline__ void inf_softmax_stats(const float *e, int rows, float &M, float &D) {
    const int l = threadIdx.x & 63;
    const float e0 = l < rows ? e[l] : -INFINITY, e1 = l + 64 < rows ? e[l + 64] : -INFINITY;
    // (a NaN logit must reach the result: fmaxf would drop it)
    const bool bad = (l < rows && e0 != e0) || (l + 64 < rows && e1 != e1);
    M = wave_max(fmaxf(e0, e1));
    float d = (l < rows ? expf(e0 - M) : 0.f) + (l + 64 < rows ? expf(e1 - M) : 0.f);
    if (bad) d = NAN;
    D = wave_sum(d);
}

// h0 = transfer_d(x[row]) into X (columns 32..63 zero); map: ego -> parent row
// (NULL: row0 + i).  A mapped row outside [r0, r1) sets *bad.
__device__ __forceinline__ void inf_entry(const float *__restrict__ x, int F, const float *sWt,
                                          const int32_t *__restrict__ map, int64_t row0, int rows,
                                          int64_t r0, int64_t r1, float *X, int *bad) {
    for (int i = threadIdx.x; i < rows * 64; i += 256) {
        const int r = i >> 6, c = i & 63;
        float v = 0.f;
        if (c < 32) {
            int64_t xr = map ? static_cast<int64_t>(map[row0 + r]) : row0 + r;
            if (xr < r0 || xr >= r1) {
                *bad = 1;
                xr = r0;
            }
            const float *xp = x + xr * F;
            for (int f = 0; f < F; ++f) v = fmaf(xp[f], sWt[c * kInfF + f], v);
        }
        X[r * kInfLd + c] = v;
    }
}

// Y[i] = ope X[i] + sum over the CSR row i (sRp: the tile's row pointers, in
// LDS, validated) of X[col - grow0]
__device__ __forceinline__ void inf_agg(const float *X, float *Y, int rows, const int *sRp,
                                        const int32_t *__restrict__ col, int64_t grow0, float ope,
                                        int *bad) {
    const int c4 = threadIdx.x & 15, rg = threadIdx.x >> 4;
    for (int i = rg; i < rows; i += 16) {
        const int e0 = sRp[i], e1 = sRp[i + 1];
        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
        for (int e = e0; e < e1; ++e) {
            const int64_t u = static_cast<int64_t>(col[e]) - grow0;
            if (u < 0 || u >= rows) {
                *bad = 1;
                continue;
            }
            const float *p = X + u * kInfLd + 4 * c4;
            a0 += p[0]; a1 += p[1]; a2 += p[2]; a3 += p[3];
        }
        const float *p = X + i * kInfLd + 4 * c4;
        float *q = Y + i * kInfLd + 4 * c4;
        q[0] = fmaf(ope, p[0], a0);
        q[1] = fmaf(ope, p[1], a1);
        q[2] = fmaf(ope, p[2], a2);
        q[3] = fmaf(ope, p[3], a3);
    }
}

// one GIN layer X -> Y (DIN = 32: layer 0, whose W1 is [64][32]); the weights'
// 16-byte loads are in flight across the aggregation
template <int DIN>
__device__ __forceinline__ void inf_layer(const InfTab &P, int enc, int l, float *X, float *Y,
                                          int rows, const int *sRp,
                                          const int32_t *__restrict__ col, int64_t grow0,
                                          float *sW1, float *sW2, float *sPar, int *bad) {
    const int tid = threadIdx.x;
    WeightRegs<DIN> wr;
    load_weights<DIN>(P.w1[enc][l], P.w2[enc][l], wr);
    float pb1 = 0.f, pb2 = 0.f, pg = 0.f, pbt = 0.f, pm = 0.f, pv = 1.f;
    if (tid < 64) {
        pb1 = P.b1[enc][l][tid];
        pb2 = P.b2[enc][l][tid];
        pg = P.gamma[enc][l][tid];
        pbt = P.beta[enc][l][tid];
        pm = P.rmean[enc][l][tid];
        pv = P.rvar[enc][l][tid];
    }
    inf_agg(X, Y, rows, sRp, col, grow0, P.ope[enc][l], bad);
    store_weights<DIN>(wr, sW1, sW2);
    if (tid < 64) {
        sPar[tid] = pb1;
        sPar[64 + tid] = pb2;
        const float a = pg / sqrtf(pv + P.bn_eps);
        sPar[128 + tid] = a;
        sPar[192 + tid] = pbt - pm * a;
    }
    __syncthreads();
    inf_mm<DIN>(Y, sW1, DIN + 1, nullptr, nullptr, X, rows, sPar, nullptr, nullptr, true);
    __syncthreads();
    inf_mm<64>(X, sW2, kInfLd, nullptr, nullptr, Y, rows, sPar + 64, sPar + 128, sPar + 192, true);
    __syncthreads();
}

// L GIN layers of encoder `enc` over rows [0, rows) held in X (h0); Y: the
// other buffer.  The tile's CSR row pointers go to LDS once (sRp), checked
// against e_cap.  Returns the buffer that holds the output.  Ends on a barrier.
__device__ __forceinline__ float *inf_gin(const InfTab &P, int enc, float *X, float *Y, int rows,
                                          const int32_t *__restrict__ rowptr,
                                          const int32_t *__restrict__ col, int64_t grow0,
                                          int64_t e_cap, float *sW1, float *sW2, float *sPar,
                                          int *sRp, int *bad) {
    for (int i = threadIdx.x; i <= rows; i += 256) sRp[i] = rowptr[grow0 + i];
    __syncthreads();
    for (int i = threadIdx.x; i < rows; i += 256)
        if (sRp[i] < 0 || sRp[i + 1] < sRp[i] || sRp[i + 1] > e_cap) *bad = 2;
    __syncthreads();
    if (*bad == 2) {  // (uniform) no edge is read: the layers run on the rows alone
        __syncthreads();
        for (int i = threadIdx.x; i <= rows; i += 256) sRp[i] = 0;
        __syncthreads();
    }
    for (int l = 0; l < P.n_layers; ++l) {
        if (l == 0) inf_layer<32>(P, enc, l, X, Y, rows, sRp, col, grow0, sW1, sW2, sPar, bad);
        else inf_layer<64>(P, enc, l, X, Y, rows, sRp, col, grow0, sW1, sW2, sPar, bad);
        float *t = X;
        X = Y;
        Y = t;
    }
    return X;
}

template <bool ATT, bool HEAD>
__global__ __launch_bounds__(256) void infer_fwd_k(
    const InfTab P, const float *__restrict__ x, int64_t n_cap, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, int64_t e_cap, const int32_t *__restrict__ gptr, int64_t B,
    const int32_t *__restrict__ dims, const int32_t *__restrict__ ego_ptr,
    const int32_t *__restrict__ ego_rowptr, const int32_t *__restrict__ ego_col,
    const int32_t *__restrict__ ego_id, int64_t en_cap, int64_t ee_cap,
    const float *__restrict__ u_gate, const float *__restrict__ u_feat, float *__restrict__ pooled,
    float *__restrict__ z1, float *__restrict__ z2, float *__restrict__ lam,
    float *__restrict__ logit, float *__restrict__ im, int32_t *__restrict__ err) {
    __shared__ float bufA[kInfRows * kInfLd], bufB[kInfRows * kInfLd], bufS[kInfRows * kInfLd];
    __shared__ float sW1[64 * kInfLd], sW2[64 * kInfLd];
    __shared__ float sWt[32 * kInfF], sPar[6 * 64], sRow[kInfRows], sLog[kInfRows];
    __shared__ float sMu[64], sSig[64], sG[256], sQ[128], sH[64], sC[64];
    __shared__ int sPtr[kInfRows + 1], sRp[kInfRows + 1];
    __shared__ int sBad;
    const int tid = threadIdx.x;
    const int F = P.n_feat;
    int64_t N = dims ? static_cast<int64_t>(dims[0]) : n_cap;
    N = N < 0 ? 0 : (N > n_cap ? n_cap : N);
    for (int i = tid; i < 32 * kInfF; i += 256) {
        const int c = i / kInfF, f = i % kInfF;
        sWt[i] = f < F ? P.transfer[c * F + f] : 0.f;
    }
    for (int64_t g = blockIdx.x; g < B; g += gridDim.x) {
        __syncthreads();  // the previous molecule's last readers of sBad, sQ, the buffers
        if (tid == 0) sBad = 0;
        __syncthreads();
        const int64_t r0 = gptr[g], r1 = gptr[g + 1];
        if (r1 == r0) {  // no rows: zero outputs (uniform)
            if (tid < 64) {
                z1[g * 64 + tid] = 0.f;
                z2[g * 64 + tid] = 0.f;
            }
            if (HEAD && tid < 128) pooled[g * 128 + tid] = 0.f;
            continue;
        }
        // a range that is no range of the batch's rows is an index error like the
        // others: NaN rows (those of it that exist) and the error word
        const bool over = r0 < 0 || r1 < r0 || r1 > N || r1 - r0 > kInfRows;
        const int64_t lo = r0 < 0 ? 0 : (r0 > N ? N : r0), hi = r1 < lo ? lo : (r1 > N ? N : r1);
        const int n = over ? 0 : static_cast<int>(r1 - r0);
        if (!over) {
            for (int i = tid; i <= n; i += 256) sPtr[i] = ego_ptr[r0 + i];
            __syncthreads();
            for (int i = tid; i < n; i += 256) {
                const int a = sPtr[i], b = sPtr[i + 1];
                if (a < 0 || b < a || b > en_cap || b - a > kInfRows) sBad = 1;
            }
            __syncthreads();
        }
        const bool run = !over && !sBad;
        __syncthreads();  // every thread has read sBad before the walk may set it
        if (run) {
            // ---- 1. Encoder2 over tiles of whole ego-nets -> bufS[v] = s_v ----
            int e0 = 0;
            while (e0 < n) {
                const int base = sPtr[e0];
                int e1 = e0;
                while (e1 < n && sPtr[e1 + 1] - base <= kInfRows) ++e1;
                const int rows = sPtr[e1] - base;
                inf_entry(x, F, sWt, ego_id, base, rows, r0, r1, bufA, &sBad);
                __syncthreads();
                const float *H = inf_gin(P, 1, bufA, bufB, rows, ego_rowptr, ego_col, base, ee_cap,
                                         sW1, sW2, sPar, sRp, &sBad);
                for (int e = e0 + (tid >> 6); e < e1; e += 4) {
                    const int c = tid & 63, ra = sPtr[e] - base, rb = sPtr[e + 1] - base;
                    float s = 0.f;
                    for (int r = ra; r < rb; ++r) s += H[r * kInfLd + c];
                    bufS[e * kInfLd + c] = s;
                }
                __syncthreads();
                e0 = e1;
            }
            // ---- 2. Encoder1 over the molecule ----
            inf_entry(x, F, sWt, nullptr, r0, n, r0, r1, bufA, &sBad);
            __syncthreads();
            float *Fb = inf_gin(P, 0, bufA, bufB, n, rowptr, col, r0, e_cap, sW1, sW2, sPar, sRp,
                                &sBad);
            float *Tb = Fb == bufA ? bufB : bufA;
            // ---- 3. interaction, eval mode ----
            stage_matrix<64>(P.c0_w, sW1);
            if (tid < 64) {
                sPar[tid] = P.c0_b[tid];
                const float a = P.cbn_gamma[tid] / sqrtf(P.cbn_rvar[tid] + P.bn_eps);
                sPar[128 + tid] = a;
                sPar[192 + tid] = P.cbn_beta[tid] - P.cbn_rmean[tid] * a;
                sPar[256 + tid] = P.c3_w[tid];
                sPar[320 + tid] = ATT ? P.att_w[64 + tid] : 0.f;
                sPar[64 + tid] = ATT ? P.att_w[tid] : 0.f;
            }
            __syncthreads();
            // y = relu(BN(compressor[0] f)) -> Tb
            inf_mm<64>(Fb, sW1, kInfLd, nullptr, nullptr, Tb, n, sPar, sPar + 128, sPar + 192, true);
            __syncthreads();
            inf_rowdot(Tb, sPar + 256, sRow, n, P.c3_b[0]);  // p
            if (ATT) inf_rowdot(bufS, sPar + 320, sLog, n, 0.f);
            if (tid < 64) {  // per-channel sum, mean and unbiased std of f, rows in order
                float s = 0.f;
                for (int r = 0; r < n; ++r) s += Fb[r * kInfLd + tid];
                z2[g * 64 + tid] = s;
                const float mu = s / static_cast<float>(n);
                float q = 0.f;
                for (int r = 0; r < n; ++r) {
                    const float d = Fb[r * kInfLd + tid] - mu;
                    q = fmaf(d, d, q);
                }
                sMu[tid] = mu;
                sSig[tid] = sqrtf(q / static_cast<float>(n - 1));  // n == 1: 0 / 0 = NaN, as torch
            }
            __syncthreads();
            if (tid < n) {  // p -> lam
                const float e = kInfGateScale * u_gate[r0 + tid] + kInfGateShift;
                const float gt = logf(e) - logf(1.f - e);
                const float lm = 1.f / (1.f + expf(-(gt + sRow[tid])));
                sRow[tid] = lm;
                if (lam) lam[r0 + tid] = lm;
                if (ATT && logit) logit[r0 + tid] = sLog[tid];
            }
            __syncthreads();
            for (int i = tid; i < n * 64; i += 256) {  // noisy -> Tb
                const int r = i >> 6, c = i & 63;
                const float lm = sRow[r], ln = 1.f - lm;
                const float v = fmaf(lm, Fb[r * kInfLd + c], ln * sMu[c]);
                Tb[r * kInfLd + c] = fmaf(u_feat[(r0 + r) * 64 + c], ln * sSig[c], v);
            }
            __syncthreads();
            if (tid < 64) {
                float s = 0.f;
                for (int r = 0; r < n; ++r) s += Tb[r * kInfLd + tid];
                z1[g * 64 + tid] = s;
                sMu[tid] = s;  // (mu is used up) z-bar for the logit's constant
            }
            if (ATT) {
                __syncthreads();
                // the reference's logit is w_lo . z-bar + b + w_hi . s_v: the
                // constant cancels in the softmax unless it is not finite (a
                // one-atom molecule: std = NaN), and then every weight is NaN
                float zc = 0.f;
                for (int c = 0; c < 64; ++c) zc = fmaf(sPar[64 + c], sMu[c], zc);
                const float zz = zc - zc;  // 0, or NaN
                float M, D;
                inf_softmax_stats(sLog, n, M, D);
                const float inv = 1.f / D;
                for (int i = tid; i < n * 64; i += 256) {
                    const int r = i >> 6, c = i & 63;
                    bufS[r * kInfLd + c] *= expf((sLog[r] - M) + zz) * inv;
                }
            }
            __syncthreads();
            if (im) {
                for (int i = tid; i < n * 128; i += 256) {
                    const int r = i >> 7, c = i & 127;
                    im[(r0 + r) * 128 + c] = c < 64 ? Tb[r * kInfLd + c] : bufS[r * kInfLd + c - 64];
                }
            }
            if constexpr (HEAD) {
                // ---- 4. MLP (128 -> 64 -> 64), Set2Set ----
                inf_stage64(P.mlp0_w, 128, 0, 64, sW1);
                inf_stage64(P.mlp0_w, 128, 64, 64, sW2);
                if (tid < 64) {
                    sPar[tid] = P.mlp0_b[tid];
                    sPar[64 + tid] = P.mlp2_b[tid];
                    sH[tid] = 0.f;
                    sC[tid] = 0.f;
                }
                if (tid < 128) sQ[tid] = 0.f;
                __syncthreads();
                inf_mm<64>(Tb, sW1, kInfLd, bufS, sW2, Fb, n, sPar, nullptr, nullptr, true);
                __syncthreads();
                stage_matrix<64>(P.mlp2_w, sW1);
                __syncthreads();
                inf_mm<64>(Fb, sW1, kInfLd, nullptr, nullptr, Tb, n, sPar + 64, nullptr, nullptr,
                           false);
                __syncthreads();
                for (int it = 0; it < P.n_iters; ++it) {
                    {  // gate tid = W_ih q* + b_ih + W_hh h + b_hh
                        const float4 *wi = reinterpret_cast<const float4 *>(P.w_ih + tid * 128);
                        const float4 *wh = reinterpret_cast<const float4 *>(P.w_hh + tid * 64);
                        float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f;
#pragma unroll 8
                        for (int k = 0; k < 32; ++k) {
                            const float4 w4 = wi[k];
                            a0 = fmaf(w4.x, sQ[4 * k], a0);
                            a1 = fmaf(w4.y, sQ[4 * k + 1], a1);
                            a2 = fmaf(w4.z, sQ[4 * k + 2], a2);
                            a3 = fmaf(w4.w, sQ[4 * k + 3], a3);
                        }
                        float h0 = 0.f, h1 = 0.f, h2 = 0.f, h3 = 0.f;
#pragma unroll 8
                        for (int k = 0; k < 16; ++k) {
                            const float4 w4 = wh[k];
                            h0 = fmaf(w4.x, sH[4 * k], h0);
                            h1 = fmaf(w4.y, sH[4 * k + 1], h1);
                            h2 = fmaf(w4.z, sH[4 * k + 2], h2);
                            h3 = fmaf(w4.w, sH[4 * k + 3], h3);
                        }
                        sG[tid] = (((a0 + a1) + (a2 + a3)) + P.b_ih[tid]) +
                                  (((h0 + h1) + (h2 + h3)) + P.b_hh[tid]);
                    }
                    __syncthreads();
                    if (tid < 64) {
                        const float gi = inf_sigmoid(sG[tid]), gf = inf_sigmoid(sG[64 + tid]);
                        const float gg = tanhf(sG[128 + tid]), go = inf_sigmoid(sG[192 + tid]);
                        const float c = gf * sC[tid] + gi * gg;
                        const float h = go * tanhf(c);
                        sC[tid] = c;
                        sH[tid] = h;
                        sQ[tid] = h;
                    }
                    __syncthreads();
                    inf_rowdot(Tb, sH, sLog, n, 0.f);  // e_v = <x_v, h>
                    __syncthreads();
                    float M, D;
                    inf_softmax_stats(sLog, n, M, D);
                    if (tid < n) sRow[tid] = expf(sLog[tid] - M);
                    __syncthreads();
                    if (tid < 64) {
                        float s = 0.f;
                        for (int r = 0; r < n; ++r) s = fmaf(sRow[r], Tb[r * kInfLd + tid], s);
                        sQ[64 + tid] = s / D;
                    }
                    __syncthreads();
                }
                if (tid < 128) pooled[g * 128 + tid] = sQ[tid];
            }
        }
        __syncthreads();
        if (over || sBad) {  // NaN rows, sticky error word; nothing out of bounds was read
            if (tid == 0) *err = 1;
            if (tid < 64) {
                z1[g * 64 + tid] = NAN;
                z2[g * 64 + tid] = NAN;
            }
            if (HEAD && tid < 128) pooled[g * 128 + tid] = NAN;
            for (int64_t r = lo + tid; r < hi; r += 256) {
                if (lam) lam[r] = NAN;
                if (logit) logit[r] = NAN;
            }
            if (im)
                for (int64_t i = lo * 128 + tid; i < hi * 128; i += 256) im[i] = NAN;
        }
    }
    // rows past the actual count: zeros
    if (lam || logit || im) {
        for (int64_t r = N + blockIdx.x; r < n_cap; r += gridDim.x) {
            if (tid == 0) {
                if (lam) lam[r] = 0.f;
                if (logit) logit[r] = 0.f;
            }
            if (im && tid < 128) im[r * 128 + tid] = 0.f;
        }
    }
}

// out[ids[g]][:] = src[g][:] for ids[g] in [0, n_out); one writer per element
// (a pass holds each id once), ids outside write nothing
__global__ __launch_bounds__(256) void infer_store_k(const float *__restrict__ src, int64_t B,
                                                     int width, const int32_t *__restrict__ ids,
                                                     int64_t n_out, float *__restrict__ out) {
    for (int64_t g = blockIdx.x; g < B; g += gridDim.x) {
        const int64_t id = ids[g];
        if (id < 0 || id >= n_out) continue;
        for (int c = threadIdx.x; c < width; c += 256) out[id * width + c] = src[g * width + c];
    }
}

}  // namespace

}  // namespace scgib

using namespace scgib;

extern "C" {

int64_t scgib_infer_max_nodes(void) { return kInfRows; }
int64_t scgib_infer_max_ego_rows(void) { return kInfRows; }
int64_t scgib_infer_ego_tile_rows(void) { return kInfRows; }
int64_t scgib_infer_max_workgroups(void) { return kInfMaxWG; }

int scgib_infer_store(const float *src, int64_t n_graphs, int32_t width, const int32_t *ids,
                      int64_t n_out, float *out, scgib_stream_t stream) {
    if (n_graphs < 0 || width < 1 || n_out < 0) return SCGIB_EINVAL;
    if (n_graphs == 0 || n_out == 0) return SCGIB_OK;
    if (!src || !ids || !out) return SCGIB_EINVAL;
    const unsigned grid = static_cast<unsigned>(n_graphs < 1024 ? n_graphs : 1024);
    infer_store_k<<<dim3(grid), 256, 0, as_stream(stream)>>>(src, n_graphs, width, ids, n_out, out);
    return launch_status();
}

int scgib_infer_fwd(const scgib_infer_params *p, const float *x, int64_t n_rows,
                    const int32_t *rowptr, const int32_t *col, int64_t e_cap,
                    const int32_t *graph_ptr, int64_t n_graphs, const int32_t *dims,
                    int64_t max_graph_nodes, const int32_t *ego_ptr, const int32_t *ego_rowptr,
                    const int32_t *ego_col, const int32_t *ego_id, int64_t ego_rows,
                    int64_t ego_e_cap, const float *u_gate, const float *u_feat, float *pooled,
                    float *z1, float *z2, float *lam, float *logit, float *im, int32_t *err,
                    scgib_stream_t stream) {
    if (!p || n_rows < 0 || n_graphs < 0 || e_cap < 0 || ego_rows < 0 || ego_e_cap < 0 || !err)
        return SCGIB_EINVAL;
    if (p->n_layers < 1 || p->n_layers > SCGIB_INFER_MAX_LAYERS || p->n_feat < 1 ||
        p->n_feat > kInfF || max_graph_nodes > kInfRows || (p->has_head && p->n_iters < 0))
        return SCGIB_EUNSUPPORTED;
    if (n_graphs == 0) return SCGIB_OK;
    if (!x || !rowptr || !col || !graph_ptr || !ego_ptr || !ego_rowptr || !ego_col || !ego_id ||
        !u_gate || !u_feat || !z1 || !z2 || (p->has_head && !pooled) || !p->transfer || !p->c0_w ||
        !p->c0_b || !p->cbn_gamma || !p->cbn_beta || !p->cbn_rmean || !p->cbn_rvar || !p->c3_w ||
        !p->c3_b || (p->use_att && !p->att_w))
        return SCGIB_EINVAL;
    // (weight matrices are staged with 16-byte loads)
    uintptr_t align = reinterpret_cast<uintptr_t>(p->c0_w);
    for (int e = 0; e < 2; ++e)
        for (int l = 0; l < p->n_layers; ++l) {
            if (!p->w1[e][l] || !p->b1[e][l] || !p->w2[e][l] || !p->b2[e][l] || !p->gamma[e][l] ||
                !p->beta[e][l] || !p->rmean[e][l] || !p->rvar[e][l])
                return SCGIB_EINVAL;
            align |= reinterpret_cast<uintptr_t>(p->w1[e][l]) | reinterpret_cast<uintptr_t>(p->w2[e][l]);
        }
    if (p->has_head) align |= reinterpret_cast<uintptr_t>(p->mlp2_w);
    if (align & 15) return SCGIB_EINVAL;
    if (p->has_head) {
        if (!p->mlp0_w || !p->mlp0_b || !p->mlp2_w || !p->mlp2_b || !p->w_ih || !p->w_hh ||
            !p->b_ih || !p->b_hh)
            return SCGIB_EINVAL;
        // the LSTM rows are read as 16-byte vectors
        if ((reinterpret_cast<uintptr_t>(p->w_ih) | reinterpret_cast<uintptr_t>(p->w_hh)) & 15)
            return SCGIB_EINVAL;
    }
    const unsigned grid = static_cast<unsigned>(n_graphs < kInfMaxWG ? n_graphs : kInfMaxWG);
    const hipStream_t st = as_stream(stream);
#define SCGIB_INFER_LAUNCH(ATT, HEAD)                                                             \
    infer_fwd_k<ATT, HEAD><<<dim3(grid), 256, 0, st>>>(                                           \
        *p, x, n_rows, rowptr, col, e_cap, graph_ptr, n_graphs, dims, ego_ptr, ego_rowptr,        \
        ego_col, ego_id, ego_rows, ego_e_cap, u_gate, u_feat, pooled, z1, z2, lam, logit, im, err)
    if (p->use_att) {
        if (p->has_head) SCGIB_INFER_LAUNCH(true, true);
        else SCGIB_INFER_LAUNCH(true, false);
    } else {
        if (p->has_head) SCGIB_INFER_LAUNCH(false, true);
        else SCGIB_INFER_LAUNCH(false, false);
    }
#undef SCGIB_INFER_LAUNCH
    return launch_status();
}

}  // extern "C"
