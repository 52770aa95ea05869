// Graph Transformer layer (gfx950), exact-f32 MFMA tiles and a per-destination
// attention walk: the reference's GraphTransformerLayer (models.py:832-918,
// :986-1005; DGL's apply_edges / send_and_recv restated) at width 64.
//
//   Q, K, V = h Wq^T + bq, ...                     [N, heads, d_h], d_h = 64 / heads
//   e(u->v, a) = K[u,a,:] . Q[v,a,:] / sqrt(d_h);  s = exp(clamp(e, -5, 5))
//   attn[v,a,:] = sum_{u->v} s V[u,a,:] / (sum_{u->v} s + 1e-6)
//   h1  = LN1(h + attn Wo^T + bo)
//   r'  = dropout(relu(h1 W1^T + b1));  out = LN2(h1 + r' W2^T + b2)
//
// Forward, five launches.  gt_lin_fwd_k is one tile kernel (64 rows per
// workgroup, the operand tile in padded LDS, the weight staged in 64 x 64
// chunks, a wave owns a 32 x 32 sub-tile per 64 output columns) with three
// epilogues: bias only (Q, K and V from one read of the h tile), ReLU +
// dropout (r' and the 128-bit keep-and-positive row masks), residual +
// LayerNorm (the O projection with LN1; FFN_layer2 with LN2).
// gt_attn_fwd_k walks the in-edges of a destination in CSR order with 16
// lanes x float4 per node row; a head's lanes are adjacent, the per-head dot
// product is an xor-shuffle over them.  Scores are not stored.
//
// Backward, six launches and one slab reduce.  gt_lin_bwd_k: workgroups
// loop over tiles; per weight dW = dY^T X and db = sum dY accumulate in MFMA
// registers / lane sums into one slab per workgroup (the weight's own
// [out][in] layout; the caller sums them with scgib_slab_reduce_multi), and
// dX = sum_s dY_s W_s [+ add] [masked] is written per tile.  With LN the
// incoming gradient first goes through the LayerNorm backward (from the saved
// pre-norm rows and row statistics), which also yields dgamma / dbeta and
// the residual's gradient dp.  The attention backward is two walks without
// atomics: over destinations (g, dz, dQ; scores recomputed from Q and K by
// the forward's own expression) and over sources on the transposed CSR (dK,
// dV).
//
// Dropout: the keep bits of row r are the 128 bits of one Philox4x32-10 block
// of counter (r, tag, offset) keyed by the seed of a device state of its own;
// the launch's last workgroup advances the offset.
//
// Capacity mode (dims): rows >= dims[0] of every output are zeros and enter
// every product as zeros.  No float atomics; every sum has a fixed order.
#include "mfma_tile.h"

namespace scgib {

constexpr int kGtW = 64;         // layer width
constexpr int kGtF = 128;        // FFN width
constexpr float kGtLnEps = 1e-5f;
constexpr float kGtZEps = 1e-6f;
constexpr uint32_t kGtDropTag = 0x47544c31u;  // counter word 1 of the dropout draws

enum { kEpiBias = 0, kEpiReluDrop = 1, kEpiResLn = 2 };

// a [64][C] block (columns c0 .. c0 + C of a row-major matrix of row length
// ld) in registers; rows >= nv read as zeros (loads unconditional, clamped)
template <int C>
struct GtRegs {
    float4 v[64 * C / 4 / 256];
};

template <int C>
__device__ __forceinline__ void gt_load(const float *__restrict__ src, int64_t row0, int ld, int c0,
                                        int nv, GtRegs<C> &r) {
    constexpr int N = 64 * C / 4 / 256, Q = C / 4;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int idx = tid + 256 * k, rr = idx / Q, cq = idx % Q;
        r.v[k] = ld_ok(reinterpret_cast<const float4 *>(src), ((row0 + rr) * ld + c0) / 4 + cq,
                       (row0 * ld + c0) / 4 + cq, rr < nv, make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

template <int C>
__device__ __forceinline__ void gt_store(const GtRegs<C> &r, float *s, int lds) {
    constexpr int N = 64 * C / 4 / 256, Q = C / 4;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int idx = tid + 256 * k, rr = idx / Q, cq = idx % Q;
        float *d = s + rr * lds + 4 * cq;
        d[0] = r.v[k].x; d[1] = r.v[k].y; d[2] = r.v[k].z; d[3] = r.v[k].w;
    }
}

// sum over the 4 lanes that share a row (lanes 4 row + part), fixed order
__device__ __forceinline__ float quad_sum(float v) {
    v += __shfl_xor(v, 1, kWave);
    v += __shfl_xor(v, 2, kWave);
    return v;
}

__device__ __forceinline__ uint4 gt_philox4x32_10(uint4 c, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int i = 0; i < 10; ++i) {
        const uint32_t lo0 = 0xD2511F53u * c.x, hi0 = __umulhi(0xD2511F53u, c.x);
        const uint32_t lo1 = 0xCD9E8D57u * c.z, hi1 = __umulhi(0xCD9E8D57u, c.z);
        c = make_uint4(hi1 ^ c.y ^ k0, lo1, hi0 ^ c.w ^ k1, lo0);
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    return c;
}

// ---------------------------------------------------------------------------
// forward tile kernel: y_s = epi(x W_s^T + b_s), W_s [DO][DI] (nn.Linear)
// ---------------------------------------------------------------------------
struct GtFwdArgs {
    const float *x;
    const float *w[3], *b[3];
    float *y[3];
    // kEpiResLn: y[0] = LN(res + x W^T + b) * gamma + beta; pre-norm rows and
    // (mean, rstd) per row are saved
    const float *res, *gamma, *beta;
    float *pre, *stats;
    // kEpiReluDrop
    uint64_t *rng;
    unsigned *cnt;
    const uint8_t *drop_mask;
    uint32_t *bits, *pos_bits, *keep_bits;
    int training;
};

template <int DI, int DO, int NS, int EPI>
__global__ __launch_bounds__(256) void gt_lin_fwd_k(const GtFwdArgs a, int64_t ncap,
                                                    const int32_t *__restrict__ dims) {
    constexpr int LDX = DI + 1, NKC = DI / 64, NQ = DO / 64;
    static_assert(EPI != kEpiResLn || (DO == 64 && NS == 1), "gt_lin_fwd_k: LN epilogue");
    static_assert(EPI != kEpiReluDrop || (DI == 64 && DO == 128 && NS == 1), "gt_lin_fwd_k: FFN");
    __shared__ float sX[TM * LDX];
    __shared__ float sW[TM * LDH];
    __shared__ uint32_t sBits[EPI == kEpiReluDrop ? 3 : 1][TM][4];  // keep | pos | keep & pos
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * TM;
    const int nv = static_cast<int>(n - row0 < TM ? (n - row0 > 0 ? n - row0 : 0) : TM);
    const bool draw = EPI == kEpiReluDrop && a.training && !a.drop_mask;
    uint64_t seed = 0, off = 0;
    if (draw) {
        seed = a.rng[0];
        off = __hip_atomic_load(a.rng + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
    if (dims) {
        const int ncr = static_cast<int>(ncap - row0 < TM ? ncap - row0 : TM);
#pragma unroll
        for (int s = 0; s < NS; ++s)
            for (int idx = nv * DO + tid; idx < ncr * DO; idx += 256) a.y[s][row0 * DO + idx] = 0.f;
        if (EPI == kEpiResLn) {
            for (int idx = nv * DO + tid; idx < ncr * DO; idx += 256) a.pre[row0 * DO + idx] = 0.f;
            for (int idx = nv * 2 + tid; idx < ncr * 2; idx += 256) a.stats[row0 * 2 + idx] = 0.f;
        }
        if (EPI == kEpiReluDrop) {
            for (int idx = nv * 4 + tid; idx < ncr * 4; idx += 256) {
                a.bits[row0 * 4 + idx] = 0u;
                if (a.pos_bits) a.pos_bits[row0 * 4 + idx] = 0u;
                if (a.keep_bits) a.keep_bits[row0 * 4 + idx] = 0u;
            }
        }
    }
    if (nv > 0) {  // block-uniform
        {
            GtRegs<DI> xr;
            gt_load<DI>(a.x, row0, DI, 0, nv, xr);
            gt_store<DI>(xr, sX, LDX);
        }
        if (EPI == kEpiReluDrop) {
            const int row = tid >> 2, w = tid & 3;
            uint32_t word = 0xffffffffu;  // eval: everything is kept
            if (a.training && a.drop_mask) {
                word = 0u;
                if (row < nv) {
                    const uint32_t *m = reinterpret_cast<const uint32_t *>(
                        a.drop_mask + (row0 + row) * kGtF + 32 * w);
#pragma unroll
                    for (int i = 0; i < 8; ++i) {
                        const uint32_t b4 = m[i];
#pragma unroll
                        for (int j = 0; j < 4; ++j)
                            word |= ((b4 >> (8 * j)) & 0xffu) ? 1u << (4 * i + j) : 0u;
                    }
                }
            }
            if (!draw) sBits[0][row][w] = word;
            if (draw && tid < TM) {
                const uint64_t r = static_cast<uint64_t>(row0 + tid);
                const uint4 k4 = gt_philox4x32_10(
                    make_uint4(static_cast<uint32_t>(r), kGtDropTag ^ static_cast<uint32_t>(r >> 32),
                               static_cast<uint32_t>(off), static_cast<uint32_t>(off >> 32)),
                    static_cast<uint32_t>(seed), static_cast<uint32_t>(seed >> 32));
                sBits[0][tid][0] = k4.x;
                sBits[0][tid][1] = k4.y;
                sBits[0][tid][2] = k4.z;
                sBits[0][tid][3] = k4.w;
            }
        }
        f32x16 acc = zero16();
#pragma unroll
        for (int s = 0; s < NS; ++s)
#pragma unroll
            for (int nq = 0; nq < NQ; ++nq) {
                acc = zero16();
#pragma unroll
                for (int kc = 0; kc < NKC; ++kc) {
                    GtRegs<64> wreg;
                    gt_load<64>(a.w[s], nq * 64, DI, kc * 64, 64, wreg);
                    __syncthreads();  // the previous chunk's reads are done (first: sX, sBits)
                    gt_store<64>(wreg, sW, LDH);
                    __syncthreads();
                    acc = mma_pf<64, false, false>(sX + wr * 32 * LDX + kc * 64, LDX,
                                                   sW + wc * 32 * LDH, LDH, acc);
                }
                const int col = nq * 64 + wc * 32 + (l & 31);
                const float b = a.b[s][col];
                if (EPI == kEpiBias) {
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int row = wr * 32 + acc_row(reg, l);
                        if (row < nv) a.y[s][(row0 + row) * DO + col] = acc[reg] + b;
                    }
                }
                if (EPI == kEpiReluDrop) {
                    const int w = col >> 5;
                    const float sc = a.training ? 2.f : 1.f;
#pragma unroll
                    for (int reg = 0; reg < 16; ++reg) {
                        const int row = wr * 32 + acc_row(reg, l);
                        const float v = acc[reg] + b;
                        const bool pos = v > 0.f;
                        const bool on = pos && ((sBits[0][row][w] >> (l & 31)) & 1u);
                        if (row < nv) st_saved(a.y[s] + (row0 + row) * DO + col, on ? sc * v : 0.f);
                        const unsigned long long bon = __ballot(on), bpos = __ballot(pos);
                        if ((l & 31) == 0) {  // lanes 0-31 hold one row, 32-63 the row 4 below
                            sBits[2][row][w] = static_cast<uint32_t>(bon >> (l & 32));
                            sBits[1][row][w] = static_cast<uint32_t>(bpos >> (l & 32));
                        }
                    }
                }
            }
        if (EPI == kEpiReluDrop) {
            __syncthreads();
            const int row = tid >> 2, w = tid & 3;
            if (row < nv) {
                a.bits[(row0 + row) * 4 + w] = sBits[2][row][w];
                if (a.pos_bits) a.pos_bits[(row0 + row) * 4 + w] = sBits[1][row][w];
                if (a.keep_bits) a.keep_bits[(row0 + row) * 4 + w] = sBits[0][row][w];
            }
        }
        if (EPI == kEpiResLn) {
            __syncthreads();  // every wave's product has read sW
            {
                const int col = wc * 32 + (l & 31);
                const float b = a.b[0][col];
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int row = wr * 32 + acc_row(reg, l);
                    const float r = a.res[(row0 + (row < nv ? row : nv - 1)) * DO + col];
                    sW[row * LDH + col] = acc[reg] + b + r;
                }
            }
            __syncthreads();
            const int row = tid >> 2, part = tid & 3;
            float x[16];
            float s1 = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) {
                x[j] = sW[row * LDH + part * 16 + j];
                s1 += x[j];
            }
            const float mean = quad_sum(s1) * (1.f / 64.f);
            float s2 = 0.f;
#pragma unroll
            for (int j = 0; j < 16; ++j) s2 = fmaf(x[j] - mean, x[j] - mean, s2);
            const float rstd = 1.f / sqrtf(quad_sum(s2) * (1.f / 64.f) + kGtLnEps);
            if (row < nv) {
                float *po = a.y[0] + (row0 + row) * DO + part * 16;
                float *pp = a.pre + (row0 + row) * DO + part * 16;
#pragma unroll
                for (int j = 0; j < 16; j += 4) {
                    const float4 g = ld4(a.gamma + part * 16 + j), be = ld4(a.beta + part * 16 + j);
                    st4(po + j, make_float4((x[j] - mean) * rstd * g.x + be.x,
                                            (x[j + 1] - mean) * rstd * g.y + be.y,
                                            (x[j + 2] - mean) * rstd * g.z + be.z,
                                            (x[j + 3] - mean) * rstd * g.w + be.w));
                    st4_saved(pp + j, make_float4(x[j], x[j + 1], x[j + 2], x[j + 3]));
                }
                if (part == 0) {
                    a.stats[(row0 + row) * 2] = mean;
                    a.stats[(row0 + row) * 2 + 1] = rstd;
                }
            }
        }
    }
    if (EPI == kEpiReluDrop) {
        // every workgroup has read the offset: the last one advances it
        if (draw && block_arrive(a.cnt, gridDim.x) && tid == 0) {
            __hip_atomic_store(a.rng + 1, off + 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            *a.cnt = 0u;
        }
    }
}

// ---------------------------------------------------------------------------
// backward tile kernel: per weight s, dW_s = dY_s^T X and db_s = sum dY_s into
// the workgroup's slab, dX = sum_s dY_s W_s [+ add] [masked by bits]
// slab: NS x dW [DY][DX] | NS x db [DY] | dgamma [64] | dbeta [64] (LN)
// ---------------------------------------------------------------------------
struct GtBwdArgs {
    const float *dy[3], *w[3];
    const float *x;
    const float *add;
    const uint32_t *bits;
    float mscale;
    float *dx;
    // LN: dy[0] is the gradient of the LayerNorm's output
    const float *pre, *stats, *gamma;
    float *dp;
    float *slab;
};

template <int DY, int DX, int NS, bool LN>
constexpr int gt_bwd_width() { return NS * DY * DX + NS * DY + (LN ? 2 * kGtW : 0); }

template <int DY, int DX, int NS, bool LN, bool MASK>
__global__ __launch_bounds__(256) void gt_lin_bwd_k(const GtBwdArgs a, int64_t ncap,
                                                    int64_t ntiles,
                                                    const int32_t *__restrict__ dims) {
    constexpr int LDD = DY + 1, NXC = DX / 64, NKC = DY / 64, IPW = DY / 64;
    constexpr int NG = 256 / DY, RPG = 64 / NG;
    static_assert(!LN || (DY == 64 && NS == 1), "gt_lin_bwd_k: LN prologue");
    static_assert(!MASK || DX == 128, "gt_lin_bwd_k: mask");
    __shared__ float sD[TM * LDD];
    __shared__ float sB[TM * LDH];  // X chunk, then weight chunk (LN: xhat first)
    __shared__ uint32_t sM[MASK ? TM : 1][4];
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const int ch = tid % DY, q = tid / DY;
    f32x16 accW[NS * NXC * IPW];
#pragma unroll
    for (int i = 0; i < NS * NXC * IPW; ++i) accW[i] = zero16();
    float db[NS];
#pragma unroll
    for (int s = 0; s < NS; ++s) db[s] = 0.f;
    float dg = 0.f, dbt = 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TM;
        const int nv = static_cast<int>(n - row0 < TM ? (n - row0 > 0 ? n - row0 : 0) : TM);
        if (dims) {
            const int ncr = static_cast<int>(ncap - row0 < TM ? ncap - row0 : TM);
            for (int idx = nv * DX + tid; idx < ncr * DX; idx += 256) a.dx[row0 * DX + idx] = 0.f;
            if (LN)
                for (int idx = nv * DY + tid; idx < ncr * DY; idx += 256) a.dp[row0 * DY + idx] = 0.f;
        }
        if (nv == 0) continue;  // block-uniform
        __syncthreads();        // the previous tile's LDS reads are done
        if (MASK) {
            const int row = tid >> 2, w = tid & 3;
            sM[row][w] = row < nv ? a.bits[(row0 + row) * 4 + w] : 0u;
        }
        f32x16 accX[NXC];
#pragma unroll
        for (int j = 0; j < NXC; ++j) accX[j] = zero16();
#pragma unroll
        for (int s = 0; s < NS; ++s) {
            if (s > 0) __syncthreads();  // the previous weight's reads of sD / sB are done
            if (!LN) {
                GtRegs<DY> d;
                gt_load<DY>(a.dy[s], row0, DY, 0, nv, d);
                gt_store<DY>(d, sD, LDD);
            } else {
                {
                    GtRegs<64> d, p;
                    gt_load<64>(a.dy[0], row0, 64, 0, nv, d);
                    gt_load<64>(a.pre, row0, 64, 0, nv, p);
#pragma unroll
                    for (int k = 0; k < 4; ++k) {
                        const int rr = (tid + 256 * k) / 16;
                        const int64_t sr = row0 + (rr < nv ? rr : nv - 1);
                        const float mean = a.stats[sr * 2], rstd = a.stats[sr * 2 + 1];
                        const bool ok = rr < nv;
                        p.v[k] = make_float4(ok ? (p.v[k].x - mean) * rstd : 0.f,
                                             ok ? (p.v[k].y - mean) * rstd : 0.f,
                                             ok ? (p.v[k].z - mean) * rstd : 0.f,
                                             ok ? (p.v[k].w - mean) * rstd : 0.f);
                    }
                    gt_store<64>(d, sD, LDD);
                    gt_store<64>(p, sB, LDH);
                }
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 16; ++r) {  // dgamma, dbeta: column sums over the tile
                    const int row = (tid >> 6) * 16 + r, c = tid & 63;
                    const float dyv = sD[row * LDD + c];
                    dg = fmaf(dyv, sB[row * LDH + c], dg);
                    dbt += dyv;
                }
                __syncthreads();
                const int row = tid >> 2, part = tid & 3;
                const float rstd = a.stats[(row0 + (row < nv ? row : nv - 1)) * 2 + 1];
                float t[16], xh[16];
                float a1 = 0.f, a2 = 0.f;
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    const int c = part * 16 + j;
                    t[j] = sD[row * LDD + c] * a.gamma[c];
                    xh[j] = sB[row * LDH + c];
                    a1 += t[j];
                    a2 = fmaf(t[j], xh[j], a2);
                }
                const float m1 = quad_sum(a1) * (1.f / 64.f), m2 = quad_sum(a2) * (1.f / 64.f);
#pragma unroll
                for (int j = 0; j < 16; ++j) {
                    t[j] = rstd * (t[j] - m1 - xh[j] * m2);
                    sD[row * LDD + part * 16 + j] = t[j];
                }
                if (row < nv) {
                    float *pd = a.dp + (row0 + row) * 64 + part * 16;
#pragma unroll
                    for (int j = 0; j < 16; j += 4)
                        st4(pd + j, make_float4(t[j], t[j + 1], t[j + 2], t[j + 3]));
                }
            }
#pragma unroll
            for (int xc = 0; xc < NXC; ++xc) {
                GtRegs<64> xr;
                gt_load<64>(a.x, row0, DX, xc * 64, nv, xr);
                __syncthreads();  // sB's readers are done; sD is complete
                gt_store<64>(xr, sB, LDH);
                __syncthreads();
                if (xc == 0) {
#pragma unroll
                    for (int r = 0; r < RPG / 16; ++r)
                        db[s] = col_sum16(db[s], sD + (q * RPG + 16 * r) * LDD + ch, LDD);
                }
#pragma unroll
                for (int i = 0; i < IPW; ++i) {
                    const int it = wv * IPW + i, bi = it >> 1, bj = it & 1;
                    f32x16 &c = accW[(s * NXC + xc) * IPW + i];
                    c = mma_pf<TM, true, true>(sD + bi * 32, LDD, sB + bj * 32, LDH, c);
                }
            }
#pragma unroll
            for (int jq = 0; jq < NXC; ++jq)
#pragma unroll
                for (int kc = 0; kc < NKC; ++kc) {
                    GtRegs<64> wreg;
                    gt_load<64>(a.w[s], kc * 64, DX, jq * 64, 64, wreg);
                    __syncthreads();
                    gt_store<64>(wreg, sB, LDH);
                    __syncthreads();
                    accX[jq] = mma_pf<64, false, true>(sD + wr * 32 * LDD + kc * 64, LDD, sB + wc * 32,
                                                       LDH, accX[jq]);
                }
        }
#pragma unroll
        for (int jq = 0; jq < NXC; ++jq) {
            const int col = jq * 64 + wc * 32 + (l & 31);
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = wr * 32 + acc_row(reg, l);
                if (row < nv) {
                    float v = accX[jq][reg];
                    if (MASK) v = ((sM[row][col >> 5] >> (col & 31)) & 1u) ? a.mscale * v : 0.f;
                    if (a.add) v += a.add[(row0 + row) * DX + col];
                    a.dx[(row0 + row) * DX + col] = v;
                }
            }
        }
    }
    float *sl = a.slab + static_cast<int64_t>(blockIdx.x) * gt_bwd_width<DY, DX, NS, LN>();
#pragma unroll
    for (int s = 0; s < NS; ++s)
#pragma unroll
        for (int xc = 0; xc < NXC; ++xc)
#pragma unroll
            for (int i = 0; i < IPW; ++i) {
                const int it = wv * IPW + i, bi = it >> 1, bj = it & 1;
                float *blk = sl + s * DY * DX;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg)
                    blk[(bi * 32 + acc_row(reg, l)) * DX + xc * 64 + bj * 32 + (l & 31)] =
                        accW[(s * NXC + xc) * IPW + i][reg];
            }
#pragma unroll
    for (int s = 0; s < NS; ++s) {
        __syncthreads();
        sB[q * DY + ch] = db[s];
        __syncthreads();
        if (tid < DY) {
            float v = sB[tid];
#pragma unroll
            for (int g = 1; g < NG; ++g) v += sB[g * DY + tid];
            sl[NS * DY * DX + s * DY + tid] = v;
        }
    }
    if (LN) {
        __syncthreads();
        sB[tid] = dg;
        sB[256 + tid] = dbt;
        __syncthreads();
        if (tid < 64) {
            float g = sB[tid], b = sB[256 + tid];
#pragma unroll
            for (int k = 1; k < 4; ++k) {
                g += sB[64 * k + tid];
                b += sB[256 + 64 * k + tid];
            }
            sl[NS * DY * DX + NS * DY + tid] = g;
            sl[NS * DY * DX + NS * DY + 64 + tid] = b;
        }
    }
}

// ---------------------------------------------------------------------------
// attention: 16 lanes x float4 per node row, LPH = 16 / heads lanes per head
// ---------------------------------------------------------------------------
template <int LPH>
__device__ __forceinline__ float head_sum(float v) {
#pragma unroll
    for (int off = 1; off < LPH; off <<= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

__device__ __forceinline__ float dot4(float4 a, float4 b) {
    return fmaf(a.w, b.w, fmaf(a.z, b.z, fmaf(a.y, b.y, a.x * b.x)));
}

// largest per-node trip count of the wave's four nodes
__device__ __forceinline__ int wave_max_deg(int d) {
    const int a = __shfl_xor(d, 16, kWave);
    d = a > d ? a : d;
    const int b = __shfl_xor(d, 32, kWave);
    return b > d ? b : d;
}

// the scaled score of one edge and its clamped exponential (the one expression
// of the forward and of both backward walks: the same bits in all three)
template <int LPH>
__device__ __forceinline__ float edge_score(float4 k4, float4 q4, float sq, float &s) {
    const float e = head_sum<LPH>(dot4(k4, q4)) / sq;
    s = expf(fminf(fmaxf(e, -5.f), 5.f));
    return e;
}

template <int LPH>
__global__ __launch_bounds__(256) void gt_attn_fwd_k(
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t ncap, float sq,
    float *__restrict__ attn, float *__restrict__ z, float *__restrict__ score,
    const int32_t *__restrict__ dims) {
    constexpr int HEADS = 16 / LPH;
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, c = tid & 15, head = c / LPH;
    const int64_t node = static_cast<int64_t>(blockIdx.x) * 16 + (tid >> 4);
    int beg = 0, deg = 0;
    float4 q4 = make_float4(0.f, 0.f, 0.f, 0.f);
    if (node < n) {
        beg = rowptr[node];
        deg = rowptr[node + 1] - beg;
        q4 = ld4(q + node * kGtW + 4 * c);
    }
    const int maxdeg = wave_max_deg(deg);
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    float zs = 0.f;
    for (int j = 0; j < maxdeg; ++j) {  // wave-uniform trip count
        const bool ok = j < deg;
        const int64_t u = col[ok ? beg + j : 0];
        const float4 k4 = ld4(k + u * kGtW + 4 * c), v4 = ld4(v + u * kGtW + 4 * c);
        float s;
        const float e = edge_score<LPH>(k4, q4, sq, s);
        if (!ok) s = 0.f;
        acc = fma4(v4, s, acc);
        zs += s;
        if (score && ok && c % LPH == 0) score[static_cast<int64_t>(beg + j) * HEADS + head] = e;
    }
    if (node < ncap) {
        const float den = zs + kGtZEps;
        st4_saved(attn + node * kGtW + 4 * c,
                  make_float4(acc.x / den, acc.y / den, acc.z / den, acc.w / den));
        if (c % LPH == 0) z[node * HEADS + head] = zs;
    }
}

// destinations: g = dattn / (z + eps), dz = -sum_d dattn attn / (z + eps),
// dQ[v] = sum_{u->v} de K[u]
template <int LPH>
__global__ __launch_bounds__(256) void gt_attn_bwd_dst_k(
    const float *__restrict__ dattn, const float *__restrict__ attn, const float *__restrict__ z,
    const float *__restrict__ q, const float *__restrict__ k, const float *__restrict__ v,
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col, int64_t ncap, float sq,
    float *__restrict__ g, float *__restrict__ dzs, float *__restrict__ dq,
    const int32_t *__restrict__ dims) {
    constexpr int HEADS = 16 / LPH;
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, c = tid & 15, head = c / LPH;
    const int64_t node = static_cast<int64_t>(blockIdx.x) * 16 + (tid >> 4);
    int beg = 0, deg = 0;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 q4 = zero, da = zero, at = zero;
    float den = 1.f;
    if (node < n) {
        beg = rowptr[node];
        deg = rowptr[node + 1] - beg;
        q4 = ld4(q + node * kGtW + 4 * c);
        da = ld4(dattn + node * kGtW + 4 * c);
        at = ld4(attn + node * kGtW + 4 * c);
        den = z[node * HEADS + head] + kGtZEps;
    }
    const float4 g4 = make_float4(da.x / den, da.y / den, da.z / den, da.w / den);
    const float dzv = -head_sum<LPH>(dot4(da, at)) / den;
    const int maxdeg = wave_max_deg(deg);
    float4 acc = zero;
    for (int j = 0; j < maxdeg; ++j) {
        const bool ok = j < deg;
        const int64_t u = col[ok ? beg + j : 0];
        const float4 k4 = ld4(k + u * kGtW + 4 * c), v4 = ld4(v + u * kGtW + 4 * c);
        float s;
        const float e = edge_score<LPH>(k4, q4, sq, s);
        const float ds = head_sum<LPH>(dot4(g4, v4)) + dzv;
        const float de = (ok && e >= -5.f && e <= 5.f) ? ds * s / sq : 0.f;
        acc = fma4(k4, de, acc);
    }
    if (node < ncap) {
        st4(g + node * kGtW + 4 * c, g4);
        st4(dq + node * kGtW + 4 * c, acc);
        if (c % LPH == 0) dzs[node * HEADS + head] = dzv;
    }
}

// sources, on the transposed CSR: dK[u] = sum_{u->v} de Q[v], dV[u] = sum s g[v]
template <int LPH>
__global__ __launch_bounds__(256) void gt_attn_bwd_src_k(
    const float *__restrict__ g, const float *__restrict__ dzs, const float *__restrict__ q,
    const float *__restrict__ k, const float *__restrict__ v, const int32_t *__restrict__ rowptr_t,
    const int32_t *__restrict__ col_t, int64_t ncap, float sq, float *__restrict__ dk,
    float *__restrict__ dv, const int32_t *__restrict__ dims) {
    constexpr int HEADS = 16 / LPH;
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, c = tid & 15, head = c / LPH;
    const int64_t node = static_cast<int64_t>(blockIdx.x) * 16 + (tid >> 4);
    int beg = 0, deg = 0;
    const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
    float4 k4 = zero, v4 = zero;
    if (node < n) {
        beg = rowptr_t[node];
        deg = rowptr_t[node + 1] - beg;
        k4 = ld4(k + node * kGtW + 4 * c);
        v4 = ld4(v + node * kGtW + 4 * c);
    }
    const int maxdeg = wave_max_deg(deg);
    float4 ak = zero, av = zero;
    for (int j = 0; j < maxdeg; ++j) {
        const bool ok = j < deg;
        const int64_t d = col_t[ok ? beg + j : 0];
        const float4 q4 = ld4(q + d * kGtW + 4 * c), g4 = ld4(g + d * kGtW + 4 * c);
        const float dzv = dzs[d * HEADS + head];
        float s;
        const float e = edge_score<LPH>(k4, q4, sq, s);
        const float ds = head_sum<LPH>(dot4(g4, v4)) + dzv;
        const float de = (ok && e >= -5.f && e <= 5.f) ? ds * s / sq : 0.f;
        ak = fma4(q4, de, ak);
        av = fma4(g4, ok ? s : 0.f, av);
    }
    if (node < ncap) {
        st4(dk + node * kGtW + 4 * c, ak);
        st4(dv + node * kGtW + 4 * c, av);
    }
}

static bool gt_heads_ok(int heads) {
    return heads == 1 || heads == 2 || heads == 4 || heads == 8 || heads == 16;
}

static int gt_grid(int64_t ntiles) { return static_cast<int>(ntiles < 256 ? ntiles : 256); }

#define SCGIB_GT_HEADS(CALL)                                                                    \
    switch (heads) {                                                                            \
        case 1: CALL(16); break;                                                                \
        case 2: CALL(8); break;                                                                 \
        case 4: CALL(4); break;                                                                 \
        case 8: CALL(2); break;                                                                 \
        default: CALL(1); break;                                                                \
    }

}  // namespace scgib

using namespace scgib;

extern "C" int64_t scgib_gt_slabs(int64_t n_nodes) {
    return n_nodes <= 0 ? 0 : gt_grid((n_nodes + TM - 1) / TM);
}

extern "C" int64_t scgib_gt_slab_width(int32_t which) {
    switch (which) {
        case 0: return gt_bwd_width<64, 128, 1, true>();   // FFN_layer2 + LN2
        case 1: return gt_bwd_width<128, 64, 1, false>();  // FFN_layer1
        case 2: return gt_bwd_width<64, 64, 1, true>();    // O + LN1
        case 3: return gt_bwd_width<64, 64, 3, false>();   // Q | K | V
        default: return 0;
    }
}

extern "C" int scgib_gt_qkv_fwd(const float *h, const float *wq, const float *bq, const float *wk,
                                const float *bk, const float *wv, const float *bv, int64_t n_nodes,
                                float *q, float *k, float *v, const int32_t *dims,
                                scgib_stream_t stream) {
    if (n_nodes < 0) return SCGIB_EINVAL;
    if (n_nodes == 0) return SCGIB_OK;
    if (!h || !wq || !bq || !wk || !bk || !wv || !bv || !q || !k || !v) return SCGIB_EINVAL;
    GtFwdArgs a{};
    a.x = h;
    a.w[0] = wq; a.w[1] = wk; a.w[2] = wv;
    a.b[0] = bq; a.b[1] = bk; a.b[2] = bv;
    a.y[0] = q; a.y[1] = k; a.y[2] = v;
    const unsigned grid = static_cast<unsigned>((n_nodes + TM - 1) / TM);
    gt_lin_fwd_k<64, 64, 3, kEpiBias><<<grid, 256, 0, as_stream(stream)>>>(a, n_nodes, dims);
    return launch_status();
}

extern "C" int scgib_gt_attn_fwd(const float *q, const float *k, const float *v,
                                 const int32_t *rowptr, const int32_t *col, int64_t n_nodes,
                                 int32_t heads, float *attn, float *z, float *score,
                                 const int32_t *dims, scgib_stream_t stream) {
    if (n_nodes < 0 || heads <= 0) return SCGIB_EINVAL;
    if (!gt_heads_ok(heads)) return SCGIB_EUNSUPPORTED;
    if (n_nodes == 0) return SCGIB_OK;
    // (col may be NULL: a graph without edges, never dereferenced then)
    if (!q || !k || !v || !rowptr || !attn || !z) return SCGIB_EINVAL;
    const unsigned grid = static_cast<unsigned>((n_nodes + 15) / 16);
    const float sq = sqrtf(static_cast<float>(kGtW / heads));
    hipStream_t st = as_stream(stream);
#define SCGIB_GT_CALL(LPH)                                                                      \
    gt_attn_fwd_k<LPH><<<grid, 256, 0, st>>>(q, k, v, rowptr, col, n_nodes, sq, attn, z, score, dims)
    SCGIB_GT_HEADS(SCGIB_GT_CALL)
#undef SCGIB_GT_CALL
    return launch_status();
}

extern "C" int scgib_gt_attn_bwd(const float *dattn, const float *attn, const float *z,
                                 const float *q, const float *k, const float *v,
                                 const int32_t *rowptr, const int32_t *col,
                                 const int32_t *rowptr_t, const int32_t *col_t, int64_t n_nodes,
                                 int32_t heads, float *g, float *dzs, float *dq, float *dk,
                                 float *dv, const int32_t *dims, scgib_stream_t stream) {
    if (n_nodes < 0 || heads <= 0) return SCGIB_EINVAL;
    if (!gt_heads_ok(heads)) return SCGIB_EUNSUPPORTED;
    if (n_nodes == 0) return SCGIB_OK;
    if (!dattn || !attn || !z || !q || !k || !v || !rowptr || !rowptr_t || !g || !dzs || !dq ||
        !dk || !dv)
        return SCGIB_EINVAL;
    const unsigned grid = static_cast<unsigned>((n_nodes + 15) / 16);
    const float sq = sqrtf(static_cast<float>(kGtW / heads));
    hipStream_t st = as_stream(stream);
#define SCGIB_GT_CALL(LPH)                                                                      \
    gt_attn_bwd_dst_k<LPH><<<grid, 256, 0, st>>>(dattn, attn, z, q, k, v, rowptr, col, n_nodes, \
                                                 sq, g, dzs, dq, dims)
    SCGIB_GT_HEADS(SCGIB_GT_CALL)
#undef SCGIB_GT_CALL
    int rc = launch_status();
    if (rc != SCGIB_OK) return rc;
#define SCGIB_GT_CALL(LPH)                                                                      \
    gt_attn_bwd_src_k<LPH><<<grid, 256, 0, st>>>(g, dzs, q, k, v, rowptr_t, col_t, n_nodes, sq, \
                                                 dk, dv, dims)
    SCGIB_GT_HEADS(SCGIB_GT_CALL)
#undef SCGIB_GT_CALL
    return launch_status();
}

extern "C" int scgib_gt_out_fwd(const float *attn, const float *h, const float *wo,
                                const float *bo, const float *gamma, const float *beta,
                                int64_t n_nodes, float *pre, float *stats, float *out,
                                const int32_t *dims, scgib_stream_t stream) {
    if (n_nodes < 0) return SCGIB_EINVAL;
    if (n_nodes == 0) return SCGIB_OK;
    if (!attn || !h || !wo || !bo || !gamma || !beta || !pre || !stats || !out) return SCGIB_EINVAL;
    GtFwdArgs a{};
    a.x = attn;
    a.w[0] = wo;
    a.b[0] = bo;
    a.y[0] = out;
    a.res = h;
    a.gamma = gamma;
    a.beta = beta;
    a.pre = pre;
    a.stats = stats;
    const unsigned grid = static_cast<unsigned>((n_nodes + TM - 1) / TM);
    gt_lin_fwd_k<64, 64, 1, kEpiResLn><<<grid, 256, 0, as_stream(stream)>>>(a, n_nodes, dims);
    return launch_status();
}

extern "C" int scgib_gt_ffn_fwd(const float *h1, const float *w1, const float *b1,
                                const float *w2, const float *b2, const float *gamma,
                                const float *beta, int64_t n_nodes, int32_t training,
                                uint64_t *rng, uint32_t *counter, const uint8_t *drop_mask,
                                float *r, uint32_t *bits, uint32_t *pos_bits, uint32_t *keep_bits,
                                float *pre, float *stats, float *out, const int32_t *dims,
                                scgib_stream_t stream) {
    if (n_nodes < 0) return SCGIB_EINVAL;
    if (n_nodes == 0) return SCGIB_OK;
    if (!h1 || !w1 || !b1 || !w2 || !b2 || !gamma || !beta || !r || !bits || !pre || !stats || !out)
        return SCGIB_EINVAL;
    if (training && !drop_mask && (!rng || !counter)) return SCGIB_EINVAL;
    const unsigned grid = static_cast<unsigned>((n_nodes + TM - 1) / TM);
    hipStream_t st = as_stream(stream);
    GtFwdArgs a{};
    a.x = h1;
    a.w[0] = w1;
    a.b[0] = b1;
    a.y[0] = r;
    a.rng = rng;
    a.cnt = counter;
    a.drop_mask = drop_mask;
    a.bits = bits;
    a.pos_bits = pos_bits;
    a.keep_bits = keep_bits;
    a.training = training != 0;
    gt_lin_fwd_k<64, 128, 1, kEpiReluDrop><<<grid, 256, 0, st>>>(a, n_nodes, dims);
    int rc = launch_status();
    if (rc != SCGIB_OK) return rc;
    GtFwdArgs c{};
    c.x = r;
    c.w[0] = w2;
    c.b[0] = b2;
    c.y[0] = out;
    c.res = h1;
    c.gamma = gamma;
    c.beta = beta;
    c.pre = pre;
    c.stats = stats;
    gt_lin_fwd_k<128, 64, 1, kEpiResLn><<<grid, 256, 0, st>>>(c, n_nodes, dims);
    return launch_status();
}

extern "C" int scgib_gt_ffn_bwd(const float *dout, const float *pre, const float *stats,
                                const float *gamma, const float *r, const uint32_t *bits,
                                int32_t training, const float *h1, const float *w1,
                                const float *w2, int64_t n_nodes, float *dp, float *dr, float *dh1,
                                float *slab2, float *slab1, const int32_t *dims,
                                scgib_stream_t stream) {
    if (n_nodes <= 0) return SCGIB_EINVAL;
    if (!dout || !pre || !stats || !gamma || !r || !bits || !h1 || !w1 || !w2 || !dp || !dr ||
        !dh1 || !slab2 || !slab1)
        return SCGIB_EINVAL;
    const int64_t nt = (n_nodes + TM - 1) / TM;
    const int grid = gt_grid(nt);
    hipStream_t st = as_stream(stream);
    GtBwdArgs a{};
    a.dy[0] = dout;
    a.w[0] = w2;
    a.x = r;
    a.bits = bits;
    a.mscale = training ? 2.f : 1.f;
    a.dx = dr;
    a.pre = pre;
    a.stats = stats;
    a.gamma = gamma;
    a.dp = dp;
    a.slab = slab2;
    gt_lin_bwd_k<64, 128, 1, true, true><<<grid, 256, 0, st>>>(a, n_nodes, nt, dims);
    int rc = launch_status();
    if (rc != SCGIB_OK) return rc;
    GtBwdArgs c{};
    c.dy[0] = dr;
    c.w[0] = w1;
    c.x = h1;
    c.add = dp;
    c.dx = dh1;
    c.slab = slab1;
    gt_lin_bwd_k<128, 64, 1, false, false><<<grid, 256, 0, st>>>(c, n_nodes, nt, dims);
    return launch_status();
}

extern "C" int scgib_gt_out_bwd(const float *dh1, const float *pre, const float *stats,
                                const float *gamma, const float *attn, const float *wo,
                                int64_t n_nodes, float *dp, float *dattn, float *slab,
                                const int32_t *dims, scgib_stream_t stream) {
    if (n_nodes <= 0) return SCGIB_EINVAL;
    if (!dh1 || !pre || !stats || !gamma || !attn || !wo || !dp || !dattn || !slab)
        return SCGIB_EINVAL;
    const int64_t nt = (n_nodes + TM - 1) / TM;
    GtBwdArgs a{};
    a.dy[0] = dh1;
    a.w[0] = wo;
    a.x = attn;
    a.dx = dattn;
    a.pre = pre;
    a.stats = stats;
    a.gamma = gamma;
    a.dp = dp;
    a.slab = slab;
    gt_lin_bwd_k<64, 64, 1, true, false><<<gt_grid(nt), 256, 0, as_stream(stream)>>>(a, n_nodes, nt,
                                                                                     dims);
    return launch_status();
}

extern "C" int scgib_gt_qkv_bwd(const float *dq, const float *dk, const float *dv, const float *h,
                                const float *wq, const float *wk, const float *wv,
                                const float *add, int64_t n_nodes, float *dh, float *slab,
                                const int32_t *dims, scgib_stream_t stream) {
    if (n_nodes <= 0) return SCGIB_EINVAL;
    if (!dq || !dk || !dv || !h || !wq || !wk || !wv || !dh || !slab) return SCGIB_EINVAL;
    const int64_t nt = (n_nodes + TM - 1) / TM;
    GtBwdArgs a{};
    a.dy[0] = dq; a.dy[1] = dk; a.dy[2] = dv;
    a.w[0] = wq; a.w[1] = wk; a.w[2] = wv;
    a.x = h;
    a.add = add;
    a.dx = dh;
    a.slab = slab;
    gt_lin_bwd_k<64, 64, 3, false, false><<<gt_grid(nt), 256, 0, as_stream(stream)>>>(a, n_nodes,
                                                                                      nt, dims);
    return launch_status();
}
