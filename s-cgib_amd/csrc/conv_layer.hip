// Fused graph-convolution layer (gfx950), exact-f32 MFMA tiles: the GCN and
// GraphSAGE encoders' layer (DGL GraphConv(norm='both') and SAGEConv('mean'),
// reference models.py:75-104):
//
//   agg[v] = c_dst[v] * sum_{u -> v} c_src[u] x[u]        (CSR order, fixed)
//   out[v] = act(agg[v] Wn + x[v] Ws + b)                 (Ws optional)
//
// conv_norm_k writes the two coefficient vectors of a graph from its row
// pointers (GCN: deg^-1/2 on both sides; mean: 1 / in-degree on the
// destination), degrees clamped to 1.
//
// conv_fwd_k, one 64-row tile per workgroup: the weighted CSR gather of the
// tile's rows (latency-batched: every load unconditional, slots past a row's
// degree enter with weight 0) lands in LDS and in `agg` (saved for dWn);
// the product walks the weight in 64 x 64 tiles (sum index x output column),
// each staged through one LDS buffer while the next is in flight in registers;
// a wave owns a 32-row x 32-column sub-tile per 64 output columns.  With a
// self term the x tile goes through the same LDS tile first, so the kernel
// holds one [64][d_in + 1] tile and one weight tile: at most 49.8 KiB, three
// workgroups per CU.  The weights are read in their own layout: [in][out]
// (GraphConv.weight, WCOL) or [out][in] (the SAGE linears).
//
// Backward, two launches.  conv_wgrad_k: workgroups loop over tiles, form
// dz = dout * [out > 0], and accumulate dWn = agg^T dz, dWs = x^T dz and
// db = sum dz in MFMA registers (TN products over the tile's rows, agg / x
// staged 64 columns at a time), one slab per workgroup in the weight's own
// layout, summed in a fixed order by scgib_slab_reduce_multi.
// dx[u] = c_src[u] sum_{u -> v} c_dst[v] (dz[v] Wn^T) + dz[u] Ws^T is
// (gather of dz over the transposed CSR, coefficients swapped) Wn^T + dz Ws^T:
// conv_fwd_k itself with d_in and d_out exchanged and the weight read the
// other way.  Its gather needs the dz of OTHER tiles' rows complete, hence
// the launch boundary between the two kernels.  The dx epilogue can apply the
// previous layer's ReLU mask [x > 0], so that layer receives its dz directly.
//
// Capacity mode (dims): rows >= dims[0] are written as zeros and are zero in
// every product operand, so they never reach a slab.  No atomics; every sum
// has a fixed order.
#include "mfma_tile.h"

namespace scgib {

constexpr int kConvGcn = 0, kConvMean = 1;

__global__ __launch_bounds__(256) void conv_norm_k(const int32_t *__restrict__ rowptr,
                                                   const int32_t *__restrict__ rowptr_t,
                                                   int64_t ncap, int mode, float *__restrict__ cs,
                                                   float *__restrict__ cd,
                                                   const int32_t *__restrict__ dims) {
    const int64_t n = eff_count(dims, 0, ncap);
    const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (v >= ncap) return;
    float s = 0.f, d = 0.f;
    if (v < n) {
        const int din = rowptr[v + 1] - rowptr[v], dout = rowptr_t[v + 1] - rowptr_t[v];
        const float fi = static_cast<float>(din > 1 ? din : 1);
        const float fo = static_cast<float>(dout > 1 ? dout : 1);
        s = mode == kConvGcn ? 1.f / sqrtf(fo) : 1.f;
        d = mode == kConvGcn ? 1.f / sqrtf(fi) : 1.f / fi;
    }
    if (cs) cs[v] = s;
    if (cd) cd[v] = d;
}

// a [64][C] block (columns c0 .. c0 + C of a row-major matrix of row length
// ld) in registers; rows >= nv read as zeros (loads unconditional, clamped)
template <int C>
struct TileRegs {
    float4 v[64 * C / 4 / 256];
};

template <int C>
__device__ __forceinline__ void load_tile(const float *__restrict__ src, int64_t row0, int ld,
                                          int c0, int nv, TileRegs<C> &r) {
    constexpr int N = 64 * C / 4 / 256, Q = C / 4;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int idx = tid + 256 * k, rr = idx / Q, cq = idx % Q;
        r.v[k] = ld_ok(reinterpret_cast<const float4 *>(src), ((row0 + rr) * ld + c0) / 4 + cq,
                       (row0 * ld + c0) / 4 + cq, rr < nv, make_float4(0.f, 0.f, 0.f, 0.f));
    }
}

// ... to LDS with row stride lds (padded strides: scalar stores)
template <int C>
__device__ __forceinline__ void store_tile(const TileRegs<C> &r, float *s, int lds) {
    constexpr int N = 64 * C / 4 / 256, Q = C / 4;
    const int tid = threadIdx.x;
#pragma unroll
    for (int k = 0; k < N; ++k) {
        const int idx = tid + 256 * k, rr = idx / Q, cq = idx % Q;
        float *d = s + rr * lds + 4 * cq;
        d[0] = r.v[k].x; d[1] = r.v[k].y; d[2] = r.v[k].z; d[3] = r.v[k].w;
    }
}

// Weighted aggregation of RPT rows (row0 + rbase + k * rpp) for the 4-channel
// chunk c: acc = cd[v] * sum_{u in N(v)} cs[u] x[u] in CSR order (cs / cd
// NULL: 1).  Loads batched as in gather_rows (mfma_tile.h): rows past nv
// duplicate row nv - 1, neighbour slots past a row's degree read a clamped
// valid edge and enter through fmaf(x, 0, acc).  Requires nv >= 1.
template <int RPT, int LPR, bool HAS_CS>
__device__ __forceinline__ void conv_gather(const float4 *__restrict__ h4,
                                            const int32_t *__restrict__ rowptr,
                                            const int32_t *__restrict__ col,
                                            const float *__restrict__ cs,
                                            const float *__restrict__ cd, int64_t row0, int nv,
                                            int rbase, int rpp, int c, float4 (&acc)[RPT]) {
    int32_t beg[RPT], deg[RPT];
    int64_t vrow[RPT];
    float cdv[RPT];
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        const int rr = rbase + k * rpp;
        vrow[k] = row0 + (rr < nv ? rr : nv - 1);
        beg[k] = rowptr[vrow[k]];
        deg[k] = rowptr[vrow[k] + 1];
        cdv[k] = 1.f;
    }
    if (cd) {
#pragma unroll
        for (int k = 0; k < RPT; ++k) cdv[k] = cd[vrow[k]];
    }
    int maxdeg = 0, maxend = 0;
#pragma unroll
    for (int k = 0; k < RPT; ++k) {
        acc[k] = make_float4(0.f, 0.f, 0.f, 0.f);
        maxend = deg[k] > maxend ? deg[k] : maxend;
        deg[k] -= beg[k];
        maxdeg = deg[k] > maxdeg ? deg[k] : maxdeg;
    }
    for (int j0 = 0; j0 < maxdeg; j0 += 4) {
        int32_t u[RPT][4];
#pragma unroll
        for (int k = 0; k < RPT; ++k)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const int32_t e = beg[k] + j0 + t;
                u[k][t] = col[e < maxend ? e : maxend - 1];
            }
        float4 a[RPT][4];
        float w[RPT][4];
#pragma unroll
        for (int k = 0; k < RPT; ++k)
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                w[k][t] = HAS_CS ? cs[u[k][t]] : 1.f;
                a[k][t] = h4[static_cast<int64_t>(u[k][t]) * LPR + c];
            }
#pragma unroll
        for (int k = 0; k < RPT; ++k)
#pragma unroll
            for (int t = 0; t < 4; ++t)
                acc[k] = fma4(a[k][t], j0 + t < deg[k] ? w[k][t] : 0.f, acc[k]);
    }
#pragma unroll
    for (int k = 0; k < RPT; ++k)
        acc[k] = make_float4(cdv[k] * acc[k].x, cdv[k] * acc[k].y, cdv[k] * acc[k].z,
                             cdv[k] * acc[k].w);
}

// the tile's aggregated rows -> sA (stride KD + 1) and, rows < nv, `agg`
template <int KD, bool HAS_CS>
__device__ __forceinline__ void conv_gather_tile(const float *__restrict__ x,
                                                 const int32_t *__restrict__ rowptr,
                                                 const int32_t *__restrict__ col,
                                                 const float *__restrict__ cs,
                                                 const float *__restrict__ cd, int64_t row0,
                                                 int nv, float *sA, float *__restrict__ agg) {
    constexpr int LPR = KD / 4, RPP = 256 / LPR, RPT = KD == 32 ? 2 : 4, NB = 64 / (RPP * RPT);
    constexpr int LDA = KD + 1;
    const int tid = threadIdx.x, c = tid % LPR, rloc = tid / LPR;
#pragma unroll 1
    for (int b = 0; b < NB; ++b) {
        const int rbase = b * RPT * RPP + rloc;
        float4 acc[RPT];
        conv_gather<RPT, LPR, HAS_CS>(reinterpret_cast<const float4 *>(x), rowptr, col, cs, cd,
                                      row0, nv, rbase, RPP, c, acc);
#pragma unroll
        for (int k = 0; k < RPT; ++k) {
            const int rr = rbase + k * RPP;
            const float4 v = rr < nv ? acc[k] : make_float4(0.f, 0.f, 0.f, 0.f);
            float *d = sA + rr * LDA + 4 * c;
            d[0] = v.x; d[1] = v.y; d[2] = v.z; d[3] = v.w;
            if (agg && rr < nv) st4_saved(agg + (row0 + rr) * KD + 4 * c, v);
        }
    }
}

// out[64][ND] tile = act(gather(x)[64][KD] Wn + xself[64][KD] Ws + b), masked
// by [mask > 0] when given.  WCOL: the weights are [KD][ND] row-major (the sum
// index first), else [ND][KD].
template <int KD, int ND, bool SELF, bool WCOL>
__global__ __launch_bounds__(256) void conv_fwd_k(
    const float *__restrict__ x, const float *__restrict__ xself,
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const float *__restrict__ cs, const float *__restrict__ cd, int64_t ncap,
    const float *__restrict__ wn, const float *__restrict__ ws, const float *__restrict__ bias,
    int relu, const float *__restrict__ mask, float *__restrict__ agg, float *__restrict__ out,
    const int32_t *__restrict__ dims) {
    constexpr int LDA = KD + 1, KC = KD < 64 ? KD : 64, NCW = ND < 64 ? ND : 64;
    constexpr int NKC = KD / KC, NQ = ND / NCW, PER = NKC * NQ, T = (SELF ? 2 : 1) * PER;
    constexpr int WR = WCOL ? KC : NCW, WC = WCOL ? NCW : KC, LDW = WC + 1;
    constexpr int WT4 = WR * WC / 4 / 256, WQ = WC / 4;
    static_assert(NQ <= 2 && WT4 >= 1, "conv_fwd_k: shape");
    __shared__ float sA[TM * LDA];
    __shared__ float sW[WR * LDW];
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const int64_t row0 = xcd_remap(blockIdx.x, gridDim.x) * TM;
    const int nv = static_cast<int>(n - row0 < TM ? (n - row0 > 0 ? n - row0 : 0) : TM);
    if (dims) {
        const int ncr = static_cast<int>(ncap - row0 < TM ? ncap - row0 : TM);
        for (int idx = nv * ND + tid; idx < ncr * ND; idx += 256) out[row0 * ND + idx] = 0.f;
        if (agg)
            for (int idx = nv * KD + tid; idx < ncr * KD; idx += 256) agg[row0 * KD + idx] = 0.f;
        if (nv == 0) return;
    }
    // weight tile of step t: source (self first), 64-wide k chunk, 64-wide column chunk
    float4 wreg[WT4];
    auto load_w = [&](int t) {
        const float *w = (SELF && t < PER) ? ws : wn;
        const int kc = (t % PER) / NQ, nq = t % NQ;
        const int r0 = WCOL ? kc * KC : nq * NCW, c0 = WCOL ? nq * NCW : kc * KC;
        const int ldw = WCOL ? ND : KD;
#pragma unroll
        for (int k = 0; k < WT4; ++k) {
            const int idx = tid + 256 * k, rr = idx / WQ, cq = idx % WQ;
            wreg[k] = reinterpret_cast<const float4 *>(w + static_cast<int64_t>(r0 + rr) * ldw + c0)[cq];
        }
    };
    load_w(0);
    f32x16 acc0 = zero16(), acc1 = zero16();
    const bool active = ND >= 64 || wc == 0;  // a 32-column output: one column of waves
#pragma unroll
    for (int t = 0; t < T; ++t) {
        if (t % PER == 0) {  // the operand tile of this source (the previous one's reads are done)
            if (SELF && t == 0) {
                TileRegs<KD> xr;
                load_tile<KD>(xself, row0, KD, 0, nv, xr);
                store_tile<KD>(xr, sA, LDA);
            } else if (cs) {
                conv_gather_tile<KD, true>(x, rowptr, col, cs, cd, row0, nv, sA, agg);
            } else {
                conv_gather_tile<KD, false>(x, rowptr, col, cs, cd, row0, nv, sA, agg);
            }
        }
#pragma unroll
        for (int k = 0; k < WT4; ++k) {
            const int idx = tid + 256 * k, rr = idx / WQ, cq = idx % WQ;
            float *d = sW + rr * LDW + 4 * cq;
            d[0] = wreg[k].x; d[1] = wreg[k].y; d[2] = wreg[k].z; d[3] = wreg[k].w;
        }
        __syncthreads();
        if (t + 1 < T) load_w(t + 1);  // in flight across this step's products
        if (active) {
            const int kc = (t % PER) / NQ, nq = t % NQ;
            const float *A = sA + wr * 32 * LDA + kc * KC;
            const float *B = WCOL ? sW + wc * 32 : sW + wc * 32 * LDW;
            if (nq == 0) acc0 = mma_pf<KC, false, WCOL>(A, LDA, B, LDW, acc0);
            else acc1 = mma_pf<KC, false, WCOL>(A, LDA, B, LDW, acc1);
        }
        if (t + 1 < T) __syncthreads();  // sW (and sA) are rewritten next
    }
    if (!active) return;
#pragma unroll
    for (int nq = 0; nq < NQ; ++nq) {
        const int ccol = nq * 64 + wc * 32 + (l & 31);
        const float b = bias ? bias[ccol] : 0.f;
        const f32x16 &acc = nq == 0 ? acc0 : acc1;
        float mv[16];
        if (mask) {  // loaded together (clamped rows) ahead of the stores
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = wr * 32 + acc_row(reg, l);
                mv[reg] = mask[(row0 + (row < nv ? row : nv - 1)) * ND + ccol];
            }
        }
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int row = wr * 32 + acc_row(reg, l);
            float v = acc[reg] + b;
            if (relu) v = fmaxf(v, 0.f);
            if (mask) v = mv[reg] > 0.f ? v : 0.f;
            if (row < nv) out[(row0 + row) * ND + ccol] = v;
        }
    }
}

// slab per workgroup: dWn [DIN * DOUT] | dWs [DIN * DOUT] (SELF) | db [DOUT],
// the weight blocks in the weight's own layout (WCOL: [DIN][DOUT])
template <int DIN, int DOUT, bool SELF, bool WCOL>
__global__ __launch_bounds__(256) void conv_wgrad_k(
    const float *__restrict__ dout, const float *__restrict__ outv, const float *__restrict__ agg,
    const float *__restrict__ x, int64_t ncap, int64_t ntiles, float *__restrict__ dz,
    float *__restrict__ slab, const int32_t *__restrict__ dims) {
    constexpr int KCH = DIN < 64 ? DIN : 64, NCH = DIN / KCH, KB = KCH / 32, JB = DOUT / 32;
    constexpr int ITEMS = KB * JB, IPW = ITEMS >= 4 ? ITEMS / 4 : 1;
    constexpr int NSRC = (SELF ? 2 : 1) * NCH, NG = 256 / DOUT;
    constexpr int DQ = DOUT / 4, DN = 64 * DOUT / 4 / 256;
    static_assert(DOUT == 64 || DOUT == 128, "conv_wgrad_k: d_out");
    // TN products read both tiles by column (consecutive lanes, consecutive
    // addresses): no padding needed
    __shared__ float sD[TM * DOUT];
    __shared__ float sA[TM * KCH];
    __shared__ float sB[256];
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    const int ch = tid % DOUT, q = tid / DOUT;
    f32x16 acc[NSRC * IPW];
#pragma unroll
    for (int i = 0; i < NSRC * IPW; ++i) acc[i] = zero16();
    float db = 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TM;
        const int nv = static_cast<int>(n - row0 < TM ? (n - row0 > 0 ? n - row0 : 0) : TM);
        if (dims && outv) {
            const int ncr = static_cast<int>(ncap - row0 < TM ? ncap - row0 : TM);
            for (int idx = nv * DOUT + tid; idx < ncr * DOUT; idx += 256) dz[row0 * DOUT + idx] = 0.f;
        }
        if (nv == 0) continue;  // block-uniform
        TileRegs<DOUT> d;
        load_tile<DOUT>(dout, row0, DOUT, 0, nv, d);
        if (outv) {
            TileRegs<DOUT> m;
            load_tile<DOUT>(outv, row0, DOUT, 0, nv, m);
#pragma unroll
            for (int k = 0; k < DN; ++k) {
                d.v[k].x = m.v[k].x > 0.f ? d.v[k].x : 0.f;
                d.v[k].y = m.v[k].y > 0.f ? d.v[k].y : 0.f;
                d.v[k].z = m.v[k].z > 0.f ? d.v[k].z : 0.f;
                d.v[k].w = m.v[k].w > 0.f ? d.v[k].w : 0.f;
            }
        }
        TileRegs<KCH> a;
        load_tile<KCH>(agg, row0, DIN, 0, nv, a);
        __syncthreads();  // previous tile's LDS reads are done
#pragma unroll
        for (int k = 0; k < DN; ++k) {
            const int idx = tid + 256 * k, rr = idx / DQ, cq = idx % DQ;
            st4(sD + rr * DOUT + 4 * cq, d.v[k]);
            if (outv && rr < nv) st4_saved(dz + (row0 + rr) * DOUT + 4 * cq, d.v[k]);
        }
#pragma unroll
        for (int s = 0; s < NSRC; ++s) {
            if (s > 0) __syncthreads();  // the previous chunk's reads are done
            store_tile<KCH>(a, sA, KCH);
            __syncthreads();
            if (s + 1 < NSRC)
                load_tile<KCH>((s + 1) / NCH ? x : agg, row0, DIN, ((s + 1) % NCH) * KCH, nv, a);
            if (s == 0) {
#pragma unroll
                for (int r = 0; r < 64 / NG / 16; ++r)
                    db = col_sum16(db, sD + (q + NG * 16 * r) * DOUT + ch, NG * DOUT);
            }
#pragma unroll
            for (int i = 0; i < IPW; ++i) {
                const int it = wv * IPW + i;
                if (it < ITEMS) {  // wave-uniform
                    const int bi = it / JB, bj = it % JB;
                    f32x16 &c = acc[s * IPW + i];
                    if (WCOL) c = mma_pf<TM, true, true>(sA + bi * 32, KCH, sD + bj * 32, DOUT, c);
                    else c = mma_pf<TM, true, true>(sD + bj * 32, DOUT, sA + bi * 32, KCH, c);
                }
            }
        }
    }
    float *sl = slab + static_cast<int64_t>(blockIdx.x) * ((SELF ? 2 : 1) * DIN * DOUT + DOUT);
#pragma unroll
    for (int s = 0; s < NSRC; ++s)
#pragma unroll
        for (int i = 0; i < IPW; ++i) {
            const int it = wv * IPW + i;
            if (it < ITEMS) {
                const int bi = it / JB, bj = it % JB;
                float *blk = sl + (s / NCH) * DIN * DOUT;
                const int k0 = (s % NCH) * KCH + bi * 32, j0 = bj * 32;
#pragma unroll
                for (int reg = 0; reg < 16; ++reg) {
                    const int ar = acc_row(reg, l), ac = l & 31;
                    if (WCOL) blk[(k0 + ar) * DOUT + j0 + ac] = acc[s * IPW + i][reg];
                    else blk[(j0 + ar) * DIN + k0 + ac] = acc[s * IPW + i][reg];
                }
            }
        }
    __syncthreads();
    sB[q * DOUT + ch] = db;
    __syncthreads();
    if (tid < DOUT) {
        float s = sB[tid];
#pragma unroll
        for (int g = 1; g < NG; ++g) s += sB[g * DOUT + tid];
        sl[(SELF ? 2 : 1) * DIN * DOUT + tid] = s;
    }
}

static int conv_grid(int64_t ntiles) { return static_cast<int>(ntiles < 256 ? ntiles : 256); }

static bool conv_shape_ok(int d_in, int d_out) {
    return (d_in == 32 && d_out == 128) || (d_in == 128 && d_out == 128) ||
           (d_in == 128 && d_out == 64) || (d_in == 32 && d_out == 64) ||
           (d_in == 64 && d_out == 64);
}

// conv_fwd_k for (kd, nd): the five layer shapes and, for the dx pass, their
// transposes
template <bool SELF, bool WCOL>
static int launch_conv_fwd(int kd, int nd, unsigned grid, hipStream_t st, const float *x,
                           const float *xself, const int32_t *rowptr, const int32_t *col,
                           const float *cs, const float *cd, int64_t n, const float *wn,
                           const float *ws, const float *bias, int relu, const float *mask,
                           float *agg, float *out, const int32_t *dims) {
#define SCGIB_CONV_FWD(KD, ND)                                                                  \
    if (kd == KD && nd == ND) {                                                                 \
        conv_fwd_k<KD, ND, SELF, WCOL><<<grid, 256, 0, st>>>(x, xself, rowptr, col, cs, cd, n,  \
                                                             wn, ws, bias, relu, mask, agg,     \
                                                             out, dims);                        \
        return launch_status();                                                                 \
    }
    SCGIB_CONV_FWD(128, 128)
    SCGIB_CONV_FWD(64, 64)
    if constexpr (SELF != WCOL) {  // the layer itself
        SCGIB_CONV_FWD(32, 128)
        SCGIB_CONV_FWD(128, 64)
        SCGIB_CONV_FWD(32, 64)
    } else {  // its dx pass
        SCGIB_CONV_FWD(128, 32)
        SCGIB_CONV_FWD(64, 128)
        SCGIB_CONV_FWD(64, 32)
    }
#undef SCGIB_CONV_FWD
    return SCGIB_EUNSUPPORTED;
}

template <bool SELF, bool WCOL>
static int launch_conv_wgrad(int d_in, int d_out, int grid, hipStream_t st, const float *dout,
                             const float *outv, const float *agg, const float *x, int64_t n,
                             int64_t nt, float *dz, float *slab, const int32_t *dims) {
#define SCGIB_CONV_WGRAD(DI, DO)                                                                \
    if (d_in == DI && d_out == DO) {                                                            \
        conv_wgrad_k<DI, DO, SELF, WCOL><<<grid, 256, 0, st>>>(dout, outv, agg, x, n, nt, dz,   \
                                                               slab, dims);                     \
        return launch_status();                                                                 \
    }
    SCGIB_CONV_WGRAD(32, 128)
    SCGIB_CONV_WGRAD(128, 128)
    SCGIB_CONV_WGRAD(128, 64)
    SCGIB_CONV_WGRAD(32, 64)
    SCGIB_CONV_WGRAD(64, 64)
#undef SCGIB_CONV_WGRAD
    return SCGIB_EUNSUPPORTED;
}

}  // namespace scgib

using namespace scgib;

extern "C" int scgib_conv_norm(const int32_t *rowptr, const int32_t *rowptr_t, int64_t n_nodes,
                               int32_t mode, float *c_src, float *c_dst, const int32_t *dims,
                               scgib_stream_t stream) {
    if (n_nodes < 0 || (mode != kConvGcn && mode != kConvMean)) return SCGIB_EINVAL;
    if (n_nodes == 0) return SCGIB_OK;
    if (!rowptr || !rowptr_t || (!c_src && !c_dst)) return SCGIB_EINVAL;
    const unsigned grid = static_cast<unsigned>((n_nodes + 255) / 256);
    conv_norm_k<<<grid, 256, 0, as_stream(stream)>>>(rowptr, rowptr_t, n_nodes, mode, c_src, c_dst,
                                                     dims);
    return launch_status();
}

extern "C" int64_t scgib_conv_slabs(int64_t n_nodes) {
    return n_nodes <= 0 ? 0 : conv_grid((n_nodes + TM - 1) / TM);
}

extern "C" int64_t scgib_conv_slab_width(int32_t d_in, int32_t d_out, int32_t has_self) {
    if (!conv_shape_ok(d_in, d_out)) return 0;
    return static_cast<int64_t>(has_self ? 2 : 1) * d_in * d_out + d_out;
}

extern "C" int scgib_conv_layer_fwd(const float *x, const int32_t *rowptr, const int32_t *col,
                                    const float *c_src, const float *c_dst, int64_t n_nodes,
                                    int32_t d_in, int32_t d_out, const float *w_neigh,
                                    const float *w_self, int32_t w_in_major, const float *bias,
                                    int32_t relu, float *agg, float *out, const int32_t *dims,
                                    scgib_stream_t stream) {
    if (n_nodes < 0 || d_in <= 0 || d_out <= 0) return SCGIB_EINVAL;
    if (!conv_shape_ok(d_in, d_out)) return SCGIB_EUNSUPPORTED;
    // (the two layer kinds: GraphConv = [in][out] weight, no self term;
    // SAGEConv = [out][in] linears with one)
    if ((w_self != nullptr) == (w_in_major != 0)) return SCGIB_EUNSUPPORTED;
    if (n_nodes == 0) return SCGIB_OK;
    // (col may be NULL: a graph without edges, never dereferenced then)
    if (!x || !rowptr || !w_neigh || !out) return SCGIB_EINVAL;
    const unsigned grid = static_cast<unsigned>((n_nodes + TM - 1) / TM);
    hipStream_t st = as_stream(stream);
    if (w_self)
        return launch_conv_fwd<true, false>(d_in, d_out, grid, st, x, x, rowptr, col, c_src, c_dst,
                                            n_nodes, w_neigh, w_self, bias, relu, nullptr, agg,
                                            out, dims);
    return launch_conv_fwd<false, true>(d_in, d_out, grid, st, x, x, rowptr, col, c_src, c_dst,
                                        n_nodes, w_neigh, nullptr, bias, relu, nullptr, agg, out,
                                        dims);
}

extern "C" int scgib_conv_layer_bwd(const float *dout, const float *out, const float *agg,
                                    const float *x, const int32_t *rowptr_t, const int32_t *col_t,
                                    const float *c_src, const float *c_dst, int64_t n_nodes,
                                    int32_t d_in, int32_t d_out, const float *w_neigh,
                                    const float *w_self, int32_t w_in_major, int32_t mask_x,
                                    float *dz, float *dx, float *slab, const int32_t *dims,
                                    scgib_stream_t stream) {
    if (n_nodes <= 0 || d_in <= 0 || d_out <= 0) return SCGIB_EINVAL;
    if (!conv_shape_ok(d_in, d_out)) return SCGIB_EUNSUPPORTED;
    if ((w_self != nullptr) == (w_in_major != 0)) return SCGIB_EUNSUPPORTED;
    if (!dout || !agg || !x || !w_neigh || !slab || (out && !dz)) return SCGIB_EINVAL;
    if (dx && !rowptr_t) return SCGIB_EINVAL;
    const int64_t nt = (n_nodes + TM - 1) / TM;
    const int grid = conv_grid(nt);
    hipStream_t st = as_stream(stream);
    const int rc = w_self ? launch_conv_wgrad<true, false>(d_in, d_out, grid, st, dout, out, agg, x,
                                                           n_nodes, nt, dz, slab, dims)
                          : launch_conv_wgrad<false, true>(d_in, d_out, grid, st, dout, out, agg,
                                                           x, n_nodes, nt, dz, slab, dims);
    if (rc != SCGIB_OK || !dx) return rc;
    // dx = (gather of dz over the transposed CSR, c_dst on the sources and
    // c_src on the destination) Wn^T + dz Ws^T [masked by x > 0]
    const float *g = out ? dz : dout;
    const float *mask = mask_x ? x : nullptr;
    const unsigned fgrid = static_cast<unsigned>(nt);
    if (w_self)
        return launch_conv_fwd<true, true>(d_out, d_in, fgrid, st, g, g, rowptr_t, col_t, c_dst,
                                           c_src, n_nodes, w_neigh, w_self, nullptr, 0, mask,
                                           nullptr, dx, dims);
    return launch_conv_fwd<false, false>(d_out, d_in, fgrid, st, g, g, rowptr_t, col_t, c_dst,
                                         c_src, n_nodes, w_neigh, nullptr, nullptr, 0, mask,
                                         nullptr, dx, dims);
}
