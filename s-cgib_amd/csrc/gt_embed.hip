// Folded entry of the Transformer encoder (gfx950), exact-f32 MFMA tiles:
//
//   h0 = (x[map] Wt^T) We^T
//   x   [rows_x][F]  raw normalised features, F <= 16
//   Wt  = transfer_d.weight  [32][F]   (no bias)
//   We  = embedding_h.weight [64][32]  (no bias)
//   map = ego -> parent row (int32 [n]), or NULL for the identity
//
// The counterpart of the GIN path's layer-0 fold: the features are gathered
// in-kernel (x_subs is never materialised), transfer_d and embedding_h are one
// launch, and t = x Wt^T [n][32] never leaves LDS: the backward recomputes it
// (a K = 16 product) instead of storing and reloading [n][32].
//
// gt_embed_fwd_k: one 64-row tile per workgroup.  The tile's rows of x go
// through map into LDS, zero-padded to 32 columns; a wave owns a 32 x 32
// sub-tile of h0; the tile is transposed through LDS for float4 stores.
// gt_embed_bwd_k: at most 256 workgroups loop over tiles (as gt_lin_bwd_k);
// per tile t is recomputed, dWe += dh0^T t, dt = dh0 We, dWt += dt^T x, in
// MFMA registers; one slab per workgroup, dWe [64][32] | dWt [32][F] (the
// weights' own layouts), summed by scgib_slab_reduce_multi jobs.  No gradient
// for x.
//
// Capacity mode (dims): rows >= dims[0] of h0 are zeros and enter no product.
// A map entry outside [0, rows_x) is clamped to the nearest row: no read
// leaves x.  No float atomics; every sum has a fixed order.
#include "mfma_tile.h"

namespace scgib {

constexpr int kGeT = 32;     // transfer width
constexpr int kGeW = 64;     // encoder width
constexpr int kGeFMax = 16;  // raw feature columns
constexpr int kGeLd = 33;    // LDS stride of the 32-wide tiles (x, t, dt, We)
constexpr int kGeLdW = 17;   // LDS stride of Wt (16 columns)

// the tile's rows of x (through map) -> sX [64][33]: columns >= F and rows
// >= nv are zeros.  Thread = (row, four columns); loads unconditional, clamped.
__device__ __forceinline__ void ge_gather_x(const float *__restrict__ x, int F, int64_t rows_x,
                                            const int32_t *__restrict__ map, int64_t row0, int nv,
                                            float *sX) {
    const int tid = threadIdx.x, rr = tid >> 2, c0 = (tid & 3) * 4;
    const bool rok = rr < nv;
    const int64_t vrow = row0 + (rok ? rr : 0);  // (nv >= 1: row0 is a valid row)
    int64_t src = map ? static_cast<int64_t>(map[vrow]) : vrow;
    src = src < 0 ? 0 : (src >= rows_x ? rows_x - 1 : src);
    float v[4];
#pragma unroll
    for (int j = 0; j < 4; ++j)
        v[j] = ld_ok(x, src * F + c0 + j, src * F, rok && c0 + j < F, 0.f);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        sX[rr * kGeLd + c0 + j] = v[j];
        sX[rr * kGeLd + 16 + c0 + j] = 0.f;
    }
}

// Wt [32][F] -> sWt [32][17] (columns >= F zero), We [64][32] -> sWe [64][33]
__device__ __forceinline__ void ge_stage_weights(const float *__restrict__ wt,
                                                 const float *__restrict__ we, int F, float *sWt,
                                                 float *sWe) {
    const int tid = threadIdx.x;
    float a[2];
    float4 b[2];
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int idx = tid + 256 * k, r = idx >> 4, c = idx & 15;
        a[k] = ld_ok(wt, static_cast<int64_t>(r) * F + c, 0, c < F, 0.f);
        b[k] = reinterpret_cast<const float4 *>(we)[idx];
    }
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int idx = tid + 256 * k;
        sWt[(idx >> 4) * kGeLdW + (idx & 15)] = a[k];
        float *d = sWe + (idx >> 3) * kGeLd + 4 * (idx & 7);
        d[0] = b[k].x; d[1] = b[k].y; d[2] = b[k].z; d[3] = b[k].w;
    }
}

// t rows [32 wr, 32 wr + 32) = x Wt^T (K = 16) -> sT; the forward's and the
// backward's one expression: the same bits in both
__device__ __forceinline__ void ge_transfer(const float *sX, const float *sWt, int wr, float *sT) {
    const int l = threadIdx.x & 63;
    const f32x16 t = mma_pf<16, false, false>(sX + wr * 32 * kGeLd, kGeLd, sWt, kGeLdW, zero16());
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
        sT[(wr * 32 + acc_row(reg, l)) * kGeLd + (l & 31)] = t[reg];
}

__global__ __launch_bounds__(256) void gt_embed_fwd_k(
    const float *__restrict__ x, int F, int64_t rows_x, const int32_t *__restrict__ map,
    const float *__restrict__ wt, const float *__restrict__ we, int64_t ncap,
    float *__restrict__ h0, const int32_t *__restrict__ dims) {
    __shared__ float sX[TM * kGeLd];
    __shared__ float sT[TM * kGeLd];
    __shared__ float sWe[kGeW * kGeLd];
    __shared__ float sWt[kGeT * kGeLdW];
    __shared__ float sH[TM * LDH];
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6, wr = wv >> 1, wc = wv & 1;
    const int64_t row0 = static_cast<int64_t>(blockIdx.x) * TM;
    const int nv = static_cast<int>(n - row0 < TM ? (n - row0 > 0 ? n - row0 : 0) : TM);
    const int ncr = static_cast<int>(ncap - row0 < TM ? ncap - row0 : TM);
    const int row = tid >> 2, part = tid & 3;
    if (nv == 0) {  // block-uniform: a tile of padded rows only
        if (row < ncr) {
            float *po = h0 + (row0 + row) * kGeW + part * 16;
#pragma unroll
            for (int j = 0; j < 16; j += 4) st4(po + j, make_float4(0.f, 0.f, 0.f, 0.f));
        }
        return;
    }
    ge_stage_weights(wt, we, F, sWt, sWe);
    ge_gather_x(x, F, rows_x, map, row0, nv, sX);
    __syncthreads();
    if (wc == 0) ge_transfer(sX, sWt, wr, sT);  // wave-uniform
    __syncthreads();
    const f32x16 acc = mma_pf<kGeT, false, false>(sT + wr * 32 * kGeLd, kGeLd,
                                                  sWe + wc * 32 * kGeLd, kGeLd, zero16());
#pragma unroll
    for (int reg = 0; reg < 16; ++reg)
        sH[(wr * 32 + acc_row(reg, l)) * LDH + wc * 32 + (l & 31)] = acc[reg];
    __syncthreads();
    if (row < ncr) {  // rows in [nv, ncr): x read as zeros, no bias: exact zeros
        const bool live = row < nv;
        float *po = h0 + (row0 + row) * kGeW + part * 16;
        const float *ps = sH + row * LDH + part * 16;
#pragma unroll
        for (int j = 0; j < 16; j += 4)
            st4(po + j, make_float4(live ? ps[j] : 0.f, live ? ps[j + 1] : 0.f,
                                    live ? ps[j + 2] : 0.f, live ? ps[j + 3] : 0.f));
    }
}

constexpr int ge_slab_width(int F) { return kGeW * kGeT + kGeT * F; }

// waves 0, 1: t (row halves), then dWe rows [32 wv, 32 wv + 32);
// waves 2, 3: dt = dh0 We (row halves); wave 2 then dWt
__global__ __launch_bounds__(256) void gt_embed_bwd_k(
    const float *__restrict__ dh0, const float *__restrict__ x, int F, int64_t rows_x,
    const int32_t *__restrict__ map, const float *__restrict__ wt, const float *__restrict__ we,
    int64_t ncap, int64_t ntiles, float *__restrict__ slab, const int32_t *__restrict__ dims) {
    __shared__ float sX[TM * kGeLd];
    __shared__ float sT[TM * kGeLd];
    __shared__ float sDt[TM * kGeLd];
    __shared__ float sWe[kGeW * kGeLd];
    __shared__ float sWt[kGeT * kGeLdW];
    __shared__ float sD[TM * LDH];
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, wv = tid >> 6;
    ge_stage_weights(wt, we, F, sWt, sWe);
    f32x16 accW = zero16();  // waves 0, 1: dWe block; wave 2: dWt
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t row0 = tile * TM;
        const int nv = static_cast<int>(n - row0 < TM ? (n - row0 > 0 ? n - row0 : 0) : TM);
        if (nv == 0) continue;  // block-uniform
        float4 d[4];  // the tile's rows of dh0; rows >= nv read as zeros
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = tid + 256 * k, rr = idx >> 4, cq = idx & 15;
            d[k] = ld_ok(reinterpret_cast<const float4 *>(dh0), (row0 + rr) * 16 + cq,
                         row0 * 16 + cq, rr < nv, make_float4(0.f, 0.f, 0.f, 0.f));
        }
        __syncthreads();  // the previous tile's LDS reads are done
        ge_gather_x(x, F, rows_x, map, row0, nv, sX);
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int idx = tid + 256 * k;
            float *p = sD + (idx >> 4) * LDH + 4 * (idx & 15);
            p[0] = d[k].x; p[1] = d[k].y; p[2] = d[k].z; p[3] = d[k].w;
        }
        __syncthreads();  // (first tile: the staged weights as well)
        if (wv < 2) {     // wave-uniform
            ge_transfer(sX, sWt, wv, sT);
        } else {
            const int wr = wv - 2;
            const f32x16 dt = mma_pf<TM, false, true>(sD + wr * 32 * LDH, LDH, sWe, kGeLd, zero16());
#pragma unroll
            for (int reg = 0; reg < 16; ++reg)
                sDt[(wr * 32 + acc_row(reg, l)) * kGeLd + (l & 31)] = dt[reg];
        }
        __syncthreads();
        if (wv < 2)
            accW = mma_pf<TM, true, true>(sD + wv * 32, LDH, sT, kGeLd, accW);
        else if (wv == 2)
            accW = mma_pf<TM, true, true>(sDt, kGeLd, sX, kGeLd, accW);
    }
    float *sl = slab + static_cast<int64_t>(blockIdx.x) * ge_slab_width(F);
    const int col = l & 31;
    if (wv < 2) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            sl[(wv * 32 + acc_row(reg, l)) * kGeT + col] = accW[reg];
    } else if (wv == 2 && col < F) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg)
            sl[kGeW * kGeT + acc_row(reg, l) * F + col] = accW[reg];
    }
}

static int ge_grid(int64_t ntiles) { return static_cast<int>(ntiles < 256 ? ntiles : 256); }

}  // namespace scgib

using namespace scgib;

extern "C" int64_t scgib_gt_embed_slabs(int64_t n_nodes) {
    return n_nodes <= 0 ? 0 : ge_grid((n_nodes + TM - 1) / TM);
}

extern "C" int64_t scgib_gt_embed_slab_width(int32_t n_feat) {
    return n_feat < 1 || n_feat > kGeFMax ? 0 : ge_slab_width(n_feat);
}

extern "C" int scgib_gt_embed_fwd(const float *x, int32_t n_feat, int64_t rows_x,
                                  const int32_t *map, const float *wt, const float *we,
                                  int64_t n_nodes, float *h0, const int32_t *dims,
                                  scgib_stream_t stream) {
    if (n_nodes < 0 || rows_x < 0) return SCGIB_EINVAL;
    if (n_feat < 1 || n_feat > kGeFMax) return SCGIB_EUNSUPPORTED;
    if (n_nodes == 0) return SCGIB_OK;
    if (!x || !wt || !we || !h0 || rows_x == 0) return SCGIB_EINVAL;
    if (!map && rows_x < n_nodes) return SCGIB_EINVAL;
    const unsigned grid = static_cast<unsigned>((n_nodes + TM - 1) / TM);
    gt_embed_fwd_k<<<grid, 256, 0, as_stream(stream)>>>(x, n_feat, rows_x, map, wt, we, n_nodes,
                                                        h0, dims);
    return launch_status();
}

extern "C" int scgib_gt_embed_bwd(const float *dh0, const float *x, int32_t n_feat,
                                  int64_t rows_x, const int32_t *map, const float *wt,
                                  const float *we, int64_t n_nodes, float *slab,
                                  const int32_t *dims, scgib_stream_t stream) {
    if (n_nodes <= 0 || rows_x <= 0) return SCGIB_EINVAL;
    if (n_feat < 1 || n_feat > kGeFMax) return SCGIB_EUNSUPPORTED;
    if (!dh0 || !x || !wt || !we || !slab) return SCGIB_EINVAL;
    if (!map && rows_x < n_nodes) return SCGIB_EINVAL;
    const int64_t nt = (n_nodes + TM - 1) / TM;
    gt_embed_bwd_k<<<ge_grid(nt), 256, 0, as_stream(stream)>>>(dh0, x, n_feat, rows_x, map, wt, we,
                                                               n_nodes, nt, slab, dims);
    return launch_status();
}
