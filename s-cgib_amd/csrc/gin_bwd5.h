// The d_in = 64 GIN layer backward on 32-row sub-tiles: gin_bwd5_k (stored
// agg), gin_bwd5z_k (agg-free), gin_bwd5r_k (r recomputed) and the steps they
// share.  Part of gin_layer.hip's translation unit, included below
// slab_fold_block / slab_fold8_block (gin_bwd5z_k's folded reduce blocks).
#pragma once
#include "gin_bn.h"

namespace scgib {

// ---------------------------------------------------------------------------
// gin_bwd5_k: the GIN layer backward (BN, d_in = 64) on 32-row sub-tiles,
// TWO workgroups per CU (63 KB LDS, <= 256 VGPRs).
//
// (Round 2 replaced gin_bwd2_k with it: 64-row tiles at one workgroup per
// CU, ~1.7 tiles per CU at QM9 B512, whose per-tile phases left the matrix
// pipe idle ~40 % of a tile and whose dword operand reads ran the GEMMs at
// ~80 % of the MFMA rate; phase trace r02.)  Here:
//   * 32-row sub-tiles, two workgroups per CU: one workgroup's non-MFMA
//     phases run under the other's MFMAs; ~3.4 sub-tiles per CU balance
//     better than 1.7 tiles;
//   * no K split: waves take whole products, 32 MFMAs per wave and pair:
//       pair A: waves 0,1 (N): dr block q = dz2 W2[:, 32q..] (K = 64, one
//               chain), dz1 = dr [r > 0] written straight from the accumulator;
//               waves 2,3 (T): dW2 rows 32q.. += dz2^T r (two blocks, K = 32 rows)
//       pair B: N: dW1 rows 32q.. += dz1^T agg;  T: d(agg) block q = dz1 W1[:, 32q..]
//   * every MFMA operand is fed four k values per ds_read_b128 (mma_rk4 /
//     mma_kk4x2, permuted k order): NN products read dz row-major and take
//     the wave's 32-column weight block from 32 VGPRs held for the whole
//     kernel (no weight image in LDS); TN products read transposed dz, r and
//     agg images [col][row];
//   * the next sub-tile's rows are loaded into registers before pair A and
//     written to the r^T / agg^T images once their last reader has passed a
//     barrier (r after pair A, agg after pair B): three barriers per sub-tile.
// The elementwise steps own one column and eight rows per thread (c = tid &
// 63, rows 8 w..8 w+7), so the transposed images are written as float4 runs
// and the row-major dz images as conflict-free dwords.
// LDS: dz2, dz1 row-major + transposed, r^T, agg^T, d(agg) staging = 63 KB.
// ---------------------------------------------------------------------------
constexpr int SM = 32;   // rows per sub-tile
constexpr int LDR = 68;  // row-major 64-wide images (= 4 mod 64: b128 reads conflict free)
constexpr int LDT = 36;  // transposed [64][32] images (rows k-contiguous)

// The steps of the sub-tile walk the three kernels share (w = tid >> 6, c =
// tid & 63; row arrays 64 floats wide).  What differs on purpose — barrier
// placement, which images a kernel keeps, when the next sub-tile's rows are
// loaded and staged — stays in the kernels.  gin_bwd5_k calls only rows_of
// and put_col8 and keeps its other steps inline, textually the helpers'
// bodies: with any further one of them called, the compiler hoists and
// schedules its loop differently (registers, LDS and instruction counts all
// within bounds) and its superbatch pass ran 472-479 -> 486-495 us, so it
// stays the instruction stream it was.  Keep the two in step.

// valid rows of sub-tile s of an n-row layer (0 past the end)
__device__ __forceinline__ int rows_of(int64_t n, int64_t s) {
    const int64_t v = n - s * SM;
    return static_cast<int>(v < SM ? (v > 0 ? v : 0) : SM);
}

// column c, rows 8 w..8 w + 7 of sub-tile s of a row-major [*, 64] array (r,
// agg, dy, z2); rows clamped to `last`, so every load is unconditional
__device__ __forceinline__ void load_col8(const float *__restrict__ src, int64_t s, int64_t last,
                                          int w, int c, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        int64_t row = s * SM + 8 * w + i;
        row = row < last ? row : last;
        v[i] = src[row * 64 + c];
    }
}

// those eight values -> [c][8 w..] of a transposed [64][LDT] image
__device__ __forceinline__ void put_col8(float *img, int w, int c, const float (&v)[8]) {
    float4 *p = reinterpret_cast<float4 *>(img + c * LDT + 8 * w);
    p[0] = make_float4(v[0], v[1], v[2], v[3]);
    p[1] = make_float4(v[4], v[5], v[6], v[7]);
}

// dz2 = sc (dy - c1 - (z2 - mean) k1), k1 = istd c2, rows past nv zero
// -> sD row-major; TR: and sDT transposed
template <bool TR>
__device__ __forceinline__ void stage_dz2(const float (&dy)[8], const float (&z2)[8], float sc,
                                          float c1, float mean, float k1, int nv, int w, int c,
                                          float *sD, float *sDT) {
    float d[8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float v = sc * (dy[i] - c1 - (z2[i] - mean) * k1);
        d[i] = 8 * w + i < nv ? v : 0.f;
        sD[(8 * w + i) * LDR + c] = d[i];
    }
    if constexpr (TR) put_col8(sDT, w, c, d);
}

// capacity mode: zero rows from.. of sub-tile s of out [ncap][64]
__device__ __forceinline__ void zero_pad(float *out, int64_t ncap, int64_t s, int from) {
    const int64_t row0 = s * SM;
    const int ncr = static_cast<int>(ncap - row0 < SM ? ncap - row0 : SM), tid = threadIdx.x;
    for (int idx = from * 64 + tid; idx < ncr * 64; idx += 256) out[row0 * 64 + idx] = 0.f;
}

// the first nv rows of the [32][LDH] staging image -> rows of sub-tile s of
// out, as full-row float4 stores
__device__ __forceinline__ void store_rows(const float *stage, float *out, int64_t s, int nv) {
    const int tid = threadIdx.x, c4 = tid & 15, rs = tid >> 4;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
        const int rr = rs + 16 * k;
        const float *pg = stage + rr * LDH + 4 * c4;
        const float4 v = make_float4(pg[0], pg[1], pg[2], pg[3]);
        if (rr < nv) st4(out + (s * SM + rr) * 64 + 4 * c4, v);
    }
}

// the slab's bias tail: the two lane halves of a wave hold partial column
// sums of its 32-wide block, whose 32 slots start at sl[at]
__device__ __forceinline__ void put_dbias(float dbias, int l, float *sl, int at) {
    dbias += __shfl_xor(dbias, 32, kWave);
    if (l < 32) sl[at + l] = dbias;
}

// WG = false: a frozen layer (the fine-tune freezing quirk, models.py:424-434:
// no parameter of it takes a gradient) — only the data-gradient chains run,
// dr and d(agg), each exactly as with WG (bitwise the same d(agg)); the
// dW products, the agg rows (read only by dW1), the transposed dz images
// and the slab are skipped.
template <int DIN, bool WG = true>
__global__ __launch_bounds__(256, 2) void gin_bwd5_k(
    const float *__restrict__ dy, const float *__restrict__ z2, const float *__restrict__ r,
    const float *__restrict__ agg, const float *__restrict__ stat,
    const float *__restrict__ coef, const float *__restrict__ w1, const float *__restrict__ w2,
    int64_t ncap, int64_t nsub, float *__restrict__ dagg_out, float *__restrict__ slab,
    const int32_t *__restrict__ dims, scgib_bn_bwd_pending pend) {
    static_assert(DIN == 64 && SM == 32, "64-wide rows, 32-row sub-tiles");
    constexpr int SLAB = 64 * 64 + 64 * DIN + 128;
    __shared__ __attribute__((aligned(16))) float sD[SM * LDR];   // dz2 [row][k]
    __shared__ __attribute__((aligned(16))) float sDT[64 * LDT];  // dz2 [col][row]
    __shared__ __attribute__((aligned(16))) float sE[SM * LDR];   // dz1
    __shared__ __attribute__((aligned(16))) float sET[64 * LDT];
    __shared__ __attribute__((aligned(16))) float sRT[64 * LDT];  // r [col][row]
    __shared__ __attribute__((aligned(16))) float sAT[DIN * LDT]; // agg [col][row]
    __shared__ float sG[SM * LDH];                                 // d(agg) staging
    __shared__ float sCoef[128];
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const int kk = l >> 5, li = l & 31;
    const bool nw = w < 2;  // wave-uniform role: N (dr, dW1) or T (dW2, d(agg))
    const int q = w & 1;    // the role's 32-wide block
    const int c = l;        // elementwise: column c, rows 8 w .. 8 w + 7
    const int64_t last = ncap - 1;
    const int64_t G = gridDim.x;
    SCGIB_MARK(0);
    SCGIB_MARK_HWID();
    BwdFin bfin;
    const int pend_ngr = static_cast<int>(((n + TM - 1) / TM + kGroup - 1) / kGroup);
    if (pend.gpart) bn_bwd_fin_load<false>(pend.gpart, pend_ngr, 0, bfin);
    const float s_mean = stat[c], s_istd = stat[64 + c], s_sc = stat[128 + c];
    float c1 = 0.f, c2 = 0.f;
    if (!pend.gpart) {
        c1 = coef[c];
        c2 = coef[64 + c];
    }
    // the wave's weight block: N waves W2[:, 32q..] (dr), T waves W1[:, 32q..] (d(agg))
    float wreg[32];
    {
        const float *wm = nw ? w2 : w1;
#pragma unroll
        for (int s = 0; s < 32; ++s) wreg[s] = wm[kperm(s, kk) * 64 + q * 32 + li];
    }
    float nx[4][8];  // a sub-tile's column c, rows 8 w + i: [0] dy, [1] z2, [2] r, [3] agg
    auto load_sub = [&](int64_t s) {
#pragma unroll
        for (int i = 0; i < 8; ++i) {  // in order of use: r, agg, then dy / z2
            int64_t row = s * SM + 8 * w + i;
            row = row < last ? row : last;
            nx[2][i] = r[row * 64 + c];
        }
        if constexpr (WG) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                int64_t row = s * SM + 8 * w + i;
                row = row < last ? row : last;
                nx[3][i] = agg[row * DIN + c];
            }
        }
#pragma unroll
        for (int i = 0; i < 8; ++i) {
            int64_t row = s * SM + 8 * w + i;
            row = row < last ? row : last;
            nx[0][i] = dy[row * 64 + c];
            nx[1][i] = z2[row * 64 + c];
        }
    };
    auto zero_pad = [&](int64_t s, int from) {
        const int64_t row0 = s * SM;
        const int ncr = static_cast<int>(ncap - row0 < SM ? ncap - row0 : SM);
        for (int idx = from * DIN + tid; idx < ncr * DIN; idx += 256) dagg_out[row0 * DIN + idx] = 0.f;
    };
    int64_t s = blockIdx.x;
    int nv = s < nsub ? rows_of(n, s) : 0;
    if (nv > 0) load_sub(s);
    if (pend.gpart) {  // finish the BN-backward sums; workgroup 0 writes dgamma, dbeta
        const double tot = bn_bwd_final<false>(pend.gpart, pend_ngr, bfin);
        const int cs = bfin_index();
        const bool lead = (tid & 63) < 32, w0 = blockIdx.x == 0 && lead;
        const float cf = bn_bwd_publish(cs, tot, n, pend.training, w0 ? pend.dgamma : nullptr,
                                        w0 ? pend.dbeta : nullptr, nullptr);
        if (lead) sCoef[cs] = cf;
    }
    if (nv > 0) {
        put_col8(sRT, w, c, nx[2]);
        if (WG) put_col8(sAT, w, c, nx[3]);
    }
    // the weight registers complete here: a load still counted at the loop
    // entry makes hipcc wait vmcnt(0..3) at their uses in EVERY iteration
    // (then for the next sub-tile's rows)
    vm_wait_all();
    __syncthreads();
    if (pend.gpart) {
        c1 = sCoef[c];
        c2 = sCoef[64 + c];
    }
    const float k1 = s_istd * c2;  // dz2 = sc (dy - c1 - (z2 - mean) istd c2)
    SCGIB_MARK(1);
    // N waves: dW1 blocks (q, 0), (q, 1) and db1; T waves: dW2 blocks and db2
    f32x16 accA = zero16(), accB = zero16();
    float dbias = 0.f;
    for (int it = 0; s < nsub; s += G, ++it) {
        if (nv == 0) {  // capacity tail: this and every later sub-tile is padding
            for (int64_t t = s; t < nsub; t += G) zero_pad(t, rows_of(n, t));
            break;
        }
        {   // dz2 (rows past nv zero) -> sD row-major and sDT transposed
            float d[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float v = s_sc * (nx[0][i] - c1 - (nx[1][i] - s_mean) * k1);
                d[i] = 8 * w + i < nv ? v : 0.f;
                sD[(8 * w + i) * LDR + c] = d[i];
            }
            if constexpr (WG) {
                float4 *p = reinterpret_cast<float4 *>(sDT + c * LDT + 8 * w);
                p[0] = make_float4(d[0], d[1], d[2], d[3]);
                p[1] = make_float4(d[4], d[5], d[6], d[7]);
            }
        }
        const int64_t next = s + G;
        const int next_nv = next < nsub ? rows_of(n, next) : 0;  // block-uniform
        if (next_nv > 0) load_sub(next);  // in flight during both product pairs
        lds_barrier();  // dz2 complete
        if (it == 0) SCGIB_MARK(2);
        if (nw) {  // dr block q, dz1 = dr [r > 0] -> sE, sET (mask by multiplication)
            const f32x16 dr = mma_rk4<8>(sD + li * LDR + 4 * kk, wreg, zero16());
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = acc_row(reg, l), col = q * 32 + li;
                const float v = dr[reg] * (sRT[col * LDT + row] > 0.f ? 1.f : 0.f);
                sE[row * LDR + col] = v;
                if (WG) sET[col * LDT + row] = v;
            }
        } else if constexpr (WG) {   // dW2 rows 32q.. += dz2^T r (db2 from the A operand)
            mma_kk4x2<4>(sDT + (q * 32 + li) * LDT + 4 * kk, sRT + li * LDT + 4 * kk,
                         sRT + (32 + li) * LDT + 4 * kk, accA, accB, dbias);
        }
        lds_barrier();  // dz1 complete; r and dz2 consumed
        if (it == 0) SCGIB_MARK(3);
        if (next_nv > 0) put_col8(sRT, w, c, nx[2]);
        if (nw) {  // dW1 rows 32q.. += dz1^T agg (db1 from the A operand)
            if constexpr (WG)
                mma_kk4x2<4>(sET + (q * 32 + li) * LDT + 4 * kk, sAT + li * LDT + 4 * kk,
                             sAT + (32 + li) * LDT + 4 * kk, accA, accB, dbias);
        } else {   // d(agg) block q = dz1 W1[:, 32q..] -> staging
            const f32x16 da = mma_rk4<8>(sE + li * LDR + 4 * kk, wreg, zero16());
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) sG[acc_row(reg, l) * LDH + q * 32 + li] = da[reg];
        }
        lds_barrier();  // d(agg) staged; agg and dz1 consumed
        if (it == 0) SCGIB_MARK(4);
        if (WG && next_nv > 0) put_col8(sAT, w, c, nx[3]);
        // d(agg) rows: full-row float4 stores (after the loads: in-order vmcnt)
        {
            const int c4 = tid & 15, rs = tid >> 4;
#pragma unroll
            for (int k = 0; k < 2; ++k) {
                const int rr = rs + 16 * k;
                const float *pg = sG + rr * LDH + 4 * c4;
                const float4 v = make_float4(pg[0], pg[1], pg[2], pg[3]);
                if (rr < nv) st4(dagg_out + (s * SM + rr) * DIN + 4 * c4, v);
            }
        }
        if (dims) zero_pad(s, nv);
        nv = next_nv;
    }
    SCGIB_MARK(5);
    if constexpr (!WG) return;
    // per-workgroup slab: dW2 | dW1 | db2 | db1 (gin_bwd_k layout)
    float *sl = slab + static_cast<int64_t>(blockIdx.x) * SLAB;
    float *dw = nw ? sl + 64 * 64 : sl;  // N: dW1 [64][DIN], T: dW2 [64][64]
    const int ld = nw ? DIN : 64;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int j = q * 32 + acc_row(reg, l);
        dw[j * ld + li] = accA[reg];
        dw[j * ld + 32 + li] = accB[reg];
    }
    dbias += __shfl_xor(dbias, 32, kWave);
    if (l < 32) sl[64 * 64 + 64 * DIN + (nw ? 64 : 0) + q * 32 + l] = dbias;
    SCGIB_MARK(6);
}

// ---------------------------------------------------------------------------
// The agg-free backward of a d_in = 64 GIN layer l >= 1.
// agg_l = (I + A) h_{l-1} is read by exactly one product of the layer's
// backward, dW1 = dz1^T agg.  A is symmetric (the reference's bidirected
// molecule graphs), so with g = (I + A)^T dz1 — the transposed gather the
// NEXT statistics kernel runs anyway, now over dz1 instead of d(agg):
//   dW1_l      = dz1^T (I + A) h_{l-1} = g^T h_{l-1}
//   d h_{l-1}  = (I + A)^T (dz1 W1) = g W1
// and h_{l-1} = relu(scale z2_{l-1} + shift) comes elementwise from the z2
// rows that kernel reads for layer l-1's BatchNorm backward.  So the forward
// stores no agg for these layers (256 B per row less of the 768 B it wrote,
// gin_fwd_k), gin_bwd5z_k runs two of gin_bwd5_k's four products (dr, dW2)
// and writes dz1 where gin_bwd5_k wrote d(agg), reading no agg; and
// gin_bwd_statsz_k gathers dz1 and adds the two products it moved (g W1 and
// g^T h, f32 MFMA), leaving dW1 as per-workgroup partials.  No flops are
// added, only moved; the sums associate differently, so results match the
// stored-agg path to rounding, not bitwise (ops.AGG_FREE selects the path).
// ---------------------------------------------------------------------------
constexpr int kZSlab = 64 * 64 + 128;  // gin_bwd5z_k slab: dW2 [64][64] | db2 | db1

// gin_bwd5z_k: gin_bwd5_k's sub-tile walk with its first product pair only —
//   waves 0,1 (N): dr block q = dz2 W2[:, 32q..] (K = 64), dz1 = dr [r > 0]
//                  -> dz1 staging (row-major) and db1 (column sums of dz1);
//   waves 2,3 (T): dW2 rows 32q.. += dz2^T r (two blocks, K = 32 rows) + db2
// — then the dz1 rows go out as full-row float4 stores: two barriers per
// sub-tile (gin_bwd5_k: three), no agg rows loaded, no W1.
// WG = false: a frozen layer (the fine-tune freezing quirk) — dz1 by the same
// dr chain, no dW2 / db products, no slab.
template <bool WG = true>
__global__ __launch_bounds__(256, 2) void gin_bwd5z_k(
    const float *__restrict__ dy, const float *__restrict__ z2, const float *__restrict__ r,
    const float *__restrict__ stat, const float *__restrict__ coef, const float *__restrict__ w2,
    int64_t ncap, int64_t nsub, int64_t G, float *__restrict__ dz1_out, float *__restrict__ slab,
    const int32_t *__restrict__ dims, scgib_bn_bwd_pending pend, scgib_slab_job fold,
    scgib_slab_job fold2) {
    static_assert(SM == 32, "32-row sub-tiles");
    __shared__ __attribute__((aligned(16))) float sD[SM * LDR];   // dz2 [row][k]
    __shared__ __attribute__((aligned(16))) float sDT[64 * LDT];  // dz2 [col][row]
    __shared__ __attribute__((aligned(16))) float sRT[64 * LDT];  // r [col][row]
    __shared__ float sE[SM * LDH];                                 // dz1 staging
    __shared__ float sCoef[128];
    if (static_cast<int64_t>(blockIdx.x) >= G) {  // block-uniform: a folded reduce block
        const int b = static_cast<int>(blockIdx.x - G), f1 = slab_fold8_blocks(fold);
        if (b < f1) slab_fold8_block(fold, b, sD);
        else slab_fold_block(fold2, b - f1, sD);
        return;
    }
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const int kk = l >> 5, li = l & 31;
    const bool nw = w < 2;  // wave-uniform role: N (dr, dz1, db1) or T (dW2, db2)
    const int q = w & 1;    // the role's 32-wide block
    const int c = l;        // elementwise: column c, rows 8 w .. 8 w + 7
    const int64_t last = ncap - 1;
    SCGIB_MARK(0);
    SCGIB_MARK_HWID();
    BwdFin bfin;
    const int pend_ngr = static_cast<int>(((n + TM - 1) / TM + kGroup - 1) / kGroup);
    if (pend.gpart) bn_bwd_fin_load<false>(pend.gpart, pend_ngr, 0, bfin);
    const float s_mean = stat[c], s_istd = stat[64 + c], s_sc = stat[128 + c];
    float c1 = 0.f, c2 = 0.f;
    if (!pend.gpart) {
        c1 = coef[c];
        c2 = coef[64 + c];
    }
    float wreg[32];  // N waves: W2[:, 32q..] (k in kperm order); T waves: unused
#pragma unroll
    for (int s = 0; s < 32; ++s) wreg[s] = nw ? w2[kperm(s, kk) * 64 + q * 32 + li] : 0.f;
    float nx[3][8];  // a sub-tile's column c, rows 8 w + i: [0] dy, [1] z2, [2] r
    auto load_sub = [&](int64_t s) {  // in order of use: r, then dy / z2
        load_col8(r, s, last, w, c, nx[2]);
        load_col8(dy, s, last, w, c, nx[0]);
        load_col8(z2, s, last, w, c, nx[1]);
    };
    int64_t s = blockIdx.x;
    int nv = s < nsub ? rows_of(n, s) : 0;
    if (nv > 0) load_sub(s);
    // finish the BN-backward sums (the barrier below, shared with the image)
    if (pend.gpart) bn_bwd_pending_finish(pend, pend_ngr, n, bfin, sCoef);
    if (nv > 0) put_col8(sRT, w, c, nx[2]);
    vm_wait_all();  // the weight registers complete before the loop (gin_bwd5_k)
    __syncthreads();
    if (pend.gpart) {
        c1 = sCoef[c];
        c2 = sCoef[64 + c];
    }
    const float k1 = s_istd * c2;  // dz2 = sc (dy - c1 - (z2 - mean) istd c2)
    SCGIB_MARK(1);
    f32x16 accA = zero16(), accB = zero16();  // T waves: dW2 blocks (q, 0), (q, 1)
    float dbias = 0.f;                         // N: db1 (column q*32 + li), T: db2
    for (int it = 0; s < nsub; s += G, ++it) {
        if (nv == 0) {  // capacity tail: this and every later sub-tile is padding
            for (int64_t t = s; t < nsub; t += G) zero_pad(dz1_out, ncap, t, rows_of(n, t));
            break;
        }
        // dz2 -> sD row-major and sDT transposed (also when frozen: as it was)
        stage_dz2<true>(nx[0], nx[1], s_sc, c1, s_mean, k1, nv, w, c, sD, sDT);
        const int64_t next = s + G;
        const int next_nv = next < nsub ? rows_of(n, next) : 0;  // block-uniform
        if (next_nv > 0) load_sub(next);  // in flight during the products
        lds_barrier();  // dz2 complete
        if (it == 0) SCGIB_MARK(2);
        if (nw) {  // dr block q, dz1 = dr [r > 0] (mask by multiplication) -> staging
            const f32x16 dr = mma_rk4<8>(sD + li * LDR + 4 * kk, wreg, zero16());
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) {
                const int row = acc_row(reg, l), col = q * 32 + li;
                const float v = dr[reg] * (sRT[col * LDT + row] > 0.f ? 1.f : 0.f);
                sE[row * LDH + col] = v;
                dbias += v;
            }
        } else if constexpr (WG) {   // dW2 rows 32q.. += dz2^T r (db2 from the A operand)
            mma_kk4x2<4>(sDT + (q * 32 + li) * LDT + 4 * kk, sRT + li * LDT + 4 * kk,
                         sRT + (32 + li) * LDT + 4 * kk, accA, accB, dbias);
        }
        lds_barrier();  // dz1 staged; r and dz2 consumed
        if (it == 0) SCGIB_MARK(3);
        if (next_nv > 0) put_col8(sRT, w, c, nx[2]);
        store_rows(sE, dz1_out, s, nv);  // dz1 rows
        if (dims) zero_pad(dz1_out, ncap, s, nv);
        nv = next_nv;
    }
    SCGIB_MARK(5);
    if constexpr (!WG) return;
    // per-workgroup slab: dW2 [64][64] | db2 [64] | db1 [64]
    float *sl = slab + static_cast<int64_t>(blockIdx.x) * kZSlab;
    if (!nw) {
#pragma unroll
        for (int reg = 0; reg < 16; ++reg) {
            const int j = q * 32 + acc_row(reg, l);
            sl[j * 64 + li] = accA[reg];
            sl[j * 64 + 32 + li] = accB[reg];
        }
    }
    put_dbias(dbias, l, sl, 64 * 64 + (nw ? 64 : 0) + q * 32);
    SCGIB_MARK(6);
}

// ---------------------------------------------------------------------------
// gin_bwd5r_k: gin_bwd5_k without the saved r.  The
// forward no longer writes r = relu(agg W1^T + b1) — one of the three [N,64]
// row sets gin_fwd_k stored, a third of its HBM writes — and this kernel
// recomputes it per sub-tile from the agg rows it stages anyway, with the
// forward's own MFMA chain (v_mfma_f32_32x32x2_f32, step s = k pair (2 s,
// 2 s + 1), s = 0..31 in order from zero, then + b1 and fmaxf 0), so every r
// element is bitwise the one the forward would have stored; every other
// product is one of gin_bwd5_k's chains unchanged (same operands, same order
// per output element), so dW1 / dW2 / db / d(agg) are bitwise gin_bwd5_k's
// (tests/test_gpu_parity.py::test_gin_r_recompute_bitwise).
// Roles, 80 MFMAs per wave and sub-tile (gin_bwd5_k: 64) in three phases:
//   1: waves 0,1: r block q = agg W1[32q.., :]^T + b1, relu -> r^T image
//                 (and the block's ReLU mask, 16 bits in one register)
//      waves 2,3: dr block q = dz2 W2[:, 32q..] -> the dz1^T image
//   2: waves 0,1: dz1 = dr [r > 0] (their own block) -> dz1 / dz1^T images
//      every wave: dW2 block (q, w >> 1) += dz2^T r (db2: waves 0,1)
//   3: waves 0,1: d(agg) block q = dz1 W1[:, 32q..] -> staging
//      waves 2,3: dW1 rows 32q.. += dz1^T agg (db1)
//   (+ the next sub-tile's dz2 staged during phase 3: three barriers)
// Registers: waves 0,1 hold W1 rows (r) and W1 columns (d(agg)), waves 2,3
// W2 columns (dr) and two dW1 accumulators — the second weight block and
// those accumulators are the same two f32x16.  LDS: gin_bwd5_k's images
// (r^T now written by phase 1) + the agg rows with each row's k split
// even | odd (lane half kk reads k = 2 s + kk, s = 0..31, as one run: b128
// operand reads) = 72 KB, two workgroups per CU.
// ---------------------------------------------------------------------------
constexpr int kEO = 32;  // even | odd split: k -> (k & 1) * 32 + (k >> 1)

template <int DIN>
__global__ __launch_bounds__(256, 2) void gin_bwd5r_k(
    const float *__restrict__ dy, const float *__restrict__ z2, const float *__restrict__ agg,
    const float *__restrict__ stat, const float *__restrict__ coef, const float *__restrict__ w1,
    const float *__restrict__ b1, const float *__restrict__ w2, int64_t ncap, int64_t nsub,
    float *__restrict__ dagg_out, float *__restrict__ slab, const int32_t *__restrict__ dims,
    scgib_bn_bwd_pending pend) {
    static_assert(DIN == 64 && SM == 32, "64-wide rows, 32-row sub-tiles");
    constexpr int SLAB = 64 * 64 + 64 * DIN + 128;
    __shared__ __attribute__((aligned(16))) float sD[SM * LDR];   // dz2 [row][k]
    __shared__ __attribute__((aligned(16))) float sDT[64 * LDT];  // dz2 [col][row]
    __shared__ __attribute__((aligned(16))) float sE[SM * LDR];   // dz1
    __shared__ __attribute__((aligned(16))) float sET[64 * LDT];
    __shared__ __attribute__((aligned(16))) float sRT[64 * LDT];  // r [col][row] (recomputed)
    __shared__ __attribute__((aligned(16))) float sAT[DIN * LDT]; // agg [col][row]
    __shared__ __attribute__((aligned(16))) float sAR[SM * LDR];  // agg [row][even | odd k]
    __shared__ float sG[SM * LDH];                                 // d(agg) staging
    __shared__ float sCoef[128];
    const int64_t n = eff_count(dims, 0, ncap);
    const int tid = threadIdx.x, l = tid & 63, w = tid >> 6;
    const int kk = l >> 5, li = l & 31;
    const bool ra = w < 2;  // wave-uniform role: r, d(agg) (waves 0,1) or dr, dW1 (2,3)
    const int q = w & 1;    // the role's 32-wide block
    const int c = l;        // elementwise: column c, rows 8 w .. 8 w + 7
    const int64_t last = ncap - 1;
    const int64_t G = gridDim.x;
    SCGIB_MARK(0);
    SCGIB_MARK_HWID();
    BwdFin bfin;
    const int pend_ngr = static_cast<int>(((n + TM - 1) / TM + kGroup - 1) / kGroup);
    if (pend.gpart) bn_bwd_fin_load<false>(pend.gpart, pend_ngr, 0, bfin);
    const float s_mean = stat[c], s_istd = stat[64 + c], s_sc = stat[128 + c];
    float c1 = 0.f, c2 = 0.f;
    if (!pend.gpart) {
        c1 = coef[c];
        c2 = coef[64 + c];
    }
    // wa: waves 0,1 W1[32q + li][2 s + kk] (r, the forward's k order);
    //     waves 2,3 W2[kperm(s, kk)][32q + li] (dr)
    // X0 | X1: waves 0,1 W1[kperm(s, kk)][32q + li] (d(agg));
    //          waves 2,3 the dW1 accumulators (q, 0) | (q, 1)
    float wa[32];
    f32x16 X0 = zero16(), X1 = zero16();
    float bias1 = 0.f;
    if (ra) {
#pragma unroll
        for (int s = 0; s < 32; ++s) wa[s] = w1[(q * 32 + li) * DIN + 2 * s + kk];
#pragma unroll
        for (int s = 0; s < 16; ++s) {
            X0[s] = w1[kperm(s, kk) * DIN + q * 32 + li];
            X1[s] = w1[kperm(s + 16, kk) * DIN + q * 32 + li];
        }
        bias1 = b1[q * 32 + li];
    } else {
#pragma unroll
        for (int s = 0; s < 32; ++s) wa[s] = w2[kperm(s, kk) * 64 + q * 32 + li];
    }
    // a sub-tile's column c, rows 8 w + i: [0] dy, [1] z2, [2] agg.  The next
    // sub-tile's agg rows are loaded a whole sub-tile ahead (its r^T / agg
    // images are written after this one's barriers 1 and 3), its dy / z2 only
    // after barrier 1 (staged in phase 3): fewer registers live across phase 1
    float nx[3][8];
    auto load_agg = [&](int64_t s) { load_col8(agg, s, last, w, c, nx[2]); };
    auto load_dz = [&](int64_t s) {
        load_col8(dy, s, last, w, c, nx[0]);
        load_col8(z2, s, last, w, c, nx[1]);
    };
    auto put_ar = [&]() {  // agg column c -> position (c & 1) * 32 + (c >> 1) of rows 8w..
        const int pos = (c & 1) * kEO + (c >> 1);
#pragma unroll
        for (int i = 0; i < 8; ++i) sAR[(8 * w + i) * LDR + pos] = nx[2][i];
    };
    int64_t s = blockIdx.x;
    int nv = s < nsub ? rows_of(n, s) : 0;
    if (nv > 0) {
        load_agg(s);
        load_dz(s);
    }
    if (pend.gpart) {  // finish the BN-backward sums (a barrier of its own: dz2 is staged below)
        bn_bwd_pending_finish(pend, pend_ngr, n, bfin, sCoef);
        __syncthreads();
        c1 = sCoef[c];
        c2 = sCoef[64 + c];
    }
    const float k1 = s_istd * c2;
    if (nv > 0) {
        put_col8(sAT, w, c, nx[2]);
        put_ar();
        stage_dz2<true>(nx[0], nx[1], s_sc, c1, s_mean, k1, nv, w, c, sD, sDT);
    }
    // the weight registers complete here (see gin_bwd5_k)
    vm_wait_all();
    __syncthreads();
    // the second sub-tile's agg rows: in flight during the first one's phase 1
    if (nv > 0 && s + G < nsub && rows_of(n, s + G) > 0) load_agg(s + G);
    SCGIB_MARK(1);
    f32x16 acc0 = zero16();  // waves 0,1: dW2 block (q, 0); waves 2,3: dW2 block (q, 1)
    float dbias = 0.f;       // waves 0,1: db2 [32q + li]; waves 2,3: db1
    for (int it = 0; s < nsub; s += G, ++it) {
        if (nv == 0) {  // capacity tail: this and every later sub-tile is padding
            for (int64_t t = s; t < nsub; t += G) zero_pad(dagg_out, ncap, t, rows_of(n, t));
            break;
        }
        const int64_t next = s + G;
        const int next_nv = next < nsub ? rows_of(n, next) : 0;  // block-uniform
        // the element (row 8 g + 4 kk + t, column 32 q + li) of block q sits in
        // register 4 g + t of every role: one b128 per g in the [col][row] images
        const int col = q * 32 + li;
        unsigned rmask = 0u;  // waves 0,1: bit 4 g + t = [r > 0] of their r block
        if (ra) {  // phase 1: r block q (the forward's chain), relu -> sRT as [col][row]
            const f32x16 z = mma_rk4<8, 4>(sAR + li * LDR + kk * kEO, wa, zero16());
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float v[4];
#pragma unroll
                for (int t = 0; t < 4; ++t) {
                    v[t] = fmaxf(z[4 * g + t] + bias1, 0.f);
                    rmask |= (v[t] > 0.f ? 1u : 0u) << (4 * g + t);
                }
                *reinterpret_cast<float4 *>(sRT + col * LDT + 8 * g + 4 * kk) = make_float4(v[0], v[1], v[2], v[3]);
            }
        } else {   // phase 1: dr block q -> sET [col][row] (masked in phase 2 by waves 0,1)
            const f32x16 dr = mma_rk4<8>(sD + li * LDR + 4 * kk, wa, zero16());
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *reinterpret_cast<float4 *>(sET + col * LDT + 8 * g + 4 * kk) =
                    make_float4(dr[4 * g], dr[4 * g + 1], dr[4 * g + 2], dr[4 * g + 3]);
        }
        lds_barrier();  // r^T and dr complete; the agg rows consumed
        if (it == 0) SCGIB_MARK(2);
        if (next_nv > 0) {
            put_ar();
            load_dz(next);  // staged in phase 3
        }
        if (ra) {  // phase 2: dz1 = dr [r > 0] -> sE, sET in place (mask by multiplication)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 *pt = reinterpret_cast<float4 *>(sET + col * LDT + 8 * g + 4 * kk);
                const float4 d = *pt;
                const float4 v = make_float4(d.x * ((rmask >> (4 * g)) & 1u ? 1.f : 0.f),
                                             d.y * ((rmask >> (4 * g + 1)) & 1u ? 1.f : 0.f),
                                             d.z * ((rmask >> (4 * g + 2)) & 1u ? 1.f : 0.f),
                                             d.w * ((rmask >> (4 * g + 3)) & 1u ? 1.f : 0.f));
                const int row = 8 * g + 4 * kk;
                sE[row * LDR + col] = v.x;
                sE[(row + 1) * LDR + col] = v.y;
                sE[(row + 2) * LDR + col] = v.z;
                sE[(row + 3) * LDR + col] = v.w;
                *pt = v;
            }
        }
        // phase 2: dW2 rows 32q.., columns 32 (w >> 1).. += dz2^T r (db2 on waves 0,1)
        if (ra)
            mma_kk4<4, true>(sDT + (q * 32 + li) * LDT + 4 * kk, sRT + li * LDT + 4 * kk, acc0, dbias);
        else
            mma_kk4<4, false>(sDT + (q * 32 + li) * LDT + 4 * kk, sRT + (32 + li) * LDT + 4 * kk, acc0, dbias);
        lds_barrier();  // dz1 complete; dz2 and r consumed
        if (it == 0) SCGIB_MARK(3);
        if (ra) {  // phase 3: d(agg) block q = dz1 W1[:, 32q..] -> staging
            const f32x16 da = mma_rk4<8>(sE + li * LDR + 4 * kk, W32{X0, X1}, zero16());
#pragma unroll
            for (int reg = 0; reg < 16; ++reg) sG[acc_row(reg, l) * LDH + q * 32 + li] = da[reg];
        } else {   // phase 3: dW1 rows 32q.. += dz1^T agg (db1 from the A operand)
            mma_kk4x2<4>(sET + (q * 32 + li) * LDT + 4 * kk, sAT + li * LDT + 4 * kk,
                         sAT + (32 + li) * LDT + 4 * kk, X0, X1, dbias);
        }
        // the next dz2: sD and sDT are free since the barrier
        if (next_nv > 0) stage_dz2<true>(nx[0], nx[1], s_sc, c1, s_mean, k1, next_nv, w, c, sD, sDT);
        lds_barrier();  // d(agg) staged, next dz2 staged; agg^T and dz1 consumed
        if (it == 0) SCGIB_MARK(4);
        if (next_nv > 0) {
            put_col8(sAT, w, c, nx[2]);
            const int64_t nn = next + G;  // the sub-tile after: in flight during the next one
            if (nn < nsub && rows_of(n, nn) > 0) load_agg(nn);
        }
        store_rows(sG, dagg_out, s, nv);  // d(agg) rows (after the loads: in-order vmcnt)
        if (dims) zero_pad(dagg_out, ncap, s, nv);
        nv = next_nv;
    }
    SCGIB_MARK(5);
    // per-workgroup slab: dW2 | dW1 | db2 | db1 (gin_bwd_k layout)
    float *sl = slab + static_cast<int64_t>(blockIdx.x) * SLAB;
#pragma unroll
    for (int reg = 0; reg < 16; ++reg) {
        const int j = q * 32 + acc_row(reg, l);
        sl[j * 64 + (ra ? 0 : 32) + li] = acc0[reg];
        if (!ra) {
            sl[64 * 64 + j * DIN + li] = X0[reg];
            sl[64 * 64 + j * DIN + 32 + li] = X1[reg];
        }
    }
    put_dbias(dbias, l, sl, 64 * 64 + 64 * DIN + (ra ? 0 : 64) + q * 32);
    SCGIB_MARK(6);
}

}  // namespace scgib
