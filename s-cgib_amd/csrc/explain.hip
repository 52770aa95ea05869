// Reading what the model learned: per-molecule attention
// softmax and ranks of the preservation gate / attention weight, the graph
// core as an induced subgraph (dgl.node_subgraph), and the dataset-wide store.
//
//   explain_rank_k        one wavefront per molecule: alpha = softmax(logit),
//                         lam_rank / alpha_rank, centres / weights [B, top_m]
//   explain_mask_k        one wavefront per molecule: the kept flag per atom
//   explain_count_k       per row: kept flag + kept-neighbour count, block scan
//   explain_scan_fixup_k  cross-block prefix (64-bit), totals, overflow bit
//   explain_fill_k        rows, relabelled columns, _ID, graph_ptr of the core
//   explain_store_k       one wavefront per molecule: rows to node_off[id]
//
// Integer and VALU work only.  No atomics anywhere: every output element has
// one writer and every reduction a fixed lane and row order, so all results
// are bitwise reproducible.
#include "common.h"

namespace scgib {
namespace {

// rows of a molecule whose two keys are staged in LDS; rows beyond are read
// from global memory (the same values: lam as given, alpha as just written)
constexpr int kStage = 512;

enum : int32_t { kErrCoreOverflow = 1 };

// u precedes v: descending key, ties by ascending id; keys compare as floats
// (-0.0 ties with +0.0); NaN after every number, NaNs among themselves by id
__device__ __forceinline__ int before(float ku, int u, float kv, int v) {
    const bool nu = ku != ku, nv = kv != kv;
    const bool b = nv ? (!nu || u < v) : (ku > kv || (ku == kv && u < v));
    return b ? 1 : 0;
}

// rank of row i (key kv) among the n rows of the molecule at r0
__device__ __forceinline__ int rank_of(const float *__restrict__ sk, const float *gk, int64_t r0,
                                       int n, float kv, int i) {
    const int ns = n < kStage ? n : kStage;
    int cnt = 0;
    for (int u = 0; u < ns; ++u) cnt += before(sk[u], u, kv, i);  // LDS broadcast reads
    for (int u = ns; u < n; ++u) cnt += before(gk[r0 + u], u, kv, i);
    return cnt;
}

__global__ __launch_bounds__(kWave) void explain_rank_k(
    const float *__restrict__ lam, const float *__restrict__ logit,
    const int32_t *__restrict__ gptr, int64_t B, int top_m, float *alpha,
    int32_t *__restrict__ lam_rank, int32_t *__restrict__ alpha_rank,
    int32_t *__restrict__ centres, float *__restrict__ weights, int64_t n_rows_cap) {
    __shared__ float sL[kStage], sA[kStage];
    const int lane = threadIdx.x;
    const int64_t gi = blockIdx.x;
    const bool att = logit != nullptr;
    if (gi >= B) {  // padding blocks: rows [N, n_rows_cap) get alpha 0 and ranks -1
        const int64_t step = static_cast<int64_t>(gridDim.x - B) * kWave;
        for (int64_t r = gptr[B] + (gi - B) * kWave + lane; r < n_rows_cap; r += step) {
            lam_rank[r] = -1;
            if (att) {
                alpha[r] = 0.f;
                alpha_rank[r] = -1;
            }
        }
        return;
    }
    const int64_t r0 = gptr[gi], r1 = gptr[gi + 1];
    const int n = r1 > r0 ? static_cast<int>(r1 - r0) : 0;
    const int rounds = (n + kWave - 1) / kWave;  // wave-uniform: every lane runs every round
    for (int j = 0; j < rounds; ++j) {
        const int i = lane + kWave * j;
        if (i < n && i < kStage) sL[i] = lam[r0 + i];
    }
    if (att) {  // (kernel-uniform) softmax: max, then sum, then normalise, fp32
        float M = -INFINITY;
        for (int j = 0; j < rounds; ++j) {
            const int i = lane + kWave * j;
            const bool ok = i < n;
            const float l = logit[r0 + (ok ? i : 0)];
            M = fmaxf(M, ok ? l : -INFINITY);
        }
        M = wave_max(M);  // all 64 lanes, rows past the end masked above
        float S = 0.f;
        for (int j = 0; j < rounds; ++j) {  // per lane in row order, then the fixed butterfly
            const int i = lane + kWave * j;
            const bool ok = i < n;
            const float l = logit[r0 + (ok ? i : 0)];
            S += ok ? expf(l - M) : 0.f;
        }
        S = wave_sum(S);
        for (int j = 0; j < rounds; ++j) {
            const int i = lane + kWave * j;
            const bool ok = i < n;
            const float a = expf(logit[r0 + (ok ? i : 0)] - M) / S;
            if (ok) {
                alpha[r0 + i] = a;
                if (i < kStage) sA[i] = a;
            }
        }
    }
    __syncthreads();  // LDS keys, and this wave's alpha rows past the staged ones
    for (int j = 0; j < rounds; ++j) {
        const int i = lane + kWave * j;
        const bool ok = i < n;
        const int ic = ok ? i : 0;
        const float kv = ic < kStage ? sL[ic] : lam[r0 + ic];
        const int rk = rank_of(sL, lam, r0, n, kv, ic);
        if (ok) lam_rank[r0 + i] = rk;
    }
    if (!att) return;
    for (int j = 0; j < rounds; ++j) {
        const int i = lane + kWave * j;
        const bool ok = i < n;
        const int ic = ok ? i : 0;
        const float kv = ic < kStage ? sA[ic] : alpha[r0 + ic];
        const int rk = rank_of(sA, alpha, r0, n, kv, ic);
        if (ok) {
            alpha_rank[r0 + i] = rk;
            if (rk < top_m) {  // ranks are a permutation of [0, n): one writer per slot
                centres[gi * top_m + rk] = static_cast<int32_t>(r0 + i);
                weights[gi * top_m + rk] = kv;
            }
        }
    }
    for (int t = n + lane; t < top_m; t += kWave) {  // entries past n_i
        centres[gi * top_m + t] = -1;
        weights[gi * top_m + t] = 0.f;
    }
}

// rule 0: lam_rank < m_i, m_i = max(1, ceil(n_i * ratio)) in IEEE double;
// rule 1: lam >= threshold (NaN never kept)
__global__ __launch_bounds__(kWave) void explain_mask_k(
    const float *__restrict__ lam, const int32_t *__restrict__ lam_rank,
    const int32_t *__restrict__ gptr, int64_t B, int rule, double ratio, float threshold,
    uint8_t *__restrict__ mask, int64_t n_rows_cap) {
    const int lane = threadIdx.x;
    const int64_t gi = blockIdx.x;
    if (gi >= B) {
        const int64_t step = static_cast<int64_t>(gridDim.x - B) * kWave;
        for (int64_t r = gptr[B] + (gi - B) * kWave + lane; r < n_rows_cap; r += step) mask[r] = 0;
        return;
    }
    const int64_t r0 = gptr[gi], r1 = gptr[gi + 1];
    double m = ceil(static_cast<double>(r1 - r0) * ratio);
    m = m < 1.0 ? 1.0 : m;
    for (int64_t r = r0 + lane; r < r1; r += kWave) {
        const bool keep = rule == 0 ? static_cast<double>(lam_rank[r]) < m : lam[r] >= threshold;
        mask[r] = keep ? 1 : 0;
    }
}

// Per row: kept flag and number of kept in-row neighbours; block-inclusive
// scan into nptr / eptr [v + 1] and the block totals (the ego builder's idiom).
__global__ __launch_bounds__(256) void explain_count_k(
    const uint8_t *__restrict__ mask, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, int64_t n, int32_t *__restrict__ nptr,
    int32_t *__restrict__ eptr, int32_t *__restrict__ blk_tot, const int32_t *__restrict__ dims) {
    __shared__ int32_t sn[256], se[256];
    const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    int32_t nb = 0, ne = 0;
    if (v < n && v < eff_count(dims, 0, n) && mask[v]) {
        nb = 1;
        const int32_t e1 = rowptr[v + 1];
        for (int32_t j = rowptr[v]; j < e1; ++j) {
            const int32_t u = col[j];
            if (u >= 0 && u < n && mask[u]) ++ne;
        }
    }
    sn[threadIdx.x] = nb;
    se[threadIdx.x] = ne;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        int32_t an = 0, ae = 0;
        if (threadIdx.x >= off) {
            an = sn[threadIdx.x - off];
            ae = se[threadIdx.x - off];
        }
        __syncthreads();
        sn[threadIdx.x] += an;
        se[threadIdx.x] += ae;
        __syncthreads();
    }
    if (v < n) {
        nptr[v + 1] = sn[threadIdx.x];
        eptr[v + 1] = se[threadIdx.x];
    }
    if (threadIdx.x == 255) {
        blk_tot[blockIdx.x] = sn[255];
        blk_tot[gridDim.x + blockIdx.x] = se[255];
    }
}

// Adds the exclusive prefix of the block totals, summed in 64 bits in a fixed
// order by each block itself; the last block leaves the totals in core_dims
// and sets the error bit where one does not fit int32 (instead of wrapping).
__global__ __launch_bounds__(256) void explain_scan_fixup_k(
    int64_t n, int32_t nblk, const int32_t *__restrict__ blk_tot, int32_t *__restrict__ nptr,
    int32_t *__restrict__ eptr, int32_t *__restrict__ core_dims, int32_t *__restrict__ err) {
    __shared__ int64_t rn[256], re[256];
    int64_t an = 0, ae = 0;
    for (int32_t j = threadIdx.x; j < static_cast<int32_t>(blockIdx.x); j += 256) {
        an += blk_tot[j];
        ae += blk_tot[nblk + j];
    }
    rn[threadIdx.x] = an;
    re[threadIdx.x] = ae;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (threadIdx.x < off) {
            rn[threadIdx.x] += rn[threadIdx.x + off];
            re[threadIdx.x] += re[threadIdx.x + off];
        }
        __syncthreads();
    }
    const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (v < n) {
        nptr[v + 1] = static_cast<int32_t>(nptr[v + 1] + rn[0]);
        eptr[v + 1] = static_cast<int32_t>(eptr[v + 1] + re[0]);
    }
    if (v == 0) {
        nptr[0] = 0;
        eptr[0] = 0;
    }
    if (static_cast<int32_t>(blockIdx.x) == nblk - 1 && threadIdx.x == 0) {
        const int64_t tn = rn[0] + blk_tot[nblk - 1], te = re[0] + blk_tot[2 * nblk - 1];
        const bool over = tn > INT32_MAX || te > INT32_MAX;
        core_dims[0] = over ? 0 : static_cast<int32_t>(tn);
        core_dims[1] = over ? 0 : static_cast<int32_t>(te);
        if (over) *err = *err | kErrCoreOverflow;  // (one writer)
    }
}

// Edges stay inside their molecule and batch order is kept, so the new id of
// a kept atom is the batch-wide exclusive prefix nptr[v]; graph_ptr_out[g] is
// that prefix at graph_ptr[g].  Rows / ids past the core's sizes: empty rows
// and id 0, as the ego builder leaves its tail.
__global__ __launch_bounds__(256) void explain_fill_k(
    const uint8_t *__restrict__ mask, const int32_t *__restrict__ rowptr,
    const int32_t *__restrict__ col, const int32_t *__restrict__ gptr, int64_t B, int64_t n,
    const int32_t *__restrict__ nptr, const int32_t *__restrict__ eptr,
    const int32_t *__restrict__ core_dims, int32_t *__restrict__ out_rowptr,
    int32_t *__restrict__ out_col, int32_t *__restrict__ out_id, int32_t *__restrict__ gptr_out,
    int64_t n_out_cap, int64_t e_out_cap, const int32_t *__restrict__ dims) {
    const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    const int64_t ns = core_dims[0], es = core_dims[1];
    for (int64_t i = ns + v; i <= n_out_cap; i += stride) {
        out_rowptr[i] = static_cast<int32_t>(es);
        if (i < n_out_cap && out_id) out_id[i] = 0;
    }
    if (gptr_out) {
        for (int64_t g = v; g <= B; g += stride) {
            const int64_t r = gptr[g];
            gptr_out[g] = nptr[r < 0 ? 0 : (r > n ? n : r)];
        }
    }
    if (v >= n || v >= eff_count(dims, 0, n) || !mask[v]) return;
    const int64_t nid = nptr[v];
    if (nid >= n_out_cap) return;
    int64_t eo = eptr[v];
    out_rowptr[nid] = static_cast<int32_t>(eo);
    if (out_id) out_id[nid] = static_cast<int32_t>(v);
    const int32_t e1 = rowptr[v + 1];
    for (int32_t j = rowptr[v]; j < e1; ++j) {
        const int32_t u = col[j];
        if (u >= 0 && u < n && mask[u]) {
            if (eo < e_out_cap) out_col[eo] = nptr[u];
            ++eo;
        }
    }
}

// One wavefront per molecule of the batch: its rows go to node_off[id] of the
// dataset-wide arrays.  Fill molecules (id -1) and ids outside the dataset
// write nothing; a pass holds each molecule once, so no two blocks share a row.
__global__ __launch_bounds__(kWave) void explain_store_k(
    const float *__restrict__ lam, const float *__restrict__ alpha,
    const int32_t *__restrict__ lam_rank, const int32_t *__restrict__ alpha_rank,
    const int32_t *__restrict__ gptr, const int32_t *__restrict__ ids,
    const int64_t *__restrict__ node_off, int64_t n_mol, int64_t total, float *__restrict__ ds_lam,
    float *__restrict__ ds_alpha, int32_t *__restrict__ ds_lam_rank,
    int32_t *__restrict__ ds_alpha_rank) {
    const int64_t gi = blockIdx.x;
    const int64_t id = ids[gi];
    if (id < 0 || id >= n_mol) return;
    const int64_t r0 = gptr[gi], d0 = node_off[id];
    int64_t n = gptr[gi + 1] - r0;
    const int64_t nd = node_off[id + 1] - d0;
    n = n < nd ? n : nd;  // (equal for a batch collated from this dataset)
    if (d0 < 0 || n > total - d0) return;  // never past the dataset arrays
    for (int64_t i = threadIdx.x; i < n; i += kWave) {
        ds_lam[d0 + i] = lam[r0 + i];
        ds_lam_rank[d0 + i] = lam_rank[r0 + i];
        if (alpha) {
            ds_alpha[d0 + i] = alpha[r0 + i];
            ds_alpha_rank[d0 + i] = alpha_rank[r0 + i];
        }
    }
}

constexpr int kPadBlocks = 8;  // capacity mode: workgroups that define the rows past dims[0]

}  // namespace
}  // namespace scgib

using namespace scgib;

extern "C" int64_t scgib_explain_stage_rows(void) { return kStage; }

extern "C" int scgib_explain_rank(const float *lam, const float *logit, const int32_t *graph_ptr,
                                  int64_t n_graphs, int64_t n_rows, int32_t top_m, float *alpha,
                                  int32_t *lam_rank, int32_t *alpha_rank, int32_t *centres,
                                  float *weights, int32_t pad, scgib_stream_t stream) {
    if (n_graphs < 0 || n_rows < 0 || top_m < 0) return SCGIB_EINVAL;
    if (n_graphs >= (int64_t(1) << 31) - kPadBlocks || n_rows >= (int64_t(1) << 31))
        return SCGIB_EUNSUPPORTED;
    if (!graph_ptr || (n_rows > 0 && (!lam || !lam_rank))) return SCGIB_EINVAL;
    if (logit && (!alpha || !alpha_rank)) return SCGIB_EINVAL;
    if (top_m > 0 && (!logit || !centres || !weights)) return SCGIB_EINVAL;
    const int64_t grid = n_graphs + (pad ? kPadBlocks : 0);
    if (grid == 0) return SCGIB_OK;
    explain_rank_k<<<static_cast<unsigned>(grid), kWave, 0, as_stream(stream)>>>(
        lam, logit, graph_ptr, n_graphs, top_m, alpha, lam_rank, alpha_rank, centres, weights,
        n_rows);
    return launch_status();
}

extern "C" int scgib_explain_core_mask(const float *lam, const int32_t *lam_rank,
                                       const int32_t *graph_ptr, int64_t n_graphs, int64_t n_rows,
                                       int32_t rule, double ratio, float threshold, uint8_t *mask,
                                       int32_t pad, scgib_stream_t stream) {
    if (n_graphs < 0 || n_rows < 0 || (rule != 0 && rule != 1)) return SCGIB_EINVAL;
    if (rule == 0 && !(ratio > 0.0 && ratio <= 1.0)) return SCGIB_EINVAL;
    if (n_graphs >= (int64_t(1) << 31) - kPadBlocks || n_rows >= (int64_t(1) << 31))
        return SCGIB_EUNSUPPORTED;
    if (!graph_ptr || (n_rows > 0 && (!mask || (rule == 0 ? !lam_rank : !lam)))) return SCGIB_EINVAL;
    const int64_t grid = n_graphs + (pad ? kPadBlocks : 0);
    if (grid == 0) return SCGIB_OK;
    explain_mask_k<<<static_cast<unsigned>(grid), kWave, 0, as_stream(stream)>>>(
        lam, lam_rank, graph_ptr, n_graphs, rule, ratio, threshold, mask, n_rows);
    return launch_status();
}

extern "C" int64_t scgib_explain_core_ws_words(int64_t n_rows) {
    const int64_t n = n_rows > 0 ? n_rows : 0, nblk = (n + 255) / 256;
    return 2 * (n + 1) + 2 * (nblk > 0 ? nblk : 1);
}

// ws layout: nptr [n + 1] | eptr [n + 1] | block totals [2 nblk]
extern "C" int scgib_explain_core_count(const uint8_t *mask, const int32_t *rowptr,
                                        const int32_t *col, int64_t n_rows, int32_t *ws,
                                        int32_t *core_dims, int32_t *err, const int32_t *dims,
                                        scgib_stream_t stream) {
    if (n_rows < 0 || !ws || !core_dims || !err) return SCGIB_EINVAL;
    if (n_rows >= (int64_t(1) << 31)) return SCGIB_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    if (n_rows == 0) {
        hipError_t e = hipMemsetAsync(ws, 0, 2 * sizeof(int32_t), st);
        if (e == hipSuccess) e = hipMemsetAsync(core_dims, 0, 2 * sizeof(int32_t), st);
        return e == hipSuccess ? SCGIB_OK : static_cast<int>(e);
    }
    if (!mask || !rowptr || !col) return SCGIB_EINVAL;
    const int32_t nblk = static_cast<int32_t>((n_rows + 255) / 256);
    int32_t *nptr = ws, *eptr = ws + n_rows + 1, *blk_tot = ws + 2 * (n_rows + 1);
    explain_count_k<<<nblk, 256, 0, st>>>(mask, rowptr, col, n_rows, nptr, eptr, blk_tot, dims);
    explain_scan_fixup_k<<<nblk, 256, 0, st>>>(n_rows, nblk, blk_tot, nptr, eptr, core_dims, err);
    return launch_status();
}

extern "C" int scgib_explain_core_fill(const uint8_t *mask, const int32_t *rowptr,
                                       const int32_t *col, const int32_t *graph_ptr,
                                       int64_t n_graphs, int64_t n_rows, const int32_t *ws,
                                       const int32_t *core_dims, int32_t *out_rowptr,
                                       int32_t *out_col, int32_t *out_id, int32_t *graph_ptr_out,
                                       int64_t n_out_cap, int64_t e_out_cap, const int32_t *dims,
                                       scgib_stream_t stream) {
    if (n_rows < 0 || n_graphs < 0 || n_out_cap < 0 || e_out_cap < 0) return SCGIB_EINVAL;
    if (n_rows >= (int64_t(1) << 31) || n_out_cap >= (int64_t(1) << 31)) return SCGIB_EUNSUPPORTED;
    if (!ws || !core_dims || !out_rowptr || (e_out_cap > 0 && !out_col)) return SCGIB_EINVAL;
    if (graph_ptr_out && !graph_ptr) return SCGIB_EINVAL;
    if (n_rows > 0 && (!mask || !rowptr || !col)) return SCGIB_EINVAL;
    const int64_t span = n_rows > 0 ? n_rows : 1;
    const int32_t nblk = static_cast<int32_t>((span + 255) / 256);
    const int32_t *nptr = ws, *eptr = ws + n_rows + 1;
    explain_fill_k<<<nblk, 256, 0, as_stream(stream)>>>(
        mask, rowptr, col, graph_ptr, n_graphs, n_rows, nptr, eptr, core_dims, out_rowptr, out_col,
        out_id, graph_ptr_out, n_out_cap, e_out_cap, dims);
    return launch_status();
}

extern "C" int scgib_explain_store(const float *lam, const float *alpha, const int32_t *lam_rank,
                                   const int32_t *alpha_rank, const int32_t *graph_ptr,
                                   int64_t n_graphs, const int32_t *ids, const int64_t *node_off,
                                   int64_t n_molecules, int64_t total_nodes, float *ds_lam,
                                   float *ds_alpha,
                                   int32_t *ds_lam_rank, int32_t *ds_alpha_rank,
                                   scgib_stream_t stream) {
    if (n_graphs < 0 || n_molecules < 0 || total_nodes < 0) return SCGIB_EINVAL;
    if (n_graphs >= (int64_t(1) << 31)) return SCGIB_EUNSUPPORTED;
    if (n_graphs == 0) return SCGIB_OK;
    if (!lam || !lam_rank || !graph_ptr || !ids || !node_off || !ds_lam || !ds_lam_rank)
        return SCGIB_EINVAL;
    if (alpha && (!alpha_rank || !ds_alpha || !ds_alpha_rank)) return SCGIB_EINVAL;
    explain_store_k<<<static_cast<unsigned>(n_graphs), kWave, 0, as_stream(stream)>>>(
        lam, alpha, lam_rank, alpha_rank, graph_ptr, ids, node_off, n_molecules, total_nodes, ds_lam,
        ds_alpha,
        ds_lam_rank, ds_alpha_rank);
    return launch_status();
}
