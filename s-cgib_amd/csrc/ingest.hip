// Device-side COO -> CSR ingest of molecule batches (graph.from_coo,
// graph.StaticBatch.ingest).
//
// Every edge stays inside a molecule of at most 512 atoms, so the neighbour
// set of row v is a bitmap of W = ceil(max_graph_nodes / 32) words relative
// to the first node of v's molecule.  Three launches, integer work only:
//
//   ingest_mark_k   over the edges: both indices range-checked against
//                   [0, n), the owner molecule found by binary search in
//                   graph_ptr, both ends checked to share it and the molecule
//                   to fit the bitmap; then atomicOr of bit (row d, col s)
//                   and, under bidirect, (row s, col d).  Integer OR commutes:
//                   the bitmaps do not depend on the order the atomics land in.
//   ingest_count_k  over the rows: popcount -> in-degree, self-loop bit,
//                   verify mode's mirrored-bit test, the skip rule, the k = 1
//                   ego bounds; block-inclusive scan of the degrees (the
//                   egonet_count_k idiom) and one record of partials per
//                   block; graph_ptr validated over the molecules.
//   ingest_fill_k   over the rows: every block reduces the block records
//                   itself in a fixed order (the egonet_scan_fixup_k idiom:
//                   no second scan launch) into the totals, its own row
//                   offset and the verdict; enumerates each row's set bits
//                   ascending into col; clears the bitmap words it read, on
//                   the error path as well, so the zero-initialised workspace
//                   resets itself; block 0 writes the status record.
//
// Capacity form: the same kernels write a StaticBatch blob (tails included,
// byte for byte what StaticBatch.pad uploads) when the batch fits, and leave
// every byte of it otherwise.  The actual sizes may come from a device
// `counts` = (n, E_raw), so the launches are capturable over staging buffers.
//
// Bounds: no value read from a caller's tensor is used as an index before it
// is checked.  A bitmap word is addressed as row * W + (local >> 5) with
// 0 <= row < n <= rows_cap and 0 <= local < molecule size <= 32 * W; col is
// written at positions below the total popcount, which the verdict compares
// with col's capacity before any store.  Index arithmetic is 64-bit.
#include <algorithm>

#include "common.h"

namespace scgib {

constexpr int kIngestMaxGraphNodes = 512;
constexpr int kPartWords = 8;    // int64 per block record
constexpr int kStatusWords = 16; // int32 status record; graph_ptr copy follows

struct IngestArgs {
    const void *src, *dst;
    const int32_t *gptr;
    const int32_t *counts;  // device (n, E_raw) or nullptr
    const float *x;         // capacity form: [n][F]
    uint32_t *bm;           // [rows_cap][W], zero between calls
    int32_t *pre;           // [rows_cap] in-block inclusive degree prefix
    int64_t *part;          // [nblk][kPartWords]
    uint32_t *head;         // [0]: error bits of the mark launch
    int32_t *status;        // [kStatusWords + B + 1] or nullptr
    int32_t *sticky;        // sticky error word or nullptr
    int32_t *rowptr, *col, *gptr_out, *dims_out;
    float *x_out;
    int64_t e_raw_cap, n_host, rows_cap, col_cap, e_cap, ego_n_cap, ego_e_cap;
    int32_t B, F, W, mgn, dmax_cap, bidirect, skip_rule, blob, nblk;
};

// Actual (n, E_raw) and the size errors: a count outside its buffer is a
// capacity error and is replaced by 0, so nothing is indexed with it.
__device__ __forceinline__ int ingest_sizes(const IngestArgs &a, int64_t &n, int64_t &er) {
    n = a.counts ? static_cast<int64_t>(a.counts[0]) : a.n_host;
    er = a.counts ? static_cast<int64_t>(a.counts[1]) : a.e_raw_cap;
    int err = 0;
    if (n < 0 || n > a.rows_cap) {
        err |= SCGIB_INGEST_ECAPACITY;
        n = 0;
    }
    if (er < 0 || er > a.e_raw_cap) {
        err |= SCGIB_INGEST_ECAPACITY;
        er = 0;
    }
    return err;
}

// largest m in [0, B) with ptr[m] <= v (B >= 1); memory-safe for any ptr contents
__device__ __forceinline__ int ingest_owner(const int32_t *ptr, int B, int64_t v) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

template <class T>
__global__ __launch_bounds__(256) void ingest_mark_k(IngestArgs a) {
    int64_t n, er;
    int err = ingest_sizes(a, n, er);
    const T *src = static_cast<const T *>(a.src), *dst = static_cast<const T *>(a.dst);
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    if (!err) {
        for (int64_t i = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x; i < er; i += stride) {
            const int64_t s = static_cast<int64_t>(src[i]), d = static_cast<int64_t>(dst[i]);
            if (s < 0 || s >= n || d < 0 || d >= n) {
                err |= SCGIB_INGEST_ERANGE;
                continue;
            }
            const int g = ingest_owner(a.gptr, a.B, d);
            const int64_t base = a.gptr[g], ng = static_cast<int64_t>(a.gptr[g + 1]) - base;
            const int64_t ls = s - base, ld = d - base;
            if (ls < 0 || ls >= ng || ld < 0 || ld >= ng) {
                err |= SCGIB_INGEST_ERANGE;
                continue;
            }
            if (ng > kIngestMaxGraphNodes) {
                err |= SCGIB_INGEST_EGRAPH;
                continue;
            }
            if (ng > 32 * static_cast<int64_t>(a.W)) {
                err |= SCGIB_INGEST_ECAPACITY;
                continue;
            }
            atomicOr(a.bm + d * a.W + (ls >> 5), 1u << (ls & 31));
            if (a.bidirect) atomicOr(a.bm + s * a.W + (ld >> 5), 1u << (ld & 31));
        }
    }
    if (err) atomicOr(a.head, static_cast<uint32_t>(err));
}

__device__ __forceinline__ unsigned long long ingest_wave_sum(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
__device__ __forceinline__ int ingest_wave_max(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v = max(v, __shfl_xor(v, off, kWave));
    return v;
}
__device__ __forceinline__ int ingest_wave_or(int v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v |= __shfl_xor(v, off, kWave);
    return v;
}

// What a block reduces: sums, maxima (minimum as the maximum of the negated
// value) and error bits.  Integer: any order gives the same bits.
struct IngestAcc {
    unsigned long long deg, ego_n, ego_e, pre;
    int dmax, neg_min_mol, max_mol, err;
};

__device__ __forceinline__ IngestAcc ingest_block_reduce(IngestAcc v) {
    __shared__ unsigned long long s_u[4][4];
    __shared__ int s_i[4][4];
    const int lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
    v.deg = ingest_wave_sum(v.deg);
    v.ego_n = ingest_wave_sum(v.ego_n);
    v.ego_e = ingest_wave_sum(v.ego_e);
    v.pre = ingest_wave_sum(v.pre);
    v.dmax = ingest_wave_max(v.dmax);
    v.neg_min_mol = ingest_wave_max(v.neg_min_mol);
    v.max_mol = ingest_wave_max(v.max_mol);
    v.err = ingest_wave_or(v.err);
    __syncthreads();  // (an earlier use of the LDS words is over)
    if (lane == 0) {
        s_u[wave][0] = v.deg;
        s_u[wave][1] = v.ego_n;
        s_u[wave][2] = v.ego_e;
        s_u[wave][3] = v.pre;
        s_i[wave][0] = v.dmax;
        s_i[wave][1] = v.neg_min_mol;
        s_i[wave][2] = v.max_mol;
        s_i[wave][3] = v.err;
    }
    __syncthreads();
    IngestAcc r = {0, 0, 0, 0, 0, INT32_MIN, 0, 0};
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        r.deg += s_u[w][0];
        r.ego_n += s_u[w][1];
        r.ego_e += s_u[w][2];
        r.pre += s_u[w][3];
        r.dmax = max(r.dmax, s_i[w][0]);
        r.neg_min_mol = max(r.neg_min_mol, s_i[w][1]);
        r.max_mol = max(r.max_mol, s_i[w][2]);
        r.err |= s_i[w][3];
    }
    return r;
}

__global__ __launch_bounds__(256) void ingest_count_k(IngestArgs a) {
    __shared__ int32_t s_deg[256];
    int64_t n, er;
    IngestAcc acc = {0, 0, 0, 0, 0, INT32_MIN, 0, 0};
    const int size_err = ingest_sizes(a, n, er);
    acc.err = size_err;
    const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    const int W = a.W;
    int deg = 0;
    if (v < n) {
        const int g = ingest_owner(a.gptr, a.B, v);
        const int64_t base = a.gptr[g], ng = static_cast<int64_t>(a.gptr[g + 1]) - base;
        const int64_t lv = v - base;
        const bool placed = lv >= 0 && lv < ng && ng <= 32 * static_cast<int64_t>(W);
        if (!placed && (lv < 0 || lv >= ng)) acc.err |= SCGIB_INGEST_EGPTR;
        int self = 0;
        const uint32_t *row = a.bm + v * W;
        for (int w = 0; w < W; ++w) {
            uint32_t m = row[w];
            deg += __popc(m);
            if (placed && (lv >> 5) == w) self = (m >> (lv & 31)) & 1u;
            if (!a.bidirect && placed) {
                // verify mode: every (v <- u) needs its mirror (u <- v)
                while (m) {
                    const int64_t u = base + w * 32 + (__ffs(m) - 1);
                    m &= m - 1u;
                    if (u < 0 || u >= n) {
                        acc.err |= SCGIB_INGEST_ESYMMETRY;
                    } else if (!((a.bm[u * W + (lv >> 5)] >> (lv & 31)) & 1u)) {
                        acc.err |= SCGIB_INGEST_ESYMMETRY;
                    }
                }
            }
        }
        if (a.skip_rule && deg == 0 && lv == ng - 1) acc.err |= SCGIB_INGEST_ELASTNODE;
        const unsigned long long ball = 1ull + static_cast<unsigned>(deg) - static_cast<unsigned>(self);
        acc.deg = static_cast<unsigned>(deg);
        acc.ego_n = ball;
        acc.ego_e = static_cast<unsigned>(deg) * ball;
        acc.dmax = deg;
    }
    // graph_ptr: a monotone partition of [0, n); molecule sizes
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    for (int64_t i = v; i < a.B; i += stride) {
        const int64_t sz = static_cast<int64_t>(a.gptr[i + 1]) - a.gptr[i];
        if (sz < 0) acc.err |= SCGIB_INGEST_EGPTR;
        if (a.blob && sz < 2) acc.err |= SCGIB_INGEST_ESMALL;
        if (sz > kIngestMaxGraphNodes) acc.err |= SCGIB_INGEST_EGRAPH;
        else if (sz > a.mgn) acc.err |= SCGIB_INGEST_ECAPACITY;
        const int szc = static_cast<int>(min(max(sz, int64_t{-1}), int64_t{INT32_MAX}));
        acc.max_mol = max(acc.max_mol, szc);
        acc.neg_min_mol = max(acc.neg_min_mol, -szc);
    }
    if (v == 0) {
        // (a count outside its buffer was replaced by 0: nothing to compare the end with)
        if (a.gptr[0] != 0 || (!size_err && static_cast<int64_t>(a.gptr[a.B]) != n))
            acc.err |= SCGIB_INGEST_EGPTR;
        acc.err |= static_cast<int>(*a.head);  // what the mark launch flagged
    }
    // block-inclusive scan of the degrees, Hillis-Steele in LDS
    s_deg[threadIdx.x] = deg;
    __syncthreads();
    for (int off = 1; off < 256; off <<= 1) {
        int32_t t = 0;
        if (threadIdx.x >= off) t = s_deg[threadIdx.x - off];
        __syncthreads();
        s_deg[threadIdx.x] += t;
        __syncthreads();
    }
    if (v < n) a.pre[v] = s_deg[threadIdx.x];
    const IngestAcc r = ingest_block_reduce(acc);
    if (threadIdx.x == 0) {
        int64_t *p = a.part + static_cast<int64_t>(blockIdx.x) * kPartWords;
        p[0] = static_cast<int64_t>(r.deg);
        p[1] = static_cast<int64_t>(r.ego_n);
        p[2] = static_cast<int64_t>(r.ego_e);
        p[3] = r.dmax;
        p[4] = r.err;
        p[5] = r.neg_min_mol;
        p[6] = r.max_mol;
        p[7] = 0;
    }
}

__global__ __launch_bounds__(256) void ingest_fill_k(IngestArgs a) {
    int64_t n, er;
    IngestAcc acc = {0, 0, 0, 0, 0, INT32_MIN, 0, 0};
    acc.err = ingest_sizes(a, n, er);
    // every block sums the block records itself: totals, and its own offset
    for (int j = threadIdx.x; j < a.nblk; j += 256) {
        const int64_t *p = a.part + static_cast<int64_t>(j) * kPartWords;
        acc.deg += static_cast<unsigned long long>(p[0]);
        if (j < static_cast<int>(blockIdx.x)) acc.pre += static_cast<unsigned long long>(p[0]);
        acc.ego_n += static_cast<unsigned long long>(p[1]);
        acc.ego_e += static_cast<unsigned long long>(p[2]);
        acc.dmax = max(acc.dmax, static_cast<int>(p[3]));
        acc.err |= static_cast<int>(p[4]);
        acc.neg_min_mol = max(acc.neg_min_mol, static_cast<int>(p[5]));
        acc.max_mol = max(acc.max_mol, static_cast<int>(p[6]));
    }
    const IngestAcc r = ingest_block_reduce(acc);
    const int64_t e = static_cast<int64_t>(r.deg);
    int err = r.err;
    const int hard = SCGIB_INGEST_ERANGE | SCGIB_INGEST_EGRAPH | SCGIB_INGEST_ECAPACITY |
                     SCGIB_INGEST_EGPTR;
    // verify mode: fewer distinct edges than given = a duplicate (when every edge was marked)
    if (!a.bidirect && !(err & hard) && e != er) err |= SCGIB_INGEST_ESYMMETRY;
    if (e > a.col_cap) err |= SCGIB_INGEST_ECAPACITY;
    if (a.blob) {
        if (e > a.e_cap || r.ego_n > static_cast<unsigned long long>(a.ego_n_cap) ||
            r.ego_e > static_cast<unsigned long long>(a.ego_e_cap) || r.dmax > a.dmax_cap)
            err |= SCGIB_INGEST_ECAPACITY;
    }
    const bool ok = err == 0;
    const int W = a.W;
    const int64_t v = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (v < n) {
        const int g = ingest_owner(a.gptr, a.B, v);
        const int64_t base = a.gptr[g];
        uint32_t *row = a.bm + v * W;
        int64_t pos = static_cast<int64_t>(r.pre) + a.pre[v];  // end of the row
        int deg = 0;
        for (int w = 0; w < W; ++w) deg += __popc(row[w]);
        pos -= deg;
        if (ok) a.rowptr[v] = static_cast<int32_t>(pos);
        for (int w = 0; w < W; ++w) {
            uint32_t m = row[w];
            if (!m) continue;
            row[w] = 0u;  // the workspace resets itself, on the error path too
            if (!ok) continue;
            while (m) {
                a.col[pos++] = static_cast<int32_t>(base + w * 32 + (__ffs(m) - 1));
                m &= m - 1u;
            }
        }
    } else if (ok && v <= a.rows_cap) {
        a.rowptr[v] = static_cast<int32_t>(e);  // rowptr[n .. rows_cap] = e
    }
    const int64_t stride = static_cast<int64_t>(gridDim.x) * 256;
    if (ok && a.blob) {
        for (int64_t i = e + v; i < a.col_cap; i += stride) a.col[i] = 0;
        const int64_t live = n * a.F, all = a.rows_cap * a.F;
        for (int64_t i = v; i < all; i += stride) a.x_out[i] = i < live ? a.x[i] : 0.f;
        for (int64_t i = v; i <= a.B; i += stride) a.gptr_out[i] = a.gptr[i];
        if (v == 0)
            *reinterpret_cast<int4 *>(a.dims_out) =
                make_int4(static_cast<int>(n), static_cast<int>(e), 0, 0);
    }
    if (a.status) {
        for (int64_t i = v; i <= a.B; i += stride) a.status[kStatusWords + i] = a.gptr[i];
        if (v == 0) {
            int32_t *s = a.status;
            s[0] = err;
            s[1] = static_cast<int>(n);
            s[2] = static_cast<int>(min(e, static_cast<int64_t>(INT32_MAX)));
            s[3] = r.dmax;
            s[4] = a.B > 0 ? -r.neg_min_mol : 0;
            s[5] = r.max_mol;
            s[6] = static_cast<int>(r.ego_n & 0xffffffffull);
            s[7] = static_cast<int>(r.ego_n >> 32);
            s[8] = static_cast<int>(r.ego_e & 0xffffffffull);
            s[9] = static_cast<int>(r.ego_e >> 32);
            s[10] = ok ? 1 : 0;
            for (int i = 11; i < kStatusWords; ++i) s[i] = 0;
        }
    }
    if (v == 0) {
        *a.head = 0u;
        if (a.sticky && err) *a.sticky |= err;
    }
}

static int words_of(int max_graph_nodes) { return (std::max(max_graph_nodes, 1) + 31) / 32; }

static int64_t blocks_of(int64_t rows_cap) { return (rows_cap + 1 + 255) / 256; }

struct WsLayout {
    int64_t bm, pre, part, head, bytes;
};

static WsLayout ws_layout(int64_t rows_cap, int max_graph_nodes) {
    auto up = [](int64_t v) { return (v + 255) / 256 * 256; };
    // (the part that has to be zero between calls first: head and bitmaps)
    WsLayout l;
    l.head = 0;
    l.bm = 256;
    l.pre = up(l.bm + 4 * rows_cap * words_of(max_graph_nodes));
    l.part = up(l.pre + 4 * rows_cap);
    l.bytes = up(l.part + 8 * kPartWords * blocks_of(rows_cap));
    return l;
}

// ws_rows: the row count the workspace was sized (and is laid out) for, >= rows_cap
static int ingest_launch(IngestArgs a, void *ws, int64_t ws_rows, int max_graph_nodes,
                         int idx_bytes, hipStream_t st) {
    const WsLayout l = ws_layout(ws_rows, max_graph_nodes);
    char *w = static_cast<char *>(ws);
    a.bm = reinterpret_cast<uint32_t *>(w + l.bm);
    a.pre = reinterpret_cast<int32_t *>(w + l.pre);
    a.part = reinterpret_cast<int64_t *>(w + l.part);
    a.head = reinterpret_cast<uint32_t *>(w + l.head);
    a.W = words_of(max_graph_nodes);
    a.mgn = max_graph_nodes;
    a.nblk = static_cast<int32_t>(blocks_of(a.rows_cap));
    const unsigned egrid =
        static_cast<unsigned>(std::max<int64_t>(1, std::min<int64_t>((a.e_raw_cap + 255) / 256, 4096)));
    if (idx_bytes == 8) ingest_mark_k<int64_t><<<egrid, 256, 0, st>>>(a);
    else ingest_mark_k<int32_t><<<egrid, 256, 0, st>>>(a);
    ingest_count_k<<<a.nblk, 256, 0, st>>>(a);
    ingest_fill_k<<<a.nblk, 256, 0, st>>>(a);
    return launch_status();
}

}  // namespace scgib

using namespace scgib;

extern "C" int64_t scgib_ingest_workspace_bytes(int64_t rows_cap, int32_t max_graph_nodes) {
    if (rows_cap < 0 || max_graph_nodes < 1 || max_graph_nodes > kIngestMaxGraphNodes) return 0;
    return ws_layout(rows_cap, max_graph_nodes).bytes;
}

extern "C" int64_t scgib_ingest_status_words(int64_t n_graphs) {
    return n_graphs < 0 ? 0 : kStatusWords + n_graphs + 1;
}

extern "C" int scgib_ingest_csr(const void *src, const void *dst, int32_t idx_bytes, int64_t e_raw,
                                const int32_t *graph_ptr, int64_t n_graphs, int64_t n_nodes,
                                int32_t max_graph_nodes, int32_t bidirect, int32_t skip_rule,
                                void *ws, int64_t ws_rows, int32_t *rowptr, int32_t *col,
                                int64_t col_cap,
                                int32_t *status, scgib_stream_t stream) {
    const int64_t lim = (int64_t{1} << 31) - 512;
    if (!graph_ptr || !ws || !rowptr || !col || !status || (e_raw > 0 && (!src || !dst)))
        return SCGIB_EINVAL;
    if ((idx_bytes != 4 && idx_bytes != 8) || e_raw < 0 || n_graphs < 1 || n_nodes < 1 ||
        col_cap < 1 || max_graph_nodes < 1 || max_graph_nodes > kIngestMaxGraphNodes ||
        ws_rows < n_nodes)
        return SCGIB_EINVAL;
    if (ws_rows >= lim || n_nodes >= lim || n_graphs >= lim || col_cap >= lim || e_raw >= lim)
        return SCGIB_EUNSUPPORTED;
    IngestArgs a = {};
    a.src = src;
    a.dst = dst;
    a.gptr = graph_ptr;
    a.status = status;
    a.rowptr = rowptr;
    a.col = col;
    a.e_raw_cap = e_raw;
    a.n_host = n_nodes;
    a.rows_cap = n_nodes;
    a.col_cap = col_cap;
    a.B = static_cast<int32_t>(n_graphs);
    a.bidirect = bidirect ? 1 : 0;
    a.skip_rule = skip_rule ? 1 : 0;
    return ingest_launch(a, ws, ws_rows, max_graph_nodes, idx_bytes, as_stream(stream));
}

extern "C" int scgib_ingest_blob(const scgib_ingest_desc *d, scgib_stream_t stream) {
    if (!d || !d->graph_ptr || !d->x || !d->ws || !d->blob || !d->sticky ||
        (d->e_raw > 0 && (!d->src || !d->dst)))
        return SCGIB_EINVAL;
    if ((d->idx_bytes != 4 && d->idx_bytes != 8) || d->e_raw < 0 || d->B < 1 || d->F < 1 ||
        d->n_cap < 1 || d->e_cap < 0 || d->ego_n_cap < 0 || d->ego_e_cap < 0 ||
        d->max_in_degree < 0 || d->max_graph_nodes < 1 ||
        d->max_graph_nodes > kIngestMaxGraphNodes)
        return SCGIB_EINVAL;
    if (!d->counts && d->n < 0) return SCGIB_EINVAL;  // (n > n_cap: a capacity error bit)
    const int64_t lim = (int64_t{1} << 31) - 512;
    if (d->n_cap >= lim || d->e_cap >= lim || d->e_raw >= lim || d->n_cap * d->F >= lim)
        return SCGIB_EUNSUPPORTED;
    // every section ends before the next one and the blob (StaticBatch._layout)
    const int64_t col_cap = std::max<int64_t>(d->e_cap, 1);
    if ((d->o_rowptr | d->o_col | d->o_gptr | d->o_dims | d->o_x | d->blob_bytes) & 15)
        return SCGIB_EINVAL;
    if (!(d->o_rowptr >= 0 && d->o_rowptr + 4 * (d->n_cap + 1) <= d->o_col &&
          d->o_col + 4 * col_cap <= d->o_gptr && d->o_gptr + 4 * (int64_t{d->B} + 1) <= d->o_dims &&
          d->o_dims + 16 <= d->o_x && d->o_x + 4 * d->n_cap * d->F <= d->blob_bytes))
        return SCGIB_EINVAL;
    char *blob = static_cast<char *>(d->blob);
    IngestArgs a = {};
    a.src = d->src;
    a.dst = d->dst;
    a.gptr = d->graph_ptr;
    a.counts = d->counts;
    a.x = d->x;
    a.status = d->status;
    a.sticky = d->sticky;
    a.rowptr = reinterpret_cast<int32_t *>(blob + d->o_rowptr);
    a.col = reinterpret_cast<int32_t *>(blob + d->o_col);
    a.gptr_out = reinterpret_cast<int32_t *>(blob + d->o_gptr);
    a.dims_out = reinterpret_cast<int32_t *>(blob + d->o_dims);
    a.x_out = reinterpret_cast<float *>(blob + d->o_x);
    a.e_raw_cap = d->e_raw;
    a.n_host = d->n;
    a.rows_cap = d->n_cap;
    a.col_cap = col_cap;
    a.e_cap = d->e_cap;
    a.ego_n_cap = d->ego_n_cap;
    a.ego_e_cap = d->ego_e_cap;
    a.B = d->B;
    a.F = d->F;
    a.dmax_cap = d->max_in_degree;
    a.bidirect = d->bidirect ? 1 : 0;
    a.skip_rule = d->skip_rule ? 1 : 0;
    a.blob = 1;
    return ingest_launch(a, d->ws, d->n_cap, d->max_graph_nodes, d->idx_bytes, as_stream(stream));
}
