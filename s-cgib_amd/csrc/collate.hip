// Device-side collation of shuffled batches from a resident dataset
// (graph.DeviceDataset / graph.DeviceLoader).
//
// The dataset sits in HBM as flat per-molecule CSRs (molecule-local column
// ids, node-local row pointers, 64-bit molecule offsets).  A collated batch
// is the offset concatenation of its molecules' CSRs, so one step's batch is
// built by two small launches inside the replayed step graph:
//
//   collate_plan_k  one workgroup: batch ids from the epoch permutation and
//                   the position counter, per-molecule counts gathered and
//                   block-scanned into graph_ptr / edge offsets (workspace),
//                   ego bounds summed, everything compared against the static
//                   batch's capacities -> fits flag; advances the position.
//   collate_fill_k  grid over the slot: every 16-byte word of the rowptr,
//                   col, graph_ptr, dims and x sections of the destination
//                   slot, tails included, so the slot is byte for byte what
//                   StaticBatch.pad would have uploaded; and the labels / ids
//                   of the batch the step is training on.
//
// Every store into the ring goes to slot + section offset + 16 * q with q
// below the section's 16-byte word count; the entry points refuse layouts in
// which a section's words would pass the next section or the slot.  On
// overflow (fits == 0) the fill writes nothing to the slot.  Integer work
// only: deterministic.  Index arithmetic into the dataset arrays is 64-bit.
//
// The sequential loader (graph.DeviceEvalLoader) runs the same
// two bodies over another batch sequence: collate_seq_plan_k takes batch j of
// an index list whose length, fill molecule and position sit in device memory
// (state[0] position, [1] overflow count, [2] list length, [3] fill id), the
// rows past the list's end being copies of the fill molecule with id -1;
// collate_seq_fill_k gathers NaN labels and id -1 for those rows.  There an
// overflowing batch marks its slot's ids -1 as well.
#include <algorithm>

#include "common.h"

namespace scgib {

constexpr int kPlanThreads = 1024;
constexpr int kPlanItems = 4;  // molecules per plan thread: B <= 4096
constexpr int kMaxBatch = kPlanThreads * kPlanItems;
// ws (int32 words): fits, n, e, dst slot, current slot, dst slot pointer (2), spare |
// gptr [B+1] | eoff [B+1] | (8-byte aligned) nbase [B] int64 | ebase [B] int64
constexpr int kWsHead = 8;
__host__ __device__ inline int64_t ws_base64(int64_t B) { return (kWsHead + 2 * (B + 1) + 1) & ~int64_t{1}; }

__device__ __forceinline__ int wave_scan_incl(int v, int lane) {
#pragma unroll
    for (int off = 1; off < kWave; off <<= 1) {
        const int u = __shfl_up(v, off, kWave);
        if (lane >= off) v += u;
    }
    return v;
}

__device__ __forceinline__ unsigned long long wave_sum_u64(unsigned long long v) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// blockDim.x = the multiple of 64 covering ceil(B / kPlanItems) threads.
// kSeq: the sequential loader's batch j = (position + ahead) mod steps of the
// index list d.perm[0 .. state[2]) (state[2] clamped to 1 .. d.M, its capacity).
template <bool kSeq>
__device__ __forceinline__ void plan_body(const scgib_collate_desc &d, int32_t ahead,
                                          int32_t slot_fixed, int32_t advance) {
    __shared__ int s_wn[kPlanThreads / kWave], s_we[kPlanThreads / kWave];
    __shared__ unsigned long long s_gn[kPlanThreads / kWave], s_ge[kPlanThreads / kWave];
    __shared__ int s_fits;
    const int tid = threadIdx.x, lane = tid & (kWave - 1), wave = tid / kWave;
    const int nwaves = blockDim.x / kWave;
    const int64_t D = d.D > 0 ? d.D : d.M;  // molecules in the dataset
    // the position's period: the two-epoch window, or the steps of one pass
    int64_t len = d.M, fill = 0, S2 = 2 * d.S;
    if (kSeq) {
        len = static_cast<int64_t>(d.state[2]);
        len = len < 1 ? 1 : (len > d.M ? d.M : len);
        fill = static_cast<int64_t>(d.state[3]);  // (clamped with the other ids below)
        S2 = (len + d.B - 1) / d.B;
    }
    const int64_t pos = static_cast<int64_t>(d.state[0]) % S2;
    const unsigned cur = d.cursor[0];
    const int64_t j = (pos + ahead) % S2;
    // batch j of the two-epoch window: permutation buffer j / S, offset (j % S) * B;
    // batch j of the index list: offset j * B
    const int64_t base = kSeq ? j * d.B : (j / d.S) * d.M + (j % d.S) * d.B;

    int id[kPlanItems], nn[kPlanItems], ee[kPlanItems];
    int64_t nb[kPlanItems], eb[kPlanItems];
    int tn = 0, te = 0;
    unsigned long long gn = 0, ge = 0;
#pragma unroll
    for (int q = 0; q < kPlanItems; ++q) {
        const int i = tid * kPlanItems + q;
        id[q] = 0;
        nn[q] = ee[q] = 0;
        nb[q] = eb[q] = 0;
        if (i < d.B) {
            const bool real = !kSeq || base + i < len;  // else a copy of the fill molecule
            int64_t m = real ? d.perm[base + i] : fill;
            m = m < 0 ? 0 : (m >= D ? D - 1 : m);  // (host-written; never out of range)
            id[q] = real ? static_cast<int>(m) : -1;
            nb[q] = d.node_off[m];
            eb[q] = d.edge_off[m];
            nn[q] = static_cast<int>(d.node_off[m + 1] - nb[q]);
            ee[q] = static_cast<int>(d.edge_off[m + 1] - eb[q]);
            gn += static_cast<unsigned>(d.ego_nodes[m]);
            ge += static_cast<unsigned>(d.ego_edges[m]);
            tn += nn[q];
            te += ee[q];
        }
    }
    const int in_n = wave_scan_incl(tn, lane), in_e = wave_scan_incl(te, lane);
    gn = wave_sum_u64(gn);
    ge = wave_sum_u64(ge);
    if (lane == kWave - 1) {
        s_wn[wave] = in_n;
        s_we[wave] = in_e;
        s_gn[wave] = gn;
        s_ge[wave] = ge;
    }
    __syncthreads();
    int off_n = in_n - tn, off_e = in_e - te;
    for (int w = 0; w < wave; ++w) {
        off_n += s_wn[w];
        off_e += s_we[w];
    }
    const unsigned dst = slot_fixed >= 0 ? static_cast<unsigned>(slot_fixed) : (cur + 1u) % 3u;
    if (tid == static_cast<int>(blockDim.x) - 1) {  // its inclusive totals are the batch's
        const int64_t n = off_n + tn, e = off_e + te;
        unsigned long long tgn = 0, tge = 0;
        for (int w = 0; w < nwaves; ++w) {
            tgn += s_gn[w];
            tge += s_ge[w];
        }
        const int fits = n <= d.n_cap && e <= d.e_cap &&
                         tgn <= static_cast<unsigned long long>(d.ego_n_cap) &&
                         tge <= static_cast<unsigned long long>(d.ego_e_cap);
        const uint64_t slot = d.srcs[dst];
        s_fits = fits;
        d.ws[0] = fits;
        d.ws[1] = static_cast<int>(n);
        d.ws[2] = static_cast<int>(e);
        d.ws[3] = static_cast<int>(dst);
        d.ws[4] = static_cast<int>((cur + 2u) % 3u);  // the slot the step's load_next read
        d.ws[5] = static_cast<int>(slot & 0xffffffffu);
        d.ws[6] = static_cast<int>(slot >> 32);
        if (!fits) d.state[1] += 1u;  // sticky overflow count (DeviceLoader.error)
        if (advance) d.state[0] = static_cast<unsigned>((pos + 1) % S2);
        d.ws[kWsHead + d.B] = static_cast<int>(n);  // graph_ptr[B], edge offset [B]
        d.ws[kWsHead + d.B + 1 + d.B] = static_cast<int>(e);
    }
    __syncthreads();
    const int fits = s_fits;
    int *gptr = d.ws + kWsHead, *eoff = gptr + d.B + 1;
    int64_t *nbase = reinterpret_cast<int64_t *>(d.ws + ws_base64(d.B)), *ebase = nbase + d.B;
    int *ids = d.slot_ids + static_cast<int64_t>(dst) * d.B;
#pragma unroll
    for (int q = 0; q < kPlanItems; ++q) {
        const int i = tid * kPlanItems + q;
        if (i < d.B) {
            gptr[i] = off_n;
            eoff[i] = off_e;
            nbase[i] = nb[q];
            ebase[i] = eb[q];
            // an overflowing batch leaves the slot's ids too; in a sequential
            // pass it marks them: the step that scores the stale bytes labels nothing
            if (fits) ids[i] = id[q];
            else if (kSeq) ids[i] = -1;
        }
        off_n += nn[q];
        off_e += ee[q];
    }
}

__global__ __launch_bounds__(kPlanThreads) void collate_plan_k(scgib_collate_desc d, int32_t ahead,
                                                               int32_t slot_fixed,
                                                               int32_t advance) {
    plan_body<false>(d, ahead, slot_fixed, advance);
}

__global__ __launch_bounds__(kPlanThreads) void collate_seq_plan_k(scgib_collate_desc d,
                                                                   int32_t ahead,
                                                                   int32_t slot_fixed,
                                                                   int32_t advance) {
    plan_body<true>(d, ahead, slot_fixed, advance);
}

// largest m in [0, B) with ptr[m] <= v, for 0 <= v < ptr[B] (ptr[0] = 0)
__device__ __forceinline__ int find_segment(const int *ptr, int B, int v) {
    int lo = 0, hi = B;
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if (ptr[mid] <= v) lo = mid;
        else hi = mid;
    }
    return lo;
}

// Segments of four consecutive elements v0 .. v0 + 3 of a section whose live
// part is [0, live): m[t] for the live ones (LDS only), 0 for the rest.
__device__ __forceinline__ void find4(const int *ptr, int B, int64_t v0, int64_t live, int scale,
                                      int (&m)[4]) {
    int cur = v0 < live ? find_segment(ptr, B, static_cast<int>(v0 / scale)) : 0;
#pragma unroll
    for (int t = 0; t < 4; ++t) {
        const int64_t v = v0 + t;
        if (v < live) {
            while (v >= static_cast<int64_t>(ptr[cur + 1]) * scale) ++cur;
        }
        m[t] = cur;
    }
}

// kMasked: a negative slot id (a fill row, or a slot whose batch overflowed in
// a sequential pass) gets a label row of NaN and id -1 instead of y[id].
template <bool kMasked>
__device__ __forceinline__ void fill_body(const scgib_collate_desc &d, int32_t labels, int *s_ptr) {
    const int B = d.B, F = d.F, T = d.T;
    // staged whatever the plan found: the header's loads stay in flight beside these
    for (int i = threadIdx.x; i < 2 * (B + 1); i += blockDim.x) s_ptr[i] = d.ws[kWsHead + i];
    const int fits = d.ws[0], n = d.ws[1], e = d.ws[2];
    const unsigned cur = static_cast<unsigned>(d.ws[4]) % 3u;
    char *slot = reinterpret_cast<char *>(static_cast<uint64_t>(static_cast<unsigned>(d.ws[5])) |
                                          (static_cast<uint64_t>(static_cast<unsigned>(d.ws[6])) << 32));
    const int *s_gptr = s_ptr, *s_eoff = s_ptr + B + 1;
    const int64_t *nbase = reinterpret_cast<const int64_t *>(d.ws + ws_base64(B)), *ebase = nbase + B;
    const int *cur_ids = d.slot_ids + static_cast<int64_t>(cur) * B;
    // (the entry points refuse capacities at or above 2^31 - 8, n_cap * F too)
    const int n_cap = static_cast<int>(d.n_cap), e_cap = static_cast<int>(d.e_cap);
    const int R4 = (n_cap + 1 + 3) / 4, C4 = ((e_cap > 1 ? e_cap : 1) + 3) / 4,
              G4 = (B + 1 + 3) / 4, X4 = (n_cap * F + 3) / 4;
    const int stride = static_cast<int>(gridDim.x * blockDim.x);
    const int gtid = static_cast<int>(blockIdx.x * blockDim.x + threadIdx.x);
    // One grid-stride loop per section (16-byte words q of the section), each
    // starting where the section before ended in the grid: with one thread
    // per word (the launch's grid, up to its cap) a thread takes one word of
    // one section, and no thread walks the sections one after the other.
    const int nlab = labels ? B * T + B : 0;
    const int first_x = gtid - nlab % stride + (gtid < nlab % stride ? stride : 0);
    const int end_x = static_cast<int>((static_cast<int64_t>(nlab) + X4) % stride);
    const int first_c = gtid - end_x + (gtid < end_x ? stride : 0);
    const int end_c = static_cast<int>((static_cast<int64_t>(end_x) + C4) % stride);
    const int first_r = gtid - end_c + (gtid < end_c ? stride : 0);
    const int end_r = static_cast<int>((static_cast<int64_t>(end_c) + R4) % stride);
    const int first_g = gtid - end_r + (gtid < end_r ? stride : 0);
    if (labels) {  // labels and ids of the batch the step trains on
        const int nl = B * T;
        for (int l = gtid; l < nl + B; l += stride) {
            if (l < nl) {
                const int64_t id = cur_ids[l / T];
                if (kMasked && id < 0) d.labels[l] = __builtin_nanf("");
                else d.labels[l] = d.y[id * T + l % T];
            } else {
                d.ids[l - nl] = cur_ids[l - nl];
            }
        }
    }
    __syncthreads();
    if (!fits) return;  // overflow: the slot keeps its earlier batch
    // Each word: the four elements' molecules from LDS, then their source
    // bases, then the data, each group of loads in flight together (ld_ok).
    // x rows; tail = 0
    const int64_t live = static_cast<int64_t>(n) * F;
    for (int q = first_x; q < X4; q += stride) {
        const int64_t i0 = static_cast<int64_t>(q) * 4;
        float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
        if ((F & 3) == 0) {  // a word stays inside its row: one 16-byte load
            if (i0 < live) {
                const int m = find_segment(s_gptr, B, static_cast<int>(i0 / F));
                const int64_t src = nbase[m] * F + (i0 - static_cast<int64_t>(s_gptr[m]) * F);
                o = *reinterpret_cast<const float4 *>(d.x + src);
            }
        } else if (i0 < live) {
            int m[4];
            find4(s_gptr, B, i0, live, F, m);
            int64_t src[4];
#pragma unroll
            for (int t = 0; t < 4; ++t)
                src[t] = nbase[m[t]] * F + (i0 + t - static_cast<int64_t>(s_gptr[m[t]]) * F);
            float out[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) out[t] = ld_ok(d.x, src[t], src[0], i0 + t < live, 0.f);
            o = make_float4(out[0], out[1], out[2], out[3]);
        }
        *reinterpret_cast<float4 *>(slot + d.o_x + 16 * static_cast<int64_t>(q)) = o;
    }
    // col: molecule-local id + node offset; tail = 0
    for (int q = first_c; q < C4; q += stride) {
        const int64_t c0 = static_cast<int64_t>(q) * 4;
        int out[4] = {0, 0, 0, 0};
        if (c0 < e) {
            int m[4];
            find4(s_eoff, B, c0, e, 1, m);
            int64_t src[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) src[t] = ebase[m[t]] + (c0 + t - s_eoff[m[t]]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const bool ok = c0 + t < e;
                out[t] = ld_ok(d.col, src[t], src[0], ok, 0) + (ok ? s_gptr[m[t]] : 0);
            }
        }
        *reinterpret_cast<int4 *>(slot + d.o_col + 16 * static_cast<int64_t>(q)) =
            make_int4(out[0], out[1], out[2], out[3]);
    }
    // rowptr: edge offset + node-local row pointer; tail = e
    for (int q = first_r; q < R4; q += stride) {
        const int64_t v0 = static_cast<int64_t>(q) * 4;
        int out[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) out[t] = v0 + t <= n_cap ? e : 0;
        if (v0 < n) {
            int m[4];
            find4(s_gptr, B, v0, n, 1, m);
            int64_t src[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) src[t] = nbase[m[t]] + (v0 + t - s_gptr[m[t]]);
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                const bool ok = v0 + t < n;
                const int r = ld_ok(d.rp_local, src[t], src[0], ok, 0);
                if (ok) out[t] = s_eoff[m[t]] + r;
            }
        }
        *reinterpret_cast<int4 *>(slot + d.o_rowptr + 16 * static_cast<int64_t>(q)) =
            make_int4(out[0], out[1], out[2], out[3]);
    }
    // graph_ptr, and dims = [n, e] with the zeroed ego error word
    for (int q = first_g; q < G4; q += stride) {
        int out[4];
#pragma unroll
        for (int t = 0; t < 4; ++t) out[t] = q * 4 + t <= B ? s_gptr[q * 4 + t] : 0;
        *reinterpret_cast<int4 *>(slot + d.o_gptr + 16 * static_cast<int64_t>(q)) =
            make_int4(out[0], out[1], out[2], out[3]);
    }
    if (gtid == stride - 1) *reinterpret_cast<int4 *>(slot + d.o_dims) = make_int4(n, e, 0, 0);
}

__global__ __launch_bounds__(256) void collate_fill_k(scgib_collate_desc d, int32_t labels) {
    extern __shared__ __attribute__((aligned(16))) int s_ptr[];  // gptr [B+1] | eoff [B+1]
    fill_body<false>(d, labels, s_ptr);
}

__global__ __launch_bounds__(256) void collate_seq_fill_k(scgib_collate_desc d, int32_t labels) {
    extern __shared__ __attribute__((aligned(16))) int s_ptr[];  // gptr [B+1] | eoff [B+1]
    fill_body<true>(d, labels, s_ptr);
}

// seq: a sequential loader's descriptor (M = the index list's capacity, S unused)
static bool desc_ok(const scgib_collate_desc *d, bool seq = false) {
    if (!d) return false;
    if (!d->node_off || !d->edge_off || !d->rp_local || !d->col || !d->x || !d->ego_nodes ||
        !d->ego_edges || !d->perm || !d->srcs || !d->cursor || !d->state || !d->ws ||
        !d->slot_ids || !d->ids)
        return false;
    if (d->B < 1 || d->B > kMaxBatch || d->M < 1 || d->F < 1 || d->T < 0 ||
        (d->T > 0 && (!d->y || !d->labels)))
        return false;
    if (seq ? d->D < 1 : (d->D < 0 || d->S < 1 || d->S * d->B > d->M)) return false;
    const int64_t lim = (int64_t{1} << 31) - 8;
    if (d->n_cap < 0 || d->e_cap < 0 || d->ego_n_cap < 0 || d->ego_e_cap < 0 || d->n_cap >= lim ||
        d->e_cap >= lim || d->n_cap * d->F >= lim)
        return false;
    // every section's 16-byte words end before the next section and the slot
    const int64_t R4 = (d->n_cap + 1 + 3) / 4, C4 = (std::max<int64_t>(d->e_cap, 1) + 3) / 4,
                  G4 = (d->B + 1 + 3) / 4, X4 = (d->n_cap * d->F + 3) / 4;
    if ((d->o_rowptr | d->o_col | d->o_gptr | d->o_dims | d->o_x | d->blob_bytes) & 15) return false;
    return d->o_rowptr >= 0 && d->o_rowptr + 16 * R4 <= d->o_col && d->o_col + 16 * C4 <= d->o_gptr &&
           d->o_gptr + 16 * G4 <= d->o_dims && d->o_dims + 16 <= d->o_x &&
           d->o_x + 16 * X4 <= d->blob_bytes;
}

}  // namespace scgib

using namespace scgib;

extern "C" int64_t scgib_collate_max_batch(void) { return kMaxBatch; }

extern "C" int64_t scgib_collate_ws_words(int64_t batch) { return ws_base64(batch) + 4 * batch; }

extern "C" int scgib_collate_plan(const scgib_collate_desc *d, int32_t ahead, int32_t slot,
                                  int32_t advance, scgib_stream_t stream) {
    if (!desc_ok(d) || ahead < 0 || ahead >= 2 * d->S || slot < -1 || slot > 2) return SCGIB_EINVAL;
    const int threads = ((d->B + kPlanItems - 1) / kPlanItems + kWave - 1) / kWave * kWave;
    collate_plan_k<<<1, threads, 0, as_stream(stream)>>>(*d, ahead, slot, advance ? 1 : 0);
    return launch_status();
}

static int launch_fill(const scgib_collate_desc *d, int32_t labels, bool seq,
                       scgib_stream_t stream) {
    if (!desc_ok(d, seq)) return SCGIB_EINVAL;
    const int64_t quads = (d->n_cap + 1 + 3) / 4 + (std::max<int64_t>(d->e_cap, 1) + 3) / 4 +
                          (d->B + 1 + 3) / 4 + 1 + (d->n_cap * d->F + 3) / 4;
    const int64_t total = quads + (labels ? static_cast<int64_t>(d->B) * d->T + d->B : 0);
    const int64_t grid = std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 2048));
    const size_t lds = sizeof(int) * 2 * (static_cast<size_t>(d->B) + 1);
    if (seq) collate_seq_fill_k<<<(unsigned)grid, 256, lds, as_stream(stream)>>>(*d, labels ? 1 : 0);
    else collate_fill_k<<<(unsigned)grid, 256, lds, as_stream(stream)>>>(*d, labels ? 1 : 0);
    return launch_status();
}

extern "C" int scgib_collate_fill(const scgib_collate_desc *d, int32_t labels,
                                  scgib_stream_t stream) {
    return launch_fill(d, labels, false, stream);
}

extern "C" int scgib_collate_seq_plan(const scgib_collate_desc *d, int32_t ahead, int32_t slot,
                                      int32_t advance, scgib_stream_t stream) {
    if (!desc_ok(d, true) || ahead < 0 || ahead > 2 || slot < -1 || slot > 2) return SCGIB_EINVAL;
    const int threads = ((d->B + kPlanItems - 1) / kPlanItems + kWave - 1) / kWave * kWave;
    collate_seq_plan_k<<<1, threads, 0, as_stream(stream)>>>(*d, ahead, slot, advance ? 1 : 0);
    return launch_status();
}

extern "C" int scgib_collate_seq_fill(const scgib_collate_desc *d, int32_t labels,
                                      scgib_stream_t stream) {
    return launch_fill(d, labels, true, stream);
}
