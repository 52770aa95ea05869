// logM reconstruction on the device (gfx950): the targets built from the
// step's own ego-nets, and the loss in Gram + sparse form.
//
// Reference: util.getM_logM / GetProbTranMat (util.py:60-91) builds, per
// molecule of n nodes, L_i[r,c] = max(0, log(A^i[r,c] / colsum_i[c]) - log(1/n))
// for i = 1..k as dense fp64 matrices; loss_recon (models.py:770-782) forms
// sum_i ||X X^T - L_i||_F^2 / (k n^2) over the dense n x n product.
//
// Support: A^i[r,c] counts the walks of length i from r to c, so L_i[r,c] is
// zero unless r lies in the k-hop ball of c -- exactly the (r, c) pairs the
// ego batch lists (slot j of ball(c) <-> r = ego_nodes[j], sorted per ball,
// c itself included).  With S = sum_i L_i, C = sum_i ||L_i||_F^2, G = X^T X:
//   sum_i ||X X^T - L_i||_F^2 = k ||G||_F^2 - 2 sum_slots S[r,c] <x_r, x_c> + C
//   d/dX = (4k X G - 2 (S + S^T) X) / (k n^2).
//
// logm_targets_k, one workgroup per molecule, k hops:
//   W_i[slot(r,c)] = sum over in-neighbours u of c of W_{i-1}[slot(r,u)]
//   (W_0 = [r == u]; slot(r,u) by binary search of r in the sorted ball(u));
//   exact integers (uint32, sums in uint64); colsum_i[c] = sum over ball(c),
//   kept in LDS as doubles (exact below 2^53).  A last pass forms the terms
//   in fp64 with the reference's own expression, rounds each to fp32 as the
//   reference's targets are, and sums them in fp64: s_in = S[r,c],
//   s_sym = S[r,c] + S[c,r] (A^i is symmetric, so W_i[slot(r,c)] is also the
//   count of walks c -> r; only the column sum differs), C_g by a fixed-order
//   tree.  Scratch: k * N_s counts.
// recon_logm_sparse_fwd_k, grid (B, 1 + T), T = ceil(max_graph_nodes / 64):
//   y = 0: the molecule's 64 x 64 Gram with the exact-f32 MFMA
//   (v_mfma_f32_32x32x2_f32, one quadrant per wave, as recon_partial_k), G
//   stored for the backward, ||G||_F^2 in fp64; y >= 1: the slot term of the
//   rows of 64-row chunks y - 1, y - 1 + T, ... (one wave per row c, lane =
//   channel), fp64 across rows.  recon_logm_sparse_fin_k combines the three
//   terms per molecule in fp64 (they cancel when X X^T ~ L); the per-molecule
//   values are summed by launch_slab_reduce.
// recon_logm_sparse_bwd_k, grid (B + 1, T): G_g staged in LDS, row c gets
//   g (4k (X G)_c - 2 sum_{j in ball(c)} s_sym[j] x_{r_j}) / (k n^2); block
//   row B zero-fills the rows in [live N, capacity).
// Every reduction has a fixed order; no floating-point atomics.
#include "recon_fin.h"

namespace scgib {

constexpr int kLogmMaxK = 8;        // colsum LDS: 8 x 512 doubles
constexpr int kLogmMaxNodes = 512;  // the ego builder's molecule limit
constexpr uint64_t kLogmMaxCount = 0x7fffffffull;
constexpr int kLogmErrEdge = 1;   // an index leaves its molecule / its buffer
constexpr int kLogmErrBig = 2;    // molecule larger than kLogmMaxNodes
constexpr int kLogmErrCount = 4;  // a walk count above kLogmMaxCount

__host__ __device__ __forceinline__ int logm_chunks(int64_t max_graph_nodes) {
    const int64_t t = (max_graph_nodes + 63) / 64;
    return static_cast<int>(t < 1 ? 1 : (t > 8 ? 8 : t));
}

// index of r in the ascending list nodes[lo, hi), or -1
__device__ __forceinline__ int logm_find(const int32_t *__restrict__ nodes, int lo, int hi, int r) {
    int a = lo, b = hi;
    while (a < b) {
        const int m = (a + b) >> 1;
        if (nodes[m] < r) a = m + 1; else b = m;
    }
    return (a < hi && nodes[a] == r) ? a : -1;
}

// c with sptr[c] <= s < sptr[c + 1], given sptr[0] <= s < sptr[n]
__device__ __forceinline__ int logm_owner(const int32_t *sptr, int n, int s) {
    int a = 0, b = n;
    while (b - a > 1) {
        const int m = (a + b) >> 1;
        if (sptr[m] <= s) a = m; else b = m;
    }
    return a;
}

__device__ __forceinline__ float logm_term(double w, double colsum, double ln_inv_n) {
    if (!(colsum > 0.0)) return 0.f;
    const double v = log(w / colsum) - ln_inv_n;
    return v > 0.0 ? static_cast<float>(v) : 0.f;
}

// molecule g's live row range; false: padded (n = 0) or not usable
__device__ __forceinline__ bool logm_rows(const int32_t *__restrict__ gptr, int64_t g,
                                          int64_t nlive, int64_t &r0, int &n) {
    r0 = gptr[g];
    const int64_t r1 = gptr[g + 1];
    n = static_cast<int>(r1 - r0);
    return r0 >= 0 && r1 > r0 && r1 <= nlive && r1 - r0 <= kLogmMaxNodes;
}

__global__ __launch_bounds__(256) void logm_targets_k(
    const int32_t *__restrict__ rowptr, const int32_t *__restrict__ col,
    const int32_t *__restrict__ gptr, int64_t ncap, int64_t ecap,
    const int32_t *__restrict__ ego_ptr, const int32_t *__restrict__ ego_nodes, int64_t ns_cap,
    int kstep, uint32_t *W, float *__restrict__ s_in, float *__restrict__ s_sym,
    double *__restrict__ C, int32_t *err, const int32_t *__restrict__ dims) {
    __shared__ int32_t sptr[kLogmMaxNodes + 1];
    __shared__ double scs[kLogmMaxK][kLogmMaxNodes];
    __shared__ double sred[256];
    const int tid = threadIdx.x;
    const int64_t g = blockIdx.x;
    const int64_t nlive = eff_count(dims, 0, ncap);
    int64_t r0;
    int n;
    if (!logm_rows(gptr, g, nlive, r0, n)) {  // block-uniform
        if (tid == 0) {
            C[g] = 0.0;
            const int64_t d = static_cast<int64_t>(gptr[g + 1]) - gptr[g];
            if (d > kLogmMaxNodes) atomicOr(err, kLogmErrBig);
            else if (d != 0) atomicOr(err, kLogmErrEdge);
        }
        return;
    }
    for (int i = tid; i <= n; i += 256) sptr[i] = ego_ptr[r0 + i];
    __syncthreads();
    int bad = sptr[0] < 0 || sptr[n] > ns_cap;
    for (int i = tid; i < n; i += 256) bad |= sptr[i] > sptr[i + 1];
    if (__syncthreads_or(bad)) {  // ego pointers not usable: no targets, flagged
        if (tid == 0) {
            C[g] = 0.0;
            atomicOr(err, kLogmErrEdge);
        }
        return;
    }
    const int s0 = sptr[0], s1 = sptr[n];
    int flags = 0;
    for (int i = 0; i < kstep; ++i) {
        uint32_t *Wi = W + static_cast<int64_t>(i) * ns_cap;
        const uint32_t *Wp = i > 0 ? Wi - ns_cap : Wi;  // W_{i-1} (unused at i = 0)
        for (int s = s0 + tid; s < s1; s += 256) {
            const int c = logm_owner(sptr, n, s);
            const int r = ego_nodes[s];
            uint64_t sum = 0;
            if (r < r0 || r >= r0 + n) {
                flags |= kLogmErrEdge;
            } else {
                const int64_t e0 = rowptr[r0 + c], e1 = rowptr[r0 + c + 1];
                if (e0 < 0 || e1 > ecap) {
                    flags |= kLogmErrEdge;
                } else {
                    for (int64_t e = e0; e < e1; ++e) {
                        const int u = col[e];
                        const int ul = u - static_cast<int>(r0);
                        if (ul < 0 || ul >= n) {
                            flags |= kLogmErrEdge;
                            continue;
                        }
                        if (i == 0) {
                            sum += u == r;
                        } else {
                            const int j = logm_find(ego_nodes, sptr[ul], sptr[ul + 1], r);
                            if (j >= 0) sum += Wp[j];
                        }
                    }
                }
            }
            if (sum > kLogmMaxCount) {
                flags |= kLogmErrCount;
                sum = 0;
            }
            Wi[s] = static_cast<uint32_t>(sum);
        }
        __syncthreads();  // (workgroup-scope fence: W_i visible to the whole workgroup)
        for (int c = tid; c < n; c += 256) {
            uint64_t t = 0;
            for (int s = sptr[c]; s < sptr[c + 1]; ++s) t += Wi[s];
            scs[i][c] = static_cast<double>(t);
        }
        __syncthreads();
    }
    if (flags) atomicOr(err, flags);
    const double ln_inv_n = log(1.0 / static_cast<double>(n));
    double cacc = 0.0;
    for (int s = s0 + tid; s < s1; s += 256) {
        const int c = logm_owner(sptr, n, s);
        const int rl = ego_nodes[s] - static_cast<int>(r0);
        double si = 0.0, so = 0.0;
        if (rl >= 0 && rl < n) {
            for (int i = 0; i < kstep; ++i) {
                const uint32_t w = W[static_cast<int64_t>(i) * ns_cap + s];
                if (w == 0) continue;
                const double wd = static_cast<double>(w);
                const float lin = logm_term(wd, scs[i][c], ln_inv_n);
                const float lout = logm_term(wd, scs[i][rl], ln_inv_n);
                si += static_cast<double>(lin);
                so += static_cast<double>(lout);
                cacc += static_cast<double>(lin) * static_cast<double>(lin);
            }
        }
        s_in[s] = static_cast<float>(si);
        s_sym[s] = static_cast<float>(si + so);
    }
    sred[tid] = cacc;
    __syncthreads();
    for (int off = 128; off >= 1; off >>= 1) {
        if (tid < off) sred[tid] += sred[tid + off];
        __syncthreads();
    }
    if (tid == 0) C[g] = sred[0];
}

// sum over the slots j of ball(c) of wgt[j] * im[ego_nodes[j]][lane]
// (wave-uniform slot walk, four rows in flight)
__device__ __forceinline__ float logm_ball_row(const float *__restrict__ im,
                                               const int32_t *__restrict__ ego_nodes,
                                               const float *__restrict__ wgt, int64_t b0,
                                               int64_t b1, int64_t r0, int n, int lane) {
    float nb = 0.f;
    int64_t j = b0;
    for (; j + 4 <= b1; j += 4) {
        float x[4], w[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int64_t r = ego_nodes[j + q];
            const bool ok = r >= r0 && r < r0 + n;
            x[q] = im[(ok ? r : r0) * 64 + lane];
            w[q] = ok ? wgt[j + q] : 0.f;
        }
#pragma unroll
        for (int q = 0; q < 4; ++q) nb += w[q] * x[q];
    }
    for (; j < b1; ++j) {
        const int64_t r = ego_nodes[j];
        const bool ok = r >= r0 && r < r0 + n;
        const float x = im[(ok ? r : r0) * 64 + lane];
        nb += (ok ? wgt[j] : 0.f) * x;
    }
    return nb;
}

// slot range of ball(v), clamped into [0, ns_cap] (an unusable range is empty)
__device__ __forceinline__ void logm_ball(const int32_t *__restrict__ ego_ptr, int64_t v,
                                          int64_t ns_cap, int64_t &b0, int64_t &b1) {
    b0 = ego_ptr[v];
    b1 = ego_ptr[v + 1];
    if (b0 < 0 || b1 > ns_cap || b0 > b1) b0 = b1 = 0;
}

__global__ __launch_bounds__(256) void recon_logm_sparse_fwd_k(
    const float *__restrict__ im, const int32_t *__restrict__ gptr, int64_t ncap,
    const int32_t *__restrict__ ego_ptr, const int32_t *__restrict__ ego_nodes, int64_t ns_cap,
    const float *__restrict__ s_in, float *__restrict__ gram, double *__restrict__ parts,
    const int32_t *__restrict__ dims) {
    const int64_t g = blockIdx.x;
    const int y = blockIdx.y, T = gridDim.y - 1;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t nlive = eff_count(dims, 0, ncap);
    double *out = parts + g * (T + 1) + y;
    int64_t r0;
    int n;
    if (!logm_rows(gptr, g, nlive, r0, n)) {  // block-uniform
        if (threadIdx.x == 0) *out = 0.0;
        return;
    }
    __shared__ double wred[4];
    double part = 0.0;
    if (y == 0) {
        const int ta = w >> 1, tb = w & 1;
        const int kk = lane >> 5, ch = lane & 31;
        const int64_t re = r0 + n;
        f32x16 acc;
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[i] = 0.f;
        int64_t r = r0;
        for (; r + 8 <= re; r += 8) {
            float a[4], b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int64_t row = r + 2 * q + kk;
                a[q] = im[row * 64 + ta * 32 + ch];
                b[q] = im[row * 64 + tb * 32 + ch];
            }
#pragma unroll
            for (int q = 0; q < 4; ++q)
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[q], b[q], acc, 0, 0, 0);
        }
        for (; r < re; r += 2) {
            const int64_t row = r + kk;
            const bool ok = row < re;
            const float a = ld_ok(im, row * 64 + ta * 32 + ch, r0 * 64, ok, 0.f);
            const float b = ld_ok(im, row * 64 + tb * 32 + ch, r0 * 64, ok, 0.f);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
        }
        float *G = gram + g * kGram;
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const int row = (j & 3) + 8 * (j >> 2) + 4 * (lane >> 5);
            G[(ta * 32 + row) * 64 + tb * 32 + (lane & 31)] = acc[j];
            part += static_cast<double>(acc[j]) * static_cast<double>(acc[j]);
        }
    } else {
        for (int cb = (y - 1) * 64; cb < n; cb += T * 64) {
            const int ce = cb + 64 < n ? cb + 64 : n;
            for (int c = cb + w; c < ce; c += 4) {
                int64_t b0, b1;
                logm_ball(ego_ptr, r0 + c, ns_cap, b0, b1);
                const float nb = logm_ball_row(im, ego_nodes, s_in, b0, b1, r0, n, lane);
                const float p = im[(r0 + c) * 64 + lane] * nb;
                part += static_cast<double>(p);  // per lane; lanes summed below
            }
        }
    }
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) part += __shfl_xor(part, off, kWave);
    if (lane == 0) wred[w] = part;
    __syncthreads();
    if (threadIdx.x == 0) *out = ((wred[0] + wred[1]) + wred[2]) + wred[3];
}

__global__ __launch_bounds__(256) void recon_logm_sparse_fin_k(
    const int32_t *__restrict__ gptr, int64_t n_graphs, int64_t ncap,
    const double *__restrict__ parts, int T, const double *__restrict__ C, int kstep,
    float *__restrict__ lossg, const int32_t *__restrict__ dims) {
    const int64_t g = static_cast<int64_t>(blockIdx.x) * 256 + threadIdx.x;
    if (g >= n_graphs) return;
    const int64_t nlive = eff_count(dims, 0, ncap);
    int64_t r0;
    int n;
    if (!logm_rows(gptr, g, nlive, r0, n)) {
        lossg[g] = 0.f;
        return;
    }
    const double *p = parts + g * (T + 1);
    double dot = 0.0;
    for (int y = 1; y <= T; ++y) dot += p[y];
    const double k = static_cast<double>(kstep), nn = static_cast<double>(n);
    lossg[g] = static_cast<float>((k * p[0] - 2.0 * dot + C[g]) / (k * nn * nn));
}

__global__ __launch_bounds__(256) void recon_logm_sparse_bwd_k(
    const float *__restrict__ im, const int32_t *__restrict__ gptr, int64_t n_graphs,
    int64_t ncap, const int32_t *__restrict__ ego_ptr, const int32_t *__restrict__ ego_nodes,
    int64_t ns_cap, const float *__restrict__ s_sym, const float *__restrict__ gram, int kstep,
    const float *__restrict__ g_loss, float *__restrict__ grad,
    const int32_t *__restrict__ dims) {
    const int y = blockIdx.y, T = gridDim.y;
    const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int64_t nlive = eff_count(dims, 0, ncap);
    if (static_cast<int64_t>(blockIdx.x) == n_graphs) {  // rows past the live N: zero
        for (int64_t v = nlive + y * 4 + w; v < ncap; v += 4 * T) grad[v * 64 + lane] = 0.f;
        return;
    }
    const int64_t g = blockIdx.x;
    int64_t r0;
    int n;
    if (!logm_rows(gptr, g, nlive, r0, n)) {  // block-uniform
        // an unusable molecule (flagged by the target build): zero its rows
        const int64_t a = gptr[g], b = gptr[g + 1];
        if (a >= 0 && b <= nlive)
            for (int64_t v = a + y * 4 + w; v < b; v += 4 * T) grad[v * 64 + lane] = 0.f;
        return;
    }
    if (y * 64 >= n) return;
    __shared__ float sg[kGram];
    __shared__ float srow[4][64];
    const float *G = gram + g * kGram;
    for (int i = threadIdx.x; i < kGram; i += 256) sg[i] = G[i];
    __syncthreads();
    const double kd = static_cast<double>(kstep), nn = static_cast<double>(n);
    const float coef = static_cast<float>(static_cast<double>(*g_loss) / (kd * nn * nn));
    const float k4 = 4.f * static_cast<float>(kstep);
    for (int cb = y * 64; cb < n; cb += T * 64) {
        const int ce = cb + 64 < n ? cb + 64 : n;
        for (int c = cb + w; c < ce; c += 4) {
            const int64_t v = r0 + c;
            srow[w][lane] = im[v * 64 + lane];
            __builtin_amdgcn_wave_barrier();
            float acc = 0.f;
#pragma unroll 16
            for (int k = 0; k < 64; ++k) acc += srow[w][k] * sg[k * 64 + lane];
            int64_t b0, b1;
            logm_ball(ego_ptr, v, ns_cap, b0, b1);
            const float nb = logm_ball_row(im, ego_nodes, s_sym, b0, b1, r0, n, lane);
            grad[v * 64 + lane] = coef * (k4 * acc - 2.f * nb);
            __builtin_amdgcn_wave_barrier();
        }
    }
}

}  // namespace scgib

using namespace scgib;

extern "C" int64_t scgib_logm_max_k(void) { return kLogmMaxK; }
extern "C" int64_t scgib_logm_max_graph_nodes(void) { return kLogmMaxNodes; }
extern "C" int64_t scgib_recon_logm_sparse_parts(int64_t max_graph_nodes) {
    return 1 + logm_chunks(max_graph_nodes);
}

extern "C" int scgib_logm_targets(const int32_t *rowptr, const int32_t *col,
                                  const int32_t *graph_ptr, int64_t n_graphs, int64_t n_nodes,
                                  int64_t n_edges, const int32_t *ego_ptr,
                                  const int32_t *ego_nodes, int64_t n_ego, int32_t kstep,
                                  uint32_t *counts, float *s_in, float *s_sym, double *C,
                                  int32_t *err, const int32_t *dims, scgib_stream_t stream) {
    if (n_graphs <= 0 || n_nodes <= 0 || n_edges < 0 || n_ego <= 0 || kstep <= 0)
        return SCGIB_EINVAL;
    if (!rowptr || (n_edges > 0 && !col) || !graph_ptr || !ego_ptr || !ego_nodes || !counts ||
        !s_in || !s_sym || !C || !err)
        return SCGIB_EINVAL;
    if (kstep > kLogmMaxK || n_graphs > 0x7fffffff || n_ego > 0x7fffffff)
        return SCGIB_EUNSUPPORTED;
    logm_targets_k<<<static_cast<unsigned>(n_graphs), 256, 0, as_stream(stream)>>>(
        rowptr, col, graph_ptr, n_nodes, n_edges, ego_ptr, ego_nodes, n_ego, kstep, counts, s_in,
        s_sym, C, err, dims);
    return launch_status();
}

extern "C" int scgib_recon_logm_sparse_fwd(const float *im, const int32_t *graph_ptr,
                                           int64_t n_graphs, int64_t n_nodes,
                                           const int32_t *ego_ptr, const int32_t *ego_nodes,
                                           int64_t n_ego, const float *s_in, const double *C,
                                           int32_t kstep, int64_t max_graph_nodes, float *gram,
                                           double *parts, float *loss_graphs, float *loss,
                                           const int32_t *dims, scgib_stream_t stream) {
    if (n_graphs <= 0 || n_nodes <= 0 || n_ego <= 0 || kstep <= 0 || max_graph_nodes <= 0)
        return SCGIB_EINVAL;
    if (!im || !graph_ptr || !ego_ptr || !ego_nodes || !s_in || !C || !gram || !parts ||
        !loss_graphs || !loss)
        return SCGIB_EINVAL;
    if (n_graphs > 0x7fffffff || n_ego > 0x7fffffff) return SCGIB_EUNSUPPORTED;
    hipStream_t st = as_stream(stream);
    const int T = logm_chunks(max_graph_nodes);
    recon_logm_sparse_fwd_k<<<dim3(static_cast<unsigned>(n_graphs), T + 1), 256, 0, st>>>(
        im, graph_ptr, n_nodes, ego_ptr, ego_nodes, n_ego, s_in, gram, parts, dims);
    recon_logm_sparse_fin_k<<<static_cast<unsigned>((n_graphs + 255) / 256), 256, 0, st>>>(
        graph_ptr, n_graphs, n_nodes, parts, T, C, kstep, loss_graphs, dims);
    const int rc = launch_status();
    if (rc != SCGIB_OK) return rc;
    return launch_slab_reduce(loss_graphs, static_cast<int>(n_graphs), 1, loss, st);
}

extern "C" int scgib_recon_logm_sparse_bwd(const float *im, const int32_t *graph_ptr,
                                           int64_t n_graphs, int64_t n_nodes,
                                           const int32_t *ego_ptr, const int32_t *ego_nodes,
                                           int64_t n_ego, const float *s_sym, const float *gram,
                                           int32_t kstep, int64_t max_graph_nodes,
                                           const float *g_loss, float *grad_im,
                                           const int32_t *dims, scgib_stream_t stream) {
    if (n_graphs <= 0 || n_nodes <= 0 || n_ego <= 0 || kstep <= 0 || max_graph_nodes <= 0)
        return SCGIB_EINVAL;
    if (!im || !graph_ptr || !ego_ptr || !ego_nodes || !s_sym || !gram || !g_loss || !grad_im)
        return SCGIB_EINVAL;
    if (n_graphs >= 0x7fffffff || n_ego > 0x7fffffff) return SCGIB_EUNSUPPORTED;
    const int T = logm_chunks(max_graph_nodes);
    recon_logm_sparse_bwd_k<<<dim3(static_cast<unsigned>(n_graphs + 1), T), 256, 0,
                              as_stream(stream)>>>(im, graph_ptr, n_graphs, n_nodes, ego_ptr,
                                                   ego_nodes, n_ego, s_sym, gram, kstep, g_loss,
                                                   grad_im, dims);
    return launch_status();
}
