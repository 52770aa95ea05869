#pragma once
#include "mfma_tile.h"
#include "running_update.h"

namespace scgib {

// ---------------------------------------------------------------------------
// BatchNorm finalize folded into the producing tile kernel (training mode).
// Hierarchical last-arriver: the tiles of a layer arrive in groups of kGroup; the
// last tile of a group combines the group's 16 tile statistics (fp64) into a
// group partial, then arrives at the layer counter; the last group combines
// the groups and writes the BN record / coefficients.  Two short load rounds
// at the tail of the kernel replace a separate 1-workgroup finalize launch.
// Fixed combination order -> deterministic.  Counters: caller-provided, zero
// on entry; each is reset by its last arriver (graph-replay safe).
// ---------------------------------------------------------------------------
// tiles per BatchNorm statistics group (8 / 32 / 64 measured +1 %, round 1)
constexpr int kGroup = 16;
static_assert(kGroup % 4 == 0 && kGroup <= 64, "group combine: 4 partitions, <= 16 loads each");

struct BnFwdFuse {          // gin_fwd_k: BN statistics + running update
    unsigned *counters;     // [ngr_cap + 1]; nullptr: not fused (separate finalize)
    double *gpart;          // [ngr_cap][128]: group sum, group centred M2
    const float *gamma, *beta;
    float *rmean, *rvar, *stat;
    int64_t *nbt;
    float eps, momentum;
    int ngr_cap;
    int defer;              // stop at the group partials (the consumer finishes)
};

struct BnBwdFuse {          // gin_bwd_stats_k: dgamma, dbeta, dz2 coefficients
    unsigned *counters;
    double *gpart;          // [ngr_cap][128]: group sum dy, group sum dy * xhat
    float *dgamma, *dbeta, *coef;
    int training, ngr_cap;
    int defer;
};

// Cross-workgroup exchange: st_agent / ld_agent / block_arrive (common.h).

// rows of tile t / group g of an n-row layer
__device__ __forceinline__ double rows_in(int64_t n, int64_t first, int64_t span) {
    const int64_t r = n - first;
    return static_cast<double>(r < span ? r : span);
}

// Layer statistics from the ngr group partials (fp64, fixed order; 256
// threads, channel c = tid & 63, partition p = tid >> 6 takes groups p, p + 4,
// ...; one load round while ngr <= 64).  Every thread returns its channel's
// mean and centred M2:  M2 = sum_g [M2_g + (S_g - n_g mean)^2 / n_g].
// AGENT: the partials were written earlier in this kernel (agent-scope loads);
// otherwise by a previous kernel (plain loads: L2-cached after the first
// workgroup of an XCD, coherent across the kernel boundary).
template <bool AGENT>
__device__ __forceinline__ double ld_part(const double *p) {
    if constexpr (AGENT) return ld_agent(p);
    else return *p;
}

// Barrier-free layer combine (wave-local shuffles, no LDS): lane l of wave w
// owns channel c = 16 w + (l & 15) and partition p = l >> 4, which takes
// groups p, p + 4, ... (fp64, fixed order); the four partitions combine as
// (p0 + p1) + (p2 + p3) through two xor shuffles (identical in every lane).
// Split into the load (issue early, registers) and the combine, so other
// loads can be in flight meanwhile; one load round for ngr <= kFinG.  (8:
// the QM9 B512 ego layers' 28 groups in one round, and 32 fewer VGPRs than
// 16 in the forward kernel, which then keeps its first neighbour-index round
// in flight across the finish)
constexpr int kFinR = 8, kFinG = 4 * kFinR;
// backward consumers: 2 partitions x kBFinR groups per load round
constexpr int kBFinR = 16;
// past one round of 64 groups the last-arriver statistics take a third
// level: 64-group supergroups (bn_fwd_hier / bn_bwd_hier)
constexpr int kSuper = 64;

struct FwdFin {
    double vs[kFinR], vq[kFinR];
};

__device__ __forceinline__ int fin_channel() { return 16 * (threadIdx.x >> 6) + (threadIdx.x & 15); }

template <bool AGENT>
__device__ __forceinline__ void bn_fwd_fin_load(const double *__restrict__ gpart, int ngr, int g0,
                                                FwdFin &f) {
    const int c = fin_channel(), p = (threadIdx.x & 63) >> 4;
#pragma unroll
    for (int u = 0; u < kFinR; ++u) {
        if (g0 + 4 * u < ngr) {  // wave-uniform: only rounds with a live group are loaded
            const int64_t gg = g0 + p + 4 * u < ngr ? g0 + p + 4 * u : 0;  // group 0 always exists
            f.vs[u] = ld_part<AGENT>(gpart + gg * 128 + c);
            f.vq[u] = ld_part<AGENT>(gpart + gg * 128 + 64 + c);
        }
    }
}

__device__ __forceinline__ double quad_sum(double a) {
    a = a + __shfl_xor(a, 16, kWave);
    return a + __shfl_xor(a, 32, kWave);
}

// mean and centred M2 of channel fin_channel():
//   mean = sum_g S_g / n,  M2 = sum_g [M2_g + (S_g - n_g mean)^2 / n_g]
// n_g = kGroup * 64 for every group but possibly the last, and dividing by a power
// of two equals multiplying by its reciprocal exactly, so only the last
// group's term (added last by its owner, the same order) divides.
// UNIT: rows of every entry but possibly the last (kGroup tiles; a 64-group
// supergroup at the third level of bn_fwd_hier).  S (or nullptr): the sum.
template <bool AGENT, int64_t UNIT = int64_t(kGroup) * TM>
__device__ void bn_fwd_final(const double *__restrict__ gpart, int64_t n, int ngr, FwdFin &f,
                             double &mean, double &M2, double *S = nullptr) {
    constexpr double kFull = static_cast<double>(UNIT), kInvFull = 1.0 / kFull;
    const int p = (threadIdx.x & 63) >> 4;
    double a = 0.0;
    for (int g0 = 0; g0 < ngr; g0 += kFinG) {
        if (g0 > 0) bn_fwd_fin_load<AGENT>(gpart, ngr, g0, f);
#pragma unroll
        for (int u = 0; u < kFinR; ++u)
            if (g0 + 4 * u < ngr) a += g0 + p + 4 * u < ngr ? f.vs[u] : 0.0;
    }
    const double sum = quad_sum(a);
    if (S) *S = sum;
    mean = sum / static_cast<double>(n);
    const int glast = ngr - 1;
    const double nlast = rows_in(n, int64_t(glast) * UNIT, UNIT);
    const bool last_partial = nlast != kFull;
    double q = 0.0, last_vq = 0.0, last_d = 0.0;
    bool owns_last = false;
    for (int g0 = 0; g0 < ngr; g0 += kFinG) {
        if (ngr > kFinG) bn_fwd_fin_load<AGENT>(gpart, ngr, g0, f);  // else still in registers
#pragma unroll
        for (int u = 0; u < kFinR; ++u) {
            if (g0 + 4 * u < ngr) {
                const int g = g0 + p + 4 * u;
                if (g < ngr) {
                    if (g == glast && last_partial) {
                        owns_last = true;
                        last_vq = f.vq[u];
                        last_d = f.vs[u] - nlast * mean;
                    } else {
                        const double d = f.vs[u] - kFull * mean;
                        q += f.vq[u] + d * d * kInvFull;
                    }
                }
            }
        }
    }
    if (owns_last) q += last_vq + last_d * last_d / nlast;
    M2 = quad_sum(q);
}

// BN record of channel c from (mean, M2): returns scale / shift; with
// `write`, also the [4][64] record and the running-statistics update
// (momentum, unbiased variance, num_batches_tracked += 1).
// (gamma_c / beta_c are passed as values: load them early, a dependent
// global load here costs a full memory latency)
__device__ __forceinline__ float2 bn_fwd_publish(int c, double mean, double M2, int64_t n,
                                                 float gamma_c, float beta_c,
                                                 float eps, float momentum, float *rmean,
                                                 float *rvar, int64_t *nbt, float *stat,
                                                 bool write) {
    const double var = M2 / static_cast<double>(n);
    if (write && rmean) {
        rmean[c] = static_cast<float>((1.0 - momentum) * rmean[c] + momentum * mean);
        rvar[c] = static_cast<float>((1.0 - momentum) * rvar[c] +
                                     momentum * (n > 1 ? M2 / static_cast<double>(n - 1) : M2));
        if (c == 0 && nbt) *nbt += 1;
    }
    const double istd = 1.0 / sqrt(var + static_cast<double>(eps));
    const double sc = gamma_c * istd;
    const float scale = static_cast<float>(sc), shift = static_cast<float>(beta_c - mean * sc);
    if (write) {
        stat[c] = static_cast<float>(mean);
        stat[64 + c] = static_cast<float>(istd);
        stat[128 + c] = scale;
        stat[192 + c] = shift;
    }
    return make_float2(scale, shift);
}

// A consumer of a deferred layer (scgib_bn_pending) that is not a GIN layer
// (the encoder output's BN + ReLU): every 256-thread workgroup finishes the
// statistics from the group partials; workgroup 0 writes the record and the
// running update.  sSS[c] = scale, sSS[64 + c] = shift.  Call from all
// threads, before any early return.
// Split into the loads (bn_pending_load: the first round of group partials,
// gamma and beta — issue it first, then the caller's own independent loads)
// and the finish, so a tile kernel keeps its rows in flight across the finish.
struct PendFin {
    FwdFin fin;
    float gam, bet;
};

__device__ __forceinline__ int pending_groups(int64_t n) {
    return static_cast<int>(((n + TM - 1) / TM + kGroup - 1) / kGroup);
}

__device__ __forceinline__ void bn_pending_load(const scgib_bn_pending &pend, int64_t n,
                                                PendFin &r) {
    const int fc = fin_channel();
    r.gam = pend.gamma[fc];
    r.bet = pend.beta[fc];
    bn_fwd_fin_load<false>(pend.gpart, pending_groups(n), 0, r.fin);
}

__device__ __forceinline__ void bn_pending_finish(const scgib_bn_pending &pend, int64_t n,
                                                  PendFin &r, float *sSS) {
    const int fc = fin_channel();
    double mean, M2;
    bn_fwd_final<false>(pend.gpart, n, pending_groups(n), r.fin, mean, M2);
    const bool lead = (threadIdx.x & 63) < 16;
    const float2 ss = bn_fwd_publish(fc, mean, M2, n, r.gam, r.bet, pend.eps, pend.momentum,
                                     pend.running_mean, pend.running_var,
                                     pend.num_batches_tracked, pend.stat, blockIdx.x == 0 && lead);
    if (lead) {
        sSS[fc] = ss.x;
        sSS[64 + fc] = ss.y;
    }
    __syncthreads();
}

__device__ __forceinline__ void bn_pending_finish(const scgib_bn_pending &pend, int64_t n,
                                                  float *sSS) {
    PendFin r;
    bn_pending_load(pend, n, r);
    bn_pending_finish(pend, n, r, sSS);
}

// 256 threads: channel c = tid & 63, partition p = tid >> 6 (4 partitions).
// Per-tile (S, M2) -> group (S_g, M2_g) -> layer (mean, M2); exact
// decomposition M2 = sum_b [M2_b + (S_b - n_b mean)^2 / n_b] at each level.
// arrivals = tiles of group g whose statistics this workgroup contributes
// (1 per tile kernel; a workgroup running several tiles of one group may
// arrive for all of them at once)
__device__ void bn_fwd_hier(const float *__restrict__ part, int64_t n, int64_t tile,
                            const BnFwdFuse &fz, unsigned arrivals = 1u) {
    const int64_t nt = (n + TM - 1) / TM;
    const int ngr = static_cast<int>((nt + kGroup - 1) / kGroup);
    const int g = static_cast<int>(tile / kGroup);
    const int gsize = static_cast<int>(nt - int64_t(g) * kGroup < kGroup ? nt - int64_t(g) * kGroup : kGroup);
    if (!block_arrive(&fz.counters[g], gsize, arrivals)) return;
    const int c = threadIdx.x & 63, p = threadIdx.x >> 6;
    __shared__ double sh[4][64];
    __shared__ double smean[64];
    {   // group combine: partition p takes tiles g*kGroup + p + 4u
        constexpr int U = kGroup / 4;
        float S[U], Q[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int64_t t = int64_t(g) * kGroup + p + 4 * u;
            const int64_t tc = p + 4 * u < gsize ? t : int64_t(g) * kGroup;
            S[u] = ld_agent(part + tc * 128 + c);
            Q[u] = ld_agent(part + tc * 128 + 64 + c);
        }
        double a = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) a += p + 4 * u < gsize ? static_cast<double>(S[u]) : 0.0;
        sh[p][c] = a;
        __syncthreads();
        if (p == 0) {
            const double sg = ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c];
            smean[c] = sg / rows_in(n, int64_t(g) * kGroup * TM, kGroup * TM);
            st_agent(fz.gpart + int64_t(g) * 128 + c, sg);
        }
        __syncthreads();
        const double mg = smean[c];
        double q = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) {
            if (p + 4 * u < gsize) {
                const int64_t t = int64_t(g) * kGroup + p + 4 * u;
                const double nb = rows_in(n, t * TM, TM);
                const double d = static_cast<double>(S[u]) - nb * mg;
                q += static_cast<double>(Q[u]) + d * d / nb;
            }
        }
        __syncthreads();
        sh[p][c] = q;
        __syncthreads();
        if (p == 0) st_agent(fz.gpart + int64_t(g) * 128 + 64 + c, ((sh[0][c] + sh[1][c]) + sh[2][c]) + sh[3][c]);
        if (threadIdx.x == 0) fz.counters[g] = 0u;
    }
    if (fz.defer) return;  // the consumer kernel finishes (bn_fwd_final there)
    double mean, M2;
    FwdFin fin;
    if (ngr > kSuper) {  // block-uniform
        // more groups than one load round: a third level, so that no single
        // workgroup walks every group partial in series at the end of the
        // kernel (1172 groups at 1.2 M rows: ~74 us of dependent load rounds).
        // The last group of each 64-group supergroup combines its groups
        // (one round), the last supergroup combines the supergroups.
        constexpr int64_t kSupRows = int64_t(kSuper) * kGroup * TM;
        const int s = g / kSuper, nsup = (ngr + kSuper - 1) / kSuper;
        const int ssize = ngr - s * kSuper < kSuper ? ngr - s * kSuper : kSuper;
        unsigned *scnt = &fz.counters[fz.ngr_cap + 1 + s];
        if (!block_arrive(scnt, ssize)) return;
        const double *gp = fz.gpart + int64_t(s) * kSuper * 128;
        double *sp = fz.gpart + int64_t(fz.ngr_cap) * 128;
        const int64_t ns = static_cast<int64_t>(rows_in(n, s * kSupRows, kSupRows));
        double S;
        bn_fwd_fin_load<true>(gp, ssize, 0, fin);
        bn_fwd_final<true>(gp, ns, ssize, fin, mean, M2, &S);
        if ((threadIdx.x & 63) < 16) {
            st_agent(sp + int64_t(s) * 128 + fin_channel(), S);
            st_agent(sp + int64_t(s) * 128 + 64 + fin_channel(), M2);
        }
        if (threadIdx.x == 0) *scnt = 0u;
        if (!block_arrive(&fz.counters[fz.ngr_cap], nsup)) return;
        const float gam = fz.gamma[fin_channel()], bet = fz.beta[fin_channel()];
        bn_fwd_fin_load<true>(sp, nsup, 0, fin);
        bn_fwd_final<true, kSupRows>(sp, n, nsup, fin, mean, M2);
        bn_fwd_publish(fin_channel(), mean, M2, n, gam, bet, fz.eps, fz.momentum, fz.rmean,
                       fz.rvar, fz.nbt, fz.stat, (threadIdx.x & 63) < 16);
        if (threadIdx.x == 0) fz.counters[fz.ngr_cap] = 0u;
        return;
    }
    if (!block_arrive(&fz.counters[fz.ngr_cap], ngr)) return;
    const float gam = fz.gamma[fin_channel()], bet = fz.beta[fin_channel()];
    bn_fwd_fin_load<true>(fz.gpart, ngr, 0, fin);
    bn_fwd_final<true>(fz.gpart, n, ngr, fin, mean, M2);
    bn_fwd_publish(fin_channel(), mean, M2, n, gam, bet, fz.eps, fz.momentum, fz.rmean,
                   fz.rvar, fz.nbt, fz.stat, (threadIdx.x & 63) < 16);
    if (threadIdx.x == 0) fz.counters[fz.ngr_cap] = 0u;
}

// Layer sums (dbeta | dgamma, 128 values) from the ngr group partials,
// barrier-free: lane l of wave w owns sum index cs = 32 w + (l & 31) and
// partition p = l >> 5 (groups p, p + 2, ...); p0 + p1 via one xor shuffle.
struct BwdFin {
    double v[kBFinR];
};

__device__ __forceinline__ int bfin_index() { return 32 * (threadIdx.x >> 6) + (threadIdx.x & 31); }

template <bool AGENT>
__device__ __forceinline__ void bn_bwd_fin_load(const double *__restrict__ gpart, int ngr, int g0,
                                                BwdFin &f) {
    const int cs = bfin_index(), p = (threadIdx.x & 63) >> 5;
#pragma unroll
    for (int u = 0; u < kBFinR; ++u) {
        if (g0 + 2 * u < ngr) {  // wave-uniform
            const int64_t gg = g0 + p + 2 * u < ngr ? g0 + p + 2 * u : 0;  // group 0 always exists
            f.v[u] = ld_part<AGENT>(gpart + gg * 128 + cs);
        }
    }
}

template <bool AGENT>
__device__ double bn_bwd_final(const double *__restrict__ gpart, int ngr, BwdFin &f) {
    const int p = (threadIdx.x & 63) >> 5;
    double a = 0.0;
    for (int g0 = 0; g0 < ngr; g0 += 2 * kBFinR) {
        if (g0 > 0) bn_bwd_fin_load<AGENT>(gpart, ngr, g0, f);
#pragma unroll
        for (int u = 0; u < kBFinR; ++u)
            if (g0 + 2 * u < ngr) a += g0 + p + 2 * u < ngr ? f.v[u] : 0.0;
    }
    return a + __shfl_xor(a, 32, kWave);
}

// dbeta = sum dy (c < 64), dgamma = sum dy xhat (c >= 64); dz2 coefficient
// coef[c] = tot / N in training (0 in eval); coef may be nullptr
__device__ __forceinline__ float bn_bwd_publish(int c, double tot, int64_t n, int training,
                                                float *dgamma, float *dbeta, float *coef) {
    const float cf = training ? static_cast<float>(tot / static_cast<double>(n)) : 0.f;
    if (dbeta) {
        if (c < 64) dbeta[c] = static_cast<float>(tot);
        else dgamma[c - 64] = static_cast<float>(tot);
    }
    if (coef) coef[c] = cf;
    return cf;
}

// The finish of a deferred BN backward (pend.gpart set) in the layer-backward
// kernel that consumes it: every workgroup sums the ngr group partials (f:
// loaded by bn_bwd_fin_load<false> at kernel entry) into sCoef[128] = c1 | c2;
// workgroup 0 also writes dgamma / dbeta.  The caller's barrier follows.
__device__ __forceinline__ void bn_bwd_pending_finish(const scgib_bn_bwd_pending &pend, int ngr,
                                                      int64_t n, BwdFin &f, float *sCoef) {
    const double tot = bn_bwd_final<false>(pend.gpart, ngr, f);
    const int cs = bfin_index();
    const int tid = threadIdx.x;
    const bool lead = (tid & 63) < 32, w0 = blockIdx.x == 0 && lead;
    const float cf = bn_bwd_publish(cs, tot, n, pend.training, w0 ? pend.dgamma : nullptr,
                                    w0 ? pend.dbeta : nullptr, nullptr);
    if (lead) sCoef[cs] = cf;
}

// backward: tile (sum dy, sum dy xhat) -> group -> layer sums (fp64);
// sh: 2 KB of LDS scratch (the caller's, so a kernel near its LDS limit can
// lend a dead tile image)
// (group g, `count` of its tiles arriving at once: gin_bwd_statsz_k's walk)
__device__ __forceinline__ void bn_bwd_hier_gs(const float *__restrict__ part, int64_t n, int g, unsigned count,
                               const BnBwdFuse &bz, double (*sh)[128]) {
    const int64_t nt = (n + TM - 1) / TM;
    const int ngr = static_cast<int>((nt + kGroup - 1) / kGroup);
    const int gsize = static_cast<int>(nt - int64_t(g) * kGroup < kGroup ? nt - int64_t(g) * kGroup : kGroup);
    if (!block_arrive(&bz.counters[g], gsize, count)) return;
    const int c = threadIdx.x & 127, p = threadIdx.x >> 7;  // 128 sums x 2 partitions
    {
        constexpr int U = kGroup / 2;
        float v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int k = p + 2 * u;
            v[u] = ld_agent(part + (int64_t(g) * kGroup + (k < gsize ? k : 0)) * 128 + c);
        }
        double a = 0.0;
#pragma unroll
        for (int u = 0; u < U; ++u) a += p + 2 * u < gsize ? static_cast<double>(v[u]) : 0.0;
        sh[p][c] = a;
        __syncthreads();
        if (p == 0) st_agent(bz.gpart + int64_t(g) * 128 + c, sh[0][c] + sh[1][c]);
        if (threadIdx.x == 0) bz.counters[g] = 0u;
    }
    if (bz.defer) return;  // the layer's gin_bwd_k finishes (bn_bwd_final there)
    BwdFin fin;
    if (ngr > kSuper) {  // block-uniform: the third level, as in bn_fwd_hier
        const int s = g / kSuper, nsup = (ngr + kSuper - 1) / kSuper;
        const int ssize = ngr - s * kSuper < kSuper ? ngr - s * kSuper : kSuper;
        unsigned *scnt = &bz.counters[bz.ngr_cap + 1 + s];
        if (!block_arrive(scnt, ssize)) return;
        const double *gp = bz.gpart + int64_t(s) * kSuper * 128;
        double *sp = bz.gpart + int64_t(bz.ngr_cap) * 128;
        bn_bwd_fin_load<true>(gp, ssize, 0, fin);
        const double st = bn_bwd_final<true>(gp, ssize, fin);
        if ((threadIdx.x & 63) < 32) st_agent(sp + int64_t(s) * 128 + bfin_index(), st);
        if (threadIdx.x == 0) *scnt = 0u;
        if (!block_arrive(&bz.counters[bz.ngr_cap], nsup)) return;
        bn_bwd_fin_load<true>(sp, nsup, 0, fin);
        const double tot = bn_bwd_final<true>(sp, nsup, fin);
        if ((threadIdx.x & 63) < 32)
            bn_bwd_publish(bfin_index(), tot, n, bz.training, bz.dgamma, bz.dbeta, bz.coef);
        if (threadIdx.x == 0) bz.counters[bz.ngr_cap] = 0u;
        return;
    }
    if (!block_arrive(&bz.counters[bz.ngr_cap], ngr)) return;
    bn_bwd_fin_load<true>(bz.gpart, ngr, 0, fin);
    const double tot = bn_bwd_final<true>(bz.gpart, ngr, fin);
    if ((threadIdx.x & 63) < 32)
        bn_bwd_publish(bfin_index(), tot, n, bz.training, bz.dgamma, bz.dbeta, bz.coef);
    if (threadIdx.x == 0) bz.counters[bz.ngr_cap] = 0u;
}

__device__ void bn_bwd_hier_s(const float *__restrict__ part, int64_t n, int64_t tile,
                              const BnBwdFuse &bz, double (*sh)[128]) {
    bn_bwd_hier_gs(part, n, static_cast<int>(tile / kGroup), 1u, bz, sh);
}

__device__ void bn_bwd_hier(const float *__restrict__ part, int64_t n, int64_t tile,
                            const BnBwdFuse &bz) {
    __shared__ double sh[2][128];
    bn_bwd_hier_s(part, n, tile, bz, sh);
}

}  // namespace scgib
