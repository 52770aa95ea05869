/* scgib.h — C-ABI of the MI355X-native S-CGIB hot path (libscgib.so).
 *
 * The reference (O-JounLee/S-CGIB) is pure Python on PyTorch + DGL and has no
 * FFI of its own; each entry point below replaces the
 * library kernel the reference reaches through DGL / torch at the cited line.
 * The Python host mirror (s-cgib_amd/ops.py, models.py) binds them with
 * ctypes; INTEGRATION.md shows the binding.
 *
 * Conventions (every function):
 *   - all pointers are DEVICE pointers (hipMalloc / torch CUDA tensors),
 *     caller-allocated; indices int32, features fp32 row-major;
 *   - `stream` is a hipStream_t (NULL = legacy default stream); every launch
 *     is asynchronous on it, nothing synchronises, nothing allocates — so a
 *     caller may capture any of them into a HIP graph;
 *   - return 0 (SCGIB_OK), a negative SCGIB_E* argument error, or a positive
 *     hipError_t from the launch; nothing throws across the ABI;
 *   - deterministic: no floating-point atomics; every reduction has a fixed
 *     order for a given shape;
 *   - capacity mode (HIP-graph replay): functions taking `const int32_t *dims`
 *     accept it NULL (the host sizes are exact) or a DEVICE array with the
 *     actual counts, dims[0] = nodes (or segments), dims[1] = edges, each <=
 *     the host size, which then only sizes the launch.  Rows past the actual
 *     count are written as zeros, so capacity-padded buffers stay finite and
 *     one captured graph serves every batch that fits.
 */
#ifndef SCGIB_H
#define SCGIB_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef void *scgib_stream_t; /* hipStream_t */

/* Deferred BatchNorm finalize (training, fused layers).  A layer launched
 * with defer = 1 leaves its batch statistics as group partials in its bn_ws
 * (at scgib_gin_bn_gpart_offset(n) floats) and does not write `stat` /
 * the running statistics; the NEXT kernel that needs them finishes the
 * combination in every workgroup (workgroup 0 writes the outputs), which
 * takes the serial last-arriver tail off the layer chain.  Layers up to
 * scgib_gin_defer_max_nodes() rows. */
typedef struct {
    const double *gpart;          /* producer's bn_ws + scgib_gin_bn_gpart_offset(n) */
    const float *gamma, *beta;    /* producer layer's BatchNorm affine */
    float *running_mean, *running_var;  /* NULL: untracked */
    int64_t *num_batches_tracked;
    float *stat;                  /* producer's [4][64] record (mean, invstd, scale, shift) */
    float eps, momentum;
} scgib_bn_pending;

typedef struct {
    const double *gpart;          /* bwd-stats bn_ws + scgib_gin_bn_gpart_offset(n) */
    float *dgamma, *dbeta;        /* written by workgroup 0 of the consumer */
    int32_t training;
} scgib_bn_bwd_pending;

enum {
    SCGIB_OK = 0,
    SCGIB_EINVAL = -1,       /* null pointer / negative size / bad dim      */
    SCGIB_EUNSUPPORTED = -2, /* shape outside what the kernels implement    */
};

#define SCGIB_HIDDEN 64     /* S-CGIB hidden width (args.dims, exp_pretraining.py:386) */
#define SCGIB_STATS_STRIDE 260 /* floats per graph in the interaction stats slab */
#define SCGIB_PGRAD_STRIDE 324 /* floats per graph in the parameter-gradient slab */

int scgib_abi_version(void);
/* Cross-queue hand-off without a stream/graph dependency: `words` is four
 * zeroed uint32 shared by one producer/consumer pair.  scgib_stream_signal
 * (producer stream, after the work to hand over) counts one signal;
 * scgib_stream_wait (consumer stream) returns once a signal it has not yet
 * consumed is there, so the consumer stream's later kernels see the
 * producer's data.  Calls must pair up in order (n-th wait <-> n-th signal).
 * A wait that sees no signal for 0.2 s gives up, counts words[2] and sets the
 * sticky *fault word (fault may be NULL): the step's loss kernels
 * (scgib_mlp2_recon_fwd / _contrastive_fwd, given the same word) then
 * report a NaN loss until the caller clears it, since some kernel of that
 * step read data before it was written.  It also sets *host_fault (may be
 * NULL): a host-visible pinned word the host reads without a sync (the
 * Python mirror raises on it at the next model forward / optimizer step,
 * ops.check_handoff — the fine-tune and domain-adaptation heads' losses are
 * torch ops, and NaN scores would trip binary_cross_entropy's range assert).
 * Correctness needs the signal and the wait on queues the device runs
 * concurrently ("Cross-queue hand-offs"). */
/* The next batch of a resident pool into a static input buffer, for a
 * replayed step graph: srcs = device table of n_src device pointers (each
 * `bytes` long, bytes a multiple of 16); copies srcs[ctr[0] % n_src] to dst
 * and advances ctr[0].  ctr: two uint32, ctr[1] zero on entry (left zero). */
int scgib_pool_copy(const uint64_t *srcs, int32_t n_src, uint32_t *ctr, void *dst, int64_t bytes,
                    scgib_stream_t stream);
/* ... and, in the same launch, bytes2 (a multiple of 16) from src2 to dst2
 * (graph.EgoPrefetch: the ego-nets built for this batch during the previous
 * step, staging -> the step's ego buffers). */
int scgib_pool_copy2(const uint64_t *srcs, int32_t n_src, uint32_t *ctr, void *dst, int64_t bytes,
                     const void *src2, void *dst2, int64_t bytes2, scgib_stream_t stream);
int scgib_stream_signal(uint32_t *words, scgib_stream_t stream);
int scgib_stream_wait(uint32_t *words, uint32_t *fault, uint32_t *host_fault,
                      scgib_stream_t stream);
/* Two-lane replay of a captured step graph (ABI 21; DESIGN.md §3, "Host
 * enqueue"): hipGraphLaunch of a graph with parallel branches costs the host
 * ~2.5-3 us per node, a linear graph ~6 us in all.  scgib_graph_split takes a
 * captured hipGraph_t (`graph`; kernel nodes only, else SCGIB_EUNSUPPORTED)
 * whose DAG is at most two chains wide, assigns its nodes to two lanes along
 * the captured chains, and builds one linear graph per lane (the kernel nodes
 * copied; each cross-lane edge becomes a scgib_stream_signal /
 * scgib_stream_wait kernel pair on its own 4-uint32 slot of `words`,
 * n_slots slots, zeroed, alive as long as the split; the last 8 slots are
 * for the queue check below).  `fault` / `host_fault` are the waits' sticky
 * fault words as for scgib_stream_wait.  `stream`: the caller's stream, the
 * one every replay must use — the split's non-blocking side stream is
 * checked at creation to run on another hardware queue than it (a
 * wait / signal pair across the two; up to 8 streams tried, else
 * SCGIB_EUNSUPPORTED).  *out receives an opaque handle; info (8 int32, may be
 * NULL): captured nodes, lane-0 kernels, lane-1 kernels, hand-offs added,
 * lane-0 nodes, lane-1 nodes, nodes serialised beyond two chains, slots used.
 * The captured graph's memory must stay alive while the split is used.
 * scgib_graph_split_launch replays lane 0 on `stream` (the creation stream,
 * else SCGIB_EINVAL) and lane 1 on the side stream, with one launch's stream
 * semantics: ordered after earlier work on `stream`, later work on `stream`
 * ordered after both lanes (the side stream waits, through an event recorded
 * at each launch, for the earlier work on `stream`, however long its queue).
 * scgib_graph_split_destroy waits for both lanes of the last replay and
 * frees the split. */
int scgib_graph_split(void *graph, uint32_t *words, int32_t n_slots, uint32_t *fault,
                      uint32_t *host_fault, scgib_stream_t stream, void **out, int32_t *info);
int scgib_graph_split_launch(void *split, scgib_stream_t stream);
/* The lane plan scgib_graph_split makes, on the host alone (no device): n
 * nodes, m edges from[k] -> to[k], n_hidden in-graph hand-off pairs
 * (signal node -> wait node).  Per node (n int32 each, may be NULL): lane,
 * position in it, the slot of the wait placed before it and of the signal
 * placed after it (-1: none); info (4 int32): slots, the start hand-off's
 * slot (a signal before lane 0's first node, a wait before lane 1's), the
 * end hand-off's slot (a signal after lane 1's last node, a wait after lane
 * 0's last), nodes serialised beyond two chains (-1: no such hand-off).
 * SCGIB_EUNSUPPORTED where scgib_graph_split refuses the graph. */
int scgib_graph_split_plan(int32_t n, int32_t m, const int32_t *from, const int32_t *to,
                           int32_t n_hidden, const int32_t *hidden_signal,
                           const int32_t *hidden_wait, int32_t *lane, int32_t *pos,
                           int32_t *wait_slot, int32_t *signal_slot, int32_t *info);
int scgib_graph_split_destroy(void *split);
/* Diagnostics: writes the 100 MHz device wall clock (s_memrealtime) to
 * buf[slot] when the stream reaches this point (ops.stamps: the timeline of
 * a replayed step with its hand-offs on; not on the product path). */
int scgib_stamp(uint64_t *buf, int32_t slot, scgib_stream_t stream);
const char *scgib_strerror(int code);

/* ---- A5: GIN neighbourhood aggregation (DGL GINConv, sum aggregator) ------
 * out[v,:] = one_plus_eps * h[v,:] + sum_{j in [rowptr[v], rowptr[v+1])} h[col[j],:]
 * CSR is dst-major (row v lists the SOURCES of v's in-edges).  With the
 * transposed CSR this is also the backward (grad_h from grad_out).
 * Replaces DGL GINConv.forward -> update_all(copy_u, sum) (models.py:69).
 * dim % 4 == 0, 4 <= dim <= 256. */
int scgib_gin_aggregate(const float *h, const int32_t *rowptr, const int32_t *col,
                        int64_t n_nodes, int32_t dim, float one_plus_eps, float *out,
                        const int32_t *dims, scgib_stream_t stream);

/* ---- GCN / GraphSAGE encoders: one fused graph-convolution layer (ABI 23) ----
 * Replaces DGL GraphConv(norm='both', allow_zero_in_degree=True) and
 * SAGEConv(aggregator 'mean') of the reference's GCN / GraphSAGE encoders
 * (models.py:75-104) and their autograd backward.  The DGL semantics are
 * restated (DGL 1.1.0, environment.yml), not linked.
 *
 *   agg[v] = c_dst[v] * sum_{u -> v} c_src[u] x[u]     (dst-major CSR order)
 *   out[v] = act(agg[v] Wn + x[v] Ws + b)              act = ReLU or identity
 *
 * scgib_conv_norm: the coefficient vectors [n] of a graph from its row
 *   pointers, din[v] = rowptr[v+1] - rowptr[v], dout[u] likewise on rowptr_t:
 *   mode 0 (GCN): c_src = max(dout,1)^-1/2, c_dst = max(din,1)^-1/2;
 *   mode 1 (mean): c_src = 1, c_dst = 1 / max(din,1).  Either output may be
 *   NULL (not written); rows >= dims[0] are written as zeros.
 * scgib_conv_layer_fwd: c_src / c_dst may each be NULL (= 1).  Two layer
 *   kinds, told apart by w_self:
 *     w_self NULL, w_in_major = 1: GraphConv — w_neigh is [d_in][d_out]
 *       (GraphConv.weight's layout), no self term;
 *     w_self given, w_in_major = 0: SAGEConv — w_neigh (fc_neigh.weight) and
 *       w_self (fc_self.weight) are [d_out][d_in] (nn.Linear's layout).
 *   Any other combination: SCGIB_EUNSUPPORTED.  bias [d_out] may be NULL.
 *   Writes agg [n][d_in] (saved for the backward; may be NULL) and
 *   out [n][d_out].  (d_in, d_out) in {(32,128), (128,128), (128,64), (32,64),
 *   (64,64)}, else SCGIB_EUNSUPPORTED.  The weights are read in place: no
 *   transposed copy is made.
 * scgib_conv_layer_bwd: with dz = dout * [out > 0] (out given: the layer had
 *   a ReLU; dz [n][d_out] is then written) or dz = dout (out NULL),
 *     dWn = agg^T dz, dWs = x^T dz, db = sum_v dz[v]   into scgib_conv_slabs(n)
 *     per-workgroup slabs of scgib_conv_slab_width(d_in, d_out, has_self)
 *     floats: dWn | dWs (has_self) | db, each weight block in the weight's own
 *     layout — the caller sums them with scgib_slab_reduce_multi;
 *     dx[u] = c_src[u] sum_{u -> v} c_dst[v] (dz[v] Wn^T) + dz[u] Ws^T over the
 *     transposed CSR (rowptr_t, col_t), times [x[u] > 0] when mask_x (x is the
 *     previous layer's ReLU output: dx is then that layer's dz).  dx NULL: the
 *     input needs no gradient, only the slabs are produced.
 *   c_src / c_dst are the FORWARD's vectors (the kernel swaps their roles).
 * Capacity mode: rows >= dims[0] of agg / out / dz / dx are zeros and do not
 * contribute to the slabs. */
int scgib_conv_norm(const int32_t *rowptr, const int32_t *rowptr_t, int64_t n_nodes, int32_t mode,
                    float *c_src, float *c_dst, const int32_t *dims, scgib_stream_t stream);
int64_t scgib_conv_slabs(int64_t n_nodes);
int64_t scgib_conv_slab_width(int32_t d_in, int32_t d_out, int32_t has_self);
int scgib_conv_layer_fwd(const float *x, const int32_t *rowptr, const int32_t *col,
                         const float *c_src, const float *c_dst, int64_t n_nodes, int32_t d_in,
                         int32_t d_out, const float *w_neigh, const float *w_self,
                         int32_t w_in_major, const float *bias, int32_t relu, float *agg,
                         float *out, const int32_t *dims, scgib_stream_t stream);
int scgib_conv_layer_bwd(const float *dout, const float *out, const float *agg, const float *x,
                         const int32_t *rowptr_t, const int32_t *col_t, const float *c_src,
                         const float *c_dst, int64_t n_nodes, int32_t d_in, int32_t d_out,
                         const float *w_neigh, const float *w_self, int32_t w_in_major,
                         int32_t mask_x, float *dz, float *dx, float *slab, const int32_t *dims,
                         scgib_stream_t stream);

/* ---- Graph Transformer encoder: one GraphTransformerLayer ------------------
 * (Entry points added to ABI 24: nothing existing changes, so the version that
 * _lib.py and tests/test_task_loss_cpu.py pin stays 24.)
 * Replaces MultiHeadAttentionLayer + GraphTransformerLayer of the reference's
 * Transformer encoder (models.py:832-918, util functions :986-1005) and their
 * autograd backward.  DGL's apply_edges / send_and_recv are restated, not
 * linked.  Width 64; heads in {1, 2, 4, 8, 16} (d_h = 64 / heads), anything
 * else SCGIB_EUNSUPPORTED.  All weights are nn.Linear's [out][in].
 *
 *   Q, K, V = h Wq^T + bq, ...
 *   e(u->v, a) = K[u,a,:] . Q[v,a,:] / sqrt(d_h),  s = exp(clamp(e, -5, 5))
 *   z[v,a] = sum_{u->v} s,  attn[v,a,:] = sum_{u->v} s V[u,a,:] / (z[v,a] + 1e-6)
 *   h1  = LN1(h + attn Wo^T + bo)              (eps 1e-5, biased variance, affine)
 *   r'  = dropout_0.5(relu(h1 W1^T + b1))      (kept entries x 2; eval: no dropout)
 *   out = LN2(h1 + r' W2^T + b2)
 *
 * Forward, five launches:
 * scgib_gt_qkv_fwd: q, k, v [n][64] from one read of each 64-row tile of h.
 * scgib_gt_attn_fwd: walks the in-edges of every destination in dst-major CSR
 *   order (fp32 running sums); writes attn [n][64] and z [n][heads].  score
 *   (may be NULL; tests) receives the scaled pre-clamp e, [n_edges][heads] in
 *   CSR edge order.  Scores are otherwise not stored.
 * scgib_gt_out_fwd: out = LN(h + attn Wo^T + bo); saves the pre-norm rows
 *   pre [n][64] and stats [n][2] = (mean, rstd).
 * scgib_gt_ffn_fwd (two launches): r [n][128] = r' above, bits [n][4] = the
 *   128-bit keep-and-positive mask of each row (bit c of word c / 32), then
 *   out = LN(h1 + r W2^T + b2) with pre / stats as above.  training != 0:
 *   the keep bits of row i are the Philox4x32-10 block of counter
 *   (i, tag, rng[1]) with tag = 0x47544c31 (the layouts are written out at
 *   scgib_noise_uniform) keyed by rng[0] (rng: uint64 {seed, offset}, a state of
 *   its own, never the compression noise's); the launch's last workgroup
 *   advances rng[1] (counter: one zeroed uint32, left zero).  drop_mask
 *   (bytes [n][128], non-zero = keep) replaces the draw; nothing advances.
 *   pos_bits / keep_bits (may be NULL; tests): the > 0 decisions and the keep
 *   mask used, same packing.
 *
 * Backward, six launches and one slab reduce; no float atomics:
 * scgib_gt_ffn_bwd (two launches): LayerNorm backward of dout from
 *   (pre, stats, gamma) -> dp [n][64] (also the residual's gradient);
 *   dr [n][128] = (dp W2) masked by bits (x 2 when training); dh1 = dp + dr W1.
 *   slab2: scgib_gt_slab_width(0) floats per workgroup = dW2 [64][128] | db2
 *   [64] | dgamma [64] | dbeta [64]; slab1: width(1) = dW1 [128][64] | db1 [128].
 * scgib_gt_out_bwd: LayerNorm backward of dh1 -> dp; dattn = dp Wo;
 *   slab: width(2) = dWo [64][64] | dbo [64] | dgamma [64] | dbeta [64].
 * scgib_gt_attn_bwd (two launches): over destinations
 *     g[v] = dattn[v] / (z[v] + 1e-6),  dzs[v,a] = -sum_d dattn attn / (z + 1e-6),
 *     dq[v] = sum_{u->v} de K[u],  de = (g[v,a,:] . V[u,a,:] + dzs[v,a]) s [|e| <= 5] / sqrt(d_h)
 *   then over sources on the transposed CSR
 *     dk[u] = sum_{u->v} de Q[v],  dv[u] = sum_{u->v} s g[v];
 *   e and s are recomputed from q and k by the forward's own expression.
 *   g [n][64] and dzs [n][heads] are workspace the second launch reads.
 * scgib_gt_qkv_bwd: dh = add + dq Wq + dk Wk + dv Wv (add may be NULL: the
 *   residual's gradient); slab: width(3) = dWq | dWk | dWv [64][64] each |
 *   dbq | dbk | dbv.
 * Every slab kernel runs scgib_gt_slabs(n) workgroups; the caller sums the
 * slabs with scgib_slab_reduce_multi (fixed order).
 * Capacity mode: rows >= dims[0] of every output are zeros and add nothing
 * to the slabs. */
int64_t scgib_gt_slabs(int64_t n_nodes);
int64_t scgib_gt_slab_width(int32_t which);
int scgib_gt_qkv_fwd(const float *h, const float *wq, const float *bq, const float *wk,
                     const float *bk, const float *wv, const float *bv, int64_t n_nodes, float *q,
                     float *k, float *v, const int32_t *dims, scgib_stream_t stream);
int scgib_gt_attn_fwd(const float *q, const float *k, const float *v, const int32_t *rowptr,
                      const int32_t *col, int64_t n_nodes, int32_t heads, float *attn, float *z,
                      float *score, const int32_t *dims, scgib_stream_t stream);
int scgib_gt_attn_bwd(const float *dattn, const float *attn, const float *z, const float *q,
                      const float *k, const float *v, const int32_t *rowptr, const int32_t *col,
                      const int32_t *rowptr_t, const int32_t *col_t, int64_t n_nodes,
                      int32_t heads, float *g, float *dzs, float *dq, float *dk, float *dv,
                      const int32_t *dims, scgib_stream_t stream);
int scgib_gt_out_fwd(const float *attn, const float *h, const float *wo, const float *bo,
                     const float *gamma, const float *beta, int64_t n_nodes, float *pre,
                     float *stats, float *out, const int32_t *dims, scgib_stream_t stream);
int scgib_gt_ffn_fwd(const float *h1, const float *w1, const float *b1, const float *w2,
                     const float *b2, const float *gamma, const float *beta, int64_t n_nodes,
                     int32_t training, uint64_t *rng, uint32_t *counter, const uint8_t *drop_mask,
                     float *r, uint32_t *bits, uint32_t *pos_bits, uint32_t *keep_bits, float *pre,
                     float *stats, float *out, const int32_t *dims, scgib_stream_t stream);
int scgib_gt_ffn_bwd(const float *dout, const float *pre, const float *stats, const float *gamma,
                     const float *r, const uint32_t *bits, int32_t training, const float *h1,
                     const float *w1, const float *w2, int64_t n_nodes, float *dp, float *dr,
                     float *dh1, float *slab2, float *slab1, const int32_t *dims,
                     scgib_stream_t stream);
int scgib_gt_out_bwd(const float *dh1, const float *pre, const float *stats, const float *gamma,
                     const float *attn, const float *wo, int64_t n_nodes, float *dp, float *dattn,
                     float *slab, const int32_t *dims, scgib_stream_t stream);
int scgib_gt_qkv_bwd(const float *dq, const float *dk, const float *dv, const float *h,
                     const float *wq, const float *wk, const float *wv, const float *add,
                     int64_t n_nodes, float *dh, float *slab, const int32_t *dims,
                     scgib_stream_t stream);

/* ---- the Transformer encoder's folded entry (csrc/gt_embed.hip) -------------
 *   h0 = (x[map] Wt^T) We^T   [n][64]
 * x [rows_x][n_feat]: the raw normalised features, 1 <= n_feat <= 16; wt =
 * transfer_d.weight [32][n_feat], we = embedding_h.weight [64][32] (neither
 * has a bias); map (int32 [n], may be NULL: the identity, rows_x >= n then)
 * gives the row of x behind each row of h0 (an ego batch's parent rows); an
 * entry outside [0, rows_x) reads the nearest row of x.  The [n][32]
 * intermediate is never written: the backward recomputes it.
 * scgib_gt_embed_bwd: slab = scgib_gt_embed_slabs(n) rows of
 * scgib_gt_embed_slab_width(n_feat) floats, dWe [64][32] | dWt [32][n_feat];
 * the caller sums the rows with scgib_slab_reduce_multi (fixed order).  No
 * gradient for x.  n_feat outside 1..16: SCGIB_EUNSUPPORTED (slab_width: 0).
 * Capacity mode: rows >= dims[0] of h0 are zeros and add nothing to the slabs. */
int64_t scgib_gt_embed_slabs(int64_t n_nodes);
int64_t scgib_gt_embed_slab_width(int32_t n_feat);
int scgib_gt_embed_fwd(const float *x, int32_t n_feat, int64_t rows_x, const int32_t *map,
                       const float *wt, const float *we, int64_t n_nodes, float *h0,
                       const int32_t *dims, scgib_stream_t stream);
int scgib_gt_embed_bwd(const float *dh0, const float *x, int32_t n_feat, int64_t rows_x,
                       const int32_t *map, const float *wt, const float *we, int64_t n_nodes,
                       float *slab, const int32_t *dims, scgib_stream_t stream);

/* ---- A5 fused: one GIN layer = GINConv(MLP) + BatchNorm1d + ReLU -----------
 * Replaces, per layer, DGL GINConv + nn.Linear x2 + ReLU + nn.BatchNorm1d +
 * F.relu of GIN.forward (models.py:63-71) and their autograd backward.
 * Tiles of 64 rows; scgib_gin_tiles(n) tiles; tile_stats holds 128 floats per
 * tile.  `stat` is the layer's [4][64] BN record: mean, invstd, scale
 * (= gamma*invstd), shift (= beta - mean*scale).
 *
 * scgib_gin_layer_fwd: agg = (1+eps) x_v + sum_{u->v} x_u with x = h_in, or
 *   x = relu(in_stat.scale * h_in + in_stat.shift) when in_stat != NULL
 *   (the previous layer's BN+ReLU applied on load; d_in must be 64);
 *   r = relu(agg W1^T + b1); z2 = r W2^T + b2; per-tile (sum, centred M2).
 *   d_in in {32, 64}; hidden 64.  Outputs agg [n,d_in], r, z2 [n,64];
 *   r may be NULL (also in scgib_gin_layer_fwd_bn / scgib_gin_layer0_fwd): it
 *   is then not stored and the backward recomputes it (below).
 * scgib_bn_finalize: training: batch mean/var from the tile stats (fp64
 *   Chan combine), running stats updated (momentum, unbiased var,
 *   num_batches_tracked += 1); eval: running stats.  Writes `stat`.
 * scgib_bn_relu_apply: out = relu(stat.scale * z + stat.shift)  [n,64].
 *   in_pending (may be NULL): the last GIN layer's deferred statistics
 *   (scgib_bn_pending below) — finished here, `stat` is then written.
 * scgib_gin_bwd_stats: dy = dh * [stat.scale z2 + stat.shift > 0], dh given,
 *   or, with (rowptr_t, col_t), gathered from the next layer's d(agg):
 *   dh_v = (1+eps) g_v + sum_{u in out(v)} g_u.  Per-tile sum(dy), sum(dy xhat).
 * scgib_bn_bwd_finalize: dgamma, dbeta [64] and coef [2][64] for dz2.
 * scgib_gin_layer_bwd: d(agg) [n,d_in] and wgrad = dW2[64*64] | dW1[64*d_in]
 *   | db2[64] | db1[64] through scgib_gin_layer_bwd_slabs(n, d_in) per-workgroup
 *   slabs of 64*64 + 64*d_in + 128 floats (scgib_gin_slab_floats(n, d_in) in
 *   total; d_in = 64: 32-row sub-tiles, up to two workgroups per CU each
 *   walking its sub-tiles), reduced in a fixed order.  With wgrad NULL the slabs are left for the
 *   caller's scgib_slab_reduce (so the GEMM kernel can be timed alone).
 *   r NULL (d_in = 64, and scgib_gin_layer0_bwd): the forward did not store r
 *   (a third of the forward's HBM writes); the kernel
 *   recomputes r = relu(agg W1^T + b1) from the saved agg with the forward's
 *   own MFMA chain — bitwise the r it would have stored, so every output is
 *   bitwise the stored-r kernel's.  b1 is read only then (may be NULL with r).
 * scgib_gin_hidden: r = relu(agg W1^T + b1) [n,64] with that same chain
 *   (inspection / tests: the hidden ReLU decisions of a step that did not
 *   store r).
 * scgib_slab_reduce: out[w] = sum_s slab[s*width + w], fixed order. */
int64_t scgib_gin_tiles(int64_t n_nodes);
int64_t scgib_gin_slab_floats(int64_t n_nodes, int32_t d_in);
int64_t scgib_gin_bwd_slabs(int64_t n_nodes);  /* layer-0 (transfer_d folded) slabs */
int64_t scgib_gin_layer_bwd_slabs(int64_t n_nodes, int32_t d_in);
/* Up to scgib_slab_reduce_max_jobs() independent scgib_slab_reduce's in one
 * launch (same fixed order per job): out[w] = sum_s slab[s*stride + w] for
 * w < width; stride 0 means width (a column range of wider slabs otherwise,
 * stride >= width). */
typedef struct {
    const float *slab;
    float *out;
    int64_t width;
    int32_t n_slabs;
    int32_t stride;
} scgib_slab_job;
int64_t scgib_slab_reduce_max_jobs(void);
int scgib_slab_reduce_multi(const scgib_slab_job *jobs, int32_t n_jobs, scgib_stream_t stream);
/* The same on at most max_workgroups workgroups (0: no cap; each loops over
 * column blocks) — for a reduce that runs beside another chain's kernels. */
int scgib_slab_reduce_multi_ex(const scgib_slab_job *jobs, int32_t n_jobs,
                               int32_t max_workgroups, scgib_stream_t stream);
int scgib_slab_reduce(const float *slab, int32_t n_slabs, int64_t width, float *out,
                      scgib_stream_t stream);
int scgib_gin_layer_fwd(const float *h_in, int32_t d_in, const float *in_stat,
                        const int32_t *rowptr, const int32_t *col, int64_t n_nodes,
                        float one_plus_eps, const float *w1, const float *b1, const float *w2,
                        const float *b2, float *agg, float *r, float *z2, float *tile_stats,
                        const int32_t *dims, scgib_stream_t stream);
int scgib_bn_finalize(const float *tile_stats, int64_t n_nodes, const float *gamma,
                      const float *beta, float eps, float momentum, int32_t training,
                      float *running_mean, float *running_var, int64_t *num_batches_tracked,
                      float *stat, const int32_t *dims, scgib_stream_t stream);
int scgib_bn_relu_apply(const float *z, const float *stat, int64_t n_nodes, float *out,
                        const int32_t *dims, const scgib_bn_pending *in_pending,
                        scgib_stream_t stream);
int scgib_gin_bwd_stats(const float *dh, const int32_t *rowptr_t, const int32_t *col_t,
                        float one_plus_eps, const float *z2, const float *stat, int64_t n_nodes,
                        float *dy, float *tile_stats, const int32_t *dims,
                        scgib_stream_t stream);
int scgib_bn_bwd_finalize(const float *tile_stats, int64_t n_nodes, int32_t training,
                          float *dgamma, float *dbeta, float *coef, const int32_t *dims,
                          scgib_stream_t stream);
/* Training-mode fused variants: the BatchNorm finalize is folded into the
 * tile kernel (hierarchical last-arriver over 16-tile groups, past 64 groups
 * also over 64-group supergroups; fp64, fixed order) — one launch per layer
 * instead of two.  `bn_ws` holds scgib_gin_bn_ws_floats(n) floats (tile
 * statistics + group and supergroup partials);
 * `counters` holds scgib_gin_counters(n) uint32 that are zero on entry and
 * left zero (graph-replay safe; one set per concurrently running encoder).
 * scgib_gin_layer_fwd_bn = scgib_gin_layer_fwd + scgib_bn_finalize(training);
 * running_mean/var/num_batches_tracked may be NULL (track_running_stats off).
 * scgib_gin_bwd_stats_bn = scgib_gin_bwd_stats + scgib_bn_bwd_finalize. */
int64_t scgib_gin_bn_ws_floats(int64_t n_nodes);
int64_t scgib_gin_counters(int64_t n_nodes);

int scgib_gin_layer_fwd_bn(const float *h_in, int32_t d_in, const float *in_stat,
                           const int32_t *rowptr, const int32_t *col, int64_t n_nodes,
                           float one_plus_eps, const float *w1, const float *b1, const float *w2,
                           const float *b2, float *agg, float *r, float *z2, const float *gamma,
                           const float *beta, float bn_eps, float momentum, float *running_mean,
                           float *running_var, int64_t *num_batches_tracked, float *stat,
                           float *bn_ws, uint32_t *counters, const int32_t *dims,
                           const scgib_bn_pending *in_pending, int32_t defer,
                           scgib_stream_t stream);
int scgib_gin_bwd_stats_bn(const float *dh, const int32_t *rowptr_t, const int32_t *col_t,
                           float one_plus_eps, const float *z2, const float *stat,
                           int64_t n_nodes, int32_t training, float *dy, float *dgamma,
                           float *dbeta, float *coef, float *bn_ws, uint32_t *counters,
                           const int32_t *dims, int32_t defer, scgib_stream_t stream);
/* scgib_gin_bwd_stats_bn for an encoder output read by a segment-sum readout
 * (dgl.sum_nodes of the ego-net features, models.py:724-726): dh[v] =
 * (dh ? dh[v] : 0) + g_seg[seg[v]] (dh may be NULL), i.e. the readout's
 * backward broadcast is folded in; seg from scgib_bn_relu_segment_sum. */
int scgib_gin_bwd_stats_seg_bn(const float *dh, const float *g_seg, const int32_t *seg,
                               const float *z2, const float *stat, int64_t n_nodes,
                               int32_t training, float *dy, float *dgamma, float *dbeta,
                               float *coef, float *bn_ws, uint32_t *counters,
                               const int32_t *dims, int32_t defer, scgib_stream_t stream);
/* Encoder output and its readout in one pass: out = relu(stat.scale z +
 * stat.shift) [n_rows][64], readout[s] = sum of out rows [ptr[s], ptr[s+1])
 * (same order as scgib_segment_sum), seg[row] = s.  seg_dims (device, may be
 * NULL): actual segment count; rows past the last valid one are zeroed.
 * in_pending / dims (row count, may be NULL): as scgib_bn_relu_apply. */
int scgib_bn_relu_segment_sum(const float *z, const float *stat, const int32_t *ptr,
                              int64_t n_seg, int64_t n_rows, float *out, float *readout,
                              int32_t *seg, const int32_t *seg_dims, const int32_t *dims,
                              const scgib_bn_pending *in_pending, scgib_stream_t stream);
/* Deferred finalize (scgib_bn_pending above): in_pending (NULL: in_stat is
 * used) names the previous layer's pending statistics — this layer finishes
 * them; defer = 1 leaves this layer's own pending (stat / running stats /
 * dgamma, dbeta, coef are then written by the consumer). */
int64_t scgib_gin_bn_gpart_offset(int64_t n_nodes);
int64_t scgib_gin_defer_max_nodes(void);
/* Layer 0 with transfer_d folded in (models.py:668-669 / :1164-1165:
 * h0 = x Wt^T, Wt = transfer_d.weight [32][F], F <= 16): the kernel gathers
 * the raw rows x[node_map[v]] (node_map NULL = identity; ego batches pass
 * the ego -> parent map, so x_subs is never built), aggx = ope x + sum_u x
 * ([n][16] zero-padded, saved) and agg = aggx Wt^T ([n][32], saved), then the
 * usual layer.  counters NULL: BN not fused (bn_ws then holds the tile
 * statistics for scgib_bn_finalize).  Backward: one slab per workgroup of
 * scgib_gin_layer0_slab_width() floats = dW2 | dW1[64*32] | db2 | db1 |
 * dWt[32][n_feat] row-major in the first 32*n_feat floats of a 512-float
 * region (the rest is not written); d(agg0) is not produced. */
int64_t scgib_gin_layer0_slab_width(void);
int scgib_gin_layer0_fwd(const float *x, int32_t n_feat, const int32_t *node_map, const float *wt,
                         const int32_t *rowptr, const int32_t *col, int64_t n_nodes,
                         float one_plus_eps, const float *w1, const float *b1, const float *w2,
                         const float *b2, float *agg, float *aggx, float *r, float *z2,
                         const float *gamma, const float *beta, float bn_eps, float momentum,
                         float *running_mean, float *running_var, int64_t *num_batches_tracked,
                         float *stat, float *bn_ws, uint32_t *counters, const int32_t *dims,
                         int32_t defer, scgib_stream_t stream);
/* scgib_gin_bwd_stats_bn with a weight-gradient slab reduce folded in
 * (`fold` NULL: none): extra workgroups past the tile grid compute
 * fold->out[w] = sum_s fold->slab[s*stride + w] (fixed order, as
 * scgib_slab_reduce_multi's job) — the previous layer's reduce runs in the
 * bandwidth the gather-bound statistics tiles leave idle. */
int scgib_gin_bwd_stats_bn_fold(const float *dh, const int32_t *rowptr_t, const int32_t *col_t,
                                float one_plus_eps, const float *z2, const float *stat,
                                int64_t n_nodes, int32_t training, float *dy, float *dgamma,
                                float *dbeta, float *coef, float *bn_ws, uint32_t *counters,
                                const int32_t *dims, int32_t defer, const scgib_slab_job *fold,
                                scgib_stream_t stream);
/* layer backward: `pending` (NULL: coef is read) finishes the deferred
 * scgib_gin_bwd_stats_bn of the same layer (coef may then be NULL). */
/* need_w = 0: the layer's W1 / b1 / W2 / b2 take no gradient (frozen: the
 * fine-tune freezing quirk, models.py:424-434) — only d(agg) (layer 0: dWt)
 * is formed, by the same chains (bitwise the need_w = 1 values); the dW
 * products and slabs are skipped (layer 0: only its dWt slab part is
 * written; agg may then be NULL; r must be given). */
int scgib_gin_layer0_bwd(const float *dy, const float *z2, const float *r, const float *agg,
                         const float *aggx, int32_t n_feat, const float *stat,
                         const float *coef, const float *w1, const float *b1, const float *w2,
                         int64_t n_nodes, float *slab, int32_t need_w, const int32_t *dims,
                         const scgib_bn_bwd_pending *pending, scgib_stream_t stream);
int scgib_gin_layer_bwd(const float *dy, const float *z2, const float *r, const float *agg,
                        int32_t d_in, const float *stat, const float *coef, const float *w1,
                        const float *b1, const float *w2, int64_t n_nodes, float *dagg,
                        float *slab, float *wgrad, int32_t need_w, const int32_t *dims,
                        const scgib_bn_bwd_pending *pending, scgib_stream_t stream);
int scgib_gin_hidden(const float *agg, int32_t d_in, const float *w1, const float *b1,
                     int64_t n_nodes, float *r, scgib_stream_t stream);
/* ---- A5: the agg-free backward of a d_in = 64 layer l >= 1 (ABI 20) ----
 * Replaces the agg half of DGL GINConv's backward (models.py:63-71, the
 * GINConv(MLP) + BatchNorm1d of GIN.forward): for a symmetric molecule graph
 * dW1 = dz1^T agg = g^T h_{l-1} and d h_{l-1} = g W1 with g = (I + A)^T dz1,
 * so the forward stores no agg for such a layer (scgib_gin_layer_fwd[_bn]
 * with agg NULL) and:
 *   scgib_gin_layer_bwd_z   dz2 (BN backward) -> dW2 += dz2^T r, dr = dz2 W2,
 *                           dz1 = dr [r > 0] written to dz1 [n][64]; one slab
 *                           per workgroup: dW2 [64][64] | db2 [64] | db1 [64]
 *                           (scgib_gin_layer_bwd_z_width floats; count
 *                           scgib_gin_layer_bwd_z_slabs); `fold`, `fold2`
 *                           (or NULL): slab jobs reduced in extra workgroups
 *                           (fold: 32 columns x 8 slab partitions each, for
 *                           the previous statistics launch's many dW1
 *                           partials; fold2: as scgib_gin_bwd_stats_bn_fold's);
 *   scgib_gin_bwd_stats_z   layer l-1's statistics from dz1 of layer l:
 *                           g gathered over the transposed CSR (one_plus_eps
 *                           of layer l), dh = g W1 (W1 of layer l), dy = dh
 *                           [scale z2 + shift > 0], BN sums as
 *                           scgib_gin_bwd_stats_bn_fold; dW1 of layer l as
 *                           one [64][64] partial per workgroup in wslab
 *                           (scgib_gin_bwd_stats_z_slabs of them); up to two
 *                           fold jobs reduced in extra workgroups.
 * need_w = 0 (a frozen layer l, resp. l + 1 for the statistics): the same
 * data chains (bitwise the need_w = 1 dz1 / dy), no weight products, no
 * slab (slab / wslab may be NULL).  Results equal the stored-agg path to
 * fp32 rounding (different association of the same sums), deterministic run
 * to run. */
int64_t scgib_gin_layer_bwd_z_slabs(int64_t n_nodes);
int64_t scgib_gin_layer_bwd_z_width(void);
int scgib_gin_layer_bwd_z(const float *dy, const float *z2, const float *r, const float *stat,
                          const float *coef, const float *w2, int64_t n_nodes, float *dz1,
                          float *slab, int32_t need_w, const int32_t *dims,
                          const scgib_bn_bwd_pending *pending, const scgib_slab_job *fold,
                          const scgib_slab_job *fold2, scgib_stream_t stream);
int64_t scgib_gin_bwd_stats_z_slabs(int64_t n_nodes);
int scgib_gin_bwd_stats_z(const float *dz1, const int32_t *rowptr_t, const int32_t *col_t,
                          float one_plus_eps, const float *w1, const float *z2, const float *stat,
                          int64_t n_nodes, int32_t training, float *dy, float *dgamma,
                          float *dbeta, float *coef, float *bn_ws, uint32_t *counters,
                          const int32_t *dims, int32_t defer, float *wslab, int32_t need_w,
                          const scgib_slab_job *fold, int32_t n_fold, scgib_stream_t stream);

/* ---- (f)1/(f)4: Set2Set readout (DGL Set2Set(dim, n_iters, 1), models.py:565) ----
 * The whole readout as Mainmodel_finetuning.forward (models.py:515) and
 * Mainmodel_domainadapt (:271-272) run it, all n_iters rounds in one launch:
 * for graph g (rows [graph_ptr[g], graph_ptr[g+1]) of x [*][dim], dim <= 64),
 * from h = c = 0, q* = 0:
 *   gates = W_ih q* + b_ih + W_hh h + b_hh  (w_ih [4 dim][2 dim], w_hh [4 dim][dim],
 *           PyTorch LSTM gate order i, f, g, o);  c = sig(f) c + sig(i) tanh(g);
 *   h = sig(o) tanh(c);  e_v = <x_v, h>;  alpha = softmax_g(e);  r = sum_v alpha_v x_v;
 *   q* = [h, r];   out [n_graphs][2 dim] = the last q*.
 * save [scgib_set2set_save_floats]: the per-round state the backward reads.
 * Backward: d out -> dx (rows past graph_ptr[n_graphs], up to n_rows:
 * capacity padding, zeroed), dw_ih, dw_hh, db_ih = db_hh; dgates
 * [n_graphs * n_iters * 4 dim] is scratch.  No host sync: graph-capturable.
 * With dw_ih, dw_hh, db_ih and db_hh all NULL, scgib_set2set_bwd writes dx and
 * dgates only, and scgib_set2set_wgrad (the same save / dgates) forms the
 * weight gradients later — the fine-tune step runs it off the critical
 * chain (ops.SlabScope).
 * Weight alignment: the kernels read a weight row as 16-byte vectors when it
 * is a multiple of 4 floats.  scgib_set2set_fwd, _bwd, _fwd2 and _bwd2 (the
 * entry points that take the weights; _wgrad and _save_floats take none)
 * return SCGIB_EINVAL before any launch when w_ih is not 16-byte aligned and
 * 2 dim % 4 == 0, or w_hh is not 16-byte aligned and dim % 4 == 0 — dim = 64
 * (weights preloaded into registers) included.  ops.set2set / set2set_pair
 * pass an aligned copy of such a weight. */
int64_t scgib_set2set_save_floats(int64_t n_graphs, int32_t dim, int32_t n_iters);
int scgib_set2set_fwd(const float *x, const int32_t *graph_ptr, int64_t n_graphs, int32_t dim,
                      int32_t n_iters, const float *w_ih, const float *b_ih, const float *w_hh,
                      const float *b_hh, float *save, float *out, scgib_stream_t stream);
int scgib_set2set_bwd(const float *x, const int32_t *graph_ptr, int64_t n_graphs, int32_t dim,
                      int32_t n_iters, const float *w_ih, const float *w_hh, const float *save,
                      const float *g_out, float *dx, int64_t n_rows, float *dgates,
                      float *dw_ih, float *dw_hh, float *db_ih, float *db_hh,
                      scgib_stream_t stream);
int scgib_set2set_wgrad(const float *save, const float *dgates, int64_t n_graphs, int32_t dim,
                        int32_t n_iters, float *dw_ih, float *dw_hh, float *db_ih, float *db_hh,
                        scgib_stream_t stream);
/* Two inputs xa, xb [*][dim] over the same graph_ptr and the same LSTM in one
 * launch per direction (the pretraining step's readouts of the noisy and the
 * plain graph features, models.py:686 / :718): 2 n_graphs workgroups,
 * workgroup g + n_graphs * which reads input `which`.  out [2][n_graphs][2 dim];
 * g_outa / g_outb [n_graphs][2 dim] each, either (not both) NULL for an output
 * no loss reads (zero gradient); save holds scgib_set2set_save_floats(2 n_graphs, ...) floats
 * and dgates 2 n_graphs * n_iters * 4 dim, input `which` in the half `which`
 * of each.  Outputs and dxa / dxb (distinct buffers) carry the bits of two
 * single-input calls.  The weight gradients are the sum over both halves in
 * index order, formed in one pass: by scgib_set2set_bwd2 itself, or, with the
 * four of them NULL, by scgib_set2set_wgrad called with 2 n_graphs. */
int scgib_set2set_fwd2(const float *xa, const float *xb, const int32_t *graph_ptr,
                       int64_t n_graphs, int32_t dim, int32_t n_iters, const float *w_ih,
                       const float *b_ih, const float *w_hh, const float *b_hh, float *save,
                       float *out, scgib_stream_t stream);
int scgib_set2set_bwd2(const float *xa, const float *xb, const int32_t *graph_ptr,
                       int64_t n_graphs, int32_t dim, int32_t n_iters, const float *w_ih,
                       const float *w_hh, const float *save, const float *g_outa,
                       const float *g_outb, float *dxa, float *dxb, int64_t n_rows,
                       float *dgates, float *dw_ih, float *dw_hh, float *db_ih, float *db_hh,
                       scgib_stream_t stream);

/* ---- A6: per-segment readouts (dgl.sum_nodes) -------------------------------
 * out[s,:] = sum_{i in [ptr[s], ptr[s+1])} x[i,:]   (models.py:716, 725, 733)
 * segment_broadcast is its adjoint: out[i,:] = g[s,:] for every row i of s.
 * dim: any >= 1 (float4 lanes when dim is 4 x a power of two <= 256, else a
 * scalar kernel, e.g. for raw node features). */
int scgib_segment_sum(const float *x, const int32_t *ptr, int64_t n_seg, int32_t dim,
                      float *out, const int32_t *dims, scgib_stream_t stream);
/* n_rows: rows of `out` (rows past ptr[actual n_seg] are zeroed, with or without
 * device dims: every row of `out` is written) */
int scgib_segment_broadcast(const float *g, const int32_t *ptr, int64_t n_seg, int32_t dim,
                            float *out, int64_t n_rows, const int32_t *dims,
                            scgib_stream_t stream);

/* ---- A2: k-hop ego-net builder (dgl.khop_in_subgraph for every node) -------
 * Replaces the per-node Python loop of exp_pretraining.py:269-272 (+ the
 * per-step dgl.batch of the ego-nets, exp_pretraining.py:308-309).
 * Graph: dst-major CSR (rowptr/col) of a batch of graphs whose node ranges are
 * [graph_ptr[g], graph_ptr[g+1]); edges must stay inside their graph, column
 * lists sorted ascending, the graph symmetric (to_bidirected output).
 * max_graph_nodes <= 512.
 *
 * Step 1, scgib_egonet_count: fills ego_ptr[0..n] and ego_eptr[0..n] with the
 * exclusive prefix sums of the ego-net node / edge counts (ego_ptr[n] = N_s,
 * ego_eptr[n] = E_s).  `workspace` holds scgib_egonet_workspace_bytes(n).
 * err (device int32, zeroed by the caller) becomes non-zero if an edge leaves
 * its graph or a graph exceeds max_graph_nodes.
 * Step 2, scgib_egonet_fill: writes, for the batched ego graph (ego j <-> node j,
 * ego nodes sorted ascending, DGL node_subgraph edge order):
 *   ego_nodes[N_s]   parent node id of every ego node (DGL's ndata['_ID'] + offset)
 *   sub_rowptr[N_s+1], sub_col[E_s]  dst-major CSR in ego-batch node ids.
 * n_ego_cap = length of ego_nodes (>= N_s): entries [N_s, n_ego_cap) get
 * parent id 0 and empty CSR rows.  ego_dims (nullable, device int32[2])
 * receives [N_s, E_s] (the ego batch's `dims` in capacity mode). */
int64_t scgib_egonet_workspace_bytes(int64_t n_nodes);
int scgib_egonet_count(const int32_t *rowptr, const int32_t *col, const int32_t *graph_ptr,
                       int64_t n_graphs, int64_t n_nodes, int32_t k, int32_t max_graph_nodes,
                       int32_t *ego_ptr, int32_t *ego_eptr, void *workspace, int32_t *err,
                       const int32_t *dims, scgib_stream_t stream);
/* k = 1 fast path, both passes in two launches: ball(v) = {v} u N(v) as a
 * 128-bit window bitmap centred on v (no molecule bitmap, no graph_ptr
 * search), batched loads; same outputs as scgib_egonet_count +
 * scgib_egonet_fill (ego_ptr, ego_eptr exclusive scans; ego_nodes;
 * sub_rowptr/sub_col in DGL order; ego_dims).  Requires every in-degree <=
 * scgib_egonet_k1_max_degree(), molecules <= scgib_egonet_k1_max_graph_nodes()
 * atoms and edges inside their molecule (the caller checks them on the host).
 * workspace: scgib_egonet_workspace_bytes(n). */
int64_t scgib_egonet_k1_max_degree(void);
int64_t scgib_egonet_k1_max_graph_nodes(void);
int scgib_egonet_k1_build(const int32_t *rowptr, const int32_t *col, int64_t n_nodes,
                          int32_t *ego_ptr, int32_t *ego_eptr, void *workspace,
                          int32_t *ego_nodes, int32_t *sub_rowptr, int32_t *sub_col,
                          int64_t n_ego_cap, const int32_t *dims, int32_t *ego_dims,
                          scgib_stream_t stream);
/* The same with the batch's max in-degree (<= scgib_egonet_k1_max_degree()):
 * <= 6 runs the kernels built for balls of <= 7 members (one load group,
 * half the neighbour slots of the general form). */
int scgib_egonet_k1_build_deg(const int32_t *rowptr, const int32_t *col, int64_t n_nodes,
                              int32_t max_in_degree, int32_t *ego_ptr, int32_t *ego_eptr,
                              void *workspace, int32_t *ego_nodes, int32_t *sub_rowptr,
                              int32_t *sub_col, int64_t n_ego_cap, const int32_t *dims,
                              int32_t *ego_dims, scgib_stream_t stream);
/* The same in ONE launch: each block of 64 parents takes its offsets by a
 * decoupled look-back over the preceding blocks instead of a second launch.
 * scan_state: scgib_egonet_k1_scan_words(n) ZEROED uint32 words, 4-byte
 * aligned, left zeroed by the launch (reusable by the next one; one launch in
 * flight per scan_state).  Output identical to scgib_egonet_k1_build_deg.
 * e_cap: sub_col's capacity; a ball that would write past n_ego_cap rows or
 * e_cap columns is dropped and ORs the flag value 4 (bit 2; flags 1 and 2
 * as above) into *err (err may be NULL). */
int64_t scgib_egonet_k1_scan_words(int64_t n_nodes);
/* Launches of up to this many blocks (64 parents each) index the look-back by
 * blockIdx.x; larger ones take each block's logical index from a ticket. */
int64_t scgib_egonet_k1_resident_blocks(void);
int scgib_egonet_k1_build_onepass(const int32_t *rowptr, const int32_t *col, int64_t n_nodes,
                                  int32_t max_in_degree, int32_t *ego_ptr, int32_t *ego_eptr,
                                  uint32_t *scan_state, int32_t *ego_nodes, int32_t *sub_rowptr,
                                  int32_t *sub_col, int64_t n_ego_cap, int64_t e_cap,
                                  int32_t *err, const int32_t *dims, int32_t *ego_dims,
                                  scgib_stream_t stream);
/* scgib_egonet_count / scgib_egonet_fill (any k) over the resident pool's
 * batch srcs[ctr[0] % n_src] (rowptr / col / graph_ptr / dims at byte offsets
 * of each graph.StaticBatch blob, capacity mode; n_nodes = the capacity),
 * resolved on the device when each kernel starts (graph.EgoPrefetch, k >= 2). */
int scgib_egonet_count_pool(const uint64_t *srcs, int32_t n_src, const uint32_t *ctr,
                            int64_t o_rowptr, int64_t o_col, int64_t o_gptr, int64_t o_dims,
                            int64_t n_graphs, int64_t n_nodes, int32_t k, int32_t max_graph_nodes,
                            int32_t *ego_ptr, int32_t *ego_eptr, void *workspace, int32_t *err,
                            scgib_stream_t stream);
int scgib_egonet_fill_pool(const uint64_t *srcs, int32_t n_src, const uint32_t *ctr,
                           int64_t o_rowptr, int64_t o_col, int64_t o_gptr, int64_t o_dims,
                           int64_t n_graphs, int64_t n_nodes, int32_t k, int32_t max_graph_nodes,
                           const int32_t *ego_ptr, const int32_t *ego_eptr, int32_t *ego_nodes,
                           int32_t *sub_rowptr, int32_t *sub_col, int32_t *err,
                           int64_t n_ego_cap, int32_t *ego_dims, scgib_stream_t stream);
/* The one-launch k = 1 build over the resident pool's batch srcs[ctr[0] % n_src]
 * (srcs, ctr as in scgib_pool_copy; rowptr / col / dims at byte offsets
 * o_rowptr / o_col / o_dims of each pool blob, capacity mode), resolved on
 * the device when the kernel starts: the ego-nets of the batch the next
 * replayed step loads, built inside the current step (graph.EgoPrefetch;
 * replaces the in-step dgl.khop_in_subgraph pass, exp_pretraining.py:269-272). */
int scgib_egonet_k1_build_onepass_pool(const uint64_t *srcs, int32_t n_src, const uint32_t *ctr,
                                       int64_t o_rowptr, int64_t o_col, int64_t o_dims,
                                       int64_t n_nodes, int32_t max_in_degree, int32_t *ego_ptr,
                                       int32_t *ego_eptr, uint32_t *scan_state,
                                       int32_t *ego_nodes, int32_t *sub_rowptr, int32_t *sub_col,
                                       int64_t n_ego_cap, int64_t e_cap, int32_t *err,
                                       int32_t *ego_dims, scgib_stream_t stream);
int scgib_egonet_fill(const int32_t *rowptr, const int32_t *col, const int32_t *graph_ptr,
                      int64_t n_graphs, int64_t n_nodes, int32_t k, int32_t max_graph_nodes,
                      const int32_t *ego_ptr, const int32_t *ego_eptr, int32_t *ego_nodes,
                      int32_t *sub_rowptr, int32_t *sub_col, int32_t *err, int64_t n_ego_cap,
                      const int32_t *dims, int32_t *ego_dims, scgib_stream_t stream);

/* ---- A6-A8 + A10/A11 inputs: core <-> subgraph interaction, fused ----------
 * One wavefront per molecule.  Restates, per graph i (models.py:595-604,
 * 631-660, 714-749):
 *   z2[i]   = sum_nodes(f)                                  (graph readout)
 *   p       = W2 . relu(BN_i(t)) + b2   with t = f W1^T + b1 given, BN_i the
 *             compressor BatchNorm over graph i's rows (train) or running
 *             stats (eval)
 *   lambda  = sigmoid(log(e) - log(1-e) + p),  e = 0.9999 - 0.9998 * u_gate
 *   (sigma, mu) = std_mean(f_i) (unbiased), noisy = lambda f + (1-lambda) mu
 *             + u_feat (1-lambda) sigma                    -> im[:, 0:64]
 *   z1[i]   = sum_nodes(noisy)
 *   logit_v = w_att[0:64].z1[i] + w_att[64:128].s_v + b_att, alpha = softmax_i
 *   im[:, 64:128] = alpha * s
 *   kl_tensor[2*n_last, 64]: the last graph's KL term, twice (models.py:659)
 * kl_mean (scalar) = mean(kl_tensor); either output may be NULL (not both).
 * pad_rows != 0: n_nodes is a row capacity and rows [graph_ptr[B], n_nodes)
 * of im, lam, logit are zeroed (capacity mode; B stays exact).
 * Saved for backward: lam[N], logit[N] (= w_att[64:128].s_v: the per-graph
 * z-bar term cancels in the softmax, so it is kept out of the saved logits and
 * their max/sum), stats[B, SCGIB_STATS_STRIDE].
 * Scalars b2, b_att are device pointers (no host sync). */
int scgib_interaction_fwd(const float *f, const float *t, const float *s,
                          const float *u_gate, const float *u_feat, const int32_t *graph_ptr,
                          int64_t n_graphs, int64_t n_nodes, const float *bn_gamma,
                          const float *bn_beta, const float *bn_running_mean,
                          const float *bn_running_var, float bn_eps, int32_t training,
                          const float *w2, const float *b2, const float *w_att,
                          const float *b_att, float *im, float *z1, float *z2, float *lam,
                          float *logit, float *stats, float *kl_tensor, float *kl_mean,
                          int32_t pad_rows, scgib_stream_t stream);

/* Device noise for the interaction (replaces the reference's torch.rand gate
 * draw u [n,1], models.py:599, and feature draw u [n,64], :650, when no noise
 * is given): counter-based Philox4x32-10 uniforms in [0, 1) keyed by
 * rng_state[0] (seed) and rng_state[1] (offset; uint64, device) -> u_gate
 * [n_rows], u_feat [n_rows][64], passed to scgib_interaction_fwd as noise.
 * The last workgroup advances rng_state[1] by one, so every launch / graph
 * replay draws fresh noise.  counter: one zeroed uint32, left zero.
 *
 * Counter layouts (Philox4x32-10 as in Random123: counter words c0..c3, key
 * (k0, k1) = (low, high) half of the seed, off_lo / off_hi the halves of the
 * offset; a 32-bit word x becomes the uniform (x >> 8) * 2^-24):
 *   u_gate[r]              = word 0 of the block of counter (r, 16, off_lo, off_hi)
 *   u_feat[r][4c .. 4c+3]  = the four words of counter (r, c, off_lo, off_hi),
 *                            c = 0..15, so the gate's word 1 (16) is no quad's
 *   dropout keep bits of row r (scgib_gt_ffn_fwd, a state of its own) = the
 *                            four words of (r_lo, tag ^ r_hi, off_lo, off_hi),
 *                            tag = 0x47544c31; bit c % 32 of word c / 32 keeps
 *                            column c, words in block order
 * The draws depend on (row, offset, seed) only, never on the grid. */
int scgib_noise_uniform(float *u_gate, float *u_feat, int64_t n_rows, uint64_t *rng_state,
                        uint32_t *counter, scgib_stream_t stream);

/* Sequential running-stat update of the per-graph compressor BatchNorm: one
 * nn.BatchNorm1d call per graph in graph order (models.py:642 inside the loop
 * of :639), i.e. B momentum updates with each graph's mean and unbiased var,
 * and num_batches_tracked += B. */
int scgib_bn_running_update(const float *stats, const int32_t *graph_ptr, int64_t n_graphs,
                            float momentum, float *running_mean, float *running_var,
                            int64_t *num_batches_tracked, scgib_stream_t stream);
/* The same update as an argument block, for launches that run it in an
 * extra workgroup beside their own work (scgib_mlp2_recon_contrastive_fwd). */
typedef struct {
    const float *stats;           /* scgib_interaction_fwd's per-graph statistics */
    const int32_t *graph_ptr;
    int64_t n_graphs;
    float momentum;
    float *running_mean, *running_var;
    int64_t *num_batches_tracked;
} scgib_running_update;

/* ---- (f)1: fine-tune prediction head + BCE (models.py:510-523) ------------
 * scgib_head_fwd: hid = relu(x W1^T + b1) [n,64] (saved), out = hid W2^T + b2
 *   [n,C], sigmoid applied when `sigmoid` (the reference's scores unless the
 *   dataset is a regression one, models.py:517-520); x [n,K], K <= 128 and a
 *   multiple of 4, C <= 16; x and w1 16-byte aligned (else SCGIB_EUNSUPPORTED).
 *   ru (may be NULL): the compressor BatchNorm's running update
 *   (scgib_running_update, below), run in one extra workgroup of the launch —
 *   nothing in the fine-tune step reads the running statistics, so it needs no
 *   launch of its own.
 * scgib_head_bwd: from d_out [n,C] (and out = the sigmoid output when
 *   `sigmoid`): dx [n,K], dW1 [64][K], db1 [64], dW2 [C][64], db2 [C]; four
 *   workgroups (dW1 row quarters, dx column quarters), each output summed in a
 *   fixed order.
 * scgib_bce_fwd / _bwd: F.binary_cross_entropy(scores, targets), mean over n
 *   elements (torch's per-element formula and log clamp at -100; fp64 fixed
 *   order sum), and d scores = g (s - t) / max((1 - s) s, 1e-12) / n with g the
 *   device scalar d loss (models.py:522-523). */
int scgib_head_fwd(const float *x, int64_t n_rows, int32_t k_in, const float *w1, const float *b1,
                   const float *w2, const float *b2, int32_t n_out, int32_t sigmoid, float *hid,
                   float *out, const scgib_running_update *ru, scgib_stream_t stream);
int scgib_head_bwd(const float *x, const float *hid, const float *out, const float *d_out,
                   int64_t n_rows, int32_t k_in, const float *w1, const float *w2, int32_t n_out,
                   int32_t sigmoid, float *dx, float *dw1, float *db1, float *dw2, float *db2,
                   scgib_stream_t stream);
int scgib_bce_fwd(const float *scores, const float *targets, int64_t n, float *loss,
                  scgib_stream_t stream);
int scgib_bce_bwd(const float *scores, const float *targets, int64_t n, const float *g_loss,
                  float *d_scores, scgib_stream_t stream);

/* ---- (f)2: wide task heads + NaN-masked task losses (ABI 24) --------------
 * The multi-label / regression fine-tunes (train_molpcba.py:108,
 * train_pep_func.py:131, train_molsider.py:109: 128 / 10 / 27 tasks; ToxCast
 * 617, Tox21 12) and the losses of models.py:522-543 taken through
 * MetricWrapper(metric, target_nan_mask="ignore-flatten") (MetricWrapper.py:
 * 64-66, target[~isnan(target)]: a data-dependent shape, hence a device-host
 * synchronise that no captured step can contain).
 * scgib_head_wide_fwd / _bwd: scgib_head_fwd / _bwd's formulas (models.py:
 *   510-520) for 16 < C <= 1024 outputs, K <= 128 and a multiple of 4; any
 *   other (K, C): SCGIB_EUNSUPPORTED, as are x, w1, w2, hid or dw2 not 16-byte
 *   aligned.  hid = relu(x W1^T + b1) [n,64] (saved), out = hid W2^T + b2
 *   [n,C] (sigmoid applied when `sigmoid`); W2 is walked in column tiles of 64
 *   staged in LDS, spread over the grid's second dimension.  ru: as
 *   scgib_head_fwd.  n = 0: the forward writes nothing, the backward zeroes
 *   the weight gradients.
 *   Backward, one launch: do = d_out * (sigmoid ? out (1 - out) : 1);
 *   ceil(C / 16) workgroups each own 16 rows of dW2 = do^T hid and db2 =
 *   sum_r do (every thread sums its outputs in row order); ceil(n / 16)
 *   workgroups each own 16 rows: dh = (do W2) [hid > 0], dx = dh W1 (written),
 *   and the partials of dW1 = dh^T x, db1 = sum_r dh into slab row b of
 *   64 K + 64 floats, which a scgib_slab_reduce_multi launch issued by this
 *   call sums in a fixed order (n <= 16: written to dw1 / db1 directly, no
 *   second launch, slab may be NULL).  slab: scgib_head_wide_slab_floats(n, K).
 * scgib_task_loss_fwd / _bwd: over scores, targets [n] (the flattened [rows,
 *   C]), with an element kept when !mask_nan or its target is not NaN, m the
 *   number kept, per kept element (fp32, torch's formulas)
 *     SCGIB_LOSS_BCE         (t-1) max(log(1-s),-100) - t max(log s,-100)
 *                              model.loss, models.py:522-523
 *     SCGIB_LOSS_BCE_LOGITS  max(x,0) - x t + log1p(exp(-|x|))
 *                              BCEWithLogitsLoss, models.py:536-539
 *     SCGIB_LOSS_MAE         |s - t|            lossMAE, models.py:541-543
 *     SCGIB_LOSS_RMSE        (s - t)^2          loss_RMSE, models.py:532-535
 *   loss = sum / m (RMSE: sqrt(sum / m)), NaN when m = 0 (torch's mean over
 *   an empty tensor); count = m (int32, device).  The sum is fp64 in a fixed
 *   order: at most 64 workgroups (a function of n only), each a fixed tree
 *   over its threads, the last to arrive adds the partials in workgroup
 *   order.  ws: scgib_task_loss_ws_doubles() doubles; counter: one zeroed
 *   uint32, left zero.  Backward, from g_loss (device scalar) and the
 *   forward's loss and count:
 *     BCE  g (s-t) / max((1-s) s, 1e-12) / m    BCE_LOGITS  g (sigmoid(x)-t) / m
 *     MAE  g sign(s-t) / m                      RMSE        g (s-t) / (m loss)
 *   and exactly 0 at elements left out (everywhere when m = 0).  Nothing is
 *   read back to the host and no shape depends on the data. */
enum { SCGIB_LOSS_BCE = 0, SCGIB_LOSS_BCE_LOGITS = 1, SCGIB_LOSS_MAE = 2, SCGIB_LOSS_RMSE = 3 };
int64_t scgib_head_wide_slab_floats(int64_t n_rows, int32_t k_in);
int scgib_head_wide_fwd(const float *x, int64_t n_rows, int32_t k_in, const float *w1,
                        const float *b1, const float *w2, const float *b2, int32_t n_out,
                        int32_t sigmoid, float *hid, float *out, const scgib_running_update *ru,
                        scgib_stream_t stream);
int scgib_head_wide_bwd(const float *x, const float *hid, const float *out, const float *d_out,
                        int64_t n_rows, int32_t k_in, const float *w1, const float *w2,
                        int32_t n_out, int32_t sigmoid, float *dx, float *dw1, float *db1,
                        float *dw2, float *db2, float *slab, scgib_stream_t stream);
int64_t scgib_task_loss_ws_doubles(void);
int scgib_task_loss_fwd(const float *scores, const float *targets, int64_t n, int32_t kind,
                        int32_t mask_nan, double *ws, uint32_t *counter, float *loss,
                        int32_t *count, scgib_stream_t stream);
int scgib_task_loss_bwd(const float *scores, const float *targets, int64_t n, int32_t kind,
                        int32_t mask_nan, const float *g_loss, const float *loss,
                        const int32_t *count, float *d_scores, scgib_stream_t stream);
/* ---- Class-index cross-entropy and TU accuracy (csrc/class_loss.hip) -------
 * (Entry points added to ABI 24: nothing existing changes.)
 * loss_CrossEntropy (models.py:527-530: F.cross_entropy on the scores and the
 * class column, train_tudataset.py:146, :205) and accuracy_TU
 * (metrics.py:146-159) in one launch.  scores [n_rows, n_classes] fp32 row
 * major; labels [n_rows] class indices of type label_type:
 *     SCGIB_LABEL_F32  masked when NaN (the device loaders' fill rows)
 *     SCGIB_LABEL_I32 / _I64  masked when -100 (torch's ignore_index)
 * A label that is neither masked nor an integer in [0, n_classes) (1.5, -1,
 * n_classes, +-inf) makes the row invalid: counted in *invalid, no loss, no
 * hit, no count, zero gradient, and it indexes nothing.  Per kept row, fp32:
 *     l_r = log(sum_c exp(s_rc - m_r)) + m_r - s_ry,  m_r the row maximum
 * (torch's log_softmax + nll); a row's hit: its argmax equals y, with torch's
 * argmax order (a NaN above every number, the lowest index among equals).
 * loss = sum l_r / count, NaN when count = 0; the sum is fp64 in a fixed
 * order (a group of 2, 8, 32 or 64 lanes per row by n_classes, a wavefront's
 * rows by a fixed butterfly and its sweeps in order, the four wavefronts of a
 * workgroup in order, at most 64 workgroups in workgroup order by the last to
 * arrive; one workgroup — up to 128 rows of two classes — writes the outputs
 * itself and touches neither ws nor counter).  ws:
 * scgib_class_loss_ws_doubles() doubles,
 * 8-byte aligned; counter: one zeroed uint32, left zero.  epoch (or NULL): 5
 * doubles { sum of loss, batches, hits, labelled, invalid }: a batch with a
 * kept row adds its loss, 1, hits and count; every batch adds invalid (one
 * thread; launches on one stream are ordered).
 * Backward, from g_loss (device scalar) and the forward's count:
 *     d s_rc = g (softmax(s_r)_c - [c = y_r]) / count
 * at kept rows, the softmax recomputed from the scores; exactly 0 at masked
 * and invalid rows and everywhere when count = 0.
 * 1 <= n_classes <= 1024 and 1 <= n_rows <= 2^30, otherwise SCGIB_EINVAL /
 * SCGIB_EUNSUPPORTED and nothing is launched. */
enum { SCGIB_LABEL_F32 = 0, SCGIB_LABEL_I32 = 1, SCGIB_LABEL_I64 = 2 };
int64_t scgib_class_loss_ws_doubles(void);
int scgib_class_loss_fwd(const float *scores, const void *labels, int32_t label_type,
                         int64_t n_rows, int32_t n_classes, double *ws, uint32_t *counter,
                         float *loss, int32_t *count, int32_t *hits, int32_t *invalid,
                         double *epoch, scgib_stream_t stream);
int scgib_class_loss_bwd(const float *scores, const void *labels, int32_t label_type,
                         int64_t n_rows, int32_t n_classes, const float *g_loss,
                         const int32_t *count, float *d_scores, scgib_stream_t stream);
/* Backward of scgib_interaction_fwd.  The KL gradient is g_kl [2 n_last, 64],
 * or g_klmean (device scalar, gradient of kl_mean), or neither (both NULL);
 * g_z1 / g_z2 may be NULL (readouts that feed no loss: zero gradient).
 * pad_rows: zero rows [graph_ptr[B], n_nodes) of df, dt, ds.
 * Outputs df, dt, ds [N,64] and per-graph parameter-gradient partials
 * pgrad[B, SCGIB_PGRAD_STRIDE] laid out as
 *   [0,64) dW2 | 64 db2 | [65,129) dgamma | [129,193) dbeta |
 *   [193,321) dW_att | 321 db_att
 * If pgrad_total (SCGIB_PGRAD_STRIDE floats) is given, the fixed-order sum
 * over graphs (the parameter gradients) is written there as well. */
int scgib_interaction_bwd(const float *g_im, const float *g_z1, const float *g_z2,
                          const float *g_kl, const float *f, const float *t, const float *s,
                          const float *u_feat, const int32_t *graph_ptr, int64_t n_graphs,
                          int64_t n_nodes, const float *bn_gamma, const float *bn_beta,
                          const float *bn_running_mean, const float *bn_running_var,
                          float bn_eps, int32_t training, const float *w2,
                          const float *w_att, const float *z1, const float *lam,
                          const float *logit, const float *stats, float *df, float *dt,
                          float *ds, float *pgrad, const float *g_klmean, int32_t pad_rows,
                          float *pgrad_total, scgib_stream_t stream);
/* The same pair with the attention selectable (scgib_interaction_fwd / _bwd
 * are use_att = 1).  use_att = 0 is the reference's useAtt = 0
 * (models.py:726): im[:, 64:] is the s row itself, logit is not written and
 * the softmax / z-bar constant slots of stats are zero; the backward gives
 * ds = g_im[:, 64:] and writes zeros for dW_att / db_att in pgrad.  w_att and
 * b_att are still required (not read).  A forward and its backward take the
 * same use_att. */
int scgib_interaction_fwd_v2(const float *f, const float *t, const float *s,
                             const float *u_gate, const float *u_feat, const int32_t *graph_ptr,
                             int64_t n_graphs, int64_t n_nodes, const float *bn_gamma,
                             const float *bn_beta, const float *bn_running_mean,
                             const float *bn_running_var, float bn_eps, int32_t training,
                             const float *w2, const float *b2, const float *w_att,
                             const float *b_att, float *im, float *z1, float *z2, float *lam,
                             float *logit, float *stats, float *kl_tensor, float *kl_mean,
                             int32_t pad_rows, int32_t use_att, scgib_stream_t stream);
int scgib_interaction_bwd_v2(const float *g_im, const float *g_z1, const float *g_z2,
                             const float *g_kl, const float *f, const float *t, const float *s,
                             const float *u_feat, const int32_t *graph_ptr, int64_t n_graphs,
                             int64_t n_nodes, const float *bn_gamma, const float *bn_beta,
                             const float *bn_running_mean, const float *bn_running_var,
                             float bn_eps, int32_t training, const float *w2,
                             const float *w_att, const float *z1, const float *lam,
                             const float *logit, const float *stats, float *df, float *dt,
                             float *ds, float *pgrad, const float *g_klmean, int32_t pad_rows,
                             float *pgrad_total, int32_t use_att, scgib_stream_t stream);

/* ---- A12: adjacency reconstruction loss, Gram form ------------------------
 * loss = sum_{u,v} (<im_u, im_v> - A_uv)^2 / N
 *      = (||IM^T IM||_F^2 - 2 sum_{(u,v) in E} <im_u, im_v> + |E|) / N
 * exactly (A 0/1, simple graph) — replaces the dense N x N form of
 * loss_recon_adj (models.py:762-768).  Two launches: partial Gram slabs
 * (MFMA f32 32x32x2) + edge dot products, then a fixed-order fp64 finalize.
 * `partials` holds scgib_recon_partials_floats(n) floats.
 * Outputs: gram[64*64] (for backward) and loss[1]. */
int64_t scgib_recon_partials_floats(int64_t n_nodes);
int scgib_recon_fwd(const float *im, const int32_t *rowptr, const int32_t *col,
                    int64_t n_nodes, int64_t n_edges, float *partials, float *gram,
                    float *loss, const int32_t *dims, scgib_stream_t stream);
/* d loss / d im = (g_loss / N) * (4 IM G - 2 (A + A^T) IM); pass the in-CSR and
 * the out-CSR (the same arrays for a symmetric graph).  g_loss is a device
 * scalar. */
int scgib_recon_bwd(const float *im, const float *gram, const int32_t *rowptr_in,
                    const int32_t *col_in, const int32_t *rowptr_out, const int32_t *col_out,
                    int64_t n_nodes, const float *g_loss, float *grad_im,
                    const int32_t *dims, scgib_stream_t stream);

/* ---- A15: logM reconstruction loss (models.py:770-782) --------------------
 * loss = (1/k) sum_g sum_i ||X_g X_g^T - logM_g,i||_F^2 / n_g^2, X_g = the rows
 * of `im` [N][64] of molecule g (graph_ptr).  Targets per molecule, packed at
 * int64 s_offsets[B+1] (n_g^2 floats each): S = sum_i logM_i, and
 * C[g] = sum_i ||logM_i||^2 (fp64).  loss_graphs [B] holds per-molecule terms;
 * loss is a device scalar (fixed-order sum).  Backward: grad_im [N][64] =
 * 2 g_loss (2k X X^T - S - S^T) X / (k n_g^2) per molecule. */
int scgib_recon_logm_fwd(const float *im, const int32_t *graph_ptr, int64_t n_graphs,
                         const float *S, const int64_t *s_offsets, const double *C,
                         int32_t kstep, float *loss_graphs, float *loss, scgib_stream_t stream);
int scgib_recon_logm_bwd(const float *im, const int32_t *graph_ptr, int64_t n_graphs,
                         const float *S, const int64_t *s_offsets, int32_t kstep,
                         const float *g_loss, float *grad_im, scgib_stream_t stream);

/* ---- A15, on the device: logM targets from the ego-nets, sparse loss -------
 * (csrc/logm.hip)  L_i[r,c] = max(0, log(A^i[r,c] /
 * colsum_i[c]) - log(1/n_g)) (util.py:60-91) is zero unless r lies in the
 * k-hop ball of c, so the targets live on the slots of the k-hop ego batch of
 * the same graph (scgib_egonet_*: slot j of ball(c) <-> r = ego_nodes[j],
 * ego_ptr [n_nodes + 1], every ball sorted and holding c).
 *
 * scgib_logm_targets: the batch's dst-major CSR (a symmetric graph: the walk
 *   counts of r -> c and c -> r are taken to be equal), graph_ptr [B + 1],
 *   kstep = k.  Writes, per slot, s_in = sum_i L_i[r,c] and
 *   s_sym = sum_i (L_i[r,c] + L_i[c,r]) (fp32; each term formed in fp64 and
 *   rounded to fp32 as the reference's targets are, then summed in fp64), and
 *   per molecule C[g] = sum_i ||L_i||_F^2 (fp64, fixed-order sum).  counts:
 *   scratch of kstep * n_ego uint32 (the walk counts, exact integers).
 *   Domain: 1 <= kstep <= scgib_logm_max_k() (8; else SCGIB_EUNSUPPORTED),
 *   molecules of at most scgib_logm_max_graph_nodes() (512) nodes, every walk
 *   count below 2^31 — which holds whenever (max in-degree)^kstep < 2^31, e.g.
 *   kstep <= 8 at in-degree <= 12.  Outside it nothing wrong is returned
 *   silently: bits are set in *err (device int32, zeroed by the caller or
 *   shared with the ego builder's): 1 an index leaves its molecule or buffer,
 *   2 a molecule above 512 nodes, 4 a walk count at or above 2^31; the
 *   affected molecule's targets are then zero or partial and its loss term
 *   and gradient rows are zero (bits 1, 2).  The reference's quirks are kept:
 *   log(1/n) uses the molecule's own n; a count of 0, a column without
 *   in-edges (its NaN) and negative values give 0.
 * scgib_recon_logm_sparse_fwd: loss = sum_g (k ||G_g||_F^2 - 2 sum_slots s_in
 *   <x_r, x_c> + C_g) / (k n_g^2), G_g = X_g^T X_g (exact-f32 MFMA), the three
 *   terms combined in fp64.  gram [B][64*64] is saved for the backward; parts
 *   holds B * scgib_recon_logm_sparse_parts(max_graph_nodes) doubles;
 *   loss_graphs [B]; loss a device scalar.  max_graph_nodes (host bound on
 *   the molecule size) only sizes the grid.
 * scgib_recon_logm_sparse_bwd: grad_im row c = g_loss (4k (X G)_c - 2 sum_{j
 *   in ball(c)} s_sym[j] x_{r_j}) / (k n_g^2).
 * Capacity mode (dims = the batch's device [nodes, edges], n_nodes / n_edges /
 * n_ego the capacities): live counts are read on the device, a padded molecule
 * (n = 0) contributes 0, grad rows in [live N, n_nodes) are written as zeros;
 * nothing is read back. */
int64_t scgib_logm_max_k(void);
int64_t scgib_logm_max_graph_nodes(void);
int scgib_logm_targets(const int32_t *rowptr, const int32_t *col, const int32_t *graph_ptr,
                       int64_t n_graphs, int64_t n_nodes, int64_t n_edges,
                       const int32_t *ego_ptr, const int32_t *ego_nodes, int64_t n_ego,
                       int32_t kstep, uint32_t *counts, float *s_in, float *s_sym, double *C,
                       int32_t *err, const int32_t *dims, scgib_stream_t stream);
int64_t scgib_recon_logm_sparse_parts(int64_t max_graph_nodes);
int scgib_recon_logm_sparse_fwd(const float *im, const int32_t *graph_ptr, int64_t n_graphs,
                                int64_t n_nodes, const int32_t *ego_ptr,
                                const int32_t *ego_nodes, int64_t n_ego, const float *s_in,
                                const double *C, int32_t kstep, int64_t max_graph_nodes,
                                float *gram, double *parts, float *loss_graphs, float *loss,
                                const int32_t *dims, scgib_stream_t stream);
int scgib_recon_logm_sparse_bwd(const float *im, const int32_t *graph_ptr, int64_t n_graphs,
                                int64_t n_nodes, const int32_t *ego_ptr,
                                const int32_t *ego_nodes, int64_t n_ego, const float *s_sym,
                                const float *gram, int32_t kstep, int64_t max_graph_nodes,
                                const float *g_loss, float *grad_im, const int32_t *dims,
                                scgib_stream_t stream);

/* ---- A11: contrastive loss (batched_semi_loss, tau = 1) --------------------
 * models.py:606-629 (sim :606-609, semi_loss :611-616, batched :618-629;
 * called at models.py:695 with z1 = sum_nodes(noisy), z2 = graph readout).
 * loss = mean_i -log(exp(z1n_i.z2n_i) / (sum_j exp(z1n_i.z1n_j)
 *        + sum_j exp(z1n_i.z2n_j) - exp(z1n_i.z1n_i))),  zn = F.normalize(z).
 * The value is independent of the reference's chunk size.  z1, z2: [B][64].
 * `workspace` holds scgib_contrastive_workspace_floats(B) floats and must be
 * passed unchanged from forward to backward.  `counters` holds
 * scgib_contrastive_counters(B) uint32 that are zero on entry; both launches
 * leave them zero (graph-replay safe).  loss and g_loss are device scalars. */
int64_t scgib_contrastive_workspace_floats(int64_t n_graphs);
int64_t scgib_contrastive_counters(int64_t n_graphs);
int scgib_contrastive_fwd(const float *z1, const float *z2, int64_t n_graphs, float *workspace,
                          float *loss, uint32_t *counters, scgib_stream_t stream);
int scgib_contrastive_bwd(const float *z1, const float *z2, int64_t n_graphs, float *workspace,
                          const float *g_loss, float *dz1, float *dz2, uint32_t *counters,
                          scgib_stream_t stream);
/* The same at row width `width` = 64 (the entries above) or 128 (the Set2Set
 * readouts, models.py:686 / :718); any other width: SCGIB_EUNSUPPORTED.  The
 * workspace grows with the width (scgib_contrastive_workspace_floats_w);
 * scgib_contrastive_counters does not depend on it. */
int64_t scgib_contrastive_workspace_floats_w(int64_t n_graphs, int32_t width);
int scgib_contrastive_fwd_w(const float *z1, const float *z2, int64_t n_graphs, int32_t width,
                            float *workspace, float *loss, uint32_t *counters,
                            scgib_stream_t stream);
int scgib_contrastive_bwd_w(const float *z1, const float *z2, int64_t n_graphs, int32_t width,
                            float *workspace, const float *g_loss, float *dz1, float *dz2,
                            uint32_t *counters, scgib_stream_t stream);

/* ---- A10 head: fused dense layers (exact-f32 MFMA tiles) -----------------
 * mlp2: out = relu(x W1^T + b1) W2^T + b2, x [N][d_in] (d_in 64 or 128),
 * W1 [64][d_in], W2 [64][64] — the interaction-map MLP of Mainmodel /
 * Mainmodel_continue (models.py:569-571 / :1055-1057, applied at :676 /
 * :1174).  Forward saves r = relu(x W1^T + b1) [N][64] for backward.
 * Backward: dx [N][d_in] and wgrad = dW2[64*64] | dW1[64*d_in] | db2 | db1
 * (fixed-order, deterministic); `slab` holds scgib_mlp2_slab_floats(n, d_in)
 * (d_in = 128 on few tiles: two workgroups, two slab rows, per tile — ABI 19);
 * wgrad NULL: the slabs are left for the caller's reduce (a deferred one).
 * linear: out = x W^T (+ b), 64 -> 64 — compressor[0] (models.py:589-592 /
 * :1081-1084, applied at :596 / :1092).  Backward writes dx = add + dy W
 * (`add` may be NULL) and wgrad = dW[64*64] | db[64]; `slab` holds
 * scgib_linear_slab_floats(n).  Capacity mode as above (dims). */
int64_t scgib_mlp2_slab_floats(int64_t n_nodes, int32_t d_in);
int64_t scgib_mlp2_recon_slab_floats(int64_t n_nodes, int32_t d_in);
int scgib_mlp2_fwd(const float *x, int32_t d_in, int64_t n_nodes, const float *w1,
                   const float *b1, const float *w2, const float *b2, float *r, float *out,
                   const int32_t *dims, scgib_stream_t stream);
int scgib_mlp2_bwd(const float *dout, const float *x, const float *r, int32_t d_in,
                   const float *w1, const float *w2, int64_t n_nodes, float *dx, float *slab,
                   float *wgrad, const int32_t *dims, scgib_stream_t stream);
/* mlp2 + recon (fused): the interaction-map MLP followed by loss_recon_adj
 * on its output (models.py:1174 then :1256-1262, i.e. Mainmodel_continue's
 * forward with recons_type 'adj'; replaces scgib_mlp2_fwd + scgib_recon_fwd
 * and their backward).  Forward: out (= IM), r, and loss; `ws` holds
 * scgib_mlp2_recon_ws_floats(n) floats (per-tile Gram partials, G, loss
 * partials) and must be passed unchanged to the backward; `counter` is three
 * zeroed uint32, left zero; `fault` (or NULL) is scgib_stream_wait's sticky
 * hand-off fault word: while it is set, *loss is NaN.  When the launch's workgroups are all co-resident
 * the MLP tiles also finish the loss (no second launch; the same bits either
 * way).  Backward: dx = d loss / d x and wgrad as
 * scgib_mlp2_bwd, for d loss / d recon = *g_loss; rowptr_t/col_t NULL for a
 * symmetric graph (A = A^T).  wgrad NULL: the per-workgroup slabs
 * (scgib_mlp2_recon_slab_floats(n, d_in) floats, width 64*64 + 64*d_in + 128) are
 * left for the caller's scgib_slab_reduce(_multi) — the model path defers
 * them into an encoder chain's final reduce, off the loss section. */
int64_t scgib_mlp2_recon_ws_floats(int64_t n_nodes);
/* Testing hook: 0 = always finish the recon loss in its own launch; returns
 * the previous setting (default 1). */
int scgib_set_recon_fold(int on);
int scgib_mlp2_recon_fwd(const float *x, int32_t d_in, int64_t n_nodes, const float *w1,
                         const float *b1, const float *w2, const float *b2, float *r, float *out,
                         const int32_t *rowptr, const int32_t *col, int64_t n_edges, float *ws,
                         uint32_t *counter, float *loss, const int32_t *dims,
                         const uint32_t *fault, scgib_stream_t stream);
int scgib_mlp2_recon_bwd(const float *x, const float *r, const float *out, const float *ws,
                         int32_t d_in, const float *w1, const float *w2, int64_t n_nodes,
                         const int32_t *rowptr, const int32_t *col, const int32_t *rowptr_t,
                         const int32_t *col_t, const float *g_loss, float *dx, float *slab,
                         float *wgrad, const int32_t *dims, scgib_stream_t stream);
/* The same with the contrastive loss (scgib_contrastive_fwd / _bwd: z1, z2
 * [n_graphs][64], cws / ccounters as documented there) run in extra
 * workgroups of the MLP launches — one launch on the step's critical chain
 * instead of two each way.  d_in must be 128 (the pretraining head).
 * Forward also writes *closs; backward takes d loss / d contrastive =
 * *g_con and writes dz1, dz2.  ru (forward, or NULL): the compressor
 * BatchNorm's running-stat update (scgib_bn_running_update) in one more
 * workgroup of the loss-finishing launch, off the critical path without a
 * second stream. */
int scgib_mlp2_recon_contrastive_fwd(const float *x, int32_t d_in, int64_t n_nodes,
                                     const float *w1, const float *b1, const float *w2,
                                     const float *b2, float *r, float *out,
                                     const int32_t *rowptr, const int32_t *col, int64_t n_edges,
                                     float *ws, uint32_t *counter, float *loss,
                                     const int32_t *dims, const float *z1, const float *z2,
                                     int64_t n_graphs, float *cws, float *closs,
                                     uint32_t *ccounters, const scgib_running_update *ru,
                                     const uint32_t *fault, scgib_stream_t stream);
int scgib_mlp2_recon_contrastive_bwd(const float *x, const float *r, const float *out,
                                     const float *ws, int32_t d_in, const float *w1,
                                     const float *w2, int64_t n_nodes, const int32_t *rowptr,
                                     const int32_t *col, const int32_t *rowptr_t,
                                     const int32_t *col_t, const float *g_loss, float *dx,
                                     float *slab, float *wgrad, const int32_t *dims,
                                     const float *z1, const float *z2, int64_t n_graphs,
                                     float *cws, const float *g_con, float *dz1, float *dz2,
                                     uint32_t *ccounters, scgib_stream_t stream);
int64_t scgib_linear_slab_floats(int64_t n_nodes);
int scgib_linear_fwd(const float *x, int64_t n_nodes, const float *w, const float *b, float *out,
                     const int32_t *dims, scgib_stream_t stream);
/* The encoder output's BatchNorm + ReLU with compressor[0] behind it, one
 * launch (csrc/dense.hip; an entry point only: the ABI version stays 24, as
 * for the other entries added since).  Replaces scgib_bn_relu_apply followed
 * by scgib_linear_fwd on its output, where the encoder pair folds
 * compressor[0] (models.py:596 / :1092 after GIN.forward's last BatchNorm +
 * ReLU, :66-72):
 *   f_out = relu(scale z2 + shift),  t_out = f_out w0^T (+ b0, may be NULL)
 * [n_nodes][64] each, bitwise the two entries' results.  scale / shift come
 * from `stat` ([4][64] record), or, with `pending` (may be NULL; n_nodes <=
 * scgib_gin_defer_max_nodes()), from the last layer's deferred statistics:
 * finished here, the record and the running statistics are then written
 * exactly once.  One 64-row tile per workgroup; the f tile stays in LDS
 * between the two steps.  dims (may be NULL): rows >= dims[0] of both
 * outputs are zeros, and every element up to n_nodes is written. */
int scgib_enc_out_linear_fwd(const float *z2, const float *stat, int64_t n_nodes,
                             const float *w0, const float *b0, float *f_out, float *t_out,
                             const int32_t *dims, const scgib_bn_pending *pending,
                             scgib_stream_t stream);
/* wgrad NULL: the slabs (scgib_linear_slab_floats(n) floats, width 64*64 + 64)
 * are left for the caller's reduce. */
int scgib_linear_bwd(const float *dy, const float *x, const float *w, int64_t n_nodes,
                     const float *add, float *dx, float *slab, float *wgrad,
                     const int32_t *dims, scgib_stream_t stream);

/* ---- optimizer: one-launch Adam over a tensor list ------------------------
 * torch.optim.Adam(params, lr, betas, eps, weight_decay) as every reference
 * training script builds it (exp_pretraining.py / exp_molhiv.py:53,
 * weight_decay=5e-5; fine-tune :157 1e-5), fused-Adam arithmetic: per
 * tensor t = *step + 1, g += wd p, m = b1 m + (1-b1) g, v = b2 v + (1-b2) g^2,
 * p -= lr/(1-b1^t) * m / (sqrt(v)/sqrt(1-b2^t) + eps), *step = t (fp32
 * device scalar per tensor, like torch's capturable state['step']); the
 * hyper-parameters are doubles and enter the moment updates in double, as
 * in torch's fused kernel.
 * n_tensors <= scgib_adam_max_tensors(); the table is copied into the kernel
 * arguments (HIP-graph capturable).  `counter`: one uint32, zero on entry,
 * left zero. */
typedef struct {
    float *param;
    const float *grad;
    float *exp_avg;
    float *exp_avg_sq;
    float *step;
    int64_t numel;
} scgib_adam_tensor;
int64_t scgib_adam_max_tensors(void);
int scgib_adam_step(const scgib_adam_tensor *tensors, int32_t n_tensors, double lr,
                    double beta1, double beta2, double eps, double weight_decay,
                    uint32_t *counter, scgib_stream_t stream);
/* scgib_slab_reduce_multi(jobs) followed by scgib_adam_step(tensors) in ONE
 * launch, with the same bits: a tensor whose gradient lies inside a job's
 * output is updated by the reduce's workgroups from the value they produce
 * (the replayed pretraining step's last weight-gradient reduce and its Adam
 * step, models.py's training loop exp_pretraining.py:321-323 — no reference
 * counterpart of its own; ABI 22).  n_jobs <= scgib_adam_reduce_max_jobs();
 * a gradient that straddles a job output's edge, or two tensors' gradients
 * overlapping inside one: SCGIB_EINVAL. */
int64_t scgib_adam_reduce_max_jobs(void);
int scgib_adam_step_reduce(const scgib_adam_tensor *tensors, int32_t n_tensors,
                           const scgib_slab_job *jobs, int32_t n_jobs, double lr, double beta1,
                           double beta2, double eps, double weight_decay, uint32_t *counter,
                           scgib_stream_t stream);

/* AdamW by value: the two launches above with decoupled weight decay, the
 * arithmetic of torch.optim.AdamW(fused=True): p -= lr wd p (in double,
 * rounded to fp32) before the update, nothing added to g.  (Entry points only,
 * as everything below in this section: the ABI version stays 24.) */
int scgib_adamw_step(const scgib_adam_tensor *tensors, int32_t n_tensors, double lr,
                     double beta1, double beta2, double eps, double weight_decay,
                     uint32_t *counter, scgib_stream_t stream);
int scgib_adamw_step_reduce(const scgib_adam_tensor *tensors, int32_t n_tensors,
                            const scgib_slab_job *jobs, int32_t n_jobs, double lr, double beta1,
                            double beta2, double eps, double weight_decay, uint32_t *counter,
                            scgib_stream_t stream);

/* ---- optimizer: hyper-parameters read from the device ------
 * A captured launch of scgib_adam_step freezes lr / betas / eps / weight_decay
 * in its graph node.  The _dyn launches read them from a device block that
 * only host copies write (one scgib_optim_hyper per param group), so a
 * learning-rate schedule, gradient clipping and the skipping of a non-finite
 * step run inside a replayed step without a host synchronisation:
 *   lr_t = lr * factor(c), c = state->calls as the step found it;
 *   c < warmup: factor = warmup_start + (1 - warmup_start) c / warmup, else
 *   u = clamp((c - warmup) / max(total - warmup, 1), 0, 1) and factor = 1
 *   (CONSTANT), 1 - (1 - min_ratio) u (LINEAR), min_ratio + (1 - min_ratio)
 *   0.5 (1 + cos(pi u)) (COSINE), all in double, by every workgroup for itself.
 * The blocks are 8-byte aligned and zeroed before their first use. */
enum { SCGIB_SCHED_CONSTANT = 0, SCGIB_SCHED_LINEAR = 1, SCGIB_SCHED_COSINE = 2 };
typedef struct {
    double lr, beta1, beta2, eps, weight_decay;
    double warmup_start, min_ratio;
    double max_grad_norm; /* < 0: no clipping (coef = 1); read by scgib_grad_norm */
    int64_t warmup, total;
    int32_t kind;         /* SCGIB_SCHED_* */
    int32_t pad_;
} scgib_optim_hyper;      /* 88 bytes */
typedef struct {
    double sumsq;         /* S = sum (double)g (double)g of the step's gradients */
    float norm;           /* (float)sqrt(S), before clipping */
    float coef;           /* min(1, max_grad_norm / (norm + 1e-6f)), fp32 (NaN stays NaN) */
    int32_t finite;       /* isfinite(norm) */
    int32_t pad_;
    int64_t calls;        /* steps taken, skipped ones included */
    int64_t skipped;
} scgib_optim_state;      /* 40 bytes */
enum {
    SCGIB_OPTIM_NORM = 1,    /* a scgib_grad_norm preceded: use g * state->coef */
    SCGIB_OPTIM_SKIP = 2,    /* with _NORM: state->finite == 0 changes no tensor */
    SCGIB_OPTIM_ADVANCE = 4  /* the step's last launch: calls (and skipped) advance */
};
/* scgib_grad_norm: the global L2 norm of the table's gradients in a fixed
 * order (1024-element chunks, a fixed tree per workgroup, the chunk partials
 * added by the last workgroup to arrive in an order that depends on their
 * number alone): bitwise reproducible, no floating-point atomics.  ws:
 * scgib_grad_norm_ws_doubles(scgib_grad_norm_chunks(tensors, n)) doubles,
 * written before they are read; counter: one uint32, zero on entry, left zero.
 * More than scgib_adam_max_tensors() tensors take several launches: first != 0
 * on the first starts state->sumsq, each adds its total in launch order,
 * last != 0 on the last writes norm, coef and finite.  hyper: the block whose
 * max_grad_norm applies (the norm is global: group 0's).  Only .grad and
 * .numel (and the validity of the other fields) of the table matter. */
int64_t scgib_grad_norm_chunks(const scgib_adam_tensor *tensors, int32_t n_tensors);
int64_t scgib_grad_norm_ws_doubles(int64_t n_chunks);
int scgib_grad_norm(const scgib_adam_tensor *tensors, int32_t n_tensors, double *ws,
                    uint32_t *counter, const scgib_optim_hyper *hyper, scgib_optim_state *state,
                    int32_t first, int32_t last, scgib_stream_t stream);
/* scgib_adam_step / _step_reduce with the hyper-parameters of `hyper` (this
 * launch's param group), the same adam_elem / adam_coef.  flags: SCGIB_OPTIM_*;
 * decoupled != 0: AdamW.  The last workgroup writes *last_lr = lr_t and, with
 * SCGIB_OPTIM_ADVANCE, advances state->calls (and ->skipped on a skip); on a
 * skip no parameter, moment or tensor step changes.  n_tensors = 0 with
 * _ADVANCE still counts the call.  The fused reduce has no norm launch before
 * it: _NORM / _SKIP there are SCGIB_EINVAL. */
int scgib_adam_step_dyn(const scgib_adam_tensor *tensors, int32_t n_tensors,
                        const scgib_optim_hyper *hyper, scgib_optim_state *state,
                        double *last_lr, int32_t flags, int32_t decoupled, uint32_t *counter,
                        scgib_stream_t stream);
int scgib_adam_step_reduce_dyn(const scgib_adam_tensor *tensors, int32_t n_tensors,
                               const scgib_slab_job *jobs, int32_t n_jobs,
                               const scgib_optim_hyper *hyper, scgib_optim_state *state,
                               double *last_lr, int32_t flags, int32_t decoupled,
                               uint32_t *counter, scgib_stream_t stream);


/* ---- data parallelism: gradient bucket (dist.GradAllReducer) --------------
 * scgib_grad_pack: flat[offset + i] = data[i] for every slice, one launch;
 * scgib_grad_unpack: data[i] = scale * flat[offset + i] (scale = 1/world after
 * the all-reduce SUM).  n_tensors <= scgib_grad_pack_max_tensors(); the table
 * is copied into the kernel arguments (HIP-graph capturable). */
typedef struct {
    float *data;
    int64_t numel;
    int64_t offset;
} scgib_grad_slice;
int64_t scgib_grad_pack_max_tensors(void);
int scgib_grad_pack(const scgib_grad_slice *tensors, int32_t n_tensors, float *flat,
                    scgib_stream_t stream);
int scgib_grad_unpack(const scgib_grad_slice *tensors, int32_t n_tensors, const float *flat,
                      float scale, scgib_stream_t stream);

/* ---- evaluation metrics on the device (csrc/eval_metrics.hip)
 * metrics.py:18-87 (eval_rocauc / eval_ap / eval_rmse / eval_acc: per task
 * column, NaN labels left out) and the score concatenation of the loops
 * (train_molpcba.py:156-159, :165-207), without a host copy.
 *
 * scgib_eval_append: copies scores / targets [n_rows][n_tasks] to row state[0]
 *   of buf_scores / buf_labels [capacity][n_tasks] and advances state[0] (the
 *   launch's last workgroup does, so a captured launch appends on every
 *   replay).  state: three uint32 — the row cursor, an arrival counter (zero on
 *   entry, left zero) and the error word.  Rows that would pass `capacity` are
 *   not written; the cursor then stops at `capacity` and error bit 1 is set.
 * scgib_eval_keys: tasks [task0, task0 + n_group) of the row-major scores /
 *   labels [n_rows][n_tasks] -> task-major keys [n_group][n_rows] (int64):
 *   ((~o(score)) << 1) | label, o the order-preserving uint32 image of the
 *   fp32 score (-0.0 as +0.0), so ascending keys are descending scores with
 *   the label in bit 0; an element whose label is not 0 or 1, and every row at
 *   or past *rows (device uint32, NULL: n_rows), gets INT64_MAX.  Per row tile
 *   t < scgib_eval_tiles(n_rows) and task c it writes sq_slab[t][c] (fp64
 *   squared error over the labelled elements) and cnt_slab[t][c][4] (labels
 *   equal to 1, equal to 0, not NaN, equal to their score).  Error bits OR-ed
 *   into *err: 2 a NaN score under a label that is not NaN, 4 a label that is
 *   neither 0, 1 nor NaN.
 * scgib_eval_scan: `sorted` = the keys sorted ascending along each row (any
 *   sort; only values).  Writes out[4][n_tasks] (fp64: ROC-AUC, average
 *   precision, RMSE, accuracy; NaN where undefined — a rank metric of a task
 *   without both classes, RMSE / accuracy of a task without labelled rows)
 *   and counts[3][n_tasks] (int32: labels 1, labels 0, labelled) for the
 *   group's tasks.  Integer sums are exact, fp64 sums have a fixed order:
 *   bitwise reproducible, and independent of how the tasks are grouped. */
int64_t scgib_eval_tiles(int64_t n_rows);
int scgib_eval_append(const float *scores, const float *targets, int64_t n_rows, int32_t n_tasks,
                      float *buf_scores, float *buf_labels, int64_t capacity, uint32_t *state,
                      scgib_stream_t stream);
int scgib_eval_keys(const float *scores, const float *labels, int64_t n_rows, int32_t n_tasks,
                    int32_t task0, int32_t n_group, const uint32_t *rows, int64_t *keys,
                    double *sq_slab, int32_t *cnt_slab, uint32_t *err, scgib_stream_t stream);
int scgib_eval_scan(const int64_t *sorted, int64_t n_rows, int32_t n_tasks, int32_t task0,
                    int32_t n_group, const double *sq_slab, const int32_t *cnt_slab, double *out,
                    int32_t *counts, scgib_stream_t stream);

/* Device-side collation of shuffled batches from a resident dataset
 * (collate.hip; graph.DeviceDataset / graph.DeviceLoader).
 * Entry points only: the ABI version does not change.
 *
 * The dataset: M molecules as flat arrays — node_off / edge_off [M+1] (64-bit
 * offsets of each molecule's nodes and edges), rp_local [nodes] (row pointer
 * of each node inside its molecule's edge range), col [edges] (molecule-local
 * source ids, dst-major CSR), x [nodes][F], y [M][T] (T = 0: none),
 * ego_nodes / ego_edges [M] (the molecule's k-hop ego bounds).
 * The sequence: perm [2][M] holds the permutations of epochs of even and odd
 * number; state[0] is the position j in [0, 2S) (S batches of B per epoch),
 * state[1] the sticky count of batches that did not fit.  Batch j is
 * perm[j / S][(j % S) * B .. + B).  perm holds molecule ids below D, the
 * dataset's molecule count (D = 0: below M), so a loader over a subset of a
 * larger dataset has M = the subset's length and D = the dataset's.
 * The ring: srcs = table of three slot pointers, each blob_bytes long in
 * StaticBatch's layout (sections rowptr [n_cap+1], col [max(e_cap,1)],
 * graph_ptr [B+1], dims [4], x [n_cap][F] at the byte offsets o_*, multiples
 * of 16); cursor = the pool cursor scgib_pool_copy advances.
 *
 * scgib_collate_plan (one workgroup, B <= scgib_collate_max_batch()): the ids
 *   of batch state[0] + ahead, their node / edge offsets into ws (int32,
 *   scgib_collate_ws_words(B)) and, when the batch fits n_cap, e_cap and the
 *   ego capacities, into slot_ids [3][B] at the destination slot: `slot` in
 *   0..2, or -1 = (cursor[0] + 1) % 3.  Else state[1] is bumped.  advance:
 *   state[0] moves on by one.
 * scgib_collate_fill: writes the planned batch into its slot — every byte of
 *   the five sections, tails as StaticBatch.pad writes them — or nothing when
 *   the plan found it not to fit; labels != 0: also gathers the labels [B][T]
 *   and ids [B] of the batch in slot (cursor[0] + 2) % 3 (the one the step's
 *   scgib_pool_copy read) as the plan saw the cursor. */
typedef struct {
    const int64_t *node_off, *edge_off;
    const int32_t *rp_local, *col;
    const float *x, *y;
    const int32_t *ego_nodes, *ego_edges;
    const int32_t *perm;
    const uint64_t *srcs;
    const uint32_t *cursor;
    uint32_t *state;
    int32_t *ws;
    int32_t *slot_ids;
    float *labels;
    int32_t *ids;
    int64_t M, S;
    int64_t n_cap, e_cap, ego_n_cap, ego_e_cap;
    int64_t o_rowptr, o_col, o_gptr, o_dims, o_x, blob_bytes;
    int32_t B, F, T;
    int32_t D; /* molecules in the dataset, which bounds the ids in perm; 0 = M */
} scgib_collate_desc;
int64_t scgib_collate_max_batch(void);
int64_t scgib_collate_ws_words(int64_t batch);
int scgib_collate_plan(const scgib_collate_desc *d, int32_t ahead, int32_t slot, int32_t advance,
                       scgib_stream_t stream);
int scgib_collate_fill(const scgib_collate_desc *d, int32_t labels, scgib_stream_t stream);

/* Sequential batches of an index list over the same dataset, ring and
 * descriptor (collate.hip; graph.DeviceEvalLoader).  Entry
 * points only: the ABI version does not change.
 *
 * The sequence lives in device memory, so that a captured graph serves one
 * list after another: perm [M] is the index list's buffer (M its capacity, D
 * >= 1 the dataset's molecule count, S unused) and state [4] = position, sticky
 * overflow count, list length len in 1..M, fill molecule id.  One pass has
 * steps = ceil(len / B) batches; batch j holds perm[j*B .. min((j+1)*B, len))
 * followed by copies of the fill molecule, and the position is cyclic.
 *
 * scgib_collate_seq_plan: as scgib_collate_plan for batch (state[0] + ahead) mod
 *   steps, ahead in 0..2.  slot_ids gets the ids of the list's rows and -1 for
 *   fill rows; a batch that does not fit sets all B ids of its slot to -1
 *   (and bumps state[1]).  advance: state[0] = (state[0] + 1) mod steps.
 * scgib_collate_seq_fill: as scgib_collate_fill; a row whose slot id is
 *   negative gets a label row of NaN and id -1. */
int scgib_collate_seq_plan(const scgib_collate_desc *d, int32_t ahead, int32_t slot,
                           int32_t advance, scgib_stream_t stream);
int scgib_collate_seq_fill(const scgib_collate_desc *d, int32_t labels, scgib_stream_t stream);

/* Device-side COO -> CSR ingest of molecule batches (ingest.hip;
 * graph.from_coo / graph.StaticBatch.ingest).  Entry points
 * only: the ABI version does not change.
 *
 * Input: src / dst [e_raw] device edge lists of idx_bytes = 4 (int32) or 8
 * (int64) per index, graph_ptr [B+1] device int32 node offsets, n rows.
 * Output: the dst-major CSR graph.collate_pyg gives for the same molecules —
 * rowptr [n+1], col ascending within each row; the graph is symmetric, so one
 * CSR serves both directions; a self-loop is kept once.
 *   bidirect = 1: the union of the edges and their reverses, deduplicated
 *     (dgl.to_bidirected per molecule);
 *   bidirect = 0: the input must already be simple and symmetric; the CSR is
 *     built and both properties are verified, not repaired.
 * Every edge must stay inside a molecule of at most 512 atoms: row v's
 * neighbour set is a bitmap of ceil(max_graph_nodes / 32) words relative to
 * its molecule's first node (integer atomicOr: deterministic bits).
 *
 * Error bits (status[0]; OR-ed into the sticky word of the capacity form): */
#define SCGIB_INGEST_ERANGE 1     /* an index outside [0, n), or an edge leaving its graph */
#define SCGIB_INGEST_EGRAPH 2     /* a graph above 512 nodes */
#define SCGIB_INGEST_ECAPACITY 4  /* a capacity exceeded */
#define SCGIB_INGEST_ELASTNODE 8  /* skip_rule: a molecule whose last node has no edge (the
                                     reference infers fewer nodes than x has rows and skips it) */
#define SCGIB_INGEST_ESYMMETRY 16 /* bidirect = 0: not symmetric, or a duplicate edge */
#define SCGIB_INGEST_ESMALL 32    /* capacity form: a molecule with fewer than two atoms */
#define SCGIB_INGEST_EGPTR 64     /* graph_ptr is not a monotone partition of [0, n) */
/* status (int32, scgib_ingest_status_words(B) = 16 + B + 1): [0] error bits,
 * [1] n, [2] e = rowptr[n], [3] max in-degree, [4] / [5] smallest / largest
 * molecule, [6..7] / [8..9] the k = 1 ego bounds as 64-bit (low, high):
 * sum_v (1 + deg(v) - selfloop(v)) and sum_v deg(v) * (1 + deg(v) -
 * selfloop(v)), [10] 1 when the outputs were written, [16..] graph_ptr.
 * With any error bit set rowptr / col (or the blob) are not written.
 *
 * ws: scgib_ingest_workspace_bytes(rows, max_graph_nodes) bytes, zeroed once
 * by the caller; the fill launch clears what the mark launch set (on the
 * error path too), so it is reused without a memset.  Its layout follows
 * `rows`: the eager entry takes the row count it was sized for as ws_rows
 * (>= n), so one workspace serves every batch up to that size; the capacity
 * form's is sized for n_cap.
 *
 * scgib_ingest_csr (eager): col_cap >= 2 * e_raw under bidirect, else e_raw.
 * scgib_ingest_blob (capacity form, capturable): writes blob in
 *   StaticBatch's layout (scgib_collate_desc's sections) byte for byte as
 *   StaticBatch.pad uploads it — rowptr[n..n_cap] = e, col 0 past e,
 *   graph_ptr, dims = [n, e, 0 (the ego error word), 0], x rows copied, 0 past
 *   n — only if no error bit is set, n <= n_cap, e <= e_cap, the k = 1 ego
 *   bounds within ego_n_cap / ego_e_cap, the max in-degree within
 *   max_in_degree, every molecule of 2..max_graph_nodes atoms.  Otherwise the
 *   blob keeps every byte and the bits are OR-ed into *sticky.  counts
 *   (device int32 (n, e_raw), or NULL): the actual sizes, src / dst / x then
 *   being staging buffers of e_raw indices and n_cap rows; NULL: n and e_raw
 *   of the descriptor.  status may be NULL. */
typedef struct {
    const void *src, *dst;
    const int32_t *graph_ptr;
    const float *x;
    const int32_t *counts;
    void *ws;
    int32_t *status;
    int32_t *sticky;
    void *blob;
    int64_t e_raw, n;
    int64_t n_cap, e_cap, ego_n_cap, ego_e_cap;
    int64_t o_rowptr, o_col, o_gptr, o_dims, o_x, blob_bytes;
    int32_t B, F, idx_bytes, max_graph_nodes, max_in_degree, bidirect, skip_rule, pad_;
} scgib_ingest_desc;
int64_t scgib_ingest_workspace_bytes(int64_t rows, int32_t max_graph_nodes);
int64_t scgib_ingest_status_words(int64_t n_graphs);
int scgib_ingest_csr(const void *src, const void *dst, int32_t idx_bytes, int64_t e_raw,
                     const int32_t *graph_ptr, int64_t n_graphs, int64_t n_nodes,
                     int32_t max_graph_nodes, int32_t bidirect, int32_t skip_rule, void *ws,
                     int64_t ws_rows, int32_t *rowptr, int32_t *col, int64_t col_cap,
                     int32_t *status, scgib_stream_t stream);
int scgib_ingest_blob(const scgib_ingest_desc *d, scgib_stream_t stream);

/* Graph cores and significant subgraphs (explain.hip; ops.explain_rank /
 * ops.core_subgraph / explain.explain_dataset).  Entry points
 * only: the ABI version does not change.
 *
 * lam / logit [n_rows]: what scgib_interaction_fwd writes.  pad != 0 (capacity
 * mode: n_rows is the row capacity, graph_ptr[n_graphs] the actual count):
 * rows past the actual count get alpha 0, ranks -1 and mask 0.  Nothing is
 * read back and no entry uses an atomic: every launch captures and every
 * result is bitwise reproducible.
 *
 * scgib_explain_rank: one wavefront per molecule.  alpha = softmax of logit
 *   over the molecule (max, sum, normalise in fp32, fixed order); lam_rank /
 *   alpha_rank [n_rows] int32 = position of the row in its molecule by
 *   descending key, ties by ascending id, keys compared as floats, NaN after
 *   every number; centres / weights [n_graphs][top_m]: global row ids and
 *   alpha of the rows with alpha_rank < top_m in rank order, -1 / 0 past the
 *   molecule's size.  logit NULL (no attention): only lam_rank is written and
 *   top_m must be 0.  Keys of the first scgib_explain_stage_rows() rows of a
 *   molecule are staged in LDS, later rows are read from memory; the ranking
 *   counts predecessors, n_i^2 / 64 comparisons per lane and key.
 * scgib_explain_core_mask: mask [n_rows] (bytes, 0 / 1).  rule 0: lam_rank <
 *   max(1, ceil(n_i * ratio)), evaluated in IEEE double, ratio in (0, 1];
 *   rule 1: lam >= threshold (NaN never kept).
 * scgib_explain_core_count / _fill: the subgraph induced on the kept rows
 *   (dgl.node_subgraph): rows in ascending id, each row's columns in CSR order,
 *   filtered and relabelled by the batch-wide exclusive prefix of the mask;
 *   graph_ptr_out[g] = that prefix at graph_ptr[g]; out_id = the kept rows' ids.
 *   ws: scgib_explain_core_ws_words(n_rows) int32.  count leaves the core's
 *   (rows, edges) in core_dims (summed in 64 bits; a total above int32 sets
 *   bit 1 of *err and core_dims to 0).  fill writes at most n_out_cap rows and
 *   e_out_cap columns; rows past the core's get empty CSR rows and id 0.
 *   out_id / graph_ptr_out may be NULL (a second CSR of the same rows).
 *   dims (capacity mode, or NULL): dims[0] = the actual row count.
 * scgib_explain_store: one wavefront per molecule g of the batch; its rows of
 *   lam / alpha / lam_rank / alpha_rank go to node_off[ids[g]] of the ds_
 *   arrays.  ids outside [0, n_molecules) (the eval loader's fill, -1) write
 *   nothing, and no row at or past total_nodes (the ds_ arrays' length) is
 *   written.  alpha NULL: only lam and lam_rank. */
int64_t scgib_explain_stage_rows(void);
int scgib_explain_rank(const float *lam, const float *logit, const int32_t *graph_ptr,
                       int64_t n_graphs, int64_t n_rows, int32_t top_m, float *alpha,
                       int32_t *lam_rank, int32_t *alpha_rank, int32_t *centres, float *weights,
                       int32_t pad, scgib_stream_t stream);
int scgib_explain_core_mask(const float *lam, const int32_t *lam_rank, const int32_t *graph_ptr,
                            int64_t n_graphs, int64_t n_rows, int32_t rule, double ratio,
                            float threshold, uint8_t *mask, int32_t pad, scgib_stream_t stream);
int64_t scgib_explain_core_ws_words(int64_t n_rows);
int scgib_explain_core_count(const uint8_t *mask, const int32_t *rowptr, const int32_t *col,
                             int64_t n_rows, int32_t *ws, int32_t *core_dims, int32_t *err,
                             const int32_t *dims, scgib_stream_t stream);
int scgib_explain_core_fill(const uint8_t *mask, const int32_t *rowptr, const int32_t *col,
                            const int32_t *graph_ptr, int64_t n_graphs, int64_t n_rows,
                            const int32_t *ws, const int32_t *core_dims, int32_t *out_rowptr,
                            int32_t *out_col, int32_t *out_id, int32_t *graph_ptr_out,
                            int64_t n_out_cap, int64_t e_out_cap, const int32_t *dims,
                            scgib_stream_t stream);
int scgib_explain_store(const float *lam, const float *alpha, const int32_t *lam_rank,
                        const int32_t *alpha_rank, const int32_t *graph_ptr, int64_t n_graphs,
                        const int32_t *ids, const int64_t *node_off, int64_t n_molecules,
                        int64_t total_nodes, float *ds_lam, float *ds_alpha, int32_t *ds_lam_rank,
                        int32_t *ds_alpha_rank, scgib_stream_t stream);

/* Molecule-resident eval forward (infer.hip; ops.infer_forward, infer.Scorer,
 * DESIGN.md §29).  Entry points only: the ABI version does not change.
 *
 * One launch runs the whole eval-mode model (every BatchNorm on its running
 * statistics) per molecule in LDS: transfer_d, Encoder1 over the molecule,
 * Encoder2 over its ego-nets (the ego batch graph.egonet_batch built: ego-net
 * v <-> row v, rows ego_ptr[v] .. ego_ptr[v + 1] of ego_rowptr / ego_col /
 * ego_id, ego_id = the parent row of an ego row), the interaction of
 * scgib_interaction_fwd with training = 0, and with has_head the MLP
 * (128 -> 64 -> 64) and Set2Set (n_iters rounds).  The parameter table is
 * copied into the kernel arguments before the call returns.  All weights are
 * nn.Linear's / nn.LSTM's [out][in]; GIN layer 0's w1 is [64][32], transfer
 * [32][n_feat]; ope = 1 + eps of the GINConv; bn_eps serves every BatchNorm.
 *
 * x [n_rows][n_feat]; u_gate [n_rows], u_feat [n_rows][64]: the noise.
 * Outputs: z1, z2 [n_graphs][64] (sum readouts of the noisy and the plain
 * features) always; pooled [n_graphs][128] with has_head; lam, logit [n_rows]
 * and im [n_rows][128] when not NULL (logit only with use_att).  dims
 * (capacity mode, or NULL): dims[0] = the actual row count, n_rows then the
 * capacity; molecules without rows write zero rows, rows of lam / logit / im
 * past the count are zeros.  e_cap / ego_rows / ego_e_cap: the lengths of col,
 * of ego_id (ego_rowptr: ego_rows + 1) and of ego_col; no index at or past
 * them is dereferenced.  max_graph_nodes: the host's bound on a molecule's
 * rows.  Supported: 1 <= n_layers <= SCGIB_INFER_MAX_LAYERS, 1 <= n_feat <= 16,
 * max_graph_nodes <= scgib_infer_max_nodes(); anything else returns
 * SCGIB_EUNSUPPORTED without a launch.  On the device, a molecule above
 * scgib_infer_max_nodes() rows, a graph_ptr range that is no range of the
 * batch's rows, an ego-net above scgib_infer_max_ego_rows()
 * rows, or an index that leaves its molecule / ego tile sets *err to 1
 * (sticky: never cleared here) and that molecule's output rows to NaN.
 * The weight matrices (w1, w2, c0_w, mlp2_w, w_ih, w_hh) are read as 16-byte
 * vectors and must be 16-byte aligned (SCGIB_EINVAL).  No atomics, nothing
 * read back: the launch captures, is bitwise reproducible, and a molecule's
 * outputs do not depend on the batch around it.
 * scgib_infer_ego_tile_rows(): ego-nets are walked in tiles of whole ego-nets
 * of at most this many rows; scgib_infer_max_workgroups(): the grid's bound
 * (workgroup b takes molecules b, b + grid, ...). */
#define SCGIB_INFER_MAX_LAYERS 8
typedef struct {
    const float *transfer;
    /* [0]: Encoder1, [1]: Encoder2 */
    const float *w1[2][SCGIB_INFER_MAX_LAYERS], *b1[2][SCGIB_INFER_MAX_LAYERS];
    const float *w2[2][SCGIB_INFER_MAX_LAYERS], *b2[2][SCGIB_INFER_MAX_LAYERS];
    const float *gamma[2][SCGIB_INFER_MAX_LAYERS], *beta[2][SCGIB_INFER_MAX_LAYERS];
    const float *rmean[2][SCGIB_INFER_MAX_LAYERS], *rvar[2][SCGIB_INFER_MAX_LAYERS];
    float ope[2][SCGIB_INFER_MAX_LAYERS];
    const float *c0_w, *c0_b, *cbn_gamma, *cbn_beta, *cbn_rmean, *cbn_rvar, *c3_w, *c3_b;
    const float *att_w;
    const float *mlp0_w, *mlp0_b, *mlp2_w, *mlp2_b;
    const float *w_ih, *w_hh, *b_ih, *b_hh;
    float bn_eps;
    int32_t n_layers, n_feat, n_iters, use_att, has_head;
} scgib_infer_params;
int64_t scgib_infer_max_nodes(void);
int64_t scgib_infer_max_ego_rows(void);
int64_t scgib_infer_ego_tile_rows(void);
int64_t scgib_infer_max_workgroups(void);
int scgib_infer_fwd(const scgib_infer_params *p, const float *x, int64_t n_rows,
                    const int32_t *rowptr, const int32_t *col, int64_t e_cap,
                    const int32_t *graph_ptr, int64_t n_graphs, const int32_t *dims,
                    int64_t max_graph_nodes, const int32_t *ego_ptr, const int32_t *ego_rowptr,
                    const int32_t *ego_col, const int32_t *ego_id, int64_t ego_rows,
                    int64_t ego_e_cap, const float *u_gate, const float *u_feat, float *pooled,
                    float *z1, float *z2, float *lam, float *logit, float *im, int32_t *err,
                    scgib_stream_t stream);
/* out[ids[g]][0, width) = src[g][0, width) for the molecules g of a batch whose
 * id lies in [0, n_out) (infer.score_dataset / embed_dataset: the eval
 * loader's fill rows, id -1, write nothing).  A pass holds each id once: one
 * writer per element, no atomics, capturable. */
int scgib_infer_store(const float *src, int64_t n_graphs, int32_t width, const int32_t *ids,
                      int64_t n_out, float *out, scgib_stream_t stream);
#ifdef __cplusplus
}
#endif
#endif /* SCGIB_H */
