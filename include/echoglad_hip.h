/*
 * echoglad_hip.h — C ABI of the MI355X (gfx950) hierarchical-GNN hot path.
 *
 * Drop-in boundary for the EchoGLAD GNN stack.  The reference has no FFI of
 * its own (it is pure Python on top of torch_geometric); the entry points
 * below are what a ctypes binding on the reference side would call in place of
 *   - torch_geometric GCNConv.forward            (call site src/core/models.py:330-332, :431)
 *   - BatchNorm1d / Dropout / ReLU / residual     (src/core/models.py:333-335, :434-435)
 *   - node-type filter + 4 classifier MLPs + cat  (src/core/models.py:485-490)
 *   - bilinear_interpolation                      (src/core/models.py:539-553)
 *   - create_graphs / from_networkx               (src/core/datasets.py:1441-1584, :1392)
 *   - DownConv / UpConv of the UNet front-end, eval (src/core/models.py:841-876: Conv2d 3x3 + ReLU + BatchNorm2d,
 *     nn.Upsample, torch.cat, nn.AdaptiveMaxPool2d)
 *   - CNNResBlock of the CNN embedder (src/core/models.py:71-152), and of the CNN pyramid in eval mode
 *     (CNNHierarchicalPatchModel, src/core/models.py:556-636: Conv2d 3x3 128 -> 128 + BatchNorm2d + residual + AdaptiveMaxPool2d + ReLU)
 *
 * Conventions
 *   - every data pointer is a DEVICE pointer, 16-byte aligned, row-major
 *     contiguous fp32 [rows, 128] unless stated otherwise;
 *   - the caller owns every data buffer; the library allocates nothing on the
 *     hot path; opaque handles own small device tables and are freed by
 *     *_destroy;
 *   - all work is enqueued on the caller's stream (a hipStream_t passed as
 *     void*), no internal synchronisation, no host reads of device data
 *     (except in *_create, which are set-up calls);
 *   - return 0 on success, <0 on failure: EG_ERR_ARG bad argument,
 *     EG_ERR_UNSUPPORTED shape/topology outside what the kernels cover,
 *     EG_ERR_HIP a HIP runtime error; text via eg_last_error() (thread local).
 *   - functions are re-entrant and may be called from several host threads
 *     and on several streams at once, also with a SHARED graph handle: the
 *     only host state a launch touches is one atomic counter in the handle
 *     that picks the launch's own slice of the handle's tile-queue ring
 *     (64 slices; a slice is all zero whenever no launch uses it -- a DEVICE
 *     invariant: the ring is zeroed at creation and every kernel that walks a
 *     queue zeroes its slice on the way out, so a launch replayed from a HIP
 *     graph finds what an eager launch finds; no host flag is involved).  The
 *     ring is guarded: once a handle has been used on more than
 *     one stream every slice carries an event recorded behind its last
 *     launch (none before that: a single stream orders its launches), and a launch that would reuse a slice whose last
 *     user is still in flight on ANOTHER stream returns EG_ERR_UNSUPPORTED
 *     instead of sharing live counters with it (use one handle per stream, or
 *     synchronise).  Launches recorded into a HIP graph carry no event and query none: a
 *     captured launch keeps its slice for every replay, so replays of such a
 *     graph and more than 64 eager launches of the same handle on other
 *     streams must not overlap.  Connection-node handles own a scratch sized
 *     for the largest batch seen so far; a launch with more frames allocates a
 *     larger one (never inside a stream capture: EG_ERR_UNSUPPORTED there) and
 *     the smaller ones stay allocated until eg_graph_destroy, so graphs
 *     captured at a smaller batch keep replaying correctly.  Process-wide state: the
 *     thread-local error string, and an idempotent per-device "kernel
 *     attribute set" flag.
 *
 *   RUN-TIME ENVIRONMENT VARIABLES -- the complete list (8; rounds 3 - 5 had ~20, one per A/B).  Each selects a
 *   FALLBACK route that has to exist anyway (handles, shapes and module states the default route does not cover take it by
 *   themselves); the GPU suite runs under every one of them (tools/knob_matrix.sh).  Everything else that used to be tunable
 *   through the environment is a compile-time constant (-D to experiment) or a Python attribute a test can flip (nn.ROUTES).
 *     library (read once per process / handle, never on a launch path)
 *       EG_LAYER_IMPL=0|1      plain layer calls: 0 the symmetric 8-wave kernel, 1 the producer / consumer kernel (default: by handle)
 *       EG_CSR_TILES=0|1|2     CSR handles: 2 (default) clustered 64-node tiles with an LDS row stash, 1 consecutive rows, 0 row by row
 *       EG_LAYER_SPLIT=0       plain eval layer of the producer / consumer kernel: the chain of fp32 MFMAs instead of six bf16 products
 *                              of exact 3-piece splits (same accuracy; the A/B switch and the fallback of that form)
 *       EG_TRAIN_PS=0          training step on the symmetric kernel (what CSR handles take; no handed-down sums)
 *     Python host side (echoglad_amd/, read at the call)
 *       EG_SEQ_FUSED=0         torch_geometric-shaped Sequential: module by module instead of one fused launch per layer
 *       EG_SUMS_DOWN=0         every layer takes its own BatchNorm-backward sums (no eg_gcn_layer_bwd_lower hand-down)
 *       EG_POOL_PYRAMID=0      create_node_pixels: torch's adaptive_avg_pool2d per level instead of eg_avg_pool_pyramid_*
 *       EG_FUSED_CRITERIA=0    engine.compute_loss: the criteria one by one instead of eg_criteria_fwd / _bwd
 *   (bench.py's own EG_BENCH_* variables configure the benchmark, not the library.)
 */
#ifndef ECHOGLAD_HIP_H
#define ECHOGLAD_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EG_OK 0
#define EG_ERR_ARG (-1)
#define EG_ERR_UNSUPPORTED (-2)
#define EG_ERR_HIP (-3)

/* ABI version: bumped whenever an entry point changes its argument list.  eg_version() of a loaded library must equal the
 * EG_ABI_VERSION the binding was written for (echoglad_amd/_lib.py refuses to load anything else: a stale .so would accept
 * the new calls with shifted arguments).  130: eg_topo_create with the reference builder's full flag set, jk_in inside
 * eg_gcn_layer_cls_fwd, eg_graph_set_precision removed (round 3); train-forward child sums, fused heads backward, the
 * 64-slice queue ring refuses instead of corrupting (round 4).  131: eg_classifier_train_fwd_act.
 * 132: eg_classifier_bwd_sums, eg_gcn_layer_bwd_presummed.  133: eg_graph_layer_launches, eg_debug_layer_timing_*, eg_elm_reduce, eg_coord_mlp_*_rows, eg_bilinear4_*_rows (round 5).
 * 134: eg_dropout_epoch_add / _set, eg_debug_dropout_epoch (round 5: a whole train step as one HIP graph).
 * 135: eg_gcn_layer_bwd_lower, eg_bilinear4_bwd_rows_sums, eg_avg_pool_pyramid_fwd / _bwd, eg_criteria_* (round 6).
 * 136: eg_classifier_train_fwd_act(h_sparse), eg_classifier_bwd_sums(layer_residual, recompute_h).  137, 138: eg_coord_update_fwd / _bwd.  139, 140: eg_adam_step.
 * 141: eg_confusion_counts.  142: eg_bce_probs_fwd / _bwd, eg_criteria_ex_fwd / _bwd.
 * 143: eg_landmark_record_workspace_bytes, eg_landmark_record_hm, eg_landmark_record_coord.  144: eg_node_labels.
 * 145: eg_conv3x3_relu_bn_fwd, eg_adaptive_max_pool_fwd.
 * 146: eg_frontend_train_workspace_bytes, eg_conv3x3_relu_fwd, eg_bn2d_train_fwd, eg_relu_bn2d_bwd, eg_conv3x3_bwd_data,
 * eg_conv3x3_bwd_weight, eg_adaptive_max_pool_idx_fwd, eg_adaptive_max_pool_bwd.  147: eg_frame_prep.
 * 148: eg_gcn_layer_cls_fold_fwd.
 * 149: eg_embed_workspace_bytes, eg_embed_block_fwd, eg_embed_conv_fwd, eg_embed_act_fwd, eg_embed_act_bwd, eg_embed_res_bwd_input.
 * 150: eg_pyramid_block_fwd, eg_pyramid_block_scratch_bytes.
 * 151: eg_pyramid_train_workspace_bytes, eg_pyramid_conv_fwd, eg_pyramid_act_fwd, eg_pyramid_act_bwd, eg_pyramid_conv_bwd_data,
 * eg_pyramid_conv_bwd_weight.  152: eg_gcn_layer_cls_fold_split_fwd.
 * 153: eg_conv1x1_relu_pack_bwd_workspace_bytes, eg_conv1x1_relu_pack_bwd_plan, eg_conv1x1_relu_pack_bwd.
 * 154: eg_conv1x1_relu_heads_fwd.
 * 155: eg_sgd_step, eg_rmsprop_step.
 * 156: eg_heatmap_render.
 * 157: eg_conn_rows_plan, eg_conn_rows_workspace_bytes, eg_conn_rows_fwd, eg_conn_rows_bwd. */
#define EG_ABI_VERSION 157

#define EG_CHANNELS 128 /* node_embedding_dim == node_hidden_dim (configs/default.yml:13-14) */

typedef void* eg_stream_t; /* hipStream_t */

/* Graph handle: either the implicit (closed-form) hierarchical topology or a
 * generic CSR built from an edge_index.  Both feed the same layer kernels. */
typedef struct eg_graph eg_graph;

int eg_version(void);
const char* eg_last_error(void);

/* ---- graph handles -------------------------------------------------------
 * Closed form of DummyDataset.create_graphs (src/core/datasets.py:1441-1584):
 * aux levels 2^k x 2^k (k = 1..naux), main grid frame x frame, 4-neighbour
 * edges, parent<->child edges, centre-crop link with Python slice semantics,
 * optional isolated K4 of coordinate nodes.  The signature is SURVEY 8(b)'s: every flag of the reference's builder is an
 * argument, and every flag has implicit-stencil tables (round 4):
 *   diag_main / diag_aux ('grid-diagonal', datasets.py:1469-1475, :1494-1500): 8-neighbour levels; the stencil of such a handle
 *     lives in the fused (producer/consumer) layer kernel, every other path reads the CSR of one frame the handle carries;
 *   conn_nodes (datasets.py:1450-1456, :1512-1515): naux + 1 connection nodes at the head of every frame; a pre-pass in front of
 *     each layer launch sums every wired level once (handle-owned scratch, one slice per slot of the queue ring, grown on demand --
 *     the one allocation a launch may make, once per new maximum batch, never inside a stream capture).
 * Arbitrary graphs: eg_csr_create. */
int eg_topo_create(int frame, int naux, int main_only, int coord_nodes, int conn_nodes, int diag_main, int diag_aux,
                   eg_graph** out);

/* Generic CSR (by target node) from a device edge_index [2, n_edges] int64 in
 * PyG layout (row 0 = source, row 1 = target).  Deterministic: neighbours keep
 * their edge_index order.  Self loops in the input are dropped and one self
 * loop per node is implied (gcn_norm / add_remaining_self_loops).  DUPLICATE
 * edges are kept and count every time, in the degree and in the sum, exactly
 * as gcn_norm's scatter_add over edge_index does (a multigraph is not
 * coalesced).  Edges with an endpoint outside [0, n_nodes) are dropped.
 * Set-up call: allocates and synchronises the stream. */
int eg_csr_create(const int64_t* edge_index_dev, int64_t n_nodes, int64_t n_edges, eg_stream_t stream,
                  eg_graph** out);

/* A_hat of a DIRECTED edge_index is not symmetric, and the backward of a layer aggregates with A_hat^T
 * (dX = (A_hat^T dY) W, dW = (A_hat^T dY)^T X).  eg_graph_is_symmetric: 1 for topology handles and for CSR handles whose
 * kept edge multiset equals its own transpose (use the handle itself in the backward), else 0: build the transposed
 * handle once from the SAME edge_index (rows = sources, normalisation (deg+1)^-1/2 taken from `base`). */
int eg_graph_is_symmetric(const eg_graph* g);
int eg_csr_create_transposed(const eg_graph* base, const int64_t* edge_index_dev, int64_t n_edges, eg_stream_t stream,
                             eg_graph** out);

int eg_graph_destroy(eg_graph* g);
int64_t eg_graph_num_nodes(const eg_graph* g);      /* nodes per frame (topo) or total (csr) */
int eg_graph_is_structured(const eg_graph* g);
int64_t eg_graph_num_tiles(const eg_graph* g);      /* 64-row work tiles per frame (8x8 patches for a topo handle) */
/* copies the (deg+1)^-1/2 table [num_nodes] to a device buffer (tests / diagnostics) */
int eg_graph_deg_inv_sqrt(const eg_graph* g, float* out_dev, eg_stream_t stream);

/* Diagnostic (stamp builds only, -DEG_STAMP): per-phase cycle sums of the layer kernel accumulated in
 * the handle since the last reset: out_host[0..7] = phase sums over all waves, out_host[8] = waves,
 * out_host[9] / out_host[10] = shader cycles / 100-MHz ticks around the tile loops (their ratio x 100 MHz = the clock the
 * chip held inside the kernel).  out_host must hold 11 values.  Synchronises the device. */
int eg_debug_phase_cycles(eg_graph* g, uint64_t* out_host, int reset);

/* Diagnostic: out_dev[b] = XCC (XCD) id workgroup b ran on, out_dev[nblocks + b] = its start time stamp. */
int eg_debug_xcc(int* out_dev, int nblocks, eg_stream_t stream);

/* Measurement (bench.py's roofline): HIP events around the next launches of the fused layer kernels -- of every handle, on
 * whatever stream they are launched (not inside a stream capture) -- so that a kernel's duration is taken INSIDE a real step
 * (a training step issues its layer launches from inside autograd nodes; timing the same kernel alone on fresh rows measured
 * 8 - 13 % more than a kernel trace of the step shows).  eg_debug_layer_timing_begin(max) arms it for at most `max` launches
 * (<= 256; process-wide, not thread-safe: a measurement tool); eg_debug_layer_timing_end synchronises the recorded events and
 * returns how many launches were timed, their milliseconds in ms[] and their kind in kinds[] (EG_LAUNCH_*), both of capacity cap. */
#define EG_LAUNCH_SYMMETRIC 0   /* k_gcn_layer (CSR graphs, plain calls on hierarchical handles) */
#define EG_LAUNCH_PS_PLAIN 1    /* k_gcn_layer_ps, inference forms (plain / chained / running maximum) */
#define EG_LAUNCH_PS_TRAIN_FWD 2
#define EG_LAUNCH_PS_DX 3       /* residual as a tensor of its own: the backward's dX launch */
#define EG_LAUNCH_PS_CLS 4      /* last layer + classifier heads */
int eg_debug_layer_timing_begin(int max_launches);
int eg_debug_layer_timing_end(float* ms, int* kinds, int cap);

/* Order-independent digest of an edge_index [2, n_edges] int64 on the device:
 * out_dev[0] = n_edges, out_dev[1] = sum over edges of mix64(src, dst) (mod 2^64).
 * Used to verify an incoming PyG edge_index against the closed form once. */
int eg_edge_hash(const int64_t* edge_index_dev, int64_t n_edges, uint64_t* out_dev, eg_stream_t stream);

/* ---- fused GCN layer, inference form -------------------------------------
 * out[i,:] = act( (sum_{j in N(i) u {i}} d_i^-1/2 d_j^-1/2 x[j,:]) W^T * scale + shift ) + residual[i,:]
 * i.e. GCNConv -> (bias, eval-mode BatchNorm folded into scale/shift) -> ReLU|Identity -> +residual
 * in one kernel (src/core/models.py:328-335, :431-435).  rows = batch * num_nodes.
 *   W        [128,128] row-major [out,in] (GCNConv.lin.weight)
 *   scale    [128] or NULL (=1), shift [128] or NULL (=0)
 *   residual [rows,128] or NULL; may alias x; must not alias out
 *   relu     0|1
 *   transpose_w  0: x W^T ; 1: x W  (the backward dX form) */
int eg_gcn_layer_fwd(const eg_graph* g, int batch, const float* x, const float* W, const float* scale,
                     const float* shift, const float* residual, int relu, int transpose_w, float* out,
                     eg_stream_t stream);

/* Chained form of eg_gcn_layer_fwd for a stack of layers on one topology handle (models.py:431-435 loops over
 * gnn_layers).  A node's children contribute sum_c d_c^-1/2 x[c,:] to its aggregate; the layer that PRODUCES x can
 * leave that sum behind for every node with children, so the layer that consumes x reads one row per aux node
 * instead of four child rows:
 *   kidsum_out [batch * eg_graph_kidsum_rows(g), 128] or NULL: child sums of `out`, for the next layer.
 *              Zero-fill the buffer ONCE before its first use (rows of childless nodes are never written).
 *   kidsum_in  same shape or NULL: child sums of `x`, written by the launch that produced x.
 * Both NULL = eg_gcn_layer_fwd.  Needs eg_graph_kidsum_rows(g) > 0 and residual in {NULL, x}
 * (EG_ERR_UNSUPPORTED otherwise). */
int64_t eg_graph_kidsum_rows(const eg_graph* g);    /* rows per frame of a child-sum buffer; 0: not available */
/* 1 when eg_gcn_layer_cls_fwd (below) covers this handle: a topology handle without coordinate / connection rows
 * whose layer kernel is the producer/consumer form (child sums available, or a single-level grid); else 0. */
int eg_graph_fused_classifier_ok(const eg_graph* g);
int eg_gcn_layer_fwd_chain(const eg_graph* g, int batch, const float* x, const float* W, const float* scale,
                           const float* shift, const float* residual, int relu, int transpose_w, float* out,
                           const float* kidsum_in, float* kidsum_out, eg_stream_t stream);

/* Last layer of a stack + node-type filter + the 4 classifier heads in ONE kernel (models.py:431-435 last iteration,
 * :485-490): the layer's output tile never leaves the chip, logits [batch * n_valid, 4] are the only output, n_valid = the
 * handle's nodes per frame minus its connection nodes (the filter drops them: the first naux + 1 rows of a frame; a handle
 * without connection nodes has n_valid = eg_graph_num_nodes).
 * Layer arguments as eg_gcn_layer_fwd (W^T form), kidsum_in as eg_gcn_layer_fwd_chain (or NULL), jk_in: NULL or the running
 * JumpingKnowledge maximum (below); classifier arguments as eg_classifier_fwd.  Needs a topology handle with
 * eg_graph_kidsum_rows(g) > 0 and no coordinate nodes (eg_graph_fused_classifier_ok) and residual in {NULL, x};
 * EG_ERR_UNSUPPORTED otherwise (run eg_gcn_layer_fwd + eg_classifier_fwd instead). */
int eg_gcn_layer_cls_fwd(const eg_graph* g, int batch, const float* x, const float* W, const float* scale,
                         const float* shift, const float* residual, int relu, const float* kidsum_in, const float* jk_in,
                         const float* w1, const float* s1, const float* t1, const float* w2, const float* s2, const float* t2,
                         const float* w3, const float* b3, int sigmoid, float* logits, eg_stream_t stream);
/* The same launch for a last layer WITHOUT ReLU (the model's: models.py:431-435 builds it with nn.Identity) and without the
 * running maximum, from parameters folded once per parameter version: the heads' first pre-activation is linear in the
 * aggregated rows and the layer's input,
 *     u = (A_hat x) m1^T + residual * x w1s^T + c1,
 *     m1 = diag(s1) w1 diag(scale) W [128,128],  w1s = diag(s1) w1 [128,128],  c1 = s1 * (w1 shift) + t1 [128]
 * (W, scale, shift, w1, s1, t1 as eg_gcn_layer_cls_fwd takes them; echoglad_amd/nn/_heads.py fold_last_into_heads computes the
 * three in float64).  The layer's output is never formed; logits agree with eg_gcn_layer_cls_fwd to rounding.  residual: 0 or
 * 1 (the residual is x).  Handles, kidsum_in, w2 .. b3, sigmoid, logits and EG_ERR_UNSUPPORTED as eg_gcn_layer_cls_fwd. */
int eg_gcn_layer_cls_fold_fwd(const eg_graph* g, int batch, const float* x, int residual, const float* kidsum_in, const float* m1,
                              const float* w1s, const float* c1, const float* w2, const float* s2, const float* t2, const float* w3,
                              const float* b3, int sigmoid, float* logits, eg_stream_t stream);
/* eg_gcn_layer_cls_fold_fwd with the two products on the bf16 matrix path (exact 3-piece splits of both operands, six piece
 * products, fp32-accurate: as the plain layer's split chain).  lo_planes: the lowest bf16 piece of every element of m1 and w1s,
 * 64 KB, 16-byte aligned, in the order the kernel's lanes fetch it -- [matrix 2][k-step 4][wave 4][column block 2][kq 4][i 16][e 8]
 * = lo(Wm[32 wave + 16 cb + i][koff(kq) + 8 step + e]), koff = {0, 64, 32, 96} (echoglad_amd/ops/infer.py fold_lo_table builds
 * it; with residual = 0 the second matrix' half is not read).  A handle created under EG_LAYER_SPLIT=0 runs the fp32 body of
 * eg_gcn_layer_cls_fold_fwd instead.  Everything else as there. */
int eg_gcn_layer_cls_fold_split_fwd(const eg_graph* g, int batch, const float* x, int residual, const float* kidsum_in, const float* m1,
                                    const float* w1s, const float* c1, const void* lo_planes, const float* w2, const float* s2,
                                    const float* t2, const float* w3, const float* b3, int sigmoid, float* logits, eg_stream_t stream);

/* JumpingKnowledge('max') of the reference (torch_geometric JumpingKnowledge as used at src/core/models.py:380-382,
 * :479-482: element-wise maximum over [node features, h_1, .., h_L]) carried through the fused stack as a running maximum:
 * eg_gcn_layer_fwd_jk is eg_gcn_layer_fwd_chain that also writes jk_out = max(jk_in, out) (the first layer passes its
 * input x as jk_in; kidsum_in / kidsum_out may be NULL); eg_gcn_layer_cls_fwd with jk_in != NULL runs the heads on
 * max(jk_in, layer output).  EG_ERR_UNSUPPORTED where the producer/consumer kernel does not cover the handle.
 * eg_graph_ps_launches: launches of that kernel on the handle so far (tests assert that a model stayed on the fused path). */
int eg_gcn_layer_fwd_jk(const eg_graph* g, int batch, const float* x, const float* W, const float* scale, const float* shift,
                        const float* residual, int relu, float* out, const float* kidsum_in, float* kidsum_out,
                        const float* jk_in, float* jk_out, eg_stream_t stream);
unsigned eg_graph_ps_launches(const eg_graph* g);
/* launches of ANY fused layer kernel (producer/consumer or symmetric; forward, train forward, dX) on the handle so far: tests
 * assert "one launch per layer" for callers that reach the kernels through the torch_geometric-shaped modules
 * (Sequential('x, edge_index', [GCNConv, BatchNorm1d, Dropout, ReLU]) of src/core/models.py:329-335). */
unsigned eg_graph_layer_launches(const eg_graph* g);

/* out = A_hat x  (aggregation only; training / backward building block) */
int eg_gcn_aggregate(const eg_graph* g, int batch, const float* x, float* out, eg_stream_t stream);

/* out = act((x W^T) * scale + shift) + residual   for rows x 128 (no graph) */
int eg_linear128_fwd(const float* x, int64_t rows, const float* W, const float* scale, const float* shift,
                     const float* residual, int relu, int transpose_w, float* out, eg_stream_t stream);

/* ---- node-type filter + 4 classifier heads, inference form ----------------
 * For every frame f and every valid row r in [row_lo, row_lo + n_valid):
 *   logits[f*n_valid + r - row_lo, c] = head_c(h[f*n_per_frame + r, :])
 * head_c = Linear(128,32)-BN-ReLU-Linear(32,16)-BN-ReLU-Linear(16,1) [-Sigmoid]
 * (src/core/models.py:363-377, :485-490) with eval-mode BN folded by the caller:
 *   w1 [128,128] = 4 heads' [32,128] stacked, s1/t1 [128]
 *   w2 [4,16,32], s2/t2 [64];  w3 [4,16], b3 [4]
 * logits [batch*n_valid, 4]. */
int eg_classifier_fwd(const float* h, int batch, int64_t n_per_frame, int64_t row_lo, int64_t n_valid,
                      const float* w1, const float* s1, const float* t1, const float* w2, const float* s2,
                      const float* t2, const float* w3, const float* b3, int sigmoid, float* logits,
                      eg_stream_t stream);

/* ---- training-mode pieces (BatchNorm batch statistics, Dropout, backward) -----------------------
 * Reference: the same Sequential (src/core/models.py:328-335) in train mode and its autograd backward
 * (engine.py:271-273).  Every reduction is two-stage through a caller-provided workspace of at least
 * eg_workspace_bytes() bytes (device memory, reusable across calls on one stream): no float atomics,
 * results are bitwise reproducible. */
size_t eg_workspace_bytes(void);

/* out[128] = sum over rows of x[rows,128]                     (GCNConv.bias gradient) */
int eg_colsum128(const float* x, int64_t rows, void* workspace, float* out, eg_stream_t stream);

/* dw[o][i] = sum_r g[r][o] * x[r][i], [128,128] row-major     (GCNConv.lin.weight gradient, g = A_hat dy) */
int eg_dweight128(const float* g, const float* x, int64_t rows, void* workspace, float* dw, eg_stream_t stream);

/* BatchNorm1d(128) batch statistics over ALL rows: mean[128], biased variance var[128] (models.py:333) */
int eg_bn_stats(const float* x, int64_t rows, void* workspace, float* mean, float* var, eg_stream_t stream);

/* Dropout epoch.  Every Dropout site below takes its seed as an ARGUMENT (the mask is a pure function of (seed, element index), so
 * forward and backward kernels regenerate it and nothing is stored).  A train step captured into a HIP graph freezes its kernel
 * arguments; what the kernels hash with is therefore  seed + EPOCH, EPOCH = one 64-bit word per device in device memory, read
 * at the top of every kernel that applies or regenerates a mask, 0 until one of these calls moves it.  eg_dropout_epoch_add is a
 * one-thread kernel on `stream` (capturable: a graph that starts with it draws fresh masks at every replay; the forward and
 * backward kernels of one step see the same value because they are ordered behind it); eg_dropout_epoch_set the same with an
 * absolute value (an eager step under epoch k reproduces replay k of a graph captured under epoch 0 with the same seeds).
 * The word is allocated at the first train-mode launch (or the first of these calls) on a device -- never inside a capture.
 * eg_debug_dropout_epoch synchronises the device and reads the word (tests). */
int eg_dropout_epoch_add(uint64_t delta, eg_stream_t stream);
int eg_dropout_epoch_set(uint64_t value, eg_stream_t stream);
int eg_debug_dropout_epoch(uint64_t* out_host);

/* out = relu?(dropout_p(z * scale + shift)) + residual ; dropout keeps element e iff hash(seed, e) >= p and
 * scales by 1/(1-p) (nn.Dropout semantics; the mask is a pure function of (seed, element index)).
 * residual may be NULL. */
int eg_bn_act_fwd(const float* z, int64_t rows, const float* scale, const float* shift, const float* residual,
                  int relu, float dropout_p, uint64_t seed, float* out, eg_stream_t stream);

/* The same pass walked in the layer kernels' tile order over a topology handle (rows = batch * eg_graph_num_nodes(g)), which lets
 * it leave the child sums of `out` behind: kidsum_out (nullable) [batch * eg_graph_kidsum_rows(g), 128], row p of a frame =
 * sum over the 4 children c of aux node p of (deg_c + 1)^-1/2 out[c] -- what eg_gcn_layer_train_fwd / eg_gcn_layer_fwd_chain take
 * as kidsum_in.  Same values as eg_bn_act_fwd (same expression per element, same dropout mask). */
int eg_bn_act_fwd_tiles(const eg_graph* g, int batch, const float* z, const float* scale, const float* shift,
                        const float* residual, int relu, float dropout_p, uint64_t seed, float* out, float* kidsum_out,
                        eg_stream_t stream);

/* backward of  y = relu?(dropout(BN_train(z)))  given dy: dz[rows,128], dgamma[128], dbeta[128].
 * mean / invstd are the batch statistics used in the forward (invstd = 1/sqrt(var + eps)). */
int eg_bn_act_bwd(const float* dy, const float* z, int64_t rows, const float* mean, const float* invstd,
                  const float* gamma, const float* beta, int relu, float dropout_p, uint64_t seed, void* workspace,
                  float* dz, float* dgamma, float* dbeta, eg_stream_t stream);

/* ---- one whole train-mode GNN layer (src/core/models.py:328-335, :431-435 in train mode; backward of engine.py:271-273) ----
 * eg_gcn_layer_train_fwd:
 *     z   = A_hat x W^T + bias                       kept for the backward          [rows,128]
 *     agg = A_hat x                                   kept for the weight gradient   [rows,128] (NULL: not kept)
 *     bn  = { batch mean, 1/sqrt(var + eps), gamma * invstd, beta - mean * scale }   [4,128]
 *     running_mean / running_var <- nn.BatchNorm1d update with `momentum` (unbiased variance); momentum < 0 or NULL: none
 *     out = relu?(dropout(z * scale + shift)) + (residual ? x : 0)    dropout mask = pure function of (seed, element)
 *           (out NULL: z, agg, bn and the running statistics only -- the activation pass is not run)
 *     kidsum_in / kidsum_out (both nullable; [batch * eg_graph_kidsum_rows(g), 128], see eg_gcn_layer_fwd_chain): chained train
 *     forward.  kidsum_out receives the child sums of `out` (written by the activation pass, which then runs in tile order);
 *     kidsum_in = the child sums of x left by the layer that produced x: aux nodes read one row instead of four child rows.
 *     (The coordinate-graph update that the reference runs between two layers rewrites only coordinate rows, which are nobody's
 *     children: the sums stay valid.)
 * eg_gcn_layer_bwd, given dy = d loss / d out and the tensors kept by the forward:
 *     dz (scratch [rows,128]; may be NULL when dx is NULL and dw is not: the first layer of a stack whose input needs no
 *         gradient never writes it) = BatchNorm'(dy * dropout / ReLU mask);  dgamma, dbeta [128]
 *     dx [rows,128] (NULL: skipped) = (A_hat^T dz) W + (residual ? dy : 0)      g_bwd: eg_graph_is_symmetric ? g : transposed handle
 *     dw [128,128]  (NULL: skipped) = dz^T agg                                   (== (A_hat^T dz)^T x)
 *     db [128]      (NULL: skipped) = 0: a bias in front of a train-mode BatchNorm has an identically zero gradient
 * workspace: eg_workspace_bytes() bytes of device memory, reusable across calls on one stream. */
int eg_gcn_layer_train_fwd(const eg_graph* g, int batch, const float* x, const float* W, const float* bias, const float* gamma,
                           const float* beta, float* running_mean, float* running_var, float momentum, float eps, int relu,
                           float dropout_p, uint64_t seed, int residual, void* workspace, float* z, float* agg, float* bn,
                           float* out, const float* kidsum_in, float* kidsum_out, eg_stream_t stream);
int eg_gcn_layer_bwd(const eg_graph* g_bwd, int batch, const float* dy, const float* z, const float* agg, const float* W,
                     const float* gamma, const float* beta, const float* bn, int relu, float dropout_p, uint64_t seed,
                     int residual, void* workspace, float* dz_scratch, float* dx, float* dw, float* db, float* dgamma,
                     float* dbeta, eg_stream_t stream);

/* ---- node-type filter + the 4 classifier heads, train mode (src/core/models.py:363-377, :485-490; batch statistics in both
 * BatchNorm layers of every head).  The four heads run as one stacked network; parameters are passed stacked:
 *   w1 [128,128] = 4 x [32,128], b1 / gamma1 / beta1 [128];  w2 [4,16,32], b2 / gamma2 / beta2 [64];  w3 [4,16], b3 [4]
 *   running_mean1 / running_var1 [128], running_mean2 / running_var2 [64]: updated in place (NULL or momentum < 0: not)
 *   p1 / p2, seed1 / seed2: the two Dropout layers (mask = pure function of (seed, element))
 * eg_classifier_train_fwd keeps z1 [batch*n_valid,128], z2 [batch*n_valid,64] and bn [4*128 + 4*64] = per layer {mean, invstd,
 * scale, shift}, and writes logits [batch*n_valid, 4].
 * eg_classifier_bwd, given dlogits [batch*n_valid,4]:
 *   dh [batch*n_per_frame,128] (NULL: skipped): gradient w.r.t. h; the rows the filter drops are written as zeros
 *   grads [19076] = dw1 [128*128], db1 [128] (= 0), dgamma1 [128], dbeta1 [128], dw2 [4*16*32], db2 [64] (= 0), dgamma2 [64],
 *                   dbeta2 [64], dw3 [64], db3 [4]
 *   dh1_scratch: [batch*n_valid,128] (the gradient of the first hidden layer on its way from the second layers' kernel to the
 *   first layers' one; dz1 = BatchNorm'(dh1 * mask) is formed on load there and never written).
 * workspace: eg_classifier_train_workspace_bytes() bytes. */
typedef struct eg_cls_train_params {
    const float *w1, *b1, *gamma1, *beta1;
    const float *w2, *b2, *gamma2, *beta2;
    const float *w3, *b3;
    float *running_mean1, *running_var1, *running_mean2, *running_var2;
    float eps1, eps2, momentum1, momentum2;
    float p1, p2;
    uint64_t seed1, seed2;
} eg_cls_train_params;
#define EG_CLS_GRADS_FLOATS 19076
size_t eg_classifier_train_workspace_bytes(void);
int eg_classifier_train_fwd(const float* h, int batch, int64_t n_per_frame, int64_t row_lo, int64_t n_valid,
                            const eg_cls_train_params* params, void* workspace, float* z1, float* z2, float* bn, int sigmoid,
                            float* logits, eg_stream_t stream);
/* The same with the activation pass of the LAST GNN layer folded into the first heads' kernel: the rows of h do not exist yet,
 *   h = relu|id(dropout(z * scale + shift)) + residual          (scale / shift = layer_bn + 256 / + 384, the bn array
 *                                                                 eg_gcn_layer_train_fwd(..., out = NULL, ...) left)
 * is computed tile by tile on the way into the heads' first product and written to h [batch*n_per_frame,128] (every row, also
 * the ones the filter drops).  One read of h less than eg_gcn_layer_train_fwd(out = h) + eg_classifier_train_fwd(h).
 * residual: NULL or the layer's input rows; (relu, dropout_p, seed) as given to the layer.  h must not alias z / residual. */
int eg_classifier_train_fwd_act(const float* z, const float* layer_bn, const float* residual, int relu, float dropout_p, uint64_t seed,
                                float* h, int batch, int64_t n_per_frame, int64_t row_lo, int64_t n_valid,
                                const eg_cls_train_params* params, void* workspace, float* z1, float* z2, float* bn, int sigmoid,
                                float* logits, int h_sparse, eg_stream_t stream);
/* h_sparse != 0: only the rows of h OUTSIDE [row_lo, row_lo + n_valid) of every frame are written (the coordinate rows the landmark
 * MLP reads; with no such rows nothing is); the heads' backward then takes recompute_h (eg_classifier_bwd_sums). */
int eg_classifier_bwd(const float* dlogits, const float* h, int batch, int64_t n_per_frame, int64_t row_lo, int64_t n_valid,
                      const eg_cls_train_params* params, const float* z1, const float* z2, const float* bn, void* workspace,
                      float* dh1_scratch, float* dh, float* grads, eg_stream_t stream);

/* The heads' backward that also takes the BatchNorm-backward sums of the GNN layer in front of the heads, where dh passes through
 * registers on its way out: layer_sums [2][128] (double) = sum g, sum g * xhat over rows [row_lo, row_lo + n_valid) of every frame,
 * g = dh * that layer's dropout / ReLU mask (layer_z, layer_bn = what eg_gcn_layer_train_fwd kept; layer_gamma / layer_beta its
 * BatchNorm parameters; layer_relu, layer_dropout_p, layer_seed as given to it).  eg_gcn_layer_bwd_presummed then runs that
 * layer's backward without its own sums pass over dy and z (2.4 GB of reads at batch 32): it only adds the rows the range
 * leaves out (frames * (rows per frame - n_valid) of them; dy may have been changed there in between -- the coordinate update's
 * backward does).  EG_ERR_UNSUPPORTED when the fused first-layers kernel does not cover the shape (dh NULL, n_valid < 64, 2^32
 * elements and more): nothing was launched, call eg_classifier_bwd + eg_gcn_layer_bwd. */
int eg_classifier_bwd_sums(const float* dlogits, const float* h, int batch, int64_t n_per_frame, int64_t row_lo, int64_t n_valid,
                           const eg_cls_train_params* params, const float* z1, const float* z2, const float* bn, void* workspace,
                           float* dh1_scratch, float* dh, float* grads, const float* layer_z, const float* layer_bn,
                           const float* layer_gamma, const float* layer_beta, int layer_relu, float layer_dropout_p,
                           uint64_t layer_seed, double* layer_sums, const float* layer_residual, int recompute_h, eg_stream_t stream);
/* recompute_h != 0 (round 6): the layer's output h = act(z) + residual was never written in full (eg_classifier_train_fwd_act with
 * h_sparse: only the rows the heads' filter drops reach memory) -- `h` is ignored (may be NULL) and the first-layers kernel rebuilds
 * its h tile from layer_z (which it reads for the sums anyway) and layer_residual (the layer's input rows; NULL: no residual)
 * with the forward's own expression and dropout mask: 1.18 GB less written per step at batch 32.  Arrays below 2 GB.
 * At 2 GiB per array and more (batch 59+ at 224 / 7) recompute_h returns EG_ERR_UNSUPPORTED before anything is launched and this entry
 * point, like eg_classifier_bwd, runs the flat-address form of its first-layers kernel; tested up to arrays below 4 GiB
 * (tests/test_gpu_big_arrays.py: batch 59 / 60), not at 2^31 elements and more. */
int eg_gcn_layer_bwd_presummed(const eg_graph* g_bwd, int batch, const float* dy, const float* z, const float* agg, const float* W,
                               const float* gamma, const float* beta, const float* bn, int relu, float dropout_p, uint64_t seed,
                               int residual, void* workspace, float* dz_scratch, float* dx, float* dw, float* db, float* dgamma,
                               float* dbeta, const double* dy_sums, int frames, int64_t row_lo, int64_t n_valid, eg_stream_t stream);

/* ---- the BatchNorm-backward sums of the layer BELOW, taken by the dX launch that writes its dy (round 6) ----------------------
 * dx of layer i + 1 IS dy of layer i, so layer i's sums  sum g, sum g * xhat  (g = dy * dropout keep * ReLU gate of layer i's
 * activation, src/core/models.py:333-335 backwards) can be taken where the finished dx rows leave the layer kernel instead of by a
 * pass of their own over dy and z (0.40 ms and 2.4 GB per layer at batch 32).  eg_gcn_layer_bwd_lower is eg_gcn_layer_bwd /
 * eg_gcn_layer_bwd_presummed (given != NULL) with that by-product:
 *   lower->z, lower->bn            layer i's pre-BatchNorm rows and {mean, invstd, scale, shift} (eg_gcn_layer_train_fwd)
 *   lower->relu, dropout_p, seed   its activation, as given to eg_gcn_layer_train_fwd
 *   lower->row_hi                  rows [0, row_hi) of every frame are summed (the coordinate nodes behind them are rewritten by the
 *                                  coordinate update's backward afterwards; the consumer of the sums adds them: given->row_lo = 0,
 *                                  given->n_valid = row_hi)
 *   lower->tile_scratch            eg_graph_num_tiles(g_bwd) * batch * 256 floats: one partial per tile (tiles are summed in
 *                                  index order afterwards: bit-reproducible under the dynamic tile queues)
 *   lower->sums_out                [2][128] doubles, the `sums` of a later eg_gcn_layer_bwd_lower(given) / _presummed call
 * given->taps (nullable): [given->frames][2][128] floats from eg_bilinear4_bwd_rows_sums -- what the bilinear backward added to
 * rows inside the summed range AFTER the sums were taken (the sums are linear in dy: the additions' own sums are simply added).
 * EG_ERR_UNSUPPORTED (nothing launched) when the dX launch is not the producer / consumer kernel's (CSR handles, dx NULL,
 * residual 0): call eg_gcn_layer_bwd and let the lower layer take its own sums. */
typedef struct eg_lower_sums {
    const float* z;
    const float* bn;
    int relu;
    float dropout_p;
    uint64_t seed;
    int64_t row_hi;
    float* tile_scratch;
    double* sums_out;
} eg_lower_sums;
typedef struct eg_given_sums {
    const double* sums;
    int frames;
    int64_t row_lo, n_valid;
    const float* taps;
} eg_given_sums;
int eg_gcn_layer_bwd_lower(const eg_graph* g_bwd, int batch, const float* dy, const float* z, const float* agg, const float* W,
                           const float* gamma, const float* beta, const float* bn, int relu, float dropout_p, uint64_t seed,
                           int residual, void* workspace, float* dz_scratch, float* dx, float* dw, float* db, float* dgamma,
                           float* dbeta, const eg_given_sums* given, const eg_lower_sums* lower, eg_stream_t stream);

/* ---- coordinate-graph landmark update (src/core/models.py:438-453) -----------------------------------
 * For the 4 landmark rows of every frame (R = 4 * batch rows):
 *   shape_feats[(f,j), 2k+d] = coords[f,k,d] - coords[f,j,d]                                   (models.py:441-444)
 *   delta = node_coordinate_mlp[i](cat(lm, shape_feats))   Linear(136,32)-BN-ReLU-Drop-Linear(32,16)-BN-ReLU-Drop-Linear(16,2)
 *   new_coords = clamp(coords + delta, 0, frame - 1)                                            (models.py:449-453)
 * in one single-workgroup launch.  params: the eg_cls_train_params struct with w1 [32,136], w2 [16,32], w3 [2,16] and
 * 32 / 16-long BatchNorm vectors.  train != 0: batch statistics, running-stat update (momentum < 0 or NULL: none) and
 * Dropout(p1, p2) with the counter-based masks (seed1, seed2); train == 0: running statistics, no dropout.
 *   lm [R,128], coords [R,2] (h, w);  saved for the backward: z1 [R,32], z2 [R,16], bn [96] = mean1, invstd1 [32 each],
 *   mean2, invstd2 [16 each], pre [R,2] = coords + delta before the clamp (nullable when no backward follows).
 * eg_coord_mlp_bwd (train-mode statistics only): d new_coords -> dlm [R,128] (nullable), dcoords [R,2] (nullable) and
 *   grads [EG_COORD_MLP_GRADS_FLOATS] = dw1 [32*136], db1 [32] (= 0), dgamma1, dbeta1 [32 each], dw2 [16*32], db2 [16] (= 0),
 *   dgamma2, dbeta2 [16 each], dw3 [2*16], db3 [2];   scratch: [R,56] floats. */
#define EG_COORD_MLP_GRADS_FLOATS 5042
int eg_coord_mlp_fwd(const float* lm, const float* coords, int batch, const eg_cls_train_params* params, int train, int frame,
                     float* z1, float* z2, float* bn, float* pre, float* new_coords, eg_stream_t stream);
int eg_coord_mlp_bwd(const float* dnew_coords, const float* lm, const float* coords, int batch,
                     const eg_cls_train_params* params, int frame, const float* z1, const float* z2, const float* bn,
                     const float* pre, float* scratch, float* dlm, float* dcoords, float* grads, eg_stream_t stream);
/* The same two with the landmark rows where they LIVE -- the 4 coordinate rows of every frame inside the [B*N,128] node array
 * (models.py:447: h[node_type == 1]) -- instead of a gathered copy: frame f's rows start at lm + f * lm_frame_stride (floats;
 * 4 * 128 = a packed array).  lm_copy (nullable): packed [R,128] copy of the rows as the MLP read them, for the backward (the
 * coordinate update overwrites the rows afterwards, :473).  Backward: dlm is written (dlm_accumulate: added) with the same
 * frame stride, i.e. straight into the coordinate rows of the gradient array.  No gather / scatter launches around the MLP. */
int eg_coord_mlp_fwd_rows(const float* lm, int64_t lm_frame_stride, float* lm_copy, const float* coords, int batch,
                          const eg_cls_train_params* params, int train, int frame, float* z1, float* z2, float* bn, float* pre,
                          float* new_coords, eg_stream_t stream);
int eg_coord_mlp_bwd_rows(const float* dnew_coords, const float* lm, const float* coords, int batch,
                          const eg_cls_train_params* params, int frame, const float* z1, const float* z2, const float* bn,
                          const float* pre, float* scratch, float* dlm, int64_t dlm_frame_stride, int dlm_accumulate,
                          float* dcoords, float* grads, eg_stream_t stream);

/* ---- coordinate-graph resampling (src/core/models.py:539-553 as a 4-tap gather) -------------------
 * coords [batch*points, 2] in (h, w) order; out[p,:] = bilinear sample of frame p/points' main grid
 * (rows main_base .. main_base + frame*frame of each frame's node block), zero outside the grid. */
int eg_bilinear4_fwd(const float* h, const float* coords, int batch, int points, int64_t n_per_frame, int64_t main_base,
                     int frame, float* out, eg_stream_t stream);
/* dh (nullable) is accumulated into (+=) at the touched rows; dcoords (nullable) [batch*points,2] is overwritten */
int eg_bilinear4_bwd(const float* dout, const float* h, const float* coords, int batch, int points, int64_t n_per_frame,
                     int64_t main_base, int frame, float* dh, float* dcoords, eg_stream_t stream);
/* ... with the sample rows of frame f at out / dout + f * frame_stride (floats): the samples land in (their gradient is read
 * from) the coordinate rows of the node array itself (models.py:473 h[node_type == 1] = new features). */
int eg_bilinear4_fwd_rows(const float* h, const float* coords, int batch, int points, int64_t n_per_frame, int64_t main_base,
                          int frame, float* out, int64_t out_frame_stride, eg_stream_t stream);
int eg_bilinear4_bwd_rows(const float* dout, int64_t dout_frame_stride, const float* h, const float* coords, int batch, int points,
                          int64_t n_per_frame, int64_t main_base, int frame, float* dh, float* dcoords, eg_stream_t stream);
/* ... and, when dh is the dy of a layer whose BatchNorm-backward sums were taken BEFORE this call (eg_gcn_layer_bwd_lower), the
 * sums of what is added here: tap_sums [batch][2][128] floats = per frame  sum add * mask, sum add * mask * xhat  over its taps
 * (lower->z, bn, relu, dropout_p, seed describe that layer; the other fields are not used). */
int eg_bilinear4_bwd_rows_sums(const float* dout, int64_t dout_frame_stride, const float* h, const float* coords, int batch, int points,
                               int64_t n_per_frame, int64_t main_base, int frame, float* dh, float* dcoords,
                               const eg_lower_sums* lower, float* tap_sums, eg_stream_t stream);

/* ---- the whole coordinate update of one GNN layer (models.py:438-473) on the node array in place -------------------------------
 * eg_coord_update_fwd = eg_coord_mlp_fwd_rows on the 4 coordinate rows of every frame of h (rows coord_base .. coord_base + 3 of
 * each frame's n_per_frame rows; lm_copy, z1, z2, bn, pre, new_coords as there; new_coords2, nullable: a second [R,2] copy of the
 * new coordinates -- one to hand out, one to keep for the backward, without a copy launch) followed, when resample != 0, by
 * eg_bilinear4_fwd_rows at the new positions into those same rows.  Up to batch 16 (64 rows) that is ONE single-workgroup launch
 * with every intermediate in LDS (a training step at batch 1 is ~1 ms: six 20-us launches were 12 % of it); above, the two launches.
 * eg_coord_update_bwd = the backward of both on the gradient array dx (the gradient w.r.t. the tensor AFTER the update, turned in
 * place into the gradient w.r.t. the tensor before it): eg_bilinear4_bwd_rows[_sums] (samples' gradient read from dx's coordinate
 * rows, taps added to its main-grid rows; lower / tap_sums as in eg_bilinear4_bwd_rows_sums, both NULL: none), then
 * eg_coord_mlp_bwd_rows with d new_coords = dnew_coords (nullable) + the resampling's d coords, dlm WRITTEN into dx's coordinate
 * rows.  dbil: [R,2] floats of workspace (the resampling's d coords; used above batch 16 only); scratch [R,56] as eg_coord_mlp_bwd.
 * One launch up to batch 16, three above. */
int eg_coord_update_fwd(float* h, int64_t n_per_frame, int64_t coord_base, int64_t main_base, const float* coords, int batch,
                        const eg_cls_train_params* params, int train, int frame, int resample, float* lm_copy, float* z1, float* z2,
                        float* bn, float* pre, float* new_coords, float* new_coords2, eg_stream_t stream);
int eg_coord_update_bwd(float* dx, int64_t n_per_frame, int64_t coord_base, int64_t main_base, const float* h, const float* new_coords,
                        const float* dnew_coords, const float* lm, const float* coords, int batch, const eg_cls_train_params* params,
                        int frame, const float* z1, const float* z2, const float* bn, const float* pre, float* scratch, float* dbil,
                        const eg_lower_sums* lower, float* tap_sums, float* dcoords, float* grads, eg_stream_t stream);

/* ---- the optimizer update of the training step (reference: torch.optim.Adam through src/engine.py's optimizer) as ONE launch ---
 * torch's fused Adam arithmetic (ADAM_MODE::ORIGINAL, amsgrad off) on up to 96 tensors per call:
 *   g = grad (maximize: -grad) + weight_decay * p;  m += (1 - beta1) (g - m);  v = beta2 v + (1 - beta2) g g
 *   p -= lr / (1 - beta1^t) * m / (sqrt(v) / sqrt(1 - beta2^t) + eps),   t = steps[k] + 1;   then steps[k] = t
 * tensors: HOST array of `count` entries (device pointers; they travel in the kernel arguments, so a captured launch keeps them);
 * steps: [count] device floats, the number of updates of each tensor so far.  lr_device (nullable): the learning rate as a device float,
 * read by the kernel instead of `lr` -- what a scheduler changes between the replays of a captured step.  EG_ERR_UNSUPPORTED (nothing
 * launched) for count > EG_ADAM_MAX_TENSORS (96, below). */
typedef struct eg_adam_tensor {
    float* param;
    const float* grad;
    float* exp_avg;
    float* exp_avg_sq;
    int64_t numel;
} eg_adam_tensor;
int eg_adam_step(const eg_adam_tensor* tensors, int count, float* steps, float lr, const float* lr_device, float beta1, float beta2, float eps, float weight_decay,
                 int maximize, eg_stream_t stream);

/* ---- the reference's other two optimizer names (src/builders/optimizer_builder.py: sgd, rmsprop), each ONE launch like eg_adam_step:
 * a HOST array of `count` entries of device pointers that travels in the kernel arguments, steps [count] device floats (the number of
 * updates of each tensor so far, advanced by the launch), lr / lr_device as in eg_adam_step.  Every argument check comes before the
 * first HIP call.  EG_ERR_UNSUPPORTED (nothing launched) for count > EG_SGD_MAX_TENSORS / EG_RMSPROP_MAX_TENSORS: split the list.
 * eg_sgd_step -- torch.optim.SGD (_single_tensor_sgd's order):
 *   g = grad (maximize: -grad) + weight_decay * p
 *   momentum != 0:  buf = steps[k] == 0 ? g : momentum * buf + (1 - dampening) * g;   g = nesterov ? g + momentum * buf : buf
 *   p -= lr * g;   then steps[k] += 1
 * The first update of a tensor copies g into the buffer; the kernel reads that from the DEVICE count, so the arguments of the launch
 * are the same in every step.  momentum == 0: momentum_buffer may be NULL and is not touched; otherwise it must not be NULL.
 * EG_ERR_ARG: nesterov with momentum <= 0 or dampening != 0, momentum < 0, weight_decay < 0 (torch's constructor checks).
 * eg_rmsprop_step -- torch.optim.RMSprop (_single_tensor_rmsprop's order):
 *   g as above;  sq = alpha * sq + (1 - alpha) * g * g
 *   centered:  ga += (1 - alpha) * (g - ga);  avg = sqrt(sq - ga * ga) + eps          else:  avg = sqrt(sq) + eps
 *   momentum > 0:  buf = momentum * buf + g / avg;  p -= lr * buf                     else:  p -= lr * g / avg;   then steps[k] += 1
 * grad_avg non-NULL exactly when centered, momentum_buffer non-NULL exactly when momentum > 0, else EG_ERR_ARG; EG_ERR_ARG as well
 * for alpha, eps, momentum or weight_decay < 0. */
#define EG_ADAM_MAX_TENSORS 96
#define EG_SGD_MAX_TENSORS 120
#define EG_RMSPROP_MAX_TENSORS 84
typedef struct eg_sgd_tensor {
    float* param;
    const float* grad;
    float* momentum_buffer; /* nullable (momentum == 0) */
    int64_t numel;
} eg_sgd_tensor;
typedef struct eg_rmsprop_tensor {
    float* param;
    const float* grad;
    float* square_avg;
    float* grad_avg;        /* non-NULL iff centered */
    float* momentum_buffer; /* non-NULL iff momentum > 0 */
    int64_t numel;
} eg_rmsprop_tensor;
int eg_sgd_step(const eg_sgd_tensor* tensors, int count, float* steps, float lr, const float* lr_device, float momentum, float dampening,
                float weight_decay, int nesterov, int maximize, eg_stream_t stream);
int eg_rmsprop_step(const eg_rmsprop_tensor* tensors, int count, float* steps, float lr, const float* lr_device, float alpha, float eps,
                    float weight_decay, float momentum, int centered, int maximize, eg_stream_t stream);

/* ---- losses on the logits and landmark decode (the steps right after the hot path) ---------------------
 * Reference: src/core/criterion.py:13-27 (WeightedBCEWithLogitsLoss), :93-151 (ExpectedLandmarkMSE),
 * src/core/evaluators.py:291-391,485-495 (softmax heat map -> expected landmark position, hard argmax).
 * The logits of a frame are [n_rows, 4]; level l occupies rows level_start[l] .. + level_side[l]^2, row-major
 * (h, w).  level_start / level_side are HOST arrays of n_levels <= 16 ints.  workspace: device memory of
 * eg_heatmap_workspace_bytes() bytes, owned by the caller.  Nothing here synchronises or reads back.
 *
 * eg_heatmap_expect_fwd: for every (frame b, level l, channel c)
 *   expect [batch,n_levels,4,2] f32  softmax over the level's nodes, expectation of (h, w)
 *   stats  [batch,n_levels,4,2] f32  (max logit, sum exp(x - max)) for the backward, or NULL
 *   argmax [batch,n_levels,4]  i64   row index (within the level) of the first maximum logit, or NULL
 *   gt     [batch,n_levels,4,2] f32  (h, w) of the label heat map: arg max over rows of the row maxima, over
 *                                    columns of the column maxima (first index wins), needs labels; or NULL
 *   vmean  [batch,n_levels,4]  f32   mean of `valid` over the level's nodes, needs valid; or NULL
 * eg_heatmap_expect_bwd: d_logits[r,c] = p[r,c] * ((h - E_h) dE_h + (w - E_w) dE_w), rows outside every level 0.
 * eg_bce_logits_fwd: out3 = { sum(w * bce(x, y) * valid), sum(valid), their ratio }, w = ones_weight where
 *   y == 1 (when ones_weight > 1) else 1; valid may be NULL (= 1).  fp64 sums in a fixed order.
 * eg_bce_logits_bwd: d_logits = (sigmoid(x) - y) * w * valid * scale_dev[0].
 * eg_bce_probs_fwd / _bwd: the same on probabilities p (nn.BCELoss, the reference's WeightedBCE, criterion.py:6-27) with torch's
 *   element formula bce(p, y) = (y - 1) max(log1p(-p), -100) - y max(log p, -100) and gradient
 *   d_probs = (p - y) / max((1 - p) p, 1e-12) * w * valid * scale_dev[0].  torch raises for p outside [0, 1]; these cannot (they may
 *   be captured into a graph), so an element outside [0, 1] or NaN makes the loss (out3[0], out3[2]) NaN -- whatever its valid --
 *   and its own gradient NaN. */
size_t eg_heatmap_workspace_bytes(int batch, const int* level_side, int n_levels);
int eg_heatmap_expect_fwd(const float* logits, const float* labels, const float* valid, int batch, int64_t n_rows,
                          const int* level_start, const int* level_side, int n_levels, void* workspace, float* expect,
                          float* stats, int64_t* argmax, float* gt, float* vmean, eg_stream_t stream);
int eg_heatmap_expect_bwd(const float* logits, const float* expect, const float* stats, const float* d_expect, int batch,
                          int64_t n_rows, const int* level_start, const int* level_side, int n_levels, float* d_logits,
                          eg_stream_t stream);
/* eg_heatmap_render: the pictures of one level of `count` consecutive frames in ONE launch (src/core/evaluators.py:485-616:
 * get_softmaxed_heatmap, the per-channel normalisation of get_heatmaps, create_overlay_image + ToPILImage).  No workspace, no
 * atomics, no read-back.  The level is rows level_start .. level_start + side * side - 1 of every frame, row-major (h, w); the
 * main grid is level_start = n_rows - F * F, side = F.
 *   logits [count * n_rows, 4] f32 (16-byte aligned); labels the same, or NULL; stats [count,4,2] f32 = (M, S) per frame and
 *   channel: what eg_heatmap_expect_fwd writes as `stats` for that ONE level.
 *   image: pixel (h, w) of frame i is image[i * image_stride + h * side + w] (channel 0 of a contiguous [B,C,F,F] tensor:
 *   image_stride = C * F * F, no copy); NULL: black.
 *   heat [count,side,side,4] f32 (16-byte aligned) = expf(x - M) / S, the p of eg_heatmap_expect_bwd; x = -inf gives 0, a channel
 *   whose M is -inf (no finite logit) is 0 everywhere.
 *   pred_rgb / gt_rgb / base_rgb [count,side,side,3] u8 (HWC: what ToPILImage yields).  In fp32, in the reference's operation
 *   order (colour * value, then max, then * 255, then truncate):
 *     e_c = expf(x_c - M_c)      the per-channel normalised map: the reference forms p / max p and max p is 1 / S -- the value
 *                                that quotient rounds to, without a second reduction
 *     base = max(0, 0.8f * image)                                (the same for R, G and B)
 *     pred_k = max(base, max_c col[c][k] * e_c),  gt_k = max(base, max_c col[c][k] * label_c)
 *     col = (0,1,1), (1,0.7,0.9), (0,1,0), (1,0,0) for channels 0..3
 *     byte = (uint8) min(v * 255.0f, 255.0f), truncated toward zero; NaN gives 0.
 *   The reference's .byte() wraps past 255 (or is undefined there); this SATURATES at 255 -- a difference that cannot arise
 *   for frames in [0, 1], where no value exceeds 1.
 * Every output may be NULL, at least one must be given; gt_rgb needs labels.  EG_ERR_ARG (nothing launched): NULL logits or
 * stats, no output, gt_rgb without labels, misaligned logits / labels / heat, count < 1, side < 1, level_start < 0,
 * level_start + side * side > n_rows. */
int eg_heatmap_render(const float* logits, const float* labels, const float* image, int64_t image_stride,
                      const float* stats, int count, int64_t n_rows, int level_start, int side,
                      float* heat, uint8_t* pred_rgb, uint8_t* gt_rgb, uint8_t* base_rgb, eg_stream_t stream);
/* ExpectedLandmarkMSE's combination of those expectations (criterion.py:133-151) and its gradient in one launch:
 *   loss[0] = weight * sum_{l,c,xy} [ sum_b ((expect - gt) * inv_side[l])^2 * vmean ] / nv,  nv = sum_b vmean (1 where 0);
 *   d_expect [batch,n_levels,4,2] = d loss / d expect.  inv_side: DEVICE array [n_levels] = 1 / level side. */
int eg_elm_reduce(const float* expect, const float* gt, const float* vmean, const float* inv_side, int batch, int n_levels,
                  float weight, float* loss, float* d_expect, eg_stream_t stream);
int eg_bce_logits_fwd(const float* logits, const float* labels, const float* valid, int64_t n, float ones_weight,
                      void* workspace, float* out3, eg_stream_t stream);
int eg_bce_logits_bwd(const float* logits, const float* labels, const float* valid, int64_t n, float ones_weight,
                      const float* scale_dev, float* d_logits, eg_stream_t stream);
int eg_bce_probs_fwd(const float* probs, const float* labels, const float* valid, int64_t n, float ones_weight,
                     void* workspace, float* out3, eg_stream_t stream);
int eg_bce_probs_bwd(const float* probs, const float* labels, const float* valid, int64_t n, float ones_weight,
                     const float* scale_dev, float* d_probs, eg_stream_t stream);

/* ---- the criteria of a training step as ONE node (src/engine.py:582-600: the sum of WeightedBCEWithLogitsLoss, ExpectedLandmarkMSE
 * and, with the coordinate graph, MSE on the landmark coordinates -- criterion.py:13-27, :36-48, :93-151).
 * eg_criteria_fwd (4 launches): *bce = w_bce * sum(w bce(x, y) valid) / sum(valid); *elm = eg_elm_reduce's loss with weight w_elm;
 *   *coord = w_coord * mean((coord_pred - coord_y)^2) over n_coord elements (coord_pred NULL: no such criterion, *coord untouched);
 *   *total = their sum.  Kept for the backward: expect, stats [batch,n_levels,4,2], d_expect (= d elm / d expect), d_coord [n_coord]
 *   (= d coord / d coord_pred), bce_scale [1].  inv_side: DEVICE [n_levels] = 1 / level side.  workspace: eg_criteria_workspace_bytes().
 * eg_criteria_bwd (1 launch): d_logits = (g_total + g_bce) * d bce / d logits + (g_total + g_elm) * d elm / d logits,
 *   d_coord_out (nullable) = (g_total + g_coord) * d_coord;  g_*: upstream gradients as DEVICE scalars, each nullable (= 0).
 * eg_criteria_ex_fwd / _bwd: the same with two more arguments (eg_criteria_* are their (0, 0) case, bit for bit), each 0 or 1:
 *   bce_on_probs = 1: the BCE term is eg_bce_probs_fwd's on the `logits` array read as probabilities (WeightedBCE, criterion.py:6-27;
 *     NaN rule as there); ExpectedLandmarkMSE still takes its softmax over the same array, as the reference's engine gives both
 *     criteria the model's output.  _bwd must get the same value.
 *   coord_l1 = 1: *coord = w_coord * mean|coord_pred - coord_y| (MAE, criterion.py:51-63), d_coord = w_coord sign(pred - y) / n_coord
 *     with sign(0) = 0 (torch's l1_loss backward).  The backward does not depend on it.
 *   Same launches as eg_criteria_*, no host synchronisation, no allocation. */
size_t eg_criteria_workspace_bytes(int batch, const int* level_side, int n_levels);
int eg_criteria_fwd(const float* logits, const float* labels, const float* valid, int batch, int64_t n_rows, const int* level_start,
                    const int* level_side, int n_levels, const float* inv_side, float bce_ones_weight, float w_bce, float w_elm,
                    const float* coord_pred, const float* coord_y, int64_t n_coord, float w_coord, void* workspace, float* expect,
                    float* stats, float* d_expect, float* d_coord, float* bce_scale, float* total, float* bce, float* elm, float* coord,
                    eg_stream_t stream);
int eg_criteria_bwd(const float* logits, const float* labels, const float* valid, int batch, int64_t n_rows, const int* level_start,
                    const int* level_side, int n_levels, float bce_ones_weight, const float* expect, const float* stats,
                    const float* d_expect, const float* bce_scale, const float* d_coord, int64_t n_coord, const float* g_total,
                    const float* g_bce, const float* g_elm, const float* g_coord, float* d_logits, float* d_coord_out,
                    eg_stream_t stream);
int eg_criteria_ex_fwd(const float* logits, const float* labels, const float* valid, int batch, int64_t n_rows, const int* level_start,
                       const int* level_side, int n_levels, const float* inv_side, float bce_ones_weight, float w_bce, float w_elm,
                       const float* coord_pred, const float* coord_y, int64_t n_coord, float w_coord, void* workspace, float* expect,
                       float* stats, float* d_expect, float* d_coord, float* bce_scale, float* total, float* bce, float* elm, float* coord,
                       int bce_on_probs, int coord_l1, eg_stream_t stream);
int eg_criteria_ex_bwd(const float* logits, const float* labels, const float* valid, int batch, int64_t n_rows, const int* level_start,
                       const int* level_side, int n_levels, float bce_ones_weight, const float* expect, const float* stats,
                       const float* d_expect, const float* bce_scale, const float* d_coord, int64_t n_coord, const float* g_total,
                       const float* g_bce, const float* g_elm, const float* g_coord, float* d_logits, float* d_coord_out,
                       int bce_on_probs, int coord_l1, eg_stream_t stream);

/* ---- confusion counts of the landmark classifier (reference: BalancedBinaryAccuracyEvaluator, src/core/evaluators.py:85-143) --
 * pred, y, valid: [rows, channels] f32 (1 <= channels <= 8, rows >= 1).  For every channel c, over the rows with valid > 0:
 *   TP = #(y != 0 and pred > 0.5), FN = #(y != 0 and not pred > 0.5), FP = #(y == 0 and pred > 0.5), TN = #(y == 0 and not pred > 0.5)
 * (a strict > 0.5 on whatever the model returned; a NaN prediction is a negative one).  ONE launch, integer counts, exact and
 * bit-reproducible.  Writes the record history[k][c][0..3] = {TP, FN, FP, TN} (int64, history: [capacity][channels][4]) where
 * k = *counter, a device int64 the launch then advances by one: a launch captured into a HIP graph appends one record per replay.
 * With k >= capacity nothing is written but *counter still advances (the reader detects the overflow).  workspace: device memory of
 * workspace_bytes bytes (8-byte aligned) for the per-workgroup partials, 512 * channels * 32 bytes for the full grid (less gives
 * fewer workgroups); it must not be shared with a launch in flight on another stream.  The completion ticket is a word per
 * (device, stream) allocated at the first launch on a stream: make that first launch outside a stream capture.
 * EG_ERR_UNSUPPORTED for channels outside 1..8, EG_ERR_ARG for a NULL buffer or misaligned 64-bit buffer; nothing launched then. */
int eg_confusion_counts(const float* pred, const float* y, const float* valid, int64_t rows, int channels, void* workspace,
                        size_t workspace_bytes, int64_t* history, int64_t capacity, int64_t* counter, eg_stream_t stream);

/* ---- landmark-evaluator records (reference: LandmarkExpectedCoordiantesEvaluator.update, src/core/evaluators.py:291-391) -----
 * One update appends ONE record to a device-side history and advances *counter (a device int64) by one: a launch sequence
 * captured into a HIP graph appends one record per replay.  Record k = *counter (history: [capacity][16] f32):
 *   [0..3]   coordinate errors of lvid_top, lvid_bot, lvpw, ivs (sum over the frames of err * vs, divided by nv)
 *   [4..7]   valid flags of the same landmarks (1.0 iff nv > 0 before a zero nv became 1)
 *   [8..10]  width MAE of ivs, lvid, lvpw;  [11..13] width MPE of ivs, lvid, lvpw;  [14..15] 0
 * and its per-frame detail block (detail: [capacity][batch][24] f32): pred (h, w) of the 4 landmarks [0..7], gt (h, w) [8..15],
 * pred widths in mm {ivs, lvid, lvpw} [16..18], gt widths [19..21], 0 [22..23].  vs = the per-(frame, landmark) mean of valid,
 * nv = its sum over the frames.  fp32 in the host class's operation order without FMA contraction, sums over the frames in
 * ascending order: bit-reproducible; a landmark without a valid row and a zero ground-truth width give the host's IEEE results.
 * With k >= capacity nothing is written but *counter still advances (the reader detects the overflow).  pix2mm_x / pix2mm_y:
 * [batch] f32 device arrays.  No allocation, no memset, no host synchronisation.
 * eg_landmark_record_hm: heat-map models.  logits / labels / valid [batch * n_rows, 4] f32 (16-byte aligned); the main grid is
 *   the last frame * frame rows of every frame: softmax-expected (h, w), the label's (h, w) and vs as eg_heatmap_expect_fwd
 *   decodes them.  TWO launches; the last workgroup of the second computes the record.  workspace: device memory of at least
 *   eg_landmark_record_workspace_bytes(batch, frame) bytes (8-byte aligned), not shared with a launch in flight on another
 *   stream.  The completion ticket is a word per (device, stream) allocated at the first launch on a stream: make that first
 *   launch outside a stream capture.
 * eg_landmark_record_coord: coordinate-graph models.  coord_pred / coord_y [batch * 4, 2] f32 (h, w); every landmark counts as
 *   valid (vs = 1).  ONE launch, no workspace.
 * EG_ERR_ARG for a NULL or misaligned buffer, a main grid larger than the frame's rows or a short workspace; nothing launched then. */
size_t eg_landmark_record_workspace_bytes(int batch, int frame);
int eg_landmark_record_hm(const float* logits, const float* labels, const float* valid, int batch, int64_t n_rows, int frame,
                          const float* pix2mm_x, const float* pix2mm_y, void* workspace, size_t workspace_bytes, float* history,
                          float* detail, int64_t capacity, int64_t* counter, eg_stream_t stream);
int eg_landmark_record_coord(const float* coord_pred, const float* coord_y, int batch, const float* pix2mm_x, const float* pix2mm_y,
                             float* history, float* detail, int64_t capacity, int64_t* counter, eg_stream_t stream);

/* ---- dense node labels from landmark coordinates (reference: create_node_labels, src/core/datasets.py:1586-1612) ----------
 * What the criteria and evaluators above read as `labels` / `valid`, built on the device from what a sample actually carries:
 *   coords [batch, 4, 2] i32  (h, w) of the 4 landmarks of every frame      valid4 [batch, 4] f32, or NULL (= 1)
 *   labels [batch * n_rows, 4] f32 (16-byte aligned)                         valid  [batch * n_rows, 4] f32, or NULL (not written)
 * level_start / level_side: HOST arrays of n_levels (1 .. 16) ints as eg_heatmap_expect_fwd takes them; the LAST level is the main
 * grid and its side must equal frame_size (F); every other level is an aux level, whatever its side.
 *   labels[b * n_rows + level_start[l] + i * p + j, c] = 1 iff (i, j) == (bin(h), bin(w)) of landmark c of frame b, else 0 (p = level_side[l])
 *     aux level:  bin(v) = (v * p) / F (integer division) for 0 <= v < F;   p - 1 for -F <= v < 0
 *     last level: bin(v) = v                              for 0 <= v < F;   v + F for -F <= v < 0
 *   which is np.digitize(v, np.linspace(0, F, p + 1)) - 1 and numpy's wrap-around of a negative index, as the reference computes them.
 *   A landmark with h or w outside [-F, F) -- an IndexError in the reference -- has no 1 on any level; the other channels are not
 *   affected.  Rows outside every level are 0.
 *   valid[b * n_rows + r, c] = valid4[b, c] (1 when valid4 is NULL).
 * ONE launch; every element is written exactly once (no fill pass, no atomics); no allocation, no synchronisation: capturable.
 * EG_ERR_ARG, nothing launched: batch < 1, n_levels outside 1 .. 16, a level that does not fit in n_rows, a last level whose side
 * is not frame_size, NULL coords or labels, misaligned labels / valid. */
int eg_node_labels(const int* coords, const float* valid4, int batch, int64_t n_rows, const int* level_start, const int* level_side,
                   int n_levels, int frame_size, float* labels, float* valid, eg_stream_t stream);

/* ---- frame preparation (reference: src/core/datasets.py, frame.float().div(255), UICLVLandmark.transform_image :317-349, the
 * landmarks through the same matrix :232-236, dataset_builder's Resize((F, F)) / Grayscale, hflip with probability flip_p) ------
 * What a dataset does per sample on the host between "a frame was read" and "x / coords exist", for a batch:
 *   src [batch, channels, src_h, src_w] uint8 (src_is_u8 != 0) or float32, channels 1 or 3
 *   out [batch, C_out, F, F] float32, F = frame_size, C_out = 1 when gray (channels must be 3 then), else channels
 *   matrix_inv, matrix_fwd [batch, 2, 3] float32 [A | b], acting on normalised (h, w) in [-1, 1]
 *   flip [batch] bytes, or NULL (no flip)
 *   warp_size = W > 0: a warp stage to a W x W image; matrix_inv must be given.  W = 0: none; matrix_inv must be NULL.
 *   coords_in [batch, 4, 2] float32 (h, w), or NULL: no coordinate part (matrix_fwd, crop_size, label_coords, coord_y are ignored)
 *   label_coords [batch, 4, 2] int32;  coord_y [batch * 4, 2] float32, or NULL
 * Pixels.  v(c, y, x) = src / 255 (a division) for uint8, src itself for float32; 0 outside [0, src_h) x [0, src_w).
 *   warped(c, i, j), 0 <= i, j < W (affine_grid + grid_sample(bilinear, zeros, align_corners=False) as transform_image drives them):
 *     n_h = (2 i + 1) / W - 1, n_w = (2 j + 1) / W - 1;   s_h = A00 n_h + A01 n_w + b0, s_w = A10 n_h + A11 n_w + b1 with matrix_inv
 *     y = ((s_h + 1) src_h - 1) / 2, x = ((s_w + 1) src_w - 1) / 2, y0 = floor(y), x0 = floor(x), fy = y - y0, fx = x - x0
 *     warped = (1-fy)(1-fx) v(y0, x0) + (1-fy) fx v(y0, x0+1) + fy (1-fx) v(y0+1, x0) + fy fx v(y0+1, x0+1)
 *   without a warp stage warped = v, of sides src_h x src_w.
 *   resized(c, i, j), 0 <= i, j < F (interpolate(bilinear, align_corners=False), no antialiasing), per axis over a side S of warped:
 *     s = max((o + 0.5) S / F - 0.5, 0), i0 = floor(s), i1 = min(i0 + 1, S - 1), l = s - i0;  the four-tap blend of warped.
 *   gray (after the resize): 0.2989 R + 0.587 G + 0.114 B.
 *   out[b, c, i, flip[b] ? F - 1 - j : j] = resized(c, i, j).
 *   Tap positions are computed in fp64, weights and blends in fp32; the W x W image is never materialised.
 * Landmarks (fp64).  With a warp stage, for c = coords_in[b, k] in crop pixels, per axis: n = c 2 / crop_size - 1,
 *   n' = A n + b with matrix_fwd, q = (n' + 1) W / 2 * F / W.  Without one q = c.  label_coords = (int) q, toward zero (saturating;
 *   NaN gives INT_MIN); then, where flip[b], w <- F - w - 1.  coord_y holds the same integers as float32.
 * ONE launch; every output element is written exactly once (no atomics: the same bits from run to run); no allocation, no
 * synchronisation: capturable.  EG_ERR_ARG, nothing launched: a size < 1 or a side above 32768, channels not 1 or 3, gray without 3
 * channels, warp_size < 0, matrix_inv missing with or given without a warp stage, NULL src / out, coords_in without label_coords or
 * (with a warp stage) without matrix_fwd / crop_size >= 1, a misaligned float pointer, batch * F^2 too large for one grid. */
int eg_frame_prep(const void* src, int src_is_u8, int batch, int channels, int src_h, int src_w, const float* matrix_inv,
                  int warp_size, int frame_size, const unsigned char* flip, int gray, float* out, const float* coords_in,
                  const float* matrix_fwd, int crop_size, int* label_coords, float* coord_y, eg_stream_t stream);

/* ---- UNet front-end, inference (reference: DownConv / UpConv, src/core/models.py:841-876, in eval mode) ---------------------
 * fp32 NCHW, contiguous, square maps of side 1 .. 512 with 1 .. 512 channels; 4-byte alignment is enough.
 * eg_conv3x3_relu_bn_fwd: Conv2d(kernel 3, padding 1, zero padding) -> ReLU -> BatchNorm2d with running statistics, ONE launch:
 *     out[b, o] = (relu(bias[o] + conv3x3(input)[b, o]) - bn_mean[o]) / sqrt(bn_var[o] + bn_eps) * bn_weight[o] + bn_bias[o]
 *   (the reference's order: the BatchNorm comes AFTER the ReLU and is not folded into the weights; bn_weight may be negative).
 *   input = the channel concatenation of
 *     x0 [batch, c0, side0, side0] resized to side by nn.Upsample(size=side)'s nearest rule, src = min(dst * side0 / side, side0 - 1)
 *        in integers (side0 == side: x0 as it is), and
 *     x1 [batch, c1, side, side], or NULL together with c1 == 0,
 *   so `upsample -> conv1` and `cat([x, skip]) -> conv2` of UpConv need no intermediate tensor.  weight [c_out, c0 + c1, 3, 3] is
 *   torch's own Conv2d layout, read in place; bias, bn_weight, bn_bias [c_out] may be NULL (0, 1, 0); bn_mean, bn_var [c_out].
 *   out [batch, c_out, side, side] must not alias an input.  Sides above 16 run an LDS-tiled kernel, sides up to 16 one that splits
 *   K = 9 (c0 + c1) over the waves of a workgroup and adds the partial sums in wave order.
 * eg_adaptive_max_pool_fwd: nn.AdaptiveMaxPool2d(side_out) on x [planes, side_in, side_in] -> out [planes, side_out, side_out];
 *   window i = [floor(i side_in / side_out), ceil((i + 1) side_in / side_out)) in both directions; a NaN in a window is its result.
 * Both: enqueue on the caller's stream, no allocation, no synchronisation, no atomics, a fixed summation order (bit-identical from
 * run to run), capturable.  EG_ERR_ARG, nothing launched: a NULL required pointer, batch / planes < 1, a channel count or side
 * < 1, x1 without c1 or c1 without x1, side_out > side_in, bn_eps < 0, out aliasing an input.  EG_ERR_UNSUPPORTED, nothing
 * launched: a channel count (c0 + c1 or c_out) or a side above 512, batch above 65535. */
int eg_conv3x3_relu_bn_fwd(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side, const float* weight,
                           const float* bias, const float* bn_weight, const float* bn_bias, const float* bn_mean,
                           const float* bn_var, float bn_eps, int c_out, float* out, eg_stream_t stream);
int eg_adaptive_max_pool_fwd(const float* x, int planes, int side_in, int side_out, float* out, eg_stream_t stream);

/* ---- UNet front-end, training (the same block with batch statistics, and its backward) ----------------------------------------
 * One conv3x3 -> ReLU -> BatchNorm2d block in training mode is eg_conv3x3_relu_fwd + eg_bn2d_train_fwd (3 launches); its backward is
 * eg_relu_bn2d_bwd, eg_conv3x3_bwd_data and eg_conv3x3_bwd_weight (up to 7).  Sources, layouts and limits are the forward's above.
 * workspace: device memory of eg_frontend_train_workspace_bytes(batch, c0 + c1, c_out, side) bytes (0: shapes out of range), owned by
 * the caller, shared by the calls of one block on one stream.
 * eg_conv3x3_relu_fwd:  r[b, o] = relu(bias[o] + conv3x3(input)[b, o]) -- the eval kernels with another epilogue.
 * eg_bn2d_train_fwd:    per channel, mean and biased variance over n = batch side^2 values of r;
 *     y = (r - mean) * gamma / sqrt(var + eps) + beta, save_mean = mean, save_invstd = 1 / sqrt(var + eps),
 *     running_mean = (1 - momentum) running_mean + momentum mean, running_var likewise with var n / (n - 1); both may be NULL.
 *     gamma, beta may be NULL (1, 0).  n == 1 is refused (EG_ERR_ARG) with torch's message.
 * eg_relu_bn2d_bwd:     dbeta = sum dy, dgamma = sum dy xhat (xhat = (r - save_mean) save_invstd),
 *     dz = gamma save_invstd (dy - dbeta / n - xhat dgamma / n) [r > 0], dbias = sum dz.  dgamma, dbeta, dbias [channels] may be NULL.
 * eg_conv3x3_bwd_data:  d input = conv3x3(dz, weight transposed, taps flipped); channels >= c0 go to dx1 [batch, c1, side, side],
 *     channels < c0 to dx0 [batch, c0, side0, side0]: where side0 != side every source pixel adds the destination pixels that read it
 *     (src = min(dst * side0 / side, side0 - 1)) in row-major order out of `full` [batch, c0, side, side], scratch the caller brings.
 *     dx0 or dx1 may be NULL (not wanted); enlargements above 16 x are EG_ERR_UNSUPPORTED for dx0.
 * eg_conv3x3_bwd_weight: dweight[o][c][ky][kx] = sum_{b, y, x} dz[b, o, y, x] input[b, c, y + ky - 1, x + kx - 1] (zero padding).
 * eg_adaptive_max_pool_idx_fwd: eg_adaptive_max_pool_fwd that also writes idx [planes, side_out, side_out], the offset y * side_in + x
 *     of the window's first maximum in row-major order (a NaN always takes over: torch's rule).
 * eg_adaptive_max_pool_bwd: dx [planes, side_in, side_in]: every input pixel adds dy of the windows whose idx it is, in window order.
 * All: the caller's stream, no allocation, no synchronisation, no atomics; every sum has a fixed order in chains of at most 256
 * terms (bit-identical from run to run), capturable.  EG_ERR_ARG / EG_ERR_UNSUPPORTED as for the forward, nothing launched. */
size_t eg_frontend_train_workspace_bytes(int batch, int c_in, int c_out, int side);
int eg_conv3x3_relu_fwd(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side, const float* weight,
                        const float* bias, int c_out, float* r, eg_stream_t stream);
int eg_bn2d_train_fwd(const float* r, int batch, int channels, int side, const float* gamma, const float* beta, float eps,
                      float momentum, float* running_mean, float* running_var, void* workspace, float* y, float* save_mean,
                      float* save_invstd, eg_stream_t stream);
int eg_relu_bn2d_bwd(const float* dy, const float* r, const float* save_mean, const float* save_invstd, const float* gamma, int batch,
                     int channels, int side, void* workspace, float* dz, float* dgamma, float* dbeta, float* dbias,
                     eg_stream_t stream);
int eg_conv3x3_bwd_data(const float* dz, const float* weight, int batch, int c_out, int side, int c0, int side0, int c1, float* dx0,
                        float* dx1, float* full, eg_stream_t stream);
int eg_conv3x3_bwd_weight(const float* x0, int c0, int side0, const float* x1, int c1, int batch, int side, const float* dz, int c_out,
                          void* workspace, float* dweight, eg_stream_t stream);
int eg_adaptive_max_pool_idx_fwd(const float* x, int planes, int side_in, int side_out, float* out, int* idx, eg_stream_t stream);
int eg_adaptive_max_pool_bwd(const float* dy, const int* idx, int planes, int side_in, int side_out, float* dx, eg_stream_t stream);

/* ---- CNN embedder (reference: CNNResBlock, src/core/models.py:71-152; the first module of every step) --------------------------
 * One residual block on x [batch, c_in, side, side], fp32 NCHW, contiguous, square: side 1 .. 512, c_in and c_out 1 .. 128,
 * batch 1 .. 65535 with batch side^2 < 2^31; 4-byte alignment is enough.
 *     z = b3 + conv3x3(x, w3, zero padding 1)            w3 [c_out, c_in, 3, 3], b3 [c_out] or NULL: nn.Conv2d's own layout, in place
 *     y = (z - mean) * gamma / sqrt(var + eps) + beta    the BatchNorm comes BEFORE the ReLU and is not folded into the weights
 *     r = b1 + w1 x  (1 x 1: w1 [c_out, c_in], b1 [c_out] or NULL)   or   r = x  where w1 == NULL (needs c_in == c_out)
 *     out = relu(y + r) * keep[b, o]                     (nn.MaxPool2d(1) is the identity; Dropout2d drops whole (b, o) planes)
 * eg_embed_block_fwd: eval mode, ONE launch: mean / var are the running statistics, keep = 1.  r comes from the centre tap of the
 *   tile staged for the convolution, so x is read once.  bn_weight, bn_bias may be NULL (1, 0).
 * Training mode forward, 4 launches:
 *   eg_embed_conv_fwd:  z (the eval kernel with the plain epilogue);
 *   eg_bn2d_train_fwd (above) on z: y, save_mean, save_invstd and the running statistics;
 *   eg_embed_act_fwd:   out = relu(y + r) * keep, and keep [batch * c_out] itself: keep[i] = 0 or 1 / (1 - p), the counter-based mask
 *     of (seed + this device's dropout epoch, i = b * c_out + o) (csrc/train_common.h keep_scale; eg_dropout_epoch_* move the epoch,
 *     so replays of a captured step draw fresh planes).  p == 0: keep = 1.
 * Training mode backward, for g = d out, n = batch side^2, xhat = (z - save_mean) save_invstd:
 *   eg_embed_act_bwd (3 launches): ds = g keep [out > 0]; dbeta = db1 = sum ds; dgamma = sum ds xhat; dw1[o][c] = sum ds[b, o] x[b, c];
 *     dz = gamma save_invstd (ds - dbeta / n - xhat dgamma / n); db3 = sum dz (zero but for rounding).  ds, dz [batch, c_out, side,
 *     side] are required and must not alias an input or each other; dgamma, dbeta, db3, db1 [c_out], dw1 [c_out, c_in] may each be
 *     NULL (not wanted).  workspace: eg_embed_workspace_bytes(batch, c_in, c_out, side) bytes of device memory (0: shapes out of
 *     range), owned by the caller.  gamma may be NULL (1).
 *   eg_conv3x3_bwd_weight / eg_conv3x3_bwd_data (above) on (x, dz) give dw3 and the 3 x 3 part of dx;
 *   eg_embed_res_bwd_input: dx += w1^T ds (w1 == NULL: dx += ds), in place, AFTER the data gradient.
 *   5 launches without an input gradient (4 where the weight gradient has one slice), 7 with one.
 * All: the caller's stream, no allocation, no synchronisation, no atomics; every sum has a fixed order in chains of at most 256
 * terms (bit-identical from run to run), capturable.  EG_ERR_ARG, nothing launched: a NULL required pointer, batch, a channel count
 * or side < 1, w1 == NULL with c_in != c_out, b1 without w1, out / z / ds / dz / dx aliasing an input, bn_eps < 0, p outside [0, 1).
 * EG_ERR_UNSUPPORTED, nothing launched: a channel count above 128, a side above 512, batch above 65535 or batch side^2 >= 2^31. */
size_t eg_embed_workspace_bytes(int batch, int c_in, int c_out, int side);
int eg_embed_block_fwd(const float* x, int batch, int c_in, int side, const float* w3, const float* b3, const float* bn_weight,
                       const float* bn_bias, const float* bn_mean, const float* bn_var, float bn_eps, const float* w1, const float* b1,
                       int c_out, float* out, eg_stream_t stream);
int eg_embed_conv_fwd(const float* x, int batch, int c_in, int side, const float* w3, const float* b3, int c_out, float* z,
                      eg_stream_t stream);
int eg_embed_act_fwd(const float* y, const float* x, int batch, int c_in, int side, const float* w1, const float* b1, int c_out, float p,
                     uint64_t seed, float* keep, float* out, eg_stream_t stream);
int eg_embed_act_bwd(const float* dout, const float* out, const float* keep, const float* x, const float* z, const float* save_mean,
                     const float* save_invstd, const float* gamma, int batch, int c_in, int c_out, int side, void* workspace, float* ds,
                     float* dz, float* dgamma, float* dbeta, float* db3, float* db1, float* dw1, eg_stream_t stream);
int eg_embed_res_bwd_input(const float* ds, const float* w1, int batch, int c_in, int c_out, int side, float* dx, eg_stream_t stream);

/* ---- CNN pyramid (reference: CNNHierarchicalPatchModel, src/core/models.py:556-636: seven CNNResBlock(128 -> 128, kernel 3,
 * AdaptiveMaxPool2d(side_out)) in a row), eval mode -------------------------------------------------------------------------------
 * eg_pyramid_block_fwd: out [batch, 128, side_out, side_out] = relu(AdaptiveMaxPool2d(side_out)(BatchNorm_eval(conv3x3(x) + b3) + x))
 *   on x [batch, 128, side, side], fp32 NCHW, contiguous: c_in == c_out == 128, the residual is x itself, zero padding 1.
 *   w3 [128, 128, 3, 3] is nn.Conv2d's own layout, read in place at every call; b3, bn_weight, bn_bias [128] may be NULL (0, 1, 0) as
 *   for eg_embed_block_fwd; running_mean, running_var [128].  1 <= side_out <= side <= 512, batch 1 .. 65535 with batch side^2 < 2^31.
 *   Two steps: the convolution with the epilogue relu(bn(z) + x) (the ReLU in front of the pool: it is monotone, relu(max S) ==
 *   max relu(S) exactly), written to `scratch` where side_out != side and straight to `out` otherwise; then eg_adaptive_max_pool_fwd
 *   from scratch to out.  Sides from 4 on run the convolution as an implicit GEMM on the f32-input matrix instruction (the measured
 *   threshold: it is the faster route at every side of the pyramid), smaller ones on eg_embed_block_fwd's kernel.  THE ORDER OF SUMMATION is fixed and the same on both: k = c * 9 + 3 dy + dx ascending, one
 *   fmaf chain per output from 0, then + b3 and eg_embed_block_fwd's epilogue -- the result equals eg_embed_block_fwd's (followed by
 *   the pool) bit for bit at every side.
 *   scratch: eg_pyramid_block_scratch_bytes(batch, side, side_out) bytes of device memory owned by the caller: batch 128 side^2
 *   floats, 0 where side_out == side (scratch may then be NULL) or where the shapes are out of range.
 * The caller's stream, no allocation, no synchronisation, no atomics, bit-identical from run to run, capturable.  EG_ERR_ARG,
 * nothing launched: a NULL required pointer (scratch where side_out != side), batch or a side < 1, side_out > side, eps < 0, out or
 * scratch aliasing an input or each other.  EG_ERR_UNSUPPORTED, nothing launched: side above 512, batch above 65535 or
 * batch side^2 >= 2^31. */
size_t eg_pyramid_block_scratch_bytes(int batch, int side, int side_out);
int eg_pyramid_block_fwd(const float* x, int batch, int side, const float* w3, const float* b3, const float* bn_weight,
                         const float* bn_bias, const float* running_mean, const float* running_var, float eps, int side_out,
                         float* scratch, float* out, eg_stream_t stream);

/* ---- CNN pyramid, training mode (the same block with batch statistics, a pool with indices, a plane mask, and its backward) ----
 * x [batch, 128, side, side], fp32 NCHW, contiguous; 1 <= side_out <= side <= 512, batch 1 .. 65535 with batch side^2 < 2^31.
 * THE ORDER IS POOL, THEN ReLU, THEN DROPOUT, as in the reference's CNNResBlock.forward:
 *     z = b3 + conv3x3(x, w3, zero padding 1)            w3 [128, 128, 3, 3] read in place, b3 [128] or NULL
 *     y = (z - mean) * gamma / sqrt(var + eps) + beta    eg_bn2d_train_fwd (above) on z, unchanged: batch statistics, running ones move
 *     v = y + x                                          full size, never written
 *     (m, idx) = AdaptiveMaxPool2d(side_out)(v)          idx: the first maximum of a window in row-major order, a NaN takes over
 *     out = relu(m) * keep[b, o]                         keep: eg_embed_act_fwd's plane mask (seed + the device's epoch; p == 0: 1)
 * Backward, for g = d out, n = batch side^2, xhat = (z - save_mean) save_invstd:
 *     gp = g keep [out > 0] (pooled);  ds = the pool's backward of gp through idx: every input pixel adds the windows whose idx it is,
 *     in window order;  dbeta = sum ds, dgamma = sum ds xhat;  dz = gamma save_invstd (ds - dbeta / n - xhat dgamma / n);  db3 = sum dz;
 *     dw3 = the weight gradient of (x, dz);  dx = the data gradient of (dz, w3) + ds, the residual's share added AFTER the chain.
 * eg_pyramid_conv_fwd: z.  The eval kernel with the plain epilogue from side 8 on (the measured threshold of this epilogue),
 *     eg_embed_conv_fwd below: the same summation order (k = c * 9 + tap ascending, one fmaf chain from 0, + b3), so z equals
 *     eg_embed_conv_fwd's bit for bit at every side.
 * eg_pyramid_act_fwd: keep [batch * 128], idx and out [batch, 128, side_out, side_out] from y and x, one launch.  With p == 0, out
 *     equals eg_adaptive_max_pool_idx_fwd of eg_embed_act_fwd's out bit for bit, and idx equals that pool's wherever out > 0 (where
 *     out == 0 the pool of the rectified map picks the first zero, this one v's largest negative).
 * eg_pyramid_act_bwd (2 launches, 3 with db3): ds, dz [batch, 128, side, side], required, not aliasing an input or each other; dgamma,
 *     dbeta, db3 [128] may each be NULL (not wanted).  gamma may be NULL (1).  n == 1 is refused (EG_ERR_ARG) with torch's message.
 * eg_pyramid_conv_bwd_data: dx = chain + ds (ds may be NULL).  From side 17 on an implicit GEMM on the f32-input matrix instruction,
 *     weights read transposed with the taps flipped; the chain is eg_conv3x3_bwd_data's (output channel o ascending, within o tap
 *     k = 0 .. 8 reads dz at offset (k / 3 - 1, k % 3 - 1) against w3[o][c][8 - k], one fmaf chain from 0): the result equals
 *     eg_conv3x3_bwd_data followed by eg_embed_res_bwd_input(w1 = NULL) bit for bit.  Up to side 16 it RUNS those two entry points
 *     (their kernel there adds 16 partial chains; one matrix chain would give other bits).
 * eg_pyramid_conv_bwd_weight: dw3[o][c][ky][kx] = sum_{b, y, x} dz[b, o, y, x] x[b, c, y + ky - 1, x + kx - 1] on the matrix
 *     instruction at every side.  Its order of summation is its own, a function of (batch, side) alone (csrc/pyramid_train.hip):
 *     one chain per 32 x 8 pixel tile, tile sums in chains of 256, at most 64 slices added by the front-end's slice sum -- the
 *     workspace does not grow with the pixel count.
 * eg_pyramid_train_workspace_bytes: one workspace for a block's calls on one stream (eg_bn2d_train_fwd at 128 channels included):
 *     chunk sums + at most 64 x 589,824 B of slices; 0 where the shapes are out of range.
 * All: the caller's stream, no allocation, no synchronisation, no atomics; every sum has a fixed order in chains of at most 256
 * terms (bit-identical from run to run), capturable.  EG_ERR_ARG, nothing launched: a NULL required pointer, batch or a side < 1,
 * side_out > side, p outside [0, 1), an output aliasing an input or another output, n == 1 (eg_pyramid_act_bwd).
 * EG_ERR_UNSUPPORTED, nothing launched: a side above 512, batch above 65535 or batch side^2 >= 2^31. */
size_t eg_pyramid_train_workspace_bytes(int batch, int side, int side_out);
int eg_pyramid_conv_fwd(const float* x, int batch, int side, const float* w3, const float* b3, float* z, eg_stream_t stream);
int eg_pyramid_act_fwd(const float* y, const float* x, int batch, int side, int side_out, float p, uint64_t seed, float* keep, int* idx,
                       float* out, eg_stream_t stream);
int eg_pyramid_act_bwd(const float* dout, const float* out, const float* keep, const int* idx, const float* z, const float* save_mean,
                       const float* save_invstd, const float* gamma, int batch, int side, int side_out, void* workspace, float* ds,
                       float* dz, float* dgamma, float* dbeta, float* db3, eg_stream_t stream);
int eg_pyramid_conv_bwd_data(const float* dz, const float* w3, const float* ds, int batch, int side, float* dx, eg_stream_t stream);
int eg_pyramid_conv_bwd_weight(const float* x, const float* dz, int batch, int side, void* workspace, float* dw3, eg_stream_t stream);

/* ---- node-feature packing (the step right before the hot path) -------------------------------------------
 * Reference: the per-sample loops at the tail of create_node_pixels (src/core/models.py:498-537, :590-636,
 * :707-756): map[i].permute(1, 2, 0).reshape(-1, 128) of every level, concatenated per frame.
 * level_maps: HOST array of n_levels (<= 16) DEVICE pointers to NCHW maps [batch, 128, side_l, side_l];
 * nodes: [batch * n_rows, 128]; level l lands at rows row_offset + sum_{k<l} side_k^2 of every frame, row-major
 * (h, w).  Rows outside the levels (connection / coordinate rows) are not touched.
 * eg_unpack_levels is the reverse copy (the gradient of the packing w.r.t. the maps).
 * 16 bytes per lane: nodes, every bias, and a level map / feature with side_l^2 % 4 == 0 must be 16-byte aligned
 * (EG_ERR_ARG otherwise, before any launch); other levels go element by element and need 4 bytes. */
int eg_pack_levels(const float* const* level_maps, const int* level_side, int n_levels, int batch, int64_t n_rows,
                   int64_t row_offset, float* nodes, eg_stream_t stream);
int eg_unpack_levels(const float* nodes, float* const* level_maps, const int* level_side, int n_levels, int batch,
                     int64_t n_rows, int64_t row_offset, eg_stream_t stream);
/* The UNet variant's `F.relu(self.linears[i](features[i]))` (Conv2d(C_l, 128, kernel_size=1) + ReLU per level,
 * src/core/models.py:707-710) fused into the packing: level_feats[l] [batch, level_channels[l], side_l, side_l] (NCHW),
 * level_weights[l] [128, level_channels[l]] (the Conv2d weight), level_biases[l] [128] (array or entries may be NULL);
 * nodes as eg_pack_levels.  The 128-channel NCHW maps are never formed. */
int eg_conv1x1_relu_pack_levels(const float* const* level_feats, const float* const* level_weights,
                                const float* const* level_biases, const int* level_channels, const int* level_side,
                                int n_levels, int batch, int64_t n_rows, int64_t row_offset, float* nodes, eg_stream_t stream);
/* The backward of eg_conv1x1_relu_pack_levels (pack_train.hip): no atomics, a fixed order of summation, two launches on the
 * caller's stream (products, then the sum over slices), no allocation, no synchronisation, no host read.
 *   dz[b, pos, o] = d_nodes[row, o] where nodes[row, o] > 0, else 0 -- nodes is the FORWARD'S OUTPUT (relu(s) > 0 <=> s > 0, and a
 *   pre-activation of exactly 0 gets gradient 0, as in torch): the product is not recomputed and the mask is the forward's own bits.
 *   d_feats[l] [batch, c_l, side_l, side_l] = sum_o W[o, c] dz;  d_weights[l] [128, c_l] = sum_{b, pos} dz f;  d_biases[l] [128] =
 *   sum_{b, pos} dz.  Each of the three arrays, and each entry, may be NULL: not wanted.  A level that wants nothing launches no
 *   work; a call that wants nothing launches nothing.  level_feats[l] is read where d_weights[l] is wanted, level_weights[l] where
 *   d_feats[l] is; workspace (eg_conv1x1_relu_pack_bwd_workspace_bytes) where a d_weights[l] or d_biases[l] is.
 * The plan: a level's batch * ceil(side^2 / 64) tiles of 64 positions, numbered frame-major, are cut into slices of
 *   tiles_per_slice = ceil(tiles / cap(c_l)) consecutive tiles, cap(c) = clamp(4096 / c, 16, 1024); slices = ceil(tiles /
 *   tiles_per_slice), the last one may be short.  One workgroup per (level, slice, pass of 32 channels) sums its tiles in ascending
 *   order, positions ascending; the slices are summed in 16 runs of ceil(slices / 16) consecutive slices, each ascending, then the
 *   16 runs ascending.  The plan depends on (sides, channels, batch) alone, never on the device or the stream: the same inputs
 *   give the same bits.  eg_conv1x1_relu_pack_bwd_plan is that arithmetic on the host (no device call), the one the launcher uses.
 * Workspace: the sum over the levels of min(cap(c_l), tiles_l) * 128 * (c_l + 1) floats -- bounded whatever the batch: at most
 *   2.62 MB per level up to 256 channels, 8 KiB * (c_l + 1) above; 19.9 MB for channels 512 .. 4 on sides 2 .. 128 and 224.
 *   0 where the shapes are out of range (what eg_conv1x1_relu_pack_bwd refuses).
 * EG_ERR_ARG before any launch, nothing written: as the forward (batch * n_rows >= 2^31, more than 16 levels, levels that do not
 *   fit n_rows), and 16-byte operands elsewhere: d_nodes, nodes, and every level_feats[l] / d_feats[l] with side_l^2 % 4 == 0. */
size_t eg_conv1x1_relu_pack_bwd_workspace_bytes(const int* level_channels, const int* level_side, int n_levels, int batch);
int eg_conv1x1_relu_pack_bwd_plan(const int* level_channels, const int* level_side, int n_levels, int batch, int* level_slices,
                                  int* level_tiles_per_slice);
int eg_conv1x1_relu_pack_bwd(const float* d_nodes, const float* nodes, const float* const* level_feats,
                             const float* const* level_weights, const int* level_channels, const int* level_side, int n_levels,
                             int batch, int64_t n_rows, int64_t row_offset, void* workspace, float* const* d_feats,
                             float* const* d_weights, float* const* d_biases, eg_stream_t stream);
/* The no-GNN baselines (src/core/models.py:759-838: create_node_pixels, h[node_type == 0], the 4 heads) behind the decoder in ONE
 * launch (tail_heads.hip): eg_classifier_fwd(eg_conv1x1_relu_pack_levels(...)) without the node-major rows in between, bit for bit
 * -- the tail keeps k_conv1x1_relu_pack's order of summation, the heads are k_classifier's body.  The level arguments as
 * eg_conv1x1_relu_pack_levels, the head arguments as eg_classifier_fwd (eval-mode BatchNorm folded into s* / t*).
 * logits [batch * sum_l side_l^2, 4]: row b * sum + sum_{k<l} side_k^2 + pos is position pos of level l of frame b.  The rows the
 * node-type filter drops (connection rows in front of the levels, coordinate rows behind them) are never computed: no row_lo.
 * No allocation, no synchronisation, no atomics; capturable.  EG_ERR_ARG before any launch: NULL pointers, n_levels outside 1..16,
 * batch < 1, a side or channel count < 1, batch * sum_l side_l^2 >= 2^31, and logits, a bias or a level map with side_l^2 % 4 == 0
 * that is not 16-byte aligned. */
int eg_conv1x1_relu_heads_fwd(const float* const* level_feats, const float* const* level_weights,
                              const float* const* level_biases, const int* level_channels, const int* level_side, int n_levels,
                              int batch, const float* w1, const float* s1, const float* t1, const float* w2, const float* s2,
                              const float* t2, const float* w3, const float* b3, int sigmoid, float* logits, eg_stream_t stream);

/* ---- connection-node features: fixed-order column means over rows of the node array, in place (conn_rows.hip) --------------
 * The reference gives every connection node (the first n_conn = naux + 1 rows of a frame, use_connection_nodes) the mean of a
 * level's map (src/core/models.py:524-533, :737-752).  The values averaged are that level's packed node rows, so:
 *   eg_conn_rows_fwd, for every frame b and connection row j < n_conn:
 *     nodes[b * n_rows + j, c] = (sum_{i < src_rows[j]} nodes[b * n_rows + src_base[j] + i, c]) / (float)src_rows[j]
 *   The level table (src_base[j], src_rows[j]) is free (HOST arrays of n_conn <= 16 entries): two rows may name the same source
 *   -- it is summed once and stored to both, equal bits -- and sources that differ must be disjoint.  Rows >= n_conn are only
 *   read; every row the call does not own keeps its bits.
 * The order of summation is a function of a source's row count alone (eg_conn_rows_plan, host arithmetic, the one the launcher
 *   uses): rows_per_chunk = max(128, ceil(rows / 512)), chunks = ceil(rows / rows_per_chunk) <= 512, the last chunk may be short
 *   (50,176 rows: 392 chunks of 128).  One workgroup sums a chunk: row lane h = 0 .. 7 adds the chunk's rows h, h + 8, h + 16, ..
 *   ascending, starting from 0; the 8 lane sums are added ascending.  A source of one chunk is divided and stored by that
 *   workgroup.  Otherwise the chunk sums go to the workspace and a SECOND LAUNCH adds them ascending and divides.  Longest chain
 *   of additions a value goes through: d(rows) = (ceil(min(rows, rows_per_chunk) / 8) - 1) + 7 + (chunks - 1); one division
 *   behind it.  No atomics, no flags, no fences between workgroups.  The order does not depend on the batch, the grid, the device
 *   or the other sources of the call: frame b's bits at batch B are its bits at batch 1.
 * Workspace: batch * (sum over the DISTINCT sources of more than one chunk of chunks) * 512 bytes
 *   (eg_conn_rows_workspace_bytes; 0 where the table is one eg_conn_rows_fwd refuses, and where no source has two chunks).
 *   It may be NULL where that is 0.
 *   eg_conn_rows_bwd, in place on d_nodes, for every distinct source range:
 *     d_nodes[b, base + i, c] += t,  t = sum_{j: source j is that range, j ascending} d_nodes[b, j, c] * inv_j
 *   with inv_j = 1.0f / (float)src_rows[j] taken in fp32 ON THE HOST; the first product starts t, each further term is a rounded
 *   multiply, then a rounded add (never fused); the row then takes one rounded add.  One launch.  Rows in no source range, and the
 *   connection rows of d_nodes themselves, keep their bits.
 * Both: one or two launches on the caller's stream, no allocation, no synchronisation, no host read; capturable.  16-byte accesses,
 *   a 512-B row per half-wave; row indices are 64-bit.
 * Before any launch, EG_ERR_ARG: NULL pointers (the workspace where it is needed), n_conn / batch / n_rows < 1, src_rows < 1, a
 *   source range that touches rows < n_conn or ends past n_rows, two sources that overlap without being equal, a node pointer
 *   (or workspace) that is not 16-byte aligned; EG_ERR_UNSUPPORTED: n_conn > 16, batch * n_rows >= 2^31. */
int eg_conn_rows_plan(int64_t rows, int* chunks, int* rows_per_chunk);
size_t eg_conn_rows_workspace_bytes(const int64_t* src_base, const int64_t* src_rows, int n_conn, int batch, int64_t n_rows);
int eg_conn_rows_fwd(float* nodes, int batch, int64_t n_rows, int n_conn, const int64_t* src_base, const int64_t* src_rows,
                     void* workspace, eg_stream_t stream);
int eg_conn_rows_bwd(float* d_nodes, int batch, int64_t n_rows, int n_conn, const int64_t* src_base, const int64_t* src_rows,
                     eg_stream_t stream);

/* ---- average-pool pyramid of the frame embedding: the head of create_node_pixels (src/core/models.py:511-521) -------------
 * eg_avg_pool_pyramid_fwd: level_maps[l] [planes, side_l, side_l] = F.adaptive_avg_pool2d(x [planes, frame, frame], side_l)
 *   for every level in ONE launch (planes = batch * channels; level_side strictly ascending, coarse to fine, as the node rows are
 *   laid out; window (i, j) = rows [floor(i F / p), ceil((i + 1) F / p)) x the same columns).
 * eg_avg_pool_pyramid_bwd: dx [planes, frame, frame] = frame_grad (nullable: the gradient that reaches the frame as the finest
 *   level of the node array) + the pooling's gradient, sum over levels and over the windows containing a pixel of
 *   level_grads[l][window] / area(window) (level_grads[l] NULL: none) -- a gather, no atomics: bit-reproducible (torch's
 *   atomic_adaptive_average_gradinput is not).  Frames up to 512 x 512. */
int eg_avg_pool_pyramid_fwd(const float* x, int64_t planes, int frame, const int* level_side, int n_levels, float* const* level_maps,
                            eg_stream_t stream);
int eg_avg_pool_pyramid_bwd(const float* const* level_grads, const float* frame_grad, int64_t planes, int frame, const int* level_side,
                            int n_levels, float* dx, eg_stream_t stream);


#ifdef __cplusplus
}
#endif
#endif /* ECHOGLAD_HIP_H */
