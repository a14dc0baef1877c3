/*
 * pemp.h — C-ABI of libpemp.so, the MI355X (gfx950) kernels of the keypoint-graph hot path of
 * nibox/Pose-Estimation-with-Message-Passing-Networks.
 *
 * Every function takes caller-owned DEVICE pointers (except where marked host), plain sizes and
 * a hipStream_t passed as void*. Work is stream-ordered; nothing synchronises the host. The
 * library owns no returned memory: outputs go to caller-allocated buffers, scratch goes to a
 * caller-allocated workspace sized by the matching *_workspace_size() query.
 * Return value: 0 (PEMP_OK) or a negative PEMP_ERR_*; pemp_last_error() gives a message
 * (thread-local).
 *
 * Reference interfaces each entry point replaces (paths relative to the reference repo):
 *   pemp_detect          ConstructGraph.py:1161-1209 joint_det_from_scoremap + cat_unique,
 *                        Utils/Utils.py:15-20 non_maximum_suppression
 *   pemp_pack_nodes      ConstructGraph.py:100-103,206-231 (node features, tags, batching)
 *   pemp_graph_offsets   ConstructGraph.py:222-223 (per-image node/edge offsets, on the device)
 *   pemp_fully_graph_build  the four above fused for GRAPH_TYPE fully (one launch)
 *   pemp_fully_graph     ConstructGraph.py:376-381 fully_connected_mpn_graph (+ batch offsets :222-223)
 *   pemp_knn_graph_*     ConstructGraph.py:363-368 knn_mpn_graph (torch_cluster knn_graph k=50,
 *                        PyG to_undirected, remove_self_loops)
 *   pemp_score_graph     ConstructGraph.py:405-422 score_based_graph (k = 75 roots)
 *   pemp_edge_features   ConstructGraph.py:289-359 (edge_attr)
 *   pemp_gather_projected  PoseEstimation.py:426-452 feature projection, sampled at the detections only
 *   pemp_gather_projected_conv  the same with feature_gather (PoseEstimation.py:64-66, 341) at the taps only
 *   pemp_pose_*          Utils.py:499-514,672-743,1445-1455 pose grouping (pred_to_ann prefix, pred_to_person,
 *                        GAEC of correlation_clustering_utils.py:187-245, graph_cluster_to_persons)
 *   pemp_label_*         ConstructGraph.py:627-694,769-942,1096-1158 training labels of EDGE_LABEL_METHOD 4 / 6
 *                        (_construct_edge_labels_4 / _6, match_cc, create_loss_mask)
 *   pemp_mpn_forward     Models/MessagePassingNetwork/NodeClassificationMPNSimple.py:62-97 with
 *                        layers.py:32-86 (MPLayer) / :157-274 (TypeAwareMPNLayer)
 *   pemp_seg_*           the graph operators of the same layers in training: torch_scatter 2.0.4 scatter /
 *                        scatter_softmax per (target, source type) (layers.py:226-251, PyG's aggregate for MPLayer)
 *                        and the backward of the x[i] / x[j] gathers (layers.py:66-67, 210-211)
 */
#ifndef PEMP_H_
#define PEMP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PEMP_ABI_VERSION 24

enum {
  PEMP_OK = 0,
  PEMP_ERR_INVALID_ARG = -1,
  PEMP_ERR_HIP = -2,
  PEMP_ERR_WORKSPACE = -3,
  PEMP_ERR_UNSUPPORTED = -4,
};

int pemp_abi_version(void);
const char* pemp_last_error(void);
/* 0 if the current HIP device is a gfx950 (MI355X); PEMP_ERR_UNSUPPORTED otherwise. */
int pemp_device_check(void);

/* ------------------------------------------------------------------------------------------
 * Detection: NMS maxima (MaxPool2d(k,1,k//2) == s, -inf padding), s *= maxima (* mask),
 * per-type top-k (ties: lower flat index first) + threshold set, cat_unique ordering:
 *   [top-k dets of type 0..J-1, each sorted by (y,x), value != 0]
 *   ++ [dets with s >= threshold not already listed, type-major then (y,x)].
 * use_threshold = 0 restates the DETECT_THRESHOLD > 1.5 branch (top-20, +1e-10).
 * Writes det_xyt[b][i] = (x, y, type) int64 and det_scores[b][i] for i < min(n, cap), and
 * n_det[b] = n (the true count, which may exceed cap: re-run with stages = PEMP_DETECT_SELECT
 * and a larger cap; the NMS stage's workspace is reused).
 * n_det_host (optional): host memory from pemp_host_alloc. Each n is stored into it by the device
 * when the selection stage starts writing the detections: the caller sets it to -1, launches, and
 * reads it while the stream keeps running (the one count read-back of ConstructGraph.py's
 * nonzero calls, without a copy or an event wait).
 * ---------------------------------------------------------------------------------------- */
enum { PEMP_DETECT_NMS = 1, PEMP_DETECT_SELECT = 2, PEMP_DETECT_ALL = 3 };
size_t pemp_detect_workspace_size(int B, int J, int H, int W, int topk);
int pemp_detect(const float* scoremaps /*[B,J,H,W]*/, const float* masks /*[B,H,W] or NULL*/,
                int B, int J, int H, int W, int pool_kernel, float threshold, int use_threshold,
                int topk, int stages, void* workspace, size_t workspace_bytes,
                int64_t* det_xyt /*[B,cap,3]*/, float* det_scores /*[B,cap]*/,
                int32_t* n_det /*[B]*/, int cap, int32_t* n_det_host /*[B] or NULL*/, void* stream);
/* The test-time front-end evaluated inside the detection instead of materialising [B,J,H,W] maps
 * (PoseEstimation.py:329-452 _get_multi_stage_outputs with flip + project2image,
 * multi_scales_testing.py:144-195 aggregate_results_mpn, PoseEstimation.py:227):
 *   s[b,j,Y,X] = (sum_s avg_s[b,j,Y,X]) / divisor,
 *   avg_s = flip_maps[s] ? (up(maps[s])[b,j] + up(flip(flip_maps[s]))[b,flip_index[j]]) / 2
 *                        : up(maps[s])[b,j],
 * up = bilinear to H x W, align_corners = False (torch's source-index rule), each product and sum rounded
 * in fp32 in the order t0 = a lx0 + b lx1, t1 = c lx0 + d lx1, v = t0 ly0 + t1 ly1; flip mirrors the
 * columns of the low-resolution map. maps[s] / flip_maps[s]: the network's outputs for scale s as it
 * produced them ([B][channels][h][w]: heatmaps in channels 0..J-1, per-joint tags in J..2J-1; the
 * flipped pass NOT un-flipped), flip_maps NULL without flip test. flip_index: device [J] int32 (the
 * FLIP_CONFIG permutation) or NULL for the identity. Scales summed in the caller's order (the reference
 * visits them in descending scale). */
#define PEMP_PROJ_MAXS 4
typedef struct pemp_proj_maps {
  int num_scales;
  int channels;
  const float* maps[PEMP_PROJ_MAXS];
  const float* flip_maps[PEMP_PROJ_MAXS];
  int h[PEMP_PROJ_MAXS], w[PEMP_PROJ_MAXS];
  const int32_t* flip_index;
  float divisor;                        /* len(TEST.SCALE_FACTOR) */
} pemp_proj_maps;
/* pemp_detect on the projected maps (same outputs, workspace and stages; the values are sampled on
 * demand in the NMS loads and at the emitted detections). */
int pemp_detect_projected(const pemp_proj_maps* maps, const float* masks, int B, int J, int H, int W,
                          int pool_kernel, float threshold, int use_threshold, int topk, int stages,
                          void* workspace, size_t workspace_bytes, int64_t* det_xyt, float* det_scores,
                          int32_t* n_det, int cap, int32_t* n_det_host, void* stream);
/* Which loader pemp_detect_projected's NMS pass takes for S scales of h[s] x w[s] projected to H x W with this
 * pool_kernel (host arithmetic only, no device call; for tests): 1 = the generic per-pixel loader, 2 = the separable
 * one (every unit's rows span at most 16 staged low-resolution rows of every scale); < 0 on bad arguments.
 * *x2_bands (optional): the bands of 16 rows in which scale 0 takes the separable loader's exact-2x register path
 * (h[0] * 2 == H and no clamped row in the band's halo); 0 with the generic loader. */
int pemp_detect_projected_path(const int* h, const int* w, int S, int H, int W, int pool_kernel, int32_t* x2_bands);
/* The same maps materialised (refine / adjust need the image-size maps; checks): scoremaps [B,J,H,W]
 * (or NULL) and tags (or NULL) as F planes [F][B,J,H,W] (f = 0 forward, 1 flipped pass), F = 2 with a
 * flipped pass. Values identical to the ones the detection samples. */
int pemp_project_maps(const pemp_proj_maps* maps, int B, int J, int H, int W, int tag_scale, float* scoremaps,
                      float* tags, void* stream);

/* HigherHRNet's multi-stage merge (_get_multi_stage_outputs, PoseEstimation.py:338-364 forward pass, :380-412 the
 * flipped pass before its flip, with TEST.WITH_HEATMAPS [True, True] / TEST.WITH_AE [True, False] of the published
 * configs): stage0 [B, C0, h0, w0] (heatmaps in channels 0..J-1, per-joint tags in J..C0-1), stage1 [B, C1, h1, w1]
 * (heatmaps in 0..J-1) -> out [B, C0, h1, w1]: (up(stage0) + stage1) / 2 in channels 0..J-1, up(stage0) in J..C0-1,
 * up = bilinear to h1 x w1 with align_corners=False (the rounding of pemp_project_maps). The merged maps of every
 * scale and pass are what pemp_proj_maps takes (a flipped pass merged in the network's orientation: the projection
 * applies the flip). Device pointers, stream-ordered. */
int pemp_stage_merge(const float* stage0, int C0, int h0, int w0, const float* stage1, int C1, int h1, int w1, int B,
                     int J, float* out, void* stream);
/* joint_tags [N, F] of the detections from the tag channels (J + type) of scale tag_scale: F = 2
 * (up(maps), up(flip(flip_maps)) at channel J + flip_index[type]) with a flipped pass, else F = 1
 * (aggregate_results_mpn's tags_list of that scale, ConstructGraph.py:103). channels >= 2 J. */
int pemp_gather_projected_tags(const pemp_proj_maps* maps, int tag_scale, int J, int H, int W,
                               const int64_t* joint_det, const int64_t* batch_index, int64_t N,
                               float* joint_tags, void* stream);
/* Mapped, coherent host memory (hipHostMalloc) that kernels may store into; NULL on failure. */
void* pemp_host_alloc(size_t bytes);
int pemp_host_free(void* p);

/* ------------------------------------------------------------------------------------------
 * Node packing into the batched layout: x[g] = features[b,:,y,x], joint_det[g], joint_scores[g],
 * batch_index[g] = b, joint_tags[g,:] = tagmaps[b,type,y,x,:] for g = node_off[b] + i.
 * node_off: device [B+1] int64. tagmaps may be NULL (then joint_tags is not written).
 * ---------------------------------------------------------------------------------------- */
int pemp_pack_nodes(const float* features /*[B,C,H,W]*/, int C, const float* tagmaps /*[B,J,H,W,F]*/,
                    int F, int B, int J, int H, int W, const int64_t* det_xyt, const float* det_scores,
                    int cap, const int64_t* node_off, int64_t n_total, float* x /*[N,C]*/,
                    int64_t* joint_det /*[N,3]*/, float* joint_scores /*[N]*/,
                    int64_t* batch_index /*[N]*/, float* joint_tags /*[N,F]*/, void* stream);

/* Batch offsets on the device from pemp_detect's per-image counts (replaces the host cumsum +
 * upload of ConstructGraph.py:222-223): node_off[b] = sum_{b'<b} n_det[b'] ([B+1] int64) and, if
 * fully_edge_off != NULL, fully_edge_off[b] = sum_{b'<b} n_b' (n_b' - 1) ([B+1] int64). */
int pemp_graph_offsets(const int32_t* n_det, int B, int64_t* node_off, int64_t* fully_edge_off, void* stream);

/* The whole fully-connected graph in ONE launch after the count read-back (equivalent to
 * pemp_graph_offsets + pemp_pack_nodes + pemp_fully_graph + pemp_edge_features, same outputs
 * bit for bit): node offsets from n_det, node packing, edge_index of every image, edge_attr
 * (mode = PEMP_EF_*; the AE modes read the tags from tagmaps). B <= 1024.
 * n_total = sum n_det, e_total = sum n (n - 1). tagmaps / joint_tags may be NULL. */
int pemp_fully_graph_build(const int32_t* n_det, int B, const int64_t* det_xyt, const float* det_scores, int cap,
                           const float* features, int C, const float* tagmaps, int F, int J, int H, int W,
                           int64_t n_total, int64_t e_total, float norm_factor, int mode, float* x,
                           int64_t* joint_det, float* joint_scores, int64_t* batch_index, float* joint_tags,
                           int64_t* edge_index, float* edge_attr, int64_t* node_off /*[B+1] or NULL*/,
                           void* stream);

/* Capacity mode of pemp_fully_graph_build, launched BEFORE the host reads the counts back (the
 * reference's nonzero/cat syncs, ConstructGraph.py:1170-1196, become one host read that overlaps
 * this launch): the totals come from n_det on the device; x / joint_* hold n_cap rows, edge_attr
 * e_cap rows and edge_index 2 * e_cap entries written as a contiguous [2, E] array. When the batch
 * exceeds either capacity nothing is written: the caller compares its read-back totals with the
 * capacities and then calls pemp_fully_graph_build with exact sizes. */
/* node_off (when given) holds B + 4 entries here: behind the B + 1 offsets the build writes the batch's
 * (N, E, overflow) at node_off[B + 1 .. B + 3] -- (0, 0, 1) for a batch past a capacity -- which
 * pemp_mpn_forward_fully_cap reads */
int pemp_fully_graph_build_cap(const int32_t* n_det, int B, const int64_t* det_xyt, const float* det_scores, int cap,
                               const float* features, int C, const float* tagmaps, int F, int J, int H, int W,
                               int64_t n_cap, int64_t e_cap, float norm_factor, int mode, float* x,
                               int64_t* joint_det, float* joint_scores, int64_t* batch_index, float* joint_tags,
                               int64_t* edge_index, float* edge_attr, int64_t* node_off /*[B+4] or NULL*/,
                               void* stream);

/* Fully connected graph per image: all (i,j), i != j, sorted by (src,dst), node-offset per image.
 * node_off / edge_off: device [B+1] int64 with edge_off[b+1]-edge_off[b] = n_b (n_b - 1). */
int pemp_fully_graph(const int64_t* node_off, const int64_t* edge_off, int B, int64_t e_total,
                     int64_t* edge_index /*[2,E]*/, void* stream);

/* knn graph per image (k nearest by squared integer distance, ties by node index; k+1 queried
 * with self removed), symmetrised and sorted by (src,dst).
 * node_off_host: HOST [B+1] copy of node_off (grid sizing). */
size_t pemp_knn_workspace_size(const int64_t* node_off_host, int B);
/* The whole graph in one call, no host round trip in the middle (replaces ConstructGraph.py:363-368 +
 * the count read-back): adjacency, per-image counts, their device scan and the emit, back to back.
 * edge_buf: device int64 [2 * e_cap], e_cap >= sum_b min(n_b (n_b - 1), 2 k n_b) (checked); the graph
 * is its leading [2, E] block (sources at 0, destinations at E). e_total_host: mapped host int32
 * (pemp_host_alloc), set to E by the device once the counts are scanned (the emit may still run);
 * the host spins on it (initialise it to -1). Batches whose images all have <= 512 nodes take the
 * fast path (3 launches: selection, LDS transpose, emit with the edge features; node coordinates must
 * fit int32), others the global-memory kernels above + the features kernel. */
int pemp_knn_graph_build(const int64_t* joint_det, const int64_t* node_off, const int64_t* node_off_host,
                         int B, int k, void* workspace, size_t workspace_bytes, int64_t e_cap,
                         int64_t* edge_buf, int32_t* e_total_host, const float* joint_tags, int F,
                         const float* joint_scores, int J, float norm_factor, int mode,
                         float* edge_attr /*[e_cap, A] or NULL: pemp_edge_features' values, leading E rows*/,
                         void* stream);

/* feature_knn graph per image (replaces ConstructGraph.py:370-374 feature_knn_mpn_graph:
 * knn_graph(x, k=50) over the node features -> to_undirected -> remove_self_loops), with the edge
 * features, in one queued call. Same contract as pemp_knn_graph_build (edge_buf, e_cap bound, mapped
 * e_total_host, fast path for images of <= 512 nodes), plus x: device [N, C] fp32 node features
 * (construct_graph's x; 16-byte aligned when C % 4 == 0; C <= 8192). Candidates are ranked by the
 * fp32 sum over c in order of (x_j[c] - x_i[c])^2 as one fma per channel (torch_cluster's CUDA knn
 * as nvcc compiles it), ties by node index; a NaN distance ranks last. The workspace also holds the
 * sum_b n_b^2 distance keys (pemp_feature_knn_workspace_size). */
size_t pemp_feature_knn_workspace_size(const int64_t* node_off_host, int B);
/* Byte offsets, inside a knn build's workspace, of the fast path's bit rows ([N][8] uint64), row starts ([N]
 * int32) and per-image edge counts ([B] int64) (offs[0..2]), for pemp_mpn_forward_knn; feature != 0 for a
 * pemp_feature_knn_graph_build workspace. Returns PEMP_ERR_UNSUPPORTED when the batch would not take the fast
 * path (an image over 512 nodes). */
int pemp_knn_rows_layout(const int64_t* node_off_host, int B, int feature, size_t* offs);
int pemp_feature_knn_graph_build(const float* x, int C, const int64_t* joint_det, const int64_t* node_off,
                                 const int64_t* node_off_host, int B, int k, void* workspace,
                                 size_t workspace_bytes, int64_t e_cap, int64_t* edge_buf,
                                 int32_t* e_total_host, const float* joint_tags, int F,
                                 const float* joint_scores, int J, float norm_factor, int mode,
                                 float* edge_attr, void* stream);

/* Node features from maps projected to the image size on demand (the test front-end's bilinear
 * projection, PoseEstimation.py:426-452, summed over scales and divided, multi_scales_testing.py:182-190
 * / PoseEstimation.py:244): x[n][c] = sum_s bilinear(maps[s][b_n][c], (y_n, x_n); H x W) / divisor,
 * align_corners = False, torch's source-index rule. maps: host array of S (<= 8) device pointers to
 * [B][C][map_h[s]][map_w[s]] fp32. Pairs with pemp_fully_graph_build / pemp_pack_nodes called with
 * features = NULL (they then leave x to this call). */
int pemp_gather_projected(const float* const* maps, const int* map_h, const int* map_w, int S, int C, int H, int W,
                          float divisor, const int64_t* joint_det, const int64_t* batch_index, int64_t N, float* x,
                          void* stream);
/* The same with the model's feature_gather Conv2d applied before the projection (PoseEstimation.py:64-66
 * nn.Conv2d(KP_OUTPUT_DIM, NODE_INPUT_DIM, FEATURE_GATHER_KERNEL, 1, FEATURE_GATHER_PADDING), applied per scale
 * at :341 and projected at :426-452): x[n][co] = sum_s bilinear(conv_s[b_n][co], (y_n, x_n); H x W) / divisor,
 * conv_s = bias + weight * maps[s] (stride 1, zero padding `pad`, output (h + 2 pad - k + 1) x (w + ...)),
 * evaluated only at the 4 taps of each detection. maps: S device pointers to [B][Cin][h_s][w_s] fp32;
 * weight_t: the Conv2d weight transposed to [Cin][k][k][Cout] (device fp32); bias: [Cout] or NULL.
 * Cout <= 512, k <= 7, Cin (k+1)^2 floats <= 64 KB. */
int pemp_gather_projected_conv(const float* const* maps, const int* map_h, const int* map_w, int S, int Cin,
                               const float* weight_t, const float* bias, int Cout, int ksize, int pad, int H, int W,
                               float divisor, const int64_t* joint_det, const int64_t* batch_index, int64_t N,
                               float* x, void* stream);

/* score_based graph per image (ConstructGraph.py:405-422 score_based_graph, k = 75 there): the k
 * highest-scoring nodes are roots (ties: lower node index; torch.topk leaves them unspecified);
 * edge (a, b), a != b, exists iff a or b is a root, sorted by (src, dst) with the per-image node
 * offsets added. Every image needs n >= k (the reference's topk raises otherwise: INVALID_ARG);
 * e_total must be sum over images of k (2 n - k - 1). */
size_t pemp_score_graph_workspace_size(const int64_t* node_off_host, int B, int k);
int pemp_score_graph(const float* joint_scores, const int64_t* node_off, const int64_t* node_off_host, int B, int k,
                     int64_t e_total, void* workspace, size_t workspace_bytes, int64_t* edge_index, void* stream);

/* Edge features. mode: */
enum {
  PEMP_EF_POSITION_CONNECTION = 0, /* [dx, dy, onehot(J)]       (J+2) */
  PEMP_EF_CONNECTION = 1,          /* [onehot(J)]               (J)   */
  PEMP_EF_NOTHING = 2,             /* [0]                       (1)   */
  PEMP_EF_POSITION = 3,            /* [dx, dy]                  (2)   */
  PEMP_EF_POSITION_ANGLE_CONNECTION = 4, /* [dx, dy, theta, onehot(J)] (J+3) */
  /* associative-embedding modes (ConstructGraph.py:337-357); dist = ||tag[dst] - tag[src]||_2 over
   * F = 1 or 2 tag dims, rounded as torch.norm on CPU: sqrt(fma(d1, d1, d0 * d0)) */
  PEMP_EF_POSITION_CONNECTION_AE = 5,    /* {position, connection_type, ae_normed}: [dx, dy, onehot(J), dist] (J+3) */
  PEMP_EF_AE = 6,                        /* {ae}: [dist] (1), F = 1 */
  PEMP_EF_AE_NORMED = 7,                 /* {ae_normed}: [round(dist) * 100 - score[src]] (1), F = 2 */
  PEMP_EF_AE_TRACKING = 8                /* {ae_tracking_1}: [(1.8425 - dist) / 1.8425] (1) */
};
/* joint_tags [N,F] / joint_scores [N] are read by the AE modes only (may be NULL otherwise). */
int pemp_edge_features(const int64_t* joint_det /*[N,3]*/, const float* joint_tags, int F, const float* joint_scores,
                       const int64_t* edge_index /*[2,E]*/, int64_t e_total, int J, float norm_factor, int mode,
                       float* edge_attr, void* stream);

/* ------------------------------------------------------------------------------------------
 * Pose grouping: Utils.py:1445-1455 (pred_to_ann: node threshold + subgraph),
 * Utils.py:499-514 (pred_to_person), correlation_clustering_utils.py:99-151,187-245 (edge matrix
 * symmetrisation, cluster_andres_graph with GAEC), Utils.py:672-743 (graph_cluster_to_persons).
 *
 * 1. pemp_pose_edge_weights (GPU, stream-ordered): edge_index [2,E] int64 must be strictly sorted by
 *    (src, dst) (construct_graph's output is). An edge survives iff use_th == 0 or both
 *    node_scores[end] > th. method 0 (GAEC): w[e] = fl32(pred[e] + pred[reverse(e)]) (0 if the reverse
 *    is absent) for surviving edges with src < dst; method 1 (threshold): w[e] = pred[e] for every
 *    surviving edge; NaN elsewhere. flags[B + 1] (device int32): flags[b] bit 0 = image b has a
 *    surviving src > dst edge with pred != 0 (the reference then averages, else adds), bit 1 = image b
 *    keeps an edge; flags[B] bit 0 = edge_index not sorted.
 * 2. pemp_pose_cluster (HOST arrays, copies of the above): per image, greedy additive edge contraction
 *    (andres graph greedyAdditiveEdgeContraction, weights (w/2 or w) - 0.5 in fp32, then double) or
 *    threshold joins (w > 0.8f); labels[ΣN] = connected-component ids per image in order of each
 *    component's lowest node (scipy connected_components), n_comp[B]. Images run on n_threads threads.
 * 3. pemp_pose_persons (HOST): graph_cluster_to_persons per image from labels: persons[cap][J][3] f64
 *    (x, y, score of the best-scoring joint per (re-)typed joint type; class_probs [ΣN,J] re-types by
 *    first argmax when non-NULL; pose_scores replaces the score when non-NULL), person_count[B],
 *    mutants[B] (a component larger than J). PEMP_ERR_WORKSPACE when more than cap persons. */
int pemp_pose_edge_weights(const int64_t* edge_index, int64_t E, const float* pred, const float* node_scores,
                           float th, int use_th, const int64_t* node_off /*[B+1] device*/, int B, int64_t N,
                           int method, int64_t* row_start /*[N+1] device scratch*/, float* w, int* flags,
                           void* stream);
int pemp_pose_cluster(int B, const int64_t* node_off, const int64_t* edge_index, int64_t E, const float* w,
                      const int* flags, int method, int n_threads, int32_t* labels, int32_t* n_comp);
int pemp_pose_persons(int B, const int64_t* node_off, const int32_t* labels, const int32_t* n_comp,
                      const int64_t* joint_det, const float* scores, const float* pose_scores,
                      const float* class_probs, int J, int allow_single, int64_t cap, double* persons,
                      int32_t* person_count, int32_t* mutants);

/* greedy_person_construction (Utils.py:517-626), HOST, per image over the surviving edges (w from
 * pemp_pose_edge_weights method 1: pred, NaN = dropped; edge_index sorted by src): taken[ΣN] (image-local
 * core node or -1), persons[cap][J][3] f64, person_count[B]. class_probs may be NULL. */
int pemp_pose_greedy(int B, const int64_t* node_off, const int64_t* edge_index, int64_t E, const float* w,
                     const int64_t* joint_det, const float* scores, const float* class_probs, int J, int32_t* taken,
                     int64_t cap, double* persons, int32_t* person_count);

/* Pose finishing, pred_to_ann (Utils.py:1468-1478) per image, keypoints [P][J][3] f64 (x, y, score):
 * pemp_pose_fill_mean (HOST): fill_mean, Utils.py:1468-1470.
 * pemp_pose_refine (GPU, keypoints in device memory, updated in place): refine, Utils.py:1026-1104 -- per
 *   person the float32 mean tag of its detected joints (numpy's summation order), per (person, joint) the
 *   first argmax over the map of s - rint(||tag - mean||) (one pass over the pixels per 8 persons), the
 *   quarter-pixel offset, and the fill of undetected joints with score 0.001. scoremaps [J][H][W] f32,
 *   tag [J][H][W][F] f32 (F = 1 or 2). Workspace: pemp_pose_refine_workspace_size(P, J, H, W, F) bytes.
 * pemp_pose_adjust (GPU, in place): adjust, Utils.py:917-936, det [J][H][W] f32. */
int pemp_pose_fill_mean(double* keypoints, int P, int J);
size_t pemp_pose_refine_workspace_size(int P, int J, int H, int W, int F);
int pemp_pose_refine(const float* scoremaps, const float* tag, int J, int H, int W, int F, double* keypoints, int P,
                     void* workspace, size_t workspace_bytes, void* stream);
int pemp_pose_adjust(const float* det, int J, int H, int W, double* keypoints, int P, void* stream);

/* Batched finishing (finish_batch, the per-image loop of valid.py:101-123 over pred_to_ann's refine / adjust):
 * every image's persons in one keypoints array [P][J][3] f64, person p of image pimg[p].
 * pemp_pose_finish_plan (HOST): from counts[B] persons per image and ref[B] (refine image b or not) fills
 *   pimg[P] and chunks[3 * n] (first person, persons, image; chunks of the refined images only, never across
 *   two images), out2 = {n, persons-per-chunk width}; at most max_chunks (P suffices).
 * pemp_pose_finish_batch (GPU, in place): refine (as pemp_pose_refine) for the persons of the images with
 *   ref[b] != 0, then adjust (adjust != 0) for all, scoremaps [B][J][H][W], tags [B][J][H][W][F] (NULL when
 *   no image is refined); pimg / chunks / ref in device memory. Workspace:
 *   pemp_pose_refine_workspace_size(P, J, H, W, F). Same keypoints as the per-image calls. */
/* pemp_pack_to_host (GPU + copy): the n <= 16 device regions src[i] (bytes[i] bytes each) gathered into the device
 * buffer staging at offsets off[i] (multiples of 16, off[i] + bytes[i] <= total), then one stream-ordered copy of
 * staging[0, total) to host_dst (pinned host memory): the grouping's read-back in one copy instead of one per
 * array. host_dst NULL: the gather only (the caller queues the copy itself). */
int pemp_pack_to_host(int n, const void* const* src, const size_t* bytes, const size_t* off, size_t total,
                      void* staging, void* host_dst, void* stream);
int pemp_pose_finish_plan(int B, const int32_t* counts, const uint8_t* ref, int32_t* pimg, int32_t* chunks,
                          int max_chunks, int32_t* out2);
int pemp_pose_finish_batch(const float* scoremaps, const float* tags, int B, int J, int H, int W, int F,
                           double* keypoints, int P, const int32_t* pimg, const int32_t* chunks, int n_chunks, int pc,
                           const uint8_t* ref, int adjust, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Message-passing network, inference (eval-mode BatchNorm folded into the next Linear by the
 * caller). All hidden widths are 64. Weights are fp32 row-major [out_pad][in_pad], zero padded
 * to multiples of 16 (the caller's folding step; see the Python mirror pemp_amd/mpn/fold.py).
 * ---------------------------------------------------------------------------------------- */
enum { PEMP_AGGR_ATTN = 0, PEMP_AGGR_SUM = 1, PEMP_AGGR_MEAN = 2, PEMP_AGGR_MAX = 3 };

/* Arithmetic of the per-edge GEMMs (edge embedding, edge MLP, message, edge head) and of the node
 * table; the other node-side GEMMs are fp32.
 *   PEMP_PREC_FP32   exact fp32 MFMA (v_mfma_f32_16x16x4_f32)
 *   PEMP_PREC_BF16X3 x·w ~= xh·wh + xl·wh + xh·wl with bf16 hi/lo parts and fp32 accumulation
 *                    (v_mfma_f32_16x16x32_bf16): ~2^-16 relative error per product.
 *   PEMP_PREC_F16X3  x·w ~= xh·wh + 2^-11 (xh·wl + xl·wh) with f16 parts, the low parts scaled by 2^11
 *                    (v_mfma_f32_16x16x32_f16, fp32 accumulation): ~2^-22 relative error per product,
 *                    fp32-level logits; fragments reaching 2^14 are range-scaled by exact powers of two.
 * Both split precisions need the *_bf weight packs, in the matching 16-bit format (the field names
 * keep "bf" for either). */
enum { PEMP_PREC_FP32 = 0, PEMP_PREC_BF16X3 = 1, PEMP_PREC_F16X3 = 2 };

typedef struct pemp_layer {
  const float* w; /* [out_pad][in_pad] */
  const float* b; /* [out_pad] */
  int32_t in_dim, out_dim, relu, pad_;
} pemp_layer;

typedef struct pemp_mlp {
  pemp_layer layer[4];
  int32_t n_layers, pad_;
} pemp_mlp;

typedef struct pemp_mpn_weights {
  pemp_mlp node_emb;   /* NODE_INPUT_DIM -> 64 */
  pemp_mlp edge_emb;   /* EDGE_INPUT_DIM -> 64 */
  const float* pre_w;  /* [128 + T*64][128]: W1[:, x_i], W1[:, x_j], W_t[:, x_i] (t < T) */
  const float* pre_b;  /* [128 + T*64]:      0,          0,          b_t               */
  const float* q0_w;   /* [64][64]  W1[:, e_init] */
  const float* q0_b;   /* [64]      b1            */
  const float* e1_w;   /* [64][64]  W1[:, e_cur]  */
  const float* e2_w;   /* [64][64]  mlp_edge.2    */
  const float* e2_b;   /* [64]                    */
  const float* msg_w;  /* [T][64][64] W_t[:, e'] */
  const float* attn_w; /* [64] attn_net.0.weight (PEMP_AGGR_ATTN); [17][64] when attn_bv is set */
  const float* upd_w;  /* [64][T*64] update_mlp.0.weight, or NULL (x_new = agg) */
  const float* upd_b;  /* [64] */
  pemp_mlp edge_head;  /* 64 -> .. -> 1 */
  pemp_mlp node_head;  /* 64 -> .. -> 1 */
  pemp_mlp class_head; /* 64 -> .. -> J */
  float attn_b;
  int32_t pad_;
  /* split-precision weight packs (16-bit patterns: bf16 hi / lo for PEMP_PREC_BF16X3, f16 hi / f16 lo
   * scaled by 2^11 for PEMP_PREC_F16X3): per matrix [hi | lo][out][64] with the input
   * columns in MFMA slot order: slot 32 kb + 8 g + j holds input 32 kb + 16 (j >> 2) + 4 g + (j & 3). */
  const uint16_t* e1_bf;   /* [2][64][64]    */
  const uint16_t* e2_bf;   /* [2][64][64]    */
  const uint16_t* msg_bf;  /* [T][2][64][64] */
  const uint16_t* head_bf; /* edge head layers 1, 2 (published 64->64->32->1): [2][64][64] then [2][32][64], or NULL */
  const uint16_t* emb_bf;  /* edge embedding layers then the e_init block of mlp_edge.0 (q0): per layer
                              [2][out_pad16][in_pad32], concatenated; or NULL (embedding stays fp32) */
  const uint16_t* upd_bf;  /* per type t: U_t = upd_w[:, 64 t : 64 t + 64] as [T][2][64][64], or NULL */
  const uint16_t* pre_bf;  /* node table weights [2][128 + T*64][128] (K = 128, 4 slot blocks), or NULL */
  const float* node_img;   /* node embedding + head weights in the kernels' LDS layout (pemp_mpn_node_image),
                              or NULL: then every forward builds it in its workspace */
  const float* attn_bv;    /* AGGR_SUB node_edge_attn_per_type (layers.py:199-201, 245-246): [17] attn_net.0.bias;
                              messages from source type t use row t of attn_w and attn_bv[t]. NULL: one shared
                              row attn_w[64] with bias attn_b (node_edge_attn) */
  pemp_mlp upd_mlp;        /* UPDATE_TYPE hierarch_mlp / hierarch_cnn (layers.py:89-154) folded into dense
                              layers over agg[n] flattened to [T*64] (ReLU each; widths % 16 == 0, last 64);
                              n_layers = 0 otherwise. Excludes upd_w. */
  /* EDGE_MLP per_type (TypeAwareEdgeUpdate, layers.py:275-303; attention aggregation), or NULL:
   *   e' = ReLU(O1 ReLU(L1[t_dst] x_dst + c1) + O2 ReLU(L2[t_src] x_src + c2) + e2_w ReLU(q0 + e1_w e) + e2_b)
   * with q0_w / q0_b / e1_w = edge_layer (e_init / e_cur columns), e2_w / e2_b = the e-block of out.1 and
   * the A / B rows of pre_w zero. L1, L2: [T][64][128] on [x_init | x_cur]; c1, c2: [T][64]; O1, O2: [64][64]. */
  const float *ept_l1_w, *ept_l1_b, *ept_l2_w, *ept_l2_b, *ept_o1_w, *ept_o2_w;
  const float* edge_img;   /* edge-pass weight image (pemp_mpn_edge_image for the same desc), or NULL: then every
                              forward builds it in its workspace */
  /* The edge embedding composed with the first edge-MLP layer (PEMP_PREC_F16X3 and the published embedding shape
   * A -> 32 -> 64 -> 64 -> 64, ReLU after all but the last layer), or NULL. The last embedding Linear (W4, b4) has no
   * ReLU, so with h3 the third layer's output: Q0 = Wq h3 + bq, Wq = q0_w W4, bq = q0_w b4 + q0_b, and
   * R0 = Wr h3 + br, Wr = (q0_w + e1_w) W4, br = (q0_w + e1_w) b4 + q0_b, formed by the caller in fp64.
   * emb_comp_bf: [2 (Wq, Wr)][2][64][64] f16x3 packs (as e1_bf); emb_comp_b: [2][64] (bq, br). */
  const uint16_t* emb_comp_bf;
  const float* emb_comp_b;
} pemp_mpn_weights;

typedef struct pemp_mpn_desc {
  int32_t num_types;      /* T: aggregation/message types (NUM_JOINTS, 6, 9) or 1 (MPLayer) */
  int32_t num_joints;     /* J: class-head width */
  int32_t steps;          /* STEPS */
  int32_t aux_loss_steps; /* heads recorded at iterations it >= steps - aux - 1 */
  int32_t aggr;           /* PEMP_AGGR_* */
  int32_t hidden;         /* must be 64 */
  int32_t edge_attr_dim;  /* EDGE_INPUT_DIM */
  int32_t node_in_dim;    /* NODE_INPUT_DIM */
  int32_t precision;      /* PEMP_PREC_* */
  int32_t types_stride;   /* element stride of node_types (e.g. 3 for joint_det[:, 2]); 0 or 1 = dense */
  int32_t flags;          /* PEMP_MPN_PREPARED: pemp_mpn_prepare already ran on this workspace and stream */
} pemp_mpn_desc;

#define PEMP_MPN_PREPARED 1
/* The edge embedding and the first pass always as two launches. Without it the published composed f16x3 attention
 * model (steps >= 2, first pass not recorded, prebuilt edge_img) runs them as one; the logits are the same bits
 * either way. For A/B runs and tests. */
#define PEMP_MPN_TWO_LAUNCH_FIRST 4
/* While the library profiler (pemp_prof_enable) records, a forward keeps the two launches and their labels
 * (edge_embed, edge_step); with this flag it runs the fused pass there too (label edge_first). */
#define PEMP_MPN_FUSED_FIRST_PROFILED 8
/* The prelude of a fully-graph forward (edge order, node embedding, wave ranges, first node table) as four launches
 * of their own. Without it the closed-form order and the fused node embedding share one launch and the ranges and
 * the first node table a second one (a forward the library profiler records keeps the four and their labels); the
 * logits are the same bits either way. For A/B runs and tests. */
#define PEMP_MPN_SEPARATE_PRELUDE 16

size_t pemp_mpn_workspace_size(const pemp_mpn_desc* desc, int64_t N, int64_t E);
/* LDS bytes of one workgroup of the fused first pass (one workgroup per CU: at most 160 KiB) */
size_t pemp_mpn_fused_first_lds_bytes(void);
/* The prelude's grids for N nodes and E edges in B images of at most nmax nodes, T types, edge_grid workgroups per
 * edge pass and a device of cus compute units (host arithmetic only). out8: blocks per image of the edge order in a
 * launch of its own, and in the paired launch A (cut down to the CUs the node embedding leaves: a CU holds one block
 * of launch A at a time); blocks of the node embedding; the block at which the embedding starts in launch A
 * (out8[1] x B); range-table blocks and all blocks of the wave ranges (0 without edges); blocks of the first node
 * table; the block at which the table starts in the paired launch B. Launch A has out8[3] + out8[2] blocks,
 * launch B out8[7] + out8[6]. */
int pemp_mpn_prelude_grids(int64_t N, int64_t E, int B, int T, int nmax, int edge_grid, int cus, int32_t* out8);
/* x [N,node_in_dim], edge_attr [E,edge_attr_dim], edge_index [2,E] (row 0 source j, row 1
 * target i), node_types [N] with element stride desc->types_stride (already mapped by
 * sum_node_types; values < T).
 * Outputs (n_rec = min(aux+1, steps) recorded iterations, NodeClassificationMPNSimple.py:81-94):
 *   edge_logits [n_rec][E]; node_logits [n_rec+1][N] and class_logits [n_rec+1][N][J], whose
 *   last slot is the head evaluation after the loop (:93-94). */
int pemp_mpn_forward(const pemp_mpn_desc* desc, const pemp_mpn_weights* weights, const float* x,
                     const float* edge_attr, const int64_t* edge_index, const int64_t* node_types,
                     int64_t N, int64_t E, float* edge_logits, float* node_logits, float* class_logits,
                     void* workspace, size_t workspace_bytes, void* stream);

/* pemp_mpn_forward for a batch whose edge_index is the fully-connected graph of
 * pemp_fully_graph_build (ConstructGraph.py:376-381) with per-image node offsets node_off (device,
 * [B+1], as written by the build) / node_off_host: the type-major edge order is produced in closed
 * form by one kernel instead of the sorting prepare; results are identical. E must equal
 * sum n_b (n_b - 1) (checked); images above 2048 nodes fall back to the sorting prepare. */
int pemp_mpn_forward_fully(const pemp_mpn_desc* desc, const pemp_mpn_weights* weights, const float* x,
                           const float* edge_attr, const int64_t* edge_index, const int64_t* node_types,
                           int64_t N, int64_t E, const int64_t* node_off, const int64_t* node_off_host, int B,
                           float* edge_logits, float* node_logits, float* class_logits,
                           void* workspace, size_t workspace_bytes, void* stream);

/* Capacity mode of pemp_mpn_forward_fully: queued right behind pemp_fully_graph_build_cap, before the host has the
 * detection counts (replaces the host read-back at ConstructGraph.py:1174,1178 ahead of the MPN). x / edge_attr /
 * node_types (= joint_det + 2, stride 3) / node_off are that build's capacity buffers (n_cap rows, e_cap edges;
 * node_off [B + 4], the batch's (N, E, overflow) read at node_off[B + 1 .. B + 3]); n_det is the detection's device
 * count array ([B], det_cap detections per image at most). The batch's N and E stay on the device; the logits are written compactly for those (edge row r at r * E, node / class row r
 * at r * N), inside arrays sized for the capacities. A batch past any capacity (the capacity build then wrote
 * nothing) runs as an empty forward and writes no logits: the caller, which reads the counts back anyway, re-runs
 * the exact path. PEMP_ERR_UNSUPPORTED for models whose node MLPs are not fused (node embedding, heads) or
 * det_cap above the closed-form image limit (2048). Results equal pemp_mpn_forward_fully's. */
int pemp_mpn_forward_fully_cap(const pemp_mpn_desc* desc, const pemp_mpn_weights* weights, const float* x,
                               const float* edge_attr, const int64_t* node_types, int64_t n_cap, int64_t e_cap,
                               const int32_t* n_det, int det_cap, const int64_t* node_off, int B,
                               float* edge_logits, float* node_logits, float* class_logits,
                               void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * One batch of the inference path in one call (no reference counterpart: a serving entry for a repeated batch
 * shape; construct_graph_start's capacity mode, ConstructGraph.py:1161-1209 + 206-231 + 376-381 and
 * NodeClassificationMPNSimple.py:62-97, takes it): pemp_detect (stages ALL, the counts stored into n_det_host) +
 * pemp_fully_graph_build_cap + pemp_mpn_forward_fully_cap (desc == NULL: none), queued on one stream. The arguments that repeat from batch to batch live in a plan that
 * pemp_step_layout completes once; every output lives in ONE caller buffer of plan.bytes bytes at the offsets it
 * computes (off[PEMP_STEP_*], 256-byte aligned):
 *   DET [B, det_cap, 3] i64, DSC [B, det_cap] f32, NDET [B] i32 (pemp_detect's outputs); X [n_cap, C],
 *   JDET [n_cap, 3] i64, JSC [n_cap], BIDX [n_cap] i64, JTAGS [n_cap, F] (F > 0), EIDX [2, e_cap] i64 written as a
 *   contiguous [2, E], EATTR [e_cap, A], NOFF [B + 4] i64 (pemp_fully_graph_build_cap's outputs); LOGITS (desc
 *   only): edge [max(n_rec, 1)][e_cap], then node [n_rec + 1][n_cap] at element elog_n rounded up to 64, then class
 *   [n_rec + 1][n_cap][J] likewise (pemp_mpn_forward_fully_cap's three arrays, rows at r * E / r * N).
 * The caller sets n_det_host[0..B) to -1, calls, and reads the counts as with pemp_detect; a batch past a capacity
 * leaves the build's and the forward's outputs unwritten (the caller re-runs the exact path, as with the capacity
 * calls). Returns PEMP_ERR_UNSUPPORTED when only the forward was refused (pemp_mpn_forward_fully_cap's conditions;
 * the detection and the build are queued). Workspaces: det_workspace >= pemp_detect_workspace_size, mpn_workspace
 * >= pemp_mpn_workspace_size(desc, n_cap, e_cap); both stream-ordered like the
 * outputs. scoremaps: [B, J, H, W] f32, or a pemp_proj_maps* when projected != 0 (pemp_detect_projected). */
enum {
  PEMP_STEP_DET = 0, PEMP_STEP_DSC, PEMP_STEP_NDET, PEMP_STEP_X, PEMP_STEP_JDET, PEMP_STEP_JSC, PEMP_STEP_BIDX,
  PEMP_STEP_JTAGS, PEMP_STEP_EIDX, PEMP_STEP_EATTR, PEMP_STEP_NOFF, PEMP_STEP_LOGITS, PEMP_STEP_NOUT
};
typedef struct pemp_step_plan {
  /* detection */
  int32_t B, J, H, W, pool_kernel, use_threshold, topk, det_cap, projected;
  float threshold;
  void* det_workspace;
  size_t det_workspace_bytes;
  /* capacity graph build */
  int32_t C, F, A, mode;        /* F = 0: no tagmaps; A: edge_attr columns of mode (PEMP_EF_*) */
  float norm_factor;
  int64_t n_cap, e_cap;
  /* forward (desc NULL: none) */
  const pemp_mpn_desc* desc;
  const pemp_mpn_weights* weights;
  void* mpn_workspace;
  size_t mpn_workspace_bytes;
  /* pemp_step_layout's results */
  int32_t n_rec;                /* recorded iterations: edge rows max(n_rec, 1), node / class rows n_rec + 1 */
  int64_t elog_n, nlog_off, clog_off;   /* edge / node / class logits: elements from off[PEMP_STEP_LOGITS] (f32) */
  size_t off[PEMP_STEP_NOUT];
  size_t bytes;
} pemp_step_plan;
/* Fills plan->off / bytes / n_rec / elog_n / nlog_off / clog_off from the other fields (host arithmetic, no device
 * call); returns plan->bytes, 0 for an invalid plan (pemp_last_error says why). */
size_t pemp_step_layout(pemp_step_plan* plan);
int pemp_step_fully_cap(const pemp_step_plan* plan, const void* scoremaps, const float* masks, const float* features,
                        const float* tagmaps, void* out, int32_t* n_det_host, void* stream);

/* Counters of pemp_mpn_forward_fully_cap's HIP graphs since the library loaded (no reference counterpart; for
 * tests and servers): out3[0] captures made, out3[1] graph launches (first launch after a capture included),
 * out3[2] captures refused (the forward then ran directly). Graphs are opt-in (PEMP_GRAPHS=1): a repeating argument
 * set is then launched directly the first time, captured the second, replayed from then on; without it, and under
 * PEMP_NO_GRAPHS, PEMP_DEBUG_SYNC or the library profiler, every call runs directly. */
int pemp_mpn_graph_stats(uint64_t* out3);

/* The CU-reservation policy of the edge passes and the edge embedding (no reference counterpart; pure host
 * arithmetic, no device call): the number of CUs a forward over E edges spreads its one-workgroup-per-CU launches
 * over on a device of num_cus CUs when reserve_request CUs are asked to stay free for another batch in flight
 * (reserve_request < 0: the library's setting, PEMP_RESERVE_CUS or 64). Graphs below 65,536 edges keep every CU;
 * above, at most a quarter of the device is reserved (rounded down to a multiple of 8). */
int pemp_edge_cus_policy(int num_cus, int64_t E, int reserve_request);

/* sizeof of the ABI structs as this library was built (host only; bindings check their mirrors against it):
 * which = 0 pemp_mpn_weights, 1 pemp_mpn_desc, 2 pemp_mlp, 3 pemp_proj_maps, 4 pemp_step_plan, 5 pemp_loss_rec, 6
 * pemp_kp_loss_rec; 0 for any other value. */
size_t pemp_abi_struct_size(int which);

/* pemp_mpn_forward for an edge_index sorted by (src, dst) without duplicates and symmetric (every s -> d has
 * its d -> s: PyG to_undirected's coalesced output, as knn_mpn_graph / feature_knn_mpn_graph / score_based_graph
 * return it, ConstructGraph.py:363-422): the type-major edge order is read off the rows of the list (segment
 * (t, d) = the type-t entries of row d) instead of the sorting prepare's scatter + segment sort; results are
 * identical. N >= 2^24 falls back to the sorting prepare. A list that breaks the contract is reported by
 * pemp_mpn_status (its logits are then undefined, every index stays in range). The caller's knowledge that a
 * list meets the contract is a hint the library does not verify on this call (the Python mirror tags
 * construct_graph's output and drops the tag on a version-counter change; call pemp_mpn_status to check). */
int pemp_mpn_forward_sym(const pemp_mpn_desc* desc, const pemp_mpn_weights* weights, const float* x,
                         const float* edge_attr, const int64_t* edge_index, const int64_t* node_types,
                         int64_t N, int64_t E, float* edge_logits, float* node_logits, float* class_logits,
                         void* workspace, size_t workspace_bytes, void* stream);

/* pemp_mpn_forward for the knn graph of pemp_knn_graph_build / pemp_feature_knn_graph_build's fast path (every
 * image <= 512 nodes), handed over as the bit rows that build emitted the edges from (pemp_knn_rows_layout):
 * knn_rows [N][8] uint64 (bit j of word w of row n: the edge n -> node 64 w + j of n's image), knn_rowstart [N]
 * int32 (the row's first edge inside its image) and ecount [B] int64 (edges per image), all device, from the
 * same build as edge_index. The edge order then comes from popcounts of the rows in one launch instead of the
 * symmetric prepare's three; results are identical to pemp_mpn_forward_sym's. B <= 64, N <= 4096 and
 * node_off_host[B] == N (checked); rows that do not belong to edge_index break the contract (reported by
 * pemp_mpn_status through the edge total, logits undefined, every index in range). */
int pemp_mpn_forward_knn(const pemp_mpn_desc* desc, const pemp_mpn_weights* weights, const float* x,
                         const float* edge_attr, const int64_t* edge_index, const int64_t* node_types,
                         int64_t N, int64_t E, const void* knn_rows, const int32_t* knn_rowstart,
                         const int64_t* node_off, const int64_t* node_off_host, const int64_t* ecount, int B,
                         float* edge_logits, float* node_logits, float* class_logits,
                         void* workspace, size_t workspace_bytes, void* stream);

/* The edge-ordering part of pemp_mpn_forward (type-major counting sort of edge_index by (source type,
 * target)), callable ahead of it: it needs no weights, so a caller can queue it as soon as the graph
 * exists and then call pemp_mpn_forward with desc->flags |= PEMP_MPN_PREPARED on the same workspace
 * and stream. */
int pemp_mpn_prepare(const pemp_mpn_desc* desc, const int64_t* edge_index, const int64_t* node_types, int64_t N,
                     int64_t E, void* workspace, size_t workspace_bytes, void* stream);

/* Where the type-major edge order lies inside a workspace of pemp_mpn_workspace_size(desc, N, E) bytes (host
 * arithmetic, no device call; no reference counterpart: for tests and tools that read the order back). Byte
 * offsets, every array int32: offs[0] seg [num_types N + 1] (segment (t, d) = [seg[t N + d], seg[t N + d + 1]):
 * the edges into d from sources of type t, in edge-id order; seg[num_types N] = the valid edge total), offs[1]
 * wg_start [18] (the edge passes' workgroup split over the types), offs[2] s_src [E], offs[3] s_dst [E], offs[4]
 * s_orig [E] (source, target and edge id of the edge at each sorted position). pemp_mpn_prepare and every
 * pemp_mpn_forward* write them. After a forward with steps >= 1, s_dst carries the edge passes' packed segment
 * positions in its high byte (edge_ranges_kernel writes them): the target is its low 24 bits. */
int pemp_mpn_order_layout(const pemp_mpn_desc* desc, int64_t N, int64_t E, size_t offs[5]);

/* The node embedding / node head / class head weights in the node kernels' LDS layout, built once
 * per weight set (stream-ordered) instead of once per forward: image of
 * pemp_mpn_node_image_floats(weights) floats, then weights->node_img = image. */
/* The edge passes' weight image (per type: the pass's 64x64 blocks in the kernels' LDS row layout, bias and
 * attention rows, the published edge head), built once per weight set and precision for `desc`
 * (precision, aggregation, num_types) into a caller buffer of pemp_mpn_edge_image_floats() floats;
 * pass it as pemp_mpn_weights.edge_img. The edge embedding's LDS image (its layers, Q0's layer and W1_e_cur, in the
 * embedding kernel's layout) follows the passes' image in the same buffer, so the embedding stages its weights
 * with one LDS-DMA round. No reference counterpart (replaces per-pass weight staging). */
size_t pemp_mpn_edge_image_floats(const pemp_mpn_desc* desc, const pemp_mpn_weights* w);
int pemp_mpn_edge_image(const pemp_mpn_desc* desc, const pemp_mpn_weights* w, float* image, size_t floats,
                        void* stream);
size_t pemp_mpn_node_image_floats(const pemp_mpn_weights* weights);
int pemp_mpn_node_image(const pemp_mpn_weights* weights, float* image, size_t floats, void* stream);

/* Synchronises `stream` and reports invalid edge_index / node_types seen by the last
 * pemp_mpn_forward on this workspace (those edges were skipped). Optional validation step. */
int pemp_mpn_status(const pemp_mpn_desc* desc, int64_t N, int64_t E, const void* workspace, void* stream);

/* Opt-in profiler: while enabled, hipEvents are recorded on the launch stream around every kernel
 * whose label contains `filter` ("*" = all, NULL or "" = off). pemp_prof_report synchronises those
 * events and writes "label count total_ms" lines into buf (returns the full length), then resets.
 * Labels: detect_nms, detect_top, detect_emit, pack_nodes, fully_graph, edge_features, score_graph,
 * mpn_prepare (the sorting prepare; the closed forms report under mpn_prepare_fully, mpn_prepare_sym and
 * mpn_prepare_knn, so the filter "mpn_prepare" catches all four), node_embed, edge_embed, node_table, edge_step, edge_step_head, node_update, heads, seg_aggr_fwd,
 * seg_aggr_bwd, seg_rows_sum, edge_mlp_fwd, edge_mlp_bwd, edge_mlp_tree, loss_fwd, loss_reduce, loss_bwd. Model shapes off the published one report their fall-back kernels under labels of
 * their own (the filter is a substring match, so "edge_embed" and "edge_step" still catch them): edge_embed_wide
 * (an embedding layer or edge_attr_dim over 64: weights read from global memory), edge_embed_generic (the LDS
 * embedding for a shape off the fixed A <= 32 -> 32 -> 64 -> 64 -> 64 layout), edge_step_head_generic (a recorded
 * pass with an edge head other than 64 -> 64 -> 32 -> 1); `heads` marks node / class heads wider than 64.
 * "label@R": launch sites that are idempotent (the edge passes) issue their launch R times between
 * one event pair, so the per-launch average excludes the event-record overhead (count += R). */
int pemp_prof_enable(const char* filter);
int pemp_prof_report(char* buf, size_t len);

/* ------------------------------------------------------------------------------------------
 * Training labels, EDGE_LABEL_METHOD 4 and 6 (ConstructGraph.py:627-694 _construct_edge_labels_4, :769-942
 * _construct_edge_labels_6 with its method == 2, :1096-1158 match_cc / create_loss_mask, :145-146).
 *
 * 1. pemp_label_candidates (GPU, stream-ordered): per image the visible ground-truth joints (joints_gt
 *    [B, P, J, 3] f32 (x, y, visible), visible != 0) in (person, joint) order: gt_tab[b][g] = person * J + joint,
 *    hdr[B + b] = G_b. For every (g, n) of the image, n its detection (joint_det [N, 3] int64 (x, y, type),
 *    node_off [B + 1] int64): sim = exp(-d2 / factors[b][person][joint]) with d2 = (clamp(rint(gt_x), 0,
 *    max(H, W)) - det_x)^2 + (likewise y)^2 in f32; the division and the exponential in f32 for f32 factors,
 *    in f64 for f64 factors (factors_f64 != 0), as torch promotes. The pairs with sim >= threshold are stored
 *    in (g, n) order at recs[b * cap + i], hdr[b] = their count. An image with more than cap pairs stores
 *    none and sets hdr[2 B] = 1 (hdr[b] is still the count: call again with cap >= max hdr[b]). hdr: int32
 *    [2 B + 1]; gt_tab: int32 [B, P J]; scratch: pemp_label_candidates_scratch_size(B, P, J) bytes.
 * 2. pemp_label_assign (HOST arrays: copies of hdr, gt_tab, recs; node_off_host [B + 1]): per image the
 *    maximum-weight assignment over the same-type pairs with sim >= matching_radius (nonzero part of the
 *    reference's dense scipy solve), for method 6 a second one over the different-type pairs that fills the
 *    rows the first left unmatched; with use_neighbours the unmatched detections whose only pair with
 *    sim >= inclusion_radius (method 4: same type and >= both radii) belongs to a matched row join it, the
 *    ones with several such pairs are ambiguous. Outputs [N]: node_labels (1 matched), node_persons (-1
 *    unmatched), node_classes (gt joint type; J for unmatched nodes with with_background), label_mask_node
 *    (0 on ambiguous nodes, method 6), class_mask (node_labels * label_mask_node, ones with
 *    with_background), ambiguous (byte). node_classes / class_mask may be NULL for method 4. Pairs are
 *    written in the reference's order, so a detection matched twice keeps its last pair. A ground-truth row
 *    count above the detection count follows the same row rule (the reference is ill-defined there).
 *    Returns PEMP_LABEL_OVERFLOW (and writes nothing) when hdr[2 B] is set.
 * 3. pemp_label_edges (GPU, stream-ordered): edge_index [2, E] int64 of the batch, the images one after the
 *    other. edge_labels[e] = 1 iff both ends are matched to the same person; label_mask[e] = 0 iff an end is
 *    ambiguous, or the edge's image has no edge with label 1. node_persons / ambiguous: device copies of
 *    step 2's outputs. scratch: pemp_label_edges_scratch_size(B) bytes. Deterministic.
 * ---------------------------------------------------------------------------------------- */
#define PEMP_LABEL_OVERFLOW 1
typedef struct pemp_label_cand {
  int32_t g;      /* row: index into the image's gt_tab */
  uint32_t n;     /* bits 0-30: detection index inside the image; bit 31: same joint type */
  double sim;
} pemp_label_cand;
size_t pemp_label_candidates_scratch_size(int B, int P, int J);
int pemp_label_candidates(const float* joints_gt, const void* factors, int factors_f64, int B, int P, int J,
                          const int64_t* joint_det, const int64_t* node_off, int H, int W, double threshold,
                          int64_t cap, pemp_label_cand* recs, int32_t* hdr, int32_t* gt_tab, void* scratch,
                          size_t scratch_bytes, void* stream);
int pemp_label_assign(int B, int P, int J, const int32_t* hdr, const int32_t* gt_tab, const pemp_label_cand* recs,
                      int64_t cap, const int64_t* node_off_host, int method, int use_neighbours, int with_background,
                      double matching_radius, double inclusion_radius, float* node_labels, int64_t* node_persons,
                      int64_t* node_classes, float* label_mask_node, float* class_mask, uint8_t* ambiguous);
size_t pemp_label_edges_scratch_size(int B);
int pemp_label_edges(const int64_t* edge_index, int64_t E, const int64_t* node_off, int B, int64_t N,
                     const int64_t* node_persons, const uint8_t* ambiguous, float* edge_labels, float* label_mask,
                     void* scratch, size_t scratch_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * Training-mode graph operators (mpn/train.py). fp32 rows of 64 floats (pemp_seg_rows_sum: 64 or 128), int32
 * indices, no atomics, every output element written exactly once per call (callers never pre-zero), results
 * bitwise identical from call to call. They consume a segment plan instead of edge_index:
 *   perm_dst [E]      edge ids sorted by (dst, type[src], edge id)
 *   seg_off [N T + 1] offsets into perm_dst; segment n T + t = the edges into node n from sources of type t
 *   perm_src [E], src_off [N + 1]   edge ids sorted by (src, edge id) and their offsets
 * Offsets are clamped into [0, E] and permutation entries outside [0, E) are skipped, never followed.
 *
 * pemp_seg_aggr_fwd: out[seg] over the segment's rows msgs[e], in list order (row groups of four combined in a
 * fixed tree); an empty segment gives zeros for every kind.
 *   PEMP_AGGR_ATTN  alpha_e = exp(s_e - max_seg) / (sum_seg exp(s - max_seg) + 1e-12), out = sum alpha_e msgs[e]
 *                   (torch_scatter scatter_softmax, then scatter add); alpha[e] is stored when alpha != NULL
 *   PEMP_AGGR_SUM / PEMP_AGGR_MEAN  sum, sum / max(count, 1)
 *   PEMP_AGGR_MAX   per feature the maximum; arg[seg][f] (when arg != NULL) = the edge id of the first edge in
 *                   segment order that attains it, -1 for an empty segment
 * pemp_seg_aggr_bwd: grad_msgs[e] (every row once: each edge lies in one segment) and, for ATTN, grad_scores[e]
 * (may be NULL) from grad_out [N T][64]:
 *   ATTN  grad_msgs[e] = alpha_e g, grad_scores[e] = alpha_e (g . msgs[e] - g . out[seg]); exact with the 1e-12
 *         term, the (below 1e-12 relative) gradient through the subtracted maximum is dropped. g . out[seg] is
 *         evaluated as sum_k alpha_k (g . msgs[k]) / sum_k alpha_k over the segment (the same number up to the
 *         1e-12 term, from the products the rows' own terms use, so that a segment's score gradients sum to zero
 *         up to single roundings); `out` is not read and may be NULL
 *   SUM   g;  MEAN  g / max(count, 1);  MAX  g[f] to row arg[seg][f], zero to the segment's other rows
 *   needs msgs and alpha for ATTN and arg for MAX; the others may be NULL.
 * pemp_seg_rows_sum: out[n] = sum of ga[e] over list a of n, then of gb[e] over list b of n (gb may be NULL), each
 * in list order: the backward of the pair gather (x[dst], x[src]) with list a = (perm_dst, seg_off[::T]) and
 * list b = (perm_src, src_off). W = 64 or 128 floats per row.
 * Argument errors (unknown kind, T < 1, W, negative sizes, a required NULL pointer, ATTN without scores) are
 * reported before the first HIP call. N == 0 returns 0 at once; E == 0 returns 0 without a launch, out zero-filled
 * (arg -1).
 *
 * The fused edge update (csrc/train_edge.hip): mlp_edge(cat([x[dst], x[src], ef])), Linear(2 Wn + We -> 64), ReLU,
 * Linear(64 -> 64), ReLU, in the per-node-table form. With W1 = [A | B | C] split by columns (A, B: Wn columns
 * each, C [64][We]) the caller computes P = nf A^T + b1 and Q = nf B^T ([N][64]); then
 *   h = relu(P[dst] + Q[src] + ef C^T),  e_new = relu(h W2^T + b2)          (exact-fp32 MFMA, k-ordered fmaf chains)
 * pemp_edge_mlp_fwd: writes h and e_new [E][64]. ef [E][We], We = 64 or 128; src32 / dst32 [E] int32 node ids
 * (edge_index rows 0 / 1); an id outside [0, N) is never followed and contributes a zero row.
 * pemp_edge_mlp_bwd: from g = dL/de_new [E][64] and the forward's ef, h, e_new: g2 = g [e_new > 0],
 * g1 = (g2 W2) [h > 0] (the gradient of the pre-activation of h: dP and dQ are its pemp_seg_rows_sum over
 * (perm_dst, dst_off) and (perm_src, src_off) at W = 64), g_ef = g1 C [E][We], and the weight gradients
 * dW2 = g2^T h [64][64], dC = g1^T ef [64][We], db2 = sum_e g2 [64]. The weight gradients are summed without
 * atomics in an order fixed by E alone (never by the grid or the device): every chunk of 256 consecutive edges is
 * one fp32 chain in edge order and stores one partial (64 We + 64 64 + 64 floats) into `workspace`
 * (pemp_edge_mlp_workspace_size(E, We) bytes; 0 for E = 0, non-decreasing in E); the partials are then added in a
 * pairwise tree, 32 partials per pass (each pass pads its last group of 32 with zeros). No chain over edges is longer than 256 terms.
 * Every output element is written exactly once; results are bitwise identical from call to call. Argument errors
 * (We, negative sizes, a required NULL pointer, a workspace that is too small) are reported before the first HIP
 * call. pemp_edge_mlp_fwd returns 0 at once for N == 0 or E == 0; pemp_edge_mlp_bwd for E == 0 zero-fills the
 * weight gradients that are not NULL, without a launch. Profiler labels: edge_mlp_fwd, edge_mlp_bwd, edge_mlp_tree.
 * ---------------------------------------------------------------------------------------- */
int pemp_seg_aggr_fwd(int kind, int T, int64_t N, int64_t E, const float* msgs /*[E][64]*/,
                      const float* scores /*[E] or NULL*/, const int32_t* perm_dst, const int32_t* seg_off,
                      float* out /*[N T][64]*/, float* alpha /*[E] or NULL*/, int32_t* arg /*[N T][64] or NULL*/,
                      void* stream);
int pemp_seg_aggr_bwd(int kind, int T, int64_t N, int64_t E, const float* grad_out /*[N T][64]*/, const float* msgs,
                      const float* alpha, const float* out, const int32_t* arg, const int32_t* perm_dst,
                      const int32_t* seg_off, float* grad_msgs /*[E][64]*/, float* grad_scores /*[E] or NULL*/,
                      void* stream);
int pemp_seg_rows_sum(int64_t N, int64_t E, int W, const float* ga /*[E][W]*/, const int32_t* perm_a,
                      const int32_t* off_a /*[N + 1]*/, const float* gb /*[E][W] or NULL*/, const int32_t* perm_b,
                      const int32_t* off_b, float* out /*[N][W]*/, void* stream);
size_t pemp_edge_mlp_workspace_size(int64_t E, int We);
int pemp_edge_mlp_fwd(int64_t N, int64_t E, int We, const float* P /*[N][64]*/, const float* Q /*[N][64]*/,
                      const float* ef /*[E][We]*/, const int32_t* src32, const int32_t* dst32, const float* C /*[64][We]*/,
                      const float* W2 /*[64][64]*/, const float* b2 /*[64]*/, float* h /*out [E][64]*/,
                      float* e_new /*out [E][64]*/, void* stream);
int pemp_edge_mlp_bwd(int64_t N, int64_t E, int We, const float* g /*[E][64]*/, const float* ef, const float* h,
                      const float* e_new, const float* C, const float* W2, float* g1 /*out [E][64]*/,
                      float* g_ef /*out [E][We]*/, float* dC /*out [64][We]*/, float* dW2 /*out [64][64]*/,
                      float* db2 /*out [64]*/, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The MPN training loss (csrc/loss.hip): the node, edge and class terms of ClassMPNLossFactory (Utils/loss.py:785-862)
 * and of the edge / node / class part of ClassMultiLossFactory (:606-621, 668-689), with the graph reduction of
 * train.py:104-112, 140-154 (mask_node_connections per node prediction), over K_e edge predictions [E], K_n node
 * predictions [N] and K_n class predictions [N, J] given as one pointer per list entry:
 *   node  = (1 / K_n) sum_k L_node(pn[k], node_labels, label_mask_node)
 *   edge  = (1 / K_e) sum_k L_edge(pe[k], edge_labels, mask_k); NaN -> 0.0 with zero gradients (:844-845, :680-681)
 *           mask_k = edge_mask[k] when edge_mask[0] != NULL (every entry then set), else
 *           label_mask * (sel_k[src] op sel_k[dst]), sel_k = sigmoid(pn[k]) > node_threshold | node_labels == 1,
 *           op = & (include_bordering 0) or | (1); src = edge_index[0], dst = edge_index[1] (needs K_n >= K_e)
 *   class = (1 / K_n) sum_k mean_n(CE(pc[k][n, :], node_classes[n]) * node_labels[n])   (node_classes NULL: none;
 *           a class outside [0, J) makes the term NaN)
 *   total = node_weight node + edge_weight edge + class_weight class; terms absent from `terms` are 0 and get no
 *           gradient.
 * L of kind PEMP_LOSS_FOCAL (FocalLoss with logits, :865-891): sum(alpha (1 - pt)^gamma BCE mask) / sum(mask), BCE =
 * binary_cross_entropy_with_logits, pt = exp(-BCE); of kind PEMP_LOSS_BCE (BCELossWtihLogits, :893-905): the plain
 * mean over all elements of BCE mask, times pos_weight where the target is 1.
 * Limits: K_e <= 8, K_n <= 9, J <= 32 (PEMP_ERR_UNSUPPORTED beyond). fp32 rows, contiguous; int64 edge_index [2, E]
 * and node_classes [N]. Ids of edge_index outside [0, N) are never followed (that end counts as not selected).
 *
 * pemp_loss_fwd: out [PEMP_LOSS_OUT] floats: out[0..3] = node, edge, class, total; out[4] the class scale
 *   class_weight / (K_n N); out[8 + k] the edge scales edge_weight / (K_e denominator_k) (all 0 under the NaN rule),
 *   out[16 + k] the node scales: what pemp_loss_bwd multiplies dF/dx by. Two launches (labels loss_fwd, loss_reduce):
 *   every block stores fp64 partial sums into a workspace slot of its own, one block adds the slots in a fixed order.
 *   No atomics; bitwise reproducible; the summation order depends on (N, E, K_e, K_n) alone.
 * pemp_loss_bwd: one launch (label loss_bwd): g_pe[k] [E], g_pn[k] [N], g_pc[k] [N, J] = d total / d logits times the
 *   device scalar grad_total[0] (NULL: 1), recomputed from the logits and `out`; host arrays of K_e / K_n / K_n device
 *   pointers, a NULL array or entry is skipped, every element of the others is written once. The node logits get
 *   the node term's gradient only (sel_k is detached).
 * Neither entry synchronises or allocates (both may be captured into a graph). Argument errors are reported before
 * any launch. pemp_loss_workspace_size is host arithmetic: per edge block (one per PEMP_LOSS_CHUNK edges, at most
 * 1024) 2 K_e doubles, per node block (K_n per 256 nodes, at most 64 K_n) 3 doubles, each array 256-byte aligned,
 * plus 256; 0 for arguments outside the limits.
 * ---------------------------------------------------------------------------------------- */
#define PEMP_LOSS_MAXKE 8
#define PEMP_LOSS_MAXKN 9
#define PEMP_LOSS_MAXJ 32
#define PEMP_LOSS_OUT 32
#define PEMP_LOSS_CHUNK 2048
enum { PEMP_LOSS_FOCAL = 0, PEMP_LOSS_BCE = 1 };
enum { PEMP_LOSS_TERM_NODE = 1, PEMP_LOSS_TERM_EDGE = 2, PEMP_LOSS_TERM_CLASS = 4 };
typedef struct pemp_loss_rec {
  int64_t N, E;
  int32_t J, K_e, K_n;
  int32_t edge_kind, node_kind;     /* PEMP_LOSS_FOCAL / PEMP_LOSS_BCE */
  int32_t include_bordering;        /* 0: both ends selected, 1: either (LOSS.INCLUDE_BORDERING_NODES) */
  int32_t terms;                    /* PEMP_LOSS_TERM_* bits */
  int32_t pad_;
  float alpha, gamma;               /* FOCAL_ALPHA, FOCAL_GAMMA (gamma == 2 takes the multiply form) */
  float edge_pos_weight, node_pos_weight;
  float node_threshold;             /* MODEL.MPN.NODE_THRESHOLD */
  float node_weight, edge_weight, class_weight;
  const float* pe[PEMP_LOSS_MAXKE];
  const float* pn[PEMP_LOSS_MAXKN];
  const float* pc[PEMP_LOSS_MAXKN];
  const int64_t* edge_index;
  const float* edge_labels;
  const float* label_mask;
  const float* node_labels;
  const float* label_mask_node;
  const int64_t* node_classes;      /* or NULL: no class term */
  const float* edge_mask[PEMP_LOSS_MAXKE];   /* caller-made mask_k, or all NULL */
} pemp_loss_rec;
size_t pemp_loss_workspace_size(int64_t N, int64_t E, int K_e, int K_n);
int pemp_loss_fwd(const pemp_loss_rec* rec, void* workspace, size_t workspace_bytes, float* out /*[PEMP_LOSS_OUT]*/,
                  void* stream);
int pemp_loss_bwd(const pemp_loss_rec* rec, const float* out, const float* grad_total, float* const* g_pe,
                  float* const* g_pn, float* const* g_pc, void* stream);

/* ------------------------------------------------------------------------------------------
 * The gradient of the node features x with respect to the maps they were read from (csrc/node_grad.hip): the
 * backward of x[n] = features[b_n, :, y_n, x_n] and of x[n] = conv(raw)[b_n, :, y_n, x_n] (stride 1, square kernel
 * k, zero padding pad; pemp_gather_projected_conv with one map of the conv output's size), with
 * (x_n, y_n) = joint_det[n][0..1] and b_n = batch_index[n]. No float atomics; results are bitwise identical from
 * call to call and depend on neither the grid nor the device.
 *
 * pemp_node_grad_pixels: dfeat [B][C][H][W] = per pixel the sum of the rows g[n][:] of the nodes on it, in ascending
 *   n, left to right in fp32 from 0; every other element 0 (one hipMemsetAsync). sorted_keys [N] / perm [N] (int64):
 *   the keys (b H + y) W + x of the nodes, sorted ascending by a stable sort, and the node of every sorted position;
 *   a key outside [0, B H W) marks a node that lands nowhere. One wave per sorted position; the wave of a segment
 *   head is the single writer of its pixel. Profiler label node_grad_pixels.
 * pemp_node_conv_bwd: from g = dL/dx [N][Cout], each of draw [B][Cin][h][w], dW [Cout][Cin][k][k], db [Cout] that is
 *   not NULL:
 *     draw: D = g W2 [N][k k][Cin] (weight_khwc = the weight as [Cout][k][k][Cin]; one fma chain over co per
 *           element), then the per-pixel sum of pemp_node_grad_pixels over the N k k rows of D with sorted_keys /
 *           perm [N k k] keyed by the pixel ((b h + y - pad + dy) w + x - pad + dx; outside the map: any key outside
 *           [0, B h w)), so a pixel's entries are added in ascending (n, dy, dx).
 *     dW, db: the nodes are the reduction dimension, in node order: every chunk of 256 consecutive nodes is one fma
 *           chain per element over the zero-padded input windows read from raw [B][Cin][h][w] and stores one partial
 *           (Cout Cin k k + Cout floats) into `workspace`; the partials are added in a pairwise tree, 32 per pass
 *           (the last group of a pass padded with zeros).
 *   v_mfma_f32_16x16x4_f32 when Cin and Cout are multiples of 16, the same chains with fmaf otherwise. Limits as the
 *   forward's: Cout <= 512, k <= 7 (PEMP_ERR_UNSUPPORTED beyond), 0 <= pad < k, Cin (k + 1)^2 floats within 64 KB,
 *   every node on the conv's output map (one that is not, or whose batch_index is outside [0, B), adds nothing to dW).
 *   Profiler labels node_conv_bwd, node_grad_pixels, node_conv_tree.
 * pemp_node_conv_workspace_size(N, Cin, Cout, k): host arithmetic; D plus the partials of both tree buffers; 0 for
 *   N <= 0 or arguments outside the limits.
 * N == 0: the gradients that are not NULL are zero-filled, without a launch. Argument errors are reported before the
 * first HIP call. Stream-ordered, no host synchronisation, no allocation (both entries may be captured).
 * ---------------------------------------------------------------------------------------- */
int pemp_node_grad_pixels(const float* g /*[N][C]*/, int64_t N, int C, const int64_t* sorted_keys, const int64_t* perm,
                          int B, int H, int W, float* dfeat /*out [B][C][H][W]*/, void* stream);
size_t pemp_node_conv_workspace_size(int64_t N, int Cin, int Cout, int ksize);
int pemp_node_conv_bwd(const float* g /*[N][Cout]*/, const float* raw, const float* weight_khwc,
                       const int64_t* joint_det /*[N][3]*/, const int64_t* batch_index /*[N]*/, int64_t N, int B, int Cin,
                       int h, int w, int Cout, int ksize, int pad, const int64_t* sorted_keys, const int64_t* perm,
                       float* draw, float* dW, float* db, void* workspace, size_t workspace_bytes, void* stream);

/* ------------------------------------------------------------------------------------------
 * The keypoint losses (csrc/kp_loss.hip): the heatmap and associative-embedding terms of ClassMultiLossFactory
 * (Utils/loss.py:641-665; HeatmapLoss :17-27, AELoss :37-98) over S <= 4 stages, fused each way. Per stage s:
 * pred [B, C, H, W] with C >= J, gt [B, J, H, W], mask [B, H, W] (any float values), tag [B, P, J, 2] int32 rows
 * (index, visible) as JointsGenerator writes them (data/utils.py:4-27); all contiguous, fp32 unless said.
 *   heatmap = sum_s [with_heatmap] heatmap_factor_s / (B J H W) sum_{b, j, y, x} (pred[b, j] - gt[b, j])^2 mask[b]
 *             over the first J planes of pred, read in place (image stride C H W)
 *   ae      = sum_s [with_ae] (push_factor_s mean_b push_b + pull_factor_s mean_b pull_b), where the tags of image b
 *             are t = pred[b, J:] flattened (T = (C - J) H W values) and a person p with n_p >= 1 entries of
 *             visible > 0 and index in [0, T) has m_p = mean(t_i), pull_p = mean((t_i - m_p)^2); with P' such persons
 *             pull_b = sum_p pull_p / P'; push_b = 0.5 (sum_{p, q} f(m_p - m_q) - P') / ((P' - 1) P') for P' >= 2 over
 *             all ordered pairs (diagonal included), f(d) = exp(-d^2) (PEMP_KP_AE_EXP) or max(0, 1 - |d|)
 *             (PEMP_KP_AE_MAX); P' = 1: push_b = 0; P' = 0: both 0 and no gradient
 *   total   = heatmap + ae
 * A visible entry whose index lies outside [0, T) is skipped and counted (the reference raises IndexError there).
 * Limits: S <= 4, P <= 32, J <= 32 (PEMP_ERR_UNSUPPORTED beyond); C H W < 2^31 per image.
 *
 * pemp_kp_loss_fwd: out [PEMP_KP_OUT] floats: out[0..2] = heatmap, ae, total; out[3 + 3 s + 0..2] the heatmap, push and
 *   pull parts of stage s (factors applied). Two launches (labels kp_loss_fwd, kp_loss_reduce). Heatmap blocks: a
 *   stage's blocks (one per PEMP_KP_CHUNK elements of an image's J H W heatmap values, at most PEMP_KP_MAXBLOCKS, the
 *   rest strided) found through the prefix table `blk0`; 16-byte loads when H W is a multiple of 4 and pred, gt and
 *   mask are 16-byte aligned, scalar ones otherwise; fp32 inside a thread's 16 elements and through the wave, fp64
 *   from there on; one fp64 partial per block. AE blocks, one per (stage, image), in the same launch: the P J tags
 *   gathered into LDS, everything after the gather in fp64; they leave push_b, pull_b, m_p, n_p, P' and the count of
 *   skipped entries in the workspace. The reduction is one block that adds the partials in a fixed order in fp64 and
 *   writes the skipped-entry count of the call to the int32 at the start of the workspace (the status word: 0 when
 *   every visible index was in range). No atomics on floats; bitwise reproducible; the order depends on the record.
 * pemp_kp_loss_bwd: g_pred[s] [B, C, H, W] (a host array of PEMP_KP_MAXS device pointers; NULL entries are skipped) =
 *   d total / d pred[s] times the device scalar grad_total[0] (NULL: 1), every element written exactly once: launch
 *   one (label kp_loss_bwd) writes 2 (pred - gt) mask heatmap_factor / (B J H W) to the heatmap planes, recomputed
 *   from pred, gt and mask, and zeros to the tag planes; launch two (label kp_loss_bwd_tags, behind it in stream
 *   order, one block per (stage, image) with with_ae) writes the listed tag entries from m_p, n_p, P' of the forward's
 *   workspace. An index listed more than once in an image (two persons on one pixel and joint) gets the sum of its
 *   entries in ascending (person, joint) order, in fp32 from the first, written by the lane of the first entry.
 *   `workspace` is the forward's, unchanged since (a caller that interleaves calls keeps one workspace per call).
 * Neither entry synchronises or allocates. Argument errors are reported before any launch.
 * pemp_kp_loss_workspace_size is host arithmetic over the record's sizes and flags (pointers are not read): 256 bytes
 *   of status, the block partials, and per (stage, image) 2 doubles + 2 int32 + P (double + int32), each array
 *   256-byte aligned; 0 for a record outside the limits.
 * ---------------------------------------------------------------------------------------- */
#define PEMP_KP_MAXS 4
#define PEMP_KP_MAXP 32
#define PEMP_KP_MAXJ 32
#define PEMP_KP_CHUNK 4096
#define PEMP_KP_MAXBLOCKS 2048
#define PEMP_KP_OUT 16
enum { PEMP_KP_AE_EXP = 0, PEMP_KP_AE_MAX = 1 };
typedef struct pemp_kp_stage {
  const float* pred;                /* [B, C, H, W] */
  const float* gt;                  /* [B, J, H, W]; read with with_heatmap */
  const float* mask;                /* [B, H, W]; read with with_heatmap */
  const int32_t* tag;               /* [B, P, J, 2]; read with with_ae */
  int32_t C, H, W;
  int32_t with_heatmap, with_ae;    /* HRNET.LOSS.WITH_HEATMAPS_LOSS[s], TRAIN.WITH_AE_LOSS[s] */
  float heatmap_factor, push_factor, pull_factor;
} pemp_kp_stage;
typedef struct pemp_kp_loss_rec {
  int32_t S, B, J, P;
  int32_t ae_kind;                  /* PEMP_KP_AE_EXP / PEMP_KP_AE_MAX */
  int32_t pad_;
  pemp_kp_stage stage[PEMP_KP_MAXS];
  int32_t blk0[PEMP_KP_MAXS + 2];   /* filled by the library on its copy of the record (callers leave it): [s] the
                                       first of stage s's streaming blocks (counted from 0), [PEMP_KP_MAXS] their
                                       number, [PEMP_KP_MAXS + 1] the grid; the forward's AE blocks come first in
                                       the grid, the streaming blocks behind them */
} pemp_kp_loss_rec;
size_t pemp_kp_loss_workspace_size(const pemp_kp_loss_rec* rec);
int pemp_kp_loss_fwd(const pemp_kp_loss_rec* rec, void* workspace, size_t workspace_bytes, float* out /*[PEMP_KP_OUT]*/,
                     void* stream);
int pemp_kp_loss_bwd(const pemp_kp_loss_rec* rec, const void* workspace, const float* grad_total,
                     float* const* g_pred /*[PEMP_KP_MAXS]*/, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PEMP_H_ */
