"""Cases and plain numpy references for the graph constructor's options that the published configuration leaves
unset: the nine EDGE_FEATURES_TO_USE modes on every writer of edge_attr, HYBRID_K other than 5 and
NORM_NODE_DISTANCE = False (tests/test_graph_options_cpu.py, tests/test_gpu_graph_options.py). No pytest hooks."""
import numpy as np

f32 = np.float32

# EDGE_FEATURES_TO_USE by mode code (include/pemp.h PEMP_EF_*)
FEATURES = [
    ["position", "connection_type"],                # 0  [dx, dy, onehot(J)]
    ["connection_type"],                            # 1  [onehot(J)]
    ["nothing"],                                    # 2  [0]
    ["position"],                                   # 3  [dx, dy]
    ["position", "angle", "connection_type"],       # 4  [dx, dy, theta, onehot(J)]
    ["position", "connection_type", "ae_normed"],   # 5  [dx, dy, onehot(J), dist]
    ["ae"],                                         # 6  [dist], F = 1
    ["ae_normed"],                                  # 7  [rint(dist) 100 - score[src]], F = 2
    ["ae_tracking_1"],                              # 8  [(1.8425 - dist) / 1.8425]
]
MODES = range(len(FEATURES))
TAG_MODES = (5, 6, 7, 8)
THETA_ULP = 2      # the bar of the angle column (tests/test_gpu_graph.py::test_knn_edge_feature_modes)


def mode_of(features):
    return [set(f) for f in FEATURES].index(set(features))


def width(mode, J):
    return (J + 2, J, 1, 2, J + 3, J + 3, 1, 1, 1)[mode]


def tag_dims(mode):
    """F of the matrix cases: 2 where the mode allows it, 1 for ae (the reference's norm over dim 1 of an [E]
    difference fails for F = 2, ConstructGraph.py:338)."""
    return 1 if mode == 6 else 2


def theta_column(mode):
    return 2 if mode == 4 else None


def expected_edge_attr(det, edge_index, J, norm, features, tags=None, scores=None):
    """ConstructGraph.py:305-359 in numpy with every fp32 rounding written out. det [N, 3] int64 (x, y, type),
    edge_index [2, E] int64, tags [N] or [N, F] float32 (F = 1 or 2), scores [N] float32 -> [E, A] float32."""
    det = np.asarray(det, np.int64)
    s, d = np.asarray(edge_index, np.int64)
    E = s.shape[0]
    jx, jy, jt = det[:, 0], det[:, 1], det[:, 2]
    mode = mode_of(features)
    with np.errstate(all="ignore"):
        dx = ((jx[d] - jx[s]).astype(f32) / f32(norm))[:, None]          # :316-317, IEEE fp32 division
        dy = ((jy[d] - jy[s]).astype(f32) / f32(norm))[:, None]
        onehot = np.zeros((E, J), f32)                                   # :305-308
        onehot[np.arange(E), jt[s]] = 1
        onehot[np.arange(E), jt[d]] = 1
        if mode == 0:
            return np.concatenate([dx, dy, onehot], 1)
        if mode == 1:
            return onehot
        if mode == 2:
            return np.zeros((E, 1), f32)
        if mode == 3:
            return np.concatenate([dx, dy], 1)
        if mode == 4:                                                    # :319-321
            ax, ay = (jx[s] - jx[d]).astype(f32), (jy[s] - jy[d]).astype(f32)
            arg = ax * (f32(1) / np.sqrt(ax * ax + ay * ay))             # a_x * rsqrt(a_x^2 + a_y^2), each op fp32
            theta = np.abs(np.arccos(arg.astype(np.float64))).astype(f32)
            theta[np.isnan(theta)] = 0
            return np.concatenate([dx, dy, theta[:, None], onehot], 1)
        t = np.asarray(tags, f32).reshape(det.shape[0], -1)
        d0 = t[d, 0] - t[s, 0]
        if t.shape[1] == 1:
            dist = np.abs(d0)                                            # torch.norm over one element
        else:                                                            # sqrt(fma(d1, d1, fl(d0 d0)))
            assert t.shape[1] == 2
            d1 = (t[d, 1] - t[s, 1]).astype(np.float64)
            dist = np.sqrt(((d0 * d0).astype(np.float64) + d1 * d1).astype(f32))
        dist = dist.astype(f32)[:, None]
        if mode == 5:
            return np.concatenate([dx, dy, onehot, dist], 1)
        if mode == 6:
            return dist
        if mode == 7:                                                    # :341-342
            return np.rint(dist) * f32(100) - np.asarray(scores, f32)[s, None]
        return (f32(1.8425) - dist) / f32(1.8425)                       # :344-350


def same_bits(a, b):
    """Elementwise: the same fp32 bit pattern, or NaN in both."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    return (a.view(np.uint32) == b.view(np.uint32)) | (np.isnan(a) & np.isnan(b))


def ulp_diff(a, b):
    """Largest distance in fp32 units in the last place between two arrays of finite, non-negative values."""
    a, b = np.ascontiguousarray(a, f32), np.ascontiguousarray(b, f32)
    if a.size == 0:
        return 0
    return int(np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64)).max())


def check_edge_attr(got, want, mode, what=""):
    """got == want bit for bit, the angle column within THETA_ULP. Returns the angle column's largest ulp distance."""
    got, want = np.asarray(got, f32), np.asarray(want, f32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    col, worst = theta_column(mode), 0
    if col is not None:
        worst = ulp_diff(got[:, col], want[:, col])
        assert worst <= THETA_ULP, f"{what}: theta differs by {worst} ulp"
        got, want = np.delete(got, col, 1), np.delete(want, col, 1)
    bad = np.argwhere(~same_bits(got, want))
    assert bad.shape[0] == 0, (what, bad[:5].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])
    return worst


# ---- planted node sets ---------------------------------------------------------------------------------------------
PLANTED_J = 17
PLANTED_HW = (304, 4096)      # the smallest maps that hold every planted pixel (y <= 300, x <= 4095)
BIG = 3e19                    # (2 BIG)^2 overflows fp32


def planted_nodes():
    """Two images of 23 and 1 nodes: det [24, 3] (x, y, type), counts, tags for F = 1 and F = 2, scores.
    Image 0 holds: two coincident pixels of different types (dx = dy = 0, theta NaN -> 0); a row (y = 100) and a
    column (x = 100) whose pairs are purely horizontal / vertical at offsets from 1 to 200 both ways, among them 41
    and 47, where the fp32 argument of the acos is 1 - 2^-24; x up to 4095 (for norm = 1); equal tags, tag distances
    of exactly 0.5, 1.5 and 2.5 (half-to-even in ae_normed), a difference whose square overflows fp32 and a NaN tag;
    a negative score and -0.0."""
    det = [(100, 100, 0), (100, 100, 5),                                   # coincident, different types
           (101, 100, 1), (141, 100, 2), (147, 100, 2), (300, 100, 3),     # row y = 100: 1, 41, 47, 200, 6, 40, ...
           (100, 101, 4), (100, 141, 6), (100, 147, 7), (100, 300, 8),     # column x = 100
           (4095, 0, 16), (0, 0, 16), (4095, 300, 9), (0, 300, 10),        # the corners of the planted maps
           (2048, 150, 11), (2047, 151, 12), (777, 13, 13), (778, 290, 14), (3333, 222, 15),
           (10, 250, 0), (250, 10, 1), (1234, 56, 5), (4000, 3, 3)]
    assert len(det) == 23 and len(set(det)) == 23
    det.append((7, 9, 4))                                                  # image 1: one node, no edge
    det = np.array(det, np.int64)
    t1 = np.array([0.0, 0.0, 0.5, 2.0, 2.5, -0.5, 1.0, 4.5, BIG, -BIG, np.nan, 0.25, 3.0, -1.5, 0.125, 7.0,
                   -2.5, 1.5, 0.75, 2.25, -0.25, 5.5, 1e-3, 0.3], f32)
    t2 = np.stack([t1, np.array([0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 2.0, 1.5, 0.0, -BIG, 1.0, np.nan, 4.0, 2.0, -0.5, 0.25,
                                 0.6, -3.0, 1e-4, 9.0, 2.0, -7.5, 0.5, 0.1], f32)], 1)
    # (node 0 -> 7 in F = 2: (4.5, 1.5), 4.74...; 2 -> 3: 1.5; 0 -> 4: 2.5; 3 -> 6: (-1, 2); 0 -> 2: 0.5)
    scores = np.array([0.9, 0.5, -0.0, -0.3, 0.0, 0.11, 0.7, 0.25, 1.0, 0.05, 0.33, 0.6, 0.2, 0.8, 0.15, 0.45,
                       0.35, 0.55, 0.65, 0.75, 0.85, 0.95, 0.125, 0.4], f32)
    return dict(det=det, counts=[23, 1], tags={1: t1.copy(), 2: t2}, scores=scores)


def sweep_nodes():
    """Every purely horizontal and vertical offset from 1 to 200, and coordinates up to 4095 on both axes: node 0 at
    (200, 200), then (200 + k, 200) and (200, 200 + k) for k = 1..200, then four far corners. Edges (directed, both
    ways) between node 0 and every other node, and between the corners. Returns det [405, 3], edge_index [2, 820]."""
    k = np.arange(1, 201)
    xs = np.concatenate([[200], 200 + k, np.full(200, 200), [0, 4095, 0, 4095]])
    ys = np.concatenate([[200], np.full(200, 200), 200 + k, [0, 0, 4095, 4095]])
    det = np.stack([xs, ys, np.arange(xs.shape[0]) % PLANTED_J], 1).astype(np.int64)
    a = np.arange(1, 401)
    c = np.array([(i, j) for i in range(401, 405) for j in range(401, 405) if i != j]).T
    src = np.concatenate([np.zeros(400, np.int64), a, a[:4] * 0, np.arange(401, 405), c[0]])
    dst = np.concatenate([a, np.zeros(400, np.int64), np.arange(401, 405), a[:4] * 0, c[1]])
    return det, np.stack([src, dst]).astype(np.int64)


def fully_pairs(counts):
    """edge_index of the batch's fully graph: per image every ordered pair i != j, sorted by (src, dst)."""
    out, off = [], 0
    for n in counts:
        i, j = np.divmod(np.arange(n * n), n) if n else (np.zeros(0, np.int64),) * 2
        keep = i != j
        out.append(np.stack([i[keep], j[keep]]) + off)
        off += n
    return np.concatenate(out, 1).astype(np.int64)


# ---- detection top-k ---------------------------------------------------------------------------------------------
def nms_numpy(hm, pool, mask=None):
    """Utils.py:15-20 on one image hm [J, H, W]: the value where it equals the maximum of its pool x pool
    neighbourhood (cut at the borders), else value * 0; times the mask [H, W]."""
    J, H, W = hm.shape
    p = pool // 2
    pad = np.full((J, H + 2 * p, W + 2 * p), -np.inf, f32)
    pad[:, p:p + H, p:p + W] = hm
    mx = np.full_like(hm, -np.inf)
    for dy in range(2 * p + 1):
        for dx in range(2 * p + 1):
            mx = np.maximum(mx, pad[:, dy:dy + H, dx:dx + W])
    keep = (mx == hm).astype(f32)
    if mask is not None:
        keep = keep * mask[None]
    return hm * keep


def brute_detect(sm, k, thr):
    """The hybrid top-k + threshold set of one image (ConstructGraph.py:1161-1196 with the threshold set) from the
    NMS-ed, masked scoremaps sm [J, H, W] (no NaN): per type the k best values, ties to the lower flat index, zeros
    dropped, in flat-index order; then every pixel with not (s < thr) and s != 0 that is not listed yet, by
    (type, y, x). det [N, 3] int64 (x, y, type), scores [N] float32."""
    J, H, W = sm.shape
    flat = sm.reshape(J, H * W)
    k = min(k, H * W)
    top = []
    for t in range(J):
        order = np.lexsort((np.arange(H * W), -flat[t]))[:k]           # by value descending, then flat index
        top += [(t, int(i)) for i in sorted(order) if flat[t, i] != 0]
    listed = set(top)
    thr32 = f32(thr)
    rest = [(t, i) for t in range(J) for i in np.flatnonzero(~(flat[t] < thr32) & (flat[t] != 0))
            if (t, i) not in listed]
    both = top + rest
    det = np.array([(i % W, i // W, t) for t, i in both], np.int64).reshape(-1, 3)
    return det, np.array([flat[t, i] for t, i in both], f32)


UNIT = (16, 62)      # rows x columns of a detection unit with POOL_KERNEL_SIZE 3 (csrc/detect.hip: SR, 64 - 2 p)
PALETTE = np.array([0.05, 0.08, 0.1, 0.3, 0.3, 0.7, 0.09, 0.9, 0.1000001, 0.7, 0.02, 0.9], f32)   # around 0.1, ties


def lattice_plane(H, W, live, salt, background=0.0):
    """One plane with `live` isolated positive maxima, one per detection unit (its centre pixel), the units taken in
    a fixed scattered order and the values from PALETTE: equal values in several units, on both sides of 0.1."""
    nb, ns = -(-H // UNIT[0]), -(-W // UNIT[1])
    units = [(by, bx) for by in range(nb) for bx in range(ns)
             if by * UNIT[0] + 8 < H - 1 and bx * UNIT[1] + 31 < W - 1]
    order = np.random.default_rng(1000 + salt).permutation(len(units))[:live]
    plane = np.full((H, W), background, f32)
    for n, u in enumerate(order):
        by, bx = units[u]
        plane[by * UNIT[0] + 8, bx * UNIT[1] + 31] = PALETTE[(5 * n + salt) % PALETTE.shape[0]]
    return plane


def topk_maps(H, W, live, K, with_masks):
    """B = 2, J = 3 planes for the fused selection: (0, 0), (0, 1), (1, 1) with `live` units each; (1, 2) with `live`
    units all below the threshold (listed entries without the threshold bit); (0, 2) a constant negative plane with
    fewer than K non-negative pixels (one positive corner pixel and the three zeros its NMS leaves; none for K = 1):
    its top-k is filled with negatives by flat index; (1, 0) all zero. The masks (one per image) remove two planted
    maxima each."""
    hm = np.zeros((2, 3, H, W), f32)
    hm[0, 0] = lattice_plane(H, W, live, 0)
    hm[0, 1] = lattice_plane(H, W, live, 1)
    hm[1, 1] = lattice_plane(H, W, live, 2)
    hm[1, 2] = np.minimum(lattice_plane(H, W, live, 3), f32(0.09))
    hm[0, 2] = -0.25
    if K > 1:
        hm[0, 2, 0, 0] = 0.4
    masks = None
    if with_masks:
        masks = np.ones((2, H, W), f32)
        for b in range(2):
            ys, xs = np.nonzero(hm[b, 1] > 0)
            masks[b, ys[:2], xs[:2]] = 0
    return hm, masks


# ---- the writers of edge_attr and how construct_graph reaches each (tests/test_gpu_graph_options.py) ---------------
# name: (GRAPH_TYPE, features kind, tagmaps kind, persons of the priming call or None, (seed, persons) of the call,
#        (H, W) or None for the 96 x 104 default, profiler labels the call must show -> launches)
PATHS = {
    "fully_exact": ("fully", "dense", "dense", None, (1, 3), None, {"graph_build": 1}),
    "fully_step": ("fully", "dense", "dense", 3, (2, 2), None, {"graph_build": 1}),
    "fully_step_bound": ("fully", "dense", "dense", 3, (2, 2), None, {"graph_build": 1, "mpn_prepare_fully": 1}),
    "fully_cap": ("fully", "projected", "dense", 3, (2, 2), None, {"graph_build": 1, "gather_projected": 1}),
    "fully_step_overflow": ("fully", "dense", "dense", 3, (4, 6), None, {"graph_build": 2}),
    "knn_fast": ("knn", "dense", "dense", None, (5, 5), None, {"pack_nodes": 1, "knn_build": 1}),
    "knn_large": ("knn", "dense", "dense", None, (51, 40), (192, 192), {"pack_nodes": 1, "knn_build": 1}),
    "feature_knn_fast": ("feature_knn", "dense", "dense", None, (5, 5), None,
                         {"pack_nodes": 1, "fknn_dist": 1, "knn_build": 1}),
    "score_based": ("score_based", "dense", "dense", None, (6, 7), None,
                    {"pack_nodes": 1, "score_graph": 1, "edge_features": 1}),
    "fully_projected_tags": ("fully", "dense", "projected", None, (1, 3), None,
                             {"pack_nodes": 1, "gather_proj_tags": 1, "fully_graph": 1, "edge_features": 1}),
}
BOUND_MODES = (0, 4, 5)      # the modes a bound model takes: EDGE_INPUT_DIM = A
