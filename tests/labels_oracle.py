"""Restatement of the reference's training-label rules for EDGE_LABEL_METHOD 4 and 6 in plain numpy (test helper).

What it restates (``src/graph_constructor/ConstructGraph.py``): ``_construct_edge_labels_4`` (:627-694),
``_construct_edge_labels_6`` with its ``method == 2`` (:769-942), ``match_cc`` (:1096-1134), ``create_loss_mask``
(:1137-1158), the "no positive edge" rule (:145-146) and the batching of :232-249. The assignments are solved densely
by a Hungarian method of this file's own (no scipy), the ground-truth-rows-above-detections case follows the row
rule of the issue (a row keeps its same-type match, else its different-type match, else is dropped).
"""
import numpy as np


def lsap_max(w):
    """Maximum-weight assignment of a dense non-negative matrix: match[row] = column, or -1 where the assigned weight
    is zero (the reference drops those). Shortest augmenting paths with potentials on -w; rows > columns transposes."""
    w = np.asarray(w, np.float64)
    r, c = w.shape
    if r == 0 or c == 0:
        return np.full(r, -1, np.int64)
    if r > c:
        rows_of = lsap_max(w.T)                       # per column: its row or -1
        match = np.full(r, -1, np.int64)
        for j, i in enumerate(rows_of):
            if i >= 0:
                match[i] = j
        return match
    cost = -w
    u, v = np.zeros(r + 1), np.zeros(c + 1)
    p, way = np.zeros(c + 1, np.int64), np.zeros(c + 1, np.int64)
    for i in range(1, r + 1):
        p[0] = i
        j0 = 0
        minv = np.full(c + 1, np.inf)
        used = np.zeros(c + 1, bool)
        while True:
            used[j0] = True
            i0 = p[j0]
            cur = cost[i0 - 1] - u[i0] - v[1:]
            free = ~used[1:]
            better = free & (cur < minv[1:])
            minv[1:][better] = cur[better]
            way[1:][better] = j0
            cand = np.where(free, minv[1:], np.inf)
            j1 = int(np.argmin(cand)) + 1
            delta = cand[j1 - 1]
            u[p[used]] += delta
            v[used] -= delta
            minv[~used] -= delta
            j0 = j1
            if p[j0] == 0:
                break
        while j0:
            j1 = way[j0]
            p[j0] = p[j1]
            j0 = j1
    match = np.full(r, -1, np.int64)
    for j in range(1, c + 1):
        if p[j] and w[p[j] - 1, j - 1] != 0.0:
            match[p[j] - 1] = j - 1
    return match


def similarity(det, gt, fac, H, W):
    """(person, joint, sim [G, N], same_type [G, N]) of one image; sim in fac's dtype as torch promotes."""
    pi, ji = np.nonzero(gt[:, :, 2])
    pos = np.clip(np.rint(gt[pi, ji, :2]).astype(np.float32), 0, max(H, W))
    d2 = ((pos[:, None, :] - det[None, :, :2].astype(np.float32)) ** 2).sum(-1, dtype=np.float32)
    f = np.asarray(fac)[pi, ji]
    sim = np.exp(-d2 / f[:, None])
    return pi, ji, sim, ji[:, None] == det[None, :, 2]


def node_labels(det, gt, fac, H, W, method, use_neighbours, with_background, mr, ir, J):
    """One image's per-detection results as a dict (ambiguous as bool)."""
    pi, ji, sim, same = similarity(det, gt, fac, H, W)
    G, N = sim.shape
    w_same = np.where(same & (sim >= mr), sim, 0)
    col = lsap_max(w_same)
    if method == 6:
        alt = lsap_max(np.where(~same & (sim >= mr), sim, 0))
        col = np.where(col >= 0, col, alt)
    rows = np.nonzero(col >= 0)[0]
    pairs = [(g, col[g]) for g in rows]
    amb = np.zeros(N, bool)
    if use_neighbours:
        w2 = np.where(sim >= ir, sim, 0) if method == 6 else np.where(w_same >= ir, w_same, 0)
        w2[:, col[rows]] = 0
        amb = (w2 != 0).sum(0) > 1
        w2[:, amb] = 0
        w2[col < 0] = 0
        pairs += list(zip(*np.nonzero(w2)))
    out = dict(node_labels=np.zeros(N, np.float32), node_persons=np.full(N, -1, np.int64),
               node_classes=np.zeros(N, np.int64), label_mask_node=np.ones(N, np.float32), ambiguous=amb)
    for g, n in pairs:                                  # sequential: the last pair of a column wins
        out["node_labels"][n] = 1.0
        out["node_persons"][n] = pi[g]
        out["node_classes"][n] = ji[g]
    if method == 6 and use_neighbours:
        out["label_mask_node"][amb] = 0.0
    out["class_mask"] = out["node_labels"] * out["label_mask_node"]
    if with_background:
        out["node_classes"][out["node_labels"] != 1.0] = J
        out["class_mask"][:] = 1.0
    return out


def edge_labels(edge_index, batch_index, persons, amb, B):
    src, dst = edge_index
    lab = ((persons[src] >= 0) & (persons[src] == persons[dst])).astype(np.float32)
    mask = (~(amb[src] | amb[dst])).astype(np.float32)
    img = batch_index[src]
    for b in range(B):
        if not lab[img == b].any():
            mask[img == b] = 0.0
    return lab, mask


def construct_labels(joint_det, batch_index, edge_index, joints_gt, factors, H, W, B, J, method, use_neighbours,
                     with_background, mr, ir):
    """The seven label slots of construct_graph's tuple, keyed by slot number (3, 4, 5, 8, 9, 10, 13)."""
    per = [node_labels(joint_det[batch_index == b], joints_gt[b], factors[b], H, W, method, use_neighbours,
                       with_background, mr, ir, J) for b in range(B)]
    cat = {k: np.concatenate([p[k] for p in per]) for k in per[0]}
    lab, mask = edge_labels(edge_index, batch_index, cat["node_persons"], cat["ambiguous"], B)
    m6 = method == 6
    return {3: lab, 4: cat["node_labels"], 5: cat["node_classes"] if m6 else None, 8: mask,
            9: cat["label_mask_node"], 10: cat["class_mask"] if m6 else None, 13: cat["node_persons"]}
