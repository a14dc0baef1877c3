"""Training labels (EDGE_LABEL_METHOD 4 / 6) without a GPU: the restated rules (tests/labels_oracle.py) against the
reference-run fixtures (tests/golden/labels_*.npz, tools/gen_golden_labels.py), and the host matching entry
pemp_label_assign through ctypes on hand-made candidate lists."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import restate
from pemp_amd import _lib, synthetic as syn
from tests import golden_util as gu, labels_oracle as lo

SLOTS = (3, 4, 5, 8, 9, 10, 13)
CASES = [n for n in gu.names("labels_") if not n.startswith("labels_lsap_")]
LSAP = gu.names("labels_lsap_")


def label_config(meta):
    g = gu.pcfg.inference_gc_config(meta["graph"], 5, False)
    g.merge({"EDGE_LABEL_METHOD": meta["method"], "USE_NEIGHBOURS": meta["use_neighbours"],
             "WITH_BACKGROUND": meta["with_background"], "MATCHING_RADIUS": meta["matching_radius"],
             "INCLUSION_RADIUS": meta["inclusion_radius"]})
    return g


def test_fixture_set_is_complete():
    assert len(CASES) == 7 and len(LSAP) >= 3
    for name in CASES:
        meta, a = gu.load(name)
        assert meta["positive_edges"] > 0 and a["slot3"].sum() == meta["positive_edges"]
        assert not meta["use_neighbours"] or meta["ambiguous_nodes"] > 0
        assert meta["method"] != 6 or meta["fill_ins"] > 0
        assert (a["joints_gt"][-1, :, :, 2] == 0).all()          # one image without ground truth


@pytest.mark.parametrize("name", CASES)
def test_oracle_equals_reference(name):
    """The restated rules on the CPU oracle's graph equal the reference's labels bit for bit, with float64 and
    float32 factors."""
    meta, a = gu.load(name)
    B, J, H, W = meta["B"], meta["J"], meta["H"], meta["W"]
    hm = torch.from_numpy(a["scoremaps"])
    feats = torch.from_numpy(syn.closed_form((B, meta["C"], H, W), gu.FEATURE_SALT))
    tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), gu.TAG_SALT))
    g = restate.construct_graph(hm, feats, tags, None, label_config(meta), J)
    assert g[7].shape[0] == meta["N"] and g[2].shape[1] == meta["E"]
    for fac in (a["factors"], a["factors"].astype(np.float32)):
        mine = lo.construct_labels(g[7].numpy(), g[12].numpy(), g[2].numpy(), a["joints_gt"], fac, H, W, B, J,
                                   meta["method"], meta["use_neighbours"], meta["with_background"],
                                   meta["matching_radius"], meta["inclusion_radius"])
        for i in SLOTS:
            if f"slot{i}" not in a:
                assert mine[i] is None, i
                continue
            assert mine[i].dtype == a[f"slot{i}"].dtype, i
            np.testing.assert_array_equal(mine[i], a[f"slot{i}"], err_msg=f"slot {i}")


# ---- pemp_label_assign through ctypes ----
def assign(images, method, nb, bg, mr, ir, J, P, thr=None, cap=None):
    """pemp_label_assign on `images` = [(sim [G, N], same [G, N], gt_tab [G])]: the records are the entries with
    sim >= thr in (g, n) order, as pemp_label_candidates stores them. Returns the per-node outputs."""
    L = _lib.load_cdll()
    B = len(images)
    thr = (min(mr, ir) if nb else mr) if thr is None else thr
    lists = []
    for sim, same, tab in images:
        g, n = np.nonzero(sim >= thr)
        rec = np.zeros(len(g), _lib.LABEL_CAND_DTYPE)
        rec["g"], rec["n"], rec["sim"] = g, n.astype(np.uint32) | (same[g, n].astype(np.uint32) << 31), sim[g, n]
        lists.append(rec)
    cap = max([len(r) for r in lists] + [1]) if cap is None else cap
    recs = np.zeros((B, cap), _lib.LABEL_CAND_DTYPE)
    hdr = np.zeros(2 * B + 1, np.int32)
    gt_tab = np.zeros((B, P * J), np.int32)
    off = np.zeros(B + 1, np.int64)
    for b, ((sim, same, tab), rec) in enumerate(zip(images, lists)):
        recs[b, :len(rec)] = rec
        hdr[b], hdr[B + b] = len(rec), sim.shape[0]
        gt_tab[b, :len(tab)] = tab
        off[b + 1] = off[b] + sim.shape[1]
    N = int(off[B])
    out = dict(node_labels=np.full(N, 7, np.float32), node_persons=np.full(N, 7, np.int64),
               node_classes=np.full(N, 7, np.int64), label_mask_node=np.full(N, 7, np.float32),
               class_mask=np.full(N, 7, np.float32), ambiguous=np.full(N, 7, np.uint8))
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    m6 = method == 6
    rc = L.pemp_label_assign(B, P, J, p(hdr), p(gt_tab), p(recs), cap, p(off), method, int(nb), int(bg), mr, ir,
                             p(out["node_labels"]), p(out["node_persons"]), p(out["node_classes"]) if m6 else None,
                             p(out["label_mask_node"]), p(out["class_mask"]) if m6 else None, p(out["ambiguous"]))
    assert rc == 0, L.pemp_last_error()
    return out


def matched_pairs(w, P=None):
    """(rows, cols) pemp_label_assign matches on the weight matrix w (all one type; row g is person g)."""
    G = w.shape[0]
    out = assign([(w, np.ones(w.shape, bool), np.arange(G, dtype=np.int32))], 4, False, False, 1e-9, 1.0, 1, G)
    cols = np.nonzero(out["node_labels"] == 1)[0]
    rows = out["node_persons"][cols]
    assert (rows >= 0).all() and len(set(rows.tolist())) == len(rows)
    assert ((out["node_persons"] >= 0) == (out["node_labels"] == 1)).all()
    order = np.argsort(rows)
    return rows[order], cols[order]


@pytest.mark.parametrize("name", LSAP)
def test_assign_returns_the_stored_scipy_pairs(name):
    z = np.load(f"{gu.GOLDEN}/{name}.npz")
    rows, cols = matched_pairs(z["cost"])
    np.testing.assert_array_equal(rows, z["rows"])
    np.testing.assert_array_equal(cols, z["cols"])


@pytest.mark.parametrize("G,N", [(12, 30), (30, 12), (40, 40), (3, 200), (64, 5)])
def test_assign_total_equals_scipy_on_ties(G, N):
    lsa = pytest.importorskip("scipy.optimize").linear_sum_assignment
    rng = np.random.default_rng(G * 1000 + N)
    for density in (0.05, 0.3, 0.9):
        w = rng.choice([0.5, 0.625, 0.75, 1.0], (G, N)) * (rng.random((G, N)) < density)
        rows, cols = matched_pairs(w)
        assert (w[rows, cols] > 0).all()
        r, c = lsa(w, maximize=True)
        assert abs(w[rows, cols].sum() - w[r, c].sum()) <= 1e-6


def random_image(rng, G_people, N, J, H, W, f_lo, f_hi):
    """Detections scattered around the ground-truth joints of G_people people (P = G_people)."""
    gt = np.zeros((G_people, J, 3), np.float32)
    gt[:, :, :2] = rng.uniform(4, min(H, W) - 4, (G_people, J, 2))
    gt[:, :, 2] = rng.random((G_people, J)) > 0.25
    fac = rng.uniform(f_lo, f_hi, (G_people, J))
    pi, ji = np.nonzero(gt[:, :, 2])
    det = np.zeros((N, 3), np.int64)
    if len(pi) and N:
        pick = rng.integers(0, len(pi), N)
        det[:, :2] = np.rint(gt[pi[pick], ji[pick], :2]).astype(np.int64) + rng.integers(-3, 4, (N, 2))
        det[:, 2] = np.where(rng.random(N) < 0.6, ji[pick], rng.integers(0, J, N))
    else:
        det[:, :2] = rng.integers(0, min(H, W), (N, 2))
        det[:, 2] = rng.integers(0, J, N)
    return det, gt, fac


def check_against_oracle(images, method, nb, bg, mr, ir, J, P, H, W):
    prepared = []
    for det, gt, fac in images:
        pi, ji, sim, same = lo.similarity(det, gt, fac, H, W)
        prepared.append((sim, same, (pi * J + ji).astype(np.int32)))
    got = assign(prepared, method, nb, bg, mr, ir, J, P)
    exp = [lo.node_labels(det, gt, fac, H, W, method, nb, bg, mr, ir, J) for det, gt, fac in images]
    keys = ["node_labels", "node_persons", "label_mask_node", "ambiguous"] + (
        ["node_classes", "class_mask"] if method == 6 else [])
    for k in keys:
        e = np.concatenate([x[k] for x in exp])
        np.testing.assert_array_equal(got[k], e.astype(got[k].dtype), err_msg=k)
    return got


@pytest.mark.parametrize("method,nb,bg", [(4, False, False), (4, True, False), (6, False, False), (6, True, False),
                                           (6, True, True), (6, False, True)])
def test_assign_equals_oracle(method, nb, bg):
    """Two-image batches with rows below and above the detection count (G > N follows the row rule), and an image
    without ground truth in the middle."""
    rng = np.random.default_rng(method * 10 + nb * 2 + bg)
    J, P, H, W = 5, 6, 64, 80
    for trial in range(6):
        a = random_image(rng, P, 40, J, H, W, 4.0, 60.0)
        none = random_image(rng, P, 9, J, H, W, 4.0, 60.0)
        none[1][:, :, 2] = 0                                   # G == 0
        c = random_image(rng, P, 7, J, H, W, 4.0, 60.0)       # G > N
        got = check_against_oracle([a, none, c], method, nb, bg, 0.5, 0.75, J, P, H, W)
        assert (got["node_labels"][40:49] == 0).all() and (got["node_persons"][40:49] == -1).all()
        assert got["node_labels"][:40].sum() > 0


def test_no_ground_truth_gives_zero_labels():
    det = np.array([[3, 4, 0], [9, 9, 1]], np.int64)
    gt = np.zeros((2, 3, 3), np.float32)
    for method, bg in ((4, False), (6, False), (6, True)):
        got = check_against_oracle([(det, gt, np.ones((2, 3)))], method, True, bg, 0.5, 0.75, 3, 2, 32, 32)
        assert (got["node_labels"] == 0).all() and (got["node_persons"] == -1).all() and (got["ambiguous"] == 0).all()
        if method == 6:
            assert (got["node_classes"] == (3 if bg else 0)).all() and (got["class_mask"] == (1 if bg else 0)).all()


def test_duplicate_column_last_write_wins():
    """Method 6: person 0's joint 0 takes detection 0 by type, person 1's joint 1 has no detection of its type and
    takes the same detection as its different-type fill-in. Both pairs are written in row order: the later one stays,
    as the reference's sequential CPU index_put leaves it."""
    det = np.array([[10, 10, 0], [40, 40, 2], [50, 20, 2]], np.int64)
    gt = np.zeros((2, 3, 3), np.float32)
    gt[0, 0] = (10.2, 9.8, 1)
    gt[1, 1] = (10.4, 10.3, 2)
    got = check_against_oracle([(det, gt, np.full((2, 3), 20.0))], 6, False, False, 0.5, 0.75, 3, 2, 64, 64)
    assert got["node_labels"].tolist() == [1, 0, 0]
    assert got["node_persons"].tolist() == [1, -1, -1] and got["node_classes"].tolist() == [1, 0, 0]


def test_assign_reports_overflow_and_bad_records():
    L = _lib.load_cdll()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    hdr = np.array([5, 2, 1], np.int32)                         # one image, 5 records needed, overflow raised
    tab = np.zeros(4, np.int32)
    recs = np.zeros(4, _lib.LABEL_CAND_DTYPE)
    off = np.array([0, 3], np.int64)
    o = [np.zeros(3, t) for t in (np.float32, np.int64, np.int64, np.float32, np.float32, np.uint8)]
    args = lambda: (1, 2, 2, p(hdr), p(tab), p(recs), 4, p(off), 6, 0, 0, 0.5, 0.75, *[p(x) for x in o])
    assert L.pemp_label_assign(*args()) == _lib.LABEL_OVERFLOW
    hdr[:] = (1, 2, 0)
    recs[0] = (1, 5, 0.9)                                       # detection 5 of 3
    assert L.pemp_label_assign(*args()) == _lib.ERR_INVALID_ARG
    recs[0] = (1, 2, 0.9)
    assert L.pemp_label_assign(*args()) == 0
    assert L.pemp_label_assign(*(args()[:8] + (5,) + args()[9:])) == _lib.ERR_UNSUPPORTED   # method 5
