"""GPU tests of the training labels (EDGE_LABEL_METHOD 4 / 6): construct_graph with ground truth against the
reference-run fixtures (tests/golden/labels_*.npz), and the two device passes (pemp_label_candidates,
pemp_label_edges) through ctypes against numpy at their edge shapes."""
import ctypes

import numpy as np
import pytest
import torch

import pemp_amd
from pemp_amd import _lib, synthetic as syn
from tests import golden_util as gu, labels_oracle as lo
from tests.test_labels_cpu import CASES, SLOTS, label_config

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
_INPUTS = {}


def inputs(name):
    """(meta, arrays, scoremaps, features, tags) of a fixture, built once."""
    if name not in _INPUTS:
        meta, a = gu.load(name)
        B, J, H, W = meta["B"], meta["J"], meta["H"], meta["W"]
        feats = torch.from_numpy(syn.closed_form((B, meta["C"], H, W), gu.FEATURE_SALT)).to(DEV)
        tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), gu.TAG_SALT)).to(DEV)
        _INPUTS[name] = (meta, a, torch.from_numpy(a["scoremaps"]).to(DEV), feats, tags)
    return _INPUTS[name]


def run_gc(cfg, J, hm, feats, tags, gt, fac, testing=True):
    return pemp_amd.get_graph_constructor(cfg, scoremaps=hm, features=feats, tagmaps=tags, joints_gt=gt,
                                          factor_list=fac, masks=None, device=DEV, testing=testing, heatmaps=None,
                                          num_joints=J).construct_graph()


def labelled(name, f64=True, **cfg_over):
    meta, a, hm, feats, tags = inputs(name)
    cfg = label_config(meta)
    cfg.merge(cfg_over)
    fac = a["factors"] if f64 else a["factors"].astype(np.float32)
    return run_gc(cfg, meta["J"], hm, feats, tags, torch.from_numpy(a["joints_gt"]), torch.from_numpy(fac))


def test_constructor_with_ground_truth_returns_labels():
    out = labelled("labels_m6_nb_fully")
    N, E = out[7].shape[0], out[2].shape[1]
    for i, (dt, n) in {3: (torch.float32, E), 4: (torch.float32, N), 5: (torch.int64, N), 8: (torch.float32, E),
                       9: (torch.float32, N), 10: (torch.float32, N), 13: (torch.int64, N)}.items():
        assert out[i].dtype == dt and tuple(out[i].shape) == (n,) and out[i].device.type == "cuda", i
    assert out[6] is None and out[3].sum() > 0


@pytest.mark.parametrize("f64", [True, False], ids=["f64", "f32"])
@pytest.mark.parametrize("name", CASES)
def test_fixture_parity(name, f64):
    """The seven label slots bit-exact against the reference's, twice on the same shape (the second call of a shape
    is the one an inference constructor sends through the capacity build)."""
    meta, a = inputs(name)[:2]
    first = labelled(name, f64)
    second = labelled(name, f64)
    for out in (first, second):
        assert out[7].shape[0] == meta["N"] and out[2].shape[1] == meta["E"]
        for i in SLOTS:
            if f"slot{i}" not in a:
                assert out[i] is None, i
                continue
            got = out[i].cpu().numpy()
            assert got.dtype == a[f"slot{i}"].dtype, i
            np.testing.assert_array_equal(got, a[f"slot{i}"], err_msg=f"slot {i}")
    for i in range(15):
        assert (first[i] is None) == (second[i] is None) and (first[i] is None or torch.equal(first[i], second[i])), i


@pytest.mark.parametrize("graph", ["score_based", "feature_knn"])
def test_other_graph_types_equal_oracle(graph):
    """GRAPH_TYPE score_based (at least 75 detections per image) and feature_knn, which have no reference-run label
    fixture, against the restated rules on the constructor's own detections and edges."""
    B, J, H, W = 2, 17, 96, 104
    hm, gt, fac = syn.make_labelled_heatmaps(3, B, J, H, W, 6)
    cfg = label_config(dict(graph=graph, method=6, use_neighbours=True, with_background=False,
                            matching_radius=0.5, inclusion_radius=0.75))
    feats = torch.from_numpy(syn.closed_form((B, 8, H, W), gu.FEATURE_SALT)).to(DEV)
    tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), gu.TAG_SALT)).to(DEV)
    out = run_gc(cfg, J, torch.from_numpy(hm).to(DEV), feats, tags, torch.from_numpy(gt), torch.from_numpy(fac))
    mine = lo.construct_labels(out[7].cpu().numpy(), out[12].cpu().numpy(), out[2].cpu().numpy(), gt, fac, H, W, B, J,
                               6, True, False, 0.5, 0.75)
    assert mine[3].sum() > 0
    for i in SLOTS:
        np.testing.assert_array_equal(out[i].cpu().numpy(), mine[i], err_msg=f"slot {i}")


def test_determinism():
    outs = [labelled("labels_m6_nb_fully") for _ in range(10)]
    for o in outs[1:]:
        for i in SLOTS:
            assert torch.equal(o[i], outs[0][i]), i


def test_refused_options_name_their_reason():
    meta, a, hm, feats, tags = inputs("labels_m6_fully")
    gt, fac = torch.from_numpy(a["joints_gt"]), torch.from_numpy(a["factors"])
    for over, testing, word in (({"USE_GT": True}, True, "USE_GT"),
                                ({"IMAGE_CENTRIC_SAMPLING": True}, True, "IMAGE_CENTRIC_SAMPLING"),
                                ({"EDGE_LABEL_METHOD": 1}, True, "EDGE_LABEL_METHOD"),
                                ({"EDGE_LABEL_METHOD": 2}, True, "EDGE_LABEL_METHOD"),
                                ({"EDGE_LABEL_METHOD": 3}, True, "EDGE_LABEL_METHOD"),
                                ({"EDGE_LABEL_METHOD": 5}, True, "EDGE_LABEL_METHOD"),
                                ({"EDGE_LABEL_METHOD": 7}, True, "EDGE_LABEL_METHOD"),
                                ({"NODE_DROPOUT": 0.1}, False, "NODE_DROPOUT"),
                                ({"WEIGHT_CLASS_LOSS": True}, True, "WEIGHT_CLASS_LOSS")):
        cfg = label_config(meta)
        cfg.merge(over)
        with pytest.raises(NotImplementedError, match=word) as e:
            run_gc(cfg, meta["J"], hm, feats, tags, gt, fac, testing)
        assert "ConstructGraph.py:" in str(e.value)
    cfg = label_config(meta)
    cfg.merge({"NODE_DROPOUT": 0.1})                     # testing=True: the dropout is off, as in the reference
    assert run_gc(cfg, meta["J"], hm, feats, tags, gt, fac, True)[3] is not None


def test_ground_truth_off_is_untouched():
    """After calls with ground truth, a constructor without it returns an existing gc_ fixture unchanged with the
    label slots None."""
    labelled("labels_m4_fully")
    meta, a = gu.load("gc_small_fully")
    hm, feats, tags, masks = gu.gc_inputs(meta, a)
    for _ in range(2):                                   # the exact build, then the capacity build
        out = run_gc(gu.gc_config(meta), meta["J"], hm.to(DEV), feats.to(DEV), tags.to(DEV), None, None)
        assert all(out[i] is None for i in (3, 4, 5, 6, 8, 9, 10, 13))
        np.testing.assert_array_equal(out[7].cpu().numpy(), a["joint_det"])
        np.testing.assert_array_equal(out[11].cpu().numpy(), a["joint_scores"])
        assert gu.sha(out[2]) == meta["sha_edge_index"] and gu.sha(out[0]) == meta["sha_x"]
        assert gu.sha(out[1]) == meta["sha_edge_attr"]


# ---- pemp_label_candidates through ctypes ----
def candidates(gt, fac, dets, H, W, thr, cap):
    """One call on a batch: gt [B, P, J, 3], fac [B, P, J] (its dtype picks the precision), dets a list of [n_b, 3].
    Returns (hdr, gt_tab [B, P J], recs [B, cap])."""
    L = _lib.lib()
    B, P, J = gt.shape[:3]
    off = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(np.int64)
    det = torch.from_numpy(np.concatenate(dets).astype(np.int64).reshape(-1, 3)).to(DEV)
    gt_d, fac_d, off_d = torch.from_numpy(gt).to(DEV), torch.from_numpy(fac).to(DEV), torch.from_numpy(off).to(DEV)
    hdr = torch.full((2 * B + 1,), -7, dtype=torch.int32, device=DEV)
    tab = torch.full((B, P * J), -7, dtype=torch.int32, device=DEV)
    recs = torch.zeros(B * max(cap, 1) * 16 + 64, dtype=torch.uint8, device=DEV)
    recs[B * cap * 16:] = 0xAB                                  # a guard behind the last record
    ws = torch.empty(L.pemp_label_candidates_scratch_size(B, P, J), dtype=torch.uint8, device=DEV)
    _lib.check(L.pemp_label_candidates(gt_d.data_ptr(), fac_d.data_ptr(), int(fac.dtype == np.float64), B, P, J,
                                       det.data_ptr(), off_d.data_ptr(), H, W, thr, cap, recs.data_ptr(),
                                       hdr.data_ptr(), tab.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream(DEV)))
    torch.cuda.synchronize()
    raw = recs.cpu().numpy()
    assert (raw[B * cap * 16:] == 0xAB).all()
    return hdr.cpu().numpy(), tab.cpu().numpy(), raw[:B * cap * 16].view(_lib.LABEL_CAND_DTYPE).reshape(B, cap)


def expected_candidates(gt, fac, det, H, W, thr):
    pi, ji, sim, same = lo.similarity(det, gt, fac, H, W)
    # the device's exp and numpy's each stay within an ulp or two of the exact value (relative 2.4e-7 in float32):
    # no similarity of the test data may lie that close to the threshold
    assert not (np.abs(sim.astype(np.float64) - thr) <= 1e-5 * thr).any()
    g, n = np.nonzero(sim >= thr)
    return pi * gt.shape[1] + ji, g, n, same[g, n], sim[g, n]


def check_candidates(gt, fac, dets, H, W, thr):
    B = gt.shape[0]
    exp = [expected_candidates(gt[b], fac[b], dets[b], H, W, thr) for b in range(B)]
    need = max(len(e[1]) for e in exp)
    hdr, tab, recs = candidates(gt, fac, dets, H, W, thr, need)
    assert hdr[2 * B] == 0
    rtol = 1e-13 if fac.dtype == np.float64 else 1e-6     # a few ulps of the format (see expected_candidates)
    for b, (t, g, n, same, sim) in enumerate(exp):
        assert hdr[b] == len(g) and hdr[B + b] == len(t), b
        np.testing.assert_array_equal(tab[b, :len(t)], t)
        r = recs[b, :len(g)]
        np.testing.assert_array_equal(r["g"], g)
        np.testing.assert_array_equal(r["n"] & 0x7FFFFFFF, n)
        np.testing.assert_array_equal(r["n"] >> 31, same)
        np.testing.assert_allclose(r["sim"], sim.astype(np.float64), rtol=rtol, atol=0)
    return need, exp


def scattered(rng, gt, n, spread):
    """n detections around the visible joints of gt [P, J, 3] (anywhere when there are none)."""
    pi, ji = np.nonzero(gt[:, :, 2])
    det = np.zeros((n, 3), np.int64)
    if len(pi):
        k = rng.integers(0, len(pi), n)
        det[:, :2] = np.rint(gt[pi[k], ji[k], :2]).astype(np.int64) + rng.integers(-spread, spread + 1, (n, 2))
        det[:, 2] = np.where(rng.random(n) < 0.5, ji[k], rng.integers(0, gt.shape[1], n))
    else:
        det[:] = rng.integers(0, 17, (n, 3))
    return det


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_candidate_kernel_edges(dtype):
    """G = 0, G = 1, N = 1, and 510 visible joints against 300 detections in one batch; a detection count that is
    no multiple of 64; a capacity one short of the need overflows and the retry returns the whole ordered list."""
    rng = np.random.default_rng(5)
    B, P, J, H, W = 5, 30, 17, 200, 232
    gt = np.zeros((B, P, J, 3), np.float32)
    gt[..., :2] = rng.uniform(5, 195, (B, P, J, 2))
    gt[1, 7, 3, 2] = 1                                          # G = 1
    gt[2, :2, :, 2] = rng.random((2, J)) > 0.5                  # a few rows against N = 1
    gt[3, :, :, 2] = rng.integers(1, 3, (P, J))                 # G = 510
    gt[4, :3, :, 2] = 1
    fac = rng.uniform(1.0, 40.0, (B, P, J)).astype(dtype)
    dets = [scattered(rng, gt[0], 5, 3), scattered(rng, gt[1], 70, 2), scattered(rng, gt[2], 1, 1),
            scattered(rng, gt[3], 300, 3), scattered(rng, gt[4], 131, 3)]
    need, exp = check_candidates(gt, fac, dets, H, W, 0.5)
    assert len(exp[0][1]) == 0 and len(exp[1][1]) > 0 and len(exp[3][1]) > 300
    # one record short: the overflow status, every image's count, and nothing stored
    hdr, tab, recs = candidates(gt, fac, dets, H, W, 0.5, need - 1)
    assert hdr[2 * B] == 1 and [hdr[b] for b in range(B)] == [len(e[1]) for e in exp]
    L = _lib.lib()
    p = lambda x: x.ctypes.data_as(ctypes.c_void_p)
    off = np.concatenate([[0], np.cumsum([len(d) for d in dets])]).astype(np.int64)
    o = [np.zeros(int(off[-1]), t) for t in (np.float32, np.int64, np.int64, np.float32, np.float32, np.uint8)]
    tab_c, recs_c = np.ascontiguousarray(tab), np.ascontiguousarray(recs)
    assert L.pemp_label_assign(B, P, J, p(hdr), p(tab_c), p(recs_c), need - 1, p(off), 6, 1, 0, 0.5, 0.75,
                               *[p(x) for x in o]) == _lib.LABEL_OVERFLOW
    hdr2, _, recs2 = candidates(gt, fac, dets, H, W, 0.5, int(hdr[:B].max()))
    assert hdr2[2 * B] == 0
    np.testing.assert_array_equal(recs2[3, :hdr2[3]]["g"], exp[3][1])
    np.testing.assert_array_equal(recs2[3, :hdr2[3]]["n"] & 0x7FFFFFFF, exp[3][2])


@pytest.mark.parametrize("dtype", [np.float32, np.float64], ids=["f32", "f64"])
def test_candidate_rounding_and_clamp(dtype):
    """Ground-truth coordinates at -3.2 (clamped to 0), exactly 2.5 and 3.5 (2 and 4: half to even), H + 5 (inside
    the clamp bound max(H, W) although past the last row) and W + 5 (clamped to max(H, W), one past the last column)."""
    H, W = 24, 32
    gt = np.zeros((1, 2, 4, 3), np.float32)
    gt[0, 0, :, 0] = (-3.2, 2.5, 3.5, W + 5)
    gt[0, 0, :, 1] = (2.5, -3.2, H + 5, 3.5)
    gt[0, 0, :, 2] = 1
    gt[0, 1, 1] = (3.5, 2.5, 2)
    fac = np.full((1, 2, 4), 3.0, dtype)
    xs = np.array([0, 1, 2, 3, 4, 5, 28, 29, 30, 31, 32])
    det = np.stack([np.repeat(xs, len(xs)), np.tile(xs, len(xs)), np.arange(len(xs) ** 2) % 4], 1)
    _, exp = check_candidates(gt, fac, [det], H, W, 0.7)
    t, g, n, same, sim = exp[0]
    exact = {(int(gg), tuple(det[nn, :2])) for gg, nn, s in zip(g, n, sim) if s == 1.0}
    assert exact == {(0, (0, 2)), (1, (2, 0)), (2, (4, 29)), (3, (32, 4)), (4, (4, 2))}


# ---- pemp_label_edges through ctypes ----
def edge_pass(ei, off, persons, amb):
    L = _lib.lib()
    B, E, N = len(off) - 1, ei.shape[1], len(persons)
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    ei_d, off_d, per_d, amb_d = t(ei), t(off), t(persons), t(amb)
    lab = torch.full((E + 2,), 7.0, device=DEV)
    mask = torch.full((E + 2,), 7.0, device=DEV)
    ws = torch.empty(L.pemp_label_edges_scratch_size(B), dtype=torch.uint8, device=DEV)
    _lib.check(L.pemp_label_edges(ei_d.data_ptr(), E, off_d.data_ptr(), B, N, per_d.data_ptr(), amb_d.data_ptr(),
                                  lab.data_ptr(), mask.data_ptr(), ws.data_ptr(), ws.numel(), _lib.stream(DEV)))
    torch.cuda.synchronize()
    lab, mask = lab.cpu().numpy(), mask.cpu().numpy()
    assert (lab[E:] == 7).all() and (mask[E:] == 7).all()      # nothing written past E
    return lab[:E], mask[:E]


@pytest.mark.parametrize("E", [0, 1, 63, 64, 65, 4097, 4098])
def test_edge_pass_edges(E):
    """Four images: positives, no edges at all, no positive edge (its mask alone is zeroed), positives; the image
    boundaries fall inside waves; the first and the last node are ambiguous."""
    rng = np.random.default_rng(E)
    sizes = np.array([6, 3, 5, 7])
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    N = int(off[-1])
    share = [E * 2 // 5, 0, E // 5, E - E * 2 // 5 - E // 5]    # edges per image
    src, dst = [], []
    for b, k in enumerate(share):
        s = rng.integers(0, sizes[b], k)
        d = (s + rng.integers(1, sizes[b], k)) % sizes[b]
        order = np.lexsort((d, s))
        src.append(s[order] + off[b])
        dst.append(d[order] + off[b])
    ei = np.stack([np.concatenate(src), np.concatenate(dst)]).astype(np.int64)
    persons = np.full(N, -1, np.int64)
    persons[0:6] = (0, 0, 1, -1, 1, 0)
    persons[14:21] = (2, 2, 2, -1, 0, 0, 2)
    amb = np.zeros(N, np.uint8)
    amb[0] = amb[N - 1] = 1
    bidx = np.repeat(np.arange(4), sizes)
    exp_lab, exp_mask = lo.edge_labels(ei, bidx, persons, amb.astype(bool), 4)
    lab, mask = edge_pass(ei, off, persons, amb)
    np.testing.assert_array_equal(lab, exp_lab)
    np.testing.assert_array_equal(mask, exp_mask)
    if E >= 63:
        img = bidx[ei[0]]
        assert lab[img == 0].any() and lab[img == 3].any() and not lab[img == 2].any()
        assert (mask[img == 2] == 0).all() and mask[img == 0].any() and mask[img == 3].any()
        assert (mask[(ei[0] == 0) | (ei[1] == N - 1)] == 0).all()
