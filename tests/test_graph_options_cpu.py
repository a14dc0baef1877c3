"""The numpy references of tests/graph_options.py against the oracle restatement (oracle/restate.py), which the
fixtures pin to the reference itself: the nine edge-feature modes, and the hybrid top-k + threshold detection at
HYBRID_K 1, 8, 9 and 32. CPU only."""
import numpy as np
import pytest
import torch

from oracle import restate
from pemp_amd import config as pcfg, synthetic as syn
from tests import graph_options as go


def _restate_ea(det, ei, J, norm, mode, tags, scores):
    t = None
    if tags is not None:
        t = torch.from_numpy(np.asarray(tags, np.float32))
    return restate.edge_features(torch.from_numpy(det), torch.from_numpy(ei), J, norm, go.FEATURES[mode], t,
                                 None if scores is None else torch.from_numpy(scores)).numpy()


def _tag_cases(mode):
    """The tag dims a mode is run with: both where the reference takes both."""
    if mode not in go.TAG_MODES:
        return (None,)
    return {5: (1, 2), 6: (1,), 7: (2,), 8: (1, 2)}[mode]


@pytest.mark.parametrize("norm", [1, 4096, 104])
@pytest.mark.parametrize("mode", go.MODES)
def test_expected_edge_attr_planted(mode, norm):
    """expected_edge_attr equals restate.edge_features bit for bit (theta within 2 ulp) on the planted nodes and on
    the sweep of every horizontal / vertical offset."""
    p = go.planted_nodes()
    sdet, sei = go.sweep_nodes()
    rng = np.random.default_rng(3)
    stags = {1: rng.standard_normal(sdet.shape[0]).astype(np.float32),
             2: rng.standard_normal((sdet.shape[0], 2)).astype(np.float32)}
    ssc = rng.random(sdet.shape[0]).astype(np.float32)
    for F in _tag_cases(mode):
        for det, ei, tags, sc in ((p["det"], go.fully_pairs([24]), p["tags"], p["scores"]), (sdet, sei, stags, ssc)):
            t = None if F is None else tags[F]
            want = _restate_ea(det, ei, go.PLANTED_J, norm, mode, t, sc)
            got = go.expected_edge_attr(det, ei, go.PLANTED_J, norm, go.FEATURES[mode], t, sc)
            assert got.dtype == np.float32 and got.shape == (ei.shape[1], go.width(mode, go.PLANTED_J))
            go.check_edge_attr(got, want, mode, f"mode {mode} F {F} norm {norm}")


def test_planted_nodes_hold_their_edge_cases():
    """The planted sets contain what their docstrings promise (so that a later edit cannot thin them out)."""
    p = go.planted_nodes()
    det, ei = p["det"], go.fully_pairs(p["counts"])
    assert ei.shape[1] == 23 * 22
    s, d = ei
    ddx, ddy = det[d, 0] - det[s, 0], det[d, 1] - det[s, 1]
    assert ((ddx == 0) & (ddy == 0) & (det[s, 2] != det[d, 2])).any()
    for off in (1, 41, 47, 200):
        for sign in (1, -1):
            assert ((ddx == sign * off) & (ddy == 0)).any() and ((ddy == sign * off) & (ddx == 0)).any()
    assert det[:, 0].max() == 4095 and det[:, 1].max() < go.PLANTED_HW[0] and det[:, 0].max() < go.PLANTED_HW[1]
    d1 = go.expected_edge_attr(det, ei, 17, 1, ["ae"], p["tags"][1])[:, 0]
    d2 = go.expected_edge_attr(det, ei, 17, 1, go.FEATURES[5], p["tags"][2])[:, -1]
    for dist in (d1, d2):
        assert {0.0, 0.5, 1.5, 2.5} <= set(dist[np.isfinite(dist)].tolist())
        assert np.isnan(dist).any()
    assert np.isinf(d2).any() and not np.isinf(d1).any()       # (2 BIG)^2 overflows only under the square
    n7 = go.expected_edge_attr(det, ei, 17, 1, ["ae_normed"], p["tags"][2], p["scores"])[:, 0]
    sc = p["scores"][s]
    assert (n7[(d2 == 0.5) & (sc == 0)] == 0).all() and (n7[(d2 == 1.5) & (sc == 0)] == 200).all()
    assert (n7[(d2 == 2.5) & (sc == 0)] == 200).all()          # half to even
    assert (p["scores"] < 0).any() and np.signbit(p["scores"][p["scores"] == 0]).any()
    sdet, sei = go.sweep_nodes()
    sdx, sdy = sdet[sei[1], 0] - sdet[sei[0], 0], sdet[sei[1], 1] - sdet[sei[0], 1]
    for k in range(1, 201):
        assert ((sdx == k) & (sdy == 0)).any() and ((sdx == -k) & (sdy == 0)).any()
        assert ((sdy == k) & (sdx == 0)).any() and ((sdy == -k) & (sdx == 0)).any()
    assert abs(sdx).max() == 4095 and abs(sdy).max() == 4095


def test_theta_reference_spread():
    """Every integer offset with |a_x|, |a_y| <= 200: torch's theta (the reference's own ops) is within 1 ulp of the
    rounded float64 acos of the same fp32 argument, which leaves 1 ulp of the 2-ulp bar to the device's acosf; the
    argument never exceeds 1 and is 1 - 2^-24 for some purely horizontal offsets (theta 3.45e-4, not 0)."""
    r = np.arange(-200, 201)
    gx, gy = np.meshgrid(r, r)
    det = np.stack([gx.ravel() + 200, gy.ravel() + 200, np.zeros(gx.size, np.int64)], 1).astype(np.int64)
    centre = 200 * 401 + 200
    dst = np.arange(det.shape[0])
    ei = np.stack([np.full(dst.shape, centre), dst]).astype(np.int64)
    want = _restate_ea(det, ei, 1, 1, 4, None, None)[:, 2]
    got = go.expected_edge_attr(det, ei, 1, 1, go.FEATURES[4])[:, 2]
    assert go.ulp_diff(got, want) <= 1
    assert got[centre] == 0 and want[centre] == 0                      # NaN -> 0
    ax = (det[centre, 0] - det[:, 0]).astype(np.float32)
    ay = (det[centre, 1] - det[:, 1]).astype(np.float32)
    with np.errstate(all="ignore"):
        arg = ax * (np.float32(1) / np.sqrt(ax * ax + ay * ay))
    assert np.nanmax(np.abs(arg)) <= 1
    short = (ay == 0) & (ax > 0) & (arg < 1)
    assert short.sum() == 23 and np.allclose(got[short], 3.4526698e-4, rtol=1e-6)


@pytest.mark.parametrize("graph,persons", [("fully", 3), ("knn", 5), ("feature_knn", 5), ("score_based", 7)])
def test_expected_edge_attr_on_constructed_batches(graph, persons):
    """One restate.construct_graph batch per graph type: its edge_attr in all nine modes equals expected_edge_attr
    on the batch's own nodes and edges."""
    B, J, H, W = 2, 17, 96, 104
    hm = torch.from_numpy(syn.make_heatmaps(20 + persons, B, J, H, W, persons, margin=4))
    feats = torch.from_numpy(syn.closed_form((B, 16, H, W), 0.25))
    for mode in go.MODES:
        F = go.tag_dims(mode)
        tags = torch.from_numpy(syn.closed_form((B, J, H, W, F), 0.75))
        for normed in (True, False):
            gc = pcfg.inference_gc_config(graph, 5, False)
            gc.EDGE_FEATURES_TO_USE = go.FEATURES[mode]
            gc.NORM_NODE_DISTANCE = normed
            out = restate.construct_graph(hm, feats, tags, None, gc, J)
            got = go.expected_edge_attr(out[7].numpy(), out[2].numpy(), J, W if normed else 1, go.FEATURES[mode],
                                        out[14].numpy().reshape(out[7].shape[0], F), out[11].numpy())
            assert out[2].shape[1] > 1000
            go.check_edge_attr(got, out[1].numpy(), mode, f"{graph} mode {mode} normed {normed}")


def _restate_detect(hm, masks, K, pool=3, thr=0.1):
    out = []
    for b in range(hm.shape[0]):
        out.append(restate.joint_det_from_scoremap(torch.from_numpy(hm[b]), hm.shape[1], threshold=thr,
                                                   pool_kernel=pool,
                                                   mask=None if masks is None else torch.from_numpy(masks[b]),
                                                   hybrid_k=K))
    return out


@pytest.mark.parametrize("with_masks", [False, True])
@pytest.mark.parametrize("live", [3, 40, 90])
@pytest.mark.parametrize("K", [1, 8, 9, 32])
def test_detect_topk_against_brute_force(K, live, with_masks):
    """restate.joint_det_from_scoremap at HYBRID_K 1, 8, 9, 32 equals the brute-force top-k + threshold set (ties
    to the lower flat index) on the planted lattice planes: same detections, same order, same scores."""
    hm, masks = go.topk_maps(192, 496, live, K, with_masks)
    if live > K:     # equal values on both sides of the top-k boundary: the lower flat index decides
        ranked = [-np.sort(-hm[b, t].ravel()) for b, t in ((0, 0), (0, 1), (1, 1))]
        assert K == 1 or any(r[K - 1] == r[K] > 0 for r in ranked)
    for b, (det, sc) in enumerate(_restate_detect(hm, masks, K)):
        sm = go.nms_numpy(hm[b], 3, None if masks is None else masks[b])
        want_det, want_sc = go.brute_detect(sm, K, 0.1)
        np.testing.assert_array_equal(det.numpy(), want_det)
        assert go.same_bits(sc.numpy(), want_sc).all()
        per_type = np.bincount(want_det[:, 2], minlength=3)
        if b == 0 and not with_masks:       # the negative plane lists its K entries less the zeros its NMS leaves
            assert per_type[2] == (1 if K == 1 else K - 3)
            assert (want_sc[want_det[:, 2] == 2] < 0).sum() == (1 if K == 1 else K - 4)
        if b == 1:                          # the zero plane lists nothing, the sub-threshold plane its top-k only
            assert per_type[0] == 0 and per_type[2] <= min(K, live)
            assert with_masks or per_type[2] == min(K, live)


def test_detect_topk_clamped_to_the_plane():
    """HYBRID_K = 32 on an 8 x 3 plane: k = H W = 24 (ConstructGraph.py:1177 topk over the whole plane)."""
    rng = np.random.default_rng(5)
    hm = (rng.random((1, 2, 8, 3)) - 0.3).astype(np.float32)
    (det, sc), = _restate_detect(hm, None, 32)
    want_det, want_sc = go.brute_detect(go.nms_numpy(hm[0], 3), 32, 0.1)
    np.testing.assert_array_equal(det.numpy(), want_det)
    assert go.same_bits(sc.numpy(), want_sc).all() and det.shape[0] > 4
