"""pemp_detect_projected on the device over the case table of tests/projected_cases.py: the generic, separable and
exact-2x loaders of the NMS strip kernel at every pool radius, with and without masks and the flipped pass, all four
threshold forms, on both sides of the separable loader's 16-row limit, planes narrower than a wave and strips past
the plane, detections on every border, a non-power-of-two divisor and the two-kernel selection. Everything bit for
bit against the oracle (oracle/restate.py) run on its own fp32 projection of the same network outputs: equal scores
are what ties the three loaders to the emission's proj_pixel."""
import numpy as np
import pytest
import torch

import pemp_amd
from oracle import restate
from pemp_amd import _lib, synthetic as syn
from pemp_amd.frontend import ProjectedHeatmaps, ProjectedMaps
from pemp_amd.graph_constructor import NaiveGraphConstructor as G
from tests import graph_options as go, projected_cases as pc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
OUTPUTS = (7, 11, 12, 14, 2, 0, 1)


@pytest.fixture(autouse=True)
def constructor_state(monkeypatch):
    """Every test starts without capacity hints or step plans and with the detection capacity at 512."""
    monkeypatch.setattr(G, "_cap", 512)
    monkeypatch.setattr(G, "_graph_hint", {})
    monkeypatch.setattr(G, "_plans", {})


def device_inputs(name):
    c = pc.BY_NAME[name]
    outs, flips, masks, low = pc.make_inputs(name)
    ph = ProjectedHeatmaps([o.to(DEV) for o in outs], c.size, c.J, None if flips is None else [o.to(DEV) for o in flips],
                           pc.flip_index(c), divisor=c.divisor)
    feats = pc.reference(name)[2].to(DEV) if low is None else ProjectedMaps([low.to(DEV)], c.size)
    return c, ph, feats, None if masks is None else masks.to(DEV)


def construct(gc, J, hm, feats, tags, masks):
    return pemp_amd.get_graph_constructor(gc, scoremaps=hm, features=feats, tagmaps=tags, joints_gt=None,
                                          factor_list=None, masks=masks, device=DEV, testing=True, heatmaps=None,
                                          num_joints=J).construct_graph()


def assert_same(out, ref, what, outputs=OUTPUTS):
    """Every listed output equal bit for bit (floats by their bit patterns), the first differences in the message."""
    for i in outputs:
        got, want = out[i].cpu().numpy(), ref[i].numpy()
        if i == 7 and got.shape != want.shape:
            a, b = set(map(tuple, got.tolist())), set(map(tuple, want.tolist()))
            raise AssertionError(f"{what}: detections {got.shape[0]} != {want.shape[0]}; only on the device "
                                 f"{sorted(a - b)[:6]}, only in the oracle {sorted(b - a)[:6]} (x, y, type)")
        assert got.shape == want.shape, (what, i, got.shape, want.shape)
        same = go.same_bits(got, want) if got.dtype == np.float32 else got == want
        bad = np.argwhere(~same)
        if bad.shape[0]:
            k = tuple(bad[0])
            where = ref[7][k[0]].tolist() if i in (7, 11, 14, 0) else None
            raise AssertionError(f"{what}: output {i} differs at {bad.shape[0]} places, first {k}: {got[k]!r} != "
                                 f"{want[k]!r}" + (f" (detection x, y, type {where})" if where else ""))


@pytest.mark.parametrize("name", pc.NAMES)
def test_project_maps(name):
    """pemp_project_maps (proj_pixel at every pixel of the plane, the borders included) equals the oracle's fp32
    projection bit for bit: scoremaps and tags."""
    c, ph, _, _ = device_inputs(name)
    s, t, _, _ = pc.reference(name)
    ps, pt = ph.project()
    bad = np.argwhere(~go.same_bits(ps.cpu().numpy(), s.numpy()))
    assert bad.shape[0] == 0, (name, bad.shape[0], bad[:5].tolist(), ps.cpu()[tuple(bad[0])].item(),
                               s[tuple(bad[0])].item())
    assert go.same_bits(pt.cpu().numpy(), t.numpy()).all(), name


@pytest.mark.parametrize("name", pc.NAMES)
def test_construct_graph(name):
    """scoremaps = tagmaps = the projected network outputs: detections, scores, batch index, tags, edge index, x and
    edge_attr equal the oracle on its projection. Twice: the second call takes the capacity / step entry. With
    features = ProjectedMaps, x is the oracle's upsampled map gathered at the detections (border ones included)."""
    c, ph, feats, masks = device_inputs(name)
    ref = pc.reference(name)[3]
    gc = pc.gc_config(c)
    for call in range(2):
        out = construct(gc, c.J, ph, feats, ph, masks)
        assert_same(out, ref, f"{name} call {call}")


@pytest.mark.parametrize("name", ["x2-p7-f1-mrand", "gen-p9-17rows"])
def test_profiled_call(name):
    """The call's NMS pass is the projected one, launched once, and the profiled call's outputs are the unprofiled
    ones."""
    c, ph, feats, masks = device_inputs(name)
    ref = pc.reference(name)[3]
    gc = pc.gc_config(c)
    plain = construct(gc, c.J, ph, feats, ph, masks)
    torch.cuda.synchronize()
    G._graph_hint.clear()
    G._plans.clear()
    G._cap = 512
    _lib.prof_enable("*")
    try:
        _lib.prof_report()
        out = construct(gc, c.J, ph, feats, ph, masks)
        rep = {label: n for label, (n, _) in _lib.prof_report().items()}
    finally:
        _lib.prof_enable(None)
    assert rep.get("detect_nms_projected") == 1 and "detect_nms" not in rep, rep
    assert_same(out, ref, f"{name} profiled")
    for i in OUTPUTS:
        assert torch.equal(out[i], plain[i]), (name, i)


@pytest.mark.parametrize("thr", [0.1, 0.0, pc.NEG_THR, 2.0])
def test_dense_thresholds(thr):
    """pemp_detect on dense maps under the four threshold forms (positive: one compare per pixel; zero and negative:
    two; above 1.5: no threshold, top-20), masks on: bit for bit the oracle."""
    c, hm, masks = pc.dense_inputs(thr)
    H, W = c.size
    feats = torch.from_numpy(syn.closed_form((c.B, 16, H, W), 0.25))
    tags = torch.from_numpy(syn.closed_form((c.B, c.J, H, W, 1), 0.75))
    gc = pc.gc_config(c)
    ref = restate.construct_graph(hm, feats, tags, masks, gc, c.J)
    assert ref[7].shape[0] > c.J
    if thr < 0:
        assert (ref[11] < 0).any()
    for call in range(2):
        out = construct(gc, c.J, hm.to(DEV), feats.to(DEV), tags.to(DEV), masks.to(DEV))
        assert_same(out, ref, f"dense thr {thr} call {call}")
