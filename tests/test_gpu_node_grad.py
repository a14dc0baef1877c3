"""The differentiable node features on the device (pemp_amd/node_gather.py, csrc/node_grad.hip): the planted operator
cases of tests/node_grad_ref.py, the gradient through construct_graph for dense features and for the sparse
feature_gather path, the paths that need no gradient, and one whole training step. The dense backward bit for bit
against a numpy loop in node order; the conv backward against torch's fp64 autograd under the derived bound."""
import contextlib
import copy

import numpy as np
import pytest
import torch

import pemp_amd
from pemp_amd import _lib, config as pcfg, synthetic as syn
from pemp_amd.graph_constructor import NaiveGraphConstructor as G
from tests import graph_options as go, node_grad_ref as nr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
WORST = {}       # tensor name -> the largest error-to-bound ratio seen (printed by every test that has one)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def note(name, r, what):
    WORST[name] = max(WORST.get(name, 0.0), r)
    print(f"node_grad gpu {what}: {name} error/bound {r:.3f} (largest so far {WORST[name]:.3f})")
    assert r <= 1.0, (what, name, r)


def on_stream(stream):
    torch.cuda.synchronize()
    return torch.cuda.stream(stream) if stream is not None else contextlib.nullcontext()


# ---- planted operator cases ----------------------------------------------------------------------------------------
def run_dense(feats, g, jd, bi, stream=None):
    f = dev(feats).requires_grad_(True)
    jd_d, bi_d, g_d = dev(jd), dev(bi), dev(g)
    with on_stream(stream):
        x = pemp_amd.gather_nodes(f, jd_d, bi_d)
        assert x.grad_fn is not None
        x.backward(g_d)
    torch.cuda.synchronize()
    return host(x), host(f.grad)


@pytest.mark.parametrize("set_name", nr.NODE_SETS)
@pytest.mark.parametrize("C", nr.DENSE_C)
def test_dense_planted(C, set_name):
    jd, bi = nr.nodes(set_name)
    feats, g = nr.values((nr.B, C, nr.H, nr.W), C), nr.values((jd.shape[0], C), C + 1)
    want = nr.dense_backward(g, jd, bi, feats.shape)
    x, df = run_dense(feats, g, jd, bi)
    assert nr.same_bits(x, nr.dense_forward(feats, jd, bi))
    assert nr.same_bits(df, want), np.argwhere(df != want)[:5]
    assert not df[1].any()                                   # the empty image
    x2, df2 = run_dense(feats, g, jd, bi)
    assert nr.same_bits(df2, df) and nr.same_bits(x2, x)     # run twice
    x3, df3 = run_dense(feats, g, jd, bi, torch.cuda.Stream(DEV))
    assert nr.same_bits(df3, df) and nr.same_bits(x3, x)     # another launch stream


def run_conv(d, needs=(True, True, True), stream=None):
    Cout, Cin, k = d["weight"].shape[:3]
    conv = torch.nn.Conv2d(Cin, Cout, k, padding=d["pad"]).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(dev(d["weight"]))
        conv.bias.copy_(dev(d["bias"]))
    raw = dev(d["raw"]).requires_grad_(needs[0])
    conv.weight.requires_grad_(needs[1])
    conv.bias.requires_grad_(needs[2])
    jd_d, bi_d, g_d = dev(d["jd"]), dev(d["bi"]), dev(d["g"])
    with on_stream(stream):
        x = pemp_amd.gather_nodes_conv(raw, conv, jd_d, bi_d)
        x.backward(g_d)
    torch.cuda.synchronize()
    return host(x), host(raw.grad), host(conv.weight.grad), host(conv.bias.grad)


CONV_CASES = [(c, s) for c in nr.CONVS for s in nr.NODE_SETS]


@pytest.mark.parametrize("case,set_name", CONV_CASES, ids=[f"{c[0]}-{c[1]}-k{c[2]}p{c[3]}-{s}" for c, s in CONV_CASES])
def test_conv_planted(case, set_name):
    d = nr.conv_inputs(case, set_name)
    ref = nr.conv_reference(d)
    got = run_conv(d)
    what = f"{case} {set_name}"
    for i, name in enumerate(("x", "draw", "dW", "db")):
        note(name, nr.ratio(got[i], *ref[name]), what)
    assert not got[1][1].any()                               # the empty image
    again = run_conv(d)
    other = run_conv(d, stream=torch.cuda.Stream(DEV))
    for a, b, c in zip(got, again, other):
        assert nr.same_bits(a, b) and nr.same_bits(a, c)
    for which in range(3):                                   # one gradient requested: its bits, and no other
        needs = tuple(i == which for i in range(3))
        one = run_conv(d, needs)
        assert nr.same_bits(one[0], got[0])
        for i in range(3):
            if needs[i]:
                assert nr.same_bits(one[1 + i], got[1 + i]), (what, which)
            else:
                assert one[1 + i] is None, (what, which, i)


def test_conv_without_bias_and_plan_reuse():
    d = nr.conv_inputs(nr.CONVS[1], "n257")
    Cout, Cin, k = d["weight"].shape[:3]
    conv = torch.nn.Conv2d(Cin, Cout, k, padding=d["pad"], bias=False).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(dev(d["weight"]))
    raw, jd, bi = dev(d["raw"]).requires_grad_(True), dev(d["jd"]), dev(d["bi"])
    plan = pemp_amd.PixelPlan(jd, bi, nr.B, raw.shape[2], raw.shape[3], k, d["pad"])
    x = pemp_amd.gather_nodes_conv(raw, conv, jd, bi, plan=plan)
    x.backward(dev(d["g"]))
    full = run_conv(d)
    assert nr.same_bits(host(raw.grad), full[1]) and nr.same_bits(host(conv.weight.grad), full[2])
    with pytest.raises(ValueError, match="PixelPlan was made for"):
        pemp_amd.gather_nodes_conv(raw, conv, jd[:5], bi[:5], plan=plan)


def test_edit_before_backward_is_caught():
    d = nr.conv_inputs(nr.CONVS[0], "base")
    f, jd, bi = dev(nr.values((nr.B, 24, nr.H, nr.W), 3)).requires_grad_(True), dev(d["jd"]), dev(d["bi"])
    x = pemp_amd.gather_nodes(f, jd, bi)
    jd[0, 0] = 1
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        x.sum().backward()


# ---- through the constructor ---------------------------------------------------------------------------------------
J, GB, GH, GW = 4, 2, 48, 250


@pytest.fixture
def fresh(monkeypatch):
    """A callable that puts the constructor's class-wide state back to a first call's (no hints, no plans); the state
    it found goes back after the test."""
    def reset():
        monkeypatch.setattr(G, "_cap", 512)
        monkeypatch.setattr(G, "_graph_hint", {})
        monkeypatch.setattr(G, "_plans", {})
    reset()
    return reset


def planted_maps():
    """[2, 4, 48, 250] planted peaks (go.lattice_plane, 12 units per plane): types 0 and 1 of image 0 are the same
    plane, so their detections share pixels."""
    hm = np.zeros((GB, J, GH, GW), np.float32)
    for b in range(GB):
        for j in range(J):
            hm[b, j] = go.lattice_plane(GH, GW, 10, 0 if (b, j) in ((0, 0), (0, 1)) else 3 * b + j)
    return dev(hm)


def construct(graph, feats, hm=None):
    gc = pcfg.inference_gc_config(graph, 3, False)
    return pemp_amd.get_graph_constructor(gc, scoremaps=planted_maps() if hm is None else hm, features=feats,
                                          tagmaps=None, joints_gt=None, factor_list=None, masks=None, device=DEV,
                                          testing=True, heatmaps=None, num_joints=J).construct_graph()


def profiled(fn):
    _lib.prof_enable("*")
    try:
        _lib.prof_report()
        out = fn()
        rep = _lib.prof_report()
    finally:
        _lib.prof_enable(None)
    return out, {label: n for label, (n, _) in rep.items()}


def shared_pixels(out):
    pix = torch.cat([out[12][:, None], out[7][:, :2]], 1).cpu().numpy()
    return pix.shape[0] - np.unique(pix, axis=0).shape[0]


@pytest.mark.parametrize("graph", ["fully", "knn", "feature_knn"])
def test_dense_features_through_the_constructor(graph, fresh):
    """x carries a grad_fn, keeps the bits of the call without grad, and (x c).sum().backward() puts the node-order
    sum on the caller's own tensor; the second fully call of a shape takes the batch-step entry."""
    C = 128
    feats = syn.closed_form((GB, C, GH, GW), 0.25)
    base, rep0 = profiled(lambda: construct(graph, dev(feats)))
    assert base[0].grad_fn is None and base[0].shape[0] > 40 and shared_pixels(base) >= 5
    cw = nr.values(tuple(base[0].shape), 11)
    want = nr.dense_backward(cw, host(base[7]), host(base[12]), feats.shape)
    for call in range(2 if graph == "fully" else 1):
        if call == 0:
            fresh()
        leaf = dev(feats).requires_grad_(True)
        out, rep = profiled(lambda: construct(graph, leaf))
        assert rep == rep0 or call == 1, (rep, rep0)        # the forward is the launches of the call without grad
        if call == 1:
            assert G._plans
        assert out[0].grad_fn is not None
        for i in (0, 1, 2, 7, 11, 12):
            assert torch.equal(out[i].detach(), base[i]), (graph, call, i)
        (out[0] * dev(cw)).sum().backward()
        assert nr.same_bits(host(leaf.grad), want), (graph, call)


def test_gradient_arrives_on_a_host_tensor_of_another_dtype(fresh):
    """The constructor's .to(device) and .float() stay torch ops in the chain: a float64 CPU leaf gets its gradient."""
    feats = syn.closed_form((GB, 24, GH, GW), 0.5)
    leaf = torch.from_numpy(feats).double().requires_grad_(True)
    out = construct("fully", leaf)
    cw = nr.values(tuple(out[0].shape), 12)
    (out[0] * dev(cw)).sum().backward()
    want = nr.dense_backward(cw, host(out[7]), host(out[12]), feats.shape)
    assert leaf.grad.dtype == torch.float64 and leaf.grad.device.type == "cpu"
    assert np.array_equal(leaf.grad.numpy(), want.astype(np.float64))


def make_conv(Cin, Cout, salt, grad=True):
    conv = torch.nn.Conv2d(Cin, Cout, 3, padding=1).to(DEV)
    with torch.no_grad():
        conv.weight.copy_(dev(nr.values((Cout, Cin, 3, 3), salt) * np.float32(0.25)))
        conv.bias.copy_(dev(nr.values((Cout,), salt + 1)))
    for p in conv.parameters():
        p.requires_grad_(grad)
    return conv


@pytest.mark.parametrize("graph", ["fully", "knn"])
def test_sparse_conv_through_the_constructor(graph, fresh):
    """ProjectedMaps(raw, (H, W), gather=conv): conv.weight.grad, conv.bias.grad and raw.grad against the fp64
    reference of the dense conv; the second fully call of a shape takes the capacity build."""
    Cin, Cout = 16, 128
    raw_h = syn.closed_form((GB, Cin, GH, GW), 0.75)
    with torch.no_grad():
        base, rep0 = profiled(lambda: construct(graph, pemp_amd.ProjectedMaps(dev(raw_h), (GH, GW),
                                                                               gather=make_conv(Cin, Cout, 5))))
    assert base[0].grad_fn is None and rep0.get("gather_projected_conv") == 1
    cw = nr.values(tuple(base[0].shape), 13)
    conv0 = make_conv(Cin, Cout, 5)
    d = dict(raw=raw_h, weight=host(conv0.weight), bias=host(conv0.bias), g=cw, jd=host(base[7]), bi=host(base[12]),
             k=3, pad=1)
    ref = nr.conv_reference(d)
    for call in range(2 if graph == "fully" else 1):
        if call == 0:
            fresh()
        conv, raw = make_conv(Cin, Cout, 5), dev(raw_h).requires_grad_(True)
        out, rep = profiled(lambda: construct(graph, pemp_amd.ProjectedMaps(raw, (GH, GW), gather=conv)))
        assert rep == rep0 or call == 1, (rep, rep0)
        assert out[0].grad_fn is not None
        for i in (0, 1, 2, 7, 11, 12):
            assert torch.equal(out[i].detach(), base[i]), (graph, call, i)
        (out[0] * dev(cw)).sum().backward()
        what = f"constructor {graph} call {call}"
        note("x", nr.ratio(host(out[0]), *ref["x"]), what)
        note("draw", nr.ratio(host(raw.grad), *ref["draw"]), what)
        note("dW", nr.ratio(host(conv.weight.grad), *ref["dW"]), what)
        note("db", nr.ratio(host(conv.bias.grad), *ref["db"]), what)


def test_projected_maps_without_a_conv_take_the_dense_backward(fresh):
    feats = syn.closed_form((GB, 24, GH, GW), 0.5)
    leaf = dev(feats).requires_grad_(True)
    out = construct("fully", pemp_amd.ProjectedMaps(leaf, (GH, GW)))
    assert out[0].grad_fn is not None
    cw = nr.values(tuple(out[0].shape), 14)
    (out[0] * dev(cw)).sum().backward()
    assert nr.same_bits(host(leaf.grad), nr.dense_backward(cw, host(out[7]), host(out[12]), feats.shape))


@pytest.mark.parametrize("graph", ["fully", "knn"])
def test_paths_that_need_no_gradient_are_unchanged(graph, fresh):
    """Without a required gradient and under torch.no_grad(): no grad_fn, and the launches of the same call with
    plain tensors."""
    feats = dev(syn.closed_form((GB, 128, GH, GW), 0.25))
    raw = dev(syn.closed_form((GB, 16, GH, GW), 0.75))
    plain, rep_plain = profiled(lambda: construct(graph, feats))
    fresh()
    with torch.no_grad():
        quiet, rep_quiet = profiled(lambda: construct(graph, feats.clone().requires_grad_(True)))
    assert plain[0].grad_fn is None and quiet[0].grad_fn is None and not quiet[0].requires_grad
    assert rep_quiet == rep_plain and torch.equal(quiet[0], plain[0])
    assert not any(label.startswith("node_") for label in rep_plain)
    fresh()
    frozen, rep_frozen = profiled(lambda: construct(graph, pemp_amd.ProjectedMaps(raw, (GH, GW),
                                                                                 gather=make_conv(16, 128, 5, False))))
    fresh()
    with torch.no_grad():
        quiet, rep_quiet = profiled(lambda: construct(graph, pemp_amd.ProjectedMaps(
            raw.clone().requires_grad_(True), (GH, GW), gather=make_conv(16, 128, 5))))
    assert frozen[0].grad_fn is None and quiet[0].grad_fn is None
    assert rep_quiet == rep_frozen and torch.equal(quiet[0], frozen[0])
    fresh()
    two = [dev(syn.closed_form((GB, 16, GH // 2, GW // 2), s)) for s in (0.1, 0.2)]       # projecting, as today
    out = construct(graph, pemp_amd.ProjectedMaps(two, (GH, GW), gather=make_conv(16, 128, 5, False)))
    assert out[0].grad_fn is None and out[0].shape[1] == 128


def test_refusals_when_a_gradient_is_required():
    """A map that requires a gradient cannot be projected (more than one map, another size): refused. With only the
    conv's parameters requiring one, the projecting call runs as it always has and x carries no gradient."""
    conv = make_conv(16, 128, 5)
    two = [dev(syn.closed_form((GB, 16, GH, GW), s)).requires_grad_(True) for s in (0.1, 0.2)]
    half = dev(syn.closed_form((GB, 16, GH // 2, GW // 2), 0.3))
    with pytest.raises(NotImplementedError, match="2 maps"):
        construct("fully", pemp_amd.ProjectedMaps(two, (GH, GW), gather=conv))
    with pytest.raises(NotImplementedError, match="does not project"):
        construct("fully", pemp_amd.ProjectedMaps(half.clone().requires_grad_(True), (GH, GW), gather=conv))
    with pytest.raises(NotImplementedError, match="does not project"):
        construct("fully", pemp_amd.ProjectedMaps(half.clone().requires_grad_(True), (GH, GW)))
    out = construct("fully", pemp_amd.ProjectedMaps(half, (GH, GW), gather=conv))
    assert out[0].grad_fn is None and not out[0].requires_grad


# ---- one whole step ------------------------------------------------------------------------------------------------
@pytest.fixture
def rocblas_dense():
    """torch's dense layers on rocBLAS while the test runs, as tests/test_gpu_loss.py::test_whole_training_step."""
    prev = torch.backends.cuda.preferred_blas_library()
    torch.backends.cuda.preferred_blas_library("hipblas")
    yield
    torch.backends.cuda.preferred_blas_library(prev)


def whole_step():
    """Sparse features -> construct_graph with joints_gt -> model.train() -> MPNLoss -> backward: the conv, raw, the x
    of the graph and the gradient of x a hook saw."""
    from tests.test_labels_cpu import label_config
    B, Jn, H, W, Cin = 1, 17, 160, 160, 48
    hm, gt, fac = syn.make_labelled_heatmaps(5, B, Jn, H, W, 9)
    gcfg = label_config(dict(graph="fully", method=6, use_neighbours=True, with_background=False, matching_radius=0.5,
                             inclusion_radius=0.75))
    conv = make_conv(Cin, 128, 21)
    raw = dev(syn.closed_form((B, Cin, H, W), 0.3)).requires_grad_(True)
    out15 = pemp_amd.get_graph_constructor(gcfg, scoremaps=dev(hm), features=pemp_amd.ProjectedMaps(raw, (H, W), gather=conv),
                                           tagmaps=None, joints_gt=torch.from_numpy(gt),
                                           factor_list=torch.from_numpy(fac), masks=None, device=DEV, testing=True,
                                           heatmaps=None, num_joints=Jn).construct_graph()
    mcfg = pcfg.published_mpn_config(Jn, 3, "attn")
    mcfg.AUX_LOSS_STEPS = 2
    cfg = pcfg.get_config()
    cfg.MODEL.MPN = mcfg
    cfg.merge({"MODEL": {"LOSS": {"NAME": ["edge", "node", "class"]}}})
    model = pemp_amd.get_mpn_model(mcfg)
    model.load_state_dict(syn.closed_form_state_dict(model, 9.5))
    model.to(DEV).train()
    seen = []
    out15[0].register_hook(lambda g: seen.append(g.detach().clone()))
    preds = model(out15[0], out15[1], out15[2], node_types=out15[7][:, 2])
    total, _ = pemp_amd.MPNLoss(cfg)(out15, preds)
    total.backward()
    torch.cuda.synchronize()
    assert len(seen) == 1
    return conv, raw, out15, seen[0]


def test_whole_training_step(fresh, rocblas_dense):
    conv, raw, out15, gx = whole_step()
    N = out15[0].shape[0]
    assert out15[0].grad_fn is not None and 100 <= N <= 250 and out15[3].sum() > 0
    wg = conv.weight.grad
    assert wg is not None and bool(torch.isfinite(wg).all()) and bool(wg.abs().sum() > 0)
    assert conv.bias.grad is not None and raw.grad is not None and bool(torch.isfinite(raw.grad).all())
    conv2, raw2 = copy.deepcopy(conv), raw.detach().clone().requires_grad_(True)
    for p in conv2.parameters():
        p.grad = None
    x2 = pemp_amd.gather_nodes_conv(raw2, conv2, out15[7], out15[12])
    assert torch.equal(x2.detach(), out15[0].detach())
    x2.backward(gx)
    assert torch.equal(conv2.weight.grad, wg) and torch.equal(conv2.bias.grad, conv.bias.grad)
    assert torch.equal(raw2.grad, raw.grad)
    fresh()
    conv3, raw3, out3, gx3 = whole_step()                     # a fresh run of the whole step
    assert torch.equal(gx3, gx) and torch.equal(conv3.weight.grad, wg) and torch.equal(conv3.bias.grad, conv.bias.grad)
    assert torch.equal(raw3.grad, raw.grad)
    print(f"node_grad gpu whole step N={N}: |dW| sum {float(wg.abs().sum()):.4g}, |x.grad| sum {float(gx.abs().sum()):.4g}")
