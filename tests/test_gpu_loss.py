"""GPU tests of the MPN training loss (pemp_amd/loss.py, csrc/loss.hip) against the plain-torch oracle
(tests/loss_oracle.py) and the reference's recorded results (tests/golden/loss_*.npz).

Bound, per tensor (test_gpu_train.py's): err <= 4 max|o32 - o64| + 2^-22 max|o64|, o32 / o64 the oracle in fp32 / fp64.
For the gradient tensors o32 is the oracle on this GPU; for each of the four scalar terms the fp32 error is the larger
of the CPU's and this GPU's (a scalar yardstick can be exact by luck). Each test prints its largest error / bound
ratio (DESIGN 7f records them).

Inputs: logits over about +-8 with +-40 and +-90 planted in every prediction (the stable softplus and the
zero-gradient ends). No node logit has |sigmoid(x) - threshold| < 1e-3, asserted in fp64, so that sel_k is the same set
in every precision; at threshold 1.0 the set ``sigmoid(x) > 1`` is empty in every precision (sigmoid <= 1, and fp32
rounds it to at most 1.0), so there the assertion is that no sigmoid exceeds 1.
"""
import ctypes

import numpy as np
import pytest
import torch

import pemp_amd
from pemp_amd import _lib, config as pcfg, loss as pl, synthetic as syn
from tests import golden_util as gu, loss_oracle as lo, train_oracle as to
from tests.test_gpu_train import FLOOR, ORDER_DEPENDENT, _KIND_NAMES, bound_ratio, tr

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
PLANTED = (40.0, -40.0, 90.0, -90.0)
SPAN = _lib.LOSS_CHUNK                      # edges of one edge block's iteration
EDGE_GRID, NODE_GRID = 1024, 64             # block caps: beyond them the blocks grid-stride


# ---- inputs -----------------------------------------------------------------------------------------------------
def _logits(g, shape):
    x = (torch.rand(shape, generator=g) * 2 - 1) * 8
    x = torch.where(x.abs() < 0.05, torch.full_like(x, 0.3), x)
    flat = x.view(-1)
    n = min(len(PLANTED), flat.numel())
    if n:
        flat[torch.randperm(flat.numel(), generator=g)[:n]] = torch.tensor(PLANTED[:n])
    return x.numpy()


def make_case(N, E, K_e, J, seed, ring=False, classes=True):
    """Random directed edges over N nodes (or the ring i <-> i + 1, E = 2 N), K_n = K_e + 1 predictions."""
    g = torch.Generator().manual_seed(seed)
    if ring:
        i = torch.arange(N)
        ei = torch.stack([torch.cat([i, (i + 1) % N]), torch.cat([(i + 1) % N, i])])
        E = 2 * N
    else:
        ei = torch.randint(0, N, (2, E), generator=g)
    a = {"edge_index": ei.numpy()}
    for k in range(K_e):
        a[f"pe{k}"] = _logits(g, (E,))
    for k in range(K_e + 1):
        a[f"pn{k}"] = _logits(g, (N,))
        if classes:
            a[f"pc{k}"] = _logits(g, (N, J))
    persons = torch.randint(0, 4, (N,), generator=g)
    labels = (torch.rand(N, generator=g) < 0.6).float()
    on = labels == 1
    a["edge_labels"] = (on[ei[0]] & on[ei[1]] & (persons[ei[0]] == persons[ei[1]])).float().numpy()
    a["label_mask"] = (torch.rand(E, generator=g) < 0.9).float().numpy()
    a["node_labels"] = labels.numpy()
    mask_node = (torch.rand(N, generator=g) < 0.9).float()
    mask_node[0] = 1.0
    a["label_mask_node"] = mask_node.numpy()
    if classes:
        a["node_classes"] = torch.randint(0, J, (N,), generator=g).numpy()
    return a


def assert_clear_of_threshold(a, th):
    k = 0
    while f"pn{k}" in a:
        s = torch.from_numpy(a[f"pn{k}"]).double().sigmoid()
        if th >= 1.0:
            assert float(s.max()) <= 1.0
        else:
            assert float((s - th).abs().min()) >= 1e-3, k
        k += 1


def n_preds(a, prefix):
    k = 0
    while f"{prefix}{k}" in a:
        k += 1
    return k


# ---- the device side -----------------------------------------------------------------------------------------------
def device_tensors(a):
    t = {k: torch.from_numpy(np.ascontiguousarray(v)).to(DEV) for k, v in a.items() if "." not in k}
    pe = [t[f"pe{k}"].requires_grad_(True) for k in range(n_preds(a, "pe"))]
    pn = [t[f"pn{k}"].requires_grad_(True) for k in range(n_preds(a, "pn"))]
    pc = [t[f"pc{k}"].requires_grad_(True) for k in range(n_preds(a, "pc"))]
    return t, pe, pn, pc


def device_run(a, opt, masks=None):
    """{"terms", "g_pe<k>", ...} as float64 arrays (loss_oracle.run's dictionary) from pemp_amd.loss.mpn_loss."""
    t, pe, pn, pc = device_tensors(a)
    total, terms = pl.mpn_loss(pe, pn, pc or None, t["edge_index"], t["edge_labels"], t["label_mask"], t["node_labels"],
                               t["label_mask_node"], t.get("node_classes"), opt, edge_masks=masks)
    assert terms.shape == (4,) and terms.dtype == torch.float32 and not terms.requires_grad
    total.backward()
    torch.cuda.synchronize()
    assert torch.equal(total.detach(), terms[3]) or (torch.isnan(total) and torch.isnan(terms[3]))
    out = {"terms": terms.cpu().double().numpy()}
    for prefix, ts in (("pe", pe), ("pn", pn), ("pc", pc)):
        for k, x in enumerate(ts):
            g = x.grad if x.grad is not None else torch.zeros_like(x)     # a logit list the call did not take
            assert g.shape == x.shape and g.dtype == torch.float32
            out[f"g_{prefix}{k}"] = g.cpu().double().numpy()
    return out


def worst_ratio(got, o64, o32_gpu, o32_cpu):
    """The largest error / bound over the four terms (each a tensor of its own) and the gradient tensors."""
    worst = ("", 0.0)
    for i, name in enumerate(("node", "edge", "class", "total")):
        g, w = got["terms"][i], o64["terms"][i]
        if np.isnan(w):
            assert np.isnan(g), name
            continue
        err32 = max(abs(o32_gpu["terms"][i] - w), abs(o32_cpu["terms"][i] - w))
        bound = 4.0 * err32 + FLOOR * abs(w)
        err = abs(g - w)
        r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if r > worst[1]:
            worst = (name, r)
    for k, w in o64.items():
        if k == "terms":
            continue
        assert got[k].shape == w.shape, k
        if np.isnan(w).any():
            assert np.array_equal(np.isnan(got[k]), np.isnan(w)), k
            continue
        r = bound_ratio(got[k], o32_gpu[k], w)
        if r > worst[1]:
            worst = (k, r)
    return worst


def check_case(tag, a, opt, th_checked=True):
    full = dict(lo.OPTIONS, **opt)
    if th_checked:
        assert_clear_of_threshold(a, full["NODE_THRESHOLD"])
    got = device_run(a, opt)
    o64 = lo.run(a, opt, torch.float64, "cpu")
    o32c = lo.run(a, opt, torch.float32, "cpu")
    o32g = lo.run(a, opt, torch.float32, "cuda:0")
    worst = worst_ratio(got, o64, o32g, o32c)
    print(f"loss {tag}: largest error/bound {worst[1]:.3f} ({worst[0]})")
    assert worst[1] <= 1.0, worst
    return got, o64


# ---- shapes --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("E", [0, 1, 63, 64, 65, 255, 256, 257, SPAN - 1, SPAN, SPAN + 1])
def test_edge_counts(E):
    """N = 41; every E around the wave, the block and one block's span (E = 0: the NaN rule, edge term 0.0)."""
    opt = dict(NODE_THRESHOLD=0.5 if E % 2 else 1.0, INCLUDE_BORDERING_NODES=bool(E % 3 == 0), EDGE_WEIGHT=1.5)
    a = make_case(41, E, 3, 17, 10 + E % 97)
    got, _ = check_case(f"N=41 E={E}", a, opt)
    if E == 0:
        assert got["terms"][1] == 0.0 and got["terms"][0] > 0


@pytest.mark.parametrize("N", [1, 64, 65, 257])
def test_node_counts_on_a_ring(N):
    opt = dict(NODE_THRESHOLD=0.5, CLASS_WEIGHT=0.5)
    check_case(f"ring N={N}", make_case(N, 0, 3, 17, 200 + N, ring=True), opt)


@pytest.mark.parametrize("K_e,J,th,border", [(1, 14, 0.5, True), (3, 17, 1.0, False), (7, 14, 0.5, False),
                                             (7, 17, 1.0, True), (3, 14, 1.0, True), (1, 17, 0.5, False)])
def test_prediction_counts_classes_thresholds(K_e, J, th, border):
    opt = dict(NODE_THRESHOLD=th, INCLUDE_BORDERING_NODES=border, NODE_WEIGHT=0.7, EDGE_WEIGHT=1.3)
    check_case(f"K_e={K_e} J={J} th={th} border={border}", make_case(41, 700, K_e, J, 300 + K_e + J), opt)


@pytest.mark.parametrize("what", ["edges", "nodes"])
def test_grid_stride(what):
    """Past the block caps (1024 edge blocks of 2048 edges, 64 node blocks of 256 nodes per prediction) the blocks
    take more than one chunk each."""
    if what == "edges":
        a = make_case(41, EDGE_GRID * SPAN + SPAN + 1, 1, 17, 400)
    else:
        a = make_case(NODE_GRID * 256 + 257, 0, 1, 17, 401, ring=True)
    check_case(f"grid stride over {what}", a, dict(NODE_THRESHOLD=0.5))


@pytest.mark.parametrize("opt", [dict(USE_FOCAL=False, NODE_USE_FOCAL=False, NODE_BCE_POS_WEIGHT=2.0,
                                      EDGE_BCE_POS_WEIGHT=3.0, NODE_THRESHOLD=0.5),
                                 dict(FOCAL_GAMMA=1.5, FOCAL_ALPHA=0.25, NODE_THRESHOLD=0.5),
                                 dict(FOCAL_GAMMA=3.0, NODE_THRESHOLD=1.0),
                                 dict(TERMS=("edge",), NODE_THRESHOLD=0.5),
                                 dict(TERMS=("node", "class"), NODE_THRESHOLD=0.5)],
                         ids=["bce", "gamma1.5", "gamma3", "edge_only", "no_edge"])
def test_kinds_gamma_and_skipped_terms(opt):
    got, _ = check_case(f"options {opt}", make_case(41, 700, 3, 17, 500), opt)
    terms = opt.get("TERMS", ("node", "edge", "class"))
    for i, name in enumerate(("node", "edge", "class")):
        if name not in terms:
            assert got["terms"][i] == 0.0
            prefix = {"node": "g_pn", "edge": "g_pe", "class": "g_pc"}[name]
            assert not any(np.any(v) for k, v in got.items() if k.startswith(prefix))


def test_no_class_term_without_node_classes():
    a = make_case(41, 300, 3, 17, 600, classes=False)
    got, _ = check_case("method-4 labels", a, dict(NODE_THRESHOLD=0.5))
    assert got["terms"][2] == 0.0


# ---- the NaN rules ---------------------------------------------------------------------------------------------
def test_one_zero_mask_zeroes_the_edge_term():
    """mask_1 all zero (node prediction 1 below the threshold everywhere, one labelled node): the edge term is exactly
    0, every edge gradient exactly 0; the node and class terms are those of the oracle."""
    a = make_case(41, 700, 3, 17, 700)
    a["node_labels"] = np.zeros(41, np.float32)
    a["node_labels"][5] = 1.0
    a["edge_labels"] = np.zeros(700, np.float32)
    a["pn1"] = -np.abs(a["pn1"])
    opt = dict(NODE_THRESHOLD=0.5)
    masks = lo.edge_masks([torch.from_numpy(a[f"pn{k}"]) for k in range(4)], torch.from_numpy(a["edge_index"]),
                          torch.from_numpy(a["label_mask"]), torch.from_numpy(a["node_labels"]), dict(lo.OPTIONS, **opt))
    assert masks[1].sum() == 0 and masks[0].sum() > 0 and masks[2].sum() > 0
    got, o64 = check_case("one zero mask", a, opt)
    assert got["terms"][1] == 0.0 and o64["terms"][1] == 0.0
    assert not any(np.any(got[f"g_pe{k}"]) for k in range(3))
    assert got["terms"][0] > 0 and got["terms"][2] > 0 and np.any(got["g_pn1"]) and np.any(got["g_pc1"])


def test_zero_node_mask_is_nan_as_in_the_reference():
    """label_mask_node all zero: the node term (and the total) NaN as in the oracle, the node gradients NaN where the
    oracle's are; the edge and class terms and their gradients under the bound."""
    a = make_case(41, 300, 3, 17, 800)
    a["label_mask_node"] = np.zeros(41, np.float32)
    got, o64 = check_case("zero node mask", a, dict(NODE_THRESHOLD=0.5))
    assert np.isnan(o64["terms"][0]) and np.isnan(got["terms"][0]) and np.isnan(got["terms"][3])
    assert np.isfinite(got["terms"][1]) and np.isfinite(got["terms"][2]) and got["terms"][2] > 0
    assert all(np.isfinite(got[f"g_pe{k}"]).all() for k in range(3))


# ---- fixtures ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", ["mpn", "multi"])
@pytest.mark.parametrize("name", gu.names("loss_"))
def test_fixture(name, variant):
    """The reference's fp64 terms and gradients (ClassMPNLossFactory / ClassMultiLossFactory) as o64."""
    meta, a = gu.load(name)
    opt = meta["variants"][variant]
    opt = dict(opt, TERMS=tuple(opt["TERMS"]))
    assert_clear_of_threshold(a, opt["NODE_THRESHOLD"])
    want = {k[len(variant) + 1:]: v for k, v in a.items() if k.startswith(variant + ".")}
    got = device_run(a, opt)
    o32c = lo.run(a, opt, torch.float32, "cpu")
    o32g = lo.run(a, opt, torch.float32, "cuda:0")
    worst = worst_ratio(got, want, o32g, o32c)
    print(f"loss fixture {name} / {variant}: largest error/bound {worst[1]:.3f} ({worst[0]})")
    assert worst[1] <= 1.0, worst
    if name == "loss_zero_mask":
        assert got["terms"][1] == 0.0 and not any(np.any(got[f"g_pe{k}"]) for k in range(meta["K_e"]))


# ---- the mask paths ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("th,border", [(0.5, False), (0.5, True), (1.0, False)])
def test_factory_masks_equal_computed_masks_bit_for_bit(th, border):
    """ClassMPNLossFactory with the masks train.py:144-150 builds (mask_node_connections on the device) against
    mpn_loss's computed masks: the same bits in every term and gradient; the logging floats are the terms."""
    a = make_case(41, SPAN + 300, 3, 17, 900)
    assert_clear_of_threshold(a, th)
    cfg = pcfg.get_config()
    cfg.merge({"MODEL": {"LOSS": {"LOSS_WEIGHTS": [1.0, 2.0, 0.5], "INCLUDE_BORDERING_NODES": border},
                         "MPN": {"NODE_THRESHOLD": th}}})
    opt = dict(NODE_THRESHOLD=th, INCLUDE_BORDERING_NODES=border, NODE_WEIGHT=1.0, EDGE_WEIGHT=2.0, CLASS_WEIGHT=0.5)
    want = device_run(a, opt)
    t, pe, pn, pc = device_tensors(a)
    masks = []
    for p in pn:
        m = pemp_amd.mask_node_connections(p.sigmoid().detach(), t["edge_index"], th, t["node_labels"],
                                           include_bordering_nodes=border)
        ref = lo.mask_node_connections(p.detach().sigmoid(), t["edge_index"], th, t["node_labels"], border)
        assert m.dtype == torch.bool and torch.equal(m, ref)
        cpu = lo.mask_node_connections(p.detach().cpu().double().sigmoid(), t["edge_index"].cpu(), th,
                                       t["node_labels"].cpu(), border)
        assert torch.equal(m.cpu(), cpu)
        masks.append(t["label_mask"] * m.float())
    factory = pemp_amd.ClassMPNLossFactory(cfg)
    assert len(masks) == len(pn) == len(pe) + 1            # the loop of train.py:144-151: one per NODE prediction
    loss, logging = factory({"edge": pe, "node": pn, "class": pc},
                            {"edge": [t["edge_labels"]] * len(pn), "node": t["node_labels"], "class": t["node_classes"]},
                            {"edge": masks, "node": t["label_mask_node"], "class": None},
                            {"edge_index": t["edge_index"]})   # train.py:154 passes the graph as a fourth argument
    loss.backward()
    torch.cuda.synchronize()
    f32 = lambda v: np.float32(v)
    assert [f32(logging[k]) for k in ("node", "edge", "class_loss", "loss")] == [f32(v) for v in want["terms"]]
    assert logging["reg"] == 0.0 and f32(loss.item()) == f32(want["terms"][3])
    for prefix, ts in (("pe", pe), ("pn", pn), ("pc", pc)):
        for k, x in enumerate(ts):
            assert np.array_equal(x.grad.cpu().double().numpy(), want[f"g_{prefix}{k}"]), (prefix, k)
    also = device_run(a, opt, masks=masks[:len(pe)])
    assert all(np.array_equal(also[k], v) for k, v in want.items())


# ---- reproducibility and capture ---------------------------------------------------------------------------------------
def test_bitwise_reproducible():
    """Two calls on the same inputs, more than one edge block and more than one node block."""
    a = make_case(300, 3 * SPAN + 77, 3, 17, 1000)
    opt = dict(NODE_THRESHOLD=0.5)
    one, two = device_run(a, opt), device_run(a, opt)
    assert set(one) == set(two)
    for k, v in one.items():
        assert np.array_equal(v, two[k]), k


def test_entries_are_capture_safe():
    """pemp_loss_fwd and pemp_loss_bwd captured into a graph and replayed once: the bits of the direct calls (no
    synchronisation or allocation hides in the entries)."""
    L = _lib.lib()
    a = make_case(300, 3 * SPAN + 77, 3, 17, 1001)
    t, pe, pn, pc = device_tensors(a)
    opt = pl.loss_options(NODE_THRESHOLD=0.5)
    rec, held = pl.build_record(opt, [p.detach() for p in pe], [p.detach() for p in pn], [p.detach() for p in pc],
                                t["edge_index"], t["edge_labels"], t["label_mask"], t["node_labels"],
                                t["label_mask_node"], t["node_classes"])
    nbytes = L.pemp_loss_workspace_size(rec.N, rec.E, rec.K_e, rec.K_n)
    one = torch.ones(1, device=DEV)

    def buffers():
        ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
        out = torch.full((_lib.LOSS_OUT,), -1.0, device=DEV)
        grads = [[torch.full_like(x, 7.0) for x in xs] for xs in held[:3]]
        arrs = [pl._ptrs(n, g) for n, g in zip((_lib.LOSS_MAXKE, _lib.LOSS_MAXKN, _lib.LOSS_MAXKN), grads)]
        return ws, out, grads, arrs

    def calls(ws, out, arrs):
        st = _lib.stream(DEV)
        _lib.check(L.pemp_loss_fwd(ctypes.byref(rec), ws.data_ptr(), nbytes, out.data_ptr(), st))
        _lib.check(L.pemp_loss_bwd(ctypes.byref(rec), out.data_ptr(), one.data_ptr(), *(ctypes.cast(x, _lib.c_p) for x in arrs),
                                   st))

    ws, out, grads, arrs = buffers()
    calls(ws, out, arrs)
    torch.cuda.synchronize()
    ws2, out2, grads2, arrs2 = buffers()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        calls(ws2, out2, arrs2)
    torch.cuda.synchronize()
    assert float(out2[3]) == -1.0                      # captured, not run
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out, out2) and float(out[3]) > 0
    for xs, ys in zip(grads, grads2):
        for x, y in zip(xs, ys):
            assert torch.equal(x, y) and not (x == 7.0).all()
    want = device_run(a, dict(NODE_THRESHOLD=0.5))
    assert np.array_equal(out[:4].cpu().double().numpy(), want["terms"])


def test_logit_written_before_backward_is_caught():
    """The backward recomputes from the logits: one written in place after the forward must not pass silently."""
    a = make_case(41, 100, 3, 17, 1101)
    t, pe, pn, pc = device_tensors(a)
    xs = [p * 1.0 for p in pe]                                   # non-leaf logits, as a model's are
    total, _ = pl.mpn_loss(xs, pn, pc, t["edge_index"], t["edge_labels"], t["label_mask"], t["node_labels"],
                           t["label_mask_node"], t["node_classes"], NODE_THRESHOLD=0.5)
    xs[1].add_(1.0)
    with pytest.raises(RuntimeError, match="inplace"):
        total.backward()
    with pytest.raises(ValueError, match="edge masks"):
        pemp_amd.ClassMPNLossFactory(pcfg.get_config())(
            {"edge": pe, "node": pn, "class": None}, {"edge": [t["edge_labels"]] * 4, "node": t["node_labels"]},
            {"edge": [t["label_mask"]] * 2, "node": t["label_mask_node"]})


def test_input_checks_on_the_device():
    a = make_case(41, 100, 3, 17, 1100)
    t, pe, pn, pc = device_tensors(a)
    rest = (t["edge_labels"], t["label_mask"], t["node_labels"], t["label_mask_node"], t["node_classes"])
    with pytest.raises(ValueError, match="shape"):
        pl.mpn_loss(pe, pn, pc, t["edge_index"][:, :50], *rest)
    with pytest.raises(TypeError, match="int64"):
        pl.mpn_loss(pe, pn, pc, t["edge_index"].int(), *rest)
    with pytest.raises(RuntimeError):
        pl.mpn_loss(pe, pn, pc, t["edge_index"], t["edge_labels"].cpu(), *rest[1:])
    with pytest.raises(ValueError, match="node prediction"):
        pl.mpn_loss(pe, pn[:2], pc[:2], t["edge_index"], *rest)
    with pytest.raises(ValueError, match="class predictions"):
        pl.mpn_loss(pe, pn, pc[:2], t["edge_index"], *rest)


# ---- one whole training step ---------------------------------------------------------------------------------------
def _labelled_graph():
    """A C2-sized graph (one 160 x 160 image like the gc_c2_like fixture's, nine people) with the constructor's labels
    (EDGE_LABEL_METHOD 6) from synthetic ground truth."""
    from tests.test_labels_cpu import label_config
    B, J, H, W, C = 1, 17, 160, 160, 128
    hm, gt, fac = syn.make_labelled_heatmaps(5, B, J, H, W, 9)
    cfg = label_config(dict(graph="fully", method=6, use_neighbours=True, with_background=False,
                            matching_radius=0.5, inclusion_radius=0.75))
    feats = torch.from_numpy(syn.closed_form((B, C, H, W), gu.FEATURE_SALT)).to(DEV)
    tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), gu.TAG_SALT)).to(DEV)
    return pemp_amd.get_graph_constructor(cfg, scoremaps=torch.from_numpy(hm).to(DEV), features=feats, tagmaps=tags,
                                          joints_gt=torch.from_numpy(gt), factor_list=torch.from_numpy(fac), masks=None,
                                          device=DEV, testing=True, heatmaps=None, num_joints=J).construct_graph()


def _module_form_step(mcfg, sd, out15, opt, monkeypatch):
    """test_gpu_train.module_form_step with loss_oracle.mpn_loss in place of the fixture loss: the torch-operator
    form through the model's own modules on this GPU (the second fp32 evaluation of the ORDER_DEPENDENT tensors)."""
    monkeypatch.setattr(tr, "seg_aggregate", lambda msgs, scores, plan, kind: to.seg_aggregate(
        msgs, scores, plan.dst, plan.type_src, plan.N, plan.T, _KIND_NAMES[kind]))
    monkeypatch.setattr(tr, "gather_pair", lambda x, plan: to.gather_pair(x, plan.src, plan.dst))
    model = pemp_amd.get_mpn_model(mcfg)
    model.load_state_dict(sd)
    model.to(DEV).train()
    x, ea = out15[0].detach().requires_grad_(True), out15[1].detach().requires_grad_(True)
    pe, pn, pc, _ = model(x, ea, out15[2], node_types=out15[7][:, 2])
    loss, _ = lo.mpn_loss(pe, pn, pc, out15[2], out15[3], out15[8], out15[4], out15[9], out15[5], opt)
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    grads = {"x": x.grad, "edge_attr": ea.grad}
    grads.update({k: p.grad for k, p in model.named_parameters()})
    return to.collect(pe, pn, pc, loss, {}, grads)


def _oracle_step(sd_in, cfg, out15, opt, dtype, device):
    """train_oracle.step with loss_oracle.mpn_loss in place of the fixture loss."""
    sd = {}
    for k, v in sd_in.items():
        v = torch.as_tensor(v).detach().to(device)
        sd[k] = v.to(dtype).requires_grad_(not k.endswith(("running_mean", "running_var"))) \
            if v.is_floating_point() else v.clone()
    x = out15[0].detach().to(device=device, dtype=dtype).requires_grad_(True)
    ea = out15[1].detach().to(device=device, dtype=dtype).requires_grad_(True)
    ei, types = out15[2].to(device), out15[7][:, 2].to(device)
    taps = []
    pe, pn, pc, stats = to.train_forward(sd, cfg, x, ea, ei, types, to.TORCH_OPS, taps)
    lab = [out15[i].to(device) for i in (3, 8, 4, 9, 5)]
    loss, terms = lo.mpn_loss(pe, pn, pc, ei, lab[0], lab[1], lab[2], lab[3], lab[4], opt)
    loss.backward()
    grads = {"x": x.grad, "edge_attr": ea.grad}
    grads.update({k: v.grad for k, v in sd.items() if v.is_floating_point() and v.requires_grad})
    res = to.collect(pe, pn, pc, loss, stats, grads)
    res["terms"] = terms.detach().cpu().double().numpy()
    res["aux.score_grad_count"] = np.float64(sum(t.numel() for t in taps))
    res["aux.score_grad_abs_sum"] = np.float64(sum(float(t.grad.abs().sum()) for t in taps))
    res["aux.pn"] = [p.detach().cpu().double() for p in pn]
    return res


@pytest.fixture
def rocblas_dense():
    """torch's dense layers on rocBLAS while the test runs. With hipBLASLt (torch's default here) the same process
    started again picks other GEMM kernels for the per-type bucket shapes, and the whole step then reads differently
    from run to run (six fresh processes: 0.27, 0.34, 0.66, 0.66, 21.5, 21.5, the last on one per-type message MLP's
    weight gradient, with the torch form through the modules agreeing with the model to three digits); on rocBLAS
    the kernels, and with them the step's figures, are the same in every process. The dense layers are torch's in
    the model and in both yardsticks alike, so the setting is the same on both sides of the comparison."""
    prev = torch.backends.cuda.preferred_blas_library()
    torch.backends.cuda.preferred_blas_library("hipblas")
    yield
    torch.backends.cuda.preferred_blas_library(prev)


def test_whole_training_step(monkeypatch, rocblas_dense):
    """Published attention model, STEPS 3, AUX_LOSS_STEPS 2: construct labels -> forward -> MPNLoss -> backward,
    every logit, term and gradient against train_oracle + loss_oracle in fp64 under test_gpu_train.py's per-tensor
    bound (the fp32 yardstick is the same oracle on this GPU; its two ORDER_DEPENDENT tensors take the larger of the
    functional and the through-the-modules evaluation, the analytically zero attention-bias gradient
    train_oracle.residue_bound). torch's dense layers run on rocBLAS throughout (rocblas_dense)."""
    out15 = _labelled_graph()
    N, E = out15[0].shape[0], out15[2].shape[1]
    assert 100 <= N <= 250 and out15[3].sum() > 0 and out15[8].sum() > 0 and out15[5] is not None
    mcfg = pcfg.published_mpn_config(17, 3, "attn")
    mcfg.AUX_LOSS_STEPS = 2
    cfg = pcfg.get_config()
    cfg.MODEL.MPN = mcfg
    cfg.merge({"MODEL": {"LOSS": {"NAME": ["edge", "node", "class"], "EDGE_WEIGHT": 2.0}}})
    th = 1.0                                                       # the published NODE_THRESHOLD
    assert cfg.MODEL.MPN.NODE_THRESHOLD == th
    model = pemp_amd.get_mpn_model(mcfg)
    sd = syn.closed_form_state_dict(model, 9.5)
    model.load_state_dict(sd)
    model.to(DEV).train()
    loss_fn = pemp_amd.MPNLoss(cfg)
    opt = dict(NODE_THRESHOLD=th, EDGE_WEIGHT=2.0)
    assert {k: loss_fn.options[k] for k in opt} == opt and loss_fn.options["TERMS"] == ("node", "edge", "class")
    x, ea = out15[0].detach().requires_grad_(True), out15[1].detach().requires_grad_(True)
    preds = model(x, ea, out15[2], node_types=out15[7][:, 2])
    assert (len(preds[0]), len(preds[1]), len(preds[2])) == (3, 4, 4)
    total, terms = loss_fn(out15, preds)
    total.backward()
    torch.cuda.synchronize()
    stats = {k: v for k, v in model.state_dict().items()
             if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    grads = {"x": x.grad, "edge_attr": ea.grad}
    grads.update({k: p.grad for k, p in model.named_parameters()})
    got = to.collect(preds[0], preds[1], preds[2], total, stats, grads)
    o64 = _oracle_step(sd, mcfg, out15, opt, torch.float64, "cpu")
    o32 = _oracle_step(sd, mcfg, out15, opt, torch.float32, "cuda:0")
    o32b = _module_form_step(mcfg, sd, out15, opt, monkeypatch)
    assert_clear_of_threshold({f"pn{k}": p.numpy() for k, p in enumerate(o64["aux.pn"])}, th)
    worst = ("", 0.0)
    for i, name in enumerate(("node", "edge", "class", "total")):
        w = o64["terms"][i]
        bound = 4.0 * abs(o32["terms"][i] - w) + FLOOR * abs(w)
        r = abs(float(terms[i]) - w) / bound
        if r > worst[1]:
            worst = ("term." + name, r)
    for k, want in o64.items():
        if k.startswith("aux.") or k == "terms":
            continue
        if k.endswith("num_batches_tracked"):
            assert np.array_equal(got[k], want), k
            continue
        have = got.get(k)
        if have is None:
            assert k.startswith("grad.") and not np.any(want), k
            continue
        assert have.shape == want.shape, k
        err = float(np.abs(have - want).max()) if want.size else 0.0
        if k == to.ATTN_BIAS:
            bound = to.residue_bound(o64, 2.0 ** -24)
        else:
            bound = to.error_bound(o32, o64, k)
            if k in ORDER_DEPENDENT:
                bound = max(bound, to.error_bound(o32b, o64, k))
        r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if r > 0.5 and k != to.ATTN_BIAS:       # the figures behind a large ratio: the two fp32 evaluations' own errors
            print(f"whole step: {k} error {err:.2e} of max {np.abs(want).max():.2e}; torch form "
                  f"{np.abs(o32[k] - want).max():.2e} (functional), {np.abs(o32b[k] - want).max():.2e} (through the modules)")
        if r > worst[1]:
            worst = (k, r)
    print(f"whole step N={N} E={E}: terms {terms.tolist()}, largest error/bound {worst[1]:.3f} ({worst[0]})")
    assert worst[1] <= 1.0, worst
    assert all(k in o64 for k in got)
