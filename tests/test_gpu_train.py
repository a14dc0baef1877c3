"""GPU tests of the training mode (mpn/train.py, csrc/train.hip): the three graph operators through their autograd
Functions against the plain-torch oracle (tests/train_oracle.py), one training step of the whole model against the
fp64 oracle for every tests/golden/train_*.npz and the C2-sized graph, bitwise reproducibility, and that the eval
path did not move.

Error bound, per tensor (operators and model): 4 * max|oracle_fp32 - oracle_fp64| + 2^-22 * max|oracle_fp64|. The
fp32 yardstick is the torch-operator form (on the CPU for the operators, on this GPU for the model, where it shares
the GEMM library with the code under test). The factor 4 covers a different but fixed summation order and exp; the
floor is 2 ulp at the tensor's scale, for tensors the yardstick happens to compute exactly. Two kinds of tensor of
the model need a word more, given where they are used: two gradients whose fp32 error in torch's own dense kernels
differs from evaluation to evaluation (ORDER_DEPENDENT) and the analytically zero gradient of attn_net.0.bias.
Each test prints its largest error / bound ratio (DESIGN 7e records them)."""
import functools

import numpy as np
import pytest
import torch

import pemp_amd
from pemp_amd import config as pcfg, synthetic as syn
from pemp_amd.mpn import train as tr
from tests import golden_util as gu, train_oracle as to

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
FLOOR = 2.0 ** -22
N_OPS = 41
SEG_SIZES = (0, 1, 2, 63, 64, 65, 130, 257)


def bound_ratio(got, o32, o64):
    """max|got - o64| / (4 max|o32 - o64| + 2^-22 max|o64|)."""
    got, o32, o64 = (np.asarray(t, np.float64) for t in (got, o32, o64))
    if not o64.size:
        return 0.0
    bound = 4.0 * np.abs(o32 - o64).max() + FLOOR * np.abs(o64).max()
    err = np.abs(got - o64).max()
    return float(err / bound) if bound > 0 else (0.0 if err == 0 else float("inf"))


# ---- operators -----------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def op_graph(T):
    """N = 41, E ~ 3000: (target, type) segments of exactly 0, 1, 2, 63, 64, 65, 130 and 257 edges (targets 0..7);
    segment 0 empty, segment N T - 1 not; node 10 has no incoming edge, node 11 no outgoing one, type 5 is never a
    source type. Multi-edges are allowed. Edge order shuffled."""
    g = torch.Generator().manual_seed(100 + T)
    N = N_OPS
    allowed = [t for t in range(17) if t != 5]
    types = torch.tensor([allowed[n % 16] for n in range(N)])
    types[N - 1] = 16
    types[12] = 16                                              # a source of the last segment's type
    seg_type = [0, 2, 3, 4, 6, 7, 8, 9] if T > 1 else [0] * 8

    def sources(t, k):
        pool = torch.tensor([n for n in range(N) if n != 11 and (T == 1 or int(types[n]) == t)])
        return pool[torch.randint(0, len(pool), (k,), generator=g)]

    src, dst = [], []
    for n, (t, k) in enumerate(zip(seg_type, SEG_SIZES)):
        src.append(sources(t, k))
        dst.append(torch.full((k,), n))
    if T > 1:                                                   # node 0 is reached, but not from type 0
        src.append(sources(1, 5))
        dst.append(torch.zeros(5, dtype=torch.int64))
    src.append(sources(16, 3))                                  # the last segment (N - 1, T - 1)
    dst.append(torch.full((3,), N - 1))
    k = 3000 - sum(len(s) for s in src)
    rs = torch.tensor([n for n in range(N) if n != 11])[torch.randint(0, N - 1, (k,), generator=g)]
    rd = torch.randint(12, N - 1, (k,), generator=g)            # targets 12..39: the sized segments stay exact
    src.append(rs)
    dst.append(rd)
    src, dst = torch.cat(src), torch.cat(dst)
    p = torch.randperm(len(src), generator=g)
    ei = torch.stack([src[p], dst[p]])
    tsrc = types[ei[0]] if T > 1 else torch.zeros_like(ei[0])
    seg = ei[1] * T + tsrc
    cnt = torch.bincount(seg, minlength=N * T)
    assert [int(cnt[n * T + t]) for n, t in enumerate(seg_type)] == list(SEG_SIZES)
    assert cnt[0] == 0 and cnt[-1] > 0 and not (ei[1] == 10).any() and not (ei[0] == 11).any() and not (tsrc == 5).any()
    E = ei.shape[1]
    # distinct values (no ties among the non-zero entries); about a third of the messages are zeros after the ReLU
    raw = (torch.randperm(E * 64, generator=g).float() / (E * 64) - 0.3).view(E, 64)
    scores = (torch.randperm(E, generator=g).float() / E - 0.5) * 6
    w_out = torch.from_numpy(syn.closed_form((N * T, 64), 0.11))
    return dict(N=N, T=T, E=E, ei=ei, types=types, tsrc=tsrc, raw=raw, scores=scores, w_out=w_out)


def oracle_aggr(G, kind, dtype):
    raw = G["raw"].clone().to(dtype).requires_grad_(True)
    sc = G["scores"].clone().to(dtype).requires_grad_(True)
    out = to.seg_aggregate(torch.relu(raw), sc if kind == "attn" else None, G["ei"][1], G["tsrc"], G["N"], G["T"], kind)
    (out * G["w_out"].to(dtype)).sum().backward()
    return out.detach(), raw.grad, (sc.grad if kind == "attn" else None)


def device_aggr(G, kind):
    plan = tr.build_plan(G["ei"].to(DEV), G["types"].to(DEV), G["N"], G["T"])
    raw = G["raw"].to(DEV).requires_grad_(True)
    sc = G["scores"].to(DEV).requires_grad_(True)
    out = tr.seg_aggregate(torch.relu(raw), sc if kind == "attn" else None, plan, kind)
    (out * G["w_out"].to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return out.detach().cpu(), raw.grad.cpu(), (sc.grad.cpu() if kind == "attn" else None)


@pytest.mark.parametrize("T", [1, 17])
def test_max_is_bit_equal(T):
    """max is exact and its backward only routes values: forward and backward bit-equal to the fp32 oracle (ties
    occur only at 0, where the ReLU in front of the operator stops the gradient under both tie rules)."""
    G = op_graph(T)
    out, g_raw, _ = device_aggr(G, "max")
    o_out, o_raw, _ = oracle_aggr(G, "max", torch.float32)
    assert torch.equal(out, o_out)
    assert torch.equal(g_raw, o_raw)
    assert not out[0].any() and out[-1].any()                   # the empty first segment, the last one


@pytest.mark.parametrize("kind", ["add", "mean", "attn"])
@pytest.mark.parametrize("T", [1, 17])
def test_aggregate_against_fp64(T, kind):
    G = op_graph(T)
    got = device_aggr(G, kind)
    o32 = oracle_aggr(G, kind, torch.float32)
    o64 = oracle_aggr(G, kind, torch.float64)
    ratios = {}
    for name, a, b, c in zip(("out", "grad_msgs", "grad_scores"), got, o32, o64):
        if c is not None:
            assert a.shape == c.shape and a.dtype == torch.float32
            ratios[name] = bound_ratio(a, b, c)
    print(f"seg_aggregate {kind} T={T} error/bound: " + ", ".join(f"{k} {v:.3f}" for k, v in ratios.items()))
    assert max(ratios.values()) <= 1.0, ratios
    assert not got[0][0].any()                                  # the empty first segment


@pytest.mark.parametrize("W", [64, 128])
@pytest.mark.parametrize("T", [1, 17])
def test_gather_pair(T, W):
    G = op_graph(T)
    N, E = G["N"], G["E"]
    x = torch.from_numpy(syn.closed_form((N, W), 0.21))
    wi = torch.from_numpy(syn.closed_form((E, W), 0.31))
    wj = torch.from_numpy(syn.closed_form((E, W), 0.41))
    res = {}
    for dtype in (torch.float32, torch.float64):
        xx = x.clone().to(dtype).requires_grad_(True)
        xi, xj = to.gather_pair(xx, G["ei"][0], G["ei"][1])
        ((xi * wi.to(dtype)).sum() + (xj * wj.to(dtype)).sum()).backward()
        res[dtype] = (xi.detach(), xj.detach(), xx.grad)
    plan = tr.build_plan(G["ei"].to(DEV), G["types"].to(DEV), N, T)
    xd = x.to(DEV).requires_grad_(True)
    xi, xj = tr.gather_pair(xd, plan)
    ((xi * wi.to(DEV)).sum() + (xj * wj.to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    assert torch.equal(xi.detach().cpu(), res[torch.float32][0]) and torch.equal(xj.detach().cpu(), res[torch.float32][1])
    ratio = bound_ratio(xd.grad.cpu(), res[torch.float32][2], res[torch.float64][2])
    print(f"gather_pair W={W} T={T} error/bound: grad_x {ratio:.3f}")
    assert ratio <= 1.0


def test_empty_graph_and_input_checks():
    """E = 0 with N > 0: zeros without a launch. CPU tensors, other dtypes and wrong shapes are refused."""
    N, T = 5, 17
    ei = torch.zeros(2, 0, dtype=torch.int64, device=DEV)
    plan = tr.build_plan(ei, torch.zeros(N, dtype=torch.int64, device=DEV), N, T)
    for kind in ("attn", "add", "mean", "max"):
        msgs = torch.zeros(0, 64, device=DEV, requires_grad=True)
        out = tr.seg_aggregate(msgs, torch.zeros(0, device=DEV) if kind == "attn" else None, plan, kind)
        assert out.shape == (N * T, 64) and not out.any()
        out.sum().backward()
        assert msgs.grad.shape == (0, 64)
    x = torch.ones(N, 128, device=DEV, requires_grad=True)
    xi, xj = tr.gather_pair(x, plan)
    (xi.sum() + xj.sum()).backward()
    assert xi.shape == (0, 128) and not x.grad.any()
    G = op_graph(17)
    plan = tr.build_plan(G["ei"].to(DEV), G["types"].to(DEV), G["N"], 17)
    m = torch.relu(G["raw"])
    with pytest.raises(RuntimeError):
        tr.seg_aggregate(m, None, plan, "add")                              # a CPU tensor
    with pytest.raises(TypeError):
        tr.seg_aggregate(m.to(DEV).double(), None, plan, "add")
    with pytest.raises(TypeError):
        tr.gather_pair(torch.ones(G["N"], 64, device=DEV, dtype=torch.float16), plan)
    with pytest.raises(RuntimeError):
        tr.gather_pair(torch.ones(G["N"], 64), plan)
    with pytest.raises(ValueError):
        tr.gather_pair(torch.ones(G["N"], 96, device=DEV), plan)
    with pytest.raises(ValueError):
        tr.seg_aggregate(m.to(DEV), None, plan, "attn")                     # attention without scores


# ---- model -----------------------------------------------------------------------------------------------------
MODEL_CASES = gu.names("train_") + ["mpn_attn_c2_t3"]


def case_inputs(name):
    if name.startswith("train_"):
        meta = gu.load(name)[0]
        src_meta, a = gu.load(meta["source"])
    else:
        src_meta, a = gu.load(name)
    return src_meta, a, gu.mpn_config(src_meta)


def fresh_model(cfg, meta):
    m = pemp_amd.get_mpn_model(cfg)
    sd = syn.closed_form_state_dict(m, meta["salt"], meta.get("attn_gain", 1.0), meta.get("weight_gain", 1.0))
    m.load_state_dict(sd)
    return m, sd


@functools.lru_cache(maxsize=None)
def oracle_step(name, dtype, device):
    meta, a, cfg = case_inputs(name)
    _, sd = fresh_model(cfg, meta)
    return to.step(sd, cfg, a["x"], a["edge_attr"], a["edge_index"], a["node_types"], dtype=dtype, device=device)


def device_step(model, a, x=None, ea=None):
    """One training forward + backward of the fixture loss on the device: train_oracle.collect's dictionary."""
    x = torch.from_numpy(a["x"]).to(DEV).requires_grad_(True) if x is None else x
    ea = torch.from_numpy(a["edge_attr"]).to(DEV).requires_grad_(True) if ea is None else ea
    ei, types = torch.from_numpy(a["edge_index"]).to(DEV), torch.from_numpy(a["node_types"]).to(DEV)
    model.zero_grad(set_to_none=True)
    pe, pn, pc, tag = model(x, ea, ei, node_types=types)
    assert tag == [None]
    loss = to.fixture_loss(pe, pn, pc)
    loss.backward()
    torch.cuda.synchronize()
    stats = {k: v for k, v in model.state_dict().items()
             if k.endswith(("running_mean", "running_var", "num_batches_tracked"))}
    grads = {"x": x.grad, "edge_attr": ea.grad}
    grads.update({k: p.grad for k, p in model.named_parameters()})
    return to.collect(pe, pn, pc, loss, stats, grads), (pe, pn, pc)


# Gradients whose fp32 error in torch's own dense kernels is not one number: sums over all E rows behind the edge
# head's first BatchNorm, whose backward makes the rows cancel. With the C2-sized inputs (E = 22,350) they come out
# 7.4e-8 from fp64 in one evaluation and 3.2e-10 in another on the same GPU: the torch-operator form showed both, and
# so did this model, bit for bit alike with the HIP operators and with the torch ones inside one process (CPU fp32:
# 1.5e-6). One GPU sample of the yardstick therefore reads 0.32 or 33 for them with identical operators.
ORDER_DEPENDENT = ("grad.edge_classification.0.weight", "grad.edge_classification.0.bias")
_KIND_NAMES = {0: "attn", 1: "add", 2: "mean", 3: "max"}


def module_form_step(cfg, meta, a, monkeypatch):
    """The torch-operator form evaluated through the model's own modules on this GPU: mpn/train.py's forward with
    the oracle's index_add_ / scatter_reduce / index_select operators in place of the HIP ones, so that it shares
    every dense kernel call (shapes, layouts, order) with the code under test."""
    monkeypatch.setattr(tr, "seg_aggregate", lambda msgs, scores, plan, kind: to.seg_aggregate(
        msgs, scores, plan.dst, plan.type_src, plan.N, plan.T, _KIND_NAMES[kind]))
    monkeypatch.setattr(tr, "gather_pair", lambda x, plan: to.gather_pair(x, plan.src, plan.dst))
    model, _ = fresh_model(cfg, meta)
    model.to(DEV).train()
    res = device_step(model, a)[0]
    monkeypatch.undo()
    return res


@pytest.mark.parametrize("name", MODEL_CASES)
def test_model_step_against_fp64(name, monkeypatch):
    """Bound per tensor, as the operators': 4 max|torch form in fp32 on this GPU - fp64| + 2^-22 max|fp64|. For the
    two ORDER_DEPENDENT tensors the fp32 error is the larger of two evaluations of the torch form on this GPU, the
    functional one and the one through the model's modules (module_form_step); every other tensor is held to the
    single functional evaluation. The gradient of attn_net.0.bias has no scale (analytically zero): it is held to
    train_oracle.residue_bound at fp32's roundoff, an absolute bound from its own terms."""
    meta, a, cfg = case_inputs(name)
    model, sd = fresh_model(cfg, meta)
    keys = list(model.state_dict().keys())
    model.to(DEV).train()
    got, (pe, pn, pc) = device_step(model, a)
    o64 = oracle_step(name, torch.float64, "cpu")
    o32 = oracle_step(name, torch.float32, "cuda:0")
    m32 = module_form_step(cfg, meta, a, monkeypatch)
    assert list(model.state_dict().keys()) == keys == list(sd.keys())
    n_rec = sum(1 for i in range(cfg.STEPS) if i >= cfg.STEPS - cfg.AUX_LOSS_STEPS - 1)
    assert (len(pe), len(pn), len(pc)) == (n_rec, n_rec + 1, n_rec + 1)
    worst = ("", 0.0)
    for k, want in o64.items():
        if k.startswith("aux."):
            continue
        if k.endswith("num_batches_tracked"):
            assert np.array_equal(got[k], want), k
            continue
        have = got.get(k)
        if have is None:          # a parameter the forward never reaches: None here, zeros in the oracle
            assert k.startswith("grad.") and not np.any(want), k
            continue
        assert have.shape == want.shape, k
        err = float(np.abs(have - want).max()) if want.size else 0.0
        if k == to.ATTN_BIAS:
            bound = to.residue_bound(o64, 2.0 ** -24)
            print(f"model step {name}: |grad attn_net.0.bias| {err:.2e} (torch form {np.abs(o32[k]).max():.2e}, "
                  f"fp64 {np.abs(want).max():.2e}), residue bound {bound:.2e}")
        else:
            bound = to.error_bound(o32, o64, k)
            if k in ORDER_DEPENDENT:
                print(f"model step {name}: {k} error {err:.2e}; torch form {np.abs(o32[k] - want).max():.2e} "
                      f"(functional), {np.abs(m32[k] - want).max():.2e} (through the modules)")
                bound = max(bound, to.error_bound(m32, o64, k))
        r = err / bound if bound > 0 else (0.0 if err == 0 else float("inf"))
        if r > worst[1]:
            worst = (k, r)
    print(f"model step {name}: largest error/bound {worst[1]:.3f} ({worst[0]})")
    assert worst[1] <= 1.0, worst
    for k in got:
        assert k in o64, k


@pytest.mark.parametrize("name", ["train_attn_t3", "train_pertype_max_t2", "train_mean_t2"])
def test_reproducible(name):
    """The same forward + backward three times: bit-identical logits and gradients (no atomics anywhere on the
    operators' paths; BatchNorm normalises with batch statistics, so its running buffers do not enter)."""
    meta, a, cfg = case_inputs(name)
    model, _ = fresh_model(cfg, meta)
    model.to(DEV).train()
    runs = [device_step(model, a)[0] for _ in range(3)]
    for k, v in runs[0].items():
        if k.startswith(("logit.", "grad.", "loss")):
            assert all(np.array_equal(v, r[k]) for r in runs[1:]), k
    assert int(runs[2]["bn.node_embedding.2.num_batches_tracked"]) == 3


def test_plan_is_cached_per_graph():
    """One plan per model, rebuilt when edge_index / node_types are other tensors or were written since."""
    meta, a, cfg = case_inputs("train_add_t2")
    model, _ = fresh_model(cfg, meta)
    model.to(DEV).train()
    x, ea, ei, types = (torch.from_numpy(a[k]).to(DEV) for k in ("x", "edge_attr", "edge_index", "node_types"))
    model(x, ea, ei, node_types=types)
    plan = model._train_plan[1]
    model(x, ea, ei, node_types=types)
    assert model._train_plan[1] is plan
    ei.add_(0)                                                   # written: _version moved
    model(x, ea, ei, node_types=types)
    assert model._train_plan[1] is not plan
    plan = model._train_plan[1]
    model(x, ea, ei.clone(), node_types=types)
    assert model._train_plan[1] is not plan
    torch.cuda.synchronize()


def test_eval_unmoved_after_a_training_step():
    """.train() + a step, then .eval(): logits bit-identical to a fresh eval-only model holding the same state_dict
    (the fold cache sees the BatchNorm statistics' update)."""
    meta, a, cfg = case_inputs("train_attn_t3")
    model, sd0 = fresh_model(cfg, meta)
    model.to(DEV).eval()
    ins = [torch.from_numpy(a[k]).to(DEV) for k in ("x", "edge_attr", "edge_index")]
    types = torch.from_numpy(a["node_types"]).to(DEV)
    with torch.no_grad():
        before = model(*ins, node_types=types)
    model.train()
    device_step(model, a)
    sd1 = {k: v.detach().clone() for k, v in model.state_dict().items()}
    assert list(sd1.keys()) == list(sd0.keys())
    assert not torch.equal(sd1["node_embedding.2.running_mean"].cpu(), sd0["node_embedding.2.running_mean"])
    model.eval()
    with torch.no_grad():
        after = model(*ins, node_types=types)
    fresh = pemp_amd.get_mpn_model(cfg)
    fresh.load_state_dict(sd1)
    fresh.to(DEV).eval()
    with torch.no_grad():
        want = fresh(*ins, node_types=types)
    torch.cuda.synchronize()
    for x, y, z in zip(after[0] + after[1] + after[2], want[0] + want[1] + want[2], before[0] + before[1] + before[2]):
        assert torch.equal(x, y)
    assert any(not torch.equal(x, z) for x, z in zip(after[1], before[1]))     # the statistics did move the logits


@pytest.mark.parametrize("name,word", [("mpn_attn_ept_t2", "EDGE_MLP"), ("mpn_attn_hmlp_t2", "UPDATE_TYPE"),
                                       ("mpn_attn_latefusion_t2", "LATE_FUSION_POS")])
def test_refused_in_training_only(name, word):
    meta, a, cfg = case_inputs(name)
    model, _ = fresh_model(cfg, meta)
    model.to(DEV)
    ins = [torch.from_numpy(a[k]).to(DEV) for k in ("x", "edge_attr", "edge_index")]
    types = torch.from_numpy(a["node_types"]).to(DEV)
    model.train()
    with pytest.raises(NotImplementedError, match=word):
        model(*ins, node_types=types)
    model.eval()
    with torch.no_grad():
        pe, pn, pc, _ = model(*ins, node_types=types)
    torch.cuda.synchronize()
    assert torch.isfinite(pn[-1]).all() and len(pe) == int(a["n_edge_preds"])


def test_cpu_and_dtype_inputs_are_refused():
    meta, a, cfg = case_inputs("train_mean_t2")
    model, _ = fresh_model(cfg, meta)
    model.to(DEV).train()
    x, ea, ei = (torch.from_numpy(a[k]) for k in ("x", "edge_attr", "edge_index"))
    types = torch.from_numpy(a["node_types"])
    with pytest.raises(RuntimeError):
        model(x, ea, ei, node_types=types)
    with pytest.raises(TypeError):
        model(x.to(DEV).double(), ea.to(DEV), ei.to(DEV), node_types=types.to(DEV))


def _label_batch(J=17, C=128):
    from tests.test_labels_cpu import label_config
    B, H, W = 2, 96, 104
    hm, gt, fac = syn.make_labelled_heatmaps(3, B, J, H, W, 6)
    cfg = label_config(dict(graph="fully", method=6, use_neighbours=True, with_background=False,
                            matching_radius=0.5, inclusion_radius=0.75))
    feats = torch.from_numpy(syn.closed_form((B, C, H, W), gu.FEATURE_SALT)).to(DEV)
    tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), gu.TAG_SALT)).to(DEV)

    def build(with_gt=True):
        return pemp_amd.get_graph_constructor(cfg, scoremaps=torch.from_numpy(hm).to(DEV), features=feats, tagmaps=tags,
                                              joints_gt=torch.from_numpy(gt) if with_gt else None,
                                              factor_list=torch.from_numpy(fac) if with_gt else None, masks=None,
                                              device=DEV, testing=True, heatmaps=None, num_joints=J).construct_graph()
    return build


def test_labels_to_gradients():
    """construct_graph with ground truth -> training forward -> masked BCE on edge_labels / label_mask -> backward:
    every parameter on the edge logits' path gets a finite, non-zero gradient."""
    out = _label_batch()()
    x, ea, ei, labels, mask, types = out[0], out[1], out[2], out[3], out[8], out[7][:, 2]
    model = pemp_amd.get_mpn_model(pcfg.published_mpn_config(17, 3, "attn"))
    model.load_state_dict(syn.closed_form_state_dict(model, 2.5))
    model.to(DEV).train()
    pe, pn, pc, _ = model(x, ea, ei, node_types=types)
    assert pe[-1].shape == labels.shape and mask.sum() > 0 and labels.sum() > 0
    loss = torch.nn.functional.binary_cross_entropy_with_logits(pe[-1], labels, weight=mask, reduction="sum") / mask.sum()
    loss.backward()
    torch.cuda.synchronize()
    assert torch.isfinite(loss)
    for prefix in ("mpn_node_cls.mlp_edge", "edge_embedding", "node_embedding", "edge_classification"):
        params = [(k, p) for k, p in model.named_parameters() if k.startswith(prefix)]
        assert params
        for k, p in params:
            assert p.grad is not None and torch.isfinite(p.grad).all() and p.grad.abs().max() > 0, k


def test_bound_training_model_is_left_alone():
    """bind_mpn + .train(): construct_graph queues nothing for the model (no tag on edge_index), the training forward
    computes; back in .eval() the capacity path serves it again."""
    from pemp_amd.graph_constructor import NaiveGraphConstructor
    NaiveGraphConstructor._graph_hint.clear()
    build = _label_batch()
    model = pemp_amd.get_mpn_model(pcfg.published_mpn_config(17, 3, "attn"))
    model.load_state_dict(syn.closed_form_state_dict(model, 2.5))
    model.to(DEV).train()
    pemp_amd.bind_mpn(model)
    try:
        for _ in range(3):                                   # the second sight of a shape is the capacity build's
            out = build(with_gt=False)
            assert getattr(out[2], "_pemp_mpn", None) is None
        pe, pn, pc, _ = model(out[0], out[1], out[2], node_types=out[7][:, 2])
        (pe[-1].sum() + pn[-1].sum()).backward()
        torch.cuda.synchronize()
        assert torch.isfinite(pn[-1]).all() and model.node_embedding[0].weight.grad is not None
        model.eval()
        tagged = [getattr(build(with_gt=False)[2], "_pemp_mpn", None) is not None for _ in range(2)]
        assert any(tagged)
    finally:
        pemp_amd.bind_mpn(None)
