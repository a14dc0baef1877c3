"""The inference MPN on model shapes other than the published one (tests/mpn_shapes.py): every shape from which
plan_forward (csrc/mpn.hip) selects another kernel -- the wide and the generic edge embedding, the generic edge
head per aggregation and precision, the unfused node / class heads, node embeddings of other input widths and depths
-- against the CPU oracle at the project's bar (logits within 1e-4), on graphs that cut every tile of those kernels.
The library profiler's labels show that each fall-back was the kernel that ran."""
import functools

import pytest
import torch

import pemp_amd
from oracle import restate
from pemp_amd import _lib, config as pcfg, synthetic as syn
from tests import mpn_shapes as ms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4          # north_star: logits within 1e-4 (tests/test_gpu_mpn.py)
REL_SUM = 2e-6      # AGGR add: plus 2e-6 relative, against the fp64 oracle (test_vs_oracle's rule)
BF16_GAINS = (1.0, 1.0)   # bf16x3 is held to the bar at small logit magnitudes only (test_vs_oracle)


@functools.lru_cache(maxsize=None)
def device_model(case, variant, prec, gains):
    """One model (and one weight fold) per (case, variant, precision); its graphs share it."""
    cfg = ms.config(case, variant)
    model, _ = ms.state_dict(cfg, gains)
    model.precision = prec
    return model.eval().to(DEV), cfg


@pytest.fixture(scope="module", autouse=True)
def release_models():
    yield
    device_model.cache_clear()


def run(model, x, ea, ei, types):
    with torch.no_grad():
        out = model(x.to(DEV), ea.to(DEV), ei.to(DEV), node_types=types.to(DEV))
    torch.cuda.synchronize()
    return out


def max_err(got, ref, rel=0.0):
    """Largest error over pe + pn + pc (equal list lengths and shapes first)."""
    assert [len(g) for g in got[:3]] == [len(r) for r in ref]
    worst = 0.0
    for a, b in zip(got[0] + got[1] + got[2], ref[0] + ref[1] + ref[2]):
        assert a.shape == b.shape
        if a.numel():
            a = a.detach().cpu().double()
            assert bool(torch.isfinite(a).all())
            worst = max(worst, ((a - b.double()).abs() - rel * b.double().abs()).max().item())
    return worst


def shape_params():
    out = []
    for case in ms.CASES:
        for variant in ms.variants(case):
            precs = ["f16x3", "fp32"]
            if case in ms.BF16_CASES and variant.startswith("attn"):
                precs.append("bf16x3")
            out += [(case, variant, prec, g) for prec in precs for g in ms.GRAPHS]
    return out


@pytest.mark.parametrize("case,variant,prec,gname", shape_params(), ids=lambda v: v)
def test_shape_vs_oracle(case, variant, prec, gname):
    gains = BF16_GAINS if prec == "bf16x3" else ms.gains_for(variant)
    model, cfg = device_model(case, variant, prec, gains)
    got = run(model, *ms.case_graph(cfg, gname))
    assert model.precision == prec                               # (no fall-back to fp32 for the weight range)
    add = variant == "add"
    ref = ms.oracle(case, variant, gname, gains, double=add)
    assert [len(r) for r in ref] == list(ms.CASES[case].lengths)
    err = max_err(got, ref, REL_SUM if add else 0.0)
    print(f"shape_err {case}-{variant}-{prec}-{gname} {err:.3e}")
    assert err < TOL


def profiled(model, inputs):
    """(labels of the launch sites of one forward, its logits)."""
    _lib.prof_enable("*")
    try:
        _lib.prof_report()
        out = run(model, *inputs)
        rep = _lib.prof_report()
    finally:
        _lib.prof_enable(None)
    return rep, out


@pytest.mark.parametrize("case", list(ms.CASES))
def test_fallback_paths_are_taken(case):
    """The launch sites of one forward (library profiler): the case's fall-back ran, no other one did, and the
    profiled forward (every kernel on one stream, between events) computes bit-identical logits."""
    c = ms.CASES[case]
    model, cfg = device_model(case, "attn", "f16x3", ms.GAINS)
    inputs = ms.case_graph(cfg, "small")
    plain = run(model, *inputs)
    rep, prof = profiled(model, inputs)
    for a, b in zip(plain[0] + plain[1] + plain[2], prof[0] + prof[1] + prof[2]):
        assert torch.equal(a, b)
    ran = set(rep)
    assert ran & set(ms.FALLBACK_LABELS) == ({c.label} if c.label else set()), rep
    assert "node_embed" in ran
    if cfg.STEPS == 0:                                           # heads on the embedding: no edge kernel at all
        assert not [k for k in ran if k.startswith("edge_")], rep
        return
    n_rec = c.lengths[0]
    embed = c.label if c.label and c.label.startswith("edge_embed") else "edge_embed"
    head = c.label if c.label and c.label.startswith("edge_step") else "edge_step_head"
    assert rep[embed][0] == 1 and rep[head][0] == n_rec, rep
    assert rep.get("edge_step", (0, 0.0))[0] == cfg.STEPS - n_rec, rep   # the passes that record no logits
    if c.label == "heads":                                       # node and class head, for each of the n_rec + 1 rows
        assert rep["heads"][0] == 2 * (n_rec + 1), rep


def test_published_shape_takes_no_fallback():
    cfg = pcfg.published_mpn_config(ms.J, 3, "attn")
    model, _ = ms.state_dict(cfg, ms.GAINS)
    rep, _ = profiled(model.eval().to(DEV), ms.case_graph(cfg, "small"))
    assert not set(rep) & set(ms.FALLBACK_LABELS), rep
    assert rep["edge_embed"][0] == 1 and rep["edge_step_head"][0] == 1 and rep["edge_step"][0] == 2, rep


def test_embedding_label_follows_the_shape_in_fp32():
    """Exact fp32 has one embedding kernel for every LDS shape (edge_embed_kernel<0, 0>), so there the label names
    the shape: the published one keeps `edge_embed`, a shape off the fixed layout reports `edge_embed_generic`."""
    cfg = pcfg.published_mpn_config(ms.J, 3, "attn")
    model, _ = ms.state_dict(cfg, ms.GAINS)
    model.precision = "fp32"
    rep, _ = profiled(model.eval().to(DEV), ms.case_graph(cfg, "small"))
    assert not set(rep) & set(ms.FALLBACK_LABELS) and rep["edge_embed"][0] == 1, rep
    model, cfg = device_model("edge_in33", "attn", "fp32", ms.GAINS)
    rep, _ = profiled(model, ms.case_graph(cfg, "small"))
    assert set(rep) & set(ms.FALLBACK_LABELS) == {"edge_embed_generic"} and "edge_embed" not in rep, rep


@pytest.mark.parametrize("case", ["heads_wide", None], ids=["heads_wide", "published"])
def test_unfused_model_leaves_the_capacity_path(case, monkeypatch):
    """bind_mpn with a model whose node / class heads are not fused: pemp_step_fully_cap refuses to queue its forward,
    construct_graph clears the model's _cap_ok and every call runs the exact forward, correct each time. Control: the
    published model stays on the capacity path and is served from the queued result."""
    from pemp_amd import graph_constructor as gcm
    from pemp_amd.mpn import model as mm
    B, H, W = 2, 96, 96
    gcm.NaiveGraphConstructor._graph_hint.clear()             # capacities from earlier tests' batches of this shape
    gcm.NaiveGraphConstructor._cap = 512
    gc = pcfg.inference_gc_config("fully", 5, False)
    cfg = ms.config(case, "attn") if case else pcfg.published_mpn_config(ms.J, 3, "attn")
    model, sd = ms.state_dict(cfg, ms.GAINS)
    model = model.eval().to(DEV)
    hm = torch.from_numpy(syn.make_heatmaps(1, B, ms.J, H, W, 3, margin=4))
    feats = torch.from_numpy(syn.closed_form((B, 128, H, W), 0.25))
    ref = restate.construct_graph(hm, feats, torch.zeros(B, ms.J, H, W), None, gc, ms.J)
    rlog = restate.mpn_forward(sd, cfg, ref[0], ref[1], ref[2], ref[7][:, 2])[:3]
    served = []
    orig_take = mm.NodeClassificationMPNSimple._take_cap

    def take(self, *a):
        r = orig_take(self, *a)
        served.append(r is not None)
        return r

    monkeypatch.setattr(mm.NodeClassificationMPNSimple, "_take_cap", take)
    assert model._cap_ok is True
    pemp_amd.bind_mpn(model)
    try:
        for _ in range(4):
            out = pemp_amd.get_graph_constructor(gc, scoremaps=hm.to(DEV), features=feats.to(DEV), tagmaps=None,
                                                 joints_gt=None, factor_list=None, masks=None, device=DEV,
                                                 testing=True, heatmaps=None, num_joints=ms.J).construct_graph()
            for i in (0, 1, 2, 7, 11, 12):
                assert torch.equal(out[i].cpu(), ref[i]), i
            with torch.no_grad():
                got = model(out[0], out[1], out[2], node_types=out[7][:, 2])
            torch.cuda.synchronize()
            assert max_err(got, rlog) < TOL
    finally:
        pemp_amd.bind_mpn(None)
    if case:
        assert model._cap_ok is False and not any(served)
    else:
        assert model._cap_ok is True and any(served)


def test_node_input_above_128_is_refused():
    """NODE_INPUT_DIM 512 with NODE_EMB [256, 128, 64]: the library refuses the forward with its argument error
    before any launch (today's behaviour; the shape is not supported), and the device is left usable."""
    cfg = pcfg.published_mpn_config(ms.J, 3, "attn")
    cfg.NODE_INPUT_DIM = 512
    cfg.NODE_EMB.OUTPUT_SIZES = [256, 128, 64]
    model, _ = ms.state_dict(cfg, ms.GAINS)
    model = model.eval().to(DEV)
    inputs = [t.to(DEV) for t in ms.case_graph(cfg, "small")]
    model._weights(DEV)                                          # the fold's own launches come first
    _lib.prof_enable("*")
    try:
        _lib.prof_report()
        with pytest.raises(ValueError, match="node embedding"):
            with torch.no_grad():
                model(inputs[0], inputs[1], inputs[2], node_types=inputs[3])
        assert _lib.prof_report() == {}                          # no launch site was reached
    finally:
        _lib.prof_enable(None)
    torch.cuda.synchronize()
    cfg = pcfg.published_mpn_config(ms.J, 3, "attn")
    model, sd = ms.state_dict(cfg, ms.GAINS)
    x, ea, ei, types = ms.case_graph(cfg, "small")
    got = run(model.eval().to(DEV), x, ea, ei, types)
    assert max_err(got, restate.mpn_forward(sd, cfg, x, ea, ei, types)[:3]) < TOL
