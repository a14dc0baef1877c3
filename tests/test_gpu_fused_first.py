"""The fused first edge pass (edge embedding + pass 0 in one launch, csrc/mpn.hip edge_step_kernel STAGE_FIRST) against
the two launches it replaces (model.fuse_first_pass = False, pemp.h PEMP_MPN_TWO_LAUNCH_FIRST).

The fused pass runs the embedding's device functions in the embedding kernel's order on each 16-edge tile, so every
logit must have the same bits on both paths; both are also held to the project's 1e-4 against oracle.restate.
The library profiler's labels show which path ran (model.fuse_first_pass = True keeps the fused pass in a profiled
forward; by default a profiled forward keeps the two launches and their labels)."""
import functools

import pytest
import torch

import pemp_amd
from oracle import restate
from pemp_amd import _lib, config as pcfg, synthetic as syn
from tests import mpn_shapes as ms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
J = ms.J


@functools.lru_cache(maxsize=None)
def weights(steps, variant="attn", aux=0):
    cfg = pcfg.published_mpn_config(J, steps, variant)
    cfg.AUX_LOSS_STEPS = aux
    sd = syn.closed_form_state_dict(pemp_amd.get_mpn_model(cfg), ms.SALT, attn_gain=ms.GAINS[0], weight_gain=ms.GAINS[1])
    return cfg, sd


def device_model(steps, fuse, variant="attn", prec="f16x3", aux=0):
    cfg, sd = weights(steps, variant, aux)
    model = pemp_amd.get_mpn_model(cfg)
    model.load_state_dict(sd)
    model.precision = prec
    model.fuse_first_pass = fuse
    return model.eval().to(DEV)


@functools.lru_cache(maxsize=None)
def graph(gname):
    """The three fully connected graphs of tests/mpn_shapes.py (36/662 cuts tiles and ranges mid-tile, 16/240 fills
    its tiles exactly, 2/2 is one tile of padding) and one whose types 0 and 16 have no node: the first and the last
    type range of the edge order are empty."""
    cfg, _ = weights(3)
    if gname != "empty_type":
        return ms.case_graph(cfg, gname)
    x, ea, ei, _ = ms.graph((20, 9), J, cfg.EDGE_INPUT_DIM, cfg.NODE_INPUT_DIM, 11)
    return x, ea, ei, 1 + torch.arange(x.shape[0]) % 15


GRAPHS = ("small", "tile", "tiny", "empty_type")


@functools.lru_cache(maxsize=None)
def oracle(steps, gname):
    cfg, sd = weights(steps)
    return restate.mpn_forward(sd, cfg, *graph(gname))[:3]


def run(model, x, ea, ei, types):
    with torch.no_grad():
        out = model(x.to(DEV), ea.to(DEV), ei.to(DEV), node_types=types.to(DEV))
    torch.cuda.synchronize()
    return out


def flat(out):
    return list(out[0]) + list(out[1]) + list(out[2])


def max_err(got, ref):
    return max(((a.detach().cpu().float() - b.float()).abs().max().item() if a.numel() else 0.0)
               for a, b in zip(flat(got), flat(ref)))


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


def same_bits(a, b):
    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(fa, fb))


@pytest.mark.parametrize("gname", GRAPHS)
@pytest.mark.parametrize("steps", [2, 3])
def test_fused_equals_two_launches(steps, gname):
    inputs = graph(gname)
    fused = run(device_model(steps, None), *inputs)
    two = run(device_model(steps, False), *inputs)
    ref = oracle(steps, gname)
    e_f, e_t = max_err(fused, ref), max_err(two, ref)
    print(f"fused_first_err T{steps}-{gname} fused {e_f:.3e} two launches {e_t:.3e}")
    assert [len(r) for r in fused[:3]] == [len(r) for r in ref]
    assert same_bits(fused, two)
    assert e_f < TOL and e_t < TOL
    # the labels of both paths, and the profiled forwards compute the same bits again
    rep_f, out_f = profiled(device_model(steps, True), inputs)
    rep_t, out_t = profiled(device_model(steps, False), inputs)
    assert rep_f["edge_first"][0] == 1 and "edge_embed" not in rep_f, rep_f
    assert rep_f.get("edge_step", (0, 0.0))[0] == steps - 2 and rep_f["edge_step_head"][0] == 1, rep_f
    assert rep_t["edge_embed"][0] == 1 and "edge_first" not in rep_t, rep_t
    assert rep_t["edge_step"][0] == steps - 1 and rep_t["edge_step_head"][0] == 1, rep_t
    assert same_bits(out_f, fused) and same_bits(out_t, fused)


def test_fused_is_deterministic():
    model, inputs = device_model(3, None), graph("small")
    first = run(model, *inputs)
    for _ in range(9):
        assert same_bits(run(model, *inputs), first)


def test_profiled_forward_keeps_two_launches_by_default():
    rep, out = profiled(device_model(3, None), graph("small"))
    assert rep["edge_embed"][0] == 1 and "edge_first" not in rep, rep


EXCLUDED = {
    # name: (steps, variant, precision, aux)
    "fp32": (3, "attn", "fp32", 0),
    "bf16x3": (3, "attn", "bf16x3", 0),
    "steps1": (1, "attn", "f16x3", 0),
    "max": (3, "max", "f16x3", 0),
    "recorded_first": (2, "attn", "f16x3", 1),       # AUX_LOSS_STEPS 1 of 2 steps: pass 0 records logits
}


@pytest.mark.parametrize("name", list(EXCLUDED))
def test_excluded_cases_keep_the_embedding_launch(name):
    steps, variant, prec, aux = EXCLUDED[name]
    model = device_model(steps, True, variant, prec, aux)
    rep, _ = profiled(model, graph("small"))
    assert model.precision == prec
    assert rep["edge_embed"][0] == 1 and "edge_first" not in rep, rep


def constructor_calls(fuse):
    """bind_mpn + three construct_graph calls on 2 x 17 x 96 x 104 maps: the first sets the capacities (exact build),
    the second takes the batch-step entry (pemp_step_fully_cap) with the forward queued on the capacity buffers, the
    third (6 persons after 3) overflows them -- its queued forward sees E = 0 on the device and runs empty -- and the
    model computes on the exact graph. -> per call (queued result used, logits, inputs on the host)."""
    from pemp_amd.graph_constructor import NaiveGraphConstructor
    from pemp_amd.mpn import model as mm
    B, H, W = 2, 96, 104
    NaiveGraphConstructor._graph_hint.clear()
    NaiveGraphConstructor._cap = 512
    gc = pcfg.inference_gc_config("fully", 5, False)
    model = device_model(3, fuse)
    feats = torch.from_numpy(syn.closed_form((B, 128, H, W), 0.25)).to(DEV)
    taken = []
    orig_take = mm.NodeClassificationMPNSimple._take_cap

    def take(self, *a):
        r = orig_take(self, *a)
        taken.append(r is not None)
        return r

    mm.NodeClassificationMPNSimple._take_cap = take
    pemp_amd.bind_mpn(model)
    calls = []
    try:
        for seed, persons in ((1, 3), (2, 2), (4, 6)):
            hm = torch.from_numpy(syn.make_heatmaps(seed, B, J, H, W, persons, margin=4)).to(DEV)
            out = pemp_amd.get_graph_constructor(gc, scoremaps=hm, features=feats, tagmaps=None, joints_gt=None,
                                                 factor_list=None, masks=None, device=DEV, testing=True,
                                                 heatmaps=None, num_joints=J).construct_graph()
            x, ea, ei, types = out[0], out[1], out[2], out[7][:, 2]
            taken.clear()
            got = run(model, x, ea, ei, types)
            calls.append((bool(taken and taken[0]), [t.clone() for t in flat(got)],
                          tuple(t.cpu().clone() for t in (x, ea, ei, types))))
    finally:
        pemp_amd.bind_mpn(None)
        mm.NodeClassificationMPNSimple._take_cap = orig_take
    return calls


def test_constructor_graphs_and_capacity_mode():
    fused, two = constructor_calls(None), constructor_calls(False)
    cfg, sd = weights(3)
    assert [c[0] for c in fused] == [c[0] for c in two] == [False, True, False]
    for k, (cf, ct) in enumerate(zip(fused, two)):
        assert all(torch.equal(a, b) for a, b in zip(cf[2], ct[2])), k     # the same graph on both runs
        assert len(cf[1]) == len(ct[1]) and all(torch.equal(a, b) for a, b in zip(cf[1], ct[1])), k
        ref = restate.mpn_forward(sd, cfg, *cf[2])[:3]
        err = max(((a.cpu() - b.reshape(a.shape).float()).abs().max().item() if a.numel() else 0.0)
                  for a, b in zip(cf[1], flat(ref)))
        print(f"fused_first_err constructor call {k} E={cf[2][2].shape[1]} {err:.3e}")
        assert err < TOL, k

