"""The paired prelude of a fully-graph forward (csrc/mpn.hip prelude_a_kernel: edge order beside node embedding,
prelude_b_kernel: wave ranges beside the first node table) against the four launches it replaces
(model.paired_prelude = False, pemp.h PEMP_MPN_SEPARATE_PRELUDE).

The paired kernels run the separate kernels' bodies block for block, so every logit must have the same bits on both
paths; the paired path is also held to the project's 1e-4 against oracle.restate. The graphs of tests/mpn_shapes.py
are plain tensors; here they carry the graph constructor's fully-graph tag (node offsets, node types as column 2 of
a joint_det array), which is what sends a forward to the closed-form order and so to the paired prelude."""
import functools

import pytest
import torch

import pemp_amd
from oracle import restate
from pemp_amd import _lib, config as pcfg, synthetic as syn
from pemp_amd import graph_constructor as gcm
from pemp_amd.mpn import model as mm
from tests import mpn_shapes as ms

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
TOL = 1e-4
J = ms.J

# name -> (per-image node counts, seed, node types or None for uniform ones)
GRAPHS = {
    "tiny": (*ms.GRAPHS["tiny"], None),              # N = 2, E = 2: one tile of padding everywhere
    "tile": (*ms.GRAPHS["tile"], None),              # N = 16, E = 240: every tile full
    "small": (*ms.GRAPHS["small"], None),            # N = 36, E = 662: tiles and ranges cut mid-tile, two images
    "empty_type": ((20, 9), 11, "skip_0_16"),        # types 0 and 16 have no node: first and last type range empty
    "empty_image": ((7, 0, 12), 5, None),            # the second image has no node
    "n17": ((17,), 7, None),                         # one full 16-row node tile and one of a single row
}


@functools.lru_cache(maxsize=None)
def weights(steps):
    cfg = pcfg.published_mpn_config(J, steps, "attn")
    sd = syn.closed_form_state_dict(pemp_amd.get_mpn_model(cfg), ms.SALT, attn_gain=ms.GAINS[0], weight_gain=ms.GAINS[1])
    return cfg, sd


def device_model(steps, paired, prec="f16x3"):
    cfg, sd = weights(steps)
    model = pemp_amd.get_mpn_model(cfg)
    model.load_state_dict(sd)
    model.precision = prec
    model.paired_prelude = paired
    return model.eval().to(DEV)


@functools.lru_cache(maxsize=None)
def graph(gname):
    """(x, edge_attr, edge_index, node_types) on the host and the per-image node counts. Read only."""
    sizes, seed, types = GRAPHS[gname]
    cfg, _ = weights(3)
    x, ea, ei, ty = ms.graph(sizes, J, cfg.EDGE_INPUT_DIM, cfg.NODE_INPUT_DIM, seed)
    if types == "skip_0_16":
        ty = 1 + torch.arange(x.shape[0]) % 15
    return (x, ea, ei, ty), sizes


@functools.lru_cache(maxsize=None)
def oracle(steps, gname):
    cfg, sd = weights(steps)
    return restate.mpn_forward(sd, cfg, *graph(gname)[0])[:3]


def tagged(gname):
    """The graph on the device as the graph constructor hands a fully graph over: edge_index tagged with the
    per-image node offsets, node_types the third column of a joint_det array."""
    (x, ea, ei, ty), sizes = graph(gname)
    jdet = torch.zeros(x.shape[0], 3, dtype=torch.int64, device=DEV)
    jdet[:, 2] = ty.to(DEV)
    noff = torch.tensor([0, *torch.tensor(sizes).cumsum(0).tolist()], dtype=torch.int64, device=DEV)
    ei = ei.to(DEV)
    gcm._tag_fully(ei, noff, sizes, jdet)
    types = jdet[:, 2]
    assert mm._fully_graph(ei, types, x.shape[0]) is not None      # the closed-form order's call
    return x.to(DEV), ea.to(DEV), ei, types


def run(model, inputs):
    x, ea, ei, types = inputs
    with torch.no_grad():
        out = model(x, ea, ei, node_types=types)
    torch.cuda.synchronize()
    return out


def flat(out):
    return list(out[0]) + list(out[1]) + list(out[2])


def same_bits(a, b):
    fa, fb = flat(a), flat(b)
    return len(fa) == len(fb) and all(p.shape == q.shape and torch.equal(p, q) for p, q in zip(fa, fb))


def max_err(got, ref):
    return max(((a.detach().cpu().float() - b.reshape(a.shape).float()).abs().max().item() if a.numel() else 0.0)
               for a, b in zip(flat(got), flat(ref)))


@pytest.mark.parametrize("prec", ["f16x3", "fp32"])
@pytest.mark.parametrize("steps", [1, 2, 3])          # 1: no middle pass, the edge embedding launch follows launch B
@pytest.mark.parametrize("gname", list(GRAPHS))
def test_paired_equals_separate(gname, steps, prec):
    inputs = tagged(gname)
    paired = run(device_model(steps, True, prec), inputs)
    separate = run(device_model(steps, False, prec), inputs)
    assert [len(r) for r in paired[:3]] == [1, 2, 2]
    assert all(torch.isfinite(t).all() for t in flat(paired))
    assert same_bits(paired, separate)


def test_paired_against_the_oracle():
    got = run(device_model(3, True), tagged("small"))
    err = max_err(got, oracle(3, "small"))
    print(f"paired_prelude_err small {err:.3e}")
    assert err < TOL


def test_paired_is_deterministic():
    model, inputs = device_model(3, True), tagged("small")
    first = run(model, inputs)
    for _ in range(5):
        assert same_bits(run(model, inputs), first)


def test_profiled_forward_keeps_the_separate_labels():
    """The library profiler's per-kernel labels are those of the separate kernels, with either setting, and the
    profiled forward computes the same bits."""
    inputs = tagged("small")
    plain = run(device_model(3, True), inputs)
    for paired in (True, False):
        model = device_model(3, paired)
        _lib.prof_enable("*")
        try:
            _lib.prof_report()
            out = run(model, inputs)
            rep = _lib.prof_report()
        finally:
            _lib.prof_enable(None)
        assert rep["mpn_prepare_fully"][0] == 1 and rep["node_embed"][0] == 1, rep
        assert rep["node_table"][0] + rep.get("node_update_table", (0, 0.0))[0] == 3, rep
        assert same_bits(out, plain)


def constructor_calls(paired):
    """bind_mpn + three construct_graph calls on 2 x 17 x 96 x 104 maps: the first sets the capacities (exact build),
    the second takes the batch-step entry (pemp_step_fully_cap) with the forward queued on the capacity buffers, the
    third (6 persons after 3) overflows them -- its queued forward sees N = E = 0 on the device and runs empty -- and
    the model computes on the exact graph. -> per call (queued result used, logits, inputs on the host)."""
    from pemp_amd.graph_constructor import NaiveGraphConstructor
    B, H, W = 2, 96, 104
    NaiveGraphConstructor._graph_hint.clear()
    NaiveGraphConstructor._cap = 512
    gc = pcfg.inference_gc_config("fully", 5, False)
    model = device_model(3, paired)
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
            got = run(model, (x, ea, ei, types))
            calls.append((bool(taken and taken[0]), [t.clone() for t in flat(got)],
                          tuple(t.cpu().clone() for t in (x, ea, ei, types))))
    finally:
        pemp_amd.bind_mpn(None)
        mm.NodeClassificationMPNSimple._take_cap = orig_take
    return calls


def test_constructor_graphs_and_capacity_mode():
    paired, separate = constructor_calls(True), constructor_calls(False)
    cfg, sd = weights(3)
    assert [c[0] for c in paired] == [c[0] for c in separate] == [False, True, False]
    for k, (cp, cs) in enumerate(zip(paired, separate)):
        assert all(torch.equal(a, b) for a, b in zip(cp[2], cs[2])), k     # the same graph on both runs
        assert len(cp[1]) == len(cs[1]) and all(torch.equal(a, b) for a, b in zip(cp[1], cs[1])), k
        ref = restate.mpn_forward(sd, cfg, *cp[2])[:3]
        err = max(((a.cpu() - b.reshape(a.shape).float()).abs().max().item() if a.numel() else 0.0)
                  for a, b in zip(cp[1], flat(ref)))
        print(f"paired_prelude_err constructor call {k} E={cp[2][2].shape[1]} {err:.3e}")
        assert err < TOL, k


def test_two_steps_in_flight_on_two_streams():
    """Whole steps (construct_graph + forward) issued round-robin on two HIP streams, at the size of
    tests/test_gpu_mpn.py::test_batches_in_flight_on_two_streams (74k-115k edges per batch): every step's outputs
    equal the same batch run serially, which in turn equals the separate prelude's."""
    B, H, W = 4, 256, 256
    gc = pcfg.inference_gc_config("fully", 5, False)
    feats = torch.from_numpy(syn.closed_form((B, 128, H, W), 0.25)).to(DEV)
    tags = torch.from_numpy(syn.closed_form((B, J, H, W, 1), 0.75)).to(DEV)
    hms = [torch.from_numpy(syn.make_heatmaps(40 + k, B, J, H, W, persons=8 + k % 3, margin=4)).to(DEV)
           for k in range(4)]

    def step(model, hm):
        out = pemp_amd.get_graph_constructor(gc, scoremaps=hm, features=feats, tagmaps=tags, joints_gt=None,
                                             factor_list=None, masks=None, device=DEV, testing=True,
                                             heatmaps=None, num_joints=J).construct_graph()
        with torch.no_grad():
            pe, pn, pc, _ = model(out[0], out[1], out[2], node_types=out[7][:, 2])
        return out[2], pe[-1], pn[-1], pc[-1]

    model, reference = device_model(3, True), device_model(3, False)
    separate = [tuple(t.cpu() for t in step(reference, hm)) for hm in hms]
    serial = [tuple(t.cpu() for t in step(model, hm)) for hm in hms]
    torch.cuda.synchronize()
    for k in range(len(hms)):
        assert all(torch.equal(a, b) for a, b in zip(serial[k], separate[k])), k
    streams = [torch.cuda.current_stream(DEV), torch.cuda.Stream(DEV)]
    got = []
    for k, hm in enumerate(hms):
        with torch.cuda.stream(streams[k % 2]):
            got.append(step(model, hm))
    torch.cuda.synchronize()
    for k in range(len(hms)):
        assert all(torch.equal(a.cpu(), b) for a, b in zip(got[k], serial[k])), k
