"""The graph constructor's options that the published configuration leaves unset, on the device: the nine
EDGE_FEATURES_TO_USE modes on every writer of edge_attr (tests/graph_options.py PATHS), NORM_NODE_DISTANCE = False,
the C entry points on planted nodes against a plain numpy reference, and HYBRID_K 1, 8, 9 and 32 through every top-k
route of the detection. Integer outputs and edge_attr bit for bit, the angle column within 2 ulp."""
import functools

import numpy as np
import pytest
import torch

import pemp_amd
from oracle import restate
from pemp_amd import _lib, config as pcfg, synthetic as syn
from pemp_amd.frontend import ProjectedHeatmaps, ProjectedMaps
from pemp_amd.graph_constructor import NaiveGraphConstructor as G
from tests import graph_options as go
from tests.test_frontend_cpu import COCO_FLIP, make_outputs

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
B = 2
CROWD_FLIP = [1, 0, 3, 2, 5, 4, 7, 6, 9, 8, 11, 10, 12, 13]
WORST_THETA = [0]      # the largest theta distance seen on the device, in ulp (printed by every test that has one)


@pytest.fixture(autouse=True)
def constructor_state(monkeypatch):
    """Every test starts without capacity hints or step plans and with the detection capacity at 512; the
    constructor's class-wide state goes back afterwards."""
    monkeypatch.setattr(G, "_cap", 512)
    monkeypatch.setattr(G, "_graph_hint", {})
    monkeypatch.setattr(G, "_plans", {})


def gc_config(graph, pool, mode, normed=True, K=5, masks=False):
    gc = pcfg.inference_gc_config(graph, pool, masks)
    gc.EDGE_FEATURES_TO_USE = list(go.FEATURES[mode])
    gc.NORM_NODE_DISTANCE = normed
    gc.HYBRID_K = K
    return gc


def construct(gc, J, hm, feats, tags, masks=None):
    return pemp_amd.get_graph_constructor(gc, scoremaps=hm, features=feats, tagmaps=tags, joints_gt=None,
                                          factor_list=None, masks=masks, device=DEV, testing=True, heatmaps=None,
                                          num_joints=J).construct_graph()


def profiled(fn):
    """fn() under the library profiler: (its result, {label: launches})."""
    _lib.prof_enable("*")
    try:
        _lib.prof_report()
        out = fn()
        rep = _lib.prof_report()
    finally:
        _lib.prof_enable(None)
    return out, {label: n for label, (n, _) in rep.items()}


def check_graph(out, ref, mode, what, outputs=(0, 2, 7, 11, 12, 14)):
    for i in outputs:
        assert out[i].shape == ref[i].shape, (what, i, out[i].shape, ref[i].shape)
        assert torch.equal(out[i].cpu(), ref[i]), f"{what}: output {i}"
    worst = go.check_edge_attr(out[1].cpu().numpy(), ref[1].numpy(), mode, what)
    WORST_THETA[0] = max(WORST_THETA[0], worst)
    return worst


# ---- mode x writer matrix through construct_graph ------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def path_inputs(name, J, F, hw):
    """The inputs of one path at one shape, on the host (for the oracle) and on the device: a dict with the priming
    call's and the profiled call's scoremaps, the features, the tags."""
    gtype, fkind, tkind, prime, (seed, persons), phw, _ = go.PATHS[name]
    H, W = hw
    d = dict(H=H, W=W, pool=3 if max(H, W) > 150 else 5)
    if tkind == "projected":      # scoremaps = tagmaps = the projected network outputs, F = 2 with a flipped pass
        flip = F == 2
        fi = None if not flip else COCO_FLIP if J == 17 else CROWD_FLIP
        outs, flips = make_outputs(7, B, J, [(H // 2, W // 2)], flip)
        ph = ProjectedHeatmaps([o.to(DEV) for o in outs], (H, W), J, None if flips is None else
                               [o.to(DEV) for o in flips], fi)
        s, t = restate.project_frontend(outs, flips, (H, W), J, fi)
        d.update(hm=s, hm_dev=ph, tags=t, tags_dev=ph, prime_dev=None)
    else:
        hm = torch.from_numpy(syn.make_heatmaps(seed, B, J, H, W, persons, margin=4))
        tags = torch.from_numpy(syn.closed_form((B, J, H, W, F), 0.75))
        d.update(hm=hm, hm_dev=hm.to(DEV), tags=tags, tags_dev=tags.to(DEV), prime_dev=None)
        if prime is not None:
            d["prime_dev"] = torch.from_numpy(syn.make_heatmaps(1, B, J, H, W, prime, margin=4)).to(DEV)
    if fkind == "projected":      # half-resolution maps; the oracle gets their fp32 projection (restate's order)
        low = syn.closed_form((B, 128, H // 2, W // 2), 0.25)
        d.update(feats=torch.from_numpy(restate.upsample_bilinear(low, (H, W))),
                 feats_dev=ProjectedMaps([torch.from_numpy(low).to(DEV)], (H, W)))
    else:
        feats = torch.from_numpy(syn.closed_form((B, 128, H, W), 0.25))
        d.update(feats=feats, feats_dev=feats.to(DEV))
    return d


@functools.lru_cache(maxsize=None)
def path_reference(name, mode, J, normed, hw):
    d = path_inputs(name, J, go.tag_dims(mode), hw)
    gc = gc_config(go.PATHS[name][0], d["pool"], mode, normed)
    return restate.construct_graph(d["hm"], d["feats"], d["tags"], None, gc, J)


def bound_model(J, A):
    cfg = pcfg.published_mpn_config(J, 3, "attn")
    cfg.EDGE_INPUT_DIM = A
    model = pemp_amd.get_mpn_model(cfg)
    sd = syn.closed_form_state_dict(model, 1.25)
    model.load_state_dict(sd)
    return cfg, sd, model.eval().to(DEV)


def run_path(name, mode, J, normed=True, hw=None):
    """One construct_graph call that reaches writer `name` with edge-feature mode `mode`, checked against the
    oracle; the call's profiler report must show the writer's launches. Returns the theta distance in ulp."""
    gtype = go.PATHS[name][0]
    hw = hw or go.PATHS[name][5] or (96, 104)
    d = path_inputs(name, J, go.tag_dims(mode), hw)
    gc = gc_config(gtype, d["pool"], mode, normed)
    ref = path_reference(name, mode, J, normed, hw)
    what = f"{name} mode {mode} J {J} {hw[0]}x{hw[1]} normed {normed}"
    assert ref[2].shape[1] > 1000, what
    bound = name == "fully_step_bound"
    if bound:
        cfg, sd, model = bound_model(J, go.width(mode, J))
        pemp_amd.bind_mpn(model)
    try:
        if d["prime_dev"] is not None:
            construct(gc, J, d["prime_dev"], d["feats_dev"], d["tags_dev"])
            torch.cuda.synchronize()
            assert G._graph_hint, what
        out, rep = profiled(lambda: construct(gc, J, d["hm_dev"], d["feats_dev"], d["tags_dev"]))
        print(f"graph_options {what}: {rep}")
        for label, n in go.PATHS[name][6].items():
            assert rep.get(label) == n, (what, label, rep)
        if name in ("fully_step", "fully_step_bound", "fully_step_overflow"):
            assert G._plans, what                         # the batch-step entry made its plan
        if name in ("knn_large",):
            assert int(np.bincount(ref[12].numpy()).max()) > 512, what
        if name in ("knn_fast", "feature_knn_fast"):
            assert int(np.bincount(ref[12].numpy()).max()) <= 512, what
        worst = check_graph(out, ref, mode, what)
        if bound:
            with torch.no_grad():
                got = model(out[0], out[1], out[2], node_types=out[7][:, 2])
            torch.cuda.synchronize()
            want = restate.mpn_forward(sd, cfg, ref[0], ref[1], ref[2], ref[7][:, 2])
            for k, head in enumerate(("edge", "node", "class")):
                err = (got[k][-1].cpu() - want[k][-1]).abs().max().item()
                print(f"graph_options {what}: {head} logits max abs err {err:.3g}")
                assert err <= 1e-4, (what, head, err)
    finally:
        if bound:
            pemp_amd.bind_mpn(None)
    if go.theta_column(mode) is not None:
        print(f"graph_options {what}: theta within {worst} ulp (largest so far {WORST_THETA[0]})")
    return worst


def _path_modes(name):
    return go.BOUND_MODES if name == "fully_step_bound" else go.TAG_MODES if name == "fully_projected_tags" \
        else tuple(go.MODES)


MATRIX = [(name, mode, 17) for name in go.PATHS for mode in _path_modes(name)] + \
         [(name, mode, 14) for name in go.PATHS for mode in (1, 5) if mode in _path_modes(name)]


@pytest.mark.parametrize("name,mode,J", MATRIX, ids=[f"{n}-m{m}-J{j}" for n, m, j in MATRIX])
def test_mode_on_writer(name, mode, J):
    run_path(name, mode, J)


@pytest.mark.parametrize("name", list(go.PATHS))
def test_norm_is_the_height(name):
    """H > W: norm = max(W, H) is H."""
    mode = 5 if name == "fully_projected_tags" else 0
    run_path(name, mode, 17, hw=(200, 192) if name == "knn_large" else (104, 96))


# modes 0 and 3 on every writer; where a writer takes neither, mode 5 (the position columns, the tag distance behind)
NORM_OFF = [(name, mode) for name in go.PATHS for mode in sorted({m if m in _path_modes(name) else 5 for m in (0, 3)})]


@pytest.mark.parametrize("name,mode", NORM_OFF, ids=[f"{n}-m{m}" for n, m in NORM_OFF])
def test_norm_node_distance_off(name, mode):
    """NORM_NODE_DISTANCE = False: dx, dy are the pixel differences themselves (norm = 1, the reference's default)."""
    run_path(name, mode, 17, normed=False)


# ---- the C entry points on the planted nodes ----------------------------------------------------------------------
F_SENT, I_SENT = -12345.0, -7


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def _direct_tag_cases(mode):
    return {5: (1, 2), 6: (1,), 7: (2,), 8: (1, 2)}.get(mode, (None,))


@functools.lru_cache(maxsize=None)
def direct_nodes():
    """The planted nodes followed by the offset sweep: det, tags per F, scores, and a scattered order of all their
    edges (every ordered pair of the planted nodes, the sweep's edges)."""
    p = go.planted_nodes()
    sdet, sei = go.sweep_nodes()
    rng = np.random.default_rng(3)
    n0, n1 = p["det"].shape[0], sdet.shape[0]
    det = np.concatenate([p["det"], sdet])
    tags = {1: np.concatenate([p["tags"][1], rng.standard_normal(n1).astype(np.float32)]),
            2: np.concatenate([p["tags"][2], rng.standard_normal((n1, 2)).astype(np.float32)])}
    scores = np.concatenate([p["scores"], rng.random(n1).astype(np.float32)])
    ei = np.concatenate([go.fully_pairs([n0]), sei + n0], 1)
    return det, tags, scores, np.ascontiguousarray(ei[:, rng.permutation(ei.shape[1])])


def call_edge_features(det_d, tags_d, F, sc_d, ei_d, E, J, norm, mode, out_d):
    return _lib.lib().pemp_edge_features(_lib.ptr(det_d), _lib.ptr(tags_d), F, _lib.ptr(sc_d), _lib.ptr(ei_d), E, J,
                                         norm, mode, _lib.ptr(out_d), _lib.stream(DEV))


@pytest.mark.parametrize("norm", [1.0, 4096.0])
@pytest.mark.parametrize("mode", go.MODES)
def test_edge_features_direct(mode, norm):
    """pemp_edge_features on planted coordinates, tags and scores at edge counts around its 256-edge step: exact
    against the numpy reference, nothing written behind row E."""
    det, tags, scores, ei = direct_nodes()
    J, A = go.PLANTED_J, go.width(mode, go.PLANTED_J)
    det_d, sc_d = dev(det), dev(scores)
    for F in _direct_tag_cases(mode):
        t = None if F is None else tags[F]
        t_d = None if F is None else dev(t)
        for E in (0, 1, 255, 256, 257, ei.shape[1]):
            e = np.ascontiguousarray(ei[:, :E])
            e_d = dev(e) if E else torch.zeros(2, 1, dtype=torch.int64, device=DEV)
            out = torch.full((E * A + 64,), F_SENT, device=DEV)
            assert call_edge_features(det_d, t_d, F or 1, sc_d, e_d, E, J, norm, mode, out) == 0
            got = out.cpu().numpy()
            assert (got[E * A:] == F_SENT).all(), (mode, F, E)
            want = go.expected_edge_attr(det, e, J, norm, go.FEATURES[mode], t, scores)
            worst = go.check_edge_attr(got[:E * A].reshape(E, A), want, mode, f"mode {mode} F {F} E {E} norm {norm}")
            WORST_THETA[0] = max(WORST_THETA[0], worst)
    if mode == 4:
        print(f"graph_options edge_features direct: theta within {WORST_THETA[0]} ulp so far")


def test_edge_features_second_grid_trip():
    """E = 256 g + 1 with g the kernel's largest grid (65536 workgroups of 256 edges): the grid-stride loop takes a
    second trip. The edges repeat the planted list, so every period of the output must repeat the first one, which
    is checked against the numpy reference. All modes; a few ms of kernel time each."""
    det, tags, scores, ei = direct_nodes()
    J, P = go.PLANTED_J, ei.shape[1]
    E = 256 * 65536 + 1
    full, rem = divmod(E, P)
    base = dev(ei)
    big = torch.cat([base.repeat(1, full), base[:, :rem]], 1).contiguous()
    assert big.shape == (2, E)
    det_d, sc_d = dev(det), dev(scores)
    for mode in go.MODES:
        A = go.width(mode, J)
        for F in _direct_tag_cases(mode):
            t = None if F is None else tags[F]
            t_d = None if F is None else dev(t)
            out = torch.full((E * A + 64,), F_SENT, device=DEV)
            assert call_edge_features(det_d, t_d, F or 1, sc_d, big, E, J, 4096.0, mode, out) == 0
            bits = out.view(torch.int32)
            first = bits[:P * A]
            assert bool((bits[:full * P * A].view(full, P * A) == first[None]).all()), (mode, F)
            assert torch.equal(bits[full * P * A:E * A], first[:rem * A]), (mode, F)
            assert bool((out[E * A:] == F_SENT).all()), (mode, F)
            want = go.expected_edge_attr(det, ei, J, 4096.0, go.FEATURES[mode], t, scores)
            go.check_edge_attr(out[:P * A].cpu().numpy().reshape(P, A), want, mode, f"mode {mode} F {F} E {E}")
            del out, bits, first
    del big
    torch.cuda.empty_cache()


BUILD_COUNTS = [23, 0, 1, 23]      # images of 0 and 1 nodes in the middle of the batch
BUILD_CAP, BUILD_C = 32, 2


@functools.lru_cache(maxsize=None)
def build_batch():
    """The planted nodes as pemp_detect's outputs of a four-image batch (the last image holds the first one's nodes
    in reverse order): det_xyt, det_scores, n_det, the node arrays the build must produce, features on the device."""
    p = go.planted_nodes()
    order = list(range(23)) + [23] + list(range(22, -1, -1))
    H, W = go.PLANTED_HW
    det_xyt = np.zeros((4, BUILD_CAP, 3), np.int64)
    det_sc = np.zeros((4, BUILD_CAP), np.float32)
    starts = np.concatenate([[0], np.cumsum(BUILD_COUNTS)])
    for b, n in enumerate(BUILD_COUNTS):
        idx = order[starts[b]:starts[b] + n]
        det_xyt[b, :n] = p["det"][idx]
        det_sc[b, :n] = p["scores"][idx]
    bidx = np.repeat(np.arange(4), BUILD_COUNTS).astype(np.int64)
    feats = ((torch.arange(4 * BUILD_C * H * W, device=DEV) % 1013).float() * 0.25).view(4, BUILD_C, H, W)
    # (the device copies live here: a pointer taken from a temporary tensor would outlive its memory)
    return dict(p=p, order=np.array(order), det_xyt=det_xyt, det_sc=det_sc, bidx=bidx, starts=starts, feats=feats,
                n_det_d=dev(np.array(BUILD_COUNTS, np.int32)), det_xyt_d=dev(det_xyt), det_sc_d=dev(det_sc))


@functools.lru_cache(maxsize=2)
def build_tagmaps(F):
    """tagmaps [4, J, H, W, F] on the device, zero but for the planted tags at the planted pixels."""
    bb = build_batch()
    H, W = go.PLANTED_HW
    tm = torch.zeros(4, go.PLANTED_J, H, W, F, device=DEV)
    det = bb["p"]["det"][bb["order"]]
    t = bb["p"]["tags"][F][bb["order"]].reshape(-1, F)
    tm[dev(bb["bidx"]), dev(det[:, 2]), dev(det[:, 1]), dev(det[:, 0])] = dev(t)
    return tm


def run_build(mode, F, with_tags, norm, n_cap=None, e_cap=None):
    """pemp_fully_graph_build (n_cap None) or pemp_fully_graph_build_cap into sentinel-filled outputs of one row more
    than the sizes passed; returns the outputs on the host and whether the batch fit."""
    bb = build_batch()
    L, J = _lib.lib(), go.PLANTED_J
    H, W = go.PLANTED_HW
    A = go.width(mode, J)
    N, E = sum(BUILD_COUNTS), sum(n * (n - 1) for n in BUILD_COUNTS)
    capacity = n_cap is not None
    n_rows, e_rows = (n_cap, e_cap) if capacity else (N, E)
    x = torch.full((n_rows + 1, BUILD_C), F_SENT, device=DEV)
    jdet = torch.full((n_rows + 1, 3), I_SENT, dtype=torch.int64, device=DEV)
    jsc = torch.full((n_rows + 1,), F_SENT, device=DEV)
    bidx = torch.full((n_rows + 1,), I_SENT, dtype=torch.int64, device=DEV)
    jtag = torch.full((n_rows + 1, F), F_SENT, device=DEV) if with_tags else None
    ei = torch.full((2 * e_rows + 2,), I_SENT, dtype=torch.int64, device=DEV)
    ea = torch.full((e_rows + 1, A), F_SENT, device=DEV)
    noff = torch.full((4 + 5,), I_SENT, dtype=torch.int64, device=DEV)
    tm = build_tagmaps(F) if with_tags else None
    fn = L.pemp_fully_graph_build_cap if capacity else L.pemp_fully_graph_build
    rc = fn(_lib.ptr(bb["n_det_d"]), 4, _lib.ptr(bb["det_xyt_d"]), _lib.ptr(bb["det_sc_d"]), BUILD_CAP, _lib.ptr(bb["feats"]), BUILD_C, _lib.ptr(tm), F, J, H, W, n_rows,
            e_rows, norm, mode, _lib.ptr(x), _lib.ptr(jdet), _lib.ptr(jsc), _lib.ptr(bidx), _lib.ptr(jtag),
            _lib.ptr(ei), _lib.ptr(ea), _lib.ptr(noff), _lib.stream(DEV))
    assert rc == 0, L.pemp_last_error().decode()
    torch.cuda.synchronize()
    fit = not capacity or (N <= n_cap and E <= e_cap)
    outs = dict(x=x, jdet=jdet, jsc=jsc, bidx=bidx, jtag=jtag, ei=ei, ea=ea, noff=noff)
    return {k: None if v is None else v.cpu().numpy() for k, v in outs.items()}, fit


def check_build(o, fit, mode, F, with_tags, norm, capacity, what):
    bb = build_batch()
    p, order, J = bb["p"], bb["order"], go.PLANTED_J
    N, E = sum(BUILD_COUNTS), sum(n * (n - 1) for n in BUILD_COUNTS)
    A = go.width(mode, J)
    if not fit:      # nothing is written but the batch's (N, E, overflow) = (0, 0, 1)
        for k in ("x", "jsc", "jtag", "ea"):
            assert o[k] is None or (o[k] == F_SENT).all(), (what, k)
        for k in ("jdet", "bidx", "ei"):
            assert (o[k] == I_SENT).all(), (what, k)
        assert (o["noff"][:5] == I_SENT).all() and o["noff"][5:8].tolist() == [0, 0, 1], (what, o["noff"])
        assert o["noff"][8] == I_SENT
        return
    det, sc = p["det"][order], p["scores"][order]
    tags = p["tags"][F][order].reshape(-1, F)
    ei = go.fully_pairs(BUILD_COUNTS)
    assert o["noff"][:5].tolist() == bb["starts"].tolist(), what
    assert o["noff"][5:8].tolist() == ([N, E, 0] if capacity else [I_SENT] * 3), (what, o["noff"])
    assert o["noff"][8] == I_SENT
    np.testing.assert_array_equal(o["jdet"][:N], det, what)
    np.testing.assert_array_equal(o["bidx"][:N], bb["bidx"], what)
    assert go.same_bits(o["jsc"][:N], sc).all(), what
    want_x = bb["feats"][dev(bb["bidx"]), :, dev(det[:, 1]), dev(det[:, 0])].cpu().numpy()
    np.testing.assert_array_equal(o["x"][:N], want_x, what)
    if with_tags:
        assert go.same_bits(o["jtag"][:N], tags).all(), what
        assert (o["jtag"][N:] == F_SENT).all(), what
    np.testing.assert_array_equal(o["ei"][:2 * E].reshape(2, E), ei, what)      # a contiguous [2, E] block
    want = go.expected_edge_attr(det, ei, J, norm, go.FEATURES[mode], tags if mode in go.TAG_MODES else None, sc)
    worst = go.check_edge_attr(o["ea"][:E], want, mode, what)
    WORST_THETA[0] = max(WORST_THETA[0], worst)
    assert (o["x"][N:] == F_SENT).all() and (o["jsc"][N:] == F_SENT).all() and (o["ea"][E:] == F_SENT).all(), what
    assert (o["jdet"][N:] == I_SENT).all() and (o["bidx"][N:] == I_SENT).all() and (o["ei"][2 * E:] == I_SENT).all()


def _build_cases():
    cases = []
    for mode in go.MODES:
        for F in _direct_tag_cases(mode):
            # the modes without tags: with tag maps to pack (F = 2) and without any
            cases.append((mode, F or 2, mode in go.TAG_MODES or mode in (0, 2, 4)))
    return cases


@pytest.mark.parametrize("norm", [1.0, 4096.0])
@pytest.mark.parametrize("mode,F,with_tags", _build_cases())
def test_fully_graph_build_direct(mode, F, with_tags, norm):
    """pemp_fully_graph_build and its capacity mode from planted detections and tag maps: node arrays, edge_index
    and edge_attr exact against the numpy reference. Capacity mode at the exact fit, with one node and one edge to
    spare, and one node / one edge over a capacity, where nothing may be written."""
    N, E = sum(BUILD_COUNTS), sum(n * (n - 1) for n in BUILD_COUNTS)
    what = f"build mode {mode} F {F} tags {with_tags} norm {norm}"
    o, fit = run_build(mode, F, with_tags, norm)
    check_build(o, fit, mode, F, with_tags, norm, False, what)
    for n_cap, e_cap, fits in ((N, E, True), (N + 1, E + 1, True), (N - 1, E, False), (N, E - 1, False)):
        o, fit = run_build(mode, F, with_tags, norm, n_cap, e_cap)
        assert fit == fits
        check_build(o, fit, mode, F, with_tags, norm, True, f"{what} n_cap {n_cap} e_cap {e_cap}")
    if mode == 4:
        print(f"graph_options build direct: theta within {WORST_THETA[0]} ulp so far")


def test_edge_feature_refusals_c_abi():
    """Unknown mode: INVALID_ARG; ae with F = 2 and ae_normed with F = 1: UNSUPPORTED; a tag mode without tags:
    INVALID_ARG -- from pemp_edge_features and from both fully-graph builds, before anything is launched."""
    det, tags, scores, ei = direct_nodes()
    det_d, sc_d, e_d, t_d = dev(det), dev(scores), dev(ei[:, :8]), dev(tags[2])
    out = torch.full((8 * 32,), F_SENT, device=DEV)
    cases = [(9, t_d, 2, _lib.ERR_INVALID_ARG), (-1, t_d, 2, _lib.ERR_INVALID_ARG), (6, t_d, 2, _lib.ERR_UNSUPPORTED),
             (7, t_d, 1, _lib.ERR_UNSUPPORTED), (5, None, 2, _lib.ERR_INVALID_ARG), (8, None, 1, _lib.ERR_INVALID_ARG)]
    for mode, t, F, want in cases:
        assert call_edge_features(det_d, t, F, sc_d, e_d, 8, go.PLANTED_J, 1.0, mode, out) == want, (mode, F)
        assert _lib.lib().pemp_last_error().decode().startswith("pemp_edge_features")
    torch.cuda.synchronize()
    assert bool((out == F_SENT).all())
    bb = build_batch()
    L = _lib.lib()
    H, W = go.PLANTED_HW
    bufs = [torch.full((4096,), F_SENT, device=DEV) for _ in range(8)]
    n_det, dx, ds = bb["n_det_d"], bb["det_xyt_d"], bb["det_sc_d"]
    for fn in (L.pemp_fully_graph_build, L.pemp_fully_graph_build_cap):
        for mode, with_tags, F, want in [(9, True, 2, _lib.ERR_INVALID_ARG), (6, True, 2, _lib.ERR_UNSUPPORTED),
                                         (7, True, 1, _lib.ERR_UNSUPPORTED), (5, False, 2, _lib.ERR_INVALID_ARG)]:
            tm = build_tagmaps(F) if with_tags else None
            rc = fn(_lib.ptr(n_det), 4, _lib.ptr(dx), _lib.ptr(ds), BUILD_CAP, _lib.ptr(bb["feats"]), BUILD_C,
                    _lib.ptr(tm), F, go.PLANTED_J, H, W, 47, 1012, 1.0, mode, *[_lib.ptr(b) for b in bufs],
                    _lib.stream(DEV))
            assert rc == want, (mode, F, rc)
            assert L.pemp_last_error().decode().startswith("pemp_fully_graph_build")
    torch.cuda.synchronize()
    assert all(bool((b == F_SENT).all()) for b in bufs)


@pytest.mark.parametrize("graph", ["fully", "knn"])
def test_edge_feature_refusals_constructor(graph):
    """The same refusals through construct_graph: each raises with a message that names EDGE_FEATURES_TO_USE."""
    J, H, W = 17, 96, 104
    hm = torch.from_numpy(syn.make_heatmaps(1, B, J, H, W, 3, margin=4)).to(DEV)
    feats = torch.from_numpy(syn.closed_form((B, 16, H, W), 0.25)).to(DEV)
    tags = {F: torch.from_numpy(syn.closed_form((B, J, H, W, F), 0.75)).to(DEV) for F in (1, 2)}
    gc = gc_config(graph, 5, 0)
    for features, t, exc in ((["position", "angle"], tags[1], NotImplementedError), (["ae"], tags[2], NotImplementedError),
                             (["ae_normed"], tags[1], NotImplementedError), (["ae_tracking_1"], None, TypeError),
                             (["position", "connection_type", "ae_normed"], None, TypeError)):
        gc.EDGE_FEATURES_TO_USE = features
        with pytest.raises(exc, match="EDGE_FEATURES_TO_USE"):
            construct(gc, J, hm, feats, t)
    gc.EDGE_FEATURES_TO_USE = go.FEATURES[0]      # and the constructor still works afterwards
    out = construct(gc, J, hm, feats, tags[1])
    assert out[2].shape[1] > 1000


# ---- detection top-k -------------------------------------------------------------------------------------------------
def run_topk(hm, masks, K, pool=3, labels=()):
    """construct_graph (fully) on planted planes at HYBRID_K = K against the oracle: outputs 7, 11, 12, 2."""
    Bq, J, H, W = hm.shape
    feats = torch.from_numpy(syn.closed_form((Bq, 8, H, W), 0.25))
    tags = torch.from_numpy(syn.closed_form((Bq, J, H, W, 1), 0.75))
    gc = gc_config("fully", pool, 0, K=K, masks=masks is not None)
    hm_t = torch.from_numpy(hm)
    m_t = None if masks is None else torch.from_numpy(masks)
    ref = restate.construct_graph(hm_t, feats, tags, m_t, gc, J)
    out, rep = profiled(lambda: construct(gc, J, hm_t.to(DEV), feats.to(DEV), tags.to(DEV),
                                          None if m_t is None else m_t.to(DEV)))
    for label in labels:
        assert rep.get(label) == 1, (label, rep)
    for i in (7, 11, 12, 2):
        assert torch.equal(out[i].cpu(), ref[i]), f"K {K}: output {i}"
    return ref, rep


@pytest.mark.parametrize("with_masks", [False, True], ids=["nomask", "masks"])
@pytest.mark.parametrize("live", [3, 40, 90])
@pytest.mark.parametrize("K", [1, 8, 9, 32])
def test_topk_fused_routes(K, live, with_masks):
    """The fused selection at 192 x 496, pool 3 (96 units per plane) with 3, 40 and 90 live units per plane: live K
    <= 256, <= 2048 and above pick its three top-k routes (all three at K = 32, the first two at K = 8 and 9); K <=
    8 and K > 8 are its two instantiations. Listed entries on both sides of the threshold, equal values across
    units, a plane with fewer than K non-negative pixels, an all-zero plane."""
    hm, masks = go.topk_maps(192, 496, live, K, with_masks)
    ref, rep = run_topk(hm, masks, K, labels=("detect_nms", "detect_select_emit"))
    sc = ref[11].numpy()
    assert "detect_top" not in rep
    assert (sc >= 0.1).any() and (sc < 0.1).any()
    if K > 1 and not with_masks:
        assert (sc < 0).sum() == K - 4             # the negative plane's fill of K - nn entries


def test_topk_clamped_to_the_plane():
    """HYBRID_K = 32 on 8 x 3 planes: K is clamped to H W = 24."""
    rng = np.random.default_rng(5)
    hm = (rng.random((2, 3, 8, 3)) - 0.3).astype(np.float32)
    ref, _ = run_topk(hm, None, 32)
    assert ref[7].shape[0] > 8


@pytest.mark.parametrize("K", [9, 32])
def test_topk_two_kernel_selection(K):
    """A plane of 1025 units (205 bands of 16 rows x 5 strips of 62 columns: the smallest past the fused stage's
    1024): plane_top_kernel<32> + emit_kernel with the threshold set."""
    H, W = 16 * 204 + 1, 62 * 4 + 1
    hm = np.stack([go.lattice_plane(H, W, 300, 4), go.lattice_plane(H, W, 7, 5)])[None]
    ref, rep = run_topk(hm, None, K, labels=("detect_nms", "detect_top", "detect_emit"))
    assert "detect_select_emit" not in rep
    assert ref[7].shape[0] > K + 7


def test_topk_past_the_limit_is_refused():
    hm, _ = go.topk_maps(192, 496, 3, 8, False)
    with pytest.raises(ValueError, match=r"topk must be in \[1, 32\] \(got 33\)"):
        run_topk(hm, None, 33)
