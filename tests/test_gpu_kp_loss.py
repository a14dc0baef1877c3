"""GPU tests of the keypoint losses (pemp_amd/kp_loss.py, csrc/kp_loss.hip) against the plain-torch oracle
(tests/kp_loss_oracle.py) and the reference's recorded results (tests/golden/kp_loss_*.npz).

Bound, per tensor (test_gpu_train.py's): err <= 4 max|o32 - o64| + 2^-22 max|o64|, o32 / o64 the oracle in fp32 / fp64.
For the gradient tensors o32 is the oracle on this GPU; for the scalar terms the fp32 error is, per term, the larger of
the CPU's and this GPU's (a scalar yardstick can be exact by luck). Each test prints its largest error / bound ratio
(DESIGN 7h records them).

Largest ratios seen on an MI355X: 0.14 over the terms and 0.21 over the gradients (DESIGN.md 7h lists them per group).

Masks carry values other than 0 / 1 throughout. For the 'max' form the tag values are chosen so that no two person
means of an image are equal or within 1e-3 of distance 1, asserted in fp64 (kp_loss_oracle.max_kinks_clear): the clamp
and the absolute value then take the same branch in every precision.
"""
import ctypes

import numpy as np
import pytest
import torch

import pemp_amd
from pemp_amd import _lib, config as pcfg, kp_loss as kl, synthetic as syn
from tests import golden_util as gu, kp_loss_oracle as ko, loss_oracle as lo
from tests.test_gpu_train import bound_ratio

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
CHUNK, CAP = _lib.KP_CHUNK, _lib.KP_MAXBLOCKS


# ---- inputs -----------------------------------------------------------------------------------------------------
def heat_arrays(seed, B, J, sizes, zero_mask=False):
    """pred / gt / mask per stage for ``sizes`` = [(C, H, W), ...]: masks uniform over [0, 1.5) with a fifth zeroed."""
    g = torch.Generator().manual_seed(seed)
    a = {}
    for s, (C, H, W) in enumerate(sizes):
        a[f"pred{s}"] = (torch.rand((B, C, H, W), generator=g) * 1.2 - 0.1).numpy()
        gt = torch.rand((B, J, H, W), generator=g)
        a[f"gt{s}"] = torch.where(gt > 0.7, gt, torch.zeros_like(gt)).numpy()
        m = torch.rand((B, H, W), generator=g) * 1.5
        m = torch.where(torch.rand((B, H, W), generator=g) < 0.2, torch.zeros_like(m), m)
        a[f"mask{s}"] = (torch.zeros_like(m) if zero_mask else m).numpy()
    return a


def options(J, S, heat=True, ae=(), kind="exp"):
    return dict(NUM_JOINTS=J, WITH_HEATMAPS_LOSS=(True,) * S if heat is True else tuple(heat),
                HEATMAPS_LOSS_FACTOR=(1.0, 0.5, 2.0, 0.25)[:S], WITH_AE_LOSS=tuple(ae), AE_LOSS_TYPE=kind,
                PUSH_LOSS_FACTOR=(0.5, 0.25, 1.0, 1.0)[:S], PULL_LOSS_FACTOR=(0.75, 0.5, 1.0, 1.0)[:S])


def ae_arrays(seed, J=5, H=8, W=8, one_plane=False, P=30):
    """B = 4, P = 30: image 0 has no person, image 1 one, image 2 two, image 3 thirty. Image 3: person 0 has all J
    joints, person 1 a single one, person 2 visible entries that are not packed to the front; persons 3 and 4 share one
    index (joint 1); person 5 sits on index T - 1; person 6 has a visible entry with index T (out of range, skipped)
    and person 7 one with index -1. Tag values: the person's centre 0.37 p plus at most 0.02."""
    B, HW = 4, H * W
    C = J + 1 if one_plane else 2 * J
    T = (C - J) * HW
    a = heat_arrays(seed, B, J, [(C, H, W)])
    g = torch.Generator().manual_seed(seed + 100)
    tag = np.zeros((B, P, J, 2), np.int32)
    tag[..., 0] = torch.randint(0, T, (B, P, J), generator=g).numpy()      # indices on invisible entries are never read
    flat = a["pred0"][:, J:].reshape(B, T)
    free = [[int(i) for i in torch.randperm(T, generator=g) if i != T - 1] for _ in range(B)]     # T - 1 is planted

    def see(b, p, j, idx=None):
        if idx is None:
            idx = free[b].pop()
            if not one_plane:
                idx = j * HW + idx % HW
                while idx in used[b]:
                    idx = j * HW + (idx + 1) % HW
        used[b].add(idx)
        tag[b, p, j] = (idx, 1)
        if 0 <= idx < T:
            flat[b, idx] = 0.37 * p + 0.02 * float(torch.rand((), generator=g))
        return idx

    used = [{T - 1} for _ in range(B)]
    see(1, 4, 2), see(1, 4, 0)
    see(2, 0, 1), see(2, 29, 3), see(2, 29, 4)
    for p in range(P):
        joints = range(J) if p == 0 else (3,) if p == 1 else (1, 2, 4) if p == 2 else (0, 1)
        for j in joints:
            see(3, p, j)
    see(3, 4, 1, int(tag[3, 3, 1, 0]))            # the duplicate: persons 3 and 4 on one pixel and joint
    see(3, 5, 0, T - 1)
    tag[3, 6, 4], tag[3, 7, 4] = (T, 1), (-1, 1)
    a["pred0"][:, J:] = flat.reshape(B, C - J, H, W)
    a["tag0"] = tag
    return a, T


def run_ours(a, opt, scale=1.0, need=None, validate=False, device_tags=False):
    S = sum(1 for k in a if k.startswith("pred"))
    need = need or (True,) * S
    t = lambda k, s: torch.from_numpy(np.asarray(a[f"{k}{s}"])).to(DEV) if f"{k}{s}" in a else None
    preds = [t("pred", s).requires_grad_(need[s]) for s in range(S)]
    tags = [torch.from_numpy(a[f"tag{s}"]).to(DEV if device_tags else "cpu") if f"tag{s}" in a else None for s in range(S)]
    total, terms = pemp_amd.keypoint_loss(preds, [t("gt", s) for s in range(S)], [t("mask", s) for s in range(S)], tags,
                                          opt, validate=validate)
    assert not terms.requires_grad and total.requires_grad == any(need)
    if total.requires_grad:
        (total * scale).backward()
    out = {"terms": terms.cpu().double().numpy()}
    assert float(total.detach()) == out["terms"][2]
    for s, p in enumerate(preds):
        out[f"g_pred{s}"] = None if p.grad is None else p.grad.cpu().double().numpy()
    return out


def term_ratio(got, o32a, o32b, o64):
    """bound_ratio per scalar term with the larger of the two fp32 errors."""
    worst = 0.0
    for i in range(len(o64)):
        o32 = o32a[i] if abs(o32a[i] - o64[i]) >= abs(o32b[i] - o64[i]) else o32b[i]
        worst = max(worst, bound_ratio(got[i:i + 1], np.asarray([o32]), o64[i:i + 1]))
    return worst


def check(a, opt, label, scale=1.0, **kw):
    """Ours against the oracle under the bound; prints and returns (ours, the fp64 oracle)."""
    o64 = ko.run(a, opt, torch.float64, "cpu", scale)
    o32c = ko.run(a, opt, torch.float32, "cpu", scale)
    o32g = ko.run(a, opt, torch.float32, DEV, scale)
    got = run_ours(a, opt, scale, **kw)
    rt = term_ratio(got["terms"], o32c["terms"], o32g["terms"], o64["terms"])
    rg = max(bound_ratio(got[k], o32g[k], o64[k]) for k in got if k.startswith("g_") and got[k] is not None)
    print(f"kp_loss {label}: terms {got['terms'].tolist()}, largest error/bound {rt:.3f} (terms), {rg:.3f} (gradients)")
    assert np.all(np.isfinite(got["terms"])) and rt <= 1.0 and rg <= 1.0, (label, rt, rg)
    return got, o64


# ---- the heatmap term -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(1, 1), (1, 3), (2, 2), (1, 5), (13, 7), (16, 24)])
def test_plane_sizes(H, W):
    """J = 3 planes of H W floats in a pred of J + 1 channels, B = 3: the 16-byte path (H W a multiple of 4) and the
    scalar one, image bases that are not 16-byte aligned (odd H W), and a tag plane that only gets zeros."""
    a = heat_arrays(1, 3, 3, [(4, H, W)])
    got, _ = check(a, options(3, 1), f"plane {H}x{W}")
    assert not np.any(got["g_pred0"][:, 3:]) and np.any(got["g_pred0"][:, :3])


@pytest.mark.parametrize("n", [CHUNK - 1, CHUNK, CHUNK + 1, 2 * CHUNK + 8])
def test_chunk_edges(n):
    """B J H W = n with B = J = H = 1: one unit short of, at and past PEMP_KP_CHUNK (n a multiple of 4 takes the
    16-byte path, the others the scalar one); then the same per image with B = 2 and two planes."""
    check(heat_arrays(2, 1, 1, [(1, 1, n)]), options(1, 1), f"chunk n={n}")
    if n % 2 == 0:
        check(heat_arrays(3, 2, 2, [(3, 1, n // 2)]), options(2, 1), f"chunk n={n} B=2 J=2")


def test_past_the_grid_cap():
    """One more unit than PEMP_KP_MAXBLOCKS: the first block takes a second unit (forward, and the backward over C H W)."""
    a = heat_arrays(4, 1, 1, [(1, CAP + 1, CHUNK)])
    check(a, options(1, 1), f"cap units={CAP + 1}")


def test_channel_counts_and_stages():
    """C = J, C = 2 J and C = J + 1; two stages of different sizes in one call; S = 4 with equal sizes; a stage
    switched off (its gradient all zero)."""
    J = 5
    check(heat_arrays(5, 2, J, [(J, 8, 12)]), options(J, 1), "C=J")
    check(heat_arrays(6, 2, J, [(2 * J, 8, 12)]), options(J, 1), "C=2J")
    check(heat_arrays(7, 2, J, [(2 * J, 16, 16), (J, 32, 32)]), options(J, 2), "two stages")
    check(heat_arrays(8, 2, J, [(J, 12, 12)] * 4), options(J, 4), "S=4")
    got, o64 = check(heat_arrays(9, 2, J, [(2 * J, 16, 16), (J, 32, 32)]), options(J, 2, heat=(False, True)), "stage 0 off")
    assert not np.any(got["g_pred0"]) and np.any(got["g_pred1"])


def test_all_zero_mask():
    a = heat_arrays(10, 2, 3, [(4, 6, 10)], zero_mask=True)
    got, _ = check(a, options(3, 1), "zero mask")
    assert got["terms"].tolist() == [0.0, 0.0, 0.0] and not np.any(got["g_pred0"])


# ---- the associative-embedding term ---------------------------------------------------------------------------------
@pytest.mark.parametrize("one_plane", [False, True])
@pytest.mark.parametrize("kind", ["exp", "max"])
def test_ae_persons(kind, one_plane):
    """P' of 0, 1, 2 and 30 in one batch, with the heatmap term on; the duplicate index gets the sum, T - 1 is
    written, the out-of-range entries are skipped; off the listed indices the tag planes are exactly zero."""
    J = 5
    a, T = ae_arrays(11, J, one_plane=one_plane)
    assert ko.max_kinks_clear(a, 0, J)
    assert [len(m) for m in ko.person_means(a, 0, J)] == [0, 1, 2, 30]
    opt = options(J, 1, ae=(True,), kind=kind)
    got, o64 = check(a, opt, f"ae {kind} C={'J+1' if one_plane else '2J'}")
    g = got["g_pred0"][:, J:].reshape(4, T)
    tag = a["tag0"]
    listed = np.zeros((4, T), bool)
    for b, p, j in zip(*np.nonzero(tag[..., 1] > 0)):
        if 0 <= tag[b, p, j, 0] < T:
            listed[b, tag[b, p, j, 0]] = True
    assert not np.any(g[~listed]) and not np.any(g[0]) and listed[3, T - 1] and g[3, T - 1] != 0
    assert listed.sum() == 2 + 3 + (J + 1 + 3 + 2 * 27) - 1                # one index of image 3 is listed twice
    dup = tag[3, 3, 1, 0]
    assert tag[3, 4, 1, 0] == dup and g[3, dup] != 0
    with pytest.raises(ValueError, match="2 visible tag entries"):
        run_ours(a, opt, validate=True)


@pytest.mark.parametrize("kind", ["exp", "max"])
def test_ae_only_and_heatmap_only(kind):
    """An AE-only call reads neither gt nor mask (both None); a heatmap-only call no tags."""
    J = 5
    a, T = ae_arrays(12, J)
    only = {k: v for k, v in a.items() if k in ("pred0", "tag0")}
    got, _ = check(only, options(J, 1, heat=(), ae=(True,), kind=kind), f"ae only {kind}")
    assert got["terms"][0] == 0.0 and got["terms"][1] != 0.0 and not np.any(got["g_pred0"][:, :J])
    heat = {k: v for k, v in a.items() if k != "tag0"}
    got, _ = check(heat, options(J, 1), "heatmap only")
    assert got["terms"][1] == 0.0 and not np.any(got["g_pred0"][:, J:])


# ---- the backward ---------------------------------------------------------------------------------------------------
def test_backward_scale_and_needs_input_grad():
    J = 5
    a, _ = ae_arrays(13, J)
    b = heat_arrays(14, 4, J, [(J, 16, 16)])
    a.update(pred1=b["pred0"], gt1=b["gt0"], mask1=b["mask0"])
    opt = options(J, 2, ae=(True, False))
    check(a, opt, "3.5 x total", scale=3.5)
    both = run_ours(a, opt)
    for need in ((True, False), (False, True)):
        got = run_ours(a, opt, need=need)
        for s in range(2):
            if need[s]:
                assert np.array_equal(got[f"g_pred{s}"], both[f"g_pred{s}"])
            else:
                assert got[f"g_pred{s}"] is None


def test_guards_and_unaligned_gradients():
    """pemp_kp_loss_bwd into caller-owned buffers: the elements after each g_pred stay as they were, and a gradient
    that is not 16-byte aligned (the scalar path) holds the same bits as the aligned one."""
    J = 5
    a, _ = ae_arrays(15, J)
    b = heat_arrays(16, 4, J, [(J, 16, 20)])
    a.update(pred1=b["pred0"], gt1=b["gt0"], mask1=b["mask0"])
    opt = kl.kp_options(options(J, 2, ae=(True, False)))
    t = lambda k: torch.from_numpy(a[k]).to(DEV)
    preds = [t("pred0"), t("pred1")]
    rec, held = kl.build_record(opt, preds, [t("gt0"), t("gt1")], [t("mask0"), t("mask1")], [t("tag0"), None])
    L = _lib.lib()
    ws = torch.empty(L.pemp_kp_loss_workspace_size(ctypes.byref(rec)), dtype=torch.uint8, device=DEV)
    out = torch.empty(_lib.KP_OUT, device=DEV)
    _lib.check(L.pemp_kp_loss_fwd(ctypes.byref(rec), ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.stream(DEV)))
    want = run_ours(a, opt)
    assert np.array_equal(out[:3].cpu().double().numpy(), want["terms"])
    GUARD, SENT = 64, -7.5
    for shift in (0, 1):
        bufs = [torch.full((shift + p.numel() + GUARD,), SENT, device=DEV) for p in preds]
        gs = [b[shift:shift + p.numel()].view(p.shape) for b, p in zip(bufs, preds)]
        assert all((g.data_ptr() % 16 == 0) == (shift == 0) for g in gs)
        kl.backward_into(rec, ws, None, gs)
        torch.cuda.synchronize()
        for s, (b, g) in enumerate(zip(bufs, gs)):
            assert bool((b[:shift] == SENT).all()) and bool((b[shift + g.numel():] == SENT).all()), (shift, s)
            assert np.array_equal(g.cpu().double().numpy(), want[f"g_pred{s}"]), (shift, s)


def test_in_place_write_before_backward_raises():
    a = heat_arrays(17, 2, 3, [(4, 8, 8)])
    pred = torch.from_numpy(a["pred0"]).to(DEV).requires_grad_(True)
    x = pred * 1.0
    total, _ = pemp_amd.keypoint_loss([x], [torch.from_numpy(a["gt0"]).to(DEV)], [torch.from_numpy(a["mask0"]).to(DEV)],
                                      None, options(3, 1))
    with torch.no_grad():
        x.add_(1.0)
    with pytest.raises(RuntimeError, match="modified by an inplace operation"):
        total.backward()


def test_non_contiguous_pred_is_copied_once():
    a = heat_arrays(18, 2, 3, [(4, 8, 8)])
    want = run_ours(a, options(3, 1))
    pred = torch.from_numpy(a["pred0"]).to(DEV).permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    assert not pred.is_contiguous()
    total, terms = pemp_amd.keypoint_loss([pred], [torch.from_numpy(a["gt0"]).to(DEV)],
                                          [torch.from_numpy(a["mask0"]).to(DEV)], None, options(3, 1))
    total.backward()
    assert np.array_equal(terms.cpu().double().numpy(), want["terms"])
    assert np.array_equal(pred.grad.cpu().double().numpy(), want["g_pred0"])


# ---- reproducibility and synchronisation --------------------------------------------------------------------------
def test_bitwise_reproducible_without_host_sync():
    J = 5
    a, _ = ae_arrays(19, J)
    b = heat_arrays(20, 4, J, [(J, 40, 52)])
    a.update(pred1=b["pred0"], gt1=b["gt0"], mask1=b["mask0"])
    opt = options(J, 2, ae=(True, False), kind="max")
    first = run_ours(a, opt)
    t = lambda k: torch.from_numpy(a[k]).to(DEV)
    preds = [t("pred0").requires_grad_(True), t("pred1").requires_grad_(True)]
    gts, masks, tags = [t("gt0"), t("gt1")], [t("mask0"), t("mask1")], [t("tag0"), None]
    scale = torch.full((), 1.0, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, terms = pemp_amd.keypoint_loss(preds, gts, masks, tags, opt, validate=False)    # validating reads the status word
        (total * scale).backward()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert np.array_equal(terms.cpu().double().numpy(), first["terms"])
    for s in range(2):
        assert np.array_equal(preds[s].grad.cpu().double().numpy(), first[f"g_pred{s}"])


# ---- the reference's recorded results -------------------------------------------------------------------------------
@pytest.mark.parametrize("name", gu.names("kp_loss_"))
def test_fixtures(name):
    """keypoint_loss on the fixture's inputs against the reference's fp64 heatmap / tagmap terms and gradients."""
    meta, a = gu.load(name)
    opt = meta["options"]
    o32g = ko.run(a, opt, torch.float32, DEV)
    o32c = ko.run(a, opt, torch.float32, "cpu")
    got = run_ours(a, opt)
    rt = term_ratio(got["terms"], o32c["terms"], o32g["terms"], a["multi.terms"])
    rg = max(bound_ratio(got[f"g_pred{s}"], o32g[f"g_pred{s}"], a[f"multi.g_pred{s}"]) for s in range(2))
    print(f"kp_loss fixture {name}: largest error/bound {rt:.3f} (terms), {rg:.3f} (gradients)")
    assert rt <= 1.0 and rg <= 1.0


def _factory_config(meta):
    o, m = meta["options"], meta["mpn_options"]
    cfg = pcfg.get_config()
    cfg.merge({"MODEL": {"LOSS": {"NAME": ["edge", "node", "heatmap", "tagmap"], "NODE_WEIGHT": m["NODE_WEIGHT"],
                                  "EDGE_WEIGHT": m["EDGE_WEIGHT"]},
                         "MPN": {"NODE_THRESHOLD": m["NODE_THRESHOLD"]},
                         "HRNET": {"NUM_JOINTS": meta["J"],
                                   "LOSS": {"HEATMAPS_LOSS_FACTOR": o["HEATMAPS_LOSS_FACTOR"], "AE_LOSS_TYPE": o["AE_LOSS_TYPE"],
                                            "PUSH_LOSS_FACTOR": o["PUSH_LOSS_FACTOR"],
                                            "PULL_LOSS_FACTOR": o["PULL_LOSS_FACTOR"]}}},
               "TRAIN": {"WITH_AE_LOSS": [True, False]}})
    return cfg


@pytest.mark.parametrize("name", gu.names("kp_loss_"))
def test_fixtures_through_the_factory(name):
    """ClassMultiLossFactory over the reference's dicts: the logging dict and every gradient against the reference's
    fp64 run of its own factory."""
    meta, a = gu.load(name)
    mpn = {k[4:]: v for k, v in a.items() if k.startswith("mpn.")}
    t = lambda v: torch.from_numpy(np.asarray(v)).to(DEV)
    K_e, K_n = meta["K_e"], meta["K_n"]
    pe = [t(mpn[f"pe{k}"]).requires_grad_(True) for k in range(K_e)]
    pn = [t(mpn[f"pn{k}"]).requires_grad_(True) for k in range(K_n)]
    preds = [t(a[f"pred{s}"]).requires_grad_(True) for s in range(2)]
    ei, lm, nl = t(mpn["edge_index"]), t(mpn["label_mask"]), t(mpn["node_labels"])
    th = meta["mpn_options"]["NODE_THRESHOLD"]
    masks = [lm * pemp_amd.mask_node_connections(p.sigmoid().detach(), ei, th, nl).float() for p in pn]
    outputs = {"edge": pe, "node": pn, "class": None, "heatmap": preds, "tag": None}
    labels = {"edge": [t(mpn["edge_labels"])] * K_n, "node": nl, "class": None,
              "heatmap": [t(a["gt0"]), t(a["gt1"])], "tag": [torch.from_numpy(a["tag0"]), None]}
    ms = {"edge": masks, "node": t(mpn["label_mask_node"]), "class": None, "heatmap": [t(a["mask0"]), t(a["mask1"])]}
    loss, log = pemp_amd.ClassMultiLossFactory(_factory_config(meta))(outputs, labels, ms, {"nodes": None})
    loss.backward()
    assert list(log) == list(meta["log_keys"]) and all(isinstance(v, float) for v in log.values())
    assert float(loss.detach()) == log["loss"]
    # the yardstick: the two oracles in fp32, on this GPU and on the CPU, assembled as the factory assembles them
    mo = dict(meta["mpn_options"], TERMS=("node", "edge"))

    def oracle_log(device):
        k, m = ko.run(a, meta["options"], torch.float32, device), lo.run(mpn, mo, torch.float32, device, masks=True)
        node, edge = m["terms"][0] * mo["NODE_WEIGHT"], m["terms"][1] * mo["EDGE_WEIGHT"]
        return np.asarray([k["terms"][0], k["terms"][1], edge, node, 0.0, k["terms"][2] + node + edge]), k, m

    lg, kg, mg = oracle_log(DEV)
    lc, _, _ = oracle_log("cpu")
    got = np.asarray([log[k] for k in meta["log_keys"]])
    rt = term_ratio(got, lc, lg, a["multi.log"])
    rg = max([bound_ratio(preds[s].grad.cpu(), kg[f"g_pred{s}"], a[f"multi.g_pred{s}"]) for s in range(2)] +
             [bound_ratio(pe[k].grad.cpu(), mg[f"g_pe{k}"], a[f"multi.g_pe{k}"]) for k in range(K_e)] +
             [bound_ratio(pn[k].grad.cpu(), mg[f"g_pn{k}"], a[f"multi.g_pn{k}"]) for k in range(K_n)])
    print(f"kp_loss factory {name}: log {log}, largest error/bound {rt:.3f} (logging), {rg:.3f} (gradients)")
    assert rt <= 1.0 and rg <= 1.0


# ---- one end-to-end step ------------------------------------------------------------------------------------------
def test_end_to_end_step():
    """construct_graph with ground truth -> model.train() -> ClassMultiLossFactory [edge, node, class, heatmap] ->
    backward: the heatmap prediction gets a gradient on its heatmap planes (zeros on its tag planes) and the MPN's
    parameters get theirs."""
    from tests.test_gpu_loss import _labelled_graph
    J = 17
    out15 = _labelled_graph()
    mcfg = pcfg.published_mpn_config(J, 3, "attn")
    mcfg.AUX_LOSS_STEPS = 2
    cfg = pcfg.get_config()
    cfg.MODEL.MPN = mcfg
    cfg.merge({"MODEL": {"LOSS": {"NAME": ["edge", "node", "class", "heatmap"]},
                         "HRNET": {"LOSS": {"WITH_HEATMAPS_LOSS": (True,), "HEATMAPS_LOSS_FACTOR": (1.0,)}}}})
    model = pemp_amd.get_mpn_model(mcfg)
    model.load_state_dict(syn.closed_form_state_dict(model, 9.5))
    model.to(DEV).train()
    hm, _, _ = syn.make_labelled_heatmaps(5, 1, J, 160, 160, 9)
    gt = torch.from_numpy(hm).to(DEV)
    pred = torch.cat([gt * 0.9 + 0.01, torch.zeros_like(gt)], 1).requires_grad_(True)      # [1, 2 J, 160, 160]
    mask = torch.full((1, 160, 160), 1.0, device=DEV)
    pe, pn, pc = model(out15[0], out15[1], out15[2], node_types=out15[7][:, 2])[:3]
    th = cfg.MODEL.MPN.NODE_THRESHOLD
    masks = [out15[8] * pemp_amd.mask_node_connections(p.sigmoid().detach(), out15[2], th, out15[4]).float() for p in pn]
    outputs = {"edge": pe, "node": pn, "class": pc, "heatmap": [pred], "tag": None}
    labels = {"edge": [out15[3]] * len(pn), "node": out15[4], "class": out15[5], "heatmap": [gt], "tag": None}
    ms = {"edge": masks, "node": out15[9], "class": None, "heatmap": [mask]}
    loss, log = pemp_amd.ClassMultiLossFactory(cfg)(outputs, labels, ms, {"nodes": out15[7]})
    loss.backward()
    torch.cuda.synchronize()
    assert log["heatmap"] > 0 and log["node"] > 0 and log["edge"] > 0 and log["class_loss"] > 0 and log["tag_loss"] == 0.0
    assert abs(log["loss"] - (log["heatmap"] + log["node"] + log["edge"] + log["class_loss"])) <= 1e-5 * log["loss"]
    g = pred.grad
    assert bool(torch.isfinite(g).all()) and bool(g[:, :J].abs().sum() > 0) and not bool(g[:, J:].any())
    grads = [p.grad for p in model.parameters() if p.requires_grad]
    assert all(x is not None and bool(torch.isfinite(x).all()) for x in grads) and any(bool(x.abs().sum() > 0) for x in grads)
    print(f"kp_loss end to end: log {log}, |pred.grad| sum {float(g.abs().sum()):.4g}")
