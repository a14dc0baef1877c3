"""CPU-side checks of the keypoint losses (pemp_amd/kp_loss.py, csrc/kp_loss.hip): the plain-torch oracle against the
reference's recorded fp64 results (tests/golden/kp_loss_*.npz), the refusals and input errors (raised before the HIP
library is touched), the record the wrapper builds, the workspace arithmetic and the config defaults. No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import pemp_amd
from pemp_amd import _lib, config as pcfg, kp_loss as kl
from tests import golden_util as gu, kp_loss_oracle as ko, loss_oracle as lo

AGREE = 1e-9
FIXTURES = gu.names("kp_loss_")


def test_fixture_set():
    assert FIXTURES == ["kp_loss_exp", "kp_loss_max"]
    assert [gu.load(n)[0]["options"]["AE_LOSS_TYPE"] for n in FIXTURES] == ["exp", "max"]


def _close(got, want, what):
    scale = np.abs(want).max()
    assert np.abs(np.asarray(got) - want).max() <= AGREE * scale, what


@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_reference(name):
    """kp_loss_oracle in fp64 against the reference's fp64 HeatmapLoss / AELoss values and gradients and against the
    heatmap and tagmap entries of ClassMultiLossFactory's logging, within 1e-9 max|.| per tensor."""
    meta, a = gu.load(name)
    J, B, opt = meta["J"], meta["B"], meta["options"]
    assert ko.max_kinks_clear(a, 0, J)
    for s in range(2):
        p = torch.from_numpy(a[f"pred{s}"]).double().requires_grad_(True)
        v = ko.heatmap_loss(p[:, :J], torch.from_numpy(a[f"gt{s}"]).double(), torch.from_numpy(a[f"mask{s}"]).double())
        v.sum().backward()
        _close(v.detach().numpy(), a[f"hm{s}"], f"hm{s}")
        _close(p.grad.numpy(), a[f"g_hm{s}"], f"g_hm{s}")
    p = torch.from_numpy(a["pred0"]).double().requires_grad_(True)
    push, pull = ko.ae_loss(p[:, J:].contiguous().view(B, -1, 1), a["tag0"], opt["AE_LOSS_TYPE"])
    (push.sum() + pull.sum()).backward()
    _close(push.detach().numpy(), a["push"], "push")
    _close(pull.detach().numpy(), a["pull"], "pull")
    _close(p.grad.numpy(), a["g_ae"], "g_ae")
    got = ko.run(a, opt, torch.float64)
    _close(got["terms"], a["multi.terms"], "terms")
    for s in range(2):
        _close(got[f"g_pred{s}"], a[f"multi.g_pred{s}"], f"g_pred{s}")
    # the factory's total: the two terms here plus the weighted node and edge terms of loss_oracle
    mpn = {k[4:]: v for k, v in a.items() if k.startswith("mpn.")}
    mo = lo.run(mpn, dict(meta["mpn_options"], TERMS=("node", "edge")), torch.float64, masks=True)
    log = dict(zip(meta["log_keys"], a["multi.log"]))
    node, edge = mo["terms"][0] * meta["mpn_options"]["NODE_WEIGHT"], mo["terms"][1] * meta["mpn_options"]["EDGE_WEIGHT"]
    assert abs(log["loss"] - (got["terms"][2] + node + edge)) <= AGREE * abs(log["loss"])
    assert meta["oracle_vs_reference"] <= AGREE and set(meta["reference_fp32_rel_err"]) >= {"multi.terms", "g_ae", "push"}


def test_fixture_persons_cover_the_cases():
    """Image 0: a person with all J joints, one with a single joint, one whose visible entries are not packed to the
    front; every image at least two persons (the reference's branches for fewer cannot run without a GPU)."""
    meta, a = gu.load("kp_loss_exp")
    vis = a["tag0"][..., 1] > 0
    counts = vis.sum(-1)
    assert counts[0].tolist() == [meta["J"], 1, 3, 2] and (counts > 0).sum(-1).tolist() == [4, 2]
    assert not vis[0, 2, 0] and vis[0, 2, 1]


def test_oracle_without_persons_and_with_one():
    """The branches the fixtures cannot hold: no person gives 0 and no gradient, one person gives push 0."""
    t = torch.arange(12, dtype=torch.float64).view(12, 1).requires_grad_(True)
    none = np.zeros((2, 3, 2), np.int64)
    push, pull = ko.single_tag_loss(t, none, "exp")
    assert push.item() == 0 and pull.item() == 0 and push.dtype == torch.float64
    one = none.copy()
    one[1, 0], one[1, 2] = (3, 1), (5, 1)
    push, pull = ko.single_tag_loss(t, one, "max")
    assert push.item() == 0 and pull.item() == 1.0          # tags 3 and 5: mean 4, squared distance 1
    one[0, 1] = (12, 1)                                      # out of range: skipped
    assert ko.single_tag_loss(t, one, "max")[1].item() == 1.0


def _cpu_inputs(S=2, J=5, B=2, P=4, C=None, dtype=torch.float32, tag_dtype=torch.int32):
    sizes = [(16, 16), (32, 32), (8, 8), (8, 8), (8, 8)][:S]
    C = C or [2 * J] + [J] * (S - 1)
    preds = [torch.zeros(B, c, h, w, dtype=dtype) for c, (h, w) in zip(C, sizes)]
    gts = [torch.zeros(B, J, h, w) for h, w in sizes]
    masks = [torch.ones(B, h, w) for h, w in sizes]
    tags = [torch.zeros(B, P, J, 2, dtype=tag_dtype)] + [None] * (S - 1)
    return preds, gts, masks, tags


OPT = dict(NUM_JOINTS=5, WITH_AE_LOSS=(True, False))


def test_refusals_come_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    monkeypatch.setattr(kl, "_device_f32", lambda name, t: _dtype_only(name, t))
    cfg = pcfg.get_config()
    cfg.MODEL.LOSS.NAME = ["edge", "node", "heatmap", "tag_loss"]
    for cls in (kl.KeypointLoss, kl.ClassMultiLossFactory):
        with pytest.raises(NotImplementedError, match=r"tag_loss.*Utils/loss.py:622"):
            cls(cfg)
    cfg.MODEL.LOSS.NAME = ["edge", "node", "heatmap"]
    for key, line in (("SYNC_TAGS", "733"), ("SYNC_GT_TAGS", "704")):
        bad = cfg.clone()
        bad.MODEL.LOSS[key] = True
        with pytest.raises(NotImplementedError, match=rf"{key}.*Utils/loss.py:{line}"):
            kl.ClassMultiLossFactory(bad)
    hg = cfg.clone()
    hg.MODEL.KP, hg.MODEL.LOSS.NAME = "hourglass", ["node", "heatmap", "tagmap"]
    with pytest.raises(NotImplementedError, match=r"hourglass.*Utils/loss.py:588"):
        kl.KeypointLoss(hg)
    none_set = cfg.clone()
    none_set.MODEL.LOSS.NAME = ["node", "tagmap"]
    with pytest.raises(ValueError, match="TRAIN.WITH_AE_LOSS"):
        kl.KeypointLoss(none_set)
    cfg.MODEL.LOSS.NAME = "heatmap"
    with pytest.raises(NotImplementedError, match="must be a list"):
        kl.ClassMultiLossFactory(cfg)
    with pytest.raises(NotImplementedError, match="S <= 4"):
        kl.keypoint_loss(*_cpu_inputs(S=5), OPT, WITH_HEATMAPS_LOSS=(True,) * 5, HEATMAPS_LOSS_FACTOR=(1.0,) * 5,
                         WITH_AE_LOSS=())
    with pytest.raises(NotImplementedError, match="P <= 32"):
        kl.keypoint_loss(*_cpu_inputs(P=33), OPT)
    with pytest.raises(NotImplementedError, match="J <= 32"):
        kl.keypoint_loss(*_cpu_inputs(J=33), OPT, NUM_JOINTS=33)
    with pytest.raises(TypeError, match="unknown option"):
        kl.keypoint_loss(*_cpu_inputs(), OPT, GAMMA=2.0)
    with pytest.raises(ValueError, match="AE_LOSS_TYPE"):
        kl.keypoint_loss(*_cpu_inputs(), OPT, AE_LOSS_TYPE="min")
    with pytest.raises(TypeError, match="float32"):
        kl.keypoint_loss(*_cpu_inputs(dtype=torch.float64), OPT)
    with pytest.raises(TypeError, match="int32 or int64"):
        kl.keypoint_loss(*_cpu_inputs(tag_dtype=torch.float32), OPT)
    with pytest.raises(ValueError, match="channels"):
        kl.keypoint_loss(*_cpu_inputs(C=[5, 5]), OPT)                 # AE without a tag plane
    with pytest.raises(ValueError, match="channels"):
        kl.keypoint_loss(*_cpu_inputs(C=[10, 4]), OPT)                # fewer channels than joints
    p, g, m, t = _cpu_inputs()
    with pytest.raises(ValueError, match=r"heatmaps_gt\[1\]: shape"):
        kl.keypoint_loss(p, [g[0], g[1][:, :, :31]], m, t, OPT)
    with pytest.raises(ValueError, match=r"masks\[0\]: shape"):
        kl.keypoint_loss(p, g, [m[0][:1], m[1]], t, OPT)
    with pytest.raises(ValueError, match=r"tag_targets\[0\]: shape"):
        kl.keypoint_loss(p, g, m, [t[0][:, :, :4], None], OPT)
    with pytest.raises(ValueError, match="WITH_HEATMAPS_LOSS has 1 entries"):
        kl.keypoint_loss(p, g, m, t, OPT, WITH_HEATMAPS_LOSS=(True,))
    with pytest.raises(ValueError, match="tag_targets has 0 entries"):
        kl.keypoint_loss(p, g, m, None, OPT)


def _dtype_only(name, t):
    """mpn.train._device_f32 without its device check (the record of a CPU-tensor call can then be inspected)."""
    if not isinstance(t, torch.Tensor) or t.dtype != torch.float32:
        raise TypeError(f"{name}: expected a float32 tensor (got {getattr(t, 'dtype', type(t))})")
    return t if t.is_contiguous() else t.contiguous()


def test_host_tensors_are_refused_before_the_library(monkeypatch):
    monkeypatch.setattr(_lib, "lib", lambda: (_ for _ in ()).throw(AssertionError("the library was touched")))
    with pytest.raises(RuntimeError, match="HIP device only"):
        kl.keypoint_loss(*_cpu_inputs(), OPT)


def test_record_of_a_two_stage_call(monkeypatch):
    """Sizes, flags, factors and pointers of the record for stage 0 [2, 10, 16, 16] with AE and stage 1 [2, 5, 32, 32]
    without; the heatmap planes are a prefix of every image, so a contiguous pred is pointed at in place and a
    non-contiguous one through one copy."""
    monkeypatch.setattr(kl, "_device_f32", _dtype_only)
    p, g, m, t = _cpu_inputs()
    p[0] = p[0].permute(0, 1, 3, 2)                                   # not contiguous
    opt = kl.kp_options(OPT, HEATMAPS_LOSS_FACTOR=(0.5, 2.0), PUSH_LOSS_FACTOR=(0.25, 9.0), PULL_LOSS_FACTOR=(0.125, 9.0),
                        AE_LOSS_TYPE="max", WITH_HEATMAPS_LOSS=(True, True))
    t64 = [t[0].long(), None]
    rec, held = kl.build_record(opt, p, g, m, t64)
    assert (rec.S, rec.B, rec.J, rec.P, rec.ae_kind) == (2, 2, 5, 4, _lib.KP_AE_MAX)
    s0, s1 = rec.stage[0], rec.stage[1]
    assert (s0.C, s0.H, s0.W, s0.with_heatmap, s0.with_ae) == (10, 16, 16, 1, 1)
    assert (s1.C, s1.H, s1.W, s1.with_heatmap, s1.with_ae) == (5, 32, 32, 1, 0)
    assert (s0.heatmap_factor, s0.push_factor, s0.pull_factor) == (0.5, 0.25, 0.125)
    assert (s1.heatmap_factor, s1.push_factor, s1.pull_factor) == (2.0, 0.0, 0.0)
    assert held[0][0].is_contiguous() and held[0][0].data_ptr() != p[0].data_ptr() and s0.pred == held[0][0].data_ptr()
    assert s1.pred == p[1].data_ptr() and s1.gt == g[1].data_ptr() and s1.mask == m[1].data_ptr() and not s1.tag
    assert held[3][0].dtype == torch.int32 and s0.tag == held[3][0].data_ptr() and held[3][1] is None
    assert not rec.stage[2].pred and rec.stage[2].C == 0
    # a stage switched off reads neither gt nor mask
    rec, held = kl.build_record(dict(opt, WITH_HEATMAPS_LOSS=(False, True)), p, [None, g[1]], [None, m[1]], t)
    assert rec.stage[0].with_heatmap == 0 and not rec.stage[0].gt and rec.stage[0].heatmap_factor == 0.0


def test_record_mirror_and_workspace_arithmetic():
    L = _lib.load_cdll()
    assert L.pemp_abi_struct_size(6) == ctypes.sizeof(_lib.PempKpLossRec)
    assert (_lib.KP_MAXS, _lib.KP_MAXP, _lib.KP_MAXJ, _lib.KP_CHUNK, _lib.KP_MAXBLOCKS) == (4, 32, 32, 4096, 2048)

    def rec(B, J, P, stages):
        r = _lib.PempKpLossRec(S=len(stages), B=B, J=J, P=P)
        for s, (C, H, W, heat, ae) in enumerate(stages):
            st = r.stage[s]
            st.C, st.H, st.W, st.with_heatmap, st.with_ae = C, H, W, heat, ae
        return r

    def want(B, J, P, stages):
        al = lambda v: (v + 255) // 256 * 256
        blocks = sum(min(B * ((J * H * W + _lib.KP_CHUNK - 1) // _lib.KP_CHUNK), _lib.KP_MAXBLOCKS)
                     for C, H, W, heat, ae in stages if heat)
        SB = len(stages) * B
        return 256 + al(8 * blocks) + al(16 * SB) + 2 * al(4 * SB) + al(8 * SB * P) + al(4 * SB * P)

    for case in ((2, 5, 4, [(10, 16, 16, 1, 1), (5, 32, 32, 1, 0)]), (4, 17, 30, [(34, 128, 128, 1, 1), (17, 256, 256, 1, 0)]),
                 (1, 1, 0, [(1, 1, 1, 1, 0)]), (3, 17, 30, [(34, 64, 64, 0, 1)]), (64, 17, 30, [(17, 256, 256, 1, 0)] * 4)):
        assert L.pemp_kp_loss_workspace_size(ctypes.byref(rec(*case))) == want(*case), case
    for bad in ((2, 5, 4, [(10, 16, 16, 1, 1)] * 5), (2, 33, 4, [(40, 8, 8, 1, 0)]), (2, 5, 33, [(10, 8, 8, 1, 1)]),
                (0, 5, 4, [(10, 8, 8, 1, 1)]), (1, 5, 4, [(10, 0, 8, 1, 1)]), (1, 5, 4, [(32, 8192, 8192, 1, 0)])):
        r = rec(bad[0], bad[1], bad[2], bad[3][:4])
        r.S = len(bad[3])
        assert L.pemp_kp_loss_workspace_size(ctypes.byref(r)) == 0, bad
    assert L.pemp_kp_loss_workspace_size(None) == 0


def test_argument_errors_need_no_gpu():
    """Bad records are refused with a message before any HIP call (the pointers are never dereferenced)."""
    L = _lib.load_cdll()
    p = 0x1000

    def rec(stage=None, **kw):
        r = _lib.PempKpLossRec(S=1, B=2, J=5, P=4, ae_kind=0)
        st = r.stage[0]
        st.pred = st.gt = st.mask = st.tag = p
        st.C, st.H, st.W, st.with_heatmap, st.with_ae = 10, 8, 8, 1, 1
        for k, v in (stage or {}).items():
            setattr(st, k, v)
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    out = (ctypes.c_float * _lib.KP_OUT)()
    g = (_lib.c_p * _lib.KP_MAXS)()
    cases = [("limits", rec(S=5), _lib.ERR_UNSUPPORTED), ("limits", rec(P=33), _lib.ERR_UNSUPPORTED),
             ("limits", rec(J=33), _lib.ERR_UNSUPPORTED), ("S = 0", rec(S=0), _lib.ERR_INVALID_ARG),
             ("ae_kind", rec(ae_kind=2), _lib.ERR_INVALID_ARG), ("C = 4", rec(dict(C=4)), _lib.ERR_INVALID_ARG),
             ("NULL pred", rec(dict(pred=None)), _lib.ERR_INVALID_ARG), ("NULL gt", rec(dict(gt=None)), _lib.ERR_INVALID_ARG),
             ("with_ae needs", rec(dict(tag=None)), _lib.ERR_INVALID_ARG),
             ("with_ae needs", rec(dict(C=5)), _lib.ERR_INVALID_ARG),
             ("exceeds", rec(dict(C=32, H=8192, W=8192)), _lib.ERR_INVALID_ARG)]
    for word, r, code in cases:
        assert L.pemp_kp_loss_fwd(ctypes.byref(r), p, 1 << 20, out, None) == code, word
        assert word in L.pemp_last_error().decode(), (word, L.pemp_last_error())
        assert L.pemp_kp_loss_bwd(ctypes.byref(r), p, None, ctypes.cast(g, _lib.c_p), None) == code, word
    assert L.pemp_kp_loss_fwd(ctypes.byref(rec()), p, 16, out, None) == _lib.ERR_WORKSPACE
    assert L.pemp_kp_loss_fwd(ctypes.byref(rec()), p, 1 << 20, None, None) == _lib.ERR_INVALID_ARG
    assert L.pemp_kp_loss_bwd(ctypes.byref(rec()), None, None, ctypes.cast(g, _lib.c_p), None) == _lib.ERR_INVALID_ARG
    # no gradient asked for: nothing to launch
    assert L.pemp_kp_loss_bwd(ctypes.byref(rec()), p, None, ctypes.cast(g, _lib.c_p), None) == 0


def test_config_defaults_read_back():
    """default_config.py:23, 53, 61, 71-78, 243, and how ClassMultiLossFactory.__init__ (:567-604) reads them."""
    cfg = pemp_amd.config.get_config()
    assert cfg.MODEL.KP == "hrnet" and cfg.MODEL.HG.NSTACK == 4 and cfg.MODEL.HRNET.NUM_JOINTS == 17
    assert dict(cfg.MODEL.HRNET.LOSS) == dict(
        NUM_STAGES=2, WITH_HEATMAPS_LOSS=(True, True), HEATMAPS_LOSS_FACTOR=(1.0, 1.0), WITH_AE_LOSS=(True, False),
        AE_LOSS_TYPE="exp", PUSH_LOSS_FACTOR=(0.001, 0.001), PULL_LOSS_FACTOR=(0.001, 0.001))
    assert cfg.TRAIN.WITH_AE_LOSS == [False, False] and cfg.TRAIN.END_TO_END is False
    assert kl.kp_options() == kl.KP_DEFAULTS == ko.OPTIONS
    # the default NAME lists neither term
    assert not kl.KeypointLoss(cfg).active
    cfg.merge({"MODEL": {"LOSS": {"NAME": ["edge", "node", "class", "heatmap"]},
                         "HRNET": {"LOSS": {"HEATMAPS_LOSS_FACTOR": [1.0, 0.5]}}}})
    opt = kl.KeypointLoss(cfg).options
    assert opt["WITH_HEATMAPS_LOSS"] == (True, True) and opt["HEATMAPS_LOSS_FACTOR"] == (1.0, 0.5)
    assert opt["WITH_AE_LOSS"] == ()                                   # no "tagmap": the HRNET key is not read
    cfg.merge({"MODEL": {"LOSS": {"NAME": ["node", "heatmap", "tagmap"]}}, "TRAIN": {"WITH_AE_LOSS": [True, False]}})
    opt = kl.KeypointLoss(cfg).options
    assert opt["WITH_AE_LOSS"] == (True, False) and opt["PUSH_LOSS_FACTOR"] == (0.001, 0.001)
    cfg.MODEL.KP, cfg.MODEL.LOSS.NAME, cfg.MODEL.HG.NSTACK = "hourglass", ["node", "heatmap"], 3
    opt = kl.KeypointLoss(cfg).options
    assert opt["WITH_HEATMAPS_LOSS"] == (True,) * 3 and opt["HEATMAPS_LOSS_FACTOR"] == (1.0,) * 4 and not opt["WITH_AE_LOSS"]
    # the factory takes the weights from NODE / EDGE / CLASS_WEIGHT, never from LOSS_WEIGHTS (:551-554)
    cfg.merge({"MODEL": {"LOSS": {"LOSS_WEIGHTS": [5.0, 5.0, 5.0], "EDGE_WEIGHT": 2.0}}})
    f = kl.ClassMultiLossFactory(cfg)
    assert f.mpn_options["EDGE_WEIGHT"] == 2.0 and f.mpn_options["NODE_WEIGHT"] == 1.0 and f.mpn_options["TERMS"] == ("node",)
    assert pemp_amd.ClassMultiLossFactory is kl.ClassMultiLossFactory and pemp_amd.keypoint_loss is kl.keypoint_loss
    assert pemp_amd.KeypointLoss is kl.KeypointLoss
