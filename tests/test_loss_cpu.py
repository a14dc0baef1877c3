"""CPU-side checks of the MPN training loss (pemp_amd/loss.py, csrc/loss.hip): the plain-torch oracle against the
reference's recorded fp64 results (tests/golden/loss_*.npz), the workspace arithmetic, the refusals (raised before
the HIP library is touched), the record's ctypes mirror and the config defaults. No GPU."""
import ctypes

import numpy as np
import pytest
import torch

import pemp_amd
from pemp_amd import _lib, config as pcfg, loss as pl
from tests import golden_util as gu, loss_oracle as lo

AGREE = 1e-9
FIXTURES = gu.names("loss_")


def test_fixture_set():
    assert FIXTURES == ["loss_bce", "loss_j14_border", "loss_j17_focal", "loss_method4", "loss_zero_mask"]


@pytest.mark.parametrize("variant", ["mpn", "multi"])
@pytest.mark.parametrize("name", FIXTURES)
def test_oracle_reproduces_the_reference(name, variant):
    """loss_oracle in fp64 against the reference's fp64 terms and logit gradients, within 1e-9 max|.| per tensor,
    through explicit masks (the factories' path) and through the computed ones."""
    meta, a = gu.load(name)
    want = {k[len(variant) + 1:]: v for k, v in a.items() if k.startswith(variant + ".")}
    assert "terms" in want and f"g_pe{meta['K_e'] - 1}" in want and f"g_pn{meta['K_n'] - 1}" in want
    for masks in (True, False):
        got = lo.run(a, meta["variants"][variant], torch.float64, masks=masks)
        for k, v in want.items():
            scale = np.abs(v).max()
            assert np.abs(got[k] - v).max() <= AGREE * scale, (k, masks)
    assert (meta["oracle_vs_reference"][variant] <= AGREE)
    assert set(meta["reference_fp32_rel_err"][variant]) == set(want)


def test_zero_mask_fixture_takes_the_nan_rule():
    meta, a = gu.load("loss_zero_mask")
    opt = meta["variants"]["mpn"]
    pn = [torch.from_numpy(a[f"pn{k}"]).double() for k in range(meta["K_n"])]
    masks = lo.edge_masks(pn, torch.from_numpy(a["edge_index"]), torch.from_numpy(a["label_mask"]).double(),
                          torch.from_numpy(a["node_labels"]).double(), dict(lo.OPTIONS, **opt))
    sums = [float(m.sum()) for m in masks[:meta["K_e"]]]
    assert sums[1] == 0.0 and sums[0] > 0 and sums[2] > 0
    assert a["mpn.terms"][1] == 0.0 and a["mpn.terms"][0] > 0 and a["mpn.terms"][2] > 0
    assert not any(np.any(a[f"mpn.g_pe{k}"]) for k in range(meta["K_e"]))


def test_workspace_size_is_host_arithmetic():
    """Per edge block (one per 2048 edges, at most 1024) 2 K_e doubles, per node block (K_n per 256 nodes, at most
    64 K_n) 3 doubles, each array 256-byte aligned, plus 256; 0 outside the limits."""
    L = _lib.load_cdll()
    size = L.pemp_loss_workspace_size

    def want(N, E, K_e, K_n):
        al = lambda v: (v + 255) // 256 * 256
        nbe = min((E + _lib.LOSS_CHUNK - 1) // _lib.LOSS_CHUNK, 1024)
        nbn = min((N + 255) // 256, 64) * K_n
        return al(nbe * 2 * K_e * 8) + al(nbn * 3 * 8) + 256

    for N, E, K_e, K_n in ((0, 0, 1, 1), (1, 0, 1, 2), (41, 2047, 3, 4), (41, 2048, 3, 4), (41, 2049, 3, 4),
                           (1224, 186_048, 3, 4), (257, 10**7, 8, 9), (10**6, 3 * 10**9, 7, 8)):
        assert size(N, E, K_e, K_n) == want(N, E, K_e, K_n), (N, E, K_e, K_n)
    assert size(41, 4096, 3, 4) >= size(41, 2048, 3, 4)
    for bad in ((-1, 0, 1, 1), (1, -1, 1, 1), (1, 1, 0, 1), (1, 1, 9, 9), (1, 1, 1, 10), (1, 1, 1, 0)):
        assert size(*bad) == 0, bad


def test_record_mirror_matches_the_library():
    L = _lib.load_cdll()
    assert L.pemp_abi_struct_size(5) == ctypes.sizeof(_lib.PempLossRec)
    assert (_lib.LOSS_MAXKE, _lib.LOSS_MAXKN, _lib.LOSS_MAXJ) == (8, 9, 32)


def test_argument_errors_need_no_gpu():
    """Bad records are refused with a message before any HIP call (the pointers are never dereferenced)."""
    L = _lib.load_cdll()
    p = 0x1000

    def rec(**kw):
        r = _lib.PempLossRec(N=4, E=8, J=17, K_e=1, K_n=2, terms=7, alpha=1.0, gamma=2.0)
        r.pe[0] = r.pn[0] = r.pn[1] = r.pc[0] = r.pc[1] = p
        r.edge_index = r.edge_labels = r.label_mask = r.node_labels = r.label_mask_node = r.node_classes = p
        for k, v in kw.items():
            setattr(r, k, v)
        return r

    out = (ctypes.c_float * _lib.LOSS_OUT)()
    cases = [("negative", rec(N=-1), _lib.ERR_INVALID_ARG), ("K_e = 0", rec(K_e=0), _lib.ERR_INVALID_ARG),
             ("limits", rec(K_e=9), _lib.ERR_UNSUPPORTED), ("limits", rec(K_n=10), _lib.ERR_UNSUPPORTED),
             ("limits", rec(J=33), _lib.ERR_UNSUPPORTED), ("kind", rec(edge_kind=2), _lib.ERR_INVALID_ARG),
             ("terms", rec(terms=8), _lib.ERR_INVALID_ARG), ("K_n = 1 < K_e = 2", rec(K_e=2, K_n=1), _lib.ERR_INVALID_ARG),
             ("NULL edge_labels", rec(edge_labels=None), _lib.ERR_INVALID_ARG),
             ("NULL pn[1]", rec(K_n=3), _lib.ERR_INVALID_ARG)]
    for word, r, code in cases:
        if word.startswith("K_n = 1"):
            r.pe[1] = p
        assert L.pemp_loss_fwd(ctypes.byref(r), p, 1 << 20, out, None) == code, word
        assert word.split()[0] in L.pemp_last_error().decode(), (word, L.pemp_last_error())
        assert L.pemp_loss_bwd(ctypes.byref(r), out, None, None, None, None, None) == code, word
    assert L.pemp_loss_fwd(ctypes.byref(rec()), p, 16, out, None) == _lib.ERR_WORKSPACE
    assert L.pemp_loss_fwd(ctypes.byref(rec()), p, 1 << 20, None, None) == _lib.ERR_INVALID_ARG


def _cpu_inputs(K_e=1, K_n=2, J=17, N=5, E=6, dtype=torch.float32):
    pe = [torch.zeros(E, dtype=dtype) for _ in range(K_e)]
    pn = [torch.zeros(N, dtype=dtype) for _ in range(K_n)]
    pc = [torch.zeros(N, J, dtype=dtype) for _ in range(K_n)]
    rest = (torch.zeros(2, E, dtype=torch.int64), torch.zeros(E), torch.ones(E), torch.zeros(N), torch.ones(N),
            torch.zeros(N, dtype=torch.int64))
    return (pe, pn, pc) + rest


def test_refusals_come_before_the_library(monkeypatch):
    def no_lib():
        raise AssertionError("the library was touched")
    monkeypatch.setattr(_lib, "lib", no_lib)
    with pytest.raises(NotImplementedError, match="EDGE_WITH_LOGITS"):
        pl.mpn_loss(*_cpu_inputs(), USE_FOCAL=False, EDGE_WITH_LOGITS=False)
    cfg = pcfg.get_config()
    cfg.MODEL.LOSS.USE_FOCAL, cfg.MODEL.LOSS.EDGE_WITH_LOGITS = False, False
    for cls in (pl.MPNLoss, pl.ClassMPNLossFactory):
        with pytest.raises(NotImplementedError, match="EDGE_WITH_LOGITS"):
            cls(cfg)
    with pytest.raises(ValueError, match="preds_edge is empty"):
        pl.mpn_loss(*_cpu_inputs(K_e=0))
    with pytest.raises(NotImplementedError, match="K_e <= 8"):
        pl.mpn_loss(*_cpu_inputs(K_e=9, K_n=9))
    with pytest.raises(NotImplementedError, match="K_n <= 9"):
        pl.mpn_loss(*_cpu_inputs(K_e=8, K_n=10))
    with pytest.raises(NotImplementedError, match="J <= 32"):
        pl.mpn_loss(*_cpu_inputs(J=33))
    with pytest.raises(RuntimeError, match="HIP device only"):
        pl.mpn_loss(*_cpu_inputs())                                   # CPU tensors
    with pytest.raises(TypeError, match="float32"):
        pl.mpn_loss(*_cpu_inputs(dtype=torch.float64))
    with pytest.raises(TypeError, match="float32"):
        pl.mpn_loss(*_cpu_inputs(dtype=torch.float16))
    with pytest.raises(TypeError, match="unknown option"):
        pl.mpn_loss(*_cpu_inputs(), GAMMA=2.0)


def test_config_defaults_read_back():
    """MODEL.LOSS of default_config.py:30-46; a YAML-style merge takes LOSS_WEIGHTS (the experiment files' key)."""
    cfg = pemp_amd.config.get_config()
    want = dict(NAME=["edge_loss"], NODE_WEIGHT=1.0, EDGE_WEIGHT=1.0, CLASS_WEIGHT=1.0, TAG_WEIGHT=1.0, SYNC_TAGS=False,
                SYNC_GT_TAGS=False, USE_FOCAL=True, EDGE_WITH_LOGITS=True, NODE_USE_FOCAL=True, FOCAL_ALPHA=1.0,
                FOCAL_GAMMA=2.0, NODE_BCE_POS_WEIGHT=1.0, EDGE_BCE_POS_WEIGHT=1.0, INCLUDE_BORDERING_NODES=False)
    assert dict(cfg.MODEL.LOSS) == want
    opt = pl.loss_options(cfg)
    assert opt == pl.DEFAULTS and pl.MPNLoss(cfg).options["TERMS"] == ("edge",)
    cfg.merge({"MODEL": {"LOSS": {"NAME": ["edge", "node", "class"], "LOSS_WEIGHTS": [1.0, 2, 0.5], "FOCAL_GAMMA": 1},
                         "MPN": {"NODE_THRESHOLD": 0.5}}})
    opt = pl.MPNLoss(cfg).options
    assert (opt["NODE_WEIGHT"], opt["EDGE_WEIGHT"], opt["CLASS_WEIGHT"]) == (1.0, 2, 0.5)
    assert opt["NODE_THRESHOLD"] == 0.5 and opt["FOCAL_GAMMA"] == 1.0 and opt["TERMS"] == ("node", "edge", "class")
    cfg.MODEL.LOSS.LOSS_WEIGHTS = [1.0, 3.0]
    assert pl.loss_options(cfg)["CLASS_WEIGHT"] == 1.0 and pl.loss_options(cfg)["EDGE_WEIGHT"] == 3.0
    cfg.MODEL.LOSS.LOSS_WEIGHTS = [1.0]
    with pytest.raises(ValueError):
        pl.loss_options(cfg)
    cfg.MODEL.LOSS.NAME = "edge_loss"
    del cfg.MODEL.LOSS["LOSS_WEIGHTS"]
    with pytest.raises(NotImplementedError):
        pl.MPNLoss(cfg)


def test_exported_from_the_package():
    assert pemp_amd.mpn_loss is pl.mpn_loss and pemp_amd.MPNLoss is pl.MPNLoss
    assert pemp_amd.ClassMPNLossFactory is pl.ClassMPNLossFactory
    assert pemp_amd.mask_node_connections is pl.mask_node_connections


def test_mask_node_connections_on_the_cpu():
    """Pure torch ops: any device; equal to the oracle, bool, and the argument is not written."""
    g = torch.Generator().manual_seed(3)
    p = torch.rand(9, generator=g)
    keep = p.clone()
    ei = torch.randint(0, 9, (2, 40), generator=g)
    labels = (torch.rand(9, generator=g) < 0.3).float()
    for border in (False, True):
        m = pl.mask_node_connections(p, ei, 0.5, labels, include_bordering_nodes=border)
        assert m.dtype == torch.bool and torch.equal(m, lo.mask_node_connections(p, ei, 0.5, labels, border))
        sel = p > 0.5                                   # the reference's form: the labelled nodes written in place
        sel[labels == 1.0] = True
        want = (sel[ei[0]] | sel[ei[1]]) if border else (sel[ei[0]] & sel[ei[1]])
        assert torch.equal(m, want) and 0 < int(m.sum()) < m.numel()
    assert torch.equal(p, keep)
    assert torch.equal(pl.mask_node_connections(p, ei, 0.5), (p > 0.5)[ei[0]] & (p > 0.5)[ei[1]])
