"""The keypoint losses on the device: the heatmap and associative-embedding terms of the reference's
``ClassMultiLossFactory`` (``Utils/loss.py:641-665``; ``HeatmapLoss`` ``:17-27``, ``AELoss`` ``:37-98``) over all
stages as one fused HIP pass each way (``csrc/kp_loss.hip``, ``pemp.h`` pemp_kp_loss_*), and the factory itself.

* ``keypoint_loss(...)``: the functional form, ``(total, terms)``; one ``torch.autograd.Function``.
* ``KeypointLoss(config)``: an ``nn.Module`` over the per-stage lists.
* ``ClassMultiLossFactory(config)``: the reference's ``forward(outputs, labels, masks, graph) -> (loss, logging)``;
  the node / edge / class part goes through ``loss.mpn_loss``, unchanged.

The forward is two launches, the backward at most two; neither synchronises the host. ``terms`` = (heatmap, ae,
total) stays on the device: a caller that logs reads it once. Not built (refused with the reference's lines):
``"tag_loss"`` (``NodeAELoss`` on MPN-predicted tags, ``:622-623, 691-747``), ``SYNC_TAGS``, ``SYNC_GT_TAGS``.
"""
import ctypes
import os

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from . import loss as _loss
from .mpn.train import _device_f32

KP_DEFAULTS = dict(NUM_JOINTS=17, WITH_HEATMAPS_LOSS=(True, True), HEATMAPS_LOSS_FACTOR=(1.0, 1.0),
                   WITH_AE_LOSS=(False, False), AE_LOSS_TYPE="exp", PUSH_LOSS_FACTOR=(0.001, 0.001),
                   PULL_LOSS_FACTOR=(0.001, 0.001))
AE_KINDS = {"exp": _lib.KP_AE_EXP, "max": _lib.KP_AE_MAX}
_VALIDATE = os.environ.get("PEMP_VALIDATE", "0") not in ("", "0")   # read once at import


def _names_of(config):
    names = config["MODEL"]["LOSS"].get("NAME")
    if isinstance(names, str):
        raise NotImplementedError("MODEL.LOSS.NAME must be a list of the losses to use (Utils/loss.py:544-547)")
    return list(names or ())


def kp_options(cfg_or_kwargs=None, **over):
    """The keypoint losses' options as a plain dict (``KP_DEFAULTS`` keys) from a config or from keyword options.

    From a config, as ``ClassMultiLossFactory.__init__`` reads it (``:567-604``): with ``"heatmap"`` in
    ``MODEL.LOSS.NAME``, ``MODEL.KP`` hrnet / mmpose_hrnet takes ``MODEL.HRNET.LOSS.WITH_HEATMAPS_LOSS`` and
    ``HEATMAPS_LOSS_FACTOR``, hourglass ``MODEL.HG.NSTACK`` stages of factor 1.0; with ``"tagmap"``,
    ``TRAIN.WITH_AE_LOSS`` (not the HRNET key) with ``MODEL.HRNET.LOSS.{AE_LOSS_TYPE, PUSH_LOSS_FACTOR,
    PULL_LOSS_FACTOR}``, and hourglass is refused (``:588``). A term the list does not name is switched off."""
    opt = dict(KP_DEFAULTS)
    src = cfg_or_kwargs
    if src is not None and "MODEL" in src:
        names = _names_of(src)
        model = src["MODEL"]
        lcfg = model.get("LOSS", {})
        if "tag_loss" in names:
            raise NotImplementedError("pemp_amd kp_loss: 'tag_loss' (NodeAELoss on MPN-predicted tags, Utils/loss.py:"
                                      "622-623, 691-747) is not built: this MPN predicts no tags")
        if lcfg.get("SYNC_TAGS", False):
            raise NotImplementedError("pemp_amd kp_loss: MODEL.LOSS.SYNC_TAGS (Utils/loss.py:733-741) is not built")
        if lcfg.get("SYNC_GT_TAGS", False):
            raise NotImplementedError("pemp_amd kp_loss: MODEL.LOSS.SYNC_GT_TAGS (Utils/loss.py:704-731) is not built")
        kp = model.get("KP", "hrnet")
        hr = model.get("HRNET", {})
        hl = hr.get("LOSS", {})
        opt["NUM_JOINTS"] = hr.get("NUM_JOINTS", opt["NUM_JOINTS"])
        nstack = model.get("HG", {}).get("NSTACK", 4)
        opt["WITH_HEATMAPS_LOSS"] = opt["WITH_AE_LOSS"] = ()
        if "heatmap" in names:
            if kp in ("hrnet", "mmpose_hrnet"):
                opt["WITH_HEATMAPS_LOSS"] = tuple(hl.get("WITH_HEATMAPS_LOSS", KP_DEFAULTS["WITH_HEATMAPS_LOSS"]))
                opt["HEATMAPS_LOSS_FACTOR"] = tuple(hl.get("HEATMAPS_LOSS_FACTOR", KP_DEFAULTS["HEATMAPS_LOSS_FACTOR"]))
            elif kp == "hourglass":
                opt["WITH_HEATMAPS_LOSS"] = (True,) * nstack
                opt["HEATMAPS_LOSS_FACTOR"] = (1.0, 1.0, 1.0, 1.0)
        if "tagmap" in names:
            if kp == "hourglass":
                raise NotImplementedError("pemp_amd kp_loss: 'tagmap' with MODEL.KP hourglass (Utils/loss.py:588 asserts)")
            opt["WITH_AE_LOSS"] = tuple(src.get("TRAIN", {}).get("WITH_AE_LOSS", KP_DEFAULTS["WITH_AE_LOSS"]))
            if not any(opt["WITH_AE_LOSS"]):
                raise ValueError("pemp_amd kp_loss: 'tagmap' with no stage set in TRAIN.WITH_AE_LOSS (Utils/loss.py:594)")
            opt["AE_LOSS_TYPE"] = hl.get("AE_LOSS_TYPE", opt["AE_LOSS_TYPE"])
            opt["PUSH_LOSS_FACTOR"] = tuple(hl.get("PUSH_LOSS_FACTOR", opt["PUSH_LOSS_FACTOR"]))
            opt["PULL_LOSS_FACTOR"] = tuple(hl.get("PULL_LOSS_FACTOR", opt["PULL_LOSS_FACTOR"]))
    elif src is not None:
        for k, v in src.items():
            if k not in opt:
                raise TypeError(f"keypoint_loss: unknown option {k}")
            opt[k] = v
    for k, v in over.items():
        if k not in opt:
            raise TypeError(f"keypoint_loss: unknown option {k}")
        opt[k] = v
    if opt["AE_LOSS_TYPE"] not in AE_KINDS:
        raise ValueError(f"pemp_amd kp_loss: unknown AE_LOSS_TYPE {opt['AE_LOSS_TYPE']!r} (Utils/loss.py:82-83)")
    return opt


def _flags(name, seq, S):
    """The per-stage switches; an empty list switches the term off, a short one is an error (the reference indexes it)."""
    if 0 < len(seq) < S:
        raise ValueError(f"pemp_amd kp_loss: {name} has {len(seq)} entries for {S} stages")
    return [bool(seq[s]) if seq else False for s in range(S)]


def _shaped(name, t, dev, shape):
    t = _device_f32(name, t)
    if t.device != dev:
        raise RuntimeError(f"{name} lies on {t.device}, preds[0] on {dev}")
    if tuple(t.shape) != tuple(shape):
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected {tuple(shape)}")
    return t


def _tags_on(name, t, dev, B, J):
    """int32 [B, P, J, 2] on ``dev``: moved once, without a host synchronisation."""
    if not isinstance(t, torch.Tensor) or t.dtype not in (torch.int32, torch.int64):
        raise TypeError(f"{name}: expected an int32 or int64 tensor (got {getattr(t, 'dtype', type(t))})")
    if t.dim() != 4 or t.shape[0] != B or t.shape[2] != J or t.shape[3] != 2:
        raise ValueError(f"{name}: shape {tuple(t.shape)}, expected ({B}, P, {J}, 2)")
    if t.shape[1] > _lib.KP_MAXP:
        raise NotImplementedError(f"pemp_amd kp_loss: P = {t.shape[1]} persons (limit: P <= {_lib.KP_MAXP})")
    if t.device.type == "cuda" and t.device != dev:
        raise RuntimeError(f"{name} lies on {t.device}, preds[0] on {dev}")
    t = t.to(dev, non_blocking=True)
    if t.dtype == torch.int64:      # an index beyond int32 is out of range for every map: keep it so
        t = t.clamp(-1, 2 ** 31 - 1).to(torch.int32)
    return t.contiguous()


def build_record(opt, preds, heatmaps_gt, masks, tag_targets):
    """``(rec, held)``: the ``pemp_kp_loss_rec`` of one call (``_lib.PempKpLossRec``) after the refusals and the input
    checks, and the tensors its raw pointers point into as four per-stage lists (preds, gt, masks, tags; ``None``
    where a stage does not read one): whoever keeps ``rec`` keeps ``held``. Touches no library."""
    preds = list(preds)
    S, J = len(preds), int(opt["NUM_JOINTS"])
    if S > _lib.KP_MAXS:
        raise NotImplementedError(f"pemp_amd kp_loss: {S} stages (limit: S <= {_lib.KP_MAXS})")
    if J > _lib.KP_MAXJ:
        raise NotImplementedError(f"pemp_amd kp_loss: J = {J} joints (limit: J <= {_lib.KP_MAXJ})")
    if S == 0 or J < 1:
        raise ValueError(f"pemp_amd kp_loss: {S} stages, J = {J}")
    heat = _flags("WITH_HEATMAPS_LOSS", opt["WITH_HEATMAPS_LOSS"], S)
    ae = _flags("WITH_AE_LOSS", opt["WITH_AE_LOSS"], S)
    for key, on in (("HEATMAPS_LOSS_FACTOR", heat), ("PUSH_LOSS_FACTOR", ae), ("PULL_LOSS_FACTOR", ae)):
        if any(on) and len(opt[key]) <= max(s for s in range(S) if on[s]):
            raise ValueError(f"pemp_amd kp_loss: {key} has {len(opt[key])} entries for {S} stages")
    for name, seq, on in (("heatmaps_gt", heatmaps_gt, heat), ("masks", masks, heat), ("tag_targets", tag_targets, ae)):
        if any(on) and (seq is None or len(seq) <= max(s for s in range(S) if on[s])):
            raise ValueError(f"pemp_amd kp_loss: {name} has {0 if seq is None else len(seq)} entries for {S} stages")
    for s, t in enumerate(preds):
        _device_f32(f"preds[{s}]", t)
        if t.dim() != 4:
            raise ValueError(f"preds[{s}]: shape {tuple(t.shape)}, expected (B, C, H, W)")
    dev, B = preds[0].device, preds[0].shape[0]
    if B < 1:
        raise ValueError("pemp_amd kp_loss: empty batch")
    rec = _lib.PempKpLossRec(S=S, B=B, J=J, P=0, ae_kind=AE_KINDS[opt["AE_LOSS_TYPE"]])
    held = ([], [], [], [])
    P = None
    for s in range(S):
        C, H, W = preds[s].shape[1:]
        p = _shaped(f"preds[{s}]", preds[s], dev, (B, C, H, W))
        if C < J or (ae[s] and C == J):
            raise ValueError(f"preds[{s}]: {C} channels for J = {J}" + (" and a tag plane" if ae[s] else ""))
        if min(H, W) < 1 or C * H * W > 2 ** 31 - 1 - 2 * _lib.KP_CHUNK:
            raise ValueError(f"preds[{s}]: C H W = {C * H * W} per image (1 .. 2^31 - 1 - {2 * _lib.KP_CHUNK})")
        g = _shaped(f"heatmaps_gt[{s}]", heatmaps_gt[s], dev, (B, J, H, W)) if heat[s] else None
        m = _shaped(f"masks[{s}]", masks[s], dev, (B, H, W)) if heat[s] else None
        t = _tags_on(f"tag_targets[{s}]", tag_targets[s], dev, B, J) if ae[s] else None
        if t is not None:
            if P is not None and t.shape[1] != P:
                raise ValueError(f"tag_targets[{s}]: P = {t.shape[1]}, an earlier stage has {P}")
            P = t.shape[1]
            if P < 1:
                raise ValueError(f"tag_targets[{s}]: no person slots")
        st = rec.stage[s]
        st.pred, st.gt, st.mask, st.tag = p.data_ptr(), _lib.ptr(g), _lib.ptr(m), _lib.ptr(t)
        st.C, st.H, st.W, st.with_heatmap, st.with_ae = C, H, W, int(heat[s]), int(ae[s])
        st.heatmap_factor = float(opt["HEATMAPS_LOSS_FACTOR"][s]) if heat[s] else 0.0
        st.push_factor = float(opt["PUSH_LOSS_FACTOR"][s]) if ae[s] else 0.0
        st.pull_factor = float(opt["PULL_LOSS_FACTOR"][s]) if ae[s] else 0.0
        for lst, v in zip(held, (p, g, m, t)):
            lst.append(v)
    rec.P = P or 0
    return rec, held


def _point(rec, held):
    for s, (p, g, m, t) in enumerate(zip(*held)):
        st = rec.stage[s]
        st.pred, st.gt, st.mask, st.tag = p.data_ptr(), _lib.ptr(g), _lib.ptr(m), _lib.ptr(t)


def backward_into(rec, ws, grad_total, g_preds):
    """``pemp_kp_loss_bwd`` into caller-owned gradients (``None`` entries are skipped); ``ws`` the forward's."""
    arr = (_lib.c_p * _lib.KP_MAXS)()
    for s, g in enumerate(g_preds):
        arr[s] = _lib.ptr(g)
    dev = ws.device
    _lib.check(_lib.lib().pemp_kp_loss_bwd(ctypes.byref(rec), ws.data_ptr(), _lib.ptr(grad_total),
                                           ctypes.cast(arr, _lib.c_p), _lib.stream(dev)))


class _KpLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, opt, heatmaps_gt, masks, tag_targets, validate, *preds):
        rec, held = build_record(opt, preds, heatmaps_gt, masks, tag_targets)
        dev = held[0][0].device
        L = _lib.lib()
        nbytes = L.pemp_kp_loss_workspace_size(ctypes.byref(rec))
        # a buffer per call, not a shared one: the backward reads what the AE blocks left in it
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        out = torch.empty(_lib.KP_OUT, dtype=torch.float32, device=dev)
        _lib.check(L.pemp_kp_loss_fwd(ctypes.byref(rec), ws.data_ptr(), ws.numel(), out.data_ptr(), _lib.stream(dev)))
        if validate:
            bad = int(ws[:4].view(torch.int32).item())
            if bad:
                raise ValueError(f"keypoint_loss: {bad} visible tag entries with an index outside [0, (C - J) H W) "
                                 "(the reference raises IndexError)")
        # the record holds raw pointers into `held`; the tensors go through save_for_backward, so that a map written
        # in place before the backward (which recomputes from it) is caught by autograd's version check
        flat = [t for lst in held for t in lst if t is not None]
        ctx.save_for_backward(ws, *flat)
        ctx.rec, ctx.layout = rec, [[t is not None for t in lst] for lst in held]
        ctx.shapes = [t.shape for t in preds]
        total, terms = out[2], out[:3]
        ctx.mark_non_differentiable(terms)
        return total, terms

    @staticmethod
    @once_differentiable
    def backward(ctx, grad_total, _grad_terms):
        ws, *flat = ctx.saved_tensors
        it = iter(flat)
        held = [[next(it) if has else None for has in row] for row in ctx.layout]
        rec = ctx.rec
        _point(rec, held)
        dev = ws.device
        gt = grad_total.to(device=dev, dtype=torch.float32).reshape(1).contiguous()
        need = ctx.needs_input_grad[5:]
        g = [torch.empty_like(p) if need[s] else None for s, p in enumerate(held[0])]
        backward_into(rec, ws, gt, g)
        return (None,) * 5 + tuple(None if t is None else t.view(shape) for t, shape in zip(g, ctx.shapes))


def keypoint_loss(preds, heatmaps_gt, masks, tag_targets, cfg_or_kwargs=None, validate=None, **options):
    """``(total, terms)`` of the heatmap and associative-embedding losses over ``S <= 4`` stages.

    ``preds[s]``: [B, C_s, H_s, W_s] with ``C_s >= J``; a non-contiguous one is copied once (the channel slice of the
    heatmap planes never is: they are read in place). ``heatmaps_gt[s]``: [B, J, H_s, W_s]; ``masks[s]``: [B, H_s, W_s],
    any float values; ``tag_targets[s]``: int32 / int64 [B, P <= 32, J, 2] rows (index, visible), on the host or the
    device (moved once, not synchronised); entries of stages that do not use them may be ``None``.
    ``cfg_or_kwargs``: a config (see ``kp_options``) or a dict of ``KP_DEFAULTS`` keys; keyword options override it.
    ``validate`` (default: ``PEMP_VALIDATE=1``): read the status word after the forward (one host synchronisation) and
    raise ``ValueError`` when a visible tag entry's index lies outside its stage's tag planes; without it such an entry
    is skipped. fp32 HIP tensors. ``total`` is differentiable in every ``preds[s]``; ``terms`` = (heatmap, ae, total)
    [3] carries no gradient."""
    opt = kp_options(cfg_or_kwargs, **options)
    preds = list(preds)
    # refusals and input errors before the library loads; the tags move to the device here, once
    _, (_, gts, ms, tags) = build_record(opt, preds, heatmaps_gt, masks, tag_targets)
    return _KpLoss.apply(opt, gts, ms, tags, _VALIDATE if validate is None else bool(validate), *preds)


class KeypointLoss(torch.nn.Module):
    """The heatmap and associative-embedding losses of one training step. Reads ``MODEL.KP``,
    ``MODEL.HRNET.NUM_JOINTS``, ``MODEL.HRNET.LOSS.*``, ``MODEL.HG.NSTACK``, ``TRAIN.WITH_AE_LOSS`` and
    ``MODEL.LOSS.NAME`` (``kp_options``)."""

    def __init__(self, config, validate=None):
        super().__init__()
        self.options = kp_options(config)
        self.validate = validate

    @property
    def active(self):
        return any(self.options["WITH_HEATMAPS_LOSS"]) or any(self.options["WITH_AE_LOSS"])

    def forward(self, preds, heatmaps_gt, masks, tag_targets=None):
        """Per-stage lists as ``keypoint_loss`` takes them. Returns ``(total, terms)``."""
        return keypoint_loss(preds, heatmaps_gt, masks, tag_targets, self.options, validate=self.validate)


class ClassMultiLossFactory(torch.nn.Module):
    """``Utils/loss.py:539-758`` for outputs without MPN-predicted tags: ``forward(outputs, labels, masks, graph)`` over
    the dicts train.py:119-154 builds returns ``(loss, logging)`` with the reference's keys. ``outputs["heatmap"]``,
    ``labels["heatmap"]``, ``labels["tag"]`` and ``masks["heatmap"]`` are the per-stage lists; the edge / node / class
    entries are the ones ``loss.ClassMPNLossFactory`` takes, weighted by ``MODEL.LOSS.{NODE, EDGE, CLASS}_WEIGHT``
    (``LOSS_WEIGHTS`` is not read here, ``:551-554``). The class term has the four-argument meaning of
    ``ClassMPNLossFactory:850`` (``:687`` raises ``TypeError`` as shipped). ``graph`` is accepted and not read. The two
    totals are added on the device; the logging floats come from one host read."""

    def __init__(self, config, validate=None):
        super().__init__()
        names = _names_of(config)
        self.kp = KeypointLoss(config, validate)
        lcfg = {k: v for k, v in config["MODEL"]["LOSS"].items() if k != "LOSS_WEIGHTS"}
        if "node" in names and not lcfg.get("NODE_USE_FOCAL", True):
            raise NotImplementedError("pemp_amd loss: NODE_USE_FOCAL False (Utils/loss.py:618-619 raises)")
        terms = tuple(t for t in ("node", "edge", "class") if t in names)
        self.mpn_options = None
        if terms:
            self.mpn_options = _loss.loss_options(lcfg, TERMS=terms)
            th = config["MODEL"].get("MPN", {}).get("NODE_THRESHOLD")
            if th is not None:
                self.mpn_options["NODE_THRESHOLD"] = th
            _loss._refusals(self.mpn_options, 1, 1, None)

    def forward(self, outputs, labels, masks, graph=None):
        total, parts = None, []
        if self.mpn_options is not None:
            if "refine" in outputs:
                raise NotImplementedError("pemp_amd loss: the refine regression term is not built")
            pe = outputs["edge"]
            el = labels["edge"]
            el = list(el) if isinstance(el, (list, tuple)) else [el] * len(pe)
            edge_masks = list(masks["edge"])
            if len(el) < len(pe) or len(edge_masks) < len(pe):
                raise ValueError(f"pemp_amd loss: {len(el)} edge labels / {len(edge_masks)} edge masks for {len(pe)} "
                                 "edge predictions")
            if any(t is not el[0] and (t.data_ptr() != el[0].data_ptr() or t.shape != el[0].shape) for t in el):
                raise NotImplementedError("pemp_amd loss: one edge label tensor for every prediction (train.py:149)")
            pc, classes = outputs.get("class"), labels.get("class")
            total, mt = _loss.mpn_loss(pe, outputs["node"], pc, None, el[0], edge_masks[0], labels["node"],
                                       masks["node"], classes if pc is not None else None, self.mpn_options,
                                       edge_masks=edge_masks[:len(pe)])
            parts.append(mt)
        if self.kp.active:
            kt, kterms = self.kp(outputs["heatmap"], labels["heatmap"], masks["heatmap"], labels.get("tag"))
            total = kt if total is None else total + kt
            parts.append(kterms)
        if total is None:
            raise ValueError("pemp_amd loss: MODEL.LOSS.NAME names no loss that is built")
        vals = torch.cat(parts + [total.detach().reshape(1)]).tolist()
        loss = vals.pop()
        node = edge = cls = heat = ae = 0.0
        if self.mpn_options is not None:
            node, edge, cls = vals[:3]
            vals = vals[4:]
            o = self.mpn_options
            node, edge, cls = node * o["NODE_WEIGHT"], edge * o["EDGE_WEIGHT"], cls * o["CLASS_WEIGHT"]
        if self.kp.active:
            heat, ae = vals[:2]
        return total, {"heatmap": heat, "tag_loss": ae, "edge": edge, "node": node, "class_loss": cls, "loss": loss}
