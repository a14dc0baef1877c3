"""Drop-in ``NaiveGraphConstructor`` (``src/graph_constructor/ConstructGraph.py:9-249``): the inference path, and
with ``joints_gt`` the training labels of EDGE_LABEL_METHOD 4 and 6 (``pemp_label_candidates`` /
``pemp_label_assign`` / ``pemp_label_edges``).

Same constructor signature, same ``construct_graph()`` 15-tuple, same dtypes (int64 indices) and
node/edge order as the reference; computed by ``libpemp.so`` (``pemp_detect``,
``pemp_pack_nodes``, ``pemp_fully_graph_build`` / ``pemp_knn_graph_*`` / ``pemp_score_graph``,
``pemp_edge_features``). GRAPH_TYPE fully, knn, feature_knn and score_based (``ConstructGraph.py:272-283``).
Host synchronisation: one count read-back after detection (the reference syncs at every
``nonzero``), plus one more for knn graphs.
"""
import ctypes
import math
import threading

import numpy as np
import torch

from . import _lib
from .frontend import ProjectedHeatmaps, ProjectedMaps

_SCORE_BASED_K = 75        # ConstructGraph.py:280 (score_based_graph roots)
# EDGE_FEATURES_TO_USE -> (mode code PEMP_EF_*, (a, b) of the edge_attr width A = a J + b: ef_width() of graph.hip)
_EF_MODES = {
    frozenset(["position", "connection_type"]): (0, (1, 2)),
    frozenset(["connection_type"]): (1, (1, 0)),
    frozenset(["nothing"]): (2, (0, 1)),
    frozenset(["position"]): (3, (0, 2)),
    frozenset(["position", "angle", "connection_type"]): (4, (1, 3)),
    frozenset(["position", "connection_type", "ae_normed"]): (5, (1, 3)),   # associative-embedding modes,
    frozenset(["ae"]): (6, (0, 1)),                                         # ConstructGraph.py:337-357
    frozenset(["ae_normed"]): (7, (0, 1)),
    frozenset(["ae_tracking_1"]): (8, (0, 1)),
}
_EF_TAG_MODES = (5, 6, 7, 8)


def _align256(n):
    return (n + 255) // 256 * 256


def _fully_edges(counts_l):
    """Edges of the batch's fully graph: every ordered pair of an image's detections."""
    return sum(c * (c - 1) for c in counts_l if c > 1)


def _fits(counts_l, cap, n_cap, e_cap):
    """(N, E) of a batch that fit the capacities its capacity build ran under, else None (it wrote nothing)."""
    N, E = sum(counts_l), _fully_edges(counts_l)
    if (max(counts_l) if counts_l else 0) > cap or N > n_cap or E > e_cap:
        return None
    return N, E


def _tag_fully(edge_index, node_off, counts, joint_det):
    """Mark edge_index as this batch's fully graph (per-image node offsets on the device, counts on
    the host) so that the MPN can take pemp_mpn_forward_fully; the versions detect in-place edits."""
    edge_index._pemp_fully = (node_off, tuple(counts), joint_det, joint_det._version, edge_index._version)


def _tag_sym(edge_index):
    """Mark edge_index as a (src, dst)-sorted symmetric graph without duplicates (PyG to_undirected's output:
    knn, feature_knn, score_based), so that the MPN can take pemp_mpn_forward_sym; the version detects in-place
    edits. The tag is only a hint: writes the version counter does not see (through .data, raw pointers from
    ctypes / DLPack / another library) keep it, and such an edited list then breaks the contract of
    pemp_mpn_forward_sym. The library flags a broken contract in its workspace; the MPN reads that flag whenever
    it validates (validate=True, PEMP_VALIDATE=1) and also under PEMP_DEBUG_SYNC=1."""
    edge_index._pemp_sym = edge_index._version


def _tag_knn(edge_index, ws, offs, node_off, node_off_h):
    """Hand the knn build's bit rows to the MPN (pemp_mpn_forward_knn): ws is that call's own workspace (kept
    alive by the tag, never reused by a later build), offs the byte offsets of its rows / row starts / edge
    counts (pemp_knn_rows_layout); the version detects in-place edits of edge_index."""
    edge_index._pemp_knn = (ws, offs, node_off, node_off_h, edge_index._version)


class _Call:
    """What the host derives from one construct_graph call's inputs, filled once before the first launch: the detection
    half here (ahead of the count buffer), the graph half in graph() (the generator's first step). src_obj is the dense
    scoremaps or (proj) the pemp_proj_maps of a ProjectedHeatmaps; the features are dense (feats) or ProjectedMaps
    (pmaps, pconv their feature_gather conv or None); the tags are absent, dense (tags) or projected (ptags). grad: how
    x carries a gradient into the features (NaiveGraphConstructor._grad_kind; None: it does not), the tensors that take
    it being feats, pmaps[0] and plive (the conv's live weight and bias)."""
    __slots__ = ("L", "st", "dev", "B", "J", "H", "W", "proj", "src_obj", "src", "detect", "masks", "use_thr", "topk",
                 "thr", "pool", "feats", "pmaps", "pconv", "divisor", "tags", "ptags", "C", "F", "A", "mode", "norm",
                 "fully", "gkey", "counts_h", "grad", "plive")

    def __init__(self, gc, L, st, grad=None):
        self.L, self.st, self.grad, self.plive = L, st, grad, None
        sm = gc.scoremaps
        self.proj = isinstance(sm, ProjectedHeatmaps)   # the test front-end evaluated inside the detection
        if self.proj:
            self.src_obj = sm.c_struct()
            self.src, self.detect = ctypes.addressof(self.src_obj), L.pemp_detect_projected
        else:
            if sm.dtype != torch.float32:
                sm = sm.float()
            self.src_obj = sm = sm.contiguous()
            self.src, self.detect = sm.data_ptr(), L.pemp_detect
        self.B, self.J, self.H, self.W = sm.shape
        if self.J != gc.num_joints:
            raise ValueError(f"scoremaps have {self.J} types, num_joints={gc.num_joints}")
        if gc.mask_crowds and gc.masks is None:
            raise TypeError("MASK_CROWDS is set but masks is None")   # reference: masks[batch] on None
        self.masks = gc.masks.float().contiguous() if gc.mask_crowds else None
        self.use_thr = use_thr = gc.detect_threshold is not None
        self.topk, self.thr = (gc.hybrid_k, float(gc.detect_threshold)) if use_thr else (20, 0.0)
        self.pool, self.dev = gc.pool_kernel_size, sm.device

    def graph(self, gc, counts_h):
        """The graph half: features, tags, edge-feature mode and the path's keys, with construct_graph's checks."""
        J, H, W = self.J, self.H, self.W
        feats, tags = gc.features, gc.tagmaps
        pmaps = pconv = divisor = ptags = None
        if isinstance(feats, ProjectedMaps):   # x sampled from the projected maps after the graph build
            if feats.size != (H, W):
                raise ValueError(f"ProjectedMaps size {feats.size} != scoremap size {(H, W)}")
            pmaps = [m.float().contiguous() for m in feats.maps]
            C, divisor = feats.shape[1], feats.divisor
            pconv = feats.conv_params() if feats.gather is not None else None
            if self.grad == "conv":
                self.plive = feats.live_params()
            feats = None
        else:
            if feats.dtype != torch.float32:
                feats = feats.float()
            feats = feats.contiguous()
            C = feats.shape[1]
        F = 1
        if isinstance(tags, ProjectedHeatmaps):   # sampled at the detections after the build
            if not tags.has_tags:
                raise ValueError(f"ProjectedHeatmaps has {tags.outputs[0].shape[1]} channels: no tag channels")
            ptags, tags, F = tags, None, tags.tag_dims
        elif tags is not None:
            tags = tags.float().contiguous()
            F = math.prod(tags.shape[4:])
        ef = _EF_MODES.get(frozenset(gc.edge_features_to_use))
        if ef is None:
            raise NotImplementedError(f"EDGE_FEATURES_TO_USE={gc.edge_features_to_use}")
        mode, (a, b) = ef
        if mode in _EF_TAG_MODES and tags is None and ptags is None:
            raise TypeError(f"EDGE_FEATURES_TO_USE={gc.edge_features_to_use} needs tagmaps")
        if mode in _EF_TAG_MODES and F != {6: 1, 7: 2}.get(mode, F if F in (1, 2) else 0):
            # (ef_tag_check of graph.hip would refuse the same, after the detection has run and without the option's name)
            raise NotImplementedError(f"EDGE_FEATURES_TO_USE={gc.edge_features_to_use} with {F} tag dims per node: ae "
                                      "takes 1, ae_normed 2, the other tag modes 1 or 2")
        self.feats, self.pmaps, self.pconv, self.divisor, self.tags = feats, pmaps, pconv, divisor, tags
        self.ptags, self.C, self.F, self.A, self.mode, self.counts_h = ptags, C, F, a * J + b, mode, counts_h
        self.norm = float(max(W, H)) if gc.normalize_node_distance else 1.0
        # (projected tags feeding the edge features: the generic path, which samples them before the features)
        self.fully = (gc.mpn_graph_type == "fully" and self.B <= 1024
                      and not (ptags is not None and mode in _EF_TAG_MODES))
        self.gkey = (self.B, J, H, W, C, F, self.A, self.dev)


class _StepPlan:
    """A pemp_step_plan (include/pemp.h) for one batch shape, capacity set and forward, with the workspaces it names
    kept alive; outputs() cuts one call's output buffer into construct_graph's tensors."""

    def __init__(self, c, cap, det_ws, n_cap, e_cap, mi):
        F = c.F if c.tags is not None else 0
        p = _lib.PempStepPlan(B=c.B, J=c.J, H=c.H, W=c.W, pool_kernel=c.pool, use_threshold=int(c.use_thr),
                              topk=c.topk, det_cap=cap, projected=int(c.proj), threshold=c.thr,
                              det_workspace=det_ws.data_ptr(), det_workspace_bytes=det_ws.numel(), C=c.C, F=F, A=c.A,
                              mode=c.mode, norm_factor=c.norm, n_cap=n_cap, e_cap=e_cap)
        self.mi = mi                                     # (desc, folded weights, workspace, key): kept alive here
        if mi is not None:
            p.desc = ctypes.pointer(mi[0])
            p.weights = ctypes.pointer(mi[1].struct)
            p.mpn_workspace = mi[2].data_ptr()
            p.mpn_workspace_bytes = mi[2].numel()
        if not c.L.pemp_step_layout(ctypes.byref(p)):
            raise ValueError(c.L.pemp_last_error().decode())
        self.struct, self.ref, self.det_ws = p, ctypes.byref(p), det_ws
        self.B, self.cap, self.C, self.F, self.A = c.B, cap, c.C, F, c.A
        self.off = [p.off[i] for i in range(_lib.STEP_NOUT)]

    def detections(self, flat):
        """(workspace, det_xyt [B, cap, 3], det_scores [B, cap], n_det [B]) of the call that wrote flat."""
        o, B, cap = self.off, self.B, self.cap
        i64, f32, i32 = flat.view(torch.int64), flat.view(torch.float32), flat.view(torch.int32)
        return (self.det_ws, i64.as_strided((B, cap, 3), (3 * cap, 3, 1), o[_lib.STEP_DET] // 8),
                f32.as_strided((B, cap), (cap, 1), o[_lib.STEP_DSC] // 4),
                i32.as_strided((B,), (1,), o[_lib.STEP_NDET] // 4))

    def outputs(self, flat, counts_l, mpn):
        """(node arrays, edge_attr, edge_index) in the call's buffer when the batch fit the capacities (else None);
        with a forward (mpn, this plan's mi), its queued logits are attached to edge_index for the model to take."""
        p = self.struct
        fit = _fits(counts_l, self.cap, p.n_cap, p.e_cap)
        if fit is None:
            return None
        N, E = fit
        o, C, F, A = self.off, self.C, self.F, self.A
        i64, f32 = flat.view(torch.int64), flat.view(torch.float32)
        x = f32.as_strided((N, C), (C, 1), o[_lib.STEP_X] // 4)
        joint_det = i64.as_strided((N, 3), (3, 1), o[_lib.STEP_JDET] // 8)
        joint_scores = f32.as_strided((N,), (1,), o[_lib.STEP_JSC] // 4)
        batch_index = i64.as_strided((N,), (1,), o[_lib.STEP_BIDX] // 8)
        joint_tags = f32.as_strided((N, F), (F, 1), o[_lib.STEP_JTAGS] // 4) if F else None
        edge_index = i64.as_strided((2, E), (E, 1), o[_lib.STEP_EIDX] // 8)
        edge_attr = f32.as_strided((E, A), (A, 1), o[_lib.STEP_EATTR] // 4)
        node_off = i64.as_strided((self.B + 4,), (1,), o[_lib.STEP_NOFF] // 8)
        _tag_fully(edge_index, node_off, counts_l, joint_det)
        if mpn is not None:   # the queued result as the model's _take_cap reads it
            res = dict(buf=f32[o[_lib.STEP_LOGITS] // 4:], a1=p.nlog_off, a2=p.clog_off, n_rec=p.n_rec,
                       key=self.mi[3])
            mpn._attach_cap(res, x, edge_attr, edge_index, joint_det, N, E)
        return (x, joint_det, joint_scores, batch_index, joint_tags), edge_attr, edge_index


def get_graph_constructor(config, **kwargs):
    """``src/graph_constructor/__init__.py:4-5``."""
    return NaiveGraphConstructor(config=config, **kwargs)


class PendingGraph:
    """construct_graph_start's handle: result() waits for the detection counts and returns the 15-tuple (once
    computed, the same tuple on every call)."""

    def __init__(self, gc, gen, dev, counts_ent):
        self._gc, self._gen, self._dev, self._counts = gc, gen, dev, counts_ent
        self._out, self._done = None, False

    def _step(self):
        try:
            next(self._gen)
        except StopIteration as stop:
            self._finish(stop.value)
        except BaseException:
            self._fail()
            raise

    def _finish(self, out):
        self._out, self._done = out, True
        NaiveGraphConstructor._host_counts_give(self._dev, self._counts)   # every count was read
        self._gen = None

    def _fail(self):
        self._done = True
        self._gen = None
        torch.cuda.current_stream(self._dev).synchronize()   # queued kernels may still store counts into it
        NaiveGraphConstructor._host_counts_give(self._dev, self._counts)

    def result(self):
        if not self._done:
            try:
                next(self._gen)
                raise RuntimeError("pemp_amd: construct_graph did not finish")   # (the generator yields once)
            except StopIteration as stop:
                self._finish(stop.value)
            except BaseException:
                if not self._done:
                    self._fail()
                raise
        if self._out is None:
            raise RuntimeError("pemp_amd: construct_graph failed")
        return self._out


class NaiveGraphConstructor:
    # Shared between instances, threads and streams (reentrant calls). Device scratch is per
    # (device, stream) (_lib.Workspace); each call takes its own mapped host count buffer from a pool and
    # returns it when the counts are read; the capacity hints are only read / raised under _mu (a stale
    # hint costs a re-build, never a wrong result).
    _ws_detect = _lib.Workspace()
    _ws_knn = _lib.Workspace()
    _mu = threading.Lock()
    _cap = 512   # detections per image kept between calls (grows on overflow)
    _graph_hint = {}   # (shape key) -> (node, edge) capacities of the fully-graph capacity build
    _host_counts_free = {}   # device index -> free (capacity, address, int32 view) mapped host buffers
    _bound_mpn = None        # capacity mode: the MPN queued right behind the capacity graph build (bind_mpn)

    @classmethod
    def bind_mpn(cls, model):
        """Capacity mode for the MPN (None unbinds): when construct_graph takes the batch-step entry (a repeated
        fully-graph batch shape with dense features, pemp_step_fully_cap), `model`'s forward is queued behind the
        capacity build before the detection counts are read back, and the output is tagged so that model(x, edge_attr,
        edge_index, node_types=joint_det[:, 2]) on it returns the queued logits instead of launching again. Any other
        call of the model -- another graph, an input or weight edited in between, a batch that overflowed the
        capacities -- runs the exact forward."""
        cls._bound_mpn = model

    @classmethod
    def _host_counts_take(cls, L, dev, B):
        """A (capacity, address, int32 view) mapped host buffer of >= B words that pemp_detect stores the
        per-image counts into, owned by the calling construct_graph until _host_counts_give."""
        with cls._mu:
            free = cls._host_counts_free.setdefault(dev.index, [])
            for i, ent in enumerate(free):
                if ent[0] >= B:
                    return free.pop(i)
        cap = max(B, 64)
        addr = L.pemp_host_alloc(4 * cap)
        if not addr:
            raise RuntimeError(f"libpemp: {L.pemp_last_error().decode()}")
        return (cap, addr, np.ctypeslib.as_array((ctypes.c_int32 * cap).from_address(addr)))

    @classmethod
    def _host_counts_give(cls, dev, ent):
        with cls._mu:
            cls._host_counts_free.setdefault(dev.index, []).append(ent)

    @staticmethod
    def _wait_counts(counts, dev):
        """Spin until the device has stored every image's count (pemp_detect's n_det_host): the host
        learns the counts while the emit and graph kernels still run. A stream sync bounds the wait."""
        spins = 0
        while counts.min() < 0:
            spins += 1
            if spins > 200000:
                torch.cuda.current_stream(dev).synchronize()
                if counts.min() < 0:
                    raise RuntimeError("pemp_detect: the device did not publish the detection counts")
        return counts.tolist()

    def __init__(self, scoremaps, tagmaps, features, joints_gt, factor_list, masks, device, config, testing,
                 heatmaps, num_joints):
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise RuntimeError("pemp_amd NaiveGraphConstructor runs on the HIP device only (no CPU fallback)")
        self.scoremaps = scoremaps.to(self.device)
        self.tagmaps = tagmaps.to(self.device) if tagmaps is not None else None
        self.features = features.to(self.device)
        self.masks = masks.to(self.device) if masks is not None else None
        self.joints_gt = joints_gt
        self.factor_list = factor_list
        self.batch_size = scoremaps.shape[0]
        self.num_joints = num_joints
        self.mask_crowds = config.MASK_CROWDS
        self.detect_threshold = config.DETECT_THRESHOLD if config.DETECT_THRESHOLD <= 1.5 else None
        self.hybrid_k = config.HYBRID_K
        self.mpn_graph_type = config.GRAPH_TYPE
        self.normalize_node_distance = config.NORM_NODE_DISTANCE
        self.edge_features_to_use = config.EDGE_FEATURES_TO_USE
        self.pool_kernel_size = config.POOL_KERNEL_SIZE
        self.testing = testing
        if getattr(config, "USE_GT", False) or getattr(config, "IMAGE_CENTRIC_SAMPLING", False):
            raise NotImplementedError("USE_GT / IMAGE_CENTRIC_SAMPLING need ground truth (training only): USE_GT replaces "
                                      "the detections (ConstructGraph.py:76-87, 114-122), IMAGE_CENTRIC_SAMPLING draws "
                                      "a random subgraph (ConstructGraph.py:182-204)")
        self._labels = None if joints_gt is None else self._label_setup(config)

    # ---- training labels (EDGE_LABEL_METHOD 4 / 6; ConstructGraph.py:123-149, 627-694, 769-942, 1096-1158) ----
    _label_cap = 1024        # candidate records per image kept between calls (grows on overflow, under _mu)

    def _label_setup(self, config):
        """Reads the label options with the reference's meaning, refuses the ones that are not built, and moves
        joints_gt [B, P, J, 3] / factor_list [B, P, J] to the device (ConstructGraph.py:16-17, 23-44)."""
        method = config.EDGE_LABEL_METHOD
        if method not in (4, 6):
            raise NotImplementedError(f"EDGE_LABEL_METHOD={method}: methods 4 and 6 are built (_construct_edge_labels_4 "
                                      "/ _6, ConstructGraph.py:627-694, 769-942); 1, 2, 3, 5 and 7 "
                                      "(ConstructGraph.py:475-625, 696-767, 944-1093) are not")
        if getattr(config, "NODE_DROPOUT", 0.0) != 0.0 and not self.testing:
            raise NotImplementedError("NODE_DROPOUT != 0 with testing=False drops a random subgraph "
                                      "(ConstructGraph.py:152-168): not built")
        if getattr(config, "WEIGHT_CLASS_LOSS", False):
            raise NotImplementedError("WEIGHT_CLASS_LOSS weights class_mask by the heatmap read at (y, type) instead of "
                                      "(y, x) (ConstructGraph.py:171-176): not built")
        gt = torch.as_tensor(self.joints_gt).to(self.device)
        if gt.dim() != 4 or gt.shape[0] != self.batch_size or gt.shape[2] != self.num_joints or gt.shape[3] != 3:
            raise ValueError(f"joints_gt {tuple(gt.shape)}: expected [{self.batch_size}, P, {self.num_joints}, 3]")
        fac = self.factor_list
        if fac is None:
            raise TypeError("joints_gt is given but factor_list is None")   # reference: factor_list[batch] on None
        if isinstance(fac, (list, tuple)):
            fac = torch.stack([torch.as_tensor(f) for f in fac])
        fac = torch.as_tensor(fac).to(self.device)
        if tuple(fac.shape) != tuple(gt.shape[:3]):
            raise ValueError(f"factor_list {tuple(fac.shape)}: expected {tuple(gt.shape[:3])}")
        f64 = fac.dtype == torch.float64   # torch promotes -distance / factor to the factors' float64, else float32
        self.joints_gt = gt
        return dict(method=method, neighbours=bool(config.USE_NEIGHBOURS), background=bool(config.WITH_BACKGROUND),
                    mr=float(config.MATCHING_RADIUS), ir=float(config.INCLUSION_RADIUS), f64=f64,
                    gt=gt.float().contiguous(), fac=(fac if f64 else fac.float()).contiguous())

    def _label_outputs(self, c, out, node_off, counts_l):
        """construct_graph's tuple with slots 3, 4, 5, 8, 9, 10 and 13 filled as ConstructGraph.py:232-249 does:
        candidate pairs on the device (pemp_label_candidates), the matching on the host (pemp_label_assign; one
        read-back of the sparse list, one upload of the per-node results), the edge pass on the device
        (pemp_label_edges)."""
        lp = self._labels
        L, st, B, H, W, dev = c.L, c.st, c.B, c.H, c.W, c.dev
        joint_det, edge_index = out[7], out[2]
        N, E = joint_det.shape[0], edge_index.shape[1]
        P, J = lp["gt"].shape[1], lp["gt"].shape[2]
        PJ = P * J
        mr, ir = lp["mr"], lp["ir"]
        if not lp["f64"]:   # a float32 similarity is compared with the radius in float32
            mr, ir = float(np.float32(mr)), float(np.float32(ir))
        thr = min(mr, ir) if lp["neighbours"] else mr
        node_off_h = np.zeros(B + 1, np.int64)
        node_off_h[1:] = np.cumsum(np.asarray(counts_l, np.int64))
        scratch = L.pemp_label_candidates_scratch_size(B, P, J)
        with NaiveGraphConstructor._mu:
            cap = NaiveGraphConstructor._label_cap
        while True:
            o_tab = _align256(4 * (2 * B + 1))
            o_rec = o_tab + _align256(4 * B * PJ)
            o_end = o_rec + _align256(16 * B * cap)
            buf = torch.empty(o_end + scratch, dtype=torch.uint8, device=dev)
            base = buf.data_ptr()
            _lib.check(L.pemp_label_candidates(lp["gt"].data_ptr(), lp["fac"].data_ptr(), int(lp["f64"]), B, P, J,
                                               _lib.ptr(joint_det), _lib.ptr(node_off), H, W, thr, cap, base + o_rec,
                                               base, base + o_tab, base + o_end, scratch, st))
            host = torch.empty(o_end, dtype=torch.uint8, pin_memory=True)
            host.copy_(buf[:o_end], non_blocking=True)
            torch.cuda.current_stream(dev).synchronize()
            hdr = host[:4 * (2 * B + 1)].view(torch.int32).numpy()
            if not hdr[2 * B]:
                break
            cap = int(hdr[:B].max())       # overflow: nothing was stored, every image's need was counted
            cap += cap // 4
            with NaiveGraphConstructor._mu:
                NaiveGraphConstructor._label_cap = cap = max(NaiveGraphConstructor._label_cap, cap)
        m6 = lp["method"] == 6
        res_h = torch.empty(max(29 * N, 1), dtype=torch.uint8, pin_memory=True)
        hp, hb = res_h.data_ptr(), host.data_ptr()
        rc = L.pemp_label_assign(B, P, J, hb, hb + o_tab, hb + o_rec, cap, node_off_h.ctypes.data, lp["method"],
                                 int(lp["neighbours"]), int(lp["background"]), mr, ir, hp + 16 * N, hp,
                                 hp + 8 * N if m6 else None, hp + 20 * N, hp + 24 * N if m6 else None, hp + 28 * N)
        _lib.check(rc)
        res = torch.empty(max(29 * N, 1), dtype=torch.uint8, device=dev)
        res.copy_(res_h, non_blocking=True)
        node_persons = res[:8 * N].view(torch.int64)
        node_classes = res[8 * N:16 * N].view(torch.int64) if m6 else None
        node_labels = res[16 * N:20 * N].view(torch.float32)
        label_mask_node = res[20 * N:24 * N].view(torch.float32)
        class_mask = res[24 * N:28 * N].view(torch.float32) if m6 else None
        ambiguous = res[28 * N:29 * N]
        edge_labels = torch.empty(E, dtype=torch.float32, device=dev)
        label_mask = torch.empty(E, dtype=torch.float32, device=dev)
        ws = torch.empty(L.pemp_label_edges_scratch_size(B), dtype=torch.uint8, device=dev)
        _lib.check(L.pemp_label_edges(_lib.ptr(edge_index), E, _lib.ptr(node_off), B, N, _lib.ptr(node_persons),
                                      _lib.ptr(ambiguous), _lib.ptr(edge_labels), _lib.ptr(label_mask), _lib.ptr(ws),
                                      ws.numel(), st))
        return (out[0], out[1], out[2], edge_labels, node_labels, node_classes, None, out[7], label_mask,
                label_mask_node, class_mask, out[11], out[12], node_persons, out[14])

    def construct_graph(self):
        """ConstructGraph.py:46-68 (inference): the 15-tuple. = construct_graph_start().result()."""
        return self.construct_graph_start().result()

    def construct_graph_start(self):
        """The launch half of construct_graph (no reference counterpart): queues the detection and, with a capacity
        hint, the graph build and the bound MPN, then returns a PendingGraph without waiting for the detection counts.
        Its result() waits for them and returns construct_graph's 15-tuple. A caller with several batches in flight (a
        server, bench.py) queues the next batch before it collects the previous one, so the host's count wait overlaps
        its other work. A pending graph must be collected (result()) before another batch is started on the same
        stream twice over (the library's scratch is per device and stream)."""
        grad = self._grad_kind()                    # (its refusals come before the library is touched)
        L = _lib.lib()
        c = _Call(self, L, _lib.stream(self.device), grad)
        counts_ent = self._host_counts_take(L, c.dev, c.B)   # one read-back of the per-image counts (pemp_detect)
        pending = PendingGraph(self, self._construct(c, counts_ent[2][:c.B]), c.dev, counts_ent)
        pending._step()                             # up to the count wait: everything is queued
        return pending

    def _construct(self, c, counts_h):
        """One of three stages, each a generator that yields once, where construct_graph_start returns. A stage prepares
        everything on the host before its first launch, so its calls are queued back to back (no host gap between them
        on the GPU), and in a loop this preparation overlaps the previous batch's GPU work."""
        c.graph(self, counts_h)
        with NaiveGraphConstructor._mu:
            # with ground truth always the exact build: the labels need the host counts before they start anyway
            hint = NaiveGraphConstructor._graph_hint.get(c.gkey) if c.fully and self._labels is None else None
            cap = NaiveGraphConstructor._cap
        if hint is None:
            return (yield from self._exact_stage(c, cap))
        if c.pmaps is None:
            return (yield from self._step_stage(c, cap, hint))
        return (yield from self._cap_stage(c, cap, hint))

    def _step_stage(self, c, cap, hint):
        """A repeated fully-graph batch shape with dense features, the batch-step entry: detection + capacity build +
        the bound MPN in one call (pemp_step_fully_cap), every output in one buffer."""
        n_cap, e_cap = hint
        mpn = NaiveGraphConstructor._bound_mpn
        bound = (mpn is not None and c.J == getattr(mpn, "num_types", None) and getattr(mpn, "_cap_ok", True)
                 and c.grad is None)     # (an x with a gradient is for a training step: nothing is queued behind it)
        mi = mpn._cap_info(c.C, c.A, n_cap, e_cap, c.dev) if bound else None
        plan = self._step_plan(c, cap, n_cap, e_cap, mi)
        flat = torch.empty(plan.struct.bytes, dtype=torch.uint8, device=c.dev)
        c.counts_h.fill(-1)
        rc = c.L.pemp_step_fully_cap(plan.ref, c.src, _lib.ptr(c.masks), c.feats.data_ptr(), _lib.ptr(c.tags),
                                     flat.data_ptr(), c.counts_h.ctypes.data, c.st)
        if rc == _lib.ERR_UNSUPPORTED and mi is not None:
            mpn._cap_ok = False     # the forward's conditions refused this model: the exact forward from now on
            mi = None
        else:
            _lib.check(rc)
        yield None                                       # (construct_graph_start returns here)
        counts_l = self._wait_counts(c.counts_h, c.dev)
        built = plan.outputs(flat, counts_l, mpn if mi is not None else None)
        if built is None:     # a capacity was exceeded: the exact build on the step's detections
            return self._exact_build(c, plan.detections(flat), cap, counts_l)
        self._update_hint(c.gkey, counts_l)
        return self._finish(c, *built, True)

    def _cap_stage(self, c, cap, hint):
        """A repeated fully-graph batch shape with ProjectedMaps features: the detection, then the capacity build queued
        ahead of the count wait (pemp_fully_graph_build_cap), then x sampled for the counts the host has read."""
        n_cap, e_cap = hint
        dets = self._det_alloc(c, cap)
        bufs = self._fully_bufs(c, n_cap, e_cap, c.B + 4)   # node offsets, then the batch's (N, E, overflow)
        self._detect_launch(c, dets, cap)
        self._fully_launch(c, c.L.pemp_fully_graph_build_cap, dets, cap, bufs)
        yield None                                       # (construct_graph_start returns here)
        counts_l = self._wait_counts(c.counts_h, c.dev)
        fit = _fits(counts_l, cap, n_cap, e_cap)
        if fit is None:
            return self._exact_build(c, dets, cap, counts_l)
        self._update_hint(c.gkey, counts_l)
        N, E = fit      # the outputs are leading (contiguous) slices of the capacity buffers
        nodes = tuple(None if t is None else t[:N] for t in bufs[:5])
        edge_index = bufs[5].view(-1)[:2 * E].view(2, E)
        _tag_fully(edge_index, bufs[7], counts_l, nodes[1])
        return self._finish(c, nodes, bufs[6][:E], edge_index, True)

    def _exact_stage(self, c, cap):
        """No capacities for this batch: the detection alone is queued, the graph is built for the exact counts."""
        dets = self._det_alloc(c, cap)
        self._detect_launch(c, dets, cap)
        yield None                                       # (construct_graph_start returns here)
        return self._exact_build(c, dets, cap, self._wait_counts(c.counts_h, c.dev))   # the one host read-back

    def _exact_build(self, c, dets, cap, counts_l):
        """The 15-tuple from the detections dets (made under capacity cap) and the counts the host has read."""
        mx = max(counts_l) if counts_l else 0
        if mx > cap:    # more detections than were kept: the emit stage again, into larger buffers
            cap = mx
            with NaiveGraphConstructor._mu:
                NaiveGraphConstructor._cap = max(NaiveGraphConstructor._cap, cap)
            dets = self._det_alloc(c, cap, dets)
            self._detect_launch(c, dets, cap, emit_only=True)
        N = sum(counts_l)
        if c.fully:     # one launch: offsets + nodes + edge_index + edge_attr (pemp_fully_graph_build)
            self._update_hint(c.gkey, counts_l)
            bufs = self._fully_bufs(c, N, _fully_edges(counts_l), c.B + 1)
            self._fully_launch(c, c.L.pemp_fully_graph_build, dets, cap, bufs)
            nodes, edge_index, edge_attr, node_off = bufs[:5], bufs[5], bufs[6], bufs[7]
            if N > 0:
                _tag_fully(edge_index, node_off, counts_l, nodes[1])
        else:
            nodes, edge_index, edge_attr, node_off = self._build_generic(c, dets, cap, counts_l, N)
        out = self._finish(c, nodes, edge_attr, edge_index, c.fully)
        if self._labels is not None:
            out = self._label_outputs(c, out, node_off, counts_l)
        return out

    @staticmethod
    def _node_bufs(c, n):
        """x, joint_det, joint_scores, batch_index and (dense tagmaps only) joint_tags for n nodes."""
        f32, i64, dev = torch.float32, torch.int64, c.dev
        return (torch.empty(n, c.C, dtype=f32, device=dev), torch.empty(n, 3, dtype=i64, device=dev),
                torch.empty(n, dtype=f32, device=dev), torch.empty(n, dtype=i64, device=dev),
                torch.empty(n, c.F, dtype=f32, device=dev) if c.tags is not None else None)

    def _fully_bufs(self, c, n, e, n_off):
        """The fused fully-graph build's outputs: the node arrays, edge_index, edge_attr, node_off [n_off]."""
        return self._node_bufs(c, n) + (torch.empty(2, e, dtype=torch.int64, device=c.dev),
                                        torch.empty(e, c.A, dtype=torch.float32, device=c.dev),
                                        torch.empty(n_off, dtype=torch.int64, device=c.dev))

    @staticmethod
    def _fully_launch(c, build, dets, cap, bufs):
        """pemp_fully_graph_build / _cap into bufs (_fully_bufs: their sizes are the exact counts / the capacities)."""
        _, det, dsc, n_det = dets
        _lib.check(build(_lib.ptr(n_det), c.B, _lib.ptr(det), _lib.ptr(dsc), cap, _lib.ptr(c.feats), c.C,
                         _lib.ptr(c.tags), c.F, c.J, c.H, c.W, bufs[0].shape[0], bufs[6].shape[0], c.norm, c.mode,
                         *[_lib.ptr(t) for t in bufs], c.st))

    def _finish(self, c, nodes, edge_attr, edge_index, late_tags):
        """The inference 15-tuple of a built graph (ConstructGraph.py:232-249, the label slots None): x sampled where
        the features are projected maps and the build did not need it, the tags in the reference's shape (projected
        ones sampled now when late_tags)."""
        x, joint_det, joint_scores, batch_index, joint_tags = nodes
        N = x.shape[0]
        if c.pmaps is not None and self.mpn_graph_type != "feature_knn":
            self._gather_projected(c, joint_det, batch_index, x)
        if c.tags is not None:   # [N, F] as the reference's tagmaps[b, type, y, x] rows: [N, *tags.shape[4:]] or [N]
            joint_tags = joint_tags.view((N,) + tuple(c.tags.shape[4:]) if c.tags.dim() > 4 else (N,))
        if c.ptags is not None and late_tags:
            joint_tags = self._gather_proj_tags(c, joint_det, batch_index, N)
        if c.grad is not None:      # the filled x, now with its backward into the features (node_gather.py)
            x = self._attach_grad(c, x, joint_det, batch_index)
        return (x, edge_attr, edge_index, None, None, None, None, joint_det, None, None, None, joint_scores,
                batch_index, None, joint_tags)

    _warned_projection = False   # the warning below was given (once per process)

    def _grad_kind(self):
        """How x is to carry a gradient into the features it is read from: None (no feature requires one, or grad mode
        is off), "dense" (a features tensor), "maps" (ProjectedMaps without a conv) or "conv" (with its feature_gather
        conv: the sparse path). Training never projects: more than one map, a size other than the map's own (the conv
        output's) or a divisor other than 1 is refused when a map requires a gradient. Where only the conv's
        parameters do, which is how every nn.Conv2d starts and how the test front-end has always been called outside
        torch.no_grad(), the projecting call runs as before, x carries no gradient, and a warning says so once."""
        f = self.features
        if not torch.is_grad_enabled():
            return None
        if not isinstance(f, ProjectedMaps):
            return "dense" if f.requires_grad else None
        if not f.requires_grad():
            return None
        h, w = f.maps[0].shape[2:]
        if f.gather is not None:
            k, pad = f.gather.kernel_size[0], f.gather.padding[0]
            h, w = h + 2 * pad - k + 1, w + 2 * pad - k + 1
        why = None
        if len(f.maps) != 1:
            why = (f"ProjectedMaps with {len(f.maps)} maps: the differentiable x reads one map (training does not sum "
                   "scales)")
        elif (h, w) != f.size or f.divisor != 1.0:
            why = (f"ProjectedMaps of size {f.size} with divisor {f.divisor} over a {(h, w)} map: the differentiable x "
                   "does not project (the size must be the map's own, or the conv output's, and the divisor 1)")
        if why is None:
            return "maps" if f.gather is None else "conv"
        if any(m.requires_grad for m in f.maps):
            raise NotImplementedError(why + "; a map requires a gradient")
        if not NaiveGraphConstructor._warned_projection:
            NaiveGraphConstructor._warned_projection = True
            import warnings
            warnings.warn("pemp_amd: " + why + "; the gather conv's parameters require a gradient but x will carry "
                          "none (freeze them, or call under torch.no_grad(), to silence this)", stacklevel=3)
        return None

    @staticmethod
    def _attach_grad(c, x, joint_det, batch_index):
        """x as the output of the autograd function of its read (the values are the build's, untouched)."""
        from . import node_gather as ng
        if c.grad == "conv":
            return ng._GatherNodesConv.apply(c.pmaps[0], c.plive[0], c.plive[1], joint_det, batch_index, c.pconv[3], x,
                                             c.pconv[0], None)
        return ng._GatherNodes.apply(c.feats if c.grad == "dense" else c.pmaps[0], joint_det, batch_index, x, None)

    def _build_generic(self, c, dets, cap, counts_l, N):
        """Offsets, node pack, then the graph type's edges and their features, a launch each (knn, feature_knn,
        score_based; fully where the fused build does not apply): (node buffers, edge_index, edge_attr, node_off)."""
        L, st, B, gtype = c.L, c.st, c.B, self.mpn_graph_type
        _, det, dsc, n_det = dets
        x, joint_det, joint_scores, batch_index, joint_tags = nodes = self._node_bufs(c, N)
        node_off_h = np.zeros(B + 1, np.int64)
        node_off_h[1:] = np.cumsum(np.asarray(counts_l, np.int64))
        # batch offsets are recomputed on the device from n_det (no host->device upload)
        offs = torch.empty(2, B + 1, dtype=torch.int64, device=c.dev)
        node_off, fully_off = offs[0], offs[1]
        _lib.check(L.pemp_graph_offsets(_lib.ptr(n_det), B, _lib.ptr(node_off),
                                        _lib.ptr(fully_off) if gtype == "fully" else None, st))
        _lib.check(L.pemp_pack_nodes(_lib.ptr(c.feats), c.C, _lib.ptr(c.tags), c.F, B, c.J, c.H, c.W, _lib.ptr(det),
                                     _lib.ptr(dsc), cap, _lib.ptr(node_off), N, _lib.ptr(x), _lib.ptr(joint_det),
                                     _lib.ptr(joint_scores), _lib.ptr(batch_index), _lib.ptr(joint_tags), st))
        if c.ptags is not None:   # before the edge features, which may read them
            nodes = nodes[:4] + (self._gather_proj_tags(c, joint_det, batch_index, N),)
        if gtype in ("knn", "feature_knn"):   # edge features written by the knn emit itself
            by_x = gtype == "feature_knn"
            if by_x and c.pmaps is not None:   # the graph ranks by x: sample it first
                self._gather_projected(c, joint_det, batch_index, x)
            edge_index, edge_attr = self._knn_edges(c, joint_det, nodes[4], joint_scores, node_off, node_off_h,
                                                    x if by_x else None)
        else:
            edge_index = self._edges(c, joint_scores, node_off, fully_off, node_off_h)
            E = edge_index.shape[1]
            edge_attr = torch.empty(E, c.A, dtype=torch.float32, device=c.dev)
            _lib.check(L.pemp_edge_features(_lib.ptr(joint_det), _lib.ptr(nodes[4]), c.F, _lib.ptr(joint_scores),
                                            _lib.ptr(edge_index), E, c.J, c.norm, c.mode, _lib.ptr(edge_attr), st))
        if gtype != "fully":   # knn, feature_knn, score_based: to_undirected's output
            _tag_sym(edge_index)
        return nodes, edge_index, edge_attr, node_off

    @staticmethod
    def _update_hint(gkey, counts_l):
        """Capacities for the next batch of this shape: 25 % headroom over this one (grow-only)."""
        N, E = sum(counts_l), _fully_edges(counts_l)
        n_hint = (N + N // 4 + 16, E + E // 4 + 256)
        with NaiveGraphConstructor._mu:
            old = NaiveGraphConstructor._graph_hint.get(gkey)
            NaiveGraphConstructor._graph_hint[gkey] = n_hint if old is None else (
                max(old[0], n_hint[0]), max(old[1], n_hint[1]))

    def _det_alloc(self, c, cap, old=None):
        """(workspace, det_xyt [B, cap, 3], det_scores [B, cap], n_det [B]); old: its workspace and n_det kept."""
        ws = old[0] if old else self._ws_detect.get(c.L.pemp_detect_workspace_size(c.B, c.J, c.H, c.W, c.topk), c.dev)
        return (ws, torch.empty(c.B, cap, 3, dtype=torch.int64, device=c.dev),
                torch.empty(c.B, cap, dtype=torch.float32, device=c.dev),
                old[3] if old else torch.empty(c.B, dtype=torch.int32, device=c.dev))

    @staticmethod
    def _detect_launch(c, dets, cap, emit_only=False):
        """pemp_detect; emit_only: its emit stage again (the counts are on the host already)."""
        ws, det, dsc, n_det = dets
        if not emit_only:
            c.counts_h.fill(-1)
        _lib.check(c.detect(c.src, _lib.ptr(c.masks), c.B, c.J, c.H, c.W, c.pool, c.thr, int(c.use_thr), c.topk,
                            2 if emit_only else 3, _lib.ptr(ws), ws.numel(), _lib.ptr(det), _lib.ptr(dsc),
                            _lib.ptr(n_det), cap, None if emit_only else c.counts_h.ctypes.data, c.st))

    _plans = {}   # (device, stream, batch shape, capacities, forward) -> _StepPlan (under _mu)

    def _step_plan(self, c, cap, n_cap, e_cap, mi):
        """The pemp_step_fully_cap plan of this call's arguments (cached per device, stream and shape)."""
        fkey = None if mi is None else (id(mi[1]), mi[2].data_ptr(), mi[2].numel(), ctypes.addressof(mi[0]))
        key = (c.gkey, c.st, c.pool, c.use_thr, c.topk, c.thr, cap, c.tags is not None, c.mode, c.norm, n_cap, e_cap,
               fkey, c.proj)   # (gkey: the shape B, J, H, W, C, F, A and the device)
        with NaiveGraphConstructor._mu:
            plan = NaiveGraphConstructor._plans.get(key)
        if plan is None:
            ws = self._ws_detect.get(c.L.pemp_detect_workspace_size(c.B, c.J, c.H, c.W, c.topk), c.dev)
            plan = _StepPlan(c, cap, ws, n_cap, e_cap, mi)
            with NaiveGraphConstructor._mu:
                if len(NaiveGraphConstructor._plans) >= 64:
                    NaiveGraphConstructor._plans.clear()
                NaiveGraphConstructor._plans[key] = plan
        return plan

    @staticmethod
    def _gather_proj_tags(c, joint_det, batch_index, N):
        """joint_tags [N, F] from the projected tag channels (pemp_gather_projected_tags); the reference's
        tagmaps there are [B, J, H, W, F] (torch.cat(tags_list, dim=4)), so F = 1 stays [N, 1]."""
        pt = c.ptags
        jt = torch.empty(N, pt.tag_dims, dtype=torch.float32, device=c.dev)
        maps = pt.c_struct()
        _lib.check(c.L.pemp_gather_projected_tags(ctypes.addressof(maps), pt.tag_scale, c.J, c.H, c.W,
                                                  _lib.ptr(joint_det), _lib.ptr(batch_index), N, _lib.ptr(jt), c.st))
        return jt

    @staticmethod
    def _gather_projected(c, joint_det, batch_index, x):
        """x [N, C] sampled at the detections from the projected maps (pemp_gather_projected), through the
        feature_gather conv at the taps where the maps carry one (pemp_gather_projected_conv)."""
        L, pmaps, vp = c.L, c.pmaps, ctypes.c_void_p
        S = len(pmaps)
        ptrs = ctypes.cast((vp * S)(*[m.data_ptr() for m in pmaps]), vp)
        hs = ctypes.cast((ctypes.c_int32 * S)(*[m.shape[2] for m in pmaps]), vp)
        ws = ctypes.cast((ctypes.c_int32 * S)(*[m.shape[3] for m in pmaps]), vp)
        tail = (c.H, c.W, c.divisor, _lib.ptr(joint_det), _lib.ptr(batch_index), x.shape[0], _lib.ptr(x), c.st)
        if c.pconv is not None:
            wt, b, k, pad = c.pconv
            _lib.check(L.pemp_gather_projected_conv(ptrs, hs, ws, S, pmaps[0].shape[1], _lib.ptr(wt), _lib.ptr(b),
                                                    x.shape[1], k, pad, *tail))
        else:
            _lib.check(L.pemp_gather_projected(ptrs, hs, ws, S, x.shape[1], *tail))

    def _edges(self, c, joint_scores, node_off, fully_off, node_off_h):
        L, st, B, dev = c.L, c.st, c.B, c.dev
        counts = np.diff(node_off_h)
        if self.mpn_graph_type == "fully":
            E = int((counts * np.maximum(counts - 1, 0)).sum())
            edge_index = torch.empty(2, E, dtype=torch.int64, device=dev)
            _lib.check(L.pemp_fully_graph(_lib.ptr(node_off), _lib.ptr(fully_off), B, E, _lib.ptr(edge_index), st))
            return edge_index
        if self.mpn_graph_type != "score_based":
            raise NotImplementedError(f"GRAPH_TYPE={self.mpn_graph_type}")
        k = _SCORE_BASED_K
        if counts.size and counts.min() < k:   # the reference's joint_scores.topk(k) raises
            raise RuntimeError(f"score_based graph: selected index k={k} out of range for "
                               f"{int(counts.min())} detections")
        E = int((k * (2 * counts - k - 1)).sum())
        edge_index = torch.empty(2, E, dtype=torch.int64, device=dev)
        nh = np.ascontiguousarray(node_off_h)
        nh_p = nh.ctypes.data_as(ctypes.c_void_p)
        ws = self._ws_knn.get(L.pemp_score_graph_workspace_size(nh_p, B, k), dev)
        _lib.check(L.pemp_score_graph(_lib.ptr(joint_scores), _lib.ptr(node_off), nh_p, B, k, E, _lib.ptr(ws),
                                      ws.numel(), _lib.ptr(edge_index), st))
        return edge_index

    _KNN_K = 50   # ConstructGraph.py:365 (knn_graph(k=50))

    def _knn_edges(self, c, joint_det, joint_tags, joint_scores, node_off, node_off_h, x=None):
        """knn_mpn_graph (ConstructGraph.py:363-368) + the edge features in one queued call
        (pemp_knn_graph_build): buffers sized by the closed-form edge bound, the total back through
        mapped memory while the emit still runs; edge_index / edge_attr are the leading contiguous
        [2, E] / [E, A] blocks of those buffers. With x: feature_knn_mpn_graph (ConstructGraph.py:370-374),
        the same graph over the node features x [N, C] (pemp_feature_knn_graph_build)."""
        L, B, A, dev, k = c.L, c.B, c.A, c.dev, self._KNN_K
        nh = np.ascontiguousarray(node_off_h)
        nh_p = nh.ctypes.data_as(ctypes.c_void_p)
        n = np.diff(nh)
        size = (L.pemp_feature_knn_workspace_size if x is not None else L.pemp_knn_workspace_size)(nh_p, B)
        # batches the MPN's knn prepare takes: a workspace of the call's own, whose bit rows go with edge_index
        rows = None
        if 1 <= B <= 64 and 0 < nh[B] <= 4096 and int(n.max()) <= 512:
            rows = (ctypes.c_size_t * 3)()
            _lib.check(L.pemp_knn_rows_layout(nh_p, B, int(x is not None), rows))
            ws = torch.empty(max(int(size), 256), dtype=torch.uint8, device=dev)
        else:
            ws = self._ws_knn.get(size, dev)
        e_cap = int(np.minimum(n * np.maximum(n - 1, 0), 2 * k * n).sum())
        buf = torch.empty(2 * max(e_cap, 1), dtype=torch.int64, device=dev)
        ea = torch.empty(max(e_cap, 1) * A, dtype=torch.float32, device=dev)
        ent = self._host_counts_take(L, dev, 1)
        try:
            word = ent[2][:1]
            word.fill(-1)
            args = (_lib.ptr(joint_det), _lib.ptr(node_off), nh_p, B, k, _lib.ptr(ws), ws.numel(), e_cap,
                    _lib.ptr(buf), ent[1], _lib.ptr(joint_tags), c.F, _lib.ptr(joint_scores), c.J, c.norm, c.mode,
                    _lib.ptr(ea), c.st)
            if x is not None:
                _lib.check(L.pemp_feature_knn_graph_build(_lib.ptr(x), x.shape[1], *args))
            else:
                _lib.check(L.pemp_knn_graph_build(*args))
            E = self._wait_counts(word, dev)[0]
        except BaseException:
            torch.cuda.current_stream(dev).synchronize()
            self._host_counts_give(dev, ent)
            raise
        self._host_counts_give(dev, ent)
        if E > e_cap:
            raise RuntimeError(f"pemp_knn_graph_build: {E} edges > bound {e_cap}")
        edge_index = buf[:2 * E].view(2, E)
        if rows is not None:
            _tag_knn(edge_index, ws, tuple(rows), node_off, nh)
        return edge_index, ea[:E * A].view(E, A)
