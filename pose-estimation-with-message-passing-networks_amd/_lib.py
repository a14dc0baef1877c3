"""ctypes binding of ``csrc/libpemp.so`` (C-ABI declared in ``include/pemp.h``).

The product path has no CPU fallback: ``lib()`` raises if the library is missing, was built for
another ABI, or no gfx950 device is present.
"""
import ctypes
import threading
import os

LIB_PATH = os.environ.get("PEMP_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "csrc",
                                                     "libpemp.so")
ABI_VERSION = 24

ERR_INVALID_ARG, ERR_HIP, ERR_WORKSPACE, ERR_UNSUPPORTED = -1, -2, -3, -4
MPN_PREPARED, MPN_TWO_LAUNCH_FIRST, MPN_FUSED_FIRST_PROFILED = 1, 4, 8   # pemp.h PEMP_MPN_*
MPN_SEPARATE_PRELUDE = 16

c_i32, c_i64, c_f32, c_sz, c_p = ctypes.c_int32, ctypes.c_int64, ctypes.c_float, ctypes.c_size_t, ctypes.c_void_p


class PempLayer(ctypes.Structure):
    _fields_ = [("w", c_p), ("b", c_p), ("in_dim", c_i32), ("out_dim", c_i32), ("relu", c_i32), ("pad_", c_i32)]


class PempMlp(ctypes.Structure):
    _fields_ = [("layer", PempLayer * 4), ("n_layers", c_i32), ("pad_", c_i32)]


class PempMpnWeights(ctypes.Structure):
    _fields_ = [("node_emb", PempMlp), ("edge_emb", PempMlp),
                ("pre_w", c_p), ("pre_b", c_p), ("q0_w", c_p), ("q0_b", c_p), ("e1_w", c_p),
                ("e2_w", c_p), ("e2_b", c_p), ("msg_w", c_p), ("attn_w", c_p), ("upd_w", c_p), ("upd_b", c_p),
                ("edge_head", PempMlp), ("node_head", PempMlp), ("class_head", PempMlp),
                ("attn_b", c_f32), ("pad_", c_i32),
                ("e1_bf", c_p), ("e2_bf", c_p), ("msg_bf", c_p), ("head_bf", c_p), ("emb_bf", c_p),
                ("upd_bf", c_p), ("pre_bf", c_p), ("node_img", c_p), ("attn_bv", c_p),
                ("upd_mlp", PempMlp),
                ("ept_l1_w", c_p), ("ept_l1_b", c_p), ("ept_l2_w", c_p), ("ept_l2_b", c_p), ("ept_o1_w", c_p),
                ("ept_o2_w", c_p), ("edge_img", c_p), ("emb_comp_bf", c_p), ("emb_comp_b", c_p)]


class PempProjMaps(ctypes.Structure):
    _fields_ = [("num_scales", c_i32), ("channels", c_i32), ("maps", c_p * 4), ("flip_maps", c_p * 4),
                ("h", c_i32 * 4), ("w", c_i32 * 4), ("flip_index", c_p), ("divisor", c_f32)]


class PempMpnDesc(ctypes.Structure):
    _fields_ = [("num_types", c_i32), ("num_joints", c_i32), ("steps", c_i32), ("aux_loss_steps", c_i32),
                ("aggr", c_i32), ("hidden", c_i32), ("edge_attr_dim", c_i32), ("node_in_dim", c_i32),
                ("precision", c_i32), ("types_stride", c_i32), ("flags", c_i32)]


STEP_DET, STEP_DSC, STEP_NDET, STEP_X, STEP_JDET, STEP_JSC, STEP_BIDX, STEP_JTAGS, STEP_EIDX, STEP_EATTR, STEP_NOFF, \
    STEP_LOGITS, STEP_NOUT = range(13)


class PempStepPlan(ctypes.Structure):
    _fields_ = [("B", c_i32), ("J", c_i32), ("H", c_i32), ("W", c_i32), ("pool_kernel", c_i32), ("use_threshold", c_i32),
                ("topk", c_i32), ("det_cap", c_i32), ("projected", c_i32), ("threshold", c_f32), ("det_workspace", c_p),
                ("det_workspace_bytes", c_sz), ("C", c_i32), ("F", c_i32), ("A", c_i32), ("mode", c_i32),
                ("norm_factor", c_f32), ("n_cap", c_i64), ("e_cap", c_i64), ("desc", ctypes.POINTER(PempMpnDesc)),
                ("weights", ctypes.POINTER(PempMpnWeights)), ("mpn_workspace", c_p), ("mpn_workspace_bytes", c_sz),
                ("n_rec", c_i32), ("elog_n", c_i64), ("nlog_off", c_i64), ("clog_off", c_i64),
                ("off", c_sz * STEP_NOUT), ("bytes", c_sz)]


LOSS_MAXKE, LOSS_MAXKN, LOSS_MAXJ, LOSS_OUT, LOSS_CHUNK = 8, 9, 32, 32, 2048   # pemp.h PEMP_LOSS_*
LOSS_FOCAL, LOSS_BCE = 0, 1
LOSS_TERM_NODE, LOSS_TERM_EDGE, LOSS_TERM_CLASS = 1, 2, 4


class PempLossRec(ctypes.Structure):
    _fields_ = [("N", c_i64), ("E", c_i64), ("J", c_i32), ("K_e", c_i32), ("K_n", c_i32), ("edge_kind", c_i32),
                ("node_kind", c_i32), ("include_bordering", c_i32), ("terms", c_i32), ("pad_", c_i32),
                ("alpha", c_f32), ("gamma", c_f32), ("edge_pos_weight", c_f32), ("node_pos_weight", c_f32),
                ("node_threshold", c_f32), ("node_weight", c_f32), ("edge_weight", c_f32), ("class_weight", c_f32),
                ("pe", c_p * LOSS_MAXKE), ("pn", c_p * LOSS_MAXKN), ("pc", c_p * LOSS_MAXKN), ("edge_index", c_p),
                ("edge_labels", c_p), ("label_mask", c_p), ("node_labels", c_p), ("label_mask_node", c_p),
                ("node_classes", c_p), ("edge_mask", c_p * LOSS_MAXKE)]


KP_MAXS, KP_MAXP, KP_MAXJ, KP_CHUNK, KP_MAXBLOCKS, KP_OUT = 4, 32, 32, 4096, 2048, 16   # pemp.h PEMP_KP_*
KP_AE_EXP, KP_AE_MAX = 0, 1


class PempKpStage(ctypes.Structure):
    _fields_ = [("pred", c_p), ("gt", c_p), ("mask", c_p), ("tag", c_p), ("C", c_i32), ("H", c_i32), ("W", c_i32),
                ("with_heatmap", c_i32), ("with_ae", c_i32), ("heatmap_factor", c_f32), ("push_factor", c_f32),
                ("pull_factor", c_f32)]


class PempKpLossRec(ctypes.Structure):
    _fields_ = [("S", c_i32), ("B", c_i32), ("J", c_i32), ("P", c_i32), ("ae_kind", c_i32), ("pad_", c_i32),
                ("stage", PempKpStage * KP_MAXS), ("blk0", c_i32 * (KP_MAXS + 2))]


# name -> (restype, argtypes); every symbol of include/pemp.h
SIGNATURES = {
    "pemp_abi_version": (c_i32, []),
    "pemp_last_error": (ctypes.c_char_p, []),
    "pemp_device_check": (c_i32, []),
    "pemp_detect_workspace_size": (c_sz, [c_i32, c_i32, c_i32, c_i32, c_i32]),
    "pemp_detect": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_i32, c_i32, c_i32, c_p, c_sz,
                            c_p, c_p, c_p, c_i32, c_p, c_p]),
    "pemp_host_alloc": (c_p, [c_sz]),
    "pemp_host_free": (c_i32, [c_p]),
    "pemp_pack_nodes": (c_i32, [c_p, c_i32, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_i32, c_p, c_i64,
                                c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_graph_offsets": (c_i32, [c_p, c_i32, c_p, c_p, c_p]),
    "pemp_fully_graph_build": (c_i32, [c_p, c_i32, c_p, c_p, c_i32, c_p, c_i32, c_p, c_i32, c_i32, c_i32, c_i32,
                                       c_i64, c_i64, c_f32, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_fully_graph_build_cap": (c_i32, [c_p, c_i32, c_p, c_p, c_i32, c_p, c_i32, c_p, c_i32, c_i32, c_i32, c_i32,
                                           c_i64, c_i64, c_f32, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_fully_graph": (c_i32, [c_p, c_p, c_i32, c_i64, c_p, c_p]),
    "pemp_knn_workspace_size": (c_sz, [c_p, c_i32]),
    "pemp_knn_graph_build": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_p, c_sz, c_i64, c_p, c_p, c_p, c_i32, c_p,
                                     c_i32, c_f32, c_i32, c_p, c_p]),
    "pemp_feature_knn_workspace_size": (c_sz, [c_p, c_i32]),
    "pemp_knn_rows_layout": (c_i32, [c_p, c_i32, c_i32, c_p]),
    "pemp_feature_knn_graph_build": (c_i32, [c_p, c_i32, c_p, c_p, c_p, c_i32, c_i32, c_p, c_sz, c_i64, c_p, c_p,
                                             c_p, c_i32, c_p, c_i32, c_f32, c_i32, c_p, c_p]),
    "pemp_score_graph_workspace_size": (c_sz, [c_p, c_i32, c_i32]),
    "pemp_score_graph": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i64, c_p, c_sz, c_p, c_p]),
    "pemp_gather_projected": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_f32, c_p, c_p, c_i64, c_p, c_p]),
    "pemp_gather_projected_conv": (c_i32, [c_p, c_p, c_p, c_i32, c_i32, c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32,
                                           c_f32, c_p, c_p, c_i64, c_p, c_p]),
    "pemp_detect_projected": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_f32, c_i32, c_i32, c_i32, c_p,
                                      c_sz, c_p, c_p, c_p, c_i32, c_p, c_p]),
    "pemp_detect_projected_path": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p]),
    "pemp_gather_projected_tags": (c_i32, [c_p, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_i64, c_p, c_p]),
    "pemp_project_maps": (c_i32, [c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_p]),
    "pemp_stage_merge": (c_i32, [c_p, c_i32, c_i32, c_i32, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_p]),
    "pemp_edge_features": (c_i32, [c_p, c_p, c_i32, c_p, c_p, c_i64, c_i32, c_f32, c_i32, c_p, c_p]),
    "pemp_mpn_workspace_size": (c_sz, [ctypes.POINTER(PempMpnDesc), c_i64, c_i64]),
    "pemp_mpn_fused_first_lds_bytes": (c_sz, []),
    "pemp_mpn_prelude_grids": (c_i32, [c_i64, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_p]),
    "pemp_mpn_forward": (c_i32, [ctypes.POINTER(PempMpnDesc), ctypes.POINTER(PempMpnWeights), c_p, c_p, c_p, c_p,
                                 c_i64, c_i64, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "pemp_mpn_forward_fully": (c_i32, [ctypes.POINTER(PempMpnDesc), ctypes.POINTER(PempMpnWeights), c_p, c_p, c_p,
                                       c_p, c_i64, c_i64, c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "pemp_mpn_forward_fully_cap": (c_i32, [ctypes.POINTER(PempMpnDesc), ctypes.POINTER(PempMpnWeights), c_p, c_p,
                                           c_p, c_i64, c_i64, c_p, c_i32, c_p, c_i32, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "pemp_mpn_graph_stats": (c_i32, [c_p]),
    "pemp_edge_cus_policy": (c_i32, [c_i32, c_i64, c_i32]),
    "pemp_abi_struct_size": (c_sz, [c_i32]),
    "pemp_mpn_forward_sym": (c_i32, [ctypes.POINTER(PempMpnDesc), ctypes.POINTER(PempMpnWeights), c_p, c_p, c_p,
                                     c_p, c_i64, c_i64, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "pemp_mpn_forward_knn": (c_i32, [ctypes.POINTER(PempMpnDesc), ctypes.POINTER(PempMpnWeights), c_p, c_p, c_p,
                                     c_p, c_i64, c_i64, c_p, c_p, c_p, c_p, c_p, c_i32, c_p, c_p, c_p, c_p, c_sz,
                                     c_p]),
    "pemp_mpn_prepare": (c_i32, [ctypes.POINTER(PempMpnDesc), c_p, c_p, c_i64, c_i64, c_p, c_sz, c_p]),
    "pemp_mpn_order_layout": (c_i32, [ctypes.POINTER(PempMpnDesc), c_i64, c_i64, c_p]),
    "pemp_mpn_edge_image_floats": (c_sz, [ctypes.POINTER(PempMpnDesc), ctypes.POINTER(PempMpnWeights)]),
    "pemp_mpn_edge_image": (c_i32, [ctypes.POINTER(PempMpnDesc), ctypes.POINTER(PempMpnWeights), c_p, c_sz, c_p]),
    "pemp_mpn_node_image_floats": (c_sz, [ctypes.POINTER(PempMpnWeights)]),
    "pemp_mpn_node_image": (c_i32, [ctypes.POINTER(PempMpnWeights), c_p, c_sz, c_p]),
    "pemp_mpn_status": (c_i32, [ctypes.POINTER(PempMpnDesc), c_i64, c_i64, c_p, c_p]),
    "pemp_pose_edge_weights": (c_i32, [c_p, c_i64, c_p, c_p, c_f32, c_i32, c_p, c_i32, c_i64, c_i32, c_p, c_p, c_p,
                                       c_p]),
    "pemp_pose_cluster": (c_i32, [c_i32, c_p, c_p, c_i64, c_p, c_p, c_i32, c_i32, c_p, c_p]),
    "pemp_pose_persons": (c_i32, [c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_i32, c_i32, c_i64, c_p, c_p, c_p]),
    "pemp_pose_greedy": (c_i32, [c_i32, c_p, c_p, c_i64, c_p, c_p, c_p, c_p, c_i32, c_p, c_i64, c_p, c_p]),
    "pemp_pose_fill_mean": (c_i32, [c_p, c_i32, c_i32]),
    "pemp_pose_refine_workspace_size": (c_sz, [c_i32, c_i32, c_i32, c_i32, c_i32]),
    "pemp_pose_refine": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, c_i32, c_p, c_sz, c_p]),
    "pemp_pose_adjust": (c_i32, [c_p, c_i32, c_i32, c_i32, c_p, c_i32, c_p]),
    "pemp_pack_to_host": (c_i32, [c_i32, c_p, c_p, c_p, c_sz, c_p, c_p, c_p]),
    "pemp_pose_finish_plan": (c_i32, [c_i32, c_p, c_p, c_p, c_p, c_i32, c_p]),
    "pemp_pose_finish_batch": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_i32, c_p, c_i32, c_p, c_p, c_i32,
                                       c_i32, c_p, c_i32, c_p, c_sz, c_p]),
    "pemp_step_layout": (c_sz, [ctypes.POINTER(PempStepPlan)]),
    "pemp_step_fully_cap": (c_i32, [ctypes.POINTER(PempStepPlan), c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_prof_enable": (c_i32, [ctypes.c_char_p]),
    "pemp_prof_report": (c_i32, [ctypes.c_char_p, c_sz]),
    "pemp_label_candidates_scratch_size": (c_sz, [c_i32, c_i32, c_i32]),
    "pemp_label_candidates": (c_i32, [c_p, c_p, c_i32, c_i32, c_i32, c_i32, c_p, c_p, c_i32, c_i32, ctypes.c_double,
                                      c_i64, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "pemp_label_assign": (c_i32, [c_i32, c_i32, c_i32, c_p, c_p, c_p, c_i64, c_p, c_i32, c_i32, c_i32,
                                  ctypes.c_double, ctypes.c_double, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_label_edges_scratch_size": (c_sz, [c_i32]),
    "pemp_label_edges": (c_i32, [c_p, c_i64, c_p, c_i32, c_i64, c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
    "pemp_seg_aggr_fwd": (c_i32, [c_i32, c_i32, c_i64, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_seg_aggr_bwd": (c_i32, [c_i32, c_i32, c_i64, c_i64, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_seg_rows_sum": (c_i32, [c_i64, c_i64, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_edge_mlp_workspace_size": (c_sz, [c_i64, c_i32]),
    "pemp_edge_mlp_fwd": (c_i32, [c_i64, c_i64, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_edge_mlp_bwd": (c_i32, [c_i64, c_i64, c_i32, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_p, c_sz,
                                  c_p]),
    "pemp_loss_workspace_size": (c_sz, [c_i64, c_i64, c_i32, c_i32]),
    "pemp_loss_fwd": (c_i32, [ctypes.POINTER(PempLossRec), c_p, c_sz, c_p, c_p]),
    "pemp_loss_bwd": (c_i32, [ctypes.POINTER(PempLossRec), c_p, c_p, c_p, c_p, c_p, c_p]),
    "pemp_kp_loss_workspace_size": (c_sz, [ctypes.POINTER(PempKpLossRec)]),
    "pemp_kp_loss_fwd": (c_i32, [ctypes.POINTER(PempKpLossRec), c_p, c_sz, c_p, c_p]),
    "pemp_kp_loss_bwd": (c_i32, [ctypes.POINTER(PempKpLossRec), c_p, c_p, c_p, c_p]),
    "pemp_node_grad_pixels": (c_i32, [c_p, c_i64, c_i32, c_p, c_p, c_i32, c_i32, c_i32, c_p, c_p]),
    "pemp_node_conv_workspace_size": (c_sz, [c_i64, c_i32, c_i32, c_i32]),
    "pemp_node_conv_bwd": (c_i32, [c_p, c_p, c_p, c_p, c_p, c_i64, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_i32, c_p,
                                   c_p, c_p, c_p, c_p, c_p, c_sz, c_p]),
}
LABEL_OVERFLOW = 1                  # pemp.h PEMP_LABEL_OVERFLOW
LABEL_CAND_DTYPE = [("g", "<i4"), ("n", "<u4"), ("sim", "<f8")]   # pemp.h pemp_label_cand

_LIB = None


def load_cdll(path: str = LIB_PATH):
    """Load and declare the library WITHOUT touching the GPU (used by the CPU symbol test)."""
    if not os.path.exists(path):
        raise RuntimeError(f"pemp_amd: {path} is missing - build it with `python -c 'import __graft_entry__ as g; g.build()'`")
    L = ctypes.CDLL(path)
    for name, (res, args) in SIGNATURES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = res, args
    if L.pemp_abi_version() != ABI_VERSION:
        raise RuntimeError(f"pemp_amd: libpemp ABI {L.pemp_abi_version()} != {ABI_VERSION}")
    return L


def lib():
    """The HIP library, ready for compute. Raises if no gfx950 HIP device is usable."""
    global _LIB
    if _LIB is None:
        import torch  # torch's HIP runtime must be loaded first: libpemp binds to it by SONAME
        if not torch.cuda.is_available():
            raise RuntimeError("pemp_amd: no HIP device available - the HIP path has no CPU fallback")
        L = load_cdll()
        torch.cuda.init()
        check(L.pemp_device_check(), L)
        _LIB = L
    return _LIB


def check(rc: int, L=None):
    if rc == 0:
        return
    msg = (L or _LIB).pemp_last_error().decode(errors="replace")
    if rc == ERR_INVALID_ARG:
        raise ValueError(msg)
    if rc == ERR_UNSUPPORTED:
        raise NotImplementedError(msg)
    raise RuntimeError(f"libpemp error {rc}: {msg}")


def ptr(t):
    # ctypes converts a Python int for a c_void_p argument; None is NULL
    return None if t is None else t.data_ptr()


def stream(device=None):
    """Raw hipStream_t of the current stream of `device` (a torch.device, an index or None for the
    current device) -- the launch stream of every libpemp call."""
    import torch
    if device is None:
        idx = torch.cuda.current_device()
    else:
        idx = device if isinstance(device, int) else device.index
        if idx is None:
            idx = torch.cuda.current_device()
    return torch._C._cuda_getCurrentRawStream(idx)


class Workspace:
    """Grow-only device scratch owned by the caller side (one per use site), one buffer per (device,
    stream): calls queued on different streams never share scratch, calls on one stream are ordered by
    it (a buffer replaced on a stream goes back to torch's stream-aware allocator). Thread-safe."""

    def __init__(self):
        self._bufs = {}
        self._mu = threading.Lock()

    def get(self, nbytes: int, device):
        import torch
        nbytes = max(int(nbytes), 256)
        idx = device.index if device.index is not None else torch.cuda.current_device()
        key = (idx, stream(idx))
        with self._mu:
            buf = self._bufs.get(key)
            if buf is None or buf.numel() < nbytes:
                with torch.cuda.device(idx):
                    buf = torch.empty(nbytes + (nbytes >> 3), dtype=torch.uint8, device=device)
                self._bufs[key] = buf
            return buf


def prof_enable(filt):
    lib().pemp_prof_enable(None if filt is None else filt.encode())


def prof_report():
    """{label: (launches, total_ms)} for the kernels recorded since the last report (syncs)."""
    L = lib()
    buf = ctypes.create_string_buffer(1 << 16)
    L.pemp_prof_report(buf, len(buf))
    out = {}
    for line in buf.value.decode().splitlines():
        name, cnt, ms = line.split()
        out[name] = (int(cnt), float(ms))
    return out
