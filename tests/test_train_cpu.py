"""CPU-side checks of the training mode: the three segment entry points of libpemp.so (exported, ABI 24, argument
errors reported before any HIP call), the segment plan on CPU tensors, and the plain-torch restatement
(tests/train_oracle.py) in fp64 against the reference's own training step (tests/golden/train_*.npz)."""
import numpy as np
import pytest
import torch

from pemp_amd import _lib
from tests import golden_util as gu, train_oracle as to

ATTN, SUM, MEAN, MAX = 0, 1, 2, 3


def test_exports_and_abi():
    L = _lib.load_cdll()
    for name in ("pemp_seg_aggr_fwd", "pemp_seg_aggr_bwd", "pemp_seg_rows_sum"):
        assert hasattr(L, name) and name in _lib.SIGNATURES
    assert L.pemp_abi_version() == 24 == _lib.ABI_VERSION


def test_argument_errors_need_no_gpu():
    L = _lib.load_cdll()
    p = 0x1000   # never dereferenced: every call below fails its argument checks first
    fwd, bwd, rows = L.pemp_seg_aggr_fwd, L.pemp_seg_aggr_bwd, L.pemp_seg_rows_sum
    bad = [
        ("kind", fwd(7, 1, 4, 8, p, p, p, p, p, p, p, None)),
        ("kind", fwd(-1, 1, 4, 8, p, p, p, p, p, p, p, None)),
        ("kind", bwd(4, 1, 4, 8, p, p, p, p, p, p, p, p, p, None)),
        ("T", fwd(SUM, 0, 4, 8, p, None, p, p, p, None, None, None)),
        ("T", bwd(SUM, -3, 4, 8, p, p, p, p, p, p, p, p, p, None)),
        ("size", fwd(SUM, 1, -1, 8, p, None, p, p, p, None, None, None)),
        ("size", fwd(SUM, 1, 4, -8, p, None, p, p, p, None, None, None)),
        ("size", bwd(SUM, 1, 4, -8, p, p, p, p, p, p, p, p, p, None)),
        ("size", fwd(SUM, 17, 2 ** 62, 8, p, None, p, p, p, None, None, None)),   # N T past int64: no wrap-around
        ("size", rows(-4, 8, 64, p, p, p, p, p, p, p, None)),
        ("size", rows(4, -8, 64, p, p, p, p, p, p, p, None)),
        ("W", rows(4, 8, 32, p, p, p, p, p, p, p, None)),
        ("W", rows(4, 8, 192, p, p, p, p, p, p, p, None)),
        ("scores", fwd(ATTN, 17, 4, 8, p, None, p, p, p, p, None, None)),
        ("NULL", fwd(SUM, 1, 4, 8, None, None, p, p, p, None, None, None)),     # msgs
        ("NULL", fwd(SUM, 1, 4, 8, p, None, None, p, p, None, None, None)),     # perm_dst
        ("NULL", fwd(SUM, 1, 4, 8, p, None, p, None, p, None, None, None)),     # seg_off
        ("NULL", fwd(SUM, 1, 4, 8, p, None, p, p, None, None, None, None)),     # out
        ("NULL", bwd(SUM, 1, 4, 8, None, p, p, p, p, p, p, p, p, None)),        # grad_out
        ("NULL", bwd(SUM, 1, 4, 8, p, p, p, p, p, p, p, None, p, None)),        # grad_msgs
        ("NULL", bwd(ATTN, 1, 4, 8, p, p, None, p, p, p, p, p, p, None)),       # alpha (ATTN)
        ("NULL", bwd(MAX, 1, 4, 8, p, p, p, p, None, p, p, p, p, None)),        # arg (MAX)
        ("NULL", rows(4, 8, 64, None, p, p, p, p, p, p, None)),                 # ga
        ("NULL", rows(4, 8, 64, p, p, p, p, None, p, p, None)),                 # gb without perm_b
        ("NULL", rows(4, 8, 128, p, p, p, None, None, None, None, None)),       # out
    ]
    for what, rc in bad:
        assert rc == _lib.ERR_INVALID_ARG, what
    assert rows(4, 8, 32, p, p, p, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert b"W = 32" in L.pemp_last_error()
    assert fwd(9, 1, 4, 8, p, p, p, p, p, p, p, None) == _lib.ERR_INVALID_ARG
    assert b"kind" in L.pemp_last_error()


def test_empty_sizes_return_ok_without_a_gpu():
    L = _lib.load_cdll()
    p = 0x1000
    for kind in (ATTN, SUM, MEAN, MAX):
        assert L.pemp_seg_aggr_fwd(kind, 17, 0, 0, None, None, None, None, None, None, None, None) == 0
        assert L.pemp_seg_aggr_fwd(kind, 17, 0, 5, p, p, p, p, p, p, p, None) == 0
        assert L.pemp_seg_aggr_bwd(kind, 17, 0, 5, p, p, p, p, p, p, p, p, p, None) == 0
        assert L.pemp_seg_aggr_bwd(kind, 17, 6, 0, None, None, None, None, None, None, None, None, None, None) == 0
    for W in (64, 128):
        assert L.pemp_seg_rows_sum(0, 0, W, None, None, None, None, None, None, None, None) == 0
        assert L.pemp_seg_rows_sum(0, 9, W, p, p, p, p, p, p, p, None) == 0


# ---- the segment plan ----------------------------------------------------------------------------------------
def _graph(N, E, ntypes, seed, isolated=None, unused_type=None):
    g = torch.Generator().manual_seed(seed)
    types = torch.randint(0, ntypes, (N,), generator=g)
    if unused_type is not None:
        types[types == unused_type] = (unused_type + 1) % ntypes
    src = torch.randint(0, N, (E,), generator=g)
    dst = torch.randint(0, N, (E,), generator=g)
    if isolated is not None:
        other = (isolated + 1) % N
        src[src == isolated] = other
        dst[dst == isolated] = other
    return torch.stack([src, dst]), types


@pytest.mark.parametrize("T", [1, 17])
@pytest.mark.parametrize("E", [0, 1, 700])
def test_build_plan(T, E):
    from pemp_amd.mpn.train import build_plan
    N = 23
    ei, types = _graph(N, E, 17, 5 * T + E, isolated=7, unused_type=3)
    plan = build_plan(ei, types, N, T)
    src, dst = ei[0], ei[1]
    tsrc = types[src] if T > 1 else torch.zeros_like(src)
    assert (plan.N, plan.E, plan.T) == (N, E, T)
    for perm, key, off, n in ((plan.perm_dst, dst * T + tsrc, plan.seg_off, N * T), (plan.perm_src, src, plan.src_off, N)):
        assert perm.dtype == torch.int32 and off.dtype == torch.int32
        assert torch.equal(perm.long().sort().values, torch.arange(E))            # a permutation of range(E)
        k = key[perm.long()]
        assert bool((k[1:] >= k[:-1]).all())                                      # keys non-decreasing
        same = k[1:] == k[:-1]
        assert bool((perm[1:][same] > perm[:-1][same]).all())                     # equal keys keep edge-id order
        want = torch.cat([torch.zeros(1, dtype=torch.int64), torch.bincount(key, minlength=n).cumsum(0)])
        assert torch.equal(off.long(), want)
    assert torch.equal(plan.dst_off, plan.seg_off[::T]) and plan.dst_off.is_contiguous()
    assert plan.dst_off.shape == (N + 1,) and int(plan.seg_off[-1]) == E
    # the isolated node has no edge either way; the unused type has no segment with an edge
    assert plan.src_off[8] == plan.src_off[7] and plan.dst_off[8] == plan.dst_off[7]
    if T > 1:
        seg_len = (plan.seg_off[1:] - plan.seg_off[:-1]).view(N, T)
        assert int(seg_len[:, 3].sum()) == 0
        assert sum(plan.bucket_sizes) == E and plan.bucket_sizes[3] == 0 and len(plan.bucket_sizes) == 17
        assert plan.bucket_sizes == torch.bincount(tsrc, minlength=17).tolist()
        bt = tsrc[plan.bucket_perm]
        assert bool((bt[1:] >= bt[:-1]).all())
        assert torch.equal(plan.bucket_perm[plan.bucket_inv], torch.arange(E))
    else:
        assert plan.bucket_perm is None


def test_build_plan_rejects_ids_it_cannot_hold():
    from pemp_amd.mpn.train import build_plan
    ei, types = _graph(10, 50, 17, 1)
    with pytest.raises(ValueError):
        build_plan(ei, types, int(ei.max()), 17)                                    # a node id >= N
    with pytest.raises(ValueError):
        build_plan(ei, types.clamp(min=14), 10, 14)                                 # a type >= T
    with pytest.raises(ValueError):
        build_plan(ei, types, 10, 0)


# ---- the restatement against the reference's training step --------------------------------------------------------
@pytest.mark.parametrize("name", gu.names("train_"))
def test_oracle_reproduces_the_reference(name):
    meta, ref = gu.load(name)
    src_meta, a = gu.load(meta["source"])
    cfg = gu.mpn_config(src_meta)
    import pemp_amd
    from pemp_amd import synthetic as syn
    sd = syn.closed_form_state_dict(pemp_amd.get_mpn_model(cfg), meta["salt"], meta.get("attn_gain", 1.0),
                                    meta.get("weight_gain", 1.0))
    mine = to.step(sd, cfg, a["x"], a["edge_attr"], a["edge_index"], a["node_types"])
    assert any(k.startswith("grad.") for k in ref) and any(k.startswith("bn.") for k in ref) and "loss" in ref
    for k, want in ref.items():
        got = to.lookup(mine, k)
        if k.endswith("num_batches_tracked"):
            assert np.array_equal(got, want), k
            continue
        if got is None:       # a parameter the forward never reaches (mlp_node.mlp.14..16 with J = 14)
            assert k.startswith("grad.") and not np.any(want), k
            continue
        assert np.shape(got) == np.shape(want), k
        if k == to.ATTN_BIAS:     # analytically zero; both sides within the rounding residue of its terms at fp64
            assert np.abs(got - want).max() <= 2 * to.residue_bound(mine, 2.0 ** -53), k
            continue
        err = np.abs(np.asarray(got, np.float64) - want).max() if np.size(want) else 0.0
        assert err <= 1e-9 * to.scale_of(ref, k), (k, err)
