"""CPU-side check of the size guard behind the packed segment positions: the edge passes keep each edge's position
in its segment in the high byte of its sorted-target entry (mpn.hip, sdst_pack), so a call whose node ids would not
fit below it must be refused before anything is launched, with a clear pemp_last_error. No GPU needed: the range
check reads only the descriptor and the sizes."""
import ctypes

from pemp_amd import _lib

LIMIT = 1 << 23


def forward(L, N, E=0):
    desc = _lib.PempMpnDesc(num_types=1, num_joints=17, steps=3, aux_loss_steps=0, aggr=-1, hidden=64,
                            edge_attr_dim=19, node_in_dim=128, precision=0, types_stride=1, flags=0)
    w = _lib.PempMpnWeights()                                   # all null: never read before the range check
    rc = L.pemp_mpn_forward(ctypes.byref(desc), ctypes.byref(w), None, None, None, None, N, E, None, None, None,
                            None, 0, None)
    return rc, L.pemp_last_error().decode()


def test_node_count_at_and_above_the_limit_is_refused():
    L = _lib.load_cdll()
    for n in (LIMIT, LIMIT + 1, 1 << 24, 1 << 31):
        rc, msg = forward(L, n)
        assert rc == _lib.ERR_INVALID_ARG and "out of range" in msg and f"N={n}" in msg and "2^23" in msg, (n, msg)


def test_node_count_below_the_limit_passes_the_range_check():
    """N = 2^23 - 1 gets past the range check: the call is then refused for the descriptor's aggregation (-1 here),
    still before any weight or GPU is touched."""
    L = _lib.load_cdll()
    rc, msg = forward(L, LIMIT - 1)
    assert rc == _lib.ERR_INVALID_ARG and "out of range" not in msg and "aggr" in msg, msg
