"""The fused first edge pass (csrc/mpn.hip, edge_step_kernel STAGE_FIRST), host side: its LDS footprint from the
library's own layout functions, and the descriptor flags that select it, as pemp.h, libpemp and _lib.py state them."""
import ctypes
import pathlib
import re

from pemp_amd import _lib

HEADER = pathlib.Path(__file__).resolve().parents[1] / "include" / "pemp.h"


def test_fused_first_lds_fits_one_workgroup_per_cu():
    """Pass image + composed embedding image + piece records: 154,768 B of the CU's 160 KiB."""
    L = _lib.load_cdll()
    n = L.pemp_mpn_fused_first_lds_bytes()
    # img_common(1) = 4 x 64 x 72 + 132 floats; 1,280 + 2,560 + 3 x 4,608 + 288 floats; 16 waves x 2 x 68 floats
    assert n == 4 * (18_564 + 17_952 + 2_176)
    assert n <= 160 * 1024


def test_flags_and_abi_round_trip():
    """The flag values of pemp.h are _lib's, the ABI number is the library's, and neither flag changes the workspace."""
    text = HEADER.read_text()
    defs = {k: int(v) for k, v in re.findall(r"#define (PEMP_MPN_[A-Z_]+) (\d+)", text)}
    assert defs["PEMP_MPN_TWO_LAUNCH_FIRST"] == _lib.MPN_TWO_LAUNCH_FIRST == 4
    assert defs["PEMP_MPN_FUSED_FIRST_PROFILED"] == _lib.MPN_FUSED_FIRST_PROFILED == 8
    assert defs["PEMP_MPN_PREPARED"] == _lib.MPN_PREPARED
    L = _lib.load_cdll()
    assert int(re.search(r"#define PEMP_ABI_VERSION (\d+)", text).group(1)) == L.pemp_abi_version() == _lib.ABI_VERSION
    sizes = set()
    for flags in (0, _lib.MPN_TWO_LAUNCH_FIRST, _lib.MPN_FUSED_FIRST_PROFILED):
        desc = _lib.PempMpnDesc(17, 17, 3, 0, 3, 64, 19, 128, 2, 1, flags)
        assert desc.flags == flags
        sizes.add(L.pemp_mpn_workspace_size(ctypes.byref(desc), 1546, 232_846))
    assert len(sizes) == 1 and sizes.pop() > 0


def test_model_attribute_maps_to_flags():
    import pemp_amd
    from pemp_amd import config as pcfg
    m = pemp_amd.get_mpn_model(pcfg.published_mpn_config(17, 3, "attn"))
    assert m.fuse_first_pass is None and m._first_flag() == 0
    m.fuse_first_pass = True
    assert m._first_flag() == _lib.MPN_FUSED_FIRST_PROFILED
    m.fuse_first_pass = False
    assert m._first_flag() == _lib.MPN_TWO_LAUNCH_FIRST
