"""The host surface of the clearance field (no GPU needed): the C ABI exports and declares vhp_map_clearance, vhp_maps_clearance and
their device forms, the Python binding has them, and its footprint arguments are checked before any library call."""
import os
import re
import subprocess

import pytest

import host_lib

CLEARANCE_SYMBOLS = ("vhp_map_clearance", "vhp_maps_clearance", "vhp_map_clearance_device", "vhp_maps_clearance_device")


def test_library_exports_the_clearance():
    import vhp_amd
    vhp_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vhp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vhp_\w+)$", nm, re.M))
    for sym in CLEARANCE_SYMBOLS:
        assert sym in exported, sym
        assert sym in vhp_amd.ABI_SYMBOLS, sym


def test_header_declares_the_clearance():
    import vhp_amd
    header = open(os.path.join(host_lib.ROOT, "include", "vhp.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (declarations, not the comments that mention them)
    want = {
        "vhp_map_clearance": r"vhp_ctx\* ctx, int shape, int p_max, int flags, uint16_t\* out",
        "vhp_map_clearance_device": r"vhp_ctx\* ctx, int shape, int p_max, int flags, uint16_t\* d_out",
        "vhp_maps_clearance": r"vhp_ctx\* ctx, int first, int n, int shape, int p_max, int flags, uint16_t\* out",
        "vhp_maps_clearance_device": r"vhp_ctx\* ctx, int first, int n, int shape, int p_max, int flags, uint16_t\* d_out",
    }
    for sym, args in want.items():
        assert re.search(r"\bint %s\(%s\);" % (sym, args), decl), sym
    assert re.search(r"#define VHP_CLEARANCE_FAR 0xFFFF\b", decl)
    assert vhp_amd.CLEARANCE_FAR == 0xFFFF
    # the header gives the definition and what the field is for
    assert "smallest p" in header and "fits at a cell exactly when c > p" in header


def test_far_value_and_tile_are_defined_once():
    csrc = os.path.join(host_lib.ROOT, "visibility-heuristic-path-planner_amd", "csrc")
    assert re.search(r"^constexpr unsigned kClearanceFar = 0xFFFF;", open(os.path.join(csrc, "vhp_clearance.hpp")).read(), re.M)
    assert len(re.findall(r"^constexpr int kClearanceTileRows = \d+;", open(os.path.join(csrc, "vhp_clearance.hip.h")).read(), re.M)) == 1


def test_docs_name_the_clearance():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(host_lib.ROOT, name)).read()
        for sym in CLEARANCE_SYMBOLS[:2]:   # (the device forms go as "+ _device" where a document lists calls)
            assert re.search(r"\b%s\b" % sym, text), (name, sym)
    design = open(os.path.join(host_lib.ROOT, "DESIGN.md")).read()
    assert re.search(r"^#+ *6e\b", design, re.M)
    assert "c > p" in open(os.path.join(host_lib.ROOT, "INTEGRATION.md")).read()


def test_binding_gives_the_clearance_its_argument_types():
    import ctypes as C
    import vhp_amd
    vhp_amd.build_library()
    lib = vhp_amd.load_library()
    vp, i32 = C.c_void_p, C.c_int
    assert lib.vhp_map_clearance.argtypes == [vp, i32, i32, i32, vp]
    assert lib.vhp_map_clearance_device.argtypes == [vp, i32, i32, i32, vp]
    assert lib.vhp_maps_clearance.argtypes == [vp, i32, i32, i32, i32, i32, vp]
    assert lib.vhp_maps_clearance_device.argtypes == [vp, i32, i32, i32, i32, i32, vp]


class _NoLibrary:
    """stands in for a Context: any use of the library, the handle or the sizes is an error of the test's"""
    def __getattr__(self, name):
        raise AssertionError("the call reached for %r before refusing its arguments" % name)


BAD_FOOTPRINTS = [dict(),                                       # neither radius nor p
                  dict(radius=2, p=4),                          # both
                  dict(radius=2.5, shape="square"),             # a fractional radius for a square
                  dict(radius=-1),
                  dict(p=-1),
                  dict(p=2.5),
                  dict(radius=2, shape="hexagon"),
                  dict(radius=float("nan")),
                  dict(radius="wide")]


@pytest.mark.parametrize("kwargs", BAD_FOOTPRINTS, ids=[repr(k) for k in BAD_FOOTPRINTS])
def test_bad_footprints_raise_before_any_library_call(kwargs):
    import vhp_amd
    with pytest.raises(ValueError):
        vhp_amd.Context.map_clearance(_NoLibrary(), **kwargs)
    with pytest.raises(ValueError):
        vhp_amd.Context.map_clearance_device(_NoLibrary(), 0, **kwargs)
    with pytest.raises(ValueError):
        vhp_amd.Context.maps_clearance(_NoLibrary(), 0, 1, **kwargs)
    with pytest.raises(ValueError):
        vhp_amd.Context.maps_clearance_device(_NoLibrary(), 0, 0, 1, **kwargs)


def test_context_has_the_clearance():
    import inspect
    import vhp_amd
    foot = [("radius", None), ("shape", "disc"), ("p", None), ("border", False)]
    want = {"map_clearance": foot, "map_clearance_device": [("d_out", inspect.Parameter.empty)] + foot,
            "maps_clearance": [("first", 0), ("n", None)] + foot,
            "maps_clearance_device": [("d_out", inspect.Parameter.empty), ("first", 0), ("n", None)] + foot}
    for name, params in want.items():
        assert callable(getattr(vhp_amd.Context, name, None)), name
        sig = inspect.signature(getattr(vhp_amd.Context, name))
        assert [(k, v.default) for k, v in sig.parameters.items()][1:] == params, name
    assert "CLEARANCE_FAR" in vhp_amd.Context.map_clearance.__doc__
