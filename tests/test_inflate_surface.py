"""The host surface of the inflation by a robot's footprint (no GPU needed): the C ABI exports and declares vhp_inflate_map,
vhp_inflate_maps, vhp_map_occupancy and its device form, the Python binding has them, and its footprint arguments are checked -- and
turned into the C ABI's (shape, p) -- before any library call."""
import os
import re
import subprocess
from decimal import Decimal
from fractions import Fraction

import pytest

import host_lib

INFLATE_SYMBOLS = ("vhp_inflate_map", "vhp_inflate_maps", "vhp_map_occupancy", "vhp_map_occupancy_device")


def test_library_exports_the_inflation():
    import vhp_amd
    vhp_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vhp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vhp_\w+)$", nm, re.M))
    for sym in INFLATE_SYMBOLS:
        assert sym in exported, sym
        assert sym in vhp_amd.ABI_SYMBOLS, sym


def test_header_declares_the_inflation():
    import vhp_amd
    header = open(os.path.join(host_lib.ROOT, "include", "vhp.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (declarations, not the comments that mention them)
    want = {
        "vhp_inflate_map": r"vhp_ctx\* ctx, int shape, int p, int flags",
        "vhp_inflate_maps": r"vhp_ctx\* ctx, int first, int n, int shape, int p, int flags",
        "vhp_map_occupancy": r"vhp_ctx\* ctx, uint8_t\* occ_out",
        "vhp_map_occupancy_device": r"vhp_ctx\* ctx, uint8_t\* d_occ_out",
    }
    for sym, args in want.items():
        assert re.search(r"\bint %s\(%s\);" % (sym, args), decl), sym
    assert re.search(r"VHP_FOOT_DISC = 0, VHP_FOOT_SQUARE = 1, VHP_FOOT_DIAMOND = 2", decl)
    assert re.search(r"#define VHP_MAX_INFLATE 64\b", decl) and re.search(r"#define VHP_INFLATE_BORDER 1\b", decl)
    assert (vhp_amd.FOOT_DISC, vhp_amd.FOOT_SQUARE, vhp_amd.FOOT_DIAMOND, vhp_amd.MAX_INFLATE, vhp_amd.INFLATE_BORDER) == (0, 1, 2, 64, 1)
    # the header says in which order inflation and windows go, and what a failed call leaves of the stack
    assert "BEFORE cutting windows" in header and "the stack is EMPTY" in header


def test_docs_name_the_inflation():
    for name in ("README.md", "INTEGRATION.md", "DESIGN.md"):
        text = open(os.path.join(host_lib.ROOT, name)).read()
        for sym in INFLATE_SYMBOLS[:3]:   # (the device form goes as "+ _device" where a document lists calls)
            assert re.search(r"\b%s\b" % sym, text), (name, sym)
    assert re.search(r"^#+ *6d\b", open(os.path.join(host_lib.ROOT, "DESIGN.md")).read(), re.M)


def test_binding_gives_the_inflation_its_argument_types():
    import ctypes as C
    import vhp_amd
    vhp_amd.build_library()
    lib = vhp_amd.load_library()
    vp, i32 = C.c_void_p, C.c_int
    assert lib.vhp_inflate_map.argtypes == [vp, i32, i32, i32]
    assert lib.vhp_inflate_maps.argtypes == [vp, i32, i32, i32, i32, i32]
    assert lib.vhp_map_occupancy.argtypes == [vp, vp]
    assert lib.vhp_map_occupancy_device.argtypes == [vp, vp]


class _NoLibrary:
    """stands in for a Context: any use of the library, the handle or the sizes is an error of the test's"""
    def __getattr__(self, name):
        raise AssertionError("the call reached for %r before refusing its arguments" % name)


BAD_FOOTPRINTS = [dict(),                                       # neither radius nor p
                  dict(radius=2, p=4),                          # both
                  dict(radius=2.5, shape="square"),             # a fractional radius for a square ...
                  dict(radius=Fraction(1, 2), shape="diamond"),  # ... and for a diamond
                  dict(radius=-1),
                  dict(radius=-0.5, shape="disc"),
                  dict(p=-1),
                  dict(p=2.5),
                  dict(radius=2, shape="hexagon"),
                  dict(radius=2, shape=0),                      # (shapes go by name here)
                  dict(radius=float("nan")),
                  dict(radius=float("inf")),
                  dict(radius="wide")]


@pytest.mark.parametrize("kwargs", BAD_FOOTPRINTS, ids=[repr(k) for k in BAD_FOOTPRINTS])
def test_bad_footprints_raise_before_any_library_call(kwargs):
    import vhp_amd
    with pytest.raises(ValueError):
        vhp_amd.footprint(**kwargs)
    with pytest.raises(ValueError):
        vhp_amd.Context.inflate_map(_NoLibrary(), **kwargs)
    with pytest.raises(ValueError):
        vhp_amd.Context.inflate_maps(_NoLibrary(), 0, 1, **kwargs)


def test_radius_to_p():
    import vhp_amd
    f = vhp_amd.footprint
    D, S, M = vhp_amd.FOOT_DISC, vhp_amd.FOOT_SQUARE, vhp_amd.FOOT_DIAMOND
    assert f(2.9) == (D, 8) and f(3) == (D, 9) and f(3.0) == (D, 9) and f(0) == (D, 0) and f(0.99) == (D, 0) and f(1) == (D, 1)
    assert f(radius=64) == (D, 4096) and f(64.99) == (D, 4223) and f(65) == (D, 4225)   # (the last one is the library's to refuse)
    # exact in the value given: 2^0.5 as a double lies above the real square root of 2, and its square is not rounded
    assert f(2 ** 0.5) == (D, 2) and f(Fraction(14142135, 10 ** 7)) == (D, 1) and f(Decimal("2.2360679")) == (D, 4)
    assert f(Fraction(5, 2)) == (D, 6) and f(Decimal("2.5")) == (D, 6)
    assert f(p=8) == (D, 8) and f(p=0, shape="square") == (S, 0) and f(p=7, shape="diamond") == (M, 7)
    assert f(3, "square") == (S, 3) and f(3.0, "diamond") == (M, 3) and f(radius=0, shape="square") == (S, 0)


def test_context_has_the_inflation():
    import inspect
    import vhp_amd
    for name in ("inflate_map", "inflate_maps", "map_occupancy", "map_occupancy_device"):
        assert callable(getattr(vhp_amd.Context, name, None)), name
    sig = inspect.signature(vhp_amd.Context.inflate_map)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("radius", None), ("shape", "disc"), ("p", None), ("border", False)]
    sig = inspect.signature(vhp_amd.Context.inflate_maps)
    assert [(k, v.default) for k, v in sig.parameters.items()][1:] == [("first", 0), ("n", None), ("radius", None), ("shape", "disc"), ("p", None),
                                                                       ("border", False)]
    assert "BEFORE cutting windows" in vhp_amd.Context.inflate_map.__doc__
