"""The host surface of the windows of the map as a stack of maps (no GPU needed): the C ABI exports and declares vhp_set_maps_windows,
vhp_maps_occupancy and their device forms, and the Python binding has them."""
import os
import re
import subprocess

import host_lib

WINDOW_SYMBOLS = ("vhp_set_maps_windows", "vhp_set_maps_windows_device", "vhp_maps_occupancy", "vhp_maps_occupancy_device")


def test_library_exports_the_windows():
    import vhp_amd
    vhp_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vhp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vhp_\w+)$", nm, re.M))
    for sym in WINDOW_SYMBOLS:
        assert sym in exported, sym
        assert sym in vhp_amd.ABI_SYMBOLS, sym


def test_header_declares_the_windows():
    header = open(os.path.join(host_lib.ROOT, "include", "vhp.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (declarations, not the comments that mention them)
    want = {
        "vhp_set_maps_windows": r"vhp_ctx\* ctx, const int32_t\* origin_xy, int n_windows, int w, int h",
        "vhp_set_maps_windows_device": r"vhp_ctx\* ctx, const int32_t\* d_origin_xy, int n_windows, int w, int h",
        "vhp_maps_occupancy": r"vhp_ctx\* ctx, int first, int n, uint8_t\* occ_out",
        "vhp_maps_occupancy_device": r"vhp_ctx\* ctx, int first, int n, uint8_t\* d_occ_out",
    }
    for sym, args in want.items():
        assert re.search(r"\bint %s\(%s\);" % (sym, args), decl), sym
    # the header says whose coordinates results on windows are in
    assert "WINDOW COORDINATES" in header


def test_binding_gives_the_windows_their_argument_types():
    import ctypes as C
    import vhp_amd
    vhp_amd.build_library()
    lib = vhp_amd.load_library()
    vp, i32 = C.c_void_p, C.c_int
    assert lib.vhp_set_maps_windows.argtypes == [vp, vp, i32, i32, i32]
    assert lib.vhp_set_maps_windows_device.argtypes == [vp, vp, i32, i32, i32]
    assert lib.vhp_maps_occupancy.argtypes == [vp, i32, i32, vp]
    assert lib.vhp_maps_occupancy_device.argtypes == [vp, i32, i32, vp]


def test_context_has_the_windows():
    import vhp_amd
    for name in ("set_maps_windows", "set_maps_windows_device", "maps_occupancy", "maps_occupancy_device", "sweep_windows"):
        assert callable(getattr(vhp_amd.Context, name, None)), name
    doc = vhp_amd.Context.sweep_windows.__doc__
    assert "REPLACES the stack" in doc and "first row and column" in doc
