"""The device-side path reconstruction's host surface and its kernels' code generation (no GPU needed): include/vhp.h declares the six
entry points, libvhp_hip.so exports them, the Python binding has them; a null context fails with VHP_ERR_ARG before any device is
touched; and in the gfx950 assembly of vhp_capi.hip the two kernels (vhp_paths_parents, vhp_paths_walk) use no scratch memory and none
of the scalar memory-store, scalar-atomic or scalar data-cache write-back instructions."""
import os
import re
import subprocess

import host_lib
from test_kernel_codegen import _compile, _kernels

SYMBOLS = ("vhp_planner_batch_paths", "vhp_planner_batch_paths_device", "vhp_planner_maps_batch_paths",
           "vhp_planner_maps_batch_paths_device", "vhp_planner_path", "vhp_planner_path_device")


def test_library_exports_the_path_calls():
    import vhp_amd
    vhp_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vhp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vhp_\w+)$", nm, re.M))
    for sym in SYMBOLS:
        assert sym in exported, sym
        assert sym in vhp_amd.ABI_SYMBOLS, sym


def test_header_declares_the_path_calls():
    header = open(os.path.join(host_lib.ROOT, "include", "vhp.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (declarations, not the comments that mention them)
    decl = re.sub(r"\s+", " ", decl)
    for sym in SYMBOLS:
        d = "d_" if sym.endswith("_device") else ""
        args = (r"vhp_ctx\* ctx, int32_t\* %spath_xy, uint32_t cap, uint32_t\* %sn_path, double\* %slength, int32_t\* %spath_status" % (d, d, d, d))
        assert re.search(r"\bint %s\(%s\);" % (sym, args), decl), sym
    # the contract is stated where a binding's author reads it
    for phrase in ("Not timed", "start-first", "VHP_ERR_TOO_LARGE for a path of more than cap points", "path_xy may be NULL"):
        assert phrase in header, phrase


def test_context_has_the_path_calls():
    import vhp_amd
    for name in ("planner_batch_paths", "planner_batch_paths_device", "planner_maps_batch_paths", "planner_maps_batch_paths_device",
                 "planner_path", "planner_path_device"):
        assert callable(getattr(vhp_amd.Context, name, None)), name


def test_null_context_is_an_argument_error():
    import vhp_amd
    vhp_amd.build_library()
    lib = vhp_amd.load_library()
    for sym in SYMBOLS:
        assert getattr(lib, sym)(None, None, 0, None, None, None) == vhp_amd.VHP_ERR_ARG, sym


def test_path_kernels_codegen(tmp_path):
    asm, remarks = _compile("vhp_capi.hip", tmp_path)
    blocks = {b.split()[0]: b for b in re.split(r"remark: Function Name: ", remarks)[1:]}
    forbidden = re.compile(r"^\s+(s_(?:buffer_|scratch_)?store_\w+|s_(?:buffer_)?atomic_\w+|s_dcache_(?:wb|discard)\w*)", re.M | re.I)
    for kernel in ("vhp_paths_parents", "vhp_paths_walk"):
        ks = _kernels(asm, kernel)
        assert len(ks) == 1, (kernel, sorted(ks))
        (name, body), = ks.items()
        get = lambda key: int(re.search(key + r":\s*(\d+)", blocks[name]).group(1))
        assert get(r"ScratchSize \[bytes/lane\]") == 0 and get(r"VGPRs Spill") == 0 and get(r"SGPRs Spill") == 0, name
        m = re.search(r"\.name:\s*%s\n\s*\.private_segment_fixed_size:\s*(\d+)" % re.escape(name), asm)
        assert m and int(m.group(1)) == 0, "%s uses scratch memory" % name
        assert not re.findall(r"^\s+scratch_\w+", body, re.M), name
        assert not forbidden.findall(body), (name, forbidden.findall(body))
        assert re.search(r"^\s+global_store_dword", body, re.M), name   # (vector stores)
