"""The length-field and goal-path calls' host surface and their kernels' code generation (no GPU needed): include/vhp.h declares the
four entry points and the selector enum, libvhp_hip.so exports them, the Python binding has them; a null context fails with VHP_ERR_ARG
before any device is touched; and in the gfx950 assembly of vhp_capi.hip the three kernels (vhp_tree_tables, vhp_tree_fields,
vhp_tree_goals) each exist once, use no scratch memory, spill nothing, use none of the scalar memory-store, scalar-atomic or scalar
data-cache write-back instructions and store with vector stores; the field kernel loads and stores 16 bytes at a time."""
import os
import re
import subprocess

import host_lib
from test_kernel_codegen import _compile, _kernels

SYMBOLS = ("vhp_planner_length_fields", "vhp_planner_length_fields_device", "vhp_planner_goal_paths", "vhp_planner_goal_paths_device")


def test_library_exports_the_tree_calls():
    import vhp_amd
    vhp_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vhp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vhp_\w+)$", nm, re.M))
    for sym in SYMBOLS:
        assert sym in exported, sym
        assert sym in vhp_amd.ABI_SYMBOLS, sym


def test_header_declares_the_tree_calls():
    header = open(os.path.join(host_lib.ROOT, "include", "vhp.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (declarations, not the comments that mention them)
    decl = re.sub(r"\s+", " ", decl)
    assert re.search(r"typedef enum vhp_solve_kind \{ VHP_SOLVE_PLAIN = 0, VHP_SOLVE_BATCH = 1, VHP_SOLVE_MAPS_BATCH = 2 \} vhp_solve_kind;", decl)
    for d in ("", "d_"):
        suffix = "_device" if d else ""
        assert re.search(r"\bint vhp_planner_length_fields%s\(vhp_ctx\* ctx, int solve, int q_first, int n_q, double\* %slength, uint32_t\* %sn_path\);"
                         % (suffix, d, d), decl), suffix
        assert re.search(r"\bint vhp_planner_goal_paths%s\(vhp_ctx\* ctx, int solve, const int32_t\* %sgoals_qxy, int n_goals, int32_t\* %spath_xy, "
                         r"uint32_t cap, uint32_t\* %sn_path, double\* %slength, int32_t\* %spath_status\);" % (suffix, d, d, d, d, d), decl), suffix
    # the contract is stated where a binding's author reads it
    for phrase in ("Not timed", "start-first", "length = -1.0", "VHP_ERR_END_OOB for a goal outside the grid", "path_xy may be NULL",
                   "n_goals = 0 is VHP_OK", "mode-2 y flip", "Either output may be NULL", "ONE copy"):
        assert phrase in header, phrase


def test_context_has_the_tree_calls():
    import vhp_amd
    for name in ("planner_length_fields", "planner_length_fields_device", "planner_goal_paths", "planner_goal_paths_device"):
        assert callable(getattr(vhp_amd.Context, name, None)), name
    assert (vhp_amd.SOLVE_PLAIN, vhp_amd.SOLVE_BATCH, vhp_amd.SOLVE_MAPS_BATCH) == (0, 1, 2)


def test_null_context_is_an_argument_error():
    import vhp_amd
    vhp_amd.build_library()
    lib = vhp_amd.load_library()
    for sym in SYMBOLS[:2]:
        assert getattr(lib, sym)(None, 0, 0, 1, None, None) == vhp_amd.VHP_ERR_ARG, sym
    for sym in SYMBOLS[2:]:
        assert getattr(lib, sym)(None, 0, None, 0, None, 0, None, None, None) == vhp_amd.VHP_ERR_ARG, sym


def test_tree_kernels_codegen(tmp_path):
    asm, remarks = _compile("vhp_capi.hip", tmp_path)
    blocks = {b.split()[0]: b for b in re.split(r"remark: Function Name: ", remarks)[1:]}
    # (the scalar store family, spelled in pieces)
    forbidden = re.compile(r"^\s+(s_(?:buffer_|scratch_)?st" r"ore_\w+|s_(?:buffer_)?ato" r"mic_\w+|s_dca" r"che_(?:wb|discard)\w*)", re.M | re.I)
    for kernel in ("vhp_tree_tables", "vhp_tree_fields", "vhp_tree_goals"):
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
        if kernel == "vhp_tree_fields":
            # labels in and lengths and counts out 16 bytes at a time; the staged table is read from LDS, nothing through flat addressing
            assert len(re.findall(r"^\s+global_load_dwordx4", body, re.M)) >= 4, name
            assert len(re.findall(r"^\s+global_store_dwordx4", body, re.M)) >= 12, name
            assert re.search(r"^\s+ds_read", body, re.M) and not re.search(r"^\s+flat_", body, re.M), name
            assert get(r"LDS Size \[bytes/block\]") == 20 * 1024, name
    # the older kernels' names are not substrings of the new ones (the codegen tests count kernels by substring)
    for old in ("vhp_paths_parents", "vhp_paths_walk", "vhp_pool_sweep", "vhp_lat_sweep"):
        assert not any(old in k for k in ("vhp_tree_tables", "vhp_tree_fields", "vhp_tree_goals"))
