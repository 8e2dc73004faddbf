"""The batch planner's host surface and its epilogue's code generation (no GPU needed): the C ABI exports and declares
vhp_planner_solve_batch and its results calls, the Python binding has them, and the gfx950 assembly of vhp_capi.hip holds
vhp_planner_batch_epilogue with no scratch and no spilled vector registers."""
import os
import re
import subprocess

import host_lib
from test_kernel_codegen import _compile, _kernels   # (one compilation of vhp_capi.hip per test session, shared with that file)

BATCH_SYMBOLS = ("vhp_planner_solve_batch", "vhp_planner_batch_results_device", "vhp_planner_batch_results", "vhp_planner_batch_group")


def test_library_exports_the_batch_planner():
    import vhp_amd
    vhp_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vhp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vhp_\w+)$", nm, re.M))
    for sym in BATCH_SYMBOLS:
        assert sym in exported, sym
        assert sym in vhp_amd.ABI_SYMBOLS, sym


def test_header_declares_the_batch_planner():
    header = open(os.path.join(host_lib.ROOT, "include", "vhp.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (declarations, not the comments that mention them)
    for sym in BATCH_SYMBOLS:
        assert re.search(r"\bint %s\s*\(" % sym, decl), sym
    assert re.search(r"int vhp_planner_solve_batch\(vhp_ctx\* ctx, const int32_t\* queries, const double\* thresholds, int n_queries, "
                     r"uint64_t max_iter,\s+int32_t\* status, uint32_t\* n_pivots\);", decl)
    assert '"planner_batch_group"' in header


def test_context_has_planner_solve_batch():
    import vhp_amd
    for name in ("planner_solve_batch", "planner_batch_results_device", "planner_batch_group"):
        assert callable(getattr(vhp_amd.Context, name, None)), name


def test_batch_epilogue_has_no_scratch_and_no_spills(tmp_path):
    asm, remarks = _compile("vhp_capi.hip", tmp_path)
    ks = _kernels(asm, "vhp_planner_batch_epilogue")
    assert len(ks) == 1, list(ks)
    name = next(iter(ks))
    m = re.search(r"\.name:\s*%s\n\s*\.private_segment_fixed_size:\s*(\d+)" % re.escape(name), asm)
    assert m and int(m.group(1)) == 0, "%s uses scratch memory" % name
    blocks = [b for b in re.split(r"remark: Function Name: ", remarks)[1:] if b.split()[0] == name]
    assert len(blocks) == 1, name
    get = lambda key: int(re.search(key + r":\s*(\d+)", blocks[0]).group(1))
    assert get(r"ScratchSize \[bytes/lane\]") == 0, name
    assert get(r"VGPRs Spill") == 0, name
    # (the epilogue's DPP goes through __builtin_amdgcn_update_dpp: no hand-written instruction of its own beyond the body's waits)
    assert not re.search(r"^\s+scratch_\w+", ks[name], re.M)
