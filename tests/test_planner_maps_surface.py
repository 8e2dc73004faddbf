"""The batch planner across a stack of maps: its host surface and its kernel's code generation (no GPU needed).  The library exports
vhp_planner_solve_maps_batch and its three companions, vhp.h declares them, the Python binding has them, and in the gfx950 assembly
of vhp_lat.hip the four vhp_lat_maps_sweep instantiations (fp64; odd and even pitch; one and several workgroups per unit) hold the
latency sweep's budgets: at most 128 VGPRs, four waves per SIMD, no scratch, no FLAT instructions, few spilled scalars and none
of them moved inside a window's steps."""
import os
import re
import subprocess

import host_lib
from test_kernel_codegen import _compile, _kernels   # (one compilation of vhp_lat.hip per test session, shared with that file)

SYMBOLS = ("vhp_planner_solve_maps_batch", "vhp_planner_maps_batch_results_device", "vhp_planner_maps_batch_results",
           "vhp_planner_maps_batch_group")


def test_library_exports_the_maps_batch():
    import vhp_amd
    vhp_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vhp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vhp_\w+)$", nm, re.M))
    for sym in SYMBOLS:
        assert sym in exported, sym
        assert sym in vhp_amd.ABI_SYMBOLS, sym


def test_header_declares_the_maps_batch():
    header = open(os.path.join(host_lib.ROOT, "include", "vhp.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (declarations, not the comments that mention them)
    decl = re.sub(r"\s+", " ", decl)
    want = {
        "vhp_planner_solve_maps_batch": r"vhp_ctx\* ctx, const int32_t\* queries, const int32_t\* map_idx, const double\* thresholds, "
                                        r"int n_queries, uint64_t max_iter, int32_t\* status, uint32_t\* n_pivots",
        "vhp_planner_maps_batch_results_device": r"vhp_ctx\* ctx, int q, const uint32_t\*\* labels, const double\*\* vis_global, "
                                                 r"const double\*\* vis_local, const int32_t\*\* pivots_xy",
        "vhp_planner_maps_batch_results": r"vhp_ctx\* ctx, int q, uint64_t\* came_from, double\* vis_global, double\* vis_local, "
                                          r"int32_t\* pivots_xy",
        "vhp_planner_maps_batch_group": r"const vhp_ctx\* ctx",
    }
    for sym, args in want.items():
        assert re.search(r"\bint %s\(%s\);" % (sym, args), decl), sym


def test_context_has_the_maps_batch():
    import vhp_amd
    for name in ("planner_solve_maps_batch", "planner_maps_batch_results_device", "planner_maps_batch_group"):
        assert callable(getattr(vhp_amd.Context, name, None)), name


def test_maps_latency_sweep_register_budget(tmp_path):
    asm, remarks = _compile("vhp_lat.hip", tmp_path)
    ks = _kernels(asm, "vhp_lat_maps_sweep")
    assert len(ks) == 4, sorted(ks)
    blocks = {b.split()[0]: b for b in re.split(r"remark: Function Name: ", remarks)[1:]}
    for name, body in ks.items():
        targs = re.search(r"vhp_lat_maps_sweepILb([01])ELb([01])EEEv", name)
        assert targs, name
        multi = targs.group(2) == "1"
        blk = blocks[name]
        get = lambda key: int(re.search(key + r":\s*(\d+)", blk).group(1))
        assert get(r"\bVGPRs") <= 128, (name, get(r"\bVGPRs"))
        assert get(r"ScratchSize \[bytes/lane\]") == 0, name
        assert get(r"VGPRs Spill") == 0, name
        assert get(r"Occupancy \[waves/SIMD\]") >= 4, name
        assert get(r"SGPRs Spill") <= (520 if multi else 240), (name, get(r"SGPRs Spill"))
        m = re.search(r"\.name:\s*%s\n\s*\.private_segment_fixed_size:\s*(\d+)" % re.escape(name), asm)
        assert m and int(m.group(1)) == 0, "%s uses scratch memory" % name
        flat = re.findall(r"^\s+flat_\w+", body, re.M)
        scratch = re.findall(r"^\s+scratch_\w+", body, re.M)
        assert not flat and not scratch, (name, sorted(set(flat + scratch)))
        for b in re.split(r"^\.LBB\d+_\d+:", body, flags=re.M):
            if len(re.findall(r"v_(?:fma|mul|add|fmac)_f64", b)) >= 90:   # (a window's sixteen steps)
                n = len(re.findall(r"v_(?:readlane|writelane)_b32", b))
                assert n <= 2, "%s: %d spilled scalars moved inside a window's steps" % (name, n)
