"""The map-stack sweep's host surface and its kernel's code generation (no GPU needed): the C ABI exports and declares
vhp_set_maps / vhp_sweep_maps_batch and their device forms, the Python binding has them, and in the gfx950 assembly of
vhp_capi.hip every vhp_sweep_fronts_maps instantiation stays within the budget of its vhp_sweep_fronts sibling: no FLAT
instructions, no more scratch, at most 8 more vector registers and the same waves per SIMD."""
import os
import re
import subprocess

import host_lib
from test_kernel_codegen import _compile, _kernels   # (one compilation of vhp_capi.hip per test session, shared with that file)

MAPS_SYMBOLS = ("vhp_set_maps", "vhp_set_maps_device", "vhp_sweep_maps_batch", "vhp_sweep_maps_batch_device")


def test_library_exports_the_maps_sweep():
    import vhp_amd
    vhp_amd.build_library()
    nm = subprocess.run(["nm", "-D", "--defined-only", vhp_amd.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\bT (vhp_\w+)$", nm, re.M))
    for sym in MAPS_SYMBOLS:
        assert sym in exported, sym
        assert sym in vhp_amd.ABI_SYMBOLS, sym


def test_header_declares_the_maps_sweep():
    header = open(os.path.join(host_lib.ROOT, "include", "vhp.h")).read()
    decl = re.sub(r"/\*.*?\*/", "", header, flags=re.S)   # (declarations, not the comments that mention them)
    want = {
        "vhp_set_maps": r"vhp_ctx\* ctx, const uint8_t\* occ, int n_maps, int nx, int ny",
        "vhp_set_maps_device": r"vhp_ctx\* ctx, const uint8_t\* d_occ, int n_maps, int nx, int ny",
        "vhp_sweep_maps_batch": r"vhp_ctx\* ctx, const int32_t\* src_xy, const int32_t\* map_idx, int n_src, int dtype, void\* out_host",
        "vhp_sweep_maps_batch_device": r"vhp_ctx\* ctx, const int32_t\* d_src_xy, const int32_t\* d_map_idx, int n_src, int dtype, void\* d_out",
    }
    for sym, args in want.items():
        assert re.search(r"\bint %s\(%s\);" % (sym, args), decl), sym


def test_context_has_the_maps_sweep():
    import vhp_amd
    for name in ("set_maps", "set_maps_device", "sweep_maps_batch", "sweep_maps_batch_device"):
        assert callable(getattr(vhp_amd.Context, name, None)), name


def _targs(name):
    """the template arguments <R, MULTI, OutT> of a vhp_sweep_fronts / vhp_sweep_fronts_maps instantiation, as mangled"""
    return re.search(r"vhp_sweep_fronts(?:_maps)?(I.*?E)Ev", name).group(1)


def _resources(remarks, name):
    blocks = [b for b in re.split(r"remark: Function Name: ", remarks)[1:] if b.split()[0] == name]
    assert len(blocks) == 1, name
    get = lambda key: int(re.search(key + r":\s*(\d+)", blocks[0]).group(1))
    return {"vgpr": get(r"\bVGPRs"), "agpr": get(r"\bAGPRs"), "occupancy": get(r"Occupancy \[waves/SIMD\]"),
            "scratch": get(r"ScratchSize \[bytes/lane\]")}


def test_maps_kernel_budget_matches_its_sibling(tmp_path):
    asm, remarks = _compile("vhp_capi.hip", tmp_path)
    maps = _kernels(asm, "vhp_sweep_fronts_maps")
    fronts = {n: b for n, b in _kernels(asm, "vhp_sweep_fronts").items() if "vhp_sweep_fronts_maps" not in n}
    assert maps and len(maps) == len(fronts), (sorted(maps), sorted(fronts))
    by_args = {_targs(n): n for n in fronts}
    for name, body in maps.items():
        sib = by_args.get(_targs(name))
        assert sib, name
        flat = re.findall(r"^\s+flat_\w+", body, re.M)
        assert not flat, "%s: FLAT instructions %r" % (name, sorted(set(flat)))
        seg = {}
        for n in (name, sib):
            m = re.search(r"\.name:\s*%s\n\s*\.private_segment_fixed_size:\s*(\d+)" % re.escape(n), asm)
            assert m, n
            seg[n] = int(m.group(1))
        assert seg[name] <= seg[sib], (name, seg)
        mine, theirs = _resources(remarks, name), _resources(remarks, sib)
        assert mine["scratch"] <= theirs["scratch"], (name, mine, theirs)
        assert mine["vgpr"] + mine["agpr"] <= theirs["vgpr"] + theirs["agpr"] + 8, (name, mine, theirs)
        assert mine["occupancy"] == theirs["occupancy"], (name, mine, theirs)
